"""Pillow's ``Image.resize`` for 8-bit channels, restated in numpy from the
rules in include/spdl_hipjpeg.h "Pillow-exact resize", over tests/turbo_ref.py.
No library source is involved; tests/test_resample.py holds it against Pillow."""

from __future__ import annotations

import functools
import math

import numpy as np

from tests import turbo_ref

PRECISION = 22


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    return 1.0 if x == 0.0 else math.sin(x * math.pi) / (x * math.pi)


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


FILTERS = {"bilinear": (_bilinear, 1.0), "bicubic": (_bicubic, 2.0), "lanczos": (_lanczos, 3.0)}


@functools.lru_cache(maxsize=None)
def axis(in_size: int, out_size: int, filt: str):
    """``(xmin[out], n[out], K[out, ksize])`` of one axis, int32."""
    f, s = FILTERS[filt]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support, ss = s * fs, 1.0 / fs
    xmin, cnt, rows = [], [], []
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_size)
        w = [f((x + lo - center + 0.5) * ss) for x in range(hi - lo)]
        ww = 0.0
        for v in w:
            ww += v
        k = [v / ww if ww != 0.0 else v for v in w]
        rows.append([int(-0.5 + v * (1 << PRECISION)) if v < 0 else int(0.5 + v * (1 << PRECISION))
                     for v in k])
        xmin, cnt = xmin + [lo], cnt + [hi - lo]
    K = np.zeros((out_size, max(cnt)), np.int32)
    for xx, r in enumerate(rows):
        K[xx, :len(r)] = r
    return np.asarray(xmin, np.int32), np.asarray(cnt, np.int32), K


def _pass(px: np.ndarray, out_size: int, filt: str) -> np.ndarray:
    """One pass along axis 1 of u8 ``[rows, in, 3]`` -> u8 ``[rows, out, 3]``."""
    xmin, cnt, K = axis(px.shape[1], out_size, filt)
    out = np.empty((px.shape[0], out_size, 3), np.uint8)
    p = px.astype(np.int64)
    for xx in range(out_size):
        k = K[xx, :cnt[xx]].astype(np.int64)
        acc = (1 << (PRECISION - 1)) + np.tensordot(p[:, xmin[xx]:xmin[xx] + cnt[xx]], k, ([1], [0]))
        out[:, xx] = np.clip(acc >> PRECISION, 0, 255)
    return out


def resize(px: np.ndarray, size, filt: str, box=None, window=None) -> np.ndarray:
    """``Image.fromarray(px).crop(box).resize(size, filt)`` of ``[H, W, 3]`` u8,
    ``box = (x, y, w, h)``; ``window = (ox, oy, w, h)`` slices the result.  Both
    passes always run: an axis that keeps its size has identity coefficients."""
    if box is not None:
        px = px[box[1]:box[1] + box[3], box[0]:box[0] + box[2]]
    hz = _pass(px, size[0], filt)
    out = _pass(hz.transpose(1, 0, 2), size[1], filt).transpose(1, 0, 2)
    if window is not None:
        out = out[window[1]:window[1] + window[3], window[0]:window[0] + window[2]]
    return np.ascontiguousarray(out)


def decode_resize(data: bytes, size, filt: str, box=None, window=None) -> np.ndarray:
    return resize(turbo_ref.rgb_u8(data), size, filt, box, window)
