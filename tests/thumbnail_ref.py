"""Pillow's float-box ``Image.resize``, ``Image.reduce``, ``reducing_gap`` and
``Image.thumbnail`` for 8-bit RGB, restated in numpy from the rules in
include/spdl_hipjpeg.h "Pillow-exact thumbnail", over tests/resample_ref.py and
tests/draft_ref.py.  tests/test_thumbnail.py holds it against Pillow."""

from __future__ import annotations

import math

import numpy as np

from tests import draft_ref
from tests.resample_ref import FILTERS, PRECISION


def axis_box(in_size: int, in0: float, in1: float, out_size: int, filt: str):
    """``(xmin[out], n[out], K[out, ksize])`` of the box [in0, in1) of an axis
    of ``in_size`` samples: xmin absolute, clamped to the whole axis."""
    f, s = FILTERS[filt]
    in0, in1 = np.float32(in0), np.float32(in1)  # (Pillow takes a box in single precision)
    scale, in0 = float(in1 - in0) / out_size, float(in0)
    fs = max(scale, 1.0)
    support, ss = s * fs, 1.0 / fs
    xmin, cnt, rows = [], [], []
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
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


def _pass(px: np.ndarray, in0: float, in1: float, out_size: int, filt: str) -> np.ndarray:
    xmin, cnt, K = axis_box(px.shape[1], in0, in1, out_size, filt)
    out = np.empty((px.shape[0], out_size, 3), np.uint8)
    p = px.astype(np.int64)
    for xx in range(out_size):
        k = K[xx, :cnt[xx]].astype(np.int64)
        acc = (1 << (PRECISION - 1)) + np.tensordot(p[:, xmin[xx]:xmin[xx] + cnt[xx]], k, ([1], [0]))
        out[:, xx] = np.clip(acc >> PRECISION, 0, 255)
    return out


def reduce(px: np.ndarray, factor, box=None) -> np.ndarray:
    """``Image.fromarray(px).reduce(factor, box)``, ``box = (x0, y0, x1, y1)``"""
    fx, fy = factor
    x0, y0, x1, y1 = box or (0, 0, px.shape[1], px.shape[0])
    cw, ch = -(-(x1 - x0) // fx), -(-(y1 - y0) // fy)
    out = np.empty((ch, cw, 3), np.uint8)
    for cy in range(ch):
        ya, yb = y0 + cy * fy, min(y0 + (cy + 1) * fy, y1)
        for cx in range(cw):
            xa, xb = x0 + cx * fx, min(x0 + (cx + 1) * fx, x1)
            d = (xb - xa) * (yb - ya)
            s = px[ya:yb, xa:xb].reshape(-1, 3).astype(np.uint64).sum(0)
            out[cy, cx] = (((s + d // 2) * ((1 << 24) // d)) & 0xFFFFFFFF) >> 24
    return out


def plan(width: int, height: int, size, filt: str, box=None, gap=None):
    """``(factors, safe box, box in the reduced picture)`` of ``resize(size,
    filt, box, reducing_gap=gap)``"""
    x0, y0, x1, y1 = box or (0, 0, width, height)
    fx = fy = 1
    if gap is not None:
        fx = int((x1 - x0) / size[0] / gap) or 1
        fy = int((y1 - y0) / size[1] / gap) or 1
    if fx == 1 and fy == 1:
        return (1, 1), (0, 0, width, height), (x0, y0, x1, y1)
    s = FILTERS[filt][1] - 0.5
    sx, sy = s * (x1 - x0) / size[0], s * (y1 - y0) / size[1]
    q = (max(0, int(x0 - sx)), max(0, int(y0 - sy)),
         min(width, math.ceil(x1 + sx)), min(height, math.ceil(y1 + sy)))
    return (fx, fy), q, ((x0 - q[0]) / fx, (y0 - q[1]) / fy, (x1 - q[0]) / fx, (y1 - q[1]) / fy)


def resize(px: np.ndarray, size, filt: str, box=None, gap=None) -> np.ndarray:
    """``Image.fromarray(px).resize(size, filt, box=box, reducing_gap=gap)``"""
    f, q, b = plan(px.shape[1], px.shape[0], size, filt, box, gap)
    if f != (1, 1):
        px = reduce(px, f, q)
    hz = _pass(px, b[0], b[2], size[0], filt)
    return np.ascontiguousarray(_pass(hz.transpose(1, 0, 2), b[1], b[3], size[1], filt).transpose(1, 0, 2))


def thumbnail_plan(width: int, height: int, size, gap):
    """``Image.thumbnail(size, f, gap)`` of a ``width x height`` JPEG: ``(draft
    level, final size, box in the draft frame | None)``; ``None``: no resize."""
    x, y = (math.floor(v) for v in size)
    if x >= width and y >= height:
        return 0, (width, height), None

    def round_aspect(number, key):
        return max(min(math.floor(number), math.ceil(number), key=key), 1)

    aspect = width / height
    if x / y >= aspect:
        x = round_aspect(y * aspect, key=lambda n: abs(aspect - n / y))
    else:
        y = round_aspect(x / aspect, key=lambda n: 0 if n == 0 else abs(aspect - x / n))
    level, box = 0, None
    if gap is not None:
        s = min(width // int(size[0] * gap), height // int(size[1] * gap))
        level = 3 if s >= 8 else 2 if s >= 4 else 1 if s >= 2 else 0
        box = (0, 0, width / (1 << level), height / (1 << level))
    frame = (-(-width // (1 << level)), -(-height // (1 << level)))
    return level, (x, y), (box or (0, 0) + frame) if frame != (x, y) else None


def thumbnail(data: bytes, width: int, height: int, size, filt: str, gap=2.0) -> np.ndarray:
    level, final, box = thumbnail_plan(width, height, size, gap)
    px = draft_ref.rgb_u8(data, level)
    return px if box is None else resize(px, final, filt, box, gap)
