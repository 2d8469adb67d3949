"""Inputs of the reduced-size decode tests (tests/test_lowres.py,
tests/test_gpu_lowres.py): small files of every sampling at the sizes where
the reduced planes have partial blocks, lanes past a component's last block
and more than one block row, plus one hand-written file whose AC energy lies
outside the 4x4 corner."""

from __future__ import annotations

import functools

import numpy as np

from spdl_amd.synthetic import synthetic_pixels
from tests import cases
from tests import jpeg_writer as jw
from tests import jpeg_writer_cases as jwc

SIZES = [(8, 8), (17, 9), (33, 31), (50, 37), (64, 48)]
SAMPLINGS = ["gray", "444", "422", "420", "440", "411"]
_PILLOW = {"444": 0, "422": 1, "420": 2}


@functools.lru_cache(maxsize=None)
def sized(samp: str, w: int, h: int, **kw) -> bytes:
    """A ``w x h`` file of sampling ``samp``; ``kw``: Pillow's save options
    (``progressive=True``, ``restart_marker_blocks=2``) for the Pillow-written ones."""
    seed = 100 + 7 * w + h
    if samp == "gray":
        return cases._enc(synthetic_pixels(seed, h, w)[..., 0], quality=90, **kw)
    if samp in _PILLOW:
        return cases._enc(synthetic_pixels(seed, h, w), quality=90, subsampling=_PILLOW[samp], **kw)
    assert not kw
    return jwc._sampling_case(samp, w, h, 0).data  # 4:4:0, 4:1:1: hand-written


@functools.lru_cache(maxsize=None)
def outside_corner(w: int = 50, h: int = 37) -> bytes:
    """4:2:0, every block a DC and AC levels only where the natural row or
    column is >= 4 -- some at zig-zag indices below 24 (the list walk passes
    them by), some above (it stops there), and every fourth block with its
    first entry above 24."""
    samp = [(2, 2), (1, 1), (1, 1)]
    rng = np.random.default_rng(77)
    nat = np.asarray(jw.NATURAL)
    outside = [k for k in range(1, 64) if nat[k] // 8 >= 4 or nat[k] % 8 >= 4]
    low, high = [k for k in outside if k < 24], [k for k in outside if k > 24]
    levels = []
    for bh, bw in [g[0] for g in jw.block_grids(w, h, samp)]:
        lv = np.zeros((bh, bw, 64), np.int32)
        lv[..., 0] = rng.integers(-60, 61, size=(bh, bw))
        for y in range(bh):
            for x in range(bw):
                ks = list(rng.choice(high, 5, replace=False))
                if (y * bw + x) % 4:
                    ks += list(rng.choice(low, 3, replace=False))
                lv[y, x, ks] = rng.integers(1, 13, size=len(ks)) * rng.choice([-1, 1], len(ks))
        levels.append(lv)
    q = {i: rng.integers(1, 7, size=64) for i in (0, 1)}
    ids = [0, 1, 1]
    return jw.write_jpeg(w, h, samp, levels, q, ids, jw.std_tables(), ids, ids)


def smooth_444(seed: int, w: int = 64, h: int = 48) -> bytes:
    """A smooth 4:4:4 file: low-pass noise, so the box average is a fair
    yardstick of the reduced planes' scale and bias."""
    rng = np.random.default_rng(seed)
    coarse = rng.uniform(32, 224, size=(h // 8 + 2, w // 8 + 2, 3))
    yy, xx = np.mgrid[0:h, 0:w] / 8.0
    y0, x0 = yy.astype(int), xx.astype(int)
    fy, fx = (yy - y0)[..., None], (xx - x0)[..., None]
    px = ((1 - fy) * (1 - fx) * coarse[y0, x0] + (1 - fy) * fx * coarse[y0, x0 + 1] +
          fy * (1 - fx) * coarse[y0 + 1, x0] + fy * fx * coarse[y0 + 1, x0 + 1])
    return cases._enc(np.clip(px + 0.5, 0, 255).astype(np.uint8), quality=95, subsampling=0)
