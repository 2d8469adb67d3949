"""The shared case table of the ``csc="turbo"`` tests (tests/test_turbo.py,
tests/test_gpu_turbo.py): small, deterministic files, each noise over a ramp,
so that a plane's edge samples and the block padding behind them differ from
their neighbours.

  Pillow-written 4:4:4 / 4:2:2 / 4:2:0 and libjpeg-9-written non-interleaved
  files with luma factors (1,2), (4,1), (4,2), (1,4), at sizes that give a
  chroma plane of 1, 2 (box fallback) and 3 (first triangle width) columns, a
  single chroma row, and odd sizes whose last real column or row is not the
  block's last; the sizes around turbo_rgb_kernel's 128 x 32 tile; one
  progressive, optimised-table, restart-interval, gray and RGB-coded file; and
  a hand-written file whose luma is sampled below its chroma.

The libjpeg-9-written files are committed (tests/golden/turbo_lj9.npz): Pillow
cannot write them.  ``python -m tests.turbo_cases`` writes that file again
where the oracle's libjpeg 9 helper is built.
"""

from __future__ import annotations

import functools
import os

import numpy as np

from tests import cases
from tests import jpeg_writer as jw

TILE_W, TILE_H = 128, 32  # turbo_rgb_kernel's tile (hj_common.h kTurboTileW / H)

SIZES = [(1, 1), (2, 2), (3, 1), (4, 3), (5, 2), (6, 5), (7, 4), (8, 8), (9, 6), (9, 7), (15, 9),
         (16, 17), (17, 15), (33, 16), (33, 33)]
TILE_SIZES = [(TILE_W - 1, TILE_H - 1), (TILE_W, TILE_H), (TILE_W + 1, TILE_H + 1),
              (2 * TILE_W + 1, 2 * TILE_H + 1)]
PILLOW = {"444": 0, "422": 1, "420": 2}
LJ9 = {"l12": (1, 2), "l41": (4, 1), "l42": (4, 2), "l14": (1, 4)}
LJ9_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "turbo_lj9.npz")


def pixels(seed: int, w: int, h: int, c: int = 3) -> np.ndarray:
    """Noise over a ramp, [h, w, c] (c == 1: [h, w])."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = np.stack([(xx * 7 + yy * 3) % 256, (xx * 2 + yy * 5 + 80) % 256,
                     (255 - xx * 3 - yy * 4) % 256], -1)[..., :c]
    px = np.clip(ramp + rng.integers(-48, 49, size=ramp.shape), 0, 255).astype(np.uint8)
    return px[..., 0] if c == 1 else px


def _seed(w: int, h: int) -> int:
    return 9000 + 131 * w + h


@functools.lru_cache(maxsize=None)
def _lj9() -> dict:
    with np.load(LJ9_FILE) as z:
        return {k: z[k].tobytes() for k in z.files}


def _lj9_names():
    return [f"{s}_{w}x{h}" for s in LJ9 for w, h in SIZES]


@functools.lru_cache(maxsize=None)
def luma_below_chroma(w: int = 21, h: int = 13) -> bytes:
    """(1x1, 2x2, 2x2): the luma plane is the subsampled one."""
    samp = [(1, 1), (2, 2), (2, 2)]
    rng = np.random.default_rng(4242)
    levels = []
    for bh, bw in [g[0] for g in jw.block_grids(w, h, samp)]:
        lv = np.zeros((bh, bw, 64), np.int32)
        lv[..., 0] = rng.integers(-40, 41, size=(bh, bw))
        lv[..., 1:10] = rng.integers(-12, 13, size=(bh, bw, 9))
        levels.append(lv)
    q = {i: rng.integers(2, 9, size=64) for i in (0, 1)}
    ids = [0, 1, 1]
    return jw.write_jpeg(w, h, samp, levels, q, ids, jw.std_tables(), ids, ids)


@functools.lru_cache(maxsize=None)
def case(name: str) -> bytes:
    if name == "progressive":
        return cases._enc(pixels(1, 35, 21), quality=88, subsampling=2, progressive=True)
    if name == "optimized":
        return cases._enc(pixels(2, 35, 21), quality=88, subsampling=1, optimize=True)
    if name == "restart":
        return cases._enc(pixels(3, 35, 21), quality=88, subsampling=2, restart_marker_blocks=2)
    if name == "gray":
        return cases._enc(pixels(4, 35, 21, 1), quality=88)
    if name == "rgb_coded":
        return cases.case("rgb_coded")
    if name == "luma_below_chroma":
        return luma_below_chroma()
    samp, size = name.split("_")
    w, h = map(int, size.split("x"))
    if samp in PILLOW:
        q = 95 if (w + h) % 2 else 75
        return cases._enc(pixels(_seed(w, h), w, h), quality=q, subsampling=PILLOW[samp])
    return _lj9()[name]


SPECIAL = ["progressive", "optimized", "restart", "gray", "rgb_coded", "luma_below_chroma"]
NAMES = ([f"{s}_{w}x{h}" for s in PILLOW for w, h in SIZES] + _lj9_names() +
         [f"420_{w}x{h}" for w, h in TILE_SIZES] +
         [f"422_{TILE_W + 1}x{TILE_H + 1}", f"444_{TILE_W + 1}x{TILE_H + 1}"] + SPECIAL)
# three cases for the formats x dtypes product: triangle on both axes with an
# odd width, the horizontal-only rule, and a box-replicated 4:1 ratio
FORMAT_CASES = ["420_17x15", "422_9x7", "l41_15x9"]


def _regen() -> None:
    from oracle import oracle as O

    out = {}
    for s, (h0, v0) in LJ9.items():
        for w, h in SIZES:
            out[f"{s}_{w}x{h}"] = np.frombuffer(
                O.lj_encode_multiscan(pixels(_seed(w, h) + h0, w, h), 90, h0, v0), np.uint8)
    np.savez(LJ9_FILE, **out)
    print(f"{LJ9_FILE}: {len(out)} files, {os.path.getsize(LJ9_FILE)} bytes")


if __name__ == "__main__":
    _regen()
