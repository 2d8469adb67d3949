"""Reference and case table for ``draft=`` (include/spdl_hipjpeg.h "Pillow-exact
draft"): libjpeg-turbo's scaled decode restated from its rules in numpy int64
-- the three reduced transforms, the per-component size, then ``turbo_ref``'s
upsampling by the ratio that remains (replication at level 3) and colour.
Cases: gray and six samplings at 83x61, 9x7, 17x3 and one MCU (Pillow's
writer; tests/jpeg_writer with levels in all 64 places for 4:4:0 / 4:1:1 /
4:1:0), a progressive file, one with restart intervals, the RGB-coded one."""

import functools

import numpy as np

from oracle import oracle as O
from tests import cases, jpeg_writer as jw, turbo_ref as T
from tests.turbo_cases import pixels

LUMA = {"gray": (1, 1), "444": (1, 1), "422": (2, 1), "420": (2, 2), "440": (1, 2), "411": (4, 1),
        "410": (4, 2)}
NAMES = [f"{s}_{z}" for s in LUMA for z in ("83x61", "9x7", "17x3", "mcu")] + [
    "progressive", "restart", "rgb_coded"]


@functools.lru_cache(maxsize=None)
def case(name: str) -> bytes:
    if name == "progressive":
        return cases._enc(pixels(1, 83, 61), quality=88, subsampling=2, progressive=True)
    if name == "restart":
        return cases._enc(pixels(3, 83, 61), quality=88, subsampling=1, restart_marker_blocks=2)
    if name == "rgb_coded":
        return cases.case("rgb_coded")
    s, size = name.split("_")
    w, h = [8 * v for v in LUMA[s]] if size == "mcu" else map(int, size.split("x"))
    if s in ("gray", "444", "422", "420"):
        return cases._enc(pixels(7, w, h, 1 if s == "gray" else 3), quality=95,
                          subsampling=("444", "422", "420").index(s) if s != "gray" else -1)
    samp, rng = [LUMA[s], (1, 1), (1, 1)], np.random.default_rng(100 * w + h)
    levels = [rng.integers(-6, 7, size=(*g[0], 64)).astype(np.int32)
              for g in jw.block_grids(w, h, samp)]
    q = {i: rng.integers(2, 9, size=64) for i in (0, 1)}
    return jw.write_jpeg(w, h, samp, levels, q, [0, 1, 1], jw.std_tables(), [0, 1, 1], [0, 1, 1])


def FIX(x: float) -> int:
    return int(round(x * 8192))


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _limit(v):
    """libjpeg's range-limit table behind the +128: index v & 1023"""
    i = v & 1023
    return np.where(i < 128, i + 128, np.where(i < 512, 255, np.where(i < 896, 0, i - 896)))


def _pass4(r, s):
    """r: [..., 8] along the transformed axis (index 4 is not read) -> [..., 4]"""
    t0 = r[..., 0] << 14
    t2 = r[..., 2] * FIX(1.847759065) - r[..., 6] * FIX(0.765366865)
    a = (-r[..., 7] * FIX(0.211164243) + r[..., 5] * FIX(1.451774981)
         - r[..., 3] * FIX(2.172734803) + r[..., 1] * FIX(1.061594337))
    c = (-r[..., 7] * FIX(0.509795579) - r[..., 5] * FIX(0.601344887)
         + r[..., 3] * FIX(0.899976223) + r[..., 1] * FIX(2.562915447))
    return np.stack([_descale(t0 + t2 + c, s), _descale(t0 - t2 + a, s), _descale(t0 - t2 - a, s),
                     _descale(t0 + t2 - c, s)], -1)


def _pass2(r, s):
    t10 = r[..., 0] << 15
    t0 = (-r[..., 7] * FIX(0.720959822) + r[..., 5] * FIX(0.850430095)
          - r[..., 3] * FIX(1.272758580) + r[..., 1] * FIX(3.624509785))
    return np.stack([_descale(t10 + t0, s), _descale(t10 - t0, s)], -1)


def idct(blocks, pc: int):
    """blocks [n, 8, 8] (row, column), dequantised, DC without bias -> [n, pc, pc]:
    columns first, then rows, the same 1-D rule in both passes"""
    b = blocks.astype(np.int64)
    if pc == 1:
        return _limit(_descale(b[:, :1, :1], 3))
    rule, s1, s2 = (_pass4, 12, 19) if pc == 4 else (_pass2, 13, 20)
    ws = np.swapaxes(rule(np.swapaxes(b, 1, 2), s1), 1, 2)  # [n, k, column]
    return _limit(rule(ws, s2))


def comp_size(P: int, h: int, v: int, hmax: int, vmax: int) -> int:
    pc = P
    while pc < 8 and (hmax * P) % (h * pc * 2) == 0 and (vmax * P) % (v * pc * 2) == 0:
        pc *= 2
    return pc


def rgb_u8(data: bytes, level: int) -> np.ndarray:
    """[h, w, 3]: ``im.draft(...)`` to scale ``8 >> level`` eighths, then
    ``np.asarray(im.convert("RGB"))``."""
    if level == 0:
        return T.rgb_u8(data)
    info, P = O.parse(data), 8 >> level
    W, H = -(-info.width * P // 8), -(-info.height * P // 8)
    blocks = O.decode_coefs(data)[0].reshape(-1, 8, 8).astype(np.int64)
    blocks[:, 0, 0] -= 1024
    full8 = O.decode_planes(data, O.IDCT_ISLOW)
    gray = info.ncomp == 1
    hmax, vmax = (1, 1) if gray else (info.hmax, info.vmax)
    full = []
    for c in range(info.ncomp):
        h, v = (1, 1) if gray else (info.comp_h[c], info.comp_v[c])
        pc = comp_size(P, h, v, hmax, vmax)
        cw, ch = -(-info.width * h * pc // (8 * hmax)), -(-info.height * v * pc // (8 * vmax))
        plane = np.zeros((info.comp_bh[c] * pc, info.comp_bw[c] * pc), np.int64)
        if pc == 8:
            plane = full8[c]
        else:
            px = idct(blocks, pc)
            for j in range(info.nblocks):
                mcu, b = divmod(j, info.bpm)
                if info.mcu_comp[b] != c:
                    continue
                my, mx = divmod(mcu, info.mcux)
                bx, by = (mx, my) if gray else (mx * h + info.mcu_dx[b], my * v + info.mcu_dy[b])
                plane[by * pc:(by + 1) * pc, bx * pc:(bx + 1) * pc] = px[j]
        plane, hr, vr = plane[:ch, :cw], hmax * P // (h * pc), vmax * P // (v * pc)
        up = (np.repeat(np.repeat(plane.astype(np.int64), vr, axis=0), hr, axis=1) if level == 3
              else T.upsample(plane, hr, vr))
        full.append(up[:H, :W])
    if gray:
        return np.repeat(full[0][..., None], 3, axis=2).astype(np.uint8)
    return np.stack(full, -1).astype(np.uint8) if info.color == T.COLOR_RGB else T.ycc_rgb(*full)
