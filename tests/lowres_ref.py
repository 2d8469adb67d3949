"""Reference for the reduced-size decode (include/spdl_hipjpeg.h "reduced-size
decode"), written from the statement of FFmpeg's ``lowres`` transforms
(libavcodec/jrevdct.c ``ff_j_rev_dct4 / 2 / 1`` + the clipping put) and from
the oracle's whole-frame functions, not from the product:

``idct4 / idct2 / idct1``  the three transforms on [N, 8, 8] int coefficient
                           blocks (dequantised, natural order, DC + 1024)
``planes``                 the reduced planes of a file, per component, at the
                           reduced frame's component sizes
``rgb``                    RGB outputs: those planes packed as a frame of their
                           own (the bytes around them poisoned) through
                           ``jo_resize_planes``, as ``src_crop_ref.rgb`` does
``planar``                 ``pix_fmt="yuv"``: ``yuv_scale_ref`` on those planes

All arithmetic is int32 with arithmetic right shifts; numpy's int64 holds the
same values (nothing here leaves the int32 range, see ``_pass4``).
"""

from __future__ import annotations

import copy
import ctypes

import numpy as np

from oracle import oracle as O
from tests import yuv_scale_ref as yref

POISON = 0xAA
CONST_BITS, PASS1_BITS = 13, 2
FIX_0_541196100, FIX_0_765366865 = 4433, 6270
FIX_1_847759065, FIX_1_306562965 = 15137, 10703


def _clip(x):
    return np.clip(x, 0, 255).astype(np.uint8)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def idct1(b: np.ndarray) -> np.ndarray:
    """[N, 8, 8] -> [N, 1, 1]"""
    b = b.astype(np.int64)
    return _clip((b[:, 0, 0] + 4) >> 3)[:, None, None]


def idct2(b: np.ndarray) -> np.ndarray:
    """[N, 8, 8] -> [N, 2, 2]"""
    b = b.astype(np.int64)
    b00 = b[:, 0, 0] + 4
    d00, d01 = b00 + b[:, 0, 1], b00 - b[:, 0, 1]
    d10, d11 = b[:, 1, 0] + b[:, 1, 1], b[:, 1, 0] - b[:, 1, 1]
    out = np.stack([np.stack([(d00 + d10) >> 3, (d01 + d11) >> 3], -1),
                    np.stack([(d00 - d10) >> 3, (d01 - d11) >> 3], -1)], -2)
    return _clip(out)


def _pass4(d0, d2, d4, d6):
    """One even-half pass on (d0, d2, d4, d6); the zero-operand branches have
    their own constants and are taken as written."""
    both = (d6 != 0) & (d2 != 0)
    only6 = (d6 != 0) & (d2 == 0)
    only2 = (d6 == 0) & (d2 != 0)
    z1 = (d2 + d6) * FIX_0_541196100
    t2 = np.where(both, z1 - d6 * FIX_1_847759065,
                  np.where(only6, -d6 * FIX_1_306562965,
                           np.where(only2, d2 * FIX_0_541196100, 0)))
    t3 = np.where(both, z1 + d2 * FIX_0_765366865,
                  np.where(only6, d6 * FIX_0_541196100,
                           np.where(only2, d2 * FIX_1_306562965, 0)))
    t0, t1 = (d0 + d4) << CONST_BITS, (d0 - d4) << CONST_BITS
    out = [t0 + t3, t1 + t2, t1 - t2, t0 - t3]
    assert all(np.abs(o).max(initial=0) < (1 << 31) for o in out)
    return out


def idct4(b: np.ndarray) -> np.ndarray:
    """[N, 8, 8] -> [N, 4, 4]"""
    b = b.astype(np.int64)[:, :4, :4].copy()
    b[:, 0, 0] += 4
    ws = np.zeros_like(b)
    for r in range(4):
        o = _pass4(b[:, r, 0], b[:, r, 1], b[:, r, 2], b[:, r, 3])
        for k in range(4):  # stored as int16
            ws[:, r, k] = _descale(o[k], CONST_BITS - PASS1_BITS).astype(np.int16)
    out = np.zeros_like(b)
    for c in range(4):
        o = _pass4(ws[:, 0, c], ws[:, 1, c], ws[:, 2, c], ws[:, 3, c])
        for k in range(4):  # a plain shift: the + 4 on the DC is the rounding
            out[:, k, c] = o[k] >> (CONST_BITS + PASS1_BITS + 3)
    return _clip(out)


IDCT = {1: idct4, 2: idct2, 3: idct1}


def frame_size(w: int, h: int, level: int) -> tuple[int, int]:
    return -(-w >> level), -(-h >> level)


def comp_sizes(info, level: int) -> list[tuple[int, int]]:
    """(w, h) of every component's plane of the reduced frame."""
    fw, fh = frame_size(info.width, info.height, level)
    if info.ncomp == 1:
        return [(fw, fh)]
    return [(-(-fw * info.comp_h[c] // info.hmax), -(-fh * info.comp_v[c] // info.vmax))
            for c in range(info.ncomp)]


def planes(data: bytes, level: int):
    """(info, [plane per component]) at level 1..3."""
    info = O.parse(data)
    coefs, _ = O.decode_coefs(data)
    px = IDCT[level](coefs.reshape(-1, 8, 8))
    p = 8 >> level
    full = [np.zeros((info.comp_bh[c] * p, info.comp_bw[c] * p), np.uint8)
            for c in range(info.ncomp)]
    for j in range(info.nblocks):
        mcu, b = divmod(j, info.bpm)
        my, mx = divmod(mcu, info.mcux)
        c = info.mcu_comp[b]
        if info.ncomp == 1:
            bx, by = mx, my
        else:
            bx, by = mx * info.comp_h[c] + info.mcu_dx[b], my * info.comp_v[c] + info.mcu_dy[b]
        full[c][by * p:by * p + p, bx * p:bx * p + p] = px[j]
    out = []
    for c, (w, h) in enumerate(comp_sizes(info, level)):
        assert h <= full[c].shape[0] and w <= full[c].shape[1]
        out.append(full[c][:h, :w].copy())
    return info, out


def _framed(info0, src, w: int, h: int):
    """The planes as a frame of their own: a doctored info and the packed,
    block-padded planes (padding poisoned)."""
    info = copy.copy(info0)
    info.width, info.height = w, h
    chunks = []
    for c, p in enumerate(src):
        ch, cw = p.shape
        info.comp_w[c], info.comp_h_px[c] = cw, ch
        info.comp_bw[c], info.comp_bh[c] = -(-cw // 8), -(-ch // 8)
        box = np.full((info.comp_bh[c] * 8, info.comp_bw[c] * 8), POISON, np.uint8)
        box[:ch, :cw] = p
        chunks.append(box.reshape(-1))
    return info, np.concatenate(chunks)


def rgb(data: bytes, level: int, rs: O.Resize | None, pix_fmt: str = "rgb24",
        normalize: bool = False, norm_dtype: str = "float16") -> np.ndarray:
    """The RGB output of ``data`` at ``level`` under ``rs`` (None: the reduced
    frame itself)."""
    info0, src = planes(data, level)
    info, packed = _framed(info0, src, *frame_size(info0.width, info0.height, level))
    rs = rs or O.Resize()
    g = O.geometry(info.width, info.height, rs)
    out = np.zeros(g["ow"] * g["oh"] * 3, np.uint16 if normalize else np.uint8)
    m = np.asarray(O.IMAGENET_MEAN, np.float32)
    s = np.asarray(O.IMAGENET_STD, np.float32)
    dtype = (O.DTYPE_BF16 if norm_dtype == "bfloat16" else O.DTYPE_F16) if normalize else O.DTYPE_U8
    rc = O.lib().jo_resize_planes(ctypes.byref(info), packed.ctypes.data, ctypes.byref(rs._c()),
                                  O.FMT[pix_fmt], dtype, m.ctypes.data, s.ctypes.data,
                                  out.ctypes.data, None)
    if rc:
        raise O.OracleError(rc)
    if normalize and norm_dtype != "bfloat16":
        out = out.view(np.float16)
    return out.reshape((3, g["oh"], g["ow"]) if pix_fmt in ("rgb", "bgr") else (g["oh"], g["ow"], 3))


def planar(data: bytes, level: int, rs: O.Resize | None) -> np.ndarray:
    """The ``pix_fmt="yuv"`` bytes (Y, U, V back to back) at ``level`` under
    ``rs`` (None: the reduced planes themselves); scale only, or scale + pad /
    crop on the chroma grid."""
    info, src = planes(data, level)
    if rs is None:
        return yref.packed(src)
    gray = info.ncomp == 1
    hs = 1 if gray else info.hmax // info.comp_h[1]
    vs = 1 if gray else info.vmax // info.comp_v[1]
    g = O.geometry(*frame_size(info.width, info.height, level), rs)
    sw, sh, ow, oh = g["sw"], g["sh"], g["ow"], g["oh"]
    bw, bh, px, py = sw, sh, 0, 0
    if rs.pad_w > 0 and rs.pad_h > 0:
        bw, bh = rs.pad_w, rs.pad_h
        if sw % hs or bw % hs or sh % vs or bh % vs:
            raise yref.Refused("pad of a size off the chroma grid")
        px, py = (bw - sw) // 2 // hs * hs, (bh - sh) // 2 // vs * vs
    cx = cy = 0
    if rs.crop_w > 0 and rs.crop_h > 0:
        if ow % hs or oh % vs:
            raise yref.Refused("crop size off the chroma grid")
        cx, cy = (bw - ow) // 2 // hs * hs, (bh - oh) // 2 // vs * vs
    dx, dy = px - cx, py - cy
    out = [yref.place(yref.scale_plane(src[0], sw, sh, rs.filter), ow, oh, dx, dy,
                      16 if gray else 0)]
    if not gray:
        csw, csh, cw, ch = -(-sw // hs), -(-sh // vs), -(-ow // hs), -(-oh // vs)
        for c in (1, 2):
            out.append(yref.place(yref.scale_plane(src[c], csw, csh, rs.filter), cw, ch,
                                  dx // hs, dy // vs, 128))
    return yref.packed(out)
