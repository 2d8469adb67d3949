"""Reference for ``csc="turbo"`` (include/spdl_hipjpeg.h "Pillow-exact
decode"): libjpeg-turbo's default decoder behind the islow IDCT, written from
the statement of its rules, not from the product:

``upsample``   one component's true plane to ``hr x vr`` times its size: the
               three triangle ("fancy") rules, box replication for every other
               ratio and for a plane of one or two columns
``ycc_rgb``    the 6b colour tables (green from FIX(0.34414) = 22554)
``rgb``        a file's output in any of the four layouts, u8 or normalised

All arithmetic is on numpy int64 with arithmetic right shifts; nothing leaves
the int32 range (the largest term is 116130 * 127 + 32768).
"""

from __future__ import annotations

import numpy as np

from oracle import oracle as O

COLOR_RGB = 2  # spdl_hj_color


def _left(p):
    return np.concatenate([p[:, :1], p[:, :-1]], axis=1)


def _right(p):
    return np.concatenate([p[:, 1:], p[:, -1:]], axis=1)


def _above(p):
    return np.concatenate([p[:1], p[:-1]], axis=0)


def _below(p):
    return np.concatenate([p[1:], p[-1:]], axis=0)


def upsample(plane: np.ndarray, hr: int, vr: int) -> np.ndarray:
    """[ch, cw] -> [ch * vr, cw * hr]; a neighbour outside the plane is the
    edge sample."""
    p = plane.astype(np.int64)
    ch, cw = p.shape
    if (hr, vr) == (1, 1):
        return p
    out = np.empty((ch * vr, cw * hr), np.int64)
    if (hr, vr) == (2, 1) and cw > 2:
        out[:, 0::2] = (3 * p + _left(p) + 1) >> 2
        out[:, 1::2] = (3 * p + _right(p) + 2) >> 2
    elif (hr, vr) == (1, 2):
        out[0::2] = (3 * p + _above(p) + 1) >> 2
        out[1::2] = (3 * p + _below(p) + 2) >> 2
    elif (hr, vr) == (2, 2) and cw > 2:
        for r, s in ((0, 3 * p + _above(p)), (1, 3 * p + _below(p))):
            out[r::2, 0::2] = (3 * s + _left(s) + 8) >> 4
            out[r::2, 1::2] = (3 * s + _right(s) + 7) >> 4
    else:
        out = np.repeat(np.repeat(p, vr, axis=0), hr, axis=1)
    return out


def ycc_rgb(y, cb, cr):
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def from_planes(info, planes) -> np.ndarray:
    """[H, W, 3] RGB of the true component planes of a 1- or 3-component frame."""
    W, H = info.width, info.height
    if info.ncomp == 1:
        return np.repeat(planes[0][:H, :W, None], 3, axis=2)
    assert info.ncomp == 3
    full = [upsample(planes[c], info.hmax // info.comp_h[c], info.vmax // info.comp_v[c])[:H, :W]
            for c in range(3)]
    if info.color == COLOR_RGB:
        return np.stack(full, -1).astype(np.uint8)
    return ycc_rgb(*full)


def rgb_u8(data: bytes) -> np.ndarray:
    """[H, W, 3]: what ``np.asarray(PIL.Image.open(f).convert("RGB"))`` is."""
    return from_planes(O.parse(data), O.decode_planes(data, O.IDCT_ISLOW))


def to_bf16_bits(f: np.ndarray) -> np.ndarray:
    """float32 -> bfloat16 bit patterns, round to nearest even."""
    x = f.astype(np.float32).view(np.uint32).astype(np.uint64)
    return ((x + 0x7FFF + ((x >> 16) & 1)) >> 16).astype(np.uint16)


def layout(px: np.ndarray, pix_fmt: str = "rgb24", normalize: bool = False,
           norm_dtype: str = "float16", mean=O.IMAGENET_MEAN, std=O.IMAGENET_STD) -> np.ndarray:
    """[H, W, 3] RGB u8 in the output's layout; normalised: (x / 255 - mean) /
    std in float32, mean and std by the position of the channel in the output,
    then float16 or bfloat16 (both as uint16 bit patterns)."""
    if pix_fmt in ("bgr", "bgr24"):
        px = px[..., ::-1]
    if normalize:
        f = px.astype(np.float32) / np.float32(255)
        f = (f - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
        assert f.dtype == np.float32
        px = to_bf16_bits(f) if norm_dtype == "bfloat16" else f.astype(np.float16).view(np.uint16)
    if pix_fmt in ("rgb", "bgr"):
        px = np.moveaxis(px, 2, 0)
    return np.ascontiguousarray(px)


def rgb(data: bytes, pix_fmt: str = "rgb24", **norm) -> np.ndarray:
    return layout(rgb_u8(data), pix_fmt, **norm)
