"""Reference for the source crop (include/spdl_hipjpeg.h "source crop"), written
from the rules there and from the oracle's whole-frame functions, not from the
product: libavfilter's ``crop`` (exact=0) on the decoder's frame moves the plane
pointers and shrinks the frame, and the chain then runs on that frame alone.

``resolve``       the rectangle rules, in Python
``region_planes`` the cropped planes: ``jo_decode_planes`` (+ ``jo_cmyk_transform``
                  for 4-component files), sliced per component
``rgb``           RGB outputs: the cropped planes packed as a frame of their own
                  (the bytes around them poisoned) through ``jo_resize_planes``
``planar``        ``pix_fmt="yuv"``: ``yuv_scale_ref`` on the cropped planes
"""

from __future__ import annotations

import copy
import ctypes

import numpy as np

from oracle import oracle as O
from tests import yuv_scale_ref as yref

CENTER = -(1 << 31)  # SPDL_HJ_CROP_CENTER
POISON = 0xAA


def ratios(ncomp: int, h_samp, v_samp) -> tuple[int, int]:
    """(hs, vs): the frame's chroma ratios (1, 1 unless it has three
    components: gray, and 4-component frames, which are all 1x1)."""
    if ncomp != 3:
        return 1, 1
    return max(h_samp[:3]) // h_samp[1], max(v_samp[:3]) // v_samp[1]


def _axis(pos: int, size: int, full: int, ratio: int):
    s = size // ratio * ratio if size > 0 else 0
    if s <= 0 or s > full:
        return None
    if pos == CENTER:
        if size % ratio:
            return None  # off-grid size, centred: refused
        pos = (full - s) // 2
    pos = max(pos, 0)
    if pos + s > full:
        pos = full - s
    return pos // ratio * ratio, s


def resolve(W: int, H: int, hs: int, vs: int, rect):
    """(x, y, w, h) of ``rect`` on a W x H frame with chroma ratios hs, vs;
    ``None``: refused (BAD_GEOMETRY).  (0, 0, 0, 0) is the whole frame."""
    x, y, w, h = rect
    if (x, y, w, h) == (0, 0, 0, 0):
        return 0, 0, W, H
    ax, ay = _axis(x, w, W, hs), _axis(y, h, H, vs)
    if ax is None or ay is None:
        return None
    return ax[0], ay[0], ax[1], ay[1]


def resolve_data(data: bytes, rect):
    info = O.parse(data)
    hs, vs = ratios(info.ncomp, list(info.comp_h), list(info.comp_v))
    return resolve(info.width, info.height, hs, vs, rect)


def region_planes(data: bytes, rect, idct: int = O.IDCT_SIMPLE):
    """(info, [plane per component]) of the resolved rectangle ``rect``: the
    decoder's planes (after FFmpeg's K transform for CMYK / YCCK), component c
    from (x / hs_c, y / vs_c), ceil(w / hs_c) x ceil(h / vs_c)."""
    info = O.parse(data)
    L = O.lib()
    L.jo_cmyk_transform.argtypes = [ctypes.POINTER(O._Info), ctypes.c_void_p]
    L.jo_cmyk_transform.restype = None
    buf = np.zeros(L.jo_planes_size(ctypes.byref(info)), np.uint8)
    a = np.frombuffer(data, np.uint8)
    rc = L.jo_decode_planes(a.ctypes.data, len(data), idct, buf.ctypes.data)
    if rc:
        raise O.OracleError(rc)
    if info.ncomp == 4:
        L.jo_cmyk_transform(ctypes.byref(info), buf.ctypes.data)
    x, y, w, h = rect
    planes, o = [], 0
    for c in range(info.ncomp):
        ph, pw = info.comp_bh[c] * 8, info.comp_bw[c] * 8
        hsc = 1 if info.ncomp == 1 else info.hmax // info.comp_h[c]
        vsc = 1 if info.ncomp == 1 else info.vmax // info.comp_v[c]
        pl = buf[o:o + ph * pw].reshape(ph, pw)
        cw, ch = -(-w // hsc), -(-h // vsc)
        planes.append(pl[y // vsc:y // vsc + ch, x // hsc:x // hsc + cw].copy())
        assert planes[-1].shape == (ch, cw)
        o += ph * pw
    return info, planes


def rgb(data: bytes, rect, rs: O.Resize | None, pix_fmt: str = "rgb24", idct: int = O.IDCT_SIMPLE,
        normalize: bool = False, norm_dtype: str = "float16") -> np.ndarray:
    """The RGB output of the resolved ``rect`` of ``data`` under ``rs`` (None:
    full resolution, the region itself)."""
    info0, planes = region_planes(data, rect, idct)
    info = copy.copy(info0)
    info.width, info.height = rect[2], rect[3]
    chunks = []
    for c, p in enumerate(planes):
        ch, cw = p.shape
        info.comp_w[c], info.comp_h_px[c] = cw, ch
        info.comp_bw[c], info.comp_bh[c] = -(-cw // 8), -(-ch // 8)
        box = np.full((info.comp_bh[c] * 8, info.comp_bw[c] * 8), POISON, np.uint8)
        box[:ch, :cw] = p
        chunks.append(box.reshape(-1))
    packed = np.concatenate(chunks)
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


def planar(data: bytes, rect, rs: O.Resize | None, idct: int = O.IDCT_SIMPLE) -> np.ndarray:
    """The ``pix_fmt="yuv"`` bytes (Y, U, V back to back) of the resolved
    ``rect`` under ``rs`` (None: the region's planes themselves)."""
    info, src = region_planes(data, rect, idct)
    if rs is None:
        return yref.packed(src)
    hs, vs = ratios(info.ncomp, list(info.comp_h), list(info.comp_v))
    gray = info.ncomp == 1
    g = O.geometry(rect[2], rect[3], rs)
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
