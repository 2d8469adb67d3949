"""numpy restatement of the planar output (``pix_fmt="yuv"``): the FFmpeg
chain ``scale[,pad][,crop]`` with no format node, on the decoder's own frame.

Written from the rules, not from the product code:

  * one swscale context yuvj4xxp -> yuvj4xxp (gray8 -> gray8).  The chroma
    planes are ceil(w / hs) x ceil(h / vs) on both sides; every plane has its
    own filters, all with centred siting (positions 128 -> 128):
    ``oracle.sws_axis(src, dst, filt, align=4, one=1 << 14)`` horizontally,
    ``align=2, one=1 << 12`` vertically;
  * hScale8To15: ``min((sum tap * x) >> 7, 32767)`` per source row;
  * swscale's 8-bit planar writers: a vertical filter of size 1 gives
    ``clip8((x + 64) >> 7)`` (yuv2plane1_8_c), any other size
    ``clip8((2^18 + sum tap * x) >> 19)`` (yuv2planeX_8_c, dither 64);
  * pad (centred, black) and crop (centred) move whole planes on the chroma
    grid: x offsets round down to a multiple of hs, y offsets to one of vs;
    black is Y 0, U = V 128 for yuvj and 16 for gray8;
  * the planes are packed Y, U, V, each tightly (av_image_copy_to_buffer).

Source planes come from ``oracle.decode_planes``, the scaled size from
``oracle.geometry`` (ratio-free: sizes do not depend on the subsampling).
"""

from __future__ import annotations

import functools

import numpy as np

from oracle import oracle as O


def frame_format(data: bytes) -> tuple[int, int, bool]:
    """(hs, vs, gray) of the frame: the chroma ratios from the SOF factors."""
    info = O.parse(data)
    if info.ncomp == 1:
        return 1, 1, True
    planes = O.decode_planes(data)
    (H, W), (ch, cw) = planes[0].shape, planes[1].shape
    hs = 1 if cw == W else 2
    vs = 1 if ch == H else 2
    assert cw == -(-W // hs) and ch == -(-H // vs), "not a 4:4:4 / 4:2:2 / 4:2:0 frame"
    return hs, vs, False


@functools.lru_cache(maxsize=None)
def _axis(src: int, dst: int, filt: str, vertical: bool):
    if vertical:
        return O.sws_axis(src, dst, filt, align=2, one=1 << 12, src_pos=128, dst_pos=128)
    return O.sws_axis(src, dst, filt, align=4, one=1 << 14, src_pos=128, dst_pos=128)


def hscale(plane: np.ndarray, dst_w: int, filt: str) -> np.ndarray:
    """hScale8To15 of every row: [H, dst_w] int32 (15-bit samples)."""
    pos, co = _axis(plane.shape[1], dst_w, filt, False)
    acc = np.zeros((plane.shape[0], dst_w), np.int64)
    src = plane.astype(np.int64)
    last = plane.shape[1] - 1
    for j in range(co.shape[1]):
        # (a tap past the row's end is zero: initFilter folds the borders)
        acc += src[:, np.minimum(pos + j, last)] * co[:, j].astype(np.int64)[None, :]
    return np.minimum(acc >> 7, (1 << 15) - 1)


def vscale(rows: np.ndarray, dst_h: int, filt: str) -> np.ndarray:
    """The planar writers over the 15-bit rows: [dst_h, W] uint8."""
    pos, co = _axis(rows.shape[0], dst_h, filt, True)
    if co.shape[1] == 1:  # yuv2plane1_8_c
        return np.clip((rows[pos] + 64) >> 7, 0, 255).astype(np.uint8)
    acc = np.full((dst_h, rows.shape[1]), 1 << 18, np.int64)  # yuv2planeX_8_c
    last = rows.shape[0] - 1
    for j in range(co.shape[1]):
        acc += rows[np.minimum(pos + j, last)] * co[:, j].astype(np.int64)[:, None]
    return np.clip(acc >> 19, 0, 255).astype(np.uint8)


def scale_plane(plane: np.ndarray, dst_w: int, dst_h: int, filt: str) -> np.ndarray:
    return vscale(hscale(plane, dst_w, filt), dst_h, filt)


def place(plane: np.ndarray, box_w: int, box_h: int, x: int, y: int, fill: int) -> np.ndarray:
    """`plane` at (x, y) of a box_w x box_h plane of `fill` (pad: x, y >= 0;
    crop: <= 0), clipped to the box."""
    out = np.full((box_h, box_w), fill, np.uint8)
    h, w = plane.shape
    x0, y0 = max(x, 0), max(y, 0)
    x1, y1 = min(x + w, box_w), min(y + h, box_h)
    if x0 < x1 and y0 < y1:
        out[y0:y1, x0:x1] = plane[y0 - y:y1 - y, x0 - x:x1 - x]
    return out


class Refused(Exception):
    """A geometry the library refuses for a subsampled frame (the header's
    pad / crop rules): the reference states no pixels for it."""


def scale_planes(data: bytes, rs: O.Resize, idct: int = O.IDCT_SIMPLE,
                 scaled: tuple[int, int] | None = None) -> list[np.ndarray]:
    """The output planes of `data` under the chain `rs` (Y, or Y, U, V).
    `scaled`: the scale node's output size given explicitly (negative scale
    sizes, which ``oracle.geometry`` does not know)."""
    hs, vs, gray = frame_format(data)
    src = O.decode_planes(data, idct)
    H, W = src[0].shape
    if scaled is None:
        g = O.geometry(W, H, rs)
        sw, sh = g["sw"], g["sh"]
    else:
        sw, sh = scaled
    # the pad box and the crop window, offsets on the chroma grid
    bw, bh, px, py = sw, sh, 0, 0
    if rs.pad_w > 0 and rs.pad_h > 0:
        bw, bh = rs.pad_w, rs.pad_h
        if sw % hs or bw % hs or sh % vs or bh % vs:
            raise Refused("pad of a size off the chroma grid")
        px, py = (bw - sw) // 2 // hs * hs, (bh - sh) // 2 // vs * vs
    ow, oh, cx, cy = bw, bh, 0, 0
    if rs.crop_w > 0 and rs.crop_h > 0:
        ow, oh = rs.crop_w, rs.crop_h
        if ow % hs or oh % vs:
            raise Refused("crop size off the chroma grid")
        cx, cy = (bw - ow) // 2 // hs * hs, (bh - oh) // 2 // vs * vs
    dx, dy = px - cx, py - cy
    out = [place(scale_plane(src[0], sw, sh, rs.filter), ow, oh, dx, dy, 16 if gray else 0)]
    if not gray:
        csw, csh = -(-sw // hs), -(-sh // vs)
        cw, ch = -(-ow // hs), -(-oh // vs)
        for c in (1, 2):
            out.append(place(scale_plane(src[c], csw, csh, rs.filter), cw, ch, dx // hs, dy // vs,
                             128))
    return out


def packed(planes: list[np.ndarray]) -> np.ndarray:
    return np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in planes])


def scale_packed(data: bytes, rs: O.Resize, idct: int = O.IDCT_SIMPLE,
                 scaled: tuple[int, int] | None = None) -> np.ndarray:
    return packed(scale_planes(data, rs, idct, scaled))
