"""Oriented resample items on the GPU (include/spdl_hipjpeg.h "Pillow-exact
orientation"): an item with code c is the item of ``im.transpose(METHOD[c])``,
every byte equal to Pillow's own array.  Files are written at test time."""

import ctypes
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image, ImageOps

import spdl_amd.io as sio
from spdl_amd import _lib
from spdl_amd._lib import Output, ResampleItems
from tests import jpeg_writer as jw, turbo_ref
from tests.test_resample import PIL_FILTER
from tests.turbo_cases import pixels

pytestmark = pytest.mark.gpu
CFG = sio.cuda_config(device_index=0)
INVALID_ARG, GUARD = 8, 0xA5
T = Image.Transpose
METHOD = {1: T.FLIP_LEFT_RIGHT, 2: T.FLIP_TOP_BOTTOM, 3: T.ROTATE_180, 4: T.TRANSPOSE,
          5: T.ROTATE_270, 6: T.ROTATE_90, 7: T.TRANSVERSE}
SAMP = {"444": (1, 1), "422": (2, 1), "420": (2, 2), "440": (1, 2)}
# 203 x 157: no multiple of 16; 75 x 45 written from a 2.6x shrink is 2 x 2 of the
# tiler's 64 x 32 tiles, whose 80-odd source rows take three 32-row strips.  5 x 3: under a unit row
BIG, SMALL = (203, 157), (5, 3)


@functools.lru_cache(maxsize=None)
def jpeg(samp: str, w: int, h: int, tag: int = 0) -> bytes:
    if samp == "440":  # (Pillow writes no 4:4:0)
        s, rng = [SAMP[samp], (1, 1), (1, 1)], np.random.default_rng(100 * w + h)
        levels = [rng.integers(-6, 7, size=(*g[0], 64)).astype(np.int32)
                  for g in jw.block_grids(w, h, s)]
        q = {i: rng.integers(2, 9, size=64) for i in (0, 1)}
        return jw.write_jpeg(w, h, s, levels, q, [0, 1, 1], jw.std_tables(), [0, 1, 1], [0, 1, 1])
    b, exif = io.BytesIO(), Image.Exif()
    if tag:
        exif[0x0112] = tag
    Image.fromarray(pixels(w + h, w, h)).save(b, "JPEG", quality=92, exif=exif,
                                              subsampling=("444", "422", "420").index(samp))
    return b.getvalue()


def pillow(im, code, box, clamp, rsz, window, filt, gap, flip) -> np.ndarray:
    im = im.convert("RGB")
    im = im.transpose(METHOD[code]) if code else im
    im = im.crop(box).resize(rsz, PIL_FILTER[filt], reducing_gap=gap) if clamp and box else \
        im.resize(rsz, PIL_FILTER[filt], box=box, reducing_gap=gap)
    ox, oy, w, h = window
    a = np.asarray(im)[oy:oy + h, ox:ox + w]
    return a[::-1 if flip & 2 else 1, ::-1 if flip & 1 else 1]


def run(decoder, datas, items, filt, out=Output(pix_fmt="rgb24", csc="turbo"), gap=None, draft=None):
    """items (image, box, clamp, (rw, rh), (ox, oy, w, h), flip, code) packed 64
    bytes apart into a guarded buffer: each item's elements."""
    esz = 1 if out.torch_dtype == torch.uint8 else 2
    offs, end = [], 0
    for it in items:
        offs.append(end)
        end += (it[4][2] * it[4][3] * 3 * esz + 63) // 64 * 64
    held = ResampleItems(filt, [(i, b, c, r, w[:2], w[2:], f, o, code)
                                for (i, b, c, r, w, f, code), o in zip(items, offs)], gap)
    t = torch.full((end + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    st = decoder.decode_batch(datas, out, t.data_ptr(), end, check=False, resample_items=held,
                              draft=draft)
    assert st == [0] * len(datas) and held.statuses == [0] * len(items)
    a = t.cpu().numpy()
    got = [a[o:o + it[4][2] * it[4][3] * 3 * esz].view(np.uint8 if esz == 1 else np.uint16)
           for o, it in zip(offs, items)]
    gaps = np.ones(end + 64, bool)
    for o, g in zip(offs, got):
        gaps[o:o + g.nbytes] = False
    assert (a[gaps] == GUARD).all(), "wrote outside the items' boxes"
    return got


def displayed(size, code):
    return size[::-1] if code & 4 else size


@pytest.mark.parametrize("samp", list(SAMP))
def test_codes_and_samplings(decoder, oracle, samp):
    """Bilinear, a clamped off-centre odd box, a window inside the resized
    picture and a flip on the odd codes: codes 1..7 of both frames in one submission."""
    datas, items = [jpeg(samp, *BIG), jpeg(samp, *SMALL)], []
    for code in range(1, 8):
        dw, dh = displayed(BIG, code)
        items.append((0, (5, 3, dw - 8, dh - 6), True, (90, 60), (7, 5, 75, 45), code & 1, code))
        items.append((1, None, True, displayed((7, 4), code), (0, 0, *displayed((7, 4), code)),
                      code & 2, code))
    got = run(decoder, datas, items, "bilinear")
    assert decoder.get_param("resample_items") == 14
    ims = [Image.open(io.BytesIO(d)) for d in datas]
    for (i, box, clamp, rsz, win, flip, code), g in zip(items, got):
        want = pillow(ims[i], code, box, clamp, rsz, win, "bilinear", None, flip)
        np.testing.assert_array_equal(g.reshape(want.shape), want, strict=True, err_msg=f"code {code}")


@pytest.mark.parametrize("what", ["reduce", "draft", "float_box"])
def test_reduce_draft_and_float_boxes(decoder, oracle, what):
    data, filt, gap, draft, frame = jpeg("420", *BIG), "lanczos", None, None, BIG
    if what == "reduce":  # (203 -> 16 and 157 -> 26 at gap 2: factors 6 x 3, turned 4 x 3; partial last cells)
        gap, req = 2.0, (None, False, (16, 26), (0, 0, 16, 26))
    elif what == "draft":  # (the boxes are the displayed DRAFT frame's)
        draft, frame, req = [1], (102, 79), (None, True, (31, 40), (2, 3, 27, 33))
    else:
        filt, req = "bicubic", ("float", False, (40, 37), (1, 0, 38, 37))
    items = []
    for code in range(1, 8):
        dw, dh = displayed(frame, code)
        box = (2.25, 1.5, dw - 3.75, dh - 0.5) if req[0] == "float" else req[0]
        items.append((0, box, *req[1:], code & 3, code))
    got = run(decoder, [data], items, filt, gap=gap, draft=draft)
    im = Image.open(io.BytesIO(data))
    if draft:
        im.draft("RGB", (101, 78))  # (scale 1/2: 102 x 79)
        assert im.size == frame
    for (_, box, clamp, rsz, win, flip, code), g in zip(items, got):
        want = pillow(im, code, box, clamp, rsz, win, filt, gap, flip)
        np.testing.assert_array_equal(g.reshape(want.shape), want, strict=True, err_msg=f"code {code}")


@pytest.mark.parametrize("dtype,code", [("float16", 5), ("bfloat16", 6)])
def test_planar_bgr_normalised(decoder, oracle, dtype, code):
    """float32 arithmetic on Pillow's bytes, then the dtype's rounding: the bit patterns"""
    data = jpeg("422", *BIG)
    out = Output(pix_fmt="bgr", csc="turbo", normalize=True, norm_dtype=dtype)
    item = (0, None, False, (67, 41), (0, 0, 67, 41), 1, code)
    (got,) = run(decoder, [data], [item], "bicubic", out)
    want = turbo_ref.layout(pillow(Image.open(io.BytesIO(data)), code, None, False, (67, 41),
                                   item[4], "bicubic", None, 1), "bgr", normalize=True,
                            norm_dtype=dtype)
    np.testing.assert_array_equal(got.reshape(want.shape), want.view(np.uint16), strict=True)


@pytest.mark.parametrize("rs", [sio.pil_resize((31, 23), "bicubic", exif_transpose=True),
                                sio.pil_thumbnail((40, 40), exif_transpose=True)], ids=["resize", "thumbnail"])
def test_exif_tags_through_load_image_list(decoder, oracle, rs):
    datas = [jpeg("420", 83, 61, tag) for tag in range(1, 9)]
    bufs, idx = sio.load_image_list(datas, csc="turbo", resample=rs, device_config=CFG)
    assert idx == list(range(8))
    for tag, data, buf in zip(range(1, 9), datas, bufs):
        im = ImageOps.exif_transpose(Image.open(io.BytesIO(data)))
        if hasattr(rs, "plan"):
            im.thumbnail(rs.size, PIL_FILTER[rs.filter], reducing_gap=rs.reducing_gap)
        else:
            im = im.resize(rs.size, PIL_FILTER[rs.filter])
        np.testing.assert_array_equal(sio.to_torch(buf).cpu().numpy(), np.asarray(im.convert("RGB")),
                                      strict=True, err_msg=f"tag {tag}")
    # (load_image and load_image_batch submit the same items)
    one = sio.load_image(datas[5], csc="turbo", resample=rs, device_config=CFG)
    both = sio.load_image_batch(datas[5:7], width=None, height=None, csc="turbo", resample=rs,
                                device_config=CFG)
    assert torch.equal(sio.to_torch(one), sio.to_torch(bufs[5]))
    assert torch.equal(sio.to_torch(both), torch.stack([sio.to_torch(b) for b in bufs[5:7]]))


@pytest.mark.parametrize("code,fmt", [(8, "rgb24"), (5, "Y")])
def test_refusals_write_nothing(decoder, oracle, code, fmt):
    data, out = jpeg("420", *BIG), Output(pix_fmt=fmt, csc="turbo")
    held = ResampleItems("bilinear", [(0, None, False, (20, 20), (0, 0), (20, 20), 0, 0, code)])
    t = torch.full((20 * 20 * 3 + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    keep = _lib.buffer_address(data)
    status, err, spec = (ctypes.c_int32 * 1)(), ctypes.create_string_buffer(1024), out.to_c()
    assert _lib.lib().spdl_hj_set_resample_items(decoder._h, *held._c(), held._status) == 0
    rc = _lib.lib().spdl_hj_decode_batch(decoder._h, (ctypes.c_void_p * 1)(keep[0]),
                                         (ctypes.c_size_t * 1)(keep[1]), 1, ctypes.byref(spec),
                                         t.data_ptr(), 20 * 20 * 3, None, 1, status, err, 1024)
    assert rc == INVALID_ARG
    torch.cuda.synchronize()
    assert bool((t == GUARD).all()), "a refused submission wrote output"


def test_unoriented_submission_is_unchanged_by_oriented_ones(decoder, oracle):
    """The same unoriented items before and after oriented submissions on the
    context: the same bytes and the same grid"""
    datas = [jpeg("420", *BIG), jpeg("444", *SMALL)]
    plain = [(0, (5, 3, 195, 151), True, (90, 60), (7, 5, 75, 45), 1, 0),
             (1, None, False, (7, 4), (0, 0, 7, 4), 0, 0)]
    before = run(decoder, datas, plain, "bilinear")
    wgs = decoder.get_param("resample_item_workgroups")
    for code in (3, 6):
        run(decoder, datas, [(*it[:6], code) for it in plain[1:]], "bilinear")
    after = run(decoder, datas, plain, "bilinear")
    assert decoder.get_param("resample_item_workgroups") == wgs
    for b, a in zip(before, after):
        np.testing.assert_array_equal(a, b, strict=True)
