"""Pillow-exact thumbnail on the GPU (include/spdl_hipjpeg.h "Pillow-exact
thumbnail"): float boxes, Image.reduce, reducing_gap and Image.thumbnail, every
pixel equal to Pillow's own array."""

import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

import spdl_amd.io as sio
from spdl_amd._lib import Output, Resample
from tests import cases, turbo_ref
from tests.test_gpu_resample import BAD_GEOMETRY, GUARD, INVALID_ARG, TURBO, _decode, _plain_follows
from tests.test_gpu_turbo import _raw
from tests.test_resample import BENCH, PIL_FILTER
from tests.turbo_cases import pixels

pytestmark = pytest.mark.gpu
CFG = sio.cuda_config(device_index=0)


@functools.lru_cache(maxsize=None)
def jpeg(w: int, h: int, sub: int = 2) -> bytes:
    return cases._enc(pixels(11, w, h), quality=92, subsampling=sub)


def pillow(data, size, filt, box=None, gap=None) -> np.ndarray:
    im = Image.open(io.BytesIO(data)).convert("RGB")
    return np.asarray(im.resize(size, PIL_FILTER[filt], box=box, reducing_gap=gap))


def rs_box(filt, size, boxes, gap=None):
    return Resample(filt, *size, tuple((b, size, (0, 0)) for b in boxes), True, gap)


# (frame, target, filter, box, gap, factors)
RESIZES = [((97, 75), (40, 30), f, (3.25, 2.5, 90.75, 70.125), None, (1, 1)) for f in PIL_FILTER]
RESIZES += [
    ((97, 75), (97, 75), "bicubic", (0.5, 0.25, 97, 75), None, (1, 1)),  # taps cross the box's edge
    ((200, 160), (40, 32), "bicubic", None, 2.0, (2, 2)),
    ((199, 157), (33, 39), "lanczos", None, 2.0, (3, 2)),     # partial right, bottom and corner cells
    ((97, 150), (60, 25), "bilinear", None, 2.0, (1, 3)),
    ((200, 160), (12, 10), "bicubic", None, 1.0, (16, 16)),   # fx fy = 256, the cap
    ((200, 160), (30, 25), "bicubic", (21.5, 13.25, 180.0, 150.5), 2.0, (2, 2)),  # safe box from (13, 5)
    ((200, 160), (70, 20), "bilinear", None, 1.0, (2, 8)),    # two tiles across
    ((640, 480), (14, 12), "lanczos", None, 3.0, (15, 13)),   # 275 taps without the gap
]


@pytest.mark.parametrize("frame,size,filt,box,gap,factors", RESIZES, ids=str)
def test_resize_table(decoder, oracle, frame, size, filt, box, gap, factors):
    data = open(BENCH, "rb").read() if frame == (640, 480) else jpeg(*frame)
    want = pillow(data, size, filt, box, gap)
    st, got = _decode(decoder, [data], TURBO, want.shape, resample=rs_box(filt, size, [box], gap))
    assert st == [0] and decoder.get_param("reduce_images") == (factors != (1, 1))
    assert decoder.get_param("resample_workgroups") > 0
    np.testing.assert_array_equal(got[0], want, strict=True)


@pytest.mark.parametrize("pix_fmt,norm", [("rgb24", "float16"), ("bgr", None)])
def test_reduce_formats_and_dtypes(decoder, oracle, pix_fmt, norm):
    kw = dict(normalize=True, norm_dtype=norm) if norm else {}
    data = jpeg(199, 157)
    want = turbo_ref.layout(pillow(data, (33, 39), "bicubic", None, 2.0), pix_fmt, **kw)
    st, got = _decode(decoder, [data], Output(pix_fmt=pix_fmt, csc="turbo", **kw), want.shape,
                      resample=rs_box("bicubic", (33, 39), [None], 2.0))
    assert st == [0] and decoder.get_param("reduce_images") == 1
    np.testing.assert_array_equal(got[0], want, strict=True)


def test_mixed_factors_and_refusals_in_one_submission(decoder, oracle):
    """Factors (1, 1) and (2, 2) beside the factor cap (80 x 60 cells) and a
    tall frame, each refused alone."""
    datas = [jpeg(97, 75, 0), open(BENCH, "rb").read(), jpeg(200, 160), jpeg(2, 300, 0)]
    boxes = [None, (0, 0, 640, 480), (0.5, 0, 200, 159.5), None]
    st, got = _decode(decoder, datas, TURBO, (30, 40, 3), resample=rs_box("bicubic", (40, 30), boxes, 2.0))
    assert st == [0, 0, 0, BAD_GEOMETRY] and decoder.get_param("reduce_images") == 2
    for k in range(3):
        np.testing.assert_array_equal(got[k], pillow(datas[k], (40, 30), "bicubic", boxes[k], 2.0), strict=True)
    assert (got[3] == GUARD).all()
    st, got = _decode(decoder, datas[:2], TURBO, (8, 8, 3), resample=rs_box("bicubic", (8, 8), [None, None], 1.0))
    assert st == [0, BAD_GEOMETRY] and (got[1] == GUARD).all()  # (12 x 9 cells; 80 x 60)
    np.testing.assert_array_equal(got[0], pillow(datas[0], (8, 8), "bicubic", None, 1.0), strict=True)


@pytest.mark.parametrize("gap,box", [(0.5, None), (2.0, (0, 0, 97.5, 75)), (2.0, (5, 5, 5, 9))])
def test_invalid_arg_writes_nothing(decoder, oracle, gap, box):
    d = jpeg(97, 75)
    t = torch.full((40 * 30 * 3 + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    decoder.set_resample(rs_box("bicubic", (40, 30), [box], gap))
    rc, msg, _ = _raw(decoder, [d], TURBO, t.data_ptr(), 40 * 30 * 3)
    assert rc == INVALID_ARG and msg, (rc, msg)
    torch.cuda.synchronize()
    assert bool((t == GUARD).all()), "a refused submission wrote output"


# 640 x 480: draft levels 0, 1, 2, 3; level 3 and a reduce by 5; a 97 x 75 file that fits
@pytest.mark.parametrize("frame,size,level", [((640, 480), (200, 200), 0), ((640, 480), (100, 100), 1),
                                              ((640, 480), (50, 50), 2), ((640, 480), (25, 25), 3),
                                              ((640, 480), (8, 8), 3), ((97, 75), (128, 128), 0)])
def test_thumbnail(decoder, oracle, frame, size, level):
    data = open(BENCH, "rb").read() if frame == (640, 480) else jpeg(*frame)
    im = Image.open(io.BytesIO(data))
    im.thumbnail(size, Image.BICUBIC, reducing_gap=2.0)
    assert sio.pil_thumbnail(size).plan(*frame)[0] == level
    got = sio.to_torch(sio.load_image(data, csc="turbo", pix_fmt="rgb24", device_config=CFG,
                                      resample=sio.pil_thumbnail(size))).cpu().numpy()
    np.testing.assert_array_equal(got, np.asarray(im.convert("RGB")), strict=True)
    batch = sio.load_image_batch([data, data], width=None, height=None, csc="turbo", device_config=CFG,
                                 resample=sio.pil_thumbnail(size))
    np.testing.assert_array_equal(sio.to_torch(batch).cpu().numpy()[1], got, strict=True)


def test_batch_of_two_aspect_ratios_is_refused(oracle):
    with pytest.raises(ValueError, match="different sizes"):
        sio.load_image_batch([jpeg(97, 75), jpeg(75, 97)], width=None, height=None, csc="turbo",
                             device_config=CFG, resample=sio.pil_thumbnail((32, 32)))


def test_set_resample_alone_is_unchanged(decoder, oracle):
    d = jpeg(97, 75)
    st, got = _decode(decoder, [d], TURBO, (30, 40, 3), resample=Resample("bicubic", 40, 30))
    wgs = decoder.get_param("resample_workgroups")
    assert st == [0] and wgs == 1 and decoder.get_param("reduce_images") == 0
    np.testing.assert_array_equal(got[0], pillow(d, (40, 30), "bicubic"), strict=True)
    # ... and the whole frame as a float box: the same kernel, tiles and bytes
    st, box = _decode(decoder, [d], TURBO, (30, 40, 3), resample=rs_box("bicubic", (40, 30), [None]))
    assert st == [0] and decoder.get_param("resample_workgroups") == wgs
    np.testing.assert_array_equal(box[0], got[0], strict=True)
