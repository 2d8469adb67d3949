"""GPU tests of the Pillow-exact resize (include/spdl_hipjpeg.h; -m gpu):
resample_kernel through the C-ABI and the Python surface, byte-exact against
tests/resample_ref.py and, where it decodes with libjpeg-turbo, Pillow itself."""

import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image, features

import spdl_amd.io as sio
from spdl_amd._lib import Output, Resample, ViewGroup
from tests import resample_ref as ref
from tests import turbo_cases as tc
from tests import turbo_ref
from tests.test_gpu_turbo import _raw
from tests.test_resample import PIL_FILTER, SHAPES, TILED, data_of

pytestmark = pytest.mark.gpu

BAD_GEOMETRY, INVALID_ARG, GUARD = 7, 8, 0xA5
TURBO = Output(pix_fmt="rgb24", csc="turbo")


@functools.lru_cache(maxsize=None)
def _want(name, size, filt, box=None, window=None) -> np.ndarray:
    a = ref.decode_resize(data_of(name), size, filt, box, window)
    a.setflags(write=False)
    return a


def _decode(dec, datas, out, shape, **kw):
    """(statuses, [n, *shape]) of one decode_batch into a guarded buffer."""
    n = len(datas)
    esz = 1 if out.torch_dtype == torch.uint8 else 2
    per = int(np.prod(shape)) * esz
    t = torch.full(((n + 1) * per + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    st = dec.decode_batch(datas, out, t.data_ptr(), n * per, check=False, **kw)
    a = t.cpu().numpy()
    assert (a[n * per:] == GUARD).all(), "wrote past the batch's output"
    body = a[: n * per]
    if esz == 2:
        body = body.view(np.uint16)
    return st, body.reshape(n, *shape)


@pytest.mark.parametrize("filt", list(PIL_FILTER))
@pytest.mark.parametrize("name,size,box", SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_shape_table(decoder, oracle, name, size, box, filt):
    data = data_of(name)
    want = _want(name, size, filt, box)
    st, got = _decode(decoder, [data], TURBO, want.shape,
                      resample=Resample(filt, *size, None if box is None else ((box, size, (0, 0)),)))
    assert st == [0] and decoder.get_param("resample_workgroups") > 0
    assert decoder.get_param("turbo_workgroups") == 0
    np.testing.assert_array_equal(got[0], want, strict=True)
    if features.check_feature("libjpeg_turbo"):
        im = Image.open(io.BytesIO(data)).convert("RGB")
        if box is not None:
            im = im.crop((box[0], box[1], box[0] + box[2], box[1] + box[3]))
        np.testing.assert_array_equal(got[0], np.asarray(im.resize(size, PIL_FILTER[filt])), strict=True)
    if size == (33, 33) and box is None:  # the identity: the plain turbo decode
        np.testing.assert_array_equal(got[0], turbo_ref.rgb_u8(data), strict=True)


def test_tap_limit_refuses_one_image_alone(decoder, oracle):
    """640 -> 14, a 275-tap lanczos axis, beside an image that decodes."""
    st, got = _decode(decoder, [data_of("bench"), tc.case("420_33x33")], TURBO, (12, 14, 3),
                      resample=Resample("lanczos", 14, 12))
    assert st == [BAD_GEOMETRY, 0]
    assert (got[0] == GUARD).all()
    np.testing.assert_array_equal(got[1], _want("420_33x33", (14, 12), "lanczos"), strict=True)


@pytest.mark.parametrize("filt", list(PIL_FILTER))
def test_boxes_window_and_mixed_sources(decoder, oracle, filt):
    """One batch of different sizes and samplings into 24 x 24: odd boxes whose
    chroma neighbours lie outside them, a window of a 40 x 30 resize, gray,
    4:4:4, 4:2:2, 4:4:0, 4:1:1 and an RGB-coded file; one bad box between them."""
    win = (8, 3, 24, 24)
    rows = [("420_33x33", (24, 24), (3, 5, 21, 17), None), ("422_33x33", (24, 24), (3, 5, 21, 17), None),
            ("420_33x33", (24, 24), (0, 0, 1, 1), None), ("422_33x33", (24, 24), (0, 0, 1, 1), None),
            ("420_33x33", (40, 30), None, win), ("gray", (24, 24), None, None),
            ("444_17x15", (24, 24), None, None), ("422_9x7", (24, 24), None, None),
            ("l12_16x17", (24, 24), None, None), ("l41_15x9", (24, 24), None, None),
            ("rgb_coded", (24, 24), None, None)]
    items = [(box, size, w[:2] if w else (0, 0)) for _, size, box, w in rows]
    bad = len(rows) // 2
    datas = [tc.case(r[0]) for r in rows]
    datas.insert(bad, tc.case("420_33x33"))
    items.insert(bad, ((20, 0, 14, 8), (24, 24), (0, 0)))
    st, got = _decode(decoder, datas, TURBO, (24, 24, 3), resample=Resample(filt, 24, 24, tuple(items)))
    assert st == [BAD_GEOMETRY if k == bad else 0 for k in range(len(datas))]
    assert (got[bad] == GUARD).all()
    got = np.delete(got, bad, axis=0)
    for k, (name, size, box, w) in enumerate(rows):
        np.testing.assert_array_equal(got[k], _want(name, size, filt, box, w), strict=True, err_msg=name)


@pytest.mark.parametrize("norm", [None, "float16", "bfloat16"])
@pytest.mark.parametrize("pix_fmt", ["rgb", "bgr", "rgb24", "bgr24"])
def test_formats_and_dtypes(decoder, oracle, pix_fmt, norm):
    kw = dict(normalize=True, norm_dtype=norm) if norm else {}
    want = turbo_ref.layout(_want(TILED, (70, 19), "bicubic"), pix_fmt, **kw)
    st, got = _decode(decoder, [tc.case(TILED)], Output(pix_fmt=pix_fmt, csc="turbo", **kw), want.shape,
                      resample=Resample("bicubic", 70, 19))
    assert st == [0]
    np.testing.assert_array_equal(got[0], want, strict=True)


@pytest.mark.parametrize("what", ["swscale", "jfif", "yuv", "ragged", "crops", "views", "flips",
                                  "orients", "lowres", "count", "out_w", "out_h"])
def test_refused_with_invalid_arg_and_nothing_written(decoder, oracle, what):
    """The raw entry point: nothing written, and the setting is consumed."""
    d, out, rs = tc.case("420_33x33"), TURBO, Resample("bilinear", 16, 16)
    nbytes = 33 * 33 * 3
    t = torch.full((nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    ptr = t.data_ptr()
    if what in ("swscale", "jfif"):
        out = Output(pix_fmt="rgb24", csc=what)
    elif what == "yuv":
        out = Output(pix_fmt="yuv")
    elif what == "views":
        decoder.set_views([ViewGroup(out, [(0, None)], ptr, nbytes)])
        ptr = nbytes = 0
    elif what == "count":
        rs = Resample("bilinear", 16, 16, ((None, (16, 16), (0, 0)),) * 2)
    elif what in ("out_w", "out_h"):
        rs = Resample("bilinear", *((0, 16) if what == "out_w" else (16, 65536)))
    else:
        getattr(decoder, "set_" + what)({"ragged": [0], "crops": [(0, 0, 16, 16)], "flips": [1],
                                         "orients": [5], "lowres": [1]}[what])
    decoder.set_resample(rs)
    rc, msg, _ = _raw(decoder, [d], out, ptr, nbytes)
    assert rc == INVALID_ARG and msg, (rc, msg)
    torch.cuda.synchronize()
    assert bool((t == GUARD).all()), "a refused submission wrote output"
    _plain_follows(decoder, d)


def _plain_follows(decoder, d):
    st, got = _decode(decoder, [d], TURBO, (33, 33, 3))
    assert st == [0] and decoder.get_param("resample_workgroups") == 0
    np.testing.assert_array_equal(got[0], turbo_ref.rgb_u8(d), strict=True)


def test_one_shot_after_a_resampled_submission(decoder, oracle):
    d = tc.case("420_33x33")
    st, got = _decode(decoder, [d], TURBO, (16, 16, 3), resample=Resample("bilinear", 16, 16))
    assert st == [0] and decoder.get_param("resample_workgroups") > 0
    np.testing.assert_array_equal(got[0], _want("420_33x33", (16, 16), "bilinear"), strict=True)
    _plain_follows(decoder, d)


def test_python_surface(oracle):
    """Mixed sizes into one [B, 224, 224, 3]; Resize(256) + CenterCrop(224)."""
    cfg = sio.cuda_config(device_index=0)
    names = ["bench", "420_33x33", TILED]
    boxes = [(101, 50, 333, 301), None, (1, 2, 100, 30)]
    buf = sio.load_image_batch([data_of(n) for n in names], width=None, height=None, csc="turbo",
                               device_config=cfg, resample=sio.pil_resize((224, 224), boxes=boxes))
    got = sio.to_torch(buf).cpu().numpy()
    assert got.shape == (3, 224, 224, 3)
    for k, n in enumerate(names):
        np.testing.assert_array_equal(got[k], _want(n, (224, 224), "bilinear", boxes[k]), err_msg=n)
    one = sio.load_image(data_of("bench"), csc="turbo", device_config=cfg,
                         resample=sio.pil_resize((224, 224), "bicubic", shorter=256))
    want = _want("bench", (341, 256), "bicubic", None, (58, 16, 224, 224))
    np.testing.assert_array_equal(sio.to_torch(one).cpu().numpy(), want, strict=True)
