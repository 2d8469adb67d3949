"""CPU tests of the Pillow-exact resize (include/spdl_hipjpeg.h): the numpy
reference against Pillow, the library's axis tables against the reference,
``pil_resize``, the Python refusals, and the tiler sweep under ASan and UBSan."""

import io
import os

import numpy as np
import pytest
from PIL import Image, features

from spdl_amd import _lib
from spdl_amd.io import _image, pil_resize
from tests import resample_ref as ref
from tests import turbo_cases as tc
from tests.test_turbo import _sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spdl_amd", "csrc")
BENCH = os.path.join(ROOT, "tests", "golden", "jpeg", "bench_1000.jpg")
PIL_FILTER = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}
TILED = f"420_{tc.TILE_W + 1}x{tc.TILE_H + 1}"
# (case, target, box); the bench file at 15 x 12: a lanczos axis of exactly 256 taps (640 -> 15)
SHAPES = [("420_33x33", s, None) for s in [(16, 16), (70, 50), (33, 12), (7, 33), (1, 1), (33, 33)]]
SHAPES += [(TILED, (300, 80), None), (TILED, (40, 9), None), ("bench", (224, 224), None),
           ("bench", (15, 12), None), ("420_33x33", (12, 9), (3, 5, 21, 17)),
           ("422_33x33", (5, 4), (0, 0, 1, 1))]


def data_of(name: str) -> bytes:
    if name == "bench":
        with open(BENCH, "rb") as f:
            return f.read()
    return tc.case(name)


@pytest.mark.skipif(not features.check_feature("libjpeg_turbo"), reason="Pillow without libjpeg-turbo")
@pytest.mark.parametrize("filt", list(PIL_FILTER))
@pytest.mark.parametrize("name,size,box", SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_reference_equals_pillow(oracle, name, size, box, filt):
    data = data_of(name)
    im = Image.open(io.BytesIO(data)).convert("RGB")
    if box is not None:
        im = im.crop((box[0], box[1], box[0] + box[2], box[1] + box[3]))
    want = np.asarray(im.resize(size, PIL_FILTER[filt]))
    np.testing.assert_array_equal(ref.decode_resize(data, size, filt, box), want, strict=True)


@pytest.mark.parametrize("filt", list(PIL_FILTER))
def test_library_tables_equal_the_reference(filt):
    axes = {(33, 16), (33, 70), (33, 12), (33, 7), (33, 1), (33, 33), (129, 300), (129, 40), (33, 80),
            (33, 9), (640, 224), (480, 224), (640, 15), (480, 12), (21, 12), (17, 9), (1, 5), (1, 1)}
    for in_size, out_size in sorted(axes):
        got, want = _lib.resample_axis(in_size, out_size, filt), ref.axis(in_size, out_size, filt)
        for g, w, what in zip(got, want, ("xmin", "n", "K")):
            np.testing.assert_array_equal(g, w, strict=True, err_msg=f"{in_size}->{out_size} {what}")


def test_tap_limit_and_binding():
    assert _lib.resample_axis(640, 15, "lanczos")[2].shape == (15, 256)
    with pytest.raises(RuntimeError, match=": 7"):  # SPDL_HJ_ERR_BAD_GEOMETRY
        _lib.resample_axis(640, 14, "lanczos")
    with open(os.path.join(ROOT, "include", "spdl_hipjpeg.h")) as f:
        assert "#define SPDL_HJ_RESAMPLE_MAX_TAPS 256" in f.read()
    assert {"spdl_hj_set_resample", "spdl_hj_debug_resample_axis"} <= set(_lib.EXPORTED)


def test_pil_resize_geometry():
    assert pil_resize((224, 224)).geometry(500, 375) == (None, (224, 224), (0, 0))
    r = pil_resize((224, 224), "bicubic", boxes=[(3, 5, 21, 17), None])
    assert r.geometry(500, 375, r.boxes[0]) == ((3, 5, 21, 17), (224, 224), (0, 0))
    # Resize(256) + CenterCrop(224): long = int(256 * long / short), the corner rounds half to even
    e = pil_resize((224, 224), shorter=256)
    assert e.geometry(500, 375) == (None, (341, 256), (58, 16))
    assert e.geometry(375, 500) == (None, (256, 341), (16, 58))
    assert pil_resize((7, 5), shorter=8).geometry(99, 50, (1, 1, 20, 31)) == ((1, 1, 20, 31), (8, 12), (0, 4))
    for bad in (dict(size=(0, 5)), dict(size=(5,)), dict(size=(5, 5), filter="box"),
                dict(size=(5, 5), shorter=0), dict(size=(5, 5), boxes=[(1, 2, 3)])):
        with pytest.raises(ValueError):
            pil_resize(**bad)


REFUSED = [dict(csc="swscale"), dict(csc="turbo", width=32, height=32),
           dict(csc="turbo", filter_desc="scale=16:16,format=pix_fmts=rgb24"),
           dict(csc="turbo", crops=[(0, 0, 8, 8)]), dict(csc="turbo", flips=["h"]),
           dict(csc="turbo", exif_orientation=True), dict(csc="turbo", lowres=1),
           dict(csc="turbo", pix_fmt=None), dict(csc="turbo", filter_desc=None)]


@pytest.mark.parametrize("kw", REFUSED, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
def test_surface_refuses_before_reading(monkeypatch, kw):
    def boom(*a, **k):
        raise AssertionError("a refused call reached the decoder")

    monkeypatch.setattr(_lib, "thread_decoder", boom)
    monkeypatch.setattr(_image, "_read", boom)
    rs = pil_resize((8, 8))
    batch = {"width": None, "height": None, **kw}
    with pytest.raises(ValueError):
        _image.load_image_batch(["a.jpg"], resample=rs, **batch)
    if not {"width", "crops", "flips"} & set(kw) and kw != {"csc": "turbo"}:
        with pytest.raises(ValueError):
            _image.load_image("a.jpg", resample=rs, **kw)
    with pytest.raises(ValueError, match="boxes for"):
        _image.load_image_batch(["a.jpg"], width=None, height=None, csc="turbo",
                                resample=pil_resize((8, 8), boxes=[None, None]))
    with pytest.raises(TypeError):
        _image.load_image_list(["a.jpg"], resample=rs)


def test_tiler_sweep_under_sanitizers(tmp_path):
    last = _sanitized(tmp_path, "resample_sweep",
                      [os.path.join(ROOT, "tests", "native", "resample_sweep.cpp"),
                       os.path.join(CSRC, "hj_resample.cpp")])
    assert last.endswith(" 0 failed expectations") and int(last.split()[0]) >= 1000000, last
