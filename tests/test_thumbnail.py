"""Pillow-exact thumbnail on the CPU: the numpy reference against Pillow, the
library's float-box tables and reducing_gap resolver against the reference, the
Python refusals, and the sanitised native sweep of the resolver and tiler."""

import io
import os

import numpy as np
import pytest
from PIL import Image, features

from spdl_amd import _lib
from spdl_amd.io import _image, pil_resize, pil_thumbnail
from tests import draft_ref
from tests import thumbnail_ref as ref
from tests.test_resample import CSRC, PIL_FILTER, ROOT
from tests.test_turbo import _sanitized

PIXELS = np.random.default_rng(5).integers(0, 256, (61, 83, 3), dtype=np.uint8)
# (factor, box): off the origin, with partial right / bottom / corner cells
REDUCE = [((2, 2), (3, 1, 80, 60)), ((3, 3), (1, 2, 83, 61)), ((5, 2), (0, 0, 83, 61)),
          ((1, 3), (7, 5, 20, 58)), ((3, 1), (2, 0, 81, 9)), ((16, 16), (1, 1, 83, 61)),
          ((2, 2), None), ((4, 4), (0, 0, 80, 60))]
# float boxes: inside, touching the frame's edges, identity size with a fractional box
BOXES = [((20, 14), (3.25, 2.5, 70.75, 50.125)), ((30, 25), (0, 0, 83, 61)),
         ((40, 31), (0.0, 0.5, 82.5, 61)), ((83, 61), (0.5, 0.25, 83, 61)), ((9, 40), (40.1, 0, 49.6, 61))]
GAPS = [((10, 8), None, 1.0), ((10, 8), None, 2.0), ((10, 8), None, 3.0),
        ((7, 9), (2.5, 1.25, 80.0, 59.5), 2.0), ((5, 30), (0, 0, 83, 61), 1.0)]
THUMBS = [("gray_83x61", (20, 20), 2.0), ("420_83x61", (40, 40), 2.0), ("420_83x61", (10, 10), 2.0),
          ("444_83x61", (30, 9), 1.0), ("progressive", (21, 40), 3.0), ("420_83x61", (42, 31), 2.0),
          ("444_9x7", (20, 20), 2.0), ("progressive", (16, 16), None)]


@pytest.mark.parametrize("factor,box", REDUCE, ids=str)
def test_reduce_reference_equals_pillow(factor, box):
    want = np.asarray(Image.fromarray(PIXELS).reduce(factor, box))
    np.testing.assert_array_equal(ref.reduce(PIXELS, factor, box), want, strict=True)


@pytest.mark.parametrize("filt", list(PIL_FILTER))
@pytest.mark.parametrize("size,box,gap", [(s, b, None) for s, b in BOXES] + GAPS, ids=str)
def test_resize_reference_equals_pillow(size, box, gap, filt):
    want = np.asarray(Image.fromarray(PIXELS).resize(size, PIL_FILTER[filt], box=box, reducing_gap=gap))
    np.testing.assert_array_equal(ref.resize(PIXELS, size, filt, box, gap), want, strict=True)


@pytest.mark.skipif(not features.check_feature("libjpeg_turbo"), reason="Pillow without libjpeg-turbo")
@pytest.mark.parametrize("name,size,gap", THUMBS, ids=str)
def test_thumbnail_reference_and_plan_equal_pillow(oracle, name, size, gap):
    data = draft_ref.case(name)
    im = Image.open(io.BytesIO(data))
    w, h = im.size
    im.thumbnail(size, Image.BICUBIC, reducing_gap=gap)
    np.testing.assert_array_equal(ref.thumbnail(data, w, h, size, "bicubic", gap),
                                  np.asarray(im.convert("RGB")), strict=True)
    level, final, box = pil_thumbnail(size, "bicubic", gap).plan(w, h)
    want = ref.thumbnail_plan(w, h, size, gap)
    assert (level, final) == want[:2] and final == im.size
    assert box == (None if want[2] is None else tuple(float(v) for v in want[2]))


@pytest.mark.parametrize("filt", list(PIL_FILTER))
def test_library_tables_and_resolver_equal_the_reference(filt):
    for in_size, in0, in1, out in [(83, 3.25, 70.75, 20), (83, 0.0, 82.5, 40), (61, 0.25, 61.0, 61),
                                   (61, 0.0, 61.0, 25), (40, 0.125, 39.5, 7), (9, 2.5, 3.0, 12)]:
        got, want = _lib.resample_axis(in_size, out, filt, (in0, in1)), ref.axis_box(in_size, in0, in1, out, filt)
        for g, w, what in zip(got, want, ("xmin", "n", "K")):
            np.testing.assert_array_equal(g, w, strict=True, err_msg=f"{in_size} {in0} {in1} {out} {what}")
    for (w, h), size, box, gap in [((640, 480), (30, 20), (1.5, 2.5, 600.25, 470.0), 2.0),
                                   ((83, 61), (10, 8), None, 1.0), ((83, 61), (10, 8), None, 3.0),
                                   ((200, 160), (12, 10), (0, 0, 200, 160), 1.0), ((83, 61), (40, 30), None, 2.0)]:
        rc, p = _lib.reduce_plan(w, h, size, filt, gap, box)
        (fx, fy), q, b = ref.plan(w, h, size, filt, box, gap)
        assert rc == 0 and (p.fx, p.fy) == (fx, fy) and tuple(p.q) == q and tuple(p.box) == tuple(b)
        qw, qh = q[2] - q[0], q[3] - q[1]
        assert (p.cw, p.ch) == (-(-qw // fx), -(-qh // fy))
        ex, ey = qw % fx or fx, qh % fy or fy
        assert list(p.div) == [fx * fy, ex * fy, fx * ey, ex * ey]
        assert list(p.mult) == [(1 << 24) // d for d in p.div]


def test_limits_and_binding():
    assert _lib.reduce_plan(640, 480, (8, 8), "bicubic", 0.5)[0] == 8        # INVALID_ARG: the gap
    assert _lib.reduce_plan(640, 480, (8, 8), "bicubic", 2.0, (0, 0, 641, 480))[0] == 8  # ... the box
    assert _lib.reduce_plan(640, 480, (10, 10), "bicubic", 1.0)[0] == 7      # BAD_GEOMETRY: 64 x 48 cells
    assert _lib.reduce_plan(640, 480, (40, 30), "bicubic", 1.0)[0] == 0      # 16 x 16: the cap itself
    assert _lib.reduce_plan(2, 300, (2, 100), "bicubic", None)[0] == 7       # H > 100 W, shrinking
    with open(os.path.join(ROOT, "include", "spdl_hipjpeg.h")) as f:
        assert "#define SPDL_HJ_REDUCE_MAX_CELL 256" in f.read()
    assert {"spdl_hj_set_resample_box", "spdl_hj_debug_resample_axis_box",
            "spdl_hj_debug_reduce_plan"} <= set(_lib.EXPORTED)


@pytest.mark.parametrize("make", [
    lambda: pil_resize((8, 8), reducing_gap=0.5),
    lambda: pil_resize((8, 8), resize_boxes=[(0, 0, 4, 4)], boxes=[(0, 0, 4, 4)]),
    lambda: pil_resize((8, 8), reducing_gap=2.0, shorter=9),
    lambda: pil_resize((8, 8), resize_boxes=[(3, 0, 3, 4)]),
    lambda: pil_thumbnail((0, 8)),
    lambda: pil_thumbnail((8, 8), "nearest"),
    lambda: pil_thumbnail((8, 8), reducing_gap=0.5),
    lambda: _image.load_image("a.jpg", csc="turbo", pix_fmt="rgb24", draft=1, resample=pil_thumbnail((8, 8))),
    lambda: _image.load_image_batch(["a.jpg"], width=None, height=None, csc="turbo",
                                    resample=pil_resize((8, 8), resize_boxes=[None, None])),
    lambda: _image._thumbnail_of(pil_thumbnail((8, 8)), [_lib.ImageInfo(width=640, height=480),
                                                          _lib.ImageInfo(width=480, height=640)]),
])
def test_python_refusals_before_reading(monkeypatch, make):
    monkeypatch.setattr(_image, "_read", lambda s: pytest.fail("read a source"))
    with pytest.raises(ValueError):
        make()


def test_resolver_and_tiler_sweep_under_sanitizers(tmp_path):
    last = _sanitized(tmp_path, "thumb_sweep", [os.path.join(ROOT, "tests", "native", "thumb_sweep.cpp"),
                                                os.path.join(CSRC, "hj_resample.cpp")])
    assert last.endswith(" 0 failed expectations") and int(last.split()[0]) >= 100000, last
