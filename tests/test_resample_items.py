"""CPU tests of the resample items (include/spdl_hipjpeg.h "resample items"):
the GPU-free layout against Pillow's sizes, what the request refuses, and the
planner's item path under sanitizers."""

import io
import os

import pytest
from PIL import Image

from spdl_amd import _lib
from spdl_amd.io import _image, pil_resize, pil_thumbnail
from tests import cases
from tests.test_resample import CSRC, ROOT
from tests.test_turbo import _sanitized

FILES = ["odd_227x333", "odd_444_101x67", "q90_420", "gray_odd", "tiny_1x1", "tiny_8x8"]
INFOS = [_lib.get_image_info(cases.case(n)) for n in FILES]
BAD_GEOMETRY = 7


def _layout(resample, align=256):
    levels, reqs, gap = _image._item_requests(resample, INFOS, list(range(len(FILES))), None, None)
    return _lib.resample_layout(INFOS, reqs, align, filter=resample.filter, reducing_gap=gap, draft=levels)


@pytest.mark.parametrize("size", [(128, 128), (64, 48), (1, 1)])
def test_thumbnail_sizes_equal_pillow(size):
    offsets, sizes, statuses, _ = _layout(pil_thumbnail(size))
    for name, got in zip(FILES, sizes):
        im = Image.open(io.BytesIO(cases.case(name)))
        im.thumbnail(size)
        assert got == im.size, name
    # (into 1 x 1 the two large frames reduce by 21 x 14 and 40 x 30: above SPDL_HJ_REDUCE_MAX_CELL)
    assert statuses == ([BAD_GEOMETRY, 0, BAD_GEOMETRY, 0, 0, 0] if size == (1, 1) else [0] * len(FILES))
    assert all(o % 256 == 0 for o in offsets[:-1])
    ends = [o + w * h * 3 for o, (w, h) in zip(offsets, sizes)]
    assert all(e <= o for e, o in zip(ends, offsets[1:])) and offsets[-1] == ends[-1]


def test_shorter_sizes_equal_the_existing_geometry():
    _, sizes, statuses, _ = _layout(pil_resize(shorter=16, filter="bicubic"), align=64)
    want = [pil_resize((1, 1), shorter=16).geometry(i.width, i.height)[1] for i in INFOS]
    assert sizes == want and statuses == [0] * len(FILES)


# (image, box, clamp, (rw, rh), window, flip) against q90_420 (640 x 480) alone
@pytest.mark.parametrize("bad", [(1, None, False, (80, 60), None, 0), (0, (0.5, 0, 99, 99), True, (80, 60), None, 0),
                                 (0, None, False, (80, 60), None, 4), (0, (0, 0, 641, 99), False, (80, 60), None, 0)],
                         ids=["image", "fractional-clamped-box", "flip", "box-outside"])
def test_the_request_is_refused_whole(bad):
    with pytest.raises(ValueError):
        _lib.resample_layout(INFOS[2:3], [bad])


def test_an_item_past_the_buffer_is_refused():
    items = _lib.ResampleItems("bicubic", [(0, None, False, (80, 60), (0, 0), (80, 60), 0, 64)])
    assert _lib.resample_items_check(INFOS[2:3], items, 1, 64 + 14400) == [0]
    with pytest.raises(ValueError):
        _lib.resample_items_check(INFOS[2:3], items, 1, 64 + 14399)


def test_a_lanczos_item_above_42_to_1_is_refused_alone():
    reqs = [(0, None, False, (40, 30), None, 0), (0, None, False, (14, 12), None, 0),
            (0, (0, 0, 64, 48), True, (9, 7), None, "h")]
    assert _lib.resample_layout(INFOS[2:3], reqs, filter="lanczos")[2] == [0, BAD_GEOMETRY, 0]
    assert _lib.resample_layout(INFOS[2:3], reqs, filter="lanczos", reducing_gap=3.0)[2] == [0, 0, 0]


GROUP = dict(resample=pil_resize((8, 8)), boxes=[[None]])
REFUSED = [
    lambda: _image.load_image_list(["a.jpg"], csc="swscale", resample=pil_thumbnail((8, 8))),
    lambda: _image.load_image_list(["a.jpg"], csc="turbo", resample=pil_thumbnail((8, 8)), crops=[(0, 0, 8, 8)]),
    lambda: _image.load_image_list(["a.jpg"], csc="turbo", resample=pil_thumbnail((8, 8)), lowres=1),
    lambda: _image.load_image_list(["a.jpg"], csc="turbo", resample=pil_thumbnail((8, 8)), draft=1),
    lambda: _image.load_image_batch(["a.jpg"], width=None, height=None, csc="turbo", resample=pil_resize(shorter=8)),
    lambda: _image.load_image_views(["a.jpg"], [GROUP, {**GROUP, "normalize": True}], csc="turbo", device_config=0),
    lambda: _image.load_image_views(["a.jpg"], [{**GROUP, "crops": [[None]]}], csc="turbo", device_config=0),
    lambda: _lib.Decoder._submit(None, 1, _lib.Output(csc="turbo"), 1, 1, None, [], None, True, True, None, None,
                                 resample_items=_lib.ResampleItems("bicubic", [])),
    lambda: _lib.Decoder._submit(None, 1, _lib.Output(csc="turbo"), 1, 1, None, None, None, True, True, None, None,
                                 lowres=[1], resample_items=_lib.ResampleItems("bicubic", [])),
]


@pytest.mark.parametrize("make", REFUSED)
def test_python_refusals_before_reading(monkeypatch, make):
    monkeypatch.setattr(_image, "_read", lambda s: pytest.fail("read a source"))
    with pytest.raises(ValueError):
        make()


def test_item_planner_sweep_under_sanitizers(tmp_path):
    last = _sanitized(tmp_path, "items_sweep", [os.path.join(ROOT, "tests", "native", "items_sweep.cpp")] +
                      [os.path.join(CSRC, f) for f in ("hj_layout.cpp", "hj_sws.cpp", "hj_resample.cpp")])
    assert last.endswith(" 0 failed expectations") and int(last.split()[0]) >= 100000, last
