"""CPU tests of the Pillow-exact draft (include/spdl_hipjpeg.h "Pillow-exact
draft"; no GPU): ``tests/draft_ref.py`` against Pillow's own ``Image.draft``
byte for byte, ``draft_level`` against the scale Pillow picks, the transforms
of hj_idct.h and the planner under sanitizers, and the Python refusals."""

import io
import os

import numpy as np
import pytest
from PIL import Image

import spdl_amd.io as sio
from spdl_amd import _lib
from tests import draft_ref as ref
from tests.test_lowres import CSRC, NATIVE, _sanitized


def _pillow(data: bytes, request):
    """(the draft frame's size, its RGB pixels) after ``im.draft("RGB", request)``"""
    im = Image.open(io.BytesIO(data))
    im.draft("RGB", request)
    return im.size, np.asarray(im.convert("RGB"))


@pytest.mark.parametrize("level", [1, 2, 3])
@pytest.mark.parametrize("name", ref.NAMES)
def test_reference_is_pillow(name, level):
    """A request of (W >> level, H >> level): Pillow decodes at the level
    ``draft_level`` names (a lower one where a side is too short), and the
    reference at that level is its frame byte for byte."""
    data = ref.case(name)
    info = _lib.get_image_info(data)
    rw, rh = max(info.width >> level, 1), max(info.height >> level, 1)
    lv = _lib.draft_level(info.width, info.height, rw, rh)
    size, px = _pillow(data, (rw, rh))
    assert size == _lib.draft_size(info.width, info.height, lv)
    np.testing.assert_array_equal(ref.rgb_u8(data, lv), px)


@pytest.mark.parametrize("request_,level", [
    ((51, 38), 0), ((50, 37), 1), ((51, 37), 0), ((50, 38), 0), ((25, 18), 2), ((26, 18), 1),
    ((25, 19), 1), ((12, 9), 3), ((13, 9), 2), ((12, 10), 2), ((1, 1), 3), ((200, 200), 0)])
def test_draft_level_is_pillows_choice(request_, level):
    """101x75: either side of the thresholds of the scales 2, 4 and 8"""
    assert _lib.draft_level(101, 75, *request_) == level
    data = ref.cases._enc(ref.pixels(9, 101, 75), quality=90)
    assert _pillow(data, request_)[0] == _lib.draft_size(101, 75, level)


def test_sweep_under_sanitizers(tmp_path):
    """tests/native/draft_sweep.cpp: the host build of the transforms against
    the rule, the planner against the size rule; it exits 1 on a failure"""
    lines = _sanitized(tmp_path, "draft_sweep", [os.path.join(NATIVE, "draft_sweep.cpp")] + [
        os.path.join(CSRC, f) for f in ("hj_layout.cpp", "hj_sws.cpp")])
    assert lines == ["0 failures"]


@pytest.mark.parametrize("kw,what", [
    (dict(draft=1), "needs csc='turbo'"),
    (dict(draft=1, csc="turbo", lowres=1), "lowres="),
    (dict(draft=4, csc="turbo"), "not in 0..3"),
    (dict(draft=[1, 1], csc="turbo"), "2 draft levels for 1 images"),
    (dict(draft="auto", csc="turbo"), "needs resample="),
    (dict(draft=(0, 5), csc="turbo"), "both at least 1"),
    (dict(draft="auto", csc="turbo", resample=sio.pil_resize((8, 8), boxes=[(0, 0, 4, 4)])),
     "the level comes first")])
def test_python_refusals_before_anything_is_read(kw, what):
    """(the source does not exist: a refusal that came after a read would be another error)"""
    with pytest.raises(ValueError, match=what):
        sio.load_image_batch(["/nonexistent.jpg"], width=None, height=None, **kw)
