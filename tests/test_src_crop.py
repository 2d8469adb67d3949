"""CPU tests of the source crop (include/spdl_hipjpeg.h "source crop"; no GPU):
``spdl_hj_crop_rect`` against the rules restated in ``tests/src_crop_ref.py``,
the filter-string parser, the region IDCT's index arithmetic under sanitizers
(tests/native/idct_region_sweep.cpp), and two checks of the reference itself.
"""

import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from spdl_amd import _lib
from spdl_amd._lib import Output
from spdl_amd.io._preprocessing import parse_image_filter
from tests import cases
from tests import src_crop_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_GEOMETRY = 7
C = ref.CENTER

# the (hs, vs) pairs of the header's table; as the SOF factors of the luma
# component over 1x1 chroma they give a three-component frame of that ratio
RATIOS = [(1, 1), (2, 1), (2, 2), (1, 2), (4, 1), (4, 4)]


def _info(W, H, hs, vs, ncomp=3):
    i = _lib.ImageInfo()
    i.width, i.height, i.ncomp = W, H, ncomp
    for c in range(ncomp):
        i.h_samp[c] = i.v_samp[c] = 1
    if ncomp == 3:
        i.h_samp[0], i.v_samp[0] = hs, vs
    i.color = {1: 0, 3: 1, 4: 3}[ncomp]
    return i


def _axis_values(full):
    pos = sorted({-100, -5, -1, 0, 1, 2, 3, 4, 5, 7, full // 2, full - 5, full - 4, full - 3,
                  full - 2, full - 1, full, full + 1, full + 9})
    size = sorted({-3, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, full // 2, full - 4, full - 3, full - 2,
                   full - 1, full, full + 1, full + 4})
    return pos + [C], size


def _one(info, hs, vs, rect):
    want = ref.resolve(info.width, info.height, hs, vs, rect)
    rc, got = _lib.crop_rect(info, rect)
    assert (rc, got) == ((0, want) if want is not None else (BAD_GEOMETRY, None)), \
        (info.width, info.height, hs, vs, rect)


@pytest.mark.parametrize("hs,vs", RATIOS)
def test_crop_rect_against_the_rules(hs, vs):
    """Every ratio pair x frame sizes 1..40 on each axis (the other axis at a
    size coprime to the ratios) x rectangles negative, overhanging, off-grid,
    centred, empty and too large."""
    n = 0
    for full in range(1, 41):
        pos, size = _axis_values(full)
        ix, iy = _info(full, 37, hs, vs), _info(37, full, hs, vs)
        for p in pos:
            for s in size:
                _one(ix, hs, vs, (p, 3, s, 20))
                _one(iy, hs, vs, (3, p, 20, s))
                n += 2
    # both axes off at once, and the "no crop" rectangle
    for W, H in ((1, 1), (7, 5), (16, 16), (33, 40), (40, 33)):
        i = _info(W, H, hs, vs)
        px, sx = _axis_values(W)
        py, sy = _axis_values(H)
        for k in range(max(len(px), len(py)) * 3):
            _one(i, hs, vs, (px[k % len(px)], py[(k * 7) % len(py)], sx[(k * 3) % len(sx)],
                             sy[(k * 5) % len(sy)]))
        assert _lib.crop_rect(i, (0, 0, 0, 0)) == (0, (0, 0, W, H))
        assert _lib.crop_rect(i, None) == (0, (0, 0, W, H))
    assert n > 40 * 300


def test_crop_rect_gray_and_four_components_have_ratio_one():
    for ncomp in (1, 4):
        i = _info(33, 21, 1, 1, ncomp)
        if ncomp == 1:
            i.h_samp[0] = i.v_samp[0] = 2  # a gray frame's factors mean nothing
        assert _lib.crop_rect(i, (5, 3, 7, 9)) == (0, (5, 3, 7, 9))
        assert _lib.crop_rect(i, (30, 20, 7, 9)) == (0, (26, 12, 7, 9))
        assert _lib.crop_rect(i, (None, None, 7, 9)) == (0, (13, 6, 7, 9))
        assert _lib.crop_rect(i, (0, 0, 34, 9)) == (BAD_GEOMETRY, None)


def test_crop_rect_spot_values():
    i = _info(333, 227, 2, 2)
    assert _lib.crop_rect(i, (301, 195, 32, 32)) == (0, (300, 194, 32, 32))
    assert _lib.crop_rect(i, (301, 195, 33, 33)) == (0, (300, 194, 32, 32))  # 301 + 32 == 333
    assert _lib.crop_rect(i, (-4, 500, 100, 100)) == (0, (0, 126, 100, 100))  # 227 - 100 = 127 -> 126
    assert _lib.crop_rect(i, (None, 0, 100, 100)) == (0, (116, 0, 100, 100))
    assert _lib.crop_rect(i, (None, 0, 101, 100)) == (BAD_GEOMETRY, None)  # centred, off-grid size
    assert _lib.crop_rect(i, (0, 0, 1, 100)) == (BAD_GEOMETRY, None)  # rounds to 0
    assert _lib.crop_rect(i, (0, 0, 334, 100)) == (BAD_GEOMETRY, None)
    assert _lib.crop_rect(i, (0, 0, 333, 227)) == (0, (0, 0, 332, 226))
    bad = _info(10, 10, 1, 1)
    bad.ncomp = 2
    assert _lib.crop_rect(bad, (0, 0, 4, 4))[0] == 8  # INVALID_ARG


# ---- the parser ----------------------------------------------------------------

@pytest.mark.parametrize("desc,crop", [
    ("crop=100:80:33:17,scale=64:64", (33, 17, 100, 80)),
    ("crop=w=100:h=80:x=33:y=17,scale=w=64:h=64", (33, 17, 100, 80)),
    ("crop=100:80:x=33:y=17,scale=64:64", (33, 17, 100, 80)),
    ("crop=w=100:h=80:x=33,scale=64:64", (33, None, 100, 80)),
    ("crop=w=100:h=80:y=17,scale=64:64", (None, 17, 100, 80)),
    ("crop=100:80:-5:400,scale=64:64", (-5, 400, 100, 80)),
])
def test_parser_takes_a_source_crop(desc, crop):
    out = parse_image_filter(desc)
    assert out.src_crop == crop
    assert (out.resize, out.fit_w, out.fit_h, out.crop_w, out.crop_h) == (True, 64, 64, 0, 0)
    assert parse_image_filter(desc + ",format=pix_fmts=rgb24").src_crop == crop


def test_parser_source_crop_alone_and_with_the_built_chain():
    out = parse_image_filter("crop=100:80:33:17")
    assert out.src_crop == (33, 17, 100, 80) and not out.resize
    out = parse_image_filter("crop=100:80:33:17,scale=w=64:h=64:flags=bilinear:"
                             "force_original_aspect_ratio=decrease,pad=w=64:h=64:x=-1:y=-1:color=black,"
                             "crop=w=32:h=32")
    assert out.src_crop == (33, 17, 100, 80)
    assert (out.filter, out.aspect, out.pad_w, out.pad_h, out.crop_w, out.crop_h) == \
        ("bilinear", "decrease", 64, 64, 32, 32)


@pytest.mark.parametrize("desc", [
    "scale=64:64,crop=32:32:1:1",                 # after scale: as before
    "scale=64:64,pad=w=80:h=80:x=-1:y=-1:color=black,crop=32:32:x=1",
    "crop=iw-16:80:0:0,scale=64:64",              # expressions
    "crop=100:80:x=(iw-100)/2:y=0,scale=64:64",
    "crop=100:80:3.5:0,scale=64:64",
    "crop=100:80:1:1:exact=1,scale=64:64",
    "crop=100:80:1:1:keep_aspect=1,scale=64:64",
    "crop=100:80:1:1:1,scale=64:64",              # positional keep_aspect
    "crop=x=1:y=1,scale=64:64",                   # no size
    "crop=100:80:1:1,crop=50:40:2:2,scale=64:64",  # two source crops
])
def test_parser_refusals(desc):
    with pytest.raises(ValueError):
        parse_image_filter(desc)


def test_parser_crop_after_scale_keeps_its_message():
    with pytest.raises(ValueError, match="only centred crop is supported"):
        parse_image_filter("scale=64:64,crop=32:32:1:1")


@pytest.mark.parametrize("desc,want", [
    ("crop=w=32:h=24", Output(pix_fmt="rgb24", resize=True, crop_w=32, crop_h=24)),
    ("crop=32:24", Output(pix_fmt="rgb24", resize=True, crop_w=32, crop_h=24)),
    ("crop=32:24,scale=64:64",
     Output(pix_fmt="rgb24", resize=True, crop_w=32, crop_h=24, fit_w=64, fit_h=64, aspect=None,
            filter="bicubic")),
    ("scale=w=64:h=64:flags=bicubic:force_original_aspect_ratio=increase,crop=w=64:h=64",
     Output(pix_fmt="rgb24", resize=True, fit_w=64, fit_h=64, aspect="increase", crop_w=64,
            crop_h=64, filter="bicubic")),
])
def test_plain_crop_is_unchanged(desc, want):
    """A crop without x and y means what it meant: the Output of today."""
    out = parse_image_filter(desc)
    assert out == want and out.src_crop is None


def test_output_src_crop_is_no_field_of_the_c_spec():
    a, b = Output(resize=True, fit_w=8, fit_h=8), Output(resize=True, fit_w=8, fit_h=8,
                                                         src_crop=(1, 2, 3, 4))
    assert bytes(a.to_c()) == bytes(b.to_c()) and a != b
    assert ctypes.sizeof(_lib.Rect) == 16 and _lib.CROP_CENTER == -(1 << 31)


# ---- the region IDCT's index arithmetic ----------------------------------------

def test_idct_region_index_sweep_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    # (runtimes linked statically: the program then runs whatever the environment preloads)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-static-libubsan"]
    probe_src = tmp_path / "probe.cpp"
    probe_src.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, *san, str(probe_src), "-o", str(tmp_path / "probe")],
                      capture_output=True).returncode:
        pytest.skip("the compiler has no sanitizer runtime")
    exe = str(tmp_path / "idct_region_sweep")
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-DHJ_HD=", *san,
                    os.path.join(ROOT, "tests", "native", "idct_region_sweep.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("rects ") and not r.stderr, r.stdout + r.stderr
    rects, positions = (int(r.stdout.split()[i]) for i in (1, 3))
    # every rectangle of the 30 small grids alone: sum over grids of
    # C(mcux + 1, 2) C(mcuy + 1, 2) = 56 * 35 per bpm
    assert rects >= 7 * 56 * 35 and positions > 10 * rects


# ---- the reference itself ------------------------------------------------------

def test_reference_whole_frame_rectangle_is_the_whole_frame_decode(oracle):
    for name in ("q90_420", "gray", "cmyk_adobe"):
        d = cases.case(name)
        info = oracle.parse(d)
        rs = oracle.Resize(fit_w=64, fit_h=64, aspect="decrease", pad_w=64, pad_h=64)
        whole = ref.resolve_data(d, (0, 0, 0, 0))
        assert whole == (0, 0, info.width, info.height)
        np.testing.assert_array_equal(ref.rgb(d, whole, rs), oracle.decode_resize(d, rs),
                                      strict=True)


def test_reference_region_is_not_always_a_slice_of_the_frame(oracle):
    # odd_227x333 (4:2:0, odd height): the whole frame takes the general
    # scaler, the even-sized region swscale's unscaled converter
    d = cases.case("odd_227x333")
    r = ref.resolve_data(d, (301, 195, 32, 32))
    assert r == (300, 194, 32, 32)
    full = oracle.decode_rgb(d, oracle.IDCT_SIMPLE, "rgb24")
    assert not np.array_equal(ref.rgb(d, r, None), full[194:226, 300:332])
    # q90_420 (640x480, even): both take the unscaled converter, whose chroma
    # is per pixel pair -- the slice
    d = cases.case("q90_420")
    r = ref.resolve_data(d, (38, 22, 112, 112))
    assert r == (38, 22, 112, 112)
    full = oracle.decode_rgb(d, oracle.IDCT_SIMPLE, "rgb24")
    np.testing.assert_array_equal(ref.rgb(d, r, None), full[22:134, 38:150], strict=True)
