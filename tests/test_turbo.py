"""CPU tests of the Pillow-exact decode (include/spdl_hipjpeg.h "Pillow-exact
decode", ``csc="turbo"``; no GPU): the numpy reference (tests/turbo_ref.py)
against Pillow itself on the whole case table; the declarations; the Python
surface's argument checks; the planner and the shared row functions as
stand-alone sweeps under ASan and UBSan (tests/native/turbo_layout_sweep.cpp,
tests/native/upsample_sweep.cpp).
"""

import io
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image, features

from spdl_amd import _lib
from spdl_amd._lib import Output
from spdl_amd.io import _image
from tests import turbo_cases as tc
from tests import turbo_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spdl_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")


def _pillow(data: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


# ---- 1. the reference is Pillow ------------------------------------------------------------------

def test_case_table():
    assert len(tc.NAMES) == len(set(tc.NAMES)) and 100 <= len(tc.NAMES) <= 125
    info = _lib.get_image_info(tc.case("luma_below_chroma"))
    assert [(info.h_samp[c], info.v_samp[c]) for c in range(3)] == [(1, 1), (2, 2), (2, 2)]
    for name, (h0, v0) in tc.LJ9.items():
        info = _lib.get_image_info(tc.case(f"{name}_9x7"))
        assert (info.h_samp[0], info.v_samp[0], info.multiscan) == (h0, v0, 1), name


@pytest.mark.parametrize("name", tc.NAMES)
def test_reference_equals_pillow(oracle, name):
    """Every case of the table, byte for byte.  The luma-below-chroma layout of
    the header's rule 2 is one of them: Pillow agrees, so the mode accepts it."""
    data = tc.case(name)
    got = ref.rgb_u8(data)
    info = oracle.parse(data)
    assert got.shape == (info.height, info.width, 3) and got.dtype == np.uint8
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not linked against libjpeg-turbo")
    np.testing.assert_array_equal(got, _pillow(data), strict=True)


def test_jfif_is_another_decode(oracle):
    """csc="jfif" replicates chroma: on a 4:2:0 file most pixels differ from
    the triangle rule's, so the new mode is no alias of it."""
    data = tc.case("420_33x33")
    jfif = oracle.decode_rgb(data, oracle.IDCT_ISLOW, "rgb24", "jfif")
    turbo = ref.rgb_u8(data)
    assert (jfif != turbo).any(axis=-1).mean() > 0.5
    # ... and on a 4:4:4 file the two differ by the green table alone, if at all
    data = tc.case("444_33x33")
    jfif = oracle.decode_rgb(data, oracle.IDCT_ISLOW, "rgb24", "jfif").astype(int)
    turbo = ref.rgb_u8(data).astype(int)
    assert np.array_equal(jfif[..., [0, 2]], turbo[..., [0, 2]])
    assert np.abs(jfif[..., 1] - turbo[..., 1]).max() <= 1


def test_reference_layouts():
    px = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3) * 9
    assert np.array_equal(ref.layout(px, "bgr24"), px[..., ::-1])
    assert np.array_equal(ref.layout(px, "rgb"), np.moveaxis(px, 2, 0))
    f16 = ref.layout(px, "bgr", normalize=True)
    assert f16.shape == (3, 2, 3) and f16.dtype == np.uint16
    # channel 0 of a BGR output is blue, normalised with mean[0] and std[0]
    want = np.float16((np.float32(px[0, 0, 2]) / np.float32(255) - np.float32(0.485)) /
                      np.float32(0.229))
    assert f16[0, 0, 0] == want.view(np.uint16)
    bf = ref.layout(px, "rgb24", normalize=True, norm_dtype="bfloat16")
    f32 = (bf.astype(np.uint32) << 16).view(np.float32)
    exact = (px.astype(np.float32) / 255 - np.float32(ref.O.IMAGENET_MEAN)) / np.float32(ref.O.IMAGENET_STD)
    assert np.abs(f32 - exact).max() <= np.abs(exact).max() * 2.0 ** -8


# ---- 2. the declarations -------------------------------------------------------------------------

def test_header_and_binding():
    with open(os.path.join(ROOT, "include", "spdl_hipjpeg.h")) as f:
        hdr = f.read()
    assert "#define SPDL_HJ_ABI_VERSION 7" in hdr
    assert "SPDL_HJ_CSC_SWSCALE = 0, SPDL_HJ_CSC_JFIF = 1, SPDL_HJ_CSC_TURBO = 2" in hdr
    at = hdr.index("---- Pillow-exact decode")
    sec = hdr[at:hdr.index("*/", at)]
    for text in ("whatever spdl_hj_output.idct says", "not\n *    consulted", "22554",
                 "(3 s[i] + s[i-1] + 8) >> 4", "(3 p[i] + p[i+1] + 2) >> 2", "cw <= 2",
                 "never neighbours", "(1x1, 2x2,\n *    2x2)", "SPDL_HJ_ERR_INVALID_ARG",
                 "SPDL_HJ_ERR_UNSUPPORTED", "spdl_hj_set_ragged", "turbo_workgroups",
                 "smooths block edges"):
        assert text in sec, text
    assert _lib.CSC["turbo"] == 2
    spec = Output(pix_fmt="bgr", csc="turbo").to_c()
    assert (spec.csc, spec.resize, spec.pix_fmt) == (2, 0, 1)
    assert _lib.lib().spdl_hj_abi_version() == 7


def test_ragged_layout_takes_the_mode():
    names = ["420_17x15", "422_9x7", "gray", "l41_15x9", "444_1x1"]
    infos = [_lib.get_image_info(tc.case(n)) for n in names]
    offs, sizes, st = _lib.ragged_layout(infos, Output(pix_fmt="rgb24", csc="turbo"), align=1)
    assert st == [0] * len(names)
    assert sizes == [(i.width, i.height) for i in infos]
    assert offs == list(np.cumsum([0] + [w * h * 3 for w, h in sizes]))
    with pytest.raises(ValueError, match="no ragged layout"):
        _lib.ragged_layout(infos, Output(pix_fmt="rgb24", csc="turbo"),
                           crops=[(0, 0, 8, 8)] + [None] * 4)
    with pytest.raises(ValueError, match="no ragged layout"):
        _lib.ragged_layout(infos, Output(pix_fmt="rgb24", csc="turbo"), orients=[1, 0, 0, 0, 0])
    with pytest.raises(ValueError, match="no ragged layout"):
        _lib.ragged_layout(infos, Output(pix_fmt="rgb24", csc="jfif"))
    # no output size for the mode with a resize: the spec is invalid
    with pytest.raises(ValueError, match="no ragged layout"):
        _lib.ragged_layout(infos, Output(pix_fmt="rgb24", csc="turbo", resize=True, fit_w=8, fit_h=8))


# ---- 3. the Python surface refuses before anything is submitted ----------------------------------

def _no_decoder(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a refused call reached the decoder")

    monkeypatch.setattr(_lib, "thread_decoder", boom)


BATCH_REFUSED = [
    dict(width=32, height=32),
    dict(width=32, height=None),
    dict(width=None, height=None, filter_desc="scale=16:16,format=pix_fmts=rgb24"),
    dict(width=None, height=None, filter_desc="crop=8:8:0:0,format=pix_fmts=rgb24"),
    dict(width=None, height=None, crops=[(0, 0, 8, 8)]),
    dict(width=None, height=None, flips=["h"]),
    dict(width=None, height=None, flips=[0]),
    dict(width=None, height=None, exif_orientation=True),
    dict(width=None, height=None, lowres=1),
    dict(width=None, height=None, lowres="auto"),
    dict(width=None, height=None, pix_fmt=None),
    dict(width=None, height=None, filter_desc=None),
]


@pytest.mark.parametrize("kw", BATCH_REFUSED, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
def test_load_image_batch_refuses(monkeypatch, kw):
    _no_decoder(monkeypatch)
    with pytest.raises(ValueError, match="csc='turbo'"):
        _image.load_image_batch([tc.case("420_17x15")], csc="turbo", **kw)


LIST_REFUSED = [
    dict(width=32), dict(height=32), dict(width=32, height=32, scale_mode="fit"),
    dict(filter_desc="scale=16:-1,format=pix_fmts=rgb24"), dict(crops=[None]), dict(flips=[None]),
    dict(exif_orientation=True), dict(lowres=[1]), dict(lowres=2),
]


@pytest.mark.parametrize("kw", LIST_REFUSED, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
def test_load_image_list_refuses(monkeypatch, kw):
    _no_decoder(monkeypatch)
    with pytest.raises(ValueError, match="csc='turbo'"):
        _image.load_image_list([tc.case("420_17x15")], csc="turbo", **kw)


def test_load_image_and_unknown_csc_refuse(monkeypatch):
    _no_decoder(monkeypatch)
    d = tc.case("420_17x15")
    for kw in (dict(flip="h"), dict(exif_orientation=True), dict(lowres=1), dict(pix_fmt=None),
               dict(filter_desc=None), dict(filter_desc="scale=8:8,format=pix_fmts=rgb24")):
        with pytest.raises(ValueError, match="csc='turbo'"):
            _image.load_image(d, csc="turbo", **kw)
    with pytest.raises(ValueError, match="no ragged planar YUV"):
        _image.load_image_list([d], csc="turbo", pix_fmt=None)
    for load in (lambda **k: _image.load_image(d, **k),
                 lambda **k: _image.load_image_batch([d], width=None, height=None, **k)):
        with pytest.raises(ValueError, match="csc must be one of"):
            load(csc="pillow")
    with pytest.raises(ValueError, match="csc='swscale' only"):
        _image.load_image_list([d], csc="pillow")
    # "jfif" stays with Output and the Decoder: these functions never took it
    with pytest.raises(ValueError, match="csc must be one of"):
        _image.load_image(d, csc="jfif")
    with pytest.raises(ValueError, match="csc must be one of"):
        _image.load_image(d, csc="jfif", filter_desc=None)


def test_chains_and_levels_that_ask_for_nothing_pass_the_checks():
    """A chain of the caller's with a format node decides the format whatever
    ``pix_fmt`` says, and all-zero levels are no levels."""
    check = _image._check_csc
    desc = "format=pix_fmts=bgr24"
    check("turbo", pix_fmt=_image._csc_pix_fmt(desc, None))
    out = _image._with_csc(_image.parse_image_filter(desc, default_pix_fmt=None), "turbo")
    assert (out.csc, out.pix_fmt) == ("turbo", "bgr24")
    with pytest.raises(ValueError, match="csc='turbo'"):  # (no format node: the planes)
        _image._with_csc(_image.parse_image_filter("scale=8:8", default_pix_fmt=None), "turbo")
    for lowres in (None, 0, [0], [0, 0]):
        check("turbo", lowres=lowres)
    for lowres in (1, [0, 2], "auto"):
        with pytest.raises(ValueError, match="lowres="):
            check("turbo", lowres=lowres)


# ---- 4. the native units under sanitizers ---------------------------------------------------------

def _sanitized(tmp_path, name, sources):
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
    exe = str(tmp_path / name)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-DHJ_HD=", *san, *sources, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr
    assert not r.stderr, r.stderr
    return r.stdout.splitlines()[-1]


def test_row_functions_sweep_under_sanitizers(tmp_path):
    """hj_upsample.h's runs against a per-pixel restatement, cw 1..20 x ch 1..6,
    every ratio, planes allocated to the byte, padding columns varied."""
    last = _sanitized(tmp_path, "upsample_sweep", [os.path.join(NATIVE, "upsample_sweep.cpp")])
    assert last.endswith(" 0 failed expectations") and int(last.split()[0]) >= 1000000, last


def test_planner_sweep_under_sanitizers(tmp_path):
    last = _sanitized(tmp_path, "turbo_layout_sweep",
                      [os.path.join(NATIVE, "turbo_layout_sweep.cpp"),
                       os.path.join(CSRC, "hj_layout.cpp"), os.path.join(CSRC, "hj_sws.cpp")])
    assert last.endswith(" 0 failed expectations") and int(last.split()[0]) >= 500, last
