"""CPU tests of ragged batches (include/spdl_hipjpeg.h "ragged batches"; no
GPU): the planner's ragged path as a self-checking stand-alone sweep under
ASan and UBSan (tests/native/ragged_sweep.cpp), ``_lib.ragged_layout`` against
``output_size`` on the suite's files, and ``load_image_list``'s argument
checks.  (That a plain request still plans byte for byte what it did is
tests/test_layout.py's golden.)
"""

import os
import shutil
import subprocess

import pytest

from spdl_amd import _lib
from spdl_amd._lib import Output
from spdl_amd.io import _image
from tests import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spdl_amd", "csrc")
SWEEP = os.path.join(ROOT, "tests", "native", "ragged_sweep.cpp")

BAD_GEOMETRY = 7
NAMES = ["q90_420", "q90_422", "q90_444", "odd_227x333", "odd_444_101x67", "gray", "gray_odd",
         "tiny_1x1", "tiny_8x8", "cmyk_pillow_odd", "rgb_coded_odd_rst", "prog_444_odd",
         "restart_every_mcu"]


def test_planner_sweep_under_sanitizers(tmp_path):
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
    exe = str(tmp_path / "ragged_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-DHJ_HD=", *san, SWEEP,
                    os.path.join(CSRC, "hj_layout.cpp"), os.path.join(CSRC, "hj_sws.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr
    assert not r.stderr, r.stderr
    last = r.stdout.splitlines()[-1]
    assert last.endswith(" 0 failed expectations") and int(last.split()[0]) >= 100, last


@pytest.fixture(scope="module")
def infos():
    return [_lib.get_image_info(cases.case(n)) for n in NAMES]


SPECS = [
    dict(),
    dict(resize=True, fit_w=64, fit_h=64, aspect="increase"),
    dict(resize=True, fit_w=48, fit_h=48, aspect="decrease"),
    dict(resize=True, fit_w=40, fit_h=-1),
    dict(resize=True, fit_w=-2, fit_h=30),
    dict(resize=True, fit_w=64, fit_h=64, aspect="decrease", pad_w=64, pad_h=64),
]


@pytest.mark.parametrize("spec", SPECS, ids=lambda s: "-".join(f"{k}{v}" for k, v in s.items()))
@pytest.mark.parametrize("pix_fmt,normalize,align", [("rgb24", False, 1), ("rgb", False, 256),
                                                     ("bgr24", True, 2), ("bgr", True, 64)])
def test_ragged_layout_is_output_size_per_image(infos, spec, pix_fmt, normalize, align):
    out = Output(pix_fmt=pix_fmt, normalize=normalize, **spec)
    esz = 2 if normalize else 1
    codes = [k % 8 for k in range(len(infos))]
    for orients in (None, codes):
        offs, sizes, st = _lib.ragged_layout(infos, out, orients=orients, align=align)
        assert st == [0] * len(infos) and len(offs) == len(infos) + 1
        end = 0
        for k, (i, (w, h)) in enumerate(zip(infos, sizes)):
            t = bool(orients and orients[k] & 4)
            # (the spec describes the final output: a transposed image is sized
            # from the stored frame's (h, w), include/spdl_hipjpeg.h)
            want = _lib.output_size(*((i.height, i.width) if t else (i.width, i.height)), out)
            assert (w, h) == want, NAMES[k]
            assert offs[k] % align == 0 and end <= offs[k] < end + align
            end = offs[k] + w * h * 3 * esz
        assert offs[-1] == end


def test_ragged_layout_with_crops_and_refusals(infos):
    out = Output(pix_fmt="rgb24")
    crops = [None] * len(infos)
    crops[0] = (38, 22, 113, 111)    # 4:2:0: rounded down to the chroma grid
    crops[3] = (301, 195, 32, 32)
    crops[5] = (0, 0, 10000, 10)     # wider than the frame: refused alone
    offs, sizes, st = _lib.ragged_layout(infos, out, crops=crops, align=16)
    for k in (0, 3):
        rc, r = _lib.crop_rect(infos[k], crops[k])
        assert rc == 0 and sizes[k] == (r[2], r[3])
    assert sizes[0] == (112, 110)
    assert st[5] == BAD_GEOMETRY and sizes[5] == (0, 0) and offs[6] == offs[5]
    assert [s for k, s in enumerate(st) if k != 5] == [0] * (len(infos) - 1)
    assert sizes[1] == (infos[1].width, infos[1].height)
    # what the extension refuses, and counts that do not match
    for bad in (Output(pix_fmt="yuv"), Output(pix_fmt="rgb24", csc="jfif")):
        with pytest.raises(ValueError, match="no ragged layout"):
            _lib.ragged_layout(infos, bad)
    with pytest.raises(ValueError, match="no ragged layout"):
        _lib.ragged_layout(infos, Output(pix_fmt="rgb", normalize=True), align=1)
    with pytest.raises(ValueError, match="2 crops for a batch of"):
        _lib.ragged_layout(infos, out, crops=crops[:2])
    with pytest.raises(ValueError, match="1 orients for a batch of"):
        _lib.ragged_layout(infos, out, orients=[0])


def test_scale_mode_spellings():
    f = _image._list_filter_desc
    assert f(None, None, None, "bicubic", "rgb24") == "format=pix_fmts=rgb24"
    assert f(40, None, None, "bicubic", "rgb24") == \
        "scale=w=40:h=-1:flags=bicubic,format=pix_fmts=rgb24"
    assert f(-2, 30, None, "bilinear", "bgr") == \
        "scale=w=-2:h=30:flags=bilinear,format=pix_fmts=bgr"
    assert f(64, 48, "fit", "bicubic", "rgb") == \
        "scale=w=64:h=48:flags=bicubic:force_original_aspect_ratio=decrease,format=pix_fmts=rgb"
    assert f(256, None, "cover", "lanczos", "rgb24") == \
        "scale=w=256:h=256:flags=lanczos:force_original_aspect_ratio=increase,format=pix_fmts=rgb24"
    # ... and what the parser makes of them: no pad, no crop
    out = _image.parse_image_filter(f(256, None, "cover", "bicubic", "rgb24"),
                                    default_pix_fmt="rgb24")
    assert (out.resize, out.fit_w, out.fit_h, out.aspect, out.pad_w, out.crop_w) == \
        (True, 256, 256, "increase", 0, 0)
    assert _lib.output_size(640, 480, out) == (341, 256)  # the shorter side meets the box
    out = _image.parse_image_filter(f(48, 48, "fit", "bicubic", "rgb24"), default_pix_fmt="rgb24")
    assert _lib.output_size(640, 480, out) == (48, 36)    # the longer side meets it
    out = _image.parse_image_filter(f(40, None, None, "bicubic", "rgb24"), default_pix_fmt="rgb24")
    assert _lib.output_size(333, 227, out) == (40, 27)
    for bad in ("pad", "crop", "stretch"):
        with pytest.raises(ValueError, match="scale_mode must be"):
            f(64, 64, bad, "bicubic", "rgb24")
    with pytest.raises(ValueError, match="needs a width or a height"):
        f(None, None, "fit", "bicubic", "rgb24")
    with pytest.raises(ValueError, match="one of width and height"):
        f(-1, None, None, "bicubic", "rgb24")


def test_load_image_list_argument_checks():
    d = [cases.case("q90_420")]
    load = _image.load_image_list
    with pytest.raises(ValueError, match="must not be empty"):
        load([])
    with pytest.raises(ValueError, match="no ragged planar YUV"):
        load(d, pix_fmt=None)
    with pytest.raises(ValueError, match="no ragged planar YUV"):
        load(d, filter_desc="scale=64:-1", pix_fmt=None)
    with pytest.raises(ValueError, match="csc='swscale' only"):
        load(d, csc="jfif")
    with pytest.raises(ValueError, match="scale_mode must be"):
        load(d, width=64, height=64, scale_mode="pad")
    with pytest.raises(ValueError, match="exclusive"):
        load(d, width=64, filter_desc="scale=64:-1")
    with pytest.raises(ValueError, match="2 crops for 1 images"):
        load(d, crops=[None, None])
    with pytest.raises(ValueError, match="2 flips for 1 images"):
        load(d, flips=[0, 1])
    with pytest.raises(ValueError, match="a flip is"):
        load(d, flips=[9])
