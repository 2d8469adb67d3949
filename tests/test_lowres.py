"""CPU tests of the reduced-size decode (include/spdl_hipjpeg.h "reduced-size
decode"; no GPU): the transforms of hj_idct.h under sanitizers and against
``tests/lowres_ref.py``, the scale of the reduced planes, libjpeg 9's own
scaled decode as a pin of the 1x1 and 2x2 transforms, the planner, and the
Python surface -- ``lowres=``, ``"auto"``, ``decode_config``."""

import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import spdl_amd.io as sio
from spdl_amd import _lib
from spdl_amd._lib import Output
from spdl_amd.io import _image
from tests import lowres_cases as lc
from tests import lowres_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spdl_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
INVALID_ARG = 8
BOX = Output(pix_fmt="rgb24", resize=True, fit_w=224, fit_h=224, aspect="decrease", pad_w=224,
             pad_h=224)


# ---- the C interface -------------------------------------------------------------------------

def test_header_and_export():
    with open(os.path.join(ROOT, "include", "spdl_hipjpeg.h")) as f:
        flat = " ".join(f.read().split())
    assert "int spdl_hj_set_lowres(spdl_hj_ctx* ctx, const uint8_t* levels, int32_t n);" in flat
    L = _lib.lib()
    assert "spdl_hj_set_lowres" in _lib.EXPORTED and hasattr(L, "spdl_hj_set_lowres")
    assert L.spdl_hj_set_lowres(None, b"\x01", 1) == INVALID_ARG  # (no context)


# ---- the transforms, under sanitizers ----------------------------------------------------------

def _sanitized(tmp_path, name, sources, std="-std=c++17", cxx_names=("g++", "c++")):
    cxx = next((shutil.which(c) for c in cxx_names if shutil.which(c)), None)
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
    subprocess.run([cxx, std, "-O2", "-g", "-DHJ_HD=", *san, *sources, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert not r.stderr, r.stderr
    return r.stdout.splitlines()


def test_transform_sweep_under_sanitizers_and_against_the_reference(tmp_path):
    """hj_idct.h's three transforms equal the sweep's plain-loop restatement on
    random corners, every (d2, d6) zero pattern and the int16 ends; the dump of
    a fixed seed equals the numpy reference."""
    lines = _sanitized(tmp_path, "lowres_sweep", [os.path.join(NATIVE, "lowres_sweep.cpp")])
    assert lines[-1] == "ok"
    counts = {m.group(1): int(m.group(2))
              for m in (re.fullmatch(r"(\w+): (\d+) corners", ln) for ln in lines) if m}
    assert counts == {"random": 240000, "patterns": 256 * 4 * 2 * 8, "ends": 3 * 65536 + 13}
    rows = np.array([[int(v) for v in ln.split()[1:]] for ln in lines if ln.startswith("blk")])
    assert rows.shape == (96, 16 + 16 + 4 + 1)
    blocks = np.zeros((96, 8, 8), np.int64)
    blocks[:, :4, :4] = rows[:, :16].reshape(96, 4, 4)
    # (the corner alone is read: whatever lies outside changes nothing)
    noisy = blocks.copy()
    noisy[:, 4:, :] = 999
    noisy[:, :, 4:] = -999
    for b in (blocks, noisy):
        np.testing.assert_array_equal(ref.idct4(b).reshape(96, 16), rows[:, 16:32])
        np.testing.assert_array_equal(ref.idct2(b).reshape(96, 4), rows[:, 32:36])
        np.testing.assert_array_equal(ref.idct1(b).reshape(96), rows[:, 36])


def test_zero_operand_branches_are_not_the_general_line():
    """d2 == 0 or d6 == 0 takes constants of its own (10703 != 15137 - 4433):
    the reference takes them as written."""
    i64 = np.int64
    only6 = ref._pass4(i64(0), i64(0), i64(0), i64(7))
    assert [int(v) for v in only6] == [7 * 4433, -7 * 10703, 7 * 10703, -7 * 4433]
    assert -7 * 10703 != 7 * 4433 - 7 * 15137  # (what the general line gives)
    only2 = ref._pass4(i64(0), i64(5), i64(0), i64(0))
    assert [int(v) for v in only2] == [5 * 10703, 5 * 4433, -5 * 4433, -5 * 10703]
    # (here the general line agrees, 4433 + 6270 = 10703: only the d2 == 0 branch is its own)
    both = ref._pass4(i64(1), i64(5), i64(2), i64(7))
    z1 = 12 * 4433
    assert [int(v) for v in both] == [3 * 8192 + z1 + 5 * 6270, -8192 + z1 - 7 * 15137,
                                      -8192 - z1 + 7 * 15137, 3 * 8192 - z1 - 5 * 6270]


def test_layout_sweep_under_sanitizers(tmp_path):
    """The planner: reduced sizes, strides, workspace bytes, windows and lanes
    for W, H in {1, 7, 8, 9, 17, 65535} x level 0..3 x gray and chroma ratios
    1, 2, 4; level-0 rows byte-identical to a plan without the call; the chain
    of a reduced frame equal to that of a frame of the reduced size; and every
    refusal: a wrong count, a level above 3, levels with crops and with csc =
    jfif (INVALID_ARG), a 4-component frame with a level (UNSUPPORTED, alone)."""
    lines = _sanitized(tmp_path, "lowres_layout_sweep",
                       [os.path.join(NATIVE, "lowres_layout_sweep.cpp"),
                        os.path.join(CSRC, "hj_layout.cpp"), os.path.join(CSRC, "hj_sws.cpp")])
    assert lines[-1] == "ok"
    m = re.fullmatch(r"(\d+) cases, 0 failures", lines[-2])
    assert m and int(m.group(1)) == 6 * 6 * 4 * 6 + 6


def test_sweeps_see_the_library_through_host_headers_alone():
    for name in ("lowres_sweep.cpp", "lowres_layout_sweep.cpp"):
        with open(os.path.join(NATIVE, name)) as f:
            src = f.read()
        assert all(i.startswith("../../spdl_amd/csrc/hj_")
                   for i in re.findall(r'#\s*include\s*"([^"]+)"', src))
        assert not re.search(r'#\s*include\s*[<"]hip/', src)


# ---- scale and bias ----------------------------------------------------------------------------

def test_reduced_planes_track_the_box_average(oracle):
    """The mean absolute difference between the reduced luma plane and the
    2^L x 2^L box average of the full decode, over four smooth 4:4:4 files.
    Measured with the reference alone: 0.55 (4x4), 1.63 (2x2), 0.23 (1x1);
    asserted at twice each.  A wrong shift or bias is off by tens; this says
    nothing about quality (the 2x2 is as crude as FFmpeg's)."""
    for level, measured in ((1, 0.55), (2, 1.63), (3, 0.23)):
        k, diffs = 1 << level, []
        for seed in (1, 2, 3, 4):
            d = lc.smooth_444(seed)
            full = oracle.decode_planes(d)[0].astype(np.float64)
            h, w = full.shape
            box = full.reshape(h // k, k, w // k, k).mean(axis=(1, 3))
            _, planes = ref.planes(d, level)
            diffs.append(np.abs(planes[0] - box).mean())
        assert np.mean(diffs) <= 2 * measured, (level, diffs)


# ---- libjpeg 9's scaled decode ---------------------------------------------------------------

LJ_PREFIX = "/opt/conda"


@pytest.mark.skipif(not os.path.exists(os.path.join(LJ_PREFIX, "include", "jpeglib.h")),
                    reason="no IJG libjpeg 9 headers")
@pytest.mark.parametrize("num,level", [(1, 3), (2, 2)])
def test_libjpeg9_scaled_decode_equals_the_luma_plane(tmp_path, oracle, num, level):
    """scale 1/8 and 2/8, JDCT_ISLOW, of gray files: byte for byte the level 3
    and level 2 luma planes (both are (DC + 4) >> 3 after the level shift; the
    2x2 butterflies are the same sums)."""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler")
    exe = str(tmp_path / "lj_scaled")
    build = subprocess.run([cc, "-O2", f"-I{LJ_PREFIX}/include", os.path.join(NATIVE, "lj_scaled.c"),
                            "-o", exe, f"-L{LJ_PREFIX}/lib", "-l:libjpeg.so.9",
                            f"-Wl,-rpath,{LJ_PREFIX}/lib"], capture_output=True, text=True)
    if build.returncode:
        pytest.skip("libjpeg 9 does not link here: " + build.stderr[-300:])
    for w, h in lc.SIZES:
        d = lc.sized("gray", w, h)
        src, raw = tmp_path / "in.jpg", tmp_path / "out.raw"
        src.write_bytes(d)
        r = subprocess.run([exe, str(src), str(num), str(raw)], capture_output=True, text=True,
                           check=True)
        ow, oh = (int(v) for v in r.stdout.split())
        _, planes = ref.planes(d, level)
        assert (oh, ow) == planes[0].shape
        got = np.frombuffer(raw.read_bytes(), np.uint8).reshape(oh, ow)
        np.testing.assert_array_equal(got, planes[0], strict=True)


# ---- "auto", levels, decode_config -----------------------------------------------------------

def test_auto_resolution_table():
    assert _lib.auto_lowres(480, 640, BOX) == 1    # 240x320 >= 168x224, 120x160 is not
    assert _lib.auto_lowres(640, 480, BOX) == 1
    assert _lib.auto_lowres(4000, 3000, BOX) == 3  # 500x375 >= 224x168
    assert _lib.auto_lowres(300, 300, BOX) == 0    # 150x150 < 224x224
    assert _lib.auto_lowres(448, 448, BOX) == 1    # exactly the scaled size
    assert _lib.auto_lowres(447, 447, BOX) == 1    # ceil(447 / 2) = 224
    assert _lib.auto_lowres(446, 446, BOX) == 0
    assert _lib.auto_lowres(4000, 3000, Output(pix_fmt="rgb24")) == 0  # native size
    stretch = Output(pix_fmt="rgb24", resize=True, fit_w=100, fit_h=400)
    assert _lib.auto_lowres(800, 800, stretch) == 1  # the taller side decides
    assert _lib.lowres_size(65535, 1, 3) == (8192, 1) and _lib.lowres_size(17, 9, 2) == (5, 3)


def _infos(sizes):
    out = []
    for w, h in sizes:
        i = _lib.ImageInfo()
        i.width, i.height, i.ncomp = w, h, 1
        i.h_samp[0] = i.v_samp[0] = 1
        out.append(i)
    return out


def test_levels_per_image():
    infos = _infos([(480, 640), (4000, 3000), (300, 300)])
    assert _lib.lowres_levels(None, infos, BOX) is None
    assert _lib.lowres_levels(0, infos, BOX) is None
    assert _lib.lowres_levels([0, 0, 0], infos, BOX) is None
    assert _lib.lowres_levels(2, infos, BOX) == [2, 2, 2]
    assert _lib.lowres_levels("auto", infos, BOX) == [1, 3, 0]
    assert _lib.lowres_levels([3, "auto", 1], infos, BOX) == [3, 3, 1]
    # a transposed image is sized from the stored frame's (h, w)
    tall = Output(pix_fmt="rgb24", resize=True, fit_w=100, fit_h=400)
    assert _lib.lowres_levels("auto", _infos([(800, 1600)]), tall) == [2]  # 200x400 >= 100x400
    assert _lib.lowres_levels("auto", _infos([(800, 1600)]), tall, orients=[5]) == [1]
    for bad in (4, -1, True, "1", 1.0, [1, 2], [1, 2, 9]):
        with pytest.raises(ValueError):
            _lib.lowres_levels(bad, infos, BOX)


def test_ragged_layout_sizes_boxes_from_the_reduced_frames():
    infos = _infos([(50, 37), (64, 48), (33, 31)])
    out = Output(pix_fmt="rgb24")
    _, sizes, st = _lib.ragged_layout(infos, out, lowres=[1, 0, 3])
    assert st == [0, 0, 0] and sizes == [(25, 19), (64, 48), (5, 4)]
    assert _lib.ragged_layout(infos, out, lowres=None)[1] == [(50, 37), (64, 48), (33, 31)]
    assert infos[0].width == 50  # (the caller's probes are left alone)


def test_decode_config_is_honoured(monkeypatch):
    monkeypatch.setattr(_image, "_IGNORED_WARNED", set())
    cfg = sio.decode_config(decoder_options={"lowres": "2"})
    assert isinstance(cfg, sio.DecodeConfig) and cfg.decoder is None
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # lowres alone: nothing is ignored, nothing warns
        assert _image._ffmpeg_configs({"decode_config": cfg}, None) == 2
        assert _image._ffmpeg_configs({"decode_config": {"decoder_options": {"lowres": 1}}}, None) == 1
        assert _image._ffmpeg_configs({"decode_config": cfg}, 2) == 2  # both spellings, agreeing
        assert _image._ffmpeg_configs({}, "auto") == "auto"
        assert _image._ffmpeg_configs({"decode_config": None}, 3) == 3
    for other in (1, "auto", 0):
        with pytest.raises(ValueError, match="disagree"):
            _image._ffmpeg_configs({"decode_config": cfg}, other)
    with pytest.raises(ValueError, match="no integer"):
        _image._ffmpeg_configs({"decode_config": sio.decode_config(decoder_options={"lowres": "x"})},
                               None)
    # every other option keeps the once-only warning, the level still comes through
    kw = {"decode_config": sio.decode_config(decoder_options={"lowres": "1", "threads": "2"})}
    with pytest.warns(RuntimeWarning, match="decode_config"):
        assert _image._ffmpeg_configs(kw, None) == 1
    assert not kw
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (once only)
        assert _image._ffmpeg_configs({"decode_config": sio.decode_config(decoder="mjpeg")}, None) \
            is None
    with pytest.warns(RuntimeWarning, match="demux_config"):
        assert _image._ffmpeg_configs({"demux_config": object()}, 1) == 1


def test_python_refusals_before_any_decode():
    d = lc.sized("420", 64, 48)
    with pytest.raises(ValueError, match="exclusive"):
        sio.load_image_batch([d], width=16, height=16, lowres=1, crops=[(0, 0, 32, 32)])
    with pytest.raises(ValueError, match="exclusive"):
        sio.load_image_list([d], lowres=[1], crops=[(0, 0, 32, 32)])
    with pytest.raises(ValueError, match="0..3"):
        sio.load_image_batch([d], width=16, height=16, lowres=4)
    with pytest.raises(ValueError, match="lowres levels for"):
        sio.load_image_batch([d], width=16, height=16, lowres=[1, 1])
    with pytest.raises(ValueError, match="disagree"):
        sio.load_image([d][0], lowres=1,
                       decode_config=sio.decode_config(decoder_options={"lowres": "2"}))
