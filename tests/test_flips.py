"""CPU tests of output flips (include/spdl_hipjpeg.h "output flips"): the
declaration and its binding, where the filter parser takes hflip / vflip and
where it refuses them, what the Python layer marshals, and -- as a stand-alone
program under ASan and UBSan -- the tile arithmetic of the store
(hj_sws_tile.h tile_flip) and the planner's rules for the flags
(tests/native/flip_sweep.cpp).
"""

import os
import re
import shutil
import subprocess

import pytest

import spdl_amd.io as sio
from spdl_amd import _lib
from spdl_amd._lib import Output, ViewGroup
from spdl_amd.io._preprocessing import parse_image_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spdl_amd", "csrc")
INVALID_ARG = 8
SCALE = "scale=w=64:h=48:flags=bicubic"


def _header() -> str:
    with open(os.path.join(ROOT, "include", "spdl_hipjpeg.h")) as f:
        return f.read()


# ---- header and binding ---------------------------------------------------------------

def test_header_declares_flips_and_keeps_the_abi():
    h = _header()
    assert "#define SPDL_HJ_ABI_VERSION 7" in h  # additive: the version stays
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", h, flags=re.S))
    assert "enum { SPDL_HJ_FLIP_H = 1, SPDL_HJ_FLIP_V = 2 };" in flat
    assert "int spdl_hj_set_flips(spdl_hj_ctx* ctx, const uint8_t* flips, int32_t n);" in flat


def test_header_states_the_contract_and_its_two_limits():
    h = re.sub(r"\s*\n \*\s*", " ", _header())
    block = h[h.index("---- output flips"):h.index("enum { SPDL_HJ_FLIP_H")]
    for phrase in ("LAST node of the chain",
                   "out'(x, y) = out(ow - 1 - x, oh - 1 - y)",
                   "every plane mirrored by its own width and height",
                   "Pad bytes belong to the image and move with it",
                   "byte-identical to the same submission without flips",
                   "whether or not it succeeds",
                   "flips == NULL or n == 0 clears them",
                   "the library copies the array",
                   "neither use nor clear them",
                   "one entry per view, the groups concatenated in group order",
                   "a value above 3",
                   "csc = JFIF with any non-zero flip",
                   "with nothing written",
                   "a flip AHEAD of the scale",
                   "runs the generic output kernel"):
        assert phrase in block, phrase


def test_binding_finds_the_symbol():
    L = _lib.lib()
    assert "spdl_hj_set_flips" in _lib.EXPORTED and hasattr(L, "spdl_hj_set_flips")
    assert _lib.ABI_VERSION == 7 and L.spdl_hj_abi_version() == 7
    assert (_lib.FLIP_H, _lib.FLIP_V) == (1, 2)
    assert L.spdl_hj_set_flips(None, b"\x01", 1) == INVALID_ARG  # (no context)
    assert L.spdl_hj_set_flips(None, None, 0) == INVALID_ARG


# ---- spelling ----------------------------------------------------------------------------

@pytest.mark.parametrize("spelt, bits", [(None, 0), (0, 0), (1, 1), (2, 2), (3, 3), ("h", 1),
                                         ("v", 2), ("hv", 3)])
def test_a_flip_is_spelt(spelt, bits):
    assert _lib._flip(spelt) == bits


@pytest.mark.parametrize("bad", [4, -1, "x", "hh", 1.0, True, (1,)])
def test_a_bad_flip_raises(bad):
    with pytest.raises(ValueError, match="a flip is 0..3"):
        _lib._flip(bad)


def test_view_group_takes_a_flip_per_view():
    out = Output(pix_fmt="rgb24", resize=True, fit_w=8, fit_h=8)
    g = ViewGroup(out, [(0, None), (0, None, "h"), (1, (1, 2, 3, 4), 2), (1, None, None)], 4096,
                  4 * 192)
    assert g.flips == [0, 1, 2, 0] and len(g.views) == 4
    assert g.to_c().nviews == 4
    # Output.flip: every view without one of its own
    g = ViewGroup(Output(pix_fmt="rgb24", flip="v"), [(0, None), (0, None, 1)], 4096, 64)
    assert g.flips == [2, 1]
    with pytest.raises(ValueError, match=r"a view is \(image, rect_or_None\)"):
        ViewGroup(out, [(0, None, 4)], 4096, 64)


class _Recorder:
    """A Decoder whose flips go to a list and whose native handle is never used."""

    _h = None
    _flips = _lib.Decoder._flips

    def __init__(self):
        self.calls = []

    def set_flips(self, flips):
        self.calls.append(bytes(flips) if isinstance(flips, (bytes, bytearray))
                          else [_lib._flip(f) for f in flips])


def test_decoder_hands_over_the_flips_of_a_submission():
    d = _Recorder()
    d._flips(Output(), [0, "h", None], 3)
    d._flips(Output(flip="hv"), None, 2)
    assert d.calls == [[0, 1, 0], [3, 3]]
    with pytest.raises(ValueError, match="2 flips for a batch of 3 images"):
        d._flips(Output(), [0, 1], 3)
    with pytest.raises(ValueError, match="exclusive"):
        d._flips(Output(flip=1), [0, 1], 2)
    # views: each view's own, the groups concatenated; none set: no call at all
    d = _Recorder()
    g0 = ViewGroup(Output(pix_fmt="rgb24"), [(0, None, 1), (0, None)], 4096, 64)
    g1 = ViewGroup(Output(pix_fmt="rgb24"), [(0, None, "v")], 4096, 64)
    d._flips(Output(), None, 1, [g0, g1])
    assert d.calls == [bytes([1, 0, 2])]
    with pytest.raises(ValueError, match="belongs to its view"):
        d._flips(Output(), [1], 1, [g0])
    d = _Recorder()
    d._flips(Output(), None, 1, [ViewGroup(Output(pix_fmt="rgb24"), [(0, None)], 4096, 64)])
    assert d.calls == []
    assert not _lib._has_flips(Output(), None, None)


def test_io_validates_flips_before_any_decode():
    cfg = sio.cuda_config(device_index=0)
    with pytest.raises(ValueError, match="2 flips for 1 images"):
        sio.load_image_batch([b"x"], width=8, height=8, device_config=cfg, flips=[0, 1])
    with pytest.raises(ValueError, match="a flip is 0..3"):
        sio.load_image_batch([b"x"], width=8, height=8, device_config=cfg, flips=[4])
    with pytest.raises(ValueError, match="needs a filter chain"):
        sio.load_image_batch([b"x"], width=None, height=None, pix_fmt=None, filter_desc=None,
                             device_config=cfg, flips=[1])
    with pytest.raises(ValueError, match="exclusive"):
        sio.load_image_batch([b"x"], width=8, height=8, device_config=cfg, flips=[1],
                             filter_desc=SCALE + ",hflip")
    ok = dict(width=64, height=64, crops=[[(1, 2, 30, 40), None]])
    with pytest.raises(ValueError, match="parallel to crops"):
        sio.load_image_views([b"x"], [dict(ok, flips=[[1]])], device_config=cfg)
    with pytest.raises(ValueError, match="a flip is 0..3"):
        sio.load_image_views([b"x"], [dict(ok, flips=[[1, 7]])], device_config=cfg)


# ---- the filter parser ---------------------------------------------------------------------

@pytest.mark.parametrize("chain, flip", [
    (SCALE + ",hflip", 1),
    (SCALE + ",vflip", 2),
    (SCALE + ",hflip,vflip", 3),
    (SCALE + ",vflip,hflip", 3),
    (SCALE + ",pad=w=80:h=80:x=-1:y=-1:color=black,hflip", 1),
    (SCALE + ",pad=w=80:h=80:x=-1:y=-1:color=black,crop=w=40:h=40,vflip", 2),
    (SCALE + ",hflip,format=pix_fmts=rgb24", 1),      # before format
    (SCALE + ",format=pix_fmts=bgr24,hflip", 1),      # ... or after it
    (SCALE + ",hflip,format=pix_fmts=rgb,vflip", 3),
    ("crop=w=32:h=32:x=4:y=4," + SCALE + ",hflip", 1),  # a source crop ahead of scale is fine
])
def test_parser_takes_flips_at_the_end_of_the_chain(chain, flip):
    out = parse_image_filter(chain)
    assert out.flip == flip and out.resize and (out.fit_w, out.fit_h) == (64, 48)


def test_repeated_flips_toggle():
    assert parse_image_filter(SCALE + ",hflip,hflip").flip is None
    assert parse_image_filter(SCALE + ",hflip,vflip,hflip").flip == 2
    assert parse_image_filter(SCALE + ",vflip,hflip,vflip,hflip").flip is None
    assert parse_image_filter(SCALE).flip is None
    # a pair that cancels leaves a chain later nodes may extend
    assert parse_image_filter(SCALE + ",hflip,hflip,crop=w=32:h=32").crop_w == 32


@pytest.mark.parametrize("chain", ["hflip," + SCALE, "vflip," + SCALE + ",format=pix_fmts=rgb24",
                                   "crop=w=32:h=32:x=4:y=4,hflip," + SCALE])
def test_a_flip_ahead_of_scale_is_refused(chain):
    with pytest.raises(ValueError) as e:
        parse_image_filter(chain)
    msg = str(e.value)
    assert "ahead of scale" in msg and "pixels would differ" in msg
    assert "filter positions" in msg and "odd-width chroma" in msg


@pytest.mark.parametrize("chain, node", [
    (SCALE + ",hflip,pad=w=80:h=80:x=-1:y=-1:color=black", "pad"),
    (SCALE + ",vflip,crop=w=32:h=32", "crop"),
    (SCALE + ",pad=w=80:h=80:x=-1:y=-1:color=black,hflip,crop=w=32:h=32", "crop"),
    (SCALE + ",hflip,scale=w=32:h=32", "scale"),
])
def test_a_flip_between_scale_and_a_later_node_is_refused(chain, node):
    with pytest.raises(ValueError) as e:
        parse_image_filter(chain)
    msg = str(e.value)
    assert f"ahead of {node}" in msg and "pixels would differ" in msg
    assert "filter positions" in msg and "odd remainder of a centred pad" in msg


@pytest.mark.parametrize("chain", ["hflip", "vflip", "hflip,vflip", "format=pix_fmts=rgb24,hflip",
                                   "crop=w=32:h=32,hflip"])
def test_a_flip_in_a_chain_without_scale_still_raises(chain):
    with pytest.raises(ValueError):
        parse_image_filter(chain)


def test_a_flip_takes_no_options():
    with pytest.raises(ValueError, match="takes no options"):
        parse_image_filter(SCALE + ",hflip=1")


# ---- the tile arithmetic and the planner, under sanitizers -----------------------------------

def test_flip_sweep_under_sanitizers(tmp_path):
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
    exe = str(tmp_path / "flip_sweep")
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-DHJ_HD=", *san,
                    os.path.join(ROOT, "tests", "native", "flip_sweep.cpp"),
                    os.path.join(CSRC, "hj_layout.cpp"), os.path.join(CSRC, "hj_sws.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert not r.stderr, r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and lines[1] == "planner: rules hold"
    m = re.fullmatch(r"tiles: (\d+) boxes, (\d+) pixels", lines[0])
    # 70 x 70 sizes x 3 chunks x 4 bands x 4 flips, the box and its chroma plane
    assert m and int(m.group(1)) == 70 * 70 * 3 * 4 * 4 * 2
    # sides of 32768 and 65535 x 1 and 17, both ways, 2 chunks x 2 bands x 4 flips, with chroma
    m = re.fullmatch(r"extreme tiles: (\d+) boxes, (\d+) pixels", lines[2])
    assert m and int(m.group(1)) == 2 * 2 * 2 * 2 * 2 * 4 * 2


def test_sweep_sees_the_library_through_host_headers_alone():
    with open(os.path.join(ROOT, "tests", "native", "flip_sweep.cpp")) as f:
        src = f.read()
    assert re.findall(r'#\s*include\s*"([^"]+)"', src) == ["../../spdl_amd/csrc/hj_layout.h",
                                                           "../../spdl_amd/csrc/hj_sws_tile.h"]
    assert not re.search(r'#\s*include\s*[<"]hip/', src)
