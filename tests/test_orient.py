"""CPU tests of output orientations (include/spdl_hipjpeg.h "output
orientation"): the declarations and their binding, the spellings and the EXIF
table, where the filter parser takes ``transpose`` and where it refuses it,
what the Python layer marshals, the EXIF reader against Pillow and against
hand-made APP1 segments, the table against ``PIL.ImageOps.exif_transpose`` --
and, as stand-alone programs under ASan and UBSan, the tile arithmetic of the
oriented store with the planner's rules (tests/native/orient_sweep.cpp) and
the EXIF reader over every truncation and corruption (tests/native/exif_sweep.cpp).
"""

import io
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import spdl_amd.io as sio
from spdl_amd import _lib
from spdl_amd._lib import Output, ViewGroup
from spdl_amd.io._preprocessing import parse_image_filter
from tests import exif_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spdl_amd", "csrc")
NOT_JPEG, INVALID_ARG = 1, 8
SCALE = "scale=w=64:h=48:flags=bicubic"
PAD = "pad=w=80:h=70:x=-1:y=-1:color=black"
EXIF_TABLE = {1: 0, 2: 1, 3: 3, 4: 2, 5: 4, 6: 5, 7: 7, 8: 6}


def _header() -> str:
    with open(os.path.join(ROOT, "include", "spdl_hipjpeg.h")) as f:
        return f.read()


def _oriented(a, code):
    """[H, W, ...] under orientation ``code``: the header's formula in numpy."""
    if code & 4:
        a = np.swapaxes(a, 0, 1)
    if code & 1:
        a = np.flip(a, 1)
    if code & 2:
        a = np.flip(a, 0)
    return np.ascontiguousarray(a)


# ---- header and binding ---------------------------------------------------------------

def test_header_declares_the_orientation_symbols_and_keeps_the_abi():
    h = _header()
    assert "#define SPDL_HJ_ABI_VERSION 7" in h  # additive: the version stays
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", h, flags=re.S))
    assert "enum { SPDL_HJ_ORIENT_H = 1, SPDL_HJ_ORIENT_V = 2, SPDL_HJ_ORIENT_T = 4 };" in flat
    assert ("int spdl_hj_set_orients(spdl_hj_ctx* ctx, const uint8_t* orients, int32_t n);"
            in flat)
    assert ("int spdl_hj_get_orientation(const uint8_t* data, size_t size, int32_t* exif);"
            in flat)
    assert "int spdl_hj_orient_code(int32_t exif);" in flat
    # the flips block stands as it was, ahead of the new one
    assert h.index("---- output flips") < h.index("int spdl_hj_set_flips") < \
        h.index("---- output orientation") < h.index("int spdl_hj_set_orients")


def test_header_states_the_contract_and_what_is_not_offered():
    h = re.sub(r"\s*\n \*\s*", " ", _header())
    block = h[h.index("---- output orientation"):h.index("int spdl_hj_orient_code")]
    for phrase in ("bit 2 is a transpose applied BEFORE them",
                   "A(x, y) = C(y, x)",
                   "out(x, y) = A(H ? aw - 1 - x : x, V ? ah - 1 - y : y)",
                   "Codes 0..3 are exactly the flips",
                   "describes the FINAL output",
                   "(fit_w, fit_h), (pad_w, pad_h), (crop_w, crop_h)",
                   "stay in the stored frame's coordinates",
                   "pass it the stored frame's (h, w)",
                   "a transpose AHEAD of the scale",
                   "a value above 7",
                   "a T code with SPDL_HJ_FMT_YUV",
                   "orients together with flips on one submission",
                   "with nothing written",
                   "byte-identical to no call and keeps the fused full-resolution path",
                   "first APP1 whose payload starts",
                   "EXIF never fails an image",
                   "5 -> 4 (T)   6 -> 5 (T|H)   7 -> 7 (T|H|V)   8 -> 6 (T|V)"):
        assert phrase in block, phrase


def test_binding_finds_the_symbols():
    L = _lib.lib()
    for name in ("spdl_hj_set_orients", "spdl_hj_get_orientation", "spdl_hj_orient_code"):
        assert name in _lib.EXPORTED and hasattr(L, name), name
    assert _lib.ABI_VERSION == 7 and L.spdl_hj_abi_version() == 7
    assert (_lib.ORIENT_H, _lib.ORIENT_V, _lib.ORIENT_T) == (1, 2, 4)
    assert L.spdl_hj_set_orients(None, b"\x05", 1) == INVALID_ARG  # (no context)
    assert L.spdl_hj_set_orients(None, None, 0) == INVALID_ARG
    assert L.spdl_hj_get_orientation(b"\xff\xd8\xff\xd9", 4, None) == INVALID_ARG
    assert L.spdl_hj_set_flips(None, b"\x01", 1) == INVALID_ARG  # (the flips' entry stands)


# ---- spellings, the EXIF table --------------------------------------------------------------

@pytest.mark.parametrize("spelt, bits", [(None, 0), ("", 0), ("h", 1), ("v", 2), ("hv", 3), ("vh", 3),
                                         ("t", 4), ("cclock_flip", 4), ("clock", 5), ("cclock", 6),
                                         ("clock_flip", 7)] + [(k, k) for k in range(8)])
def test_an_orientation_is_spelt(spelt, bits):
    assert _lib._orient(spelt) == bits


@pytest.mark.parametrize("bad", [8, -1, "x", "tt", 1.0, True, (1,)])
def test_a_bad_orientation_raises(bad):
    with pytest.raises(ValueError, match="an orientation is 0..7"):
        _lib._orient(bad)


def test_a_flip_still_stops_at_three():
    with pytest.raises(ValueError, match="a flip is 0..3"):
        _lib._flip(4)


def test_exif_table_in_python_and_in_the_library():
    L = _lib.lib()
    for exif, code in EXIF_TABLE.items():
        assert _lib.exif_code(exif) == code == L.spdl_hj_orient_code(exif)
    for bad in (0, 9, -1, 100):
        assert L.spdl_hj_orient_code(bad) == -1
        with pytest.raises(ValueError, match="an EXIF orientation is 1..8"):
            _lib.exif_code(bad)
    with pytest.raises(ValueError):
        _lib.exif_code(True)


def test_a_flip_of_the_displayed_image_is_xor():
    """Flipping the oriented image horizontally / vertically is the code with
    that bit toggled, for every code: the composition the io layer uses."""
    a = np.arange(5 * 7).reshape(5, 7)
    for code in range(8):
        for f in range(4):
            np.testing.assert_array_equal(_oriented(_oriented(a, code), f), _oriented(a, code ^ f))


# ---- the table against Pillow ----------------------------------------------------------------

def test_table_against_pillow_exif_transpose():
    Image = pytest.importorskip("PIL.Image")
    ImageOps = pytest.importorskip("PIL.ImageOps")
    a = np.arange(5 * 7, dtype=np.uint8).reshape(5, 7)  # 7 wide, 5 tall: an index image
    for exif in range(1, 9):
        img = Image.fromarray(a)
        ex = img.getexif()
        ex[0x0112] = exif
        img.info["exif"] = ex.tobytes()
        shown = ImageOps.exif_transpose(img)
        np.testing.assert_array_equal(np.asarray(shown), _oriented(a, _lib.exif_code(exif)),
                                      err_msg=f"EXIF {exif}")


# ---- get_orientation ---------------------------------------------------------------------------

def test_get_orientation_of_files_pillow_writes():
    Image = pytest.importorskip("PIL.Image")
    img = Image.new("RGB", (24, 16), (200, 100, 50))
    plain = io.BytesIO()
    img.save(plain, "JPEG")
    assert _lib.get_orientation(plain.getvalue()) == 1  # (JFIF alone: no APP1)
    for exif in range(1, 9):
        ex = Image.Exif()
        ex[0x0112] = exif
        ex[0x010F] = "a camera"  # (Make, ahead of it in IFD0)
        buf = io.BytesIO()
        img.save(buf, "JPEG", exif=ex)
        data = buf.getvalue()
        assert Image.open(io.BytesIO(data)).getexif()[0x0112] == exif
        assert _lib.get_orientation(data) == exif
        assert _lib.get_orientation(memoryview(data)) == exif


def test_get_orientation_fails_only_where_the_probe_fails():
    for junk in (b"", b"\x89PNG\r\n", b"\xff\xd8\xff\xd9"):
        with pytest.raises(RuntimeError, match="header probe"):
            _lib.get_image_info(junk)
        with pytest.raises(RuntimeError, match="header probe"):
            _lib.get_orientation(junk)


@pytest.fixture(scope="module")
def base_jpeg():
    pytest.importorskip("PIL")
    return ec.base_jpeg()


def test_hand_made_segments(base_jpeg):
    seen = set()
    for name, payloads, want in ec.cases():
        data, lo, hi = ec.with_app1(base_jpeg, payloads)
        assert data[lo:lo + 2] == (b"\xff\xe1" if payloads else data[2:4])
        assert _lib.get_orientation(data) == want, name
        assert _lib.get_image_info(data).width == 16  # EXIF never fails an image
        seen.add(name)
    for must in ("ii_short_6", "mm_short_8", "mm_long_6", "ii_not_first", "second_exif", "no_app1",
                 "xmp_app1", "ii_truncated_in_entry", "mm_offset_outside", "ii_type_byte",
                 "mm_count_2", "ii_value_0", "mm_value_9"):
        assert must in seen, must


def test_a_segment_running_past_the_file_is_orientation_one(base_jpeg):
    # the walk stops at a segment whose length runs past the file; here the
    # probe has its frame first (APP1 behind SOF), so the image still stands
    from tests import jpeg_headers as jh

    segs, tail = jh.split(base_jpeg)
    app1 = ec.EXIF + ec.tiff("little", [ec.orientation("little", 6)])
    ahead = jh.join(jh.edit(segs, insert=[(jh.APP1, app1)], before=jh.SOS), tail)
    assert _lib.get_orientation(ahead) == 6
    cut = ahead[:ahead.index(b"\xff\xe1") + 4 + 20]  # the file ends inside the APP1
    assert _lib.get_image_info(cut).width == 16 and _lib.get_orientation(cut) == 1


# ---- what the Python layer marshals ---------------------------------------------------------

def test_view_group_takes_an_orientation_as_its_fourth_element():
    out = Output(pix_fmt="rgb24", resize=True, fit_w=8, fit_h=8)
    g = ViewGroup(out, [(0, None), (0, None, "h"), (1, (1, 2, 3, 4), None, 5), (1, None, None, "t")],
                  4096, 4 * 192)
    assert g.flips == [0, 1, 0, 0] and g.orients == [None, None, 5, 4] and len(g.views) == 4
    g = ViewGroup(Output(pix_fmt="rgb24", orient="clock"), [(0, None), (0, None, None, 2)], 4096, 64)
    assert g.orients == [5, 2] and g.flips == [0, 0]
    for bad in ([(0, None, 1, 5)], [(0, None, None, 8)], [(0, None, None, 5, 1)]):
        with pytest.raises(ValueError, match=r"a view is \(image, rect_or_None\)"):
            ViewGroup(out, bad, 4096, 64)
    with pytest.raises(ValueError, match="exclusive"):
        ViewGroup(Output(pix_fmt="rgb24", flip=1, orient=4), [(0, None)], 4096, 64)


class _Recorder:
    """A Decoder whose flips and orientations go to a list and whose native
    handle is never used."""

    _h = None
    _flips = _lib.Decoder._flips
    _crops = _lib.Decoder._crops
    set_crops = None

    def __init__(self):
        self.calls = []

    def set_flips(self, flips):
        self.calls.append(("flips", bytes(flips) if isinstance(flips, (bytes, bytearray))
                           else bytes(_lib._flip(f) for f in flips)))

    def set_orients(self, orients):
        self.calls.append(("orients", bytes(orients) if isinstance(orients, (bytes, bytearray))
                           else bytes(_lib._orient(o) for o in orients)))

    def submit(self, out, n, flips=None, orients=None, views=None):
        self.calls = []
        _lib.Decoder._submit(self, n, out, 0, 0, None, views, flips, True, True, [0] * n,
                             lambda err: 0, orients)
        return self.calls


def test_decoder_hands_over_the_orientations_of_a_submission(monkeypatch):
    monkeypatch.setattr(_lib, "_check_views", lambda *a: None)
    d = _Recorder()
    d.set_views = lambda views: None
    assert d.submit(Output(), 3, orients=[0, "clock", None]) == [("orients", bytes([0, 5, 0]))]
    assert d.submit(Output(orient=6), 2) == [("orients", bytes([6, 6]))]
    assert d.submit(Output(), 2, flips=[1, 0]) == [("flips", bytes([1, 0]))]  # (flips stay flips)
    assert d.submit(Output(), 2) == []
    with pytest.raises(ValueError, match="2 orients for a batch of 3 images"):
        d.submit(Output(), 3, orients=[0, 1])
    with pytest.raises(ValueError, match="flips= and orients= are exclusive"):
        d.submit(Output(), 2, flips=[0, 1], orients=[4, 0])
    with pytest.raises(ValueError, match="exclusive"):
        d.submit(Output(orient=4), 2, orients=[4, 0])
    with pytest.raises(ValueError, match="exclusive"):
        d.submit(Output(flip=1), 2, orients=[4, 0])
    # views: each view's own code -- its orientation, else its flip -- the groups concatenated
    g0 = ViewGroup(Output(pix_fmt="rgb24"), [(0, None, 1), (0, None, None, 5)], 4096, 64)
    g1 = ViewGroup(Output(pix_fmt="rgb24"), [(0, None, "v")], 4096, 64)
    assert d.submit(Output(), 1, views=[g0, g1]) == [("orients", bytes([1, 5, 2]))]
    assert d.submit(Output(), 1, views=[g1]) == [("flips", bytes([2]))]
    with pytest.raises(ValueError, match="belongs to its view"):
        d.submit(Output(), 1, orients=[5], views=[g0])


def test_io_validates_before_any_decode():
    cfg = sio.cuda_config(device_index=0)
    with pytest.raises(ValueError, match="needs a filter chain"):
        sio.load_image_batch([b"x"], width=None, height=None, pix_fmt=None, filter_desc=None,
                             device_config=cfg, exif_orientation=True)
    with pytest.raises(ValueError, match="need a filter chain"):
        sio.load_image(b"\xff\xd8", filter_desc=None, device_config=cfg, exif_orientation=True)


# ---- the filter parser ---------------------------------------------------------------------

@pytest.mark.parametrize("chain, orient", [
    (SCALE + ",transpose=cclock_flip", 4),
    (SCALE + ",transpose=clock", 5),
    (SCALE + ",transpose=cclock", 6),
    (SCALE + ",transpose=clock_flip", 7),
    (SCALE + ",transpose=0", 4),
    (SCALE + ",transpose=dir=1", 5),
    (SCALE + ",transpose=2", 6),
    (SCALE + ",transpose=dir=3", 7),
    (SCALE + ",transpose=dir=clock", 5),
    (SCALE + ",transpose=clock,format=pix_fmts=rgb24", 5),   # before format
    (SCALE + ",format=pix_fmts=bgr24,transpose=clock", 5),   # ... or after it
    ("crop=w=32:h=32:x=4:y=4," + SCALE + ",transpose=clock", 5),  # a source crop ahead of scale
])
def test_parser_takes_transpose_at_the_end_of_the_chain(chain, orient):
    out = parse_image_filter(chain)
    assert out.orient == orient and out.flip is None and out.resize
    assert (out.fit_w, out.fit_h) == (48, 64)  # the final-spec form: the pair swapped
    if chain.startswith("crop="):
        assert out.src_crop == (4, 4, 32, 32)  # (the stored frame's coordinates: not swapped)


def test_parser_swaps_every_pair():
    out = parse_image_filter(SCALE + ":force_original_aspect_ratio=decrease," + PAD +
                             ",crop=w=72:h=60,transpose=clock")
    assert (out.fit_w, out.fit_h, out.pad_w, out.pad_h, out.crop_w, out.crop_h) == \
        (48, 64, 70, 80, 60, 72)
    assert out.orient == 5 and out.aspect == "decrease"
    # a flip alone swaps nothing
    out = parse_image_filter(SCALE + "," + PAD + ",hflip")
    assert (out.fit_w, out.fit_h, out.pad_w, out.pad_h) == (64, 48, 80, 70) and out.orient is None


@pytest.mark.parametrize("tail, orient, flip", [
    ("transpose=clock,hflip", 5 ^ 1, None),          # a flip of the turned image toggles its bit
    ("transpose=clock,vflip", 5 ^ 2, None),
    ("hflip,transpose=cclock_flip", 6, None),        # H then T: T then V
    ("vflip,transpose=cclock_flip", 5, None),
    ("hflip,transpose=clock,vflip", 5, None),        # T(H C) = V T C; then H, then V again: H T C
    ("transpose=clock,transpose=clock", None, 3),    # two quarter turns: 180 degrees, a flip
    ("transpose=clock,transpose=cclock", None, None),
    ("transpose=cclock_flip,transpose=cclock_flip", None, None),
    ("transpose=clock,transpose=clock,transpose=clock", 6, None),
])
def test_transpose_composes_with_flips_in_chain_order(tail, orient, flip):
    out = parse_image_filter(SCALE + "," + tail)
    assert (out.orient, out.flip) == (orient, flip)
    assert (out.fit_w, out.fit_h) == ((48, 64) if orient is not None else (64, 48))
    # ... which is what the nodes do to an image, one after the other
    a, want = np.arange(5 * 7).reshape(5, 7), np.arange(5 * 7).reshape(5, 7)
    for node in tail.split(","):
        code = {"hflip": 1, "vflip": 2}.get(node) or _lib._orient(node.partition("=")[2])
        want = _oriented(want, code)
    np.testing.assert_array_equal(_oriented(a, (orient or 0) | (flip or 0)), want)


@pytest.mark.parametrize("chain", ["transpose=clock," + SCALE,
                                   "transpose=1," + SCALE + ",format=pix_fmts=rgb24",
                                   "crop=w=32:h=32:x=4:y=4,transpose=clock," + SCALE])
def test_a_transpose_ahead_of_scale_is_refused(chain):
    with pytest.raises(ValueError) as e:
        parse_image_filter(chain)
    msg = str(e.value)
    assert "transpose ahead of scale" in msg and "pixels would differ" in msg
    assert "round differently" in msg


@pytest.mark.parametrize("chain, node", [
    (SCALE + ",transpose=clock," + PAD, "pad"),
    (SCALE + ",transpose=clock,crop=w=32:h=32", "crop"),
    (SCALE + ",transpose=clock,scale=w=32:h=32", "scale"),
    (SCALE + ",transpose=clock,transpose=cclock,crop=w=32:h=32", "crop"),
])
def test_a_transpose_between_scale_and_a_later_node_is_refused(chain, node):
    with pytest.raises(ValueError) as e:
        parse_image_filter(chain)
    msg = str(e.value)
    assert f"transpose ahead of {node}" in msg and "pixels would differ" in msg


def test_other_transpose_refusals():
    with pytest.raises(ValueError, match="passthrough"):
        parse_image_filter(SCALE + ",transpose=dir=clock:passthrough=portrait")
    with pytest.raises(ValueError, match="transpose takes dir="):
        parse_image_filter(SCALE + ",transpose=4")
    with pytest.raises(ValueError, match="transpose takes dir="):
        parse_image_filter(SCALE + ",transpose=sideways")
    with pytest.raises(ValueError, match="planar format"):
        parse_image_filter(SCALE + ",transpose=clock", default_pix_fmt=None)
    # a pair of transposes that cancels leaves the planar chain be; so does a flip
    assert parse_image_filter(SCALE + ",transpose=clock,transpose=cclock",
                              default_pix_fmt=None).pix_fmt == "yuv"
    with pytest.raises(ValueError):
        parse_image_filter("transpose=clock")


# ---- the sweeps, under sanitizers ---------------------------------------------------------------

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
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-DHJ_HD=", *san,
                    os.path.join(ROOT, "tests", "native", name + ".cpp"), *sources, "-o", exe],
                   check=True)
    return exe


def test_orient_sweep_under_sanitizers(tmp_path):
    exe = _sanitized(tmp_path, "orient_sweep",
                     [os.path.join(CSRC, "hj_layout.cpp"), os.path.join(CSRC, "hj_sws.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert not r.stderr, r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and lines[1] == "planner: rules hold"
    m = re.fullmatch(r"tiles: (\d+) boxes, (\d+) pixels", lines[0])
    # 70 x 70 sizes x 3 chunks x 4 bands x 8 codes
    assert m and int(m.group(1)) == 70 * 70 * 3 * 4 * 8
    # sides of 32768 and 65535 x 1 and 17, both ways, 2 chunks x 2 bands x 8 codes
    m = re.fullmatch(r"extreme tiles: (\d+) boxes, (\d+) pixels", lines[2])
    assert m and int(m.group(1)) == 2 * 2 * 2 * 2 * 2 * 8


def test_orient_sweep_sees_the_library_through_host_headers_alone():
    with open(os.path.join(ROOT, "tests", "native", "orient_sweep.cpp")) as f:
        src = f.read()
    assert re.findall(r'#\s*include\s*"([^"]+)"', src) == ["../../spdl_amd/csrc/hj_layout.h",
                                                           "../../spdl_amd/csrc/hj_sws_tile.h"]
    assert not re.search(r'#\s*include\s*[<"]hip/', src)


def test_exif_sweep_under_sanitizers(tmp_path, base_jpeg):
    exe = _sanitized(tmp_path, "exif_sweep", [os.path.join(CSRC, "hj_probe.cpp")])
    args = []
    for name, payloads, want in ec.cases():
        data, lo, hi = ec.with_app1(base_jpeg, payloads)
        path = tmp_path / (name + ".jpg")
        path.write_bytes(data)
        args.append(f"{path}:{want}:{lo}:{hi}")
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert not r.stderr, r.stderr
    lines = r.stdout.splitlines()
    m = re.fullmatch(r"exif: (\d+) files, (\d+) buffers", lines[0])
    assert lines[-1] == "ok" and m and int(m.group(1)) == len(args)
    assert int(m.group(2)) > 255 * 20 * len(args)  # (every APP1 byte, every other value)
