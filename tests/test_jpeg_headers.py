"""CPU tests of the header-structure cases (tests/jpeg_header_cases.py): the
segment editor, the oracle against libjpeg 9 and Pillow on every legal layout,
the host probe against the oracle on every case, the refused rows' statuses
and their coverage of the device parser's refusals, and the sanitised native
sweep (tests/native/header_sweep.cpp) over the whole table and a mutation
sweep of every legal header."""

import ctypes
import io
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import jpeg_header_cases as hc
from tests import jpeg_headers as jh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LEGAL = hc.names(legal=True)
REFUSED = hc.names(legal=False)
# what libjpeg and Pillow are asked about: every legal layout but the files
# cut short (libjpeg decodes what is there; only the oracle says what that is)
# and the rows that say libjpeg refuses them (two SOF segments)
INDEPENDENT = [n for n in LEGAL if hc.case(n).family != "truncated"]
FOUR_COMPONENT = ("ycck", "pcycck")


@pytest.fixture(scope="module")
def decoded(oracle):
    """name -> (status, (coefs, levels), rgb) from the oracle, computed once."""
    memo = {}

    def get(key, data):
        if key not in memo:
            try:
                memo[key] = (0, oracle.decode_coefs(data), oracle.decode_rgb(data))
            except oracle.OracleError as e:
                memo[key] = (e.code, None, None)
        return memo[key]
    return get


def _probe(data):
    from spdl_amd import _lib

    info = _lib.ImageInfo()
    addr, size, keep = _lib.buffer_address(data)
    rc = _lib.lib().spdl_hj_get_image_info(addr, size, ctypes.byref(info))
    del keep
    return rc, info


# ---- the editor -------------------------------------------------------------

@pytest.mark.parametrize("src", hc.SOURCES)
def test_split_join_round_trip(src):
    d = hc.source(src)
    segs, tail = jh.split(d)
    assert segs[-1][0] == jh.SOS and jh.join(segs, tail) == d
    items = jh.split_tail(tail)
    assert jh.serialise(items) == tail and items[-1] == (jh.EOI, None)
    nscans = 1 + sum(m == jh.SOS for m, _ in items)
    assert (nscans > 1) == (src in hc.MULTISCAN)
    # fill bytes are transparent to split
    assert jh.split(jh.join(segs, tail, fill=3)) == (segs, tail)


def test_window_streams_cover_every_header_byte():
    """Offset 4096 falls on every byte from the APP14 marker to the first scan
    byte, once each; the nh streams have every size % 16."""
    d = hc.source("win")
    segs, tail = jh.split(d)
    assert [m for m, _ in segs] == [jh.APP14, jh.DQT, jh.DQT, jh.SOF0] + [jh.DHT] * 4 + [jh.DRI, jh.SOS]
    assert segs[1][1][0] == 0x10 and segs[2][1][0] == 0x01  # a 16-bit and an 8-bit table
    hit = set()
    for name, data in hc.window_streams():
        s2, t2 = jh.split(data)
        assert s2[0][0] == jh.COM and s2[1:] == segs and t2 == tail
        hit.add(4096 - (2 + 4 + len(s2[0][1])))
    assert hit == set(range(len(jh.serialise(segs)) + 3))
    sizes = {len(data) % 16 for _, data in hc.nh_streams()}
    assert sizes == set(range(16))


# ---- legal layouts ----------------------------------------------------------

@pytest.mark.parametrize("name", LEGAL)
def test_legal_case_class(decoded, name):
    """same: the source's levels, coefficients and RGB exactly; ok: a decode
    that differs from the source's; `other` (the stream in which the wrong
    table wins) decodes to something else, or not at all."""
    c = hc.case(name)
    st, dec, rgb = decoded(name, c.data)
    sst, sdec, srgb = decoded("source:" + c.source, hc.source(c.source))
    assert sst == 0
    assert st == 0, st
    if c.expect == "oracle":  # (a missing EOI, bytes behind it: the oracle decodes what is there)
        return
    same = (all(np.array_equal(a, b) for a, b in zip(dec[1], sdec[1])) and
            (c.reordered or np.array_equal(dec[0], sdec[0])) and np.array_equal(rgb, srgb))
    assert same == (c.expect == "same")
    if c.other is not None:
        ost, odec, orgb = decoded("other:" + name, c.other)
        assert ost != 0 or not (np.array_equal(odec[0], dec[0]) and np.array_equal(orgb, rgb))


@pytest.mark.parametrize("name", [n for n in INDEPENDENT if hc.case(n).libjpeg])
def test_levels_match_libjpeg(oracle, decoded, name):
    """libjpeg 9's jpeg_read_coefficients returns the oracle's levels (its
    warnings -- garbage between segments, a missing EOI -- are not fatal)."""
    if oracle.ljpin() is None:
        pytest.skip("libjpeg 9 not available on this host")
    c = hc.case(name)
    st, dec, _ = decoded(name, c.data)
    assert st == 0
    got = oracle.lj_read_coefs(c.data)
    assert len(got) == len(dec[1])
    for g, w in zip(got, dec[1]):
        np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("name", [n for n in INDEPENDENT if hc.case(n).pillow
                                  and hc.case(n).source not in FOUR_COMPONENT])
def test_luma_matches_pillow(oracle, name):
    """Pillow's luma is within 1 level of the oracle's islow luma plane (the
    bound of test_jpeg_writer: Pillow's YCbCr round trip): a quantiser table
    taken from the wrong definition moves it further."""
    from PIL import Image

    c = hc.case(name)
    info = oracle.parse(c.data)
    im = Image.open(io.BytesIO(c.data))
    assert im.size == (info.width, info.height)
    if info.ncomp == 1:
        assert im.mode == "L"
        luma = np.asarray(im).astype(int)
    else:
        assert im.mode == "RGB"
        im.draft("YCbCr", im.size)
        luma = np.asarray(im.convert("YCbCr"))[..., 0].astype(int)
    ref = oracle.decode_planes(c.data, oracle.IDCT_ISLOW)[0].astype(int)
    assert luma.shape == ref.shape
    assert np.abs(luma - ref).max() <= 1


def test_wrong_quantiser_table_moves_pillow_luma(oracle):
    """The check above can see a wrong table: against the oracle's decode of
    the stream in which the other definition wins, Pillow is further than 1."""
    from PIL import Image

    c = hc.case("redef_dqt_later_wins_q90_420")
    im = Image.open(io.BytesIO(c.data))
    im.draft("YCbCr", im.size)
    luma = np.asarray(im.convert("YCbCr"))[..., 0].astype(int)
    wrong = oracle.decode_planes(c.other, oracle.IDCT_ISLOW)[0].astype(int)
    assert np.abs(luma - wrong).max() > 1


# ---- refused headers --------------------------------------------------------

@pytest.mark.parametrize("name", REFUSED)
def test_refused_status(oracle, name):
    """The status the row lists, from the oracle: from the parse where the
    header is at fault, else from the decode."""
    c = hc.case(name)
    with pytest.raises(oracle.OracleError) as e:
        oracle.decode_rgb(c.data)
    assert e.value.code == c.expect
    rs = oracle.Resize(fit_w=32, fit_h=32, aspect="decrease", pad_w=32, pad_h=32)
    with pytest.raises(oracle.OracleError) as e:
        oracle.decode_resize(c.data, rs, "rgb24")
    assert e.value.code == c.expect


def _conditions(text, start, end, stmt):
    """The conditions of the `if`s whose statement begins with `stmt`, in
    the source between two anchors, whitespace collapsed."""
    body = " ".join(text[text.index(start):text.index(end, text.index(start))].split())
    out = []
    for m in re.finditer(re.escape(stmt), body):
        j = m.start() - 1
        while body[j] in " {":
            j -= 1
        assert body[j] == ")", body[max(0, j - 60):m.end()]
        depth, i = 0, j
        while True:
            depth += (body[i] == ")") - (body[i] == "(")
            if depth == 0:
                break
            i -= 1
        assert body[i - 3:i] == "if ", body[max(0, i - 20):m.end()]
        out.append(body[i + 1:j])
    return out


def test_every_refusal_of_the_device_parser_has_a_row():
    """Every `return kErr...` of parse_headers and every `err = kErr...` of
    multiscan_kernel's marker walk is the key of a refused row (or is listed
    with the place that pins it)."""
    with open(os.path.join(ROOT, "spdl_amd", "csrc", "hj_kernels.hip")) as f:
        text = f.read()
    keys = {hc.case(n).key for n in REFUSED} | set(hc.ELSEWHERE)
    parse = _conditions(text, "__device__ static int parse_headers(", "__global__ void", "return kErr")
    assert len(parse) >= 30
    walk = _conditions(text, "// ---- thread 0: sort the candidates, walk the segments",
                       "S.nscans = ns;", "err = kErr")
    assert len(walk) >= 8
    missing = [c for c in parse if c not in keys] + [c for c in walk if "ms: " + c not in keys]
    assert not missing, missing


# ---- the probe against the oracle -------------------------------------------

@pytest.mark.parametrize("family", sorted({hc.case(n).family for n in hc.table()}))
def test_probe_agrees_with_the_oracle(oracle, family):
    """Every case of the family: the probe and oracle.parse return one status;
    where the fault lies in what the probe does not read (a table, the scan
    header, anything behind the SOF -- the row's `probe` is 0) the probe
    accepts and the status comes from the oracle.  Ahead of a complete SOF the
    probe returns NOT_JPEG, BAD_HEADER or UNSUPPORTED only.  On success the
    frames are equal."""
    for name in hc.names(family=family):
        c = hc.case(name)
        rc, pi = _probe(c.data)
        try:
            oi = oracle.parse(c.data)
            orc = 0
        except oracle.OracleError as e:
            orc = e.code
        legal = not isinstance(c.expect, int)
        want = 0 if legal else c.probe
        assert rc == want, (name, rc, want)
        assert rc in (0, hc.NOT_JPEG, hc.UNSUPPORTED, hc.BAD_HEADER), name
        if rc:
            assert orc == rc, (name, orc, rc)
        if orc == 0:
            assert rc == 0, name
            assert (pi.width, pi.height, pi.ncomp, pi.color) == (oi.width, oi.height, oi.ncomp,
                                                                  oi.color), name
            assert bool(pi.multiscan) == bool(oi.multiscan), name
            for k in range(oi.ncomp):
                assert (pi.h_samp[k], pi.v_samp[k]) == (oi.comp_h[k], oi.comp_v[k]), name


def test_two_sofs_the_last_is_the_frame(oracle):
    """The probe keeps the last SOF before the first SOS, as the oracle and
    the device parser do: 24x16 4:2:0 behind a SOF that claims 16x16 4:4:4."""
    for name in hc.names(family="two_sofs"):
        rc, pi = _probe(hc.case(name).data)
        assert rc == 0 and (pi.width, pi.height) == (24, 16)
        assert [pi.h_samp[k] for k in range(3)] == [2, 1, 1]
        assert oracle.decode_rgb(hc.case(name).data).shape == (16, 24, 3)


# ---- the sanitised native sweep ---------------------------------------------

_INTERPRETED = (jh.DQT, jh.DHT, jh.DRI, jh.SOS, jh.APP14) + jh.SOFS + (0xC3, 0xC9)


def header_ranges(data: bytes):
    """[first, end) byte ranges of a legal stream's header that a marker walk
    interprets: SOI, every marker and length, the payloads of tables, frame
    and scan headers and APP14, and the first 16 payload bytes of the segments
    skipped by length (fill bytes and garbage between segments included)."""
    out, pos = [(0, 2)], 2
    while True:
        start = pos
        while data[pos] != 0xFF or data[pos + 1] == 0xFF:
            pos += 1
        m = data[pos + 1]
        if m == jh.TEM or 0xD0 <= m <= 0xD7:
            pos += 2
            out.append((start, pos))
            continue
        n = int.from_bytes(data[pos + 2:pos + 4], "big")
        stop = pos + 2 + n
        out.append((start, stop if m in _INTERPRETED else min(stop, pos + 4 + 16)))
        pos = stop
        if m == jh.SOS:
            return out


def write_corpus(path):
    """The whole case table, the window streams and the nh streams; mutation
    ranges for the legal named cases (not for the window sweep, which is one
    header shifted) -- headers already in the corpus are not swept twice."""
    streams, seen = [], set()
    for name in hc.table():
        c = hc.case(name)
        legal = not isinstance(c.expect, int)
        ranges = []
        if legal and c.family not in ("truncated", "ends"):
            ranges = header_ranges(c.data)
            key = b"".join(c.data[a:b] for a, b in ranges)
            if key in seen:
                ranges = []
            seen.add(key)
        want = 0 if c.expect in ("same", "ok") else -1 if legal else c.expect
        streams.append((c.data, want, 0 if legal else c.probe, ranges))
    for _, d in (*hc.window_streams(), *hc.nh_streams()):
        streams.append((d, 0, 0, []))
    with open(path, "wb") as f:
        f.write(b"HSW1" + struct.pack("<I", len(streams)))
        for d, wo, wp, ranges in streams:
            f.write(struct.pack("<IiiI", len(d), wo, wp, len(ranges)))
            for a, b in ranges:
                f.write(struct.pack("<II", a, b))
            f.write(d)
    return len(streams)


def test_header_sweep_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    cc = shutil.which("gcc") or shutil.which("cc")
    if cxx is None or cc is None:
        pytest.skip("no host C / C++ compiler")
    # (runtimes linked statically: the program then runs whatever the environment preloads)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    static = ["-static-libasan", "-static-libubsan"]
    probe_src = tmp_path / "probe.cpp"
    probe_src.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, *san, *static, str(probe_src), "-o", str(tmp_path / "probe")],
                      capture_output=True).returncode:
        pytest.skip("the compiler has no sanitizer runtime")
    objs = []
    for src in ("jpeg_oracle.c", "sws_oracle.c"):
        objs.append(str(tmp_path / (src[:-2] + ".o")))
        subprocess.run([cc, "-O1", "-g", "-ffp-contract=off", *san, "-c",
                        os.path.join(ROOT, "oracle", src), "-o", objs[-1]], check=True)
    exe = str(tmp_path / "header_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-DHJ_HD=", *san, *static,
                    os.path.join(ROOT, "tests", "native", "header_sweep.cpp"),
                    os.path.join(ROOT, "spdl_amd", "csrc", "hj_probe.cpp"), *objs,
                    "-lpthread", "-lm", "-o", exe], check=True)
    corpus = str(tmp_path / "corpus.bin")
    n = write_corpus(corpus)
    r = subprocess.run([exe, corpus], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("streams ") and not r.stderr, r.stdout + r.stderr
    print(r.stdout.strip())
    w = r.stdout.split()
    streams, mutants = int(w[1]), int(w[7])
    assert streams == n == len(hc.table()) + len(hc.window_streams()) + len(hc.nh_streams())
    assert mutants > 100 * len(LEGAL)
    # some mutants still decode (a table value, a comment byte), most do not
    assert 0 < int(w[9]) < mutants and int(w[9]) <= int(w[11])
