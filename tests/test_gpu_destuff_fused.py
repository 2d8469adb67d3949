"""destuff_image_kernel (one launch, one workgroup per image, tiles of 512
groups of 16 bytes) against the count / prefix / write kernels and the
oracle: every batch is decoded with "destuff_fused_bytes" forced high (fused)
and at 0 (three kernels); the outputs are compared with the oracle's and with
each other, the destuffed bytes and the segment count with the scan destuffed
here byte by byte, at 1 and 4 lanes.

Streams (tests/destuff_cases.py, tests/jpeg_writer.py): a tile is 8192 bytes
from scan_start & ~15.
  sized      a restart-every-block scan stretched by fill 0xFFs in front of its
             RSTn markers to exactly L scan bytes, L = tile - 16, tile - 1, tile,
             tile + 1, 2 tiles - 1, 2 tiles, 2 tiles + 1, each at every
             scan_start % 16: the scan's end with its FF D9 takes all 16 byte
             positions on both sides of a tile boundary
  one_byte   a scan of one byte
  swept      destuff_cases' stuffed / rst_every_block / rst_fill and plain_rst (a
             second restart-every-block scan), each at every scan_start % 16,
             and all_ones (a scan that is all FF 00 pairs, one
             tile and 128 bytes: the output is half the input); long_ones, the
             same over two tiles and a half
  fill_00    a sized stream with FF FF .. FF 00 written over it: a fill run that
             ends in 0x00 ends the scan at its first 0xFF.  The run starts at
             each of the 16 positions before and after the first tile boundary,
             short (inside a group or over the boundary by its last bytes) and
             18 bytes long (over a whole group and the boundary).  Not a
             decodable stream: the paths are compared with each other and with
             a byte loop -- status, clean_len, nseg, the clean bytes, the output
test_streams_cross_the_tile_boundary (no GPU) asserts that over these streams
a stuffed pair, a plain RSTn, a fill run and the scan's end each begin at all
32 positions around a tile boundary.
"""

import functools

import numpy as np
import pytest
import torch

from spdl_amd._lib import Output
from tests import cases
from tests import destuff_cases as dc
from tests import jpeg_writer as jw
from tests import jpeg_writer_cases as hw
from tests.test_gpu_destuff import destuffed

gpu = pytest.mark.gpu

TILE = 8192
RESIZE32 = dict(fit_w=32, fit_h=32, aspect="decrease", pad_w=32, pad_h=32)
# (label, "destuff_fused_bytes")
PATHS = (("fused", 1 << 30), ("three", 0))
AROUND = set(range(-16, 16))  # byte positions against a tile boundary


@functools.lru_cache(maxsize=None)
def _base(two_tiles: bool) -> hw.Stream:
    """A restart-every-block gray stream a little under one / two tiles."""
    side = 208 if two_tiles else 144
    return dc._gray(f"fused_base_{side}", side, side, 31, restart_interval=1)


def sized(base: bytes, length: int) -> bytes:
    """`base` with fill 0xFFs spread over its RSTn markers: a scan of exactly `length` bytes."""
    a, b = dc.scan_extent(base)
    marks = [j for j in range(a, b - 1)
             if base[j] == 0xFF and 0xD0 <= base[j + 1] <= 0xD7 and base[j - 1] != 0xFF]
    extra = length - (b - a)
    assert 0 <= extra and len(marks) > 64, (extra, len(marks))
    each, rest = divmod(extra, len(marks))
    out, p = bytearray(base[:a]), a
    for i, j in enumerate(marks):
        out += base[p:j] + b"\xff" * (each + (i < rest))
        p = j
    out += base[p:]
    a2, b2 = dc.scan_extent(bytes(out))
    assert b2 - a2 == length
    return bytes(out)


LENGTHS = (TILE - 16, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1)


@functools.lru_cache(maxsize=None)
def sized_batch(length: int):
    base = _base(length > TILE + 1).data
    s = sized(base, length)
    return base, [dc.aligned(s, k) for k in range(16)]


@functools.lru_cache(maxsize=None)
def one_byte() -> hw.Stream:
    lv = np.zeros((1, 1, 64), np.int32)
    s = hw._write("one_byte", 8, 8, [(1, 1)], [lv], {0: np.full(64, 4)}, [0], jw.std_tables(),
                  [0], [0])
    a, b = dc.scan_extent(s.data)
    assert b - a == 1, b - a
    return s


@functools.lru_cache(maxsize=None)
def long_ones() -> hw.Stream:
    """destuff_cases' all_ones over two tiles and a half: 320 x 128 blocks, two
    1-bits each, every scan byte 0xFF and stuffed."""
    lv = np.zeros((128, 320, 64), np.int32)
    s = hw._write("long_ones", 2560, 1024, [(1, 1)], [lv], {0: np.full(64, 4)}, [0],
                  jw.short_table(inverted=True), [0], [0])
    a, b = dc.scan_extent(s.data)
    assert 2 * TILE + 1024 < b - a < 3 * TILE and s.data[a:b] == b"\xff\x00" * ((b - a) // 2)
    return s


@functools.lru_cache(maxsize=None)
def plain_rst() -> hw.Stream:
    """A second restart-every-block scan a little over one tile: with
    destuff_cases' rst_every_block, a plain RSTn at every position around the
    boundary."""
    s = dc._gray("fused_plain_rst", 192, 192, 47, restart_interval=1)
    a, b = dc.scan_extent(s.data)
    assert TILE + 16 <= b - a < 2 * TILE
    return s


def _swept(name: str) -> bytes:
    return {"long_ones": long_ones, "plain_rst": plain_rst}[name]().data if name in (
        "long_ones", "plain_rst") else dc.case(name).data


# ---- fill runs that end in 0x00 ---------------------------------------------------------

FILL_00 = [(side, run) for side in (-16, 0) for run in (4, 18) if (side, run) != (0, 18)]


def fill_00(k: int, side: int, run: int) -> tuple[bytes, int]:
    """The 2 TILE + 1 sized stream at scan_start % 16 == k with `run` 0xFFs and a
    0x00 written at tile boundary + side + k (no 0xFF before them); the file and
    the position of the run's first byte."""
    d = bytearray(sized_batch(2 * TILE + 1)[1][k])
    a, _ = dc.scan_extent(bytes(d))
    pos = (a & ~15) + TILE + side + k
    j = pos - 1
    d[j] = 0x55
    while d[j - 1] == 0xFF:  # an 0xFF run that led up to the byte before
        j -= 1
        d[j] = 0x55
    d[pos:pos + run] = b"\xff" * run
    d[pos + run] = 0x00
    return bytes(d), pos


def destuffed_to_terminator(data: bytes):
    """(data bytes, restart segments, scan end) of a one-scan file whose scan
    ends at the first 0xFF run that neither a 0x00 alone nor an RSTn follows."""
    a, _ = dc.scan_extent(data)
    out, nseg, j = bytearray(), 1, a
    while j < len(data):
        if data[j] != 0xFF:
            out.append(data[j])
            j += 1
        elif j + 1 < len(data) and data[j + 1] == 0x00:
            out.append(0xFF)
            j += 2
        else:
            k = j + 1
            while k < len(data) and data[k] == 0xFF:
                k += 1
            if k < len(data) and 0xD0 <= data[k] <= 0xD7:
                nseg += 1
                j = k + 1
            else:
                break
    return bytes(out), nseg, j


# ---- the streams reach the boundaries (no GPU) -----------------------------------------

def _against_boundary(data: bytes, j: int) -> int:
    """File byte j against the nearest tile boundary of its scan: -TILE/2 .. TILE/2 - 1."""
    a, _ = dc.scan_extent(data)
    return (j - (a & ~15) + TILE // 2) % TILE - TILE // 2


def _gpu_streams():
    """Every one-scan file the GPU tests below decode (the fill_00 files apart)."""
    for length in LENGTHS:
        yield from sized_batch(length)[1]
    for name in ("stuffed", "rst_every_block", "rst_fill", "plain_rst"):
        yield from (dc.aligned(_swept(name), k) for k in range(16))
    yield from (dc.aligned(dc.case("all_ones").data, k) for k in (0, 1, 15))
    yield from (dc.aligned(long_ones().data, k) for k in (0, 1))


def test_streams_cross_the_tile_boundary():
    for length in LENGTHS:
        base, datas = sized_batch(length)
        assert dc.scan_extent(base)[1] - dc.scan_extent(base)[0] < length
        for k, d in enumerate(datas):
            a, b = dc.scan_extent(d)
            assert b - a == length and a % 16 == k
    hit = {"pair": set(), "rst": set(), "fill": set(), "end": set()}
    for d in _gpu_streams():
        a, b = dc.scan_extent(d)
        hit["end"].add(_against_boundary(d, b))
        j = a
        while j < b:
            if d[j] != 0xFF:
                j += 1
                continue
            k = j
            while d[k] == 0xFF:
                k += 1
            n, after = k - j, d[k]
            if j - (a & ~15) >= TILE // 2:  # (boundary 0 is the scan's start)
                kind = "pair" if (n, after) == (1, 0) else "rst" if n == 1 else "fill"
                hit[kind].add(_against_boundary(d, j))
            j = k + 1
    for kind, at in hit.items():
        assert AROUND <= at, (kind, sorted(AROUND - at))
    # the fill runs that end in 0x00: the scan ends at the run's first byte, at every position
    starts = set()
    for side, run in FILL_00:
        for k in range(16):
            d, pos = fill_00(k, side, run)
            out, nseg, end = destuffed_to_terminator(d)
            assert end == pos and d[pos:pos + run + 1] == b"\xff" * run + b"\x00" and nseg > 100
            assert _against_boundary(d, pos) == side + k
            starts.add((run, side + k))
    assert {(4, p) for p in AROUND} | {(18, p) for p in range(-16, 0)} == starts


# ---- GPU ------------------------------------------------------------------------------

def _decode(dec, datas, out: Output, shape, check=True):
    t = torch.empty((len(datas),) + tuple(shape), dtype=torch.uint8, device="cuda:0")
    st = dec.decode_batch(datas, out, t.data_ptr(), t.numel(), stream=torch.cuda.current_stream(),
                          check=check)
    if check:
        assert not any(st), st
        return t.cpu().numpy()
    return st, t.cpu().numpy()


class _Path:
    """The decoder with a "destuff_fused_bytes" (and a lane count) for a with-block."""

    def __init__(self, dec, threshold, lanes=None):
        self.dec, self.threshold, self.lanes = dec, threshold, lanes

    def __enter__(self):
        d = self.dec
        self.prev = {k: d.get_param(k) for k in ("destuff_fused_bytes", "lanes")}
        d.set_param("destuff_fused_bytes", self.threshold)
        if self.lanes:
            d.set_param("lanes", self.lanes)
        return d

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            self.dec.set_param(k, v)


def _both_paths(dec, datas, out, shape):
    """The batch on either path: the outputs, equal."""
    hyps = {}
    for name, threshold in PATHS:
        with _Path(dec, threshold) as d:
            hyps[name] = _decode(d, datas, out, shape)
            assert d.get_param("destuff_fused") == int(threshold > 0), name
    np.testing.assert_array_equal(hyps["fused"], hyps["three"], strict=True)
    return hyps["fused"]


def _check_destuffed(dec, oracle, d):
    """debug_entropy on either path: the destuffed bytes, the segments, the coefficients."""
    ref, _ = oracle.decode_coefs(d)
    want, nseg = destuffed(d)
    for name, threshold in PATHS:
        with _Path(dec, threshold) as dd:
            hyp, clean, diag = dd.debug_entropy(d, ref.shape[0])
        assert diag["status"] == 0, (name, diag)
        assert diag["clean_len"] == len(want) and diag["nseg"] == nseg, (name, diag, len(want), nseg)
        np.testing.assert_array_equal(clean, np.frombuffer(want, np.uint8), err_msg=name)
        np.testing.assert_array_equal(hyp, ref, strict=True, err_msg=name)


@gpu
@pytest.mark.parametrize("length", LENGTHS)
def test_scan_lengths_around_the_tiles(decoder, oracle, length):
    base, datas = sized_batch(length)
    ref = oracle.decode_rgb(base, oracle.IDCT_SIMPLE, "rgb24")
    np.testing.assert_array_equal(oracle.decode_rgb(datas[5], oracle.IDCT_SIMPLE, "rgb24"), ref)
    hyp = _both_paths(decoder, datas, Output(pix_fmt="rgb24"), ref.shape)
    for k in range(16):
        np.testing.assert_array_equal(hyp[k], ref, strict=True, err_msg=f"scan_start % 16 = {k}")
    for k in (0, 7, 15):
        _check_destuffed(decoder, oracle, datas[k])


@gpu
def test_one_byte_scan(decoder, oracle):
    d = one_byte().data
    ref = oracle.decode_rgb(d, oracle.IDCT_SIMPLE, "rgb24")
    datas = [dc.aligned(d, k) for k in (0, 1, 15)]
    hyp = _both_paths(decoder, datas, Output(pix_fmt="rgb24"), ref.shape)
    for h in hyp:
        np.testing.assert_array_equal(h, ref, strict=True)
    _check_destuffed(decoder, oracle, datas[2])


@gpu
@pytest.mark.parametrize("name", dc.NAMES + ("long_ones", "plain_rst"))
def test_swept_streams_on_either_path(decoder, oracle, name):
    """Stuffed pairs, RSTn and fill runs at every alignment, and the scans of
    FF 00 pairs alone (all_ones: one tile and 128 bytes; long_ones: two tiles
    and a half; the output half the input)."""
    base = _swept(name)
    ref = oracle.decode_rgb(base, oracle.IDCT_SIMPLE, "rgb24")
    ks = {"all_ones": (0, 1, 15), "long_ones": (0, 1)}.get(name, range(16))
    datas = [dc.aligned(base, k) for k in ks]
    hyp = _both_paths(decoder, datas, Output(pix_fmt="rgb24"), ref.shape)
    for k, h in enumerate(hyp):
        np.testing.assert_array_equal(h, ref, strict=True, err_msg=f"image {k}")
    _check_destuffed(decoder, oracle, datas[1])


@gpu
@pytest.mark.parametrize("side,run", FILL_00)
def test_fill_run_ending_in_00(decoder, side, run):
    """FF FF .. FF 00 starting at each of the 16 positions before (side -16)
    or after (0) the first tile boundary: the scan ends at the run's first
    byte.  Either path against the byte loop (clean_len, nseg, the clean
    bytes) and against the other (those, the status, the decoded batch)."""
    stream = _base(True)
    nblocks = ((stream.width + 7) // 8) * ((stream.height + 7) // 8)
    datas = [fill_00(k, side, run)[0] for k in range(16)]
    got = {}
    for name, threshold in PATHS:
        with _Path(decoder, threshold) as d:
            st, px = _decode(d, datas, Output(pix_fmt="rgb24"),
                             (stream.height, stream.width, 3), check=False)
            assert d.get_param("destuff_fused") == int(threshold > 0)
            dbg = [d.debug_entropy(x, nblocks) for x in datas]
        got[name] = (st, px, dbg)
        for k, (coefs, clean, diag) in enumerate(dbg):
            want, nseg, _ = destuffed_to_terminator(datas[k])
            assert diag["clean_len"] == len(want) and diag["nseg"] == nseg, (name, k, diag)
            np.testing.assert_array_equal(clean, np.frombuffer(want, np.uint8),
                                          err_msg=f"{name} {k}")
    (st_f, px_f, dbg_f), (st_t, px_t, dbg_t) = got["fused"], got["three"]
    assert list(st_f) == list(st_t), (st_f, st_t)
    np.testing.assert_array_equal(px_f, px_t, strict=True)
    for k in range(16):
        assert dbg_f[k][2]["status"] == dbg_t[k][2]["status"], k
        np.testing.assert_array_equal(dbg_f[k][0], dbg_t[k][0], strict=True, err_msg=f"coefs {k}")


@functools.lru_cache(maxsize=None)
def _mixed():
    datas = [cases.case("bench_1000"), dc.aligned(dc.case("stuffed").data, 5),
             sized_batch(TILE + 1)[1][3], dc.case("all_ones").data,
             dc.aligned(dc.case("rst_fill").data, 9), cases.case("bench_1001")]
    return datas


@gpu
@pytest.mark.parametrize("lanes", [1, 4])
def test_one_image_above_the_threshold(decoder, oracle, lanes):
    """A threshold between the batch's file sizes: the one larger image sends
    the whole batch through the three kernels; above all of them the batch is
    fused.  Four batches in a row, so that at four lanes every lane takes one."""
    datas = _mixed()
    sizes = sorted(len(d) for d in datas)
    assert sizes[-2] < sizes[-1]
    refs = [oracle.decode_resize(d, oracle.Resize(**RESIZE32), pix_fmt="rgb24") for d in datas]
    out = Output(pix_fmt="rgb24", resize=True, **RESIZE32)
    for threshold, fused in ((sizes[-1] - 1, 0), (sizes[-1], 1)):
        with _Path(decoder, threshold, lanes) as d:
            for _ in range(4):
                hyp = _decode(d, datas, out, (32, 32, 3))
                assert d.get_param("destuff_fused") == fused
                for i, r in enumerate(refs):
                    np.testing.assert_array_equal(hyp[i], r, strict=True, err_msg=f"image {i}")


@gpu
@pytest.mark.parametrize("lanes", [1, 4])
def test_batch_with_a_progressive_image(decoder, oracle, lanes):
    """The multi-scan image is left to multiscan_kernel on either path."""
    datas = [cases.case("bench_1000"), cases.case("prog_420"),
             dc.aligned(dc.case("stuffed").data, 15), cases.case("bench_1002")]
    refs = [oracle.decode_resize(d, oracle.Resize(**RESIZE32), pix_fmt="rgb24") for d in datas]
    out = Output(pix_fmt="rgb24", resize=True, **RESIZE32)
    for name, threshold in PATHS:
        with _Path(decoder, threshold, lanes) as d:
            for _ in range(2):
                hyp = _decode(d, datas, out, (32, 32, 3))
                for i, r in enumerate(refs):
                    np.testing.assert_array_equal(hyp[i], r, strict=True,
                                                  err_msg=f"{name} image {i}")


@gpu
def test_host_choice(decoder):
    """The threshold is a decoder parameter; 0 selects the three kernels, and
    the path a submission took is reported."""
    assert decoder.get_param("destuff_fused_bytes") > 0
    with pytest.raises(ValueError):
        decoder.set_param("destuff_fused_bytes", -1)
    d = cases.case("bench_1000")
    out = Output(pix_fmt="rgb24", resize=True, **RESIZE32)
    got = {}
    for threshold in (0, len(d) - 1, len(d)):
        with _Path(decoder, threshold) as dec:
            assert dec.get_param("destuff_fused_bytes") == threshold
            got[threshold] = _decode(dec, [d, d], out, (32, 32, 3))
            assert dec.get_param("destuff_fused") == int(threshold == len(d))
    np.testing.assert_array_equal(got[0], got[len(d)], strict=True)
    np.testing.assert_array_equal(got[len(d) - 1], got[len(d)], strict=True)
