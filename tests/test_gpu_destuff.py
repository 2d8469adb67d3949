"""The destuff kernels (count, prefix, write) at their boundaries: the 16-byte
group a thread classifies and compacts in registers, and the 4096-byte chunk a
workgroup stages and copies out.  Streams: tests/destuff_cases.py, scans a
little over two chunks, moved over the boundaries by a COM segment that takes
scan_start % 16 through all 16 values.

Bar: bit-exact vs the oracle (np.testing.assert_array_equal) on the decoded
output, and on Decoder.debug_entropy's coefficients; the destuffed bytes and
the segment count debug_entropy returns are also compared with the scan
destuffed here byte by byte.  A file cut after a lone 0xFF gets the oracle's
status.
"""

import numpy as np
import pytest
import torch

from spdl_amd._lib import Output
from tests import cases
from tests import destuff_cases as dc

gpu = pytest.mark.gpu

RESIZE32 = dict(fit_w=32, fit_h=32, aspect="decrease", pad_w=32, pad_h=32)
SWEPT = ("stuffed", "rst_every_block", "rst_fill")


def destuffed(data: bytes):
    """(the scan's data bytes, restart segments) of a one-scan file."""
    a, b = dc.scan_extent(data)
    out, nseg, j = bytearray(), 1, a
    while j < b:
        if data[j] != 0xFF:
            out.append(data[j])
            j += 1
        elif data[j + 1] == 0x00:
            out.append(0xFF)
            j += 2
        else:
            while data[j + 1] == 0xFF:  # fill
                j += 1
            assert 0xD0 <= data[j + 1] <= 0xD7 and j + 1 < b, (j, data[j + 1])
            nseg += 1
            j += 2
    return bytes(out), nseg


def _ff_runs(data: bytes):
    """(file position of the first 0xFF, run length, the byte after) per run of the scan."""
    a, b = dc.scan_extent(data)
    j = a
    while j < b:
        if data[j] != 0xFF:
            j += 1
            continue
        k = j
        while data[k] == 0xFF:
            k += 1
        yield j, k - j, data[k]
        j = k + 1


# ---- the streams reach the boundaries (no GPU) ---------------------------------------

def test_streams_cross_the_boundaries():
    hit = {n: set() for n in SWEPT}
    for name in SWEPT:
        base = dc.case(name).data
        a, b = dc.scan_extent(base)
        assert 2 * dc.CHUNK + 16 <= b - a <= 2 * dc.CHUNK + 1024, (name, b - a)
        for k in range(16):
            d = dc.aligned(base, k)
            for j, n, after in _ff_runs(d):
                first, last = dc.chunk_pos(d, j), dc.chunk_pos(d, j + n - 1)
                kind = "pair" if after == 0 and n == 1 else "rst" if 0xD0 <= after <= 0xD7 else "?"
                if first == dc.CHUNK - 1:
                    hit[name].add(kind + " | chunk")  # the 0xFF ends a chunk
                if first % 16 == 15:
                    hit[name].add(kind + " | group")
                if n > 1 and first // 16 != last // 16:
                    hit[name].add("fill over groups")
                if n > 1 and first > last:
                    hit[name].add("fill over chunks")
    assert {"pair | chunk", "pair | group"} <= hit["stuffed"], hit
    assert {"rst | chunk", "rst | group"} <= hit["rst_every_block"], hit
    assert {"rst | chunk", "fill over groups", "fill over chunks"} <= hit["rst_fill"], hit
    ones = dc.case("all_ones").data
    a, b = dc.scan_extent(ones)
    assert ones[a:b] == b"\xff\x00" * ((b - a) // 2) and b - a >= 2 * dc.CHUNK + 16
    assert ones.endswith(b"\xff\x00\xff\xd9")


# ---- GPU -----------------------------------------------------------------------------

def _decode(dec, datas, out: Output, shape, check=True):
    t = torch.empty((len(datas),) + tuple(shape), dtype=torch.uint8, device="cuda:0")
    st = dec.decode_batch(datas, out, t.data_ptr(), t.numel(), stream=torch.cuda.current_stream(),
                          check=check)
    return st, t.cpu().numpy()


def check_destuffed(dec, oracle, d):
    """debug_entropy: the destuffed bytes and segment count, and the coefficients."""
    ref, _ = oracle.decode_coefs(d)
    hyp, clean, diag = dec.debug_entropy(d, ref.shape[0])
    assert diag["status"] == 0, diag
    want, nseg = destuffed(d)
    assert diag["clean_len"] == len(want) and diag["nseg"] == nseg, (diag, len(want), nseg)
    np.testing.assert_array_equal(clean, np.frombuffer(want, np.uint8))
    np.testing.assert_array_equal(hyp, ref, strict=True)


@gpu
@pytest.mark.parametrize("name", SWEPT)
def test_every_scan_alignment(decoder, oracle, name):
    """scan_start % 16 = 0..15 in one batch: every stuffed pair, marker and
    fill run of the stream takes every place against the group and chunk
    boundaries."""
    base = dc.case(name).data
    ref = oracle.decode_rgb(base, oracle.IDCT_SIMPLE, "rgb24")
    datas = [dc.aligned(base, k) for k in range(16)]
    np.testing.assert_array_equal(oracle.decode_rgb(datas[7], oracle.IDCT_SIMPLE, "rgb24"), ref)
    st, hyp = _decode(decoder, datas, Output(pix_fmt="rgb24"), ref.shape)
    assert not any(st), st
    for k in range(16):
        np.testing.assert_array_equal(hyp[k], ref, strict=True, err_msg=f"scan_start % 16 = {k}")
    for k in range(16):
        check_destuffed(decoder, oracle, datas[k])


@gpu
def test_all_ones_scan(decoder, oracle):
    """Every scan byte 0xFF and stuffed: eight drops in every group, a pair on
    every boundary at an odd alignment, 0xFF 0x00 directly before EOI."""
    base = dc.case("all_ones").data
    ref = oracle.decode_rgb(base, oracle.IDCT_SIMPLE, "rgb24")
    datas = [dc.aligned(base, k) for k in (0, 1, 15)]
    st, hyp = _decode(decoder, datas, Output(pix_fmt="rgb24"), ref.shape)
    assert not any(st), st
    for h in hyp:
        np.testing.assert_array_equal(h, ref, strict=True)
    for d in datas[:2]:
        check_destuffed(decoder, oracle, d)


def _lone_ff_cuts():
    s = dc.case("stuffed").data
    a, b = dc.scan_extent(s)
    mid = next(j for j, n, after in _ff_runs(s) if j > a + dc.CHUNK + 100 and after == 0)
    ones = dc.case("all_ones").data
    return {"mid_scan": s[:mid + 1], "before_eoi": ones[:-3], "eoi_ff": ones[:-1],
            "rst_ff": _cut_at_rst()}


def _cut_at_rst():
    d = dc.case("rst_every_block").data
    a, _ = dc.scan_extent(d)
    j = next(j for j, n, after in _ff_runs(d) if j > a + dc.CHUNK and 0xD0 <= after <= 0xD7)
    return d[:j + 1]


@gpu
@pytest.mark.parametrize("cut", ["mid_scan", "before_eoi", "eoi_ff", "rst_ff"])
def test_file_cut_after_a_lone_ff(decoder, oracle, cut):
    """The file ends with an 0xFF that nothing follows: the bytes past the
    file read as EOI.  Status (or, where the oracle decodes it, pixels) as the
    oracle gives."""
    d = _lone_ff_cuts()[cut]
    assert d[-1] == 0xFF and d[-2] != 0xFF
    full = dc.case("stuffed" if cut == "mid_scan" else
                   "rst_every_block" if cut == "rst_ff" else "all_ones")
    shape = (full.height, full.width, 3)
    try:
        ref, code = oracle.decode_rgb(d, oracle.IDCT_SIMPLE, "rgb24"), 0
    except oracle.OracleError as e:
        ref, code = None, e.code
    st, hyp = _decode(decoder, [d], Output(pix_fmt="rgb24"), shape, check=False)
    assert st == [code], (cut, st, code)
    if ref is not None:
        np.testing.assert_array_equal(hyp[0], ref, strict=True)


@gpu
@pytest.mark.parametrize("lanes", [1, 4])
def test_mixed_batch(decoder, oracle, lanes):
    """The boundary streams beside benchmark images in one batch (sizes that
    differ widely: the flat destuff grid), four batches in a row so that at
    four lanes every lane takes one."""
    datas = [cases.case("bench_1000"), dc.aligned(dc.case("stuffed").data, 5),
             dc.aligned(dc.case("all_ones").data, 1), dc.aligned(dc.case("rst_every_block").data, 9),
             cases.case("bench_1001"), dc.aligned(dc.case("rst_fill").data, 3),
             dc.case("all_ones").data, cases.case("bench_1002")]
    refs = [oracle.decode_resize(d, oracle.Resize(**RESIZE32), pix_fmt="rgb24") for d in datas]
    out = Output(pix_fmt="rgb24", resize=True, **RESIZE32)
    prev = decoder.get_param("lanes")
    decoder.set_param("lanes", lanes)
    try:
        for _ in range(4):
            st, hyp = _decode(decoder, datas, out, (32, 32, 3))
            assert not any(st), st
            for i, r in enumerate(refs):
                np.testing.assert_array_equal(hyp[i], r, strict=True, err_msg=f"image {i}")
    finally:
        decoder.set_param("lanes", prev)
