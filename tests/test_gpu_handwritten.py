"""GPU parity on hand-written JPEG bitstreams (tests/jpeg_writer.py): sampling
layouts, Huffman table shapes, coefficient values and block structures that no
encoder in the suite emits.  Families and streams: tests/jpeg_writer_cases.py.

Bar: bit-exact vs the oracle on every surface (np.testing.assert_array_equal):
  (a) Decoder.debug_entropy's dequantised coefficients vs oracle.decode_coefs
      -- the one check the 0 / 255 output clamp cannot hide;
  (b) decode_planes, simple and islow IDCT;
  (c) full-resolution rgb24: the default (fused) path and output_path 1 and 2;
  (d) a small resize (fit 32x32 decrease, pad 32x32, bicubic), default and
      with sws_prepass = 1.
Families 2-5 (entropy-sensitive) also run on a second Decoder with
sub_bits = 32 and entropy_threads = 128, so these small scans still split
into many subsequences and chain hand-offs.

Family 6 (scan scripts: SOF2 with successive approximation) runs on the one
Decoder: multiscan_kernel takes no sub_bits / entropy_threads.

Families 1, 2, 4, 5 and the capped cases of 6 assert that at most 25 % of the oracle's RGB samples are
0 or 255.  Family 3 saturates by nature (share of saturated RGB samples in
the oracle's output, interleaved / one scan per component: ac1023_q255 0.51 /
0.51, ac_sizes_11_15 0.52 / 0.53, pq1 0.52 / 0.52, dense 0.00 / 0.00, dc_ramp
0.68 / 0.56, dc_cat15 0.48 / 0.48, idct_worst 0.51 / 0.51): there (a) and (b)
carry the check.
"""

import numpy as np
import pytest
import torch

from spdl_amd._lib import Output
from tests import cases
from tests import jpeg_writer_cases as hw

pytestmark = pytest.mark.gpu

RESIZE32 = dict(fit_w=32, fit_h=32, aspect="decrease", pad_w=32, pad_h=32)
UNSUPPORTED = 2  # SPDL_HJ_ERR_UNSUPPORTED == JO_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def fine_decoder(decoder):
    """32-bit subsequences, 128 entropy threads (as test_subsequence_sizes);
    asks for `decoder` first, so it skips where there is no device."""
    from spdl_amd._lib import Decoder

    dec = Decoder(0)
    dec.set_param("sub_bits", 32)
    dec.set_param("entropy_threads", 128)
    yield dec
    dec.close()


def _decode(dec, datas, out: Output, shape):
    t = torch.empty((len(datas),) + tuple(shape), dtype=torch.uint8, device="cuda:0")
    st = dec.decode_batch(datas, out, t.data_ptr(), t.numel(), stream=torch.cuda.current_stream())
    assert all(s == 0 for s in st), st
    return t.cpu().numpy()


def _with_param(dec, name, value, restore, fn):
    dec.set_param(name, value)
    try:
        return fn()
    finally:
        dec.set_param(name, restore)


def check_coefs(dec, oracle, d):
    """(a): [nblocks, 64], MCU order, natural order, dequantised, DC + 1024."""
    ref, _ = oracle.decode_coefs(d)
    hyp, _, diag = dec.debug_entropy(d, ref.shape[0])
    assert diag["status"] == 0, diag
    np.testing.assert_array_equal(hyp, ref, strict=True)


def check_planes(dec, oracle, d):
    for idct, oi in (("simple", oracle.IDCT_SIMPLE), ("islow", oracle.IDCT_ISLOW)):
        hyp = dec.decode_planes(d, idct=idct)
        ref = oracle.decode_planes(d, idct=oi)
        assert len(hyp) == len(ref)
        for c, (h, r) in enumerate(zip(hyp, ref)):
            np.testing.assert_array_equal(h, r, strict=True, err_msg=f"{idct} plane {c}")


def check_rgb(dec, oracle, d, paths=(0, 2, 1)):
    ref = oracle.decode_rgb(d, oracle.IDCT_SIMPLE, "rgb24")
    for path in paths:
        hyp = _with_param(dec, "output_path", path, 0,
                          lambda: _decode(dec, [d], Output(pix_fmt="rgb24"), ref.shape)[0])
        np.testing.assert_array_equal(hyp, ref, strict=True, err_msg=f"output_path {path}")
    return ref


def check_resize(dec, oracle, d):
    ref = oracle.decode_resize(d, oracle.Resize(**RESIZE32), pix_fmt="rgb24")
    out = Output(pix_fmt="rgb24", resize=True, **RESIZE32)
    for pre in (-1, 1):
        hyp = _with_param(dec, "sws_prepass", pre, -1,
                          lambda: _decode(dec, [d], out, ref.shape)[0])
        np.testing.assert_array_equal(hyp, ref, strict=True, err_msg=f"sws_prepass {pre}")


def check_all(dec, oracle, d, capped):
    check_coefs(dec, oracle, d)
    check_planes(dec, oracle, d)
    ref = check_rgb(dec, oracle, d)
    check_resize(dec, oracle, d)
    if capped:
        assert hw.saturated_share(ref) <= 0.25, "the clamp could carry this case"


# ---- family 1: samplings ----------------------------------------------------

@pytest.mark.parametrize("name", hw.SAMPLING_CASES)
def test_samplings(decoder, oracle, name):
    check_all(decoder, oracle, hw.case(name).data, capped=True)


@pytest.mark.parametrize("key", list(hw.SAMPLINGS))
def test_samplings_between_ordinary_images(decoder, oracle, key):
    """Each accepted sampling in one batch between q90_420 and gray: its
    neighbours' descriptors, plans and tables must not be disturbed."""
    mine = [hw.case(n).data for n in hw.SAMPLING_CASES if n.startswith(f"samp_{key}_")]
    datas = [cases.case("q90_420")]
    for d in mine:
        datas += [d, cases.case("gray") if len(datas) % 4 == 1 else cases.case("q90_420")]
    out = Output(pix_fmt="rgb24", resize=True, **RESIZE32)
    hyp = _decode(decoder, datas, out, (32, 32, 3))
    for i, d in enumerate(datas):
        ref = oracle.decode_resize(d, oracle.Resize(**RESIZE32), pix_fmt="rgb24")
        np.testing.assert_array_equal(hyp[i], ref, strict=True, err_msg=f"image {i}")


@pytest.mark.parametrize("name", hw.JFIF_CASES)
def test_samplings_jfif_islow(decoder, oracle, name):
    """libjpeg's conversion (csc="jfif", islow IDCT: pinned to libjpeg 9 by
    test_jpeg_writer) on every sampling, and on the layouts only this path
    takes: luma sampled below chroma, a 3:1 ratio, unlike chroma components.
    Every component is replicated from its own grid, the first included."""
    d = hw.case(name).data
    for fmt in ("rgb24", "bgr"):
        ref = oracle.decode_rgb(d, oracle.IDCT_ISLOW, fmt, csc="jfif")
        hyp = _decode(decoder, [d], Output(pix_fmt=fmt, idct="islow", csc="jfif"), ref.shape)[0]
        np.testing.assert_array_equal(hyp, ref, strict=True, err_msg=fmt)


@pytest.mark.parametrize("name", hw.REFUSED_CASES)
def test_refused_layouts(decoder, oracle, name):
    """Luma under chroma, a 3x1 ratio, unlike chroma components, more than 10
    blocks per MCU, and 4-component / RGB-id frames with sampled components:
    the unsupported status from both decoders, full resolution and resized;
    the decoder then decodes q90_444 correctly."""
    d = hw.case(name).data
    for out, shape, ref in (
            (Output(pix_fmt="rgb24"), (29, 37, 3), lambda: oracle.decode_rgb(d)),
            (Output(pix_fmt="rgb24", resize=True, **RESIZE32), (32, 32, 3),
             lambda: oracle.decode_resize(d, oracle.Resize(**RESIZE32), "rgb24"))):
        with pytest.raises(oracle.OracleError) as e:
            ref()
        assert e.value.code == UNSUPPORTED
        t = torch.empty(shape, dtype=torch.uint8, device="cuda:0")
        st = decoder.decode_batch([d], out, t.data_ptr(), t.numel(),
                                  stream=torch.cuda.current_stream(), check=False)
        assert st == [UNSUPPORTED]
        with pytest.raises(RuntimeError, match="Failed to decode an image"):
            decoder.decode_batch([d], out, t.data_ptr(), t.numel(),
                                 stream=torch.cuda.current_stream())
    good = cases.case("q90_444")
    hyp = _decode(decoder, [good], Output(pix_fmt="rgb24"), (240, 320, 3))[0]
    np.testing.assert_array_equal(hyp, oracle.decode_rgb(good, 0, "rgb24"), strict=True)


# ---- families 2-5 -----------------------------------------------------------

@pytest.mark.parametrize("name", hw.TABLE_CASES)
def test_tables(decoder, fine_decoder, oracle, name):
    s = hw.case(name)
    if name.startswith("tab_deep_all_symbols"):
        from tests import jpeg_writer as jw

        assert set(s.stats[("dc", 0)]) == set(jw.DC_SYMBOLS)  # all 16 categories
        assert set(s.stats[("ac", 0)]) == set(jw.AC_SYMBOLS)  # EOB, ZRL, 240 run/size pairs
    check_all(decoder, oracle, s.data, capped=True)
    check_coefs(fine_decoder, oracle, s.data)
    check_rgb(fine_decoder, oracle, s.data, paths=(0,))


@pytest.mark.parametrize("name", hw.EXTREME_CASES)
def test_coefficient_extremes(decoder, fine_decoder, oracle, name):
    d = hw.case(name).data
    check_all(decoder, oracle, d, capped=False)
    check_coefs(fine_decoder, oracle, d)
    check_planes(fine_decoder, oracle, d)


@pytest.mark.parametrize("name", hw.STRUCTURE_CASES)
def test_block_structure(decoder, fine_decoder, oracle, name):
    d = hw.case(name).data
    check_all(decoder, oracle, d, capped=True)
    check_coefs(fine_decoder, oracle, d)
    check_rgb(fine_decoder, oracle, d, paths=(0,))


@pytest.mark.parametrize("name", hw.PROGRESSIVE_CASES)
def test_spectral_selection(decoder, fine_decoder, oracle, name):
    """SOF2 by spectral selection alone (one interleaved DC scan, AC band
    scans per component, no refinement, every EOBRUN 0) in samplings and with
    tables Pillow's progressive writer never uses."""
    d = hw.case(name).data
    check_all(decoder, oracle, d, capped=True)
    check_coefs(fine_decoder, oracle, d)
    check_rgb(fine_decoder, oracle, d, paths=(0,))


# ---- family 6: scan scripts -------------------------------------------------

BAD_HUFFMAN = 4  # SPDL_HJ_ERR_BAD_HUFFMAN == JO_ERR_BAD_HUFFMAN


def _status(dec, d, out, shape):
    t = torch.empty(shape, dtype=torch.uint8, device="cuda:0")
    return dec.decode_batch([d], out, t.data_ptr(), t.numel(), stream=torch.cuda.current_stream(),
                            check=False)


def _good_image_decodes(dec, oracle):
    good = cases.case("q90_444")
    hyp = _decode(dec, [good], Output(pix_fmt="rgb24"), (240, 320, 3))[0]
    np.testing.assert_array_equal(hyp, oracle.decode_rgb(good, 0, "rgb24"), strict=True)


@pytest.mark.parametrize("name", hw.SCRIPT_CASES)
def test_scan_scripts(decoder, oracle, name):
    """Hand-written progressive streams: Al up to 13 and up to fourteen passes
    over a coefficient, correction fields of 15..63 bits, EOB runs of every
    category (across chunk boundaries, cut by restarts, with correction bits
    inside), refinement bands unlike the first scans', DC scans per
    component, odd scan orders, deep / flat / redefined refinement tables,
    refinement through the stuffed reader, and three kinds of stream libjpeg
    warns about but decodes (a refinement repeated, first scans that overlap,
    a ZRL past Se in a refinement scan).  The oracle's levels are pinned to
    libjpeg 9's by test_jpeg_writer.  No fine_decoder here: multiscan_kernel
    takes no EntropyParams (neither sub_bits nor entropy_threads reaches it;
    it always runs 256 threads)."""
    d = hw.case(name).data
    if name == "scr_eob_run_14":  # 1032 x 1024: coefficients and the simple-IDCT planes only
        check_coefs(decoder, oracle, d)
        for h, r in zip(decoder.decode_planes(d, idct="simple"),
                        oracle.decode_planes(d, idct=oracle.IDCT_SIMPLE)):
            np.testing.assert_array_equal(h, r, strict=True)
        return
    check_all(decoder, oracle, d, capped=name in hw.SCRIPT_CAPPED)


def test_scan_scripts_in_a_batch(decoder, oracle):
    """Scripted streams between encoder-made ones in one batch, decoded twice
    on the same Decoder: levels, masks or destuffed copies left over from a
    neighbour or from the first pass would show."""
    datas = [cases.case("q90_420"), hw.case("scr_deep_al").data, cases.case("gray"),
             hw.case("scr_band_merge").data, hw.case("prog_420").data, hw.case("scr_order").data,
             hw.case("scr_eob_restart_ri5").data, hw.case("scr_dense_history").data]
    out = Output(pix_fmt="rgb24", resize=True, **RESIZE32)
    refs = [oracle.decode_resize(d, oracle.Resize(**RESIZE32), pix_fmt="rgb24") for d in datas]
    for again in (0, 1):
        hyp = _decode(decoder, datas, out, (32, 32, 3))
        for i, ref in enumerate(refs):
            np.testing.assert_array_equal(hyp[i], ref, strict=True, err_msg=f"pass {again} image {i}")


def test_scan_limit(decoder, oracle):
    """64 scans decode; the 65th SOS is refused as unsupported (kMsMaxScans:
    the documented limit -- the oracle decodes that stream); the decoder
    then decodes q90_444."""
    s = hw.case("scr_scans_64")  # (every surface: test_scan_scripts)
    assert len(s.script) == 64
    check_coefs(decoder, oracle, s.data)
    check_rgb(decoder, oracle, s.data, paths=(0,))
    s = hw.case("scr_scans_65")
    assert len(s.script) == 65
    assert oracle.decode_rgb(s.data).shape == (s.height, s.width, 3)
    for out, shape in ((Output(pix_fmt="rgb24"), (s.height, s.width, 3)),
                       (Output(pix_fmt="rgb24", resize=True, **RESIZE32), (32, 32, 3))):
        assert _status(decoder, s.data, out, shape) == [UNSUPPORTED]
        t = torch.empty(shape, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(RuntimeError, match="Failed to decode an image"):
            decoder.decode_batch([s.data], out, t.data_ptr(), t.numel(),
                                 stream=torch.cuda.current_stream())
    _good_image_decodes(decoder, oracle)


@pytest.mark.parametrize("name", hw.SCRIPT_BAD)
def test_refused_refinement_symbols(decoder, oracle, name):
    """A refinement symbol of size 2, and a (r, 1) whose run passes Se: the
    oracle's status from the device, alone and between two good images (which
    decode); a good image decodes afterwards."""
    s = hw.case(name)
    with pytest.raises(oracle.OracleError) as e:
        oracle.decode_rgb(s.data)
    assert e.value.code == BAD_HUFFMAN
    out = Output(pix_fmt="rgb24")
    assert _status(decoder, s.data, out, (s.height, s.width, 3)) == [e.value.code]
    twin = hw.case("scr_zrl_overshoot_refine")  # the same layout and size, accepted
    assert (twin.width, twin.height) == (s.width, s.height)
    t = torch.empty((3, s.height, s.width, 3), dtype=torch.uint8, device="cuda:0")
    st = decoder.decode_batch([twin.data, s.data, twin.data], out, t.data_ptr(), t.numel(),
                              stream=torch.cuda.current_stream(), check=False)
    assert st == [0, e.value.code, 0]
    ref = oracle.decode_rgb(twin.data, oracle.IDCT_SIMPLE, "rgb24")
    for i in (0, 2):
        np.testing.assert_array_equal(t[i].cpu().numpy(), ref, strict=True)
    _good_image_decodes(decoder, oracle)
