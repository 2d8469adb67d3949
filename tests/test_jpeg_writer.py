"""CPU tests of the coefficient-level JPEG writer (tests/jpeg_writer.py) and of
the reference side of the hand-written stream families
(tests/jpeg_writer_cases.py): the oracle returns what was written, follows the
clip / wrap rules of FFmpeg's mjpeg dequantisation, refuses what it should,
and Pillow / libjpeg agree on the streams they accept."""

import io
from collections import Counter

import numpy as np
import pytest

from tests import jpeg_writer as jw
from tests import jpeg_writer_cases as hw
from tests.test_oracle import _py_simple_idct


def _i16(x):
    """Wrap to int16 (a C cast)."""
    return (np.asarray(x, np.int64) & 0xFFFF).astype(np.uint16).view(np.int16)


def expected_coefs(oracle, s: hw.Stream):
    """[nblocks, 64] dequantised coefficients in MCU order, natural order, by
    the rules DESIGN.md section 4 attributes to FFmpeg's mjpeg decoder: AC =
    int16(level * q) (wraps); DC biased by 1024 -- in a one-scan baseline
    frame accumulated from the differences in 32 bits (restarting from 1024
    at every restart interval) and clipped to int16, in a multi-scan frame
    int16(1024 + level * q) (wraps)."""
    info = oracle.parse(s.data)
    nat = s.natural_levels()
    out = np.zeros((info.nblocks, 64), np.int16)
    for b in range(info.nblocks):
        mcu, k = divmod(b, info.bpm)
        c = info.mcu_comp[k]
        mx, my = mcu % info.mcux, mcu // info.mcux
        if info.ncomp == 1:
            bx, by = mx, my
        else:
            bx = mx * info.comp_h[c] + info.mcu_dx[k]
            by = my * info.comp_v[c] + info.mcu_dy[k]
        q = np.zeros(64, np.int64)
        q[jw.NATURAL] = np.asarray(s.qtables[s.tq[c]], np.int64)
        lv = nat[c][by, bx].astype(np.int64)
        blk = _i16(lv * q)
        if info.multiscan:
            blk[0] = _i16(1024 + lv[0] * q[0])
        else:
            # 1024 + sum of diff * q over the restart interval == 1024 + level * q
            # (mod 2^32: |level * q| < 2^31 here, so no wrap), then the clip
            blk[0] = np.clip(1024 + lv[0] * q[0], -32768, 32767)
        out[b] = blk
    return out


@pytest.mark.parametrize("name", hw.ACCEPTED_CASES + hw.SCRIPT_LEGAL)
def test_level_round_trip(oracle, name):
    """The oracle returns the levels that were written (for the scripted
    streams libjpeg warns about: the levels the case expects by libjpeg's
    rule), and its dequantised coefficients follow the clip and wrap rules."""
    s = hw.case(name)
    info = oracle.parse(s.data)
    assert (info.width, info.height, info.ncomp) == (s.width, s.height, len(s.samp))
    assert bool(info.progressive) == (s.scans in ("spectral", "script"))
    assert bool(info.multiscan) == (s.scans in ("spectral", "script") or
                                    (s.scans == "per_component" and len(s.samp) > 1))
    coefs, levels = oracle.decode_coefs(s.data)
    for got, want in zip(levels, s.natural_levels()):
        np.testing.assert_array_equal(got, want.astype(np.int16), strict=True)
    np.testing.assert_array_equal(coefs, expected_coefs(oracle, s), strict=True)
    planes = oracle.decode_planes(s.data)
    hmax = max(h for h, _ in s.samp)
    vmax = max(v for _, v in s.samp)
    for p, (h, v) in zip(planes, s.samp):
        want = (s.height, s.width) if len(s.samp) == 1 else \
            (-(-s.height * v // vmax), -(-s.width * h // hmax))
        assert p.shape == want
    assert oracle.decode_rgb(s.data).shape == (s.height, s.width, 3)


def test_extremes_reach_the_clip_and_wrap_edges(oracle):
    """The family-3 streams do reach what they are for: baseline DC past the
    int16 clip on both sides, multi-scan DC and AC products that wrap."""
    c, _ = oracle.decode_coefs(hw.case("ext_dc_ramp").data)
    assert (c[:, 0] == 32767).sum() > 20 and (c[:, 0] == -32768).sum() > 20
    s = hw.case("ext_dc_ramp_pc")
    c, _ = oracle.decode_coefs(s.data)
    true_dc = 1024 + s.levels[0][..., 0].astype(np.int64) * 255
    assert (np.abs(true_dc) > 32768).sum() > 20  # these wrapped
    assert not ((c[:, 0] == 32767) | (c[:, 0] == -32768)).any()
    for name in ("ext_ac1023_q255", "ext_pq1", "ext_ac_sizes_11_15"):
        s = hw.case(name)
        prod = s.levels[0][..., 1:].astype(np.int64) * np.asarray(s.qtables[s.tq[0]])[1:]
        assert (np.abs(prod) > 32768).sum() > 20, name
    st = hw.case("ext_dc_cat15").stats
    assert st[("dc", 0)][15] > 10
    st = hw.case("ext_ac_sizes_11_15").stats[("ac", 0)]
    for size in range(11, 16):
        assert sum(n for sym, n in st.items() if sym & 15 == size) > 10


@pytest.mark.parametrize("name", ["tab_deep_all_symbols", "tab_deep_all_symbols_reversed"])
def test_every_symbol_occurs(name):
    st = hw.case(name).stats
    assert set(st[("dc", 0)]) == set(jw.DC_SYMBOLS)
    assert set(st[("ac", 0)]) == set(jw.AC_SYMBOLS) and len(jw.AC_SYMBOLS) == 242


def test_table_shapes():
    bits, vals = jw.deep_table(jw.AC_SYMBOLS)
    assert bits == [0] + [1] * 14 + [228] and len(vals) == 242
    lengths = sorted(n for _, n in jw.canonical_codes(bits, vals).values())
    assert lengths[:14] == list(range(2, 16)) and set(lengths[14:]) == {16}
    codes = jw.canonical_codes(*jw.flat_table(jw.AC_SYMBOLS))
    assert {n for _, n in codes.values()} == {8} and (0xFF, 8) not in codes.values()
    sh = jw.short_table()
    assert jw.canonical_codes(*sh[("dc", 0)])[0] == (0, 1)
    assert jw.canonical_codes(*sh[("ac", 0)])[jw.EOB] == (0, 1)
    inv = jw.short_table(inverted=True)
    assert jw.canonical_codes(*inv[("dc", 0)])[0] == (1, 1)
    assert jw.canonical_codes(*inv[("ac", 0)])[jw.EOB] == (1, 1)
    # 2 bits per block: 256 blocks in 64 bytes; the inverted all-zero scan is
    # all 1-bits, every byte stuffed
    s = hw.case("tab_short_inverted_ones")
    scan = s.data[s.data.index(b"\xff\xda") + 10:-2]
    assert scan == b"\xff\x00" * 64
    s = hw.case("tab_short")
    scan = s.data[s.data.index(b"\xff\xda") + 10:-2]
    # one category-4 difference (8 + 4 bits) and its EOB, then 2 bits a block
    assert len(scan) == -(-(8 + 4 + 1 + 255 * 2) // 8)


def test_std_tables_are_annex_k():
    """The literal Annex K tables equal the ones libjpeg writes by default."""
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(b, "JPEG", quality=90)
    d, p, found = b.getvalue(), 2, {}
    while d[p + 1] != 0xDA:
        n = (d[p + 2] << 8) | d[p + 3]
        if d[p + 1] == 0xC4:
            s = d[p + 4:p + 2 + n]
            while s:
                cnt = sum(s[1:17])
                found[("ac" if s[0] >> 4 else "dc", s[0] & 15)] = (list(s[1:17]), list(s[17:17 + cnt]))
                s = s[17 + cnt:]
        p += 2 + n
    assert found == {k: (list(b_), list(v)) for k, (b_, v) in jw.std_tables().items()}


def test_writer_structure():
    """Byte-level properties: stuffing, 1-padding, RSTn numbering and fill
    bytes, no EOB after k = 63, ZRLs for long runs, segment layouts."""
    s = hw.case("blk_rst_fill_3")
    d = s.data
    scan = d[d.index(b"\xff\xda"):]
    rst = [i for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    assert [scan[i + 1] & 7 for i in rst] == [i % 8 for i in range(len(rst))] and len(rst) == 5
    for i in rst:
        assert scan[i - 3:i] == b"\xff\xff\xff"
    st = hw.case("blk_k63_no_eob").stats
    nblk = sum(lv.shape[0] * lv.shape[1] for lv in hw.case("blk_k63_no_eob").levels)
    assert st[("ac", 0)][jw.EOB] == 0 and st[("ac", 1)][jw.EOB] == 0
    # blocks j % 4 == z carry z ZRLs
    assert st[("ac", 0)][jw.ZRL] + st[("ac", 1)][jw.ZRL] == sum(
        j % 4 for lv in hw.case("blk_k63_no_eob").levels for j in range(lv.shape[0] * lv.shape[1]))
    assert nblk == 24 + 6 + 6
    st = hw.case("blk_zrl_overshoot").stats
    assert st[("ac", 0)][jw.ZRL] > 20
    assert hw.case("blk_single_table_segments").data.count(b"\xff\xc4") == 4
    assert hw.case("blk_dri_zero").data.count(b"\xff\xdd\x00\x04\x00\x00") == 1
    assert hw.case("blk_rst_fill_1").data.count(b"\xff\xc4") == 1


def _scans(name, refine):
    """The statistics of a case's AC first (refine False) / refinement scans."""
    return [t for t in hw.case(name).stats["scans"]
            if t["entry"][1] > 0 and (t["entry"][3] > 0) == refine]


def test_script_symbol_coverage():
    """What the scripted streams are for, counted by the writer: every EOBn
    category in both AC scan kinds, the 32 refinement symbols, correction
    fields past the 15 bits of the kernel's short path and up to 63 bits,
    correction bits inside EOB runs, runs cut by restarts."""
    for refine in (False, True):
        cats = set()
        for name in ("scr_eob_runs", "scr_eob_run_14"):
            for t in _scans(name, refine):
                cats |= set(t["eob"])
                assert set(t["eob"]) == {sym >> 4 for sym in t["ac"] if sym & 15 == 0 and sym != jw.ZRL}
        assert cats == set(range(15)), (refine, cats)
        assert {c for t in _scans("scr_eob_runs", refine) for c in t["eob"]} == set(range(9))
        assert {c for t in _scans("scr_eob_runs_cap1", refine) for c in t["eob"]} == {0, 1}
    assert sum(t["corr_bits_inside_runs"] for t in _scans("scr_eob_runs", True)) >= 10
    assert sum(t["corr_bits_inside_runs"] for t in _scans("scr_eob_restart_ri5", True)) >= 10
    # a restart ends a run: no run of the 5-block intervals is longer than 5
    for refine in (False, True):
        assert {c for t in _scans("scr_eob_restart_ri5", refine) for c in t["eob"]} == {0, 1, 2}
    used = set()
    for name in hw.SCRIPT_LEGAL:
        for t in _scans(name, True):
            used |= set(t["ac"])
    assert used == set(hw.REFINE_SYMBOLS) and len(used) == 32
    # every (r, 1) and ZRL under the deep and the flat tables of scr_refine_tables
    st = hw.case("scr_refine_tables").stats
    assert {(r << 4) | 1 for r in range(16)} | {jw.ZRL} <= set(st[("ac", 2)])
    assert len(st[("ac", 3)]) > 4 and len(st[("ac", 1)]) > 4
    fields = Counter()
    for t in _scans("scr_dense_history", True):
        fields += t["corr_fields"]
    assert fields[63] > 10 and fields[62] > 20  # after EOB: 63 or 62; after (0, 1): 62
    fields = Counter()
    for t in _scans("scr_dense_history_17", True):
        fields += t["corr_fields"]
    assert all(fields[n] > 10 for n in (15, 16, 17))
    # scr_all_ones: the refinement data is ones -- stuffed 0xFF bytes
    for name in ("scr_all_ones", "scr_all_ones_ri4"):
        d = hw.case(name).data
        scan = d[d.rindex(b"\xff\xda"):]
        assert scan.count(b"\xff\x00") * 2 > 0.5 * len(scan), name  # (bytes in 0xFF 0x00 pairs)


def test_script_streams_keep_the_spectral_bytes():
    """scans="script" with Ah = Al = 0 and EOBRUN 0 writes the bytes of
    scans="spectral" (whose streams the existing cases depend on)."""
    s = hw.case("prog_420")
    script = [([0, 1, 2], 0, 0, 0, 0)] + [([c], a, b, 0, 0) for c in range(3) for a, b in ((1, 5), (6, 63))]
    ids = [0, 1, 1]
    again = jw.write_jpeg(s.width, s.height, s.samp, s.levels, s.qtables, s.tq, jw.std_tables(), ids, ids,
                          scans="script", script=script)
    assert again == s.data


@pytest.mark.parametrize("name", hw.CAPPED_CASES)
def test_clamp_cap(oracle, name):
    """Families 1, 2, 4, 5 and the capped cases of 6: at most 25 % of the oracle's RGB samples sit at 0
    or 255, so the output clamp cannot carry a parity test."""
    assert hw.saturated_share(oracle.decode_rgb(hw.case(name).data)) <= 0.25


@pytest.mark.parametrize("name", hw.REFUSED_CASES + hw.SCRIPT_BAD)
def test_oracle_refuses(oracle, name):
    # JO_ERR_UNSUPPORTED for the layouts; JO_ERR_BAD_HUFFMAN for a refinement
    # symbol of size 2 and for a new coefficient whose run passes Se
    code = 4 if name in hw.SCRIPT_BAD else 2
    with pytest.raises(oracle.OracleError) as e:
        oracle.decode_rgb(hw.case(name).data)
    assert e.value.code == code
    rs = oracle.Resize(fit_w=32, fit_h=32, aspect="decrease", pad_w=32, pad_h=32)
    with pytest.raises(oracle.OracleError) as e:
        oracle.decode_resize(hw.case(name).data, rs, "rgb24")
    assert e.value.code == code


def test_zrl_overshoot_ends_the_block(oracle):
    """ZRL symbols that carry k past 63 end the block silently (FFmpeg's
    decode_block leaves its loop at i >= 63): the stream decodes to the
    written levels, as the same levels with plain EOBs do."""
    s = hw.case("blk_zrl_overshoot")
    plain = jw.write_jpeg(s.width, s.height, s.samp, s.levels, s.qtables, s.tq, jw.std_tables(),
                          s.tq, s.tq)
    assert plain != s.data
    np.testing.assert_array_equal(oracle.decode_rgb(s.data), oracle.decode_rgb(plain))


PILLOW_SAMPLINGS = ["440", "411", "410", "22_12"]


def _pillow_stream(key):
    samp = hw.SAMPLINGS[key]
    w, h = (70, 29) if samp[0][0] == 4 else (37, 29)
    rng = np.random.default_rng(3)
    levels = hw.moderate_levels(rng, [g[0] for g in jw.block_grids(w, h, samp)], ac=30, dc=300,
                                nnz=6)
    q = {0: np.ones(64, int), 1: np.ones(64, int)}
    return w, h, jw.write_jpeg(w, h, samp, levels, q, [0, 1, 1], jw.std_tables(), [0, 1, 1],
                               [0, 1, 1]), levels


@pytest.mark.parametrize("key", PILLOW_SAMPLINGS + hw.SCRIPT_PILLOW)
def test_pillow_decodes_the_legal_streams(oracle, key):
    """Moderate levels (|AC| <= 30, |DC| <= 300, q = 1), 8-bit tables, Annex K
    codes: Pillow (libjpeg) opens the stream at the right size and mode, and
    its luma is within 1 of the oracle's islow plane (the 1 is Pillow's
    YCbCr -> RGB -> YCbCr round trip; luma is never subsampled).  The same
    for the scripted progressive streams that are legal T.81."""
    from PIL import Image

    if key.startswith("scr_"):
        s = hw.case(key)
        w, h, data = s.width, s.height, s.data
    else:
        w, h, data, _ = _pillow_stream(key)
    im = Image.open(io.BytesIO(data))
    assert im.size == (w, h) and im.mode == ("L" if key == "scr_eob_runs" else "RGB")
    im.draft("YCbCr", (w, h))
    luma = np.asarray(im.convert("YCbCr"))[..., 0].astype(int)
    ref = oracle.decode_planes(data, oracle.IDCT_ISLOW)[0].astype(int)
    assert luma.shape == ref.shape
    assert np.abs(luma - ref).max() <= 1


@pytest.mark.parametrize("key", PILLOW_SAMPLINGS + ["1x4", "22_21", "gray22"] + hw.SCRIPT_LEGAL)
def test_coefficients_match_libjpeg(oracle, key):
    """libjpeg 9's jpeg_read_coefficients returns the written levels.  The
    scripted streams too: for scr_order (DC first scan after its refinement),
    scr_repeat_refine, scr_overlap_first and scr_zrl_overshoot_refine libjpeg
    warns of a bogus progression or decodes silently, and returns the levels
    the case expects (its warnings are not fatal here: ljpin.c's emit_message
    drops them)."""
    if oracle.ljpin() is None:
        pytest.skip("libjpeg 9 not available on this host")
    name = key if key.startswith("scr_") else next(
        n for n in hw.SAMPLING_CASES if n.startswith(f"samp_{key}_") and n.endswith("ri1"))
    s = hw.case(name)
    for got, want in zip(oracle.lj_read_coefs(s.data), s.natural_levels()):
        np.testing.assert_array_equal(got, want.astype(np.int16))


@pytest.mark.parametrize("name", hw.JFIF_CASES)
def test_islow_jfif_matches_libjpeg(oracle, name):
    """islow IDCT + box-replicated components + JFIF conversion: bit-exact
    vs libjpeg 9 (no fancy upsampling) on every sampling, luma sampled below
    chroma included (the first component is replicated like the others)."""
    if oracle.ljpin() is None:
        pytest.skip("libjpeg 9 not available on this host")
    d = hw.case(name).data
    hyp = oracle.decode_rgb(d, oracle.IDCT_ISLOW, "rgb24", csc="jfif")
    np.testing.assert_array_equal(hyp, oracle.lj_decode_rgb(d), strict=True)


def test_jfif_replicates_luma_sampled_below_chroma(oracle):
    """Without libjpeg: (1x1, 2x2, 2x2) through csc="jfif" equals converting
    the planes by hand, each component read at x * h / hmax, y * v / vmax."""
    d = hw.case("refused_luma_under_chroma").data
    y, cb, cr = [p.astype(np.int64) for p in oracle.decode_planes(d, oracle.IDCT_ISLOW)]
    H, W = cb.shape
    assert y.shape == (-(-H // 2), -(-W // 2))
    yy, xx = np.mgrid[0:H, 0:W]
    y = y[yy // 2, xx // 2]
    # libjpeg jdcolor.c build_ycc_rgb_table, 16-bit fixed point
    def fix(v):
        return int(v * 65536 + 0.5)
    r = y + ((fix(1.402) * (cr - 128) + 32768) >> 16)
    g = y + ((-fix(0.344136286) * (cb - 128) - fix(0.714136286) * (cr - 128) + 32768) >> 16)
    b = y + ((fix(1.772) * (cb - 128) + 32768) >> 16)
    want = np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)
    hyp = oracle.decode_rgb(d, oracle.IDCT_ISLOW, "rgb24", csc="jfif")
    np.testing.assert_array_equal(hyp, want, strict=True)


def test_simple_idct_full_range_blocks_of_the_streams(oracle):
    """The family-3 worst-case blocks through both restatements of
    simple_idct (the same check as test_oracle's, on the exact blocks the GPU
    tests decode)."""
    for blk in hw.idct_worst_blocks():
        b = np.clip(blk, -32768, 32767).astype(np.int16)
        np.testing.assert_array_equal(oracle.idct_block(b, 0), _py_simple_idct(b))
