"""GPU parity of entropy_kernel where the instruction cuts of its symbol step
(listed in hj_common.h above kSubShare; the forms they replaced were measured
and removed, profiles/r15/entropy_step: the second-level address from a fixed share of the
sub-table pool, the level-1 mark, the entry's flag bits as a bound on z, the
funnel-shifted second step of a window read) could go wrong, on hand-written
streams (tests/jpeg_writer.py).  Bit-exact against the oracle:
Decoder.debug_entropy's coefficients and decode_planes, at 1 and 4 lanes,
alone and in a batch between two ordinary images; the coefficients also on a
decoder with 32-bit subsequences and 128 entropy threads, where these small
scans still split into many runs.

  code lengths   deep, reversed deep, flat (one length, and 16), ranked and
                 short tables: together every code length 1-16 in a DC and in
                 an AC table.  AC tables whose long codes take 8 level-1
                 cells -- a table slot's share of the LDS pool exactly, from a
                 cell that is a multiple of 8 and from one that is not (the
                 share wraps) -- and 9 (the image goes to the wide path); six
                 distinct tables in one scan (two of them read from HBM).
  values         every size 1-10 (DC: 1-11) at +-2^(s-1) and +-(2^s - 1), DC
                 size 0; the same levels through Annex K tables (entries that
                 hold the value) and reversed deep tables (entries that hold
                 the code alone).
  block ends     EOB at every z of 1..63; ZRLs that end a block at exactly 64;
                 a coefficient at 63 after three ZRLs; 63 non-zero ACs; a
                 coefficient run past 63 and an AC size-0 symbol other than EOB
                 / ZRL: the oracle's error status (a failed image hands out no
                 coefficients, so the blocks before the symbol are checked
                 where the same stream without it decodes: the twin stream),
                 and its neighbours in a batch still decode.
  MCU order      4:2:0, 4:2:2, 4:4:4, 4:1:1, gray, 2x2 luma with 2x1 chroma
                 and 4x2 luma (10 blocks per MCU); one table pair for every
                 component, and four distinct tables; restart intervals of one
                 MCU and of an MCU row; segments of 2 bits.
  slot edges     one stream behind a first block of 12..43 bits: every symbol
                 of the rest crosses the 384-bit slot ends at each of the 32
                 bit offsets.
  list groups    AC counts 0, 1, 2, 3, 4, 5, 63 over consecutive blocks: the
                 16-byte groups of the packed lists end inside, at and across
                 block ends, and the run ends in a partial group.

All streams are uncapped (as test_gpu_idct_cuts): extreme values saturate by
design, the coefficients and planes carry the check.
"""

import functools

import numpy as np
import pytest

from spdl_amd._lib import Output
from tests import cases
from tests import jpeg_writer as jw
from tests import jpeg_writer_cases as hw
from tests.test_gpu_handwritten import RESIZE32, check_coefs, check_planes

gpu = pytest.mark.gpu  # (the tests of the streams themselves need the oracle only)
BAD_HUFFMAN = 4  # SPDL_HJ_ERR_BAD_HUFFMAN == JO_ERR_BAD_HUFFMAN
LUT_BITS = 10    # hj_common.h kLutBits: codes longer than this live in sub-tables
SHARE_CELLS = 8  # ... kSubShare >> kSubBits: level-1 cells of long codes a table slot holds

GRAY = [(1, 1)]
S444 = [(1, 1)] * 3
ONES = {0: np.ones(64, int), 1: np.ones(64, int)}


def _grid(lv, bh, bw):
    """[n, 64] zig-zag levels, raster block order -> [bh, bw, 64], zero blocks after the last."""
    out = np.zeros((bh * bw, 64), np.int32)
    assert len(lv) <= bh * bw, (len(lv), bh * bw)
    out[:len(lv)] = lv
    return out.reshape(bh, bw, 64)


def _gray(name, lv, bh, bw, dht, **kw):
    return hw._write(name, 8 * bw, 8 * bh, GRAY, [_grid(lv, bh, bw)], {0: np.ones(64, int)}, [0], dht,
                     [0], [0], **kw)


def _lengths(stream, key):
    """Histogram of the code lengths the writer used from table `key`."""
    codes = jw.canonical_codes(*stream.dht[key])
    out = {}
    for sym, n in stream.stats[key].items():
        out[codes[sym][1]] = out.get(codes[sym][1], 0) + n
    return out


def _long_cells(bits):
    """Level-1 cells that continue in a sub-table (lut_kernel's p_lo..p_hi): first, count."""
    code, lo, hi = 0, 1 << LUT_BITS, -1
    for length in range(1, 17):
        n = bits[length - 1]
        if n and length > LUT_BITS:
            lo = min(lo, code >> (length - LUT_BITS))
            hi = max(hi, (code + n - 1) >> (length - LUT_BITS))
        code = (code + n) << 1
    return (lo, hi - lo + 1) if hi >= lo else (0, 0)


class _S:
    """A stream and the tables it was written with."""

    def __init__(self, stream, dht):
        self.stream, self.dht = stream, dht
        self.data, self.stats = stream.data, stream.stats


def _mk(stream, dht):
    return _S(stream, dht)


# ---- code lengths ------------------------------------------------------------------

def _all_length_levels():
    """Gray levels that use, from deep_table(DC_SYMBOLS) / deep_table(AC_SYMBOLS)
    in either order, a code of every length the table has: DC categories
    0-15, and EOB, ZRL, the runs 0-15 of size 1 and sizes 1-15 of run 0."""
    lv = []
    dc = 0
    for s in range(16):  # DC categories as differences
        d = 0 if s == 0 else (1 << (s - 1)) + (s % 3 if s > 2 else 0)
        dc = dc + d if dc <= 0 else dc - d
        b = np.zeros(64, np.int32)
        b[0] = dc
        lv.append(b)
    k, b = 1, np.zeros(64, np.int32)
    b[0] = dc
    for r in range(16):  # runs 0-15 of size 1
        if k + r > 63:
            lv.append(b)
            k, b = 1, np.zeros(64, np.int32)
            b[0] = dc
        b[k + r] = 1 if r % 2 else -1
        k += r + 1
    lv.append(b)
    b = np.zeros(64, np.int32)
    b[0] = dc
    for s in range(1, 16):  # sizes 1-15 of run 0
        b[s] = (1 << s) - 1 if s % 2 else -(1 << (s - 1))
    b[40] = 3  # a run of 24: ZRL
    lv.append(b)
    rng = np.random.default_rng(7)
    for _ in range(12):  # small texture
        b = np.zeros(64, np.int32)
        b[0] = dc + int(rng.integers(-9, 10))
        b[rng.integers(1, 20, size=5)] = rng.integers(-6, 7, size=5)
        lv.append(b)
    return np.array(lv)


def _share_table(n_long, offset):
    """An AC table with EOB on '0', `offset` symbols on 10-bit codes and n_long
    on 11-bit codes: the long codes start `offset` level-1 cells past a
    multiple of 8 and take ceil(n_long / 2) cells."""
    long_syms = [(r << 4) | s for r in range(3) for s in range(1, 9)][:n_long]
    ten = [jw.ZRL, 0x31, 0x41, 0x51][:offset]
    bits = [0] * 16
    bits[0], bits[9], bits[10] = 1, len(ten), len(long_syms)
    jw._check_kraft(bits)
    return bits, [jw.EOB] + ten + long_syms


def _share_levels(n_long):
    """Every long symbol of _share_table(n_long, .) in turn: run r, size s."""
    syms = [(r, s) for r in range(3) for s in range(1, 9)][:n_long]
    lv = []
    for j in range(40):
        b = np.zeros(64, np.int32)
        b[0] = (j * 13) % 41 - 20
        k = 1
        for i in range(6):
            r, s = syms[(6 * j + i) % len(syms)]
            k += r
            mag = (1 << (s - 1)) + (j + i) % (1 << (s - 1))
            b[k] = mag if (i + j) % 2 else -mag
            k += 1
        lv.append(b)
    return np.array(lv)


@functools.lru_cache(maxsize=None)
def _length_stream(key):
    dc, ac = jw.DC_SYMBOLS, jw.AC_SYMBOLS
    if key in ("deep", "deep_reversed", "ranked", "ranked_reversed"):
        rev = key.endswith("reversed")
        make = jw.deep_table if key.startswith("deep") else jw.ranked_table
        dht = {("dc", 0): make(dc[::-1] if rev else dc), ("ac", 0): make(ac[::-1] if rev else ac)}
        return _mk(_gray("len_" + key, _all_length_levels(), 6, 8, dht,
                         restart_interval=5 if rev else 0), dht)
    if key in ("flat", "flat16"):
        n = 16 if key == "flat16" else None
        dht = {("dc", 0): jw.flat_table(dc, n), ("ac", 0): jw.flat_table(ac, n)}
        return _mk(_gray("len_" + key, _all_length_levels(), 6, 8, dht), dht)
    if key == "short":  # 1-bit DC 0 and EOB, the rest on 8 bits
        dht = jw.short_table()
        lv = np.zeros((64, 64), np.int32)
        lv[:, 0] = 9 + np.repeat(np.arange(8), 8) % 3  # mostly unchanged DC: 2-bit blocks
        lv[5::9, 1] = 2
        lv[7::11, 17] = -1  # ZRL + (0, 1)
        return _mk(_gray("len_short", lv, 8, 8, dht), dht)
    if key.startswith("share"):  # share_<long codes>_<offset cells>
        n_long, offset = (int(x) for x in key.split("_")[1:])
        dht = {("dc", 0): jw.std_tables()[("dc", 0)], ("ac", 0): _share_table(n_long, offset)}
        return _mk(_gray("len_" + key, _share_levels(n_long), 5, 8, dht), dht)
    if key == "six_tables":
        rng = np.random.default_rng(29)
        w, h = 40, 24
        levels = hw.moderate_levels(rng, hw._grid_shapes(w, h, S444))
        dht = {("dc", 0): jw.deep_table(dc), ("ac", 2): jw.ranked_table(ac),
               ("dc", 1): jw.ranked_table(dc[::-1]), ("ac", 0): jw.deep_table(ac[::-1]),
               ("dc", 2): jw.deep_table(dc[8:] + dc[:8]), ("ac", 1): jw.ranked_table(ac[100:] + ac[:100])}
        return _mk(hw._write("len_six_tables", w, h, S444, levels, hw._small_q(rng, (0, 1, 2)),
                             [0, 1, 2], dht, [0, 1, 2], [2, 0, 1], restart_interval=2), dht)
    raise KeyError(key)


SHARE_KEYS = ["share_16_0", "share_16_3", "share_18_0", "share_17_3"]
LENGTH_KEYS = ["deep", "deep_reversed", "ranked", "ranked_reversed", "flat", "flat16", "short",
               "six_tables"] + SHARE_KEYS


def test_length_streams_hold_every_code_length():
    """Per symbol class, the writer's histogram of code lengths over the family
    covers 1..16; the share tables' long codes take the cells they are named
    for, each long symbol is used, and 8 cells fill a slot's share."""
    seen = {"dc": set(), "ac": set()}
    for key in LENGTH_KEYS:
        s = _length_stream(key)
        for (cls, tid) in s.dht:
            if s.stats.get((cls, tid)):
                seen[cls] |= set(_lengths(s, (cls, tid)))
    assert seen["dc"] == set(range(1, 17)), sorted(seen["dc"])
    assert seen["ac"] == set(range(1, 17)), sorted(seen["ac"])
    cells = {}
    for key in SHARE_KEYS:
        s = _length_stream(key)
        bits, vals = s.dht[("ac", 0)]
        cells[key] = _long_cells(bits)
        long_syms = vals[1 + bits[9]:]
        assert set(long_syms) <= set(s.stats[("ac", 0)]), key
    assert cells == {"share_16_0": (512, 8), "share_16_3": (515, 8), "share_18_0": (512, 9),
                     "share_17_3": (515, 9)}
    assert SHARE_CELLS == 8 and 515 % SHARE_CELLS != 0


# ---- values ------------------------------------------------------------------------

def _extremes(s):
    return [1 << (s - 1), (1 << s) - 1, -(1 << (s - 1)), -((1 << s) - 1)]


def _value_levels():
    """Restart interval 1 (every DC level is its own difference): block (s, e)
    holds DC extreme e of size s (1-11), the four AC extremes of size min(s,
    10) at k = 1..4 and extreme e again at k = 10 (run 5); a last block of DC 0."""
    lv = []
    for s in range(1, 12):
        for e in range(4):
            b = np.zeros(64, np.int32)
            b[0] = _extremes(s)[e]
            sa = min(s, 10)
            b[1:5] = _extremes(sa)
            b[10] = _extremes(sa)[e]
            lv.append(b)
    lv.append(np.zeros(64, np.int32))
    return np.array(lv)


@functools.lru_cache(maxsize=None)
def _value_stream():
    std = jw.std_tables()
    dht = {("dc", 0): std[("dc", 0)], ("ac", 0): std[("ac", 0)],
           ("dc", 1): jw.deep_table(jw.DC_SYMBOLS[::-1]), ("ac", 1): jw.deep_table(jw.AC_SYMBOLS[::-1])}
    lv = _grid(_value_levels(), 7, 7)
    return _mk(hw._write("val_extremes", 56, 56, S444, [lv, lv.copy(), lv.copy()], ONES, [0, 1, 1],
                         dht, [0, 1, 1], [0, 1, 1], restart_interval=1), dht)


def _kinds(table, used, is_dc):
    """Symbol -> does a level-1 / sub-table entry hold its value (Full) or the
    code alone (Code): lut_kernel's rule, code + value bits within the level."""
    codes = jw.canonical_codes(*table)
    out = {}
    for sym in used:
        length = codes[sym][1]
        size = sym if is_dc else sym & 15
        out[sym] = "full" if length + size <= (LUT_BITS if length <= LUT_BITS else 16) else "code"
    return out


def test_value_stream_holds_every_extreme(oracle):
    s = _value_stream()
    _, levels = oracle.decode_coefs(s.data)
    for c in range(3):
        flat = levels[c].reshape(-1, 64).astype(np.int64)
        for sz in range(1, 12):
            for v in _extremes(sz):
                assert (flat[:, 0] == v).any(), (c, "dc", v)
                if sz <= 10:  # (natural index 1 = zig-zag 1)
                    assert (flat[:, 1:] == v).any(), (c, "ac", v)
        assert (flat[:45, 0] == 0).any()
    for cls in ("dc", "ac"):
        a = _kinds(s.dht[(cls, 0)], s.stats[(cls, 0)], cls == "dc")
        b = _kinds(s.dht[(cls, 1)], s.stats[(cls, 1)], cls == "dc")
        assert set(a) == set(b)
        assert any(a[sym] == "full" and b[sym] == "code" for sym in a), cls


# ---- block ends --------------------------------------------------------------------

def _eob_levels():
    """Block j = 1..63: its EOB comes at z = j (the last non-zero level at j -
    1); even j dense up to there, odd j one level (ZRLs and a run)."""
    lv = []
    for j in range(1, 64):
        b = np.zeros(64, np.int32)
        b[0] = j % 7 - 3
        if j > 1:
            if j % 2 == 0:
                b[1:j] = np.where(np.arange(j - 1) % 2, 2, -1)
            else:
                b[j - 1] = 3 if j % 4 == 1 else -2
        lv.append(b)
    dense = np.zeros(64, np.int32)
    dense[1:] = np.where(np.arange(63) % 3, 1, -2)  # 63 non-zero ACs
    lv.append(dense)
    return np.array(lv)


_ZRL = ("ac", jw.ZRL, 0, 0)


def _zrl_levels():
    """Blocks whose ZRLs (in place of the EOB) end them at exactly z = 64, a
    coefficient at 63 after three ZRLs, and ordinary blocks between them."""
    lv, ex = [], {}
    rng = np.random.default_rng(3)
    for j in range(32):
        b = np.zeros(64, np.int32)
        b[0] = j % 9 - 4
        if j % 4 == 0:  # z: 16 -> 32 -> 48 -> 64
            b[15] = 2
            ex[(0, j // 8, j % 8)] = [_ZRL] * 3
        elif j % 4 == 1:  # z: 48 -> 64
            b[3], b[47] = -1, 5
            ex[(0, j // 8, j % 8)] = [_ZRL]
        elif j % 4 == 2:  # run 62 = three ZRLs and run 14, no EOB
            b[63] = 1 + j % 3
        else:
            b[rng.integers(1, 30, size=4)] = rng.integers(-5, 6, size=4)
        lv.append(b)
    return np.array(lv), ex


def _with_refused():
    """deep_table over the AC alphabet and the size-0 symbol 0x30, which no
    decoder accepts."""
    return jw.deep_table(jw.AC_SYMBOLS + [0x30])


@functools.lru_cache(maxsize=None)
def _end_stream(key):
    std = {("dc", 0): jw.std_tables()[("dc", 0)], ("ac", 0): jw.std_tables()[("ac", 0)]}
    if key == "eob_every_z":
        return _mk(_gray("end_" + key, _eob_levels(), 8, 8, std), std)
    if key == "zrl_to_64":
        lv, ex = _zrl_levels()
        return _mk(_gray("end_" + key, lv, 4, 8, std, extra_symbols=ex), std)
    # the error streams and their twins: 32 ordinary blocks, block 21 ends in
    # the symbol (twin: in its EOB)
    rng = np.random.default_rng(11)
    lv = np.zeros((32, 64), np.int32)
    lv[:, 0] = rng.integers(-20, 21, size=32)
    for j in range(32):
        lv[j, rng.integers(1, 40, size=5)] = rng.integers(-7, 8, size=5)
    lv[21, 1:] = 0
    lv[21, 60] = 1
    dht = {("dc", 0): std[("dc", 0)], ("ac", 0): _with_refused()}
    ex = None
    if key == "run_past_63":  # z = 61, run 5: the coefficient would land at 66
        ex = {(0, 21 // 8, 21 % 8): [("ac", (5 << 4) | 1, 1, 1)]}
    elif key == "refused_size0":
        ex = {(0, 21 // 8, 21 % 8): [("ac", 0x30, 0, 0)]}
    else:
        assert key == "twin"
    return _mk(_gray("end_" + key, lv, 4, 8, dht, extra_symbols=ex), dht)


END_KEYS = ["eob_every_z", "zrl_to_64", "twin"]
ERROR_KEYS = ["run_past_63", "refused_size0"]


def test_end_streams_are_as_listed(oracle):
    _, levels = oracle.decode_coefs(_end_stream("eob_every_z").data)
    zz = levels[0].reshape(-1, 64)[:, jw.NATURAL]  # back to zig-zag order
    last = [int(np.nonzero(b[1:])[0][-1]) + 2 if b[1:].any() else 1 for b in zz[:63]]
    assert last == list(range(1, 64))  # the z at which each block's EOB is read
    assert (zz[63, 1:] != 0).all()
    s = _end_stream("zrl_to_64")
    assert s.stats[("ac", 0)][jw.ZRL] >= 8 * 3 + 8 * 1 + 8 * 3
    oracle.decode_coefs(s.data)
    oracle.decode_coefs(_end_stream("twin").data)
    for key in ERROR_KEYS:
        with pytest.raises(oracle.OracleError) as e:
            oracle.decode_coefs(_end_stream(key).data)
        assert e.value.code == BAD_HUFFMAN, key


# ---- MCU order ---------------------------------------------------------------------

ORDER_CASES = {
    # name: (w, h, sampling, table ids per component, restart interval)
    "420_std": (40, 24, [(2, 2), (1, 1), (1, 1)], [0, 1, 1], 0),
    "420_one_pair_ri1": (40, 24, [(2, 2), (1, 1), (1, 1)], [0, 0, 0], 1),
    "422_std_row": (40, 24, [(2, 1), (1, 1), (1, 1)], [0, 1, 1], 3),       # 3 MCUs to a row
    "444_one_pair": (24, 16, S444, [0, 0, 0], 0),
    "444_std_ri1": (24, 16, S444, [0, 1, 1], 1),
    "411_std_row": (64, 16, hw.SAMPLINGS["411"], [0, 1, 1], 2),            # 2 MCUs to a row
    "gray_row": (40, 24, GRAY, [0], 5),                                    # 5 blocks to a row
    "22_21_std": (40, 24, hw.SAMPLINGS["22_21"], [0, 1, 1], 0),            # 8 blocks per MCU
    "410_std_ri1": (64, 32, hw.SAMPLINGS["410"], [0, 1, 1], 1),            # 10 blocks per MCU
}


@functools.lru_cache(maxsize=None)
def _order_stream(name):
    if name == "gray_2bit_segments":  # 2-bit blocks, one to a restart segment
        dht = jw.short_table()
        lv = np.zeros((6, 64), np.int32)
        return _mk(_gray("ord_" + name, lv, 2, 3, dht, restart_interval=1), dht)
    w, h, samp, ids, ri = ORDER_CASES[name]
    rng = np.random.default_rng(600 + list(ORDER_CASES).index(name))
    levels = hw.moderate_levels(rng, hw._grid_shapes(w, h, samp))
    std = jw.std_tables()
    dht = {k: v for k, v in std.items() if k[1] in ids}
    return _mk(hw._write("ord_" + name, w, h, samp, levels, hw._small_q(rng, (0, 1)), ids, dht, ids,
                         ids, restart_interval=ri), dht)


ORDER_KEYS = list(ORDER_CASES) + ["gray_2bit_segments"]


def test_order_streams_are_as_listed(oracle):
    bpm = {}
    for name in ORDER_KEYS:
        s = _order_stream(name)
        info = oracle.parse(s.data)
        bpm[name] = info.bpm
        oracle.decode_coefs(s.data)
    assert [bpm[n] for n in ORDER_KEYS] == [6, 6, 4, 3, 3, 6, 1, 8, 10, 1]
    d = _order_stream("gray_2bit_segments").data
    scan = d[d.index(b"\xff\xda"):]
    assert scan.count(b"\xff\xd0") + scan.count(b"\xff\xd1") >= 2 and len(scan) < 14 + 6 * 3 + 2


# ---- slot edges --------------------------------------------------------------------

SHIFTS = range(6, 38)  # AC bits of the first block: 3 a + 4 b


def _first_block(m):
    """A block of DC 0 whose AC symbols take m bits of the Annex K luminance
    table besides the EOB: (0, 1) is 3 bits with its value, (0, 2) 4."""
    b4 = next(b for b in range(m // 4 + 1) if (m - 4 * b) % 3 == 0)
    a3 = (m - 4 * b4) // 3
    blk = np.zeros(64, np.int32)
    blk[1:1 + a3] = np.where(np.arange(a3) % 2, 1, -1)
    blk[1 + a3:1 + a3 + b4] = np.where(np.arange(b4) % 2, 2, -3)
    return blk


@functools.lru_cache(maxsize=None)
def _shift_stream(m):
    std = {("dc", 0): jw.std_tables()[("dc", 0)], ("ac", 0): jw.std_tables()[("ac", 0)]}
    rng = np.random.default_rng(77)  # the same 63 blocks behind every first block
    rest = hw.moderate_levels(rng, [(1, 63)], ac=40, nnz=12)[0].reshape(63, 64)
    lv = np.concatenate([_first_block(m)[None], rest])
    return _mk(_gray(f"shift_{m}", lv, 8, 8, std), std)


def test_shift_streams_cover_every_offset():
    """The first block of stream m is m bits longer than DC 0 + EOB, the rest
    of the scan is the same symbols: 32 consecutive shifts, so each symbol
    that crosses a multiple of 384 bits does so at every bit offset, and the
    scan spans several slots."""
    std_ac = jw.canonical_codes(*jw.std_tables()[("ac", 0)])
    assert std_ac[0x01][1] + 1 == 3 and std_ac[0x02][1] + 2 == 4
    for m in SHIFTS:
        s = _shift_stream(m)
        st = s.stats[("ac", 0)]
        base = _shift_stream(6).stats[("ac", 0)]
        extra = 3 * (st[0x01] - base[0x01]) + 4 * (st[0x02] - base[0x02])
        assert extra == m - 6, m
    assert len(set(SHIFTS)) == 32 and max(SHIFTS) - min(SHIFTS) == 31
    d = _shift_stream(6).data
    assert (len(d) - d.index(b"\xff\xda")) * 8 > 4 * 384


# ---- list groups -------------------------------------------------------------------

GROUP_COUNTS = [0, 1, 2, 3, 4, 5, 63]  # sum 78 = 2 mod 4: over two periods every start offset


@functools.lru_cache(maxsize=None)
def _group_stream():
    std = {("dc", 0): jw.std_tables()[("dc", 0)], ("ac", 0): jw.std_tables()[("ac", 0)]}
    lv = np.zeros((61, 64), np.int32)  # the last period stops short: a partial last group
    for j in range(61):
        n = GROUP_COUNTS[j % 7]
        ks = 1 + np.random.default_rng(900 + j).choice(63, size=n, replace=False)
        for k in ks:
            lv[j, k] = (1 + (5 * j + 3 * int(k)) % 6) * (-1 if (j + int(k)) % 2 else 1)
        lv[j, 0] = (j * 29) % 61 - 30
    return _mk(_gray("groups", lv, 8, 8, std), std)


def test_group_counts_are_as_listed(oracle):
    ref, _ = oracle.decode_coefs(_group_stream().data)
    got = (ref[:, 1:] != 0).sum(axis=1)
    assert got[:61].tolist() == [GROUP_COUNTS[j % 7] for j in range(61)]
    assert got[:61].sum() % 4 != 0 and not got[61:].any()


# ---- the GPU checks ----------------------------------------------------------------

ALL = ([("length", k) for k in LENGTH_KEYS] + [("value", None)] + [("end", k) for k in END_KEYS]
       + [("order", k) for k in ORDER_KEYS] + [("groups", None)])


def _stream(family, key):
    return {"length": _length_stream, "end": _end_stream, "order": _order_stream,
            "value": lambda _: _value_stream(), "groups": lambda _: _group_stream()}[family](key)


def test_every_stream_decodes_on_the_oracle(oracle):
    """The oracle's own decode returns the levels that were written."""
    streams = [_stream(f, k) for f, k in ALL] + [_shift_stream(m) for m in SHIFTS]
    for s in streams:
        _, levels = oracle.decode_coefs(s.data)
        for got, want in zip(levels, s.stream.natural_levels()):
            np.testing.assert_array_equal(got, want.astype(np.int16), strict=True, err_msg=s.stream.name)
        oracle.decode_planes(s.data)


@pytest.fixture(scope="module")
def fine_decoder(decoder):
    """32-bit subsequences, 128 entropy threads (as test_gpu_handwritten)."""
    from spdl_amd._lib import Decoder

    dec = Decoder(0)
    dec.set_param("sub_bits", 32)
    dec.set_param("entropy_threads", 128)
    yield dec
    dec.close()


@pytest.fixture(params=[1, 4])
def lanes(decoder, request):
    prev = decoder.get_param("lanes")
    decoder.set_param("lanes", request.param)
    yield request.param
    decoder.set_param("lanes", prev)


def _between(decoder, oracle, datas, expect=None):
    """Each stream in one batch between q90_420 and gray, resized to 32 x 32:
    every image as the oracle's, or the status `expect` gives it."""
    import torch

    batch = [cases.case("q90_420")]
    mine = []
    for d in datas:
        mine.append(len(batch))
        batch += [d, cases.case("gray") if len(batch) % 4 == 1 else cases.case("q90_420")]
    out = Output(pix_fmt="rgb24", resize=True, **RESIZE32)
    t = torch.empty((len(batch), 32, 32, 3), dtype=torch.uint8, device="cuda:0")
    st = decoder.decode_batch(batch, out, t.data_ptr(), t.numel(),
                              stream=torch.cuda.current_stream(), check=False)
    hyp = t.cpu().numpy()
    want = [0] * len(batch)
    for i, code in zip(mine, expect or [0] * len(mine)):
        want[i] = code
    assert list(st) == want
    for i, d in enumerate(batch):
        if want[i] == 0:
            ref = oracle.decode_resize(d, oracle.Resize(**RESIZE32), pix_fmt="rgb24")
            np.testing.assert_array_equal(hyp[i], ref, strict=True, err_msg=f"image {i}")


@gpu
@pytest.mark.parametrize("family,key", ALL, ids=[f"{f}-{k}" if k else f for f, k in ALL])
def test_stream_alone(decoder, oracle, lanes, family, key):
    d = _stream(family, key).data
    check_coefs(decoder, oracle, d)
    check_planes(decoder, oracle, d)


@gpu
@pytest.mark.parametrize("family", ["length", "value", "end", "order", "groups"])
def test_streams_between_ordinary_images(decoder, oracle, lanes, family):
    _between(decoder, oracle, [_stream(f, k).data for f, k in ALL if f == family])


@gpu
@pytest.mark.parametrize("family,key", ALL, ids=[f"{f}-{k}" if k else f for f, k in ALL])
def test_stream_in_many_runs(fine_decoder, oracle, family, key):
    check_coefs(fine_decoder, oracle, _stream(family, key).data)


@gpu
def test_slot_edges_alone(decoder, oracle, lanes):
    for m in SHIFTS:
        check_coefs(decoder, oracle, _shift_stream(m).data)
    check_planes(decoder, oracle, _shift_stream(SHIFTS[0]).data)


@gpu
def test_slot_edges_between_ordinary_images(decoder, oracle, lanes):
    _between(decoder, oracle, [_shift_stream(m).data for m in SHIFTS])


@gpu
def test_slot_edges_in_many_runs(fine_decoder, oracle):
    for m in SHIFTS:
        check_coefs(fine_decoder, oracle, _shift_stream(m).data)


@gpu
@pytest.mark.parametrize("key", ERROR_KEYS)
def test_refused_symbols(decoder, fine_decoder, oracle, lanes, key):
    """The careful path takes over at the symbol: the oracle's status, alone
    (both decoders) and in a batch whose other images decode; the twin stream
    -- the same blocks, an EOB in the symbol's place -- is among ALL."""
    d = _end_stream(key).data
    for dec in (decoder, fine_decoder):
        _, _, diag = dec.debug_entropy(d, 32)
        assert diag["status"] == BAD_HUFFMAN, diag
    _between(decoder, oracle, [d, _end_stream("twin").data], expect=[BAD_HUFFMAN, 0])
