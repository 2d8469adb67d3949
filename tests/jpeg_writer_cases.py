"""The hand-written stream families (tests/jpeg_writer.py), shared by the CPU
tests (test_jpeg_writer.py) and the GPU parity tests (test_gpu_handwritten.py).

`case(name)` returns a `Stream`: the bytes, what was written (levels in
zig-zag order, tables, sampling) and the writer's symbol histogram.  Families:

  1  samplings        SAMPLING_CASES, REFUSED_CASES
  2  Huffman tables   TABLE_CASES
  3  coefficient extremes (deep tables)   EXTREME_CASES (+ per_component twins)
  4  block structure  STRUCTURE_CASES
  5  spectral selection (SOF2 without refinement)   PROGRESSIVE_CASES
  6  scan scripts (SOF2 with successive approximation, EOB runs, odd scan
     orders, streams libjpeg only warns about)   SCRIPT_CASES, SCRIPT_BAD

Families 1, 2, 4, 5 and most of 6 keep amplitudes small (CAPPED: at most 25 %
of the oracle's RGB samples at 0 or 255, asserted by the tests); family 3 and
SCRIPT_UNCAPPED saturate by nature or decode to other levels than were coded.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from tests import jpeg_writer as jw

SAMPLINGS = {
    "440": [(1, 2), (1, 1), (1, 1)],
    "411": [(4, 1), (1, 1), (1, 1)],
    "410": [(4, 2), (1, 1), (1, 1)],  # 10 blocks per MCU
    "1x4": [(1, 4), (1, 1), (1, 1)],
    "22_12": [(2, 2), (1, 2), (1, 2)],  # 4:2:2 spelt with doubled vertical factors
    "22_21": [(2, 2), (2, 1), (2, 1)],  # 4:4:0 spelt with doubled horizontal factors
    "gray22": [(2, 2)],  # one component declared 2x2: its factors mean nothing
}
# canonical spellings Pillow / libjpeg take as they are (every chroma factor 1)
CANONICAL = ("440", "411", "410", "1x4")

REFUSED = {
    "luma_under_chroma": dict(samp=[(1, 1), (2, 2), (2, 2)]),
    "3x1": dict(samp=[(3, 1), (1, 1), (1, 1)]),
    "chroma_unlike": dict(samp=[(2, 2), (2, 1), (1, 1)]),
    "over_10_blocks": dict(samp=[(4, 4), (1, 1), (1, 1)]),  # 18 blocks per MCU
    "four_comp_sampled": dict(samp=[(2, 2), (1, 1), (1, 1), (2, 2)]),
    "rgb_ids_sampled": dict(samp=[(2, 2), (1, 1), (1, 1)], comp_ids=(ord("R"), ord("G"), ord("B"), 4)),
}


@dataclass
class Stream:
    name: str
    data: bytes
    width: int
    height: int
    samp: list
    levels: list  # per component [bh, bw, 64], zig-zag order, as written
    qtables: dict
    tq: list
    pq: int = 0
    scans: str = "interleaved"
    stats: dict = field(default_factory=dict)
    restart_interval: int = 0
    script: list | None = None  # scans="script": the scan script
    expect: list | None = None  # the levels a decoder returns, where they differ from `levels`

    def natural_levels(self):
        """Per component [bh, bw, 64] in natural order (the oracle's layout):
        the levels a decoder returns."""
        out = []
        for lv in self.levels if self.expect is None else self.expect:
            nat = np.zeros_like(lv)
            nat[..., jw.NATURAL] = lv
            out.append(nat)
        return out


def _sizes(samp):
    """37x29 (partial MCUs on both axes), 70x29 when h = 4, and a size of at
    least 3x3 MCUs with partial ones."""
    hmax = max(h for h, _ in samp)
    vmax = max(v for _, v in samp)
    out = [(37, 29)]
    if hmax == 4:
        out.append((70, 29))
    out.append((min(3 * 8 * hmax + 5, 128), min(3 * 8 * vmax + 3, 128)))
    return out


def _grid_shapes(w, h, samp):
    return [g[0] for g in jw.block_grids(w, h, samp)]


def moderate_levels(rng, shapes, ac=12, dc=60, nnz=10, kmax=63):
    """Random levels small enough not to clamp at q <= 8: a bounded DC walk
    and `nnz` AC values of |v| <= ac per block, mostly at low frequencies."""
    out = []
    for bh, bw in shapes:
        lv = np.zeros((bh, bw, 64), np.int32)
        walk = np.cumsum(rng.integers(-dc // 3, dc // 3 + 1, size=bh * bw))
        lv[..., 0] = (np.abs((walk + dc) % (4 * dc) - 2 * dc) - dc).reshape(bh, bw)  # folded into +-dc
        for y in range(bh):
            for x in range(bw):
                k = np.minimum((rng.exponential(10.0, size=nnz)).astype(int) + 1, kmax)
                lv[y, x, k] = rng.integers(-ac, ac + 1, size=nnz)
        out.append(lv)
    return out


def _small_q(rng, ids, qmax=6):
    return {i: rng.integers(1, qmax + 1, size=64) for i in ids}


def _write(name, w, h, samp, levels, qtables, tq, dht, td, ta, **kw) -> Stream:
    stats: dict = {}
    data = jw.write_jpeg(w, h, samp, levels, qtables, tq, dht, td, ta, stats=stats, **kw)
    return Stream(name, data, w, h, samp, [np.asarray(x) for x in levels], qtables, list(tq),
                  pq=kw.get("pq", 0), scans=kw.get("scans", "interleaved"), stats=stats,
                  restart_interval=kw.get("restart_interval", 0))


def _std_ids(nc):
    return [0, 1, 1, 0][:nc]


# ---- family 1: samplings ----------------------------------------------------

def _sampling_case(key, w, h, ri) -> Stream:
    samp = SAMPLINGS[key]
    rng = np.random.default_rng(w * 1000 + h + list(SAMPLINGS).index(key))
    nc = len(samp)
    levels = moderate_levels(rng, _grid_shapes(w, h, samp))
    q = _small_q(rng, (0, 1))
    ids = _std_ids(nc)
    return _write(f"samp_{key}_{w}x{h}_ri{ri}", w, h, samp, levels, q, ids, jw.std_tables(), ids, ids,
                  restart_interval=ri)


SAMPLING_CASES = [f"samp_{k}_{w}x{h}_ri{ri}" for k, s in SAMPLINGS.items() for (w, h) in _sizes(s)
                  for ri in (0, 1)]


def _refused_case(key) -> Stream:
    spec = REFUSED[key]
    samp = spec["samp"]
    w, h = 37, 29
    rng = np.random.default_rng(5)
    nc = len(samp)
    levels = moderate_levels(rng, _grid_shapes(w, h, samp))
    ids = _std_ids(nc)
    return _write("refused_" + key, w, h, samp, levels, _small_q(rng, (0, 1)), ids, jw.std_tables(),
                  ids, ids, comp_ids=spec.get("comp_ids", (1, 2, 3, 4)))


REFUSED_CASES = ["refused_" + k for k in REFUSED]
# libjpeg's own conversion (csc="jfif": box-replicated components, no swscale
# frame format behind it) takes every factor that divides the largest one:
# the accepted samplings, and three of the layouts the default output refuses
JFIF_CASES = [n for n in SAMPLING_CASES if n.endswith("_ri0")] + [
    "refused_luma_under_chroma", "refused_3x1", "refused_chroma_unlike"]


# ---- family 2: tables -------------------------------------------------------

def all_symbol_levels(shape):
    """Levels of one component in which every DC category 0..15 and every AC
    symbol (EOB, ZRL, the 240 run/size pairs) occurs.  The large sizes come
    last and share as few blocks as possible, so most of the image stays
    unsaturated."""
    bh, bw = shape
    lv = np.zeros((bh * bw, 64), np.int32)
    rng = np.random.default_rng(17)
    b = 0
    # AC: the 16 runs of every size, packed greedily into blocks, small sizes first
    for s in range(1, 16):
        k = 1
        for r in range(16):
            if k + r > 63:
                b, k = b + 1, 1
            k += r
            mag = int(rng.integers(1 << (s - 1), 1 << s))
            lv[b, k] = mag if (r + s) % 2 else -mag
            k += 1
        b += 1
    # ZRL: a lone coefficient at k = 40 (two ZRLs); EOB occurs in most blocks
    lv[b, 40] = 3
    b += 1
    # DC categories 0..15 as differences: up by 2^(s-1) + a bit, then down
    dc = 0
    for s in list(range(0, 16)) + list(range(15, 0, -1)):
        d = 0 if s == 0 else int(rng.integers(1 << (s - 1), min(1 << s, 32768 - abs(dc))))
        dc = dc + d if dc <= 0 else dc - d
        lv[b, 0] = dc
        b += 1
    lv[b:, 0] = 0
    assert b <= bh * bw, "image too small for every symbol"
    # the rest: small texture so the unsaturated share is real content
    for j in range(b, bh * bw):
        lv[j, 0] = int(rng.integers(-40, 41))
        lv[j, rng.integers(1, 20, size=6)] = rng.integers(-8, 9, size=6)
    return lv.reshape(bh, bw, 64)


def _table_case(key) -> Stream:
    rng = np.random.default_rng(23)
    if key == "deep_all_symbols":  # gray, 128x128 = 256 blocks
        w = h = 128
        samp = [(1, 1)]
        levels = [all_symbol_levels(_grid_shapes(w, h, samp)[0])]
        dht = {("dc", 0): jw.deep_table(jw.DC_SYMBOLS), ("ac", 0): jw.deep_table(jw.AC_SYMBOLS)}
        return _write("tab_" + key, w, h, samp, levels, {0: np.ones(64, int)}, [0], dht, [0], [0])
    if key == "deep_all_symbols_reversed":  # the short codes go to the rare, large symbols
        w = h = 128
        samp = [(1, 1)]
        levels = [all_symbol_levels(_grid_shapes(w, h, samp)[0])]
        dht = {("dc", 0): jw.deep_table(jw.DC_SYMBOLS[::-1]),
               ("ac", 0): jw.deep_table(jw.AC_SYMBOLS[::-1])}
        return _write("tab_" + key, w, h, samp, levels, {0: np.ones(64, int)}, [0], dht, [0], [0],
                      restart_interval=7)
    if key == "flat":
        w, h, samp = 70, 29, SAMPLINGS["411"]
        levels = moderate_levels(rng, _grid_shapes(w, h, samp))
        dht = {("dc", 0): jw.flat_table(jw.DC_SYMBOLS), ("ac", 0): jw.flat_table(jw.AC_SYMBOLS),
               ("dc", 1): jw.flat_table(jw.DC_SYMBOLS, 16), ("ac", 1): jw.flat_table(jw.AC_SYMBOLS, 16)}
        return _write("tab_" + key, w, h, samp, levels, _small_q(rng, (0, 1)), [0, 1, 1], dht,
                      [0, 1, 1], [0, 1, 1])
    if key in ("short", "short_ri", "short_inverted_ones", "short_inverted_walk"):
        # gray 128x128: 256 blocks of 2 bits (16 blocks in a 32-bit subsequence)
        w = h = 128
        samp = [(1, 1)]
        lv = np.zeros((16, 16, 64), np.int32)
        inv = key.startswith("short_inverted")
        if key in ("short", "short_ri"):
            lv[..., 0] = 9  # one category-4 difference, then 2-bit blocks
        elif key == "short_inverted_walk":
            # categories 0 and 1 only: steps of -1 / 0 / +1, mostly 0
            steps = rng.choice([-1, 0, 0, 0, 0, 1], size=256)
            lv[..., 0] = np.clip(np.cumsum(steps), -30, 30).reshape(16, 16)
            d = np.diff(lv[..., 0].reshape(-1), prepend=0)
            assert np.abs(d).max() <= 1
        return _write("tab_" + key, w, h, samp, [lv], {0: np.full(64, 4)}, [0],
                      jw.short_table(inverted=inv), [0], [0],
                      restart_interval=48 if key == "short_ri" else 0)
    if key == "ids_2_3":
        w, h, samp = 37, 29, [(1, 1)] * 3
        levels = moderate_levels(rng, _grid_shapes(w, h, samp))
        std = jw.std_tables()
        dht = {("dc", 2): std[("dc", 0)], ("dc", 3): std[("dc", 1)],
               ("ac", 3): std[("ac", 0)], ("ac", 2): std[("ac", 1)]}
        q = _small_q(rng, (2, 3))
        return _write("tab_" + key, w, h, samp, levels, q, [3, 2, 2], dht, [2, 3, 3], [3, 2, 2])
    if key == "three_pairs_deep":
        w, h, samp = 37, 29, SAMPLINGS["22_21"]
        levels = moderate_levels(rng, _grid_shapes(w, h, samp))
        ac = jw.AC_SYMBOLS
        dht = {("dc", 0): jw.deep_table(jw.DC_SYMBOLS), ("ac", 2): jw.deep_table(ac),
               ("dc", 1): jw.deep_table(jw.DC_SYMBOLS[::-1]), ("ac", 0): jw.deep_table(ac[::-1]),
               ("dc", 2): jw.deep_table(jw.DC_SYMBOLS[8:] + jw.DC_SYMBOLS[:8]),
               ("ac", 1): jw.deep_table(ac[100:] + ac[:100])}
        q = _small_q(rng, (0, 1, 2))
        return _write("tab_" + key, w, h, samp, levels, q, [0, 1, 2], dht, [0, 1, 2], [2, 0, 1],
                      restart_interval=2)
    raise KeyError(key)


TABLE_KEYS = ["deep_all_symbols", "deep_all_symbols_reversed", "flat", "short", "short_ri",
              "short_inverted_ones", "short_inverted_walk", "ids_2_3", "three_pairs_deep"]
TABLE_CASES = ["tab_" + k for k in TABLE_KEYS]
# tables holding the all-ones code: outside what libjpeg (so Pillow) accepts
ALL_ONES_CODE = ("tab_short_inverted_ones", "tab_short_inverted_walk")


# ---- family 3: coefficient extremes -----------------------------------------

def _basis_signs(n):
    """Sign of the 8-point IDCT basis at output n for each frequency k."""
    return np.array([1 if np.cos((2 * n + 1) * k * np.pi / 16) >= 0 else -1 for k in range(8)])


def idct_worst_blocks():
    """Natural-order [n, 64] coefficient levels (q = 1): for every output
    (row, column) pair a block whose signs follow that output's basis signs at
    maximum magnitude, in both polarities (every partial sum of that output
    has one sign), and DC-only rows (only column 0 non-zero) whose row[0] << 3
    leaves int16."""
    out = []
    for r in range(8):
        for c in range(8):
            s = np.outer(_basis_signs(r), _basis_signs(c)).reshape(64)
            for pol in (1, -1):
                out.append(np.where(s * pol > 0, 32767, -32767))
    rng = np.random.default_rng(31)
    for i in range(16):
        blk = np.zeros(64, np.int64)
        mags = rng.integers(4096, 32768, size=8) * rng.choice([-1, 1], size=8)
        if i < 4:
            mags = np.array([32767, -32767][i % 2]).repeat(8) * (1 if i < 2 else _basis_signs(3))
        blk[0::8] = mags  # column 0: every row is DC-only
        out.append(blk)
    return np.array(out)


def _extreme_levels(key, rng, shapes):
    out = []
    for ci, (bh, bw) in enumerate(shapes):
        n = bh * bw
        lv = np.zeros((n, 64), np.int32)
        if key == "ac1023_q255":
            lv[:, 0] = rng.integers(-1023, 1024, size=n)
            mask = rng.random((n, 63)) < 0.3
            lv[:, 1:] = np.where(mask, rng.integers(-1023, 1024, size=(n, 63)), 0)
        elif key == "ac_sizes_11_15":
            for j in range(n):
                ks = rng.choice(np.arange(1, 64), size=8, replace=False)
                s = rng.integers(11, 16, size=8)
                mag = np.array([rng.integers(1 << (x - 1), 1 << x) for x in s])
                lv[j, ks] = mag * rng.choice([-1, 1], size=8)
            lv[:, 0] = rng.integers(-2000, 2001, size=n)
        elif key == "pq1":
            lv[:, 0] = rng.integers(-1023, 1024, size=n)
            mask = rng.random((n, 63)) < 0.25
            lv[:, 1:] = np.where(mask, rng.integers(-1023, 1024, size=(n, 63)), 0)
        elif key == "dense":
            v = rng.integers(1, 4, size=(n, 63)) * rng.choice([-1, 1], size=(n, 63))
            lv[:, 1:] = v
            lv[:, 0] = rng.integers(-100, 101, size=n)
        elif key == "dc_ramp":
            # +2047 per block for 16 blocks, -2047 for 32, +2047 for 16, ...: with
            # q = 255 the dequantised DC passes +-32767 after one step and stays there
            step = np.where((np.arange(n) // 16 + 1) // 2 % 2 == 0, 2047, -2047)
            lv[:, 0] = np.cumsum(step)
            assert np.abs(lv[:, 0]).max() <= 32767
        elif key == "dc_cat15":
            big = rng.integers(16384, 32768, size=n)
            dc = np.zeros(n, np.int64)
            cur = 0
            for j in range(n):
                d = int(big[j]) if j % 3 else int(rng.integers(-500, 501))
                cur = cur - d if cur > 0 else cur + d
                cur = max(min(cur, 32767), -32768)
                dc[j] = cur
            lv[:, 0] = dc
            lv[:, 5] = rng.integers(-3, 4, size=n)
        elif key == "idct_worst":
            blocks = idct_worst_blocks()
            nat = np.zeros((n, 64), np.int64)
            m = min(n, len(blocks))
            # each component takes the blocks from another offset
            nat[:m] = np.roll(blocks, 37 * ci, axis=0)[:m]
            lv[:] = nat[:, jw.NATURAL]  # zig-zag k holds natural NATURAL[k]
            # DC: the restart interval is 1, so every difference is the level
            # itself; +31743 dequantises to 32767 (q = 1, bias 1024)
            worst = np.arange(n) < min(m, 128)
            lv[:, 0] = np.where(worst & (lv[:, 0] > 0), 31743, lv[:, 0])
        else:
            raise KeyError(key)
        out.append(lv.reshape(bh, bw, 64))
    return out


EXTREME_KEYS = ["ac1023_q255", "ac_sizes_11_15", "pq1", "dense", "dc_ramp", "dc_cat15", "idct_worst"]


def _extreme_case(key, scans) -> Stream:
    rng = np.random.default_rng(41 + EXTREME_KEYS.index(key))
    if key == "idct_worst":
        w, h, samp = 96, 96, [(1, 1)] * 3  # 144 blocks per component: one per worst case
    elif key in ("dc_ramp", "dc_cat15"):
        w, h, samp = 128, 29, SAMPLINGS["411"]  # 64 luma blocks: a whole ramp period
    else:
        w, h, samp = 37, 29, [(2, 1), (1, 1), (1, 1)]
    nc = len(samp)
    shapes = _grid_shapes(w, h, samp)
    if scans == "per_component":
        own = [g[1] for g in jw.block_grids(w, h, samp)]
        levels = []
        for full, part, lv in zip(shapes, own, _extreme_levels(key, rng, own)):
            pad = np.zeros(full + (64,), np.int32)
            pad[:part[0], :part[1]] = lv
            levels.append(pad)
    else:
        levels = _extreme_levels(key, rng, shapes)
    pq = 1 if key == "pq1" else 0
    if key in ("ac1023_q255", "dc_ramp"):
        q = {0: np.full(64, 255), 1: np.full(64, 255)}
    elif key == "pq1":
        q = {0: rng.integers(1, 65536, size=64), 1: rng.integers(256, 65536, size=64)}
    elif key == "ac_sizes_11_15":
        q = {0: rng.integers(1, 256, size=64), 1: rng.integers(1, 256, size=64)}
    elif key == "dense":
        q = _small_q(rng, (0, 1), 4)
    else:
        q = {0: np.ones(64, int), 1: np.ones(64, int)}
    dht = {("dc", 0): jw.deep_table(jw.DC_SYMBOLS), ("ac", 0): jw.deep_table(jw.AC_SYMBOLS),
           ("dc", 1): jw.deep_table(jw.DC_SYMBOLS[::-1]), ("ac", 1): jw.deep_table(jw.AC_SYMBOLS[::-1])}
    ids = _std_ids(nc)
    ri = 5 if key in ("dc_ramp", "dc_cat15") else 1 if key == "idct_worst" else 0
    tag = "" if scans == "interleaved" else "_pc"
    return _write(f"ext_{key}{tag}", w, h, samp, levels, q, ids, dht, ids, ids, pq=pq, scans=scans,
                  restart_interval=ri)


EXTREME_CASES = [f"ext_{k}{t}" for k in EXTREME_KEYS for t in ("", "_pc")]


# ---- family 4: block structure ----------------------------------------------

def _structure_case(key) -> Stream:
    rng = np.random.default_rng(53)
    w, h, samp = 37, 29, [(2, 2), (1, 1), (1, 1)]
    shapes = _grid_shapes(w, h, samp)
    levels = moderate_levels(rng, shapes, kmax=30)
    q = _small_q(rng, (0, 1))
    ids = _std_ids(3)
    kw: dict = {}
    dht = jw.std_tables()
    if key == "k63_no_eob":
        # a coefficient at k = 63 (no EOB follows) after 0, 1, 2 and 3 ZRLs
        for lv in levels:
            flat = lv.reshape(-1, 64)
            for j in range(len(flat)):
                z = j % 4
                flat[j, 1:] = 0
                flat[j, 63] = 2 + j % 5
                prev = 63 - 16 * z - 1 - (j % 7 if z < 3 else 0)
                if z < 3:  # dense up to `prev`, so the only long run is the last one
                    flat[j, 1:prev + 1] = np.where(np.arange(prev) % 2, 1, -1)
                # z == 3: the run from k = 1 is 62 = 3 ZRLs + run 14
    elif key == "zrl_overshoot":
        # ZRL symbols carrying k past 63 in place of the EOB
        ex = {}
        zrl = ("ac", jw.ZRL, 0, 0)
        for c, lv in enumerate(levels):
            bh, bw = lv.shape[:2]
            for y in range(bh):
                for x in range(bw):
                    j = y * bw + x
                    if j % 3 == 0:
                        lv[y, x, 41:] = 0
                        lv[y, x, 40] = 4
                        ex[(c, y, x)] = [zrl, zrl]  # k: 41 -> 57 -> 73
                    elif j % 3 == 1:
                        lv[y, x, 56:] = 0
                        lv[y, x, 55] = -2
                        ex[(c, y, x)] = [zrl]  # k: 56 -> 72
                    elif j % 7 == 2:
                        lv[y, x, 1:] = 0
                        ex[(c, y, x)] = [zrl] * 4  # k: 1 -> 65
        kw["extra_symbols"] = ex
    elif key == "rst_fill_1":
        kw.update(restart_interval=2, rst_fill=1)
    elif key == "rst_fill_3":
        kw.update(restart_interval=1, rst_fill=3)
    elif key == "ri_is_mcu_count":
        kw.update(restart_interval=3 * 2)  # 37x29 at 2x2: 3 x 2 MCUs
    elif key == "ri_65535":
        kw.update(restart_interval=65535)
    elif key == "dri_zero":
        kw.update(emit_dri=True)
    elif key == "single_table_segments":
        kw.update(table_segments="single")
    else:
        raise KeyError(key)
    return _write("blk_" + key, w, h, samp, levels, q, ids, dht, ids, ids, **kw)


STRUCTURE_KEYS = ["k63_no_eob", "zrl_overshoot", "rst_fill_1", "rst_fill_3", "ri_is_mcu_count",
                  "ri_65535", "dri_zero", "single_table_segments"]
STRUCTURE_CASES = ["blk_" + k for k in STRUCTURE_KEYS]


# ---- family 5: spectral selection (SOF2, Ah = Al = 0, EOBRUN 0) -------------

PROGRESSIVE = {
    # key: (w, h, sampling, bands, restart interval, deep tables)
    "420": (37, 29, [(2, 2), (1, 1), (1, 1)], ((1, 5), (6, 63)), 0, False),
    "411_ri2": (70, 29, SAMPLINGS["411"], ((1, 1), (2, 20), (21, 63)), 2, False),
    "410_one_band": (70, 29, SAMPLINGS["410"], ((1, 63),), 0, False),
    "gray22_ri1": (53, 51, SAMPLINGS["gray22"], ((1, 5), (6, 63)), 1, False),
    "440_deep": (29, 51, SAMPLINGS["440"], ((1, 9), (10, 62), (63, 63)), 0, True),
}


def _progressive_case(key) -> Stream:
    w, h, samp, bands, ri, deep = PROGRESSIVE[key]
    rng = np.random.default_rng(61 + list(PROGRESSIVE).index(key))
    grids = jw.block_grids(w, h, samp)
    levels = moderate_levels(rng, [g[0] for g in grids])
    for lv, (_, own) in zip(levels, grids):  # AC scans cover the own grid only
        lv[own[0]:, :, 1:] = 0
        lv[:, own[1]:, 1:] = 0
        lv[::2, ::2, 63] = 2  # the last band's last coefficient: no EOB there
        lv[own[0]:, :, 63] = 0
        lv[:, own[1]:, 63] = 0
    if deep:
        dht = {("dc", 0): jw.deep_table(jw.DC_SYMBOLS), ("ac", 0): jw.deep_table(jw.AC_SYMBOLS),
               ("dc", 1): jw.deep_table(jw.DC_SYMBOLS[::-1]),
               ("ac", 1): jw.deep_table(jw.AC_SYMBOLS[::-1])}
    else:
        dht = jw.std_tables()
    ids = _std_ids(len(samp))
    return _write("prog_" + key, w, h, samp, levels, _small_q(rng, (0, 1)), ids, dht, ids, ids,
                  scans="spectral", bands=bands, restart_interval=ri)


PROGRESSIVE_CASES = ["prog_" + k for k in PROGRESSIVE]


# ---- family 6: scan scripts (SOF2 with successive approximation) -------------
#
# What each stream holds, counted by the writer (stats["scans"]): scans / AC
# refinement scans / deepest Al / EOBn categories in AC first and in AC
# refinement scans / longest correction-bit field / fields over 15 bits (the
# kernel's ms_take_corr_long) / correction bits of blocks inside EOB runs /
# the reader multiscan_kernel gives the scans by its rule (a restart interval:
# the stuffed reader; else the word reader over the destuffed copy).
#
#   deep_al               21 12  5  0        0         17    1     0  word
#   al13                  18  3 13  0        0..1      20    9    77  word
#   dense_history          7  3  1  0        1         63   60  1302  word
#   dense_history_17       7  3  1  -        0         17  141     0  word
#   eob_runs               3  1  1  0..8     0..8       2    0    16  word
#   eob_runs_cap1          3  1  1  0..1     0..1       2    0     8  word
#   eob_run_14             5  2  1  3,4,9..14 3,4,9..14 1    0     0  word
#   eob_restart_ri5        3  1  1  0..2     0..2       2    0    14  stuffed
#   eob_restart_ri64       3  1  1  0..6     0..6       2    0    16  stuffed
#   eob_restart_fill2      3  1  1  0..2     0..2       2    0    14  stuffed
#   band_split            13  9  1  0        0..3       7    0   107  word
#   band_merge            13  3  1  0..2     0..1       8    0     5  word
#   band_merge_ri3        13  3  1  0..1     0          7    0     0  stuffed
#   dc_per_component      12  0  1  0        -          0    0     0  word
#   order                 10  4  1  0        0,1,3      6    0    47  word
#   refine_tables          8  4  2  0        0..1       8    0    15  word
#   all_ones               3  1  1  -        0..1      63   32    63  word
#   all_ones_ri4           3  1  1  0        0         63   29     0  stuffed
#   scans_64 / scans_65   64 / 65 one-coefficient bands, no refinement of AC
#   repeat_refine          8  4  1  0        0,1,4     12    0   176  word
#   overlap_first          5  0  0  0        -          0    0     0  word
#   overlap_first_long     3  0  0  0,2      -          0    0     0  word
#   zrl_overshoot_refine   7  3  1  0        0          7    0     0  word
#
# deep_al keeps Annex K's tables, which hold no EOBn above EOB0, so its blocks
# close one by one; the streams with EOB runs use jw.ranked_table.

# the alphabet of an AC refinement scan: EOB0..EOB14, ZRL, (r, 1) for r = 0..15
REFINE_SYMBOLS = [n << 4 for n in range(15)] + [jw.ZRL] + [(r << 4) | 1 for r in range(16)]

S420 = [(2, 2), (1, 1), (1, 1)]
RUNS = {"eobrun": "max"}


def _dc_chain(comps, al, **opt):
    """A DC first scan at `al`, then one refinement per bit down to 0."""
    return [(comps, 0, 0, 0, al, opt)] + [(comps, 0, 0, a + 1, a, opt) for a in range(al - 1, -1, -1)]


def _ac_chain(c, ss, se, al, **opt):
    return [([c], ss, se, 0, al, opt)] + [([c], ss, se, a + 1, a, opt) for a in range(al - 1, -1, -1)]


def sa_levels(rng, grids, dc_al, ac_al, ac=3, dc=20, nnz=8, late=0.1, dc_own=False):
    """moderate_levels scaled for successive approximation: every value moves
    up by the deepest Al of its chain (so the first scans still code it) and
    takes random low bits, which the refinement scans correct; a share `late`
    of the zero AC coefficients holds low bits alone and turns non-zero in a
    refinement scan.  AC levels cover the component's own grid (the AC scans'),
    DC levels the padded one unless `dc_own`."""
    out = []
    base = moderate_levels(rng, [g[0] for g in grids], ac=ac, dc=dc, nnz=nnz)
    for lv, (_, own) in zip(base, grids):
        a = lv[..., 1:]
        mag = np.abs(a)
        sign = np.where(a < 0, -1, np.where(a > 0, 1, rng.choice([-1, 1], size=a.shape)))
        low = rng.integers(0, 1 << ac_al, size=a.shape)
        mag = np.where(mag > 0, (mag << ac_al) | low, np.where(rng.random(a.shape) < late, low, 0))
        lv[..., 1:] = sign * mag
        lv[..., 0] = (lv[..., 0] << dc_al) | rng.integers(0, 1 << dc_al, size=lv.shape[:2])
        lv[own[0]:, :, 1:] = 0
        lv[:, own[1]:, 1:] = 0
        if dc_own:
            lv[own[0]:, :, 0] = 0
            lv[:, own[1]:, 0] = 0
        out.append(lv)
    return out


def _starts(lengths):
    return [int(x) for x in np.cumsum([0] + list(lengths[:-1]))]


# run lengths (the block that holds the EOBn included) of eob_runs' 576 blocks:
# every category 0..8, blocks coded at 63, 64 and 65 (either side of the first
# 64-block chunk boundary), the long runs across several boundaries
_EOB_FIRST = [63, 1, 1, 256, 128, 2, 4, 8, 16, 64, 33]
_EOB_REFINE = [1, 2, 4, 8, 16, 33, 1, 64, 128, 256, 63]
# eob_run_14's 16 512 blocks, band 1-5: category 14 between two coded blocks;
# band 6-63: categories 13 down to 9
_EOB14_A = [10, 16384 + 100, 18]
_EOB14_B = [8192, 4096, 2048, 1024, 512, 640]


def _eob_levels(rng, nblk, bands):
    """[nblk, 64]: per (ss, first-scan run lengths, refinement run lengths) the
    blocks that start a run hold, in the first scan, values of magnitude 2 or
    3 (coded at Al = 1; a correction bit in the refinement), in the
    refinement scan new +-1; every other block is empty in the band.  The
    first scan's blocks lie inside the refinement's runs."""
    lv = np.zeros((nblk, 64), np.int32)
    for ss, first, refine in bands:
        assert sum(first) == nblk and sum(refine) == nblk
        for b in _starts(first):
            lv[b, [ss, ss + 2]] = rng.choice([-3, -2, 2, 3], size=2)
        for b in _starts(refine):
            lv[b, [ss + 1, ss + 4]] = rng.choice([-1, 1], size=2)
    return lv


def _script_case(key) -> Stream:
    rng = np.random.default_rng(71 + SCRIPT_KEYS.index(key))
    w, h, samp = 37, 29, S420
    dht = jw.std_tables()
    if key not in ("deep_al", "dc_per_component", "scans_64", "scans_65", "refine_tables"):
        # scans with EOB runs: Annex K's AC tables hold no EOBn above EOB0
        syms = jw.progressive_ac_symbols()
        dht.update({("ac", 0): jw.ranked_table(syms), ("ac", 1): jw.ranked_table(syms, share=8)})
    kw: dict = {}
    expect = None
    q = None

    def grids_of():
        return jw.block_grids(w, h, samp)

    if key == "deep_al":
        levels = sa_levels(rng, grids_of(), 5, 4)
        script = _dc_chain([0, 1, 2], 5) + [e for c in range(3) for e in _ac_chain(c, 1, 63, 4)]
        q = {0: np.ones(64, int), 1: np.ones(64, int)}
    elif key == "al13":
        w, h, samp = 24, 16, [(1, 1)]
        lv = np.zeros((2, 3, 64), np.int32)
        lv[..., 0] = rng.integers(-32767, 32768, size=(2, 3))
        lv[..., 1:21] = 1024 * rng.integers(-31, 32, size=(2, 3, 20))
        lv[0, 0, 1:4] = [31744, -31744, 8192]
        levels = [lv]
        script = _dc_chain([0], 13) + [([0], 1, 20, 0, 13, RUNS)] + [
            ([0], 1, 20, a + 1, a, RUNS) for a in (12, 11, 10)]
        q = {0: np.ones(64, int)}
    elif key in ("dense_history", "dense_history_17"):
        samp = [(1, 1)] * 3
        levels = sa_levels(rng, grids_of(), 0, 0)
        for lv in levels:
            flat = lv.reshape(-1, 64)
            n = len(flat)
            flat[:, 1:] = rng.choice([-3, -2, 2, 3], size=(n, 63))
            for j in range(n):
                if key == "dense_history":  # 63 bits after EOB / 62 after EOB / 62 after (0, 1)
                    if j % 3:
                        flat[j, 63] = 0 if j % 3 == 1 else (-1) ** j
                else:  # fields of 15, 16 and 17 bits between new coefficients
                    flat[j, [(17, 34, 51), (16, 34, 52), (18, 34, 51)][j % 3]] = rng.choice([-1, 1], size=3)
        for lv, (_, own) in zip(levels, grids_of()):
            lv[own[0]:, :, 1:] = 0
            lv[:, own[1]:, 1:] = 0
        script = [([0, 1, 2], 0, 0, 0, 0)] + [e for c in range(3) for e in _ac_chain(c, 1, 63, 1, **RUNS)]
        q = {0: np.ones(64, int), 1: np.ones(64, int)}
    elif key.startswith("eob_runs") or key.startswith("eob_restart"):
        w, h, samp = 192, 192, [(1, 1)]
        lv = _eob_levels(rng, 576, [(1, _EOB_FIRST, _EOB_REFINE)])
        lv[:, 0] = moderate_levels(rng, [(24, 24)])[0][..., 0].reshape(-1)
        levels = [lv.reshape(24, 24, 64)]
        opt = {"eobrun": 1} if key == "eob_runs_cap1" else RUNS
        script = [([0], 0, 0, 0, 0), ([0], 1, 63, 0, 1, opt), ([0], 1, 63, 1, 0, opt)]
        q = {0: np.full(64, 3)}
        if key.startswith("eob_restart"):
            kw.update({"ri5": dict(restart_interval=5), "ri64": dict(restart_interval=64),
                       "fill2": dict(restart_interval=5, rst_fill=2)}[key.rsplit("_", 1)[1]])
    elif key == "eob_run_14":
        w, h, samp = 1032, 1024, [(1, 1)]
        lv = _eob_levels(rng, 129 * 128, [(1, _EOB14_A, _EOB14_A), (6, _EOB14_B, _EOB14_B)])
        lv[::97, 0] = rng.integers(-60, 61, size=len(lv[::97]))
        levels = [lv.reshape(128, 129, 64)]
        script = [([0], 0, 0, 0, 0), ([0], 1, 5, 0, 1, RUNS), ([0], 6, 63, 0, 1, RUNS),
                  ([0], 1, 5, 1, 0, RUNS), ([0], 6, 63, 1, 0, RUNS)]
        q = {0: np.full(64, 3)}
    elif key in ("band_split", "band_merge", "band_merge_ri3"):
        levels = sa_levels(rng, grids_of(), 0, 1, ac=5)
        bands = ((1, 5), (6, 20), (21, 63))
        script = [([0, 1, 2], 0, 0, 0, 0)]
        for c in range(3):
            if key == "band_split":
                script += [([c], 1, 63, 0, 1, RUNS)] + [([c], a, b, 1, 0, RUNS) for a, b in bands]
            else:
                script += [([c], a, b, 0, 1, RUNS) for a, b in bands] + [([c], 1, 63, 1, 0, RUNS)]
        if key == "band_merge_ri3":
            kw.update(restart_interval=3)
    elif key == "dc_per_component":
        w, h, samp = 70, 29, SAMPLINGS["411"]
        levels = sa_levels(rng, grids_of(), 1, 0, ac=10, dc_own=True)
        script = [([c], 0, 0, 0, 1) for c in (1, 2, 0)] + [([c], 0, 0, 1, 0) for c in (1, 2, 0)]
        script += [([c], a, b, 0, 0) for c in range(3) for a, b in ((1, 5), (6, 63))]
    elif key == "order":
        levels = sa_levels(rng, grids_of(), 1, 1, ac=5)
        script = _ac_chain(2, 1, 63, 1, **RUNS) + _ac_chain(1, 1, 63, 1, **RUNS)
        script += [([0], 1, 5, 0, 1, RUNS), ([0], 6, 63, 0, 1, RUNS),
                   ([0], 1, 5, 1, 0, RUNS), ([0], 6, 63, 1, 0, RUNS),
                   ([0, 1, 2], 0, 0, 1, 0), ([0, 1, 2], 0, 0, 0, 1)]
        # the DC first scan stores pred << 1 over what the refinement scan set
        expect = [lv.copy() for lv in levels]
        for lv in expect:
            lv[..., 0] &= ~1
    elif key == "refine_tables":
        w, h, samp = 29, 51, SAMPLINGS["440"]
        levels = sa_levels(rng, grids_of(), 0, 1, ac=5)
        y = levels[0]
        y[..., 1:] = 0
        (_, (bh, bw)) = grids_of()[0]
        for j in range(bh * bw):  # (r, 1) for every r, ZRL, a history coefficient behind them
            blk, r = y[j // bw, j % bw], j % 16
            blk[1 + r] = 2 * (-1) ** j  # new at Al = 1 behind r zeros
            if 1 + r + 17 <= 63:
                blk[1 + r + 17] = -2 * (-1) ** j  # 16 zeros: ZRL, then (0, 1)
            if 1 + r + 19 <= 63:
                blk[1 + r + 19] = rng.choice([-7, -5, 4, 6])  # first scan (Al = 2)
            blk[63 - r] = rng.choice([-1, 1])  # new at Al = 0
        dht.update({("ac", 2): jw.deep_table(REFINE_SYMBOLS),
                    ("ac", 3): jw.deep_table(REFINE_SYMBOLS[::-1])})
        t2, t3 = {"ta": [2, 2, 2]}, {"ta": [3, 3, 3]}
        script = [([0, 1, 2], 0, 0, 0, 0), ([0], 1, 63, 0, 2), ([1], 1, 63, 0, 1), ([2], 1, 63, 0, 1),
                  ([0], 1, 63, 2, 1, dict(RUNS, **t2)), ([1], 1, 63, 1, 0, dict(RUNS, **t3)),
                  # ids redefined between a component's scans: 2 deep -> flat, 1 Annex K -> flat
                  ([0], 1, 63, 1, 0, dict(t2, dht={("ac", 2): jw.flat_table(REFINE_SYMBOLS, 7)})),
                  ([2], 1, 63, 1, 0, dict(RUNS, dht={("ac", 1): jw.flat_table(REFINE_SYMBOLS, 16)}))]
    elif key in ("all_ones", "all_ones_ri4"):
        samp = [(1, 1)]
        lv = np.zeros((4, 5, 64), np.int32)
        lv[..., 1:] = np.where(rng.random((4, 5, 63)) < 0.97, 3, 1)  # history + bit 1 / new, positive
        lv[..., 0] = rng.integers(0, 40, size=(4, 5))
        levels = [lv]
        script = [([0], 0, 0, 0, 0)] + _ac_chain(0, 1, 63, 1, **RUNS)
        q = {0: np.ones(64, int)}
        if key == "all_ones_ri4":
            kw.update(restart_interval=4)
    elif key in ("scans_64", "scans_65"):
        w, h, samp = 64, 8, [(1, 1)]
        levels = sa_levels(rng, grids_of(), 1, 0, ac=6, nnz=24)
        levels[0][..., 1:] = np.where(rng.random((1, 8, 63)) < 0.4, rng.integers(-6, 7, size=(1, 8, 63)), 0)
        al = 1 if key == "scans_65" else 0
        script = [([0], 0, 0, 0, al)] + [([0], k, k, 0, 0) for k in range(1, 64)]
        script += [([0], 0, 0, 1, 0)] * al
    elif key == "repeat_refine":
        levels = sa_levels(rng, grids_of(), 0, 1, ac=5)
        script = [([0, 1, 2], 0, 0, 0, 0)] + [e for c in (1, 2, 0) for e in _ac_chain(c, 1, 63, 1, **RUNS)]
        script.append(([0], 1, 63, 1, 0, dict(RUNS, repeat=True)))
        # every luma coefficient that is non-zero takes a correction bit 1:
        # a clear bit 0 is set (the magnitude grows by 1), a set one stays
        expect = [lv.copy() for lv in levels]
        a = expect[0][..., 1:]
        a[...] = np.where((a != 0) & (a % 2 == 0), a + np.sign(a), a)
    elif key == "overlap_first":
        levels = sa_levels(rng, grids_of(), 0, 0, ac=10)
        y2 = levels[0].copy()
        y2[..., 1:5] = 0  # (not coded by the second scan)
        flat = y2.reshape(-1, 64)
        for j in range(len(flat)):
            if flat[j, 1:].any():
                flat[j, 11 + j % 40] = 5 if j % 2 else -5  # the scan codes something in every block
            if j % 2 == 0:
                flat[j, 5:11] = 0  # zeros where the first scan set values
            else:
                flat[j, 5:11] = np.where(flat[j, 5:11] != 0, -flat[j, 5:11], flat[j, 5:11])
        levels[0][..., 11:] = y2[..., 11:]
        script = [([0, 1, 2], 0, 0, 0, 0), ([0], 1, 10, 0, 0, RUNS),
                  ([0], 5, 63, 0, 0, dict(RUNS, levels=[y2, levels[1], levels[2]])),
                  ([1], 1, 63, 0, 0), ([2], 1, 63, 0, 0)]
        # a first scan writes the coefficients it codes and leaves the others
        expect = [lv.copy() for lv in levels]
        expect[0][..., 5:] = np.where(y2[..., 5:] != 0, y2[..., 5:], levels[0][..., 5:])
    elif key == "overlap_first_long":
        # a long first scan of 1-63, then a short one of 5-10 that changes every
        # 7th block: the short one must start after the long one, not beside it
        w, h, samp = 192, 192, [(1, 1)]
        levels = sa_levels(rng, grids_of(), 0, 0, ac=10, nnz=30)
        levels[0][..., 5:11] = rng.choice([-4, -3, 3, 4], size=(24, 24, 6))
        y2 = np.zeros_like(levels[0])
        flat = y2.reshape(-1, 64)
        flat[::7, 5:11] = rng.choice([-9, 0, 9], size=(len(flat[::7]), 6))
        script = [([0], 0, 0, 0, 0), ([0], 1, 63, 0, 0, RUNS), ([0], 5, 10, 0, 0, dict(RUNS, levels=[y2]))]
        expect = [np.where(y2 != 0, y2, levels[0])]
    elif key in ("zrl_overshoot_refine", "bad_size2", "bad_past_se"):
        levels = sa_levels(rng, grids_of(), 0, 1, ac=5)
        (_, (bh, bw)) = grids_of()[0]
        ex = {}
        for j in range(bh * bw):
            if j % 2 == 0 if key == "zrl_overshoot_refine" else j == 3:
                blk = levels[0][j // bw, j % bw]
                blk[50:] = 0
                blk[50] = (-1) ** (j // 2)  # the last new coefficient
                blk[55], blk[60] = 2, -3  # history behind it: 11 zero-history coefficients are left
                ex[(2, 0, j // bw, j % bw)] = {
                    "zrl_overshoot_refine": [("ac", jw.ZRL, 0, 0)],
                    "bad_size2": [("ac", 0x02, 2, 2)],
                    "bad_past_se": [("ac", 0xF1, 1, 1)]}[key]
        script = [([0, 1, 2], 0, 0, 0, 0)] + [e for c in range(3) for e in _ac_chain(c, 1, 63, 1, **RUNS)]
        kw.update(extra_symbols=ex)
    else:
        raise KeyError(key)
    ids = _std_ids(len(samp))
    if q is None:
        q = _small_q(rng, (0, 1), 3)
    s = _write("scr_" + key, w, h, samp, levels, q, ids, dht, ids, ids, scans="script", script=script, **kw)
    s.expect = expect
    s.script = script
    return s


SCRIPT_KEYS = ["deep_al", "al13", "dense_history", "dense_history_17", "eob_runs", "eob_runs_cap1",
               "eob_run_14", "eob_restart_ri5", "eob_restart_ri64", "eob_restart_fill2", "band_split",
               "band_merge", "band_merge_ri3", "dc_per_component", "order", "refine_tables", "all_ones",
               "all_ones_ri4", "scans_64", "scans_65", "repeat_refine", "overlap_first",
               "zrl_overshoot_refine", "bad_size2", "bad_past_se", "overlap_first_long"]
# streams a decoder must refuse (a refinement symbol of size 2; a new coefficient past Se)
SCRIPT_BAD = ["scr_bad_size2", "scr_bad_past_se"]
# saturate by nature, or decode to other levels than an encoder's: no clamp cap
SCRIPT_UNCAPPED = ["scr_al13", "scr_repeat_refine", "scr_overlap_first", "scr_overlap_first_long"]
# the oracle decodes all of these; the device refuses scr_scans_65 (64 scans at most)
SCRIPT_LEGAL = ["scr_" + k for k in SCRIPT_KEYS if "scr_" + k not in SCRIPT_BAD]
SCRIPT_CASES = [n for n in SCRIPT_LEGAL if n != "scr_scans_65"]
SCRIPT_CAPPED = [n for n in SCRIPT_LEGAL if n not in SCRIPT_UNCAPPED]
# decoded by libjpeg without a warning
SCRIPT_PILLOW = ["scr_deep_al", "scr_band_split", "scr_band_merge", "scr_dc_per_component",
                 "scr_eob_runs"]

CAPPED_CASES = SAMPLING_CASES + TABLE_CASES + STRUCTURE_CASES + PROGRESSIVE_CASES + SCRIPT_CAPPED
ACCEPTED_CASES = SAMPLING_CASES + TABLE_CASES + STRUCTURE_CASES + PROGRESSIVE_CASES + EXTREME_CASES


@functools.lru_cache(maxsize=None)
def case(name: str) -> Stream:
    kind, _, rest = name.partition("_")
    if kind == "samp":
        key, size, ri = rest.rsplit("_", 2)
        w, h = size.split("x")
        return _sampling_case(key, int(w), int(h), int(ri[2:]))
    if kind == "refused":
        return _refused_case(rest)
    if kind == "tab":
        return _table_case(rest)
    if kind == "ext":
        if rest.endswith("_pc"):
            return _extreme_case(rest[:-3], "per_component")
        return _extreme_case(rest, "interleaved")
    if kind == "blk":
        return _structure_case(rest)
    if kind == "prog":
        return _progressive_case(rest)
    if kind == "scr":
        return _script_case(rest)
    raise KeyError(name)


def pillow_legal(name: str) -> bool:
    """Streams inside what libjpeg decodes as written: canonical samplings
    (every chroma factor 1), categories <= 11 / sizes <= 10, 8-bit tables."""
    if name.startswith("samp_"):
        return name.split("_")[1] in CANONICAL
    return False


def saturated_share(rgb: np.ndarray) -> float:
    return float(np.mean((rgb == 0) | (rgb == 255)))
