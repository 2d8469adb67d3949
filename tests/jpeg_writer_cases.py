"""The hand-written stream families (tests/jpeg_writer.py), shared by the CPU
tests (test_jpeg_writer.py) and the GPU parity tests (test_gpu_handwritten.py).

`case(name)` returns a `Stream`: the bytes, what was written (levels in
zig-zag order, tables, sampling) and the writer's symbol histogram.  Families:

  1  samplings        SAMPLING_CASES, REFUSED_CASES
  2  Huffman tables   TABLE_CASES
  3  coefficient extremes (deep tables)   EXTREME_CASES (+ per_component twins)
  4  block structure  STRUCTURE_CASES
  5  spectral selection (SOF2 without refinement)   PROGRESSIVE_CASES

Families 1, 2, 4 and 5 keep amplitudes small (CAPPED: at most 25 % of the
oracle's RGB samples at 0 or 255, asserted by the tests); family 3 saturates
by nature.
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

    def natural_levels(self):
        """Per component [bh, bw, 64] in natural order (the oracle's layout)."""
        out = []
        for lv in self.levels:
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

CAPPED_CASES = SAMPLING_CASES + TABLE_CASES + STRUCTURE_CASES + PROGRESSIVE_CASES
ACCEPTED_CASES = CAPPED_CASES + EXTREME_CASES


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
    raise KeyError(name)


def pillow_legal(name: str) -> bool:
    """Streams inside what libjpeg decodes as written: canonical samplings
    (every chroma factor 1), categories <= 11 / sizes <= 10, 8-bit tables."""
    if name.startswith("samp_"):
        return name.split("_")[1] in CANONICAL
    return False


def saturated_share(rgb: np.ndarray) -> float:
    return float(np.mean((rgb == 0) | (rgb == 255)))
