"""Coefficient-level JPEG writer (ITU-T T.81), for tests: baseline, and
progressive by a scan script (spectral selection, successive approximation,
EOB runs).

Every other JPEG the suite decodes was made by an encoder from pixels, so it
only holds what an encoder emits.  `write_jpeg` takes the quantised levels,
the sampling factors, the Huffman and quantiser tables and the restart
interval themselves and writes the stream by the standard's rules: any legal
(and some deliberately odd) sampling layout, table shape, code length and
coefficient value can be put in front of a decoder.

Plain module: no fixtures, no pixels, no forward DCT.
"""

from __future__ import annotations

from collections import Counter

import numpy as np

# zig-zag index -> natural (row-major) index, T.81 figure A.6
NATURAL = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

EOB, ZRL = 0x00, 0xF0
DC_SYMBOLS = list(range(16))
# EOB, ZRL and the 240 (run, size) pairs with size 1..15
AC_SYMBOLS = [EOB, ZRL] + [(r << 4) | s for s in range(1, 16) for r in range(16)]


# ---- tables -----------------------------------------------------------------

def _h(s: str) -> list[int]:
    return [int(x, 16) for x in s.split()]


_STD_DC_LUM = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
_STD_DC_CHR = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
_STD_AC_LUM = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], _h(
    "01 02 03 00 04 11 05 12 21 31 41 06 13 51 61 07 22 71 14 32 81 91 a1 08 23 42 b1 c1 15 52 "
    "d1 f0 24 33 62 72 82 09 0a 16 17 18 19 1a 25 26 27 28 29 2a 34 35 36 37 38 39 3a 43 44 45 "
    "46 47 48 49 4a 53 54 55 56 57 58 59 5a 63 64 65 66 67 68 69 6a 73 74 75 76 77 78 79 7a 83 "
    "84 85 86 87 88 89 8a 92 93 94 95 96 97 98 99 9a a2 a3 a4 a5 a6 a7 a8 a9 aa b2 b3 b4 b5 b6 "
    "b7 b8 b9 ba c2 c3 c4 c5 c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da e1 e2 e3 e4 e5 e6 e7 e8 "
    "e9 ea f1 f2 f3 f4 f5 f6 f7 f8 f9 fa"))
_STD_AC_CHR = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], _h(
    "00 01 02 03 11 04 05 21 31 06 12 41 51 07 61 71 13 22 32 81 08 14 42 91 a1 b1 c1 09 23 33 "
    "52 f0 15 62 72 d1 0a 16 24 34 e1 25 f1 17 18 19 1a 26 27 28 29 2a 35 36 37 38 39 3a 43 44 "
    "45 46 47 48 49 4a 53 54 55 56 57 58 59 5a 63 64 65 66 67 68 69 6a 73 74 75 76 77 78 79 7a "
    "82 83 84 85 86 87 88 89 8a 92 93 94 95 96 97 98 99 9a a2 a3 a4 a5 a6 a7 a8 a9 aa b2 b3 b4 "
    "b5 b6 b7 b8 b9 ba c2 c3 c4 c5 c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da e2 e3 e4 e5 e6 e7 "
    "e8 e9 ea f2 f3 f4 f5 f6 f7 f8 f9 fa"))


def std_tables() -> dict:
    """The Annex K tables: {("dc", 0), ("ac", 0)} luminance, {.., 1} chrominance."""
    return {("dc", 0): _STD_DC_LUM, ("ac", 0): _STD_AC_LUM,
            ("dc", 1): _STD_DC_CHR, ("ac", 1): _STD_AC_CHR}


def _check_kraft(bits) -> None:
    code = 0
    for n in bits:
        code = (code + n) << 1
    # (code >> 1) / 2^16 is the Kraft sum in units of 2^-16
    assert (code >> 1) <= 1 << 16, "code lengths overflow the code space"


def deep_table(symbols):
    """One code at each length 2..15 (the first 14 symbols, in order), every
    other symbol at length 16: all code lengths past a 9- or 10-bit first
    level table occur, none of them the all-ones code."""
    symbols = list(symbols)
    bits = [0] * 16
    for i in range(min(14, len(symbols))):
        bits[1 + i] = 1
    bits[15] = max(len(symbols) - 14, 0)
    assert bits[15] <= 255
    _check_kraft(bits)
    return bits, symbols


def flat_table(symbols, length: int | None = None):
    """Every symbol at one code length (the shortest that leaves the all-ones
    code free, unless given)."""
    symbols = list(symbols)
    if length is None:
        length = max(len(symbols), 1).bit_length()
    assert len(symbols) < (1 << length) and len(symbols) <= 255
    bits = [0] * 16
    bits[length - 1] = len(symbols)
    return bits, symbols


def ranked_table(symbols, share: int = 4):
    """Code lengths that grow along `symbols` the way an optimiser's do along
    falling frequencies: each symbol takes the shortest length (from 2 bits)
    that costs at most 1 / `share` of the code space still free and leaves
    every later symbol a 16-bit code; the all-ones code stays free."""
    symbols = list(symbols)
    bits = [0] * 16
    free = (1 << 16) - 1  # in units of 2^-16
    length = 2
    for i in range(len(symbols)):
        later = len(symbols) - i - 1
        while length < 16 and (1 << (16 - length)) * share > free - later:
            length += 1
        bits[length - 1] += 1
        free -= 1 << (16 - length)
        assert free >= later
    _check_kraft(bits)
    return bits, symbols


def progressive_ac_symbols():
    """The alphabet of a progressive AC scan -- EOB0..EOB14, ZRL, the 240
    (run, size) pairs; Annex K's tables hold no EOBn above 0 -- short runs
    and small sizes first."""
    def rank(sym):
        r, s = sym >> 4, sym & 15
        return (r + 2 if r < 15 else 6) if s == 0 else r + 2 * s
    return sorted([n << 4 for n in range(1, 15)] + AC_SYMBOLS, key=lambda sym: (rank(sym), sym))


def short_table(inverted: bool = False) -> dict:
    """DC symbol 0 and EOB on 1-bit codes: a block of all-zero AC and
    unchanged DC takes 2 bits.  Plain: both codes are '0' and the other
    symbols follow at 2..; `inverted`: a dummy symbol takes '0' and the
    wanted one '1', so such a scan is all 1-bits (every byte 0xFF, stuffed).
    The inverted tables use the all-ones code, which T.81 forbids an encoder
    and libjpeg refuses; FFmpeg's VLC builder takes it."""
    def one(first, others):
        bits = [0] * 16
        if inverted:  # the 1-bit level is full: no room for more symbols
            bits[0] = 2
            return bits, [others[0], first]
        bits[0] = 1
        bits[7] = len(others)  # at 8 bits, inside the free half of the code space
        assert len(others) <= 127
        _check_kraft(bits)
        return bits, [first] + others
    dc = one(0, list(range(1, 12)))
    ac = one(EOB, [ZRL] + [(r << 4) | s for s in range(1, 7) for r in range(16)])
    return {("dc", 0): dc, ("ac", 0): ac}


def canonical_codes(bits, values) -> dict:
    """symbol -> (code, length), T.81 annex C."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            assert values[k] not in out, "symbol listed twice"
            out[values[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


# ---- geometry ---------------------------------------------------------------

def block_grids(width: int, height: int, samp):
    """Per component: ((bh, bw) of the interleaved scan's padded block grid,
    (bh, bw) of the component's own grid, which a non-interleaved scan
    codes).  One-component frames have only their own grid (T.81 A.2.2)."""
    hmax = max(h for h, _ in samp)
    vmax = max(v for _, v in samp)
    mcux = -(-width // (8 * hmax))
    mcuy = -(-height // (8 * vmax))
    out = []
    for h, v in samp:
        own = (-(-(-(-height * v // vmax)) // 8), -(-(-(-width * h // hmax)) // 8))
        out.append((own if len(samp) == 1 else (mcuy * v, mcux * h), own))
    return out


# ---- bit writer -------------------------------------------------------------

class _Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value: int, nbits: int) -> None:
        if nbits == 0:
            return
        assert 0 <= value < (1 << nbits)
        self.acc = (self.acc << nbits) | value
        self.n += nbits
        while self.n >= 8:
            self.n -= 8
            b = (self.acc >> self.n) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0x00)  # byte stuffing
        self.acc &= (1 << self.n) - 1

    def pad(self) -> None:
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)  # 1-padding before a marker

    def marker(self, m: int, fill: int = 0) -> None:
        self.pad()
        self.out += b"\xff" * fill + bytes([0xFF, m])


def _size(v: int) -> int:
    return abs(int(v)).bit_length()


def _amp(v: int, s: int) -> int:
    v = int(v)
    return v if v >= 0 else v + (1 << s) - 1


class _Coder:
    def __init__(self, bw: _Bits, dht: dict, stats):
        self.bw = bw
        self.codes = {k: canonical_codes(*t) for k, t in dht.items()}
        self.stats = stats
        self.sst = None  # the statistics of one scripted scan

    def sym(self, cls: str, tid: int, symbol: int) -> None:
        code, length = self.codes[(cls, tid)][symbol]
        self.bw.put(code, length)
        if self.stats is not None:
            self.stats[(cls, tid)][symbol] += 1
        if self.sst is not None:
            self.sst[cls][symbol] += 1

    def block(self, lv, pred: int, td: int, ta: int, extra) -> int:
        """One block (64 levels, zig-zag order, lv[0] absolute). Returns the new predictor."""
        diff = int(lv[0]) - pred
        s = _size(diff)
        assert s <= 15, "DC difference needs category 16"
        self.sym("dc", td, s)
        self.bw.put(_amp(diff, s), s)
        nz = np.nonzero(lv[1:])[0]
        last = int(nz[-1]) + 1 if nz.size else 0
        run = 0
        for k in range(1, last + 1):
            v = int(lv[k])
            if v == 0:
                run += 1
                continue
            while run > 15:
                self.sym("ac", ta, ZRL)
                run -= 16
            s = _size(v)
            assert s <= 15
            self.sym("ac", ta, (run << 4) | s)
            self.bw.put(_amp(v, s), s)
            run = 0
        if extra is not None:  # raw symbols in place of the EOB
            for cls, symbol, value, nbits in extra:
                self.sym(cls, td if cls == "dc" else ta, symbol)
                self.bw.put(value, nbits)
        elif last < 63:
            self.sym("ac", ta, EOB)
        return int(lv[0])


    def dc_first(self, lv0: int, pred: int, td: int) -> int:
        """Progressive DC first scan (Al = 0): the difference alone."""
        diff = int(lv0) - pred
        s = _size(diff)
        assert s <= 15
        self.sym("dc", td, s)
        self.bw.put(_amp(diff, s), s)
        return int(lv0)

    def ac_first(self, lv, ss: int, se: int, ta: int) -> None:
        """Progressive AC first scan of the band [ss, se] (Al = 0), every
        block closed on its own (EOBRUN 0: EOB0 unless lv[se] is non-zero)."""
        band = np.asarray(lv[ss:se + 1])
        nz = np.nonzero(band)[0]
        last = ss + int(nz[-1]) if nz.size else ss - 1
        run = 0
        for k in range(ss, last + 1):
            v = int(lv[k])
            if v == 0:
                run += 1
                continue
            while run > 15:
                self.sym("ac", ta, ZRL)
                run -= 16
            s = _size(v)
            assert s <= 15
            self.sym("ac", ta, (run << 4) | s)
            self.bw.put(_amp(v, s), s)
            run = 0
        if last < se:
            self.sym("ac", ta, EOB)

    # -- scripted progressive scans (T.81 G.1.2): successive approximation and
    # -- EOB runs.  One coder per scan; `run` is the pending EOBRUN, `run_bits`
    # -- the correction bits of its blocks, written after the EOBn symbol.

    def begin(self, policy, sst) -> None:
        """policy: 0 closes every block on its own (EOB0), n > 0 lets a run
        grow to the largest length of category n (2^(n+1) - 1 blocks), "max"
        to 32767; sst: this scan's statistics (or None)."""
        self.limit = 32767 if policy == "max" else 1 if policy == 0 else min((2 << policy) - 1, 32767)
        self.run, self.run_bits, self.sst = 0, [], sst

    def _field(self, bits) -> None:
        """One correction-bit field: the bits a decoder takes in one step."""
        for b in bits:
            self.bw.put(b, 1)
        if self.sst is not None and bits:
            self.sst["corr_fields"][len(bits)] += 1

    def flush_run(self, ta: int) -> None:
        if self.run:
            n = self.run.bit_length() - 1
            self.sym("ac", ta, n << 4)
            self.bw.put(self.run - (1 << n), n)
            if self.sst is not None:
                self.sst["eob"][n] += 1
            self.run = 0
        for bits in self.run_bits:
            self._field(bits)
        self.run_bits = []

    def _close(self, ta: int, bits) -> None:
        """The block ends inside an EOB run, which carries its correction bits."""
        if self.sst is not None and self.run and bits:
            self.sst["corr_bits_inside_runs"] += len(bits)
        self.run += 1
        self.run_bits.append(list(bits))
        if self.run >= self.limit:
            self.flush_run(ta)

    def _raw(self, td: int, ta: int, extra) -> None:
        for cls, symbol, value, nbits in extra:
            self.sym(cls, td if cls == "dc" else ta, symbol)
            self.bw.put(value, nbits)

    def dc_first_al(self, lv0: int, pred: int, td: int, al: int) -> int:
        """DC first scan: the difference of level >> Al (arithmetic shift)."""
        return self.dc_first(int(lv0) >> al, pred, td)

    def dc_refine(self, lv0: int, al: int) -> None:
        self.bw.put((int(lv0) >> al) & 1, 1)

    def ac_first_al(self, lv, ss: int, se: int, al: int, td: int, ta: int, extra) -> None:
        """AC first scan of [ss, se]: sign * (|level| >> Al), with EOB runs."""
        if extra is None and not np.any(lv[ss:se + 1]):
            return self._close(ta, [])
        run = 0
        for k in range(ss, se + 1):
            v = int(lv[k])
            a = abs(v) >> al
            if a == 0:
                run += 1
                continue
            self.flush_run(ta)
            while run > 15:
                self.sym("ac", ta, ZRL)
                run -= 16
            s = a.bit_length()
            assert s <= 15
            self.sym("ac", ta, (run << 4) | s)
            self.bw.put(_amp(a if v > 0 else -a, s), s)
            run = 0
        if extra is not None:
            self.flush_run(ta)
            self._raw(td, ta, extra)
        elif run:
            self._close(ta, [])

    def ac_refine(self, lv, ss: int, se: int, ah: int, al: int, td: int, ta: int, extra,
                  repeat: bool) -> None:
        """AC refinement of [ss, se] at bit Al.  History: |level| >> Ah != 0.
        A coefficient that turns non-zero is coded (run of zero-history
        coefficients, 1) plus its sign; every history coefficient passed adds
        one correction bit, written after the symbol that passes it (or after
        the EOBn of the run the block ends in); 16 zero-history coefficients
        in front of a new one are a ZRL.  `repeat`: the scan comes a second
        time -- the history is |level| >> Al, nothing is new and every
        correction bit is 1.  `extra`: raw symbols in place of the block's
        EOB; the block's remaining correction bits follow them."""
        if extra is None and not np.any(lv[ss:se + 1]):
            return self._close(ta, [])
        hs = al if repeat else ah
        mag = [abs(int(lv[k])) for k in range(se + 1)]
        hist = [m >> hs != 0 for m in mag]
        new = [not h and m >> al != 0 for h, m in zip(hist, mag)]
        last_new = max((k for k in range(ss, se + 1) if new[k]), default=ss - 1)
        run, bits = 0, []
        for k in range(ss, se + 1):
            if not hist[k] and not new[k]:
                run += 1
                continue
            while run > 15 and k <= last_new:
                self.flush_run(ta)
                self.sym("ac", ta, ZRL)
                run -= 16
                self._field(bits)
                bits = []
            if hist[k]:
                bits.append(1 if repeat else (mag[k] >> al) & 1)
                continue
            assert mag[k] >> al == 1, "a coefficient enters a refinement scan as +-1"
            self.flush_run(ta)
            self.sym("ac", ta, (run << 4) | 1)
            self.bw.put(1 if lv[k] > 0 else 0, 1)
            self._field(bits)
            run, bits = 0, []
        if extra is not None:
            self.flush_run(ta)
            self._raw(td, ta, extra)
            self._field(bits)
        elif run or bits:
            self._close(ta, bits)


# ---- the writer -------------------------------------------------------------

def _seg(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def write_jpeg(width, height, samp, levels, qtables, tq, dht, td, ta, *, restart_interval=0,
               pq=0, comp_ids=(1, 2, 3, 4), scans="interleaved", rst_fill=0, adobe=None,
               extra_symbols=None, emit_dri=False, table_segments="merged", stats=None,
               bands=((1, 5), (6, 63)), script=None) -> bytes:
    """A baseline (SOF0) JPEG of the given quantised levels (or, with
    scans="spectral", a progressive one by spectral selection alone; with
    scans="script", a progressive one scan by scan as `script` lists them).

    samp      [(h, v)] per component
    levels    per component [bh, bw, 64] (block_grids' first shape), zig-zag
              order, DC as the absolute level: the writer takes the
              differences and resets them at restarts
    qtables   {id: 64 entries, zig-zag order}; tq: table id per component
    dht       {("dc" | "ac", id): (bits[16], values)}; td / ta: ids per component
    restart_interval  in MCUs (blocks, in a non-interleaved scan); DRI is
              written when non-zero or when emit_dri is set
    pq        0: 8-bit quantiser entries, 1: 16-bit
    scans     "interleaved": one scan of all components; "per_component": one
              non-interleaved scan per component over that component's own
              ceil(w / 8) x ceil(h / 8) grid (levels outside it must be zero)
              "spectral": SOF2 -- one interleaved DC scan, then for every
              component one non-interleaved AC scan per band of `bands`
              (Ah = Al = 0, every EOBRUN 0); AC levels outside the own grid
              must be zero
    rst_fill  extra 0xFF fill bytes in front of every RSTn
    adobe     None, or the APP14 transform byte
    extra_symbols  {(c, by, bx): [(cls, symbol, value, nbits), ...]}: raw
              symbols of the block's own tables written after the block's last
              non-zero coefficient, in place of the EOB
    table_segments  "merged": one DQT and one DHT segment hold all tables;
              "single": one segment per table
    stats     a dict, filled with {(cls, id): Counter(symbol -> count)}; a
              scripted stream adds stats["scans"], one dict per scan:
              "entry" (components, ss, se, ah, al), "dc" / "ac"
              Counter(symbol), "eob" Counter(EOBn category), "corr_fields"
              Counter(length of a correction-bit field: the bits that follow
              one symbol, or one block's bits inside an EOB run) and
              "corr_bits_inside_runs" (correction bits of blocks a run skips)
    script    scans="script": SOF2 with one SOS per entry
              (components, ss, se, ah, al[, options]), coded by T.81 G.1.2:
              DC first (the difference of level >> al), DC refinement (bit al
              of the level), AC first (sign * (|level| >> al)) and AC
              refinement, each with the entry's Ss / Se / Ah / Al bytes.
              Several components make an interleaved scan (DC only), one
              component a scan over its own grid.  Nothing checks that the
              entries form a legal progression: the same refinement may come
              twice and first scans may overlap.  options:
                "eobrun"  0 (default): every block closed by its own EOB0; n:
                          runs up to the longest of category n; "max": a run
                          ends at 32767 blocks, at a restart and at the
                          scan's end
                "td", "ta"  table ids per component for this scan
                "dht"     {(cls, id): table} written in a DHT segment in front
                          of this SOS; replaces that id from here on
                "levels"  levels this scan codes in place of `levels`
                "repeat"  AC refinement written again at the same Al: the
                          history is |level| >> al, every correction bit 1
              extra_symbols is keyed (scan index, c, by, bx) here; in a
              refinement scan the block's pending correction bits follow the
              raw symbols
    """
    nc = len(samp)
    assert nc in (1, 3, 4) and len(levels) == nc
    grids = block_grids(width, height, samp)
    for c in range(nc):
        assert tuple(np.shape(levels[c])) == grids[c][0] + (64,), (c, np.shape(levels[c]), grids[c])
    if stats is not None:
        stats.clear()
        stats.update({k: Counter() for k in dht})
    extra_symbols = extra_symbols or {}

    out = bytearray(b"\xff\xd8")
    if adobe is not None:
        out += _seg(0xEE, b"Adobe" + bytes([0, 100, 0, 0, 0, 0, adobe]))
    dqt = []
    for tid in sorted(qtables):
        q = [int(x) for x in qtables[tid]]
        assert len(q) == 64 and all(0 < x < (65536 if pq else 256) for x in q)
        body = b"".join(x.to_bytes(2, "big") for x in q) if pq else bytes(q)
        dqt.append(bytes([(pq << 4) | tid]) + body)
    dhts = []
    for (cls, tid) in sorted(dht, key=lambda k: (k[0] != "dc", k[1])):
        bits, vals = dht[(cls, tid)]
        assert len(bits) == 16 and sum(bits) == len(vals)
        dhts.append(bytes([((cls == "ac") << 4) | tid]) + bytes(bits) + bytes(vals))
    if table_segments == "merged":
        out += _seg(0xDB, b"".join(dqt))
    else:
        for t in dqt:
            out += _seg(0xDB, t)
    sof = bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([nc])
    for c in range(nc):
        sof += bytes([comp_ids[c], (samp[c][0] << 4) | samp[c][1], tq[c]])
    out += _seg(0xC2 if scans in ("spectral", "script") else 0xC0, sof)
    if table_segments == "merged":
        out += _seg(0xC4, b"".join(dhts))
    else:
        for t in dhts:
            out += _seg(0xC4, t)
    if restart_interval or emit_dri:
        out += _seg(0xDD, restart_interval.to_bytes(2, "big"))

    def sos(comps, ss=0, se=63, ahal=0, td=td, ta=ta):
        p = bytes([len(comps)])
        for c in comps:
            p += bytes([comp_ids[c], (td[c] << 4) | ta[c]])
        return _seg(0xDA, p + bytes([ss, se, ahal]))

    def script_scan(i, entry, tables):
        comps, ss, se, ah, al = entry[:5]
        opt = entry[5] if len(entry) > 5 else {}
        comps = list(comps)
        std, sta = opt.get("td", td), opt.get("ta", ta)
        lvs = opt.get("levels", levels)
        assert (ss == 0) == (se == 0) and (ss == 0 or len(comps) == 1)
        if len(comps) > 1:
            units = [[u for u in mcu if u[0] in comps] for mcu in mcus]
        else:
            bh, bw_ = grids[comps[0]][1]
            units = [[(comps[0], y, x)] for y in range(bh) for x in range(bw_)]
        sst = None
        if stats is not None:
            sst = {"entry": (tuple(comps), ss, se, ah, al), "dc": Counter(), "ac": Counter(),
                   "eob": Counter(), "corr_fields": Counter(), "corr_bits_inside_runs": 0}
            stats["scans"].append(sst)
        bw = _Bits()
        coder = _Coder(bw, tables, stats)
        coder.begin(opt.get("eobrun", 0), sst)
        pred = [0] * nc
        for j, unit in enumerate(units):
            if restart_interval and j and j % restart_interval == 0:
                if ss:
                    coder.flush_run(sta[comps[0]])
                bw.marker(0xD0 + (j // restart_interval - 1) % 8, rst_fill)
                pred = [0] * nc
            for c, by, bx in unit:
                lv = lvs[c][by][bx]
                ex = extra_symbols.get((i, c, by, bx))
                if ss == 0 and ah == 0:
                    pred[c] = coder.dc_first_al(lv[0], pred[c], std[c], al)
                elif ss == 0:
                    coder.dc_refine(lv[0], al)
                elif ah == 0 and not opt.get("repeat"):
                    coder.ac_first_al(lv, ss, se, al, std[c], sta[c], ex)
                else:
                    coder.ac_refine(lv, ss, se, ah, al, std[c], sta[c], ex,
                                    bool(opt.get("repeat")))
        if ss:
            coder.flush_run(sta[comps[0]])
        bw.pad()
        return sos(comps, ss, se, (ah << 4) | al, std, sta) + bytes(bw.out)

    def scan(comps, units, band=None):
        """units: per MCU, the list of (c, by, bx) blocks.  band: None for a
        sequential scan, else the (ss, se) of a progressive first scan."""
        bw = _Bits()
        coder = _Coder(bw, dht, stats)
        pred = [0] * nc
        for i, unit in enumerate(units):
            if restart_interval and i and i % restart_interval == 0:
                bw.marker(0xD0 + (i // restart_interval - 1) % 8, rst_fill)
                pred = [0] * nc
            for c, by, bx in unit:
                if band is None:
                    pred[c] = coder.block(levels[c][by][bx], pred[c], td[c], ta[c],
                                          extra_symbols.get((c, by, bx)))
                elif band[0] == 0:
                    pred[c] = coder.dc_first(levels[c][by][bx][0], pred[c], td[c])
                else:
                    coder.ac_first(levels[c][by][bx], band[0], band[1], ta[c])
        bw.pad()
        return bytes(bw.out)

    if nc == 1:
        bh, bw_ = grids[0][0]
        mcus = [[(0, y, x)] for y in range(bh) for x in range(bw_)]
    else:
        mcuy = grids[0][0][0] // samp[0][1]
        mcux = grids[0][0][1] // samp[0][0]
        mcus = [[(c, my * v + y, mx * h + x) for c, (h, v) in enumerate(samp)
                 for y in range(v) for x in range(h)]
                for my in range(mcuy) for mx in range(mcux)]
    if scans == "interleaved":
        out += sos(list(range(nc))) + scan(list(range(nc)), mcus)
    elif scans == "spectral":
        assert bands[0][0] == 1 and bands[-1][1] == 63
        assert all(b[1] + 1 == n[0] for b, n in zip(bands, bands[1:]))
        out += sos(list(range(nc)), 0, 0) + scan(list(range(nc)), mcus, (0, 0))
        for c in range(nc):
            bh, bw_ = grids[c][1]
            lv = np.asarray(levels[c])
            assert not lv[bh:, :, 1:].any() and not lv[:, bw_:, 1:].any(), \
                "AC levels outside the own grid"
            for ss, se in bands:
                out += sos([c], ss, se) + scan(
                    [c], [[(c, y, x)] for y in range(bh) for x in range(bw_)], (ss, se))
    elif scans == "script":
        tables = dict(dht)
        if stats is not None:
            stats["scans"] = []
        for i, entry in enumerate(script):
            more = entry[5].get("dht") if len(entry) > 5 else None
            if more:
                tables.update(more)
                seg = b""
                for (cls, tid), (bits, vals) in more.items():
                    assert len(bits) == 16 and sum(bits) == len(vals)
                    seg += bytes([((cls == "ac") << 4) | tid]) + bytes(bits) + bytes(vals)
                    if stats is not None:
                        stats.setdefault((cls, tid), Counter())
                out += _seg(0xC4, seg)
            out += script_scan(i, entry, tables)
    elif scans == "per_component":
        for c in range(nc):
            bh, bw_ = grids[c][1]
            lv = np.asarray(levels[c])
            assert not lv[bh:].any() and not lv[:, bw_:].any(), "levels outside the own grid"
            out += sos([c]) + scan([c], [[(c, y, x)] for y in range(bh) for x in range(bw_)])
    else:
        raise ValueError(scans)
    out += b"\xff\xd9"
    return bytes(out)
