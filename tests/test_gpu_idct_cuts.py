"""GPU parity of the simple IDCT kernels (idct_kernel<simple>,
idct_rgb_kernel<simple>) where their instruction cuts could go wrong, on
hand-written streams (tests/jpeg_writer.py).  Bit-exact against the oracle:
decode_planes (simple and islow) and full-resolution rgb24 (the fused path,
idct_rgb_kernel, and output_path 1 and 2), as tests/test_gpu_handwritten.py's
check_planes / check_rgb.

  DC-only rows   the row pass's shortcut (row[0] << 3 where row[1..7] are
                 zero) is a bias of the full sums: every row 0-7 with each of
                 -32768, -2048, -1025, -1024, -1023, -1, 1, 1023, 1024, 1025,
                 2047, 32767 in column 0 and nothing else, and the same with a
                 single +-1 in column 2 (the high half of the row's first
                 word), column 1 and column 7, which must not take the shortcut.
  clip           a DC ramp whose unclipped outputs (recomputed from the
                 oracle's coefficients) run through every value of -2..257, and
                 blocks of idct_worst_blocks() at +-2047 and +-32767.
  scatter        AC counts 0, 1, 2, 3, 4, 5, 13, 15, 16, 17, 31, 32, 33, 63, 0,
                 63, 1 over consecutive blocks; 16-bit quantisers whose
                 products wrap int16.
  block index    block counts that are no multiple of 256 over several
                 workgroups, odd MCU columns, alone and in a batch between two
                 ordinary images (the flat grid).

All these streams are uncapped (nothing bounds the share of 0 / 255 samples,
as in test_gpu_handwritten's family 3): the DC-only, clip and int16-wrap
streams saturate by design; the planes carry the check there.
"""

import functools

import numpy as np
import pytest

from spdl_amd._lib import Output
from tests import cases
from tests import jpeg_writer as jw
from tests import jpeg_writer_cases as hw
from tests.test_gpu_handwritten import RESIZE32, _decode, check_planes, check_rgb

gpu = pytest.mark.gpu  # (the tests of the streams themselves need the oracle only)
W4 = 16383  # simple_idct (8-bit)

S422 = [(2, 1), (1, 1), (1, 1)]
S444 = [(1, 1), (1, 1), (1, 1)]


def _deep():
    return {("dc", 0): jw.deep_table(jw.DC_SYMBOLS), ("ac", 0): jw.deep_table(jw.AC_SYMBOLS)}


def _levels(nat, shape):
    """Natural-order [n, 64] levels -> [bh, bw, 64] zig-zag, raster block
    order, zero blocks after the last."""
    bh, bw = shape
    lv = np.zeros((bh * bw, 64), np.int32)
    assert len(nat) <= bh * bw
    lv[:len(nat)] = np.asarray(nat)[:, jw.NATURAL]
    return lv.reshape(bh, bw, 64)


def _stream_422(name, luma, q, mcux):
    """4:2:2 (idct_rgb_kernel's MCU): the blocks as luma, the even ones as U
    and the odd ones as V; restart interval 1, so a DC level is coded as it is
    after a restart and as a difference only inside the luma pair."""
    n = len(luma)
    assert n % (2 * mcux) == 0
    mcuy = n // (2 * mcux)
    lv = [_levels(luma, (mcuy, 2 * mcux)), _levels(luma[0::2], (mcuy, mcux)),
          _levels(luma[1::2], (mcuy, mcux))]
    return hw._write(name, 16 * mcux, 8 * mcuy, S422, lv, {0: q}, [0, 0, 0], _deep(), [0, 0, 0],
                     [0, 0, 0], restart_interval=1)


# ---- DC-only rows -----------------------------------------------------------------

DC_VALUES = [-32768, -2048, -1025, -1024, -1023, -1, 1, 1023, 1024, 1025, 2047, 32767]
NEAR_MISS = [None] + [(c, s) for c in (2, 1, 7) for s in (1, -1)]


def _dc_row_blocks(values, q0):
    """Natural-order levels: for each row and value, the block whose row holds
    the value (dequantised, by quantiser q0 in column 0) in column 0 alone,
    then its six near misses.  The DC level carries the decoder's + 1024."""
    out = []
    for r in range(8):
        for v in values:
            for miss in NEAR_MISS:
                blk = np.zeros(64, np.int64)
                x = v - 1024 if r == 0 else v
                assert x % q0 == 0
                blk[8 * r] = x // q0
                if miss:
                    blk[8 * r + miss[0]] = miss[1]
                out.append(blk)
    return np.array(out)


@functools.lru_cache(maxsize=None)
def _dc_row_stream(which):
    if which == "q1":  # every value a level reaches at q = 1
        vals = [v for v in DC_VALUES if v != -32768]
        return _stream_422("dc_rows_q1", _dc_row_blocks(vals, 1), np.ones(64, int), 14), vals
    # -32768 = -16384 x 2: quantiser 2 in column 0 (1 elsewhere, for the +-1)
    vals = [-32768, -2048, 1024, 32766]
    q = np.where(jw.NATURAL % 8 == 0, 2, 1)
    return _stream_422("dc_rows_q2", _dc_row_blocks(vals, 2), q, 14), vals


def test_dc_row_streams_hold_the_boundary(oracle):
    """The streams are what the docstring says, on the oracle's coefficients:
    per row, every value alone in the row, and with each near miss."""
    seen = {r: {m: set() for m in NEAR_MISS} for r in range(8)}
    for which in ("q1", "q2"):
        s, _ = _dc_row_stream(which)
        ref, _ = oracle.decode_coefs(s.data)
        rows = ref.reshape(-1, 8, 8).astype(np.int64)
        for r in range(8):
            rest = rows[:, r, 1:]
            nz = (rest != 0).sum(axis=1)
            seen[r][None] |= set(rows[nz == 0, r, 0].tolist())
            for c, sg in NEAR_MISS[1:]:
                hit = (nz == 1) & (rows[:, r, c] == sg)
                seen[r][(c, sg)] |= set(rows[hit, r, 0].tolist())
    for r in range(8):
        for m in NEAR_MISS:
            assert set(DC_VALUES) <= seen[r][m], (r, m, sorted(set(DC_VALUES) - seen[r][m]))


@gpu
@pytest.mark.parametrize("which", ["q1", "q2"])
def test_dc_only_rows(decoder, oracle, which):
    s, _ = _dc_row_stream(which)
    check_planes(decoder, oracle, s.data)
    check_rgb(decoder, oracle, s.data)


# ---- clip boundaries ----------------------------------------------------------------

RAMP = np.arange(-40, 2104)  # the DC coefficient (level + 1024): 2144 blocks


def _worst(mag, n=16):
    blocks = hw.idct_worst_blocks()
    b = np.sign(blocks[:: len(blocks) // n][:n]) * mag
    if mag + 1024 > 32767:  # (as ext_idct_worst: + 1024 must stay in int16)
        b[:, 0] = np.where(b[:, 0] > 0, 31743, b[:, 0])
    return b


def _ramp_blocks():
    nat = np.zeros((len(RAMP), 64), np.int64)
    nat[:, 0] = RAMP - 1024
    return nat


@functools.lru_cache(maxsize=None)
def _clip_stream(kind):
    ramp = _ramp_blocks()
    if kind == "gray":  # 32 blocks a row: the ramp, then +-2047 and +-32767 extremes
        nat = np.concatenate([ramp, _worst(2047), _worst(32767)])
        lv = [_levels(nat, (len(nat) // 32, 32))]
        return hw._write("clip_gray", 256, 8 * (len(nat) // 32), [(1, 1)], lv, {0: np.ones(64, int)},
                         [0], _deep(), [0], [0], restart_interval=1)
    # (a luma pair codes a DC difference: the +-2047 blocks only, sorted by DC)
    w = _worst(2047, 32)
    nat = np.concatenate([ramp, w[np.argsort(w[:, 0], kind="stable")]])
    return _stream_422("clip_422", nat, np.ones(64, int), 16)


def test_clip_ramp_reaches_every_value(oracle):
    """The ramp blocks are DC-only, so every pixel of one is
    (W4 (8 x0 + 32)) >> 20 before the clip (row pass x0 << 3, column pass
    W4 (c0 + 32)): from the oracle's coefficients these run through every
    value of -2..257, and clipped they are the oracle's plane."""
    s = _clip_stream("gray")
    ref, _ = oracle.decode_coefs(s.data)
    ref = ref.astype(np.int64)[:len(RAMP)]
    assert not ref[:, 1:].any()
    unclipped = (W4 * (8 * ref[:, 0] + 32)) >> 20
    assert set(range(-2, 258)) <= set(unclipped.tolist())
    plane = oracle.decode_planes(s.data)[0]
    rows = len(RAMP) // 32
    blocks = plane[:8 * rows].reshape(rows, 8, 32, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
    np.testing.assert_array_equal(blocks, np.clip(unclipped, 0, 255)[:, None].repeat(64, axis=1))


@gpu
def test_clip_boundaries_gray(decoder, oracle):
    check_planes(decoder, oracle, _clip_stream("gray").data)
    check_rgb(decoder, oracle, _clip_stream("gray").data)


@gpu
def test_clip_boundaries_422(decoder, oracle):
    check_planes(decoder, oracle, _clip_stream("422").data)
    check_rgb(decoder, oracle, _clip_stream("422").data)


# ---- scatter -----------------------------------------------------------------------------

# 17 counts summing to 299 = 3 mod 4: lists are packed back to back, so over
# four periods a count meets every start offset 0-3; 0 / 16 / 17, 32 / 33 and
# 63 sit on both sides of the scatter loop's trips of 16 entries.
AC_COUNTS = [0, 1, 2, 3, 4, 5, 13, 15, 16, 17, 31, 32, 33, 63, 0, 63, 1]


def _scatter_levels(nblocks, value):
    """[nblocks, 64] zig-zag levels, block j (MCU order) with AC_COUNTS[j % 17]
    non-zero AC coefficients at positions drawn per block, each value a
    function of (block, k)."""
    lv = np.zeros((nblocks, 64), np.int32)
    for j in range(nblocks):
        n = AC_COUNTS[j % len(AC_COUNTS)]
        ks = 1 + np.random.default_rng(1000 + j).choice(63, size=n, replace=False)
        for k in ks:
            lv[j, k] = value(j, int(k))
        lv[j, 0] = (j * 37) % 101 - 50
    return lv


@functools.lru_cache(maxsize=None)
def _scatter_stream(kind):
    mcux, mcuy = 12, 8  # 288 blocks: 16 periods and a part, two workgroups
    n = mcux * mcuy * 3
    if kind == "q1":
        lv = _scatter_levels(n, lambda j, k: (1 + (7 * j + 5 * k) % 9) * (-1 if (j + k) % 2 else 1))
        q, pq = {0: np.ones(64, int)}, 0
    else:  # 16-bit quantisers >= 256, levels of both signs: products past int16
        lv = _scatter_levels(n, lambda j, k: (1 + (11 * j + 3 * k) % 700) * (-1 if (j + k) % 2 else 1))
        q = {0: 256 + (np.arange(64) * 1021 + 77) % (65536 - 256)}
        pq = 1
        prod = np.abs(lv[:, 1:].astype(np.int64) * q[0][None, 1:])
        assert (prod[lv[:, 1:] != 0] > 32767).mean() > 0.5
    # MCU order (Y, U, V of an MCU are consecutive lists) -> per component
    per = [_zz_grid(lv[c::3], mcuy, mcux) for c in range(3)]
    return hw._write(f"scatter_{kind}", 8 * mcux, 8 * mcuy, S444, per, q, [0, 0, 0], _deep(),
                     [0, 0, 0], [0, 0, 0], pq=pq)


def _zz_grid(lv, bh, bw):
    return lv.reshape(bh, bw, 64)


def test_scatter_counts_are_as_listed(oracle):
    s = _scatter_stream("q1")
    ref, _ = oracle.decode_coefs(s.data)
    got = (ref[:, 1:] != 0).sum(axis=1)
    want = [AC_COUNTS[j % len(AC_COUNTS)] for j in range(len(got))]
    assert got.tolist() == want


@gpu
@pytest.mark.parametrize("kind", ["q1", "pq1"])
def test_scatter(decoder, oracle, kind):
    s = _scatter_stream(kind)
    check_planes(decoder, oracle, s.data)
    check_rgb(decoder, oracle, s.data)


# ---- block index ---------------------------------------------------------------------------

INDEX_CASES = {
    "420_344x200": (344, 200, [(2, 2), (1, 1), (1, 1)]),  # 22 x 13 MCUs, 1716 blocks
    "420_40x24": (40, 24, [(2, 2), (1, 1), (1, 1)]),      # mcux 3
    "411_344x200": (344, 200, hw.SAMPLINGS["411"]),       # 11 x 25 MCUs, 1650 blocks
    "440_344x200": (344, 200, hw.SAMPLINGS["440"]),       # 43 x 13 MCUs, 2236 blocks
    "gray_8x8": (8, 8, [(1, 1)]),                         # one block
}


@functools.lru_cache(maxsize=None)
def _index_stream(name):
    w, h, samp = INDEX_CASES[name]
    rng = np.random.default_rng(500 + list(INDEX_CASES).index(name))
    levels = hw.moderate_levels(rng, hw._grid_shapes(w, h, samp))
    ids = hw._std_ids(len(samp))
    return hw._write("idx_" + name, w, h, samp, levels, hw._small_q(rng, (0, 1)), ids,
                     jw.std_tables(), ids, ids)


def test_index_streams_are_as_listed():
    n = {}
    for name, (w, h, samp) in INDEX_CASES.items():
        grids = hw._grid_shapes(w, h, samp)
        n[name] = sum(a * b for a, b in grids)
    assert n == {"420_344x200": 1716, "420_40x24": 36, "411_344x200": 1650, "440_344x200": 2236,
                 "gray_8x8": 1}
    assert all(v % 256 for v in n.values())


@gpu
@pytest.mark.parametrize("name", list(INDEX_CASES))
def test_block_index(decoder, oracle, name):
    s = _index_stream(name)
    check_planes(decoder, oracle, s.data)
    check_rgb(decoder, oracle, s.data)


@gpu
def test_block_index_between_ordinary_images(decoder, oracle):
    """Each of them in one batch between q90_420 and gray (sizes that differ
    widely: the flat grid's workgroup -> image map)."""
    datas = [cases.case("q90_420")]
    for name in INDEX_CASES:
        datas += [_index_stream(name).data,
                  cases.case("gray") if len(datas) % 4 == 1 else cases.case("q90_420")]
    out = Output(pix_fmt="rgb24", resize=True, **RESIZE32)
    hyp = _decode(decoder, datas, out, (32, 32, 3))
    for i, d in enumerate(datas):
        ref = oracle.decode_resize(d, oracle.Resize(**RESIZE32), pix_fmt="rgb24")
        np.testing.assert_array_equal(hyp[i], ref, strict=True, err_msg=f"image {i}")
