"""The arithmetic inside an output-stage tile (sws_kernel, hpass): the pixel
pairs of the table writers, the rows dealt across waves, the pad rectangles
and the v_dot4 horizontal pass, at the smallest shapes where each can go
wrong.  Through the C-ABI as tests/test_gpu_sws_sweep.py does: every batch in
front of a guard image, bit-exact against ``oracle.decode_resize`` (planar
output: tests/yuv_scale_ref.py).  Sources are seeded textures and 0 / 255 bar
images of at most 64 x 48, and the committed RGB-coded file (150 x 100).

The CPU tests at the end (no GPU) check that the case table reaches the tile
kinds and register buckets it is there for, and that the tap split of the
dot4 pass restores every tap of every table the cases use.
"""

import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

from spdl_amd import _lib
from spdl_amd._lib import Output
from spdl_amd.synthetic import synthetic_pixels
from tests import cases, yuv_scale_ref

gpu = pytest.mark.gpu

GUARD = 0xA5
GUARD_WORD = 0x5A5A
FILTERS = ("bicubic", "bilinear", "lanczos")
PIX_FMTS = ("rgb24", "bgr24", "rgb", "bgr")

# ---- sources --------------------------------------------------------------------
# name -> (seed, w, h, Pillow subsampling; None = gray), q92
TEXTURE = {
    "t420": (70, 64, 48, 2), "t422": (71, 64, 48, 1), "t444": (72, 64, 48, 0),
    "tgray": (73, 64, 48, None),
    "t420_16": (74, 64, 16, 2), "tgray_16": (75, 64, 16, None),
    "t420_8": (76, 64, 8, 2),
}
BAR_PERIODS = (1, 2, 3, 7)
BARS = tuple(f"bar{k}_{s}" for k in BAR_PERIODS for s in ("gray", "420"))
SAMPLINGS = ("t420", "t422", "t444", "tgray", "rgb_coded")  # rgb_coded: committed, gbr path


def bar_row(period: int, w: int = 64) -> np.ndarray:
    """0 / 255 columns, `period` pixels off then `period` on."""
    return ((np.arange(w) // period % 2) * 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def source(name: str) -> bytes:
    if name in TEXTURE:
        seed, w, h, sub = TEXTURE[name]
        px = synthetic_pixels(seed, h, w)
        if sub is None:
            return cases._enc(px[..., 0], quality=92)
        return cases._enc(px, quality=92, subsampling=sub)
    if name in BARS:
        g = np.repeat(bar_row(int(name[3]))[None], 8, axis=0)
        if name.endswith("gray"):
            return cases._enc(g, quality=100)
        return cases._enc(np.repeat(g[..., None], 3, axis=2), quality=100, subsampling=2)
    return cases.case(name)


@functools.lru_cache(maxsize=None)
def meta(name: str):
    i = _lib.get_image_info(source(name))
    hs = vs = 0
    if i.ncomp == 3:
        hs = (i.h_samp[0] // i.h_samp[1]).bit_length() - 1
        vs = (i.v_samp[0] // i.v_samp[1]).bit_length() - 1
    mode = "gray" if i.ncomp == 1 else "gbr" if i.color in (2, 3) else "yuv"
    return i.width, i.height, hs, vs, mode


# ---- cases ----------------------------------------------------------------------
# names: one decode_batch (planar output: one call per name); rs: the resize
# spec as keywords; knobs: ("sws_prepass", "sws_cols")
Case = namedtuple("Case", "id names rs filt pix_fmt norm pre cols", defaults=("rgb24", None, -1, 256))


def _rs(**kw):
    return tuple(sorted(kw.items()))


def _pairs_cases():
    out = []
    # even scaled widths (full = 0: pairs) and odd ones (full chroma, unpaired)
    for w in (2, 4, 14, 16, 1, 3, 15):
        out.append(Case(f"w{w}", SAMPLINGS, _rs(fit_w=w, fit_h=12), "bicubic"))
    # an even width at an odd pad offset: dx 1, dy 1
    out.append(Case("w14_in17", SAMPLINGS, _rs(fit_w=14, fit_h=12, pad_w=17, pad_h=15), "bicubic"))
    # 28 wide at dx 3 of a 34-wide output, 16-column tiles: xs [0, 13) ends on
    # the even half of a pair, xs [13, 28) starts on the odd half of that pair,
    # the last tile is all pad
    for f in ("rgb24", "rgb"):
        out.append(Case(f"w28_in34_cols16_{f}", SAMPLINGS,
                        _rs(fit_w=28, fit_h=12, pad_w=34, pad_h=14), "bicubic", f, None, -1, 16))
    # crops at odd offsets: dx -7, dy -3; 16-column tiles start at xs 7, 23
    out.append(Case("w30_crop16", SAMPLINGS, _rs(fit_w=30, fit_h=12, crop_w=16, crop_h=6),
                    "bicubic"))
    out.append(Case("w62_crop48_cols16", SAMPLINGS, _rs(fit_w=62, fit_h=12, crop_w=48, crop_h=6),
                    "bilinear", "bgr24", None, -1, 16))
    return out


def _row_cases():
    out = []
    short = ("t420_16", "tgray_16")
    for w in (14, 15):  # paired and unpaired
        # bands of 1, 2, 3 and 5 rows (X rows)
        for h in (1, 2, 3, 5):
            out.append(Case(f"h{h}_w{w}", short, _rs(fit_w=w, fit_h=h), "bicubic"))
        # an unscaled height: size-1 vertical filters (One)
        # (4:2:0 under bilinear: One with the chroma blend)
        out.append(Case(f"h48_w{w}", SAMPLINGS, _rs(fit_w=w, fit_h=48), "bicubic"))
        out.append(Case(f"h48_w{w}_bilinear", SAMPLINGS, _rs(fit_w=w, fit_h=48), "bilinear"))
        # a bilinear 2x upscale (Two; One with a chroma blend where the plan makes it)
        out.append(Case(f"up96_w{w}", SAMPLINGS, _rs(fit_w=w, fit_h=96), "bilinear"))
        out.append(Case(f"up32_w{w}", ("t420_16", "t420_8"), _rs(fit_w=w, fit_h=32), "bilinear"))
        # 2.9x downscales (X)
        for filt in ("bicubic", "lanczos"):
            out.append(Case(f"h17_w{w}_{filt}", SAMPLINGS, _rs(fit_w=w, fit_h=17), filt))
    # more than 64 pairs in a row: two (row, 64 pairs) units per row, 5 rows
    # over 4 waves; and its unpaired neighbour
    for w in (132, 131):
        out.append(Case(f"h5_w{w}", short, _rs(fit_w=w, fit_h=5), "bicubic"))
        out.append(Case(f"h5_w{w}_norm", short, _rs(fit_w=w, fit_h=5), "bilinear", "rgb", "float16"))
    return out


# 38 x 70 at (5, 5) of 48 x 80 in 16-column tiles: tiles across each of the
# four edges, across two at once (the corners) and of content alone;
# 14 x 6 at (18, 33) of 50 x 72: tiles of pad alone, and one band that holds
# the content's top and bottom edge
PAD_GEOMETRIES = {
    "edges": _rs(fit_w=38, fit_h=70, pad_w=48, pad_h=80),
    "island": _rs(fit_w=14, fit_h=6, pad_w=50, pad_h=72),
}


def _pad_cases():
    out = []
    for g, rs in PAD_GEOMETRIES.items():
        for f in PIX_FMTS:
            out.append(Case(f"{g}_{f}", ("t420", "tgray"), rs, "bicubic", f, None, -1, 16))
        for norm in ("float16", "bfloat16"):
            for f in ("rgb24", "rgb"):
                out.append(Case(f"{g}_{f}_{norm}", ("t420", "tgray"), rs, "bilinear", f, norm, -1, 16))
    return out


# 64 columns scaled by 1.0, 1.5, 2.9, 5 and 9
DOT4_WIDTHS = (64, 43, 22, 13, 7)
DOT4_SOURCES = (*BARS, "t420_8")


def _dot4_cases():
    out = []
    for w in DOT4_WIDTHS:
        for filt in FILTERS:
            rs = _rs(fit_w=w, fit_h=0)
            out.append(Case(f"w{w}_{filt}", DOT4_SOURCES, rs, filt))
            out.append(Case(f"w{w}_{filt}_pre", DOT4_SOURCES, rs, filt, "rgb24", None, 1))
            out.append(Case(f"w{w}_{filt}_yuv", DOT4_SOURCES, rs, filt, "yuv"))
    return out


PAIRS, ROWS, PAD, DOT4 = _pairs_cases(), _row_cases(), _pad_cases(), _dot4_cases()
ALL = (*PAIRS, *ROWS, *PAD, *DOT4)


def output(c: Case) -> Output:
    return Output(resize=True, filter=c.filt, pix_fmt=c.pix_fmt, normalize=bool(c.norm),
                  norm_dtype=c.norm or "float16", **dict(c.rs))


def probe(c: Case, name: str) -> dict:
    w, h, hs, vs, mode = meta(name)
    return _lib.debug_sws_plan(w, h, hs, vs, mode, output(c), c.pre, c.cols)


# ---- the GPU runs ---------------------------------------------------------------
def _decode(dec, c: Case, names, n_out: int, shape):
    """One decode_batch of `names` into a guard-filled buffer with an image's
    worth of guard behind it: [len(names), *shape]."""
    n = len(names)
    per = n_out // n
    if c.norm:
        t = torch.full(((n + 1) * per,), GUARD_WORD, dtype=torch.int16, device="cuda:0")
        want = GUARD_WORD
    else:
        t = torch.full(((n + 1) * per,), GUARD, dtype=torch.uint8, device="cuda:0")
        want = GUARD
    dec.set_param("sws_prepass", c.pre)
    dec.set_param("sws_cols", c.cols)
    try:
        st = dec.decode_batch([source(x) for x in names], output(c), t.data_ptr(),
                              n * per * t.element_size(), stream=torch.cuda.current_stream())
    finally:
        dec.set_param("sws_prepass", -1)
        dec.set_param("sws_cols", 256)
    assert all(s == 0 for s in st), st
    a = t.cpu().numpy()
    assert (a[n * per:] == want).all(), f"{c.id}: wrote past the batch's output"
    a = a[: n * per].reshape((n,) + tuple(shape))
    return a.view(np.uint16) if c.norm else a


def _check(dec, O, c: Case):
    rs = O.Resize(filter=c.filt, **dict(c.rs))
    if c.pix_fmt == "yuv":  # plane sizes follow the source's sampling: one call each
        for name in c.names:
            want = yuv_scale_ref.scale_packed(source(name), rs)
            hyp = _decode(dec, c, [name], want.size, want.shape)
            np.testing.assert_array_equal(hyp[0], want, strict=True, err_msg=f"{c.id} {name}")
        return
    kw = dict(normalize=True, norm_dtype=c.norm) if c.norm else {}
    refs = [O.decode_resize(source(x), rs, pix_fmt=c.pix_fmt, **kw) for x in c.names]
    refs = [r.view(np.uint16) if c.norm else r for r in refs]
    hyp = _decode(dec, c, c.names, refs[0].size * len(refs), refs[0].shape)
    for i, (name, ref) in enumerate(zip(c.names, refs)):
        np.testing.assert_array_equal(hyp[i], ref, strict=True, err_msg=f"{c.id} {name}[{i}]")


def _ids(cs):
    return [c.id for c in cs]


@gpu
@pytest.mark.parametrize("c", PAIRS, ids=_ids(PAIRS))
def test_pixel_pairs(decoder, oracle, c):
    """Even scaled widths (one work item per chroma column and its one or two
    pixels), odd ones (full chroma: one column per thread), tiles that begin
    or end inside a pair, on every sampling; gray and RGB-coded frames keep
    their own writers."""
    _check(decoder, oracle, c)


@gpu
@pytest.mark.parametrize("c", ROWS, ids=_ids(ROWS))
def test_row_modes_and_dealing(decoder, oracle, c):
    """Bands of 1, 2, 3 and 5 rows, every row writer (X, Two, One, One with a
    chroma blend) and rows of more than 64 pairs, paired and unpaired."""
    _check(decoder, oracle, c)


@gpu
@pytest.mark.parametrize("c", PAD, ids=_ids(PAD))
def test_pad_rectangles(decoder, oracle, c):
    """Tiles of pad alone, of content alone, across one pad edge and across
    two: the u8 tile in all four layouts and the normalised fp16 / bf16
    stores (whose pad is (0 - mean) / std)."""
    _check(decoder, oracle, c)


@gpu
@pytest.mark.parametrize("c", DOT4, ids=_ids(DOT4))
def test_dot4_horizontal_pass(decoder, oracle, c):
    """0 / 255 bars of period 1, 2, 3 and 7 and a texture through every
    register bucket of the horizontal pass, in sws_kernel, hscale_kernel
    (forced pre-pass) and yuv_planes_kernel."""
    _check(decoder, oracle, c)


# ---- CPU: what the table reaches, and the tap split --------------------------------
def _tile_kinds(p: dict) -> set:
    kinds = set()
    rb, cc, ow, oh = p["rb"], p["col_chunk"], p["ow"], p["oh"]
    dx, dy, sw, sh = p["dx"], p["dy"], p["sw"], p["sh"]
    for y0 in range(0, oh, rb):
        y1 = min(y0 + rb, oh)
        for x0 in range(0, ow, cc):
            x1 = min(x0 + cc, ow)
            if not (max(y0, dy) < min(y1, dy + sh) and max(x0, dx) < min(x1, dx + sw)):
                kinds.add("pad")
                continue
            e = [k for k, out in (("left", x0 < dx), ("right", x1 > dx + sw), ("top", y0 < dy),
                                  ("bottom", y1 > dy + sh)) if out]
            kinds.update(e or ["content"])
            if len(e) >= 2:
                kinds.add("two")
    return kinds


def _quads(taps: int) -> int:
    q = (taps + 3) // 4
    return next(b for b in (1, 2, 3, 4, 6, 8, 12, 16, 1 << 30) if q <= b)


def test_table_reaches_tiles_and_buckets():
    kinds = set()
    for c in PAD:
        kinds |= _tile_kinds(probe(c, c.names[0]))
    assert kinds >= {"pad", "content", "left", "right", "top", "bottom", "two"}, kinds
    buckets, modes = set(), set()
    for c in DOT4:
        for name in ("bar1_gray", "t420_8"):
            p = probe(c, name)
            assert p["rc"] == 0, (c.id, name)
            buckets.add(_quads(p["hl"]["taps"]))
            if not p["gray"]:
                buckets.add(_quads(p["hc"]["taps"]))
            if c.pre == 1:
                assert p["pre"], c.id
    assert buckets == {1, 2, 3, 4, 6, 8, 12, 16}, sorted(buckets)
    for c in (*PAIRS, *ROWS):
        for name in c.names:
            p = probe(c, name)
            assert p["rc"] == 0, (c.id, name)
            if meta(name)[2]:  # subsampled columns: pairs at even widths
                assert p["full"] == p["sw"] % 2, (c.id, name)
            if not (p["full"] or p["gray"] or p["gbr"]):  # the paired writers' rows
                modes |= {(int(v) & 15, bool((int(v) >> 17) & 8191)) for v in p["vmode"]}
    assert modes >= {(0, False), (1, False), (1, True), (2, True)}, modes


def test_tap_split_restores_every_tap():
    """tap = 256 hi + lo with lo in 0..255 and hi a signed byte, on every tap
    table the cases above use."""
    seen = 0
    for c in ALL:
        for name in c.names:
            p = probe(c, name)
            assert p["rc"] == 0, (c.id, name)
            for ax in ("hl", "hc", "vl", "vc"):
                t = p[ax]["coef"].astype(np.int32)
                hi, lo = t >> 8, t & 255
                ok = (256 * hi + lo == t).all() and hi.min(initial=0) >= -128 and hi.max(initial=0) <= 127
                assert ok, (f"{c.id} {name} {ax}: the dot4 split assumes int16 taps, -32768 .. 32767, "
                            f"with hi = tap >> 8 in -128 .. 127; the table holds {t.min()} .. {t.max()}")
                seen += t.size
    assert seen


def test_dot4_sum_equals_the_tap_sum_on_bars():
    """udot4(p, lo) + 256 (sdot4(p ^ 0x80, hi) + 128 sum hi) == sum p tap
    (mod 2^32) for every output column of every bar row and filter."""
    for c in DOT4:
        if c.pre != -1 or c.pix_fmt != "rgb24":
            continue
        hl = probe(c, "bar1_gray")["hl"]
        t = hl["coef"].astype(np.int64)
        hi, lo = t >> 8, t & 255
        for k in BAR_PERIODS:
            row = np.concatenate([bar_row(k), np.zeros(t.shape[1], np.uint8)]).astype(np.int64)
            win = row[hl["pos"][:, None] + np.arange(t.shape[1])[None]]
            want = (win * t).sum(axis=1)
            signed = (win ^ 0x80) - 256 * ((win ^ 0x80) >= 128)  # the byte p ^ 0x80 as int8
            u = (win * lo).sum(axis=1) % (1 << 32)
            s = ((signed * hi).sum(axis=1) + 128 * hi.sum(axis=1)) % (1 << 32)
            got = (u + (s << 8)) % (1 << 32)
            np.testing.assert_array_equal(got, want % (1 << 32), err_msg=f"{c.id} period {k}")
