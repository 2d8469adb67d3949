"""CPU tests of frames at the format's limits (no GPU): sides of 32767 ..
65535 pixels through the header probe, the oracle's entropy decoder (against
libjpeg up to its 65500), the scale planner (against the oracle's plan), the
ratio limit of the scaler, and the stated limits of the layout planner.

The sources are tests/extreme_cases.py; the GPU side is test_gpu_extreme.py.
"""

import ctypes
import io

import numpy as np
import pytest

from spdl_amd import _lib
from spdl_amd._lib import Output
from tests import extreme_cases as X
from tests.test_sws_plan import BAD_GEOMETRY, _axis_src, check_plan

FILTERS = ("bicubic", "bilinear", "lanczos")
UNSUPPORTED = 2


# ---- the sources ---------------------------------------------------------------------

def test_the_source_table_covers_the_grid():
    """Every (long, short, orientation) size is there, every sampling meets
    every long side in both orientations, and 65535 is hand-written."""
    sizes = {(s.w, s.h) for s in X.SOURCES.values()}
    assert sizes == {(a, b) for L in X.LONG for S in X.SHORT for a, b in ((L, S), (S, L))}
    seen = {(s.samp, max(s.w, s.h), s.tall) for s in X.SOURCES.values()}
    assert seen == {(k, L, t) for k in X.SAMPLINGS for L in X.LONG for t in (False, True)}
    assert all(s.enc == "hw" for s in X.ALL.values() if not s.libjpeg)
    assert {s.enc for s in X.SOURCES.values()} == {"pil", "pilp", "hw"}
    assert len(X.HANDWRITTEN_65535) >= 12


@pytest.mark.parametrize("name", list(X.ALL))
def test_probe_and_levels(oracle, name):
    """The product's header probe equals the oracle's parse; the oracle's
    levels equal libjpeg's (files up to 65500) or the written ones (the
    hand-written files); Pillow's luma is within 1 of the oracle's islow plane
    (the bound of test_jpeg_headers: Pillow's YCbCr round trip)."""
    s, data = X.ALL[name], X.source(name)
    info, ref = _lib.get_image_info(data), oracle.parse(data)
    assert (info.width, info.height, info.ncomp) == (s.w, s.h, len(X.SAMPLINGS[s.samp]))
    assert (info.width, info.height, info.ncomp) == (ref.width, ref.height, ref.ncomp)
    for c in range(info.ncomp):
        assert (info.h_samp[c], info.v_samp[c]) == (ref.comp_h[c], ref.comp_v[c]), c
        assert (info.h_samp[c], info.v_samp[c]) == X.SAMPLINGS[s.samp][c], c
    assert info.multiscan == ref.multiscan == int(s.enc == "pilp")
    coefs, levels = oracle.decode_coefs(data)
    assert coefs.shape == (s.nblocks, 64)
    if s.enc == "hw":
        for got, want in zip(levels, X.written_levels(name)):
            np.testing.assert_array_equal(got, want)
    if not s.libjpeg:
        return
    if oracle.ljpin() is not None:
        got = oracle.lj_read_coefs(data)
        assert len(got) == len(levels)
        for g, w in zip(got, levels):
            np.testing.assert_array_equal(g, w)
    from PIL import Image

    im = Image.open(io.BytesIO(data))
    assert im.size == (s.w, s.h)
    if info.ncomp == 1:
        luma = np.asarray(im).astype(int)
    else:
        im.draft("YCbCr", im.size)
        luma = np.asarray(im.convert("YCbCr"))[..., 0].astype(int)
    plane = oracle.decode_planes(data, oracle.IDCT_ISLOW)[0].astype(int)
    assert luma.shape == plane.shape and np.abs(luma - plane).max() <= 1


# ---- planner against oracle ---------------------------------------------------------------

PLAN_SUBS = ((0, 0, "yuv"), (1, 1, "yuv"), (1, 0, "yuv"), (2, 0, "yuv"), (0, 0, "gray"))


def destinations(w, h):
    """Identity, 1/2, 1/3, 1/63, 1/64, twice the short side (capped at 65535),
    one column, one row, and the widest output."""
    def div(k):
        return max(1, -(-w // k)), max(1, -(-h // k))
    up = (w, min(2 * h, 65535)) if w > h else (min(2 * w, 65535), h)
    return list(dict.fromkeys([(w, h), div(2), div(3), div(63), div(64), up, (1, h), (w, 1),
                               (65535, h)]))


def plan_cells():
    """(w, h, dw, dh, hsub, vsub, mode, filter): every size of the source
    table, every destination, the samplings and the filters rotating over
    them (each size sees all five samplings and all three filters)."""
    sizes = sorted({(s.w, s.h) for s in X.SOURCES.values()})
    for i, (w, h) in enumerate(sizes):
        for j, (dw, dh) in enumerate(destinations(w, h)):
            for k in range(2):
                hsub, vsub, mode = PLAN_SUBS[(i + 2 * j + 3 * k) % 5]
                yield w, h, dw, dh, hsub, vsub, mode, FILTERS[(i + j + k) % 3]


def test_extreme_plans_match_oracle(oracle):
    n = refused = 0
    seen = set()
    for w, h, dw, dh, hsub, vsub, mode, filt in plan_cells():
        out = Output(pix_fmt="rgb24", resize=True, fit_w=dw, fit_h=dh, filter=filt)
        p = _lib.debug_sws_plan(w, h, hsub, vsub, mode, out)
        q = oracle.sws_plan(w, h, hsub, vsub, mode == "gray", dw, dh, filt)
        check_plan(p, q, _axis_src(w, h, hsub, vsub, mode == "gray"),
                   f"{w}x{h}->{dw}x{dh} {filt} sub{hsub}{vsub} {mode}", True)
        # no accepted plan has an axis at a ratio of 32768 or more
        assert q is None or max(w // dw, h // dh) < 32768, (w, h, dw, dh)
        n += 1
        refused += q is None
        seen.add((w, h, filt))
        seen.add((w, h, hsub, vsub, mode))
    assert n >= 600 and 0 < refused < n
    # every size under every filter and every sampling
    assert len(seen) == 40 * (len(FILTERS) + len(PLAN_SUBS))


# ---- the ratio limit -----------------------------------------------------------------------

def _axis_plan(oracle, axis, src, dst, filt, mode="gray", hsub=0, vsub=0):
    w, h, dw, dh = (src, 8, dst, 8) if axis == "h" else (8, src, 8, dst)
    out = Output(pix_fmt="rgb24", resize=True, fit_w=dw, fit_h=dh, filter=filt)
    p = _lib.debug_sws_plan(w, h, hsub, vsub, mode, out)
    q = oracle.sws_plan(w, h, hsub, vsub, mode == "gray", dw, dh, filt)
    return p, q, _axis_src(w, h, hsub, vsub, mode == "gray")


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("axis", ["h", "v"])
def test_ratio_boundary(oracle, axis, filt):
    """src -> 1 is refused by product and oracle from 32767 through 65535:
    below 32768 by the 256-tap limit, from 32768 on because swscale's int
    increment no longer holds the ratio (before the fix the wrapped value
    selected an upscale's four taps at position 0)."""
    for src in (32767, 32768, 32769, 40000, 65535):
        p, q, _ = _axis_plan(oracle, axis, src, 1, filt)
        assert q is None, f"{axis} {filt}: the oracle accepts {src} -> 1"
        assert p["rc"] == BAD_GEOMETRY, f"{axis} {filt}: the product accepts {src} -> 1 ({p['rc']})"


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("axis", ["h", "v"])
@pytest.mark.parametrize("src", [32768, 65535])
def test_ratio_boundary_nearest_accepted(oracle, axis, filt, src):
    """Walking dst up from the 256-tap estimate: the first accepted dst has a
    filter just under 256 taps (one dst step moves the window by less than a
    tap, the alignment by at most 4 and the 0.002 cut-off trims a few: within
    16 of the limit), and matches the oracle tap for tap."""
    factor = {"bicubic": 4, "bilinear": 2, "lanczos": 6}[filt]
    dst = factor * src // 256
    key = "hl" if axis == "h" else "vl"
    for _ in range(64):
        p, q, srcs = _axis_plan(oracle, axis, src, dst, filt)
        if q is not None:
            break
        assert p["rc"] == BAD_GEOMETRY, (src, dst)
        dst += 1
    assert q is not None, f"no accepted dst near {dst}"
    check_plan(p, q, srcs, f"{axis} {src}->{dst} {filt}", True)
    assert 240 <= q[key]["size"] < 256, q[key]["size"]
    assert p[key]["taps"] > 128


@pytest.mark.parametrize("filt", FILTERS)
def test_chroma_axis_refused_on_its_own_ratio(oracle, filt):
    """65535 -> 2 columns of a 4:2:2 frame: chroma 32768 -> 1.  The plan is
    refused in both, and so is the chroma axis taken alone (the oracle's
    axis entry, which the planar tests build their references from)."""
    p, q, _ = _axis_plan(oracle, "h", 65535, 2, filt, "yuv", 1, 0)
    assert q is None and p["rc"] == BAD_GEOMETRY
    for src in (32768, 32769, 65535):
        with pytest.raises(oracle.OracleError):
            oracle.sws_axis(src, 1, filt, src_pos=64, dst_pos=128)
    out = Output(pix_fmt="yuv", resize=True, fit_w=2, fit_h=8, filter=filt)
    assert _lib.debug_sws_plan(65535, 8, 1, 0, "yuv", out)["rc"] == BAD_GEOMETRY


# ---- the limits ----------------------------------------------------------------------------------

def test_header_only_frame_is_probed(oracle):
    """65535 x 65535 4:4:4: 8192 x 8192 x 3 blocks, past nblocks < 2^24.  The
    probe and the oracle's parse read it; nothing decodes it here (the GPU
    test pins the decoder's refusal)."""
    data = X.header_only()
    info, ref = _lib.get_image_info(data), oracle.parse(data)
    assert (info.width, info.height, info.ncomp) == (65535, 65535, 3)
    assert (ref.width, ref.height, ref.nblocks) == (65535, 65535, 3 * 8192 * 8192)
    assert ref.nblocks >= 1 << 24


@pytest.mark.parametrize("spec", [
    dict(fit_w=65535, fit_h=8, pad_w=65536, pad_h=8),  # a pad over the limit
    dict(fit_w=65536, fit_h=8),  # an upscale over it
    dict(fit_w=8, fit_h=65536),
])
def test_output_sides_over_65535_are_refused(spec):
    out = Output(pix_fmt="rgb24", resize=True, **spec)
    assert _lib.debug_sws_plan(32768, 8, 0, 0, "yuv", out)["rc"] == BAD_GEOMETRY
    ow, oh = ctypes.c_int32(), ctypes.c_int32()
    c = out.to_c()
    assert _lib.lib().spdl_hj_output_size(32768, 8, ctypes.byref(c), ctypes.byref(ow),
                                          ctypes.byref(oh)) == BAD_GEOMETRY


def test_output_side_of_65535_is_accepted():
    out = Output(pix_fmt="rgb24", resize=True, fit_w=65535, fit_h=8)
    assert _lib.output_size(32768, 8, out) == (65535, 8)
    assert _lib.debug_sws_plan(32768, 8, 0, 0, "yuv", out)["rc"] == 0
