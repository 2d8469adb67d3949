"""GPU tests of frames at the format's limits (-m gpu): sides of 32767 ..
65535 pixels (tests/extreme_cases.py) through every stage of the C-ABI,
bit-exact against the oracle, tests/src_crop_ref.py or tests/yuv_scale_ref.py;
the decoder's stated limits; and output and input buffers past 2^31 and 2^32
bytes.

Batches are [ordinary, extreme, ordinary] wherever the images may differ in
size (every scaled output); where the output is the frame itself the
neighbours are the same size's other sampling (a full-resolution batch has one
size).  Every output buffer has 0xA5 guard bytes behind it.

The limits, as the decoder has them today:
  * nblocks >= 2^24 (the 65535 x 65535 header): the planner refuses the CALL on
    the host -- the image's status is SPDL_HJ_ERR_UNSUPPORTED, its neighbours'
    statuses stay 0, but none of them is decoded: no output byte is written
    and ``last_ticket()`` does not move;
  * a scaled or output side over 65535, a scale filter of 256 taps or more, a
    ratio of 32768 or more: SPDL_HJ_ERR_BAD_GEOMETRY, likewise on the host.
"""

import functools
import time

import numpy as np
import pytest
import torch

from spdl_amd import _lib
from spdl_amd._lib import Output, ViewGroup
from spdl_amd.synthetic import synthetic_jpeg
from tests import cases
from tests import extreme_cases as X
from tests import src_crop_ref as cref
from tests import yuv_scale_ref as yref
from tests.test_extreme import FILTERS, destinations

pytestmark = pytest.mark.gpu

GUARD = 0xA5
UNSUPPORTED, BAD_GEOMETRY = 2, 7
KEYS = [(k, t) for k in X.SAMPLINGS for t in (False, True)]
IDS = [f"{k}-{'tall' if t else 'wide'}" for k, t in KEYS]
PLANAR_YUV = ("gray", "444", "422", "420")  # the frame formats the planar output takes


@functools.lru_cache(maxsize=None)
def ordinary(seed=5) -> bytes:
    return synthetic_jpeg(seed, 40, 40)  # (40 -> 1 is a filter swscale still takes)


@pytest.fixture
def knobs(decoder):
    """Set decoder parameters for one test; put back afterwards."""
    saved = {}

    def set_(name, value):
        saved.setdefault(name, -1 if name == "chain_after" else decoder.get_param(name))
        decoder.set_param(name, value)

    yield set_
    for k, v in saved.items():
        decoder.set_param(k, v)


def _decode(dec, datas, out, shape, **kw):
    """(statuses, [n, *shape]) of one decode_batch into a guarded buffer (16-bit
    outputs as their bit patterns)."""
    n = len(datas)
    esz = 1 if out.torch_dtype == torch.uint8 else 2
    per = int(np.prod(shape)) * esz
    t = torch.full((n * per + 4096,), GUARD, dtype=torch.uint8, device="cuda:0")
    st = dec.decode_batch(datas, out, t.data_ptr(), n * per, **kw)
    a = t.cpu().numpy()
    assert (a[n * per:] == GUARD).all(), "wrote past the batch's output"
    body = a[: n * per]
    if esz == 2:
        body = body.view(np.uint16)
    return st, body.reshape(n, *shape)


def _eq(got, want, msg):
    np.testing.assert_array_equal(got, want, strict=True, err_msg=msg)


def _twin(s: X.Source) -> X.Source:
    """The source table's other sampling of the same size."""
    return next(t for t in X.SOURCES.values() if (t.w, t.h) == (s.w, s.h) and t.name != s.name)


# ---- coefficients and planes ----------------------------------------------------------------

@pytest.mark.parametrize("name", X.HANDWRITTEN_65535)
def test_entropy_of_the_handwritten_65535_sources(decoder, oracle, name):
    d = X.source(name)
    ref, _ = oracle.decode_coefs(d)
    hyp, _, diag = decoder.debug_entropy(d, ref.shape[0])
    assert diag["status"] == 0, diag
    _eq(hyp, ref, name)


@pytest.mark.parametrize("name", list(X.ALL))
def test_planes_of_every_source_with_both_idcts(decoder, oracle, name):
    """Every source of the table, the restart layouts and the multi-scan files
    included."""
    d = X.source(name)
    for idct, oi in (("simple", oracle.IDCT_SIMPLE), ("islow", oracle.IDCT_ISLOW)):
        hyp, ref = decoder.decode_planes(d, idct=idct), oracle.decode_planes(d, idct=oi)
        assert len(hyp) == len(ref)
        for c, (h, r) in enumerate(zip(hyp, ref)):
            _eq(h, r, f"{name} {idct} plane {c}")


def test_pieces_and_chain_rounds_on_the_two_largest_files(decoder, oracle, knobs):
    """16 KiB entropy pieces and chain rounds from the first sync round on: the
    files are 20 and more pieces long."""
    big = sorted(X.ALL, key=lambda n: len(X.source(n)))[-2:]
    assert all(len(X.source(n)) > 8 * 16 * 1024 for n in big), [len(X.source(n)) for n in big]
    knobs("entropy_piece_bytes", 16 * 1024)
    knobs("chain_after", 1)
    for name in big:
        d = X.source(name)
        for h, r in zip(decoder.decode_planes(d), oracle.decode_planes(d)):
            _eq(h, r, name)
        s = X.ALL[name]
        rs = dict(fit_w=max(1, s.w // 32), fit_h=max(1, s.h // 32))
        ref = oracle.decode_resize(d, oracle.Resize(**rs))
        st, got = _decode(decoder, [ordinary(), d, ordinary()],
                          Output(pix_fmt="rgb24", resize=True, **rs), ref.shape)
        assert st == [0, 0, 0]
        _eq(got[1], ref, name)
        _eq(got[0], oracle.decode_resize(ordinary(), oracle.Resize(**rs)), "neighbour")
        _eq(got[2], got[0], "neighbour")


# ---- full resolution ---------------------------------------------------------------------------

@pytest.mark.parametrize("samp,tall", KEYS, ids=IDS)
def test_full_resolution(decoder, oracle, knobs, samp, tall):
    """rgb24 through the fused kernel and output_path 1 and 2, csc="jfif",
    planar rgb as fp16 and bf16, and the frame's own planes.  The pick is an odd
    long side where the table has one: 4:2:0 / 4:2:2 then take the general
    scaler; the even twin below takes the unscaled converter."""
    s = X.pick(samp, tall)
    batch = [s, _twin(s), s]
    datas = [X.source(b.name) for b in batch]
    refs = [oracle.decode_rgb(d, oracle.IDCT_SIMPLE, "rgb24") for d in datas]
    for path in (0, 1, 2):
        knobs("output_path", path)
        st, got = _decode(decoder, datas, Output(pix_fmt="rgb24"), refs[0].shape)
        assert st == [0, 0, 0]
        for k in range(3):
            _eq(got[k], refs[k], f"{batch[k].name} output_path {path}")
    knobs("output_path", 0)
    st, got = _decode(decoder, datas, Output(pix_fmt="rgb24", csc="jfif"), refs[0].shape)
    assert st == [0, 0, 0]
    for k in range(3):
        _eq(got[k], oracle.decode_rgb(datas[k], oracle.IDCT_SIMPLE, "rgb24", csc="jfif"),
            f"{batch[k].name} jfif")
    for norm in ("float16", "bfloat16"):
        out = Output(pix_fmt="rgb", normalize=True, norm_dtype=norm)
        want = [oracle.decode_resize(d, oracle.Resize(), "rgb", normalize=True,
                                     norm_dtype=norm).view(np.uint16) for d in datas]
        st, got = _decode(decoder, datas, out, want[0].shape)
        assert st == [0, 0, 0]
        for k in range(3):
            _eq(got[k], want[k], f"{batch[k].name} planar {norm}")
    if samp in PLANAR_YUV:
        want = yref.packed(oracle.decode_planes(datas[0]))
        st, got = _decode(decoder, [datas[0], datas[0]], Output(pix_fmt="yuv"), want.shape)
        assert st == [0, 0]
        _eq(got[0], want, f"{s.name} planes")
        _eq(got[1], want, f"{s.name} planes")


@pytest.mark.parametrize("samp", ["422", "420"])
@pytest.mark.parametrize("tall", [False, True])
def test_full_resolution_even_side_takes_the_unscaled_converter(decoder, oracle, samp, tall):
    s = X.pick(samp, tall, lambda s: s.w % 2 == 0 and s.h % 2 == 0)
    hsub, vsub = s.shifts
    assert _lib.debug_sws_plan(s.w, s.h, hsub, vsub, "yuv", Output(pix_fmt="rgb24"))["special"] == 1
    d = X.source(s.name)
    ref = oracle.decode_rgb(d, oracle.IDCT_SIMPLE, "rgb24")
    st, got = _decode(decoder, [d, d], Output(pix_fmt="rgb24"), ref.shape)
    assert st == [0, 0]
    _eq(got[0], ref, s.name)
    _eq(got[1], ref, s.name)


# ---- scaled ------------------------------------------------------------------------------------------

def _scaled_cells(oracle, s: X.Source):
    """(dw, dh, filter, accepted) per destination of the CPU grid whose output
    stays under about 1 MP; the filters rotate."""
    hsub, vsub = s.shifts
    out = []
    for j, (dw, dh) in enumerate(destinations(s.w, s.h)):
        if (dw, dh) == (s.w, s.h) or dw * dh > 1_200_000:
            continue
        filt = FILTERS[j % 3]
        q = oracle.sws_plan(s.w, s.h, hsub, vsub, s.samp == "gray", dw, dh, filt)
        # (the neighbours are scaled to the same size: 40 -> dw, 40 -> dh)
        qn = oracle.sws_plan(40, 40, 1, 1, False, dw, dh, filt)
        assert qn is not None
        out.append((dw, dh, filt, q is not None))
    return out


@pytest.mark.parametrize("samp,tall", KEYS, ids=IDS)
def test_scaled_and_refused(decoder, oracle, knobs, samp, tall):
    """Every accepted destination under the default pre-pass choice and with the
    pre-pass forced on and off; every refused one in a call of its own (status
    BAD_GEOMETRY, nothing written), then an exact decode.  What the product
    refuses is exactly what the oracle refuses."""
    s = X.pick(samp, tall)
    d = X.source(s.name)
    hsub, vsub = s.shifts
    mode = "gray" if samp == "gray" else "yuv"
    cells = _scaled_cells(oracle, s)
    assert sum(ok for *_, ok in cells) >= 3, cells
    assert any(not ok for *_, ok in cells), cells
    good = None
    for dw, dh, filt, ok in cells:
        out = Output(pix_fmt="rgb24", resize=True, fit_w=dw, fit_h=dh, filter=filt)
        tag = f"{s.name} -> {dw}x{dh} {filt}"
        if not ok:
            t = torch.full((1 << 16,), GUARD, dtype=torch.uint8, device="cuda:0")
            st = decoder.decode_batch([d], out, t.data_ptr(), t.numel(), check=False)
            assert st == [BAD_GEOMETRY], f"{tag}: {st}"
            assert bool((t == GUARD).all()), f"{tag}: a refused call wrote output"
            continue
        rs = oracle.Resize(fit_w=dw, fit_h=dh, filter=filt)
        ref = oracle.decode_resize(d, rs)
        nref = oracle.decode_resize(ordinary(), rs)
        for pre in (-1, 1, 0):
            if _lib.debug_sws_plan(s.w, s.h, hsub, vsub, mode, out, prepass=pre)["rc"]:
                assert pre == 0, f"{tag}: refused with the pre-pass allowed"
                continue
            knobs("sws_prepass", pre)
            st, got = _decode(decoder, [ordinary(), d, ordinary()], out, ref.shape)
            assert st == [0, 0, 0], tag
            _eq(got[1], ref, f"{tag} pre={pre}")
            _eq(got[0], nref, f"{tag} pre={pre}: neighbour")
            _eq(got[2], nref, f"{tag} pre={pre}: neighbour")
        knobs("sws_prepass", -1)
        good = good or (out, ref)
    # after the refusals: an exact decode
    st, got = _decode(decoder, [d], good[0], good[1].shape)
    assert st == [0]
    _eq(got[0], good[1], "after the refusals")


def test_scaled_planar_yuv(decoder, oracle):
    """pix_fmt="yuv" of a wide 4:2:0 and a tall 4:2:2 source, halved and cut to
    1/63 (the longest filters), against tests/yuv_scale_ref.py."""
    for s in (X.pick("420", False, lambda s: s.w % 2 == 0 and s.h % 2 == 0),
              X.pick("422", True, lambda s: s.w % 2 == 0)):
        d = X.source(s.name)
        for k, filt in ((2, "bicubic"), (63, "bilinear")):
            dw, dh = (s.w // k // 2 * 2, s.h) if s.w > s.h else (s.w, s.h // k // 2 * 2)
            rs = oracle.Resize(fit_w=dw, fit_h=dh, filter=filt)
            want = yref.scale_packed(d, rs)
            out = Output(pix_fmt="yuv", resize=True, fit_w=dw, fit_h=dh, filter=filt)
            st, got = _decode(decoder, [d, d], out, want.shape)
            assert st == [0, 0]
            _eq(got[0], want, f"{s.name} -> {dw}x{dh}")
            _eq(got[1], want, f"{s.name} -> {dw}x{dh}")


def test_4096_column_chunks(decoder, oracle, knobs):
    """sws_cols 16 on a 65535-wide output: 4096 column chunks, the last one 15
    wide."""
    s = X.pick("444", False, lambda s: s.w == 65535)
    d = X.source(s.name)
    out = Output(pix_fmt="rgb24", resize=True, fit_w=65535, fit_h=2 * s.h)
    p = _lib.debug_sws_plan(s.w, s.h, 0, 0, "yuv", out, max_cols=16)
    assert p["rc"] == 0 and p["chunks"] == 4096 and p["col_chunk"] == 16
    rs = oracle.Resize(fit_w=65535, fit_h=2 * s.h)
    ref, nref = oracle.decode_resize(d, rs), oracle.decode_resize(ordinary(), rs)
    knobs("sws_cols", 16)
    st, got = _decode(decoder, [ordinary(), d, ordinary()], out, ref.shape)
    assert st == [0, 0, 0]
    _eq(got[1], ref, s.name)
    _eq(got[0], nref, "neighbour")
    _eq(got[2], nref, "neighbour")


# ---- crops and views ------------------------------------------------------------------------------

def _far(s: X.Source, back: int):
    """A 64 x 8 (tall: 8 x 64) rectangle `back` samples before the far end --
    resolve clamps it into the frame -- and the one from pixel 0 to the last."""
    short = min(s.w, s.h, 8)
    if s.tall:
        return (0, s.h - back, short, 64), (0, 0, s.w, s.h)
    return (s.w - back, 0, 64, short), (0, 0, s.w, s.h)


@pytest.mark.parametrize("samp,tall", KEYS, ids=IDS)
def test_crops_at_the_far_end(decoder, oracle, samp, tall):
    s = X.pick(samp, tall, lambda s: min(s.w, s.h) >= 8)
    d = X.source(s.name)
    far, whole = _far(s, 9)
    # (a) the far-end region, scaled to 32 x 32 between ordinary images
    spec = dict(fit_w=32, fit_h=32)
    out = Output(pix_fmt="rgb24", resize=True, **spec)
    rs = oracle.Resize(**spec)
    want = cref.rgb(d, cref.resolve_data(d, far), rs)
    st, got = _decode(decoder, [ordinary(), d, ordinary()], out, want.shape,
                      crops=[None, far, None])
    assert st == [0, 0, 0]
    _eq(got[1], want, f"{s.name} {far}")
    _eq(got[0], oracle.decode_resize(ordinary(), rs), "neighbour")
    _eq(got[2], got[0], "neighbour")
    # (b) the same region at full resolution (its own size), and as planes
    want = cref.rgb(d, cref.resolve_data(d, far), None)
    st, got = _decode(decoder, [d, d], Output(pix_fmt="rgb24"), want.shape, crops=[far, far])
    assert st == [0, 0]
    _eq(got[0], want, f"{s.name} {far} full resolution")
    _eq(got[1], want, f"{s.name} {far} full resolution")
    # (c) pixel 0 to the last as a rectangle, scaled by 1/32 on the long side
    spec = dict(fit_w=s.w if tall else s.w // 32, fit_h=s.h // 32 if tall else s.h)
    rs = oracle.Resize(**spec)
    want = cref.rgb(d, cref.resolve_data(d, whole), rs)
    st, got = _decode(decoder, [ordinary(), d], Output(pix_fmt="rgb24", resize=True, **spec),
                      want.shape, crops=[None, whole])
    assert st == [0, 0]
    _eq(got[1], want, f"{s.name} whole span")
    _eq(got[0], oracle.decode_resize(ordinary(), rs), "neighbour")


@pytest.mark.parametrize("samp,tall", [("444", False), ("420", True), ("411", False),
                                       ("gray", True)])
def test_views_at_both_ends(decoder, oracle, samp, tall):
    """Two views of one extreme image, at pixel 0 and at the far end, in one
    group with a view of an ordinary image."""
    s = X.pick(samp, tall, lambda s: min(s.w, s.h) >= 8)
    d = X.source(s.name)
    far, _ = _far(s, 64)
    near = (0, 0, far[2], far[3])
    spec = dict(fit_w=24, fit_h=24)
    out, rs = Output(pix_fmt="rgb24", resize=True, **spec), oracle.Resize(**spec)
    views = [(1, near), (0, None), (1, far)]
    per = 24 * 24 * 3
    t = torch.full((4 * per,), GUARD, dtype=torch.uint8, device="cuda:0")
    g = ViewGroup(out, views, t.data_ptr(), 3 * per)
    st = decoder.decode_batch([ordinary(), d], Output(pix_fmt="rgb24"), 0, 0, views=[g])
    assert st == [0, 0] and g.statuses == [0, 0, 0]
    a = t.cpu().numpy()
    assert (a[3 * per:] == GUARD).all(), "wrote past the group's output"
    a = a[:3 * per].reshape(3, 24, 24, 3)
    _eq(a[0], cref.rgb(d, cref.resolve_data(d, near), rs), f"{s.name} {near}")
    _eq(a[1], oracle.decode_resize(ordinary(), rs), "the ordinary image's view")
    _eq(a[2], cref.rgb(d, cref.resolve_data(d, far), rs), f"{s.name} {far}")


# ---- flips and orientations --------------------------------------------------------------------------

def _oriented(a, code, planar):
    ax_w, ax_h = (a.ndim - 1, a.ndim - 2) if planar else (1, 0)
    if code & 4:
        a = np.swapaxes(a, ax_w, ax_h)
    if code & 1:
        a = np.flip(a, ax_w)
    if code & 2:
        a = np.flip(a, ax_h)
    return np.ascontiguousarray(a)


@pytest.mark.parametrize("fmt", ["rgb24", "f16"])
@pytest.mark.parametrize("size", [(65535, 8), (8, 65535)])
def test_flips_and_orientations(decoder, oracle, size, fmt):
    """Flips 1..3 (the frame's own box) and codes 4..7 (65535 x 8 lands in
    8 x 65535, and the reverse), at full resolution."""
    s = next(s for s in X.SOURCES.values() if (s.w, s.h) == size and s.samp != "gray")
    d = X.source(s.name)
    if fmt == "rgb24":
        out, planar = Output(pix_fmt="rgb24"), False
        base = oracle.decode_rgb(d, oracle.IDCT_SIMPLE, "rgb24")
    else:
        out, planar = Output(pix_fmt="rgb", normalize=True), True
        base = oracle.decode_resize(d, oracle.Resize(), "rgb", normalize=True).view(np.uint16)
    for codes in ((1, 2, 3), (4, 5, 6, 7)):
        wants = [_oriented(base, c, planar) for c in codes]
        st, got = _decode(decoder, [d] * len(codes), out, wants[0].shape, orients=list(codes))
        assert st == [0] * len(codes)
        for k, c in enumerate(codes):
            _eq(got[k], wants[k], f"{s.name} code {c} {fmt}")
    # ... and the flips through spdl_hj_set_flips
    wants = [_oriented(base, c, planar) for c in (0, 1, 2, 3)]
    st, got = _decode(decoder, [d] * 4, out, wants[0].shape, flips=[0, 1, 2, 3])
    assert st == [0] * 4
    for c in range(4):
        _eq(got[c], wants[c], f"{s.name} flip {c} {fmt}")


@pytest.mark.parametrize("samp,tall", [("420", False), ("422", True), ("444", False),
                                       ("gray", True)])
def test_planar_yuv_flips(decoder, oracle, samp, tall):
    """The frame's own planes with flips 0..3: every plane mirrored by its own
    size."""
    s = X.pick(samp, tall)
    d = X.source(s.name)
    planes = oracle.decode_planes(d)
    wants = [yref.packed([_oriented(p, c, True) for p in planes]) for c in range(4)]
    st, got = _decode(decoder, [d] * 4, Output(pix_fmt="yuv"), wants[0].shape, flips=[0, 1, 2, 3])
    assert st == [0] * 4
    for c in range(4):
        _eq(got[c], wants[c], f"{s.name} flip {c}")


# ---- the limits --------------------------------------------------------------------------------------

def test_too_many_blocks_is_refused_on_the_host(decoder, oracle):
    """The 65535 x 65535 header between two ordinary images: see the header
    comment for what happens to each of them."""
    datas = [ordinary(), X.header_only(), ordinary()]
    out = Output(pix_fmt="rgb24", resize=True, fit_w=32, fit_h=32)
    ticket = decoder.last_ticket()
    t = torch.full((3 * 32 * 32 * 3 + 4096,), GUARD, dtype=torch.uint8, device="cuda:0")
    st = decoder.decode_batch(datas, out, t.data_ptr(), 3 * 32 * 32 * 3, check=False)
    assert st == [0, UNSUPPORTED, 0]
    torch.cuda.synchronize()
    assert bool((t == GUARD).all()), "a refused submission wrote output"
    assert decoder.last_ticket() == ticket
    with pytest.raises(RuntimeError, match="image 1: image too large"):
        decoder.decode_batch(datas, out, t.data_ptr(), 3 * 32 * 32 * 3)
    assert decoder.last_ticket() == ticket
    # the same neighbours without it: exact
    ref = oracle.decode_resize(ordinary(), oracle.Resize(fit_w=32, fit_h=32))
    st, got = _decode(decoder, [ordinary(), ordinary()], out, ref.shape)
    assert st == [0, 0]
    _eq(got[0], ref, "after the refusal")
    assert decoder.last_ticket() == ticket + 1


@pytest.mark.parametrize("spec", [dict(fit_w=65535, fit_h=8, pad_w=65536, pad_h=8),
                                  dict(fit_w=65536, fit_h=8)])
def test_output_side_over_65535_is_refused_on_the_host(decoder, spec):
    s = X.pick("444", False, lambda s: s.h == 8)
    ticket = decoder.last_ticket()
    t = torch.full((1 << 16,), GUARD, dtype=torch.uint8, device="cuda:0")
    st = decoder.decode_batch([X.source(s.name)], Output(pix_fmt="rgb24", resize=True, **spec),
                              t.data_ptr(), t.numel(), check=False)
    assert st == [BAD_GEOMETRY]
    torch.cuda.synchronize()
    assert bool((t == GUARD).all()) and decoder.last_ticket() == ticket


# ---- buffers past 2^31 and 2^32 --------------------------------------------------------------------------

def _tiny_16x16() -> bytes:
    return synthetic_jpeg(11, 16, 16)


@pytest.mark.parametrize("fmt,n", [("rgb24", 352), ("f16", 176)])
def test_output_buffer_past_4_gib(decoder, oracle, fmt, n):
    """n copies of one 16 x 16 source scaled to 2048 x 2048 into one tensor of
    4.125 GiB (rgb24: bytes past 2^32; planar fp16: elements past 2^31), guard
    bytes on both sides.  The flips cycle 0..3, so a row that lands in another
    row's or image's place differs.  One oracle image and its three flips,
    compared on the device."""
    d = _tiny_16x16()
    spec = dict(fit_w=2048, fit_h=2048)
    rs = oracle.Resize(**spec)
    if fmt == "rgb24":
        out = Output(pix_fmt="rgb24", resize=True, **spec)
        base = torch.from_numpy(oracle.decode_resize(d, rs))
        dims = (1, 0)  # (w, h) axes
    else:
        out = Output(pix_fmt="rgb", normalize=True, resize=True, **spec)
        base = torch.from_numpy(oracle.decode_resize(d, rs, "rgb", normalize=True).view(np.int16))
        dims = (2, 1)
    refs = []
    for f in range(4):
        r = base
        if f & 1:
            r = torch.flip(r, (dims[0],))
        if f & 2:
            r = torch.flip(r, (dims[1],))
        refs.append(r.contiguous().to("cuda:0"))
    assert len({r.cpu().numpy().tobytes() for r in refs}) == 4, "the flips do not differ"
    per = base.numel()
    esz = base.element_size()
    assert n * per * esz > (1 << 32) and (esz == 1 or n * per > (1 << 31))
    G = 4096  # guard elements on each side
    buf = torch.full((n * per + 2 * G,), GUARD if esz == 1 else 0x5A5A, dtype=base.dtype,
                     device="cuda:0")
    body = buf[G:G + n * per]
    flips = [i % 4 for i in range(n)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = decoder.decode_batch([d] * n, out, body.data_ptr(), n * per * esz, flips=flips)
    torch.cuda.synchronize()
    print(f"\noutput past 4 GiB, {fmt}: {n} images, decode {time.perf_counter() - t0:.2f} s")
    assert st == [0] * n
    guard = GUARD if esz == 1 else 0x5A5A
    assert bool((buf[:G] == guard).all()) and bool((buf[G + n * per:] == guard).all()), \
        "wrote outside the batch's output"
    body = body.view(n, *base.shape)
    bad = [i for i in range(n) if not torch.equal(body[i], refs[flips[i]])]
    assert not bad, f"images {bad[:8]} of {n} differ (first at byte {bad[0] * per * esz})"


def test_input_buffer_past_4_gib(decoder, oracle):
    """decode_batch_device over a zeroed device buffer of 4 GiB + 1 MiB: small
    files at offset 0, straddling 2^31, at 2^31, straddling 2^32 and behind
    2^32, each against the oracle."""
    pool = [cases.case(n) for n in ("q90_420", "restart_rows", "prog_420", "gray",
                                    "restart_every_mcu", "q90_444")]
    assert all(len(f) > 512 for f in pool)
    total = (1 << 32) + (1 << 20)
    dev = torch.zeros((total,), dtype=torch.uint8, device="cuda:0")
    # (a file that straddles 2^31 covers the byte at 2^31: two layouts)
    for which, offs in enumerate(([0, (1 << 31) - 256, (1 << 32) - 256, (1 << 32) + (1 << 19)],
                                  [256, 1 << 31, 1 << 32, (1 << 32) + (1 << 19) + 256])):
        files = [pool[(k + 3 * which) % len(pool)] for k in range(len(offs))]
        _decode_at(decoder, oracle, dev, offs, files)
        dev.zero_()


def _decode_at(decoder, oracle, dev, offs, files):
    total = dev.numel()
    sizes = [len(f) for f in files]
    assert all(o % 256 == 0 for o in offs)
    assert all(a + n + 64 <= b for a, n, b in zip(offs, sizes, offs[1:] + [total]))
    for o, f in zip(offs, files):
        dev[o:o + len(f)] = torch.frombuffer(bytearray(f), dtype=torch.uint8).to("cuda:0")
    infos = [_lib.get_image_info(f) for f in files]
    spec = dict(fit_w=48, fit_h=40)
    out = Output(pix_fmt="rgb24", resize=True, **spec)
    per = 40 * 48 * 3
    n = len(files)
    t = torch.full((n * per + 4096,), GUARD, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = decoder.decode_batch_device(dev.data_ptr(), dev.numel(), offs, sizes, infos, out,
                                     t.data_ptr(), n * per)
    torch.cuda.synchronize()
    print(f"\ninput past 4 GiB: {n} files at {offs}, decode {time.perf_counter() - t0:.2f} s")
    assert st == [0] * n
    a = t.cpu().numpy()
    assert (a[n * per:] == GUARD).all(), "wrote past the batch's output"
    a = a[:n * per].reshape(n, 40, 48, 3)
    rs = oracle.Resize(**spec)
    for k, f in enumerate(files):
        _eq(a[k], oracle.decode_resize(f, rs), f"file {k} at offset {offs[k]}")
