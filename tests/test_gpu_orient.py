"""GPU tests of output orientations (spdl_hj_set_orients; -m gpu): the eight
orientations of a rectangle -- the flips, and a transpose ahead of them -- in
the store of sws_kernel, per image and per view, and EXIF orientation on top.

An orientation is the chain's last node and a pure permutation, so the
expected bytes are ``np.transpose`` + ``np.flip`` of what the existing
references state -- the oracle (``decode_resize`` / ``decode_rgb``),
``tests/src_crop_ref.py`` for crops and views, ``tests/yuv_scale_ref.py`` for
the planar output -- never of the library's own output.  For a code with the
transpose bit the reference runs the SWAPPED spec (the output spec describes
the final output).  Every comparison is bit-exact.  Output buffers are
pre-filled with 0xA5 and carry a 0xA5 tail.

The shapes are the smallest at which the store can go wrong: a final pitch of
3 * 37 bytes (odd: every row segment starts at another offset within 4 bytes,
so byte heads, word bodies and byte tails all occur), several column chunks
with a ragged last one, several bands with a ragged last one; each case asserts
through the plan probe (``debug_sws_plan``) that it has them.
"""

import ctypes
import io

import numpy as np
import pytest
import torch

import spdl_amd.io as sio
from spdl_amd import _lib
from spdl_amd._lib import Output, ViewGroup
from tests import cases
from tests import src_crop_ref as cref
from tests import yuv_scale_ref as yref

pytestmark = pytest.mark.gpu

BAD_GEOMETRY, INVALID_ARG = 7, 8
GUARD = 0xA5
F37 = dict(resize=True, fit_w=37, fit_h=50)  # the FINAL box: 37 wide, 50 tall
ALL = list(range(8))


@pytest.fixture
def knobs(decoder):
    """Set decoder parameters for one test; put back afterwards."""
    saved = {}

    def set_(name, value):
        saved.setdefault(name, decoder.get_param(name))
        decoder.set_param(name, value)

    yield set_
    for k, v in saved.items():
        decoder.set_param(k, v)


def _swapped(spec):
    """The chain ahead of a transpose: every pair of the final spec swapped."""
    s = dict(spec)
    for a, b in (("fit_w", "fit_h"), ("pad_w", "pad_h"), ("crop_w", "crop_h")):
        if a in spec or b in spec:
            s[a], s[b] = spec.get(b, 0), spec.get(a, 0)
    return s


def _chain(spec, code):
    return _swapped(spec) if code & 4 else spec


def _rs(oracle, spec):
    return oracle.Resize(**{k: v for k, v in spec.items() if k != "resize"})


def _oriented(a, code, planar):
    """``a`` ([H, W, 3], or [3, H, W] / one plane [H, W] when ``planar``) under
    orientation ``code``: the header's formula in numpy."""
    ax_w, ax_h = (a.ndim - 1, a.ndim - 2) if planar else (1, 0)
    if code & 4:
        a = np.swapaxes(a, ax_w, ax_h)  # A(x, y) = C(y, x)
    if code & 1:
        a = np.flip(a, ax_w)
    if code & 2:
        a = np.flip(a, ax_h)
    return np.ascontiguousarray(a)


def _shape(out, w, h):
    return (3, h, w) if out.planar else (h, w, 3)


def _decode(dec, datas, out, shape, **kw):
    """(statuses, [n, *shape]) of one decode_batch into a guarded buffer
    (16-bit outputs as their bit patterns)."""
    n = len(datas)
    esz = 1 if out.torch_dtype == torch.uint8 else 2
    per = int(np.prod(shape)) * esz
    t = torch.full(((n + 1) * per,), GUARD, dtype=torch.uint8, device="cuda:0")
    st = dec.decode_batch(datas, out, t.data_ptr(), n * per, **kw)
    a = t.cpu().numpy()
    assert (a[n * per:] == GUARD).all(), "wrote past the batch's output"
    body = a[: n * per]
    if esz == 2:
        body = body.view(np.uint16)
    return st, body.reshape(n, *shape)


def _plan(oracle, data, out, **kw):
    """The plan the library makes of ``data``'s whole frame under ``out``."""
    info = oracle.parse(data)
    if info.ncomp == 1:
        hsub = vsub = 0
        mode = "gray"
    else:
        hs, vs = cref.ratios(info.ncomp, list(info.comp_h), list(info.comp_v))
        hsub, vsub = hs.bit_length() - 1, vs.bit_length() - 1
        mode = "yuv"
    p = _lib.debug_sws_plan(info.width, info.height, hsub, vsub, mode, out, **kw)
    assert p["rc"] == 0
    return p


_WANT = {}


def _want(oracle, data, out, spec):
    """The oracle's chain result, computed once per (file, chain, format)."""
    key = (id(data), tuple(sorted(spec.items())), out.pix_fmt, out.normalize, out.norm_dtype)
    if key not in _WANT:
        w = oracle.decode_resize(data, _rs(oracle, spec), pix_fmt=out.pix_fmt,
                                 normalize=out.normalize, norm_dtype=out.norm_dtype)
        _WANT[key] = w.view(np.uint16) if out.normalize else w
    return _WANT[key]


def _rgb_orients(dec, oracle, data, out, spec, codes, **kw):
    """Copies of ``data`` through ``out`` (the FINAL spec), one per code, against
    the oriented oracle; a transposed copy's oracle runs the swapped spec."""
    codes = [_lib._orient(c) for c in codes]
    wants = [_oriented(_want(oracle, data, out, _chain(spec, c)), c, out.planar) for c in codes]
    assert len({w.shape for w in wants}) == 1  # one final shape, whatever the code
    st, got = _decode(dec, [data] * len(codes), out, wants[0].shape, orients=codes, **kw)
    assert st == [0] * len(codes)
    for k, c in enumerate(codes):
        np.testing.assert_array_equal(got[k], wants[k], strict=True,
                                      err_msg=f"image {k}, code {c}")
    return got


# ---- all eight codes: column chunks with a ragged last one, an odd final pitch ----------

@pytest.mark.parametrize("pix_fmt", ["rgb24", "bgr24", "rgb", "bgr"])
def test_eight_codes_over_column_chunks(decoder, oracle, knobs, pix_fmt):
    d = cases.case("q90_420")
    out = Output(pix_fmt=pix_fmt, **F37)
    for spec in (F37, _swapped(F37)):  # the plain images' chain, the transposed ones'
        p = _plan(oracle, d, Output(pix_fmt=pix_fmt, **spec), max_cols=16)
        assert p["chunks"] >= 2 and spec["fit_w"] % p["col_chunk"], p
    knobs("sws_cols", 16)
    _rgb_orients(decoder, oracle, d, out, F37, ALL)


# ---- several bands, a ragged last one ---------------------------------------------------

@pytest.mark.parametrize("pix_fmt", ["rgb24", "rgb"])
def test_bands_with_a_ragged_last_one(decoder, oracle, pix_fmt):
    d = cases.case("q90_420")
    spec = None
    for oh in (37, 53, 71, 97, 131, 181, 241):  # the first height the default tiler cuts in bands
        s = dict(resize=True, fit_w=48, fit_h=oh)
        p = _plan(oracle, d, Output(pix_fmt=pix_fmt, **s))
        if p["bands"] >= 2 and oh % p["rb"]:
            spec = s
            break
    assert spec is not None, "no height with two bands and a ragged last one"
    # final oh x 48: the transposed images run `spec`, banded; the plain ones its swap
    _rgb_orients(decoder, oracle, d, Output(pix_fmt=pix_fmt, **_swapped(spec)), _swapped(spec),
                 [4, 5, 6, 7, 0, 3])


# ---- pad and crop ---------------------------------------------------------------------------

def test_unequal_pads_land_where_the_formula_says(decoder, oracle, knobs):
    """odd_227x333 (333 x 227) under ``decrease``, padded into a FINAL 63 x 65:
    the transposed chain scales into 64 x 64 -> 64 x 44 and pads to 65 x 63 --
    one spare column right of the content, 9 pad rows above and 10 below --
    which the transpose turns into rows and columns."""
    d = cases.case("odd_227x333")
    knobs("sws_cols", 16)
    spec = dict(resize=True, fit_w=64, fit_h=64, aspect="decrease", pad_w=63, pad_h=65)
    g = oracle.geometry(333, 227, _rs(oracle, _swapped(spec)))
    assert (g["sw"], g["sh"], g["ow"], g["oh"], g["dx"], g["dy"]) == (64, 44, 65, 63, 0, 9)
    out = Output(pix_fmt="rgb24", **spec)
    assert _plan(oracle, d, Output(pix_fmt="rgb24", **_swapped(spec)), max_cols=16)["chunks"] >= 2
    got = _rgb_orients(decoder, oracle, d, out, spec, [4, 5, 6, 7])  # (63 < 64: no plain image fits)
    # code 4, the plain transpose: the chain's 9 pad rows are the 9 left columns,
    # its 10 the right ones, and its spare right column the bottom row
    assert not got[0][:, :9].any() and not got[0][:, 53:].any() and not got[0][64].any()
    assert got[0][:64, 9].any() and got[0][:64, 52].any()
    # code 5 (a quarter turn clockwise) mirrors that: 10 left, 9 right
    assert not got[1][:, :10].any() and not got[1][:, 54:].any() and got[1][:64, 10].any()
    # code 6: the spare row on top
    assert not got[2][0].any() and got[2][1:, 9].any()
    # an increase + crop chain
    spec = dict(resize=True, fit_w=40, fit_h=48, aspect="increase", crop_w=40, crop_h=48)
    _rgb_orients(decoder, oracle, d, Output(pix_fmt="rgb", **spec), spec, [5, 6, 7, 1])


# ---- normalised stores --------------------------------------------------------------------

@pytest.mark.parametrize("pix_fmt", ["rgb", "rgb24"])
@pytest.mark.parametrize("norm_dtype", ["float16", "bfloat16"])
def test_normalised_stores(decoder, oracle, knobs, norm_dtype, pix_fmt):
    d = cases.case("q90_420")
    out = Output(pix_fmt=pix_fmt, normalize=True, norm_dtype=norm_dtype, **F37)
    assert _plan(oracle, d, Output(pix_fmt=pix_fmt, **_swapped(F37)), max_cols=16)["chunks"] >= 2
    knobs("sws_cols", 16)
    _rgb_orients(decoder, oracle, d, out, F37, [4, 7, 2])
    # ... and with a pad, whose pixels go straight to the output as well
    spec = dict(resize=True, fit_w=40, fit_h=40, aspect="decrease", pad_w=45, pad_h=47)
    out = Output(pix_fmt=pix_fmt, normalize=True, norm_dtype=norm_dtype, **spec)
    _rgb_orients(decoder, oracle, d, out, spec, [5, 6, 0])


# ---- gbr and K-transform inputs, the pre-pass ------------------------------------------------

@pytest.mark.parametrize("name", ["rgb_coded", "cmyk_adobe"])
def test_gbr_and_k_transform_inputs(decoder, oracle, knobs, name):
    knobs("sws_cols", 16)
    _rgb_orients(decoder, oracle, cases.case(name), Output(pix_fmt="rgb24", **F37), F37, [5, 4, 0])


def test_prepass(decoder, oracle, knobs):
    d = cases.case("q90_420")
    out = Output(pix_fmt="rgb24", **F37)
    assert _plan(oracle, d, Output(pix_fmt="rgb24", **_swapped(F37)), prepass=1,
                 max_cols=16)["pre"] == 1
    knobs("sws_prepass", 1)
    knobs("sws_cols", 16)
    _rgb_orients(decoder, oracle, d, out, F37, [6, 7, 1])


# ---- full resolution -------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["q90_420", "odd_227x333"])
def test_full_resolution(decoder, oracle, name):
    d = cases.case(name)
    want = oracle.decode_rgb(d, oracle.IDCT_SIMPLE, "rgb24")
    h, w = want.shape[:2]
    out = Output(pix_fmt="rgb24")
    # one picture: codes without the transpose share a batch, and so do those with it
    for codes, shape in (([0, 1, 2, 3], (h, w, 3)), ([4, 5, 6, 7], (w, h, 3)), ([0, 3], (h, w, 3)),
                         ([5, 6], (w, h, 3))):
        st, got = _decode(decoder, [d] * len(codes), out, shape, orients=codes)
        assert st == [0] * len(codes)
        for k, c in enumerate(codes):
            np.testing.assert_array_equal(got[k], _oriented(want, c, False), strict=True,
                                          err_msg=f"code {c}")
    # ... a frame at code 0 beside its own code-5 partner does not: final sizes differ
    t = torch.full((2 * w * h * 3 + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    decoder.set_orients([0, 5])
    rc, msg = _raw(decoder, [d, d], out, t.data_ptr(), 2 * w * h * 3)
    assert rc == INVALID_ARG and "same output size" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert bool((t == GUARD).all())


def test_full_resolution_all_zero_is_no_call(decoder, oracle):
    """All-zero codes keep the fused full-resolution kernel, which launches no
    separate IDCT ("idct_workgroups" 0 with "output_path" 0); any code takes
    the generic output kernel behind idct_kernel."""
    d = cases.case("q90_420")
    want = oracle.decode_rgb(d, oracle.IDCT_SIMPLE, "rgb24")
    out = Output(pix_fmt="rgb24")
    assert decoder.get_param("output_path") == 0
    _, none = _decode(decoder, [d] * 2, out, want.shape)
    assert decoder.get_param("idct_workgroups") == 0
    _, zero = _decode(decoder, [d] * 2, out, want.shape, orients=[0, 0])
    assert decoder.get_param("idct_workgroups") == 0
    np.testing.assert_array_equal(none, zero, strict=True)
    np.testing.assert_array_equal(zero[1], want, strict=True)
    _decode(decoder, [d] * 2, out, want.shape, orients=[0, 3])
    assert decoder.get_param("idct_workgroups") > 0


# ---- crops ------------------------------------------------------------------------------------

def test_crops_with_transposes(decoder, oracle, knobs):
    """The rectangles stay in the stored frame's coordinates; the chain is swapped."""
    datas = [cases.case("q90_420"), cases.case("q90_444"), cases.case("q90_420")]
    rects = [(38, 22, 212, 150), (101, 67, 90, 120), (38, 22, 212, 150)]
    codes = [5, 6, 2]
    knobs("sws_cols", 16)
    for pix_fmt in ("rgb24", "rgb"):
        out = Output(pix_fmt=pix_fmt, **F37)
        st, got = _decode(decoder, datas, out, _shape(out, 37, 50), crops=rects, orients=codes)
        assert st == [0, 0, 0]
        for k, c in enumerate(codes):
            r = cref.resolve_data(datas[k], rects[k])
            want = cref.rgb(datas[k], r, _rs(oracle, _chain(F37, c)), pix_fmt)
            np.testing.assert_array_equal(got[k], _oriented(want, c, out.planar), strict=True,
                                          err_msg=f"{pix_fmt} image {k}")


# ---- views ---------------------------------------------------------------------------------------

def test_views_carry_their_own_codes(decoder, oracle, knobs):
    datas = [cases.case("q90_420"), cases.case("q90_444")]
    rect, rect1, big = (38, 22, 212, 150), (20, 10, 100, 80), (0, 0, 9999, 10)
    sa, sb = dict(resize=True, fit_w=37, fit_h=50), dict(resize=True, fit_w=24, fit_h=20)
    oa = Output(pix_fmt="rgb24", **sa)
    ob = Output(pix_fmt="rgb", normalize=True, norm_dtype="float16", **sb)
    va = [(0, rect), (0, rect, None, 5), (0, rect, "v"), (0, big, None, 7), (1, rect1, None, 6)]
    vb = [(1, rect1, None, "clock"), (0, big, 2), (0, rect, None, 4)]
    knobs("sws_cols", 16)
    bufs, groups = [], []
    for out, views, (w, h) in ((oa, va, (37, 50)), (ob, vb, (24, 20))):
        esz = 1 if out.torch_dtype == torch.uint8 else 2
        per = w * h * 3 * esz
        t = torch.full(((len(views) + 1) * per,), GUARD, dtype=torch.uint8, device="cuda:0")
        bufs.append((t, per))
        groups.append(ViewGroup(out, views, t.data_ptr(), len(views) * per))
    assert groups[0].orients == [None, 5, None, 7, 6] and groups[0].flips == [0, 0, 2, 0, 0]
    assert groups[1].orients == [5, None, 4]
    want_codes = [[0, 5, 2, 7, 6], [5, 2, 4]]
    st = decoder.decode_batch(datas, Output(pix_fmt="rgb24"), 0, 0, views=groups, check=False)
    assert st == [0, 0]
    assert groups[0].statuses == [0, 0, 0, BAD_GEOMETRY, 0]
    assert groups[1].statuses == [0, BAD_GEOMETRY, 0]
    for (t, per), out, spec, views, codes in zip(bufs, (oa, ob), (sa, sb), (va, vb), want_codes):
        a = t.cpu().numpy()
        assert (a[len(views) * per:] == GUARD).all(), "wrote past a group's output"
        for k, (image, r, *_) in enumerate(views):
            row = a[k * per:(k + 1) * per]
            rr = cref.resolve_data(datas[image], r)
            if rr is None:  # the refused view: its row untouched
                assert (row == GUARD).all(), f"refused view {k} was written"
                continue
            want = cref.rgb(datas[image], rr, _rs(oracle, _chain(spec, codes[k])), out.pix_fmt,
                            normalize=out.normalize, norm_dtype=out.norm_dtype)
            want = _oriented(want, codes[k], out.planar)
            if out.normalize:
                row, want = row.view(np.uint16), want.view(np.uint16)
            np.testing.assert_array_equal(row.reshape(want.shape), want, strict=True,
                                          err_msg=f"{out.pix_fmt} view {k}")
    # the codes are gone after one submission: the same views again with no
    # orientation and no flip named, so neither set_orients nor set_flips is called
    for g in groups:
        g.orients = [None] * len(g.orients)
        g.flips = [0] * len(g.flips)
    bufs[0][0].fill_(GUARD)
    decoder.decode_batch(datas, Output(pix_fmt="rgb24"), 0, 0, views=groups, check=False)
    a = bufs[0][0].cpu().numpy()
    per = bufs[0][1]
    np.testing.assert_array_equal(a[per:2 * per], a[:per], strict=True)
    np.testing.assert_array_equal(a[2 * per:3 * per], a[:per], strict=True)


# ---- planar YUV -----------------------------------------------------------------------------

def test_planar_yuv_takes_flip_codes_and_refuses_a_transpose(decoder, oracle, knobs):
    d = cases.case("q90_420")
    spec = dict(resize=True, fit_w=45, fit_h=31)
    planes = yref.scale_planes(d, _rs(oracle, spec))
    per = sum(p.size for p in planes)
    knobs("sws_cols", 16)
    out = Output(pix_fmt="yuv", **spec)
    st, got = _decode(decoder, [d] * 3, out, (per,), orients=[1, 2, 3])
    assert st == [0, 0, 0]
    for k, c in enumerate((1, 2, 3)):  # (test_gpu_flips' reference: every plane by its own size)
        want = yref.packed([_oriented(p, c, True) for p in planes])
        np.testing.assert_array_equal(got[k], want, strict=True, err_msg=f"code {c}")
    t = torch.full((2 * per + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    decoder.set_orients([0, 4])
    rc, msg = _raw(decoder, [d, d], out, t.data_ptr(), 2 * per)
    assert rc == INVALID_ARG and "planar YUV" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert bool((t == GUARD).all()), "a refused submission wrote output"


# ---- errors ---------------------------------------------------------------------------------------

def _raw(dec, datas, out, ptr, nbytes):
    """spdl_hj_decode_batch as it is: (rc, message)."""
    n = len(datas)
    keep = [_lib.buffer_address(d) for d in datas]
    ptrs = (ctypes.c_void_p * n)(*[k[0] for k in keep])
    sizes = (ctypes.c_size_t * n)(*[k[1] for k in keep])
    status = (ctypes.c_int32 * n)()
    err = ctypes.create_string_buffer(1024)
    spec = out.to_c()
    rc = _lib.lib().spdl_hj_decode_batch(dec._h, ptrs, sizes, n, ctypes.byref(spec), ptr, nbytes,
                                         None, 1, status, err, 1024)
    return rc, err.value.decode()


@pytest.mark.parametrize("orients, flips, out, text", [
    (bytes([5, 0, 1]), None, Output(pix_fmt="rgb24", **F37), "3 codes for 2 images"),
    (bytes([5]), None, Output(pix_fmt="rgb24", **F37), "1 codes for 2 images"),
    (bytes([0, 8]), None, Output(pix_fmt="rgb24", **F37), "code 1 is 8"),
    (bytes([0, 1]), None, Output(pix_fmt="rgb24", csc="jfif"), "csc = swscale"),
    (bytes([0, 5]), bytes([0, 1]), Output(pix_fmt="rgb24", **F37), "on one submission"),
])
def test_errors_write_nothing_and_consume_the_codes(decoder, oracle, orients, flips, out, text):
    datas = [cases.case("q90_420")] * 2
    w, h = (37, 50) if out.resize else (640, 480)
    t = torch.full((2 * w * h * 3 + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    decoder.set_orients(orients)
    if flips is not None:
        decoder.set_flips(flips)
    rc, msg = _raw(decoder, datas, out, t.data_ptr(), 2 * w * h * 3)
    assert rc == INVALID_ARG and text in msg, (rc, msg)
    torch.cuda.synchronize()
    assert bool((t == GUARD).all()), "a refused submission wrote output"
    # the failed call consumed them (both): the next one is a plain submission
    rc, msg = _raw(decoder, datas, out, t.data_ptr(), 2 * w * h * 3)
    assert rc == 0, msg
    torch.cuda.synchronize()
    got = t.cpu().numpy()[: 2 * w * h * 3].reshape(2, h, w, 3)
    np.testing.assert_array_equal(got[0], got[1], strict=True)
    if out.resize:
        np.testing.assert_array_equal(got[0], oracle.decode_resize(datas[0], _rs(oracle, F37)),
                                      strict=True)


def test_set_orients_null_clears_and_planes_leave_them(decoder, oracle):
    d = cases.case("q90_420")
    out = Output(pix_fmt="rgb24", **F37)
    want = oracle.decode_resize(d, _rs(oracle, F37))
    decoder.set_orients([5])
    decoder.set_orients(None)
    st, got = _decode(decoder, [d], out, want.shape)
    np.testing.assert_array_equal(got[0], want, strict=True)
    decoder.set_orients([6])
    planes = decoder.decode_planes(d)  # neither uses nor clears them
    np.testing.assert_array_equal(planes[0], oracle.decode_planes(d)[0], strict=True)
    st, got = _decode(decoder, [d], out, want.shape)
    np.testing.assert_array_equal(
        got[0], _oriented(oracle.decode_resize(d, _rs(oracle, _swapped(F37))), 6, False), strict=True)


# ---- the other entry points, both transports ------------------------------------------------

def _packed(datas):
    offs, total = [], 0
    for d in datas:
        offs.append(total)
        total += (len(d) + 64 + 255) // 256 * 256
    host = np.zeros(total + 512, np.uint8)
    for o, d in zip(offs, datas):
        host[o:o + len(d)] = np.frombuffer(d, np.uint8)
    return host, offs, [len(d) for d in datas], total


@pytest.mark.parametrize("host_staging", [1, 0])
def test_device_and_staged_entry_points(decoder, oracle, knobs, host_staging):
    datas = [cases.case("q90_420"), cases.case("q90_444"), cases.case("q90_422")]
    codes = [6, 0, 5]
    out = Output(pix_fmt="rgb24", **F37)
    want = [_oriented(oracle.decode_resize(d, _rs(oracle, _chain(F37, c))), c, False)
            for d, c in zip(datas, codes)]
    host, offs, sizes, total = _packed(datas)
    knobs("host_staging", host_staging)
    knobs("sws_cols", 16)
    n = 3 * 50 * 37 * 3
    dev = torch.from_numpy(host).to("cuda:0")
    infos = [_lib.get_image_info(d) for d in datas]
    t = torch.full((n + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    st = decoder.decode_batch_device(dev.data_ptr(), dev.numel(), offs, sizes, infos, out,
                                     t.data_ptr(), n, orients=codes)
    assert st == [0, 0, 0]
    a = t.cpu().numpy()
    assert (a[n:] == GUARD).all()
    for k in range(3):
        np.testing.assert_array_equal(a[:n].reshape(3, 50, 37, 3)[k], want[k], strict=True,
                                      err_msg=f"device, image {k}")
    t.fill_(GUARD)
    ptr, ticket = decoder.staging_acquire(total)
    ctypes.memmove(ptr, host.ctypes.data, total)
    st = decoder.decode_staged(ticket, total, offs, sizes, out, t.data_ptr(), n, orients=codes)
    assert st == [0, 0, 0]
    a = t.cpu().numpy()
    assert (a[n:] == GUARD).all()
    for k in range(3):
        np.testing.assert_array_equal(a[:n].reshape(3, 50, 37, 3)[k], want[k], strict=True,
                                      err_msg=f"staged, image {k}")
    st, got = _decode(decoder, datas, out, (50, 37, 3), orients=codes)
    for k in range(3):
        np.testing.assert_array_equal(got[k], want[k], strict=True, err_msg=f"host, image {k}")


# ---- the Python surface --------------------------------------------------------------------------

def _tagged(data, exif):
    """``data`` with an Exif APP1 of orientation ``exif`` as Pillow writes it (the
    coded image untouched: the segment goes in behind SOI)."""
    from PIL import Image

    ex = Image.Exif()
    ex[0x0112] = exif
    app1 = b"Exif\x00\x00" + ex.tobytes().removeprefix(b"Exif\x00\x00")
    return data[:2] + b"\xff\xe1" + (len(app1) + 2).to_bytes(2, "big") + app1 + data[2:]


def test_python_surface(oracle):
    pytest.importorskip("PIL")
    from PIL import Image

    cfg = sio.cuda_config(device_index=0)
    d = cases.case("q90_420")
    R = oracle.Resize
    tags = [1, 6, 8, 3]
    datas = [_tagged(d, t) for t in tags]
    for t, f in zip(tags, datas):  # (Pillow reads back what the files say)
        assert Image.open(io.BytesIO(f)).getexif()[0x0112] == t == _lib.get_orientation(f)
    box = {False: R(fit_w=64, fit_h=40, aspect="decrease", pad_w=64, pad_h=40),
           True: R(fit_w=40, fit_h=64, aspect="decrease", pad_w=40, pad_h=64)}
    chain = {t: oracle.decode_resize(d, box[bool(t)]) for t in (0, 4)}

    def want(code):
        return _oriented(chain[code & 4], code, False)

    # tags 1, 6, 8 and 3 of one picture into 64 x 40: the oracle of the swapped box, transposed
    buf = sio.load_image_batch(datas, width=64, height=40, device_config=cfg, exif_orientation=True)
    got = sio.to_torch(buf).cpu().numpy()
    assert got.shape == (4, 40, 64, 3)
    for k, t in enumerate(tags):
        np.testing.assert_array_equal(got[k], want(_lib.exif_code(t)), strict=True,
                                      err_msg=f"tag {t}")
    # without the flag the tags mean nothing
    buf = sio.load_image_batch(datas, width=64, height=40, device_config=cfg)
    np.testing.assert_array_equal(sio.to_torch(buf).cpu().numpy()[1], want(0), strict=True)
    # flips= on top: the flip acts on the displayed image
    flips = ["h", "h", "v", None]
    buf = sio.load_image_batch(datas, width=64, height=40, device_config=cfg, exif_orientation=True,
                               flips=flips)
    got = sio.to_torch(buf).cpu().numpy()
    for k, (t, f) in enumerate(zip(tags, flips)):
        shown = _oriented(want(_lib.exif_code(t)), _lib._flip(f), False)
        np.testing.assert_array_equal(got[k], shown, strict=True, err_msg=f"tag {t} flip {f}")
        np.testing.assert_array_equal(got[k], want(_lib.exif_code(t) ^ _lib._flip(f)), strict=True)
    # load_image: the flag, and transpose=clock at the end of the chain
    w64 = _oriented(oracle.decode_resize(d, R(fit_w=48, fit_h=64)), 5, False)  # final 64 x 48
    buf = sio.load_image(datas[1], device_config=cfg, exif_orientation=True,
                         filter_desc="scale=w=64:h=48:flags=bicubic,format=pix_fmts=rgb24")
    np.testing.assert_array_equal(sio.to_torch(buf).cpu().numpy(), w64, strict=True)
    buf = sio.load_image(d, device_config=cfg,
                         filter_desc="scale=w=48:h=64:flags=bicubic,transpose=clock,"
                                     "format=pix_fmts=rgb24")
    np.testing.assert_array_equal(sio.to_torch(buf).cpu().numpy(), w64, strict=True)
    # load_image_views: the image's tag on every view of it
    rect, rect1 = (38, 22, 212, 150), (20, 10, 100, 80)
    res = sio.load_image_views(
        [datas[1], datas[0]], [dict(width=48, height=40, scale_mode=None,
                                    crops=[[rect, rect], [rect1]], flips=[[0, "h"], ["v"]])],
        device_config=cfg, exif_orientation=True)
    (vbuf, idx), = res
    assert idx == [0, 0, 1]
    got = sio.to_torch(vbuf).cpu().numpy()
    assert got.shape == (3, 40, 48, 3)
    for k, (r, code) in enumerate(((rect, 5), (rect, 5 ^ 1), (rect1, 0 ^ 2))):
        rs = R(fit_w=40, fit_h=48) if code & 4 else R(fit_w=48, fit_h=40)
        w = cref.rgb(d, cref.resolve_data(d, r), rs, "rgb24")
        np.testing.assert_array_equal(got[k], _oriented(w, code, False), strict=True,
                                      err_msg=f"view {k}")
