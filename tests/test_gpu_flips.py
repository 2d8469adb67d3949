"""GPU tests of output flips (spdl_hj_set_flips; -m gpu): per-image and
per-view hflip / vflip in the store of sws_kernel and yuv_planes_kernel.

The flip is the chain's last node, so the expected bytes are ``np.flip`` of
what the existing references state for the unflipped chain -- the oracle
(``decode_resize`` / ``decode_rgb``), ``tests/src_crop_ref.py`` for crops and
views, ``tests/yuv_scale_ref.py`` for the planar output (flipped per plane) --
never of the library's own output.  Every comparison is bit-exact.  Output
buffers are pre-filled with 0xA5 and carry a 0xA5 tail.

The shapes are the smallest at which the store can go wrong, and each case
asserts through the plan probe (``debug_sws_plan``) that it really has the
several column chunks or bands it is about.
"""

import ctypes

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
S50 = dict(resize=True, fit_w=50, fit_h=37)  # 50 x 37: odd height, no multiple of 16 wide
NAMES = {0: "none", 1: "h", 2: "v", 3: "hv"}


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


def _rs(oracle, spec):
    return oracle.Resize(**{k: v for k, v in spec.items() if k != "resize"})


def _flipped(a, flip, planar):
    """``a`` ([H, W, 3], or [3, H, W] / one plane [H, W] when ``planar``) under ``flip``."""
    ax_w, ax_h = (a.ndim - 1, a.ndim - 2) if planar else (1, 0)
    if flip & 1:
        a = np.flip(a, ax_w)
    if flip & 2:
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


def _rgb_flips(dec, oracle, data, out, spec, flips, **kw):
    """Copies of ``data`` through ``out``, one per flip, against the flipped oracle."""
    want = oracle.decode_resize(data, _rs(oracle, spec), pix_fmt=out.pix_fmt,
                                normalize=out.normalize, norm_dtype=out.norm_dtype)
    if out.normalize:
        want = want.view(np.uint16)
    st, got = _decode(dec, [data] * len(flips), out, want.shape, flips=flips, **kw)
    assert st == [0] * len(flips)
    for k, f in enumerate(flips):
        np.testing.assert_array_equal(got[k], _flipped(want, _lib._flip(f), out.planar),
                                      strict=True, err_msg=f"image {k}, flip {f!r}")
    return got


# ---- several column chunks, a ragged last one ------------------------------------------

@pytest.mark.parametrize("pix_fmt", ["rgb24", "bgr24", "rgb", "bgr"])
def test_column_chunks_with_a_ragged_last_one(decoder, oracle, knobs, pix_fmt):
    d = cases.case("q90_420")
    out = Output(pix_fmt=pix_fmt, **S50)
    p = _plan(oracle, d, out, max_cols=16)
    assert p["chunks"] >= 2 and 50 % p["col_chunk"], p  # the last chunk is narrower
    knobs("sws_cols", 16)
    _rgb_flips(decoder, oracle, d, out, S50, [0, 1, 2, 3])


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
    _rgb_flips(decoder, oracle, d, Output(pix_fmt=pix_fmt, **spec), spec, ["h", "v", "hv"])


# ---- pad and crop ---------------------------------------------------------------------------

def test_pad_moves_with_the_image(decoder, oracle, knobs):
    """A flip that moved only the content would leave the unequal pads where
    they were.  odd_227x333 (333 x 227) under ``decrease`` into 64 x 64 scales
    to 64 x 44 -- ten pad rows above and below; into 65 x 63 the one spare
    column lies right of the content and the pad rows are 9 above, 10 below."""
    d = cases.case("odd_227x333")
    knobs("sws_cols", 16)
    for pw, ph, asym in ((64, 64, False), (65, 63, True)):
        spec = dict(resize=True, fit_w=64, fit_h=64, aspect="decrease", pad_w=pw, pad_h=ph)
        g = oracle.geometry(333, 227, _rs(oracle, spec))
        assert (g["sw"], g["sh"], g["ow"], g["oh"]) == (64, 44, pw, ph)
        assert (g["ow"] - g["sw"] - 2 * g["dx"] != 0) == asym
        assert (g["oh"] - g["sh"] - 2 * g["dy"] != 0) == asym
        out = Output(pix_fmt="rgb24", **spec)
        assert _plan(oracle, d, out, max_cols=16)["chunks"] >= 2
        got = _rgb_flips(decoder, oracle, d, out, spec, [1, 2, 3])
        if asym:  # the spare pad column is on the left of the h-flipped image
            assert not got[0][:, 0].any() and got[0][g["dy"]:g["dy"] + 44, -1].any()
    spec = dict(resize=True, fit_w=48, fit_h=40, aspect="increase", crop_w=48, crop_h=40)
    _rgb_flips(decoder, oracle, d, Output(pix_fmt="rgb", **spec), spec, [1, 2, 3])


# ---- normalised stores --------------------------------------------------------------------

@pytest.mark.parametrize("pix_fmt", ["rgb", "rgb24"])
@pytest.mark.parametrize("norm_dtype", ["float16", "bfloat16"])
def test_normalised_stores(decoder, oracle, knobs, norm_dtype, pix_fmt):
    d = cases.case("q90_420")
    out = Output(pix_fmt=pix_fmt, normalize=True, norm_dtype=norm_dtype, **S50)
    assert _plan(oracle, d, out, max_cols=16)["chunks"] >= 2
    knobs("sws_cols", 16)
    _rgb_flips(decoder, oracle, d, out, S50, ["h", "hv"])
    # ... and with a pad, whose pixels go straight to the output as well
    spec = dict(resize=True, fit_w=40, fit_h=40, aspect="decrease", pad_w=45, pad_h=37)
    out = Output(pix_fmt=pix_fmt, normalize=True, norm_dtype=norm_dtype, **spec)
    _rgb_flips(decoder, oracle, d, out, spec, ["h", "hv"])


# ---- planar YUV -----------------------------------------------------------------------------

def _yuv_flips(dec, oracle, data, spec, flips, **kw):
    planes = yref.scale_planes(data, _rs(oracle, spec))
    per = sum(p.size for p in planes)
    st, got = _decode(dec, [data] * len(flips), Output(pix_fmt="yuv", **spec), (per,), flips=flips,
                      **kw)
    assert st == [0] * len(flips)
    for k, f in enumerate(flips):
        want = yref.packed([_flipped(p, f, True) for p in planes])  # every plane by its own size
        np.testing.assert_array_equal(got[k], want, strict=True, err_msg=f"image {k}, flip {f}")
    return planes


@pytest.mark.parametrize("name", ["q90_420", "q90_422"])
def test_planar_yuv_odd_size(decoder, oracle, knobs, name):
    d = cases.case(name)
    spec = dict(resize=True, fit_w=45, fit_h=31)
    p = _plan(oracle, d, Output(pix_fmt="yuv", **spec), max_cols=16)
    # (a planar plan counts its tiles over the three planes: luma ceil(45 / 16) = 3
    # chunks, the last one of 13 columns; chroma, 23 wide, 2 chunks, the last of 7)
    assert p["planar"] and p["col_chunk"] == 16 and p["bands"] * p["chunks"] >= 3 + 2 * 2, p
    knobs("sws_cols", 16)
    planes = _yuv_flips(decoder, oracle, d, spec, [1, 2, 3])
    assert planes[1].shape[1] == 23  # cw = ceil(45 / 2): mirrored by 23, not by 45 / 2
    assert planes[1].shape[0] == (16 if name == "q90_420" else 31)


def test_planar_yuv_gray_and_padded_444(decoder, oracle, knobs):
    knobs("sws_cols", 16)
    _yuv_flips(decoder, oracle, cases.case("gray_odd"), dict(resize=True, fit_w=45, fit_h=31),
               [1, 2, 3])
    # 320 x 240 4:4:4 under decrease into 48 x 48: 48 x 36, padded to 51 x 41 --
    # one pad column left, two right; two pad rows above, three below; U = V = 128
    spec = dict(resize=True, fit_w=48, fit_h=48, aspect="decrease", pad_w=51, pad_h=41)
    planes = _yuv_flips(decoder, oracle, cases.case("q90_444"), spec, [1, 2, 3])
    assert (planes[1][:2] == 128).all() and (planes[1][:, 49:] == 128).all()
    assert (planes[0][:, 0] == 0).all() and planes[0][2:38, 1].any()
    # default tiling as well (one chunk per band)
    knobs("sws_cols", 256)
    _yuv_flips(decoder, oracle, cases.case("q90_444"), spec, [3, 0, 1])


def test_planar_yuv_full_resolution(decoder, oracle):
    d = cases.case("odd_227x333")
    planes = oracle.decode_planes(d)
    per = sum(p.size for p in planes)
    st, got = _decode(decoder, [d] * 3, Output(pix_fmt="yuv"), (per,), flips=[1, 2, 3])
    assert st == [0, 0, 0]
    for k, f in enumerate((1, 2, 3)):
        want = yref.packed([_flipped(p, f, True) for p in planes])
        np.testing.assert_array_equal(got[k], want, strict=True, err_msg=f"flip {f}")


# ---- gbr and K-transform inputs, the pre-pass ------------------------------------------------

@pytest.mark.parametrize("name", ["rgb_coded", "cmyk_adobe"])
def test_gbr_and_k_transform_inputs(decoder, oracle, knobs, name):
    knobs("sws_cols", 16)
    _rgb_flips(decoder, oracle, cases.case(name), Output(pix_fmt="rgb24", **S50), S50, ["h", 0])


def test_prepass(decoder, oracle, knobs):
    d = cases.case("q90_420")
    out = Output(pix_fmt="rgb24", **S50)
    assert _plan(oracle, d, out, prepass=1, max_cols=16)["pre"] == 1
    knobs("sws_prepass", 1)
    knobs("sws_cols", 16)
    _rgb_flips(decoder, oracle, d, out, S50, ["hv", "h"])


# ---- full resolution -------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["q90_420", "odd_227x333"])
def test_full_resolution(decoder, oracle, name):
    """q90_420 takes the fused kernel without flips (the unscaled converter
    with "output_path" 2), odd_227x333 the general scaler; a flipped batch
    takes the generic output kernel, whose pixels are the same."""
    d = cases.case(name)
    want = oracle.decode_rgb(d, oracle.IDCT_SIMPLE, "rgb24")
    out = Output(pix_fmt="rgb24")
    st, got = _decode(decoder, [d] * 4, out, want.shape, flips=[0, 1, 2, 3])
    assert st == [0] * 4
    for f in range(4):  # (image 0: the unflipped oracle)
        np.testing.assert_array_equal(got[f], _flipped(want, f, False), strict=True,
                                      err_msg=f"flip {f}")
    # no flips, and all-zero flips: the same bytes
    _, none = _decode(decoder, [d] * 4, out, want.shape, flips=None)
    _, zero = _decode(decoder, [d] * 4, out, want.shape, flips=[0, 0, 0, 0])
    np.testing.assert_array_equal(none, zero, strict=True)
    np.testing.assert_array_equal(none[3], want, strict=True)


def test_full_resolution_planar_rgb(decoder, oracle):
    d = cases.case("q90_420")
    want = oracle.decode_rgb(d, oracle.IDCT_SIMPLE, "bgr")
    st, got = _decode(decoder, [d] * 2, Output(pix_fmt="bgr"), want.shape, flips=["hv", "h"])
    np.testing.assert_array_equal(got[0], _flipped(want, 3, True), strict=True)
    np.testing.assert_array_equal(got[1], _flipped(want, 1, True), strict=True)


# ---- crops with flips ------------------------------------------------------------------------

def test_crops_with_flips(decoder, oracle, knobs):
    datas = [cases.case("q90_420"), cases.case("q90_444")]
    rects = [(38, 22, 212, 150), (101, 67, 90, 120)]
    spec = dict(resize=True, fit_w=50, fit_h=37)
    knobs("sws_cols", 16)
    for pix_fmt in ("rgb24", "rgb"):
        out = Output(pix_fmt=pix_fmt, **spec)
        st, got = _decode(decoder, datas, out, _shape(out, 50, 37), crops=rects, flips=[0, "hv"])
        assert st == [0, 0]
        for k, f in enumerate((0, 3)):
            r = cref.resolve_data(datas[k], rects[k])
            want = cref.rgb(datas[k], r, _rs(oracle, spec), pix_fmt)
            np.testing.assert_array_equal(got[k], _flipped(want, f, out.planar), strict=True,
                                          err_msg=f"{pix_fmt} image {k}")


# ---- views ---------------------------------------------------------------------------------------

def test_views_carry_their_own_flips(decoder, oracle, knobs):
    datas = [cases.case("q90_420"), cases.case("q90_444")]
    rect, rect1, big = (38, 22, 212, 150), (20, 10, 100, 80), (0, 0, 9999, 10)
    sa, sb = dict(resize=True, fit_w=50, fit_h=37), dict(resize=True, fit_w=24, fit_h=20)
    oa = Output(pix_fmt="rgb24", **sa)
    ob = Output(pix_fmt="rgb", normalize=True, norm_dtype="float16", **sb)
    va = [(0, rect, 0), (0, rect, 1), (0, rect, 2), (0, big, 3), (1, rect1, "hv")]
    vb = [(1, rect1, "h"), (0, big, 2), (0, rect, "v")]
    knobs("sws_cols", 16)
    bufs, groups = [], []
    for out, views, (w, h) in ((oa, va, (50, 37)), (ob, vb, (24, 20))):
        esz = 1 if out.torch_dtype == torch.uint8 else 2
        per = w * h * 3 * esz
        t = torch.full(((len(views) + 1) * per,), GUARD, dtype=torch.uint8, device="cuda:0")
        bufs.append((t, per))
        groups.append(ViewGroup(out, views, t.data_ptr(), len(views) * per))
    assert groups[0].flips == [0, 1, 2, 3, 3] and groups[1].flips == [1, 2, 2]
    st = decoder.decode_batch(datas, Output(pix_fmt="rgb24"), 0, 0, views=groups, check=False)
    assert st == [0, 0]
    assert groups[0].statuses == [0, 0, 0, BAD_GEOMETRY, 0]
    assert groups[1].statuses == [0, BAD_GEOMETRY, 0]
    for (t, per), g, out, spec, views, (w, h) in zip(bufs, groups, (oa, ob), (sa, sb), (va, vb),
                                                     ((50, 37), (24, 20))):
        a = t.cpu().numpy()
        assert (a[len(views) * per:] == GUARD).all(), "wrote past a group's output"
        for k, (image, r, _) in enumerate(views):
            row = a[k * per:(k + 1) * per]
            rr = cref.resolve_data(datas[image], r)
            if rr is None:  # the refused view: its row untouched
                assert (row == GUARD).all(), f"refused view {k} was written"
                continue
            want = cref.rgb(datas[image], rr, _rs(oracle, spec), out.pix_fmt,
                            normalize=out.normalize, norm_dtype=out.norm_dtype)
            want = _flipped(want, g.flips[k], out.planar)
            if out.normalize:
                row, want = row.view(np.uint16), want.view(np.uint16)
            np.testing.assert_array_equal(row.reshape(want.shape), want, strict=True,
                                          err_msg=f"{out.pix_fmt} view {k}")
    # the flips are gone after one submission: the same views, none flipped
    for g in groups:
        g.flips = [0] * len(g.flips)
    bufs[0][0].fill_(GUARD)
    decoder.decode_batch(datas, Output(pix_fmt="rgb24"), 0, 0, views=groups, check=False)
    a = bufs[0][0].cpu().numpy()
    per = bufs[0][1]
    np.testing.assert_array_equal(a[per:2 * per], a[:per], strict=True)


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


@pytest.mark.parametrize("flips, out, text", [
    (bytes([1, 0, 1]), Output(pix_fmt="rgb24", **S50), "3 flips for 2 images"),
    (bytes([1]), Output(pix_fmt="rgb24", **S50), "1 flips for 2 images"),
    (bytes([0, 4]), Output(pix_fmt="rgb24", **S50), "flip 1 is 4"),
    (bytes([0, 1]), Output(pix_fmt="rgb24", csc="jfif"), "csc = swscale"),
])
def test_errors_write_nothing_and_consume_the_flips(decoder, oracle, flips, out, text):
    datas = [cases.case("q90_420")] * 2
    w, h = (50, 37) if out.resize else (640, 480)
    t = torch.full((2 * w * h * 3 + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    decoder.set_flips(flips)
    rc, msg = _raw(decoder, datas, out, t.data_ptr(), 2 * w * h * 3)
    assert rc == INVALID_ARG and text in msg, (rc, msg)
    torch.cuda.synchronize()
    assert bool((t == GUARD).all()), "a refused submission wrote output"
    # the failed call consumed them: the next one is a plain submission
    rc, msg = _raw(decoder, datas, out, t.data_ptr(), 2 * w * h * 3)
    assert rc == 0, msg
    torch.cuda.synchronize()
    got = t.cpu().numpy()[: 2 * w * h * 3].reshape(2, h, w, 3)
    np.testing.assert_array_equal(got[0], got[1], strict=True)
    if out.resize:
        np.testing.assert_array_equal(got[0], oracle.decode_resize(datas[0], _rs(oracle, S50)),
                                      strict=True)


def test_set_flips_null_clears_and_planes_leave_them(decoder, oracle):
    d = cases.case("q90_420")
    out = Output(pix_fmt="rgb24", **S50)
    want = oracle.decode_resize(d, _rs(oracle, S50))
    decoder.set_flips([1])
    decoder.set_flips(None)
    st, got = _decode(decoder, [d], out, want.shape)
    np.testing.assert_array_equal(got[0], want, strict=True)
    # decode_planes neither uses nor clears them
    decoder.set_flips([2])
    planes = decoder.decode_planes(d)
    np.testing.assert_array_equal(planes[0], oracle.decode_planes(d)[0], strict=True)
    st, got = _decode(decoder, [d], out, want.shape)
    np.testing.assert_array_equal(got[0], _flipped(want, 2, False), strict=True)


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
    flips = [2, 0, 3]
    out = Output(pix_fmt="rgb24", **S50)
    want = [_flipped(oracle.decode_resize(d, _rs(oracle, S50)), f, False)
            for d, f in zip(datas, flips)]
    host, offs, sizes, total = _packed(datas)
    knobs("host_staging", host_staging)
    knobs("sws_cols", 16)
    n = 3 * 37 * 50 * 3
    # device-resident bytes
    dev = torch.from_numpy(host).to("cuda:0")
    infos = [_lib.get_image_info(d) for d in datas]
    t = torch.full((n + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    st = decoder.decode_batch_device(dev.data_ptr(), dev.numel(), offs, sizes, infos, out,
                                     t.data_ptr(), n, flips=flips)
    assert st == [0, 0, 0]
    a = t.cpu().numpy()
    assert (a[n:] == GUARD).all()
    for k in range(3):
        np.testing.assert_array_equal(a[:n].reshape(3, 37, 50, 3)[k], want[k], strict=True,
                                      err_msg=f"device, image {k}")
    # the staging ring
    t.fill_(GUARD)
    ptr, ticket = decoder.staging_acquire(total)
    ctypes.memmove(ptr, host.ctypes.data, total)
    st = decoder.decode_staged(ticket, total, offs, sizes, out, t.data_ptr(), n, flips=flips)
    assert st == [0, 0, 0]
    a = t.cpu().numpy()
    assert (a[n:] == GUARD).all()
    for k in range(3):
        np.testing.assert_array_equal(a[:n].reshape(3, 37, 50, 3)[k], want[k], strict=True,
                                      err_msg=f"staged, image {k}")
    # host bytes, same transport
    st, got = _decode(decoder, datas, out, (37, 50, 3), flips=flips)
    for k in range(3):
        np.testing.assert_array_equal(got[k], want[k], strict=True, err_msg=f"host, image {k}")


# ---- the Python surface --------------------------------------------------------------------------

def test_python_surface(oracle):
    cfg = sio.cuda_config(device_index=0)
    datas = [cases.case("q90_420"), cases.case("q90_444")]
    R = oracle.Resize
    # load_image_batch: the default chain (decrease + centred pad) and a flip per image
    buf = sio.load_image_batch(datas, width=64, height=40, device_config=cfg, flips=["h", None])
    got = sio.to_torch(buf).cpu().numpy()
    rs = R(fit_w=64, fit_h=40, aspect="decrease", pad_w=64, pad_h=40)
    np.testing.assert_array_equal(got[0], _flipped(oracle.decode_resize(datas[0], rs), 1, False),
                                  strict=True)
    np.testing.assert_array_equal(got[1], oracle.decode_resize(datas[1], rs), strict=True)
    # load_image: hflip at the end of the chain, and the keyword
    want = oracle.decode_resize(datas[0], R(fit_w=64, fit_h=64))
    buf = sio.load_image(datas[0], device_config=cfg,
                         filter_desc="scale=w=64:h=64:flags=bicubic,format=pix_fmts=rgb24,hflip")
    np.testing.assert_array_equal(sio.to_torch(buf).cpu().numpy(), _flipped(want, 1, False),
                                  strict=True)
    buf = sio.load_image(datas[0], device_config=cfg, flip="v",
                         filter_desc="scale=w=64:h=64:flags=bicubic,format=pix_fmts=rgb24")
    np.testing.assert_array_equal(sio.to_torch(buf).cpu().numpy(), _flipped(want, 2, False),
                                  strict=True)
    # load_image at full resolution with the keyword
    buf = sio.load_image(datas[1], device_config=cfg, flip="hv")
    np.testing.assert_array_equal(sio.to_torch(buf).cpu().numpy(),
                                  _flipped(oracle.decode_rgb(datas[1]), 3, False), strict=True)
    # load_image_views: flips parallel to crops
    rect, rect1 = (38, 22, 212, 150), (20, 10, 100, 80)
    res = sio.load_image_views(
        datas, [dict(width=48, height=40, scale_mode=None, crops=[[rect, rect], [rect1]],
                     flips=[[0, "h"], ["v"]])], device_config=cfg)
    (vbuf, idx), = res
    assert idx == [0, 0, 1]
    got = sio.to_torch(vbuf).cpu().numpy()
    rs = R(fit_w=48, fit_h=40)
    for k, (image, r, f) in enumerate(((0, rect, 0), (0, rect, 1), (1, rect1, 2))):
        want = cref.rgb(datas[image], cref.resolve_data(datas[image], r), rs, "rgb24")
        np.testing.assert_array_equal(got[k], _flipped(want, f, False), strict=True,
                                      err_msg=f"view {k}")
