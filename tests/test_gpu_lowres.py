"""GPU tests of the reduced-size decode (spdl_hj_set_lowres / ``lowres=``;
-m gpu): FFmpeg's lowres 1..3 in the IDCT stage.  Through the C-ABI
(``Decoder``) and the Python surface; every comparison is bit-exact against
``tests/lowres_ref.py``, a numpy restatement of the transforms on the oracle's
coefficients, with the chain run by the oracle on the reduced planes.
"""

import ctypes

import numpy as np
import pytest
import torch

import spdl_amd.io as sio
from spdl_amd import _lib
from spdl_amd._lib import Output, ViewGroup
from tests import cases
from tests import lowres_cases as lc
from tests import lowres_ref as ref

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID_ARG = 2, 8
GUARD = 0xA5


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


def _check_planes(dec, data, level):
    _, want = ref.planes(data, level)
    got = dec.decode_planes(data, lowres=level)
    assert len(got) == len(want)
    for c, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g, w, strict=True, err_msg=f"component {c} level {level}")


# ---- 1. planes: the transform alone ------------------------------------------------------------

@pytest.mark.parametrize("level", [1, 2, 3])
@pytest.mark.parametrize("samp", lc.SAMPLINGS)
def test_planes(decoder, oracle, samp, level):
    for w, h in lc.SIZES:
        _check_planes(decoder, lc.sized(samp, w, h), level)


@pytest.mark.parametrize("level", [1, 2, 3])
def test_planes_scan_structures(decoder, oracle, level):
    _check_planes(decoder, lc.sized("420", 50, 37, progressive=True), level)
    _check_planes(decoder, lc.sized("422", 64, 48, restart_marker_blocks=2), level)
    _check_planes(decoder, cases.case("multiscan_444_odd"), level)  # non-interleaved scans


@pytest.mark.parametrize("level", [1, 2, 3])
def test_planes_energy_outside_the_corner(decoder, oracle, level):
    """Every AC entry lies outside the 4x4 corner: the list walk passes some
    by, stops at the others, and the DC still comes through."""
    _check_planes(decoder, lc.outside_corner(), level)


def test_planes_level_0_and_consumption(decoder, oracle):
    d = lc.sized("420", 50, 37)
    full = oracle.decode_planes(d)
    for g, w in zip(decoder.decode_planes(d, lowres=0), full):
        np.testing.assert_array_equal(g, w, strict=True)
    # a level is consumed by the call it was set for
    _check_planes(decoder, d, 2)
    for g, w in zip(decoder.decode_planes(d), full):
        np.testing.assert_array_equal(g, w, strict=True)


# ---- 2. chains -------------------------------------------------------------------------------

def _check_rgb(dec, oracle, data, level, spec, pix_fmt="rgb24", code=0, **norm):
    """One image at ``level`` through chain ``spec`` (the FINAL output's; a
    transposed code runs it swapped) against the reference."""
    chain = dict(spec)
    if code & 4:
        for a, b in (("fit_w", "fit_h"), ("pad_w", "pad_h")):
            chain[a], chain[b] = spec.get(b, 0), spec.get(a, 0)
    rs = oracle.Resize(**chain) if spec else None
    want = ref.rgb(data, level, rs, pix_fmt, **norm)
    planar = pix_fmt in ("rgb", "bgr")
    ax_w, ax_h = (2, 1) if planar else (1, 0)
    if code & 4:
        want = np.swapaxes(want, ax_w, ax_h)
    if code & 1:
        want = np.flip(want, ax_w)
    if code & 2:
        want = np.flip(want, ax_h)
    want = np.ascontiguousarray(want)
    if want.dtype == np.float16:
        want = want.view(np.uint16)
    out = Output(pix_fmt=pix_fmt, resize=bool(spec), normalize=bool(norm),
                 **{k: v for k, v in norm.items() if k != "normalize"}, **spec)
    st, got = _decode(dec, [data], out, want.shape, lowres=[level],
                      **({"orients": [code]} if code else {}))
    assert st == [0]
    np.testing.assert_array_equal(got[0], want, strict=True)


CHAIN_SAMPLINGS = ["420", "422", "gray"]


@pytest.mark.parametrize("samp", CHAIN_SAMPLINGS)
def test_chain_scale_8x8_bicubic(decoder, oracle, samp):
    for level in (1, 2):
        _check_rgb(decoder, oracle, lc.sized(samp, 50, 37), level, dict(fit_w=8, fit_h=8))


@pytest.mark.parametrize("samp", CHAIN_SAMPLINGS)
def test_chain_bilinear_upscale(decoder, oracle, samp):
    """17x9 at level 2 is a 5x3 frame; up to 40x40."""
    _check_rgb(decoder, oracle, lc.sized(samp, 17, 9), 2,
               dict(fit_w=40, fit_h=40, filter="bilinear"), "rgb")


@pytest.mark.parametrize("samp", CHAIN_SAMPLINGS)
def test_chain_lanczos_with_pad(decoder, oracle, samp):
    spec = dict(fit_w=24, fit_h=24, aspect="decrease", pad_w=24, pad_h=24, filter="lanczos")
    _check_rgb(decoder, oracle, lc.sized(samp, 64, 48), 1, spec)
    _check_rgb(decoder, oracle, lc.sized(samp, 33, 31), 1, spec, "bgr24")


@pytest.mark.parametrize("samp", CHAIN_SAMPLINGS)
def test_chain_native_size(decoder, oracle, samp):
    """No scale: the generic output kernel on the reduced frame."""
    for level in (1, 3):
        _check_rgb(decoder, oracle, lc.sized(samp, 50, 37), level, {})
    assert decoder.get_param("idct_workgroups") > 0 and decoder.get_param("lowres_images") == 1


@pytest.mark.parametrize("samp", CHAIN_SAMPLINGS)
def test_chain_planar_yuv(decoder, oracle, samp):
    """64x48 at level 1: a 32x24 frame, even on both chroma axes."""
    d = lc.sized(samp, 64, 48)
    for spec in ({}, dict(fit_w=16, fit_h=12)):
        want = ref.planar(d, 1, oracle.Resize(**spec) if spec else None)
        out = Output(pix_fmt="yuv", resize=bool(spec), **spec)
        st, got = _decode(decoder, [d], out, want.shape, lowres=[1])
        assert st == [0]
        np.testing.assert_array_equal(got[0], want, strict=True)


@pytest.mark.parametrize("samp", CHAIN_SAMPLINGS)
def test_chain_variants(decoder, oracle, samp):
    d = lc.sized(samp, 50, 37)
    spec = dict(fit_w=20, fit_h=12)
    _check_rgb(decoder, oracle, d, 1, spec, "rgb", normalize=True, norm_dtype="float16")
    _check_rgb(decoder, oracle, d, 2, spec, "rgb24", code=1)  # a horizontal flip
    _check_rgb(decoder, oracle, d, 1, spec, "rgb24", code=5)  # transposed + flipped


# ---- 3. mixed levels -------------------------------------------------------------------------

MIXED = [0, 1, 2, 3, 0, 3]


def _mixed_files():
    return [lc.sized("420", 64, 48), lc.sized("422", 50, 37), lc.sized("gray", 33, 31),
            lc.sized("444", 64, 48), lc.sized("440", 50, 37), lc.sized("420", 50, 37)]


def test_mixed_levels_plain_batch(decoder, oracle):
    datas = _mixed_files()
    spec = dict(fit_w=16, fit_h=16)
    out = Output(pix_fmt="rgb24", resize=True, **spec)
    st, got = _decode(decoder, datas, out, (16, 16, 3), lowres=MIXED)
    assert st == [0] * 6 and decoder.get_param("lowres_images") == 4
    st, plain = _decode(decoder, datas, out, (16, 16, 3))
    assert st == [0] * 6 and decoder.get_param("lowres_images") == 0
    rs = oracle.Resize(**spec)
    for k, (d, level) in enumerate(zip(datas, MIXED)):
        want = plain[k] if level == 0 else ref.rgb(d, level, rs)
        np.testing.assert_array_equal(got[k], want, strict=True, err_msg=f"image {k}")
        if level == 0:
            np.testing.assert_array_equal(got[k], oracle.decode_resize(d, rs), strict=True)


def test_mixed_levels_ragged_native_size(decoder, oracle):
    datas = _mixed_files()
    cfg = sio.cuda_config(device_index=0)
    bufs, idx = sio.load_image_list(datas, device_config=cfg, lowres=MIXED)
    assert idx == list(range(6))
    assert _lib.thread_decoder(0).get_param("lowres_images") == 4
    plain, _ = sio.load_image_list(datas, device_config=cfg)
    for k, (d, level) in enumerate(zip(datas, MIXED)):
        got = sio.to_torch(bufs[k]).cpu().numpy()
        want = sio.to_torch(plain[k]).cpu().numpy() if level == 0 else ref.rgb(d, level, None)
        np.testing.assert_array_equal(got, want, strict=True, err_msg=f"image {k}")


# ---- 4. workspace hygiene --------------------------------------------------------------------

@pytest.mark.parametrize("samp,w,h,level", [("420", 50, 37, 1), ("422", 17, 9, 2), ("gray", 33, 31, 3),
                                            ("411", 50, 37, 3)])
def test_no_output_byte_depends_on_stale_planes(decoder, oracle, samp, w, h, level):
    """The same decode after a larger all-white and after a larger all-black
    image on the same decoder (the same workspace): identical outputs."""
    d = lc.sized(samp, w, h)
    spec = dict(fit_w=24, fit_h=24, aspect="decrease", pad_w=24, pad_h=24, filter="lanczos")
    out = Output(pix_fmt="rgb24", resize=True, **spec)
    full = Output(pix_fmt="rgb24")
    results = []
    for value in (255, 0):
        flood = cases._enc(np.full((96, 128, 3), value, np.uint8), quality=90, subsampling=0)
        st, px = _decode(decoder, [flood], full, (96, 128, 3))
        assert st == [0] and abs(int(px.mean()) - value) <= 1
        st, got = _decode(decoder, [d], out, (24, 24, 3), lowres=[level])
        assert st == [0]
        results.append(got)
    np.testing.assert_array_equal(results[0], results[1], strict=True)
    np.testing.assert_array_equal(results[0][0], ref.rgb(d, level, oracle.Resize(**spec)), strict=True)


# ---- 5. "auto" -------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,level", [(64, 48, 1), (200, 150, 3)])
def test_auto_equals_the_fixed_level(oracle, w, h, level):
    d = lc.sized("420", w, h)
    cfg = sio.cuda_config(device_index=0)
    info = _lib.get_image_info(d)
    box = Output(pix_fmt="rgb24", resize=True, fit_w=24, fit_h=24, aspect="decrease", pad_w=24,
                 pad_h=24)
    assert _lib.auto_lowres(info.width, info.height, box) == level
    kw = dict(width=24, height=24, pix_fmt="rgb24", device_config=cfg)
    auto = sio.to_torch(sio.load_image_batch([d], lowres="auto", **kw)).cpu().numpy()
    fixed = sio.to_torch(sio.load_image_batch([d], lowres=level, **kw)).cpu().numpy()
    conf = sio.to_torch(sio.load_image_batch(
        [d], decode_config=sio.decode_config(decoder_options={"lowres": str(level)}),
        **kw)).cpu().numpy()
    np.testing.assert_array_equal(auto, fixed, strict=True)
    np.testing.assert_array_equal(conf, fixed, strict=True)
    rs = oracle.Resize(fit_w=24, fit_h=24, aspect="decrease", pad_w=24, pad_h=24)
    np.testing.assert_array_equal(fixed[0], ref.rgb(d, level, rs), strict=True)


# ---- 6. refusals -----------------------------------------------------------------------------

def _raw(dec, datas, out, ptr, nbytes):
    """spdl_hj_decode_batch as it is: (rc, message, statuses)."""
    n = len(datas)
    keep = [_lib.buffer_address(d) for d in datas]
    ptrs = (ctypes.c_void_p * n)(*[k[0] for k in keep])
    sizes = (ctypes.c_size_t * n)(*[k[1] for k in keep])
    status = (ctypes.c_int32 * n)()
    err = ctypes.create_string_buffer(1024)
    spec = out.to_c()
    rc = _lib.lib().spdl_hj_decode_batch(dec._h, ptrs, sizes, n, ctypes.byref(spec), ptr, nbytes,
                                         None, 1, status, err, 1024)
    return rc, err.value.decode(), list(status)


@pytest.mark.parametrize("what", ["crops", "views", "jfif", "level 4", "count"])
def test_refused_with_invalid_arg_and_nothing_written(decoder, oracle, what):
    datas = [lc.sized("420", 64, 48)] * 2
    out = Output(pix_fmt="rgb24", resize=True, fit_w=16, fit_h=16)
    nbytes = 2 * 16 * 16 * 3
    t = torch.full((nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    ptr = t.data_ptr()
    levels = [1, 0]
    if what == "crops":
        decoder.set_crops([(0, 0, 32, 32), None])
    elif what == "views":
        decoder.set_views([ViewGroup(out, [(0, None), (1, None)], ptr, nbytes)])
        ptr = nbytes = 0
    elif what == "jfif":
        out = Output(pix_fmt="rgb24", csc="jfif")
        t = torch.full((2 * 64 * 48 * 3 + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
        ptr, nbytes = t.data_ptr(), 2 * 64 * 48 * 3
    elif what == "level 4":
        levels = [0, 4]
    else:
        levels = [1, 1, 1]
    decoder.set_lowres(levels)
    rc, msg, _ = _raw(decoder, datas, out, ptr, nbytes)
    assert rc == INVALID_ARG and ("lowres" in msg or "reduced-size" in msg), (rc, msg)
    torch.cuda.synchronize()
    assert bool((t == GUARD).all()), "a refused submission wrote output"
    # the failed call consumed the levels: the next one is a plain submission
    out = Output(pix_fmt="rgb24", resize=True, fit_w=16, fit_h=16)
    st, got = _decode(decoder, datas, out, (16, 16, 3))
    assert st == [0, 0] and decoder.get_param("lowres_images") == 0
    np.testing.assert_array_equal(got[0], oracle.decode_resize(datas[0], oracle.Resize(fit_w=16, fit_h=16)),
                                  strict=True)


def test_cmyk_with_a_level_fails_alone(decoder, oracle):
    datas = [lc.sized("420", 64, 48), cases.case("cmyk_pillow"), lc.sized("gray", 50, 37)]
    spec = dict(fit_w=16, fit_h=16)
    out = Output(pix_fmt="rgb24", resize=True, **spec)
    st, got = _decode(decoder, datas, out, (16, 16, 3), lowres=[1, 1, 2], check=False)
    assert st == [0, UNSUPPORTED, 0]
    rs = oracle.Resize(**spec)
    np.testing.assert_array_equal(got[0], ref.rgb(datas[0], 1, rs), strict=True)
    np.testing.assert_array_equal(got[2], ref.rgb(datas[2], 2, rs), strict=True)
    assert (got[1] == GUARD).all(), "the refused image's bytes were written"
    # at level 0 the same file decodes among reduced neighbours
    st, got = _decode(decoder, datas, out, (16, 16, 3), lowres=[1, 0, 2])
    assert st == [0, 0, 0]
    np.testing.assert_array_equal(got[1], oracle.decode_resize(datas[1], rs), strict=True)
