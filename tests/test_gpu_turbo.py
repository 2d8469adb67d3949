"""GPU tests of the Pillow-exact decode (``csc="turbo"``, include/spdl_hipjpeg.h
"Pillow-exact decode"; -m gpu): turbo_rgb_kernel through the C-ABI
(``Decoder``) and the Python surface.  Every comparison is byte-exact against
``tests/turbo_ref.py``, a numpy restatement of the rules over the oracle's
islow planes, and, where this Pillow is linked against libjpeg-turbo, against
Pillow itself.
"""

import ctypes
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image, features

import spdl_amd.io as sio
from spdl_amd import _lib
from spdl_amd._lib import Output, ViewGroup
from tests import cases
from tests import turbo_cases as tc
from tests import turbo_ref as ref

pytestmark = pytest.mark.gpu

UNSUPPORTED, TRUNCATED, INVALID_ARG = 2, 5, 8
GUARD = 0xA5


@functools.lru_cache(maxsize=None)
def _want(name: str) -> np.ndarray:
    """[H, W, 3] of a case, computed once; read-only."""
    a = ref.rgb_u8(tc.case(name))
    a.setflags(write=False)
    return a


def _decode(dec, datas, out, shape, **kw):
    """(statuses, [n, *shape]) of one decode_batch into a guarded buffer
    (16-bit outputs as their bit patterns)."""
    n = len(datas)
    esz = 1 if out.torch_dtype == torch.uint8 else 2
    per = int(np.prod(shape)) * esz
    t = torch.full(((n + 1) * per + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    st = dec.decode_batch(datas, out, t.data_ptr(), n * per, **kw)
    a = t.cpu().numpy()
    assert (a[n * per:] == GUARD).all(), "wrote past the batch's output"
    body = a[: n * per]
    if esz == 2:
        body = body.view(np.uint16)
    return st, body.reshape(n, *shape)


# ---- 1. every case, plain ------------------------------------------------------------------------

@pytest.mark.parametrize("name", tc.NAMES)
def test_case_equals_the_reference_and_pillow(decoder, oracle, name):
    data = tc.case(name)
    want = _want(name)
    st, got = _decode(decoder, [data], Output(pix_fmt="rgb24", csc="turbo"), want.shape)
    assert st == [0]
    h, w = want.shape[:2]
    assert decoder.get_param("turbo_workgroups") == -(-w // tc.TILE_W) * -(-h // tc.TILE_H)
    assert decoder.get_param("idct_workgroups") > 0 and decoder.get_param("fused_workgroups") == 0
    np.testing.assert_array_equal(got[0], want, strict=True)
    if features.check_feature("libjpeg_turbo"):
        pil = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        np.testing.assert_array_equal(got[0], pil, strict=True)


def test_idct_field_is_not_consulted(decoder, oracle):
    data = tc.case("420_33x33")
    for idct in ("simple", "islow"):
        st, got = _decode(decoder, [data], Output(pix_fmt="rgb24", csc="turbo", idct=idct), (33, 33, 3))
        assert st == [0]
        np.testing.assert_array_equal(got[0], _want("420_33x33"), strict=True)


def test_batch_of_one_size(decoder, oracle):
    """Several images in one plain submission: every sampling at 17x15."""
    names = [f"{s}_17x15" for s in (*tc.PILLOW, *tc.LJ9)]
    st, got = _decode(decoder, [tc.case(n) for n in names], Output(pix_fmt="rgb24", csc="turbo"),
                      (15, 17, 3))
    assert st == [0] * len(names)
    for k, n in enumerate(names):
        np.testing.assert_array_equal(got[k], _want(n), strict=True, err_msg=n)


# ---- 2. formats x dtypes -------------------------------------------------------------------------

@pytest.mark.parametrize("norm", [None, "float16", "bfloat16"])
@pytest.mark.parametrize("pix_fmt", ["rgb", "bgr", "rgb24", "bgr24"])
def test_formats_and_dtypes(decoder, oracle, pix_fmt, norm):
    for name in tc.FORMAT_CASES + [f"420_{tc.TILE_W + 1}x{tc.TILE_H + 1}"]:
        kw = dict(normalize=True, norm_dtype=norm) if norm else {}
        want = ref.layout(_want(name), pix_fmt, **kw)
        st, got = _decode(decoder, [tc.case(name)], Output(pix_fmt=pix_fmt, csc="turbo", **kw),
                          want.shape)
        assert st == [0]
        np.testing.assert_array_equal(got[0], want, strict=True, err_msg=name)


# ---- 3. ragged -----------------------------------------------------------------------------------

@pytest.mark.parametrize("pix_fmt,norm,align", [("rgb24", None, 1), ("rgb", None, 1),
                                                ("bgr24", "float16", 2), ("rgb24", None, 256)])
def test_ragged_whole_table(decoder, oracle, pix_fmt, norm, align):
    """The whole table at native sizes in one submission: every box exact and
    every byte outside the boxes untouched (align 1: boxes abut at odd
    addresses)."""
    datas = [tc.case(n) for n in tc.NAMES]
    kw = dict(normalize=True, norm_dtype=norm) if norm else {}
    out = Output(pix_fmt=pix_fmt, csc="turbo", **kw)
    esz = 2 if norm else 1
    infos = [_lib.get_image_info(d) for d in datas]
    offs, sizes, st = _lib.ragged_layout(infos, out, align=align)
    assert st == [0] * len(datas)
    lead = 3 * esz  # (an odd start for the u8 boxes; a multiple of the element size)
    total = offs[-1] + lead + 64
    t = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda:0")
    status = decoder.decode_batch(datas, out, t.data_ptr(), lead + offs[-1],
                                  ragged=[o + lead for o in offs[:-1]])
    assert status == [0] * len(datas)
    tiles = sum(-(-w // tc.TILE_W) * -(-h // tc.TILE_H) for w, h in sizes)
    assert decoder.get_param("turbo_workgroups") == tiles
    a = t.cpu().numpy()
    untouched = np.ones(total, bool)
    for k, name in enumerate(tc.NAMES):
        want = ref.layout(_want(name), pix_fmt, **kw)
        first, nbytes = lead + offs[k], want.size * esz
        got = a[first:first + nbytes]
        got = (got.view(np.uint16) if esz == 2 else got).reshape(want.shape)
        np.testing.assert_array_equal(got, want, strict=True, err_msg=name)
        untouched[first:first + nbytes] = False
    assert (a[untouched] == GUARD).all(), "a byte outside the boxes was written"


def test_load_image_list_native_sizes(decoder, oracle):
    names = ["420_17x15", "422_9x7", "gray", "l14_33x33", "444_1x1", "rgb_coded",
             f"420_{2 * tc.TILE_W + 1}x{2 * tc.TILE_H + 1}"]
    cfg = sio.cuda_config(device_index=0)
    bufs, idx = sio.load_image_list([tc.case(n) for n in names], device_config=cfg, csc="turbo",
                                    align=1)
    assert idx == list(range(len(names)))
    for n, b in zip(names, bufs):
        np.testing.assert_array_equal(sio.to_torch(b).cpu().numpy(), _want(n), strict=True, err_msg=n)


def test_load_image_and_batch(decoder, oracle):
    cfg = sio.cuda_config(device_index=0)
    got = sio.to_torch(sio.load_image(tc.case("422_9x7"), device_config=cfg, csc="turbo"))
    np.testing.assert_array_equal(got.cpu().numpy(), _want("422_9x7"), strict=True)
    names = ["420_33x33", "l42_33x33", "444_33x33"]
    got = sio.to_torch(sio.load_image_batch([tc.case(n) for n in names], width=None, height=None,
                                            pix_fmt="bgr", device_config=cfg, csc="turbo"))
    assert got.shape == (3, 3, 33, 33)
    for k, n in enumerate(names):
        np.testing.assert_array_equal(got[k].cpu().numpy(), ref.layout(_want(n), "bgr"), strict=True)


# ---- 4. failed images ----------------------------------------------------------------------------

def test_failed_image_among_good_ones(decoder, oracle):
    """A truncated file between two good ones of its size: its status, its
    bytes untouched, the others exact."""
    info = _lib.get_image_info(cases.truncated())
    w, h = info.width, info.height
    good = cases._enc(tc.pixels(77, w, h), quality=90, subsampling=2)
    datas = [good, cases.truncated(), good]
    st, got = _decode(decoder, datas, Output(pix_fmt="rgb24", csc="turbo"), (h, w, 3), check=False)
    assert st[0] == 0 and st[2] == 0 and st[1] != 0
    want = ref.rgb_u8(good)
    np.testing.assert_array_equal(got[0], want, strict=True)
    np.testing.assert_array_equal(got[2], want, strict=True)
    assert (got[1] == GUARD).all(), "the failed image's bytes were written"


def test_cmyk_is_unsupported(decoder, oracle):
    st = None
    with pytest.raises(RuntimeError, match="csc=turbo"):
        st, _ = _decode(decoder, [cases.case("cmyk_pillow")], Output(pix_fmt="rgb24", csc="turbo"),
                        (64, 64, 3))
    assert st is None


# ---- 5. refusals ---------------------------------------------------------------------------------

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


@pytest.mark.parametrize("what", ["resize", "yuv", "crops", "views", "flips", "orients", "lowres"])
def test_refused_with_invalid_arg_and_nothing_written(decoder, oracle, what):
    datas = [tc.case("420_33x33")] * 2
    out = Output(pix_fmt="rgb24", csc="turbo")
    nbytes = 2 * 33 * 33 * 3
    t = torch.full((nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    ptr = t.data_ptr()
    if what == "resize":
        out = Output(pix_fmt="rgb24", csc="turbo", resize=True, fit_w=16, fit_h=16)
    elif what == "yuv":
        out = Output(pix_fmt="yuv", csc="turbo")
    elif what == "crops":
        decoder.set_crops([(0, 0, 16, 16), None])
    elif what == "views":
        decoder.set_views([ViewGroup(out, [(0, None), (1, None)], ptr, nbytes)])
        ptr = nbytes = 0
    elif what == "flips":
        decoder.set_flips([0, 1])
    elif what == "orients":
        decoder.set_orients([4, 0])
    else:
        decoder.set_lowres([0, 1])
    rc, msg, _ = _raw(decoder, datas, out, ptr, nbytes)
    assert rc == INVALID_ARG and msg, (rc, msg)
    torch.cuda.synchronize()
    assert bool((t == GUARD).all()), "a refused submission wrote output"
    # the failed call consumed what was set: the next one is a plain submission
    st, got = _decode(decoder, datas, Output(pix_fmt="rgb24", csc="turbo"), (33, 33, 3))
    assert st == [0, 0]
    np.testing.assert_array_equal(got[1], _want("420_33x33"), strict=True)


def test_ragged_jfif_stays_refused(decoder, oracle):
    datas = [tc.case("420_33x33")]
    t = torch.full((33 * 33 * 3,), GUARD, dtype=torch.uint8, device="cuda:0")
    decoder.set_ragged([0])
    rc, msg, _ = _raw(decoder, datas, Output(pix_fmt="rgb24", csc="jfif"), t.data_ptr(), t.numel())
    assert rc == INVALID_ARG and "csc = swscale" in msg
    torch.cuda.synchronize()
    assert bool((t == GUARD).all())


# ---- 6. workspace hygiene ------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["420_17x15", "422_9x7", "l12_15x9", "l42_5x2", "420_3x1"])
def test_no_output_byte_depends_on_stale_planes(decoder, oracle, name):
    """The same decode after a larger all-white and after a larger all-black
    image on the same decoder (the same workspace): identical outputs -- the
    padding behind a plane's true columns and rows is never a neighbour."""
    want = _want(name)
    out = Output(pix_fmt="rgb24", csc="turbo")
    results = []
    for value in (255, 0):
        flood = cases._enc(np.full((96, 128, 3), value, np.uint8), quality=90, subsampling=0)
        st, px = _decode(decoder, [flood], out, (96, 128, 3))
        assert st == [0] and abs(int(px.mean()) - value) <= 1
        st, got = _decode(decoder, [tc.case(name)], out, want.shape)
        assert st == [0]
        results.append(got)
    np.testing.assert_array_equal(results[0], results[1], strict=True)
    np.testing.assert_array_equal(results[0][0], want, strict=True)


def test_other_modes_launch_no_turbo_workgroup(decoder, oracle):
    data = tc.case("420_33x33")
    st, got = _decode(decoder, [data], Output(pix_fmt="rgb24", csc="jfif", idct="islow"), (33, 33, 3))
    assert st == [0] and decoder.get_param("turbo_workgroups") == 0
    np.testing.assert_array_equal(got[0], oracle.decode_rgb(data, oracle.IDCT_ISLOW, "rgb24", "jfif"),
                                  strict=True)
