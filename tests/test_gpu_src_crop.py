"""GPU tests of the source crop (spdl_hj_set_crops; -m gpu): per-image regions of
the decoder's frame, scaled / converted as frames of their own, with the IDCT
run over the region's MCUs only.  Through the C-ABI (``Decoder``) and the
Python surface; every comparison is bit-exact against ``tests/src_crop_ref.py``.
"""

import ctypes

import numpy as np
import pytest
import torch

import spdl_amd.io as sio
from spdl_amd import _lib
from spdl_amd._lib import Output
from tests import cases, jpeg_writer_cases
from tests import src_crop_ref as ref

pytestmark = pytest.mark.gpu

BAD_GEOMETRY, INVALID_ARG = 7, 8
GUARD = 0xA5
CHAIN = dict(resize=True, fit_w=64, fit_h=64, aspect="decrease", pad_w=64, pad_h=64)
IDCT_THREADS = 256  # blocks per idct_kernel workgroup


def _rs(oracle, filt="bicubic", **over):
    kw = {k: v for k, v in CHAIN.items() if k != "resize"}
    kw.update(over)
    return oracle.Resize(filter=filt, **kw)


def _decode(dec, datas, crops, out, shape, check=True):
    """(statuses, [n, *shape]) of one decode_batch into a guarded buffer."""
    n, per = len(datas), int(np.prod(shape))
    t = torch.full(((n + 1) * per,), GUARD, dtype=out.torch_dtype, device="cuda:0")
    esz = t.element_size()
    st = dec.decode_batch(datas, out, t.data_ptr(), n * per * esz, check=check, crops=crops)

    def host(x):
        x = x.cpu()
        return x.view(torch.int16).numpy().view(np.uint16) if esz == 2 else x.numpy()

    a = host(t)
    assert (a[n * per:] == host(torch.full((1,), GUARD, dtype=out.torch_dtype))[0]).all(), \
        "wrote past the batch's output"
    return st, a[: n * per].reshape(n, *shape)


def _check_rgb(dec, oracle, data, rect, pix_fmt="rgb24", filt="bicubic", rs="chain", **spec):
    """One region through a chain (default: fit 64x64, decrease, pad 64x64;
    rs=None: full resolution) against the reference."""
    r = ref.resolve_data(data, rect)
    rs = _rs(oracle, filt) if rs == "chain" else rs
    want = ref.rgb(data, r, rs, pix_fmt)
    kw = dict(CHAIN, filter=filt) if rs is not None and not spec else spec
    st, got = _decode(dec, [data], [rect], Output(pix_fmt=pix_fmt, **kw), want.shape)
    assert st == [0]
    np.testing.assert_array_equal(got[0], want, strict=True)


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


# ---- origins, formats, filters ---------------------------------------------------

@pytest.mark.parametrize("rect", [(17, 9, 6, 4), (1, 0, 33, 21), (2, 3, 50, 40), (3, 5, 64, 48)])
def test_444_origins_of_any_alignment(decoder, oracle, rect):
    """Origin = 1, 2, 3 mod 4 and a region inside one block."""
    d = cases.case("q90_444")
    for pix_fmt in ("rgb24", "rgb"):
        _check_rgb(decoder, oracle, d, rect, pix_fmt)
    _check_rgb(decoder, oracle, d, rect, "rgb24", "bilinear")
    _check_rgb(decoder, oracle, d, rect, "rgb", "lanczos")


def _idct_wgs(dec):
    return dec.get_param("idct_workgroups")


def test_gray_region_runs_two_idct_workgroups(decoder, oracle):
    d = cases.case("gray")
    assert oracle.parse(d).nblocks == 950
    for pix_fmt in ("rgb24", "rgb"):
        _check_rgb(decoder, oracle, d, (17, 9, 136, 128), pix_fmt)
        assert _idct_wgs(decoder) == 2  # blocks 2..19 x 1..17: 306
    _check_rgb(decoder, oracle, d, (0, 0, 0, 0))
    assert _idct_wgs(decoder) == 4


def test_420_region_runs_two_idct_workgroups(decoder, oracle):
    """The region's 8 x 8 MCUs (384 blocks) take two IDCT workgroups; the
    whole 640x480 frame (7200 blocks) one per 256 blocks, 29."""
    d = cases.case("q90_420")
    nblocks = oracle.parse(d).nblocks
    for pix_fmt in ("rgb24", "rgb"):
        _check_rgb(decoder, oracle, d, (38, 22, 112, 112), pix_fmt)
        assert _idct_wgs(decoder) == 2  # MCUs 2..9 x 1..8, 6 blocks each: 384
    _check_rgb(decoder, oracle, d, (38, 22, 112, 112), "rgb24", "lanczos")
    _check_rgb(decoder, oracle, d, (0, 0, 0, 0))
    assert _idct_wgs(decoder) == -(-nblocks // IDCT_THREADS) > 2


@pytest.mark.parametrize("name,rect", [
    ("odd_227x333", (301, 195, 32, 32)),  # -> (300, 194): the right and bottom partial MCUs
    ("q90_422", (11, 13, 51, 37)),        # 4:2:2 rounding: (10, 13, 50, 37)
    ("samp_440_37x29_ri0", (5, 3, 22, 17)),
    ("samp_411_70x29_ri0", (9, 3, 41, 20)),   # -> x 8, w 40: chroma origin 2
    ("samp_410_70x29_ri0", (13, 5, 45, 19)),  # -> (12, 4, 44, 18): chroma origin 3
    ("restart_blocks", (101, 57, 120, 90)),
    ("prog_420", (33, 41, 150, 101)),
    ("multiscan_422_rst", (21, 10, 99, 77)),
    ("cmyk_adobe", (13, 7, 90, 71)),
    ("rgb_coded", (7, 9, 101, 63)),
])
def test_samplings_and_scan_structures(decoder, oracle, name, rect):
    d = jpeg_writer_cases.case(name).data if name.startswith("samp_") else cases.case(name)
    for pix_fmt in ("rgb24", "rgb"):
        _check_rgb(decoder, oracle, d, rect, pix_fmt)
    _check_rgb(decoder, oracle, d, rect, "rgb24", "bilinear")


def test_rounded_rectangles_are_what_the_header_says(oracle):
    assert ref.resolve_data(cases.case("odd_227x333"), (301, 195, 32, 32)) == (300, 194, 32, 32)
    assert ref.resolve_data(cases.case("q90_422"), (11, 13, 51, 37)) == (10, 13, 50, 37)
    assert ref.resolve_data(jpeg_writer_cases.case("samp_410_70x29_ri0").data, (13, 5, 45, 19)) == \
        (12, 4, 44, 18)


# ---- the horizontal pre-pass and the multi-piece entropy decode ------------------

def test_large_downscale_takes_the_prepass(decoder, oracle):
    d = cases.case("large_1080p")
    rect, spec = (100, 60, 1600, 900), dict(resize=True, fit_w=96, fit_h=54)
    plan = _lib.debug_sws_plan(1600, 900, 1, 1, "yuv", Output(pix_fmt="rgb24", **spec))
    assert plan["rc"] == 0 and plan["pre"] == 1  # the region's plan runs hscale_kernel
    _check_rgb(decoder, oracle, d, rect, "rgb24", rs=oracle.Resize(fit_w=96, fit_h=54), **spec)


def test_prepass_forced_on_a_small_region(decoder, oracle, knobs):
    knobs("sws_prepass", 1)
    for pix_fmt in ("rgb24", "rgb"):
        _check_rgb(decoder, oracle, cases.case("q90_420"), (38, 22, 112, 112), pix_fmt)
    _check_rgb(decoder, oracle, cases.case("q90_444"), (3, 5, 64, 48), "rgb24", "lanczos")


def test_multi_piece_entropy_with_a_region(decoder, oracle, knobs):
    knobs("entropy_piece_bytes", 16384)
    d = cases.case("large_1080p")
    assert len(d) > 4 * 16384
    _check_rgb(decoder, oracle, d, (100, 60, 1600, 900), "rgb24",
               rs=oracle.Resize(fit_w=96, fit_h=54), resize=True, fit_w=96, fit_h=54)


def test_handoff_redecode_carries_the_rectangle(decoder, oracle, knobs):
    """A piece hand-off that gives up (handoff_wait_us 0) re-decodes the image
    in one workgroup: that one-image batch must crop as the batch did."""
    knobs("entropy_piece_bytes", 16384)
    knobs("handoff_wait_us", 0)
    before = decoder.get_param("handoff_retries")
    _check_rgb(decoder, oracle, cases.case("large_1080p"), (100, 60, 1600, 900), "rgb24",
               rs=oracle.Resize(fit_w=96, fit_h=54), resize=True, fit_w=96, fit_h=54)
    assert decoder.get_param("handoff_retries") > before, "no hand-off gave up"


# ---- full resolution -------------------------------------------------------------

@pytest.mark.parametrize("path", [0, 1, 2])
def test_full_resolution_is_the_region_itself(decoder, oracle, knobs, path):
    knobs("output_path", path)
    for name, rect in (("q90_420", (38, 22, 112, 112)), ("odd_227x333", (301, 195, 32, 32))):
        for pix_fmt in ("rgb24", "rgb"):
            _check_rgb(decoder, oracle, cases.case(name), rect, pix_fmt, rs=None)


def test_full_resolution_regions_must_share_a_size(decoder):
    d = cases.case("q90_420")
    t = torch.zeros(2 * 112 * 112 * 3, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(RuntimeError, match="same output size"):
        decoder.decode_batch([d, d], Output(pix_fmt="rgb24"), t.data_ptr(), t.numel(),
                             crops=[(38, 22, 112, 112), (0, 0, 112, 96)])


def test_jfif_conversion_takes_no_crop(decoder):
    d = cases.case("q90_420")
    t = torch.zeros(112 * 112 * 3, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(RuntimeError, match="swscale"):
        decoder.decode_batch([d], Output(pix_fmt="rgb24", csc="jfif"), t.data_ptr(), t.numel(),
                             crops=[(38, 22, 112, 112)])


# ---- planar output ---------------------------------------------------------------

@pytest.mark.parametrize("name,rect", [("q90_420", (38, 22, 112, 112)),
                                       ("q90_422", (11, 13, 51, 37)),
                                       ("q90_444", (3, 5, 64, 48)), ("gray", (17, 9, 136, 128))])
def test_planar_output_of_a_region(decoder, oracle, name, rect):
    d = cases.case(name)
    r = ref.resolve_data(d, rect)
    for rs, spec in ((_rs(oracle), CHAIN), (None, {})):
        want = ref.planar(d, r, rs)
        st, got = _decode(decoder, [d], [rect], Output(pix_fmt="yuv", **spec), want.shape)
        assert st == [0]
        np.testing.assert_array_equal(got[0], want, strict=True)


# ---- normalised output -----------------------------------------------------------

def test_normalised_fp16_output(decoder, oracle):
    d = cases.case("q90_420")
    rect = (38, 22, 112, 112)
    want = ref.rgb(d, ref.resolve_data(d, rect), _rs(oracle), "rgb", normalize=True)
    st, got = _decode(decoder, [d], [rect], Output(pix_fmt="rgb", normalize=True, **CHAIN),
                      want.shape)
    assert st == [0]
    np.testing.assert_array_equal(got[0], want.view(np.uint16), strict=True)


# ---- a mixed batch, through the three entry points -------------------------------

MIXED = [("q90_420", (38, 22, 112, 112)), ("gray", (17, 9, 136, 128)), ("q90_444", None),
         ("odd_227x333", (301, 195, 32, 32)), ("prog_420", (33, 41, 150, 101)),
         ("q90_422", None), ("cmyk_adobe", (0, 0, 161, 50)),  # wider than the 160 px frame
         ("rgb_coded", (7, 9, 101, 63))]
TOO_LARGE = 6


@pytest.fixture(scope="module")
def mixed(oracle):
    """(datas, crops, expected [8, 64, 64, 3] with image TOO_LARGE left out)."""
    datas = [cases.case(n) for n, _ in MIXED]
    crops = [r for _, r in MIXED]
    rs = _rs(oracle)
    want = []
    for i, (d, r) in enumerate(zip(datas, crops)):
        if i == TOO_LARGE:
            assert ref.resolve_data(d, r) is None
            want.append(None)
        elif r is None:
            want.append(oracle.decode_resize(d, rs, "rgb24"))
        else:
            want.append(ref.rgb(d, ref.resolve_data(d, r), rs, "rgb24"))
    return datas, crops, want


def _check_mixed(st, got, want):
    assert st == [BAD_GEOMETRY if i == TOO_LARGE else 0 for i in range(len(want))]
    for i, w in enumerate(want):
        if w is None:
            assert (got[i] == GUARD).all()  # a refused image leaves its bytes untouched
        else:
            np.testing.assert_array_equal(got[i], w, strict=True, err_msg=f"image {i}")


def test_mixed_batch(decoder, mixed):
    datas, crops, want = mixed
    out = Output(pix_fmt="rgb24", **CHAIN)
    st, got = _decode(decoder, datas, crops, out, (64, 64, 3), check=False)
    _check_mixed(st, got, want)
    # images 2 and 5 have no rectangle: today's output, bit for bit
    st0, plain = _decode(decoder, [datas[2], datas[5]], None, out, (64, 64, 3))
    assert st0 == [0, 0]
    np.testing.assert_array_equal(got[2], plain[0], strict=True)
    np.testing.assert_array_equal(got[5], plain[1], strict=True)
    # without check=False the refused image raises, as any failed image does
    t = torch.zeros(8 * 64 * 64 * 3, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(RuntimeError, match="image 6"):
        decoder.decode_batch(datas, out, t.data_ptr(), t.numel(), crops=crops)


def _packed(datas):
    offs, total = [], 0
    for d in datas:
        offs.append(total)
        total += (len(d) + 64 + 255) // 256 * 256
    host = np.zeros(total + 512, np.uint8)
    for o, d in zip(offs, datas):
        host[o:o + len(d)] = np.frombuffer(d, np.uint8)
    return host, offs, [len(d) for d in datas], total


def test_mixed_batch_device_resident(decoder, mixed):
    datas, crops, want = mixed
    host, offs, sizes, _ = _packed(datas)
    dev = torch.from_numpy(host).to("cuda:0")
    infos = [_lib.get_image_info(d) for d in datas]
    out = Output(pix_fmt="rgb24", **CHAIN)
    t = torch.full((8, 64, 64, 3), GUARD, dtype=torch.uint8, device="cuda:0")
    st = decoder.decode_batch_device(dev.data_ptr(), dev.numel(), offs, sizes, infos, out,
                                     t.data_ptr(), t.numel(), crops=crops, check=False)
    _check_mixed(st, t.cpu().numpy(), want)
    # the rectangles are gone after one submission: the same call, whole frames
    t.fill_(GUARD)
    st = decoder.decode_batch_device(dev.data_ptr(), dev.numel(), offs, sizes, infos, out,
                                     t.data_ptr(), t.numel())
    assert st == [0] * 8
    plain = t.cpu().numpy()
    np.testing.assert_array_equal(plain[2], want[2], strict=True)
    assert not np.array_equal(plain[0], want[0])
    # a rectangle count that differs from the batch's: INVALID_ARG, and consumed
    decoder.set_crops(crops[:3])
    with pytest.raises(RuntimeError, match="3 rectangles for a batch of 8"):
        decoder.decode_batch_device(dev.data_ptr(), dev.numel(), offs, sizes, infos, out,
                                    t.data_ptr(), t.numel())
    st = decoder.decode_batch_device(dev.data_ptr(), dev.numel(), offs, sizes, infos, out,
                                     t.data_ptr(), t.numel())
    assert st == [0] * 8
    np.testing.assert_array_equal(t.cpu().numpy(), plain, strict=True)
    # NULL / 0 clears
    decoder.set_crops(crops)
    decoder.set_crops(None)
    st = decoder.decode_batch_device(dev.data_ptr(), dev.numel(), offs, sizes, infos, out,
                                     t.data_ptr(), t.numel())
    np.testing.assert_array_equal(t.cpu().numpy(), plain, strict=True)


def test_mixed_batch_staged(decoder, mixed):
    datas, crops, want = mixed
    host, offs, sizes, total = _packed(datas)
    out = Output(pix_fmt="rgb24", **CHAIN)
    t = torch.full((8, 64, 64, 3), GUARD, dtype=torch.uint8, device="cuda:0")
    ptr, ticket = decoder.staging_acquire(total)
    ctypes.memmove(ptr, host.ctypes.data, total)
    st = decoder.decode_staged(ticket, total, offs, sizes, out, t.data_ptr(), t.numel(),
                               crops=crops, check=False)
    _check_mixed(st, t.cpu().numpy(), want)
    # decode_planes neither uses nor clears the rectangles
    decoder.set_crops(crops)
    planes = decoder.decode_planes(datas[1])
    assert planes[0].shape == (200, 300)
    t.fill_(GUARD)
    st, got = _decode(decoder, datas, None, out, (64, 64, 3), check=False)
    _check_mixed(st, got, want)


# ---- the Python surface ----------------------------------------------------------

def test_load_image_batch_crops(oracle):
    names = ["q90_420", "gray", "q90_444"]
    datas = [cases.case(n) for n in names]
    crops = [(38, 22, 112, 112), None, (3, 5, 64, 48)]
    cfg = sio.cuda_config(device_index=0)
    got = sio.to_torch(sio.load_image_batch(datas, width=64, height=64, crops=crops,
                                            device_config=cfg)).cpu().numpy()
    rs = _rs(oracle)
    for i, (d, r) in enumerate(zip(datas, crops)):
        want = oracle.decode_resize(d, rs, "rgb24") if r is None else \
            ref.rgb(d, ref.resolve_data(d, r), rs, "rgb24")
        np.testing.assert_array_equal(got[i], want, strict=True)
    with pytest.raises(ValueError, match="exclusive"):
        sio.load_image_batch(datas, width=None, height=None, crops=crops, device_config=cfg,
                             filter_desc="crop=100:80:33:17,scale=64:64")
    with pytest.raises(ValueError, match="2 crops for 3 images"):
        sio.load_image_batch(datas, width=64, height=64, crops=crops[:2], device_config=cfg)


def test_load_image_filter_desc_with_a_source_crop(oracle):
    d = cases.case("q90_420")
    cfg = sio.cuda_config(device_index=0)
    got = sio.to_torch(sio.load_image(d, filter_desc="crop=100:80:33:17,scale=64:64",
                                      device_config=cfg)).cpu().numpy()
    r = ref.resolve_data(d, (33, 17, 100, 80))
    assert r == (32, 16, 100, 80)
    np.testing.assert_array_equal(got, ref.rgb(d, r, oracle.Resize(fit_w=64, fit_h=64), "rgb24"),
                                  strict=True)
    # the same chain for a batch, and the region itself without a scale node
    got = sio.to_torch(sio.load_image_batch([d, d], width=None, height=None, device_config=cfg,
                                            filter_desc="crop=100:80:33:17,scale=64:64"))
    assert got.shape == (2, 64, 64, 3)
    full = sio.to_torch(sio.load_image(d, filter_desc="crop=100:80:33:17",
                                       device_config=cfg)).cpu().numpy()
    np.testing.assert_array_equal(full, ref.rgb(d, r, None, "rgb24"), strict=True)
