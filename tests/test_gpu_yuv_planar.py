"""GPU tests of the planar output (``pix_fmt="yuv"``, SPDL_HJ_FMT_YUV; -m gpu):
the scale / pad / crop chain on the decoder's own frame format, through the
C-ABI and through ``load_image`` / ``load_image_batch(pix_fmt=None)``.

Every comparison is bit-exact against the numpy restatement
``tests/yuv_scale_ref.py`` (filters from ``oracle.sws_axis``, planes from
``oracle.decode_planes``).
"""

import io

import numpy as np
import pytest
import torch
from PIL import Image

import spdl_amd.io as sio
from spdl_amd import _lib
from spdl_amd._lib import Output
from spdl_amd.synthetic import synthetic_pixels
from tests import cases, jpeg_writer_cases
from tests import yuv_scale_ref as ref

pytestmark = pytest.mark.gpu

FILTERS = ["bicubic", "bilinear", "lanczos"]
UNSUPPORTED, BAD_GEOMETRY = 2, 7
GUARD = 0xA5


def _per_image(data, ow, oh):
    hs, vs, gray = ref.frame_format(data)
    return ow * oh + (0 if gray else 2 * (-(-ow // hs)) * (-(-oh // vs)))


def _decode(dec, datas, per, check=True, **spec):
    """(statuses, [n, per] bytes) of one decode_batch into a 0xA5-filled
    buffer with one image's worth of guard behind it, which must stay."""
    n = len(datas)
    t = torch.full(((n + 1) * per,), GUARD, dtype=torch.uint8, device="cuda:0")
    out = Output(pix_fmt="yuv", **spec)
    st = dec.decode_batch(datas, out, t.data_ptr(), n * per, check=check)
    a = t.cpu().numpy()
    assert (a[n * per:] == GUARD).all(), "wrote past the batch's output"
    return st, a[: n * per].reshape(n, per)


def _check(dec, oracle, data, rs, scaled=None, **extra):
    """One image through the chain `rs`, against the reference."""
    want = ref.scale_packed(data, rs, scaled=scaled)
    spec = dict(resize=True, fit_w=rs.fit_w, fit_h=rs.fit_h, aspect=rs.aspect, pad_w=rs.pad_w,
                pad_h=rs.pad_h, crop_w=rs.crop_w, crop_h=rs.crop_h, filter=rs.filter)
    spec.update(extra)
    st, got = _decode(dec, [data], want.size, **spec)
    assert st == [0]
    np.testing.assert_array_equal(got[0], want, strict=True)


# ---- formats x filters ---------------------------------------------------------

@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("name", ["q90_444", "q90_422", "noise_420", "gray", "prog_420",
                                  "multiscan_420"])
def test_formats_and_filters(decoder, oracle, name, filt):
    d = cases.case(name)
    info = oracle.parse(d)
    R = oracle.Resize
    for rs in (
        R(fit_w=112, fit_h=96, filter=filt),                                       # stretch
        R(fit_w=112, fit_h=112, aspect="decrease", pad_w=112, pad_h=112, filter=filt),
        R(fit_w=96, fit_h=96, aspect="increase", crop_w=96, crop_h=96, filter=filt),
        R(fit_w=160, fit_h=0, filter=filt),                                        # width only
    ):
        _check(decoder, oracle, d, rs)
    # scale to the source size: the decoder's planes
    planes = ref.packed(oracle.decode_planes(d))
    st, got = _decode(decoder, [d], planes.size, resize=True, fit_w=info.width,
                      fit_h=info.height, filter=filt)
    assert st == [0]
    np.testing.assert_array_equal(got[0], planes, strict=True)


@pytest.mark.parametrize("filt", FILTERS)
def test_upscale_tiny(decoder, oracle, filt):
    _check(decoder, oracle, cases.case("tiny_8x8"), oracle.Resize(fit_w=40, fit_h=24, filter=filt))


@pytest.mark.parametrize("idct", ["simple", "islow"])
def test_both_idcts(decoder, oracle, idct):
    d = cases.case("noise_420")
    rs = oracle.Resize(fit_w=112, fit_h=96)
    want = ref.scale_packed(d, rs, idct=oracle.IDCT_ISLOW if idct == "islow" else oracle.IDCT_SIMPLE)
    st, got = _decode(decoder, [d], want.size, resize=True, fit_w=112, fit_h=96, idct=idct)
    assert st == [0]
    np.testing.assert_array_equal(got[0], want, strict=True)


# ---- odd geometry ---------------------------------------------------------------

@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("name", ["odd_444_101x67", "gray_odd"])
def test_odd_sizes_and_odd_pad_box(decoder, oracle, name, filt):
    d = cases.case(name)
    _check(decoder, oracle, d, oracle.Resize(fit_w=51, fit_h=37, filter=filt))
    _check(decoder, oracle, d, oracle.Resize(fit_w=51, fit_h=37, pad_w=55, pad_h=41, filter=filt))
    _check(decoder, oracle, d, oracle.Resize(fit_w=51, fit_h=37, crop_w=33, crop_h=21, filter=filt))


@pytest.mark.parametrize("filt", FILTERS)
def test_odd_source_chroma(decoder, oracle, filt):
    """333x227 4:2:0: the source chroma planes are 167x114 (ceil)."""
    d = cases.case("odd_227x333")
    assert [p.shape for p in oracle.decode_planes(d)] == [(227, 333), (114, 167), (114, 167)]
    _check(decoder, oracle, d, oracle.Resize(fit_w=112, fit_h=76, filter=filt))
    # an odd destination with no pad: chroma 56x38 = ceil(111 / 2) x ceil(75 / 2)
    _check(decoder, oracle, d, oracle.Resize(fit_w=111, fit_h=75, filter=filt))
    assert _per_image(d, 111, 75) == 111 * 75 + 2 * 56 * 38


def test_offsets_round_down_to_the_chroma_grid(decoder, oracle):
    R = oracle.Resize
    d420, d422 = cases.case("noise_420"), cases.case("q90_422")
    # crop: centred offsets (118 - 96) / 2 = 11 -> 10 and (90 - 64) / 2 = 13 -> 12
    _check(decoder, oracle, d420, R(fit_w=118, fit_h=90, crop_w=96, crop_h=64))
    y = ref.scale_planes(d420, R(fit_w=118, fit_h=90, crop_w=96, crop_h=64))[0]
    full = ref.scale_planes(d420, R(fit_w=118, fit_h=90))[0]
    np.testing.assert_array_equal(y, full[12:76, 10:106])
    # pad: (112 - 102) / 2 = 5 -> 4 and (112 - 90) / 2 = 11 -> 10
    _check(decoder, oracle, d420, R(fit_w=102, fit_h=90, pad_w=112, pad_h=112))
    y = ref.scale_planes(d420, R(fit_w=102, fit_h=90, pad_w=112, pad_h=112))[0]
    assert (y[:10] == 0).all() and (y[:, :4] == 0).all() and y[10, 4:106].any()
    # 4:2:2: x rounds (5 -> 4), y does not ((112 - 91) / 2 = 10, an odd height is fine)
    _check(decoder, oracle, d422, R(fit_w=102, fit_h=91, pad_w=112, pad_h=112))
    _check(decoder, oracle, d422, R(fit_w=118, fit_h=91, crop_w=96, crop_h=65))


# ---- refusals, per image --------------------------------------------------------

def _enc420(seed, h, w):
    b = io.BytesIO()
    Image.fromarray(synthetic_pixels(seed, h, w), "RGB").save(b, "JPEG", quality=90, subsampling=2)
    return b.getvalue()


def test_odd_scaled_content_with_pad_is_refused(decoder, oracle):
    """decrease into 112x112: 320x240 -> 112x84, 300x200 -> 112x75.  An odd
    4:2:0 height under a pad is refused for that image alone."""
    good, odd = cases.case("noise_420"), _enc420(41, 200, 300)
    rs = oracle.Resize(fit_w=112, fit_h=112, aspect="decrease", pad_w=112, pad_h=112)
    assert oracle.geometry(300, 200, rs)["sh"] == 75
    want = ref.scale_packed(good, rs)
    st, got = _decode(decoder, [good, odd, good], want.size, check=False, resize=True, fit_w=112,
                      fit_h=112, aspect="decrease", pad_w=112, pad_h=112)
    assert st == [0, BAD_GEOMETRY, 0]
    np.testing.assert_array_equal(got[0], want, strict=True)
    np.testing.assert_array_equal(got[2], want, strict=True)
    assert (got[1] == GUARD).all()  # a refused image's slot is left alone
    with pytest.raises(RuntimeError, match="Failed to decode"):
        _decode(decoder, [good, odd], want.size, resize=True, fit_w=112, fit_h=112,
                aspect="decrease", pad_w=112, pad_h=112)


@pytest.mark.parametrize("kw", [dict(pad_w=111, pad_h=112), dict(pad_w=112, pad_h=111),
                                dict(crop_w=95, crop_h=80), dict(crop_w=96, crop_h=79)])
def test_sizes_off_the_chroma_grid_are_refused(decoder, kw):
    d = cases.case("noise_420")
    ow = kw.get("pad_w") or kw["crop_w"]
    oh = kw.get("pad_h") or kw["crop_h"]
    st, _ = _decode(decoder, [d], _per_image(d, ow, oh), check=False, resize=True, fit_w=100,
                    fit_h=90, **kw)
    assert st == [BAD_GEOMETRY]
    # (gray and 4:4:4 have ratio 1: the same chain is fine there)
    g = cases.case("gray")
    st, _ = _decode(decoder, [g], _per_image(g, ow, oh), resize=True, fit_w=100, fit_h=90, **kw)
    assert st == [0]


def test_unsupported_frames_are_refused_alone(decoder, oracle):
    """RGB-coded, 4-component, 4:4:0 and a 4:4:4 image in a 4:2:0 batch."""
    a, b = cases.case("noise_420"), cases.case("q90_420")
    s440 = jpeg_writer_cases.case("samp_440_37x29_ri0").data
    datas = [a, cases.case("rgb_coded"), cases.case("cmyk_adobe"), s440, cases.case("q90_444"), b]
    rs = oracle.Resize(fit_w=112, fit_h=96)
    wa, wb = ref.scale_packed(a, rs), ref.scale_packed(b, rs)
    st, got = _decode(decoder, datas, wa.size, check=False, resize=True, fit_w=112, fit_h=96)
    assert st == [0, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, 0]
    np.testing.assert_array_equal(got[0], wa, strict=True)
    np.testing.assert_array_equal(got[5], wb, strict=True)
    assert (got[1:5] == GUARD).all()
    # image 0 decides the layout: an unsupported one fails the call
    for first in (datas[1], datas[2], s440):
        with pytest.raises(RuntimeError, match="Failed to decode"):
            _decode(decoder, [first, a], wa.size, resize=True, fit_w=112, fit_h=96)


@pytest.mark.parametrize("bad", [dict(normalize=True), dict(csc="jfif")])
def test_invalid_specs_are_refused_up_front(decoder, bad):
    d = cases.case("q90_444")
    with pytest.raises(RuntimeError, match="invalid argument"):
        _decode(decoder, [d], _per_image(d, 320, 240) * 2, **bad)


# ---- long filters ------------------------------------------------------------------

@pytest.mark.parametrize("size", [(96, 54), (480, 270)])
def test_large_downscale(decoder, oracle, size):
    """1920x1080 -> 96x54: more than 64 horizontal taps, through the
    horizontal pre-pass; -> 480x270: the pre-pass with short filters."""
    d = cases.case("large_1080p")
    rs = oracle.Resize(fit_w=size[0], fit_h=size[1])
    if size == (96, 54):
        assert oracle.sws_axis(1920, 96, "bicubic")[1].shape[1] > 64
    _check(decoder, oracle, d, rs)


@pytest.mark.parametrize("prepass", [0, 1])
def test_prepass_choice_changes_nothing(oracle, prepass):
    dec = _lib.Decoder(0)
    dec.set_param("sws_prepass", prepass)
    _check(dec, oracle, cases.case("noise_420"), oracle.Resize(fit_w=112, fit_h=96))
    _check(dec, oracle, cases.case("large_1080p"), oracle.Resize(fit_w=96, fit_h=54))
    dec.close()


def test_wide_output_in_column_chunks(decoder, oracle):
    """An output wider than a workgroup's column chunk, of a width that is no
    multiple of 16: rows of a chunked tile start at every alignment."""
    d = cases.case("q90_420")
    _check(decoder, oracle, d, oracle.Resize(fit_w=598, fit_h=50, filter="bilinear"))
    dec = _lib.Decoder(0)
    dec.set_param("sws_cols", 16)
    _check(dec, oracle, cases.case("noise_420"), oracle.Resize(fit_w=102, fit_h=90, pad_w=112, pad_h=112))
    _check(dec, oracle, cases.case("gray_odd"), oracle.Resize(fit_w=51, fit_h=37, pad_w=55, pad_h=41))
    dec.close()


# ---- batches ------------------------------------------------------------------------

PAD112 = dict(fit_w=112, fit_h=112, aspect="decrease", pad_w=112, pad_h=112)
BATCH = ["bench_0", "noise_420", "odd_227x333", "bench_1", "prog_420", "q90_420", "multiscan_420",
         "bench_2", "odd_227x333", "q75_420", "bench_3", "noise_420", "q95_420", "bench_4",
         "prog_420", "bench_5"]


@pytest.fixture(scope="module")
def batch(oracle):
    datas = [cases.case(n) for n in BATCH]
    assert {(oracle.parse(d).width, oracle.parse(d).height) for d in datas} == \
        {(640, 480), (320, 240), (333, 227)}
    assert all(ref.frame_format(d) == (2, 2, False) for d in datas)
    rs = oracle.Resize(**PAD112)
    uniq = {n: ref.scale_packed(cases.case(n), rs) for n in set(BATCH)}
    return datas, [uniq[n] for n in BATCH]


def test_mixed_size_batch(decoder, batch):
    datas, want = batch
    st, got = _decode(decoder, datas, want[0].size, resize=True, **PAD112)
    assert not any(st) and want[0].size == 112 * 112 * 3 // 2
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w, strict=True)


@pytest.mark.parametrize("lanes", [1, 4])
def test_mixed_size_batch_device(batch, lanes):
    datas, want = batch
    offs, sizes, total = [], [], 0
    for d in datas:
        offs.append(total)
        sizes.append(len(d))
        total += (len(d) + 64 + 255) // 256 * 256
    host = np.zeros(total, np.uint8)
    for o, d in zip(offs, datas):
        host[o:o + len(d)] = np.frombuffer(d, np.uint8)
    dev = torch.from_numpy(host).to("cuda:0")
    infos = (_lib.ImageInfo * len(datas))(*[_lib.get_image_info(d) for d in datas])
    dec = _lib.Decoder(0)
    dec.set_param("lanes", lanes)
    n, per = len(datas), want[0].size
    outs = [torch.full(((n + 1) * per,), GUARD, dtype=torch.uint8, device="cuda:0")
            for _ in range(3)]
    spec = Output(pix_fmt="yuv", resize=True, **PAD112)
    tickets = []
    for o in outs:
        dec.decode_batch_device(dev.data_ptr(), dev.numel(), offs, sizes, infos, spec,
                                o.data_ptr(), n * per, stream=torch.cuda.current_stream(),
                                sync=False)
        tickets.append(dec.last_ticket())
    for t in tickets:
        assert not any(dec.wait(t, n))
    torch.cuda.synchronize()
    for o in outs:
        a = o.cpu().numpy()
        assert (a[n * per:] == GUARD).all()
        for g, w in zip(a[: n * per].reshape(n, per), want):
            np.testing.assert_array_equal(g, w, strict=True)
    dec.close()


def test_output_buffer_too_small(decoder):
    d = cases.case("noise_420")
    per = 112 * 96 * 3 // 2
    t = torch.empty(per, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(RuntimeError, match="output buffer too small"):
        decoder.decode_batch([d], Output(pix_fmt="yuv", resize=True, fit_w=112, fit_h=96),
                             t.data_ptr(), per - 1)


# ---- resize == 0 --------------------------------------------------------------------

@pytest.mark.parametrize("name", ["q90_420", "gray_odd", "odd_227x333", "q90_422"])
def test_full_resolution_equals_decode_planes(decoder, oracle, name):
    d = cases.case(name)
    planes = decoder.decode_planes(d)
    want = ref.packed(planes)
    np.testing.assert_array_equal(want, ref.packed(oracle.decode_planes(d)))
    st, got = _decode(decoder, [d, d], want.size)
    assert st == [0, 0]
    np.testing.assert_array_equal(got[0], want, strict=True)
    np.testing.assert_array_equal(got[1], want, strict=True)


# ---- the io surface -----------------------------------------------------------------

@pytest.mark.parametrize("names,shape", [
    (["q90_420", "noise_420"], (1, 168, 112)),
    (["q90_422", "prog_422"], (1, 224, 112)),
    (["q90_444", "odd_444_101x67"], (3, 112, 112)),
    (["gray", "gray_odd"], (112, 112, 1)),
])
@pytest.mark.parametrize("on_device", [False, True])
def test_load_image_batch_without_a_format(oracle, names, shape, on_device):
    datas = [cases.case(n) for n in names]
    cfg = sio.cuda_config(device_index=0) if on_device else None
    buf = sio.load_image_batch(datas, width=112, height=112, pix_fmt=None, device_config=cfg)
    hyp = sio.to_torch(buf).cpu().numpy() if on_device else sio.to_numpy(buf)
    assert hyp.shape == (len(datas), *shape) and hyp.dtype == np.uint8
    rs = oracle.Resize(**PAD112)
    for h, d in zip(hyp, datas):
        np.testing.assert_array_equal(h.reshape(-1), ref.scale_packed(d, rs), strict=True)
    # image 0 is 4:3 landscape in every pair: 112x84 (gray 300x200: 112x75)
    # under 14 (18) rows of pad: 0 / 128 / 128, gray 16
    flat = hyp[0].reshape(-1)
    if shape == (112, 112, 1):
        assert (flat[: 18 * 112] == 16).all() and flat[18 * 112: 19 * 112].any()
    else:
        hs, vs, _ = ref.frame_format(datas[0])
        cw, ch = 112 // hs, 112 // vs
        y = flat[: 112 * 112].reshape(112, 112)
        u = flat[112 * 112: 112 * 112 + cw * ch].reshape(ch, cw)
        v = flat[112 * 112 + cw * ch:].reshape(ch, cw)
        assert (y[:14] == 0).all() and (y[98:] == 0).all() and y[14].any()
        assert (u[: 14 // vs] == 128).all() and (v[98 // vs:] == 128).all()
        assert (u[14 // vs] != 128).any()


def test_load_image_batch_mixed_formats_raise():
    datas = [cases.case("q90_420"), cases.case("q90_444")]
    with pytest.raises(RuntimeError, match="must have the same size and pixel format"):
        sio.load_image_batch(datas, width=112, height=112, pix_fmt=None)
    for name in ("rgb_coded", "cmyk_adobe"):
        with pytest.raises(RuntimeError, match="Unsupported pixel format"):
            sio.load_image_batch([cases.case(name)], width=112, height=112, pix_fmt=None)
    with pytest.raises(RuntimeError, match="Unsupported pixel format"):
        sio.load_image_batch([jpeg_writer_cases.case("samp_440_37x29_ri0").data], width=112,
                             height=112, pix_fmt=None)
    with pytest.raises(ValueError, match="normalize"):
        sio.load_image_batch(datas[:1], width=112, height=112, pix_fmt=None, normalize=True)


def test_load_image_batch_odd_subsampled_size_fails_the_copy():
    d = cases.case("q90_420")
    with pytest.raises(RuntimeError, match="Failed to copy image data"):
        sio.load_image_batch([d], width=None, height=None, pix_fmt=None,
                             filter_desc="scale=w=111:h=96")
    with pytest.raises(RuntimeError, match="Failed to copy image data"):
        sio.load_image(d, pix_fmt=None, filter_desc="scale=w=112:h=95")
    # 4:2:2 subsamples the width only
    buf = sio.load_image(cases.case("q90_422"), pix_fmt=None, filter_desc="scale=w=112:h=95")
    assert sio.to_numpy(buf).shape == (1, 190, 112)


def test_load_image_batch_not_strict_keeps_the_survivors(oracle):
    good = [cases.case("q90_420"), cases.case("noise_420")]
    srcs = [good[0], b"not a jpeg", cases.truncated(), good[1]]
    with pytest.raises(RuntimeError):
        sio.load_image_batch(srcs, width=112, height=112, pix_fmt=None)
    hyp = sio.to_numpy(sio.load_image_batch(srcs, width=112, height=112, pix_fmt=None,
                                            strict=False))
    assert hyp.shape == (2, 1, 168, 112)
    rs = oracle.Resize(**PAD112)
    for h, d in zip(hyp, good):
        np.testing.assert_array_equal(h.reshape(-1), ref.scale_packed(d, rs), strict=True)


def test_load_image_negative_scale_size(oracle):
    """scale=w=112:h=-2 on 320x240: h = rescale(112 * 240, 320 * 2) * 2 = 84."""
    d = cases.case("noise_420")
    hyp = sio.to_numpy(sio.load_image(d, pix_fmt=None,
                                      filter_desc="scale=w=112:h=-2:flags=bicubic"))
    assert hyp.shape == (1, 84 + 42, 112)
    want = ref.scale_packed(d, oracle.Resize(fit_w=112, fit_h=84), scaled=(112, 84))
    np.testing.assert_array_equal(hyp.reshape(-1), want, strict=True)
    # 333x227, h=-2: rescale(112 * 227, 333 * 2) = 38 (38.17) -> 76
    d = cases.case("odd_227x333")
    hyp = sio.to_numpy(sio.load_image(d, pix_fmt=None,
                                      filter_desc="scale=w=112:h=-2:flags=lanczos"))
    assert hyp.shape == (1, 76 + 38, 112)
    want = ref.scale_packed(d, oracle.Resize(fit_w=112, fit_h=76, filter="lanczos"))
    np.testing.assert_array_equal(hyp.reshape(-1), want, strict=True)
    # the same rule ahead of an RGB format node
    rgb = sio.to_numpy(sio.load_image(
        d, filter_desc="scale=w=112:h=-2:flags=bicubic,format=pix_fmts=rgb24"))
    np.testing.assert_array_equal(
        rgb, oracle.decode_resize(d, oracle.Resize(fit_w=112, fit_h=76), "rgb24"), strict=True)


def test_load_image_without_a_format_or_chain(oracle):
    """pix_fmt=None and the default (empty) chain: the decoder's planes."""
    d = cases.case("q90_422")
    hyp = sio.to_numpy(sio.load_image(d, pix_fmt=None))
    np.testing.assert_array_equal(hyp, sio.to_numpy(sio.load_image(d, filter_desc=None)),
                                  strict=True)
