"""GPU tests of ragged batches (spdl_hj_set_ragged; -m gpu): one submission,
every image its own size at its own offset, the output kernel chosen per
image.  Every image is compared bit for bit with the oracle's decode of that
image alone (``decode_rgb`` at native size, ``decode_resize`` for chains,
``tests/src_crop_ref.py`` for source crops), never with another path of the
library.  Buffers start as 0xA5; every byte between the images and behind
the last must still be 0xA5.
"""

import ctypes

import numpy as np
import pytest
import torch

import spdl_amd.io as sio
from spdl_amd import _lib
from spdl_amd._lib import Output
from spdl_amd.synthetic import synthetic_pixels
from tests import cases
from tests import src_crop_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 0xA5
TAIL = 512
TRUNCATED, UNSUPPORTED, BAD_GEOMETRY, INVALID_ARG = 5, 2, 7, 8

# the fused tile is 256 / bpm MCUs of one MCU row: 42 MCUs (672 px) of 4:2:0, 64 (1024 px) of 4:2:2
FUSED = ["one_tile_420", "two_tiles_420", "two_tiles_422", "q90_420"]
GENERIC = ["odd_227x333", "odd_444_101x67", "gray_odd", "odd_height_420", "tiny_1x1",
           "cmyk_pillow_odd", "rgb_coded_odd_rst", "prog_444_odd"]
# (interleaved: neither kernel's images are contiguous in the batch)
SPLIT = ["odd_227x333", "one_tile_420", "odd_444_101x67", "two_tiles_420", "gray_odd",
         "two_tiles_422", "odd_height_420", "q90_420", "tiny_1x1", "cmyk_pillow_odd",
         "rgb_coded_odd_rst", "prog_444_odd"]
assert sorted(SPLIT) == sorted(FUSED + GENERIC)
# tiles per MCU row x MCU rows: 16x16; 688x48 (43 MCUs, 3 rows); 1040x16 4:2:2 (65 MCUs, 2 rows
# of 8 lines); q90_420 is 640x480 (40 MCUs, 30 rows)
FUSED_TILES = 1 * 1 + 2 * 3 + 2 * 2 + 1 * 30


def _file(name):
    if name == "one_tile_420":
        return cases._enc(synthetic_pixels(61, 16, 16), quality=90, subsampling=2)
    if name == "two_tiles_420":  # 43 MCUs: two tiles per MCU row, three rows
        return cases._enc(synthetic_pixels(62, 48, 688), quality=90, subsampling=2)
    if name == "two_tiles_422":  # 65 MCUs: two tiles per MCU row, two rows
        return cases._enc(synthetic_pixels(63, 16, 1040), quality=90, subsampling=1)
    if name == "two_tiles_420_short":  # ... two rows
        return cases._enc(synthetic_pixels(65, 32, 688), quality=90, subsampling=2)
    if name == "odd_height_420":
        return cases._enc(synthetic_pixels(64, 33, 64), quality=90, subsampling=2)
    return cases.case(name)


_FILES, _WANT = {}, {}


def files(names):
    for n in names:
        if n not in _FILES:
            _FILES[n] = _file(n)
    return [_FILES[n] for n in names]


def want_rgb(oracle, name, pix_fmt="rgb24", idct=0):
    """The oracle's native-size decode of a file, computed once."""
    key = (name, pix_fmt, idct)
    if key not in _WANT:
        _WANT[key] = oracle.decode_rgb(files([name])[0], idct, pix_fmt)
    return _WANT[key]


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


def _shape(out, w, h):
    return (3, h, w) if out.planar else (h, w, 3)


def _layout(datas, out, crops=None, codes=None, align=256, infos=None):
    infos = infos or [_lib.get_image_info(d) for d in datas]
    return _lib.ragged_layout(infos, out, crops, codes, align)


def _split_buffer(a, out, offs, sizes):
    """The images of a ragged buffer (16-bit ones as bit patterns); asserts
    that every byte outside them is still the guard."""
    esz = 1 if out.torch_dtype == torch.uint8 else 2
    covered = np.zeros(a.size, bool)
    imgs = []
    for o, (w, h) in zip(offs, sizes):
        nb = w * h * 3 * esz
        seg = a[o:o + nb]
        covered[o:o + nb] = True
        imgs.append((seg.view(np.uint16) if esz == 2 else seg).reshape(_shape(out, w, h)))
    assert (a[~covered] == GUARD).all(), "wrote between or behind the images"
    return imgs


def _ragged(dec, datas, out, crops=None, orients=None, flips=None, align=256, check=True):
    """(statuses, images, sizes) of one ragged decode_batch into a guarded buffer."""
    n = len(datas)
    offs, sizes, _ = _layout(datas, out, crops, orients if orients is not None else flips, align)
    t = torch.full((offs[n] + TAIL,), GUARD, dtype=torch.uint8, device="cuda:0")
    st = dec.decode_batch(datas, out, t.data_ptr(), offs[n], check=check, crops=crops,
                          orients=orients, flips=flips, ragged=offs[:n])
    return st, _split_buffer(t.cpu().numpy(), out, offs[:n], sizes), sizes


# ---- 1. the native-size split ------------------------------------------------------

@pytest.mark.parametrize("path,idct", [(0, "simple"), (1, "simple"), (2, "simple"), (0, "islow")])
def test_native_size_split(decoder, oracle, knobs, path, idct):
    knobs("output_path", path)
    datas = files(SPLIT)
    st, got, sizes = _ragged(decoder, datas, Output(pix_fmt="rgb24", idct=idct))
    assert st == [0] * len(datas)
    for name, g in zip(SPLIT, got):
        w = want_rgb(oracle, name, "rgb24", 1 if idct == "islow" else 0)
        np.testing.assert_array_equal(g, w, strict=True, err_msg=name)
    fused, generic = decoder.get_param("fused_workgroups"), decoder.get_param("generic_workgroups")
    if path == 0:  # both kernels ran
        assert fused == FUSED_TILES and generic >= len(GENERIC)
    else:
        assert fused == 0 and generic >= len(SPLIT)


@pytest.mark.parametrize("names,launched", [
    # alike: 6 + 6 + 4 + 6 tiles, no empty workgroup for the shorter image
    (["two_tiles_420", "two_tiles_420", "two_tiles_420_short", "two_tiles_420"], 22),
    # unlike: 1 + 30 tiles
    (["one_tile_420", "q90_420"], 31),
])
def test_every_image_eligible_runs_the_fused_kernel_alone(decoder, oracle, names, launched):
    st, got, _ = _ragged(decoder, files(names), Output(pix_fmt="rgb24"), align=1)
    assert st == [0] * len(names)
    for name, g in zip(names, got):
        np.testing.assert_array_equal(g, want_rgb(oracle, name), strict=True, err_msg=name)
    assert decoder.get_param("fused_workgroups") == launched
    assert decoder.get_param("generic_workgroups") == 0
    assert decoder.get_param("idct_workgroups") == 0


# ---- 2. formats, dtypes, alignment -------------------------------------------------

SIX = ["two_tiles_420", "odd_227x333", "gray_odd", "two_tiles_422", "tiny_1x1", "odd_444_101x67"]


@pytest.mark.parametrize("pix_fmt", ["rgb", "bgr", "bgr24"])
def test_formats_at_odd_offsets(decoder, oracle, pix_fmt):
    st, got, _ = _ragged(decoder, files(SIX), Output(pix_fmt=pix_fmt), align=1)
    assert st == [0] * 6
    for name, g in zip(SIX, got):
        np.testing.assert_array_equal(g, want_rgb(oracle, name, pix_fmt), strict=True, err_msg=name)
    assert decoder.get_param("fused_workgroups") > 0  # (planar and BGR stores of the fused kernel)


@pytest.mark.parametrize("norm_dtype,pix_fmt,align", [("float16", "rgb24", 2), ("bfloat16", "rgb", 2),
                                                      ("float16", "bgr", 2), ("bfloat16", "bgr24", 2)])
def test_normalised_at_two_byte_alignment(decoder, oracle, norm_dtype, pix_fmt, align):
    out = Output(pix_fmt=pix_fmt, normalize=True, norm_dtype=norm_dtype)
    datas = files(SIX)
    offs, _, _ = _layout(datas, out, align=align)
    assert any(o % 4 for o in offs[:6]), "no 16-bit image starts off a 4-byte boundary"
    st, got, _ = _ragged(decoder, datas, out, align=align)
    assert st == [0] * 6
    for name, d, g in zip(SIX, datas, got):
        w = oracle.decode_resize(d, oracle.Resize(), pix_fmt=pix_fmt, normalize=True,
                                 norm_dtype=norm_dtype)
        np.testing.assert_array_equal(g, w.view(np.uint16), strict=True, err_msg=name)
    assert decoder.get_param("fused_workgroups") == 0  # (u8 only)


def test_u8_align_one_gives_odd_offsets():
    out = Output(pix_fmt="rgb24")
    offs, sizes, st = _layout(files(SIX), out, align=1)
    assert st == [0] * 6 and any(o % 2 for o in offs[:6])
    assert all(offs[k + 1] == offs[k] + w * h * 3 for k, (w, h) in enumerate(sizes))


# ---- 3. aspect-preserving chains ---------------------------------------------------

SHAPES = ["odd_227x333", "odd_444_101x67", "one_tile_420", "gray_odd", "two_tiles_420"]
CHAINS = {
    "cover64": dict(fit_w=64, fit_h=64, aspect="increase"),
    "fit48": dict(fit_w=48, fit_h=48, aspect="decrease"),
    "scale=40:-1": dict(fit_w=40, fit_h=-1),
    "scale=-2:30": dict(fit_w=-2, fit_h=30),
}


def _explicit(spec, w, h):
    """``spec`` with a ``-n`` side resolved for a w x h frame by vf_scale's rule
    (ff_scale_adjust_dimensions: the other side times the aspect ratio, to the
    nearest multiple of n, av_rescale's ties away from zero).  The oracle's
    geometry takes explicit sides only."""
    s = dict(spec)
    if s["fit_h"] < 0:
        n = max(-s["fit_h"], 1)
        s["fit_h"] = (s["fit_w"] * h + (w * n) // 2) // (w * n) * n
    if s["fit_w"] < 0:
        n = max(-s["fit_w"], 1)
        s["fit_w"] = (s["fit_h"] * w + (h * n) // 2) // (h * n) * n
    return s


@pytest.mark.parametrize("chain", list(CHAINS))
def test_aspect_preserving_chains(decoder, oracle, chain):
    spec = CHAINS[chain]
    datas = files(SHAPES)
    st, got, sizes = _ragged(decoder, datas, Output(pix_fmt="rgb24", resize=True, **spec))
    assert st == [0] * len(datas)
    seen = set()
    for name, d, g, size in zip(SHAPES, datas, got, sizes):
        i = oracle.parse(d)
        rs = oracle.Resize(**_explicit(spec, i.width, i.height))
        geo = oracle.geometry(i.width, i.height, rs)
        assert size == (geo["ow"], geo["oh"]), name
        seen.add(size)
        np.testing.assert_array_equal(g, oracle.decode_resize(d, rs, "rgb24"), strict=True,
                                      err_msg=name)
    assert len(seen) > 2, "the chain gave these files one size"


def test_large_downscale_takes_the_prepass_beside_small_images(decoder, oracle):
    names = ["one_tile_420", "large_1080p", "gray_odd"]
    datas = files(names)
    spec = dict(fit_w=24, fit_h=24, aspect="increase")  # the shorter side to 24 px
    rs = oracle.Resize(**spec)
    out = Output(pix_fmt="rgb24", resize=True, **spec)
    i = oracle.parse(datas[1])
    plan = _lib.debug_sws_plan(i.width, i.height, 1, 1, "yuv",
                               Output(pix_fmt="rgb24", resize=True, fit_w=43, fit_h=24))
    assert plan["rc"] == 0 and plan["pre"], "1080p to 43x24 does not take hscale_kernel"
    st, got, sizes = _ragged(decoder, datas, out)
    assert st == [0, 0, 0] and sizes[1] == (43, 24)
    for name, d, g in zip(names, datas, got):
        np.testing.assert_array_equal(g, oracle.decode_resize(d, rs, "rgb24"), strict=True,
                                      err_msg=name)


# ---- 4. crops, flips, orientations -------------------------------------------------

def test_source_crops_of_different_sizes(decoder, oracle):
    names = ["q90_420", "odd_227x333", "two_tiles_420", "gray_odd", "odd_444_101x67"]
    crops = [(38, 22, 112, 112), (301, 195, 32, 20), None, (17, 9, 60, 50), (3, 5, 40, 33)]
    datas = files(names)
    st, got, sizes = _ragged(decoder, datas, Output(pix_fmt="rgb24"), crops=crops)
    assert st == [0] * 5
    for name, d, r, g, size in zip(names, datas, crops, got, sizes):
        if r is None:
            w = want_rgb(oracle, name)
        else:
            rr = ref.resolve_data(d, r)
            assert size == (rr[2], rr[3]), name
            w = ref.rgb(d, rr, None, "rgb24")
        np.testing.assert_array_equal(g, w, strict=True, err_msg=name)
    assert decoder.get_param("fused_workgroups") == 6  # (the image without a crop alone)


def test_flips(decoder, oracle):
    names = ["two_tiles_420", "odd_227x333", "gray_odd", "one_tile_420"]
    flips = [1, 2, 3, 0]
    st, got, _ = _ragged(decoder, files(names), Output(pix_fmt="rgb24"), flips=flips)
    assert st == [0] * 4
    for name, f, g in zip(names, flips, got):
        w = want_rgb(oracle, name)
        if f & 1:
            w = np.flip(w, 1)
        if f & 2:
            w = np.flip(w, 0)
        np.testing.assert_array_equal(g, np.ascontiguousarray(w), strict=True, err_msg=name)
    assert decoder.get_param("fused_workgroups") == 1  # (the unflipped one)


@pytest.mark.parametrize("pix_fmt", ["rgb24", "rgb"])
def test_eight_orientations_share_a_buffer(decoder, oracle, pix_fmt):
    """A non-square file under the eight codes at native size: the transposed
    copies have their boxes swapped within one buffer."""
    name = "odd_227x333"
    codes = list(range(8))
    out = Output(pix_fmt=pix_fmt)
    st, got, sizes = _ragged(decoder, files([name]) * 8, out, orients=codes)
    assert st == [0] * 8
    w0 = want_rgb(oracle, name, pix_fmt)
    ax_w, ax_h = (2, 1) if out.planar else (1, 0)
    for c, g, size in zip(codes, got, sizes):
        assert size == ((227, 333) if c & 4 else (333, 227))
        w = np.swapaxes(w0, ax_w, ax_h) if c & 4 else w0  # A(x, y) = C(y, x)
        if c & 1:
            w = np.flip(w, ax_w)
        if c & 2:
            w = np.flip(w, ax_h)
        np.testing.assert_array_equal(g, np.ascontiguousarray(w), strict=True, err_msg=f"code {c}")


# ---- 5. one failure among many -----------------------------------------------------

def _packed(datas):
    offs, total = [], 0
    for d in datas:
        offs.append(total)
        total += (len(d) + 64 + 255) // 256 * 256
    host = np.zeros(total + 512, np.uint8)
    for o, d in zip(offs, datas):
        host[o:o + len(d)] = np.frombuffer(d, np.uint8)
    return host, offs, [len(d) for d in datas], total


def test_failures_leave_their_bytes_and_the_rest_decodes(decoder, oracle):
    """A truncated file, an arithmetic-coded file (through the device entry
    point, whose probes are the caller's: the host entry points fail such a
    file's whole call at the probe, as they always did) and a crop that rounds
    to nothing among good images."""
    names = ["two_tiles_420", "odd_227x333", "q90_420", "gray_odd", "q90_420", "one_tile_420",
             "q90_420", "q90_420"]
    n = len(names)
    datas = files(names)
    datas[2] = cases.truncated()
    datas[4] = cases.arithmetic()
    crops = [None] * n
    crops[6] = (1, 0, 1, 10)    # one column of a 4:2:0 frame: rounds down to no column
    crops[7] = (0, 0, 642, 10)  # wider than the 640 px frame (641 rounds down to the chroma grid)
    want_st = [0, 0, TRUNCATED, 0, UNSUPPORTED, 0, BAD_GEOMETRY, BAD_GEOMETRY]
    infos = [_lib.get_image_info(d) for d in files(names)]
    out = Output(pix_fmt="rgb24")
    offs, sizes, planned = _layout(datas, out, crops, infos=infos)
    assert planned == [0] * 6 + [BAD_GEOMETRY] * 2
    assert sizes[6] == sizes[7] == (0, 0) and offs[n] == offs[7] == offs[6]
    host, in_offs, in_sizes, _ = _packed(datas)
    dev = torch.from_numpy(host).to("cuda:0")
    t = torch.full((offs[n] + TAIL,), GUARD, dtype=torch.uint8, device="cuda:0")
    st = decoder.decode_batch_device(dev.data_ptr(), dev.numel(), in_offs, in_sizes, infos, out,
                                     t.data_ptr(), offs[n], crops=crops, check=False,
                                     ragged=offs[:n])
    assert st == want_st
    a = t.cpu().numpy()
    for k in (2, 4):  # their regions: untouched
        w, h = sizes[k]
        assert (a[offs[k]:offs[k] + w * h * 3] == GUARD).all(), k
    got = _split_buffer(a, out, offs[:n], sizes)
    for k in (0, 1, 3, 5):
        np.testing.assert_array_equal(got[k], want_rgb(oracle, names[k]), strict=True,
                                      err_msg=names[k])


def test_an_extent_past_the_buffer_writes_nothing(decoder):
    datas = files(SIX)
    out = Output(pix_fmt="rgb24")
    offs, sizes, _ = _layout(datas, out)
    t = torch.full((offs[6] + TAIL,), GUARD, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(RuntimeError, match="reaches past the output buffer"):
        decoder.decode_batch(datas, out, t.data_ptr(), offs[6] - 1, ragged=offs[:6])
    assert (t.cpu().numpy() == GUARD).all()
    for bad, text in ((Output(pix_fmt="yuv"), "planar YUV"),
                      (Output(pix_fmt="rgb24", csc="jfif"), "csc = swscale")):
        with pytest.raises(RuntimeError, match=text):
            decoder.decode_batch(datas, bad, t.data_ptr(), offs[6], ragged=offs[:6])
    with pytest.raises(RuntimeError, match="element size"):
        decoder.decode_batch(datas, Output(pix_fmt="rgb24", normalize=True), t.data_ptr(),
                             t.numel(), ragged=[1] + [2 * o for o in offs[1:6]])
    assert (t.cpu().numpy() == GUARD).all()


# ---- 6. the other two entry points -------------------------------------------------

def _check_split(oracle, a, out, offs, sizes):
    for name, g in zip(SPLIT, _split_buffer(a, out, offs, sizes)):
        np.testing.assert_array_equal(g, want_rgb(oracle, name), strict=True, err_msg=name)


def test_device_resident_entry_point(decoder, oracle):
    datas = files(SPLIT)
    n = len(datas)
    out = Output(pix_fmt="rgb24")
    infos = [_lib.get_image_info(d) for d in datas]
    offs, sizes, _ = _layout(datas, out, infos=infos)
    host, in_offs, in_sizes, _ = _packed(datas)
    dev = torch.from_numpy(host).to("cuda:0")
    t = torch.full((offs[n] + TAIL,), GUARD, dtype=torch.uint8, device="cuda:0")
    st = decoder.decode_batch_device(dev.data_ptr(), dev.numel(), in_offs, in_sizes, infos, out,
                                     t.data_ptr(), offs[n], ragged=offs[:n])
    assert st == [0] * n
    _check_split(oracle, t.cpu().numpy(), out, offs[:n], sizes)
    assert decoder.get_param("fused_workgroups") == FUSED_TILES


def test_staged_entry_point(decoder, oracle):
    datas = files(SPLIT)
    n = len(datas)
    out = Output(pix_fmt="rgb24")
    offs, sizes, _ = _layout(datas, out)
    host, in_offs, in_sizes, total = _packed(datas)
    t = torch.full((offs[n] + TAIL,), GUARD, dtype=torch.uint8, device="cuda:0")
    ptr, ticket = decoder.staging_acquire(total)
    ctypes.memmove(ptr, host.ctypes.data, total)
    st = decoder.decode_staged(ticket, total, in_offs, in_sizes, out, t.data_ptr(), offs[n],
                               ragged=offs[:n])
    assert st == [0] * n
    _check_split(oracle, t.cpu().numpy(), out, offs[:n], sizes)


# ---- 7. hand-off re-decode ---------------------------------------------------------

def test_handoff_redecode_lands_at_its_own_offset(decoder, oracle, knobs):
    """A piece hand-off that gives up (handoff_wait_us 0) re-decodes the image
    in one workgroup, as a one-image batch: into its own place and size."""
    knobs("entropy_piece_bytes", 16384)
    knobs("handoff_wait_us", 0)
    names = ["gray_odd", "large_1080p", "one_tile_420"]
    datas = files(names)
    assert len(datas[1]) > 4 * 16384 and all(len(datas[k]) <= 16384 for k in (0, 2))
    before = decoder.get_param("handoff_retries")
    st, got, sizes = _ragged(decoder, datas, Output(pix_fmt="rgb24"))
    assert decoder.get_param("handoff_retries") > before, "no hand-off gave up"
    assert st == [0, 0, 0] and sizes[1] == (1920, 1080)
    # the split reported is the batch's, not the one-image re-decode's: 120 MCUs
    # in 3 tiles x 68 MCU rows, and the 16 x 16 image's one tile
    assert decoder.get_param("fused_workgroups") == 3 * 68 + 1
    assert decoder.get_param("generic_workgroups") >= 1
    for name, g in zip(names, got):
        np.testing.assert_array_equal(g, want_rgb(oracle, name), strict=True, err_msg=name)


# ---- 8. the consumption rule -------------------------------------------------------

def test_a_failing_call_consumes_the_offsets(decoder):
    datas = files(SIX)
    out = Output(pix_fmt="rgb24")
    offs, _, _ = _layout(datas, out)
    t = torch.full((offs[6] + TAIL,), GUARD, dtype=torch.uint8, device="cuda:0")
    decoder.set_ragged(offs[:5])
    with pytest.raises(RuntimeError, match="5 offsets for a batch of 6 images"):
        decoder.decode_batch(datas, out, t.data_ptr(), offs[6])
    # consumed: the next plain call is under the one-size rule again
    with pytest.raises(RuntimeError, match="same output size"):
        decoder.decode_batch(datas, out, t.data_ptr(), offs[6])
    # NULL / 0 clears
    decoder.set_ragged(offs[:6])
    decoder.set_ragged(None)
    with pytest.raises(RuntimeError, match="same output size"):
        decoder.decode_batch(datas, out, t.data_ptr(), offs[6])
    assert (t.cpu().numpy() == GUARD).all()
    # views and ragged exclude each other
    v = torch.zeros(64 * 64 * 3, dtype=torch.uint8, device="cuda:0")
    group = _lib.ViewGroup(Output(pix_fmt="rgb24", resize=True, fit_w=64, fit_h=64), [(0, None)],
                           v.data_ptr(), v.numel())
    with pytest.raises(RuntimeError, match="views and spdl_hj_set_ragged"):
        decoder.decode_batch(datas[:1], out, 0, 0, views=[group], ragged=[0])


# ---- 9. load_image_list ------------------------------------------------------------

def _host(buf):
    if hasattr(buf, "__cuda_array_interface__"):
        return sio.to_torch(buf).cpu().numpy()
    return sio.to_numpy(buf)


@pytest.mark.parametrize("on_device", [True, False])
def test_load_image_list(oracle, on_device):
    names = ["two_tiles_420", "odd_227x333", "gray_odd", "odd_444_101x67"]
    datas = files(names)
    cfg = sio.cuda_config(device_index=0) if on_device else None
    for kw in (dict(), dict(width=64, height=64, scale_mode="cover"),
               dict(width=40), dict(width=48, scale_mode="fit", pix_fmt="rgb")):
        bufs, idx = sio.load_image_list(datas, device_config=cfg, **kw)
        assert idx == [0, 1, 2, 3]
        desc = None
        if kw:
            w, h = kw.get("width"), kw.get("height", kw.get("width") if "scale_mode" in kw else -1)
            ar = {"cover": ":force_original_aspect_ratio=increase",
                  "fit": ":force_original_aspect_ratio=decrease"}.get(kw.get("scale_mode"), "")
            desc = f"scale=w={w}:h={h}:flags=bicubic{ar},format=pix_fmts={kw.get('pix_fmt', 'rgb24')}"
        for d, b in zip(datas, bufs):
            one = sio.load_image(d, device_config=cfg, pix_fmt=kw.get("pix_fmt", "rgb24"),
                                 **({"filter_desc": desc} if desc else {}))
            got, want = _host(b), _host(one)
            np.testing.assert_array_equal(got, want, strict=True)
    # native size against the oracle itself
    bufs, _ = sio.load_image_list(datas, device_config=cfg)
    for name, b in zip(names, bufs):
        np.testing.assert_array_equal(_host(b), want_rgb(oracle, name), strict=True, err_msg=name)
    # strict=False drops the failed image
    broken = [datas[0], cases.truncated(), datas[2], b"not a jpeg", datas[1]]
    with pytest.raises(RuntimeError, match="Failed to load some images"):
        sio.load_image_list(broken, device_config=cfg)
    bufs, idx = sio.load_image_list(broken, device_config=cfg, strict=False)
    assert idx == [0, 2, 4]
    for k, name in zip(range(3), ("two_tiles_420", "gray_odd", "odd_227x333")):
        np.testing.assert_array_equal(_host(bufs[k]), want_rgb(oracle, name), strict=True)


@pytest.mark.parametrize("kw", [dict(), dict(normalize=True, norm_dtype="bfloat16")],
                         ids=["u8", "bf16"])
def test_load_image_list_views_keep_the_allocation(oracle, kw):
    """With cuda_config(allocator=...) the one allocation lives as long as any
    returned buffer, or a tensor made of one, does: its deleter runs once, after
    the last of them is gone."""
    import gc

    calls = {"alloc": 0, "free": 0}

    def alloc(size, device, stream):
        calls["alloc"] += 1
        return torch.cuda.caching_allocator_alloc(size, device, stream)

    def free(ptr):
        calls["free"] += 1
        torch.cuda.caching_allocator_delete(ptr)

    names = ["two_tiles_420", "odd_227x333", "gray_odd"]
    datas = files(names)

    def want(name, d):
        if not kw:
            return want_rgb(oracle, name)
        return oracle.decode_resize(d, oracle.Resize(), pix_fmt="rgb24", normalize=True,
                                    norm_dtype="bfloat16")

    def host(t):
        return t.cpu().view(torch.int16).numpy().view(np.uint16) if kw else t.cpu().numpy()

    cfg = sio.cuda_config(0, allocator=(alloc, free))
    bufs, idx = sio.load_image_list(datas, device_config=cfg, **kw)
    gc.collect()
    assert idx == [0, 1, 2] and calls == {"alloc": 1, "free": 0}
    # a tensor of the last buffer outlives every buffer
    last = sio.to_torch(bufs[2])
    first = bufs.pop(0)
    del bufs
    gc.collect()
    assert calls["free"] == 0
    # (another allocation of the pool would land on freed memory)
    scratch = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device="cuda:0")
    np.testing.assert_array_equal(host(sio.to_torch(first)), want(names[0], datas[0]), strict=True)
    del first
    gc.collect()
    assert calls["free"] == 0
    np.testing.assert_array_equal(host(last), want(names[2], datas[2]), strict=True)
    del last, scratch
    gc.collect()
    assert calls == {"alloc": 1, "free": 1}


def _tagged(data, exif):
    """``data`` with an Exif APP1 of orientation ``exif`` as Pillow writes it (the
    coded image untouched: the segment goes in behind SOI)."""
    from PIL import Image

    ex = Image.Exif()
    ex[0x0112] = exif
    app1 = b"Exif\x00\x00" + ex.tobytes().removeprefix(b"Exif\x00\x00")
    return data[:2] + b"\xff\xe1" + (len(app1) + 2).to_bytes(2, "big") + app1 + data[2:]


def test_load_image_list_exif_orientation(oracle):
    """Portrait and landscape files at native size in one call: each file's tag
    turns its own box; a flip acts on the displayed image."""
    name = "odd_227x333"
    d = files([name])[0]
    tags = [1, 6, 8, 3, 5]
    datas = [_tagged(d, t) for t in tags]
    cfg = sio.cuda_config(device_index=0)
    w0 = want_rgb(oracle, name)

    def want(code):
        w = np.swapaxes(w0, 0, 1) if code & 4 else w0
        if code & 1:
            w = np.flip(w, 1)
        if code & 2:
            w = np.flip(w, 0)
        return np.ascontiguousarray(w)

    bufs, idx = sio.load_image_list(datas, device_config=cfg, exif_orientation=True)
    assert idx == list(range(5))
    for t, b in zip(tags, bufs):
        code = _lib.exif_code(t)
        got = _host(b)
        assert got.shape == ((333, 227, 3) if code & 4 else (227, 333, 3))
        np.testing.assert_array_equal(got, want(code), strict=True, err_msg=f"tag {t}")
    flips = [1, 0, 2, 3, 1]
    bufs, _ = sio.load_image_list(datas, device_config=cfg, exif_orientation=True, flips=flips)
    for t, f, b in zip(tags, flips, bufs):
        np.testing.assert_array_equal(_host(b), want(_lib.exif_code(t) ^ f), strict=True,
                                      err_msg=f"tag {t}, flip {f}")
    # without the flag the tags mean nothing
    bufs, _ = sio.load_image_list(datas, device_config=cfg)
    for b in bufs:
        np.testing.assert_array_equal(_host(b), w0, strict=True)
