"""GPU tests of the Pillow-exact grayscale formats (``pix_fmt="L"`` / ``"Y"``
with ``csc="turbo"``, include/spdl_hipjpeg.h "Pillow-exact grayscale"; -m gpu):
the one-channel instantiations of turbo_rgb_kernel and turbo_rgb_draft_kernel
and the luma-only IDCT stage, byte for byte against Pillow itself."""

import ctypes
import io

import numpy as np
import pytest
import torch
from PIL import Image

import spdl_amd.io as sio
from spdl_amd import _lib
from spdl_amd._lib import Output
from tests import cases
from tests import turbo_cases as tc
from tests import turbo_ref as ref

pytestmark = pytest.mark.gpu

INVALID_ARG = 8
GUARD = 0xA5
# odd widths (the vector store's ragged tail), every sampling, gray, RGB-coded
NAMES = ["420_33x33", "422_33x33", "444_17x15", "gray", "l12_16x17", "l41_15x9", "rgb_coded"]


def pillow(data: bytes, fmt: str, level: int = 0) -> np.ndarray:
    """[h, w, 1]: convert("L") of the (draft) RGB frame, or draft("L", size)."""
    im = Image.open(io.BytesIO(data))
    size = _lib.draft_size(*im.size, level)
    # (a request of (W >> level, H >> level): Pillow decodes at this level)
    im.draft("L" if fmt == "Y" else "RGB", (max(im.width >> level, 1), max(im.height >> level, 1)))
    assert im.size == tuple(size)
    return np.asarray(im.convert("L"))[..., None]


def ragged(dec, datas, out, wants, **kw):
    """One ragged submission at byte alignment 1 from an odd first byte into a
    guarded buffer: every box equal to its `want`, no other byte written."""
    esz = 1 if out.torch_dtype == torch.uint8 else 2
    offs, _, st = _lib.ragged_layout([_lib.get_image_info(d) for d in datas], out, align=esz,
                                     **({"draft": kw["draft"]} if "draft" in kw else {}))
    assert st == [0] * len(datas)
    lead = 3 * esz
    t = torch.full((lead + offs[-1] + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    assert dec.decode_batch(datas, out, t.data_ptr(), lead + offs[-1],
                            ragged=[o + lead for o in offs[:-1]], **kw) == [0] * len(datas)
    a = t.cpu().numpy()
    untouched = np.ones(a.size, bool)
    for k, want in enumerate(wants):
        first, nbytes = lead + offs[k], want.size * esz
        got = a[first:first + nbytes]
        got = (got.view(np.uint16) if esz == 2 else got).reshape(want.shape)
        np.testing.assert_array_equal(got, want, strict=True, err_msg=str(k))
        untouched[first:first + nbytes] = False
    assert (a[untouched] == GUARD).all(), "a byte outside the boxes was written"


@pytest.mark.parametrize("fmt", ["L", "Y"])
def test_native_size_ragged_and_plain(decoder, oracle, fmt):
    datas = [tc.case(n) for n in NAMES]
    ragged(decoder, datas, Output(pix_fmt=fmt, csc="turbo"), [pillow(d, fmt) for d in datas])
    got = sio.to_torch(sio.load_image_batch(datas[:2], width=None, height=None, pix_fmt=fmt,
                                            device_config=sio.cuda_config(device_index=0), csc="turbo"))
    assert got.shape == (2, 33, 33, 1)
    for k in range(2):
        np.testing.assert_array_equal(got[k].cpu().numpy(), pillow(datas[k], fmt), strict=True)


@pytest.mark.parametrize("fmt", ["L", "Y"])
def test_draft_levels(decoder, oracle, fmt):
    names = ["420_33x33", "422_33x33", "444_17x15", "gray", "l12_16x17", "luma_below_chroma"]
    for level in (1, 2, 3):
        datas = [tc.case(n) for n in names]
        ragged(decoder, datas, Output(pix_fmt=fmt, csc="turbo"),
               [pillow(d, fmt, level) for d in datas], draft=[level] * len(datas))
        assert decoder.get_param("draft_images") == len(datas)


@pytest.mark.parametrize("norm", ["float16", "bfloat16"])
def test_normalised_dtypes_use_channel_0(decoder, oracle, norm):
    """(x / 255 - mean[0]) / std[0], rounded as the RGB formats round channel 0."""
    datas = [tc.case(n) for n in ("420_33x33", "l41_15x9", "444_1x1")]
    for fmt in ("L", "Y"):
        wants = [ref.layout(np.repeat(pillow(d, fmt), 3, axis=2), "rgb24", normalize=True,
                            norm_dtype=norm)[..., :1] for d in datas]
        ragged(decoder, datas, Output(pix_fmt=fmt, csc="turbo", normalize=True, norm_dtype=norm), wants)


def test_y_lays_out_and_transforms_luma_alone(decoder, oracle):
    # 4:2:0, 8 x 6 MCUs: 288 blocks are two IDCT workgroups of 256, the 192 luma blocks one
    data = cases._enc(tc.pixels(5, 128, 96), quality=90, subsampling=2)
    info = _lib.get_image_info(data)
    figures = {}
    for fmt in ("rgb24", "Y"):
        out = Output(pix_fmt=fmt, csc="turbo")
        n = info.width * info.height * out.channels
        t = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        assert decoder.decode_batch([data], out, t.data_ptr(), n) == [0]
        figures[fmt] = (decoder.get_param("planes_bytes"), decoder.get_param("idct_workgroups"))
        if fmt == "Y":
            np.testing.assert_array_equal(t.cpu().numpy().reshape(info.height, info.width, 1),
                                          pillow(data, "Y"), strict=True)
    assert figures["Y"][0] < figures["rgb24"][0] and figures["Y"][1] < figures["rgb24"][1], figures


CFG = dict(width=None, height=None, csc="turbo")
TILED = f"420_{tc.TILE_W + 1}x{tc.TILE_H + 1}"
FILTERS = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}


def gray(data: bytes, fmt: str) -> Image.Image:
    """The mode-L image the passes run on: convert("L"), or draft("L", size)."""
    im = Image.open(io.BytesIO(data))
    if fmt == "Y":
        im.draft("L", im.size)
    return im.convert("L")


@pytest.mark.parametrize("filt", list(FILTERS))
@pytest.mark.parametrize("fmt", ["L", "Y"])
def test_pil_resize(decoder, oracle, fmt, filt):
    """An odd box whose chroma neighbours lie outside it, a frame of several
    tiles, an RGB-coded file; into (24, 24) and a wide (70, 19)."""
    names, boxes = ["420_33x33", TILED, "rgb_coded"], [(3, 5, 21, 17), None, (1, 1, 99, 64)]
    cfg = sio.cuda_config(device_index=0)
    for size in ((24, 24), (70, 19)):
        got = sio.to_torch(sio.load_image_batch(
            [tc.case(n) for n in names], pix_fmt=fmt, device_config=cfg, **CFG,
            resample=sio.pil_resize(size, filt, boxes=boxes))).cpu().numpy()
        assert got.shape == (3, size[1], size[0], 1)
        for k, (n, b) in enumerate(zip(names, boxes)):
            im = gray(tc.case(n), fmt)
            if b is not None:
                im = im.crop((b[0], b[1], b[0] + b[2], b[1] + b[3]))
            np.testing.assert_array_equal(got[k, ..., 0], np.asarray(im.resize(size, FILTERS[filt])),
                                          strict=True, err_msg=f"{n} {size}")


@pytest.mark.parametrize("fmt", ["L", "Y"])
def test_thumbnail_and_reducing_gap(decoder, oracle, fmt):
    cfg = sio.cuda_config(device_index=0)
    names = ["420_33x33", TILED, "gray", "l12_16x17"]
    bufs, idx = sio.load_image_list([tc.case(n) for n in names], csc="turbo", pix_fmt=fmt, align=1,
                                    device_config=cfg, resample=sio.pil_thumbnail((16, 16)))
    assert idx == list(range(len(names)))
    for n, b in zip(names, bufs):
        # Image.thumbnail's steps with the gray conversion ahead of the resize: its
        # draft request (size x reducing_gap 2.0), then resize(box=the draft's box)
        final = Image.open(io.BytesIO(tc.case(n)))
        final.thumbnail((16, 16))
        im = Image.open(io.BytesIO(tc.case(n)))
        res = im.draft("L" if fmt == "Y" else "RGB", (32, 32))
        want = im.convert("L").resize(final.size, Image.BICUBIC, box=res[1] if res else None,
                                      reducing_gap=2.0)
        np.testing.assert_array_equal(sio.to_torch(b).cpu().numpy()[..., 0], np.asarray(want),
                                      strict=True, err_msg=n)
    # factors (8, 4): cell sums ahead of the passes
    got = sio.to_torch(sio.load_image_batch([tc.case(TILED)], pix_fmt=fmt, device_config=cfg, **CFG,
                                            resample=sio.pil_resize((16, 8), "bicubic", reducing_gap=1.0)))
    assert _lib.thread_decoder(0).get_param("reduce_images") == 1  # (the loaders' decoder)
    want = gray(tc.case(TILED), fmt).resize((16, 8), Image.BICUBIC, reducing_gap=1.0)
    np.testing.assert_array_equal(got[0, ..., 0].cpu().numpy(), np.asarray(want), strict=True)


@pytest.mark.parametrize("fmt", ["L", "Y"])
def test_items_two_boxes_per_image_and_a_flip(decoder, oracle, fmt):
    names = ["420_33x33", TILED]
    boxes = [[(3, 5, 21, 17), None], [(0, 0, 100, 30), (64, 1, 65, 32)]]
    flips = [[0, 1], [2, 3]]
    ((buf, src),) = sio.load_image_views(
        [tc.case(n) for n in names], [dict(resample=sio.pil_resize((20, 11), "bilinear"), boxes=boxes,
                                           flips=flips, pix_fmt=fmt)],
        device_config=sio.cuda_config(device_index=0), csc="turbo")
    got = sio.to_torch(buf).cpu().numpy()
    assert got.shape == (4, 11, 20, 1) and src == [0, 0, 1, 1]
    for r, (i, j) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        im, b = gray(tc.case(names[i]), fmt), boxes[i][j]
        if b is not None:
            im = im.crop((b[0], b[1], b[0] + b[2], b[1] + b[3]))
        want = np.asarray(im.resize((20, 11), Image.BILINEAR))
        want = want[::-1 if flips[i][j] & 2 else 1, ::-1 if flips[i][j] & 1 else 1]
        np.testing.assert_array_equal(got[r, ..., 0], want, strict=True, err_msg=str((i, j)))


@pytest.mark.parametrize("csc", ["swscale", "jfif"])
@pytest.mark.parametrize("fmt", ["L", "Y"])
def test_refusals_write_nothing(decoder, oracle, fmt, csc):
    data = tc.case("420_33x33")
    out = Output(pix_fmt=fmt, csc=csc)
    t = torch.full((33 * 33 * 3 + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    keep = _lib.buffer_address(data)  # (address, size, and what holds the bytes alive)
    status, err, spec = (ctypes.c_int32 * 1)(), ctypes.create_string_buffer(1024), out.to_c()
    rc = _lib.lib().spdl_hj_decode_batch(decoder._h, (ctypes.c_void_p * 1)(keep[0]),
                                         (ctypes.c_size_t * 1)(keep[1]), 1, ctypes.byref(spec),
                                         t.data_ptr(), 33 * 33 * 3, None, 1, status, err, 1024)
    assert rc == INVALID_ARG
    torch.cuda.synchronize()
    assert bool((t == GUARD).all()), "a refused submission wrote output"
