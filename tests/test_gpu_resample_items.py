"""Resample items on the GPU (include/spdl_hipjpeg.h "resample items"): several
outputs per image, each its own size, box and flip, every byte equal to
Pillow's own array."""

import io

import numpy as np
import pytest
import torch
from PIL import Image, ImageOps

import spdl_amd.io as sio
from spdl_amd._lib import Output, Resample, ResampleItems
from tests import cases, turbo_ref
from tests.test_resample import PIL_FILTER

pytestmark = pytest.mark.gpu
CFG = sio.cuda_config(device_index=0)
BAD_GEOMETRY, GUARD = 7, 0xA5
FILES = ["odd_227x333", "odd_444_101x67", "q90_420", "gray_odd", "tiny_1x1", "tiny_8x8"]
# (box, clamp, size) of the three items of an image; frame 333 x 227 and 640 x 480
MULTI = {"odd_227x333": [((100, 50, 333, 227), True, (67, 13)), (None, False, (224, 224)),
                         ((10.5, 3.25, 333, 227), False, (9, 70))],
         "q90_420": [((3.5, 7.25, 600.0, 470.5), False, (67, 13)), ((320, 240, 640, 480), True, (224, 224)),
                     ((0, 0, 63, 479), True, (9, 70))]}


def pillow(name, size, filt, box=None, clamp=False, gap=None, flip=0) -> np.ndarray:
    im = Image.open(io.BytesIO(cases.case(name))).convert("RGB")
    im = im.crop(box).resize(size, PIL_FILTER[filt], reducing_gap=gap) if clamp and box else \
        im.resize(size, PIL_FILTER[filt], box=box, reducing_gap=gap)
    im = ImageOps.mirror(im) if flip & 1 else im
    return np.asarray(ImageOps.flip(im) if flip & 2 else im)


def run(decoder, names, items, filt, out=Output(pix_fmt="rgb24", csc="turbo"), gap=None):
    """items (image, box, clamp, size, flip) packed 64 bytes apart into a guarded
    buffer: (image statuses, ResampleItems, each item's bytes in the output's dtype)."""
    esz = 1 if out.torch_dtype == torch.uint8 else 2
    offs, end = [], 0
    for _, _, _, (w, h), _ in items:
        offs.append(end)
        end += (w * h * 3 * esz + 63) // 64 * 64
    held = ResampleItems(filt, [(i, b, c, s, (0, 0), s, f, o) for (i, b, c, s, f), o in zip(items, offs)], gap)
    t = torch.full((end + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    st = decoder.decode_batch([cases.case(n) for n in names], out, t.data_ptr(), end, check=False,
                              resample_items=held)
    a = t.cpu().numpy()
    got = [a[o:o + w * h * 3 * esz].view(np.uint8 if esz == 1 else np.uint16)
           for o, (_, _, _, (w, h), _) in zip(offs, items)]
    gaps = np.ones(end + 64, bool)
    for o, g in zip(offs, got):
        gaps[o:o + g.nbytes] = False
    assert (a[gaps] == GUARD).all(), "wrote outside the items' boxes"
    return st, held, got


@pytest.mark.parametrize("thumb", [sio.pil_thumbnail((128, 128)),
                                   sio.pil_thumbnail((64, 48), "lanczos", reducing_gap=3.0)], ids=str)
def test_ragged_thumbnails(decoder, oracle, thumb):
    bufs, idx = sio.load_image_list([cases.case(n) for n in FILES], csc="turbo", resample=thumb,
                                    device_config=CFG)
    assert idx == list(range(len(FILES)))
    for name, buf in zip(FILES, bufs):
        im = Image.open(io.BytesIO(cases.case(name)))
        im.thumbnail(thumb.size, PIL_FILTER[thumb.filter], reducing_gap=thumb.reducing_gap)
        np.testing.assert_array_equal(sio.to_torch(buf).cpu().numpy(), np.asarray(im.convert("RGB")),
                                      strict=True)


def test_shorter_side_and_flips_through_load_image_list(decoder, oracle):
    names = ["odd_227x333", "odd_444_101x67"]
    bufs, _ = sio.load_image_list([cases.case(n) for n in names], csc="turbo", flips=["h", None],
                                  resample=sio.pil_resize(shorter=40, filter="bicubic"), device_config=CFG)
    for name, buf, flip in zip(names, bufs, (1, 0)):
        w, h = Image.open(io.BytesIO(cases.case(name))).size
        size = (40, int(40 * h / w)) if w <= h else (int(40 * w / h), 40)
        np.testing.assert_array_equal(sio.to_torch(buf).cpu().numpy(),
                                      pillow(name, size, "bicubic", flip=flip), strict=True)


def test_three_items_per_image_interleaved(decoder, oracle):
    names = list(MULTI)
    items = [(i, *MULTI[names[i]][k], 0) for k in range(3) for i in range(2)]
    st, held, got = run(decoder, names, items, "bicubic")
    assert st == [0, 0] and held.statuses == [0] * 6
    assert decoder.get_param("resample_items") == 6
    for (i, box, clamp, size, _), g in zip(items, got):
        want = pillow(names[i], size, "bicubic", box, clamp)
        np.testing.assert_array_equal(g.reshape(want.shape), want, strict=True)


@pytest.mark.parametrize("pix_fmt", ["rgb24", "rgb", "bgr24"])
@pytest.mark.parametrize("flip", [0, 1, 2, 3])
def test_flips(decoder, oracle, pix_fmt, flip):
    items = [(0, *MULTI["odd_227x333"][k], flip) for k in (0, 2)]
    st, held, got = run(decoder, ["odd_227x333"], items, "bilinear", Output(pix_fmt=pix_fmt, csc="turbo"))
    assert st == [0] and held.statuses == [0, 0]
    for (_, box, clamp, size, _), g in zip(items, got):
        want = turbo_ref.layout(pillow("odd_227x333", size, "bilinear", box, clamp, flip=flip), pix_fmt)
        np.testing.assert_array_equal(g.reshape(want.shape), want, strict=True)


def test_f16_equals_the_u8_bytes_normalised(decoder, oracle):
    box, clamp, size = MULTI["odd_227x333"][0]
    out = Output(pix_fmt="rgb24", csc="turbo", normalize=True, norm_dtype="float16")
    st, _, got = run(decoder, ["odd_227x333"], [(0, box, clamp, size, 1)], "bicubic", out)
    want = turbo_ref.layout(pillow("odd_227x333", size, "bicubic", box, clamp, flip=1), "rgb24",
                            normalize=True, norm_dtype="float16")
    assert st == [0]
    np.testing.assert_array_equal(got[0].reshape(want.shape), want.view(np.uint16), strict=True)


def test_a_refused_item_between_two_good_ones(decoder, oracle):
    """640 -> 14 in lanczos takes 275 taps: that item alone is refused."""
    items = [(0, None, False, (40, 30), 0), (0, None, False, (14, 12), 0), (0, (0, 0, 64, 48), True, (9, 7), 1)]
    st, held, got = run(decoder, ["q90_420"], items, "lanczos")
    assert st == [0] and held.statuses == [0, BAD_GEOMETRY, 0]
    assert (got[1] == GUARD).all() and decoder.get_param("resample_items") == 2
    for k in (0, 2):
        _, box, clamp, size, flip = items[k]
        want = pillow("q90_420", size, "lanczos", box, clamp, flip=flip)
        np.testing.assert_array_equal(got[k].reshape(want.shape), want, strict=True)


def test_one_whole_frame_item_per_image_equals_the_plain_submission(decoder, oracle):
    names = ["odd_227x333", "q90_420", "gray_odd"]
    datas = [cases.case(n) for n in names]
    out = Output(pix_fmt="rgb24", csc="turbo")
    t = torch.zeros((3, 224, 224, 3), dtype=torch.uint8, device="cuda:0")
    assert decoder.decode_batch(datas, out, t.data_ptr(), t.numel(), resample=Resample("bicubic", 224, 224)) == [0] * 3
    plain_wgs = decoder.get_param("resample_workgroups")
    st, _, got = run(decoder, names, [(i, None, False, (224, 224), 0) for i in range(3)], "bicubic")
    assert st == [0] * 3 and decoder.get_param("resample_items") == 3
    # (the same tiles, and one workgroup for the three images' statuses)
    assert decoder.get_param("resample_item_workgroups") == plain_wgs + 1
    assert decoder.get_param("resample_workgroups") == 0
    for k in range(3):
        np.testing.assert_array_equal(got[k].reshape(224, 224, 3), t[k].cpu().numpy(), strict=True)


def test_multi_crop_views(decoder, oracle):
    names = ["odd_227x333", "q90_420"]
    boxes = [[[(0, 0, 100, 100), (33, 27, 300, 200)], [(5, 5, 600, 400), (320, 240, 320, 240)]],
             [[(1, 1, 50, 60)], [None]]]
    flips = [[[0, "h"], [None, "v"]], [[0], ["hv"]]]
    groups = [dict(resample=sio.pil_resize(s, "bicubic"), boxes=b, flips=f)
              for s, b, f in zip([(32, 32), (17, 9)], boxes, flips)]
    res = sio.load_image_views([cases.case(n) for n in names], groups, csc="turbo", device_config=CFG)
    for (buf, idx), g, size in zip(res, groups, [(32, 32), (17, 9)]):
        rows = [(i, b, f) for i in range(2) for b, f in zip(g["boxes"][i], g["flips"][i])]
        assert idx == [r[0] for r in rows] and sio.to_torch(buf).data_ptr() % 256 == 0
        for r, (i, b, f) in enumerate(rows):
            box = None if b is None else (b[0], b[1], b[0] + b[2], b[1] + b[3])
            want = pillow(names[i], size, "bicubic", box, True, flip={0: 0, None: 0, "h": 1, "v": 2, "hv": 3}[f])
            np.testing.assert_array_equal(sio.to_torch(buf)[r].cpu().numpy(), want, strict=True)
