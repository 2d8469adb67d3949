"""GPU tests of the Pillow-exact draft (``draft=`` with ``csc="turbo"``,
include/spdl_hipjpeg.h "Pillow-exact draft"; -m gpu): idct_draft_kernel and the
draft instantiations of the output kernels through the C-ABI (``Decoder``) and
the Python surface, byte-exact against ``tests/draft_ref.py`` (which
tests/test_draft.py holds against Pillow), the resize against Pillow itself."""

import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

import spdl_amd.io as sio
from spdl_amd._lib import Output
from tests import draft_ref as ref
from tests import turbo_ref
from tests.test_gpu_turbo import GUARD, _decode

pytestmark = pytest.mark.gpu

TURBO = Output(pix_fmt="rgb24", csc="turbo")
CFG = sio.cuda_config(device_index=0)


@functools.lru_cache(maxsize=None)
def _want(name: str, level: int) -> np.ndarray:
    a = ref.rgb_u8(ref.case(name), level)
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("level", [1, 2, 3])
@pytest.mark.parametrize("size", ["83x61", "9x7", "17x3"])
def test_plain_batch_of_one_size(decoder, oracle, size, level):
    """Gray and every sampling at one size and level in one plain submission
    (83x61: the progressive and the restart file as well)."""
    names = [f"{s}_{size}" for s in ref.LUMA] + (["progressive", "restart"] if size == "83x61" else [])
    st, got = _decode(decoder, [ref.case(n) for n in names], TURBO, _want(names[0], level).shape,
                      draft=[level] * len(names))
    assert st == [0] * len(names) and decoder.get_param("draft_images") == len(names)
    for k, n in enumerate(names):
        np.testing.assert_array_equal(got[k], _want(n, level), strict=True, err_msg=n)


@pytest.mark.parametrize("shift,pix_fmt,norm", [(0, "rgb24", None), (1, "bgr", None),
                                                (2, "rgb24", "float16"), (3, "bgr24", "bfloat16")])
def test_ragged_mixed_levels_and_formats(decoder, oracle, shift, pix_fmt, norm):
    """The whole table in one ragged submission through load_image_list, image
    k at level (k + shift) % 4 -- level 0 among them -- in four layouts."""
    levels = [(k + shift) % 4 for k in range(len(ref.NAMES))]
    kw = dict(normalize=True, norm_dtype=norm) if norm else {}
    bufs, idx = sio.load_image_list([ref.case(n) for n in ref.NAMES], csc="turbo", draft=levels,
                                    pix_fmt=pix_fmt, device_config=CFG, **kw)
    assert idx == list(range(len(ref.NAMES)))
    for n, lv, b in zip(ref.NAMES, levels, bufs):
        got = sio.to_torch(b).cpu()
        got = got.view(torch.int16).numpy().view(np.uint16) if norm else got.numpy()
        np.testing.assert_array_equal(got, turbo_ref.layout(_want(n, lv), pix_fmt, **kw),
                                      strict=True, err_msg=f"{n} L{lv}")


@pytest.mark.parametrize("filter", ["bilinear", "lanczos"])
def test_resample_of_the_draft_frame_is_pillows(decoder, oracle, filter):
    """Image.draft(...), then crop(box).resize(...): boxes in the draft frame's
    coordinates; draft="auto" picks the largest level that covers the output."""
    names = ["420_83x61", "422_83x61", "gray_83x61", "progressive"]
    boxes = [(3, 2, 30, 25), None, (0, 0, 41, 30), (5, 5, 17, 11)]
    flt = {"bilinear": Image.BILINEAR, "lanczos": Image.LANCZOS}[filter]

    def pillow(name, request, size, box):
        im = Image.open(io.BytesIO(ref.case(name)))
        im.draft("RGB", request)
        assert im.size == size
        im = im.convert("RGB")
        if box is not None:
            im = im.crop((box[0], box[1], box[0] + box[2], box[1] + box[3]))
        return np.asarray(im.resize((20, 14), flt))

    def load(srcs, **kw):
        return sio.to_torch(sio.load_image_batch(srcs, width=None, height=None, csc="turbo",
                                                 device_config=CFG, **kw)).cpu().numpy()
    got = load([ref.case(n) for n in names], draft=1,
               resample=sio.pil_resize((20, 14), filter, boxes=boxes))
    for k, (n, b) in enumerate(zip(names, boxes)):
        np.testing.assert_array_equal(got[k], pillow(n, (41, 30), (42, 31), b), err_msg=n)
    # (83x61 into 20x14: level 2, a frame of 21x16, is the largest that covers it)
    auto = load([ref.case(names[1])], draft="auto", resample=sio.pil_resize((20, 14), filter))
    np.testing.assert_array_equal(auto[0], pillow(names[1], (20, 15), (21, 16), None))


def test_stale_workspace_and_all_zero_levels(decoder, oracle):
    """The same file after an all-white and an all-black larger one: every
    plane byte the output stage reads is written by this submission.  All-zero
    levels are the submission without the call, and lay out its planes."""
    name, data = "420_83x61", ref.case("420_83x61")
    planes = []
    for fill in (255, 0):
        big = ref.cases._enc(np.full((200, 300, 3), fill, np.uint8), quality=90, subsampling=0)
        assert _decode(decoder, [big], TURBO, (200, 300, 3))[0] == [0]
        for level in (3, 2, 1, 0):
            st, got = _decode(decoder, [data], TURBO, _want(name, level).shape, draft=[level])
            assert st == [0] and decoder.get_param("draft_images") == (level > 0)
            np.testing.assert_array_equal(got[0], _want(name, level), strict=True)
            planes.append(decoder.get_param("planes_bytes"))
    _decode(decoder, [data], TURBO, _want(name, 0).shape)
    assert planes[:4] == sorted(planes[:4]) and planes[3] == decoder.get_param("planes_bytes")


@pytest.mark.parametrize("out,kw", [
    (TURBO, dict(draft=[4])), (TURBO, dict(draft=[1, 1])),
    (Output(pix_fmt="rgb24"), dict(draft=[1])), (Output(pix_fmt="rgb24", csc="jfif"), dict(draft=[1])),
    (TURBO, dict(draft=[1], crops=[(0, 0, 16, 16)])), (TURBO, dict(draft=[0], flips=[1])),
    (TURBO, dict(draft=[1], orients=[5])), (TURBO, dict(draft=[1], lowres=[1]))])
def test_c_abi_refusals_write_nothing(decoder, oracle, out, kw):
    t = torch.full((83 * 61 * 3,), GUARD, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(RuntimeError):
        decoder.decode_batch([ref.case("420_83x61")], out, t.data_ptr(), t.numel(), **kw)
    assert (t.cpu().numpy() == GUARD).all()
    # (the levels were consumed: the next submission is a plain one)
    st, got = _decode(decoder, [ref.case("420_83x61")], TURBO, (61, 83, 3))
    assert st == [0] and decoder.get_param("draft_images") == 0
    np.testing.assert_array_equal(got[0], _want("420_83x61", 0), strict=True)
