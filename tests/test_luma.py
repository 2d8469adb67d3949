"""CPU tests of the Pillow-exact grayscale formats (``pix_fmt="L"`` / ``"Y"``,
include/spdl_hipjpeg.h "Pillow-exact grayscale"): the two rules against Pillow
over the oracle's islow planes, and what the Python surface refuses before it
reads anything."""

import io

import numpy as np
import pytest
from PIL import Image

import spdl_amd.io as sio
from oracle import oracle as O
from spdl_amd import _lib
from spdl_amd._lib import Output
from tests import turbo_cases as tc
from tests import turbo_ref as ref

NAMES = ["420_33x33", "422_33x33", "444_17x15", "gray", "l12_16x17", "l41_15x9", "rgb_coded"]


def l24(rgb: np.ndarray) -> np.ndarray:
    a = rgb.astype(np.int64)
    return ((a[..., 0] * 19595 + a[..., 1] * 38470 + a[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


@pytest.mark.parametrize("name", NAMES)
def test_l_is_l24_of_the_turbo_rgb_and_y_is_plane_0(name):
    data = tc.case(name)
    rgb = ref.rgb_u8(data)
    np.testing.assert_array_equal(l24(rgb), np.asarray(Image.open(io.BytesIO(data)).convert("L")),
                                  strict=True)
    im = Image.open(io.BytesIO(data))
    im.draft("L", im.size)
    info = O.parse(data)
    # (an RGB-coded frame has no luma plane: libjpeg's rgb_gray_convert is L24)
    want = l24(rgb) if info.color == ref.COLOR_RGB else \
        O.decode_planes(data, O.IDCT_ISLOW)[0][:info.height, :info.width]
    np.testing.assert_array_equal(np.asarray(im), want, strict=True)


@pytest.mark.parametrize("fmt", ["L", "Y"])
def test_python_refusals_come_before_any_read(fmt):
    unread = ["/nonexistent/a.jpg"]
    with pytest.raises(ValueError, match="needs csc='turbo'"):
        sio.load_image_batch(unread, width=None, height=None, pix_fmt=fmt)
    with pytest.raises(ValueError, match="needs csc='turbo'"):
        sio.load_image(unread[0], pix_fmt=fmt)
    with pytest.raises(ValueError, match="needs csc='turbo'"):
        sio.load_image_list(unread, pix_fmt=fmt)
    with pytest.raises(ValueError, match="needs csc='turbo'"):  # (a format node of the caller's chain)
        sio.load_image_batch(unread, width=None, height=None, filter_desc=f"format=pix_fmts={fmt}")
    with pytest.raises(RuntimeError, match="Unexpected pix_fmt"):
        sio.decode_image_nvjpeg(b"", device_config=object(), pix_fmt=fmt)


def test_formats_in_the_spec():
    assert Output(pix_fmt="L").to_c().pix_fmt == 5 and Output(pix_fmt="Y").to_c().pix_fmt == 6
    assert Output(pix_fmt="L").channels == 1 and Output(pix_fmt="rgb24").channels == 3
    infos = [_lib.get_image_info(tc.case(n)) for n in ("420_33x33", "gray")]
    offs, sizes, st = _lib.ragged_layout(infos, Output(pix_fmt="Y", csc="turbo"), align=1)
    assert offs == [0, 33 * 33, 33 * 33 + 35 * 21] and st == [0, 0]
    with pytest.raises(ValueError):  # (a one-channel box of csc = swscale: no such output)
        _lib.ragged_layout(infos, Output(pix_fmt="Y"), align=1)
