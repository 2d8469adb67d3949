"""Oriented resample items without a GPU (include/spdl_hipjpeg.h "Pillow-exact
orientation"): the request's geometry on the displayed frame, what is refused
before a file is read, the items' statuses, and the tiler's stored rectangles."""

import os
import shutil
import subprocess
from types import SimpleNamespace

import pytest

import spdl_amd.io as sio
from spdl_amd import _lib
from spdl_amd.io import _image
from tests import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spdl_amd", "csrc")
BAD_GEOMETRY = 7
LANDSCAPE = [SimpleNamespace(width=640, height=480)]


@pytest.mark.parametrize("code,rsz,window", [(0, (341, 256), (58, 16, 224, 224)),
                                             (3, (341, 256), (58, 16, 224, 224)),
                                             (5, (256, 341), (16, 58, 224, 224))])
def test_shorter_side_is_the_displayed_frames(code, rsz, window):
    rs = sio.pil_resize((224, 224), shorter=256, orients=code)
    _, reqs, _ = _image._item_requests(rs, LANDSCAPE, [0], None, None, [code])
    assert reqs == [(0, None, True, rsz, window, 0, code)]


@pytest.mark.parametrize("code,size", [(0, (64, 48)), (6, (48, 64))])
def test_thumbnail_of_a_portrait_by_tag_file_takes_no_draft(code, size):
    """Unoriented, 640 x 480 into 64 x 64 at gap 2 drafts to 320 x 240; the
    transposed image is no JPEG file, so level 0 and the gap on the full frame."""
    thumb = sio.pil_thumbnail((64, 64), orients=code) if code else sio.pil_thumbnail((64, 64))
    levels, reqs, gap = _image._item_requests(thumb, LANDSCAPE, [0], None, None, [code])
    assert reqs[0][3] == size and reqs[0][6] == code and gap == 2.0
    assert levels == ([1] if not code else None)
    assert reqs[0][1] == ((0.0, 0.0, 320.0, 240.0) if not code else (0.0, 0.0, 480.0, 640.0))


@pytest.mark.parametrize("call", [
    lambda: sio.pil_resize((8, 8), exif_transpose=True, orients=5),
    lambda: sio.pil_thumbnail((8, 8), orients=8),
    lambda: sio.load_image("no.jpg", csc="turbo", pix_fmt="L",
                           resample=sio.pil_resize((8, 8), exif_transpose=True)),
    lambda: sio.load_image_list(["no.jpg"], csc="turbo", pix_fmt="Y",
                                resample=sio.pil_thumbnail((8, 8), orients=5)),
    lambda: sio.load_image_batch(["no.jpg", "no.jpg"], width=None, height=None, csc="turbo",
                                 resample=sio.pil_resize((8, 8), orients=[5])),
    lambda: sio.load_image_views(["no.jpg"], [dict(resample=sio.pil_resize((8, 8), orients=1),
                                                   boxes=[[None]])],
                                 csc="turbo", device_config=sio.cuda_config(device_index=0)),
], ids=["both", "code_8", "L", "Y", "count", "views"])
def test_refused_before_a_file_is_read(call):
    with pytest.raises(ValueError):
        call()


@pytest.mark.parametrize("code,status", [(0, BAD_GEOMETRY), (3, BAD_GEOMETRY), (5, 0), (6, 0)])
def test_a_clamped_box_is_held_against_the_displayed_frame(code, status):
    """480 x 640 fits the 640 x 480 file turned, not as stored"""
    infos = [_lib.get_image_info(cases.case("q90_420"))]
    items = _lib.ResampleItems("bilinear", [(0, (0, 0, 480, 640), True, (30, 40), (0, 0), (30, 40),
                                             0, 0, code)])
    assert _lib.resample_items_check(infos, items, 1, 30 * 40 * 3) == [status]


def test_a_code_above_7_fails_the_request():
    infos = [_lib.get_image_info(cases.case("q90_420"))]
    items = _lib.ResampleItems("bilinear", [(0, None, False, (30, 40), (0, 0), (30, 40), 0, 0, 8)])
    with pytest.raises(ValueError):
        _lib.resample_items_check(infos, items, 1, 30 * 40 * 3)


def test_stored_rectangles_sweep_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    # (runtimes linked statically: the program then runs whatever the environment preloads)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-static-libubsan"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, *san, str(probe), "-o", str(tmp_path / "probe")],
                      capture_output=True).returncode:
        pytest.skip("the compiler has no sanitizer runtime")
    exe = str(tmp_path / "items_orient_sweep")
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-DHJ_HD=", *san,
                    os.path.join(ROOT, "tests", "native", "items_orient_sweep.cpp"),
                    os.path.join(CSRC, "hj_resample.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
    last = r.stdout.splitlines()[-1]
    assert last.endswith(" 0 failed expectations") and int(last.split()[0]) >= 1000000, last
