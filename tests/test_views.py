"""CPU tests of views (include/spdl_hipjpeg.h "views"): the declarations and
their binding, what the Python layer refuses before any library call, and the
host arithmetic of hj_views.h swept under sanitizers by a stand-alone program.
"""

import ctypes
import os
import re
import shutil
import subprocess

import pytest

import spdl_amd.io as sio
from spdl_amd import _lib
from spdl_amd._lib import Output, ViewGroup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 8


def _header() -> str:
    with open(os.path.join(ROOT, "include", "spdl_hipjpeg.h")) as f:
        return f.read()


# ---- header and bindings -----------------------------------------------------------

def test_header_declares_views():
    h = _header()
    assert "#define SPDL_HJ_ABI_VERSION 7" in h  # additive: the version stays
    flat = re.sub(r"/\*.*?\*/", " ", h, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert "typedef struct { int32_t image; spdl_hj_rect rect; } spdl_hj_view;" in flat
    assert ("typedef struct { spdl_hj_output out; void* out_dev; size_t out_bytes; "
            "const spdl_hj_view* views; int32_t nviews; int32_t* status; } spdl_hj_view_group;") \
        in flat
    assert ("int spdl_hj_set_views(spdl_hj_ctx* ctx, const spdl_hj_view_group* groups, "
            "int32_t ngroups);") in flat


def test_header_states_the_contract():
    h = re.sub(r"\s*\n \*\s*", " ", _header())
    block = h[h.index("---- views"):h.index("} spdl_hj_view;")]
    for phrase in ("consumes the views, whether or not it succeeds",
                   "groups == NULL or ngroups == 0 clears them",
                   "ngroups is 1..4 and nviews at least 1",
                   "SPDL_HJ_ERR_INVALID_ARG and writes nothing",
                   "follows the source-crop rules exactly",
                   "one swscale context per view",
                   "[nviews, ...] in view order",
                   "out_dev must be NULL and out_bytes 0",
                   "every group's out.idct must equal it",
                   "SPDL_HJ_FMT_YUV or csc = JFIF in a group gives SPDL_HJ_ERR_INVALID_ARG",
                   "Its bytes stay untouched",
                   "both 0",
                   "ONE entropy workgroup"):
        assert phrase in block, phrase
    assert '"entropy_workgroups"' in h


def test_binding_and_struct_layout():
    L = _lib.lib()
    assert "spdl_hj_set_views" in _lib.EXPORTED and hasattr(L, "spdl_hj_set_views")
    assert _lib.ABI_VERSION == 7 and L.spdl_hj_abi_version() == 7
    # spdl_hj_view: int32 + spdl_hj_rect; spdl_hj_view_group: the 76-byte output
    # spec, padded to the pointer that follows, three pointers, a size and a count
    assert ctypes.sizeof(_lib.View) == 20 and _lib.View.rect.offset == 4
    assert ctypes.sizeof(_lib.OutputSpec) == 76
    G = _lib.ViewGroupSpec
    assert (G.out_dev.offset, G.out_bytes.offset, G.views.offset, G.nviews.offset,
            G.status.offset, ctypes.sizeof(G)) == (80, 88, 96, 104, 112, 120)


def test_set_views_without_a_context_is_invalid_arg():
    L = _lib.lib()
    g = ViewGroup(Output(pix_fmt="rgb24"), [(0, None)], 0, 0)
    arr = (_lib.ViewGroupSpec * 1)(g.to_c())
    assert L.spdl_hj_set_views(None, arr, 1) == INVALID_ARG
    assert L.spdl_hj_set_views(None, None, 0) == INVALID_ARG


def test_view_group_marshals_its_views():
    g = ViewGroup(Output(pix_fmt="rgb", resize=True, fit_w=8, fit_h=8),
                  [(2, (1, 2, 3, 4)), (0, None), (1, (None, 5, 6, 7))], 4096, 3 * 192)
    c = g.to_c()
    assert (c.nviews, c.out_dev, c.out_bytes, c.out.fit_w) == (3, 4096, 576, 8)
    got = [(c.views[k].image, c.views[k].rect.x, c.views[k].rect.y, c.views[k].rect.w,
            c.views[k].rect.h) for k in range(3)]
    assert got == [(2, 1, 2, 3, 4), (0, 0, 0, 0, 0), (1, _lib.CROP_CENTER, 5, 6, 7)]
    assert g.statuses == [0, 0, 0]


# ---- what Python refuses with no GPU -----------------------------------------------

class _NoLibrary:
    """A Decoder whose native handle must never be used."""

    _h = None
    set_views = _lib.Decoder.set_views
    set_crops = _lib.Decoder.set_crops
    _crops = _lib.Decoder._crops
    decode_batch = _lib.Decoder.decode_batch
    decode_batch_device = _lib.Decoder.decode_batch_device
    decode_staged = _lib.Decoder.decode_staged


def _group():
    return ViewGroup(Output(pix_fmt="rgb24"), [(0, (1, 2, 30, 40))], 4096, 30 * 40 * 3)


def test_views_with_crops_raise():
    d = _NoLibrary()
    with pytest.raises(ValueError, match="views= and crops= are exclusive"):
        d.decode_batch([b"x"], Output(), 0, 0, views=[_group()], crops=[(1, 2, 3, 4)])
    with pytest.raises(ValueError, match="views= and crops= are exclusive"):
        d.decode_batch_device(0, 0, [0], [1], [], Output(), 0, 0, views=[_group()],
                              crops=[(1, 2, 3, 4)])
    with pytest.raises(ValueError, match="views= and crops= are exclusive"):
        d.decode_staged(1, 1, [0], [1], Output(), 0, 0, views=[_group()], crops=[None])


def test_views_with_a_source_crop_in_the_output_raise():
    d = _NoLibrary()
    with pytest.raises(ValueError, match="Output.src_crop"):
        d.decode_batch([b"x"], Output(src_crop=(1, 2, 3, 4)), 0, 0, views=[_group()])
    with pytest.raises(ValueError, match="Output.src_crop"):
        ViewGroup(Output(src_crop=(1, 2, 3, 4)), [(0, None)], 4096, 64)


def test_views_take_no_output_pointer_of_the_call():
    with pytest.raises(ValueError, match="out_ptr and out_bytes must be 0"):
        _NoLibrary().decode_batch([b"x"], Output(), 4096, 64, views=[_group()])


@pytest.mark.parametrize("views", [
    [(0, (1, 2, 3, 4))],          # views, not groups
    [[(0, (1, 2, 3, 4))]],
    "group",
])
def test_wrong_nesting_of_groups_raises(views):
    with pytest.raises(ValueError, match="sequence of ViewGroup"):
        _NoLibrary().decode_batch([b"x"], Output(), 0, 0, views=views)


def test_a_single_group_is_no_sequence_of_groups():
    with pytest.raises(ValueError, match="sequence of ViewGroup"):
        _NoLibrary().decode_batch([b"x"], Output(), 0, 0, views=_group())


@pytest.mark.parametrize("views", [[0, 1], [(0,)], [((1, 2, 3, 4), 0)], [(0, (1, 2, 3, 4), 5)]])
def test_wrong_nesting_of_views_raises(views):
    with pytest.raises(ValueError, match=r"a view is \(image, rect_or_None\)"):
        ViewGroup(Output(pix_fmt="rgb24"), views, 4096, 64)


@pytest.mark.parametrize("rect", [(1, 2, 3), (1, 2, 3, 4, 5), 7, ()])
def test_rect_of_the_wrong_length_raises(rect):
    with pytest.raises(ValueError, match=r"a view's rect is \(x, y, w, h\) or None"):
        ViewGroup(Output(pix_fmt="rgb24"), [(0, rect)], 4096, 64)


def test_load_image_views_validates_its_groups():
    cfg = sio.cuda_config(device_index=0)
    ok = dict(width=64, height=64, crops=[[(1, 2, 30, 40)]])
    with pytest.raises(ValueError, match="unknown group keys \\['filter_desc'\\]"):
        sio.load_image_views([b"x"], [dict(ok, filter_desc="scale=8:8")], device_config=cfg)
    with pytest.raises(ValueError, match="needs crops="):
        sio.load_image_views([b"x"], [dict(width=64, height=64)], device_config=cfg)
    with pytest.raises(ValueError, match="2 crop lists for 1 images"):
        sio.load_image_views([b"x"], [dict(ok, crops=[[None], [None]])], device_config=cfg)
    with pytest.raises(ValueError, match="a view's rect is"):
        sio.load_image_views([b"x"], [dict(ok, crops=[[(1, 2, 3)]])], device_config=cfg)
    with pytest.raises(ValueError, match="list of rectangles per image"):
        sio.load_image_views([b"x"], [dict(ok, crops=[5])], device_config=cfg)
    with pytest.raises(ValueError, match="1 to 4 groups"):
        sio.load_image_views([b"x"], [ok] * 5, device_config=cfg)
    with pytest.raises(ValueError, match="pix_fmt is rgb, bgr, rgb24 or bgr24"):
        sio.load_image_views([b"x"], [dict(ok, pix_fmt=None)], device_config=cfg)
    with pytest.raises(ValueError, match="mapping"):
        sio.load_image_views([b"x"], [[(1, 2, 30, 40)]], device_config=cfg)


# ---- the host arithmetic, swept ----------------------------------------------------

def test_views_arithmetic_sweep_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    # (runtimes linked statically: the program then runs whatever the environment preloads)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-static-libubsan"]
    probe_src = tmp_path / "probe.cpp"
    probe_src.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, *san, str(probe_src), "-o", str(tmp_path / "probe")],
                      capture_output=True).returncode:
        pytest.skip("the compiler has no sanitizer runtime")
    exe = str(tmp_path / "views_sweep")
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-DHJ_HD=", *san,
                    os.path.join(ROOT, "tests", "native", "views_sweep.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("sets ") and not r.stderr, r.stdout + r.stderr
    sets, checks = (int(r.stdout.split()[i]) for i in (1, 3))
    # 400 frames (5 formats, 20 grids, 4 edge variants), 25 rectangles each:
    # the empty set and C(25, 1) + C(25, 2) + C(25, 3) = 2625 more
    assert sets == 400 * 2626 and checks > 5 * sets
    # frames with a side of 32768, 65500 and 65535 (5 formats, 3 x 3 sizes, both ways): 16
    # origins x 7 sizes x 2 extents at the far end, each in sets of 1, 2 and 3
    far = r.stdout.splitlines()[1].split()
    assert far[:2] == ["far-end", "sets"] and int(far[2]) == 5 * 18 * 16 * 7 * 2 * 3
    assert int(far[4]) > 5 * int(far[2])


def test_sweep_includes_only_the_two_host_headers():
    with open(os.path.join(ROOT, "tests", "native", "views_sweep.cpp")) as f:
        inc = re.findall(r'#include "([^"]+)"', f.read())
    assert sorted(os.path.basename(i) for i in inc) == ["hj_common.h", "hj_views.h"]
    with open(os.path.join(ROOT, "spdl_amd", "csrc", "hj_views.h")) as f:
        text = f.read()
    assert "hip" not in "".join(re.findall(r"#include.*", text)).lower()
