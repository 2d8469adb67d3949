"""GPU tests of views (spdl_hj_set_views; -m gpu): several rectangles and sizes
of one image from one entropy decode, grouped by output chain.  Through the
C-ABI (``Decoder``) and ``load_image_views``; every comparison is bit-exact
against ``tests/src_crop_ref.py`` (a view is a source crop that shares its
image's decode).  Every group's buffer is pre-filled with 0xA5 and has a 0xA5
tail, so "untouched" and "wrote past the end" are both checkable.
"""

import ctypes

import numpy as np
import pytest
import torch

import spdl_amd.io as sio
from spdl_amd import _lib
from spdl_amd._lib import Output, ViewGroup
from tests import cases, jpeg_writer_cases
from tests import src_crop_ref as ref

pytestmark = pytest.mark.gpu

BAD_GEOMETRY, INVALID_ARG = 7, 8
GUARD = 0xA5
PAD64 = dict(resize=True, fit_w=64, fit_h=64, aspect="decrease", pad_w=64, pad_h=64)
CROP32 = dict(resize=True, fit_w=32, fit_h=32, aspect="increase", crop_w=32, crop_h=32)
CALL = Output(pix_fmt="rgb24")  # the consuming call's own spec: only its idct counts


def _rs(oracle, spec):
    return oracle.Resize(**{k: v for k, v in spec.items() if k != "resize"})


def _data(name):
    return jpeg_writer_cases.case(name).data if name.startswith("samp_") else cases.case(name)


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


class Bufs:
    """Guarded device buffers of a submission's groups: (out, views, shape) per
    group -> ViewGroups whose buffers are 0xA5 bytes with one more view of 0xA5
    behind them."""

    def __init__(self, specs):
        self.specs, self.t, self.groups = specs, [], []
        for out, views, shape in specs:
            esz = 1 if out.torch_dtype == torch.uint8 else 2
            per = int(np.prod(shape)) * esz
            t = torch.full(((len(views) + 1) * max(per, 16),), GUARD, dtype=torch.uint8,
                           device="cuda:0")
            self.t.append(t)
            self.groups.append(ViewGroup(out, views, t.data_ptr(), len(views) * per))

    def host(self):
        """[nviews, *shape] per group (16-bit outputs as their bit patterns);
        asserts the tails."""
        res = []
        for (out, views, shape), t in zip(self.specs, self.t):
            esz = 1 if out.torch_dtype == torch.uint8 else 2
            per = int(np.prod(shape)) * esz
            a = t.cpu().numpy()
            assert (a[len(views) * per:] == GUARD).all(), "wrote past a group's output"
            body = a[: len(views) * per]
            if esz == 2:
                body = body.view(np.uint16)
            res.append(body.reshape(len(views), *shape))
        return res

    def untouched(self):
        return all(bool((t == GUARD).all()) for t in self.t)


def _want(oracle, datas, out, spec, views, idct=None):
    """The reference rows of one group (None for a rectangle that does not resolve)."""
    rs = _rs(oracle, spec) if spec else None
    rows = []
    for image, rect in views:
        r = ref.resolve_data(datas[image], rect or (0, 0, 0, 0))
        if r is None:
            rows.append(None)
            continue
        kw = {} if idct is None else {"idct": idct}
        w = ref.rgb(datas[image], r, rs, out.pix_fmt, normalize=out.normalize,
                    norm_dtype=out.norm_dtype, **kw)
        rows.append(w.view(np.uint16) if out.normalize else w)
    return rows


def _shape(out, w, h):
    return (3, h, w) if out.planar else (h, w, 3)


def _check_rows(got, want, what=""):
    for k, w in enumerate(want):
        if w is None:
            assert (got[k].view(np.uint8) == GUARD).all(), f"{what} view {k} was written"
        else:
            np.testing.assert_array_equal(got[k], w, strict=True, err_msg=f"{what} view {k}")


def _run(decoder, oracle, datas, groups, **kw):
    """groups: (Output, chain spec or None, [(image, rect)], (w, h)).  One
    decode_batch; every row against the reference.  Returns the Bufs."""
    b = Bufs([(o, v, _shape(o, *wh)) for o, _, v, wh in groups])
    st = decoder.decode_batch(datas, kw.pop("call", CALL), 0, 0, views=b.groups, **kw)
    assert st == [0] * len(datas)
    for gi, ((o, spec, v, _), got) in enumerate(zip(groups, b.host())):
        assert b.groups[gi].statuses == [0] * len(v)
        idct = oracle.IDCT_ISLOW if o.idct == "islow" else None
        _check_rows(got, _want(oracle, datas, o, spec, v, idct), f"group {gi}")
    return b


# ---- 1: one image, one group, overlapping views -----------------------------------

OVERLAP = [(38, 22, 112, 112), (300, 200, 64, 64), (30, 30, 120, 100)]


@pytest.mark.parametrize("pix_fmt", ["rgb24", "rgb"])
def test_overlapping_views_of_one_image(decoder, oracle, pix_fmt):
    """q90_420 is 4:2:0, 16 x 16 MCUs, 6 blocks each, 40 x 30 of them.  The
    views touch MCUs x 2..9 y 1..8, x 18..22 y 12..16 and -- its origin (30, 30)
    lies in MCU column 30 / 16 = 1 -- x 1..9 y 1..8: the bounding rectangle is
    x 1..22, y 1..16, 22 x 16 = 352 MCUs, 2112 blocks, ceil(2112 / 256) = 9 IDCT
    workgroups.  (With the third view from x = 32 the rectangle is x 2..22, 336
    MCUs, 2016 blocks: 8 workgroups, the next test.)"""
    d = cases.case("q90_420")
    out = Output(pix_fmt=pix_fmt, **PAD64)
    _run(decoder, oracle, [d], [(out, PAD64, [(0, r) for r in OVERLAP], (64, 64))])
    assert decoder.get_param("entropy_workgroups") == 1
    assert decoder.get_param("idct_workgroups") == 9
    # one more view, the whole frame: the whole grid, 7200 blocks
    _run(decoder, oracle, [d], [(out, PAD64, [(0, r) for r in OVERLAP] + [(0, (0, 0, 0, 0))],
                                 (64, 64))])
    assert decoder.get_param("idct_workgroups") == 29
    assert decoder.get_param("entropy_workgroups") == 1


def test_bounding_rectangle_of_mcu_columns_2_to_22(decoder, oracle):
    """The bounding MCUs x 2..22, y 1..16: 336 MCUs, 2016 blocks, 8 workgroups."""
    d = cases.case("q90_420")
    out = Output(pix_fmt="rgb24", **PAD64)
    views = [(0, (38, 22, 112, 112)), (0, (300, 200, 64, 64)), (0, (32, 30, 120, 100))]
    _run(decoder, oracle, [d], [(out, PAD64, views, (64, 64))])
    assert decoder.get_param("entropy_workgroups") == 1
    assert decoder.get_param("idct_workgroups") == 8


# ---- 2: one view per image is the crop path ---------------------------------------

@pytest.mark.parametrize("filt", ["bicubic", "bilinear", "lanczos"])
def test_one_view_per_image_is_the_crop_path(decoder, filt):
    datas = [cases.case(n) for n in ("q90_444", "odd_227x333", "gray")]
    rects = [(3, 5, 64, 48), (301, 195, 32, 32), (17, 9, 136, 128)]
    out = Output(pix_fmt="rgb24", filter=filt, **PAD64)
    b = Bufs([(out, list(enumerate(rects)), (64, 64, 3))])
    assert decoder.decode_batch(datas, CALL, 0, 0, views=b.groups) == [0, 0, 0]
    t = torch.full((4, 64, 64, 3), GUARD, dtype=torch.uint8, device="cuda:0")
    assert decoder.decode_batch(datas, out, t.data_ptr(), 3 * 64 * 64 * 3, crops=rects) == [0] * 3
    np.testing.assert_array_equal(b.host()[0], t.cpu().numpy()[:3], strict=True)


# ---- 3: two groups, uneven fan-out, mixed frame formats ---------------------------

MIX = ["q90_444", "odd_227x333", "gray", "q90_422"]
MIX_G0 = [(0, (3, 5, 64, 48)), (1, (301, 195, 32, 32)), (0, (17, 9, 200, 150)),
          (3, (11, 13, 51, 37))]
MIX_G1 = [(2, (17, 9, 136, 128)), (1, (40, 30, 100, 90)), (0, (100, 60, 80, 64)),
          (1, (0, 0, 0, 0)), (2, (150, 100, 77, 55)), (1, (200, 101, 96, 71))]


@pytest.mark.parametrize("norm_dtype", ["float16", "bfloat16"])
def test_two_groups_uneven_fanout(decoder, oracle, norm_dtype):
    datas = [cases.case(n) for n in MIX]
    g0 = Output(pix_fmt="rgb24", **PAD64)
    g1 = Output(pix_fmt="rgb", normalize=True, norm_dtype=norm_dtype, **CROP32)
    _run(decoder, oracle, datas, [(g0, PAD64, MIX_G0, (64, 64)), (g1, CROP32, MIX_G1, (32, 32))])
    assert decoder.get_param("entropy_workgroups") == 4


# ---- 4: pre-pass and no pre-pass in one group -------------------------------------

@pytest.mark.parametrize("prepass", [-1, 0, 1])
def test_prepass_and_no_prepass_in_one_group(decoder, oracle, knobs, prepass):
    knobs("sws_prepass", prepass)
    spec = dict(resize=True, fit_w=64, fit_h=64)
    out = Output(pix_fmt="rgb24", **spec)
    if prepass == -1:
        plan = _lib.debug_sws_plan(512, 384, 1, 1, "yuv", out)
        assert plan["rc"] == 0 and plan["pre"] == 1  # the first view runs hscale_kernel
        plan = _lib.debug_sws_plan(96, 96, 1, 1, "yuv", out)
        assert plan["rc"] == 0 and plan["pre"] == 0
    views = [(0, (0, 0, 512, 384)), (0, (100, 100, 96, 96))]
    _run(decoder, oracle, [cases.case("q90_420")], [(out, spec, views, (64, 64))])


# ---- 5: scan structures and colour models -----------------------------------------

STRUCTS = [
    ("prog_420", (33, 41, 150, 101), (7, 3, 90, 200)),
    ("multiscan_422_rst", (21, 10, 99, 77), (101, 33, 64, 50)),
    ("restart_blocks", (101, 57, 120, 90), (3, 150, 301, 71)),
    ("cmyk_adobe", (13, 7, 90, 71), (77, 41, 50, 60)),
    ("rgb_coded", (7, 9, 101, 63), (55, 31, 80, 60)),
    ("samp_411_70x29_ri0", (9, 3, 41, 20), (21, 5, 30, 17)),
    ("samp_410_70x29_ri0", (13, 5, 45, 19), (3, 9, 50, 15)),
]


@pytest.mark.parametrize("name,r0,r1", STRUCTS)
def test_scan_structures_and_colour_models(decoder, oracle, name, r0, r1):
    d = _data(name)
    for pix_fmt in ("rgb24", "rgb"):
        out = Output(pix_fmt=pix_fmt, **PAD64)
        _run(decoder, oracle, [d], [(out, PAD64, [(0, r0), (0, r1)], (64, 64))])


def test_progressive_and_baseline_in_one_batch(decoder, oracle):
    """The multi-scan side stream joins before the first group's output."""
    datas = [cases.case("prog_420"), cases.case("q90_444")]
    g0 = Output(pix_fmt="rgb24", **PAD64)
    g1 = Output(pix_fmt="rgb", **CROP32)
    _run(decoder, oracle, datas,
         [(g0, PAD64, [(1, (3, 5, 64, 48)), (0, (33, 41, 150, 101))], (64, 64)),
          (g1, CROP32, [(0, (7, 3, 90, 200)), (1, (100, 60, 80, 64)), (0, (0, 0, 0, 0))],
           (32, 32))])
    assert decoder.get_param("entropy_workgroups") == 2


# ---- 6: full resolution -----------------------------------------------------------

def test_full_resolution_views(decoder, oracle):
    datas = [cases.case("q90_420"), cases.case("odd_227x333")]
    out = Output(pix_fmt="rgb24")
    views = [(0, (38, 22, 112, 96)), (1, (301, 195, 112, 96)), (0, (301, 195, 112, 96))]
    _run(decoder, oracle, datas, [(out, None, views, (112, 96))])
    b = Bufs([(out, [(0, (38, 22, 112, 96)), (1, (0, 0, 112, 112))], (96, 112, 3))])
    with pytest.raises(RuntimeError, match="same output size"):
        decoder.decode_batch(datas, CALL, 0, 0, views=b.groups)
    assert b.untouched()


# ---- 7: refusals ------------------------------------------------------------------

def test_refused_view_leaves_its_row_alone(decoder, oracle):
    datas = [cases.case("q90_444"), cases.case("gray")]
    out = Output(pix_fmt="rgb24", **PAD64)
    views = [(0, (3, 5, 64, 48)), (0, (0, 0, 9999, 10)), (1, (17, 9, 136, 128)),
             (0, (100, 60, 80, 64))]
    b = Bufs([(out, views, (64, 64, 3))])
    st = decoder.decode_batch(datas, CALL, 0, 0, views=b.groups, check=False)
    assert st == [0, 0]
    assert b.groups[0].statuses == [0, BAD_GEOMETRY, 0, 0]
    want = _want(oracle, datas, out, PAD64, views)
    assert want[1] is None
    _check_rows(b.host()[0], want)
    # a synchronous call that checks fails, as the crop path does for a refused image
    b = Bufs([(out, views, (64, 64, 3))])
    with pytest.raises(RuntimeError, match="group 0, view 1"):
        decoder.decode_batch(datas, CALL, 0, 0, views=b.groups)


def test_failed_image_leaves_its_views_alone(decoder, oracle):
    good, cut = cases.case("q90_420"), cases.truncated()
    datas = [good, cut, cases.case("q90_444")]
    t = torch.zeros(3 * 64 * 64 * 3, dtype=torch.uint8, device="cuda:0")
    out = Output(pix_fmt="rgb24", **PAD64)
    today = decoder.decode_batch(datas, out, t.data_ptr(), t.numel(), check=False)
    assert today[0] == 0 and today[1] != 0 and today[2] == 0
    views = [(1, (38, 22, 112, 112)), (0, (38, 22, 112, 112)), (2, (3, 5, 64, 48)),
             (1, (0, 0, 0, 0)), (0, (300, 200, 64, 64))]
    b = Bufs([(out, views, (64, 64, 3))])
    st = decoder.decode_batch(datas, CALL, 0, 0, views=b.groups, check=False)
    assert st == today
    assert b.groups[0].statuses == [0] * 5
    want = _want(oracle, [good, good, datas[2]], out, PAD64, views)
    want[0] = want[3] = None
    _check_rows(b.host()[0], want)


def _plain_decode_is_normal(decoder, oracle):
    d = cases.case("q90_444")
    out = Output(pix_fmt="rgb24", **PAD64)
    t = torch.zeros(64 * 64 * 3, dtype=torch.uint8, device="cuda:0")
    assert decoder.decode_batch([d], out, t.data_ptr(), t.numel()) == [0]
    np.testing.assert_array_equal(t.cpu().numpy().reshape(64, 64, 3),
                                  oracle.decode_resize(d, _rs(oracle, PAD64), "rgb24"), strict=True)


@pytest.mark.parametrize("what", ["image_n", "image_neg", "five_groups", "no_views", "yuv_group",
                                  "jfif_group", "idct_differs", "call_out_dev", "with_crops"])
def test_broken_limits_are_invalid_arg_and_consume_the_views(decoder, oracle, what):
    datas = [cases.case("q90_444"), cases.case("gray")]
    out = Output(pix_fmt="rgb24", **PAD64)
    ok = [(0, (3, 5, 64, 48)), (1, (17, 9, 136, 128))]
    specs = [(out, ok, (64, 64, 3))]
    call, crops = CALL, None
    if what == "image_n":
        specs = [(out, ok + [(2, None)], (64, 64, 3))]
    elif what == "image_neg":
        specs = [(out, [(-1, None)] + ok, (64, 64, 3))]
    elif what == "five_groups":
        specs = specs * 5
    elif what == "no_views":
        specs = specs + [(out, [], (64, 64, 3))]
    elif what == "yuv_group":
        specs = specs + [(Output(pix_fmt="yuv", **PAD64), ok, (64, 64, 3))]
    elif what == "jfif_group":
        specs = specs + [(Output(pix_fmt="rgb24", csc="jfif"), ok, (240, 320, 3))]
    elif what == "idct_differs":
        specs = specs + [(Output(pix_fmt="rgb24", idct="islow", **PAD64), ok, (64, 64, 3))]
    b = Bufs(specs)
    extra = torch.full((64,), GUARD, dtype=torch.uint8, device="cuda:0")
    decoder.set_views(b.groups)
    if what == "with_crops":
        decoder.set_crops([(3, 5, 64, 48), None])
    status = (ctypes.c_int32 * 2)(-1, -1)
    err = ctypes.create_string_buffer(512)
    keep = [_lib.buffer_address(d) for d in datas]
    ptrs = (ctypes.c_void_p * 2)(*[k[0] for k in keep])
    sizes = (ctypes.c_size_t * 2)(*[k[1] for k in keep])
    spec = call.to_c()
    out_ptr, out_bytes = (extra.data_ptr(), 64) if what == "call_out_dev" else (None, 0)
    rc = _lib.lib().spdl_hj_decode_batch(decoder._h, ptrs, sizes, 2, ctypes.byref(spec), out_ptr,
                                         out_bytes, None, 1, status, err, 512)
    assert rc == INVALID_ARG, err.value
    assert b.untouched() and bool((extra == GUARD).all())
    assert all(g.statuses == [0] * len(g.views) for g in b.groups)
    # the views (and the crops) were consumed: a plain batch decodes as ever
    _plain_decode_is_normal(decoder, oracle)


# ---- 8: entry points and lanes ----------------------------------------------------

def _two_groups():
    g0 = Output(pix_fmt="rgb24", **PAD64)
    g1 = Output(pix_fmt="rgb", normalize=True, **CROP32)
    return [(g0, PAD64, MIX_G0, (64, 64)), (g1, CROP32, MIX_G1, (32, 32))]


def _packed(datas):
    offs, total = [], 0
    for d in datas:
        offs.append(total)
        total += (len(d) + 64 + 255) // 256 * 256
    host = np.zeros(total + 512, np.uint8)
    for o, d in zip(offs, datas):
        host[o:o + len(d)] = np.frombuffer(d, np.uint8)
    return host, offs, [len(d) for d in datas], total


@pytest.fixture(scope="module")
def two_group_rows(oracle):
    datas = [cases.case(n) for n in MIX]
    return datas, [_want(oracle, datas, o, spec, v) for o, spec, v, _ in _two_groups()]


@pytest.mark.parametrize("entry", ["batch", "device", "staged"])
def test_entry_points(decoder, two_group_rows, entry):
    datas, want = two_group_rows
    groups = _two_groups()
    b = Bufs([(o, v, _shape(o, *wh)) for o, _, v, wh in groups])
    host, offs, sizes, total = _packed(datas)
    if entry == "batch":
        st = decoder.decode_batch(datas, CALL, 0, 0, views=b.groups)
    elif entry == "device":
        dev = torch.from_numpy(host).to("cuda:0")
        infos = [_lib.get_image_info(d) for d in datas]
        st = decoder.decode_batch_device(dev.data_ptr(), dev.numel(), offs, sizes, infos, CALL,
                                         0, 0, views=b.groups)
    else:
        ptr, ticket = decoder.staging_acquire(total)
        ctypes.memmove(ptr, host.ctypes.data, total)
        st = decoder.decode_staged(ticket, total, offs, sizes, CALL, 0, 0, views=b.groups)
    assert st == [0] * 4
    for gi, got in enumerate(b.host()):
        _check_rows(got, want[gi], f"{entry} group {gi}")
    assert decoder.get_param("entropy_workgroups") == 4


def test_async_submissions_on_two_lanes(decoder, two_group_rows, knobs):
    """Three submissions in flight with different views into different
    buffers: workspace reuse across lanes and the per-group launches."""
    knobs("lanes", 2)
    datas, want = two_group_rows
    groups = _two_groups()
    orders = [(0, 1), (1, 0), (0, 1)]  # the groups, swapped in the second submission
    subs = []
    for k, order in enumerate(orders):
        sel = [groups[g] for g in order]
        # (different views per submission: each drops another view of its first group)
        sel[0] = (sel[0][0], sel[0][1], [v for i, v in enumerate(sel[0][2]) if i != k], sel[0][3])
        b = Bufs([(o, v, _shape(o, *wh)) for o, _, v, wh in sel])
        decoder.decode_batch(datas, CALL, 0, 0, views=b.groups, sync=False)
        subs.append((decoder.last_ticket(), b, order, k))
    for ticket, b, order, k in subs:
        assert decoder.wait(ticket, 4) == [0] * 4
        for gi, got in enumerate(b.host()):
            w = want[order[gi]]
            if gi == 0:
                w = [r for i, r in enumerate(w) if i != k]
            _check_rows(got, w, f"ticket {ticket} group {gi}")


# ---- 9: a large file under views --------------------------------------------------

def test_large_file_is_one_entropy_workgroup(decoder, oracle, knobs):
    knobs("entropy_piece_bytes", 16384)
    d = cases.case("q90_420")
    assert len(d) > 2 * 16384
    out = Output(pix_fmt="rgb24", **PAD64)
    # (without views this file takes several pieces)
    t = torch.zeros(64 * 64 * 3, dtype=torch.uint8, device="cuda:0")
    decoder.decode_batch([d], out, t.data_ptr(), t.numel())
    assert decoder.get_param("entropy_workgroups") == -(-len(d) // 16384) > 1
    before = decoder.get_param("handoff_retries")
    _run(decoder, oracle, [d], [(out, PAD64, [(0, (38, 22, 112, 112)), (0, (300, 200, 64, 64))],
                                 (64, 64))])
    assert decoder.get_param("entropy_workgroups") == 1
    assert decoder.get_param("handoff_retries") == before


# ---- 10: islow --------------------------------------------------------------------

def test_islow_group(decoder, oracle):
    d = cases.case("q90_444")
    out = Output(pix_fmt="rgb24", idct="islow", **PAD64)
    _run(decoder, oracle, [d], [(out, PAD64, [(0, (3, 5, 64, 48)), (0, (100, 60, 80, 64))],
                                 (64, 64))], call=Output(pix_fmt="rgb24", idct="islow"))


# ---- 11: the Python surface -------------------------------------------------------

def test_load_image_views(oracle):
    names = ["q90_420", "gray", "q90_444"]
    datas = [cases.case(n) for n in names]
    cfg = sio.cuda_config(device_index=0)
    c0 = [[(38, 22, 112, 112), (300, 200, 64, 64)], [], [(3, 5, 64, 48)]]
    c1 = [[None], [(17, 9, 136, 128), (150, 100, 77, 55)], [(100, 60, 80, 64)]]
    res = sio.load_image_views(
        datas, [dict(width=64, height=64, crops=c0),
                dict(width=32, height=32, scale_mode="crop", pix_fmt="rgb", normalize=True,
                     dtype="bfloat16", crops=c1)], device_config=cfg)
    (b0, i0), (b1, i1) = res
    t0, t1 = sio.to_torch(b0), sio.to_torch(b1)
    assert t0.shape == (3, 64, 64, 3) and t0.dtype == torch.uint8 and i0 == [0, 0, 2]
    assert t1.shape == (4, 3, 32, 32) and t1.dtype == torch.bfloat16 and i1 == [0, 1, 1, 2]
    g0, g1 = Output(pix_fmt="rgb24", **PAD64), Output(pix_fmt="rgb", normalize=True,
                                                     norm_dtype="bfloat16", **CROP32)
    v0 = [(i, r) for i, rs in enumerate(c0) for r in rs]
    v1 = [(i, r) for i, rs in enumerate(c1) for r in rs]
    _check_rows(t0.cpu().numpy(), _want(oracle, datas, g0, PAD64, v0))
    _check_rows(t1.cpu().view(torch.int16).numpy().view(np.uint16),
                _want(oracle, datas, g1, CROP32, v1))


def test_load_image_views_not_strict_drops_rows():
    good = cases.case("q90_444")
    datas = [good, cases.truncated(), cases.case("gray")]
    cfg = sio.cuda_config(device_index=0)
    crops = [[(3, 5, 64, 48), (0, 0, 9999, 10)], [(38, 22, 112, 112)], [(17, 9, 136, 128)]]
    with pytest.raises(RuntimeError):
        sio.load_image_views(datas, [dict(width=64, height=64, crops=crops)], device_config=cfg)
    [(buf, idx)] = sio.load_image_views(datas, [dict(width=64, height=64, crops=crops)],
                                        device_config=cfg, strict=False)
    assert idx == [0, 2] and sio.to_torch(buf).shape == (2, 64, 64, 3)
    [(alone, _)] = sio.load_image_views([good, datas[2]], [dict(
        width=64, height=64, crops=[[(3, 5, 64, 48)], [(17, 9, 136, 128)]])], device_config=cfg)
    assert torch.equal(sio.to_torch(buf), sio.to_torch(alone))
