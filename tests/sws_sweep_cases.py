"""The case table of the output-stage sweep: (source, resize spec, filter,
knobs), shared by the CPU plan tests (tests/test_sws_plan.py) and the GPU
sweep (tests/test_gpu_sws_sweep.py).

The output stage is sws_kernel, hscale_kernel and yuv_planes_kernel with the
host tiler (PlanCache::build).  Which of their data-dependent paths a decode
takes follows from the geometry alone, so the table is chosen with the plan
probe (spdl_hj_debug_sws_plan) and `census()` below says, per path, which
table entry takes it; test_sws_plan.py asserts that no path is left out.

Sources are a few KB each: seeded textures (as tests/cases.py makes its
images), the hand-written sampling streams, the committed RGB-coded and
4-component files, and two "edges" images whose 0 / 255 bars drive the
horizontal sums past the h15 cap and below zero.
"""

from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from spdl_amd import _lib
from spdl_amd._lib import Output
from spdl_amd.synthetic import synthetic_pixels
from tests import cases, jpeg_writer_cases

FILTERS = ("bicubic", "bilinear", "lanczos")
LDS_BUDGET = 32 * 1024  # hj_common.h kSwsLdsBudget

# ---- sources ------------------------------------------------------------------
# texture family: name -> (seed, w, h, Pillow subsampling; None = gray; "cmyk" =
# Pillow's Adobe CMYK, which decodes to three RGB planes), q92
TEXTURE = {
    "tex_420_400x24": (50, 400, 24, 2),
    "tex_gray_400x24": (51, 400, 24, None),
    "tex_422_776x16": (52, 776, 16, 1),
    "tex_gray_24x400": (53, 24, 400, None),
    "tex_444_64x400": (54, 64, 400, 0),
    "tex_420_272x40": (55, 272, 40, 2),
    "tex_422_137x91": (56, 137, 91, 1),
    "tex_444_64x48": (57, 64, 48, 0),
    "tex_420_64x48": (58, 64, 48, 2),
    "tex_gray_9x17": (59, 9, 17, None),
    "tex_420_3x2": (60, 3, 2, 2),
    "tex_444_3x2": (61, 3, 2, 0),
    "tex_cmyk_272x24": (62, 272, 24, "cmyk"),
    "tiny_1x1": None,  # tests/cases.py
}
HANDWRITTEN = {"hw_440": "samp_440_37x29_ri0", "hw_411": "samp_411_70x29_ri0",
               "hw_410": "samp_410_70x29_ri0", "hw_1x4": "samp_1x4_37x29_ri0"}
COMMITTED = ("rgb_coded", "rgb_coded_odd_rst", "cmyk_adobe", "ycck_adobe", "ycck_odd_rst")
# edges family: 112 x 64, q100; name -> Pillow subsampling (None = gray)
EDGES = {"edges_gray": None, "edges_444": 0, "edges_420": 2}
PRIMARIES = {"prim_444": 0, "prim_420": 2}
SOURCES = (*TEXTURE, *HANDWRITTEN, *COMMITTED, *EDGES, *PRIMARIES)


def edges_pixels(w: int = 112, h: int = 64) -> np.ndarray:
    """Bars two pixels on, two off, 0 / 255: vertical in the top half,
    horizontal in the bottom half."""
    y, x = np.mgrid[0:h, 0:w]
    on = np.where(y < h // 2, x % 4 < 2, y % 4 < 2)
    return (on * 255).astype(np.uint8)


def primaries_pixels(w: int = 112, h: int = 64) -> np.ndarray:
    """The same bars in saturated primaries and their complements: every
    two-pixel bar one of R, G, B, C, M, Y, black, white."""
    pal = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [0, 255, 255], [255, 0, 255],
                    [255, 255, 0], [0, 0, 0], [255, 255, 255]], np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    idx = np.where(y < h // 2, x // 2, y // 2 + 3) % 8
    return pal[idx]


@functools.lru_cache(maxsize=None)
def source(name: str) -> bytes:
    if name in TEXTURE:
        if TEXTURE[name] is None:
            return cases.case(name)
        seed, w, h, sub = TEXTURE[name]
        px = synthetic_pixels(seed, h, w)
        if sub is None:
            return cases._enc(px[..., 0], quality=92)
        if sub == "cmyk":
            return cases._cmyk_pillow(px, quality=92)
        return cases._enc(px, quality=92, subsampling=sub)
    if name in HANDWRITTEN:
        return jpeg_writer_cases.case(HANDWRITTEN[name]).data
    if name in COMMITTED:
        return cases.case(name)
    if name in EDGES:
        g = edges_pixels()
        if EDGES[name] is None:
            return cases._enc(g, quality=100)
        return cases._enc(np.repeat(g[..., None], 3, axis=2), quality=100, subsampling=EDGES[name])
    if name in PRIMARIES:
        return cases._enc(primaries_pixels(), quality=100, subsampling=PRIMARIES[name])
    raise KeyError(name)


Meta = namedtuple("Meta", "w h hsub vsub mode")


@functools.lru_cache(maxsize=None)
def meta(name: str) -> Meta:
    """Size, chroma shifts and plan mode of a source, from the host probe (the
    rule of build_layout: gray, RGB planes for RGB-coded and CMYK frames,
    YCbCr otherwise; 4-component frames are unsampled)."""
    i = _lib.get_image_info(source(name))
    hs = vs = 0
    if i.ncomp == 3:
        hs = (i.h_samp[0] // i.h_samp[1]).bit_length() - 1
        vs = (i.v_samp[0] // i.v_samp[1]).bit_length() - 1
    mode = "gray" if i.ncomp == 1 else "gbr" if i.color in (2, 3) else "yuv"
    return Meta(i.width, i.height, hs, vs, mode)


# ---- resize specs ---------------------------------------------------------------
SPECS = {
    "w8": dict(fit_w=8, fit_h=0),                 # stretch to 8 columns, height unchanged
    "h8": dict(fit_w=0, fit_h=8),                 # ... to 8 rows, width unchanged
    "w4": dict(fit_w=4, fit_h=0),                 # (272 -> 4: refused on RGB planes too)
    "up64x200": dict(fit_w=64, fit_h=200),        # rows upscaled (bilinear: Two on every writer)
    "w96": dict(fit_w=96, fit_h=0),               # width only (bilinear 4:2:0: One | ua rows)
    "w97": dict(fit_w=97, fit_h=0),               # ... to an odd width (full chroma)
    "odd51x37": dict(fit_w=51, fit_h=37),
    "pad57x41": dict(fit_w=51, fit_h=37, pad_w=57, pad_h=41),   # dx 3, dy 2
    "pad57x43": dict(fit_w=51, fit_h=37, pad_w=57, pad_h=43),   # dx 3, dy 3
    "crop33x21": dict(fit_w=51, fit_h=37, crop_w=33, crop_h=21),  # dx -9, dy -8
    "crop33x19": dict(fit_w=51, fit_h=37, crop_w=33, crop_h=19),  # dx -9, dy -9
    "fitpad48": dict(fit_w=48, fit_h=48, aspect="decrease", pad_w=48, pad_h=48),
    "fitcrop48": dict(fit_w=48, fit_h=48, aspect="increase", crop_w=48, crop_h=48),
    "pad300x70": dict(fit_w=40, fit_h=20, pad_w=300, pad_h=70),  # tiles wholly in the pad
    "wide598x10": dict(fit_w=598, fit_h=10),
    "up300x70": dict(fit_w=300, fit_h=70),
    "out1x1": dict(fit_w=1, fit_h=1),
    "out1x7": dict(fit_w=1, fit_h=7),
    "out9x1": dict(fit_w=9, fit_h=1),
}
# (prepass, max_cols) of "sws_prepass" / "sws_cols": default, forced pre-pass,
# pre-pass off; and the narrowest tile
KNOBS = ((-1, 256), (1, 256), (0, 256))
NARROW = (-1, 16)
NARROW_SPECS = ("wide598x10", "up300x70", "odd51x37")
# the same image eight times: one plan, the (band, chunk, image) grid
HOMOGENEOUS = ("tex_422_137x91", "fitpad48", "bicubic", 8)
# pix_fmt of a (spec, filter) cell beside rgb24: rotating
ROTATION = ("rgb", "bgr", "bgr24")
# normalised fp16 / bf16: a pad, >= 2 column chunks, an odd size
NORM_SPECS = ("pad57x43", "wide598x10", "odd51x37")


def output(spec: str, filt: str, **kw) -> Output:
    return Output(resize=True, filter=filt, **{"pix_fmt": "rgb24", **SPECS[spec], **kw})


def resize(O, spec: str, filt: str):
    return O.Resize(filter=filt, **SPECS[spec])


def probe(name: str, spec: str, filt: str, prepass: int = -1, max_cols: int = 256,
          pix_fmt: str = "rgb24") -> dict:
    m = meta(name)
    return _lib.debug_sws_plan(m.w, m.h, m.hsub, m.vsub, m.mode, output(spec, filt, pix_fmt=pix_fmt),
                               prepass, max_cols)


def oracle_plan(O, name: str, spec: str, filt: str):
    """(geometry, plan or None) of the oracle for a table cell."""
    m = meta(name)
    g = O.geometry(m.w, m.h, resize(O, spec, filt))
    return g, O.sws_plan(m.w, m.h, m.hsub, m.vsub, m.mode != "yuv", g["sw"], g["sh"], filt)


@functools.lru_cache(maxsize=None)
def _cells(spec: str, filt: str):
    from oracle import oracle as O

    ok, refused = {}, []
    for name in SOURCES:
        g, plan = oracle_plan(O, name, spec, filt)
        if plan is None:
            refused.append(name)
        else:
            ok.setdefault((g["ow"], g["oh"]), []).append(name)
    return ok, refused


def batches(spec: str, filt: str) -> list[list[str]]:
    """The sources the ORACLE accepts under (spec, filter), grouped by output
    size: each group is one decode_batch call.  Mixed plans make the flat
    grid; the homogeneous batch and single images the 3-D one."""
    out = [list(v) for v in _cells(spec, filt)[0].values()]
    if (spec, filt) == HOMOGENEOUS[1:3]:
        out.append([HOMOGENEOUS[0]] * HOMOGENEOUS[3])
    return out


def refused(spec: str, filt: str) -> list[str]:
    """The sources whose scale filter swscale refuses (256 taps or more)."""
    return list(_cells(spec, filt)[1])


def knobs(spec: str):
    return KNOBS + ((NARROW,) if spec in NARROW_SPECS else ())


# ---- the census -------------------------------------------------------------------
def _quad_bucket(taps: int) -> str:
    q = (taps + 3) // 4
    for hi, name in ((1, "1"), (2, "2"), (3, "3"), (4, "4"), (6, "5-6"), (8, "7-8"), (12, "9-12"),
                     (16, "13-16")):
        if q <= hi:
            return name
    return ">16"


def _taps_range(t: int) -> str:
    return "<=64" if t <= 64 else "65-128" if t <= 128 else "129-192" if t <= 192 else "193-255"


def plan_buckets(p: dict, mode: str, prepass: int, max_cols: int, index: int = 0) -> set[str]:
    """The census buckets one accepted packed plan (probe dict) falls in, as
    image `index` of an rgb24 batch whose buffer is 16-byte aligned."""
    b = set()
    hl, hc, vl, vc = p["hl"], p["hc"], p["vl"], p["vc"]
    if p["special"]:
        return {"special"}
    if not p["pre"]:
        if hl["taps"] <= 64:
            b.add("H-a luma quads " + _quad_bucket(hl["taps"]))
            if not p["gray"] and hc["stride"] != hl["stride"]:
                b.add("H-a chroma bucket differs from luma")
        else:
            b.add("H-b pre=0 over 64 taps")
    elif hl["taps"] <= 64:
        b.add("H-c pre=1 <=64 taps " + ("forced" if prepass == 1 else "auto"))
    else:
        b.add(f"H-d pre=1 {_taps_range(hl['taps'])} {mode}")
    writer = "gbr" if p["gbr"] else "gray" if p["gray"] else "full" if p["full"] else "table"
    vm = p["vmode"]
    for m, ua in {(int(v) & 15, bool((int(v) >> 17) & 8191)) for v in vm}:
        row = {0: "X", 1: "One", 2: "Two"}[m] + (" ua" if m == 1 and ua else "")
        b.add(f"V {row} {writer}")
    s = vl["stride"]
    b.add("V-size " + ("4" if s == 4 else "8-16" if s <= 16 else ">=200" if s >= 200 else
                       ">=64" if s >= 64 else "17-63"))
    if s >= 200:
        b.add("V-size >=64")
    if not p["gray"] and vl["stride"] != vc["stride"]:
        b.add("V-size vl != vc")
    rb, cc, ow, oh = p["rb"], p["col_chunk"], p["ow"], p["oh"]
    b.add("T-a rb " + ("32" if rb == 32 else "1" if rb == 1 else "2-24"))
    if 1 < rb < 32:
        b.add(f"T-a rb={rb}")
    if oh % rb:
        b.add("T-a short last band")
    if p["chunks"] >= 2 and ow % cc:
        b.add("T-b narrower last chunk")
    if cc < min(ow, max_cols):
        b.add("T-b col_chunk halved by the LDS budget")
    if max_cols == 16 and p["chunks"] >= 2:
        b.add("T-b sws_cols=16")
    if rb == 1 and p["lds"] > LDS_BUDGET:
        b.add("T-c one-row band over the budget")
    dx, dy, sw, sh = p["dx"], p["dy"], p["sw"], p["sh"]
    if dx > 0 and dx % 2 and dy > 0 and dy % 2:
        b.add("T-d odd dx and dy")
    if dx < 0 and dx % 2 and dy < 0 and dy % 2:
        b.add("T-d negative odd crop offsets")
    for y0 in range(0, oh, rb):
        y1 = min(y0 + rb, oh)
        rows = max(y0, dy) < min(y1, dy + sh)
        for x0 in range(0, ow, cc):
            x1 = min(x0 + cc, ow)
            cols = max(x0, dx) < min(x1, dx + sw)
            if not (rows and cols):
                b.add("T-d tile wholly in the pad")
                continue
            if x0 < dx:
                b.add("T-d tile straddles the left edge")
            if x1 > dx + sw:
                b.add("T-d tile straddles the right edge")
            if y0 < dy:
                b.add("T-d tile straddles the top edge")
            if y1 > dy + sh:
                b.add("T-d tile straddles the bottom edge")
            # sws_kernel's epilogue (rgb24): whole aligned rows leave as 16-byte stores
            off = (index * ow * oh + y0 * ow + x0) * 3
            run = (y1 - y0) * (x1 - x0) * 3
            wide = x1 - x0 == ow and off % 16 == 0 and run % 16 == 0
            b.add("T-e wide stores" if wide else "T-e byte stores")
    if index >= 1 and (index * ow * oh * 3) % 16:
        b.add("T-e image >= 1 at an unaligned offset")
    return b


def grid_bucket(plans: list[dict]) -> str:
    """Mirrors use_flat of hj_host.cpp for the sws grid: flat when (max bands x
    max chunks) x images exceeds 1.25 x the batch's own tiles."""
    tiles = sum(p["bands"] * p["chunks"] for p in plans)
    most = max(p["bands"] for p in plans) * max(p["chunks"] for p in plans)
    return "G flat grid" if most * len(plans) > 1.25 * tiles else "G 3-D grid"


REQUIRED = (
    *(f"H-a luma quads {q}" for q in ("1", "2", "3", "4", "5-6", "7-8", "9-12", "13-16")),
    "H-a chroma bucket differs from luma",
    "H-b pre=0 over 64 taps",
    "H-c pre=1 <=64 taps auto", "H-c pre=1 <=64 taps forced",
    *(f"H-d pre=1 {r} {m}" for r in ("65-128", "129-192", "193-255")
      for m in ("yuv", "gray", "gbr")),
    *(f"V {r} {w}" for w in ("table", "full") for r in ("One", "One ua", "Two", "X")),
    *(f"V {r} {w}" for w in ("gray", "gbr") for r in ("One", "Two", "X")),
    "V-size 4", "V-size 8-16", "V-size >=64", "V-size >=200", "V-size vl != vc",
    "T-a rb 32", "T-a rb 1", "T-a short last band",
    "T-b narrower last chunk", "T-b col_chunk halved by the LDS budget", "T-b sws_cols=16",
    "T-c one-row band over the budget",
    "T-d tile wholly in the pad", "T-d tile straddles the left edge",
    "T-d tile straddles the right edge", "T-d tile straddles the top edge",
    "T-d tile straddles the bottom edge", "T-d odd dx and dy", "T-d negative odd crop offsets",
    "T-e wide stores", "T-e byte stores", "T-e image >= 1 at an unaligned offset",
    "G flat grid", "G 3-D grid",
)
# a gray or gbr plan has no chroma filter, so packed_vscale never gives it a
# chroma blend: "V One ua gray" and "V One ua gbr" do not exist


def census() -> dict[str, str]:
    """bucket -> the first table entry (source/spec/filter/knobs[index]) in it."""
    hit: dict[str, str] = {}
    for spec in SPECS:
        for filt in FILTERS:
            for group in batches(spec, filt):
                for pre, cols in knobs(spec):
                    plans = []
                    for i, name in enumerate(group):
                        p = probe(name, spec, filt, pre, cols)
                        if p["rc"]:
                            continue  # (test_sws_plan.py: the refusals agree with the oracle)
                        plans.append(p)
                        tag = f"{name}/{spec}/{filt}/pre{pre}/cols{cols}[{i}]"
                        for bk in plan_buckets(p, meta(name).mode, pre, cols, i):
                            hit.setdefault(bk, tag)
                    if len(plans) == len(group):
                        hit.setdefault(grid_bucket(plans), f"{group}/{spec}/{filt}/pre{pre}")
    return hit
