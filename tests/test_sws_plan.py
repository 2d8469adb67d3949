"""CPU tests of the output stage's host plan (no GPU): the product's plan
probe (spdl_hj_debug_sws_plan: geometry() + PlanCache::build) against the
oracle's plan (oracle.sws_plan: jo_sws_init), bit for bit, on the sweep's case
table (tests/sws_sweep_cases.py) and on a wider grid; the refusal boundary;
the census of kernel and tiler paths the table reaches; and the value
conditions of its source families.

Reading a census failure: the message names the buckets no table entry
falls in any more.  A retuned tiler (band heights, the LDS budget, the
pre-pass rule) moved the table off that path: add or change an entry of
sws_sweep_cases.py until the bucket is hit again -- do not drop the bucket.
"""

import numpy as np
import pytest

from spdl_amd import _lib
from spdl_amd._lib import Output
from tests import sws_sweep_cases as S

AXES = ("hl", "hc", "vl", "vc")
BAD_GEOMETRY = 7


def _axis_src(w, h, hsub, vsub, gray):
    """Source samples of the hl, hc, vl, vc axes (chroma: AV_CEIL_RSHIFT)."""
    hs, vs = (0, 0) if gray else (hsub, vsub)
    return w, -(-w >> hs), h, -(-h >> vs)


def _vmode_of(q):
    """packed_vscale's writer per row from the ORACLE's vertical filters:
    mode | yalpha << 4 | uvalpha << 17 (0 X, 1 One, 2 Two)."""
    vl, vc = q["vl"], q["vc"]
    n = vl["n"]
    if q["special"]:
        return np.full(n, 1, np.int64)

    def bilin(f):
        c = f["coef"].astype(np.int64)
        return (c[:, 0] + c[:, 1] == 4096) & (c[:, 1] >= 0) & (c[:, 1] <= 4096)

    out = np.zeros(n, np.int64)
    lfs, cfs = vl["size"], (1 if q["gray"] else vc["size"])
    if q["gray"]:
        if lfs == 1:
            out[:] = 1
        elif lfs == 2:
            out = np.where(bilin(vl), 2 | (vl["coef"][:, 1].astype(np.int64) << 4), 0)
    elif lfs == 1 and cfs == 1:
        out[:] = 1
    elif lfs == 1 and cfs == 2:
        out = np.where(bilin(vc), 1 | (vc["coef"][:, 1].astype(np.int64) << 17), 0)
    elif lfs == 2 and cfs == 2:
        out = np.where(bilin(vl) & bilin(vc), 2 | (vl["coef"][:, 1].astype(np.int64) << 4)
                       | (vc["coef"][:, 1].astype(np.int64) << 17), 0)
    return out


def check_plan(p, q, src, tag, trivial_placement):
    """Product probe `p` against oracle plan `q` (None: refused), and the
    invariants of the tables the device gets."""
    if q is None:
        assert p["rc"] == BAD_GEOMETRY, f"{tag}: the oracle refuses, the product returns {p['rc']}"
        return
    assert p["rc"] == 0, f"{tag}: the oracle accepts, the product returns {p['rc']}"
    assert (p["full"], p["gray"]) == (q["full"], q["gray"]), tag
    assert p["special"] == (q["special"] if trivial_placement else 0), tag
    if not q["gray"]:
        assert p["chr_w"] == q["chrDstW"], tag
    for a, one, n_src in zip(AXES, (1 << 14, 1 << 14, 1 << 12, 1 << 12), src):
        pa, qa = p[a], q[a]
        eff, stride = pa["taps"], pa["stride"]
        assert pa["n"] == qa["n"], f"{tag} {a}: rows"
        if qa["n"] == 0:
            continue
        assert 1 <= eff <= qa["size"] and eff <= stride and stride % 4 == 0, f"{tag} {a}: sizes"
        np.testing.assert_array_equal(pa["pos"], qa["pos"], err_msg=f"{tag} {a}: positions")
        np.testing.assert_array_equal(pa["coef"][:, :eff], qa["coef"][:, :eff],
                                      err_msg=f"{tag} {a}: taps")
        assert not qa["coef"][:, eff:].any(), f"{tag} {a}: a tap the product cut is not zero"
        assert not pa["coef"][:, eff:].any(), f"{tag} {a}: padding taps are not zero"
        assert (pa["coef"].astype(np.int64).sum(axis=1) == one).all(), f"{tag} {a}: row sums"
        assert (np.diff(pa["pos"]) >= 0).all() and pa["pos"][0] >= 0, f"{tag} {a}: positions order"
        if eff <= n_src:
            assert int(pa["pos"].max()) + eff <= n_src, f"{tag} {a}: taps past the source"
    np.testing.assert_array_equal(p["vmode"], _vmode_of(q), err_msg=f"{tag}: row writers")


# ---- parity of the plans ------------------------------------------------------------

@pytest.mark.parametrize("spec", list(S.SPECS))
def test_table_plans_match_oracle(oracle, spec):
    """Every table entry (refused ones included), under every knob setting:
    the tables do not depend on the knobs, the tiling does."""
    for filt in S.FILTERS:
        for name in S.SOURCES:
            m = S.meta(name)
            g, q = S.oracle_plan(oracle, name, spec, filt)
            src = _axis_src(m.w, m.h, m.hsub, m.vsub, m.mode != "yuv")
            for pre, cols in S.knobs(spec):
                p = S.probe(name, spec, filt, pre, cols)
                tag = f"{name}/{spec}/{filt}/pre{pre}/cols{cols}"
                assert {k: p[k] for k in g} == g, f"{tag}: geometry"
                trivial = (g["dx"], g["dy"], g["ow"], g["oh"]) == (0, 0, g["sw"], g["sh"])
                check_plan(p, q, src, tag, trivial)
                if p["rc"]:
                    continue
                assert p["gbr"] == (m.mode == "gbr"), tag
                # the tiling covers the output, inside what a workgroup may take
                assert 1 <= p["rb"] <= 32 and 1 <= p["col_chunk"] <= min(cols, max(g["ow"], 1)), tag
                assert p["bands"] == -(-g["oh"] // p["rb"]), tag
                assert p["chunks"] == -(-g["ow"] // p["col_chunk"]), tag
                assert p["lds"] <= 64 * 1024 and (p["lds"] <= S.LDS_BUDGET or
                                                  (p["rb"] == 1 and not p["pre"])), tag
                assert p["pre"] == {1: 1, 0: 0}.get(pre, p["pre"]), tag


GRID_SRC = [(1, 1), (2, 3), (3, 2), (4, 5), (5, 4), (7, 1), (1, 9), (8, 8), (17, 16), (31, 64),
            (137, 91), (272, 40), (400, 24), (24, 400), (776, 16)]
GRID_DST = [(1, 1), (2, 1), (1, 3), (3, 4), (4, 2), (5, 5), (8, 9), (33, 21), (51, 37), (64, 48),
            (300, 70)]
# every (hsub, vsub) chroma_shifts lets through with vs, hs <= 2, and gray
GRID_SUB = [(0, 0), (1, 0), (1, 1), (0, 1), (2, 0), (2, 1), (0, 2), (1, 2), (2, 2)]


@pytest.mark.parametrize("filt", S.FILTERS)
def test_grid_plans_match_oracle(oracle, filt):
    """A wider grid (15 x 11 sizes x 10 samplings per filter, sources and
    destinations down to 1): parity, refusals and invariants."""
    n = refused = 0
    for w, h in GRID_SRC:
        for dw, dh in GRID_DST:
            out = Output(pix_fmt="rgb24", resize=True, fit_w=dw, fit_h=dh, filter=filt)
            for hsub, vsub, mode in [*((a, b, "yuv") for a, b in GRID_SUB), (0, 0, "gray")]:
                p = _lib.debug_sws_plan(w, h, hsub, vsub, mode, out)
                q = oracle.sws_plan(w, h, hsub, vsub, mode == "gray", dw, dh, filt)
                check_plan(p, q, _axis_src(w, h, hsub, vsub, mode == "gray"),
                           f"{w}x{h}->{dw}x{dh} {filt} sub{hsub}{vsub} {mode}", True)
                n += 1
                refused += q is None
    assert n == len(GRID_SRC) * len(GRID_DST) * 10 and 0 < refused < n


@pytest.mark.parametrize("filt", S.FILTERS)
def test_planar_plans_match_oracle_axes(oracle, filt):
    """The planar destination (pix_fmt="yuv"): every plane through its own
    filters with centred siting on both sides, chroma ceil-shifted on both
    sides -- the axes of oracle.sws_axis, as tests/yuv_scale_ref.py uses them."""
    n = 0
    for (w, h), (dw, dh) in [((400, 24), (8, 24)), ((272, 40), (8, 40)), ((400, 24), (598, 10)),
                             ((137, 91), (51, 37)), ((9, 17), (33, 21)), ((3, 2), (8, 9)),
                             ((1, 1), (5, 5)), ((64, 400), (64, 8)), ((776, 16), (8, 16))]:
        for hsub, vsub, mode in ((0, 0, "yuv"), (1, 0, "yuv"), (1, 1, "yuv"), (0, 0, "gray")):
            out = Output(pix_fmt="yuv", resize=True, fit_w=dw, fit_h=dh, filter=filt)
            p = _lib.debug_sws_plan(w, h, hsub, vsub, mode, out)
            gray = mode == "gray"
            sizes = [(w, dw, 4, 1 << 14), (-(-w >> hsub), -(-dw >> hsub), 4, 1 << 14),
                     (h, dh, 2, 1 << 12), (-(-h >> vsub), -(-dh >> vsub), 2, 1 << 12)]
            try:
                want = [oracle.sws_axis(a, b, filt, align=al, one=one)
                        for k, (a, b, al, one) in enumerate(sizes) if not (gray and k in (1, 3))]
            except oracle.OracleError:
                assert p["rc"] == BAD_GEOMETRY, (w, h, dw, dh, hsub, vsub, mode)
                continue
            assert p["rc"] == 0 and p["planar"] == 1, (w, h, dw, dh, hsub, vsub, mode)
            axes = [a for k, a in enumerate(AXES) if not (gray and k in (1, 3))]
            for a, (pos, coef) in zip(axes, want):
                eff = p[a]["taps"]
                np.testing.assert_array_equal(p[a]["pos"], pos, err_msg=a)
                np.testing.assert_array_equal(p[a]["coef"][:, :eff], coef[:, :eff], err_msg=a)
                assert not coef[:, eff:].any() and not p[a]["coef"][:, eff:].any(), a
            n += 1
    assert n >= 20


# ---- the refusal boundary -------------------------------------------------------------

@pytest.mark.parametrize("src", [400, 776, 272])
@pytest.mark.parametrize("filt", S.FILTERS)
def test_refusal_boundary(oracle, src, filt):
    """Walking dst down from src: product and oracle refuse exactly the same
    widths, from the same one on, and the last accepted filter has fewer than
    256 taps."""
    first_refused, last_taps = None, None
    for dst in range(src, 0, -1):
        out = Output(pix_fmt="rgb24", resize=True, fit_w=dst, fit_h=0, filter=filt)
        p = _lib.debug_sws_plan(src, 16, 0, 0, "gray", out)
        q = oracle.sws_plan(src, 16, 0, 0, True, dst, 16, filt)
        assert (p["rc"] == BAD_GEOMETRY) == (q is None) and p["rc"] in (0, BAD_GEOMETRY), (src, dst)
        if q is None:
            first_refused = first_refused or dst
        else:
            assert first_refused is None, f"{src}->{dst} accepted below the refused {first_refused}"
            assert q["hl"]["size"] < 256 and p["hl"]["taps"] <= q["hl"]["size"]
            last_taps = p["hl"]["taps"]
    assert first_refused is not None and first_refused > 1
    assert 128 < last_taps < 256, "the boundary is not in the four-chunk range"


# ---- the census -------------------------------------------------------------------------

def test_census_every_bucket_is_hit():
    hit = S.census()
    print("\n".join(f"{b:45s} {hit[b]}" for b in S.REQUIRED if b in hit))
    missing = [b for b in S.REQUIRED if b not in hit]
    assert not missing, "no table entry takes these paths any more: " + "; ".join(missing)
    between = sorted(b for b in hit if b.startswith("T-a rb="))
    assert len(between) >= 2, f"band heights between 32 and 1: only {between}"
    # a gray / gbr plan has no chroma filter: no chroma blend on a One row
    assert "V One ua gray" not in hit and "V One ua gbr" not in hit


def test_refused_entries_exist_past_the_boundary():
    """The GPU sweep's refusal cases: the table holds entries swscale refuses."""
    cells = [(s, f, n) for s in S.SPECS for f in S.FILTERS for n in S.refused(s, f)]
    assert len(cells) >= 10
    assert {S.meta(n).mode for _, _, n in cells} == {"yuv", "gray", "gbr"}


# ---- value conditions of the source families -----------------------------------------------

def _content(ref, g):
    y0, x0 = max(g["dy"], 0), max(g["dx"], 0)
    y1, x1 = min(g["dy"] + g["sh"], g["oh"]), min(g["dx"] + g["sw"], g["ow"])
    return ref[y0:y1, x0:x1]


@pytest.mark.parametrize("filt", S.FILTERS)
def test_texture_family_is_unsaturated(oracle, filt):
    """The texture family must not hide arithmetic behind clamps: at most 25 %
    of the oracle's output samples inside the content region are 0 or 255
    (the suite's figure for unsaturated families), per (spec, filter) cell."""
    for spec in S.SPECS:
        sat = tot = 0
        for group in S.batches(spec, filt):
            for name in set(group):
                if name not in S.TEXTURE:
                    continue
                m = S.meta(name)
                rs = S.resize(oracle, spec, filt)
                c = _content(oracle.decode_resize(S.source(name), rs), oracle.geometry(m.w, m.h, rs))
                sat += int(((c == 0) | (c == 255)).sum())
                tot += c.size
        assert tot and sat <= 0.25 * tot, f"{spec}/{filt}: {sat} of {tot} samples saturated"


@pytest.mark.parametrize("name", list(S.EDGES))
@pytest.mark.parametrize("filt", ["bicubic", "lanczos"])
def test_edges_family_reaches_both_clamps(oracle, name, filt):
    """112 -> 300 upscale of the 0 / 255 bars: the horizontal luma sums,
    recomputed here from the oracle's planes and luma filter, exceed the h15
    cap ((sum >> 7) > 32767) and go negative, and the output holds 0 and 255."""
    m = S.meta(name)
    _, q = S.oracle_plan(oracle, name, "up300x70", filt)
    luma = oracle.decode_planes(S.source(name))[0].astype(np.int64)
    pos, coef = q["hl"]["pos"], q["hl"]["coef"].astype(np.int64)
    sums = np.zeros((m.h, q["hl"]["n"]), np.int64)
    for j in range(q["hl"]["size"]):
        sums += luma[:, np.minimum(pos + j, m.w - 1)] * coef[:, j][None, :]
    assert ((sums >> 7) > 32767).any(), "no horizontal sum reaches the h15 cap"
    assert (sums < 0).any(), "no horizontal sum goes negative"
    ref = oracle.decode_resize(S.source(name), S.resize(oracle, "up300x70", filt))
    assert (ref == 0).any() and (ref == 255).any()


# ---- the planner under sanitizers (stand-alone program, host code only) ---------------------

def test_planner_sweep_under_sanitizers(tmp_path):
    """tests/native/sws_plan_sweep.cpp + hj_sws.cpp built with ASan and UBSan
    and run as a program of its own: about 45 000 plans of sws_plan and
    sws_plan_planar, each accepted one packed and tiled (PlanCache::build)
    under four placements and both knobs and every tile walked with
    hj_sws_tile.h; no report and every built-in check green."""
    import os
    import shutil
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    exe = str(tmp_path / "sws_plan_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-DHJ_HD=", *san,
                    os.path.join(root, "tests", "native", "sws_plan_sweep.cpp"),
                    os.path.join(root, "spdl_amd", "csrc", "hj_sws.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("plans ") and not r.stderr, r.stdout + r.stderr
