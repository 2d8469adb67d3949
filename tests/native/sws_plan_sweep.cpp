// sws_plan_sweep.cpp -- stand-alone sweep of the host planner (hj_sws.cpp:
// sws_plan, sws_plan_planar, and the packer / tiler PlanCache::build) for a
// sanitizer build on the CPU:
//   g++ -std=c++17 -DHJ_HD= -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -static-libasan -static-libubsan \
//       tests/native/sws_plan_sweep.cpp spdl_amd/csrc/hj_sws.cpp -o sws_plan_sweep
// About 45 000 plans: sources and destinations from 1 pixel up, every chroma
// shift pair, the three filters; and some 250 with a side of 32768 or 65535.  Beside what the sanitizers see, every accepted
// plan is checked to keep its taps inside the source and its rows normalised;
// then it is packed and tiled under four placements (trivial, a pad with odd
// offsets, a crop with negative odd offsets, a pad that holds whole tiles) and
// both knobs, and every tile is walked with the functions the kernels use
// (hj_sws_tile.h): the launch's LDS holds the tile's layout, the tiles cover
// the output, and every index a kernel forms from the plan stays inside its
// section of the blob.  Prints "plans N refused M (packed P, tiles T)" and
// exits 0, or 1 at the first violated check.
#include <stdio.h>

#include <algorithm>

#include "../../spdl_amd/csrc/hj_sws.h"
#include "../../spdl_amd/csrc/hj_sws_tile.h"

namespace {

long g_plans = 0, g_refused = 0, g_packed = 0, g_tiles = 0;

bool check_axis(const hj::SwsAxis& a, int src, int one, const char* what) {
  if (a.n == 0) return true;
  if ((int)a.pos.size() != a.n || (int)a.coef.size() != a.n * a.size || a.eff < 1 || a.eff > a.size) {
    fprintf(stderr, "%s: sizes\n", what);
    return false;
  }
  for (int i = 0; i < a.n; i++) {
    long sum = 0;
    for (int j = 0; j < a.size; j++) sum += a.coef[(size_t)i * a.size + j];
    if (sum != one || a.pos[i] < 0 || (i && a.pos[i] < a.pos[i - 1]) ||
        (a.eff <= src && a.pos[i] + a.eff > src)) {
      fprintf(stderr, "%s: row %d (pos %d, eff %d, src %d, sum %ld)\n", what, i, a.pos[i], a.eff, src,
              sum);
      return false;
    }
  }
  return true;
}

#define REQUIRE(cond, ...)          \
  do {                              \
    if (!(cond)) {                  \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");        \
      return false;                 \
    }                               \
  } while (0)

// One axis of a packed plan as the kernels index it: pos[i] and the tap row
// [i * size, (i + 1) * size) for i < n, each inside its section of the blob
// (a section ends where the next one starts).
struct Axis {
  const int32_t* pos;
  int n, taps, size;
};
bool axis_of(const hj::PackedPlan& pp, int i, int need, Axis* a) {
  const hj::SwsDesc& d = pp.d;
  const int taps[4] = {d.hl_taps, d.hc_taps, d.vl_taps, d.vc_taps};
  const int sizes[4] = {d.hl_size, d.hc_size, d.vl_size, d.vc_size};
  const long blob = (long)pp.blob.size();
  const long p0 = d.off[2 * i], c0 = d.off[2 * i + 1], c1 = d.off[2 * i + 2];
  REQUIRE(0 <= p0 && p0 <= c0 && c0 <= c1 && c1 <= blob && p0 % 4 == 0 && c0 % 4 == 0,
          "axis %d: sections %ld %ld %ld of %ld", i, p0, c0, c1, blob);
  REQUIRE(pp.axis_n[i] >= need && taps[i] <= sizes[i] && sizes[i] % 4 == 0 && (need == 0 || taps[i] >= 1),
          "axis %d: %d rows for %d, taps %d of %d", i, pp.axis_n[i], need, taps[i], sizes[i]);
  REQUIRE(p0 + need <= c0, "axis %d: pos[%d] past its section", i, need - 1);
  REQUIRE(c0 * 2 + (long)need * sizes[i] <= c1 * 2, "axis %d: tap row %d past its section", i, need - 1);
  *a = {pp.blob.data() + p0, pp.axis_n[i], taps[i], sizes[i]};
  return true;
}

// The int16 rows [r0, r1) a band's vertical filter reads, and whether every
// padded tap read of the vertical pass (vdot_pairs: words (p >> 1) ..
// (p >> 1) + size / 2 of the column) stays inside a column of stride `cst`.
bool band_rows(const Axis& v, int ys0, int ys1, int pre_rows, bool pre, int* r0, int* r1) {
  *r0 = v.pos[ys0];
  *r1 = v.pos[ys1 - 1] + v.taps;
  REQUIRE(*r0 >= 0 && *r1 > *r0, "band rows %d..%d", *r0, *r1);
  REQUIRE(!pre || *r1 <= pre_rows, "pre-pass rows %d do not cover row %d", pre_rows, *r1);
  const int cst = hj::sws_col_stride(*r1 - *r0);
  for (int ys = ys0; ys < ys1; ys++) {
    const int p = v.pos[ys] - *r0;
    REQUIRE(p >= 0 && p + v.taps <= *r1 - *r0, "row %d starts at %d of %d", ys, p, *r1 - *r0);
    REQUIRE(2 * (p >> 1) + v.size + 2 <= cst, "row %d: padded taps past the column (%d + %d > %d)", ys,
            p, v.size, cst);
  }
  return true;
}

bool check_lds(const hj::PackedPlan& pp) {
  const hj::SwsDesc& d = pp.d;
  REQUIRE(pp.lds > 0 && pp.lds <= 64 * 1024, "lds %d", pp.lds);
  REQUIRE(pp.lds <= hj::kSwsLdsBudget || (d.rb == 1 && !d.pre), "lds %d over the budget, rb %d pre %d",
          pp.lds, d.rb, d.pre);
  REQUIRE(d.rb >= 1 && d.rb <= 32 && d.col_chunk >= 1 && d.col_chunk <= hj::kSwsMaxCols, "tile %d x %d",
          d.rb, d.col_chunk);
  REQUIRE(d.pre || (d.pre_rl == 0 && d.pre_rc == 0), "pre-pass rows without a pre-pass");
  if (!d.pre) return true;
  // hscale_kernel: its tiles cover every plane's rows, and the planes lie back
  // to back in the image's hbuf region
  const hj::HsTiles ht = hj::hs_tiles(d);
  const int nplanes = ht.tc ? 3 : 1;
  REQUIRE(ht.wgs == ht.tl + 2 * ht.tc && (ht.tc > 0) == (d.gbr || !d.gray), "hscale tiles");
  long end = 0;
  for (int c = 0; c < nplanes; c++) {
    const hj::HsPlane p = hj::hs_plane(d, c);
    const int tiles = c ? ht.tc : ht.tl;
    REQUIRE(p.off == end && p.rows >= 1 && p.w >= 1, "hbuf plane %d at %ld, the last ends at %ld", c,
            (long)p.off, end);
    REQUIRE((tiles - 1) * hj::kHsRows < p.rows && p.rows <= tiles * hj::kHsRows,
            "hbuf plane %d: %d tiles for %d rows", c, tiles, p.rows);
    REQUIRE(p.rows == (c == 0 || d.gbr ? d.pre_rl : d.pre_rc) && p.w == (c == 0 || d.gbr ? d.sw : d.chr_w),
            "hbuf plane %d is %d x %d", c, p.rows, p.w);
    end += (long)p.rows * p.w;
  }
  REQUIRE(end == (long)hj::hs_hbuf_size(d), "hbuf region %ld, planes end at %ld", (long)hj::hs_hbuf_size(d),
          end);
  return true;
}

// sws_kernel's tiles (bands x chunks)
bool walk_rgb(const hj::PlanKey& k, const hj::PackedPlan& pp) {
  const hj::SwsDesc& d = pp.d;
  if (!check_lds(pp)) return false;
  Axis hl, hc{}, vl, vc{};
  const bool chroma = !d.gray;
  if (!axis_of(pp, 0, k.sw, &hl) || !axis_of(pp, 2, k.sh, &vl)) return false;
  if (!axis_of(pp, 1, chroma ? d.chr_w : 0, &hc) || !axis_of(pp, 3, chroma ? k.sh : 0, &vc)) return false;
  const long vm = d.off[hj::kVmode];
  REQUIRE(d.off[hj::kVcCoef] <= vm && vm + k.sh <= (long)pp.blob.size(), "vmode past the blob");
  REQUIRE(d.sw == k.sw && d.sh == k.sh && (!d.gbr || d.gray), "desc");
  REQUIRE(pp.bands == hj::tile_div_up(k.oh, d.rb) && pp.chunks == hj::tile_div_up(k.ow, d.col_chunk),
          "%d x %d tiles of %d x %d for %d x %d", pp.bands, pp.chunks, d.rb, d.col_chunk, k.ow, k.oh);
  long area = 0;
  for (int band = 0; band < pp.bands; band++)
    for (int chunk = 0; chunk < pp.chunks; chunk++) {
      const int yo0 = band * d.rb, xo0 = chunk * d.col_chunk;
      REQUIRE(yo0 < k.oh && xo0 < k.ow, "tile %d, %d starts outside the output", band, chunk);
      const hj::SwsWindow w =
          hj::sws_window(yo0, xo0, d.rb, d.col_chunk, k.dx, k.dy, k.ow, k.oh, k.sw, k.sh);
      REQUIRE(w.yo1 > yo0 && w.xo1 > xo0 && w.yo1 <= k.oh && w.xo1 <= k.ow, "tile %d, %d", band, chunk);
      area += (long)(w.yo1 - yo0) * (w.xo1 - xo0);
      g_tiles++;
      int ncl = 0, ncc = 0, lr0 = 0, lr1 = 0, cr0 = 0, cr1 = 0;
      if (w.content) {
        REQUIRE(w.ys0 >= 0 && w.ys1 <= k.sh && w.xs0 >= 0 && w.xs1 <= k.sw, "window past the content");
        ncl = w.xs1 - w.xs0;
        if (!band_rows(vl, w.ys0, w.ys1, d.pre_rl, d.pre, &lr0, &lr1)) return false;
        if (chroma) {
          const hj::SwsChromaCols cc = hj::sws_chroma_cols(w.xs0, w.xs1, d.full);
          ncc = cc.ncc;
          REQUIRE(cc.cx0 >= 0 && ncc >= 1 && cc.cx0 + ncc <= d.chr_w, "chroma columns %d + %d of %d",
                  cc.cx0, ncc, d.chr_w);
          // (every luma column's chroma column is one of the tile's)
          const int last = (d.full ? w.xs1 - 1 : (w.xs1 - 1) >> 1) - cc.cx0;
          REQUIRE(last == ncc - 1, "chroma column of the last pixel");
          if (!band_rows(vc, w.ys0, w.ys1, d.pre_rc, d.pre, &cr0, &cr1)) return false;
        }
      }
      const hj::SwsLds l = hj::sws_lds_layout(ncl, ncc, lr1 - lr0, cr1 - cr0, d.gbr, d.gray, d.rb,
                                              d.col_chunk, d.vl_size, d.vc_size);
      REQUIRE(2 * l.hu <= l.tile && 2 * l.hv <= l.tile && l.hu <= l.hv && l.tile % 16 == 0 &&
                  l.vt % 16 == 0 && l.tile + (w.yo1 - yo0) * (w.xo1 - xo0) * 3 <= l.vt &&
                  l.vt + (w.ys1 > w.ys0 ? w.ys1 - w.ys0 : 0) * l.vrw * 4 <= l.end,
              "layout regions overlap");
      REQUIRE(l.end <= pp.lds, "tile %d, %d needs %d bytes of LDS, the plan has %d", band, chunk, l.end,
              pp.lds);
    }
  REQUIRE(area == (long)k.ow * k.oh, "tiles cover %ld of %ld pixels", area, (long)k.ow * k.oh);
  return true;
}

// yuv_planes_kernel's tiles: the luma plane's, then U's and V's
bool walk_planar(const hj::PlanKey& k, const hj::PackedPlan& pp) {
  const hj::SwsDesc& d = pp.d;
  if (!check_lds(pp)) return false;
  REQUIRE(d.yuv && pp.chunks == 1 && d.sw == k.sw && d.sh == k.sh, "desc");
  const hj::PlanarTiles pt = hj::planar_tiles(k.ow, k.oh, d.hsub, d.vsub, d.rb, d.col_chunk, d.gray);
  REQUIRE(pp.bands == pt.total && pt.total == pt.ltiles + (d.gray ? 0 : 2 * pt.ctiles),
          "%d tiles, the planes have %d + 2 x %d", pp.bands, pt.ltiles, pt.ctiles);
  for (int c = 0; c < (d.gray ? 1 : 2); c++) {  // (V's tiles are U's)
    const bool luma = c == 0;
    const int W = luma ? k.ow : pt.cw, H = luma ? k.oh : pt.ch;
    const int psw = luma ? d.sw : d.chr_w, psh = luma ? d.sh : d.chr_h;
    const int pdx = luma ? k.dx : k.dx >> d.hsub, pdy = luma ? k.dy : k.dy >> d.vsub;
    Axis h, v;
    if (!axis_of(pp, luma ? 0 : 1, psw, &h) || !axis_of(pp, luma ? 2 : 3, psh, &v)) return false;
    const int chunks = luma ? pt.lchunks : pt.cchunks, ntiles = luma ? pt.ltiles : pt.ctiles;
    REQUIRE((chunks - 1) * d.col_chunk < W && W <= chunks * d.col_chunk &&
                ntiles == chunks * hj::tile_div_up(H, d.rb),
            "plane %d: %d chunks, %d tiles", c, chunks, ntiles);
    long area = 0;
    for (int t = 0; t < ntiles; t++) {
      const int band = t / chunks, chunk = t - band * chunks;
      const int yo0 = band * d.rb, xo0 = chunk * d.col_chunk;
      REQUIRE(yo0 < H && xo0 < W, "plane %d tile %d starts outside the plane", c, t);
      const hj::SwsWindow w = hj::sws_window(yo0, xo0, d.rb, d.col_chunk, pdx, pdy, W, H, psw, psh);
      const int th = w.yo1 - yo0, tw = w.xo1 - xo0;
      REQUIRE(th > 0 && tw > 0 && w.yo1 <= H && w.xo1 <= W, "plane %d tile %d", c, t);
      area += (long)th * tw;
      g_tiles++;
      int ncl = 0, r0 = 0, r1 = 0;
      if (w.content) {
        REQUIRE(w.ys0 >= 0 && w.ys1 <= psh && w.xs0 >= 0 && w.xs1 <= psw, "window past the content");
        ncl = w.xs1 - w.xs0;
        if (!band_rows(v, w.ys0, w.ys1, luma ? d.pre_rl : d.pre_rc, d.pre, &r0, &r1)) return false;
      }
      // the tile's runs: whole (one run of th * W bytes) or th runs `pitch`
      // apart, each up to 15 bytes into its 16
      const hj::PlanarLds l = hj::planar_lds_layout(ncl, r1 - r0, th, tw);
      const int last = tw == W ? 15 + th * W : (th - 1) * l.pitch + 15 + tw;
      REQUIRE(l.tile % 16 == 0 && 2 * ncl * l.cst <= l.tile && l.tile + last <= l.bound,
              "plane %d tile %d: the tile's runs end past the layout's bound", c, t);
      REQUIRE(l.bound <= pp.lds, "plane %d tile %d needs %d bytes of LDS, the plan has %d", c, t, l.bound,
              pp.lds);
    }
    REQUIRE(area == (long)W * H, "plane %d: tiles cover %ld of %ld", c, area, (long)W * H);
  }
  return true;
}

// The plan packed and tiled as build_layout would for an image placed at
// (dx, dy) in an ow x oh output, under both knobs.
bool pack_and_walk(hj::PlanKey k, bool planar, int which) {
  // placements of the dw x dh content: trivial; a pad with odd offsets; a
  // crop with negative odd offsets; a pad that holds whole tiles.  (A planar
  // destination keeps its offsets on the chroma grid: shifted.)
  const int hs = planar ? k.hsub : 0, vs = planar ? k.vsub : 0;
  switch (which) {
    case 0: break;
    case 1:
      k.dx = 3 << hs, k.dy = 5 << vs;
      k.ow = k.sw + (7 << hs), k.oh = k.sh + (9 << vs);
      break;
    case 2:
      k.dx = -(3 << hs), k.dy = -(1 << vs);
      k.ow = k.sw - (5 << hs), k.oh = k.sh - (3 << vs);
      if (k.ow < 1 || k.oh < 1) return true;  // (nothing left to crop to)
      break;
    default:
      k.dx = 260 << hs, k.dy = 36 << vs;
      k.ow = k.sw + (261 << hs), k.oh = k.sh + (37 << vs);  // (left and above: fewer tiles)
  }
  for (int pre = -1; pre <= 1; pre++)
    for (int cols : {256, 16}) {
      int rc = 0;
      const auto pp = hj::PlanCache::build(k, &rc, pre, cols);
      g_packed++;
      // (the planner accepted this size: the tiler has a one-row band for it)
      bool ok = pp && rc == 0;
      if (!ok) fprintf(stderr, "the packer refuses (%d)\n", rc);
      ok = ok && pp->d.col_chunk <= cols && (pre < 0 || pp->d.pre == pre);
      ok = ok && (planar ? walk_planar(k, *pp) : walk_rgb(k, *pp));
      if (!ok) {
        fprintf(stderr, "  placement %d: %d, %d in %d x %d, prepass %d, max_cols %d\n", which, k.dx, k.dy,
                k.ow, k.oh, pre, cols);
        return false;
      }
    }
  return true;
}

bool one_plan(int w, int h, int hs, int vs, bool gray, int dw, int dh, int kind, bool planar) {
  hj::SwsPlan p;
  const int rc = planar ? hj::sws_plan_planar(w, h, hs, vs, gray, dw, dh, kind, &p)
                        : hj::sws_plan(w, h, hs, vs, gray, dw, dh, kind, &p);
  g_plans++;
  if (rc) {
    g_refused++;
    return true;
  }
  bool ok = check_axis(p.hl, w, 1 << 14, "hl") && check_axis(p.vl, h, 1 << 12, "vl");
  if (!gray)
    ok = ok && check_axis(p.hc, p.chrSrcW, 1 << 14, "hc") && check_axis(p.vc, p.chrSrcH, 1 << 12, "vc");
  if (!planar && (int)p.vmode.size() != dh) ok = false;
  // every placement; a gray plan as the three RGB planes (gbr) every other
  // time (the turn shifts with every group of six calls, so that no size
  // meets one of the two only)
  const int mode = planar ? (gray ? hj::kPlanGray : hj::kPlanYuv) | hj::kPlanPlanar
                   : !gray ? hj::kPlanYuv
                           : ((g_plans + g_plans / 6) & 1 ? hj::kPlanGbr : hj::kPlanGray);
  const hj::PlanKey k{w, h, hs, vs, mode, kind, dw, dh, 0, 0, dw, dh};
  for (int which = 0; which < 4; which++) ok = ok && pack_and_walk(k, planar, which);
  if (!ok)
    fprintf(stderr, "  %dx%d sub %d%d gray %d -> %dx%d filter %d planar %d\n", w, h, hs, vs, gray, dw,
            dh, kind, planar);
  return ok;
}

}  // namespace

int main() {
  static const int kSrc[] = {1, 2, 3, 4, 5, 7, 8, 9, 16, 31, 64, 137, 272, 400, 776};
  static const int kDst[] = {1, 2, 3, 4, 5, 8, 9, 33, 51, 64, 97, 300};
  const int ns = sizeof(kSrc) / sizeof(*kSrc), nd = sizeof(kDst) / sizeof(*kDst);
  // widths against a few heights (the axes are planned independently), then
  // heights against a few widths
  static const int kFew[] = {1, 5, 40};
  for (int kind = 0; kind < 3; kind++)
    for (int hs = 0; hs <= 2; hs++)
      for (int vs = 0; vs <= 2; vs++)
        for (int gray = 0; gray <= (hs == 0 && vs == 0 ? 1 : 0); gray++)
          for (int planar = 0; planar <= (hs <= 1 && vs <= hs ? 1 : 0); planar++)
            for (int a = 0; a < ns; a++)
              for (int b = 0; b < nd; b++)
                for (int f : kFew) {
                  if (!one_plan(kSrc[a], f, hs, vs, gray, kDst[b], f == 40 ? 37 : f, kind, planar) ||
                      !one_plan(f, kSrc[a], hs, vs, gray, f == 40 ? 37 : f, kDst[b], kind, planar))
                    return 1;
                }
  // Frames at the format's limit: one side of 32768 or 65535 against 17, to
  // itself, to 1/63 (the longest filters swscale takes) and to one sample
  // (refused: the ratio leaves swscale's int).
  static const int kLong[] = {32768, 65535};
  const long before = g_refused;
  for (int kind = 0; kind < 3; kind++)
    for (int sub = 0; sub < 4; sub++) {  // gray, 4:4:4, 4:2:0, 4:1:1
      const int hs = sub == 3 ? 2 : sub == 2 ? 1 : 0, vs = sub == 2 ? 1 : 0, gray = sub == 0;
      for (int planar = 0; planar <= (sub < 3 ? 1 : 0); planar++)
        for (int L : kLong)
          for (int S : {17}) {
            const int dst[] = {L, (L + 62) / 63, 1};
            for (int d : dst)
              if (!one_plan(L, S, hs, vs, gray, d, S, kind, planar) ||
                  !one_plan(S, L, hs, vs, gray, S, d, kind, planar))
                return 1;
            // (the last two, L -> 1, were refused)
            hj::SwsPlan p;
            if (hj::sws_plan(L, S, hs, vs, gray, 1, S, kind, &p) != 7 /* BAD_GEOMETRY */ ||
                hj::sws_plan_planar(S, L, hs, vs, gray, S, 1, kind, &p) != 7) {
              fprintf(stderr, "%d -> 1 is accepted (filter %d, sub %d%d)\n", L, kind, hs, vs);
              return 1;
            }
          }
    }
  if (g_refused - before < 3 * 4 * 2 * 2) return 1;
  printf("plans %ld refused %ld (packed %ld, tiles %ld)\n", g_plans, g_refused, g_packed, g_tiles);
  return g_refused > 0 && g_refused < g_plans && g_tiles > g_packed ? 0 : 1;
}
