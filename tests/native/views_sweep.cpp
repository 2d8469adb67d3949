// views_sweep.cpp -- stand-alone sweep of the host arithmetic of views
// (spdl_amd/csrc/hj_views.h), for a sanitizer build on the CPU:
//   g++ -std=c++17 -O2 -DHJ_HD= -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -static-libasan -static-libubsan tests/native/views_sweep.cpp -o views_sweep
// Frames: gray, 4:4:4, 4:2:0, 4:1:1 and 4:1:0 on grids of 1..5 x 1..4 MCUs whose
// last column / row of MCUs is partial (one sample wide) or full.  Of every
// frame 24 rectangles -- origins and sizes on and off the MCU and chroma grids,
// the whole frame, one that does not resolve -- and every set of 1..3 of them
// as the views of one image.  For each set:
//   the bounding MCU rectangle holds every view's MCU rectangle, and each of
//     its four sides is some view's (it is the smallest such rectangle);
//   every view's component windows lie inside the samples the IDCT of the
//     bounding rectangle writes, and inside the component's plane;
//   a view that does not resolve adds nothing; no view at all: zero blocks;
//   a whole-frame view makes it the whole grid.
// The same properties on frames with one side of 32768, 65500 and 65535 for
// rectangles within 16 samples of the far end (sweep_far_end).
// And for the descriptor slices: the groups' slices follow the n images, in
// order, without gap or overlap.  Prints "sets N checks M", then "far-end sets
// N checks M", and exits 0, or 1 at the first failure.
#include <stdio.h>

#include <vector>

#include "../../spdl_amd/csrc/hj_common.h"
#include "../../spdl_amd/csrc/hj_views.h"

namespace {

using namespace hj::views;

long g_sets = 0, g_checks = 0;

#define CHECK(cond, ...)          \
  do {                            \
    g_checks++;                   \
    if (!(cond)) {                \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");      \
      return false;               \
    }                             \
  } while (0)

struct Format {
  const char* name;
  int ncomp, h0, v0;
};
const Format kFormats[] = {{"gray", 1, 1, 1}, {"444", 3, 1, 1}, {"420", 3, 2, 2},
                           {"411", 3, 4, 1},  {"410", 3, 4, 4}};

Frame frame(const Format& f, int mcux, int mcuy, bool partial_x, bool partial_y) {
  Frame fr{};
  fr.ncomp = f.ncomp;
  for (int c = 0; c < f.ncomp; c++) fr.h_samp[c] = fr.v_samp[c] = 1;
  fr.h_samp[0] = f.h0;
  fr.v_samp[0] = f.v0;
  const int mw8 = 8 * (f.ncomp == 1 ? 1 : f.h0), mh8 = 8 * (f.ncomp == 1 ? 1 : f.v0);
  fr.width = mcux * mw8 - (partial_x ? mw8 - 1 : 0);
  fr.height = mcuy * mh8 - (partial_y ? mh8 - 1 : 0);
  return fr;
}

struct View {
  Rect in, r;
  int rc;
  McuRect m;
};

bool in_window(const Window& inner, const Window& outer) {
  return inner.x >= outer.x && inner.y >= outer.y && inner.x + inner.w <= outer.x + outer.w &&
         inner.y + inner.h <= outer.y + outer.h;
}

bool check_set(const Frame& f, const Grid& g, const View* const* set, int n) {
  g_sets++;
  McuRect bound{0, 0, 0, 0};
  bool whole = false;
  int live = 0;
  for (int i = 0; i < n; i++) {
    if (set[i]->rc) continue;
    live++;
    whole = whole || rect_is_none(set[i]->in);
    mcu_union(&bound, set[i]->m);
  }
  if (!live) {
    CHECK(bound.mw == 0 && idct_blocks(g, bound) == 0, "views that do not resolve made blocks");
    return true;
  }
  CHECK(bound.mx0 >= 0 && bound.my0 >= 0 && bound.mw >= 1 && bound.mh >= 1 &&
            bound.mx0 + bound.mw <= g.mcux && bound.my0 + bound.mh <= g.mcuy,
        "bounding rectangle (%d, %d, %d, %d) outside the %d x %d grid", bound.mx0, bound.my0,
        bound.mw, bound.mh, g.mcux, g.mcuy);
  if (whole)
    CHECK(idct_blocks(g, bound) == g.mcux * g.mcuy * g.bpm, "a whole-frame view: %d blocks of %d",
          idct_blocks(g, bound), g.mcux * g.mcuy * g.bpm);
  bool side[4] = {false, false, false, false};
  for (int i = 0; i < n; i++) {
    const View& v = *set[i];
    if (v.rc) continue;
    CHECK(v.m.mx0 >= bound.mx0 && v.m.my0 >= bound.my0 &&
              v.m.mx0 + v.m.mw <= bound.mx0 + bound.mw && v.m.my0 + v.m.mh <= bound.my0 + bound.mh,
          "view (%d, %d, %d, %d): its MCUs leave the bounding rectangle", v.r.x, v.r.y, v.r.w,
          v.r.h);
    side[0] = side[0] || v.m.mx0 == bound.mx0;
    side[1] = side[1] || v.m.my0 == bound.my0;
    side[2] = side[2] || v.m.mx0 + v.m.mw == bound.mx0 + bound.mw;
    side[3] = side[3] || v.m.my0 + v.m.mh == bound.my0 + bound.mh;
    for (int c = 0; c < f.ncomp; c++) {
      const Window w = window(f, g, v.r, c), area = mcu_plane_area(f, bound, c);
      const int bh = f.ncomp == 1 ? 1 : f.h_samp[c], bv = f.ncomp == 1 ? 1 : f.v_samp[c];
      const Window plane{0, 0, g.mcux * bh * 8, g.mcuy * bv * 8};
      CHECK(w.w >= 1 && w.h >= 1 && in_window(w, area),
            "view (%d, %d, %d, %d) component %d: window (%d, %d, %d, %d) leaves the bounding "
            "rectangle's samples (%d, %d, %d, %d)",
            v.r.x, v.r.y, v.r.w, v.r.h, c, w.x, w.y, w.w, w.h, area.x, area.y, area.w, area.h);
      CHECK(in_window(area, plane), "the bounding rectangle's samples leave plane %d", c);
    }
  }
  CHECK(side[0] && side[1] && side[2] && side[3], "the bounding rectangle is not the smallest");
  return true;
}

// One candidate resolved and checked: the rectangle inside the frame and on the
// chroma grid, its MCU rectangle the one its corners fall in
bool resolve_view(const Format& fmt, const Frame& f, const Grid& g, View& v, bool* refused) {
  int hsub, vsub;
  CHECK(chroma_shifts(f, &hsub, &vsub) == hj::kOk, "%s: chroma shifts", fmt.name);
  const int hs = 1 << hsub, vs = 1 << vsub, mw8 = 8 * g.hmax, mh8 = 8 * g.vmax;
  const int W = f.width, H = f.height;
  v.rc = resolve(f, v.in, &v.r);
  if (v.rc) {
    CHECK(v.rc == hj::kErrBadGeometry, "resolve: status %d", v.rc);
    *refused = true;
    return true;
  }
  CHECK(v.r.x >= 0 && v.r.y >= 0 && v.r.w >= 1 && v.r.h >= 1 && v.r.x + v.r.w <= W &&
            v.r.y + v.r.h <= H && v.r.x % hs == 0 && v.r.y % vs == 0 &&
            // (the whole frame is taken as it is, odd sizes included)
            (rect_is_none(v.in) || (v.r.w % hs == 0 && v.r.h % vs == 0)),
        "%s %dx%d: (%d, %d, %d, %d) resolved to (%d, %d, %d, %d)", fmt.name, W, H, v.in.x, v.in.y,
        v.in.w, v.in.h, v.r.x, v.r.y, v.r.w, v.r.h);
  v.m = mcu_rect(g, v.r);
  // the MCU rectangle is the one the rectangle's corners fall in
  CHECK(v.m.mx0 * mw8 <= v.r.x && v.r.x < (v.m.mx0 + 1) * mw8 &&
            (v.m.mx0 + v.m.mw - 1) * mw8 <= v.r.x + v.r.w - 1 &&
            v.r.x + v.r.w - 1 < (v.m.mx0 + v.m.mw) * mw8 && v.m.my0 * mh8 <= v.r.y &&
            v.r.y < (v.m.my0 + 1) * mh8 && (v.m.my0 + v.m.mh - 1) * mh8 <= v.r.y + v.r.h - 1 &&
            v.r.y + v.r.h - 1 < (v.m.my0 + v.m.mh) * mh8,
        "%s: MCU rectangle of (%d, %d, %d, %d)", fmt.name, v.r.x, v.r.y, v.r.w, v.r.h);
  return true;
}

bool sweep_frame(const Format& fmt, const Frame& f) {
  const Grid g = grid_of(f);
  int hsub, vsub;
  CHECK(chroma_shifts(f, &hsub, &vsub) == hj::kOk, "%s: chroma shifts", fmt.name);
  const int hs = 1 << hsub, mw8 = 8 * g.hmax, mh8 = 8 * g.vmax;
  // axis candidates: (origin, size), on and off the grids, clamped and centred
  const int W = f.width, H = f.height;
  const int xs[][2] = {{0, W}, {1, W / 2 + 1}, {mw8 - 1, 2}, {mw8, mw8}, {W - 1, 1}, {kCenter, hs}};
  const int ys[][2] = {{0, H}, {1, H / 2 + 1}, {mh8 - 1, 2}, {H - 1, 1}};
  std::vector<View> cand;
  for (const auto& x : xs)
    for (const auto& y : ys) {
      if (&x == &xs[0] && &y == &ys[0]) {
        cand.push_back({{0, 0, 0, 0}, {}, 0, {}});  // the whole frame
        continue;
      }
      cand.push_back({{x[0], y[0], x[1], y[1]}, {}, 0, {}});
    }
  cand.push_back({{0, 0, W + hs, 1}, {}, 0, {}});  // wider than the frame: does not resolve
  bool refused = false;
  for (View& v : cand)
    if (!resolve_view(fmt, f, g, v, &refused)) return false;
  CHECK(refused, "no candidate was refused");
  const View* set[3];
  if (!check_set(f, g, set, 0)) return false;  // an image without views
  const int n = (int)cand.size();
  for (int a = 0; a < n; a++) {
    set[0] = &cand[a];
    if (!check_set(f, g, set, 1)) return false;
    for (int b = a + 1; b < n; b++) {
      set[1] = &cand[b];
      if (!check_set(f, g, set, 2)) return false;
      for (int c = b + 1; c < n; c++) {
        set[2] = &cand[c];
        if (!check_set(f, g, set, 3)) return false;
      }
    }
  }
  return true;
}

// Frames at the format's limit: one side of 65535 pixels (and 32768, where a
// 16-bit sign would first matter), the other 1, 8 or 17.  Rectangles whose
// origin lies within 16 samples of the far end, of sizes on and off the grids
// (resolve clamps them into the frame), alone and together with one at the near
// end and the whole frame: the same properties as above.
bool sweep_far_end(const Format& fmt, int W, int H) {
  Frame f{};
  f.ncomp = fmt.ncomp;
  for (int c = 0; c < fmt.ncomp; c++) f.h_samp[c] = f.v_samp[c] = 1;
  f.h_samp[0] = fmt.h0;
  f.v_samp[0] = fmt.v0;
  f.width = W;
  f.height = H;
  const Grid g = grid_of(f);
  CHECK((int64_t)g.mcux * g.mcuy * g.bpm < (1 << 24), "%s %dx%d: too many blocks", fmt.name, W, H);
  const bool wide = W > H;
  const int L = wide ? W : H, S = wide ? H : W;
  const int sizes[] = {1, 2, 3, 8, 16, 17, 64};
  View near{wide ? Rect{0, 0, 64, S} : Rect{0, 0, S, 64}, {}, 0, {}};
  View whole{{0, 0, 0, 0}, {}, 0, {}};
  bool refused = false, accepted = false;
  if (!resolve_view(fmt, f, g, near, &refused) || !resolve_view(fmt, f, g, whole, &refused))
    return false;
  for (int back = 1; back <= 16; back++)
    for (int n : sizes)
      for (int across : {1, S}) {
        View v{wide ? Rect{L - back, 0, n, across} : Rect{0, L - back, across, n}, {}, 0, {}};
        if (!resolve_view(fmt, f, g, v, &refused)) return false;
        if (!v.rc) {
          accepted = true;
          CHECK((wide ? v.r.x + v.r.w : v.r.y + v.r.h) <= L && (wide ? v.r.x : v.r.y) >= L - 16 - n - 8,
                "%s %dx%d: (%d, %d, %d, %d) moved away from the far end", fmt.name, W, H, v.r.x,
                v.r.y, v.r.w, v.r.h);
        }
        const View* set[3] = {&v, &near, &whole};
        for (int k = 1; k <= 3; k++)
          if (!check_set(f, g, set, k)) return false;
      }
  // (a short side under the chroma ratio holds no rectangle but the whole frame)
  int hsub, vsub;
  CHECK(chroma_shifts(f, &hsub, &vsub) == hj::kOk, "%s: chroma shifts", fmt.name);
  CHECK(accepted == (S >= 1 << (wide ? vsub : hsub)), "%s %dx%d: far-end rectangles resolved: %d",
        fmt.name, W, H, (int)accepted);
  return true;
}

bool sweep_slices() {
  for (int n = 1; n <= 5; n++)
    for (int ngroups = 1; ngroups <= kMaxGroups; ngroups++)
      for (int code = 0; code < 81; code++) {  // 1..3 views per group
        int32_t nviews[kMaxGroups];
        int total = n;
        for (int g = 0, k = code; g < ngroups; g++, k /= 3) total += nviews[g] = 1 + k % 3;
        Slice s[kMaxGroups];
        CHECK(group_slices(n, nviews, ngroups, s) == total, "group_slices: total");
        std::vector<int> owner((size_t)total, -1);
        for (int i = 0; i < n; i++) owner[(size_t)i] = -2;  // the images'
        for (int g = 0; g < ngroups; g++) {
          CHECK(s[g].count == nviews[g] && s[g].first >= n && s[g].first + s[g].count <= total,
                "group %d: slice [%d, +%d) of %d", g, s[g].first, s[g].count, total);
          CHECK(g == 0 || s[g].first == s[g - 1].first + s[g - 1].count, "group %d: not in order", g);
          for (int k = 0; k < s[g].count; k++) {
            CHECK(owner[(size_t)(s[g].first + k)] == -1, "descriptor %d taken twice", s[g].first + k);
            owner[(size_t)(s[g].first + k)] = g;
          }
        }
        for (int i = 0; i < total; i++) CHECK(owner[(size_t)i] != -1, "descriptor %d unowned", i);
      }
  return true;
}

}  // namespace

int main() {
  for (const Format& fmt : kFormats)
    for (int mcux = 1; mcux <= 5; mcux++)
      for (int mcuy = 1; mcuy <= 4; mcuy++)
        for (int partial = 0; partial < 4; partial++)
          if (!sweep_frame(fmt, frame(fmt, mcux, mcuy, partial & 1, partial & 2))) return 1;
  if (!sweep_slices()) return 1;
  printf("sets %ld checks %ld\n", g_sets, g_checks);
  g_sets = g_checks = 0;
  for (const Format& fmt : kFormats)
    for (int L : {32768, 65500, 65535})
      for (int S : {1, 8, 17})
        if (!sweep_far_end(fmt, L, S) || !sweep_far_end(fmt, S, L)) return 1;
  printf("far-end sets %ld checks %ld\n", g_sets, g_checks);
  return 0;
}
