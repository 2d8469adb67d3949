// draft_sweep.cpp -- stand-alone, self-checking sweep of the Pillow-exact draft
// (spdl_hj_set_draft) for a sanitizer build on the CPU (tests/test_draft.py):
// hj_idct.h draft_idct4 / 2 / 1 against a 64-bit restatement of the rule WITH
// the source's zero-column shortcut (random operand sets, every zero pattern of
// a column's AC operands, the int16 ends), and the planner's per-component
// sizes, planes, strides, windows and lanes against the rule of
// include/spdl_hipjpeg.h "Pillow-exact draft".  Exit status 1 on a failure.
#include "../../spdl_amd/csrc/hj_idct.h"
#include "../../spdl_amd/csrc/hj_layout.h"

#include <stdio.h>
#include <string.h>

#include <random>

using namespace hj;

static int failures = 0;
#define EXPECT(cond, ...)             \
  do {                                \
    if (!(cond) && failures++ < 40) { \
      printf("FAIL %s: ", #cond);     \
      printf(__VA_ARGS__);            \
      printf("\n");                   \
    }                                 \
  } while (0)

static int64_t fix(double x) { return (int64_t)(x * 8192 + 0.5); }
static int64_t descale(int64_t x, int n) { return (x + ((int64_t)1 << (n - 1))) >> n; }
static int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
static int limit(int64_t v) {  // libjpeg's range-limit table behind the +128
  const int i = (int)(v & 1023);
  return i < 128 ? i + 128 : i < 512 ? 255 : i < 896 ? 0 : i - 896;
}

// N = 7: r0 r1 r2 r3 r5 r6 r7 -> 4 outputs; N = 5: r0 r1 r3 r5 r7 -> 2 outputs
template <int N>
static void pass(const int64_t* r, int s, bool shortcut, int64_t* o) {
  bool ac = false;
  for (int i = 1; i < N; i++) ac = ac || r[i];
  if (shortcut && !ac) {  // (pass 1 alone: the DC scaled by PASS1_BITS)
    for (int k = 0; k < (N == 7 ? 4 : 2); k++) o[k] = r[0] * 4;
  } else if (N == 7) {
    const int64_t t0 = r[0] * 16384, t2 = r[2] * fix(1.847759065) - r[5] * fix(0.765366865);
    const int64_t a = -r[6] * fix(0.211164243) + r[4] * fix(1.451774981) - r[3] * fix(2.172734803) +
                      r[1] * fix(1.061594337);
    const int64_t c = -r[6] * fix(0.509795579) - r[4] * fix(0.601344887) + r[3] * fix(0.899976223) +
                      r[1] * fix(2.562915447);
    o[0] = descale(t0 + t2 + c, s), o[1] = descale(t0 - t2 + a, s);
    o[2] = descale(t0 - t2 - a, s), o[3] = descale(t0 + t2 - c, s);
  } else {
    const int64_t t0 = -r[4] * fix(0.720959822) + r[3] * fix(0.850430095) - r[2] * fix(1.272758580) +
                       r[1] * fix(3.624509785);
    o[0] = descale(r[0] * 32768 + t0, s), o[1] = descale(r[0] * 32768 - t0, s);
  }
}

template <int N>
static void check(const int32_t* b) {
  constexpr int P = N == 7 ? 4 : 2;
  int64_t ws[P][N], col[N], t[P];
  for (int c = 0; c < N; c++) {
    for (int r = 0; r < N; r++) col[r] = b[r * N + c];
    pass<N>(col, N == 7 ? 12 : 13, true, t);
    for (int k = 0; k < P; k++) ws[k][c] = t[k];
  }
  int32_t got[P * P];
  if (N == 7) draft_idct4(b, got, P);
  else draft_idct2(b, got, P);
  for (int k = 0; k < P; k++) {
    pass<N>(ws[k], N == 7 ? 19 : 20, false, t);
    for (int x = 0; x < P; x++)
      EXPECT(got[k * P + x] == limit(t[x]), "N %d (%d, %d): %d", N, k, x, got[k * P + x]);
  }
}

template <int N>
static void transforms() {
  std::mt19937 rng(2022 + N);
  int32_t b[N * N];
  for (int it = 0; it < 100000; it++) {  // random sets, sparse half the time
    const int amp = it % 3 == 0 ? 2040 : 300;
    for (int i = 0; i < N * N; i++)
      b[i] = (it & 1) && rng() % 3 ? 0 : (int)(rng() % (2 * amp + 1)) - amp;
    b[0] = (int)(rng() % 16321) - 8160;
    check<N>(b);
  }
  for (int m = 0; m < (1 << (N - 1)); m++)  // every zero pattern of a column's AC operands
    for (int c = 0; c < N; c++) {
      memset(b, 0, sizeof(b));
      b[0] = 37, b[c] = c ? -211 : 37;
      for (int r = 1; r < N; r++) b[r * N + c] = (m >> (r - 1)) & 1 ? 97 * r - 300 : 0;
      check<N>(b);
    }
  for (int v : {-32768, -8160, -1, 0, 1, 8160, 32767})  // the int16 ends, one operand at a time
    for (int i = 0; i < N * N; i++) {
      memset(b, 0, sizeof(b));
      b[i] = v;
      check<N>(b);
      EXPECT(draft_idct1(v) == limit(descale(v, 3)), "1x1 of %d", v);
    }
}

static void planner() {
  const int sizes[] = {1, 7, 8, 9, 17, 61, 83, 4000};
  const int samp[][2] = {{1, 1}, {2, 1}, {2, 2}, {1, 2}, {4, 1}, {4, 2}};
  for (int w : sizes)
    for (int h : sizes)
      for (int ncomp : {1, 3})
        for (const auto& s : samp)
          for (int lv = 0; lv < 4 && !failures; lv++) {
            if (ncomp == 1 && s[0] * s[1] != 1) continue;
            spdl_hj_image_info p{};
            p.width = w, p.height = h, p.ncomp = ncomp;
            for (int c = 0; c < ncomp; c++) p.h_samp[c] = p.v_samp[c] = 1;
            p.h_samp[0] = s[0], p.v_samp[0] = s[1];
            p.color = ncomp == 1 ? SPDL_HJ_COLOR_GRAY : SPDL_HJ_COLOR_YCBCR;
            spdl_hj_output o{};
            o.csc = SPDL_HJ_CSC_TURBO;
            const int64_t off = 0, size = 1000;
            const uint8_t level = (uint8_t)lv;
            PlanCache cache;
            Layout L, L0;
            LayoutRequest rq{&off, &size, &p, 1, &o, 0, &cache};
            EXPECT(build_layout(rq, L0).rc == 0, "plain plan");
            rq.draft = &level, rq.ndraft = 1;
            EXPECT(build_layout(rq, L).rc == 0, "%dx%d L%d", w, h, lv);
            if (failures) return;
            const ImageDesc& d = L.desc[0];
            if (lv == 0) {  // the submission without the call
              EXPECT(L.draft.empty() && !memcmp(&d, &L0.desc[0], sizeof(d)) &&
                         L.total_planes == L0.total_planes && L.idct_wgs == L0.idct_wgs,
                     "level 0 differs");
              continue;
            }
            const int P = 8 >> lv, hmax = s[0], vmax = s[1];
            const int64_t mcux = cdiv(w, 8 * hmax), mcuy = cdiv(h, 8 * vmax);
            EXPECT(d.ow == cdiv((int64_t)w * P, 8) && d.oh == cdiv((int64_t)h * P, 8), "frame");
            int64_t lanes = 0, total = 0;
            for (int c = 0; c < ncomp; c++) {
              const int hc = p.h_samp[c], vc = p.v_samp[c];
              int pc = P;  // (the rule by trial: doubled while both ratios stay whole)
              while (pc < 8 && (hmax * P) % (hc * pc * 2) == 0 && (vmax * P) % (vc * pc * 2) == 0)
                pc *= 2;
              const draft::Desc& r = L.draft[0];
              const int64_t bw = mcux * hc, bh = mcuy * vc;
              EXPECT(r.level == lv && r.pc[c] == pc && r.hr[c] * hc * pc == hmax * P &&
                         r.vr[c] * vc * pc == vmax * P,
                     "c%d record %d %d %d", c, r.pc[c], r.hr[c], r.vr[c]);
              EXPECT(d.win_w[c] == cdiv((int64_t)w * hc * pc, 8 * hmax) && !d.win_x[c] && !d.win_y[c] &&
                         d.win_h[c] == cdiv((int64_t)h * vc * pc, 8 * vmax) &&
                         (int64_t)d.win_w[c] * r.hr[c] >= d.ow && (int64_t)d.win_h[c] * r.vr[c] >= d.oh,
                     "c%d window %dx%d", c, d.win_w[c], d.win_h[c]);
              EXPECT(d.plane_stride[c] == 8 * cdiv(bw * pc, 8) && d.plane_stride[c] >= d.win_w[c] &&
                         bh * pc >= d.win_h[c] && d.plane_off[c] == total,
                     "c%d stride %d", c, d.plane_stride[c]);
              total += cdiv(d.plane_stride[c] * bh * pc, 256) * 256;
              lanes += cdiv(bw * pc, 8) * bh;
            }
            EXPECT(L.total_planes == total && d.idct_blocks == lanes && L.draft_images == 1 &&
                       L.idct_wgs == cdiv(lanes, kIdctThreads),
                   "totals: planes %lld lanes %d", (long long)L.total_planes, d.idct_blocks);
          }
}

int main() {
  transforms<7>();
  transforms<5>();
  planner();
  printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
