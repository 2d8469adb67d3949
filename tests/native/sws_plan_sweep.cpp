// sws_plan_sweep.cpp -- stand-alone sweep of the host planner (hj_sws.cpp:
// sws_plan, sws_plan_planar) for a sanitizer build on the CPU:
//   g++ -std=c++17 -DHJ_HD= -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -static-libasan -static-libubsan \
//       tests/native/sws_plan_sweep.cpp spdl_amd/csrc/hj_sws.cpp -o sws_plan_sweep
// About 45 000 plans: sources and destinations from 1 pixel up, every chroma
// shift pair, the three filters.  Beside what the sanitizers see, every accepted
// plan is checked to keep its taps inside the source and its rows normalised.
// Prints "plans N refused M" and exits 0, or 1 at the first violated check.
#include <stdio.h>

#include "../../spdl_amd/csrc/hj_sws.h"

namespace {

long g_plans = 0, g_refused = 0;

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
  printf("plans %ld refused %ld\n", g_plans, g_refused);
  return g_refused > 0 && g_refused < g_plans ? 0 : 1;
}
