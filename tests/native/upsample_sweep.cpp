// upsample_sweep.cpp -- stand-alone, self-checking sweep of the csc = TURBO
// row functions (spdl_amd/csrc/hj_upsample.h), for a sanitizer build on the CPU:
//   g++ -std=c++17 -O1 -g -DHJ_HD= -fsanitize=address,undefined -fno-sanitize-recover=all
//       -static-libasan -static-libubsan tests/native/upsample_sweep.cpp -o upsample_sweep
// Every plane of cw = 1..20 columns and ch = 1..6 rows, under every ratio the
// decoder can meet, holds random bytes in an allocation of exactly stride x ch
// bytes (stride: cw rounded up to 8, as the IDCT lays planes out), so a load
// outside it is the sanitizer's to report.  hj::up::run8x2 is held against a
// per-pixel restatement of the rules (include/spdl_hipjpeg.h "Pillow-exact
// decode") that reads single samples and checks every one of them to lie in
// [0, cw) x [0, ch); and each run is made twice, with other bytes in the
// padding columns, and must not change.  The colour conversion is held
// against floor divisions.  Prints one line per failed expectation and a
// count; exit status 1 when any failed.
#include "../../spdl_amd/csrc/hj_upsample.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

namespace {

using namespace hj;

int failures = 0;
long checks = 0;

#define EXPECT(cond, ...)            \
  do {                               \
    checks++;                        \
    if (!(cond)) {                   \
      if (failures++ < 40) {         \
        printf("FAIL %s: ", #cond);  \
        printf(__VA_ARGS__);         \
        printf("\n");                \
      }                              \
    }                                \
  } while (0)

uint32_t rng_state = 12345;
uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

struct Plane {
  const uint8_t* p;
  int stride, cw, ch;
  int at(int x, int y) const {  // one true sample, edge-clamped by the caller
    if (x < 0 || x >= cw || y < 0 || y >= ch) {
      if (failures++ < 40) printf("FAIL the restatement read (%d, %d) of %dx%d\n", x, y, cw, ch);
      return 0;
    }
    return p[(size_t)y * stride + x];
  }
  int clamped(int x, int y) const {
    x = x < 0 ? 0 : x >= cw ? cw - 1 : x;
    y = y < 0 ? 0 : y >= ch ? ch - 1 : y;
    return at(x, y);
  }
};

// Output sample (x, y) of a component of ratio (hr, vr), from the rules
int naive(const Plane& pl, int hr, int vr, int x, int y) {
  const int cw = pl.cw;
  if (hr == 1 && vr == 1) return pl.at(x, y);
  if (hr == 2 && vr == 1 && cw > 2) {
    const int i = x / 2, p = pl.at(i, y);
    if (x == 0) return p;                 // the first and last output columns are
    if (x == 2 * cw - 1) return p;        // p[0] and p[cw - 1] unchanged
    return x % 2 == 0 ? (3 * p + pl.at(i - 1, y) + 1) >> 2 : (3 * p + pl.at(i + 1, y) + 2) >> 2;
  }
  if (hr == 1 && vr == 2) {
    const int j = y / 2, p = pl.at(x, j);
    return y % 2 == 0 ? (3 * p + pl.clamped(x, j - 1) + 1) >> 2
                      : (3 * p + pl.clamped(x, j + 1) + 2) >> 2;
  }
  if (hr == 2 && vr == 2 && cw > 2) {
    const int i = x / 2, j = y / 2, jn = y % 2 == 0 ? j - 1 : j + 1;
    auto s = [&](int c) { return 3 * pl.at(c, j) + pl.clamped(c, jn); };
    if (x == 0) return (4 * s(0) + 8) >> 4;
    if (x == 2 * cw - 1) return (4 * s(cw - 1) + 7) >> 4;
    return x % 2 == 0 ? (3 * s(i) + s(i - 1) + 8) >> 4 : (3 * s(i) + s(i + 1) + 7) >> 4;
  }
  return pl.at(x / hr, y / vr);
}

void sweep_plane(int cw, int ch, int hr, int vr) {
  const int stride = (cw + 7) / 8 * 8;
  const size_t bytes = (size_t)stride * ch;
  uint8_t* buf = static_cast<uint8_t*>(malloc(bytes));  // (exactly the plane: no slack)
  for (size_t i = 0; i < bytes; i++) buf[i] = (uint8_t)rnd();
  const Plane pl{buf, stride, cw, ch};
  const int mode = up::mode_of(hr, vr, cw);
  // every frame size with this plane: ceil(W / hr) == cw, ceil(H / vr) == ch
  for (int W = (cw - 1) * hr + 1; W <= cw * hr; W++)
    for (int H = (ch - 1) * vr + 1; H <= ch * vr; H++) {
      std::vector<int> first;
      for (int pass = 0; pass < 2; pass++) {
        if (pass)  // other bytes behind the true columns
          for (int y = 0; y < ch; y++)
            for (int x = cw; x < stride; x++) buf[(size_t)y * stride + x] ^= (uint8_t)(1 + rnd() % 255);
        size_t at = 0;
        for (int y0 = 0; y0 < H; y0 += 2)
          for (int x0 = 0; x0 < W; x0 += 8) {
            int r0[8], r1[8];
            up::run8x2(buf, stride, cw, ch, mode, hr, vr, x0, y0, r0, r1);
            for (int r = 0; r < 2 && y0 + r < H; r++)
              for (int k = 0; k < 8 && x0 + k < W; k++) {
                const int got = r ? r1[k] : r0[k];
                if (!pass) {
                  const int want = naive(pl, hr, vr, x0 + k, y0 + r);
                  EXPECT(got == want, "(%d,%d) plane %dx%d frame %dx%d at (%d,%d): %d want %d", hr,
                         vr, cw, ch, W, H, x0 + k, y0 + r, got, want);
                  first.push_back(got);
                } else {
                  EXPECT(got == first[at], "(%d,%d) plane %dx%d frame %dx%d at (%d,%d) depends on "
                         "the padding: %d then %d", hr, vr, cw, ch, W, H, x0 + k, y0 + r, first[at],
                         got);
                  at++;
                }
              }
          }
      }
    }
  free(buf);
}

void sweep_colour() {
  auto fdiv = [](long long a) { return (int)((a >= 0 ? a : a - 65535) / 65536); };  // floor
  auto clip = [](int v) { return v < 0 ? 0 : v > 255 ? 255 : v; };
  for (int y = 0; y < 256; y += 5)
    for (int cb = 0; cb < 256; cb++)
      for (int cr = 0; cr < 256; cr++) {
        int rgb[3];
        up::ycc_rgb(y, cb, cr, rgb);
        const long long b = cb - 128, r = cr - 128;
        const int wr = clip(y + fdiv(91881 * r + 32768));
        const int wg = clip(y + fdiv(-22554 * b + 32768 - 46802 * r));
        const int wb = clip(y + fdiv(116130 * b + 32768));
        EXPECT(rgb[0] == wr && rgb[1] == wg && rgb[2] == wb, "ycc (%d,%d,%d): %d %d %d want %d %d %d",
               y, cb, cr, rgb[0], rgb[1], rgb[2], wr, wg, wb);
      }
}

}  // namespace

int main() {
  const int ratios[][2] = {{1, 1}, {2, 1}, {1, 2}, {2, 2}, {4, 1}, {4, 2}, {1, 4}, {3, 1}, {2, 4},
                           {4, 4}, {1, 3}};
  for (const auto& r : ratios)
    for (int cw = 1; cw <= 20; cw++)
      for (int ch = 1; ch <= 6; ch++) sweep_plane(cw, ch, r[0], r[1]);
  // the modes: the triangle rules with a horizontal part need three columns
  EXPECT(up::mode_of(2, 1, 2) == up::kBox && up::mode_of(2, 1, 3) == up::kH2V1, "h2v1 threshold");
  EXPECT(up::mode_of(2, 2, 2) == up::kBox && up::mode_of(2, 2, 3) == up::kH2V2, "h2v2 threshold");
  EXPECT(up::mode_of(1, 2, 1) == up::kH1V2 && up::mode_of(1, 1, 1) == up::kCopy, "h1v2, copy");
  EXPECT(up::mode_of(4, 1, 9) == up::kBox && up::mode_of(1, 4, 9) == up::kBox, "other ratios");
  sweep_colour();
  printf("%ld checks, %d failed expectations\n", checks, failures);
  return failures ? 1 : 0;
}
