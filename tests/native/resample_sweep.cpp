// resample_sweep.cpp -- stand-alone, self-checking sweep of the Pillow-exact
// resize's tiler (spdl_amd/csrc/hj_resample.h) for a sanitizer build on the CPU,
// built and run by tests/test_resample.py with hj_resample.cpp.  Sizes 1..300
// into 1..300 per axis, on a stride, with and without a box and a window, and
// the tap limit.  Prints one line per failed expectation and a count; exit
// status 1 when any failed.
#include "../../spdl_amd/csrc/hj_resample.h"

#include <stdio.h>

namespace {

using namespace hj;

int failures = 0, checks = 0;

#define EXPECT(cond, ...)                   \
  do {                                      \
    checks++;                               \
    if (!(cond) && failures++ < 40) {       \
      printf("FAIL %s: ", #cond);           \
      printf(__VA_ARGS__);                  \
      printf("\n");                         \
    }                                       \
  } while (0)

int taps_bound(int in, int out, int filter) {
  const double s = filter == SPDL_HJ_FILTER_BILINEAR ? 1 : filter == SPDL_HJ_FILTER_BICUBIC ? 2 : 3;
  const double scale = (double)in / out;
  const int span = (int)(2 * s * (scale > 1 ? scale : 1)) + 2;
  return in < span ? in : span;
}

void check_tiling(rs::AxisCache& cache, int filter, int W, int H, const spdl_hj_resample_item& it,
                  int ow, int oh) {
  rs::Placed p{};
  const int rc = rs::place(cache, filter, &it, W, H, ow, oh, &p);
  const int bx = it.box.w ? it.box.x : 0, by = it.box.w ? it.box.y : 0;
  const int bw = it.box.w ? it.box.w : W, bh = it.box.w ? it.box.h : H;
  // (taps <= min(samples, 2 support + 2): under the limit it tiles, over it nothing is laid out)
  const bool fits = taps_bound(bw, it.rw ? it.rw : ow, filter) <= 256 &&
                    taps_bound(bh, it.rh ? it.rh : oh, filter) <= 256;
  EXPECT(rc == SPDL_HJ_OK || (!fits && rc == SPDL_HJ_ERR_BAD_GEOMETRY && p.d.tw == 0 && !p.bands),
         "%dx%d -> %dx%d filter %d: rc %d", W, H, ow, oh, filter, rc);
  if (rc) return;
  const rs::ResampleDesc& d = p.d;
  EXPECT(d.tw >= 8 && d.tw % 8 == 0 && d.th >= 1 && d.sr >= 2 && (d.sr & (d.sr - 1)) == 0 &&
             (d.pitch & 1),
         "tile %dx%d strip %d pitch %d", d.tw, d.th, d.sr, d.pitch);
  EXPECT(rs::lds_layout(d).words * 4 <= 64 * 1024, "LDS %d bytes", rs::lds_layout(d).words * 4);
  EXPECT(p.chunks == (ow + d.tw - 1) / d.tw && p.bands == (oh + d.th - 1) / d.th,
         "%d x %d tiles of %dx%d for %dx%d", p.chunks, p.bands, d.tw, d.th, ow, oh);
  // per axis: windows inside the box and held by LDS, outputs inside their window, covered once
  auto axis = [&](const rs::Axis& A, int b0, int bsz, int o0, int on, int tile, int tiles, int align,
                  int held, int ksize) {
    int covered = 0;
    for (int t = 0; t < tiles; t++) {
      const rs::Window w = rs::tile_window(A.xmin(), A.n(), b0, o0, on, tile, t, align);
      EXPECT(w.lo % align == 0 && w.lo > b0 - align && w.lo >= 0 && w.hi <= b0 + bsz && w.hi > w.lo &&
                 ((w.hi - w.lo + align - 1) & ~(align - 1)) <= held,
             "align %d: [%d, %d) of box [%d, %d), %d held", align, w.lo, w.hi, b0, b0 + bsz, held);
      for (int x = t * tile; x < on && x < (t + 1) * tile; x++, covered++) {
        const int lo = b0 + A.xmin()[o0 + x], n = A.n()[o0 + x];
        EXPECT(lo >= w.lo && lo + n <= w.hi && n <= ksize, "output %d reads outside its window", x);
      }
    }
    EXPECT(covered == on, "align %d: covered %d of %d", align, covered, on);
  };
  axis(*p.H, bx, bw, it.ox, ow, d.tw, p.chunks, 8, d.pitch, d.kh);
  axis(*p.V, by, bh, it.oy, oh, d.th, p.bands, 2, d.rows + 1, d.kv);
}

}  // namespace

int main() {
  rs::AxisCache cache;
  static const int sizes[] = {1, 2, 3, 7, 8, 9, 16, 33, 64, 65, 129, 224, 300};
  for (int filter = 0; filter < 3; filter++)
    for (int W : sizes)
      for (int H : {1, 9, 65, 300})
        for (int ow : sizes)
          for (int oh : {1, 8, 33, 300}) {
            check_tiling(cache, filter, W, H, spdl_hj_resample_item{}, ow, oh);
            if (W < 9 || H < 9) continue;
            // an odd box inside the frame, a window of a larger resized picture
            const spdl_hj_resample_item it{{3, 5, W - 4, H - 6}, ow + 9, oh + 4, 8, 3};
            check_tiling(cache, filter, W, H, it, ow, oh);
          }
  // the tap limit: 256 taps on both axes tile (lanczos 640 -> 15, bilinear at 1 / 127.5)
  check_tiling(cache, SPDL_HJ_FILTER_LANCZOS, 640, 640, spdl_hj_resample_item{}, 15, 15);
  check_tiling(cache, SPDL_HJ_FILTER_BILINEAR, 65535, 65535, spdl_hj_resample_item{}, 514, 514);
  EXPECT(rs::axis_taps(640, 15, SPDL_HJ_FILTER_LANCZOS) == 256 &&
             rs::axis_taps(640, 14, SPDL_HJ_FILTER_LANCZOS) > 256,
         "taps %d, %d", rs::axis_taps(640, 15, 2), rs::axis_taps(640, 14, 2));
  printf("%d checks, %d failed expectations\n", checks, failures);
  return failures != 0;
}
