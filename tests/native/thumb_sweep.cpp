// thumb_sweep.cpp -- stand-alone, self-checking sweep of the reducing_gap
// resolver and resample_reduce_kernel's tiler (spdl_amd/csrc/hj_resample.h) for
// a sanitizer build on the CPU, built and run by tests/test_thumbnail.py with
// hj_resample.cpp.  Frames 1..700 into 1..300 with gaps 1, 2 and 3, whole
// frames and fractional boxes: what the kernel indexes by stays inside the
// frame, the strip and the LDS budget.  Prints one line per failed expectation
// and a count; exit status 1 when any failed.
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

void check(rs::AxisCache& cache, int filter, double gap, int W, int H,
           const spdl_hj_resample_box_item& it, int ow, int oh) {
  rs::BoxGeo g;
  int rc = rs::resolve_box(&it, W, H, ow, oh, filter, gap, &g);
  EXPECT(rc == SPDL_HJ_OK || rc == SPDL_HJ_ERR_BAD_GEOMETRY, "%dx%d -> %dx%d: rc %d", W, H, ow, oh, rc);
  if (rc) return;
  EXPECT(g.fx >= 1 && g.fy >= 1 && g.fx * g.fy <= rs::kReduceMaxCell && g.q[0] >= 0 && g.q[1] >= 0 &&
             g.q[0] < g.q[2] && g.q[1] < g.q[3] && g.q[2] <= W && g.q[3] <= H,
         "factors %dx%d safe box %d %d %d %d of %dx%d", g.fx, g.fy, g.q[0], g.q[1], g.q[2], g.q[3], W, H);
  EXPECT(g.box[0] >= 0 && g.box[1] >= 0 && g.box[0] < g.box[2] && g.box[1] < g.box[3] &&
             g.box[2] <= g.cw && g.box[3] <= g.ch,
         "box %g %g %g %g of the reduced %dx%d", g.box[0], g.box[1], g.box[2], g.box[3], g.cw, g.ch);
  for (int k = 0; k < 4; k++)
    EXPECT(g.div[k] >= 1 && g.div[k] <= g.div[0] && g.mult[k] == (1u << 24) / (uint32_t)g.div[k] &&
               (255ull * g.div[k] + g.div[k] / 2) * g.mult[k] < (1ull << 32),
           "class %d: d %d mult %u", k, g.div[k], g.mult[k]);
  std::vector<int32_t> tables;
  ResamplePool pool;
  rs::ResampleDesc d;
  rs::ReduceDesc r;
  int bands, chunks;
  rc = rs::place_box_into(&cache, filter, gap, &it, W, H, ow, oh, tables, pool, &d, &r, &bands, &chunks);
  EXPECT(rc == SPDL_HJ_OK || rc == SPDL_HJ_ERR_BAD_GEOMETRY, "place: rc %d", rc);
  if (rc) return;
  EXPECT(rs::reduce_lds_words(d) * 4 <= rs::kLdsBudget && (d.pitch & 1) && d.sr >= 2 &&
             (d.sr & (d.sr - 1)) == 0 && d.tw % 8 == 0,
         "LDS %d bytes, pitch %d, strip %d", rs::reduce_lds_words(d) * 4, d.pitch, d.sr);
  EXPECT(r.cw == g.cw && r.ch == g.ch && r.qx + r.qw <= W && r.qy + r.qh <= H, "record");
  // every tile's window: inside the reduced picture and the strip, its
  // source rectangle inside the safe box, every output's taps inside it
  for (int t = 0; t < chunks; t++) {
    const rs::Window w = rs::tile_window(tables.data() + d.hx, tables.data() + d.hn, 0, d.ox, ow, d.tw, t, 1);
    EXPECT(w.lo >= 0 && w.lo < w.hi && w.hi <= r.cw && w.hi - w.lo <= d.pitch &&
               r.qx + w.lo * r.fx < r.qx + r.qw,
           "columns [%d, %d) of %d cells, pitch %d", w.lo, w.hi, r.cw, d.pitch);
    for (int x = t * d.tw; x < ow && x < (t + 1) * d.tw; x++) {
      const int lo = tables[d.hx + d.ox + x], n = tables[d.hn + d.ox + x];
      EXPECT(lo >= w.lo && lo + n <= w.hi && n <= d.kh, "column %d reads outside its window", x);
    }
  }
  for (int t = 0; t < bands; t++) {
    const rs::Window w = rs::tile_window(tables.data() + d.vx, tables.data() + d.vn, 0, d.oy, oh, d.th, t, 1);
    EXPECT(w.lo >= 0 && w.lo < w.hi && w.hi <= r.ch && w.hi - w.lo <= d.rows,
           "rows [%d, %d) of %d cells, %d held", w.lo, w.hi, r.ch, d.rows);
    for (int y = t * d.th; y < oh && y < (t + 1) * d.th; y++) {
      const int lo = tables[d.vx + d.oy + y], n = tables[d.vn + d.oy + y];
      EXPECT(lo >= w.lo && lo + n <= w.hi && n <= d.kv, "row %d reads outside its window", y);
    }
  }
}

}  // namespace

int main() {
  rs::AxisCache cache;
  static const int frames[] = {1, 2, 9, 33, 97, 200, 333, 700}, outs[] = {1, 3, 8, 33, 65, 300};
  for (int filter = 0; filter < 3; filter++)
    for (double gap : {0.0, 1.0, 2.0, 3.0})
      for (int W : frames)
        for (int H : frames)
          for (int ow : outs)
            for (int oh : outs) {
              check(cache, filter, gap, W, H, spdl_hj_resample_box_item{}, ow, oh);
              if (W < 9 || H < 9) continue;
              // a fractional box, a window of a larger resized picture
              check(cache, filter, gap, W, H,
                    spdl_hj_resample_box_item{1.25, 2.5, W - 0.75, H - 3.0, ow + 5, oh + 2, 4, 1}, ow, oh);
            }
  rs::BoxGeo g;
  EXPECT(rs::resolve_box(nullptr, 640, 480, 8, 8, 1, 0.5, &g) == SPDL_HJ_ERR_INVALID_ARG, "gap 0.5");
  const spdl_hj_resample_box_item out_of_frame{0, 0, 641, 480, 0, 0, 0, 0};
  EXPECT(rs::resolve_box(&out_of_frame, 640, 480, 8, 8, 1, 2.0, &g) == SPDL_HJ_ERR_INVALID_ARG, "box");
  EXPECT(rs::resolve_box(nullptr, 640, 480, 10, 10, 1, 1.0, &g) == SPDL_HJ_ERR_BAD_GEOMETRY, "cap");
  EXPECT(rs::resolve_box(nullptr, 2, 300, 2, 100, 1, 0.0, &g) == SPDL_HJ_ERR_BAD_GEOMETRY, "tall");
  printf("%d checks, %d failed expectations\n", checks, failures);
  return failures != 0;
}
