// items_orient_sweep.cpp -- stand-alone, self-checking sweep of what the
// orienting instantiation of resample_items_kernel takes from the host
// (spdl_amd/csrc/hj_resample.h, hj_common.h rs::stored_rect): an item's record
// for each of the eight codes, and per tile and strip the producer's walk
// restated -- the stored rectangle under the strip, its 8 x 2 units, every
// pixel's displayed place.  Built and run by tests/test_items_orient.py with
// hj_resample.cpp under the sanitizers.  Prints one line per failed
// expectation and a count; exit status 1 when any failed.
#include "../../spdl_amd/csrc/hj_resample.h"

#include <stdio.h>

#include <vector>

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

// One strip of displayed rows [Y0, Y1) x columns [X0, X1) of an item with
// `code` over a stored W x H frame: every pixel of the rectangle is produced
// exactly once, by a unit the producer may read
void check_strip(int code, int W, int H, int dw, int dh, int X0, int X1, int Y0, int Y1) {
  EXPECT(X0 >= 0 && X0 < X1 && X1 <= dw && Y0 >= 0 && Y0 < Y1 && Y1 <= dh,
         "code %d: [%d, %d) x [%d, %d) of %dx%d", code, X0, X1, Y0, Y1, dw, dh);
  const rs::StoredRect sr = rs::stored_rect(code, dw, dh, X0, X1, Y0, Y1);
  const int ux0 = sr.x0 >> 3, units_x = ((sr.x1 + 7) >> 3) - ux0;
  const int uy0 = sr.y0 >> 1, units_y = ((sr.y1 + 1) >> 1) - uy0;
  std::vector<int> hit((size_t)(X1 - X0) * (Y1 - Y0), 0);
  int outside = 0;
  for (int uy = 0; uy < units_y; uy++)
    for (int ux = 0; ux < units_x; ux++) {
      const int x0 = (ux0 + ux) * 8, y0 = (uy0 + uy) * 2;
      // (turbo_samples' unit: a multiple of 8 below the width, even and below the height)
      EXPECT(x0 >= 0 && x0 < W && y0 >= 0 && y0 < H, "code %d: unit (%d, %d) of %dx%d", code, x0, y0,
             W, H);
      for (int j = 0; j < 2; j++)
        for (int k = 0; k < 8; k++) {
          if (x0 + k < sr.x0 || x0 + k >= sr.x1 || y0 + j < sr.y0 || y0 + j >= sr.y1) continue;
          const int dx = rs::displayed_x(code, dw, x0 + k, y0 + j);
          const int dy = rs::displayed_y(code, dh, x0 + k, y0 + j);
          if (dx < X0 || dx >= X1 || dy < Y0 || dy >= Y1) outside++;
          else hit[(size_t)(dy - Y0) * (X1 - X0) + dx - X0]++;
        }
    }
  int wrong = outside;
  for (int h : hit) wrong += h != 1;
  EXPECT(wrong == 0, "code %d: %d pixels of [%d, %d) x [%d, %d) not produced once", code, wrong, X0,
         X1, Y0, Y1);
}

void check_item(rs::AxisCache& cache, int filter, double gap, int W, int H,
                const spdl_hj_resample_items_item& it) {
  int reduces = 0;
  const int rc = rs::probe_item(filter, gap, &it, W, H, &reduces);
  if (rc) return;
  const bool sum = reduces != 0;
  std::vector<int32_t> tables;
  ResamplePool pool;
  rs::ItemDesc rec{};
  int bands = 0, chunks = 0;
  if (rs::place_item_into(&cache, filter, gap, &it, W, H, sum, tables, pool, &rec, &bands, &chunks))
    return;
  const rs::ResampleDesc& d = rec.rd;
  const int dw = it.orient & 4 ? H : W, dh = it.orient & 4 ? W : H;
  EXPECT(rec.orient == it.orient && rec.dw == dw && rec.dh == dh, "code %d: record %d, %dx%d",
         it.orient, rec.orient, rec.dw, rec.dh);
  const int words = sum ? rs::reduce_lds_words(d) : rs::lds_layout(d).words;
  EXPECT((d.pitch & 1) && words * 4 <= rs::kLdsBudget, "pitch %d, LDS %d bytes", d.pitch, words * 4);
  const int ax = sum || it.orient ? 1 : 8, ay = sum || it.orient ? 1 : 2;
  for (int ty = 0; ty < bands; ty++)
    for (int tx = 0; tx < chunks; tx++) {
      const rs::Window wc = rs::tile_window(tables.data() + d.hx, tables.data() + d.hn, d.bx, d.ox,
                                            it.out_w, d.tw, tx, ax);
      const rs::Window wr = rs::tile_window(tables.data() + d.vx, tables.data() + d.vn, d.by, d.oy,
                                            it.out_h, d.th, ty, ay);
      EXPECT(wc.hi - wc.lo <= d.pitch && wr.hi - wr.lo <= d.rows, "window %d x %d, held %d x %d",
             wc.hi - wc.lo, wr.hi - wr.lo, d.pitch, d.rows);
      for (int s0 = wr.lo; s0 < wr.hi; s0 += d.sr) {
        const int srows = s0 + d.sr < wr.hi ? d.sr : wr.hi - s0;
        if (!sum) {  // (rs_produce_oriented: the strip is the frame's pixels; aligned items
                     // of such a submission produce up to the window's end alone)
          check_strip(it.orient, W, H, dw, dh, wc.lo, wc.hi, s0, s0 + srows);
          continue;
        }
        // (rs_strips_sum: the pixels under the strip's cells, clipped to the safe box)
        const rs::ReduceDesc& r = rec.rr;
        const int X1 = r.qx + wc.hi * r.fx, Y1 = r.qy + (s0 + srows) * r.fy;
        check_strip(it.orient, W, H, dw, dh, r.qx + wc.lo * r.fx, X1 < r.qx + r.qw ? X1 : r.qx + r.qw,
                    r.qy + s0 * r.fy, Y1 < r.qy + r.qh ? Y1 : r.qy + r.qh);
      }
    }
}

}  // namespace

int main() {
  rs::AxisCache cache;
  static const int sizes[] = {1, 2, 3, 5, 8, 9, 17, 64, 131, 300};
  for (int code = 0; code < 8; code++)
    for (int W : sizes)
      for (int H : {1, 3, 16, 67, 301}) {
        const int dw = code & 4 ? H : W, dh = code & 4 ? W : H;
        for (int ow : {1, 7, 40, 150}) {
          spdl_hj_resample_items_item it{};
          it.orient = code;
          it.out_w = ow;
          it.out_h = (ow * 3 + 3) / 4;
          it.rw = it.out_w;
          it.rh = it.out_h;
          // the whole displayed frame, unclamped, without and with factors
          check_item(cache, SPDL_HJ_FILTER_BILINEAR, 0.0, W, H, it);
          check_item(cache, SPDL_HJ_FILTER_LANCZOS, 1.0, W, H, it);
          if (dw < 9 || dh < 9) continue;
          // an odd clamped box and a window inside a larger resized picture
          it.clamp = 1;
          it.x0 = 3, it.y0 = 2, it.x1 = dw - 2, it.y1 = dh - 3;
          it.rw = it.out_w + 5, it.rh = it.out_h + 2, it.ox = 4, it.oy = 1;
          check_item(cache, SPDL_HJ_FILTER_BICUBIC, 0.0, W, H, it);
          check_item(cache, SPDL_HJ_FILTER_BILINEAR, 1.5, W, H, it);
        }
      }
  // the displayed frame decides a clamped box: 40 x 20 fits 50 x 30 stored as it is,
  // not turned; a code above 7 fails the request
  spdl_hj_resample_items_item it{};
  it.clamp = 1, it.x1 = 40, it.y1 = 20, it.out_w = it.rw = 8, it.out_h = it.rh = 8;
  int any = 0;
  EXPECT(rs::probe_item(0, 0.0, &it, 50, 30, &any) == SPDL_HJ_OK, "code 0");
  it.orient = 5;
  EXPECT(rs::probe_item(0, 0.0, &it, 50, 30, &any) == SPDL_HJ_ERR_BAD_GEOMETRY, "code 5");
  it.orient = 8;
  EXPECT(rs::probe_item(0, 0.0, &it, 50, 30, &any) == SPDL_HJ_ERR_INVALID_ARG, "code 8");
  printf("%d checks, %d failed expectations\n", checks, failures);
  return failures != 0;
}
