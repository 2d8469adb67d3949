// idct_region_sweep.cpp -- stand-alone sweep of idct_kernel's block index over a
// source crop (hj_common.h: idct_region_block, then idct_block_pos) against
// plain / and %, for a sanitizer build on the CPU:
//   g++ -std=c++17 -O2 -DHJ_HD= -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -static-libasan -static-libubsan tests/native/idct_region_sweep.cpp -o idct_region_sweep
// For every bpm in {1, 2, 3, 4, 6, 8, 10} and MCU grid: every rectangle of the
// small grids (mcux x mcuy up to 6 x 5), and of the wide ones (41, 80, 257,
// 4096 MCUs to a row) rectangles at the corners, of one MCU, of one row, one
// column and the whole grid.  Every local index l below mw * mh * bpm must
// give the block (l % bpm) of MCU (mx0 + (l / bpm) % mw, my0 + (l / bpm) / mw):
// its index in the image's MCU order, and the component and plane position
// idct_block_pos makes of it.  Each block of the rectangle is reached once and
// no block outside it.  Prints "rects N positions P" and exits 0, or 1 at the
// first difference.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../spdl_amd/csrc/hj_common.h"

namespace {

long g_rects = 0, g_pos = 0;

// (as tests/native/idct_index_sweep.cpp) an MCU of bpm blocks: bpm - 2 luma
// blocks, then two 1x1 components; bpm 2: two 1x1 components; bpm 1: gray
void layout(hj::ImageInfo& in, int bpm) {
  in.bpm = bpm;
  if (bpm == 1) {
    in.ncomp = 1;
    in.comp_h[0] = in.comp_v[0] = 2;  // a gray frame's factors mean nothing
    return;
  }
  const int luma = bpm >= 3 ? bpm - 2 : 1;
  const int lh = luma == 8 ? 4 : luma == 4 ? 2 : luma, lv = luma / lh;
  in.ncomp = bpm >= 3 ? 3 : 2;
  in.comp_h[0] = lh;
  in.comp_v[0] = lv;
  int b = 0;
  for (int y = 0; y < lv; y++)
    for (int x = 0; x < lh; x++) {
      in.mcu_comp[b] = 0;
      in.mcu_dx[b] = x;
      in.mcu_dy[b] = y;
      b++;
    }
  for (int c = 1; c < in.ncomp; c++) {
    in.comp_h[c] = in.comp_v[c] = 1;
    in.mcu_comp[b] = c;
    in.mcu_dx[b] = in.mcu_dy[b] = 0;
    b++;
  }
}

bool rect(const hj::ImageInfo& in, int mx0, int my0, int mw, int mh) {
  const uint32_t magic = hj::idct_div_magic((uint32_t)mw);
  const uint32_t n = (uint32_t)(mw * mh * in.bpm);
  std::vector<unsigned char> seen((size_t)in.nblocks, 0);
  g_rects++;
  for (uint32_t l = 0; l < n; l++) {
    const uint32_t m = l / (uint32_t)in.bpm, b = l % (uint32_t)in.bpm;
    const int mx = mx0 + (int)(m % (uint32_t)mw), my = my0 + (int)(m / (uint32_t)mw);
    const uint32_t want = (uint32_t)((my * in.mcux + mx) * in.bpm) + b;
    const uint32_t j = hj::idct_region_block(in, mx0, my0, mw, magic, l);
    g_pos++;
    if (j != want || j >= (uint32_t)in.nblocks || seen[j]) {
      fprintf(stderr, "bpm %d mcux %d rect (%d, %d, %d, %d) l %u: block %u, plain %u\n", in.bpm,
              in.mcux, mx0, my0, mw, mh, l, j, want);
      return false;
    }
    seen[j] = 1;
    const int c = in.mcu_comp[b];
    const int bx = in.ncomp == 1 ? mx : mx * in.comp_h[c] + in.mcu_dx[b];
    const int by = in.ncomp == 1 ? my : my * in.comp_v[c] + in.mcu_dy[b];
    const hj::IdctBlockPos p = hj::idct_block_pos(in, j);
    if (p.c != c || p.bx != bx || p.by != by) {
      fprintf(stderr, "bpm %d mcux %d rect (%d, %d, %d, %d) l %u: (%d, %d, %d), plain (%d, %d, %d)\n",
              in.bpm, in.mcux, mx0, my0, mw, mh, l, p.c, p.bx, p.by, c, bx, by);
      return false;
    }
  }
  // nothing outside the rectangle
  for (int my = 0; my < in.mcuy; my++)
    for (int mx = 0; mx < in.mcux; mx++) {
      const bool inside = mx >= mx0 && mx < mx0 + mw && my >= my0 && my < my0 + mh;
      for (int b = 0; b < in.bpm; b++)
        if ((seen[(size_t)(my * in.mcux + mx) * in.bpm + b] != 0) != inside) {
          fprintf(stderr, "bpm %d mcux %d rect (%d, %d, %d, %d): MCU (%d, %d) block %d %s\n", in.bpm,
                  in.mcux, mx0, my0, mw, mh, mx, my, b, inside ? "missed" : "touched");
          return false;
        }
    }
  return true;
}

}  // namespace

int main() {
  const int bpms[] = {1, 2, 3, 4, 6, 8, 10};
  for (int bpm : bpms) {
    // small grids: every rectangle
    for (int mcux = 1; mcux <= 6; mcux++)
      for (int mcuy = 1; mcuy <= 5; mcuy++) {
        hj::ImageInfo in;
        memset(&in, 0, sizeof in);
        layout(in, bpm);
        in.mcux = mcux;
        in.mcuy = mcuy;
        in.nblocks = mcux * mcuy * bpm;
        in.bpm_magic = hj::idct_div_magic((uint32_t)bpm);
        in.mcux_magic = hj::idct_div_magic((uint32_t)mcux);
        for (int mx0 = 0; mx0 < mcux; mx0++)
          for (int my0 = 0; my0 < mcuy; my0++)
            for (int mw = 1; mx0 + mw <= mcux; mw++)
              for (int mh = 1; my0 + mh <= mcuy; mh++)
                if (!rect(in, mx0, my0, mw, mh)) return 1;
      }
    // wide grids: corners, single MCUs, rows, columns, the whole grid
    const int wide[] = {41, 80, 257, 4096};
    for (int mcux : wide) {
      const int mcuy = mcux == 4096 ? 9 : 33;
      hj::ImageInfo in;
      memset(&in, 0, sizeof in);
      layout(in, bpm);
      in.mcux = mcux;
      in.mcuy = mcuy;
      in.nblocks = mcux * mcuy * bpm;
      in.bpm_magic = hj::idct_div_magic((uint32_t)bpm);
      in.mcux_magic = hj::idct_div_magic((uint32_t)mcux);
      const int xs[] = {0, 1, mcux / 2, mcux - 2, mcux - 1}, ys[] = {0, 1, mcuy / 2, mcuy - 1};
      const int ws[] = {1, 2, 3, 7, 16, 17, 40, mcux / 2, mcux - 1, mcux};
      const int hs[] = {1, 2, 7, mcuy - 1, mcuy};
      for (int mx0 : xs)
        for (int my0 : ys)
          for (int mw : ws)
            for (int mh : hs)
              if (mw >= 1 && mh >= 1 && mx0 + mw <= mcux && my0 + mh <= mcuy)
                if (!rect(in, mx0, my0, mw, mh)) return 1;
    }
  }
  printf("rects %ld positions %ld\n", g_rects, g_pos);
  return 0;
}
