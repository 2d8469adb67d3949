// idct_index_sweep.cpp -- stand-alone sweep of idct_kernel's block index
// function (hj_common.h: idct_block_pos, idct_divmod, idct_div_magic) against
// plain / and %, for a sanitizer build on the CPU:
//   g++ -std=c++17 -O2 -DHJ_HD= -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -static-libasan -static-libubsan tests/native/idct_index_sweep.cpp -o idct_index_sweep
// For every bpm in {1, 2, 3, 4, 6, 8, 10} and mcux in {1, 2, 3, 5, 41, 80, 255,
// 256, 257, 4096, 8192}: an image of as many MCU rows as keep nblocks below
// 2^24 (the host's limit), every j below min(nblocks, 2^20), then the last
// 2^16 values below 2^24 (the function is exact for any j; past nblocks the
// MCU row runs on).  idct_divmod alone also on divisors and dividends up to
// 2^32 - 1.  Prints "images N positions P divmod D" and exits 0, or 1 at the
// first difference.
#include <stdio.h>
#include <string.h>

#include "../../spdl_amd/csrc/hj_common.h"

namespace {

long g_pos = 0, g_div = 0;

// an MCU of bpm blocks: bpm - 2 luma blocks in a row (bpm >= 3), then two 1x1
// components; bpm 2: two 1x1 components; bpm 1: one component (gray)
void layout(hj::ImageInfo& in, int bpm) {
  in.bpm = bpm;
  if (bpm == 1) {
    in.ncomp = 1;
    in.comp_h[0] = in.comp_v[0] = 2;  // a gray frame's factors mean nothing
    return;
  }
  const int luma = bpm >= 3 ? bpm - 2 : 1;
  // 8 luma blocks as 4 x 2, 4 as 2 x 2, otherwise one row
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

bool check(const hj::ImageInfo& in, uint32_t j) {
  const uint32_t mcu = j / (uint32_t)in.bpm, b = j % (uint32_t)in.bpm;
  const int mx = (int)(mcu % (uint32_t)in.mcux), my = (int)(mcu / (uint32_t)in.mcux);
  const int c = in.mcu_comp[b];
  const int bx = in.ncomp == 1 ? mx : mx * in.comp_h[c] + in.mcu_dx[b];
  const int by = in.ncomp == 1 ? my : my * in.comp_v[c] + in.mcu_dy[b];
  const hj::IdctBlockPos p = hj::idct_block_pos(in, j);
  g_pos++;
  if (p.c == c && p.bx == bx && p.by == by) return true;
  fprintf(stderr, "bpm %d mcux %d j %u: (%d, %d, %d), plain (%d, %d, %d)\n", in.bpm, in.mcux, j,
          p.c, p.bx, p.by, c, bx, by);
  return false;
}

bool check_div(uint32_t n, uint32_t d) {
  const hj::IdctDivMod r = hj::idct_divmod(n, d, hj::idct_div_magic(d));
  g_div++;
  if (r.q == n / d && r.r == n % d) return true;
  fprintf(stderr, "%u / %u: (%u, %u), plain (%u, %u)\n", n, d, r.q, r.r, n / d, n % d);
  return false;
}

}  // namespace

int main() {
  const int bpms[] = {1, 2, 3, 4, 6, 8, 10};
  const int mcuxs[] = {1, 2, 3, 5, 41, 80, 255, 256, 257, 4096, 8192};
  long images = 0;
  for (int bpm : bpms)
    for (int mcux : mcuxs) {
      hj::ImageInfo in;
      memset(&in, 0, sizeof in);
      layout(in, bpm);
      in.mcux = mcux;
      in.mcuy = ((1 << 24) - 1) / (bpm * mcux);
      in.nblocks = in.mcux * in.mcuy * in.bpm;
      in.bpm_magic = hj::idct_div_magic((uint32_t)in.bpm);
      in.mcux_magic = hj::idct_div_magic((uint32_t)in.mcux);
      const uint32_t n = (uint32_t)in.nblocks < (1u << 20) ? (uint32_t)in.nblocks : (1u << 20);
      for (uint32_t j = 0; j < n; j++)
        if (!check(in, j)) return 1;
      for (uint32_t j = (1u << 24) - (1u << 16); j < (1u << 24); j++)
        if (!check(in, j)) return 1;
      images++;
    }
  // the division alone, far past what the kernel asks of it
  const uint32_t ds[] = {1, 2, 3, 5, 6, 7, 10, 41, 255, 256, 257, 641, 4096, 8192, 65535, 65536,
                         65537, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFFFFFEu, 0xFFFFFFFFu};
  for (uint32_t d : ds) {
    for (uint32_t n = 0; n < (1u << 16); n++)
      if (!check_div(n, d) || !check_div(0xFFFFFFFFu - n, d)) return 1;
    for (uint32_t k = 1; k < (1u << 12) && (uint64_t)k * d <= 0xFFFFFFFFull; k++)  // multiples and neighbours
      if (!check_div(k * d, d) || !check_div(k * d - 1, d)) return 1;
    const uint32_t top = 0xFFFFFFFFu / d * d;  // the largest multiple
    if (!check_div(top, d) || !check_div(top - 1, d)) return 1;
  }
  printf("images %ld positions %ld divmod %ld\n", images, g_pos, g_div);
  return 0;
}
