// lowres_sweep.cpp -- hj_idct.h's reduced-size transforms (lowres_idct4 / 2 /
// 1) against a second restatement in plain loops, kept here: 64-bit
// arithmetic that checks every intermediate against the int32 range the
// transforms' own arithmetic lives in.  Built with -DHJ_HD= under
// -fsanitize=address,undefined (tests/test_lowres.py), no HIP.
//
//   random corners (several magnitudes), every zero / non-zero pattern of
//   (d2, d6) in rows and in columns, coefficients at +-32767 and the DC at the
//   int16 ends.
//
// Then the blocks of a fixed seed with their results, one line each
// ("blk" + 16 corner coefficients + 16 + 4 + 1 samples), which the Python
// test holds against tests/lowres_ref.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>

#include "../../spdl_amd/csrc/hj_idct.h"

namespace {

int fails = 0;
long checked = 0;

int64_t in32(int64_t v) {
  if (v < INT32_MIN || v > INT32_MAX) {
    printf("FAIL: %lld leaves int32\n", (long long)v);
    fails++;
  }
  return v;
}
int clip8(int64_t v) { return v < 0 ? 0 : v > 255 ? 255 : (int)v; }
int64_t asr(int64_t v, int n) { return v >= 0 ? v >> n : -((-v + (1LL << n) - 1) >> n); }  // floor

void ref_pass(const int64_t d[4], int64_t o[4]) {
  const int64_t d0 = d[0], d2 = d[1], d4 = d[2], d6 = d[3];
  int64_t t2 = 0, t3 = 0;
  if (d6 != 0 && d2 != 0) {
    const int64_t z1 = in32((d2 + d6) * 4433);
    t2 = in32(z1 - in32(d6 * 15137));
    t3 = in32(z1 + in32(d2 * 6270));
  } else if (d6 != 0) {
    t2 = in32(-d6 * 10703);
    t3 = in32(d6 * 4433);
  } else if (d2 != 0) {
    t2 = in32(d2 * 4433);
    t3 = in32(d2 * 10703);
  }
  const int64_t t0 = in32((d0 + d4) * 8192), t1 = in32((d0 - d4) * 8192);
  o[0] = in32(t0 + t3);
  o[1] = in32(t1 + t2);
  o[2] = in32(t1 - t2);
  o[3] = in32(t0 - t3);
}

void ref4(const int32_t* b, int* px) {
  int64_t ws[4][4];
  for (int r = 0; r < 4; r++) {
    int64_t d[4], o[4];
    for (int k = 0; k < 4; k++) d[k] = b[4 * r + k];
    if (r == 0) d[0] += 4;
    ref_pass(d, o);
    for (int k = 0; k < 4; k++) ws[r][k] = (int16_t)asr(o[k] + (1 << 10), 11);
  }
  for (int c = 0; c < 4; c++) {
    int64_t d[4], o[4];
    for (int k = 0; k < 4; k++) d[k] = ws[k][c];
    ref_pass(d, o);
    for (int k = 0; k < 4; k++) px[4 * k + c] = clip8(asr(o[k], 18));
  }
}

void ref2(const int32_t* b, int* px) {
  const int64_t b00 = (int64_t)b[0] + 4, b01 = b[1], b10 = b[4], b11 = b[5];
  const int64_t d00 = b00 + b01, d01 = b00 - b01, d10 = b10 + b11, d11 = b10 - b11;
  px[0] = clip8(asr(d00 + d10, 3));
  px[1] = clip8(asr(d01 + d11, 3));
  px[2] = clip8(asr(d00 - d10, 3));
  px[3] = clip8(asr(d01 - d11, 3));
}

int ref1(int32_t dc) { return clip8(asr((int64_t)dc + 4, 3)); }

// the three transforms of one corner b[16] (row stride 4) against the restatement
void check(const int32_t* b, bool dump) {
  int32_t o4[16], o2[4];
  int r4[16], r2[4];
  hj::lowres_idct4(b, 4, o4, 4);
  hj::lowres_idct2(b, 4, o2, 2);
  const int32_t o1 = hj::lowres_idct1(b[0]);
  ref4(b, r4);
  ref2(b, r2);
  bool bad = o1 != ref1(b[0]);
  for (int i = 0; i < 16; i++) bad = bad || o4[i] != r4[i];
  for (int i = 0; i < 4; i++) bad = bad || o2[i] != r2[i];
  checked++;
  if (bad && fails++ < 10) {
    printf("FAIL: corner");
    for (int i = 0; i < 16; i++) printf(" %d", b[i]);
    printf("\n");
  }
  if (dump) {
    printf("blk");
    for (int i = 0; i < 16; i++) printf(" %d", b[i]);
    for (int i = 0; i < 16; i++) printf(" %d", o4[i]);
    for (int i = 0; i < 4; i++) printf(" %d", o2[i]);
    printf(" %d\n", o1);
  }
}

uint32_t rng_state = 1;
uint32_t rng() {  // xorshift32
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}
int32_t coef(int mag) { return (int32_t)(rng() % (2u * mag + 1u)) - mag; }

void random_corner(int32_t* b, int mag, int zero_pct) {
  for (int i = 0; i < 16; i++) b[i] = (int)(rng() % 100u) < zero_pct ? 0 : coef(mag);
  b[0] = 1024 + coef(mag < 1024 ? mag : 1024);
}

}  // namespace

int main() {
  int32_t b[16];
  // random corners: small (typical files), medium, the whole int16 range; sparse and dense
  for (int mag : {8, 300, 2000, 32767})
    for (int zero_pct : {0, 50, 90})
      for (int i = 0; i < 20000; i++) {
        random_corner(b, mag, zero_pct);
        check(b, false);
      }
  printf("random: %ld corners\n", checked);
  // every zero / non-zero pattern of (d2, d6) -- elements 1 and 3 -- in all
  // four rows (8 bits).  The column pass's d2 and d6 are rows 1 and 3 of the
  // row pass's output: zero exactly when the whole input row is (2 bits: the
  // row zeroed), and non-zero with the row's own d2 = d6 = 0 when its elements
  // 0 and 2 are filled (1 bit) -- so every pattern of the columns as well.
  long patterns = 0;
  for (int rows = 0; rows < 256; rows++)
    for (int zrow = 0; zrow < 4; zrow++)
      for (int fill = 0; fill < 2; fill++)
        for (int rep = 0; rep < 8; rep++) {
          for (int i = 0; i < 16; i++) b[i] = 0;
          for (int r = 0; r < 4; r++) {
            if (fill) b[4 * r] = coef(400) | 1, b[4 * r + 2] = coef(400) | 1;
            if (rows >> (2 * r) & 1) b[4 * r + 1] = coef(400) | 1;
            if (rows >> (2 * r + 1) & 1) b[4 * r + 3] = coef(400) | 1;
          }
          b[0] = 1024 + coef(500);
          for (int k = 0; k < 4; k++) {
            if (zrow & 1) b[4 + k] = 0;
            if (zrow & 2) b[12 + k] = 0;
          }
          check(b, false);
          patterns++;
        }
  printf("patterns: %ld corners\n", patterns);
  // the ends: every coefficient at +-32767 in every sign pattern, the DC at the int16 ends
  long ends = 0;
  for (int signs = 0; signs < (1 << 16); signs++) {
    for (int i = 0; i < 16; i++) b[i] = signs >> i & 1 ? -32767 : 32767;
    for (int dc : {-32768, 32767, b[0]}) {
      b[0] = dc;
      check(b, false);
      ends++;
    }
  }
  for (int dc : {-32768, -32767, -5, -4, 0, 3, 4, 1020, 1024, 2035, 2036, 2044, 32767}) {
    for (int i = 0; i < 16; i++) b[i] = 0;
    b[0] = dc;
    check(b, false);
    ends++;
  }
  printf("ends: %ld corners\n", ends);
  // the dump of a fixed seed
  rng_state = 20240607u;
  for (int i = 0; i < 96; i++) {
    random_corner(b, i < 32 ? 40 : i < 64 ? 1500 : 32767, i % 3 == 0 ? 60 : 10);
    check(b, true);
  }
  if (fails) {
    printf("%d failures\n", fails);
    return 1;
  }
  printf("ok\n");
  return 0;
}
