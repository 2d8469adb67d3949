// hj_upsample.h -- csc = TURBO (spdl_hipjpeg.h "Pillow-exact decode"): the
// per-component upsampling and the colour conversion of libjpeg-turbo's
// default decoder, restated from their rules.  turbo_rgb_kernel and a native
// sweep (tests/native/upsample_sweep.cpp) share this one definition.
// HJ_HD marks functions that also compile for the host.
//
// A component of ratio (hr, vr) = (hmax / h_c, vmax / v_c) is brought to the
// frame's size from its TRUE plane, cw x ch samples; a neighbour outside it is
// the edge sample.  The plane lies in rows of `stride` bytes (a multiple of 8,
// the base 8-byte aligned) whose columns from cw on hold whatever the IDCT
// left there: the functions below load aligned words, which may cover such
// columns, and use no byte of them.  Rows from ch on are never addressed.
#pragma once
#include <stdint.h>

#include "hj_idct.h"

namespace hj {
namespace up {

// The rule a component takes, uniform over an image.  The triangle rules with
// a horizontal part need more than two columns; every other ratio, (4,1),
// (4,2), (1,4) and the like, replicates.
enum Mode { kCopy = 0, kH2V1, kH1V2, kH2V2, kBox };
HJ_HD inline int mode_of(int hr, int vr, int cw) {
  if (hr == 1 && vr == 1) return kCopy;
  if (hr == 2 && vr == 1 && cw > 2) return kH2V1;
  if (hr == 1 && vr == 2) return kH1V2;
  if (hr == 2 && vr == 2 && cw > 2) return kH2V2;
  return kBox;
}

// ---- the three rules, one output sample each ---------------------------------
// (2,1): p and its left / right neighbour -> out[2i], out[2i + 1]
HJ_HD inline int h2v1_even(int p, int l) { return (3 * p + l + 1) >> 2; }
HJ_HD inline int h2v1_odd(int p, int r) { return (3 * p + r + 2) >> 2; }
// (1,2): p and the row above / below -> out[2j], out[2j + 1]
HJ_HD inline int h1v2_upper(int p, int a) { return (3 * p + a + 1) >> 2; }
HJ_HD inline int h1v2_lower(int p, int b) { return (3 * p + b + 2) >> 2; }
// (2,2): the column sum of p with the row above (upper output row) or below,
// then the horizontal step on the sums
HJ_HD inline int h2v2_sum(int p, int n) { return 3 * p + n; }
HJ_HD inline int h2v2_even(int s, int sl) { return (3 * s + sl + 8) >> 4; }
HJ_HD inline int h2v2_odd(int s, int sr) { return (3 * s + sr + 7) >> 4; }

// ---- the colour conversion (6b tables, SCALEBITS 16; green from
// FIX(0.34414) = 22554, where csc = JFIF has libjpeg 9's 22553) ------------------
constexpr int32_t kCrR = 91881, kCbB = 116130, kCbG = 22554, kCrG = 46802;
HJ_HD inline void ycc_rgb(int y, int cb, int cr, int* rgb) {
  const int32_t x_cb = cb - 128, x_cr = cr - 128;
  rgb[0] = clip_u8_opaque(y + ((kCrR * x_cr + 32768) >> 16));
  rgb[1] = clip_u8_opaque(y + ((-kCbG * x_cb + 32768 - kCrG * x_cr) >> 16));
  rgb[2] = clip_u8_opaque(y + ((kCbB * x_cb + 32768) >> 16));
}

// ---- runs: 8 consecutive output samples of one component ---------------------
HJ_HD inline uint32_t load_word(const uint8_t* p) { return *reinterpret_cast<const uint32_t*>(p); }
HJ_HD inline int byte_of(uint32_t w, int k) { return (int)((w >> (8 * k)) & 0xFFu); }

// The samples cx0 - 1 .. cx0 + 4 of a plane row (cx0 a multiple of 4, below
// cw), each column clamped into [0, cw): the word at cx0 and its two
// neighbours, whose addresses are clamped to the row's first and last word
// with a real sample, so every load is one the plane holds.
HJ_HD inline void window6(const uint8_t* row, int cx0, int cw, int (&s)[6]) {
  const int last = (cw - 1) & ~3;
  const uint32_t wp = load_word(row + (cx0 > 0 ? cx0 - 4 : 0));
  const uint32_t wc = load_word(row + cx0);
  const uint32_t wn = load_word(row + (cx0 + 4 < last ? cx0 + 4 : last));
  s[0] = cx0 > 0 ? byte_of(wp, 3) : byte_of(wc, 0);
  s[1] = byte_of(wc, 0);
#pragma unroll
  for (int k = 1; k < 4; k++) s[k + 1] = cx0 + k < cw ? byte_of(wc, k) : s[k];
  s[5] = cx0 + 4 < cw ? byte_of(wn, 0) : s[4];
}

// The samples x0 .. x0 + 7 of a plane row (x0 a multiple of 8, below cw).
// Those from cw on are the row's padding: their outputs lie outside the frame.
HJ_HD inline void row8(const uint8_t* row, int x0, int (&v)[8]) {
  const uint32_t w0 = load_word(row + x0), w1 = load_word(row + x0 + 4);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    v[k] = byte_of(w0, k);
    v[k + 4] = byte_of(w1, k);
  }
}

// Replication, samples K .. 7 of a run: column (x0 + k) / hr of the two plane
// rows q0 and q1 (a recursion, so that every index into r0 / r1 is a constant
// and the arrays stay in registers)
template <int K>
HJ_HD inline void box8(const uint8_t* q0, const uint8_t* q1, int x0, int hr, int cw, int (&r0)[8],
                       int (&r1)[8]) {
  if constexpr (K < 8) {
    int cx = (x0 + K) / hr;
    cx = cx < cw ? cx : cw - 1;  // (columns past the frame's width)
    r0[K] = q0[cx];
    r1[K] = q1[cx];
    box8<K + 1>(q0, q1, x0, hr, cw, r0, r1);
  }
}

// Output samples x0 .. x0 + 7 of the output rows y0 and y0 + 1 (x0 a multiple
// of 8 below the frame's width, y0 even and below its height) of a component
// in mode `mode` with ratio (hr, vr): r0 and r1.  Under (., 2) both rows come
// from plane row y0 / 2, whose triple products serve both.  Row y0 + 1 may lie
// below the frame: it is computed from clamped rows and not to be stored.
HJ_HD inline void run8x2(const uint8_t* plane, int stride, int cw, int ch, int mode, int hr,
                         int vr, int x0, int y0, int (&r0)[8], int (&r1)[8]) {
  const int ylast = ch - 1;
  if (mode == kCopy) {
    row8(plane + (int64_t)y0 * stride, x0, r0);
    row8(plane + (int64_t)(y0 + 1 < ylast ? y0 + 1 : ylast) * stride, x0, r1);
  } else if (mode == kH1V2) {
    const int cy = y0 >> 1;
    int p[8], a[8], b[8];
    row8(plane + (int64_t)cy * stride, x0, p);
    row8(plane + (int64_t)(cy > 0 ? cy - 1 : 0) * stride, x0, a);
    row8(plane + (int64_t)(cy < ylast ? cy + 1 : ylast) * stride, x0, b);
#pragma unroll
    for (int k = 0; k < 8; k++) {
      r0[k] = h1v2_upper(p[k], a[k]);
      r1[k] = h1v2_lower(p[k], b[k]);
    }
  } else if (mode == kH2V1) {
    const int cx0 = x0 >> 1;
    int s[6], t[6];
    window6(plane + (int64_t)y0 * stride, cx0, cw, s);
    window6(plane + (int64_t)(y0 + 1 < ylast ? y0 + 1 : ylast) * stride, cx0, cw, t);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      r0[2 * k] = h2v1_even(s[k + 1], s[k]);
      r0[2 * k + 1] = h2v1_odd(s[k + 1], s[k + 2]);
      r1[2 * k] = h2v1_even(t[k + 1], t[k]);
      r1[2 * k + 1] = h2v1_odd(t[k + 1], t[k + 2]);
    }
  } else if (mode == kH2V2) {
    const int cx0 = x0 >> 1, cy = y0 >> 1;
    int p[6], a[6], b[6];
    window6(plane + (int64_t)cy * stride, cx0, cw, p);
    window6(plane + (int64_t)(cy > 0 ? cy - 1 : 0) * stride, cx0, cw, a);
    window6(plane + (int64_t)(cy < ylast ? cy + 1 : ylast) * stride, cx0, cw, b);
    int su[6], sl[6];
#pragma unroll
    for (int k = 0; k < 6; k++) {
      su[k] = h2v2_sum(p[k], a[k]);
      sl[k] = h2v2_sum(p[k], b[k]);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      r0[2 * k] = h2v2_even(su[k + 1], su[k]);
      r0[2 * k + 1] = h2v2_odd(su[k + 1], su[k + 2]);
      r1[2 * k] = h2v2_even(sl[k + 1], sl[k]);
      r1[2 * k + 1] = h2v2_odd(sl[k + 1], sl[k + 2]);
    }
  } else {
    // replication: sample (x / hr, y / vr), a byte load each (ratios of 3 and
    // 4 and the planes of one or two columns: rare, and small)
    const int cy0 = y0 / vr, cy1 = (y0 + 1) / vr;
    const uint8_t* q0 = plane + (int64_t)cy0 * stride;
    const uint8_t* q1 = plane + (int64_t)(cy1 < ylast ? cy1 : ylast) * stride;
    box8<0>(q0, q1, x0, hr, cw, r0, r1);
  }
}

}  // namespace up
}  // namespace hj
