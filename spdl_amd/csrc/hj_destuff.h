// Destuffing core, host + device: classify and compact one 16-byte group of an
// entropy-coded segment run in words (SWAR), no byte array.
//
// The rule per byte (T.81 B.1.1.5, F.1.2.3), prev_ff = the raw previous byte
// is 0xFF (false at `start`):
//   keep = !prev_ff && (cur != 0xFF || next == 0x00)   data byte
//   slow =  cur == 0xFF && !prev_ff && next != 0x00    RSTn, terminating marker or fill
// and everything else is dropped (stuffed 0x00, fill 0xFF, a marker's code).
// The slow positions are rare (restart markers, and the marker that ends the
// scan); ds_resolve walks them byte by byte.
//
// The destuff kernels (hj_kernels.hip) and tests/native/destuff_sweep.cpp
// build from this one header.
#pragma once
#include <cstdint>

#ifndef HJ_HD
#define HJ_HD __host__ __device__
#endif

namespace hj {

HJ_HD inline int ds_ctz(uint32_t v) {  // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return __ffs((int)v) - 1;
#else
  return __builtin_ctz(v);
#endif
}
HJ_HD inline int ds_top(uint32_t v) {  // index of the highest set bit, v != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return 31 - __clz((int)v);
#else
  return 31 - __builtin_clz(v);
#endif
}
HJ_HD inline int ds_popc(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(v);
#else
  return __builtin_popcount(v);
#endif
}
// Bytes 0..7 of {hi, lo} picked by the selector's four byte indices; index
// 0x0C gives 0x00 and 0x0D 0xFF (v_perm_b32; its other indices are not used).
HJ_HD inline uint32_t ds_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(hi, lo, sel);
#else
  const uint64_t v = (uint64_t)hi << 32 | lo;
  uint32_t r = 0;
  for (int b = 0; b < 4; b++) {
    const uint32_t ix = (sel >> (8 * b)) & 0xFFu;
    const uint32_t byte = ix == 0x0Du ? 0xFFu : ix == 0x0Cu ? 0u : (uint32_t)(v >> (8 * (ix & 7u))) & 0xFFu;
    r |= byte << (8 * b);
  }
  return r;
#endif
}
// {hi, lo} >> 8 * n, low word; n in 0..3 (v_alignbyte_b32).
HJ_HD inline uint32_t ds_alignbyte(uint32_t hi, uint32_t lo, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, n);
#else
  return (uint32_t)(((uint64_t)hi << 32 | lo) >> (8 * (n & 3u)));
#endif
}

// Bit 7 of every byte (the other bits are scrap), four words at once, to a
// 16-bit mask (bit 4 w + b).
HJ_HD inline uint32_t ds_flags16(uint32_t f0, uint32_t f1, uint32_t f2, uint32_t f3) {
  // two words per pass: flags at bits 8 b (even word) and 8 b + 4 (odd word);
  // folding by 7 gathers b = 0..3 of each into one nibble
  const uint32_t c0 = (f0 & 0x80808080u) >> 7 | (f1 & 0x80808080u) >> 3;
  const uint32_t c1 = (f2 & 0x80808080u) >> 7 | (f3 & 0x80808080u) >> 3;
  const uint32_t n0 = (c0 | (c0 >> 7) | (c0 >> 14) | (c0 >> 21)) & 0xFFu;
  const uint32_t n1 = (c1 | (c1 >> 7) | (c1 >> 14) | (c1 >> 21)) & 0xFFu;
  return n0 | n1 << 8;
}

struct DsMasks {
  uint32_t keep, slow;  // bit i: byte j0 + i
};

// A group's neighbours and, near the file's end, its words: the byte before
// (0 where there is none), the byte after and bytes past the file read as 0xD9.
HJ_HD inline uint32_t ds_prev_byte(const uint8_t* d, int size, int j0) {
  return j0 > 0 && j0 - 1 < size ? d[j0 - 1] : 0u;
}
HJ_HD inline uint32_t ds_next_byte(const uint8_t* d, int size, int j0) {
  return j0 + 16 < size ? d[j0 + 16] : 0xD9u;
}
HJ_HD inline void ds_load_bytes(const uint8_t* d, int size, int j0, uint32_t (&w)[4]) {
#pragma unroll
  for (int i = 0; i < 4; i++) {
    uint32_t v = 0;
    for (int b = 0; b < 4; b++) {
      const int j = j0 + 4 * i + b;
      v |= (j < size ? (uint32_t)d[j] : 0xD9u) << (8 * b);
    }
    w[i] = v;
  }
}

// The word-parallel pass over a group: `w` holds bytes [j0, j0 + 16) (bytes
// past the file as 0xD9), `prev` is byte j0 - 1 (anything where there is
// none) and `next` byte j0 + 16 (0xD9 past the file).  Bit 7 of every byte
// of the outputs is a flag, the other bits are scrap (the byte sums cannot
// carry): ff = the byte is 0xFF, nz = it is not 0x00, drop = not a data byte,
// and *slow is non-zero where the group holds a slow byte.
struct DsFlags {
  uint32_t ff[5], nz[5];  // ff[0]: byte j0 - 1 (top byte), nz[4]: byte j0 + 16 (low byte)
  uint32_t drop[4];
  uint32_t slow;
};
HJ_HD inline DsFlags ds_flags(const uint32_t (&w)[4], uint32_t prev, uint32_t next) {
  DsFlags f;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint32_t a = w[i] & 0x7F7F7F7Fu;
    f.ff[i + 1] = (a + 0x01010101u) & w[i];
    f.nz[i] = (a + 0x7F7F7F7Fu) | w[i];
  }
  f.ff[0] = prev == 0xFFu ? 0x80000000u : 0u;
  f.nz[4] = next != 0u ? 0x80u : 0u;
  f.slow = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint32_t pf = ds_alignbyte(f.ff[i + 1], f.ff[i], 3);  // the byte before is 0xFF
    const uint32_t nn = ds_alignbyte(f.nz[i + 1], f.nz[i], 1);  // the byte after is not 0x00
    const uint32_t t = f.ff[i + 1] & nn;
    f.drop[i] = t | pf;
    f.slow |= t & ~pf;
  }
  f.slow &= 0x80808080u;
  return f;
}

// A group with no slow byte that lies inside the scan, its first byte
// excluded, needs no more than the drop flags.  Nearly every group is plain.
HJ_HD inline bool ds_plain(const DsFlags& f, int j0, int start, int end) {
  return f.slow == 0u && start < j0 && j0 + 16 <= end;
}

// The masks of any group, bit by bit: only bytes in [start, end) get a bit
// (end <= the file size) and the first scan byte has no byte before it.
HJ_HD inline DsMasks ds_masks_edge(const DsFlags& f, int j0, int start, int end) {
  const int lo = start > j0 ? (start - j0 < 16 ? start - j0 : 16) : 0;
  const int hi = end > j0 ? (end - j0 < 16 ? end - j0 : 16) : 0;
  const uint32_t valid = hi > lo ? (0xFFFFu >> (16 - hi)) & (0xFFFFu << lo) : 0u;
  const uint32_t first = start >= j0 && start < j0 + 16 ? 1u << lo : 0u;
  const uint32_t f16 = ds_flags16(f.ff[1], f.ff[2], f.ff[3], f.ff[4]);
  const uint32_t n16 = ds_flags16(f.nz[0], f.nz[1], f.nz[2], f.nz[3]);
  const uint32_t pf16 = ((f16 << 1) | (f.ff[0] >> 31)) & ~first;
  const uint32_t nn16 = (n16 >> 1) | (f.nz[4] << 8);
  DsMasks m;
  m.keep = ~pf16 & (~f16 | ~nn16) & valid;
  m.slow = f16 & ~pf16 & nn16 & valid;
  return m;
}

// Classify bytes [j0, j0 + 16) of the scan [start, end).
HJ_HD inline DsMasks ds_classify_words(const uint32_t (&w)[4], uint32_t prev, uint32_t next,
                                       int j0, int start, int end) {
  const DsFlags f = ds_flags(w, prev, next);
  if (!ds_plain(f, j0, start, end)) return ds_masks_edge(f, j0, start, end);
  DsMasks m;
  m.keep = ~ds_flags16(f.drop[0], f.drop[1], f.drop[2], f.drop[3]) & 0xFFFFu;
  m.slow = 0;
  return m;
}

// The same, for counting alone: the number of data bytes and the slow mask.
HJ_HD inline int ds_count_words(const uint32_t (&w)[4], uint32_t prev, uint32_t next, int j0,
                                int start, int end, uint32_t& slow) {
  const DsFlags f = ds_flags(w, prev, next);
  if (!ds_plain(f, j0, start, end)) {
    const DsMasks m = ds_masks_edge(f, j0, start, end);
    slow = m.slow;
    return ds_popc(m.keep);
  }
  slow = 0;
  return 16 - ds_popc(f.drop[0] & 0x80808080u) - ds_popc(f.drop[1] & 0x80808080u) -
         ds_popc(f.drop[2] & 0x80808080u) - ds_popc(f.drop[3] & 0x80808080u);
}

// The slow positions of a group, byte by byte: an 0xFF run that ends in RSTn
// is a restart marker (rst), anything else ends the scan (term: the smallest
// such position, 0x7FFFFFFF where there is none).  `d` is the file.
HJ_HD inline void ds_resolve(const uint8_t* d, int size, int j0, uint32_t slow, uint32_t& rst,
                             int& term) {
  rst = 0;
  term = 0x7FFFFFFF;
  while (slow) {
    const int i = ds_ctz(slow);
    slow &= slow - 1;
    int k = j0 + i + 1;
    while (k < size && d[k] == 0xFF) k++;
    if (k < size && d[k] >= 0xD0 && d[k] <= 0xD7) {
      rst |= 1u << i;
    } else if (j0 + i < term) {
      term = j0 + i;
    }
  }
}

// Compaction, step 0: zero the bytes `keep` drops and return in `drop` the
// dropped bytes that lie between kept ones; only those need removing (the
// ones below the first kept byte stay, as zeros, and the caller stores the
// group that much lower; the ones above the last are zeros past the data).
HJ_HD inline void ds_compact_begin(uint32_t (&w)[4], uint32_t keep, uint32_t& drop) {
#pragma unroll
  for (int i = 0; i < 4; i++) {
    // nibble -> 0x01 per kept byte (bit b lands on 8 b; a 24-bit product) -> 0xFF
    const uint32_t m = (((keep >> (4 * i)) & 15u) * 0x204081u) & 0x01010101u;
    w[i] &= ds_perm(0u, 0u, 0x0C0C0C0Cu + m);
  }
  drop = keep ? ~keep & ((1u << ds_top(keep)) - 1u) & ~((1u << ds_ctz(keep)) - 1u) : 0u;
}

// Compaction, one step: take the lowest byte of `drop` out of the group (the
// bytes above it move down one, and so do their bits in `drop`; a zero comes
// in at the top).  No bits in `drop`: nothing changes, so a wave can loop on
// its largest count.
HJ_HD inline void ds_compact_step(uint32_t (&w)[4], uint32_t& drop) {
  const int p = ds_ctz(drop | 0x10000u);  // 16: nothing to drop
  drop = (drop >> 1) & (0xFFFFFFFFu << p);
  const uint32_t up = 0xFFFF0000u >> (16 - p);  // low 16 bits: the bytes from p on
#pragma unroll
  for (int i = 0; i < 4; i++) {
    // a byte from p on comes from one higher: its index in {w[i + 1], w[i]} plus one
    // (nibble -> 0x01 per byte: bit b lands on 8 b, a 24-bit product)
    const uint32_t inc = (((up >> (4 * i)) & 15u) * 0x204081u) & 0x01010101u;
    w[i] = ds_perm(i < 3 ? w[i + 1] : 0u, w[i], 0x03020100u + inc);
  }
}

// The compacted group moved up by s = 0..3 bytes into five words, to be
// stored at a byte offset that is s past a word boundary.
HJ_HD inline void ds_shift_words(const uint32_t (&w)[4], uint32_t s, uint32_t (&x)[5]) {
  const uint32_t sel = 0x07060504u - ds_perm(0u, s, 0u);  // s in every byte
  x[0] = ds_perm(w[0], 0u, sel);
  x[1] = ds_perm(w[1], w[0], sel);
  x[2] = ds_perm(w[2], w[1], sel);
  x[3] = ds_perm(w[3], w[2], sel);
  x[4] = ds_perm(0u, w[3], sel);
}

}  // namespace hj
