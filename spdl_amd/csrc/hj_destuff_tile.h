// Destuffing one image in one pass, host + device: the step a thread of
// destuff_image_kernel (hj_kernels.hip) takes on its 16-byte group of a tile,
// and the walk over a scan's tiles that the kernel's workgroup makes with it.
//
// A tile is `groups` consecutive 16-byte groups (one per thread), the first
// tile starting at scan_start & ~15.  What crosses from one group to the next
// -- inside a tile or over its boundary -- is one byte each way: the raw last
// byte of the group before (a stuffed pair, a fill run or a marker that
// straddles the boundary turns on it being 0xFF) and the first byte of the
// group after (0x00 after an 0xFF makes the pair).  The running output offset
// is the sum of what the tiles before kept.  The first terminating marker
// ends the scan: the tile that holds it is cut there and is the last.
//
// tests/native/destuff_tile_sweep.cpp walks whole scans with ds_tile_walk
// against a byte loop.
#pragma once
#include "hj_destuff.h"

namespace hj {

constexpr int kDsNoTerm = 0x7FFFFFFF;

struct DsStep {
  uint32_t keep, slow;  // bit i: byte j0 + i (hj_destuff.h DsMasks)
  int kept;             // data bytes of the group
  uint32_t carry_out;   // the group's raw last byte: the next group's carry_in
};

// One group of a tile: `w` holds bytes [j0, j0 + 16) (bytes past the file as
// 0xD9), carry_in is the raw byte j0 - 1 (anything where there is none),
// `next` byte j0 + 16 (0xD9 past the file).  The scan is [start, size): its
// end is not known before the walk reaches it.
HJ_HD inline DsStep ds_tile_step(const uint32_t (&w)[4], uint32_t carry_in, uint32_t next, int j0,
                                 int start, int size) {
  const DsMasks m = ds_classify_words(w, carry_in, next, j0, start, size);
  DsStep s;
  s.keep = m.keep;
  s.slow = m.slow;
  s.kept = ds_popc(m.keep);
  s.carry_out = w[3] >> 24;
  return s;
}

// A group's mask cut at the scan's end `term` (a file position): the bits of
// bytes below it.  A byte's class does not depend on where the scan ends, so
// the cut mask is the mask of the scan [start, term).
HJ_HD inline uint32_t ds_tile_cut(uint32_t mask, int j0, int term) {
  const int n = term - j0;
  return n >= 16 ? mask : n <= 0 ? 0u : mask & ((1u << n) - 1u);
}

// The bytes of a tile of `groups` groups.
HJ_HD inline int ds_tile_bytes(int groups) { return 16 * groups; }

// What a walk leaves behind (ImageInfo's clean_len, nseg - 1 and scan_end).
struct DsWalk {
  int clean_len, rst, scan_end;
};

// The whole walk, one group after another: `out` receives the data bytes
// (room for size bytes) and seg[r] the output offset at which restart segment
// r = 1.. begins (room for seg_cap entries; seg may be null).  The kernel runs
// the groups of a tile side by side and scans their counts; the carries, the
// cut and the running offset are these.
inline DsWalk ds_tile_walk(const uint8_t* d, int size, int start, int groups, uint8_t* out,
                           uint32_t* seg, int seg_cap) {
  DsWalk r{0, 0, size};
  const int tile = ds_tile_bytes(groups);
  uint32_t carry = ds_prev_byte(d, size, start & ~15);
  for (int tb = start & ~15; tb < size; tb += tile) {
    int term = kDsNoTerm;
    // pass 1 (the kernel: before its first barrier): the tile's terminator
    uint32_t last = carry;
    for (int g = 0; g < groups; g++) {
      const int j0 = tb + 16 * g;
      uint32_t w[4];
      ds_load_bytes(d, size, j0, w);
      const DsStep s = ds_tile_step(w, last, ds_next_byte(d, size, j0), j0, start, size);
      last = s.carry_out;
      if (s.slow) {
        uint32_t rst;
        int t;
        ds_resolve(d, size, j0, s.slow, rst, t);
        if (t < term) term = t;
      }
    }
    // pass 2: cut, count, compact at the running offset
    last = carry;
    for (int g = 0; g < groups; g++) {
      const int j0 = tb + 16 * g;
      uint32_t w[4];
      ds_load_bytes(d, size, j0, w);
      const DsStep s = ds_tile_step(w, last, ds_next_byte(d, size, j0), j0, start, size);
      last = s.carry_out;
      uint32_t rst = 0;
      if (s.slow) {
        int t;
        ds_resolve(d, size, j0, s.slow, rst, t);
      }
      const uint32_t keep = ds_tile_cut(s.keep, j0, term);
      rst = ds_tile_cut(rst, j0, term);
      for (uint32_t q = rst; q; q &= q - 1) {
        r.rst++;
        if (seg && r.rst < seg_cap)
          seg[r.rst] = (uint32_t)(r.clean_len + ds_popc(keep & ((1u << ds_ctz(q)) - 1u)));
      }
      uint32_t drop;
      ds_compact_begin(w, keep, drop);
      while (drop) ds_compact_step(w, drop);
      const int lead = keep ? ds_ctz(keep) : 0, n = ds_popc(keep);
      for (int i = 0; i < n; i++) out[r.clean_len + i] = (uint8_t)(w[(lead + i) >> 2] >> (8 * ((lead + i) & 3)));
      r.clean_len += n;
    }
    carry = last;
    if (term != kDsNoTerm) {
      r.scan_end = term;
      break;
    }
  }
  return r;
}

}  // namespace hj
