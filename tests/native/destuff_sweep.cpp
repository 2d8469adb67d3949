// Stand-alone sweep of the destuffing core (spdl_amd/csrc/hj_destuff.h) against
// a byte-loop reference: the classification rule one byte at a time with its
// look-ahead over fill 0xFFs, then a byte-serial compaction.  Host code only;
// tests/test_destuff_core.py builds it with ASan and UBSan and runs it.
//
//   g++ -std=c++17 -O2 -DHJ_HD= -fsanitize=address,undefined destuff_sweep.cpp
//
// Coverage: every 3-byte pattern over {00, FF, D0, D7, D9, 5A} at every
// position of the 18-byte window (byte before, group, byte after) on every
// filler of that alphabet, with every start / end cut in the group and the
// file ending at every byte of it; then 1 M random groups (0xFF with
// probability 1/8).  Masks, restart bits, the terminator and the compacted
// bytes must be equal.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../spdl_amd/csrc/hj_destuff.h"

namespace {

constexpr int kJ0 = 16;    // the group under test: bytes 16..31 of the file
constexpr int kFile = 56;  // window at 15..32, then room for the look-ahead

struct Ref {
  uint32_t keep, rst;
  int term;
  uint8_t out[16];
  int n;
};

// One byte at a time, as the kernels did before the word-parallel core.
Ref reference(const uint8_t* d, int size, int start, int end, int j0) {
  uint8_t b[18];
  b[0] = j0 > 0 && j0 - 1 < size ? d[j0 - 1] : 0;
  for (int i = 0; i < 16; i++) b[1 + i] = j0 + i < size ? d[j0 + i] : 0xD9;
  b[17] = j0 + 16 < size ? d[j0 + 16] : 0xD9;
  Ref r{};
  r.term = 0x7FFFFFFF;
  for (int i = 0; i < 16; i++) {
    const int j = j0 + i;
    if (j < start || j >= size) continue;
    const bool prev_ff = j > start && b[i] == 0xFF;
    if (b[1 + i] != 0xFF) {
      r.keep |= (uint32_t)!prev_ff << i;
    } else if (!prev_ff) {
      if (b[2 + i] == 0x00) {
        r.keep |= 1u << i;
      } else {
        int k = j + 1;
        while (k < size && d[k] == 0xFF) k++;
        if (k < size && d[k] >= 0xD0 && d[k] <= 0xD7) r.rst |= 1u << i;
        else if (j < end && j < r.term) r.term = j;
      }
    }
  }
  const int lim = end - j0;  // bytes at or past the scan end are not part of it
  const uint32_t m = lim >= 16 ? 0xFFFFu : (lim <= 0 ? 0u : ((1u << lim) - 1u));
  r.keep &= m;
  r.rst &= m;
  for (int i = 0; i < 16; i++)
    if (r.keep >> i & 1u) r.out[r.n++] = b[1 + i];
  return r;
}

long long g_checked = 0;

[[noreturn]] void fail(const char* what, const uint8_t* d, int size, int start, int end) {
  std::printf("MISMATCH %s: size %d start %d end %d file", what, size, start, end);
  for (int i = 0; i < kFile; i++) std::printf(" %02X", d[i]);
  std::printf("\n");
  std::exit(1);
}

void check(const uint8_t* d, int size, int start, int end) {
  const int j0 = kJ0;
  const Ref r = reference(d, size, start, end, j0);
  uint32_t w[4];
  hj::ds_load_bytes(d, size, j0, w);
  const hj::DsMasks m = hj::ds_classify_words(w, hj::ds_prev_byte(d, size, j0),
                                              hj::ds_next_byte(d, size, j0), j0, start, end);
  if (m.keep != r.keep) fail("keep", d, size, start, end);
  if (m.keep & m.slow) fail("keep and slow overlap", d, size, start, end);
  uint32_t cslow = 0;
  const int cnt = hj::ds_count_words(w, hj::ds_prev_byte(d, size, j0), hj::ds_next_byte(d, size, j0),
                                     j0, start, end, cslow);
  if (cnt != r.n || cslow != m.slow) fail("count", d, size, start, end);
  uint32_t rst = 0;
  int term = 0x7FFFFFFF;
  if (m.slow) hj::ds_resolve(d, size, j0, m.slow, rst, term);
  if (rst != r.rst) fail("rst", d, size, start, end);
  if (term != r.term) fail("term", d, size, start, end);
  // compaction: the kept bytes end up in [lead, lead + n), zeros around them
  uint32_t drop;
  hj::ds_compact_begin(w, m.keep, drop);
  if (hj::ds_popc(drop) > 14) fail("drop count", d, size, start, end);
  int steps = 0;
  while (drop) {
    hj::ds_compact_step(w, drop);
    if (++steps > 16) fail("steps", d, size, start, end);
  }
  uint32_t idle[4] = {w[0], w[1], w[2], w[3]};
  hj::ds_compact_step(idle, drop);  // a lane with nothing left to drop
  if (std::memcmp(idle, w, 16) || drop) fail("idle step", d, size, start, end);
  const int lead = m.keep ? hj::ds_ctz(m.keep) : 0;
  uint8_t got[16];
  std::memcpy(got, w, 16);
  for (int i = 0; i < 16; i++) {
    const uint8_t want = i >= lead && i < lead + r.n ? r.out[i - lead] : 0;
    if (got[i] != want) fail("compacted bytes", d, size, start, end);
  }
  // the shift into the stage's words (uncut groups: the cuts only thin them)
  for (uint32_t s = 0; s < 4 && start == 0 && end == size; s++) {
    uint32_t x[5];
    hj::ds_shift_words(w, s, x);
    uint8_t xb[20];
    std::memcpy(xb, x, 20);
    for (int i = 0; i < 20; i++) {
      const int src = i - (int)s;
      if (xb[i] != (src >= 0 && src < 16 ? got[src] : 0)) fail("shift", d, size, start, end);
    }
  }
  g_checked++;
}

// every start cut, end cut and file end for one file content
void cuts(const uint8_t* d) {
  for (int start = kJ0 - 2; start <= kJ0 + 17; start++) {
    const int st = start < kJ0 - 1 ? 0 : start;  // 0: a scan that began long before
    for (int end = kJ0; end <= kJ0 + 17; end++) check(d, kFile, st, end);
    check(d, kFile, st, kFile);
    // the file ends inside the group (or right around it)
    for (int size = kJ0; size <= kJ0 + 18; size++) check(d, size, st, size);
  }
}

uint32_t g_rng = 0x9E3779B9u;
uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 17;
  g_rng ^= g_rng << 5;
  return g_rng;
}

}  // namespace

int main() {
  static const uint8_t alpha[6] = {0x00, 0xFF, 0xD0, 0xD7, 0xD9, 0x5A};
  // heap copies of exactly kFile bytes: a read past the file is an ASan report
  uint8_t* d = static_cast<uint8_t*>(std::malloc(kFile));
  long long windows = 0;
  for (int fill = 0; fill < 6; fill++)
    for (int pos = 0; pos < 16; pos++)
      for (int a = 0; a < 6; a++)
        for (int b = 0; b < 6; b++)
          for (int c = 0; c < 6; c++) {
            std::memset(d, alpha[fill], kFile);
            const int at = kJ0 - 1 + pos;  // window byte `pos`
            d[at] = alpha[a];
            d[at + 1] = alpha[b];
            d[at + 2] = alpha[c];
            cuts(d);
            windows++;
          }
  // fill 0xFFs running out of the group into an RSTn, a marker and the file's end
  for (int from = kJ0 - 1; from <= kJ0 + 16; from++)
    for (int to = from; to < kFile; to++)
      for (int code = 0; code < 6; code++) {
        std::memset(d, 0x5A, kFile);
        for (int j = from; j <= to; j++) d[j] = 0xFF;
        if (to + 1 < kFile) d[to + 1] = alpha[code];
        cuts(d);
        windows++;
      }
  const long long swept = g_checked;
  for (int it = 0; it < 1000000; it++) {
    for (int j = 0; j < kFile; j++) {
      const uint32_t r = rnd();
      // 0xFF 1/8, 0x00 1/8, RSTn 1/16, anything else
      d[j] = (r & 7u) == 0 ? 0xFF : (r & 7u) == 1 ? 0x00 : (r & 0x78u) == 0x10 ? 0xD0 | (r >> 8 & 7u)
                                                                              : (uint8_t)(r >> 16);
    }
    const uint32_t r = rnd();
    const int size = (r & 3u) ? kFile : kJ0 + (int)(r >> 2) % (kFile - kJ0 + 1);
    const int start = (r >> 8 & 3u) ? 0 : (int)(r >> 10) % (kJ0 + 18);
    const int end = (r >> 16 & 3u) ? size : (int)(r >> 18) % (size + 1);
    check(d, size, start < size ? start : 0, end);
  }
  std::free(d);
  std::printf("groups %lld windows %lld random %lld\n", g_checked, windows, g_checked - swept);
  return 0;
}
