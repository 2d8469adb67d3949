// Stand-alone sweep of the one-pass destuffing walk (spdl_amd/csrc/hj_destuff_tile.h:
// the per-group step with its carries, the cut at the terminator, the running
// offset over tiles) against a byte loop over the whole scan.  Host code only;
// tests/test_destuff_tile_core.py builds it with ASan and UBSan and runs it.
//
//   g++ -std=c++17 -O2 -DHJ_HD= -fsanitize=address,undefined destuff_tile_sweep.cpp
//
// Tiles of 1, 2, 3 and 8 groups (16 to 128 bytes: the boundaries are the
// kernel's, only closer together).  Coverage: every pattern FF 00, FF FF.. FF
// 00, FF FF.. Dn, FF D9 and a lone FF at every byte position of the 34 bytes
// around a tile boundary, for every scan_start % 16 and with the file ending
// at every byte after the pattern; scans of 1 byte, tile - 1, tile, tile + 1
// and 2 tiles +- 1 bytes; an all-FF00 scan; then 200 k random scans of up to
// five tiles.  The data bytes, the segment starts, the restart count and the
// scan end must be equal, and ds_tile_step's carry the raw byte.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../spdl_amd/csrc/hj_destuff_tile.h"

namespace {

struct Ref {
  std::vector<uint8_t> out;
  std::vector<uint32_t> seg;  // seg[r - 1]: start of restart segment r
  int scan_end;
};

Ref reference(const uint8_t* d, int size, int start) {
  Ref r;
  r.scan_end = size;
  int j = start;
  while (j < size) {
    if (d[j] != 0xFF) {
      r.out.push_back(d[j++]);
    } else if (j + 1 < size && d[j + 1] == 0x00) {
      r.out.push_back(0xFF);
      j += 2;
    } else {
      int k = j + 1;
      while (k < size && d[k] == 0xFF) k++;
      if (k < size && d[k] >= 0xD0 && d[k] <= 0xD7) {
        r.seg.push_back((uint32_t)r.out.size());
        j = k + 1;
      } else {
        r.scan_end = j;
        break;
      }
    }
  }
  return r;
}

long long g_checked = 0;

[[noreturn]] void fail(const char* what, const uint8_t* d, int size, int start, int groups) {
  std::printf("MISMATCH %s: size %d start %d groups %d file", what, size, start, groups);
  for (int i = 0; i < size && i < 400; i++) std::printf(" %02X", d[i]);
  std::printf("\n");
  std::exit(1);
}

// heap copies of exactly `size` bytes: a read past the file is an ASan report
void check(const uint8_t* file, int size, int start, int groups) {
  uint8_t* d = static_cast<uint8_t*>(std::malloc(size ? size : 1));
  std::memcpy(d, file, size);
  const Ref r = reference(d, size, start);
  const int seg_cap = size / 2 + 2;
  std::vector<uint8_t> out(size + 1, 0xEE);
  std::vector<uint32_t> seg(seg_cap, 0xEEEEEEEEu);
  const hj::DsWalk w = hj::ds_tile_walk(d, size, start, groups, out.data(), seg.data(), seg_cap);
  if (w.clean_len != (int)r.out.size()) fail("clean_len", d, size, start, groups);
  if (!r.out.empty() && std::memcmp(out.data(), r.out.data(), r.out.size())) fail("bytes", d, size, start, groups);
  if (out[r.out.size()] != 0xEE) fail("write past the data", d, size, start, groups);
  if (w.rst != (int)r.seg.size()) fail("restart count", d, size, start, groups);
  for (size_t i = 0; i < r.seg.size(); i++)
    if (seg[i + 1] != r.seg[i]) fail("segment start", d, size, start, groups);
  if (w.scan_end != r.scan_end) fail("scan_end", d, size, start, groups);
  // the carry is the raw last byte, whatever the group holds
  for (int j0 = start & ~15; j0 + 16 <= size; j0 += 16) {
    uint32_t g[4];
    hj::ds_load_bytes(d, size, j0, g);
    const hj::DsStep s = hj::ds_tile_step(g, hj::ds_prev_byte(d, size, j0),
                                          hj::ds_next_byte(d, size, j0), j0, start, size);
    if (s.carry_out != d[j0 + 15] || s.kept != hj::ds_popc(s.keep))
      fail("carry", d, size, start, groups);
  }
  std::free(d);
  g_checked++;
}

uint32_t g_rng = 0x9E3779B9u;
uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 17;
  g_rng ^= g_rng << 5;
  return g_rng;
}

const int kGroups[4] = {1, 2, 3, 8};

}  // namespace

int main() {
  std::vector<uint8_t> f(4096);
  long long patterns = 0;
  // ---- patterns around the first tile boundary -------------------------------------
  for (int gi = 0; gi < 4; gi++) {
    const int groups = kGroups[gi], tile = hj::ds_tile_bytes(groups);
    for (int k = 0; k < 16; k++) {       // scan_start % 16
      const int start = 32 + k;          // tiles begin at 32
      const int edge = 32 + tile;        // the first tile boundary
      for (int pos = edge - 17; pos <= edge + 16; pos++) {
        if (pos < start) continue;
        for (int fill = 0; fill < 4; fill++)  // extra 0xFFs ahead of the second byte
          for (int code = 0; code < 5; code++) {
            // 0: FF.. 00, 1: FF.. D0, 2: FF.. D7, 3: FF.. D9, 4: FF.. then the file ends
            const int size0 = edge + 2 * tile + 40;
            for (int j = 0; j < size0; j++) f[j] = (uint8_t)(0x11 + j % 0xC0);
            for (int j = pos; j <= pos + fill; j++) f[j] = 0xFF;
            const int at = pos + fill + 1;
            static const uint8_t codes[4] = {0x00, 0xD0, 0xD7, 0xD9};
            if (code < 4) f[at] = codes[code];
            if (code == 4) {
              check(f.data(), at, start, groups);
            } else {
              check(f.data(), size0, start, groups);
              // the file ends at every byte from the pattern's end on (a little way)
              for (int size = at; size <= at + 18; size++) check(f.data(), size, start, groups);
            }
            patterns++;
          }
      }
    }
  }
  // ---- scan lengths --------------------------------------------------------------------
  for (int gi = 0; gi < 4; gi++) {
    const int groups = kGroups[gi], tile = hj::ds_tile_bytes(groups);
    const int lens[7] = {1, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1};
    for (int k = 0; k < 16; k++)
      for (int li = 0; li < 7; li++)
        for (int eoi = 0; eoi < 2; eoi++) {
          const int start = 48 + k, n = lens[li];
          for (int j = 0; j < start + n + 2; j++) f[j] = (uint8_t)(0x21 + j % 0xB0);
          f[start + n] = 0xFF;
          f[start + n + 1] = 0xD9;
          check(f.data(), start + n + 2 * eoi, start, groups);
        }
    // all FF 00 pairs: the output is half the input, 0xFF 0x00 right before EOI
    for (int k = 0; k < 16; k++) {
      const int start = 48 + k, n = 4 * tile + 2 * k;
      for (int j = 0; j < n; j += 2) {
        f[start + j] = 0xFF;
        f[start + j + 1] = 0x00;
      }
      f[start + n] = 0xFF;
      f[start + n + 1] = 0xD9;
      check(f.data(), start + n + 2, start, groups);
    }
  }
  // ---- random scans ----------------------------------------------------------------------
  const long long swept = g_checked;
  for (int it = 0; it < 200000; it++) {
    const uint32_t r = rnd();
    const int groups = kGroups[r & 3u], tile = hj::ds_tile_bytes(groups);
    const int start = (int)(r >> 2 & 63u);
    const int size = start + 1 + (int)(r >> 8) % (5 * tile);
    const bool markers = r >> 30 & 1u;  // terminators mid-scan, or RSTn alone
    for (int j = 0; j < size; j++) {
      const uint32_t q = rnd();
      // 0xFF 1/8, 0x00 1/8, RSTn 1/16, anything else
      uint8_t b = (q & 7u) == 0 ? 0xFF : (q & 7u) == 1 ? 0x00 : (q & 0x78u) == 0x10 ? 0xD0 | (q >> 8 & 7u)
                                                                                   : (uint8_t)(q >> 16);
      // without `markers`, what follows an 0xFF is 0x00, 0xFF or RSTn: the scan runs on
      if (!markers && j > 0 && f[j - 1] == 0xFF && b != 0x00 && b != 0xFF) b = 0xD0 | (q >> 8 & 7u);
      f[j] = b;
    }
    check(f.data(), size, start, groups);
  }
  std::printf("scans %lld patterns %lld random %lld\n", g_checked, patterns, g_checked - swept);
  return 0;
}
