// pack_sweep.cpp -- stand-alone sweep of the pinned-staging copier
// (spdl_amd/csrc/hj_pack.h: CopyPool, parallel_pack, parallel_pread), for
// sanitizer builds on the CPU, once with ASan + UBSan and once with TSan:
//   g++ -std=c++17 -O1 -g -pthread -fsanitize=thread -static-libtsan \
//       tests/native/pack_sweep.cpp spdl_amd/csrc/hj_pack.cpp -o pack_sweep
//   pack_sweep <scratch file>
// Pools of 1, 2, 4 and 8 workers (built with explicit sizes: copy_workers()
// reads the machine) live across 50 rounds of the whole program, so every run
// after the first reuses a pool's generation counter and pending count.
// Per round and pool, item lists on both sides of the 4 MiB threshold below
// which the pool is bypassed:
//   small      1 MB in all: the serial branch
//   exact      len == padded
//   tails      len < padded, the bench's round_up(len + 64, 256)
//   empties    zero-length items, with and without a tail, among others
//   giant      one item larger than any worker's share
//   bench      256 items of about 110 KB
// Every item is followed by 64 bytes that no item covers.  The packed buffer
// must equal a single-threaded pack byte for byte, those gaps still holding
// the sentinel the buffer was filled with.  Then parallel_pread over a file
// of 9 MiB + 1 byte: from offsets 0 and 4097 to its end, a short read below
// the threshold, and a read reaching one byte past the end, which is false.
// Prints "rounds R cases C" and exits 0, or 1 at the first failure.
#include <fcntl.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <memory>
#include <string>
#include <vector>

#include "../../spdl_amd/csrc/hj_pack.h"

namespace {

using hj::CopyItem;
using hj::CopyPool;

constexpr uint8_t kSentinel = 0xA5;
constexpr int64_t kGap = 64;

struct Case {
  const char* name;
  std::vector<int64_t> len, padded;
};

int64_t bench_pad(int64_t len) { return (len + 64 + 255) / 256 * 256; }

std::vector<Case> cases() {
  std::vector<Case> cs;
  Case small{"small", {}, {}}, exact{"exact", {}, {}}, tails{"tails", {}, {}},
      empties{"empties", {}, {}}, giant{"giant", {}, {}}, bench{"bench", {}, {}};
  for (int i = 0; i < 10; i++) {
    small.len.push_back(100000 + i);
    small.padded.push_back(bench_pad(100000 + i));
  }
  for (int i = 0; i < 20; i++) {
    exact.len.push_back(256 * 1024 + (i % 3));  // (odd lengths: ragged worker boundaries)
    exact.padded.push_back(exact.len.back());
  }
  for (int i = 0; i < 48; i++) {
    tails.len.push_back(100000 + 37 * i);
    tails.padded.push_back(bench_pad(tails.len.back()) + (i % 4 == 0 ? 4096 : 0));
  }
  for (int i = 0; i < 60; i++) {
    const bool empty = i % 4 == 1 || i % 4 == 2;
    empties.len.push_back(empty ? 0 : 150000 + i);
    empties.padded.push_back(empty ? (i % 4 == 1 ? 256 : 0) : bench_pad(150000 + i));
  }
  for (int i = 0; i < 21; i++) {
    giant.len.push_back(i == 7 ? (3 << 20) + 5 : 60000 + i);
    giant.padded.push_back(bench_pad(giant.len.back()));
  }
  for (int i = 0; i < 256; i++) {
    bench.len.push_back(110000 + (i * 977) % 4096);
    bench.padded.push_back(bench_pad(bench.len.back()));
  }
  for (Case* c : {&small, &exact, &tails, &empties, &giant, &bench}) cs.push_back(*c);
  return cs;
}

int fail(const char* what, const char* name, int workers, int round) {
  printf("FAIL %s: case %s, %d workers, round %d\n", what, name, workers, round);
  return 1;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return fail("usage: pack_sweep <scratch file>", "-", 0, 0);
  const int kRounds = 50;
  // source bytes: an LCG's, never the sentinel
  std::vector<uint8_t> src((32 << 20) + 4096);
  uint32_t x = 12345;
  for (uint8_t& b : src) {
    x = x * 1664525u + 1013904223u;
    b = (uint8_t)(x >> 24);
    if (b == kSentinel) b = 0x5A;
  }
  std::vector<std::unique_ptr<CopyPool>> pools;
  for (int w : {1, 2, 4, 8}) pools.emplace_back(new CopyPool(w - 1));
  const std::vector<Case> cs = cases();
  const std::string path = argv[1];
  const size_t fsize = (9u << 20) + 1;
  {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || fwrite(src.data(), 1, fsize, f) != fsize) return fail("write", "file", 0, 0);
    fclose(f);
  }
  const int fd = open(path.c_str(), O_RDONLY);
  if (fd < 0) return fail("open", "file", 0, 0);
  // (one expected and one packed buffer per case and pool, filled with the
  // sentinel once: the gaps must hold it to the end)
  std::vector<std::vector<uint8_t>> wants(cs.size()), gots(cs.size() * pools.size());
  std::vector<uint8_t> got, rd(fsize + 1);
  for (int round = 0; round < kRounds; round++) {
    for (size_t ci = 0; ci < cs.size(); ci++) {
      const Case& c = cs[ci];
      // items laid out one behind the other, a gap after each; the sources
      // move with the round, so a byte a pack left out shows the round before
      std::vector<CopyItem> items;
      int64_t at = 0, so = round * 61;
      for (size_t i = 0; i < c.len.size(); i++) {
        items.push_back({at, src.data() + so, c.len[i], c.padded[i]});
        at += c.padded[i] + kGap;
        so += c.len[i];
      }
      if ((size_t)so > src.size()) return fail("source too small", c.name, 0, round);
      std::vector<uint8_t>& want = wants[ci];
      if (want.empty()) want.assign((size_t)at, kSentinel);
      for (const CopyItem& it : items) {
        memcpy(want.data() + it.dst_off, it.src, (size_t)it.len);
        memset(want.data() + it.dst_off + it.len, 0, (size_t)(it.padded - it.len));
      }
      for (size_t pi = 0; pi < pools.size(); pi++) {
        std::vector<uint8_t>& out = gots[ci * pools.size() + pi];
        if (out.empty()) out.assign((size_t)at, kSentinel);
        hj::parallel_pack(pools[pi].get(), out.data(), items);
        if (memcmp(out.data(), want.data(), (size_t)at) != 0)
          return fail("packed bytes differ", c.name, pools[pi]->workers(), round);
      }
    }
    for (auto& pool : pools) {
      for (size_t off : {(size_t)0, (size_t)4097}) {
        memset(rd.data(), kSentinel, rd.size());
        if (!hj::parallel_pread(pool.get(), fd, (int64_t)off, rd.data(), fsize - off) ||
            memcmp(rd.data(), src.data() + off, fsize - off) != 0 || rd[fsize - off] != kSentinel)
          return fail("pread", off ? "offset 4097" : "offset 0", pool->workers(), round);
        if (hj::parallel_pread(pool.get(), fd, (int64_t)off, rd.data(), fsize - off + 1))
          return fail("pread past the end succeeded", "eof", pool->workers(), round);
      }
      if (!hj::parallel_pread(pool.get(), fd, 12345, rd.data(), 1 << 20) ||
          memcmp(rd.data(), src.data() + 12345, 1 << 20) != 0)
        return fail("pread", "short", pool->workers(), round);
    }
  }
  close(fd);
  // without a pool: one thread
  std::vector<CopyItem> one{{0, src.data(), 1000, 1024}};
  got.assign(1024, kSentinel);
  hj::parallel_pack(nullptr, got.data(), one);
  if (memcmp(got.data(), src.data(), 1000) != 0 || got[1000] != 0 || got[1023] != 0)
    return fail("packed bytes differ", "no pool", 1, kRounds);
  printf("rounds %d cases %zu\n", kRounds, cs.size());
  return 0;
}
