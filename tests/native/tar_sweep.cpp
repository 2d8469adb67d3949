// tar_sweep.cpp -- stand-alone driver of the tar member walk
// (spdl_amd/csrc/hj_tar.h), for a sanitizer build on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -static-libasan -static-libubsan tests/native/tar_sweep.cpp \
//       spdl_amd/csrc/hj_tar.cpp -o tar_sweep
//   tar_sweep <archive> [--cap BYTES] [--start POS] [--truncate]
// Walks the archive as the binding does -- up to four members per call, a
// names buffer of --cap bytes (default 64 KiB), resumed at next_pos until a
// call returns no member or the end -- and prints "offset size name" per
// member, then "next_pos P".  The archive lies in a heap block of exactly its
// size, so a read past it is a sanitizer report.  --truncate repeats the walk
// on the first L bytes (a block of exactly L) for every L that is a multiple
// of 512 or one off it, each under a line "limit L".  A member that does not
// lie inside the bytes walked exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../spdl_amd/csrc/hj_tar.h"

namespace {

int walk(const uint8_t* data, size_t size, size_t start, size_t cap) {
  std::vector<char> names(cap ? cap : 1);
  size_t pos = start;
  for (;;) {
    int64_t offs[4], szs[4], noffs[4];
    int32_t n = 0;
    size_t next = 0;
    hj::tar_index(data, size, pos, 4, offs, szs, noffs, names.data(), cap, &n, &next);
    for (int i = 0; i < n; i++) {
      if (offs[i] < 0 || szs[i] < 0 || (size_t)(offs[i] + szs[i]) > size) {
        printf("member outside the buffer: %lld + %lld > %zu\n", (long long)offs[i],
               (long long)szs[i], size);
        return 1;
      }
      printf("%lld %lld %s\n", (long long)offs[i], (long long)szs[i], names.data() + noffs[i]);
    }
    pos = next;
    if (n == 0 || pos >= size) break;
  }
  printf("next_pos %zu\n", pos);
  return 0;
}

// the first n bytes of `all` in a block of their own
int walk_prefix(const std::vector<uint8_t>& all, size_t n, size_t start, size_t cap) {
  uint8_t* block = static_cast<uint8_t*>(malloc(n ? n : 1));
  memcpy(block, all.data(), n);
  const int rc = walk(block, n, start, cap);
  free(block);
  return rc;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  size_t cap = 65536, start = 0;
  bool truncate = false;
  for (int i = 2; i < argc; i++) {
    if (!strcmp(argv[i], "--truncate")) truncate = true;
    else if (!strcmp(argv[i], "--cap") && i + 1 < argc) cap = strtoull(argv[++i], nullptr, 10);
    else if (!strcmp(argv[i], "--start") && i + 1 < argc) start = strtoull(argv[++i], nullptr, 10);
    else return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> all;
  uint8_t buf[4096];
  for (size_t r; (r = fread(buf, 1, sizeof(buf), f)) > 0;) all.insert(all.end(), buf, buf + r);
  fclose(f);
  if (!truncate) return walk_prefix(all, all.size(), start, cap);
  for (size_t m = 0; m <= all.size() + 1; m += 512)
    for (size_t n : {m - 1, m, m + 1}) {
      if (n > all.size()) continue;  // (m - 1 of m = 0 wraps: skipped as well)
      printf("limit %zu\n", n);
      if (walk_prefix(all, n, start, cap)) return 1;
    }
  return 0;
}
