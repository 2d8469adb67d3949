// exif_sweep.cpp -- stand-alone checks of the EXIF orientation reader
// (spdl_hj_get_orientation, hj_probe.cpp) on the CPU, for a sanitizer build:
//   g++ -std=c++17 -O2 -g -DHJ_HD= -fsanitize=address,undefined -fno-sanitize-recover=all
//       -static-libasan -static-libubsan tests/native/exif_sweep.cpp
//       spdl_amd/csrc/hj_probe.cpp -o exif_sweep
//   exif_sweep FILE:EXPECTED:LO:HI ...
// Every FILE is a JPEG with hand-made APP1 segments in bytes [LO, HI) (LO == HI:
// none) whose orientation is EXPECTED.  For each file:
//   1. the whole file reads as EXPECTED with return 0;
//   2. every truncation of the file, and
//   3. every single-byte corruption of its APP1 bytes (all 255 other values)
//      return what the header probe returns for the same bytes -- EXIF never
//      fails an image -- with a value in 1..8, and hj::exif_orientation, which
//      cannot fail, stays in 1..8 as well.
// Every buffer is a heap block of exactly its size, so a read outside it stops
// the sanitizer build.  Prints one line and "ok"; exit status 1 and the first
// failures on stderr.
#include "../../spdl_amd/csrc/hj_probe.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

namespace {

int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (failures++ < 20) {                              \
        fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
        fprintf(stderr, __VA_ARGS__);                     \
        fprintf(stderr, "\n");                            \
      }                                                   \
    }                                                     \
  } while (0)

long long buffers = 0;

// One buffer of exactly n bytes through both functions; returns the value
int one(const uint8_t* src, size_t n, const char* what, size_t at) {
  uint8_t* b = static_cast<uint8_t*>(malloc(n ? n : 1));
  if (n) memcpy(b, src, n);
  buffers++;
  spdl_hj_image_info info;
  const int prc = hj::probe(n ? b : nullptr, n, &info);
  int32_t exif = -1;
  const int rc = spdl_hj_get_orientation(n ? b : nullptr, n, &exif);
  CHECK(rc == prc, "%s %zu: get_orientation %d, the probe %d", what, at, rc, prc);
  CHECK(exif >= 1 && exif <= 8, "%s %zu: orientation %d", what, at, (int)exif);
  const int v = hj::exif_orientation(n ? b : nullptr, n);
  CHECK(v >= 1 && v <= 8, "%s %zu: exif_orientation %d", what, at, v);
  CHECK(rc || v == exif, "%s %zu: %d against %d", what, at, v, (int)exif);
  free(b);
  return exif;
}

void sweep(const std::string& arg) {
  char path[1024];
  int expected = 0;
  long lo = 0, hi = 0;
  const size_t c3 = arg.rfind(':'), c2 = arg.rfind(':', c3 - 1), c1 = arg.rfind(':', c2 - 1);
  snprintf(path, sizeof(path), "%s", arg.substr(0, c1).c_str());
  expected = atoi(arg.substr(c1 + 1, c2 - c1 - 1).c_str());
  lo = atol(arg.substr(c2 + 1, c3 - c2 - 1).c_str());
  hi = atol(arg.substr(c3 + 1).c_str());
  FILE* f = fopen(path, "rb");
  if (!f) {
    CHECK(false, "cannot open %s", path);
    return;
  }
  std::vector<uint8_t> d;
  uint8_t buf[4096];
  for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) d.insert(d.end(), buf, buf + n);
  fclose(f);
  CHECK(lo >= 0 && lo <= hi && (size_t)hi <= d.size(), "%s: range %ld..%ld", path, lo, hi);
  int32_t exif = -1;
  const int rc = spdl_hj_get_orientation(d.data(), d.size(), &exif);
  CHECK(rc == 0 && exif == expected, "%s: rc %d, orientation %d, expected %d", path, rc, (int)exif,
        expected);
  for (size_t n = 0; n < d.size(); n++) one(d.data(), n, "truncation at", n);
  std::vector<uint8_t> m = d;
  for (size_t p = (size_t)lo; p < (size_t)hi; p++) {
    for (int v = 0; v < 256; v++) {
      if (v == d[p]) continue;
      m[p] = (uint8_t)v;
      one(m.data(), m.size(), "corruption at", p);
    }
    m[p] = d[p];
  }
}

}  // namespace

int main(int argc, char** argv) {
  // the function's own arguments
  int32_t e = 7;
  if (spdl_hj_get_orientation(nullptr, 0, nullptr) != SPDL_HJ_ERR_INVALID_ARG) failures++;
  if (spdl_hj_get_orientation(nullptr, 0, &e) != SPDL_HJ_ERR_NOT_JPEG || e != 1) failures++;
  for (int i = 1; i < argc; i++) sweep(argv[i]);
  printf("exif: %d files, %lld buffers\n", argc - 1, buffers);
  if (failures) {
    fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
