// header_sweep.cpp -- stand-alone sweep of the two host-side marker walks, the
// probe (spdl_amd/csrc/hj_probe.cpp) and the oracle (oracle/jpeg_oracle.c:
// jo_parse, and ms_decode behind jo_decode_coefs), for a sanitizer build on
// the CPU:
//   gcc -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -c oracle/jpeg_oracle.c \
//       oracle/sws_oracle.c
//   g++ -std=c++17 -O1 -g -DHJ_HD= -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -static-libasan -static-libubsan tests/native/header_sweep.cpp \
//       spdl_amd/csrc/hj_probe.cpp jpeg_oracle.o sws_oracle.o -lpthread -lm -o header_sweep
//   header_sweep CORPUS
// The corpus (tests/test_jpeg_headers.py writes it from tests/jpeg_header_cases.py):
//   "HSW1", u32 streams, then per stream
//   u32 size, i32 oracle status wanted (-1: any), i32 probe status wanted (-1: any),
//   u32 ranges, ranges x (u32 first, u32 end), the bytes
// Every stream is copied into a heap block of exactly its size (a read one
// byte past it is a sanitizer report), probed and parsed; where the parse
// succeeds the coefficients and the planes (both IDCTs) are decoded too.  Then
// the mutation sweep: every byte inside the stream's ranges replaced in turn by
// 00, 01, 7F, 80, FF, and the stream cut at every offset inside them.  (The
// ranges are the header bytes a walk interprets: markers, lengths, tables,
// frame and scan headers, and the first 16 payload bytes of segments skipped
// by length.  A mutant is decoded only while its frame stays small.)
// On all of them:
//   the oracle accepts  =>  the probe accepts, and width, height, components,
//                           sampling factors, colour model and the multi-scan
//                           flag are equal
//   the probe refuses   =>  with NOT_JPEG, UNSUPPORTED or BAD_HEADER, and the
//                           oracle refuses too
// and a named stream returns the statuses its row wants.
// Prints "streams N oracle_ok A probe_ok B mutants M oracle_ok C probe_ok D"
// and exits 0, or 1 at the first violation.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../spdl_amd/csrc/hj_probe.h"

extern "C" {
#include "../../oracle/jpeg_oracle.h"
}

namespace {

struct Counts {
  long n = 0, oracle_ok = 0, probe_ok = 0;
};

int fail(const char* what, long stream, long at, int value, int po, int pp) {
  fprintf(stderr, "header_sweep: %s (stream %ld, offset %ld, value %d: oracle %d, probe %d)\n",
          what, stream, at, value, po, pp);
  return 1;
}

// 0, or 1 after a violation.  max_blocks: frames above it are parsed only.
int run_one(const uint8_t* src, size_t size, int want_oracle, int want_probe, int max_blocks,
            Counts& k, long stream, long at, int value) {
  uint8_t* d = (uint8_t*)malloc(size ? size : 1);
  if (!d) return fail("out of memory", stream, at, value, 0, 0);
  if (size) memcpy(d, src, size);
  // (a zero-length stream still gets a block; neither walk may read it)
  spdl_hj_image_info pi;
  jo_info oi;
  const int pp = hj::probe(d, size, &pi);
  int po = jo_parse(d, size, &oi);
  k.n++;
  k.probe_ok += pp == 0;
  int rc = 0;
  if (po == 0) {
    if (pp != 0) rc = fail("the oracle accepts what the probe refuses", stream, at, value, po, pp);
    else if (pi.width != oi.width || pi.height != oi.height || pi.ncomp != oi.ncomp ||
             pi.color != oi.color || (pi.multiscan != 0) != (oi.multiscan != 0))
      rc = fail("probe and oracle read another frame", stream, at, value, po, pp);
    for (int c = 0; c < oi.ncomp && !rc; c++)
      if (pi.h_samp[c] != oi.comp_h[c] || pi.v_samp[c] != oi.comp_v[c])
        rc = fail("probe and oracle read other sampling factors", stream, at, value, po, pp);
  } else if (pp != 0 && pp != SPDL_HJ_ERR_NOT_JPEG && pp != SPDL_HJ_ERR_UNSUPPORTED &&
             pp != SPDL_HJ_ERR_BAD_HEADER) {
    rc = fail("a probe status outside NOT_JPEG / UNSUPPORTED / BAD_HEADER", stream, at, value, po,
              pp);
  }
  if (!rc && po == 0 && oi.nblocks <= max_blocks) {
    size_t blocks = 0;
    for (int c = 0; c < oi.ncomp; c++) blocks += (size_t)oi.comp_bw[c] * oi.comp_bh[c];
    std::vector<int16_t> coefs((size_t)oi.nblocks * 64), levels(blocks * 64);
    po = jo_decode_coefs(d, size, &oi, coefs.data(), levels.data());
    if (po == 0) {
      std::vector<uint8_t> planes(jo_planes_size(&oi));
      for (int idct = 0; idct < 2 && po == 0; idct++)
        po = jo_decode_planes(d, size, idct, planes.data());
    }
  }
  k.oracle_ok += po == 0;
  if (!rc && want_oracle >= 0 && po != want_oracle)
    rc = fail("the oracle's status is not the row's", stream, at, value, po, pp);
  if (!rc && want_probe >= 0 && pp != want_probe)
    rc = fail("the probe's status is not the row's", stream, at, value, po, pp);
  free(d);
  return rc;
}

uint32_t rd32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: header_sweep CORPUS\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  std::vector<uint8_t> all;
  uint8_t buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) all.insert(all.end(), buf, buf + got);
  fclose(f);
  if (all.size() < 8 || memcmp(all.data(), "HSW1", 4) != 0) {
    fprintf(stderr, "header_sweep: not a corpus\n");
    return 2;
  }
  const uint32_t n = rd32(all.data() + 4);
  size_t pos = 8;
  Counts named, mutants;
  static const int kValues[5] = {0x00, 0x01, 0x7F, 0x80, 0xFF};
  for (uint32_t s = 0; s < n; s++) {
    if (pos + 16 > all.size()) return fail("corpus cut short", s, 0, 0, 0, 0);
    const uint32_t size = rd32(&all[pos]);
    const int want_oracle = (int32_t)rd32(&all[pos + 4]), want_probe = (int32_t)rd32(&all[pos + 8]);
    const uint32_t nr = rd32(&all[pos + 12]);
    pos += 16;
    if (pos + 8ull * nr + size > all.size()) return fail("corpus cut short", s, 0, 0, 0, 0);
    const uint8_t* ranges = &all[pos];
    pos += 8ull * nr;
    std::vector<uint8_t> d(all.begin() + pos, all.begin() + pos + size);
    pos += size;
    if (run_one(d.data(), size, want_oracle, want_probe, 1 << 16, named, s, -1, -1)) return 1;
    for (uint32_t r = 0; r < nr; r++) {
      const uint32_t a = rd32(ranges + 8 * r), b = rd32(ranges + 8 * r + 4);
      if (a > b || b > size) return fail("bad range", s, a, 0, 0, 0);
      for (uint32_t i = a; i < b; i++) {
        const uint8_t keep = d[i];
        for (int v : kValues) {
          if (v == keep) continue;
          d[i] = (uint8_t)v;
          if (run_one(d.data(), size, -1, -1, 256, mutants, s, i, v)) return 1;
        }
        d[i] = keep;
        if (run_one(d.data(), i, -1, -1, 256, mutants, s, i, -2)) return 1;  // cut in front of i
      }
    }
  }
  printf("streams %ld oracle_ok %ld probe_ok %ld mutants %ld oracle_ok %ld probe_ok %ld\n", named.n,
         named.oracle_ok, named.probe_ok, mutants.n, mutants.oracle_ok, mutants.probe_ok);
  return 0;
}
