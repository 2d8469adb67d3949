// flip_sweep.cpp -- stand-alone checks of the output flips (spdl_hj_set_flips)
// on the CPU, for a sanitizer build:
//   g++ -std=c++17 -O2 -g -DHJ_HD= -fsanitize=address,undefined -fno-sanitize-recover=all
//       -static-libasan -static-libubsan tests/native/flip_sweep.cpp
//       spdl_amd/csrc/hj_layout.cpp spdl_amd/csrc/hj_sws.cpp -o flip_sweep
// 1. The tile arithmetic the output kernels use (hj_sws_tile.h tile_flip) over
//    every output size 1..70 x 1..70, the tilers' column chunks and band
//    heights and the four flips: the mirrored tiles partition the box exactly
//    once, every pixel lands at its mirrored coordinate, the tile coordinate
//    stays inside the tile, and the inverse map finds the pixel again -- for
//    the box and for a 4:2:0 chroma plane of it, ceil(ow / 2) x ceil(oh / 2).
//    The same for boxes with one side of 32768 or 65535 and the other 1 or 17.
// 2. The planner's rules (hj_layout.h build_layout): counts, values, the JFIF
//    refusal, all-zero flips being no flips, and the flag vector of a views
//    submission with a refused view in the middle.
// Prints one line per part; exit status 1 and the first failures on stderr.
#include "../../spdl_amd/csrc/hj_layout.h"
#include "../../spdl_amd/csrc/hj_sws_tile.h"

#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

namespace {

using namespace hj;

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

// ---- 1. the tile arithmetic ---------------------------------------------------
long long sweep_box(int W, int H, int rb, int cc, int flip, std::vector<uint8_t>& seen) {
  const bool fh = flip & 1, fv = flip & 2;
  seen.assign((size_t)W * H, 0);
  long long px = 0;
  for (int yo0 = 0; yo0 < H; yo0 += rb)
    for (int xo0 = 0; xo0 < W; xo0 += cc) {
      const SwsWindow win = sws_window(yo0, xo0, rb, cc, 0, 0, W, H, W, H);
      const int th = win.yo1 - yo0, tw = win.xo1 - xo0;
      const TileFlip tf = tile_flip(xo0, win.xo1, yo0, win.yo1, W, H, flip);
      CHECK(tf.mx0 == (fh ? W - win.xo1 : xo0) && tf.my0 == (fv ? H - win.yo1 : yo0),
            "origin %dx%d rb=%d cc=%d flip=%d tile (%d,%d)", W, H, rb, cc, flip, xo0, yo0);
      CHECK(tf.mx0 >= 0 && tf.my0 >= 0 && tf.mx0 + tw <= W && tf.my0 + th <= H,
            "tile leaves the box %dx%d rb=%d cc=%d flip=%d tile (%d,%d)", W, H, rb, cc, flip, xo0,
            yo0);
      for (int yo = yo0; yo < win.yo1; yo++)
        for (int xo = xo0; xo < win.xo1; xo++, px++) {
          const int tx = tf.tx(xo), ty = tf.ty(yo);
          if (tx < 0 || tx >= tw || ty < 0 || ty >= th) {
            CHECK(false, "tile coordinate (%d,%d) outside %dx%d: %dx%d flip=%d px (%d,%d)", tx, ty,
                  tw, th, W, H, flip, xo, yo);
            continue;
          }
          const int gx = tf.mx0 + tx, gy = tf.my0 + ty;
          CHECK(gx == (fh ? W - 1 - xo : xo) && gy == (fv ? H - 1 - yo : yo),
                "px (%d,%d) of %dx%d flip=%d lands at (%d,%d)", xo, yo, W, H, flip, gx, gy);
          CHECK(tf.sx(tx) == xo && tf.sy(ty) == yo, "inverse of (%d,%d) flip=%d: (%d,%d)", xo, yo,
                flip, tf.sx(tx), tf.sy(ty));
          seen[(size_t)gy * W + gx]++;
        }
    }
  for (size_t i = 0; i < seen.size(); i++)
    if (seen[i] != 1) {
      CHECK(false, "%dx%d rb=%d cc=%d flip=%d: output %zu written %d times", W, H, rb, cc, flip, i,
            (int)seen[i]);
      break;
    }
  return px;
}

void sweep_tiles() {
  const int chunks[] = {16, 32, 256}, bands[] = {1, 3, 8, 64};
  std::vector<uint8_t> seen;
  long long px = 0, boxes = 0;
  for (int ow = 1; ow <= 70; ow++)
    for (int oh = 1; oh <= 70; oh++)
      for (int cc : chunks)
        for (int rb : bands)
          for (int flip = 0; flip < 4; flip++) {
            px += sweep_box(ow, oh, rb, cc, flip, seen);
            // the 4:2:0 chroma plane of the same output, mirrored by its own size
            px += sweep_box((ow + 1) / 2, (oh + 1) / 2, rb, cc, flip, seen);
            boxes += 2;
          }
  printf("tiles: %lld boxes, %lld pixels\n", boxes, px);
}

// The same at the format's limit (printed after the planner's line)
void sweep_extreme_tiles() {
  std::vector<uint8_t> seen;
  long long px = 0, boxes = 0;
  // boxes at the format's limit: one side of 65535 (and 32768), the other 1 or
  // 17, with their chroma planes
  for (int L : {32768, 65535})
    for (int S : {1, 17})
      for (int wide = 0; wide < 2; wide++)
        for (int cc : {16, 256})
          for (int rb : {1, 64})
            for (int flip = 0; flip < 4; flip++) {
              const int ow = wide ? L : S, oh = wide ? S : L;
              px += sweep_box(ow, oh, rb, cc, flip, seen);
              px += sweep_box((ow + 1) / 2, (oh + 1) / 2, rb, cc, flip, seen);
              boxes += 2;
            }
  printf("extreme tiles: %lld boxes, %lld pixels\n", boxes, px);
}

// ---- 2. the planner ---------------------------------------------------------------
uint64_t fnv1a(const void* p, size_t n) {
  uint64_t h = 1469598103934665603ull;
  const uint8_t* b = static_cast<const uint8_t*>(p);
  for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

spdl_hj_image_info y420(int w, int h) {
  spdl_hj_image_info p{};
  p.width = w;
  p.height = h;
  p.ncomp = 3;
  for (int c = 0; c < 3; c++) p.h_samp[c] = p.v_samp[c] = 1;
  p.h_samp[0] = p.v_samp[0] = 2;
  p.color = SPDL_HJ_COLOR_YCBCR;
  return p;
}

spdl_hj_output chain(int fit_w = 0, int fit_h = 0) {
  spdl_hj_output o{};
  o.pix_fmt = SPDL_HJ_FMT_RGB24;
  for (int c = 0; c < 3; c++) o.std[c] = 1.f;
  if (fit_w) {
    o.resize = 1;
    o.fit_w = fit_w;
    o.fit_h = fit_h;
  }
  return o;
}

struct Built {
  LayoutResult r;
  Layout L;
};

// n images of 64 x 48 (4:2:0) through `out`, with `flips` (null: none)
Built plan(int n, const spdl_hj_output& out, const uint8_t* flips, int64_t nflips,
           const HeldViews* hv = nullptr) {
  std::vector<spdl_hj_image_info> infos(n, y420(64, 48));
  std::vector<int64_t> offs(n), sizes(n, 3000);
  for (int i = 0; i < n; i++) offs[i] = (int64_t)i * round_up(3000 + 64, 256);
  PlanCache cache;
  LayoutRequest rq{offs.data(), sizes.data(), infos.data(), n, &out, hv ? 0 : 128 * 1024, &cache};
  rq.views = hv;
  rq.flips = flips;
  rq.nflips = nflips;
  Built b;
  b.r = build_layout(rq, b.L);
  return b;
}

// every scalar of a layout and the bytes the device gets, as one string
std::string digest(const Layout& L) {
  char buf[1024];
  snprintf(buf, sizeof(buf),
           "%lld %lld %lld %lld %lld %d %lld %lld %d %dx%d %d,%d,%d %d %d %d,%d,%d %lld %d %lld "
           "%lld %lld %lld %lld %lld %zu %zu %zu %016llx %016llx %016llx",
           (long long)L.total_blocks, (long long)L.total_planes, (long long)L.total_segs,
           (long long)L.total_recs, (long long)L.out_elems_per_image, L.max_blocks,
           (long long)L.max_px, (long long)L.total_ds, L.max_chunks, L.ow, L.oh, L.sws_bands,
           L.sws_chunks, L.sws_lds, (int)L.all_special, (int)L.fuse_ok, L.yuv_hs, L.yuv_vs,
           (int)L.yuv_gray, (long long)L.cmyk_px, L.fused_tiles, (long long)L.chain_granules,
           (long long)L.ds_wgs, (long long)L.idct_wgs, (long long)L.hs_wgs,
           (long long)L.total_hbuf, (long long)L.sws_wgs, L.desc.size(), L.tables.size(),
           L.work.size(),
           (unsigned long long)fnv1a(L.desc.data(), L.desc.size() * sizeof(ImageDesc)),
           (unsigned long long)fnv1a(L.tables.data(), L.tables.size() * 4),
           (unsigned long long)fnv1a(L.work.data(), L.work.size() * 4));
  return buf;
}

void planner_rules() {
  const spdl_hj_output full = chain(), r32 = chain(32, 32);
  spdl_hj_output jfif = chain();
  jfif.csc = SPDL_HJ_CSC_JFIF;
  const uint8_t f01[] = {0, 1, 0}, f4[] = {0, 4}, zero[] = {0, 0}, hv3[] = {3, 2};
  // counts
  CHECK(plan(2, r32, f01, 1).r.rc == SPDL_HJ_ERR_INVALID_ARG, "one flip for two images");
  CHECK(plan(2, r32, f01, 3).r.rc == SPDL_HJ_ERR_INVALID_ARG, "three flips for two images");
  CHECK(plan(2, r32, f01, 2).r.rc == SPDL_HJ_OK, "two flips for two images");
  // values
  const Built v4 = plan(2, r32, f4, 2);
  CHECK(v4.r.rc == SPDL_HJ_ERR_INVALID_ARG && v4.r.image == -1 && strstr(v4.r.err, "0 to 3"),
        "a flip of 4: rc=%d err=%s", v4.r.rc, v4.r.err);
  CHECK(v4.L.desc.empty(), "a refused submission plans nothing");
  // the JFIF conversion takes no flip (all-zero flips are none)
  CHECK(plan(2, jfif, f01, 2).r.rc == SPDL_HJ_ERR_INVALID_ARG, "JFIF with a flip");
  CHECK(plan(2, jfif, zero, 2).r.rc == SPDL_HJ_OK, "JFIF with all-zero flips");
  // all-zero flips: the layout of no flips, byte for byte, and no flag vector
  for (const spdl_hj_output& o : {full, r32}) {
    const Built none = plan(2, o, nullptr, 0), z = plan(2, o, zero, 2);
    CHECK(!none.r.rc && !z.r.rc, "rc %d %d", none.r.rc, z.r.rc);
    CHECK(z.L.flips.empty() && none.L.flips.empty(), "all-zero flips leave a flag vector");
    CHECK(digest(none.L) == digest(z.L), "\n  none %s\n  zero %s", digest(none.L).c_str(),
          digest(z.L).c_str());
  }
  // a set flip: one flag per descriptor; at full resolution the generic output
  // kernel (all_special off), every other byte as without flips
  {
    const Built none = plan(2, full, nullptr, 0), f = plan(2, full, hv3, 2);
    CHECK(!f.r.rc && f.L.flips.size() == 2 && f.L.flips[0] == 3 && f.L.flips[1] == 2, "flags");
    CHECK(none.L.all_special && !f.L.all_special, "special %d -> %d", (int)none.L.all_special,
          (int)f.L.all_special);
    CHECK(fnv1a(none.L.desc.data(), none.L.desc.size() * sizeof(ImageDesc)) ==
              fnv1a(f.L.desc.data(), f.L.desc.size() * sizeof(ImageDesc)),
          "a flip changes no descriptor byte");
  }
  // views: flags by concatenated view order behind the n image descriptors,
  // a refused view (a rectangle larger than the frame) keeps its entry
  {
    int32_t st0[3] = {-7, -7, -7}, st1[2] = {-7, -7};
    HeldViews hv;
    hv.groups.push_back({chain(24, 24), reinterpret_cast<void*>(0x1000), (size_t)3 * 24 * 24 * 3,
                         {{0, {4, 4, 30, 30}}, {0, {0, 0, 70, 10}}, {1, {8, 8, 32, 32}}}, st0});
    hv.groups.push_back({chain(16, 12), reinterpret_cast<void*>(0x2000), (size_t)2 * 16 * 12 * 3,
                         {{1, {0, 0, 0, 0}}, {0, {2, 2, 20, 20}}}, st1});
    const uint8_t vf[] = {1, 2, 3, 1, 2};
    const Built b = plan(2, full, vf, 5, &hv);
    CHECK(!b.r.rc, "views with flips: rc=%d err=%s", b.r.rc, b.r.err);
    const uint8_t want[] = {0, 0, 1, 2, 3, 1, 2};
    CHECK(b.L.flips.size() == 7 && b.L.desc.size() == 7 &&
              !memcmp(b.L.flips.data(), want, 7),
          "view flags (%zu of them)", b.L.flips.size());
    CHECK(st0[0] == 0 && st0[1] == SPDL_HJ_ERR_BAD_GEOMETRY && st0[2] == 0 && st1[0] == 0 &&
              st1[1] == 0,
          "view statuses %d %d %d | %d %d", st0[0], st0[1], st0[2], st1[0], st1[1]);
    CHECK(b.L.desc.size() == 7 && b.L.desc[3].refuse && !b.L.desc[2].refuse && !b.L.desc[4].refuse,
          "the refused view's descriptor");
    // counts go by the views' total, not by n
    CHECK(plan(2, full, vf, 2, &hv).r.rc == SPDL_HJ_ERR_INVALID_ARG, "n flips for 5 views");
    CHECK(plan(2, full, vf, 4, &hv).r.rc == SPDL_HJ_ERR_INVALID_ARG, "4 flips for 5 views");
    // ... and all-zero flips are the views submission without flips
    const uint8_t vz[5] = {};
    const Built z = plan(2, full, vz, 5, &hv), none = plan(2, full, nullptr, 0, &hv);
    CHECK(z.L.flips.empty() && digest(z.L) == digest(none.L), "views, all-zero flips");
  }
  printf("planner: rules hold\n");
}

}  // namespace

int main() {
  sweep_tiles();
  planner_rules();
  sweep_extreme_tiles();
  if (failures) {
    fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
