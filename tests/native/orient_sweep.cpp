// orient_sweep.cpp -- stand-alone checks of the output orientations
// (spdl_hj_set_orients) on the CPU, for a sanitizer build:
//   g++ -std=c++17 -O2 -g -DHJ_HD= -fsanitize=address,undefined -fno-sanitize-recover=all
//       -static-libasan -static-libubsan tests/native/orient_sweep.cpp
//       spdl_amd/csrc/hj_layout.cpp spdl_amd/csrc/hj_sws.cpp -o orient_sweep
// 1. The tile arithmetic of the oriented store (hj_sws_tile.h tile_orient) over
//    every chain box 1..70 x 1..70, the tilers' column chunks and band heights
//    and the eight codes: the landed tiles partition the final box exactly
//    once, every chain pixel lands where the header's formula says, the landed
//    coordinate stays inside the landed tile, and the inverse map finds the
//    pixel again.  Codes 0..3 agree with tile_flip.  The same for boxes with
//    one side of 32768 or 65535 and the other 1 or 17.
// 2. The planner's rules (hj_layout.h build_layout): a transposed image is
//    planned from the swapped chain and keeps that chain's box, the "one size"
//    rule is about final boxes, the refusals (count, value, JFIF, planar YUV
//    with a transpose, flips beside orients), all-zero codes being none, codes
//    0..3 being the flips, and the code vector of a views submission.
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
// The header's formula, written out: chain pixel (x, y) of the cw x ch box in
// the final box
void formula(int cw, int ch, int code, int x, int y, int* fx, int* fy) {
  const bool t = code & 4;
  const int aw = t ? ch : cw, ah = t ? cw : ch;
  const int ax = t ? y : x, ay = t ? x : y;  // A(ax, ay) = C(x, y)
  *fx = (code & 1) ? aw - 1 - ax : ax;
  *fy = (code & 2) ? ah - 1 - ay : ay;
}

long long sweep_box(int W, int H, int rb, int cc, int code, std::vector<uint8_t>& seen) {
  const bool t = code & 4;
  const int FW = t ? H : W, FH = t ? W : H;
  seen.assign((size_t)W * H, 0);
  long long px = 0;
  for (int yo0 = 0; yo0 < H; yo0 += rb)
    for (int xo0 = 0; xo0 < W; xo0 += cc) {
      const SwsWindow win = sws_window(yo0, xo0, rb, cc, 0, 0, W, H, W, H);
      const int th = win.yo1 - yo0, tw = win.xo1 - xo0;
      const TileOrient to = tile_orient(xo0, win.xo1, yo0, win.yo1, W, H, code);
      CHECK(to.fw == FW && to.fh == FH && to.lw == (t ? th : tw) && to.lh == (t ? tw : th),
            "sizes %dx%d code=%d: final %dx%d landed %dx%d", W, H, code, to.fw, to.fh, to.lw, to.lh);
      CHECK(to.mx0() >= 0 && to.my0() >= 0 && to.mx0() + to.lw <= FW && to.my0() + to.lh <= FH,
            "tile leaves the box %dx%d rb=%d cc=%d code=%d tile (%d,%d)", W, H, rb, cc, code, xo0,
            yo0);
      if (!t) {  // codes 0..3: the flips
        const TileFlip tf = tile_flip(xo0, win.xo1, yo0, win.yo1, W, H, code);
        CHECK(tf.mx0 == to.mx0() && tf.my0 == to.my0(), "flip origin, code %d", code);
      }
      for (int yo = yo0; yo < win.yo1; yo++)
        for (int xo = xo0; xo < win.xo1; xo++, px++) {
          const int lx = to.lx(xo, yo), ly = to.ly(xo, yo);
          if (lx < 0 || lx >= to.lw || ly < 0 || ly >= to.lh) {
            CHECK(false, "landed coordinate (%d,%d) outside %dx%d: %dx%d code=%d px (%d,%d)", lx,
                  ly, to.lw, to.lh, W, H, code, xo, yo);
            continue;
          }
          int fx, fy;
          formula(W, H, code, xo, yo, &fx, &fy);
          const int gx = to.mx0() + lx, gy = to.my0() + ly;
          CHECK(gx == fx && gy == fy, "px (%d,%d) of %dx%d code=%d lands at (%d,%d), not (%d,%d)",
                xo, yo, W, H, code, gx, gy, fx, fy);
          CHECK(to.cx(lx, ly) == xo && to.cy(lx, ly) == yo, "inverse of (%d,%d) code=%d: (%d,%d)",
                xo, yo, code, to.cx(lx, ly), to.cy(lx, ly));
          if (!t) {
            const TileFlip tf = tile_flip(xo0, win.xo1, yo0, win.yo1, W, H, code);
            CHECK(tf.tx(xo) == lx && tf.ty(yo) == ly, "flip coordinate, code %d", code);
          }
          seen[(size_t)gy * FW + gx]++;
        }
    }
  for (size_t i = 0; i < seen.size(); i++)
    if (seen[i] != 1) {
      CHECK(false, "%dx%d rb=%d cc=%d code=%d: output %zu written %d times", W, H, rb, cc, code, i,
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
          for (int code = 0; code < 8; code++) {
            px += sweep_box(ow, oh, rb, cc, code, seen);
            boxes++;
          }
  printf("tiles: %lld boxes, %lld pixels\n", boxes, px);
}

// The same at the format's limit (printed after the planner's line)
void sweep_extreme_tiles() {
  std::vector<uint8_t> seen;
  long long px = 0, boxes = 0;
  // boxes at the format's limit: one side of 65535 (and 32768), the other 1 or
  // 17 -- a transposing code makes the long side the other one
  for (int L : {32768, 65535})
    for (int S : {1, 17})
      for (int wide = 0; wide < 2; wide++)
        for (int cc : {16, 256})
          for (int rb : {1, 64})
            for (int code = 0; code < 8; code++) {
              px += sweep_box(wide ? L : S, wide ? S : L, rb, cc, code, seen);
              boxes++;
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

spdl_hj_output chain(int fit_w = 0, int fit_h = 0, int pad_w = 0, int pad_h = 0, int crop_w = 0,
                     int crop_h = 0) {
  spdl_hj_output o{};
  o.pix_fmt = SPDL_HJ_FMT_RGB24;
  for (int c = 0; c < 3; c++) o.std[c] = 1.f;
  if (fit_w) {
    o.resize = 1;
    o.fit_w = fit_w;
    o.fit_h = fit_h;
    o.pad_w = pad_w;
    o.pad_h = pad_h;
    o.crop_w = crop_w;
    o.crop_h = crop_h;
  }
  return o;
}

struct Built {
  LayoutResult r;
  Layout L;
};

// images of the given sizes (4:2:0) through `out`, with orients and / or flips
Built plan(const std::vector<spdl_hj_image_info>& infos, const spdl_hj_output& out,
           const uint8_t* orients, int64_t norients, const HeldViews* hv = nullptr,
           const uint8_t* flips = nullptr, int64_t nflips = 0) {
  const int n = (int)infos.size();
  std::vector<int64_t> offs(n), sizes(n, 3000);
  for (int i = 0; i < n; i++) offs[i] = (int64_t)i * round_up(3000 + 64, 256);
  PlanCache cache;
  LayoutRequest rq{offs.data(), sizes.data(), infos.data(), n, &out, hv ? 0 : 128 * 1024, &cache};
  rq.views = hv;
  rq.orients = orients;
  rq.norients = norients;
  rq.flips = flips;
  rq.nflips = nflips;
  Built b;
  b.r = build_layout(rq, b.L);
  return b;
}

std::string digest(const Layout& L) {
  char buf[1024];
  snprintf(buf, sizeof(buf),
           "%lld %lld %lld %lld %lld %d %lld %lld %d %dx%d %d,%d,%d %d %d %lld %lld %lld %lld %zu "
           "%zu %zu %d %016llx %016llx %016llx %016llx",
           (long long)L.total_blocks, (long long)L.total_planes, (long long)L.total_segs,
           (long long)L.total_recs, (long long)L.out_elems_per_image, L.max_blocks,
           (long long)L.max_px, (long long)L.total_ds, L.max_chunks, L.ow, L.oh, L.sws_bands,
           L.sws_chunks, L.sws_lds, (int)L.all_special, (int)L.fuse_ok, (long long)L.ds_wgs,
           (long long)L.idct_wgs, (long long)L.hs_wgs, (long long)L.sws_wgs, L.desc.size(),
           L.tables.size(), L.work.size(), (int)L.transposed,
           (unsigned long long)fnv1a(L.desc.data(), L.desc.size() * sizeof(ImageDesc)),
           (unsigned long long)fnv1a(L.tables.data(), L.tables.size() * 4),
           (unsigned long long)fnv1a(L.work.data(), L.work.size() * 4),
           (unsigned long long)fnv1a(L.flips.data(), L.flips.size()));
  return buf;
}

void planner_rules() {
  const std::vector<spdl_hj_image_info> two(2, y420(64, 48));
  const spdl_hj_output full = chain(), r = chain(40, 24);
  spdl_hj_output jfif = chain();
  jfif.csc = SPDL_HJ_CSC_JFIF;
  const uint8_t c05[] = {0, 5, 0}, c8[] = {0, 8}, zero[] = {0, 0}, c32[] = {3, 2}, c40[] = {4, 0};
  // counts and values
  CHECK(plan(two, r, c05, 1).r.rc == SPDL_HJ_ERR_INVALID_ARG, "one code for two images");
  CHECK(plan(two, r, c05, 3).r.rc == SPDL_HJ_ERR_INVALID_ARG, "three codes for two images");
  CHECK(plan(two, r, c05, 2).r.rc == SPDL_HJ_OK, "two codes for two images");
  const Built v8 = plan(two, r, c8, 2);
  CHECK(v8.r.rc == SPDL_HJ_ERR_INVALID_ARG && v8.r.image == -1 && strstr(v8.r.err, "0 to 7"),
        "a code of 8: rc=%d err=%s", v8.r.rc, v8.r.err);
  CHECK(v8.L.desc.empty(), "a refused submission plans nothing");
  // JFIF takes no code; all-zero codes are none
  CHECK(plan(two, jfif, c32, 2).r.rc == SPDL_HJ_ERR_INVALID_ARG, "JFIF with a code");
  CHECK(plan(two, jfif, zero, 2).r.rc == SPDL_HJ_OK, "JFIF with all-zero codes");
  // flips beside orients, whatever their values
  CHECK(plan(two, r, zero, 2, nullptr, zero, 2).r.rc == SPDL_HJ_ERR_INVALID_ARG,
        "flips and orients on one submission");
  // the planar YUV output: codes 0..3 as the flips, a transpose refused
  {
    spdl_hj_output yuv = chain(40, 24);
    yuv.pix_fmt = SPDL_HJ_FMT_YUV;
    const Built t = plan(two, yuv, c40, 2);
    CHECK(t.r.rc == SPDL_HJ_ERR_INVALID_ARG && t.L.desc.empty() && strstr(t.r.err, "planar YUV"),
          "YUV with a transpose: rc=%d err=%s", t.r.rc, t.r.err);
    const Built f = plan(two, yuv, nullptr, 0, nullptr, c32, 2), o = plan(two, yuv, c32, 2);
    CHECK(!f.r.rc && !o.r.rc && digest(f.L) == digest(o.L), "YUV codes 0..3 are the flips");
  }
  // all-zero codes: the layout of none, byte for byte; codes 0..3: the flips'
  for (const spdl_hj_output& o : {full, r}) {
    const Built none = plan(two, o, nullptr, 0), z = plan(two, o, zero, 2);
    CHECK(!none.r.rc && !z.r.rc && z.L.flips.empty() && !z.L.transposed, "all-zero codes");
    CHECK(digest(none.L) == digest(z.L), "\n  none %s\n  zero %s", digest(none.L).c_str(),
          digest(z.L).c_str());
    const Built f = plan(two, o, nullptr, 0, nullptr, c32, 2), c = plan(two, o, c32, 2);
    CHECK(!f.r.rc && !c.r.rc && digest(f.L) == digest(c.L) && !c.L.transposed &&
              !c.L.all_special,
          "codes 0..3 against flips");
  }
  // T swaps the chain: final 40 x 24 with pad and crop; the transposed image is
  // planned as the plain image of the swapped spec and keeps that chain's box
  {
    const spdl_hj_output fin = chain(40, 24, 44, 30, 42, 26), sw = chain(24, 40, 30, 44, 26, 42);
    spdl_hj_output dec = fin, decsw = sw;
    dec.aspect = decsw.aspect = SPDL_HJ_ASPECT_DECREASE;
    for (int pass = 0; pass < 2; pass++) {
      const spdl_hj_output& a = pass ? dec : fin;
      const spdl_hj_output& b = pass ? decsw : sw;
      const std::vector<spdl_hj_image_info> one(1, y420(64, 48));
      for (int code = 4; code < 8; code++) {
        const uint8_t cc[] = {(uint8_t)code};
        const Built t = plan(one, a, cc, 1), p = plan(one, b, nullptr, 0);
        CHECK(!t.r.rc && !p.r.rc, "rc %d (%s) %d", t.r.rc, t.r.err, p.r.rc);
        if (t.r.rc || p.r.rc) continue;
        CHECK(!memcmp(&t.L.desc[0], &p.L.desc[0], sizeof(ImageDesc)),
              "a transposed descriptor is the swapped chain's");
        CHECK(t.L.ow == p.L.oh && t.L.oh == p.L.ow && t.L.ow == 42 && t.L.oh == 26,
              "final box %dx%d", t.L.ow, t.L.oh);
        CHECK(t.L.transposed && t.L.flips.size() == 1 && t.L.flips[0] == code, "code vector");
        CHECK(t.L.out_elems_per_image == p.L.out_elems_per_image, "bytes per image");
      }
    }
    // one batch, every code: one final shape
    const std::vector<spdl_hj_image_info> eight(8, y420(64, 48));
    const uint8_t all[] = {0, 1, 2, 3, 4, 5, 6, 7};
    const Built b = plan(eight, fin, all, 8);
    CHECK(!b.r.rc && b.L.ow == 42 && b.L.oh == 26 && b.L.transposed, "eight codes: rc=%d %s",
          b.r.rc, b.r.err);
    for (int i = 0; !b.r.rc && i < 8; i++)
      CHECK(b.L.desc[i].ow == (i & 4 ? 26 : 42) && b.L.desc[i].oh == (i & 4 ? 42 : 26) &&
                b.L.desc[i].out_off == (int64_t)i * 42 * 26 * 3,
            "descriptor %d: %dx%d", i, b.L.desc[i].ow, b.L.desc[i].oh);
  }
  // full resolution: the "one size" rule is about final sizes
  {
    const std::vector<spdl_hj_image_info> same{y420(64, 48), y420(64, 48)};
    const std::vector<spdl_hj_image_info> turned{y420(64, 48), y420(48, 64)};
    const uint8_t c0_5[] = {0, 5}, c5_6[] = {5, 6}, c0_3[] = {0, 3};
    const Built bad = plan(same, full, c0_5, 2);
    CHECK(bad.r.rc == SPDL_HJ_ERR_INVALID_ARG && strstr(bad.r.err, "same output size") &&
              strstr(bad.r.err, "48x64"),
          "64x48 at code 0 beside its code-5 partner: rc=%d err=%s", bad.r.rc, bad.r.err);
    const Built ok = plan(turned, full, c0_5, 2);
    CHECK(!ok.r.rc && ok.L.ow == 64 && ok.L.oh == 48 && !ok.L.all_special && ok.L.transposed,
          "64x48 at code 0 beside 48x64 at code 5: rc=%d err=%s", ok.r.rc, ok.r.err);
    const Built t = plan(same, full, c5_6, 2);
    CHECK(!t.r.rc && t.L.ow == 48 && t.L.oh == 64, "codes 5, 6: %dx%d", t.L.ow, t.L.oh);
    const Built f = plan(same, full, c0_3, 2);
    CHECK(!f.r.rc && f.L.ow == 64 && f.L.oh == 48 && !f.L.transposed, "codes 0, 3");
  }
  // views: codes by concatenated view order behind the n image descriptors; a
  // refused view keeps its entry; each group's box is its final one
  {
    int32_t st0[3] = {-7, -7, -7}, st1[2] = {-7, -7};
    HeldViews hv;
    hv.groups.push_back({chain(24, 20), reinterpret_cast<void*>(0x1000), (size_t)3 * 24 * 20 * 3,
                         {{0, {4, 4, 30, 30}}, {0, {0, 0, 70, 10}}, {1, {8, 8, 32, 32}}}, st0});
    hv.groups.push_back({chain(16, 12), reinterpret_cast<void*>(0x2000), (size_t)2 * 16 * 12 * 3,
                         {{1, {0, 0, 0, 0}}, {0, {2, 2, 20, 20}}}, st1});
    const uint8_t vc[] = {5, 6, 0, 7, 2};
    const Built b = plan(two, full, vc, 5, &hv);
    CHECK(!b.r.rc, "views with codes: rc=%d err=%s", b.r.rc, b.r.err);
    const uint8_t want[] = {0, 0, 5, 6, 0, 7, 2};
    CHECK(b.L.flips.size() == 7 && b.L.desc.size() == 7 && !memcmp(b.L.flips.data(), want, 7) &&
              b.L.transposed,
          "view codes (%zu of them)", b.L.flips.size());
    CHECK(st0[0] == 0 && st0[1] == SPDL_HJ_ERR_BAD_GEOMETRY && st0[2] == 0 && st1[0] == 0 &&
              st1[1] == 0,
          "view statuses %d %d %d | %d %d", st0[0], st0[1], st0[2], st1[0], st1[1]);
    if (!b.r.rc && b.L.desc.size() == 7 && b.L.groups.size() == 2) {
      CHECK(b.L.desc[2].ow == 20 && b.L.desc[2].oh == 24 && b.L.desc[4].ow == 24 &&
                b.L.desc[4].oh == 20 && b.L.desc[3].refuse,
            "group 0: %dx%d, %dx%d", b.L.desc[2].ow, b.L.desc[2].oh, b.L.desc[4].ow, b.L.desc[4].oh);
      CHECK(b.L.desc[5].ow == 12 && b.L.desc[5].oh == 16 && b.L.desc[6].ow == 16 &&
                b.L.desc[6].oh == 12,
            "group 1");
      CHECK(b.L.groups[0].ow == 24 && b.L.groups[0].oh == 20 && b.L.groups[1].ow == 16 &&
                b.L.groups[1].oh == 12,
            "group boxes");
    }
    CHECK(plan(two, full, vc, 2, &hv).r.rc == SPDL_HJ_ERR_INVALID_ARG, "n codes for 5 views");
    // a transpose in a planar group alone is refused
    HeldViews hy = hv;
    hy.groups[1].out.pix_fmt = SPDL_HJ_FMT_YUV;
    CHECK(plan(two, full, vc, 5, &hy).r.rc == SPDL_HJ_ERR_INVALID_ARG, "a T view of a YUV group");
    const uint8_t vz[5] = {};
    const Built z = plan(two, full, vz, 5, &hv), none = plan(two, full, nullptr, 0, &hv);
    CHECK(z.L.flips.empty() && digest(z.L) == digest(none.L), "views, all-zero codes");
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
