// lowres_layout_sweep.cpp -- stand-alone, self-checking sweep of reduced-size
// levels (spdl_hj_set_lowres) through the batch planner
// (spdl_amd/csrc/hj_layout.h), for a sanitizer build on the CPU:
//   g++ -std=c++17 -O1 -g -DHJ_HD= -fsanitize=address,undefined -fno-sanitize-recover=all
//       -static-libasan -static-libubsan tests/native/lowres_layout_sweep.cpp
//       spdl_amd/csrc/hj_layout.cpp spdl_amd/csrc/hj_sws.cpp -o lowres_layout_sweep
// Hand-filled probes (no JPEG bytes): W, H in {1, 7, 8, 9, 17, 65535} x level
// 0..3 x gray and chroma ratios 1, 2 and 4.  Every expectation is stated here
// from the rules (include/spdl_hipjpeg.h "reduced-size decode"), none is read
// back from the code under test.  Prints one line per failed expectation and
// a count; exit status 1 when any failed.
#include "../../spdl_amd/csrc/hj_layout.h"

#include <stdio.h>
#include <string.h>

#include <string>

namespace {

using namespace hj;

int failures = 0;
long cases = 0;
std::string where;

#define EXPECT(cond, ...)                              \
  do {                                                 \
    if (!(cond)) {                                     \
      if (failures++ < 40) {                           \
        printf("FAIL %s: %s: ", where.c_str(), #cond); \
        printf(__VA_ARGS__);                           \
        printf("\n");                                  \
      }                                                \
    }                                                  \
  } while (0)

spdl_hj_image_info frame(int w, int h, int ncomp, int h0, int v0) {
  spdl_hj_image_info p{};
  p.width = w;
  p.height = h;
  p.ncomp = ncomp;
  for (int c = 0; c < ncomp; c++) p.h_samp[c] = p.v_samp[c] = 1;
  p.h_samp[0] = h0;
  p.v_samp[0] = v0;
  p.color = ncomp == 1 ? SPDL_HJ_COLOR_GRAY : ncomp == 4 ? SPDL_HJ_COLOR_CMYK : SPDL_HJ_COLOR_YCBCR;
  return p;
}

int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

LayoutResult plan(const spdl_hj_image_info* infos, int n, const spdl_hj_output& out,
                  const uint8_t* levels, int64_t nlevels, PlanCache* cache, Layout& L,
                  const spdl_hj_rect* crops = nullptr) {
  std::vector<int64_t> offs(n), sizes(n);
  for (int i = 0; i < n; i++) {
    offs[i] = 4096 * i;
    sizes[i] = 1000 + i;
  }
  LayoutRequest rq{offs.data(), sizes.data(), infos, n, &out, 0, cache};
  rq.crops = crops;
  rq.lowres = levels;
  rq.nlowres = nlevels;
  L = Layout{};
  return build_layout(rq, L);
}

// one frame at one level, planes only: sizes, strides, workspace bytes, windows, lanes
void one(const spdl_hj_image_info& p, int lv) {
  char tag[96];
  snprintf(tag, sizeof(tag), "%dx%d ncomp %d %dx%d L%d", p.width, p.height, p.ncomp, p.h_samp[0],
           p.v_samp[0], lv);
  where = tag;
  cases++;
  spdl_hj_output o{};
  const uint8_t level = (uint8_t)lv;
  Layout L, L0;
  const LayoutResult r = plan(&p, 1, o, &level, 1, nullptr, L);
  const LayoutResult r0 = plan(&p, 1, o, nullptr, 0, nullptr, L0);
  // (a frame of 2^24 blocks or more is refused at every level alike)
  EXPECT(r.rc == r0.rc, "rc %d, without levels %d", r.rc, r0.rc);
  const int hmax = p.ncomp == 1 ? 1 : p.h_samp[0], vmax = p.ncomp == 1 ? 1 : p.v_samp[0];
  const int64_t mcux = cdiv(p.width, 8 * hmax), mcuy = cdiv(p.height, 8 * vmax);
  const int64_t bpm = p.ncomp == 1 ? 1 : hmax * vmax + p.ncomp - 1;
  EXPECT((r0.rc != 0) == (mcux * mcuy * bpm >= (1 << 24)), "rc %d", r0.rc);
  if (r.rc || r0.rc) return;
  const ImageDesc& d = L.desc[0];
  if (lv == 0) {
    // byte-identical to the plan made without the call
    EXPECT(L.lowres.empty() && L.lowres_images == 0, "levels kept");
    EXPECT(!memcmp(&d, &L0.desc[0], sizeof(ImageDesc)), "descriptor differs");
    EXPECT(L.total_planes == L0.total_planes && L.idct_wgs == L0.idct_wgs &&
               L.max_blocks == L0.max_blocks && L.total_blocks == L0.total_blocks,
           "totals differ");
    return;
  }
  EXPECT(L.lowres.size() == 1 && L.lowres[0] == lv && L.lowres_images == 1, "levels");
  const int P = 8 >> lv, NB = 1 << lv;
  const int64_t fw = cdiv(p.width, NB), fh = cdiv(p.height, NB);
  int64_t total = 0, lanes = 0;
  for (int c = 0; c < p.ncomp; c++) {
    const int hc = p.ncomp == 1 ? 1 : p.h_samp[c], vc = p.ncomp == 1 ? 1 : p.v_samp[c];
    const int64_t bw = mcux * hc, bh = mcuy * vc;
    const int64_t cw = cdiv(fw * hc, hmax), ch = cdiv(fh * vc, vmax);
    const int64_t stride = 8 * cdiv(bw, NB), rows = bh * P;
    EXPECT(d.plane_stride[c] == stride, "c%d stride %d, want %lld", c, d.plane_stride[c],
           (long long)stride);
    EXPECT(d.plane_stride[c] % 8 == 0 && d.plane_off[c] % 256 == 0, "c%d alignment", c);
    EXPECT(d.plane_off[c] == total, "c%d off %lld, want %lld", c, (long long)d.plane_off[c],
           (long long)total);
    total += cdiv(stride * rows, 256) * 256;
    lanes += cdiv(bw, NB) * bh;
    EXPECT(d.win_x[c] == 0 && d.win_y[c] == 0 && d.win_w[c] == cw && d.win_h[c] == ch,
           "c%d window %d,%d %dx%d, want %lldx%lld", c, d.win_x[c], d.win_y[c], d.win_w[c],
           d.win_h[c], (long long)cw, (long long)ch);
    // the window lies in what the stage writes: bw P valid columns, every row
    EXPECT(cw <= bw * P && bw * P <= stride && ch <= rows, "c%d window outside the plane", c);
  }
  EXPECT(L.total_planes == total, "planes %lld, want %lld", (long long)L.total_planes,
         (long long)total);
  EXPECT(d.idct_blocks == lanes, "lanes %d, want %lld", d.idct_blocks, (long long)lanes);
  EXPECT(L.idct_wgs == cdiv(lanes, kIdctThreads) && d.idct_wg0 == 0, "workgroups %lld",
         (long long)L.idct_wgs);
  EXPECT(d.reg_mw == 0, "a region");
  // the front end is the full frame's
  EXPECT(d.width == p.width && d.height == p.height && d.nblocks == mcux * mcuy * bpm &&
             L.total_blocks == L0.total_blocks && d.seg_cap == L0.desc[0].seg_cap,
         "front end differs");
  EXPECT(L.total_planes <= L0.total_planes, "more plane bytes than the full decode");
}

// the chain sees the reduced frame: plan, geometry and tiles equal those of a
// frame of the reduced size decoded in full
void chain_of_reduced_frame(PlanCache* cache) {
  spdl_hj_output o{};
  o.pix_fmt = SPDL_HJ_FMT_RGB24;
  o.resize = 1;
  o.fit_w = o.fit_h = o.pad_w = o.pad_h = 24;
  o.aspect = SPDL_HJ_ASPECT_DECREASE;
  for (int c = 0; c < 3; c++) o.std[c] = 1.f;
  for (int lv = 1; lv <= 3; lv++)
    for (int v0 : {1, 2}) {
      const spdl_hj_image_info p = frame(203, 151, 3, 2, v0);
      const spdl_hj_image_info q = frame((203 + (1 << lv) - 1) >> lv, (151 + (1 << lv) - 1) >> lv, 3, 2, v0);
      char tag[64];
      snprintf(tag, sizeof(tag), "chain L%d v%d", lv, v0);
      where = tag;
      cases++;
      const uint8_t level = (uint8_t)lv;
      Layout L, Q;
      const LayoutResult r = plan(&p, 1, o, &level, 1, cache, L);
      const LayoutResult rq = plan(&q, 1, o, nullptr, 0, cache, Q);
      EXPECT(!r.rc && !rq.rc, "rc %d %d", r.rc, rq.rc);
      if (r.rc || rq.rc) continue;
      const ImageDesc &a = L.desc[0], &b = Q.desc[0];
      EXPECT(!memcmp(&a.sws, &b.sws, sizeof(SwsDesc)), "plan differs");
      EXPECT(a.dx == b.dx && a.dy == b.dy && a.ow == b.ow && a.oh == b.oh, "geometry differs");
      EXPECT(a.sws_bands == b.sws_bands && a.sws_chunks == b.sws_chunks, "tiles differ");
      EXPECT(L.tables == Q.tables, "tables differ");
      for (int c = 0; c < 3; c++)
        EXPECT(a.win_w[c] == b.win_w[c] && a.win_h[c] == b.win_h[c], "c%d window differs", c);
      EXPECT(!L.all_special && !L.fuse_ok, "a reduced image on a full-resolution fast path");
    }
  // native size: never the fused or the unscaled kernel
  spdl_hj_output n{};
  n.pix_fmt = SPDL_HJ_FMT_RGB24;
  for (int c = 0; c < 3; c++) n.std[c] = 1.f;
  const spdl_hj_image_info p = frame(64, 48, 3, 2, 2);
  const uint8_t one_level = 1;
  Layout L;
  where = "native size";
  const LayoutResult r = plan(&p, 1, n, &one_level, 1, cache, L);
  EXPECT(!r.rc && L.ow == 32 && L.oh == 24 && !L.all_special && !L.fuse_ok, "rc %d %dx%d", r.rc,
         L.ow, L.oh);
}

// mixed levels in one submission, and what the planner refuses
void batch_rules(PlanCache* cache) {
  spdl_hj_output o{};
  o.pix_fmt = SPDL_HJ_FMT_RGB24;
  o.resize = 1;
  o.fit_w = o.fit_h = 16;
  for (int c = 0; c < 3; c++) o.std[c] = 1.f;
  const spdl_hj_image_info infos[4] = {frame(50, 37, 3, 2, 2), frame(64, 48, 1, 1, 1),
                                       frame(33, 31, 3, 2, 1), frame(40, 40, 4, 1, 1)};
  where = "mixed";
  {
    const uint8_t lv[4] = {0, 2, 3, 0};
    Layout L, L0;
    const LayoutResult r = plan(infos, 4, o, lv, 4, cache, L);
    const LayoutResult r0 = plan(infos, 4, o, nullptr, 0, cache, L0);
    EXPECT(!r.rc && !r0.rc, "rc %d %d", r.rc, r0.rc);
    EXPECT(L.lowres_images == 2 && L.lowres.size() == 4, "count %d", L.lowres_images);
    // a level-0 image among reduced ones: the full decode's planes and lanes
    EXPECT(L.desc[0].idct_blocks == L0.desc[0].idct_blocks &&
               !memcmp(L.desc[0].plane_stride, L0.desc[0].plane_stride, sizeof(L.desc[0].plane_stride)) &&
               !memcmp(&L.desc[0].sws, &L0.desc[0].sws, sizeof(SwsDesc)),
           "level 0 differs");
    EXPECT(!L.desc[3].refuse && L.desc[3].idct_blocks == L0.desc[3].idct_blocks, "CMYK at level 0");
    // every image's workgroups follow the one before in the flat grid
    int64_t wg = 0;
    for (int i = 0; i < 4; i++) {
      EXPECT(L.desc[i].idct_wg0 == wg, "image %d wg0 %d", i, L.desc[i].idct_wg0);
      wg += cdiv(L.desc[i].idct_blocks, kIdctThreads);
    }
    EXPECT(L.idct_wgs == wg, "workgroups");
  }
  where = "refusals";
  {
    Layout L;
    const uint8_t all0[4] = {0, 0, 0, 0}, short3[3] = {1, 1, 1}, four[4] = {0, 4, 0, 0},
                  cmyk[4] = {0, 0, 0, 1}, some[4] = {1, 0, 0, 0};
    const spdl_hj_rect crops[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    EXPECT(plan(infos, 4, o, short3, 3, cache, L).rc == SPDL_HJ_ERR_INVALID_ARG, "a wrong count");
    EXPECT(plan(infos, 4, o, four, 4, cache, L).rc == SPDL_HJ_ERR_INVALID_ARG, "level 4");
    EXPECT(plan(infos, 4, o, some, 4, cache, L, crops).rc == SPDL_HJ_ERR_INVALID_ARG, "with crops");
    EXPECT(plan(infos, 4, o, all0, 4, cache, L, crops).rc == SPDL_HJ_OK, "all-zero levels with crops");
    spdl_hj_output j = o;
    j.resize = 0;
    j.csc = SPDL_HJ_CSC_JFIF;
    EXPECT(plan(infos, 1, j, some, 1, cache, L).rc == SPDL_HJ_ERR_INVALID_ARG, "with csc = jfif");
    // a 4-component frame with a level: refused alone, the batch plans
    const LayoutResult r = plan(infos, 4, o, cmyk, 4, cache, L);
    EXPECT(!r.rc && L.desc[3].refuse == SPDL_HJ_ERR_UNSUPPORTED && !L.desc[0].refuse, "rc %d refuse %d",
           r.rc, r.rc ? 0 : L.desc[3].refuse);
    // ... and on the planes surface (no output stage) the call's own failure
    const uint8_t l1 = 1;
    EXPECT(plan(&infos[3], 1, spdl_hj_output{}, &l1, 1, nullptr, L).rc == SPDL_HJ_ERR_UNSUPPORTED,
           "CMYK planes");
  }
}

}  // namespace

int main() {
  const int sides[] = {1, 7, 8, 9, 17, 65535};
  for (int w : sides)
    for (int h : sides)
      for (int lv = 0; lv <= 3; lv++) {
        one(frame(w, h, 1, 1, 1), lv);  // gray
        one(frame(w, h, 3, 1, 1), lv);  // 4:4:4: chroma ratio 1
        one(frame(w, h, 3, 2, 2), lv);  // 4:2:0: 2 both ways
        one(frame(w, h, 3, 2, 1), lv);  // 4:2:2
        one(frame(w, h, 3, 1, 2), lv);  // 4:4:0
        one(frame(w, h, 3, 4, 1), lv);  // 4:1:1: ratio 4
      }
  PlanCache cache;
  chain_of_reduced_frame(&cache);
  batch_rules(&cache);
  printf("%ld cases, %d failures\n", cases, failures);
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
