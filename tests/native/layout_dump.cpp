// layout_dump.cpp -- stand-alone dump of the batch planner
// (spdl_amd/csrc/hj_layout.h), for a sanitizer build on the CPU:
//   g++ -std=c++17 -O1 -g -DHJ_HD= -fsanitize=address,undefined -fno-sanitize-recover=all
//       -static-libasan -static-libubsan tests/native/layout_dump.cpp
//       spdl_amd/csrc/hj_layout.cpp spdl_amd/csrc/hj_sws.cpp -o layout_dump
// A fixed table of submissions built from hand-filled probes (no JPEG bytes):
// frame formats, front-end sizes, output chains, planar YUV, source crops,
// views and frames at the format's limits.  One line per case: the return code, the error text, the statuses the
// planner wrote (per image: i:rc; per view group: every entry, -7 = untouched)
// and, for a layout that was built, every scalar of Layout and FNV-1a hashes of
// the raw bytes of desc, tables and work -- the bytes the device gets.
// tests/golden/layout_dump.txt holds the lines the planner printed before it
// became a unit of its own (tests/test_layout.py compares).
//   layout_dump --time   ns per call of two warm-cache workloads instead
#include "../../spdl_amd/csrc/hj_layout.h"

#include <stdio.h>
#include <string.h>

#include <chrono>
#include <string>

namespace {

using namespace hj;

uint64_t fnv1a(const void* p, size_t n) {
  uint64_t h = 1469598103934665603ull;
  const uint8_t* b = static_cast<const uint8_t*>(p);
  for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

// ---- probes ------------------------------------------------------------------
spdl_hj_image_info frame(int w, int h, int ncomp, int h0, int v0, int color) {
  spdl_hj_image_info p{};
  p.width = w;
  p.height = h;
  p.ncomp = ncomp;
  for (int c = 0; c < ncomp; c++) p.h_samp[c] = p.v_samp[c] = 1;
  p.h_samp[0] = h0;
  p.v_samp[0] = v0;
  p.color = color;
  return p;
}
spdl_hj_image_info gray(int w, int h) { return frame(w, h, 1, 1, 1, SPDL_HJ_COLOR_GRAY); }
spdl_hj_image_info y444(int w, int h) { return frame(w, h, 3, 1, 1, SPDL_HJ_COLOR_YCBCR); }
spdl_hj_image_info y422(int w, int h) { return frame(w, h, 3, 2, 1, SPDL_HJ_COLOR_YCBCR); }
spdl_hj_image_info y420(int w, int h) { return frame(w, h, 3, 2, 2, SPDL_HJ_COLOR_YCBCR); }
spdl_hj_image_info y440(int w, int h) { return frame(w, h, 3, 1, 2, SPDL_HJ_COLOR_YCBCR); }
spdl_hj_image_info y411(int w, int h) { return frame(w, h, 3, 4, 1, SPDL_HJ_COLOR_YCBCR); }
spdl_hj_image_info rgb3(int w, int h) { return frame(w, h, 3, 1, 1, SPDL_HJ_COLOR_RGB); }
spdl_hj_image_info four(int w, int h, int color) { return frame(w, h, 4, 1, 1, color); }

// ---- output chains -------------------------------------------------------------
spdl_hj_output chain(int pix_fmt = SPDL_HJ_FMT_RGB24) {
  spdl_hj_output o{};
  o.pix_fmt = pix_fmt;
  for (int c = 0; c < 3; c++) o.std[c] = 1.f;
  return o;
}
spdl_hj_output fit(int w, int h, int aspect = SPDL_HJ_ASPECT_NONE, int pix_fmt = SPDL_HJ_FMT_RGB24) {
  spdl_hj_output o = chain(pix_fmt);
  o.resize = 1;
  o.fit_w = w;
  o.fit_h = h;
  o.aspect = aspect;
  return o;
}
spdl_hj_output pad(spdl_hj_output o, int w, int h) {
  o.pad_w = w;
  o.pad_h = h;
  return o;
}
spdl_hj_output crop(spdl_hj_output o, int w, int h) {
  o.crop_w = w;
  o.crop_h = h;
  return o;
}
spdl_hj_output with(spdl_hj_output o, int spdl_hj_output::*field, int v) {
  o.*field = v;
  return o;
}

// ---- one submission --------------------------------------------------------------
struct Views {
  spdl_hj_output out;
  std::vector<spdl_hj_view> views;
  long slack = 0;        // bytes the group's buffer has beyond (< 0: short of) what it needs
  int per = 0;           // elements per view (slack is counted from per * views)
  bool status = true;    // the group has a status array
};
struct Sub {
  std::string name;
  std::vector<spdl_hj_image_info> infos;
  std::vector<int64_t> sizes;  // file sizes (default 3000 each)
  spdl_hj_output out = chain();
  int64_t piece_bytes = 128 * 1024;
  bool plans = true;
  std::vector<spdl_hj_rect> crops;
  std::vector<Views> groups;
};

void dump(const Sub& s, PlanCache* cache) {
  const int n = (int)s.infos.size();
  std::vector<int64_t> offs(n), sizes(n, 3000);
  for (size_t i = 0; i < s.sizes.size(); i++) sizes[i] = s.sizes[i];
  int64_t total = 0;
  for (int i = 0; i < n; i++) {
    offs[i] = total;
    total += round_up(sizes[i] + 64, 256);
  }
  HeldViews hv;
  std::vector<std::vector<int32_t>> vstat(s.groups.size());
  for (size_t g = 0; g < s.groups.size(); g++) {
    const Views& v = s.groups[g];
    vstat[g].assign(v.views.size(), -7);
    const long esz = v.out.dtype == SPDL_HJ_DTYPE_U8 ? 1 : 2;
    hv.groups.push_back({v.out, reinterpret_cast<void*>(0x1000 * (g + 1)),
                         (size_t)((long)v.per * (long)v.views.size() * esz + v.slack), v.views,
                         v.status ? vstat[g].data() : nullptr});
  }
  PlanCache own;
  LayoutRequest rq{offs.data(), sizes.data(), s.infos.data(), n, &s.out,
                   s.groups.empty() ? s.piece_bytes : 0, s.plans ? (cache ? cache : &own) : nullptr};
  rq.crops = s.crops.empty() ? nullptr : s.crops.data();
  rq.views = s.groups.empty() ? nullptr : &hv;
  Layout L;
  const LayoutResult r = build_layout(rq, L);
  printf("%s rc=%d err=\"%s\" st={", s.name.c_str(), r.rc, r.err);
  if (r.image >= 0) printf("%d:%d", r.image, r.rc);
  printf("}");
  for (size_t g = 0; g < vstat.size(); g++) {
    printf(" v%zu=[", g);
    for (size_t k = 0; k < vstat[g].size(); k++) printf(k ? ",%d" : "%d", vstat[g][k]);
    printf("]");
  }
  if (r.rc) {
    printf("\n");
    return;
  }
  printf(" L{blocks=%lld planes=%lld segs=%lld recs=%lld elems=%lld maxb=%d maxpx=%lld ds=%lld "
         "maxch=%d box=%dx%d sws=%d,%d,%d special=%d fuse=%d yuv=%d,%d,%d cmyk=%lld fused=%d "
         "chain=%lld dswg=%lld idctwg=%lld hswg=%lld hbuf=%lld swswg=%lld ms=%d,%d refused=%d,%d,%d "
         "ndesc=%zu ntab=%zu nwork=%zu multi=[",
         (long long)L.total_blocks, (long long)L.total_planes, (long long)L.total_segs,
         (long long)L.total_recs, (long long)L.out_elems_per_image, L.max_blocks,
         (long long)L.max_px, (long long)L.total_ds, L.max_chunks, L.ow, L.oh, L.sws_bands,
         L.sws_chunks, L.sws_lds, (int)L.all_special, (int)L.fuse_ok, L.yuv_hs, L.yuv_vs,
         (int)L.yuv_gray, (long long)L.cmyk_px, L.fused_tiles, (long long)L.chain_granules,
         (long long)L.ds_wgs, (long long)L.idct_wgs, (long long)L.hs_wgs, (long long)L.total_hbuf,
         (long long)L.sws_wgs, (int)L.ms_side, (int)L.ms_known, L.view_refused,
         L.view_refused_group, L.view_refused_index, L.desc.size(), L.tables.size(),
         L.work.size());
  for (size_t k = 0; k < L.multi.size(); k++)
    printf(k ? ",%d:%016llx" : "%d:%016llx", L.multi[k].first,
           (unsigned long long)fnv1a(&L.multi[k].second, sizeof(spdl_hj_image_info)));
  printf("]");
  for (const Layout::Group& G : L.groups)
    printf(" G{out=%016llx dev=%p first=%d count=%d wg0=%d wgs=%d lds=%d box=%dx%d}",
           (unsigned long long)fnv1a(&G.out, sizeof(G.out)), G.out_dev, G.first, G.count, G.sws_wg0,
           G.sws_wgs, G.sws_lds, G.ow, G.oh);
  printf("} desc=%016llx tables=%016llx work=%016llx\n",
         (unsigned long long)fnv1a(L.desc.data(), L.desc.size() * sizeof(ImageDesc)),
         (unsigned long long)fnv1a(L.tables.data(), L.tables.size() * 4),
         (unsigned long long)fnv1a(L.work.data(), L.work.size() * 4));
}

// ---- the case table ----------------------------------------------------------------
Sub sub(const char* name, std::vector<spdl_hj_image_info> infos, spdl_hj_output out = chain()) {
  Sub s;
  s.name = name;
  s.infos = std::move(infos);
  s.out = out;
  return s;
}
Sub sized(Sub s, std::vector<int64_t> sizes, int64_t piece_bytes) {
  s.sizes = std::move(sizes);
  s.piece_bytes = piece_bytes;
  return s;
}
Sub cropped(Sub s, std::vector<spdl_hj_rect> crops) {
  s.crops = std::move(crops);
  return s;
}
Sub viewed(Sub s, std::vector<Views> groups) {
  s.groups = std::move(groups);
  return s;
}
Views vg(spdl_hj_output out, int ow, int oh, std::vector<spdl_hj_view> views, long slack = 0,
         bool status = true) {
  return {out, std::move(views), slack, ow * oh * 3, status};
}

constexpr spdl_hj_rect kNone{0, 0, 0, 0};
constexpr int32_t kC = SPDL_HJ_CROP_CENTER;

std::vector<Sub> cases() {
  std::vector<Sub> t;
  const spdl_hj_output full = chain(), r32 = fit(32, 32), jfif = with(chain(), &spdl_hj_output::csc, SPDL_HJ_CSC_JFIF);
  const spdl_hj_output yuv = chain(SPDL_HJ_FMT_YUV), yuv32 = fit(32, 24, 0, SPDL_HJ_FMT_YUV);
  spdl_hj_image_info chroma_wider = y444(64, 48);  // no swscale input format
  chroma_wider.h_samp[1] = chroma_wider.h_samp[2] = 2;
  // formats
  t.push_back(sub("fmt-gray", {gray(33, 17)}));
  t.push_back(sub("fmt-444", {y444(33, 17)}));
  t.push_back(sub("fmt-422", {y422(33, 17)}));
  t.push_back(sub("fmt-420", {y420(33, 17)}));
  t.push_back(sub("fmt-440", {y440(33, 17)}));
  t.push_back(sub("fmt-411", {y411(64, 48)}));
  t.push_back(sub("fmt-rgb", {rgb3(33, 17)}));
  t.push_back(sub("fmt-cmyk", {four(33, 17, SPDL_HJ_COLOR_CMYK)}));
  t.push_back(sub("fmt-ycck", {four(33, 17, SPDL_HJ_COLOR_YCCK)}, r32));
  t.push_back(sub("fmt-ycbcrk", {four(33, 17, SPDL_HJ_COLOR_YCBCRK)}, r32));
  t.push_back(sub("fmt-cmyk-jfif", {y444(33, 17), four(33, 17, SPDL_HJ_COLOR_CMYK)}, jfif));
  {
    spdl_hj_image_info p = y420(32, 32);  // 3 does not divide into 2
    p.h_samp[0] = 3;
    p.h_samp[1] = 2;
    t.push_back(sub("fmt-hmax-indivisible", {y420(32, 32), p}, r32));
    p = frame(32, 32, 3, 4, 2, SPDL_HJ_COLOR_YCBCR);  // 8 + 2 + 2 blocks
    p.h_samp[1] = p.h_samp[2] = 2;
    t.push_back(sub("fmt-bpm-12", {p}, r32));
    t.push_back(sub("fmt-too-large", {gray(32768, 32768)}, r32));
    Sub largest = sub("fmt-largest", {gray(32760, 32768)}, r32);
    largest.plans = false;
    t.push_back(largest);
    t.push_back(sub("fmt-empty-frame", {gray(0, 16)}, r32));
    t.push_back(sub("fmt-chroma-wider", {y420(32, 32), chroma_wider}, r32));
  }
  // front end
  const int64_t K = 1024;
  t.push_back(sized(sub("fe-16k", {y420(64, 48), y420(64, 48), y420(64, 48), y420(64, 48)}, r32),
                    {16 * K - 1, 16 * K, 16 * K + 1, 40 * K}, 16 * K));
  t.push_back(sized(sub("fe-128k", {y420(64, 48), y420(64, 48), y420(64, 48), y420(64, 48)}, r32),
                    {128 * K - 1, 128 * K, 128 * K + 1, 1000 * K}, 128 * K));
  t.push_back(sized(sub("fe-max-pieces", {y420(64, 48), y420(64, 48), y420(64, 48)}, r32),
                    {63 * 16 * K + 1, 64 * 16 * K + 1, 200 * 16 * K}, 16 * K));
  {
    spdl_hj_image_info ms = y420(64, 48);
    ms.multiscan = 1;
    t.push_back(sized(sub("fe-multiscan", {ms, y420(64, 48)}, r32), {100 * K, 100 * K}, 16 * K));
  }
  t.push_back(sized(sub("fe-pieces-off", {y420(64, 48), gray(16, 16)}, r32), {900 * K, 1}, 0));
  t.push_back(sized(sub("fe-mixed", {y420(64, 48), y444(16, 16), gray(40, 40), y422(64, 48),
                                     y420(64, 48), y420(64, 48)}, r32),
                    {20 * K, 70 * K, 500, 70 * K, 33 * K, 0}, 16 * K));
  {
    Sub s = sized(sub("fe-no-plans", {y420(64, 48), gray(64, 48)}), {40 * K, 100}, 16 * K);
    s.plans = false;
    t.push_back(s);
  }
  // outputs
  t.push_back(sub("out-full", {y420(48, 32), y420(48, 32)}, full));
  t.push_back(sub("out-fit", {y420(64, 48), y444(40, 30)}, fit(24, 18)));
  t.push_back(sub("out-fit-decrease", {y420(64, 48), y444(30, 40)},
                  pad(fit(32, 32, SPDL_HJ_ASPECT_DECREASE), 32, 32)));
  t.push_back(sub("out-fit-increase", {y420(64, 48), y444(30, 40)},
                  crop(fit(32, 32, SPDL_HJ_ASPECT_INCREASE), 32, 32)));
  t.push_back(sub("out-fit-neg1", {y420(64, 48), y420(64, 48)}, fit(40, -1)));
  t.push_back(sub("out-fit-neg4", {y420(64, 48)}, fit(-4, 37)));
  t.push_back(sub("out-fit-both-neg", {y420(64, 48)}, fit(-1, -2)));
  t.push_back(sub("out-fit-zero", {y420(64, 48)}, fit(0, 20)));
  t.push_back(sub("out-pad", {y422(64, 48)}, pad(fit(30, 20), 41, 33)));
  t.push_back(sub("out-crop", {y422(64, 48)}, crop(fit(30, 20), 17, 9)));
  t.push_back(sub("out-pad-crop", {gray(64, 48)}, crop(pad(fit(30, 20), 40, 40), 36, 12)));
  t.push_back(sub("out-pad-small", {y420(64, 48), y420(64, 48)}, pad(fit(30, 20), 29, 40)));
  t.push_back(sub("out-crop-large", {y420(64, 48)}, crop(fit(30, 20), 31, 20)));
  t.push_back(sub("out-pad-negative", {y420(64, 48)}, pad(fit(30, 20), -1, 40)));
  t.push_back(sub("out-jfif", {y420(48, 32), y444(48, 32), gray(48, 32)}, jfif));
  t.push_back(sub("out-f16", {y420(64, 48)}, with(r32, &spdl_hj_output::dtype, SPDL_HJ_DTYPE_F16)));
  t.push_back(sub("out-bf16-planar", {y420(64, 48)},
                  with(fit(32, 32, 0, SPDL_HJ_FMT_BGR), &spdl_hj_output::dtype, SPDL_HJ_DTYPE_BF16)));
  t.push_back(sub("out-bilinear", {y420(64, 48)}, with(r32, &spdl_hj_output::filter, SPDL_HJ_FILTER_BILINEAR)));
  t.push_back(sub("out-lanczos", {y420(64, 48)}, with(r32, &spdl_hj_output::filter, SPDL_HJ_FILTER_LANCZOS)));
  t.push_back(sub("out-prepass", {y420(640, 480), gray(640, 480), rgb3(640, 480)}, fit(64, 48)));
  t.push_back(sub("out-filter-too-long", {y420(64, 48), gray(776, 16)}, fit(8, 16)));
  t.push_back(sub("out-sizes-differ", {y420(48, 32), y420(48, 32), y420(40, 32)}, full));
  t.push_back(sub("out-special-420", {y420(48, 32), y420(48, 32)}, full));
  t.push_back(sub("out-special-422", {y422(48, 32), y420(48, 32)}, full));
  t.push_back(sub("out-special-odd-height", {y420(48, 32), y420(48, 32), y420(48, 32)}, crop(fit(0, 0), 48, 31)));
  t.push_back(sub("out-special-broken", {y420(48, 32), y444(48, 32)}, full));
  t.push_back(sub("out-fuse-broken", {y420(48, 32), y440(48, 32)}, full));
  t.push_back(sub("out-fuse-gray", {gray(48, 32)}, full));
  t.push_back(sub("out-same-plan", {y420(64, 48), y420(64, 48), y422(64, 48), y420(64, 48)}, r32));
  // planar YUV
  t.push_back(sub("yuv-full-420", {y420(48, 32), y420(48, 32)}, yuv));
  t.push_back(sub("yuv-full-odd", {y420(47, 31)}, yuv));
  t.push_back(sub("yuv-gray", {gray(47, 31), gray(20, 20)}, yuv32));
  t.push_back(sub("yuv-444", {y444(47, 31)}, yuv32));
  t.push_back(sub("yuv-422", {y422(47, 31), y422(64, 48)}, yuv32));
  t.push_back(sub("yuv-mismatch", {y420(48, 32), y422(48, 32), gray(48, 32), y420(48, 32),
                                   rgb3(48, 32), four(48, 32, SPDL_HJ_COLOR_YCCK), y440(48, 32)}, yuv32));
  t.push_back(sub("yuv-first-440", {y440(48, 32), y420(48, 32)}, yuv32));
  t.push_back(sub("yuv-first-411", {y411(48, 32)}, yuv32));
  t.push_back(sub("yuv-first-rgb", {rgb3(48, 32)}, yuv32));
  t.push_back(sub("yuv-pad-on-grid", {y420(64, 48)}, pad(yuv32, 40, 30)));
  t.push_back(sub("yuv-pad-off-grid", {y420(64, 48), y420(64, 48)}, pad(yuv32, 41, 30)));
  t.push_back(sub("yuv-crop-off-grid", {y420(64, 48), y420(64, 48)}, crop(yuv32, 20, 11)));
  t.push_back(sub("yuv-scaled-off-grid", {y420(64, 48)}, pad(fit(31, 24, 0, SPDL_HJ_FMT_YUV), 40, 30)));
  t.push_back(sub("yuv-crop-444", {y444(64, 48)}, crop(yuv32, 21, 11)));
  t.push_back(cropped(sub("yuv-first-crop-refused", {y420(64, 48), y422(64, 48), y420(64, 48), y422(64, 48)}, yuv32),
                      {{0, 0, 100, 10}, {2, 2, 30, 30}, kNone, kNone}));
  t.push_back(sub("yuv-prepass", {y420(640, 480)}, fit(64, 48, 0, SPDL_HJ_FMT_YUV)));
  // source crops
  t.push_back(cropped(sub("crop-whole", {y420(64, 48), gray(64, 48)}, r32), {{0, 0, 64, 48}, {0, 0, 64, 48}}));
  t.push_back(cropped(sub("crop-interior", {y420(64, 48), y444(64, 48), gray(64, 48), y411(64, 48)}, r32),
                      {{17, 9, 30, 20}, {17, 9, 30, 20}, {17, 9, 30, 20}, {17, 9, 30, 20}}));
  t.push_back(cropped(sub("crop-on-mcu", {y420(64, 48), y422(64, 48)}, r32), {{16, 16, 32, 16}, {16, 8, 32, 24}}));
  t.push_back(cropped(sub("crop-off-mcu", {y420(64, 48), y422(64, 48)}, r32), {{15, 15, 34, 18}, {1, 1, 63, 47}}));
  t.push_back(cropped(sub("crop-center", {y420(64, 48), y420(64, 48), gray(64, 48)}, r32),
                      {{kC, kC, 32, 32}, {kC, 4, 31, 32}, {10, kC, 33, 31}}));
  t.push_back(cropped(sub("crop-clamped", {y420(64, 48), y420(64, 48)}, r32), {{-5, -5, 30, 30}, {60, 40, 30, 30}}));
  t.push_back(cropped(sub("crop-unresolved", {y420(64, 48), y420(64, 48), y420(64, 48)}, r32),
                      {{4, 4, 20, 20}, {0, 0, 65, 10}, {8, 8, 40, 1}}));
  t.push_back(cropped(sub("crop-none-among", {y420(64, 48), y420(64, 48), y420(64, 48)}, r32),
                      {kNone, {4, 4, 20, 20}, kNone}));
  t.push_back(cropped(sub("crop-full-res", {y420(64, 48), y420(80, 64)}, full), {{2, 2, 32, 32}, {40, 30, 32, 32}}));
  t.push_back(cropped(sub("crop-full-res-differ", {y420(64, 48), y420(80, 64)}, full),
                      {{2, 2, 32, 32}, {40, 30, 32, 30}}));
  t.push_back(cropped(sub("crop-unsupported-sampling",{y420(64, 48), frame(64, 48, 3, 3, 1, SPDL_HJ_COLOR_YCBCR)}, r32),
                      {{2, 2, 32, 32}, {2, 2, 32, 32}}));
  t.push_back(cropped(sized(sub("crop-pieces", {y420(64, 48), y420(64, 48)}, r32), {50 * K, 10 * K}, 16 * K),
                      {{2, 2, 32, 32}, kNone}));
  t.push_back(cropped(sub("crop-yuv", {y420(64, 48), y420(64, 48)}, yuv32), {{3, 3, 33, 33}, {kC, kC, 40, 40}}));
  // views
  const spdl_hj_output v24 = fit(24, 24), v16 = with(fit(16, 12), &spdl_hj_output::dtype, SPDL_HJ_DTYPE_F16);
  t.push_back(viewed(sub("view-1-group", {y420(64, 48), gray(64, 48)}, full),
                     {vg(v24, 24, 24, {{0, {4, 4, 30, 30}}, {1, {4, 4, 30, 30}}})}));
  t.push_back(viewed(sub("view-2-groups", {y420(64, 48), y444(64, 48), y420(64, 48)}, full),
                     {vg(v24, 24, 24, {{0, {4, 4, 30, 30}}, {0, {30, 20, 30, 28}}, {1, {0, 0, 16, 16}}}),
                      vg(v16, 16, 12, {{1, {40, 30, 24, 18}}, {0, {17, 1, 9, 9}}})}));
  t.push_back(viewed(sub("view-3-groups", {y420(64, 48), y422(64, 48)}, full),
                     {vg(v24, 24, 24, {{1, {4, 4, 30, 30}}}), vg(v16, 16, 12, {{0, {1, 1, 9, 9}}}),
                      vg(fit(8, 8), 8, 8, {{1, {50, 40, 10, 8}}, {0, {50, 40, 10, 8}}})}));
  t.push_back(viewed(sub("view-4-groups", {y420(64, 48), gray(33, 17)}, full),
                     {vg(v24, 24, 24, {{0, {4, 4, 30, 30}}}), vg(v16, 16, 12, {{1, {1, 1, 9, 9}}}),
                      vg(fit(8, 8), 8, 8, {{0, {50, 40, 10, 8}}}),
                      vg(with(v24, &spdl_hj_output::pix_fmt, SPDL_HJ_FMT_BGR), 24, 24, {{1, kNone}})}));
  t.push_back(viewed(sub("view-image-without", {y420(64, 48), y420(64, 48), y420(64, 48)}, full),
                     {vg(v24, 24, 24, {{2, {4, 4, 30, 30}}, {0, {8, 8, 8, 8}}})}));
  t.push_back(viewed(sub("view-whole-frame", {y420(64, 48), y420(64, 48)}, full),
                     {vg(v24, 24, 24, {{0, kNone}, {0, {8, 8, 8, 8}}, {1, {0, 0, 64, 48}}})}));
  t.push_back(viewed(sub("view-full-res", {y420(64, 48), y444(64, 48)}, full),
                     {vg(full, 20, 10, {{0, {8, 8, 20, 10}}, {1, {9, 9, 20, 10}}})}));
  t.push_back(viewed(sub("view-center", {y420(64, 48)}, full),
                     {vg(v24, 24, 24, {{0, {kC, kC, 32, 32}}, {0, {kC, 0, 33, 32}}})}));
  t.push_back(viewed(sub("view-unresolved", {y420(64, 48), y420(64, 48)}, full),
                     {vg(v24, 24, 24, {{0, {4, 4, 30, 30}}, {0, {0, 0, 70, 10}}, {1, {0, 0, 10, 1}}})}));
  t.push_back(viewed(sub("view-all-unresolved", {y420(64, 48)}, full),
                     {vg(v24, 24, 24, {{0, {0, 0, 70, 10}}, {0, {0, 0, 10, 1}}})}));
  t.push_back(viewed(sub("view-bad-geometry", {y420(64, 48)}, full),
                     {vg(pad(fit(-1, 20), 30, 30), 30, 30, {{0, {4, 4, 20, 20}}, {0, {4, 4, 40, 20}}})}));
  t.push_back(viewed(sub("view-filter-too-long", {gray(776, 16), gray(64, 16)}, full),
                     {vg(fit(8, 16), 8, 16, {{1, {0, 0, 32, 16}}, {0, kNone}, {0, {0, 0, 100, 16}}})}));
  t.push_back(viewed(sub("view-sizes-differ", {y420(64, 48)}, full),
                     {vg(v24, 24, 24, {{0, {4, 4, 30, 30}}}),
                      vg(full, 20, 10, {{0, {8, 8, 20, 10}}, {0, {8, 8, 20, 12}}})}));
  t.push_back(viewed(sub("view-buffer-exact", {y420(64, 48)}, full),
                     {vg(v16, 16, 12, {{0, {4, 4, 30, 30}}, {0, {0, 0, 70, 10}}}, 0)}));
  t.push_back(viewed(sub("view-buffer-short", {y420(64, 48)}, full),
                     {vg(v24, 24, 24, {{0, {0, 0, 70, 10}}}),
                      vg(v16, 16, 12, {{0, {4, 4, 30, 30}}, {0, {0, 0, 70, 10}}}, -1)}));
  t.push_back(viewed(sub("view-no-status", {y420(64, 48)}, full),
                     {vg(v24, 24, 24, {{0, {4, 4, 30, 30}}, {0, {0, 0, 70, 10}}}, 0, false)}));
  t.push_back(viewed(sub("view-unsupported-sampling", {y420(64, 48), chroma_wider}, full),
                     {vg(v24, 24, 24, {{0, {4, 4, 30, 30}}, {1, kNone}})}));
  t.push_back(viewed(sub("view-unsupported-rect", {y420(64, 48), chroma_wider}, full),
                     {vg(v24, 24, 24, {{0, {4, 4, 30, 30}}, {1, {4, 4, 30, 30}}})}));
  t.push_back(viewed(sub("view-prepass", {y420(640, 480), y420(64, 48)}, full),
                     {vg(fit(64, 48), 64, 48, {{0, kNone}, {1, kNone}, {0, {0, 0, 600, 400}}})}));
  t.push_back(viewed(sized(sub("view-large-files", {y420(64, 48), y420(64, 48)}, full), {900 * K, 20 * K}, 16 * K),
                     {vg(v24, 24, 24, {{0, {4, 4, 30, 30}}, {1, {4, 4, 30, 30}}})}));
  t.push_back(viewed(sub("view-cmyk", {four(64, 48, SPDL_HJ_COLOR_CMYK), rgb3(64, 48)}, full),
                     {vg(v24, 24, 24, {{0, {4, 4, 30, 30}}, {1, {4, 4, 30, 30}}})}));
  return t;
}

// One plan key reached by two images, and by an image and a view (the second
// submission shares the first one's cache): the blob is placed once each time
void shared_cache_cases() {
  PlanCache cache;
  dump(sub("share-images", {y420(64, 48), y420(64, 48)}, fit(24, 24)), &cache);
  dump(viewed(sub("share-image-view", {y420(80, 64), y420(64, 48)}, chain()),
              {vg(fit(24, 24), 24, 24, {{0, {8, 8, 64, 48}}, {1, kNone}, {1, {0, 0, 64, 48}}})}),
       &cache);
}

// More distinct plans in one batch than the cache holds (512): it empties
// mid-batch, and the images that come back to the first key get a new plan,
// placed again (the table pool goes by the plan, which it keeps alive)
void eviction_case() {
  Sub s = sub("cache-evicts", {}, fit(16, 16));
  for (int i = 0; i < 520; i++) s.infos.push_back(gray(16 + i, 16));
  s.infos.push_back(gray(16, 16));
  s.infos.push_back(gray(16 + 519, 16));
  PlanCache cache;
  dump(s, &cache);
}

// Frames at the format's limits (printed last: the lines above stay in place):
// sides of 65535 among ordinary images, the three limits of the scale (output
// sides over 65535, 256 taps, a ratio of 32768), nblocks >= 2^24 beside
// ordinary neighbours, and rectangles at the far end of a 65535-pixel side.
void extreme_cases() {
  const spdl_hj_output full = chain(), r32 = fit(32, 32), v24 = fit(24, 24);
  dump(sub("ext-wide-444", {y420(64, 48), y444(65535, 8), y420(64, 48)}, fit(2048, 8)), nullptr);
  dump(sub("ext-tall-420", {y420(64, 48), y420(17, 65535), y420(64, 48)}, fit(17, 2048)), nullptr);
  dump(sub("ext-tall-411", {y411(16, 65535)}, fit(16, 4096)), nullptr);
  dump(sub("ext-wide-440", {y440(65535, 17)}, fit(4096, 17)), nullptr);
  dump(sub("ext-full-gray", {gray(65535, 1), gray(65535, 1)}, full), nullptr);
  dump(sub("ext-full-420-odd", {y420(65535, 16)}, full), nullptr);
  dump(sub("ext-full-420-even", {y420(65534, 16)}, full), nullptr);
  dump(sub("ext-full-tall-422", {y422(8, 65535)}, full), nullptr);
  dump(sub("ext-f16-planar", {y444(1, 65535)}, with(with(chain(SPDL_HJ_FMT_RGB), &spdl_hj_output::dtype,
                                                         SPDL_HJ_DTYPE_F16), &spdl_hj_output::resize, 0)),
       nullptr);
  dump(sub("ext-yuv-420", {y420(65534, 16)}, fit(2048, 16, 0, SPDL_HJ_FMT_YUV)), nullptr);
  dump(sub("ext-yuv-full", {y420(65535, 17)}, chain(SPDL_HJ_FMT_YUV)), nullptr);
  // the limits of the scale: 40 -> 1 is the only one swscale takes (a refused
  // scale fails its call, so one call each)
  dump(sub("ext-ratio-40", {gray(40, 16), gray(16, 40)}, fit(1, 1)), nullptr);
  for (int src : {32767, 32768, 32769, 40000, 65535}) {
    dump(sub(("ext-ratio-h-" + std::to_string(src)).c_str(), {gray(40, 16), gray(src, 16)}, fit(1, 16)), nullptr);
    dump(sub(("ext-ratio-v-" + std::to_string(src)).c_str(), {gray(16, 40), gray(16, src)}, fit(16, 1)), nullptr);
  }
  dump(sub("ext-ratio-chroma", {y422(64, 16), y422(65535, 16)}, fit(2, 16)), nullptr);
  dump(sub("ext-out-65535", {gray(32768, 8)}, fit(65535, 8)), nullptr);
  dump(sub("ext-out-over-upscale", {gray(64, 8), gray(32768, 8)}, fit(65536, 8)), nullptr);
  dump(sub("ext-out-over-pad", {gray(32768, 8)}, pad(fit(65535, 8), 65536, 8)), nullptr);
  // nblocks >= 2^24 and its neighbours
  dump(sub("ext-too-large-first", {y444(65535, 65535), y420(64, 48)}, r32), nullptr);
  dump(sub("ext-too-large-middle", {y420(64, 48), y444(65535, 65535), y420(64, 48)}, r32), nullptr);
  dump(viewed(sub("ext-too-large-viewed", {y420(64, 48), y444(65535, 65535)}, full),
              {vg(v24, 24, 24, {{0, {4, 4, 30, 30}}, {1, {0, 0, 64, 64}}})}),
       nullptr);
  // rectangles at the far end
  dump(cropped(sub("ext-crop-far", {y420(65535, 17), y411(17, 65535), gray(65535, 8), y420(64, 48)}, r32),
               {{65535 - 70, 0, 64, 8}, {0, 65535 - 70, 8, 64}, {65535 - 9, 0, 64, 8}, kNone}),
       nullptr);
  dump(cropped(sub("ext-crop-whole-span", {y444(65535, 8), y444(65535, 8)}, fit(2048, 8)),
               {{0, 0, 65535, 8}, kNone}),
       nullptr);
  dump(viewed(sub("ext-view-ends", {y444(65535, 8), y420(64, 48), y420(16, 65535)}, full),
              {vg(v24, 24, 24, {{0, {0, 0, 64, 8}}, {0, {65535 - 64, 0, 64, 8}}, {1, kNone},
                                {2, {0, 65535 - 65, 8, 64}}, {2, {0, 0, 8, 64}}})}),
       nullptr);
}

// ---- --time ---------------------------------------------------------------------------
double ns_per_call(const Sub& s, int reps) {
  const int n = (int)s.infos.size();
  std::vector<int64_t> offs(n), sizes(n, 110000);
  for (int i = 0; i < n; i++) offs[i] = (int64_t)i * round_up(110000 + 64, 256);
  HeldViews hv;
  std::vector<std::vector<int32_t>> vstat(s.groups.size());
  for (size_t g = 0; g < s.groups.size(); g++) {
    const Views& v = s.groups[g];
    vstat[g].assign(v.views.size(), 0);
    hv.groups.push_back({v.out, reinterpret_cast<void*>(0x1000), (size_t)v.per * v.views.size(), v.views,
                         vstat[g].data()});
  }
  PlanCache cache;
  LayoutRequest rq{offs.data(), sizes.data(), s.infos.data(), n, &s.out,
                   s.groups.empty() ? s.piece_bytes : 0, &cache};
  rq.views = s.groups.empty() ? nullptr : &hv;
  long long sink = 0;
  auto once = [&] {
    Layout L;
    const LayoutResult r = build_layout(rq, L);
    sink += r.rc + (long long)L.sws_wgs + (long long)L.desc.size();
  };
  once();  // (warms the plan cache)
  const auto t0 = std::chrono::steady_clock::now();
  for (int k = 0; k < reps; k++) once();
  const auto t1 = std::chrono::steady_clock::now();
  if (sink == 42) printf(" ");
  return std::chrono::duration<double, std::nano>(t1 - t0).count() / reps;
}

int time_mode() {
  Sub batch = sub("batch256", {}, pad(fit(224, 224, SPDL_HJ_ASPECT_DECREASE), 224, 224));
  for (int i = 0; i < 256; i++) batch.infos.push_back(y420(500, 375));
  // tools/views_bench.py: 32 images of 640 x 480, two views to 224 x 224 and
  // six to 96 x 96 of each (rectangles from a fixed generator)
  Sub vb = sub("views32x8", {}, chain());
  for (int i = 0; i < 32; i++) vb.infos.push_back(y420(640, 480));
  Views big = vg(fit(224, 224), 224, 224, {}), small = vg(fit(96, 96), 96, 96, {});
  uint32_t seed = 12345;
  auto next = [&](int lo, int hi) {
    seed = seed * 1664525u + 1013904223u;
    return lo + (int)((seed >> 8) % (uint32_t)(hi - lo + 1));
  };
  for (int i = 0; i < 32; i++)
    for (int k = 0; k < 8; k++) {
      const int w = k < 2 ? next(180, 640) : next(100, 340), h = k < 2 ? next(140, 480) : next(80, 260);
      (k < 2 ? big : small).views.push_back({i, {next(0, 640 - w), next(0, 480 - h), w, h}});
    }
  vb.groups = {big, small};
  printf("batch256 %.0f ns/call\nviews32x8 %.0f ns/call\n", ns_per_call(batch, 2000),
         ns_per_call(vb, 2000));
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--time")) return time_mode();
  for (const Sub& s : cases()) dump(s, nullptr);
  shared_cache_cases();
  eviction_case();
  extreme_cases();
  return 0;
}
