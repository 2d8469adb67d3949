// ragged_sweep.cpp -- stand-alone, self-checking sweep of ragged submissions
// through the batch planner (spdl_amd/csrc/hj_layout.h), for a sanitizer
// build on the CPU:
//   g++ -std=c++17 -O1 -g -DHJ_HD= -fsanitize=address,undefined -fno-sanitize-recover=all
//       -static-libasan -static-libubsan tests/native/ragged_sweep.cpp
//       spdl_amd/csrc/hj_layout.cpp spdl_amd/csrc/hj_sws.cpp -o ragged_sweep
// Hand-filled probes (no JPEG bytes) of five samplings and a dozen sizes go
// through hj::ragged_layout and build_layout with every combination of chain,
// source crops, orientation codes, dtype, alignment and output path.  Every
// expectation is stated here from the rules (include/spdl_hipjpeg.h "ragged
// batches"), none is read back from the code under test.  Prints one line
// per failed expectation and a count; exit status 1 when any failed.
#include "../../spdl_amd/csrc/hj_layout.h"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>

namespace {

using namespace hj;

int failures = 0;
std::string where;

#define EXPECT(cond, ...)                         \
  do {                                            \
    if (!(cond)) {                                \
      if (failures++ < 40) {                      \
        printf("FAIL %s: %s: ", where.c_str(), #cond); \
        printf(__VA_ARGS__);                      \
        printf("\n");                             \
      }                                           \
    }                                             \
  } while (0)

spdl_hj_image_info frame(int w, int h, int ncomp, int h0, int v0) {
  spdl_hj_image_info p{};
  p.width = w;
  p.height = h;
  p.ncomp = ncomp;
  for (int c = 0; c < ncomp; c++) p.h_samp[c] = p.v_samp[c] = 1;
  p.h_samp[0] = h0;
  p.v_samp[0] = v0;
  p.color = ncomp == 1 ? SPDL_HJ_COLOR_GRAY : SPDL_HJ_COLOR_YCBCR;
  return p;
}

spdl_hj_output chain(int dtype) {
  spdl_hj_output o{};
  o.pix_fmt = SPDL_HJ_FMT_RGB24;
  o.dtype = dtype;
  for (int c = 0; c < 3; c++) o.std[c] = 1.f;
  return o;
}
spdl_hj_output scale(int dtype, int w, int h, int aspect) {
  spdl_hj_output o = chain(dtype);
  o.resize = 1;
  o.fit_w = w;
  o.fit_h = h;
  o.aspect = aspect;
  return o;
}

struct Case {
  const char* name;
  spdl_hj_output out;
};

// The rule of the fused path for one image by itself: u8, full resolution,
// no crop, code 0, "output_path" 0, and swscale's unscaled converter's frames
// -- 4:2:0 with even width and height, 4:2:2 with even width
bool eligible(const spdl_hj_image_info& p, const spdl_hj_output& o, bool cropped, int code,
              int output_path) {
  if (o.dtype != SPDL_HJ_DTYPE_U8 || o.resize || cropped || code || output_path) return false;
  if (p.ncomp != 3 || p.h_samp[0] != 2 || p.width % 2) return false;
  return p.v_samp[0] == 1 || (p.v_samp[0] == 2 && p.height % 2 == 0);
}

void run(const std::vector<spdl_hj_image_info>& infos, const Case& c, bool with_crops,
         bool with_codes, int64_t align, int output_path, PlanCache* cache) {
  const int n = (int)infos.size();
  const int64_t esz = c.out.dtype == SPDL_HJ_DTYPE_U8 ? 1 : 2;
  char tag[160];
  snprintf(tag, sizeof(tag), "%s dtype=%d crops=%d codes=%d align=%lld path=%d", c.name, c.out.dtype,
           with_crops, with_codes, (long long)align, output_path);
  where = tag;
  std::vector<spdl_hj_rect> crops(n, spdl_hj_rect{0, 0, 0, 0});
  std::vector<uint8_t> codes(n, 0);
  for (int i = 0; i < n; i++) {
    const int w = infos[i].width, h = infos[i].height;
    // every third image whole; a 1 x 1 region far out rounds to nothing
    if (with_crops && i % 3 == 1 && w >= 4 && h >= 4) crops[i] = {3, 2, w / 2 + 1, h / 2 + 1};
    if (with_crops && i % 3 == 2) crops[i] = {w + 5, h + 5, 1, 1};
    if (with_codes) codes[i] = (uint8_t)(i % 8);
  }
  std::vector<int64_t> offsets(n + 1, -1);
  std::vector<int32_t> ow(n, -1), oh(n, -1), status(n, -7);
  const int rc = ragged_layout(infos.data(), n, &c.out, with_crops ? crops.data() : nullptr,
                               with_codes ? codes.data() : nullptr, align, offsets.data(), ow.data(),
                               oh.data(), status.data());
  EXPECT(rc == SPDL_HJ_OK, "rc %d", rc);
  if (rc) return;
  // sizes: each image alone through crop_resolve and geometry(), swapped for a transposed code
  int64_t end = 0;
  std::vector<int> want_rc(n, 0);
  bool sizes_differ = false;
  for (int i = 0; i < n; i++) {
    spdl_hj_rect r{0, 0, infos[i].width, infos[i].height};
    int want = SPDL_HJ_OK;
    if (with_crops && !rect_is_none(crops[i])) want = crop_resolve(infos[i], crops[i], &r);
    Geom g{};
    if (!want) {
      const spdl_hj_output o = codes[i] & 4 ? swapped_chain(c.out) : c.out;
      want = geometry(r.w, r.h, &o, &g);
    }
    const int box_rc = want;  // (what ragged_layout, which builds no plan, can know)
    // a size the scaler has no filter for (swscale's own limit, hj_sws.cpp) is
    // the plan cache's to say: the planner refuses that image alone
    if (!want) {
      int hs, vs, prc;
      views::chroma_shifts(frame_of(infos[i]), &hs, &vs);
      const PlanKey key{r.w, r.h, hs, vs, infos[i].ncomp == 1 ? kPlanGray : kPlanYuv,
                        c.out.resize ? c.out.filter : 0, g.sw, g.sh, g.dx, g.dy, g.ow, g.oh};
      if (!cache->get(key, &prc)) want = prc;
    }
    want_rc[i] = want;
    want = box_rc;
    const int fw = want ? 0 : codes[i] & 4 ? g.oh : g.ow, fh = want ? 0 : codes[i] & 4 ? g.ow : g.oh;
    EXPECT(status[i] == want, "image %d status %d want %d", i, status[i], want);
    EXPECT(ow[i] == fw && oh[i] == fh, "image %d: %dx%d want %dx%d", i, ow[i], oh[i], fw, fh);
    EXPECT(offsets[i] % align == 0, "image %d offset %lld", i, (long long)offsets[i]);
    EXPECT(offsets[i] >= end && offsets[i] < end + align, "image %d offset %lld after %lld", i,
           (long long)offsets[i], (long long)end);
    end = offsets[i] + (int64_t)fw * fh * 3 * esz;
    if (!want && (fw != ow[0] || fh != oh[0])) sizes_differ = true;
  }
  EXPECT(offsets[n] == end, "buffer %lld want %lld", (long long)offsets[n], (long long)end);

  // the planner fed those offsets
  std::vector<int64_t> in_off(n), in_size(n, 3000);
  for (int i = 0; i < n; i++) in_off[i] = (int64_t)i * 3328;
  LayoutRequest rq{in_off.data(), in_size.data(), infos.data(), n, &c.out, 128 * 1024, cache};
  rq.crops = with_crops ? crops.data() : nullptr;
  rq.orients = with_codes ? codes.data() : nullptr;
  rq.norients = with_codes ? n : 0;
  rq.ragged = offsets.data();
  rq.out_bytes = offsets[n];
  rq.output_path = output_path;
  Layout L;
  const LayoutResult res = build_layout(rq, L);
  EXPECT(res.rc == SPDL_HJ_OK, "build_layout %d \"%s\"", res.rc, res.err);
  if (res.rc) return;
  EXPECT(L.ragged && (int)L.desc.size() == n, "ragged %d, %zu descriptors", L.ragged, L.desc.size());
  struct Range {
    int64_t first, count;
    bool fused;
  };
  std::vector<Range> ranges;
  int64_t idct_wgs = 0, fused_sum = 0;
  int nfused = 0;
  for (int i = 0; i < n; i++) {
    const ImageDesc& d = L.desc[i];
    EXPECT(d.out_off * esz == offsets[i], "image %d out_off %lld, offset %lld", i,
           (long long)d.out_off, (long long)offsets[i]);
    EXPECT((d.refuse != 0) == (want_rc[i] != 0) && d.refuse == want_rc[i], "image %d refuse %d want %d",
           i, d.refuse, want_rc[i]);
    if (!want_rc[i]) {
      const bool t = codes[i] & 4;
      EXPECT((t ? d.oh : d.ow) == ow[i] && (t ? d.ow : d.oh) == oh[i], "image %d box %dx%d want %dx%d",
             i, d.ow, d.oh, ow[i], oh[i]);
    }
    const bool cropped = with_crops && !rect_is_none(crops[i]);
    const bool fused = !want_rc[i] && eligible(infos[i], c.out, cropped, codes[i], output_path);
    FrameBlocks fb;
    EXPECT(frame_blocks(infos[i], &fb) == SPDL_HJ_OK, "image %d", i);
    if (fused) {
      EXPECT(d.idct_blocks == 0, "image %d is fused-eligible, idct_blocks %d", i, d.idct_blocks);
      const int tw = kFusedThreads / fb.grid.bpm;
      const int64_t tiles = (int64_t)((fb.grid.mcux + tw - 1) / tw) * fb.grid.mcuy;
      EXPECT((int64_t)d.sws_bands * d.sws_chunks == tiles && d.sws_bands == fb.grid.mcuy,
             "image %d: %d x %d fused tiles want %lld", i, d.sws_bands, d.sws_chunks, (long long)tiles);
      fused_sum += tiles;
      nfused++;
    } else if (!cropped || want_rc[i]) {
      EXPECT(d.idct_blocks == (int)fb.nblocks, "image %d idct_blocks %d of %lld", i, d.idct_blocks,
             (long long)fb.nblocks);
    } else {
      EXPECT(d.idct_blocks > 0 && d.idct_blocks <= (int)fb.nblocks, "image %d idct_blocks %d of %lld",
             i, d.idct_blocks, (long long)fb.nblocks);
    }
    EXPECT(d.idct_wg0 == idct_wgs, "image %d idct_wg0 %d want %lld", i, d.idct_wg0, (long long)idct_wgs);
    idct_wgs += (d.idct_blocks + kIdctThreads - 1) / kIdctThreads;
    EXPECT(d.sws_bands >= 1 && d.sws_chunks >= 1, "image %d has no output workgroup", i);
    ranges.push_back({d.sws_wg0, (int64_t)d.sws_bands * d.sws_chunks, fused});
  }
  EXPECT(L.idct_wgs == idct_wgs, "idct_wgs %lld want %lld", (long long)L.idct_wgs, (long long)idct_wgs);
  EXPECT(L.fused_wgs == fused_sum, "fused_wgs %lld want %lld", (long long)L.fused_wgs,
         (long long)fused_sum);
  if (output_path) EXPECT(nfused == 0 && L.fused_wgs == 0, "%d fused with output_path", nfused);
  // the two tile ranges: disjoint, contiguous, the fused one first
  std::sort(ranges.begin(), ranges.end(), [](const Range& a, const Range& b) { return a.first < b.first; });
  int64_t at = 0;
  for (const Range& r : ranges) {
    EXPECT(r.first == at, "tiles at %lld want %lld", (long long)r.first, (long long)at);
    EXPECT(r.fused == (r.first < L.fused_wgs), "tiles at %lld fused %d, fused_wgs %lld",
           (long long)r.first, r.fused, (long long)L.fused_wgs);
    at = r.first + r.count;
  }
  EXPECT(at == L.sws_wgs, "sws_wgs %lld want %lld", (long long)L.sws_wgs, (long long)at);

  // the buffer one byte short; an offset off the element size
  if (offsets[n] > 0) {
    LayoutRequest bad = rq;
    bad.out_bytes = offsets[n] - 1;
    Layout Lb;
    EXPECT(build_layout(bad, Lb).rc == SPDL_HJ_ERR_INVALID_ARG, "a short buffer was accepted");
  }
  if (esz == 2) {
    std::vector<int64_t> odd(offsets);
    odd[n / 2] += 1;
    LayoutRequest bad = rq;
    bad.ragged = odd.data();
    bad.out_bytes = offsets[n] + 2;
    Layout Lb;
    EXPECT(build_layout(bad, Lb).rc == SPDL_HJ_ERR_INVALID_ARG, "an odd f16 offset was accepted");
    EXPECT(Lb.desc.empty(), "L touched");
  }
  // the same request, plain: the one-size rule
  if (sizes_differ) {
    LayoutRequest plain = rq;
    plain.ragged = nullptr;
    Layout Lp;
    const LayoutResult pr = build_layout(plain, Lp);
    EXPECT(pr.rc == SPDL_HJ_ERR_INVALID_ARG &&
               strstr(pr.err, "all images of a batch must produce the same output size"),
           "plain rc %d \"%s\"", pr.rc, pr.err);
  }
}

void refusals(const std::vector<spdl_hj_image_info>& infos, PlanCache* cache) {
  where = "refusals";
  const int n = (int)infos.size();
  const spdl_hj_output rgb = chain(SPDL_HJ_DTYPE_U8);
  std::vector<int64_t> offsets(n + 1);
  std::vector<int32_t> ow(n), oh(n), status(n);
  EXPECT(ragged_layout(infos.data(), n, &rgb, nullptr, nullptr, 64, offsets.data(), ow.data(),
                       oh.data(), status.data()) == SPDL_HJ_OK, "plain rgb24");
  std::vector<int64_t> in_off(n), in_size(n, 3000);
  for (int i = 0; i < n; i++) in_off[i] = (int64_t)i * 3328;
  const auto request = [&](const spdl_hj_output* o) {
    LayoutRequest rq{in_off.data(), in_size.data(), infos.data(), n, o, 128 * 1024, cache};
    rq.ragged = offsets.data();
    rq.out_bytes = offsets[n];
    return rq;
  };
  spdl_hj_output yuv = rgb, jfif = rgb;
  yuv.pix_fmt = SPDL_HJ_FMT_YUV;
  jfif.csc = SPDL_HJ_CSC_JFIF;
  for (const spdl_hj_output* o : {&yuv, &jfif}) {
    Layout L;
    const LayoutResult r = build_layout(request(o), L);
    EXPECT(r.rc == SPDL_HJ_ERR_INVALID_ARG, "pix_fmt %d csc %d: rc %d", o->pix_fmt, o->csc, r.rc);
    EXPECT(L.desc.empty() && L.tables.empty() && L.work.empty() && !L.sws_wgs && !L.total_blocks,
           "L touched");
    EXPECT(ragged_layout(infos.data(), n, o, nullptr, nullptr, 64, offsets.data(), ow.data(),
                         oh.data(), status.data()) == SPDL_HJ_ERR_INVALID_ARG,
           "ragged_layout took pix_fmt %d csc %d", o->pix_fmt, o->csc);
  }
  {
    HeldViews hv;
    int32_t vst = -7;
    hv.groups.push_back({rgb, reinterpret_cast<void*>(0x1000), (size_t)1 << 30,
                         {spdl_hj_view{0, {0, 0, 0, 0}}}, &vst});
    LayoutRequest rq = request(&rgb);
    rq.views = &hv;
    rq.piece_bytes = 0;
    Layout L;
    const LayoutResult r = build_layout(rq, L);
    EXPECT(r.rc == SPDL_HJ_ERR_INVALID_ARG, "views with ragged: rc %d", r.rc);
    EXPECT(L.desc.empty() && L.groups.empty() && vst == -7, "L or the view status touched");
  }
  // alignment below or off the element size
  spdl_hj_output f16 = chain(SPDL_HJ_DTYPE_F16);
  for (int64_t a : {0, 1, 3})
    EXPECT(ragged_layout(infos.data(), n, &f16, nullptr, nullptr, a, offsets.data(), ow.data(),
                         oh.data(), status.data()) == SPDL_HJ_ERR_INVALID_ARG, "f16 align %lld",
           (long long)a);
  EXPECT(ragged_layout(infos.data(), n, &rgb, nullptr, nullptr, 0, offsets.data(), ow.data(), oh.data(),
                       status.data()) == SPDL_HJ_ERR_INVALID_ARG, "u8 align 0");
}

}  // namespace

int main() {
  std::vector<spdl_hj_image_info> infos;
  const int sizes[][2] = {{1, 1},    {2, 2},     {7, 5},     {16, 16},  {17, 16},   {64, 33},
                          {101, 67}, {227, 333}, {640, 480}, {688, 48}, {1040, 16}, {2000, 1500},
                          {1999, 1501}};
  for (const auto& s : sizes) {
    infos.push_back(frame(s[0], s[1], 1, 1, 1));  // gray
    infos.push_back(frame(s[0], s[1], 3, 1, 1));  // 4:4:4
    infos.push_back(frame(s[0], s[1], 3, 2, 1));  // 4:2:2
    infos.push_back(frame(s[0], s[1], 3, 2, 2));  // 4:2:0
    infos.push_back(frame(s[0], s[1], 3, 4, 1));  // 4:1:1
  }
  PlanCache cache;
  int runs = 0;
  for (int dtype : {SPDL_HJ_DTYPE_U8, SPDL_HJ_DTYPE_F16}) {
    const Case cases[] = {
        {"native", chain(dtype)},
        {"fit48", scale(dtype, 48, 48, SPDL_HJ_ASPECT_DECREASE)},
        {"cover64", scale(dtype, 64, 64, SPDL_HJ_ASPECT_INCREASE)},
        {"scale=40:-1", scale(dtype, 40, -1, SPDL_HJ_ASPECT_NONE)},
        {"scale=-2:30", scale(dtype, -2, 30, SPDL_HJ_ASPECT_NONE)},
    };
    for (const Case& c : cases)
      for (int with_crops = 0; with_crops < 2; with_crops++)
        for (int with_codes = 0; with_codes < 2; with_codes++)
          for (int64_t align : {1, 2, 64, 256}) {
            if (align % (dtype == SPDL_HJ_DTYPE_U8 ? 1 : 2)) continue;
            for (int path = 0; path < (c.out.resize ? 1 : 3); path++, runs++)
              run(infos, c, with_crops, with_codes, align, path, &cache);
          }
  }
  refusals(infos, &cache);
  printf("%d runs of %zu images, %d failed expectations\n", runs, infos.size(), failures);
  return failures ? 1 : 0;
}
