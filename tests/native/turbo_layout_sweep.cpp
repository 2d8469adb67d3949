// turbo_layout_sweep.cpp -- stand-alone, self-checking sweep of csc = TURBO
// submissions through the batch planner (spdl_amd/csrc/hj_layout.h), for a
// sanitizer build on the CPU:
//   g++ -std=c++17 -O1 -g -DHJ_HD= -fsanitize=address,undefined -fno-sanitize-recover=all
//       -static-libasan -static-libubsan tests/native/turbo_layout_sweep.cpp
//       spdl_amd/csrc/hj_layout.cpp spdl_amd/csrc/hj_sws.cpp -o turbo_layout_sweep
// Hand-filled probes (no JPEG bytes) go through valid_output, ragged_layout
// and build_layout, plain and ragged.  Every expectation is stated here from
// the rules (include/spdl_hipjpeg.h "Pillow-exact decode"): the tiles of
// turbo_rgb_kernel, 128 x 32 pixels, counted from each image's own size and
// numbered in image order; what the mode refuses, with nothing planned.
// Prints one line per failed expectation and a count; exit status 1 when any
// failed.
#include "../../spdl_amd/csrc/hj_layout.h"

#include <stdio.h>
#include <string.h>

#include <string>

namespace {

using namespace hj;

int failures = 0, checks = 0;
std::string where;

#define EXPECT(cond, ...)                              \
  do {                                                 \
    checks++;                                          \
    if (!(cond)) {                                     \
      if (failures++ < 40) {                           \
        printf("FAIL %s: %s: ", where.c_str(), #cond); \
        printf(__VA_ARGS__);                           \
        printf("\n");                                  \
      }                                                \
    }                                                  \
  } while (0)

constexpr int kTileW = 128, kTileH = 32;  // (stated here, not read from the code under test)

spdl_hj_image_info frame(int w, int h, int ncomp, int h0, int v0) {
  spdl_hj_image_info p{};
  p.width = w;
  p.height = h;
  p.ncomp = ncomp;
  for (int c = 0; c < ncomp; c++) p.h_samp[c] = p.v_samp[c] = 1;
  p.h_samp[0] = h0;
  p.v_samp[0] = v0;
  p.color = ncomp == 1 ? SPDL_HJ_COLOR_GRAY : ncomp == 3 ? SPDL_HJ_COLOR_YCBCR : SPDL_HJ_COLOR_CMYK;
  return p;
}

spdl_hj_output turbo(int dtype, int pix_fmt = SPDL_HJ_FMT_RGB24) {
  spdl_hj_output o{};
  o.pix_fmt = pix_fmt;
  o.dtype = dtype;
  o.csc = SPDL_HJ_CSC_TURBO;
  for (int c = 0; c < 3; c++) o.std[c] = 1.f;
  return o;
}

struct Inputs {
  std::vector<spdl_hj_image_info> infos;
  std::vector<int64_t> in_off, in_size;
  explicit Inputs(std::vector<spdl_hj_image_info> v) : infos(std::move(v)) {
    for (size_t i = 0; i < infos.size(); i++) {
      in_off.push_back((int64_t)i * 3328);
      in_size.push_back(3000);
    }
  }
  LayoutRequest request(const spdl_hj_output* o, PlanCache* cache) const {
    return LayoutRequest{in_off.data(), in_size.data(), infos.data(), (int)infos.size(), o,
                         128 * 1024, cache};
  }
};

// the tiles of every image, in image order, and what the IDCT stage keeps
void check_tiles(const Inputs& in, const Layout& L) {
  int64_t wg = 0;
  for (size_t i = 0; i < in.infos.size(); i++) {
    const ImageDesc& d = L.desc[i];
    const int W = in.infos[i].width, H = in.infos[i].height;
    EXPECT(d.ow == W && d.oh == H && d.dx == 0 && d.dy == 0, "image %zu box %dx%d", i, d.ow, d.oh);
    EXPECT(d.sws_chunks == (W + kTileW - 1) / kTileW && d.sws_bands == (H + kTileH - 1) / kTileH,
           "image %zu: %d x %d tiles of %dx%d", i, d.sws_chunks, d.sws_bands, W, H);
    EXPECT(d.sws_wg0 == wg, "image %zu sws_wg0 %d want %lld", i, d.sws_wg0, (long long)wg);
    wg += (int64_t)d.sws_chunks * d.sws_bands;
    FrameBlocks fb;
    EXPECT(frame_blocks(in.infos[i], &fb) == SPDL_HJ_OK, "image %zu", i);
    EXPECT(d.idct_blocks == (int)fb.nblocks && !d.refuse, "image %zu idct_blocks %d refuse %d", i,
           d.idct_blocks, d.refuse);
    for (int c = 0; c < in.infos[i].ncomp; c++) {
      const int hr = fb.grid.hmax / in.infos[i].h_samp[c], vr = fb.grid.vmax / in.infos[i].v_samp[c];
      EXPECT(d.win_x[c] == 0 && d.win_y[c] == 0 && d.win_w[c] == (W + hr - 1) / hr &&
                 d.win_h[c] == (H + vr - 1) / vr && d.plane_stride[c] >= (d.win_w[c] + 7) / 8 * 8,
             "image %zu component %d: the true plane %dx%d, stride %d", i, c, d.win_w[c], d.win_h[c],
             d.plane_stride[c]);
    }
  }
  EXPECT(L.sws_wgs == wg, "sws_wgs %lld want %lld", (long long)L.sws_wgs, (long long)wg);
  EXPECT(L.tables.empty() && L.hs_wgs == 0 && L.fused_wgs == 0, "a swscale plan was placed");
}

void plain(PlanCache* cache) {
  where = "plain";
  static const int sizes[][2] = {{300, 200}, {1, 1}, {129, 33}, {128, 32}};
  for (int dtype : {SPDL_HJ_DTYPE_U8, SPDL_HJ_DTYPE_BF16})
    for (const auto& s : sizes) {
      const Inputs in({frame(s[0], s[1], 3, 2, 2), frame(s[0], s[1], 1, 1, 1), frame(s[0], s[1], 3, 4, 1),
                       frame(s[0], s[1], 3, 1, 2)});
      const spdl_hj_output o = turbo(dtype, SPDL_HJ_FMT_BGR);
      Layout L;
      const LayoutResult r = build_layout(in.request(&o, cache), L);
      EXPECT(r.rc == SPDL_HJ_OK, "%dx%d: rc %d \"%s\"", s[0], s[1], r.rc, r.err);
      if (r.rc) continue;
      check_tiles(in, L);
      EXPECT(!L.ragged && L.ow == s[0] && L.oh == s[1], "box %dx%d", L.ow, L.oh);
      for (size_t i = 0; i < in.infos.size(); i++)
        EXPECT(L.desc[i].out_off == (int64_t)i * s[0] * s[1] * 3, "image %zu out_off", i);
    }
  // the one-size rule holds
  const Inputs mixed({frame(64, 48, 3, 2, 2), frame(65, 48, 3, 2, 2)});
  const spdl_hj_output o = turbo(SPDL_HJ_DTYPE_U8);
  Layout L;
  const LayoutResult r = build_layout(mixed.request(&o, cache), L);
  EXPECT(r.rc == SPDL_HJ_ERR_INVALID_ARG && strstr(r.err, "same output size"), "rc %d \"%s\"", r.rc,
         r.err);
}

void ragged(PlanCache* cache) {
  where = "ragged";
  const Inputs in({frame(1, 1, 3, 2, 2), frame(640, 480, 3, 2, 2), frame(227, 333, 3, 2, 1),
                   frame(129, 33, 1, 1, 1), frame(17, 5, 3, 1, 4), frame(128, 64, 3, 4, 2)});
  const int n = (int)in.infos.size();
  for (int dtype : {SPDL_HJ_DTYPE_U8, SPDL_HJ_DTYPE_F16})
    for (int64_t align : {1, 2, 256}) {
      const int64_t esz = dtype == SPDL_HJ_DTYPE_U8 ? 1 : 2;
      if (align % esz) continue;
      const spdl_hj_output o = turbo(dtype);
      std::vector<int64_t> offsets(n + 1, -1);
      std::vector<int32_t> ow(n), oh(n), status(n, -7);
      const int rc = ragged_layout(in.infos.data(), n, &o, nullptr, nullptr, align, offsets.data(),
                                   ow.data(), oh.data(), status.data());
      EXPECT(rc == SPDL_HJ_OK, "ragged_layout %d", rc);
      if (rc) continue;
      int64_t end = 0;
      for (int i = 0; i < n; i++) {
        EXPECT(status[i] == 0 && ow[i] == in.infos[i].width && oh[i] == in.infos[i].height,
               "image %d: status %d, %dx%d", i, status[i], ow[i], oh[i]);
        EXPECT(offsets[i] % align == 0 && offsets[i] >= end && offsets[i] < end + align,
               "image %d at %lld after %lld", i, (long long)offsets[i], (long long)end);
        end = offsets[i] + (int64_t)ow[i] * oh[i] * 3 * esz;
      }
      EXPECT(offsets[n] == end, "buffer %lld want %lld", (long long)offsets[n], (long long)end);
      LayoutRequest rq = in.request(&o, cache);
      rq.ragged = offsets.data();
      rq.out_bytes = offsets[n];
      Layout L;
      const LayoutResult r = build_layout(rq, L);
      EXPECT(r.rc == SPDL_HJ_OK, "build_layout %d \"%s\"", r.rc, r.err);
      if (r.rc) continue;
      check_tiles(in, L);
      EXPECT(L.ragged, "not ragged");
      for (int i = 0; i < n; i++)
        EXPECT(L.desc[i].out_off * esz == offsets[i], "image %d out_off %lld", i,
               (long long)L.desc[i].out_off);
      rq.out_bytes = offsets[n] - 1;
      Layout Lb;
      EXPECT(build_layout(rq, Lb).rc == SPDL_HJ_ERR_INVALID_ARG, "a short buffer was accepted");
    }
}

void refusals(PlanCache* cache) {
  where = "refusals";
  spdl_hj_output o = turbo(SPDL_HJ_DTYPE_U8);
  EXPECT(valid_output(&o), "csc 2 at full resolution");
  spdl_hj_output bad = o;
  bad.resize = 1;
  bad.fit_w = bad.fit_h = 64;
  EXPECT(!valid_output(&bad), "csc 2 with a resize");
  bad = o;
  bad.pix_fmt = SPDL_HJ_FMT_YUV;
  EXPECT(!valid_output(&bad), "csc 2 with the planar output");
  bad = o;
  bad.csc = 3;
  EXPECT(!valid_output(&bad), "csc 3");
  bad = o;
  bad.idct = SPDL_HJ_IDCT_SIMPLE;  // (not consulted, and valid)
  EXPECT(valid_output(&bad), "csc 2 with idct simple");

  const Inputs in({frame(64, 48, 3, 2, 2), frame(64, 48, 3, 2, 2)});
  const auto refused = [&](const char* what, LayoutRequest rq, const char* text) {
    Layout L;
    const LayoutResult r = build_layout(rq, L);
    EXPECT(r.rc == SPDL_HJ_ERR_INVALID_ARG && strstr(r.err, text), "%s: rc %d \"%s\"", what, r.rc,
           r.err);
    EXPECT(L.desc.empty() && L.work.empty() && !L.sws_wgs && !L.total_blocks, "%s: L touched", what);
  };
  const uint8_t one[2] = {0, 1}, zero[2] = {0, 0};
  LayoutRequest rq = in.request(&o, cache);
  rq.flips = one;
  rq.nflips = 2;
  refused("a flip", rq, "flip");
  rq = in.request(&o, cache);
  rq.orients = one;
  rq.norients = 2;
  refused("an orientation", rq, "orientation");
  rq = in.request(&o, cache);
  rq.lowres = one;
  rq.nlowres = 2;
  refused("a level", rq, "reduced-size");
  const spdl_hj_rect rects[2] = {{0, 0, 32, 32}, {0, 0, 0, 0}};
  rq = in.request(&o, cache);
  rq.crops = rects;
  refused("a source crop", rq, "source crop");
  {
    HeldViews hv;
    int32_t vst = -7;
    hv.groups.push_back({o, reinterpret_cast<void*>(0x1000), (size_t)1 << 30,
                         {spdl_hj_view{0, {0, 0, 0, 0}}}, &vst});
    rq = in.request(&o, cache);
    rq.views = &hv;
    rq.piece_bytes = 0;
    refused("views", rq, "views");
    EXPECT(vst == -7, "the view status was touched");
  }
  // all-zero flips, codes and levels are the plain submission
  rq = in.request(&o, cache);
  rq.flips = zero;
  rq.nflips = 2;
  rq.lowres = zero;
  rq.nlowres = 2;
  Layout L;
  EXPECT(build_layout(rq, L).rc == SPDL_HJ_OK && L.flips.empty() && L.lowres.empty(), "zero flips");
  check_tiles(in, L);

  // a 4-component frame: refused with its index
  const Inputs cmyk({frame(64, 48, 3, 2, 2), frame(64, 48, 4, 1, 1)});
  Layout Lc;
  const LayoutResult rc = build_layout(cmyk.request(&o, cache), Lc);
  EXPECT(rc.rc == SPDL_HJ_ERR_UNSUPPORTED && rc.image == 1 && strstr(rc.err, "csc=turbo"),
         "CMYK: rc %d image %d \"%s\"", rc.rc, rc.image, rc.err);

  // ragged_layout: this csc at native size alone; JFIF stays refused
  std::vector<int64_t> offsets(3);
  std::vector<int32_t> ow(2), oh(2), status(2);
  const auto layout = [&](const spdl_hj_output* out, const spdl_hj_rect* crops, const uint8_t* codes) {
    return ragged_layout(in.infos.data(), 2, out, crops, codes, 1, offsets.data(), ow.data(),
                         oh.data(), status.data());
  };
  EXPECT(layout(&o, nullptr, nullptr) == SPDL_HJ_OK, "turbo");
  EXPECT(layout(&o, nullptr, zero) == SPDL_HJ_OK, "turbo with zero codes");
  EXPECT(layout(&o, rects, nullptr) == SPDL_HJ_ERR_INVALID_ARG, "turbo with a crop");
  EXPECT(layout(&o, nullptr, one) == SPDL_HJ_ERR_INVALID_ARG, "turbo with a code");
  spdl_hj_output jfif = o;
  jfif.csc = SPDL_HJ_CSC_JFIF;
  EXPECT(layout(&jfif, nullptr, nullptr) == SPDL_HJ_ERR_INVALID_ARG, "jfif");
  rq = in.request(&jfif, cache);
  rq.ragged = offsets.data();
  rq.out_bytes = offsets[2];
  refused("ragged jfif", rq, "csc = swscale");
}

}  // namespace

int main() {
  PlanCache cache;
  plain(&cache);
  ragged(&cache);
  refusals(&cache);
  printf("%d checks, %d failed expectations\n", checks, failures);
  return failures ? 1 : 0;
}
