// hj_layout.cpp -- the batch planner (hj_layout.h): geometry of the output
// chain, the per-image front-end and IDCT accounting, and the one placement of
// an output's plan that images and views share.
#include "hj_layout.h"

#include <stdio.h>

#include <algorithm>
#include <map>

#include "hj_sws_tile.h"

namespace hj {

const char* status_str(int s) {
  switch (s) {
    case SPDL_HJ_OK: return "OK";
    case SPDL_HJ_ERR_NOT_JPEG: return "not a JPEG";
    case SPDL_HJ_ERR_UNSUPPORTED: return "unsupported JPEG (arithmetic, lossless, 12-bit or CMYK)";
    case SPDL_HJ_ERR_BAD_HEADER: return "corrupt JPEG header";
    case SPDL_HJ_ERR_BAD_HUFFMAN: return "corrupt entropy-coded data";
    case SPDL_HJ_ERR_TRUNCATED: return "truncated entropy-coded data";
    case SPDL_HJ_ERR_BAD_RESTART: return "restart marker mismatch";
    case SPDL_HJ_ERR_BAD_GEOMETRY: return "invalid resize geometry";
    case SPDL_HJ_ERR_INVALID_ARG: return "invalid argument";
    case SPDL_HJ_ERR_HIP: return "HIP runtime error";
    case SPDL_HJ_ERR_OOM: return "out of device memory";
    case SPDL_HJ_ERR_HANDOFF: return "entropy piece hand-off gave up";
    default: return "unknown error";
  }
}

static int64_t rescale_rnd(int64_t a, int64_t b, int64_t c) { return (a * b + c / 2) / c; }

int geometry(int w, int h, const spdl_hj_output* o, Geom* g, int hs, int vs) {
  if (w <= 0 || h <= 0) return SPDL_HJ_ERR_BAD_GEOMETRY;
  if (!o->resize) {
    *g = {w, h, 0, 0, w, h};
    return SPDL_HJ_OK;
  }
  if (o->pad_w < 0 || o->pad_h < 0 || o->crop_w < 0 || o->crop_h < 0)
    return SPDL_HJ_ERR_BAD_GEOMETRY;
  // vf_scale's ff_scale_adjust_dimensions: 0 is the input size; -n keeps the
  // aspect ratio from the other side and makes the result divisible by n
  // (av_rescale: nearest, ties away from zero); both negative: the input size
  int64_t fw = o->fit_w ? o->fit_w : w, fh = o->fit_h ? o->fit_h : h;
  const int64_t dw = fw < -1 ? -fw : 1, dh = fh < -1 ? -fh : 1;
  if (fw < 0 && fh < 0) {
    fw = w;
    fh = h;
  }
  if (fw < 0) fw = rescale_rnd(fh, w, (int64_t)h * dw) * dw;
  if (fh < 0) fh = rescale_rnd(fw, h, (int64_t)w * dh) * dh;
  int64_t sw = fw, sh = fh;
  if (o->aspect != SPDL_HJ_ASPECT_NONE) {
    int64_t tw = rescale_rnd(fh, w, h), th = rescale_rnd(fw, h, w);
    if (o->aspect == SPDL_HJ_ASPECT_DECREASE) {
      sw = tw < fw ? tw : fw;
      sh = th < fh ? th : fh;
    } else {
      sw = tw > fw ? tw : fw;
      sh = th > fh ? th : fh;
    }
  }
  if (sw < 1) sw = 1;
  if (sh < 1) sh = 1;
  int64_t cw = sw, ch = sh, px = 0, py = 0;
  if (o->pad_w > 0 && o->pad_h > 0) {
    cw = o->pad_w;
    ch = o->pad_h;
    if (cw < sw || ch < sh) return SPDL_HJ_ERR_BAD_GEOMETRY;
    // a subsampled frame: vf_pad rounds an input or box size that is no
    // multiple of the chroma ratio in ways not pinned here -- refused
    if (sw % hs || cw % hs || sh % vs || ch % vs) return SPDL_HJ_ERR_BAD_GEOMETRY;
    px = (cw - sw) / 2 / hs * hs;
    py = (ch - sh) / 2 / vs * vs;
  }
  int64_t ow = cw, oh = ch, cx = 0, cy = 0;
  if (o->crop_w > 0 && o->crop_h > 0) {
    ow = o->crop_w;
    oh = o->crop_h;
    if (ow > cw || oh > ch) return SPDL_HJ_ERR_BAD_GEOMETRY;
    // (vf_crop would shrink such a size to a multiple without saying so)
    if (ow % hs || oh % vs) return SPDL_HJ_ERR_BAD_GEOMETRY;
    cx = (cw - ow) / 2 / hs * hs;
    cy = (ch - oh) / 2 / vs * vs;
  }
  if (sw > 65535 || sh > 65535 || ow > 65535 || oh > 65535) return SPDL_HJ_ERR_BAD_GEOMETRY;
  *g = {(int)sw, (int)sh, (int)(px - cx), (int)(py - cy), (int)ow, (int)oh};
  return SPDL_HJ_OK;
}

bool valid_output(const spdl_hj_output* o) {
  // the JFIF and TURBO conversions have no scaler: full resolution only
  // ... and the planar output is u8 planes of swscale's scaler alone
  if (o && o->pix_fmt == SPDL_HJ_FMT_YUV &&
      (o->dtype != SPDL_HJ_DTYPE_U8 || o->csc != SPDL_HJ_CSC_SWSCALE))
    return false;
  return o && o->pix_fmt >= 0 && o->pix_fmt <= SPDL_HJ_FMT_YUV && (o->dtype >= 0 && o->dtype <= 2) &&
         (o->idct == 0 || o->idct == 1) && (o->filter >= 0 && o->filter <= 2) &&
         o->aspect >= 0 && o->aspect <= 2 &&
         (o->csc == SPDL_HJ_CSC_SWSCALE ||
          ((o->csc == SPDL_HJ_CSC_JFIF || o->csc == SPDL_HJ_CSC_TURBO) && !o->resize));
}

views::Frame frame_of(const spdl_hj_image_info& p) {
  views::Frame f{p.width, p.height, p.ncomp, {}, {}};
  for (int c = 0; c < kMaxComp; c++) {
    f.h_samp[c] = p.h_samp[c];
    f.v_samp[c] = p.v_samp[c];
  }
  return f;
}

int crop_resolve(const spdl_hj_image_info& p, const spdl_hj_rect& in, spdl_hj_rect* out) {
  views::Rect r;
  const int rc = views::resolve(frame_of(p), views::Rect{in.x, in.y, in.w, in.h}, &r);
  if (!rc) *out = {r.x, r.y, r.w, r.h};
  return rc;
}

int frame_blocks(const spdl_hj_image_info& p, FrameBlocks* fb) {
  fb->frame = frame_of(p);
  fb->grid = views::grid_of(fb->frame);
  const views::Grid& g = fb->grid;
  if (p.ncomp == 1) {
    fb->bw[0] = g.mcux;
    fb->bh[0] = g.mcuy;
  } else {
    for (int c = 0; c < p.ncomp; c++) {
      if (g.hmax % p.h_samp[c] || g.vmax % p.v_samp[c]) return SPDL_HJ_ERR_UNSUPPORTED;
      fb->bw[c] = g.mcux * p.h_samp[c];
      fb->bh[c] = g.mcuy * p.v_samp[c];
    }
    if (g.bpm > kMaxBpm) return SPDL_HJ_ERR_UNSUPPORTED;
  }
  fb->nblocks = (int64_t)g.mcux * g.mcuy * g.bpm;
  return SPDL_HJ_OK;
}

namespace {

// plan -> offset in the table pool: a plan's blob is placed once.  `alive`
// holds every placed plan until the layout is built: the cache may evict (and
// free) a plan mid-batch, and a new plan at a recycled address must not match
// a stale `placed` entry
struct TablePool {
  std::map<const PackedPlan*, int64_t> placed;
  std::vector<std::shared_ptr<const PackedPlan>> alive;
  int64_t place(std::vector<int32_t>& tables, const std::shared_ptr<const PackedPlan>& plan) {
    auto it = placed.find(plan.get());
    if (it == placed.end()) {
      it = placed.emplace(plan.get(), (int64_t)tables.size()).first;
      alive.push_back(plan);
      tables.insert(tables.end(), plan->blob.begin(), plan->blob.end());
    }
    return it->second;
  }
};

// The one output size of a batch's images, or of a group's views: set by the
// first of them that gets that far
struct BoxSize {
  bool set = false;
  int ow = 0, oh = 0;
};

// What place_output made of an output: rc == 0, its plan (nullptr: the batch
// has no swscale stage); else the step that refused it.
enum PlaceStep { kPlaced, kAtGeometry, kAtSize, kAtSampling, kAtFirstFormat, kAtPlanar, kAtFilter };
struct Placement {
  int rc;
  PlaceStep at;
  const PackedPlan* plan;
};

// THE policy: which refusals of place_output cost one output alone (the rest
// of the batch decodes) and which fail the call.  A planar image off the
// batch's format or off its chroma grid is refused alone.  A view whose size
// the chain cannot take -- BAD_GEOMETRY from geometry(), or a scale filter too
// long -- is refused alone as well; the same two fail an image's call, as
// does everything else.
// (An image of a ragged submission has a box of its own, so it is refused
// alone where a view is.)
bool refused_alone(bool view, const Placement& pl) {
  return pl.at == kAtPlanar ||
         (view && pl.rc == SPDL_HJ_ERR_BAD_GEOMETRY && (pl.at == kAtGeometry || pl.at == kAtFilter));
}

struct Planner {
  const LayoutRequest& rq;
  Layout& L;
  LayoutResult res;
  TablePool pool;
  BoxSize size;           // the images' output size (L.ow x L.oh)
  bool have_fmt = false;  // the planar output's frame format is set (L.yuv_*)
  std::vector<uint8_t> fused_image;  // a ragged submission's fused-eligible images

  // The submission's orientation codes (orients, else flips) and descriptor
  // k's: image k of a plain submission, or view k - n of a views submission
  const uint8_t* codes() const { return rq.orients ? rq.orients : rq.flips; }
  int64_t ncodes() const { return rq.orients ? rq.norients : rq.nflips; }
  int code_of(int64_t k) const {
    const int64_t q = rq.views ? k - rq.n : k;
    return codes() && q >= 0 && q < ncodes() ? codes()[q] : 0;
  }

  int fail(int i, int rc, const char* what) {
    res.rc = rc;
    res.image = i;
    snprintf(res.err, sizeof(res.err), "Failed to decode an image. (image %d: %s)", i,
             what ? what : status_str(rc));
    return rc;
  }
  // (what place_output left in d.ow x d.oh against the box it had to match)
  int size_mismatch(const char* fmt, const BoxSize& box, size_t a, size_t b, const ImageDesc& d) {
    res.rc = SPDL_HJ_ERR_INVALID_ARG;
    const bool t = code_of(&d - L.desc.data()) & 4;  // (a transposed output: its final box)
    snprintf(res.err, sizeof(res.err), fmt, a, box.ow, box.oh, b, t ? d.oh : d.ow, t ? d.ow : d.oh);
    return res.rc;
  }

  // an output the host refuses alone (ImageDesc::refuse): its one output
  // workgroup reports the status, every other kernel skips it
  void refuse(ImageDesc& d, int why) {
    d.refuse = why;
    d.sws_wg0 = (int32_t)L.sws_wgs++;
    d.sws_bands = d.sws_chunks = 1;
    L.sws_bands = std::max(L.sws_bands, 1);
    L.sws_chunks = std::max(L.sws_chunks, 1);
  }

  // The single writer of the IDCT region: idct_kernel visits MCU rectangle m
  // of the grid (gray: its blocks) -- a source crop's, or the bounding one of
  // an image's views (none: no block)
  static void set_region(ImageDesc& d, const views::Grid& grid, const views::McuRect& m) {
    d.idct_blocks = views::idct_blocks(grid, m);
    d.reg_mx0 = m.mx0;
    d.reg_my0 = m.my0;
    d.reg_mw = m.mw;
    d.reg_mh = m.mh;
    d.reg_mw_magic = idct_div_magic((uint32_t)std::max(m.mw, 1));
  }

  // The output kernels' window of rectangle r of the frame, per component
  static void set_windows(ImageDesc& d, const views::Frame& f, const views::Grid& grid,
                          const views::Rect& r) {
    for (int c = 0; c < f.ncomp; c++) {
      const views::Window w = views::window(f, grid, r, c);
      d.win_x[c] = w.x;
      d.win_y[c] = w.y;
      d.win_w[c] = w.w;
      d.win_h[c] = w.h;
    }
  }

  // d's workgroups in the flat IDCT grid, in image order (d.idct_blocks is set)
  void idct_share(ImageDesc& d) {
    if (d.idct_blocks > L.max_blocks) L.max_blocks = d.idct_blocks;
    d.idct_wg0 = (int32_t)L.idct_wgs;
    L.idct_wgs += (d.idct_blocks + kIdctThreads - 1) / kIdctThreads;
  }

  // Image i's share of what the front end and the IDCT work on: coefficient
  // lists, planes, segments, destuff chunks, entropy pieces and records, and
  // its workgroups in the flat destuff and IDCT grids (d.idct_blocks is set)
  void front_end(int i, const FrameBlocks& fb, int lv) {
    ImageDesc& d = L.desc[i];
    const spdl_hj_image_info& p = rq.infos[i];
    const int64_t bytes = rq.sizes[i];
    d.in_off = rq.offsets[i];
    d.in_size = bytes;
    d.nblocks = (int)fb.nblocks;
    d.coef_off = L.total_blocks;
    L.total_blocks += fb.nblocks;
    for (int c = 0; c < p.ncomp; c++) {
      // (a reduced plane: 8 >> L samples a block, each row padded to 8 bytes
      // a lane of idct_lowres_kernel, which writes the padding as well)
      d.plane_stride[c] = lv ? lowres_lanes_row(fb.bw[c], lv) * 8 : fb.bw[c] * 8;
      d.plane_off[c] = L.total_planes;
      L.total_planes += round_up((int64_t)d.plane_stride[c] * fb.bh[c] * (8 >> lv), 256);
    }
    d.seg_cap = (int32_t)(bytes / 2 + 2);
    d.seg_off = L.total_segs;
    L.total_segs += d.seg_cap;
    d.ds_cap = (int32_t)(bytes / kDsChunk + 2);
    d.ds_off = L.total_ds;
    L.total_ds += d.ds_cap;
    d.ds_wg0 = (int32_t)L.ds_wgs;
    L.ds_wgs += d.ds_cap;
    // (a ragged submission decides idct_blocks with each image's output path:
    // its IDCT workgroups are counted in finish_ragged)
    if (!rq.ragged) idct_share(d);
    if (d.ds_cap > L.max_chunks) L.max_chunks = d.ds_cap;
    // size-adaptive entropy decode: a file larger than piece_bytes is
    // decoded by ceil(size / piece_bytes) workgroups (progressive and
    // multi-scan images take multiscan_kernel: one)
    int pieces = 1;
    if (rq.piece_bytes > 0 && !p.multiscan && bytes > rq.piece_bytes)
      pieces = (int)std::min<int64_t>(kMaxPieces, (bytes + rq.piece_bytes - 1) / rq.piece_bytes);
    d.pieces = pieces;
    d.chain_off = pieces > 1 ? (int32_t)L.chain_granules : 0;
    if (pieces > 1) {
      L.chain_granules += (int64_t)pieces * kChainGranules;
      L.multi.emplace_back(i, p);
    }
    // entropy slot state (u32 units): kMaxSlots uint4 + slack per piece
    d.rec_cap = (int64_t)kMaxSlots * 8 * pieces;
    d.rec_off = L.total_recs;
    L.total_recs += d.rec_cap;
  }

  // The frame's own planes (SPDL_HJ_FMT_YUV): gray8 or yuvj444p / 422p / 420p,
  // every image in the format of image 0 (or of the first one after images
  // whose source crop was refused).  0, or why this frame has no such output.
  int planar_format(const views::Frame& f, int color, int hs, int vs, int why, bool* first) {
    const bool gray = f.ncomp == 1;
    if (!why && (f.ncomp == 4 || color == kColorRgb || hs > 1 || vs > hs))
      why = SPDL_HJ_ERR_UNSUPPORTED;
    *first = !have_fmt;
    if (!have_fmt) {
      have_fmt = true;
      if (why) return why;
      L.yuv_hs = hs;
      L.yuv_vs = vs;
      L.yuv_gray = gray;
    } else if (!why && (hs != L.yuv_hs || vs != L.yuv_vs || gray != L.yuv_gray)) {
      why = SPDL_HJ_ERR_UNSUPPORTED;
    }
    return why;
  }

  // The single copy of plan placement: the w x h frame that descriptor d reads
  // (a whole image, a source crop, a view) through chain `out` into a box of
  // size `box` -- its geometry, its plan (placed once in L.tables), its
  // hscale_kernel and sws_kernel tiles.  What a refusal costs is the caller's
  // to say (refused_alone).
  // `code`: the output's orientation (0..7).  With its transpose bit the
  // chain is `out0` with its pairs swapped, d keeps that chain's box, and
  // `box` is matched against the final one, oh x ow.
  Placement place_output(ImageDesc& d, int w, int h, const views::Frame& f, int color,
                         const spdl_hj_output& out0, BoxSize& box, int code) {
    const bool t = code & 4;
    const spdl_hj_output out = t ? swapped_chain(out0) : out0;
    Geom g;
    int fw, fh;
    int rc = final_box(w, h, out0, code, &g, &fw, &fh);
    if (rc) return {rc, kAtGeometry, nullptr};
    d.dx = g.dx;
    d.dy = g.dy;
    d.ow = g.ow;
    d.oh = g.oh;
    // (a ragged submission's images each have their box: `box` stays unset)
    if (!rq.ragged) {
      if (!box.set) box = {true, fw, fh};
      else if (fw != box.ow || fh != box.oh) return {SPDL_HJ_ERR_INVALID_ARG, kAtSize, nullptr};
    }
    if (!rq.plans || out.csc == SPDL_HJ_CSC_JFIF) return {SPDL_HJ_OK, kPlaced, nullptr};
    if (out.csc == SPDL_HJ_CSC_TURBO) {
      // no plan: turbo_rgb_kernel's tiles of this image's own box, in the flat
      // grid the sws fields map (rows of tiles x tiles per row)
      d.sws_wg0 = (int32_t)L.sws_wgs;
      d.sws_bands = (g.oh + kTurboTileH - 1) / kTurboTileH;
      d.sws_chunks = (g.ow + kTurboTileW - 1) / kTurboTileW;
      L.sws_wgs += (int64_t)d.sws_bands * d.sws_chunks;
      return {SPDL_HJ_OK, kPlaced, nullptr};
    }
    int hs, vs, mode;
    rc = views::chroma_shifts(f, &hs, &vs);
    if (out.pix_fmt == SPDL_HJ_FMT_YUV) {
      // An image that is not in the batch's format, or whose pad / crop does
      // not fall on its chroma grid, is refused
      bool first;
      int why = planar_format(f, color, hs, vs, rc, &first);
      if (why && first) return {why, kAtFirstFormat, nullptr};
      if (!why) why = geometry(w, h, &out, &g, 1 << hs, 1 << vs);
      if (why) return {why, kAtPlanar, nullptr};
      d.dx = g.dx;
      d.dy = g.dy;
      mode = (f.ncomp == 1 ? kPlanGray : kPlanYuv) | kPlanPlanar;
    } else {
      if (rc) return {rc, kAtSampling, nullptr};
      // RGB planes (gbrp; CMYK after the K transform, gbrap) through the luma
      // filters; YCCK after the transform and YCbCr + K are YCbCr 4:4:4
      mode = f.ncomp == 1                                  ? kPlanGray
             : color == kColorRgb || color == kColorCmyk ? kPlanGbr
                                                          : kPlanYuv;
    }
    const PlanKey key{w, h, hs, vs, mode, out.resize ? out.filter : 0,
                      g.sw, g.sh, g.dx, g.dy, g.ow, g.oh};
    const auto plan = rq.plans->get(key, &rc);
    if (!plan) return {rc, kAtFilter, nullptr};
    d.wt_off = pool.place(L.tables, plan);
    d.sws = plan->d;
    if (plan->d.pre) {  // hscale_kernel's tiles and rows (hj_sws_tile.h)
      d.hs_wg0 = (int32_t)L.hs_wgs;
      d.hs_wgs = hs_tiles(plan->d).wgs;
      L.hs_wgs += d.hs_wgs;
      d.hbuf_off = L.total_hbuf;
      L.total_hbuf += hs_hbuf_size(plan->d);
    }
    d.sws_wg0 = (int32_t)L.sws_wgs;  // flat sws grid: this output's tiles only
    d.sws_bands = plan->bands;
    d.sws_chunks = plan->chunks;
    L.sws_wgs += (int64_t)plan->bands * plan->chunks;
    return {SPDL_HJ_OK, kPlaced, plan.get()};  // (the pool keeps it alive)
  }

  // What a views submission found of its rectangles: resolved with their
  // images (plan_image), placed group by group (plan_views).  `order` lists
  // them by image (image i's: [start[i], start[i + 1]))
  struct ViewRes {
    views::Rect in, r;
    int rc;
  };
  std::vector<ViewRes> vres;
  std::vector<int> vstart, vorder;

  void index_views() {
    const HeldViews& hv = *rq.views;
    vstart.assign(rq.n + 1, 0);
    for (const auto& g : hv.groups)
      for (const spdl_hj_view& v : g.views) {
        vstart[v.image + 1]++;
        vres.push_back({{v.rect.x, v.rect.y, v.rect.w, v.rect.h}, {}, 0});
      }
    for (int i = 0; i < rq.n; i++) vstart[i + 1] += vstart[i];
    vorder.resize(vres.size());
    std::vector<int> fill(vstart.begin(), vstart.end() - 1);
    int q = 0;
    for (const auto& g : hv.groups)
      for (const spdl_hj_view& v : g.views) vorder[fill[v.image]++] = q++;
    L.desc.reserve(rq.n + vres.size());
  }

  // The bounding MCU rectangle of image i's views over all groups (the whole
  // grid if one of them is the whole frame; no view: no block).  A rectangle
  // that does not resolve refuses its view alone.
  int views_region(int i, ImageDesc& d, const views::Frame& f, const views::Grid& grid) {
    views::McuRect bound{0, 0, 0, 0};
    bool whole = false;
    for (int q = vstart[i]; q < vstart[i + 1]; q++) {
      ViewRes& vr = vres[vorder[q]];
      vr.rc = views::resolve(f, vr.in, &vr.r);
      if (vr.rc && vr.rc != SPDL_HJ_ERR_BAD_GEOMETRY) return fail(i, vr.rc, nullptr);
      if (vr.rc) continue;
      whole = whole || views::rect_is_none(vr.in);
      views::mcu_union(&bound, views::mcu_rect(grid, vr.r));
    }
    if (!whole) set_region(d, grid, bound);
    return SPDL_HJ_OK;
  }

  int plan_image(int i) {
    ImageDesc& d = L.desc[i];
    const spdl_hj_image_info& p = rq.infos[i];
    const spdl_hj_output& out = *rq.out;
    d.width = p.width;
    d.height = p.height;
    d.ncomp = p.ncomp;
    d.color = p.color;
    if (p.ncomp == 4) {
      // libjpeg's JFIF conversion has no CMYK -> RGB; the K transform
      // (FFmpeg's, cmyk_kernel) runs unless the planes are YCbCr + K
      if (out.csc == SPDL_HJ_CSC_JFIF) return fail(i, SPDL_HJ_ERR_UNSUPPORTED, "CMYK with csc=jfif");
      // ... and csc = TURBO is pinned for 1- and 3-component files alone
      if (out.csc == SPDL_HJ_CSC_TURBO) return fail(i, SPDL_HJ_ERR_UNSUPPORTED, "CMYK with csc=turbo");
      if (p.color != kColorYcbcrk) L.cmyk_px = std::max(L.cmyk_px, (int64_t)p.width * p.height);
    }
    for (int c = 0; c < p.ncomp; c++) {
      d.h_samp[c] = p.h_samp[c];
      d.v_samp[c] = p.v_samp[c];
    }
    FrameBlocks fb;
    if (int rc = frame_blocks(p, &fb)) return fail(i, rc, nullptr);
    // the entropy kernel's 32-bit byte offsets into an image's coefficient
    // lists (4 bytes x 64 entries per block) must not wrap
    if (fb.nblocks >= (1 << 24)) return fail(i, SPDL_HJ_ERR_UNSUPPORTED, "image too large");
    // The source crop: the frame every later step sees (src; the whole frame
    // without one), idct_kernel the MCUs it touches.  A rectangle that does
    // not resolve refuses its image alone.
    const views::Frame& f = fb.frame;
    const views::Rect whole{0, 0, p.width, p.height};
    views::Rect src = whole;
    const bool has_rect = rq.crops && !rect_is_none(rq.crops[i]);
    int crop_rc = SPDL_HJ_OK;
    d.idct_blocks = (int)fb.nblocks;
    d.src = i;
    // Reduced-size decode: every later step sees the frame FFmpeg's decoder
    // emits at this level, and the IDCT stage is counted in lanes
    const int lv = level_of(i);
    if (lv) {
      src = views::Rect{0, 0, lowres_side(p.width, lv), lowres_side(p.height, lv)};
      d.idct_blocks = 0;
      for (int c = 0; c < p.ncomp; c++) d.idct_blocks += lowres_lanes_row(fb.bw[c], lv) * fb.bh[c];
      L.lowres_images++;
    }
    if (rq.views) {
      if (int rc = views_region(i, d, f, fb.grid)) return rc;
    } else if (has_rect) {
      crop_rc = source_frame(p, &rq.crops[i], &src);
      if (crop_rc && crop_rc != SPDL_HJ_ERR_BAD_GEOMETRY) return fail(i, crop_rc, nullptr);
      if (crop_rc) src = whole;
      else set_region(d, fb.grid, views::mcu_rect(fb.grid, src));
    }
    set_windows(d, f, fb.grid, src);
    front_end(i, fb, lv);
    if (rq.views) return SPDL_HJ_OK;  // (the outputs are the views': plan_views)
    if (has_rect) L.all_special = false;  // the full-resolution converters read whole planes
    if (lv) {
      // (the unscaled converters and the fused kernel address by the file's size)
      L.all_special = L.fuse_ok = false;
      // cmyk_kernel addresses by the file's size as well: no reduced RGB-coded
      // or 4-component frame
      if (p.ncomp == 4 || p.color == kColorRgb) {
        if (!rq.plans) return fail(i, SPDL_HJ_ERR_UNSUPPORTED, "lowres of an RGB or 4-component frame");
        refuse(d, SPDL_HJ_ERR_UNSUPPORTED);
        return SPDL_HJ_OK;
      }
    }
    if (crop_rc) {
      refuse(d, crop_rc);
      return SPDL_HJ_OK;
    }
    const Placement pl = place_output(d, src.w, src.h, f, p.color, out, size, code_of(i));
    if (pl.at != kAtGeometry) L.max_px = std::max(L.max_px, (int64_t)d.ow * d.oh);
    if (pl.rc && refused_alone(rq.ragged != nullptr, pl)) {
      if (pl.at == kAtGeometry) d.dx = d.dy = d.ow = d.oh = 0;  // (placed nowhere)
      refuse(d, pl.rc);
      return SPDL_HJ_OK;
    }
    if (pl.at == kAtSize)
      return size_mismatch("all images of a batch must produce the same output size "
                           "(image %zu: %dx%d, image %zu: %dx%d); pass a resize target",
                           size, 0, (size_t)i, d);
    if (pl.rc)
      return fail(i, pl.rc,
                  pl.at == kAtFirstFormat ? "no planar output for this frame format"
                  : pl.at == kAtFilter && pl.rc == SPDL_HJ_ERR_BAD_GEOMETRY ? "scale filter too long"
                                                                            : nullptr);
    if (!pl.plan) return SPDL_HJ_OK;
    L.all_special = L.all_special && pl.plan->special;
    // idct_rgb_kernel's MCU shapes: Y 2x2 or 2x1, U and V 1x1
    const bool fusable = p.ncomp == 3 && p.h_samp[0] == 2 && (p.v_samp[0] == 1 || p.v_samp[0] == 2) &&
                         p.h_samp[1] == 1 && p.v_samp[1] == 1 && p.h_samp[2] == 1 && p.v_samp[2] == 1;
    const int tw = kFusedThreads / fb.grid.bpm;
    const int tiles_x = (fb.grid.mcux + tw - 1) / tw;
    if (fusable) L.fused_tiles = std::max(L.fused_tiles, tiles_x * fb.grid.mcuy);
    else L.fuse_ok = false;
    // A ragged submission chooses per image what a plain one chooses per batch
    // (hj_host.cpp run_pipeline): a fused-eligible image leaves idct_kernel and
    // sws_kernel nothing, its idct_rgb_kernel tiles stand in the sws fields
    // (finish_ragged numbers them)
    if (rq.ragged && fusable && pl.plan->special && !pl.plan->d.pre &&
        out.dtype == SPDL_HJ_DTYPE_U8 && !has_rect && !code_of(i) && !lv && rq.output_path == 0) {
      d.idct_blocks = 0;
      d.sws_bands = fb.grid.mcuy;
      d.sws_chunks = tiles_x;
      fused_image[i] = 1;
      return SPDL_HJ_OK;
    }
    L.sws_bands = std::max(L.sws_bands, pl.plan->bands);
    L.sws_chunks = std::max(L.sws_chunks, pl.plan->chunks);
    L.sws_lds = std::max(L.sws_lds, pl.plan->lds);
    return SPDL_HJ_OK;
  }

  // The view descriptors, group by group behind the images': each view a
  // frame of its own (its window of image `src`'s planes, its geometry, its
  // plan), tiled in its group's part of the flat sws grid.
  int plan_views() {
    const HeldViews& hv = *rq.views;
    L.all_special = L.fuse_ok = false;  // (the full-resolution converters read whole planes)
    std::vector<int32_t> vstatus(vres.size(), SPDL_HJ_OK);
    int32_t nviews[views::kMaxGroups];
    views::Slice slice[views::kMaxGroups];
    for (size_t gi = 0; gi < hv.groups.size(); gi++) nviews[gi] = (int32_t)hv.groups[gi].views.size();
    views::group_slices(rq.n, nviews, (int)hv.groups.size(), slice);
    size_t q = 0;
    for (size_t gi = 0; gi < hv.groups.size(); gi++) {
      const HeldViews::Group& hg = hv.groups[gi];
      Layout::Group G;
      G.out = hg.out;
      G.out_dev = hg.out_dev;
      G.first = slice[gi].first;  // (== L.desc.size(): the descriptors are appended in this order)
      G.count = slice[gi].count;
      G.sws_wg0 = (int)L.sws_wgs;
      BoxSize gsize;
      for (size_t k = 0; k < hg.views.size(); k++, q++) {
        const ViewRes& vr = vres[q];
        const int img = hg.views[k].image;
        const spdl_hj_image_info& p = rq.infos[img];
        L.desc.push_back(L.desc[img]);
        ImageDesc& v = L.desc.back();
        v.idct_blocks = 0;  // (the front-end and IDCT fields mean nothing here)
        Placement pl{vr.rc, kAtGeometry, nullptr};
        if (!vr.rc) {
          const views::Frame f = frame_of(p);
          set_windows(v, f, views::grid_of(f), vr.r);
          pl = place_output(v, vr.r.w, vr.r.h, f, p.color, hg.out, gsize,
                            code_of((int64_t)L.desc.size() - 1));
        }
        if (pl.rc && (vr.rc || refused_alone(true, pl))) {
          vstatus[q] = pl.rc;
          if (!L.view_refused) {
            L.view_refused = pl.rc;
            L.view_refused_group = (int)gi;
            L.view_refused_index = (int)k;
          }
          v.dx = v.dy = v.ow = v.oh = 0;  // (a refused view is placed nowhere)
          refuse(v, pl.rc);
          continue;
        }
        if (pl.at == kAtSize)
          return size_mismatch("all views of a group must produce the same output size "
                               "(group %zu: %dx%d, view %zu: %dx%d); pass a resize target",
                               gsize, gi, k, v);
        if (pl.rc) return fail(img, pl.rc, nullptr);
        G.sws_lds = std::max(G.sws_lds, pl.plan->lds);
      }
      G.ow = gsize.ow;
      G.oh = gsize.oh;
      const int64_t per = (int64_t)G.ow * G.oh * 3;
      const size_t esz = hg.out.dtype == SPDL_HJ_DTYPE_U8 ? 1 : 2;
      if ((size_t)(per * G.count) * esz > hg.out_bytes) {
        res.rc = SPDL_HJ_ERR_INVALID_ARG;
        snprintf(res.err, sizeof(res.err),
                 "group %zu: output buffer too small: need %lld bytes, have %zu", gi,
                 (long long)(per * G.count * (int64_t)esz), hg.out_bytes);
        return res.rc;
      }
      for (int k = 0; k < G.count; k++) L.desc[G.first + k].out_off = (int64_t)k * per;
      G.sws_wgs = (int)L.sws_wgs - G.sws_wg0;
      L.groups.push_back(G);
    }
    // (nothing is written before every limit has held)
    q = 0;
    for (const HeldViews::Group& hg : hv.groups)
      for (size_t k = 0; k < hg.views.size(); k++, q++)
        if (hg.status) hg.status[k] = vstatus[q];
    return SPDL_HJ_OK;
  }

  // The flips of the submission against its count, values and chain; nothing
  // has been planned or written yet
  int check_flips() {
    res.rc = SPDL_HJ_ERR_INVALID_ARG;
    if (rq.flips && rq.orients) {
      snprintf(res.err, sizeof(res.err),
               "spdl_hj_set_flips and spdl_hj_set_orients on one submission");
      return res.rc;
    }
    res.rc = SPDL_HJ_OK;
    if (rq.orients) return check_orients();
    if (!rq.flips) return SPDL_HJ_OK;
    int64_t want = rq.n;
    if (rq.views) {
      want = 0;
      for (const auto& g : rq.views->groups) want += (int64_t)g.views.size();
    }
    res.rc = SPDL_HJ_ERR_INVALID_ARG;
    if (rq.nflips != want) {
      snprintf(res.err, sizeof(res.err), "spdl_hj_set_flips gave %lld flips for %lld %s",
               (long long)rq.nflips, (long long)want,
               rq.views ? "views" : "images");
      return res.rc;
    }
    bool any = false;
    for (int64_t i = 0; i < want; i++) {
      if (rq.flips[i] > 3) {
        snprintf(res.err, sizeof(res.err), "spdl_hj_set_flips: flip %lld is %d (0 to 3)",
                 (long long)i, (int)rq.flips[i]);
        return res.rc;
      }
      any = any || rq.flips[i];
    }
    if (any && rq.out->csc != SPDL_HJ_CSC_SWSCALE) {
      snprintf(res.err, sizeof(res.err), "a flip needs csc = swscale");
      return res.rc;
    }
    res.rc = SPDL_HJ_OK;
    return SPDL_HJ_OK;
  }

  // The orientations likewise: codes 0 to 7, no code with csc = JFIF, no
  // transpose of the planar YUV output (a transposed 4:2:2 frame is another
  // pixel format)
  int check_orients() {
    int64_t want = rq.n;
    if (rq.views) {
      want = 0;
      for (const auto& g : rq.views->groups) want += (int64_t)g.views.size();
    }
    res.rc = SPDL_HJ_ERR_INVALID_ARG;
    if (rq.norients != want) {
      snprintf(res.err, sizeof(res.err), "spdl_hj_set_orients gave %lld codes for %lld %s",
               (long long)rq.norients, (long long)want, rq.views ? "views" : "images");
      return res.rc;
    }
    bool any = false;
    for (int64_t i = 0; i < want; i++) {
      const int c = rq.orients[i];
      if (c > 7) {
        snprintf(res.err, sizeof(res.err), "spdl_hj_set_orients: code %lld is %d (0 to 7)",
                 (long long)i, c);
        return res.rc;
      }
      if (c & 4) {
        // (views: each group has its own chain)
        bool yuv = rq.out->pix_fmt == SPDL_HJ_FMT_YUV;
        if (rq.views) {
          int64_t q = i;
          for (const auto& g : rq.views->groups) {
            if (q < (int64_t)g.views.size()) {
              yuv = g.out.pix_fmt == SPDL_HJ_FMT_YUV;
              break;
            }
            q -= (int64_t)g.views.size();
          }
        }
        if (yuv) {
          snprintf(res.err, sizeof(res.err),
                   "spdl_hj_set_orients: code %lld transposes the planar YUV output", (long long)i);
          return res.rc;
        }
      }
      any = any || c;
    }
    if (any && rq.out->csc != SPDL_HJ_CSC_SWSCALE) {
      snprintf(res.err, sizeof(res.err), "an orientation needs csc = swscale");
      return res.rc;
    }
    res.rc = SPDL_HJ_OK;
    return SPDL_HJ_OK;
  }

  // The levels of the submission against its count, values and what else it
  // asks for; nothing has been planned or written yet
  int check_lowres() {
    if (!rq.lowres) return SPDL_HJ_OK;
    const char* what = nullptr;
    char buf[96];
    int any = 0;
    if (rq.nlowres != rq.n) {
      snprintf(buf, sizeof(buf), "spdl_hj_set_lowres gave %lld levels for %d images",
               (long long)rq.nlowres, rq.n);
      what = buf;
    }
    for (int64_t i = 0; !what && i < rq.nlowres; i++) {
      if (rq.lowres[i] > 3) {
        snprintf(buf, sizeof(buf), "spdl_hj_set_lowres: level %lld is %d (0 to 3)", (long long)i,
                 (int)rq.lowres[i]);
        what = buf;
      }
      any |= rq.lowres[i];
    }
    if (!what && any) {
      if (rq.crops) what = "spdl_hj_set_lowres and spdl_hj_set_crops on one submission";
      else if (rq.views) what = "spdl_hj_set_lowres and views on one submission";
      else if (rq.out->csc != SPDL_HJ_CSC_SWSCALE) what = "a reduced-size decode needs csc = swscale";
    }
    if (!what) {
      if (any) L.lowres.assign(rq.lowres, rq.lowres + rq.nlowres);
      return SPDL_HJ_OK;
    }
    res.rc = SPDL_HJ_ERR_INVALID_ARG;
    snprintf(res.err, sizeof(res.err), "%s", what);
    return res.rc;
  }
  int level_of(int i) const { return L.lowres.empty() ? 0 : L.lowres[i]; }

  // csc = TURBO is the whole frame as stored (spdl_hipjpeg.h "Pillow-exact
  // decode"): no source crop and no views; flips, orientations and levels are
  // refused by their own checks, a resize and the planar output by valid_output
  int check_turbo() {
    if (rq.out->csc != SPDL_HJ_CSC_TURBO) return SPDL_HJ_OK;
    const char* what = nullptr;
    if (rq.crops) what = "a source crop needs csc = swscale";
    else if (rq.views) what = "views need csc = swscale";
    if (!what) return SPDL_HJ_OK;
    res.rc = SPDL_HJ_ERR_INVALID_ARG;
    snprintf(res.err, sizeof(res.err), "%s", what);
    return res.rc;
  }

  // One flag per descriptor, once every descriptor stands; none when every
  // flip is 0.  A flipped full-resolution batch takes the generic output
  // kernel (the unscaled converters do not flip).
  void place_flips() {
    if (!codes()) return;
    int any = 0;
    for (int64_t i = 0; i < ncodes(); i++) any |= codes()[i];
    if (!any) return;
    L.flips.assign(L.desc.size(), 0);
    std::copy(codes(), codes() + ncodes(), L.flips.begin() + (rq.views ? rq.n : 0));
    L.transposed = any & 4;
    L.all_special = false;
  }

  // A ragged request against what the extension takes (spdl_hipjpeg.h "ragged
  // batches"); nothing has been planned or written yet
  int check_ragged() {
    if (!rq.ragged) return SPDL_HJ_OK;
    const char* what = nullptr;
    if (rq.views) what = "views and spdl_hj_set_ragged on one submission";
    else if (!rq.plans) what = "spdl_hj_set_ragged needs an output stage";
    else if (rq.out->pix_fmt == SPDL_HJ_FMT_YUV) what = "no ragged planar YUV output";
    else if (rq.out->csc == SPDL_HJ_CSC_JFIF) what = "a ragged submission needs csc = swscale or turbo";
    const int64_t esz = rq.out->dtype == SPDL_HJ_DTYPE_U8 ? 1 : 2;
    for (int i = 0; i < rq.n && !what; i++)
      if (rq.ragged[i] < 0 || rq.ragged[i] % esz)
        what = "spdl_hj_set_ragged: an offset is negative or no multiple of the element size";
    if (!what) return SPDL_HJ_OK;
    res.rc = SPDL_HJ_ERR_INVALID_ARG;
    snprintf(res.err, sizeof(res.err), "%s", what);
    return res.rc;
  }

  // A ragged submission once every descriptor stands: each image at its own
  // offset, inside the buffer; the IDCT grid of the images idct_kernel
  // transforms; the flat sws grid with the fused-eligible images' tiles
  // first, [0, L.fused_wgs), then every other image's
  int finish_ragged() {
    const int n = rq.n;
    const int64_t esz = rq.out->dtype == SPDL_HJ_DTYPE_U8 ? 1 : 2;
    for (int i = 0; i < n; i++) {
      ImageDesc& d = L.desc[i];
      const int64_t extent = (int64_t)d.ow * d.oh * 3 * esz;  // (a refused image: none)
      if (rq.ragged[i] > rq.out_bytes || extent > rq.out_bytes - rq.ragged[i]) {
        res.rc = SPDL_HJ_ERR_INVALID_ARG;
        res.image = i;
        snprintf(res.err, sizeof(res.err),
                 "image %d: %dx%d at byte %lld reaches past the output buffer of %lld bytes", i,
                 code_of(i) & 4 ? d.oh : d.ow, code_of(i) & 4 ? d.ow : d.oh, (long long)rq.ragged[i],
                 (long long)rq.out_bytes);
        return res.rc;
      }
      d.out_off = rq.ragged[i] / esz;
      idct_share(d);
    }
    int64_t wg = 0;
    for (int pass = 0; pass < 2; pass++) {
      for (int i = 0; i < n; i++)
        if ((fused_image[i] != 0) == (pass == 0)) {
          L.desc[i].sws_wg0 = (int32_t)wg;
          wg += (int64_t)L.desc[i].sws_bands * L.desc[i].sws_chunks;
        }
      if (pass == 0) L.fused_wgs = wg;
    }
    L.sws_wgs = wg;
    L.ragged = true;
    return SPDL_HJ_OK;
  }

  // Output offsets and the entropy work list, once every descriptor stands
  void finish() {
    const int n = rq.n;
    L.ow = size.ow;
    L.oh = size.oh;
    L.out_elems_per_image = (int64_t)L.ow * L.oh * 3;
    if (rq.out->pix_fmt == SPDL_HJ_FMT_YUV)  // Y, then U and V of ceil(ow / hs) x ceil(oh / vs) (gray: Y alone)
      L.out_elems_per_image =
          (int64_t)L.ow * L.oh + (L.yuv_gray ? 0
                                             : 2 * (int64_t)(-((-L.ow) >> L.yuv_hs)) *
                                                   (-((-L.oh) >> L.yuv_vs)));
    for (int i = 0; i < n; i++) L.desc[i].out_off = (int64_t)i * L.out_elems_per_image;
    // entropy work list: the images with the most pieces first (their pieces
    // start early and in ticket order), each image's pieces in order
    std::vector<int> order(n);
    for (int i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(),
                     [&](int a, int b) { return L.desc[a].pieces > L.desc[b].pieces; });
    L.work.clear();
    for (int i : order)
      for (int q = 0; q < L.desc[i].pieces; q++) L.work.push_back((uint32_t)i | ((uint32_t)q << 24));
  }
};

}  // namespace

LayoutResult build_layout(const LayoutRequest& rq, Layout& L) {
  Planner P{rq, L};
  if (P.check_flips() || P.check_ragged() || P.check_lowres() || P.check_turbo()) return P.res;
  L.desc.assign(rq.n, ImageDesc{});
  if (rq.ragged) P.fused_image.assign(rq.n, 0);
  if (rq.views) P.index_views();
  for (int i = 0; i < rq.n; i++)
    if (P.plan_image(i)) return P.res;
  if (rq.views && P.plan_views()) return P.res;
  P.finish();
  if (rq.ragged && P.finish_ragged()) return P.res;
  P.place_flips();
  return P.res;
}

int source_frame(const spdl_hj_image_info& p, const spdl_hj_rect* in, views::Rect* src) {
  *src = views::Rect{0, 0, p.width, p.height};
  if (!in || rect_is_none(*in)) return SPDL_HJ_OK;
  return views::resolve(frame_of(p), views::Rect{in->x, in->y, in->w, in->h}, src);
}

int final_box(int w, int h, const spdl_hj_output& out, int code, Geom* g, int* fw, int* fh) {
  const bool t = code & 4;
  const spdl_hj_output chain = t ? swapped_chain(out) : out;
  if (const int rc = geometry(w, h, &chain, g)) return rc;
  *fw = t ? g->oh : g->ow;
  *fh = t ? g->ow : g->oh;
  return SPDL_HJ_OK;
}

int ragged_layout(const spdl_hj_image_info* infos, int n, const spdl_hj_output* out,
                  const spdl_hj_rect* crops, const uint8_t* orients, int64_t align_bytes,
                  int64_t* offsets, int32_t* ow, int32_t* oh, int32_t* status) {
  if (!infos || n < 0 || !valid_output(out) || !offsets || !ow || !oh || !status)
    return SPDL_HJ_ERR_INVALID_ARG;
  const int64_t esz = out->dtype == SPDL_HJ_DTYPE_U8 ? 1 : 2;
  if (out->pix_fmt == SPDL_HJ_FMT_YUV || out->csc == SPDL_HJ_CSC_JFIF || align_bytes < esz ||
      align_bytes % esz)
    return SPDL_HJ_ERR_INVALID_ARG;
  // csc = TURBO is the whole frame as stored: no crop, no orientation code
  if (out->csc == SPDL_HJ_CSC_TURBO)
    for (int i = 0; i < n; i++)
      if ((crops && !rect_is_none(crops[i])) || (orients && orients[i]))
        return SPDL_HJ_ERR_INVALID_ARG;
  int64_t end = 0;
  for (int i = 0; i < n; i++) {
    const spdl_hj_image_info& p = infos[i];
    views::Rect src;
    Geom g;
    int fw = 0, fh = 0;
    int rc = orients && orients[i] > 7 ? SPDL_HJ_ERR_INVALID_ARG : SPDL_HJ_OK;
    if (!rc && p.ncomp != 1 && p.ncomp != 3 && p.ncomp != 4) rc = SPDL_HJ_ERR_INVALID_ARG;
    for (int c = 0; !rc && c < p.ncomp; c++)  // (as spdl_hj_crop_rect asks of a probe)
      if (p.h_samp[c] < 1 || p.h_samp[c] > 4 || p.v_samp[c] < 1 || p.v_samp[c] > 4)
        rc = SPDL_HJ_ERR_INVALID_ARG;
    if (!rc) rc = source_frame(p, crops ? &crops[i] : nullptr, &src);
    if (!rc) rc = final_box(src.w, src.h, *out, orients ? orients[i] : 0, &g, &fw, &fh);
    if (rc) fw = fh = 0;
    status[i] = rc;
    ow[i] = fw;
    oh[i] = fh;
    offsets[i] = round_up(end, align_bytes);
    end = offsets[i] + (int64_t)fw * fh * 3 * esz;
  }
  offsets[n] = end;
  return SPDL_HJ_OK;
}

}  // namespace hj
