// hj_views.h -- the host arithmetic of rectangles of a decoded frame: the
// source crop's rules and what views (spdl_hj_set_views) add to them.  Pure
// integer code with no HIP include, so a stand-alone program can sweep it
// (tests/native/views_sweep.cpp).
//
// A view is a rectangle of one image of the batch that becomes an output of
// its own.  An image is decoded once: entropy decode covers its whole scan, the
// IDCT the bounding MCU rectangle of all of its views, and every view then
// reads its window of the image's planes.  Plane bytes outside the bounding
// rectangle are stale; a view's window lies inside its own MCU rectangle and
// that inside the bounding one, so no view reads them.
#pragma once
#include <stdint.h>

#include "hj_common.h"

namespace hj {
namespace views {

constexpr int kMaxGroups = 4;            // groups of one submission
constexpr int32_t kCenter = INT32_MIN;   // SPDL_HJ_CROP_CENTER
constexpr int kInvalidArg = 8;           // SPDL_HJ_ERR_INVALID_ARG

struct Rect {
  int32_t x, y, w, h;
};

// What the SOF says of a frame (spdl_hj_image_info's geometry fields)
struct Frame {
  int32_t width, height, ncomp;
  int32_t h_samp[kMaxComp], v_samp[kMaxComp];
};

// The frame's MCU grid as the decoder lays its planes out (gray and
// non-interleaved frames: the blocks are the MCUs)
struct Grid {
  int32_t hmax, vmax, mcux, mcuy, bpm;
};
inline Grid grid_of(const Frame& f) {
  Grid g{1, 1, 0, 0, 0};
  if (f.ncomp == 1) {
    g.mcux = (f.width + 7) / 8;
    g.mcuy = (f.height + 7) / 8;
    g.bpm = 1;
    return g;
  }
  for (int c = 0; c < f.ncomp; c++) {
    g.hmax = f.h_samp[c] > g.hmax ? f.h_samp[c] : g.hmax;
    g.vmax = f.v_samp[c] > g.vmax ? f.v_samp[c] : g.vmax;
    g.bpm += f.h_samp[c] * f.v_samp[c];
  }
  g.mcux = (f.width + 8 * g.hmax - 1) / (8 * g.hmax);
  g.mcuy = (f.height + 8 * g.vmax - 1) / (8 * g.vmax);
  return g;
}

// chroma subsampling shifts of the yuvj4xxp frame FFmpeg's mjpeg decoder
// makes of this sampling (444 / 422 / 420 / 440 / 411 ...); others are not
// a swscale input format here
inline int chroma_shifts(const Frame& p, int* hs, int* vs) {
  *hs = *vs = 0;
  if (p.ncomp != 3) return kOk;  // gray, or 4 components all 1x1 (probe)
  int hmax = p.h_samp[0], vmax = p.v_samp[0];
  for (int c = 1; c < 3; c++) {
    hmax = p.h_samp[c] > hmax ? p.h_samp[c] : hmax;
    vmax = p.v_samp[c] > vmax ? p.v_samp[c] : vmax;
  }
  if (p.h_samp[0] != hmax || p.v_samp[0] != vmax || p.h_samp[1] != p.h_samp[2] ||
      p.v_samp[1] != p.v_samp[2] || hmax % p.h_samp[1] || vmax % p.v_samp[1])
    return kErrUnsupported;
  const int rh = hmax / p.h_samp[1], rv = vmax / p.v_samp[1];
  if ((rh & (rh - 1)) || (rv & (rv - 1))) return kErrUnsupported;
  while ((1 << *hs) < rh) (*hs)++;
  while ((1 << *vs) < rv) (*vs)++;
  return kOk;
}

// One axis of a rectangle: the size rounded down to the chroma ratio, the
// origin clamped into the frame and then rounded down likewise.  A centred
// origin with an off-grid size is refused (vf_crop's order of rounding and
// centring there is not pinned).
inline int rect_axis(int64_t pos, int64_t size, int64_t full, int ratio, int32_t* opos,
                     int32_t* osize) {
  const int64_t s = size / ratio * ratio;
  if (size <= 0 || s <= 0 || s > full) return kErrBadGeometry;
  if (pos == kCenter) {
    if (size % ratio) return kErrBadGeometry;
    pos = (full - s) / 2;
  }
  if (pos < 0) pos = 0;
  if (pos + s > full) pos = full - s;
  *opos = (int32_t)(pos / ratio * ratio);
  *osize = (int32_t)s;
  return kOk;
}

inline bool rect_is_none(const Rect& r) { return !(r.x | r.y | r.w | r.h); }

// A source crop's or a view's rectangle by the rules of spdl_hipjpeg.h
// ("source crop"); (0, 0, 0, 0) is the whole frame.
inline int resolve(const Frame& p, const Rect& in, Rect* out) {
  if (p.width <= 0 || p.height <= 0) return kInvalidArg;
  if (rect_is_none(in)) {
    *out = {0, 0, p.width, p.height};
    return kOk;
  }
  int hsub, vsub;
  if (int rc = chroma_shifts(p, &hsub, &vsub)) return rc;
  if (int rc = rect_axis(in.x, in.w, p.width, 1 << hsub, &out->x, &out->w)) return rc;
  return rect_axis(in.y, in.h, p.height, 1 << vsub, &out->y, &out->h);
}

// MCUs [mx0, mx0 + mw) x [my0, my0 + mh); mw == 0: none
struct McuRect {
  int32_t mx0, my0, mw, mh;
};

// The MCUs a resolved rectangle touches
inline McuRect mcu_rect(const Grid& g, const Rect& r) {
  const int mw8 = 8 * g.hmax, mh8 = 8 * g.vmax;
  McuRect m;
  m.mx0 = r.x / mw8;
  m.my0 = r.y / mh8;
  m.mw = (r.x + r.w - 1) / mw8 - m.mx0 + 1;
  m.mh = (r.y + r.h - 1) / mh8 - m.my0 + 1;
  return m;
}

// acc grown to hold r as well: the bounding rectangle of an image's views
inline void mcu_union(McuRect* acc, const McuRect& r) {
  if (!r.mw) return;
  if (!acc->mw) {
    *acc = r;
    return;
  }
  const int x1 = acc->mx0 + acc->mw > r.mx0 + r.mw ? acc->mx0 + acc->mw : r.mx0 + r.mw;
  const int y1 = acc->my0 + acc->mh > r.my0 + r.mh ? acc->my0 + acc->mh : r.my0 + r.mh;
  acc->mx0 = acc->mx0 < r.mx0 ? acc->mx0 : r.mx0;
  acc->my0 = acc->my0 < r.my0 ? acc->my0 : r.my0;
  acc->mw = x1 - acc->mx0;
  acc->mh = y1 - acc->my0;
}

// Blocks idct_kernel transforms of an image whose views cover m (none: 0)
inline int32_t idct_blocks(const Grid& g, const McuRect& m) { return m.mw * m.mh * g.bpm; }

// Component c's window of a resolved rectangle: origin (x / hs_c, y / vs_c),
// size ceil(w / hs_c) x ceil(h / vs_c), in the component's plane
struct Window {
  int32_t x, y, w, h;
};
inline Window window(const Frame& f, const Grid& g, const Rect& r, int c) {
  const int hsc = f.ncomp == 1 ? 1 : g.hmax / f.h_samp[c];
  const int vsc = f.ncomp == 1 ? 1 : g.vmax / f.v_samp[c];
  return {r.x / hsc, r.y / vsc, (r.w + hsc - 1) / hsc, (r.h + vsc - 1) / vsc};
}

// The samples of component c's plane that the IDCT of m writes:
// [x, x + w) x [y, y + h) (whole blocks)
inline Window mcu_plane_area(const Frame& f, const McuRect& m, int c) {
  const int bh = f.ncomp == 1 ? 1 : f.h_samp[c], bv = f.ncomp == 1 ? 1 : f.v_samp[c];
  return {m.mx0 * bh * 8, m.my0 * bv * 8, m.mw * bh * 8, m.mh * bv * 8};
}

// Descriptor slices: a views submission of n images keeps its n image
// descriptors first and appends every group's view descriptors in group
// order, views in the order given.  Group g's are [first, first + count).
struct Slice {
  int32_t first, count;
};
inline int32_t group_slices(int32_t n, const int32_t* nviews, int ngroups, Slice* out) {
  int32_t at = n;
  for (int g = 0; g < ngroups; g++) {
    out[g] = {at, nviews[g]};
    at += nviews[g];
  }
  return at;  // descriptors in all
}

}  // namespace views
}  // namespace hj
