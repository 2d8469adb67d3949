// hj_sws.h -- host-side plan of the scale / colour-conversion stage.
//
// The reference's CPU path converts the decoded yuvj4xxp frame to rgb24 with
// ONE libswscale context (the scale filter of the graph SPDL builds,
// src/spdl/io/_preprocessing.py:214-254, run by FilterGraphImpl::filter,
// src/libspdl/core/detail/ffmpeg/filter_graph.cpp:280-313; pad/crop only move
// pixels afterwards).  Everything that context decides from the geometry alone
// -- filter taps and positions per axis, chroma sizes, the full-chroma switch,
// which output writer each row uses, the yuv2rgb coefficients -- is computed
// here on the host, once per distinct geometry, and shipped to the device as
// one int32 blob; the gfx950 kernel (sws_kernel) only runs the arithmetic.
#pragma once
#include <stdint.h>

#include <map>
#include <memory>
#include <tuple>
#include <vector>

#include "hj_common.h"

namespace hj {

// One axis of libswscale's initFilter (utils.c): per output sample the first
// source sample and `size` taps normalised to `one`.
struct SwsAxis {
  int size = 0, n = 0;
  int eff = 0;  // taps actually non-zero at the end of some row (<= size)
  std::vector<int32_t> pos;
  std::vector<int16_t> coef;
};

struct SwsPlan {
  int srcW = 0, srcH = 0, dstW = 0, dstH = 0;
  int chrSrcW = 0, chrSrcH = 0, chrDstW = 0, chrDstH = 0;
  int hsub = 0, vsub = 0;  // source chroma subsampling shifts
  bool full = false;       // SWS_FULL_CHR_H_INT
  bool gray = false;
  bool special = false;    // unscaled yuv420p/422p -> rgb24 converter
  SwsAxis hl, hc, vl, vc;
  std::vector<int32_t> vmode;  // per output row
};

SwsCsc sws_csc();  // (hj_common.h)

// kind: SPDL_HJ_FILTER_*.  Returns 0, or an SPDL_HJ_ERR_* code (a filter
// longer than swscale handles without cascading: BAD_GEOMETRY).
int sws_plan(int srcW, int srcH, int hsub, int vsub, bool gray, int dstW, int dstH, int kind,
             SwsPlan* out);

// The plan of a planar destination that keeps the source's format
// (SPDL_HJ_FMT_YUV: yuvj4xxp -> yuvj4xxp, gray8 -> gray8; a scale filter with
// no format node after it): chrDstW x chrDstH = ceil(dstW >> hsub) x
// ceil(dstH >> vsub), luma filters as sws_plan, chroma filters from chroma
// plane to chroma plane with centred siting on both sides.  No colour tables,
// no `full`, no `special`: swscale's 8-bit planar writers (vscale.c
// lum_planar_vscale / chr_planar_vscale -> yuv2plane1_8_c, yuv2planeX_8_c)
// take every row, and `vmode` stays empty.  A vertical filter of size 1 holds
// the tap 4096, with which yuv2planeX's (2^18 + tap x) >> 19 is yuv2plane1's
// (x + 64) >> 7, the writer swscale picks for that size whatever the tap.
int sws_plan_planar(int srcW, int srcH, int hsub, int vsub, bool gray, int dstW, int dstH, int kind,
                    SwsPlan* out);

// ---- plans packed for the device -------------------------------------------
// One per distinct (source size, sampling, output placement, filter): the
// tables as one blob, and the tiling the kernels run it with (hj_sws_tile.h).
enum { kPlanYuv = 0, kPlanGray = 1, kPlanGbr = 2 };  // source planes of a plan
constexpr int kPlanPlanar = 4;  // | kPlanYuv / kPlanGray: the planar destination (SPDL_HJ_FMT_YUV)
struct PlanKey {
  int w, h, hsub, vsub, mode, filter, sw, sh, dx, dy, ow, oh;
  bool operator<(const PlanKey& o) const {
    return std::tie(w, h, hsub, vsub, mode, filter, sw, sh, dx, dy, ow, oh) <
           std::tie(o.w, o.h, o.hsub, o.vsub, o.mode, o.filter, o.sw, o.sh, o.dx, o.dy, o.ow, o.oh);
  }
};

struct PackedPlan {
  SwsDesc d{};                  // offsets relative to the blob
  std::vector<int32_t> blob;    // tables, 16-byte aligned sections
  int bands = 0, chunks = 0, lds = 0;  // tiles (planar: `bands` counts them all), LDS bytes
  bool special = false;         // swscale's unscaled yuv2rgb_c_24_rgb converter
  int axis_n[4] = {};           // rows of the hl, hc, vl, vc tables (spdl_hj_debug_sws_plan)
};

// Cached per context, so a stream of same-size images plans once.
class PlanCache {
 public:
  // the horizontal pass of large downscales in hscale_kernel (SwsDesc::pre):
  // -1 when the vertical ratio is >= kPreRatio or the luma filter is longer
  // than the kernel's register buckets (64 taps), 0 never, 1 always
  // (spdl_hj_set_param "sws_prepass"; outputs are identical)
  static constexpr int kPreRatio = 4;
  void set_pre_mode(int m) {
    if (m != pre_mode_) map_.clear();
    pre_mode_ = m;
  }
  int pre_mode() const { return pre_mode_; }
  // widest column chunk a tile may take (16-256; the tiler then picks the
  // tallest band that fits the LDS budget)
  void set_max_cols(int c) {
    if (c != max_cols_) map_.clear();
    max_cols_ = c;
  }
  int max_cols() const { return max_cols_; }
  std::shared_ptr<const PackedPlan> get(const PlanKey& k, int* rc);  // nullptr: *rc says why
  // one plan outside any cache (spdl_hj_debug_sws_plan, tests/native)
  static std::shared_ptr<const PackedPlan> build(const PlanKey& k, int* rc, int pre_mode,
                                                 int max_cols);

 private:
  std::map<PlanKey, std::shared_ptr<const PackedPlan>> map_;
  int pre_mode_ = -1;
  int max_cols_ = kSwsMaxCols;
};

}  // namespace hj
