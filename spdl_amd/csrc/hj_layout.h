// hj_layout.h -- the batch planner: from the host probes, the output spec, the
// source crops and the views of one submission to the descriptors, the table
// pool and the work list the kernels get (Layout).  Host arithmetic only, no
// HIP include: it builds with -DHJ_HD= beside hj_sws.cpp, so a stand-alone
// program pins its bytes and runs it under sanitizers
// (tests/native/layout_dump.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <memory>
#include <utility>
#include <vector>

#include "../../include/spdl_hipjpeg.h"
#include "hj_common.h"
#include "hj_sws.h"
#include "hj_views.h"

namespace hj {

const char* status_str(int s);

inline int64_t round_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// ---- geometry (FFmpeg scale/pad/crop semantics; see oracle jo_geometry) ----
struct Geom {
  int sw, sh, dx, dy, ow, oh;
};

// hs / vs: the chroma ratios of a planar destination (SPDL_HJ_FMT_YUV), which
// pad and crop offsets and sizes must respect; 1 for every packed output
int geometry(int w, int h, const spdl_hj_output* o, Geom* g, int hs = 1, int vs = 1);

bool valid_output(const spdl_hj_output* o);

// The rectangle rules (chroma shifts, the source crop's rounding) are pure
// arithmetic shared with views: hj_views.h.
views::Frame frame_of(const spdl_hj_image_info& p);
inline bool rect_is_none(const spdl_hj_rect& r) { return !(r.x | r.y | r.w | r.h); }

// ---- source crop (spdl_hipjpeg.h: libavfilter's crop, exact=0, on the
// decoder's frame) -----------------------------------------------------------
int crop_resolve(const spdl_hj_image_info& p, const spdl_hj_rect& in, spdl_hj_rect* out);

// A frame's MCU grid (gray: hmax = vmax = bpm = 1, its factors mean nothing),
// component c's plane of bw[c] x bh[c] blocks and the blocks in all; returns
// SPDL_HJ_ERR_UNSUPPORTED for sampling factors that do not divide the largest
// or more than kMaxBpm blocks per MCU.
struct FrameBlocks {
  views::Frame frame;
  views::Grid grid;
  int bw[kMaxComp], bh[kMaxComp];  // (set for the frame's components)
  int64_t nblocks;
};
int frame_blocks(const spdl_hj_image_info& p, FrameBlocks* fb);

struct Layout {
  std::vector<ImageDesc> desc;
  std::vector<int32_t> tables;  // the batch's swscale table pool
  int64_t total_blocks = 0, total_planes = 0, total_segs = 0, total_recs = 0;
  int64_t out_elems_per_image = 0;
  int max_blocks = 0;  // most blocks idct_kernel transforms of one image (ImageDesc::idct_blocks)
  int64_t max_px = 0;
  int64_t total_ds = 0;
  int max_chunks = 0;
  int ow = 0, oh = 0;
  int sws_bands = 0, sws_chunks = 0, sws_lds = 0;
  bool all_special = true;  // every image takes swscale's unscaled converter
  bool fuse_ok = true;      // ... with standard 4:2:0 / 4:2:2 MCUs (idct_rgb_kernel)
  int yuv_hs = 0, yuv_vs = 0;  // SPDL_HJ_FMT_YUV: image 0's chroma shifts, and whether it is
  bool yuv_gray = false;      // gray -- the batch's plane layout
  int64_t cmyk_px = 0;      // 4-component images needing cmyk_kernel's K transform: max pixels
  int fused_tiles = 0;      // idct_rgb_kernel workgroups per image (max)
  // entropy work items (image | piece << 24), the images with the most
  // pieces first, and the granules of their hand-off records (hj_common.h)
  std::vector<uint32_t> work;
  int64_t chain_granules = 0;
  // flat destuff / IDCT grids: workgroups over the whole batch
  int64_t ds_wgs = 0, idct_wgs = 0;
  // hscale_kernel (large downscales): workgroups and int16 rows
  int64_t hs_wgs = 0, total_hbuf = 0;
  int64_t sws_wgs = 0;  // sws_kernel tiles over the batch (per-image plans)
  // a progressive (SOF2) image is in the batch: multiscan_kernel runs on a
  // side stream beside destuff + entropy (only the host-bytes entry points
  // see the headers; elsewhere it runs after entropy on the lane's stream)
  bool ms_side = false;
  // the entry point knows every image's scan structure (host probes, or the
  // caller's ABI-5 image_info): a batch without multi-scan images may skip
  // the multi-scan launch
  bool ms_known = false;
  // images decoded by several entropy workgroups (hand-offs): their probes,
  // for a one-workgroup re-decode should a hand-off give up
  std::vector<std::pair<int, spdl_hj_image_info>> multi;
  // A views submission (spdl_hj_set_views): desc holds the n image
  // descriptors, then every group's view descriptors (views::group_slices);
  // the output stage runs once per group over its slice.  Empty otherwise.
  struct Group {
    spdl_hj_output out;
    void* out_dev = nullptr;
    int first = 0, count = 0;        // its view descriptors in desc
    int sws_wg0 = 0, sws_wgs = 0;    // its tiles in the flat sws grid (sws_map)
    int sws_lds = 0;
    int ow = 0, oh = 0;              // every view's output size
  };
  std::vector<Group> groups;
  // Output flips (spdl_hj_set_flips): one byte per descriptor (SPDL_HJ_FLIP_*;
  // in a views submission 0 for the n image descriptors, the views carry
  // theirs).  Empty when no flip of the submission is set: such a submission
  // is the path without flips exactly.
  std::vector<uint8_t> flips;
  // Output orientations (spdl_hj_set_orients) travel in `flips` as well, one
  // code 0..7 per descriptor (bit 2: transposed).  A transposed descriptor's
  // ow / oh / dx / dy stay the chain's box, planned from the swapped spec; its
  // final box is oh x ow, and ow / oh above, every group's and the "one size"
  // rule are about final boxes.  transposed: some descriptor has bit 2.
  bool transposed = false;
  int view_refused = 0;  // the first status the host gave a view alone (0: none)
  int view_refused_group = 0, view_refused_index = 0;
  // A ragged submission (spdl_hj_set_ragged): every image its own box at its
  // own offset, so ow / oh / out_elems_per_image above address nothing, and
  // the output path is chosen per image.  The flat sws grid (sws_map) holds
  // the tiles of the fused-eligible images first, [0, fused_wgs): those images
  // have idct_blocks == 0 and their idct_rgb_kernel tiles in sws_wg0,
  // sws_bands (MCU rows) and sws_chunks (tiles per MCU row).  The tiles of
  // every other image (and the one workgroup of a refused one) follow,
  // [fused_wgs, sws_wgs): sws_kernel's.
  bool ragged = false;
  int64_t fused_wgs = 0;
  // Reduced-size decode (spdl_hj_set_lowres): one level 0..3 per image.  Empty
  // when every level of the submission is 0: such a submission is the path
  // without the call exactly.  Otherwise idct_lowres_kernel transforms every
  // image over the flat IDCT grid: ImageDesc::idct_blocks counts its lanes --
  // the blocks of a level-0 image, lowres_lanes() of any other -- and the
  // planes, windows and plans of an image with L > 0 are the reduced frame's.
  std::vector<uint8_t> lowres;
  int lowres_images = 0;  // images with L > 0
};

// The frame FFmpeg's decoder emits at lowres L: ceil(x / 2^L) a side
inline int lowres_side(int x, int lv) { return (x + (1 << lv) - 1) >> lv; }
// idct_lowres_kernel's lanes of component plane bw x bh blocks at level L > 0:
// a lane owns 8 bytes of each of the 8 >> L plane rows of one block row --
// the 2^L blocks under them -- so a block row takes ceil(bw / 2^L) lanes and
// the plane's stride is 8 bytes a lane
inline int lowres_lanes_row(int bw, int lv) { return (bw + (1 << lv) - 1) >> lv; }

// What spdl_hj_set_views left for the next submission: the groups, their view
// arrays copied.  `bad`: the call's own arguments broke a limit (more groups
// than views::kMaxGroups, a group without views) -- the consuming call says so.
struct HeldViews {
  struct Group {
    spdl_hj_output out;
    void* out_dev;
    size_t out_bytes;
    std::vector<spdl_hj_view> views;
    int32_t* status;
  };
  std::vector<Group> groups;
  bool bad = false;
  bool any() const { return bad || !groups.empty(); }
};

// One submission as the planner sees it: n images at offsets[i], sizes[i] of
// the batch's bytes with their probes.  piece_bytes: the size from which a
// file is decoded by several entropy workgroups (0: never).  plans == nullptr:
// no output stage (the raw planes surface).  crops (n rectangles) and views
// are optional and exclude each other.  flips (nflips bytes, SPDL_HJ_FLIP_*):
// optional, one per image, or with views one per view, the groups
// concatenated in group order.  lowres (nlowres bytes, 0..3): optional, one
// level per image; excludes crops and views.  orients (norients bytes, 0..7): the same
// places and counts; flips and orients on one request are refused.
// ragged (n byte offsets into an output of out_bytes bytes): optional, lifts
// the one-size rule (spdl_hipjpeg.h "ragged batches"); output_path: the
// context's knob, which in a ragged submission decides per image (0: the
// fused kernel where an image is eligible; else the generic kernel alone).
struct LayoutRequest {
  const int64_t* offsets;
  const int64_t* sizes;
  const spdl_hj_image_info* infos;
  int n;
  const spdl_hj_output* out;
  int64_t piece_bytes;
  PlanCache* plans;
  const spdl_hj_rect* crops = nullptr;
  const HeldViews* views = nullptr;
  const uint8_t* flips = nullptr;
  int64_t nflips = 0;
  const uint8_t* orients = nullptr;
  int64_t norients = 0;
  const int64_t* ragged = nullptr;
  int64_t out_bytes = 0;
  int output_path = 0;
  // spdl_hj_set_lowres: nlowres levels (0..3), one per image; null: none
  const uint8_t* lowres = nullptr;
  int64_t nlowres = 0;
};

// The chain that runs ahead of a transpose: the output spec describes the
// final output, so fit, pad and crop each have their pair swapped.
inline spdl_hj_output swapped_chain(spdl_hj_output o) {
  std::swap(o.fit_w, o.fit_h);
  std::swap(o.pad_w, o.pad_h);
  std::swap(o.crop_w, o.crop_h);
  return o;
}

// rc, and on failure its text and the image it is the status of (-1: none --
// the call's own arguments).  The statuses of views the planner refuses alone
// go to their groups' status arrays, once every limit has held.
struct LayoutResult {
  int rc = SPDL_HJ_OK;
  int image = -1;
  char err[256] = "";
};

LayoutResult build_layout(const LayoutRequest& rq, Layout& L);

// The frame image p's output chain reads: the whole frame, or its source crop
// `in` resolved (null or all zero: none).  0, or why the crop does not resolve.
int source_frame(const spdl_hj_image_info& p, const spdl_hj_rect* in, views::Rect* src);

// The box of a w x h frame through chain `out` under orientation `code`
// (0..7): g is the geometry of the chain that runs ahead of the transpose
// (swapped_chain with bit 2), *fw x *fh the final box -- g's, swapped with bit 2.
int final_box(int w, int h, const spdl_hj_output& out, int code, Geom* g, int* fw, int* fh);

// spdl_hj_ragged_layout (spdl_hipjpeg.h): each image's final box resolved
// alone, packed at multiples of align_bytes.  The planner resolves a ragged
// submission's boxes through the same two functions above.
int ragged_layout(const spdl_hj_image_info* infos, int n, const spdl_hj_output* out,
                  const spdl_hj_rect* crops, const uint8_t* orients, int64_t align_bytes,
                  int64_t* offsets, int32_t* ow, int32_t* oh, int32_t* status);

}  // namespace hj
