// hj_resample.h -- the Pillow-exact resize (spdl_hipjpeg.h "Pillow-exact
// resize"): Pillow's ImagingResample coefficient rule for 8-bit channels,
// restated, the per-axis tables resample_kernel reads, and its tiler.  Host
// arithmetic only -- integers and doubles, no HIP type -- so a native program
// links hj_resample.cpp beside the planner (tests/native/resample_sweep.cpp).
// What the kernel shares with it -- ResampleDesc, the LDS layout, a tile's
// window -- is in hj_common.h.
#pragma once
#include <stdint.h>

#include <map>
#include <memory>
#include <tuple>
#include <vector>

#include "../../include/spdl_hipjpeg.h"
#include "hj_common.h"
#include "hj_layout.h"

namespace hj {
namespace rs {

// The most taps one output sample may take on an axis
// (SPDL_HJ_RESAMPLE_MAX_TAPS); the smallest tile of an axis pair at the limit
// fits kLdsBudget with any of the three filters (see tile()).
constexpr int kMaxTaps = SPDL_HJ_RESAMPLE_MAX_TAPS;
// resample_kernel's dynamic LDS: the most a launch may ask for without an
// attribute of its own.  A typical training resize (2x down into 224) takes 36 KiB.
constexpr int kLdsBudget = 64 * 1024;
constexpr int kTileW = 64, kTileH = 32, kStripRows = 32;  // the tiler's first choice
// ... and of a one-channel output (SPDL_HJ_FMT_L / _Y): a pixel is a byte in
// the strip and the intermediate, a quarter of the words, so twice the columns
// still take half the LDS of a three-channel tile and the halo columns two
// neighbouring tiles both stage are staged half as often.  The rows stay: the
// vertical pass runs 8 columns a thread, and 128 x 32 is two such groups a
// thread, where a taller tile would only lengthen the intermediate.
constexpr int kTileW1 = 128;

// One axis of a resample: the box [in0, in1) of inSize samples into outSize
// (an integer request: in0 = 0, in1 = inSize of the cropped frame).
// Output xx sums n[xx] samples from xmin[xx] on with the row K[xx * ksize ..];
// ksize = max n.  blob is the three tables as the pool holds them:
// xmin[outSize], n[outSize], K[outSize * ksize].
struct Axis {
  int in = 0, out = 0, filter = 0, ksize = 0;
  double in0 = 0, in1 = 0;
  std::vector<int32_t> blob;
  const int32_t* xmin() const { return blob.data(); }
  const int32_t* n() const { return blob.data() + out; }
  const int32_t* K() const { return blob.data() + 2 * (size_t)out; }
  int xmax(int xx) const { return xmin()[xx] + n()[xx]; }
};

// The tap count of the widest output of an axis, without building it
int axis_taps(int in, double in0, double in1, int out, int filter);
inline int axis_taps(int in, int out, int filter) { return axis_taps(in, 0.0, (double)in, out, filter); }
// The axis, or null: sizes outside 1..65535, an unknown filter, or more than
// kMaxTaps taps (*rc = SPDL_HJ_ERR_BAD_GEOMETRY)
std::shared_ptr<const Axis> make_axis(int in, double in0, double in1, int out, int filter, int* rc);
inline std::shared_ptr<const Axis> make_axis(int in, int out, int filter, int* rc) {
  return make_axis(in, 0.0, (double)in, out, filter, rc);
}

// Axes by (inSize, in0, in1, outSize, filter): an integer box's origin is not
// in the key, the kernel adds it; a float box's xmin is absolute in its frame.  The context's; a RandomResizedCrop stream has a new key per
// image, so the cache is emptied when it has grown to kCap axes.
struct AxisCache {
  static constexpr size_t kCap = 512;
  // The channel count the tiler sizes its tiles for, 3 or 1: the host sets it
  // from the submission's format ahead of the plan (place* take no such
  // argument: their signatures are the planner's function pointers)
  int channels = 3;
  std::map<std::tuple<int, double, double, int, int>, std::shared_ptr<const Axis>> held;
  std::shared_ptr<const Axis> get(int in, double in0, double in1, int out, int filter, int* rc);
  std::shared_ptr<const Axis> get(int in, int out, int filter, int* rc) {
    return get(in, 0.0, (double)in, out, filter, rc);
  }
};

// One image's request against its W x H frame and the out_w x out_h box:
// the box (it->box.w == 0: the whole frame), the resized picture, the window.
struct Geo {
  int bx, by, bw, bh, rw, rh, ox, oy;
};
int resolve(const spdl_hj_resample_item* it, int W, int H, int out_w, int out_h, Geo* g);

// The tiling of one image: the largest tile whose coefficient rows, strip and
// intermediate fit kLdsBudget.  0 and *d (tables' offsets left 0), *bands x
// *chunks tiles; SPDL_HJ_ERR_BAD_GEOMETRY and everything zero when the
// smallest tile does not fit.
int tile(const Axis& H, const Axis& V, const Geo& g, int out_w, int out_h, ResampleDesc* d,
         int* bands, int* chunks, int nch = 3);

// One image of a resampled submission, whole: its request resolved, its two
// axes from the cache, its tiling.  0, or why the image is refused alone.
struct Placed {
  std::shared_ptr<const Axis> H, V;
  ResampleDesc d;
  int bands, chunks;
};
int place(AxisCache& cache, int filter, const spdl_hj_resample_item* it, int W, int H, int out_w,
          int out_h, Placed* out);
// ... and its axes' tables placed, each once, in the submission's table pool:
// the planner's ResampleRequest::place (`cache`: an AxisCache)
int place_into(void* cache, int filter, const spdl_hj_resample_item* it, int W, int H, int out_w,
               int out_h, std::vector<int32_t>& tables, ResamplePool& pool, ResampleDesc* d,
               int* bands, int* chunks);

// ---- spdl_hj_set_resample_box: Pillow's float box= and reducing_gap= ----
// One image's request against its W x H frame, resolved in Pillow's order: the
// factors (1, 1 without a gap), the safe box q = (x0, y0, x1, y1), the reduced
// picture cw x ch (the frame itself when both factors are 1: q the frame), the
// box in it, and the four cell classes' divisors -- interior, right, bottom,
// corner -- with floor(2^24 / d).
struct BoxGeo {
  int fx, fy, q[4], cw, ch;
  double box[4];
  int div[4];
  uint32_t mult[4];
  int rw, rh, ox, oy;
};
// 0; SPDL_HJ_ERR_INVALID_ARG (the submission's): a gap in (0, 1) or no number,
// a box that is empty or outside the frame; SPDL_HJ_ERR_BAD_GEOMETRY (the
// image's): the resized picture or the window, fx fy above kReduceMaxCell, a
// frame with H > 100 W whose height shrinks
int resolve_box(const spdl_hj_resample_box_item* it, int W, int H, int out_w, int out_h, int filter,
                double gap, BoxGeo* g);

// The tiling for resample_reduce_kernel: windows in reduced cells, no
// alignment (the producer's units are the frame's, not the strip's), and the
// B sums' plane beside the strip (rs::reduce_lds_words)
int tile_reduce(const Axis& H, const Axis& V, const Geo& g, int out_w, int out_h, ResampleDesc* d,
                int* bands, int* chunks, int nch = 3);

// The tiling of an item with an orientation code and no factor: tile()'s for
// three channels, its windows unaligned as tile_reduce()'s -- the producer's
// units are aligned to the STORED frame, which a mirror or a transpose sends
// to no fixed alignment of the displayed one; the kernel drops what a unit
// holds outside the window instead (rs::stored_rect)
int tile_oriented(const Axis& H, const Axis& V, const Geo& g, int out_w, int out_h, ResampleDesc* d,
                  int* bands, int* chunks);

// place_into for a box request.  red == null: the submission has no factor
// above 1 and the record is resample_kernel's; else resample_reduce_kernel's,
// *red beside it.  The planner's ResampleRequest::place_box.
int place_box_into(void* cache, int filter, double gap, const spdl_hj_resample_box_item* it, int W,
                   int H, int out_w, int out_h, std::vector<int32_t>& tables, ResamplePool& pool,
                   ResampleDesc* d, ReduceDesc* red, int* bands, int* chunks);
// ... and what the planner asks ahead of every image: the request's status
// against this frame and whether it has a factor above 1 (ResampleRequest::probe_box)
int probe_box(int filter, double gap, const spdl_hj_resample_box_item* it, int W, int H, int out_w,
              int out_h, int* reduces);

// ---- spdl_hj_set_resample_items: one item against its image's W x H frame ----
// W x H is the STORED frame; an item with an orientation code (it->orient,
// 0..7) is resolved against the displayed one, H x W for codes 4..7, and so
// are its statuses.
// resolve_box of the item's own request.  clamp = 0: as it stands.  clamp = 1:
// the integral box (bx, by) + bw x bh is a frame of its own, the request its
// whole frame: q, cw x ch and the box are relative to (bx, by).
struct ItemGeo {
  BoxGeo b;
  int bx, by;
};
// 0; SPDL_HJ_ERR_INVALID_ARG (the submission's): what resolve_box gives it for,
// a flip outside 0..3, an orientation outside 0..7, an output box outside 1..65535, a clamped box that is
// not integral; SPDL_HJ_ERR_BAD_GEOMETRY (the item's): what resolve_box gives
// it for, a clamped box that is empty or outside the frame
int resolve_item(const spdl_hj_resample_items_item* it, int W, int H, int filter, double gap,
                 ItemGeo* g);
// ... its status and whether it has a factor above 1 (ResampleRequest::probe_item)
int probe_item(int filter, double gap, const spdl_hj_resample_items_item* it, int W, int H,
               int* reduces);
// ... and its record for resample_items_kernel, tables placed once per
// submission.  sum: some item of the submission has a factor above 1 -- every
// record is then tile_reduce()'s with rec->rr set, else tile()'s, or
// tile_oriented()'s for an item with a code.
// (ResampleRequest::place_item; the image, the flip, the offset and the tiles'
// place in the grid are the planner's to fill.)
int place_item_into(void* cache, int filter, double gap, const spdl_hj_resample_items_item* it,
                    int W, int H, bool sum, std::vector<int32_t>& tables, ResamplePool& pool,
                    ItemDesc* rec, int* bands, int* chunks);

}  // namespace rs
}  // namespace hj
