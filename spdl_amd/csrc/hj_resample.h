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

// One axis of a resample: inSize samples over [0, inSize) into outSize.
// Output xx sums n[xx] samples from xmin[xx] on with the row K[xx * ksize ..];
// ksize = max n.  blob is the three tables as the pool holds them:
// xmin[outSize], n[outSize], K[outSize * ksize].
struct Axis {
  int in = 0, out = 0, filter = 0, ksize = 0;
  std::vector<int32_t> blob;
  const int32_t* xmin() const { return blob.data(); }
  const int32_t* n() const { return blob.data() + out; }
  const int32_t* K() const { return blob.data() + 2 * (size_t)out; }
  int xmax(int xx) const { return xmin()[xx] + n()[xx]; }
};

// The tap count of the widest output of an axis, without building it
int axis_taps(int in, int out, int filter);
// The axis, or null: sizes outside 1..65535, an unknown filter, or more than
// kMaxTaps taps (*rc = SPDL_HJ_ERR_BAD_GEOMETRY)
std::shared_ptr<const Axis> make_axis(int in, int out, int filter, int* rc);

// Axes by (inSize, outSize, filter): a box's origin is not in the key, the
// kernel adds it.  The context's; a RandomResizedCrop stream has a new key per
// image, so the cache is emptied when it has grown to kCap axes.
struct AxisCache {
  static constexpr size_t kCap = 512;
  std::map<std::tuple<int, int, int>, std::shared_ptr<const Axis>> held;
  std::shared_ptr<const Axis> get(int in, int out, int filter, int* rc);
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
         int* bands, int* chunks);

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

}  // namespace rs
}  // namespace hj
