// hj_launch.h -- the seam between the host driver (hj_host.cpp) and the
// kernels (hj_kernels.hip): the one declaration of every launcher, included
// by both, so the compiler checks each definition against the driver's calls.
// A launcher takes the batch's device buffers as one struct plus what is
// particular to its stage, and unpacks the struct into kernel arguments.
#pragma once
#include <hip/hip_runtime.h>

#include "hj_common.h"

namespace hj {

// One batch's device buffers (layouts: hj_common.h), filled once per batch
struct BatchBuffers {
  const uint8_t* bytes;  // the packed files (the caller's, or the slot's copy)
  uint8_t *clean, *planes;
  uint32_t *segs, *ents, *recs;
  uint32_t* work;  // entropy work list, nwork items (behind the descriptors)
  DsChunk* dschunks;
  ImageDesc* desc;
  ImageInfo* infos;
  HuffTable* luts;
  uint2* bdesc;
  uint64_t* chain;
  int32_t* wts;
  int16_t* hbuf;
  // flat-grid dispatch maps (workgroup -> image, written by parse_kernel).  A
  // launcher's `flat` picks that grid; else (largest image's tiles, image), no map
  uint32_t *ds_map, *idct_map, *hs_map, *sws_map;
  int n, nwork;  // images, entropy work items
  // descriptors: n, or in a views submission the n images' and then the views'
  // (ImageDesc::src).  The front-end kernels launch over n; parse_kernel also
  // brings the views' descriptors over and maps their output workgroups.
  int ndesc;
  // output flips (spdl_hj_set_flips): one byte per descriptor behind the work
  // list; null when the submission sets none -- sws_kernel and
  // yuv_planes_kernel then load nothing
  const uint8_t* flips;
  // ... or its orientation codes (spdl_hj_set_orients, 0..7) in the same place;
  // transposed: one of them has bit 2, and sws_kernel<true> runs
  bool transposed;
  // reduced-size levels (spdl_hj_set_lowres): one byte per image behind the
  // flips; null when every level is 0 -- idct_kernel then runs as ever
  const uint8_t* lowres;
};

// parse_kernel + lut_kernel.  host_desc (descriptors, then the work list) and
// host_tables (the swscale tables, -> wts): what parse_kernel pulls from the
// slot's pinned staging, as the device sees those pages; null / 0 when DMA
// copies brought them ("host_staging" 0).
hipError_t launch_parse(const BatchBuffers& b, const ImageDesc* host_desc, const void* host_tables,
                        int64_t table_bytes, int threads, hipStream_t st);
hipError_t launch_destuff(const BatchBuffers& b, bool flat, int ds_wgs, int max_chunks,
                          hipStream_t st);
hipError_t launch_entropy(const BatchBuffers& b, const EntropyParams& ep, int threads, int lds_pad,
                          hipStream_t st);
hipError_t launch_multiscan(const BatchBuffers& b, hipStream_t st);
// idct_kernel<idct> (0 simple, 1 islow, 2 kAblIdctNone); xcd: XCD-aware tile order
hipError_t launch_idct(const BatchBuffers& b, int idct, bool flat, int idct_wgs, int max_blocks,
                       int xcd, hipStream_t st);
// idct_lowres_kernel<idct> over the flat IDCT grid: every image of a submission
// with reduced-size levels (b.lowres), the level-0 ones as idct_kernel does
hipError_t launch_idct_lowres(const BatchBuffers& b, int idct, int idct_wgs, hipStream_t st);
hipError_t launch_cmyk(const BatchBuffers& b, int64_t max_px, hipStream_t st);
// Output kernels.  host_status: the slot's pinned status array (device view) or null
hipError_t launch_csc(const BatchBuffers& b, void* out, const BatchParams& p, int64_t max_px,
                      int32_t* host_status, hipStream_t st);
// turbo_rgb_kernel (csc = TURBO) over its flat grid: every image's own tiles, the first
// turbo_wgs workgroups of sws_map (Layout::sws_wgs), plain and ragged submissions alike
hipError_t launch_turbo_rgb(const BatchBuffers& b, void* out, const BatchParams& p, int turbo_wgs,
                            int32_t* host_status, hipStream_t st);
hipError_t launch_rgb_unscaled(const BatchBuffers& b, void* out, const BatchParams& p,
                               int64_t max_px, int32_t* host_status, hipStream_t st);
hipError_t launch_idct_rgb(const BatchBuffers& b, void* out, const BatchParams& p, int idct,
                           int tiles, int32_t* host_status, hipStream_t st);
// idct_rgb_kernel over its flat grid: the fused-eligible images of a ragged submission, the
// first fused_wgs workgroups of sws_map (Layout::fused_wgs)
hipError_t launch_idct_rgb_flat(const BatchBuffers& b, void* out, const BatchParams& p, int idct,
                                int fused_wgs, int32_t* host_status, hipStream_t st);
// hscale_kernel first when hs_wgs > 0; yuv_planes_kernel's grid is always flat.
// wg0 (flat grids): the launch's first workgroup in sws_map -- a views
// submission launches sws_kernel once per group over that group's tiles.
hipError_t launch_sws(const BatchBuffers& b, void* out, const BatchParams& p, bool flat,
                      int sws_wgs, int bands, int chunks, int lds_bytes, int hs_wgs,
                      int32_t* host_status, hipStream_t st, int wg0 = 0);
hipError_t launch_yuv_planes(const BatchBuffers& b, void* out, int sws_wgs, int lds_bytes,
                             int hs_wgs, int32_t* host_status, hipStream_t st);
// The video path's converter, outside any batch (spdl_hj_nv12_to_planar_rgb).
hipError_t launch_nv12(const uint8_t* src, uint8_t* dst, int frames, int height, int width,
                       int bgr, int coeff, hipStream_t st);

}  // namespace hj
