/*
 * spdl_hipjpeg.h -- C-ABI of the MI355X (gfx950) JPEG decode stage.
 *
 * This is the drop-in boundary that replaces SPDL's nvJPEG/NPP stack:
 *   Python  spdl.io.decode_image_nvjpeg / load_image_batch_nvjpeg
 *           (reference src/spdl/io/_core.py:868-915, src/spdl/io/_composite.py:486-524)
 *   binding src/spdl/io/lib/cuda/decoding_nvjpeg.cpp:39-97 (nanobind, GIL released)
 *   engine  src/libspdl/cuda/nvjpeg/decoding.cpp:157-255 (decode_image_nvjpeg single/batch)
 *           src/libspdl/cuda/npp/detail/resize.cpp:36-116 (resize_npp)
 * and, for the CPU-path-compatible entry points, the FFmpeg image path behind
 *   spdl.io.load_image_batch (src/spdl/io/_composite.py:358-465).
 *
 * Plain C types only: pointers, sizes, ints.  No torch types.  Every function
 * returns 0 on success or a SPDL_HJ_ERR_* code, and writes a NUL-terminated
 * message into `err` (when non-NULL) on failure -- the Python layer turns that
 * into RuntimeError("Failed to decode an image. (...)"), matching the
 * reference's CHECK_NVJPEG behaviour (src/libspdl/cuda/nvjpeg/detail/utils.h:53-61).
 *
 * Threading: a context is used by one thread at a time (the reference keeps
 * its nvJPEG state thread_local, decoding.cpp:107-112); create one per thread.
 * Every call is GIL-free (ctypes releases the GIL).
 */
#ifndef SPDL_HIPJPEG_H
#define SPDL_HIPJPEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPDL_HJ_ABI_VERSION 7

enum spdl_hj_status {
  SPDL_HJ_OK = 0,
  SPDL_HJ_ERR_NOT_JPEG = 1,
  SPDL_HJ_ERR_UNSUPPORTED = 2,  /* arithmetic, lossless, hierarchical, 12-bit */
  SPDL_HJ_ERR_BAD_HEADER = 3,
  SPDL_HJ_ERR_BAD_HUFFMAN = 4,
  SPDL_HJ_ERR_TRUNCATED = 5,
  SPDL_HJ_ERR_BAD_RESTART = 6,
  SPDL_HJ_ERR_BAD_GEOMETRY = 7,
  SPDL_HJ_ERR_INVALID_ARG = 8,
  SPDL_HJ_ERR_HIP = 9,
  SPDL_HJ_ERR_OOM = 10,
  /* (since ABI 6) a large restart-free file is decoded by several entropy
   * workgroups that hand run states across; a hand-off wait that polled
   * "handoff_wait_us" with nothing arriving gives up with this status.  The
   * library then re-decodes that image in one workgroup before reporting the
   * batch (spdl_hj_wait / a sync call), so callers see it only if that
   * re-decode itself fails to run. */
  SPDL_HJ_ERR_HANDOFF = 11,
};

/* output pixel formats (reference nvjpeg/detail/utils.cpp:94-110):
 * RGB/BGR planar [3,H,W]; RGB24/BGR24 interleaved [H,W,3].
 *
 * YUV (since ABI 7): the frame's own planar format -- what the reference's
 * filter graph returns when the chain has no format node (load_image_batch
 * with pix_fmt=None, src/spdl/io/_composite.py:438-462): gray8 stays gray8,
 * yuvj444p / yuvj422p / yuvj420p keep their subsampling.  With hs, vs the
 * frame's chroma ratios (1,1 / 2,1 / 2,2) and ow x oh the output size,
 *   cw = ceil(ow / hs), ch = ceil(oh / vs)
 *   per image: Y plane oh x ow, then U ch x cw, then V ch x cw, every plane
 *   tightly packed (av_image_copy_to_buffer order); gray: the Y plane alone
 *   bytes per image = ow * oh + 2 * cw * ch        (gray: ow * oh)
 * and image i starts at i * bytes per image; size out_dev from these.
 * Accepted: gray, and YCbCr with chroma ratios (1,1), (2,1), (2,2).  4:4:0,
 * 4:1:1, 4:1:0, 1x4, RGB-coded and 4-component frames, and an image whose
 * format differs from image 0's, get SPDL_HJ_ERR_UNSUPPORTED (that image
 * alone when it is not image 0; the others decode).  dtype must be U8 and csc
 * SWSCALE (otherwise the spec is invalid); both IDCTs are allowed. */
enum spdl_hj_pix_fmt {
  SPDL_HJ_FMT_RGB = 0,
  SPDL_HJ_FMT_BGR = 1,
  SPDL_HJ_FMT_RGB24 = 2,
  SPDL_HJ_FMT_BGR24 = 3,
  SPDL_HJ_FMT_YUV = 4,
};

enum spdl_hj_aspect { SPDL_HJ_ASPECT_NONE = 0, SPDL_HJ_ASPECT_DECREASE = 1, SPDL_HJ_ASPECT_INCREASE = 2 };
/* BICUBIC / BILINEAR: swscale flags of the CPU path's scale filter
 * (src/spdl/io/_preprocessing.py:214-234).  LANCZOS: Lanczos-3, the NPP
 * NPPI_INTER_LANCZOS kernel of load_image_batch_nvjpeg's resize
 * (src/libspdl/cuda/npp/detail/resize.cpp:36-116), also swscale flags=lanczos. */
enum spdl_hj_filter {
  SPDL_HJ_FILTER_BICUBIC = 0,
  SPDL_HJ_FILTER_BILINEAR = 1,
  SPDL_HJ_FILTER_LANCZOS = 2
};
/* F16 / BF16: (x/255 - mean)/std in IEEE fp32 (the reference's
 * Preprocessing.forward, examples/imagenet_classification.py:95-106), rounded
 * to nearest even into half / bfloat16. */
enum spdl_hj_dtype { SPDL_HJ_DTYPE_U8 = 0, SPDL_HJ_DTYPE_F16 = 1, SPDL_HJ_DTYPE_BF16 = 2 };
/* IDCT: FFmpeg simple_idct (the reference CPU path) or IJG islow (libjpeg). */
enum spdl_hj_idct { SPDL_HJ_IDCT_SIMPLE = 0, SPDL_HJ_IDCT_ISLOW = 1 };
/* Colour conversion / scaling: SWSCALE is the reference CPU path's libswscale
 * (one context: bicubic/bilinear/lanczos scale + yuvj -> rgb24, BT.601 full
 * range, swscale's chroma siting and fixed-point arithmetic; FilterGraphImpl,
 * src/libspdl/core/detail/ffmpeg/filter_graph.cpp:280-313).  JFIF is IJG
 * libjpeg's integer YCbCr -> RGB with nearest chroma (full resolution only).
 * TURBO (additive in ABI 7) is libjpeg-turbo's default decoder, what Pillow,
 * OpenCV and torchvision decode with: islow IDCT, triangle ("fancy") chroma
 * upsampling and the libjpeg 6b colour tables, full resolution only -- see
 * "Pillow-exact decode" below. */
enum spdl_hj_csc { SPDL_HJ_CSC_SWSCALE = 0, SPDL_HJ_CSC_JFIF = 1, SPDL_HJ_CSC_TURBO = 2 };

/* Output specification.  resize == 0: full resolution, every image in the
 * batch must have the same size (but see "ragged batches").  Otherwise the
 * FFmpeg filter chain SPDL builds (src/spdl/io/_preprocessing.py:214-234) is
 * applied per image:
 *   scale=w=fit_w:h=fit_h[:force_original_aspect_ratio=decrease|increase]
 *   [,pad=w=pad_w:h=pad_h:x=-1:y=-1:color=black][,crop=w=crop_w:h=crop_h]
 * fit_w/fit_h == 0 mean "input size"; pad/crop == 0 mean "absent"; a
 * negative pad or crop size is SPDL_HJ_ERR_BAD_GEOMETRY, as in FFmpeg.
 * Negative fit_w/fit_h (since ABI 7) have vf_scale's meaning
 * (ff_scale_adjust_dimensions): -1 keeps the aspect ratio, -n also makes the
 * result divisible by n.  With fw = max(1, -fit_w), fh = max(1, -fit_h) and
 * rescale(a, b) = a / b rounded to nearest, ties away from zero (av_rescale):
 *   both negative        the input size
 *   fit_w < 0            w = rescale(h * inW, inH * fw) * fw
 *   fit_h < 0            h = rescale(w * inH, inW * fh) * fh
 * before force_original_aspect_ratio is applied (which may undo the
 * divisibility, as in FFmpeg).
 *
 * SPDL_HJ_FMT_YUV with resize == 0 returns the full-resolution planes cropped
 * to each component's true size (the bytes of spdl_hj_decode_planes).  With
 * resize == 1 the chain runs on the frame's own format: one swscale context
 * yuvj4xxp -> yuvj4xxp (gray8 -> gray8), luma and chroma planes each through
 * their own filters (chroma ceil(w / hs) x ceil(h / vs) on both sides, centred
 * siting) and swscale's 8-bit planar writers; pad and crop then move whole
 * planes on the chroma grid:
 *   crop  x = ((w - crop_w) / 2) rounded down to a multiple of hs, y likewise
 *         with vs; a crop_w / crop_h that is no multiple of its ratio gives
 *         that image SPDL_HJ_ERR_BAD_GEOMETRY (vf_crop would shrink it
 *         silently)
 *   pad   x = ((pad_w - w) / 2) rounded down to a multiple of hs, y likewise;
 *         a scaled size or a pad size that is no multiple of its ratio gives
 *         that image SPDL_HJ_ERR_BAD_GEOMETRY: vf_pad rounds the input there
 *         in a way nothing here can pin, and a refusal is better than a guess
 *   pad bytes (color=black): yuvj Y = 0, U = V = 128; gray8 16 (drawutils
 *         uses the limited-range luma of black for gray8)
 * Gray and 4:4:4 have ratio 1: none of the rounding applies to them.
 *
 * Limits of the scale (each SPDL_HJ_ERR_BAD_GEOMETRY for that image): no
 * scaled or output side over 65535; no axis, luma or chroma, whose filter
 * reaches swscale's 256 taps (it would cascade two contexts); and no axis
 * whose ratio src / dst reaches 32768, where swscale's own increment
 * ((src << 16) / dst, an int) no longer fits. */
typedef struct spdl_hj_output {
  int32_t pix_fmt;      /* spdl_hj_pix_fmt */
  int32_t dtype;        /* spdl_hj_dtype; F16/BF16 apply (x/255 - mean)/std */
  int32_t idct;         /* spdl_hj_idct */
  int32_t resize;       /* 0 = none, 1 = apply the chain below */
  int32_t fit_w, fit_h, aspect;
  int32_t pad_w, pad_h;
  int32_t crop_w, crop_h;
  int32_t filter;       /* spdl_hj_filter */
  float mean[3], std[3];
  int32_t csc;          /* enum spdl_hj_csc, since ABI 2 */
} spdl_hj_output;

/* The frame's colour model (since ABI 4), decided at the SOF as FFmpeg's
 * mjpeg decoder picks its pix_fmt: from the Adobe APP14 transform flag seen
 * before the SOF and the component ids.
 *   GRAY    1 component                                        (gray8)
 *   YCBCR   3 components                                       (yuvj4xxp)
 *   RGB     3, Adobe transform 0 or ids 'R' 'G' 'B'; all 1x1   (gbrp)
 *   CMYK    4, all 1x1, Adobe transform 0: inverted CMYK, converted to RGB
 *           in the decoder (R = C K 257 >> 16 ...)              (gbrap)
 *   YCCK    4, Adobe transform 2: converted to YCbCr            (yuva444p)
 *   YCBCRK  4, other or no marker: YCbCr, K dropped             (yuva444p)
 * 4-component files may be sequential (interleaved or not) or progressive. */
enum spdl_hj_color {
  SPDL_HJ_COLOR_GRAY = 0,
  SPDL_HJ_COLOR_YCBCR = 1,
  SPDL_HJ_COLOR_RGB = 2,
  SPDL_HJ_COLOR_CMYK = 3,
  SPDL_HJ_COLOR_YCCK = 4,
  SPDL_HJ_COLOR_YCBCRK = 5,
};

typedef struct spdl_hj_image_info {
  int32_t width, height, ncomp;
  int32_t h_samp[4], v_samp[4];
  int32_t color;  /* enum spdl_hj_color, since ABI 4 */
  /* 1: the multi-scan path decodes the file -- progressive (SOF2), or a
   * first scan holding fewer components than the frame (since ABI 5).  A
   * batch holding such a file runs that path on a side stream beside the
   * baseline stages (spdl_hj_decode_batch_device included). */
  int32_t multiscan;
} spdl_hj_image_info;

typedef struct spdl_hj_ctx spdl_hj_ctx;

/* ---- source crop (additive in ABI 7: two functions, one type, one read-only
 * parameter; a binding finds them by symbol) --------------------------------
 * A rectangle of the decoder's own frame, taken before anything else: what
 * the reference's filter graph does for "crop=w:h:x:y,scale=..."
 * (src/spdl/io/_preprocessing.py:248-249) -- libavfilter's crop filter with
 * exact=0, applied while the frame is still yuvj4xxp / gray8 / gbrp (the
 * format constraint reaches back only as far as scale).  The crop moves the
 * plane pointers and shrinks the frame; the chain of spdl_hj_output then
 * builds ONE swscale context for the cropped size.  swscale never reads
 * outside the crop: border taps fold at the crop's edges and chroma comes from
 * the cropped chroma planes.  The result is therefore NOT a slice of the
 * uncropped result (a whole 4:2:0 frame of odd height takes the general
 * scaler, an even-sized crop of it the unscaled converter).
 *
 * With hs, vs the frame's chroma ratios as FFmpeg's pixel format states them
 * (gray, RGB-coded, 4-component and 4:4:4 frames 1, 1; 4:2:2 2, 1; 4:2:0 2, 2;
 * 4:4:0 1, 2; 4:1:1 4, 1; 4:1:0 4, 4; in general hmax / h_samp[1],
 * vmax / v_samp[1]) and W x H the frame:
 *   w is rounded down to a multiple of hs, h to a multiple of vs; a rounded
 *     w or h of 0, or one larger than the frame, is SPDL_HJ_ERR_BAD_GEOMETRY
 *     for that image alone -- the rest of the batch decodes
 *   x < 0 becomes 0, x + w > W becomes W - w, then x is rounded down to a
 *     multiple of hs; y likewise with vs
 *   component c's window is (x >> log2 hs_c, y >> log2 vs_c), of size
 *     ceil(w / hs_c) x ceil(h / vs_c)
 *   x or y may be SPDL_HJ_CROP_CENTER: (W - w) / 2; with a w (h) that is no
 *     multiple of hs (vs) the image is refused with SPDL_HJ_ERR_BAD_GEOMETRY
 *     (vf_crop's order of rounding and centring is not pinned here, and a
 *     refusal beats a guess)
 *   (0, 0, 0, 0) means no crop for that image
 * These rules restate vf_crop's documented behaviour ("rounded to nearest
 * smaller value"); they are not pinned against FFmpeg itself.
 *
 * Every output format and dtype takes crops (SPDL_HJ_FMT_YUV with its pad /
 * crop grid rules); csc = JFIF with crops is SPDL_HJ_ERR_INVALID_ARG.  With
 * resize == 0 the output is the region itself and all regions of the batch
 * must resolve to one size.  spdl_hj_output_size is unchanged: pass it the
 * resolved w, h.  Only the MCUs a region touches are inverse-transformed
 * ("idct_workgroups"); entropy decode still covers the whole scan. */
#define SPDL_HJ_CROP_CENTER INT32_MIN
typedef struct {
  int32_t x, y, w, h;
} spdl_hj_rect;

/* Resolve one rectangle by the rules above (host only: no device, no
 * context).  (0, 0, 0, 0) resolves to the whole frame. */
int spdl_hj_crop_rect(const spdl_hj_image_info* info, const spdl_hj_rect* in, spdl_hj_rect* out);

/* Set the rectangles of the next batch submission on `ctx`: the next
 * spdl_hj_decode_batch, _device or _staged call consumes them, whether it
 * succeeds or not; n must equal that call's n (else that call returns
 * SPDL_HJ_ERR_INVALID_ARG).  rects == NULL or n == 0 clears them.
 * spdl_hj_decode_planes and spdl_hj_debug_entropy neither use nor clear them. */
int spdl_hj_set_crops(spdl_hj_ctx* ctx, const spdl_hj_rect* rects, int32_t n);

/* ---- views (additive in ABI 7: one function, two types, one read-only
 * parameter; a binding finds them by symbol) ---------------------------------
 * Several outputs of one image from one decode: multi-crop augmentation (two
 * crops at 224 and six at 96 of every file), a thumbnail beside a training
 * crop.  A view is a rectangle of one image of the batch; a group is a list of
 * views that share one output chain and one output buffer.  A views submission
 * parses, destuffs and Huffman-decodes every image once, inverse-transforms
 * the bounding MCU rectangle of all of the image's views once
 * ("idct_workgroups"), and runs the output stage once per group.
 *
 * Consumption.  The next spdl_hj_decode_batch, _device or _staged call on
 * `ctx` consumes the views, whether or not it succeeds (the rule of
 * spdl_hj_set_crops).  groups == NULL or ngroups == 0 clears them.  The
 * library copies the groups and their view arrays at spdl_hj_set_views; a
 * group's out_dev and status must stay valid until the batch has been waited
 * for.  spdl_hj_decode_planes and spdl_hj_debug_entropy neither use nor clear
 * them.
 *
 * Limits.  ngroups is 1..4 and nviews at least 1 in every group; every `image`
 * lies in [0, n) of the consuming call.  If a limit is broken -- here or
 * below -- the consuming call returns SPDL_HJ_ERR_INVALID_ARG and writes
 * nothing (spdl_hj_set_views itself fails only for a NULL ctx or a negative
 * ngroups).
 *
 * Rectangles.  A view's `rect` follows the source-crop rules exactly:
 * (0, 0, 0, 0) is the whole frame, SPDL_HJ_CROP_CENTER is accepted, sizes and
 * origins round to the chroma grid, and spdl_hj_crop_rect resolves it.  From
 * there on the view is a frame of its own: its own geometry, its own plan, one
 * swscale context per view.
 *
 * Output layout.  Group g's output is [nviews, ...] in view order in its
 * out_dev (out_bytes long); the layout and the per-view size come from its
 * `out` as they do for a batch.  All views of a group must produce one size
 * (with resize == 0: resolve to one size), else SPDL_HJ_ERR_INVALID_ARG, as for
 * crops.  An image may have any number of views in any group, none included
 * (it is then entropy-decoded and no more); views may name images in any
 * order and one image more than once.
 *
 * The consuming call's own arguments.  `out` must be a valid spec with csc =
 * SWSCALE; only its idct field is used, and every group's out.idct must equal
 * it.  out_dev must be NULL and out_bytes 0.  Views and spdl_hj_set_crops on
 * one submission give SPDL_HJ_ERR_INVALID_ARG.
 *
 * Per group.  out.pix_fmt is one of the four RGB / BGR formats, dtype any of
 * the three, csc SWSCALE.  SPDL_HJ_FMT_YUV or csc = JFIF in a group gives
 * SPDL_HJ_ERR_INVALID_ARG (planar-YUV views: not yet).
 *
 * Statuses.  A view the host refuses alone -- a rectangle that does not
 * resolve, a chain its size cannot take (SPDL_HJ_ERR_BAD_GEOMETRY) -- has
 * that status in its group's status[k] (optional, host, nviews ints; 0 for
 * the others) before the consuming call returns.  Its bytes stay untouched;
 * the other views and images decode.  An image's decode status arrives as for
 * any batch: the call's status[n], or spdl_hj_wait.  A view is valid when its
 * own status and its image's are both 0; the views of a failed image are left
 * untouched.  With sync != 0 the call fails if any image failed or any view
 * was refused, as the crop path fails for a refused image.
 *
 * Large files.  A views submission decodes every image in ONE entropy
 * workgroup, as "entropy_piece_bytes" 0 does: no piece hand-off exists that
 * could give up, and no image is re-decoded (multi-piece decode under views:
 * not yet). */
typedef struct {
  int32_t image;     /* index into the consuming call's batch */
  spdl_hj_rect rect; /* source-crop rules; (0, 0, 0, 0): the whole frame */
} spdl_hj_view;
typedef struct {
  spdl_hj_output out; /* the chain of every view of this group */
  void* out_dev;      /* device memory, [nviews, ...] in view order */
  size_t out_bytes;
  const spdl_hj_view* views;
  int32_t nviews;
  int32_t* status;    /* optional, host, nviews */
} spdl_hj_view_group;
int spdl_hj_set_views(spdl_hj_ctx* ctx, const spdl_hj_view_group* groups, int32_t ngroups);

/* ---- output flips (additive in ABI 7: one function, one enum; a binding
 * finds it by symbol) -----------------------------------------------------------
 * The random horizontal flip of a training recipe, in the store of the output
 * kernel.  The flip is the LAST node of the chain: libavfilter's
 *   scale=...[,pad=...][,crop=...][,format=...],hflip / vflip
 * where format negotiates back to scale, so hflip and vflip run on the final
 * pixel format.  With ow x oh the output size, for the bits that are set:
 *   packed and planar RGB / BGR   out'(x, y) = out(ow - 1 - x, oh - 1 - y)
 *   SPDL_HJ_FMT_YUV               every plane mirrored by its own width and
 *                                 height (cw = ceil(ow / hs), ch = ceil(oh / vs)),
 *                                 as vf_hflip / vf_vflip do; gray8 its one plane
 * for every dtype, with and without resize, with source crops, and in views.
 * Pad bytes belong to the image and move with it.  An image or view whose flip
 * is 0 is byte-identical to the same submission without flips; a failed image
 * or a refused view stays untouched.
 *
 * Not offered: a flip AHEAD of the scale.  Its pixels differ -- swscale's
 * filter positions are not mirror-symmetric, and the chroma of an odd width
 * pairs differently -- and nothing here pins them.
 *
 * Consumption follows spdl_hj_set_crops: the next spdl_hj_decode_batch,
 * _device or _staged call consumes the flips, whether or not it succeeds;
 * flips == NULL or n == 0 clears them; the library copies the array;
 * spdl_hj_decode_planes and spdl_hj_debug_entropy neither use nor clear them.
 * A plain or cropped submission takes n == the call's n.  A views submission
 * takes one entry per view, the groups concatenated in group order (a refused
 * view keeps its entry: the indexing never shifts).  A wrong count, a value
 * above 3, or csc = JFIF with any non-zero flip give SPDL_HJ_ERR_INVALID_ARG
 * from the consuming call, with nothing written.
 *
 * Cost.  With resize != 0 and for SPDL_HJ_FMT_YUV the flip is address
 * arithmetic in the kernel that stores the tile.  A full-resolution (resize ==
 * 0) RGB / BGR u8 submission with any flip set runs the generic output kernel
 * ("output_path" 1, byte-identical pixels) instead of the unscaled converters,
 * which is slower; all-zero flips keep the fast path. */
enum { SPDL_HJ_FLIP_H = 1, SPDL_HJ_FLIP_V = 2 }; /* both: a rotation by 180 degrees */
int spdl_hj_set_flips(spdl_hj_ctx* ctx, const uint8_t* flips, int32_t n);

/* ---- output orientation (additive in ABI 7: three functions, one enum; a
 * binding finds them by symbol) ------------------------------------------------
 * The other four orientations of a rectangle -- transpose, transverse and the
 * two quarter turns -- and with them what a JPEG's EXIF tag 0x0112 asks for,
 * in the store of the output kernel.  An orientation code is 0..7: bits 0 and
 * 1 are the flips above, bit 2 is a transpose applied BEFORE them.  With C the
 * chain's result, cw wide and ch tall:
 *   with T      A(x, y) = C(y, x), ch wide and cw tall;   without   A = C
 *   then        out(x, y) = A(H ? aw - 1 - x : x, V ? ah - 1 - y : y)
 * with aw x ah the size of A.  Codes 0..3 are exactly the flips.
 *
 * The output spec describes the FINAL output.  For an image or view with T,
 * the chain ahead of the transpose is the spdl_hj_output with each pair
 * swapped -- (fit_w, fit_h), (pad_w, pad_h), (crop_w, crop_h) -- so a final
 * W x H is libavfilter's
 *   scale=w=H:h=W...,pad=w=PH:h=PW,crop=w=CH:h=CW,transpose=dir
 * A source crop rectangle and a view's rectangle stay in the stored frame's
 * coordinates: they are not swapped.  Every image of a batch and every view of
 * a group so still produces one shape and one byte count, whatever its code;
 * spdl_hj_output_size is unchanged -- for a T image pass it the stored
 * frame's (h, w).  With resize == 0 the "one size" rule is about final sizes:
 * a stored 640x480 frame with code 0 and a stored 480x640 frame with code 5
 * share a batch.  Like a flip, the orientation changes no pixel: the bytes are
 * the chain's, permuted, pad included.
 *
 * Not offered: a transpose AHEAD of the scale.  swscale's horizontal pass (to
 * 15 bits) and its vertical pass round differently, so rotating the source
 * first has other pixels, and nothing here pins them.  The geometry is the
 * same; the pixels are those of the stored frame's chain.  Nor a transposed
 * SPDL_HJ_FMT_YUV: a transposed 4:2:2 frame is another pixel format.
 *
 * Consumption, counts, the indexing with views (one entry per view, the
 * groups concatenated), NULL clearing and "spdl_hj_decode_planes and
 * spdl_hj_debug_entropy neither use nor clear" are exactly as for
 * spdl_hj_set_flips.  SPDL_HJ_ERR_INVALID_ARG from the consuming call, with
 * nothing written: a value above 7; a wrong count; csc = JFIF with any
 * non-zero code; a T code with SPDL_HJ_FMT_YUV; orients together with flips
 * on one submission.  Codes 0..3 with SPDL_HJ_FMT_YUV behave as flips do.  An
 * all-zero array is byte-identical to no call and keeps the fused
 * full-resolution path; any non-zero code at full resolution takes the
 * generic output kernel, as a flip does.
 *
 * Cost.  A submission without a T code runs the kernels of a flipped one.  One
 * with a T code runs another instantiation of the output kernel, whose u8
 * tile leaves as row segments of 4-byte stores with byte ends: for the 256
 * bench images into 224 x 224 rgb24 on one lane, 0.97 of the unoriented rate
 * with the eight codes dealt evenly and 0.96 with every image turned, where
 * a torch pass after an unoriented decode leaves 0.74. */
enum { SPDL_HJ_ORIENT_H = 1, SPDL_HJ_ORIENT_V = 2, SPDL_HJ_ORIENT_T = 4 };
int spdl_hj_set_orients(spdl_hj_ctx* ctx, const uint8_t* orients, int32_t n);

/* The EXIF orientation (tag 0x0112) of a JPEG, 1..8, host only.  The walk goes
 * from SOI to the first SOS and takes the first APP1 whose payload starts
 * "Exif\0\0"; its TIFF header is "II*\0" or "MM\0*"; in IFD0, at its offset,
 * the tag counts when its type is SHORT or LONG, its count 1 and its value in
 * 1..8.  Every read is checked against the segment.  Anything else -- no APP1,
 * XMP in APP1, a truncated segment, an offset outside it, another type or
 * count, a value of 0 or 9 -- is orientation 1 with return 0: EXIF never fails
 * an image.  The function fails only for what spdl_hj_get_image_info fails
 * for (spdl_hj_image_info itself does not grow: callers pass arrays of it). */
int spdl_hj_get_orientation(const uint8_t* data, size_t size, int32_t* exif);

/* EXIF orientation -> orientation code (-1 outside 1..8):
 *   1 -> 0       2 -> 1 (H)     3 -> 3 (HV)      4 -> 2 (V)
 *   5 -> 4 (T)   6 -> 5 (T|H)   7 -> 7 (T|H|V)   8 -> 6 (T|V)
 * so the decoded output is the image as a viewer shows it (Pillow's
 * ImageOps.exif_transpose).  A flip of the displayed image composes as
 * code ^ flip bits. */
int spdl_hj_orient_code(int32_t exif);

/* ---- ragged batches (additive in ABI 7: two functions, two read-only
 * parameters; a binding finds them by symbol) ----------------------------------
 * Every image of one submission its own output size: full-resolution decode
 * of files as they come, and aspect-preserving resizes ("shorter side to 256",
 * scale=256:-1), which the "one size" rule leaves to one call per image.
 *
 * spdl_hj_ragged_layout is host arithmetic, no context and no device.  It
 * resolves each image alone -- crops[i] (NULL or all zero: none) by
 * spdl_hj_crop_rect's rule, the chain by spdl_hj_output_size's, orients[i]
 * (NULL: 0) by the orientation section's, so ow[i] x oh[i] is the FINAL box --
 * and packs image i at offsets[i], a multiple of align_bytes, behind image
 * i - 1; offsets[n] is the size of the buffer.  align_bytes is a multiple of
 * the element size (1 for u8, 2 for f16 / bf16) and at least that.  An image
 * whose crop or geometry does not resolve gets its status in status[i], a
 * 0 x 0 box and no bytes; the call itself fails (INVALID_ARG) only for its own
 * arguments: a NULL array, an invalid spec, or one this extension refuses.
 *
 * spdl_hj_set_ragged gives the NEXT spdl_hj_decode_batch / _device / _staged
 * call n byte offsets; that call consumes them whether or not it succeeds, and
 * NULL / 0 clears them (spdl_hj_set_crops' rule; spdl_hj_decode_planes and
 * spdl_hj_debug_entropy neither use nor clear).  The call then lifts the "one
 * size" rule and writes image i at byte offsets[i] of out_dev in the layout
 * of its own final box: [oh][ow][3] for RGB24 / BGR24, [3][oh][ow] for the
 * planar formats, u8, f16 or bf16.  Nothing else of the buffer is written.
 * The offsets need not come from spdl_hj_ragged_layout and need not ascend;
 * two images placed over each other are the caller's business -- the call
 * checks each image against the buffer, not against its neighbours.
 *
 * Accepted: the four RGB / BGR formats, the three dtypes, resize 0 and 1,
 * source crops, flips and orientation codes (the latter two take the generic
 * output kernel, as in a plain batch; EXIF-oriented full-resolution batches of
 * mixed portrait and landscape files fit one submission this way).  An image
 * whose chain has no geometry, or a size the scaler has no filter for
 * (SPDL_HJ_ERR_BAD_GEOMETRY; the latter is the plan's to say, so
 * spdl_hj_ragged_layout still gives it a box), is refused alone, as one whose
 * crop rounds to nothing is: its bytes stay untouched, its status says so,
 * the rest of the batch decodes.  Every other per-image failure is what it is
 * in a plain batch.
 *
 * SPDL_HJ_ERR_INVALID_ARG from the consuming call, with nothing written: a
 * count other than the batch's n; SPDL_HJ_FMT_YUV; csc = JFIF; views on the
 * same submission; an offset that is negative or no multiple of the element
 * size; an image whose extent reaches past out_bytes.
 *
 * Output kernels.  A plain batch chooses one output kernel for all its images;
 * a ragged one chooses per image.  An image takes the fused IDCT + unscaled
 * converter (idct_rgb_kernel, over a flat grid of the eligible images' tiles
 * alone) when, by itself, it meets what a plain batch must meet as a whole:
 * u8 output, full resolution without crop, flip or orientation, standard
 * 4:2:0 with even width and height or 4:2:2 with even width, "output_path" 0.  Every
 * other image of the same submission goes through idct_kernel and the generic
 * sws_kernel.  "output_path" 1 and 2 both send every image of a ragged
 * submission there (the separate unscaled converter has no ragged launch).
 * The read-only parameters "fused_workgroups" and "generic_workgroups" report
 * what the last ragged submission launched of each (0 after a plain one).
 *
 * Cost (256 images of mixed sizes and samplings at native size to rgb24, one
 * lane / four lanes): one ragged submission 179 k / 254 k img/s, the same
 * images as 256 single-image submissions 2.5 k / 7.9 k, the ragged submission
 * with every image on the generic kernel 166 k / 232 k.  A uniform batch
 * submitted ragged runs the fused kernel over the flat grid at 0.993 to 0.999
 * of the plain batch's rate, within run-to-run spread
 * (tools/ragged_bench.py, profiles/r18/ragged/README.md). */
int spdl_hj_ragged_layout(const spdl_hj_image_info* infos, int32_t n, const spdl_hj_output* out,
                          const spdl_hj_rect* crops, const uint8_t* orients, int64_t align_bytes,
                          int64_t* offsets /* n + 1 */, int32_t* ow, int32_t* oh /* n each */,
                          int32_t* status /* n */);
int spdl_hj_set_ragged(spdl_hj_ctx* ctx, const int64_t* offsets, int32_t n);

/* ---- reduced-size decode (additive in ABI 7: one function; a binding finds
 * it by symbol) ------------------------------------------------------------
 * FFmpeg's mjpeg decoder option `lowres` 1..3 (the reference passes it as
 * decode_config(decoder_options={"lowres": ...})): level L inverse-transforms
 * only the low (8 >> L) x (8 >> L) corner of each block, so the decoder's
 * frame is ceil(width / 2^L) x ceil(height / 2^L) and component c's plane
 * ceil(W' h_c / hmax) x ceil(H' v_c / vmax).  Scale plans, geometry, pad and
 * crop rules, ragged boxes, flips and orientations all take that frame, as
 * FFmpeg's filter graph does.  The pixels are NOT those of the full decode
 * scaled down; the transforms are restated from libavcodec/jrevdct.c
 * (ff_j_rev_dct4 / 2 / 1) whatever `idct` says.
 *
 * levels[i] in 0..3 is image i's level in the next spdl_hj_decode_batch /
 * _device / _staged call, which consumes them whether or not it succeeds;
 * n == that call's n; NULL / 0 clears (spdl_hj_set_flips' rules).  An image of
 * level 0 in such a submission gives the bytes it gives without the call, and
 * all-zero levels are the submission without the call exactly.
 * spdl_hj_decode_planes consumes a one-element setting as well and then
 * returns the reduced planes, tightly packed at the reduced component sizes.
 * spdl_hj_output_size and spdl_hj_ragged_layout know nothing of levels: hand
 * them the reduced width and height.
 *
 * SPDL_HJ_ERR_INVALID_ARG from the consuming call, with nothing written: a
 * count other than n; a level above 3; any level above 0 together with source
 * crops, with views, or with csc = JFIF.  An RGB-coded or 4-component frame
 * with a level above 0 is refused alone (SPDL_HJ_ERR_UNSUPPORTED); the rest of
 * the batch decodes.  The read-only parameter "lowres_images" reports the
 * images with a level above 0 in the last submission, "planes_bytes" the
 * component planes it laid out in the workspace. */
int spdl_hj_set_lowres(spdl_hj_ctx* ctx, const uint8_t* levels, int32_t n);

/* ---- Pillow-exact decode (additive in ABI 7: one value of spdl_hj_csc, one
 * read-only parameter) -----------------------------------------------------------
 * csc = SPDL_HJ_CSC_TURBO is libjpeg-turbo's decoder at its defaults, full
 * resolution: for a 1- or 3-component file the output is
 *   np.asarray(PIL.Image.open(f).convert("RGB"))
 * byte for byte (Pillow linked against libjpeg-turbo), in any of the four
 * RGB / BGR layouts; F16 / BF16 normalise those bytes as every output does.
 * The rules are restated here; no library source is involved.
 *
 * 1. IDCT.  islow, whatever spdl_hj_output.idct says: the field is not
 *    consulted in this mode.
 *
 * 2. Upsampling.  Component c is brought to the frame's size by its own ratio
 *    (hr, vr) = (hmax / h_c, vmax / v_c) from its TRUE plane of
 *    cw x ch = ceil(W h_c / hmax) x ceil(H v_c / vmax) samples.  A neighbour
 *    outside that plane is the edge sample, on both axes; the padded columns
 *    and rows the IDCT wrote behind cw / ch are never neighbours.  With p the
 *    plane, a and b its rows above and below:
 *      (1,1)             copy
 *      (2,1), cw > 2     out[2i]     = (3 p[i] + p[i-1] + 1) >> 2
 *                        out[2i + 1] = (3 p[i] + p[i+1] + 2) >> 2
 *      (1,2)             out[2j]     = (3 p + a + 1) >> 2
 *                        out[2j + 1] = (3 p + b + 2) >> 2
 *      (2,2), cw > 2     s = 3 p + a (upper output row) or 3 p + b (lower), then
 *                        out[2i]     = (3 s[i] + s[i-1] + 8) >> 4
 *                        out[2i + 1] = (3 s[i] + s[i+1] + 7) >> 4
 *      anything else     box replication, as csc = JFIF: (2,1) and (2,2) with
 *                        cw <= 2, and the ratios (4,1), (4,2), (1,4) ...
 *    (with the edge rule the first and last columns of (2,1) are p[0] and
 *    p[cw-1] unchanged, those of (2,2) (4 s + 8) >> 4 and (4 s + 7) >> 4).  The
 *    result is cropped to W x H.  The rules apply to every component, luma
 *    included: a frame whose luma is sampled below its chroma -- (1x1, 2x2,
 *    2x2) -- is accepted and pinned as well.
 *
 * 3. Colour.  With cb, cr centred on 128 and arithmetic right shifts:
 *      R = Y + ((91881 cr + 32768) >> 16)
 *      B = Y + ((116130 cb + 32768) >> 16)
 *      G = Y + ((-22554 cb + 32768 - 46802 cr) >> 16)
 *    clipped to 0..255 (libjpeg 6b's green table, FIX(0.34414) = 22554; csc =
 *    JFIF keeps libjpeg 9's 22553).  Gray replicates Y; an RGB-coded frame is a
 *    copy of its three planes.
 *
 * Accepted: plain submissions (one size per batch) and ragged ones
 * (spdl_hj_set_ragged and spdl_hj_ragged_layout take this csc: files of every
 * size at native size in one submission); the four RGB / BGR formats; the
 * three dtypes; baseline, progressive and non-interleaved files, gray, and
 * every sampling the front end decodes.
 *
 * SPDL_HJ_ERR_INVALID_ARG, nothing written: resize != 0; SPDL_HJ_FMT_YUV;
 * source crops; views; any non-zero flip, orientation code or reduced-size
 * level.  A 4-component frame is refused with SPDL_HJ_ERR_UNSUPPORTED, as
 * with csc = JFIF.
 *
 * Not pinned: a progressive file whose script leaves low AC coefficients
 * unrefined (libjpeg smooths block edges there; this decoder does not), and
 * damaged files.
 *
 * One kernel, turbo_rgb_kernel, converts every image of the submission over a
 * flat grid of 128 x 32 pixel tiles; the read-only parameter
 * "turbo_workgroups" reports its workgroups in the last submission (0 for any
 * other csc). */

/* ABI version of the loaded library (== SPDL_HJ_ABI_VERSION). */
int spdl_hj_abi_version(void);

/* Header probe on the host: SOF fields without decoding.
 * Replaces nvjpegGetImageInfo (reference nvjpeg/decoding.cpp:114-130). */
int spdl_hj_get_image_info(const uint8_t* data, size_t size, spdl_hj_image_info* info);

/* Output geometry (width/height of the output image) for an input of w x h
 * under `out`; lets the caller allocate the output tensor. */
int spdl_hj_output_size(int32_t w, int32_t h, const spdl_hj_output* out, int32_t* out_w,
                        int32_t* out_h);

/* Create / destroy a per-thread decoder context bound to `device`.  The
 * context owns its device workspace (grown on demand) and pinned staging. */
spdl_hj_ctx* spdl_hj_create(int device, char* err, size_t errlen);
void spdl_hj_destroy(spdl_hj_ctx* ctx);

/* Decode a batch of host-resident JPEGs into caller-allocated device memory
 * `out_dev` (out_bytes long) on `stream` (a hipStream_t; NULL = legacy
 * default stream, (void*)2 = per-thread default, the reference's 0x2 sentinel
 * in src/libspdl/cuda/types.h:22-39).  The batch is packed into pinned
 * staging and copied with one hipMemcpyAsync.  Output layout per image is
 * [3,H,W] (planar) or [H,W,3] (interleaved) at offset i * per-image-size
 * (SPDL_HJ_FMT_YUV: the Y, U, V planes and the bytes per image stated at
 * spdl_hj_pix_fmt; an image the call refuses leaves its bytes untouched).
 * status[i] (optional, host) receives the per-image code.  With sync != 0 the
 * call returns after the stream has drained (reference default sync=true,
 * decoding.cpp:247-251) and fails if any image failed. */
int spdl_hj_decode_batch(spdl_hj_ctx* ctx, const uint8_t* const* data, const size_t* sizes,
                         int32_t n, const spdl_hj_output* out, void* out_dev, size_t out_bytes,
                         void* stream, int32_t sync, int32_t* status, char* err, size_t errlen);

/* Device-resident variant: the JPEG bytes are already in HBM, packed in
 * `dev_data` at host-known offsets (each 256-byte aligned).  `infos` are the
 * host probes of the same images (spdl_hj_get_image_info).  No H2D copy of
 * image bytes happens inside the call. */
int spdl_hj_decode_batch_device(spdl_hj_ctx* ctx, const uint8_t* dev_data, size_t dev_bytes,
                                const int64_t* offsets, const int64_t* sizes,
                                const spdl_hj_image_info* infos, int32_t n,
                                const spdl_hj_output* out, void* out_dev, size_t out_bytes,
                                void* stream, int32_t sync, int32_t* status, char* err,
                                size_t errlen);

/* ---- asynchronous submission and the pinned staging ring ----------------
 * A context owns a ring of 10 slots (pinned staging + device copy of the
 * JPEG bytes + descriptor/status staging).  Every decode call takes the next
 * slot; a call with sync == 0 returns once the batch is enqueued: the H2D copy
 * runs on the context's own copy stream and `stream` waits for it, so the host
 * can pack batch k+1 and its copy can run while batch k's kernels execute
 * (the reference copies synchronously: transfer_buffer_impl,
 * src/libspdl/cuda/transfer.cpp:37-67; transfer_tensor's pinned cache,
 * src/spdl/io/_transfer.py:82-177).  A slot is reused 10 submissions later, so
 * wait for a ticket before submitting 10 more batches or its statuses are lost. */

/* Ticket of the most recent submission on `ctx` (0 if none). */
int64_t spdl_hj_last_ticket(spdl_hj_ctx* ctx);

/* Block until the batch `ticket` has finished; per-image codes into
 * status[0..n) (optional); returns the first failure like the sync call. */
int spdl_hj_wait(spdl_hj_ctx* ctx, int64_t ticket, int32_t* status, int32_t n, char* err,
                 size_t errlen);

/* Make `stream` wait (on the device, no host block) for batch `ticket`.
 * The per-image statuses -- and the re-decode of an image whose piece
 * hand-off gave up (SPDL_HJ_ERR_HANDOFF), which rewrites its output slot --
 * come only from spdl_hj_wait: work queued on `stream` may see such an
 * image's output before spdl_hj_wait has re-decoded it. */
int spdl_hj_stream_wait(spdl_hj_ctx* ctx, int64_t ticket, void* stream, char* err,
                        size_t errlen);

/* Zero-repack ingest: take the next slot and return its pinned staging
 * (>= bytes long) so the caller can place a region of its source there
 * directly -- e.g. a run of consecutive tar members, whose payloads are
 * 512-byte aligned inside the archive (reference iter_tarfile,
 * src/spdl/io/_tar.py:33-82, yields them as zero-copy views). */
int spdl_hj_staging_acquire(spdl_hj_ctx* ctx, size_t bytes, uint8_t** host_ptr, int64_t* ticket,
                            char* err, size_t errlen);

/* Multi-threaded memcpy of host memory into an acquired slot. */
int spdl_hj_staging_fill(spdl_hj_ctx* ctx, int64_t ticket, size_t dst_off, const uint8_t* src,
                         size_t len, char* err, size_t errlen);

/* Multi-threaded pread(2) of [file_off, file_off + len) of `fd` into an
 * acquired slot (page cache -> pinned staging, no intermediate copy). */
int spdl_hj_staging_read(spdl_hj_ctx* ctx, int64_t ticket, size_t dst_off, int fd,
                         int64_t file_off, size_t len, char* err, size_t errlen);

/* Decode the images at offsets[i] (256-byte aligned), sizes[i] inside the
 * first `len` staged bytes of slot `ticket`: one hipMemcpyAsync of the whole
 * region, then the device pipeline (same output contract as
 * spdl_hj_decode_batch). */
int spdl_hj_decode_staged(spdl_hj_ctx* ctx, int64_t ticket, size_t len, const int64_t* offsets,
                          const int64_t* sizes, int32_t n, const spdl_hj_output* out,
                          void* out_dev, size_t out_bytes, void* stream, int32_t sync,
                          int32_t* status, char* err, size_t errlen);

/* Index the regular-file members of an in-memory tar archive from byte
 * `start`, at most max_entries: payload offsets/sizes, NUL-terminated names
 * concatenated into `names` (name_offs[i] indexes them; names/name_offs may
 * be NULL).  Same member walk as the reference's InMemoryTarParserImpl
 * (src/spdl/io/lib/archive/tar_iterator.cpp:125-195: ustar magic + checksum,
 * GNU 'L' long names, pax 'x' path records, empty name = end).  *next_pos is
 * where to resume (== size at the end of the archive). */
int spdl_hj_tar_index(const uint8_t* data, size_t size, size_t start, int32_t max_entries,
                      int64_t* offsets, int64_t* sizes, int64_t* name_offs, char* names,
                      size_t names_cap, int32_t* n_out, size_t* next_pos);

/* Raw decoded planes (parity surface, the reference's load_image with
 * filter_desc=None -> yuvj4xxp planes, src/spdl/io/_composite.py:254-295):
 * plane c of image 0 copied to host buffer planes[c] (comp_w x comp_h bytes,
 * tightly packed).  Single image. */
int spdl_hj_decode_planes(spdl_hj_ctx* ctx, const uint8_t* data, size_t size, int32_t idct,
                          uint8_t* const* planes, void* stream, char* err, size_t errlen);

/* Debug/parity surface: run parse + destuff + entropy decode of one image
 * and copy back the dequantised coefficients (nblocks x 64 int16, natural
 * order, MCU order, DC carries the FFmpeg +1024 bias), the destuffed scan
 * bytes, and diagnostics diag[0..3] = {status, clean_len, nseg, sync_rounds},
 * diag[4..7] = entropy phase durations (wall_clock64 ticks, 100 MHz) for
 * round 0, sync rounds, prefix scan, write pass; diag[8..11] debug counters
 * (round-0 symbols, wave iterations, shader clocks, realtime ticks);
 * diag[12 + 3 s .. 14 + 3 s] multi-scan images, scan s < 16: start and end
 * (realtime ticks from the decode start) and Huffman symbols; diag must hold
 * 60 ints. */
int spdl_hj_debug_entropy(spdl_hj_ctx* ctx, const uint8_t* data, size_t size, int16_t* coefs,
                          size_t coef_cap, uint8_t* clean, size_t clean_cap, int32_t* diag,
                          char* err, size_t errlen);

/* Debug/parity surface (additive in ABI 7; needs no device and no context):
 * the scale / colour-conversion plan the library makes of one image, as its
 * decode calls do -- the chain's geometry, then the swscale tables and the
 * tiling of sws_kernel / yuv_planes_kernel.  The algorithm is libswscale's
 * (third-party FFmpeg: sws_init_context and initFilter, libswscale/utils.c;
 * packed_vscale, vscale.c), which runs behind the reference's filter graph
 * (FilterGraphImpl::filter, src/libspdl/core/detail/ffmpeg/filter_graph.cpp:
 * 280-313).
 *   width, height, hsub, vsub  the frame and its chroma shifts (0-2)
 *   mode     0 YCbCr planes, 1 gray, 2 three RGB planes through the luma filters
 *   planar   1: the SPDL_HJ_FMT_YUV destination (mode 0 or 1)
 *   prepass, max_cols  the "sws_prepass" (-1, 0, 1) and "sws_cols" knobs
 * Returns what a decode call's plan returns (SPDL_HJ_ERR_BAD_GEOMETRY: scale
 * filter too long, or a refused chain).  info must hold 40 ints:
 *   [0..4]   special (the unscaled converter), full, gray, gbr, pre
 *   [5..10]  sw, sh, dx, dy, ow, oh (filled even when the plan is refused)
 *   [11..14] taps of the hl, hc, vl, vc filters (trailing zeros cut)
 *   [15..18] their row strides in the tables (taps, multiples of 4)
 *   [19..22] their row counts
 *   [23..31] rb, col_chunk, bands, chunks, LDS bytes, pre_rl, pre_rc, chr_w,
 *            chr_h (planar only)
 * vmode (optional, sh ints; packed outputs only): the row writers, mode |
 * yalpha << 4 | uvalpha << 17 with mode 0 X, 1 One, 2 Two.  pos[i] / coef[i]
 * (optional, i = hl, hc, vl, vc): count[i] positions and count[i] * stride[i]
 * taps, as shipped to the device; call once without them for the sizes. */
int spdl_hj_debug_sws_plan(int32_t width, int32_t height, int32_t hsub, int32_t vsub, int32_t mode,
                           int32_t planar, const spdl_hj_output* out, int32_t prepass,
                           int32_t max_cols, int32_t* info, int32_t* vmode, int32_t* const* pos,
                           int16_t* const* coef);

/* Batched NV12 -> planar RGB (bgr == 0) or BGR: src_dev is
 * [num_frames, h2 = 1.5 H, width] u8 in device memory (pitch = width), dst_dev
 * [num_frames, 3, H, width] u8.  matrix_coeff selects the matrix (1 BT.709
 * default, 4 FCC, 5 BT.470, 6 BT.601, 7 SMPTE240M, 8 YCgCo, 9 BT.2020,
 * 10 BT.2020C; other values mean 1).  Replaces nv12_to_planar_rgb/bgr
 * (reference src/libspdl/cuda/color_conversion.cpp:27-95,
 * detail/color_conversion.cu:90-138); like it, quads with x + 1 >= width are
 * not written.  Needs no context (stateless). */
int spdl_hj_nv12_to_planar_rgb(const uint8_t* src_dev, int32_t num_frames, int32_t h2,
                               int32_t width, int32_t bgr, int32_t matrix_coeff, uint8_t* dst_dev,
                               size_t dst_bytes, int device, void* stream, int32_t sync, char* err,
                               size_t errlen);

/* Host <-> device copy of `bytes` (kind 0: host -> device, 1: device ->
 * host).  pinned != 0: hipMemcpyAsync on `stream`, then the stream is
 * synchronised; otherwise a synchronous hipMemcpy.  Replaces
 * transfer_buffer_impl / transfer_buffer (reference
 * src/libspdl/cuda/transfer.cpp:37-105). */
int spdl_hj_copy(void* dst, const void* src, size_t bytes, int32_t kind, int device, void* stream,
                 int32_t pinned, char* err, size_t errlen);

/* Per-stage timing of the last batch, in microseconds, measured with HIP
 * events on the decode stream (filled only when enabled; -1 for a stage
 * outside "profile_stages").  The "idct" stage
 * includes the multi-scan launch (or the wait for its side stream). */
int spdl_hj_set_profiling(spdl_hj_ctx* ctx, int32_t enable);
int spdl_hj_last_timings(spdl_hj_ctx* ctx, float* us, int32_t cap, int32_t* n_out);
/* Names of the timed stages in the order spdl_hj_last_timings reports them. */
const char* spdl_hj_stage_name(int32_t i);

/* Tuning knobs: "sub_bits" (slot size of the parallel Huffman decode,
 * default 384), "entropy_threads" (256/512/1024; default 512 with one lane,
 * 256 with more), "warmup_slots" (0-64: slots a Huffman run decodes from a
 * guessed state before its own first slot; default 6 with 256 threads, 12
 * with more), "lanes" (1-8 concurrent pipelines, 0 = automatic: 4, or the
 * hardware queues when fewer; with N > 1, successive
 * batches rotate over N device workspaces and run on the context's own N
 * streams, each ordered after the caller's stream at submission; completion
 * is then observed through the ticket -- spdl_hj_wait / spdl_hj_stream_wait
 * -- not by the caller's stream; each lane wants a hardware queue of its own,
 * so the value is clamped to "hw_queues"; a lane's stream is created when
 * first enabled), "lane_priority" (stream priority of the lanes: 1 = low,
 * the default, 0 = normal, -1 = high; HIP keeps up to "hw_queues" hardware
 * queues per priority, so low-priority lanes get queues of their own beside
 * the normal-priority null / torch streams; changing it re-creates the lane
 * streams after their work), "hw_queues" (hardware queues per priority pool:
 * read from GPU_MAX_HW_QUEUES at spdl_hj_create, default 4; set it when HIP
 * initialised with another value), "output_path" (0 = by
 * batch, 1 = the generic swscale kernel, 2 = separate IDCT + unscaled
 * converter at full resolution: byte-identical outputs, for A/B and tests),
 * "entropy_piece_bytes" (size-adaptive Huffman decode: a file larger than
 * this is decoded by ceil(size / value) workgroups, at most 64; default
 * 131072, 0 = one workgroup per image; since ABI 5 round 5), "sws_prepass"
 * (-1 = automatic: the horizontal scaling pass of a downscale by >= 4x or
 * with a > 64-tap filter runs once per source row in its own kernel; 0 =
 * never, 1 = always; byte-identical outputs), "handoff_wait_us" (ABI 6: the
 * bound of a piece hand-off wait, in microseconds of polling with no awaited
 * record arriving -- time while the waves are switched out does not count;
 * default 2000000; 0 gives up at once, which only tests use: every image
 * whose pieces would have waited is re-decoded in one workgroup).
 * "chain_after" (ABI 6: entropy sync rounds after which runs still out of
 * step with their left neighbour are re-decoded chain by chain by whole
 * waves; default -1 = 1 with 512+ entropy threads, 2 with fewer; 0 =
 * never; byte-identical outputs), "min_run_slots"
 * (ABI 6: the fewest slots an entropy run decodes; default 0 = one run per
 * thread; byte-identical outputs),
 * "profile_stages" (ABI 6: bitmask of the stages, by spdl_hj_stage_name
 * index, whose HIP events are recorded while profiling; default all; stages
 * outside it report -1), "lean_waits" (ABI 6: 1, the default, skips the
 * cross-stream event waits stream order already implies -- a workspace's
 * previous batch on the same stream, a caller stream with nothing pending;
 * 0 = always wait), "xcd_order" (ABI 6: XCD-aware tile order, bit 0 the
 * swscale kernel, bit 1 the IDCT kernel; default 1; byte-identical outputs).
 * A/B knobs, byte-identical outputs: "entropy_prio" (0-3, s_setprio of the
 * entropy waves; default 0), "parse_threads" (64/128/256; default 64),
 * "sws_cols" (16-256 output columns per swscale workgroup; default 256),
 * "entropy_lds_pad" (extra LDS bytes per entropy workgroup; default 0),
 * "ms_skip_empty" (1: skip the multi-scan launch of a batch known to hold
 * no multi-scan image; default 0), "host_staging" (1, the default: kernels
 * move descriptors / statuses through mapped pinned memory; 0: DMA copies).
 * Read-only (spdl_hj_get_param): "handoff_retries", images re-decoded after a
 * hand-off gave up, since the context was created; "streams", the HIP
 * streams a batch holding a progressive image may use (one per lane, a
 * multi-scan side stream per lane when the hardware queues allow, the copy
 * stream); "idct_workgroups" (with the source crop), the IDCT workgroups the last submission
 * launched (0 when the fused full-resolution kernel ran instead): a source
 * crop's region-only IDCT shows here; "entropy_workgroups" (with views), the
 * entropy work items of the last submission (one per image, or per piece of
 * a multi-piece image): with "idct_workgroups" it shows that a views
 * submission ran the front end once per image; "fused_workgroups" and
 * "generic_workgroups" (with ragged batches), the workgroups of the fused
 * full-resolution kernel and of the generic output kernel in the last ragged
 * submission, which chooses between them per image (0 and 0 after a plain
 * submission); "lowres_images" and "planes_bytes" (with the reduced-size
 * decode), the images of the last submission with a level above 0 and the
 * bytes of the component planes it laid out in the workspace;
 * "turbo_workgroups" (with the Pillow-exact decode), the workgroups of
 * turbo_rgb_kernel in the last submission.
 * Builds with -DHJ_ABLATIONS=1 also take "debug_mask" (timing ablations that
 * skip kernel phases; outputs wrong); release builds reject it. */
int spdl_hj_set_param(spdl_hj_ctx* ctx, const char* name, int64_t value);

/* Value in effect of a knob above (ABI 3), or of "copy_threads" (host
 * threads packing pinned staging) / "device". */
int spdl_hj_get_param(spdl_hj_ctx* ctx, const char* name, int64_t* value);

#ifdef __cplusplus
}
#endif
#endif
