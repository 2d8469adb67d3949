// hj_host.cpp -- host driver behind include/spdl_hipjpeg.h.
//
// Replaces src/libspdl/cuda/nvjpeg/decoding.cpp (decode_image_nvjpeg single
// :157-202 and batch :204-255) and src/libspdl/cuda/npp/detail/resize.cpp.
// Differences by design: the whole batch goes through one kernel
// sequence instead of a per-image nvjpegDecode + 3x nppiResize loop; the
// header probe replaces nvjpegGetImageInfo; bytes travel to HBM in one
// hipMemcpyAsync from pinned staging.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/spdl_hipjpeg.h"
#include "hj_common.h"
#include "hj_launch.h"
#include "hj_layout.h"
#include "hj_pack.h"
#include "hj_probe.h"
#include "hj_sws.h"
#include "hj_tar.h"
#include "hj_views.h"

using namespace hj;

namespace {

constexpr int kStages = 8;
const char* kStageNames[kStages] = {"h2d",  "parse",  "destuff", "entropy",
                                    "idct", "tables", "output",  "d2h_status"};

void set_err(char* err, size_t errlen, const char* fmt, ...) {
  if (!err || !errlen) return;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err, errlen, fmt, ap);
  va_end(ap);
}

// The batch's layout (hj_layout.h) with the entry points' error convention:
// the text into err, the failing image's status into status[]
int plan_batch(const LayoutRequest& rq, Layout& L, int32_t* status, char* err, size_t errlen) {
  const LayoutResult r = build_layout(rq, L);
  if (r.rc) {
    if (status && r.image >= 0) status[r.image] = r.rc;
    set_err(err, errlen, "%s", r.err);
  }
  return r.rc;
}

// A grow-only device buffer.  Given a stream, a growth is stream-ordered
// (hipFreeAsync / hipMallocAsync on it, after the work it already holds):
// hipFree synchronises the whole device, so a workspace that grew while a
// trainer's kernels ran on another stream used to wait for all of them (a
// decode beside a 0.46 s GEMM loop took 0.46 s; tests/test_gpu_pieces.py).
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t n, hipStream_t st = nullptr, bool async = false) {
    if (n <= cap) return hipSuccess;
    if (p) (void)(async ? hipFreeAsync(p, st) : hipFree(p));
    p = nullptr;
    cap = 0;
    size_t want = n + n / 4 + 4096;
    hipError_t e = async ? hipMallocAsync(&p, want, st) : hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// A grow-only pinned host buffer.  hipHostFree synchronises the whole
// device, so a buffer outgrown while the context runs is not freed then --
// that stalled a decode behind a trainer's kernels on another stream
// (tests/test_gpu_pieces.py: a 0.48 s GEMM loop) -- but kept until release();
// growth doubles, so the kept ones total less than the live buffer.
struct PinBuf {
  void* p = nullptr;
  void* dev = nullptr;  // the same pages as the device sees them (kernels read / write them)
  size_t cap = 0;
  std::vector<void*> old;  // outgrown buffers, freed by release()
  hipError_t ensure(size_t n) {
    if (n <= cap) return hipSuccess;
    if (p) old.push_back(p);
    p = dev = nullptr;
    const size_t want = std::max(2 * cap, n + n / 4 + 4096);
    cap = 0;
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    e = hipHostGetDevicePointer(&dev, p, 0);
    if (e != hipSuccess) {
      (void)hipHostFree(p);
      p = dev = nullptr;
      return e;
    }
    cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    for (void* q : old) (void)hipHostFree(q);
    old.clear();
    p = nullptr;
    dev = nullptr;
    cap = 0;
  }
};

}  // namespace

// One in-flight batch: pinned staging + device copy of the JPEG bytes, the
// descriptor/status staging, and the events that say when each may be reused.
// kSlots of them form the ring that lets batch k+1 be packed on the host and
// copied (on the context's copy stream) while batch k's kernels run.
constexpr int kSlots = 10;

struct Slot {
  PinBuf pin_in, pin_desc, pin_status, pin_tables;
  DevBuf bytes;
  hipEvent_t h2d_done = nullptr;  // bytes are in HBM
  hipEvent_t done = nullptr;      // the batch's last kernel / status copy finished
  int64_t ticket = 0;             // ticket of the batch occupying the slot (0 = none)
  bool pending = false;           // submitted, not yet waited
  bool staged = false;            // acquired by spdl_hj_staging_acquire, not submitted
  bool profiled = false;          // ev[] were recorded for this batch
  uint32_t profiled_stages = 0;   // ... for these stages
  hipEvent_t submitted = nullptr; // lanes > 1: the caller's stream reached the submit
  int n = 0;
  hipEvent_t ev[kStages + 1] = {};  // stage boundaries (profiling only)
  // A batch with multi-piece images: what re-decoding one of them in one
  // workgroup needs, should a piece hand-off give up (kErrHandoff)
  struct Retry {
    int64_t ticket = 0;              // the batch's (its lane's workspace)
    const uint8_t* bytes = nullptr;  // the batch's bytes in HBM
    size_t len = 0;
    spdl_hj_output out{};
    uint8_t* out_dev = nullptr;
    struct Item {  // one multi-piece image of the batch
      int idx;
      // its place in the batch's output: idx x the one size of a plain batch,
      // its own offset and extent in a ragged one (bytes)
      size_t out_off, out_bytes;
      int64_t off, size;
      spdl_hj_image_info info;
      spdl_hj_rect rect;  // its source crop (has_rects)
      uint8_t flip;       // its output flip or orientation code (has_flips)
      uint8_t lowres;     // its reduced-size level
    };
    std::vector<Item> items;
    bool has_rects = false, has_flips = false;  // the batch had crops / flips
    bool oriented = false;  // ... the flips came as orientation codes (spdl_hj_set_orients)
  } retry;
};

// Device workspace of one pipeline "lane".  With lanes > 1 successive
// batches alternate between workspaces and run on the lanes' own streams, so
// batch k+1's kernels can occupy the CUs that batch k's latency-bound
// entropy kernel leaves idle (its sync rounds park most waves at barriers).
constexpr int kMaxLanes = 8;

struct Workspace {
  DevBuf clean, segs, desc, info, luts, ents, bdesc, planes, wts, recs, dschunks;
  DevBuf chain;  // entropy ticket counter + piece hand-off records (hj_common.h)
  DevBuf maps;   // flat-grid dispatch maps: destuff chunks, IDCT tiles, hscale rows -> image
  DevBuf hbuf;   // hscale_kernel's horizontal-pass rows (large downscales)
  hipEvent_t done = nullptr;      // the workspace is free after this
  hipStream_t stream = nullptr;   // lanes > 1 only
  // multiscan_kernel beside the baseline stages (batches with a progressive
  // image, host-bytes entry points): created on first use
  hipStream_t side = nullptr;
  hipEvent_t ev_parsed = nullptr, ev_ms = nullptr;
  hipStream_t last_st = nullptr;  // the stream the workspace's last batch ran on
  bool used = false;
};

struct spdl_hj_ctx {
  int device = 0;
  Workspace ws[kMaxLanes];
  int lanes = 1;
  // the ring, and a spare slot outside it for the one-workgroup re-decode of
  // an image whose piece hand-off gave up (it must not take a ring slot a
  // caller's un-waited ticket may still hold)
  Slot slots[kSlots + 1];
  int64_t next_ticket = 1;
  int64_t last_ticket = 0;
  int lanes_ready = 0;                // workspaces [0, lanes_ready) have their event / stream
  hipStream_t copy = nullptr;         // H2D stream of the staging ring
  CopyPool* pool = nullptr;           // created on the first large host copy
  // hardware queues HIP gives this process (GPU_MAX_HW_QUEUES when HIP
  // initialised; 4 is HIP's default): each lane's stream wants one of its own
  int hw_queues = 4;
  // stream priority of the lanes' streams: 1 low (default), 0 normal, -1
  // high.  HIP keeps a pool of up to GPU_MAX_HW_QUEUES hardware queues per
  // priority, so low-priority lanes get queues of their own beside the
  // normal-priority pool that the null stream, torch's streams and the copy
  // stream share (measured with 4 queues, 4 lanes: 408k img/s at normal
  // priority -- the lanes landed on two queues -- 508k at low, as with 16).
  // Multiscan side streams are high priority (a third pool): they carry the
  // mixed batch's critical path.
  int lane_priority = 1;
  // output kernels: 0 = by batch (fused IDCT + converter at full resolution
  // when possible), 1 = the generic swscale kernel, 2 = separate IDCT +
  // unscaled converter -- byte-identical outputs (tests compare them)
  int output_path = 0;
  bool profiling = false;
  // stages whose HIP events are recorded while profiling (bit i: stage i of
  // kStageNames; a bench brackets only its dominant kernel in the timed steps)
  uint32_t profile_stages = (1u << kStages) - 1u;
  float timings[kStages] = {};
  int ntimings = 0;
  int sub_bits = 384;
  int debug_mask = 0;  // timing ablations, settable only in HJ_ABLATIONS builds
  // the first kernel pulls descriptors + tables from pinned memory and the
  // last writes statuses back (1), or DMA copies do it (0; kept for A/B)
  int host_staging = 1;
  // Huffman workgroup size; 0 = by schedule: 512 with one lane (shortest
  // kernel), 256 with two or more (the smaller workgroups leave the other
  // lane's kernels more room: +3 % in the 2-lane bench, r02 A/B)
  int entropy_threads = 0;
  // entropy round 0: slots decoded before a run's first slot; -1 = by
  // workgroup size: 12 with 512+ threads, 6 with 256 (each run then spans
  // twice the slots; 4-lane A/B: 459-461k vs 450-454k img/s, r02_v5)
  int warm_slots = -1;
  // entropy piece size: a file larger than this is decoded by several
  // workgroups (hj_common.h kMaxPieces); 0 = one workgroup per image
  int64_t piece_bytes = 128 * 1024;
  // entropy runs hold at least this many slots (0: one run per thread)
  int min_run_slots = 0;
  // entropy sync rounds after which unresolved chains are re-decoded by
  // whole waves (chain rounds; 0 = never; -1 = by workgroup size: 1 with
  // 512+ threads, 2 with 256).  r06: the mixed set's slowest image (q94,
  // optimised tables, 11 sync rounds) 1.02 -> 0.63 ms alone, one-lane mixed
  // entropy 0.90 -> 0.69 ms; at one lane 1 also takes the uniform batch's
  // entropy 0.450 -> 0.434 ms (318 k -> 325 k img/s); at four lanes 2 and 1
  // measure the same (profiles/r06/ab/warm_chain.txt)
  int chain_after = -1;
  // s_setprio of the entropy waves (0-3; A/B knob)
  int entropy_prio = 0;
  // parse_kernel workgroup size (its marker walk is one thread's)
  int parse_threads = 64;  // (r05 A/B: 64 +1 % over 256 at four lanes)
  int entropy_lds_pad = 0;  // extra (unused) dynamic LDS per entropy workgroup: CU packing
  PlanCache plans;          // swscale plans per distinct geometry
  // skip the event waits that stream order already implies: the workspace's
  // previous batch on the same stream, and a caller stream with nothing
  // pending (r06 A/B, profiles/r06/ab/lean_waits.txt: +0.5-1 %)
  int lean_waits = 1;
  // skip the multi-scan launch of a batch known to hold no multi-scan image
  // (A/B knob; r05: 1 % slower, the empty launch staggered the lanes)
  int ms_skip_empty = 0;
  // XCD-aware tile order (bit 0 sws_kernel, bit 1 idct_kernel): each XCD
  // takes a contiguous range of tiles, so neighbouring bands of an image
  // share their overlapping source rows in one L2 (r06 A/B: mixed 4 lanes
  // +1.4 %, uniform unchanged)
  int xcd_order = 1;
  // piece hand-off wait bound (us of polling with nothing arriving), and the
  // images re-decoded in one workgroup after a wait gave up
  int64_t handoff_wait_us = 2000000;
  int64_t handoff_retries = 0;
  // spdl_hj_set_crops: the source crops of the next batch submission
  std::vector<spdl_hj_rect> crops;
  // spdl_hj_set_flips: the output flips of the next batch submission
  std::vector<uint8_t> flips;
  // spdl_hj_set_orients: its orientation codes (both set: the planner refuses)
  std::vector<uint8_t> orients;
  // spdl_hj_set_lowres: its reduced-size levels, and the images with one
  // above 0 in the last submission
  std::vector<uint8_t> lowres;
  int64_t lowres_images = 0;
  int64_t planes_bytes = 0;  // the planes the last submission laid out in the workspace
  int64_t idct_workgroups = 0;  // IDCT workgroups the last submission launched
  int64_t entropy_workgroups = 0;  // ... and its entropy work items (images, or their pieces)
  // ... the fused-eligible images' idct_rgb_kernel workgroups, and those of
  // the generic output kernel (sws_kernel)
  int64_t fused_workgroups = 0, generic_workgroups = 0;
  int64_t turbo_workgroups = 0;  // turbo_rgb_kernel's in the last submission (csc = TURBO)
  // spdl_hj_set_views: the views of the next batch submission
  HeldViews views;
  // spdl_hj_set_ragged: the images' byte offsets in the next batch submission's output
  std::vector<int64_t> ragged;
};

namespace {

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// The copy pool is only needed by host-side packing of large batches; the
// device-resident entry points never create it.
CopyPool* copy_pool(spdl_hj_ctx* c) {
  if (!c->pool) c->pool = new CopyPool(copy_workers());  // + the calling thread
  return c->pool;
}

hipError_t create_stream(hipStream_t* s, int priority) {
  int least = 0, greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&least, &greatest);  // (1, -1) on gfx950
  return hipStreamCreateWithPriority(s, hipStreamNonBlocking,
                                     std::max(greatest, std::min(least, priority)));
}

// side streams (multiscan beside the lanes' stages) have queues to spare: the
// high-priority pool holds them alone unless the lanes are high priority too
bool side_streams_fit(const spdl_hj_ctx* c) {
  return (c->lane_priority < 0 ? 2 * c->lanes : c->lanes) <= c->hw_queues;
}

// Workspaces [0, n) get their completion event and (n > 1) their stream.
bool ensure_lanes(spdl_hj_ctx* c, int n) {
  DeviceGuard g(c->device);
  for (int i = c->lanes_ready; i < n; i++) {
    Workspace& w = c->ws[i];
    if (!w.done && hipEventCreateWithFlags(&w.done, hipEventDisableTiming) != hipSuccess) return false;
    if (!w.stream && create_stream(&w.stream, c->lane_priority) != hipSuccess) return false;
    c->lanes_ready = i + 1;
  }
  return true;
}

#define HJ_HIP(expr)                                                                     \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) {                                                              \
      set_err(err, errlen, "HIP error %s at %s:%d (%s)", hipGetErrorString(e_), __FILE__, \
              __LINE__, #expr);                                                          \
      return e_ == hipErrorOutOfMemory ? SPDL_HJ_ERR_OOM : SPDL_HJ_ERR_HIP;             \
    }                                                                                    \
  } while (0)

// stage boundary i: recorded when profiling and a profiled stage starts or
// ends there ("profile_stages": stage i spans ev[i] .. ev[i + 1])
inline void mark(spdl_hj_ctx* c, Slot& s, int i, hipStream_t st) {
  if (c->profiling && ((c->profile_stages | (c->profile_stages << 1)) >> i & 1u))
    (void)hipEventRecord(s.ev[i], st);
}

// Take the next ring slot: its previous batch (if any) must have finished
// before its pinned staging may be rewritten.  An un-waited ticket's
// statuses are dropped here (the ring holds kSlots batches in flight).
int acquire_slot(spdl_hj_ctx* ctx, Slot** out, char* err, size_t errlen) {
  Slot& s = ctx->slots[ctx->next_ticket % kSlots];
  if (s.staged) {
    set_err(err, errlen, "staging slot of ticket %lld was acquired but never submitted",
            (long long)s.ticket);
    return SPDL_HJ_ERR_INVALID_ARG;
  }
  if (s.ticket) HJ_HIP(hipEventSynchronize(s.done));
  s.pending = false;
  s.ticket = ctx->next_ticket++;
  *out = &s;
  return SPDL_HJ_OK;
}

Slot* find_slot(spdl_hj_ctx* ctx, int64_t ticket) {
  if (ticket <= 0) return nullptr;
  Slot& s = ctx->slots[ticket % kSlots];
  return s.ticket == ticket ? &s : nullptr;
}

int retry_image(spdl_hj_ctx* ctx, const Slot::Retry& r, const Slot::Retry::Item& item);

// Per-image statuses of a finished slot -> status[], first error -> err;
// its stage timings -> ctx->timings when it was profiled.
int collect_status(spdl_hj_ctx* ctx, Slot& s, int32_t* status, char* err, size_t errlen) {
  if (s.profiled) {
    ctx->ntimings = kStages;
    for (int i = 0; i < kStages; i++) {
      float ms = -1.f;  // (stages not profiled, or a failed query: -1)
      if (!(s.profiled_stages >> i & 1u) ||
          hipEventElapsedTime(&ms, s.ev[i], s.ev[i + 1]) != hipSuccess)
        ms = -1.f;
      ctx->timings[i] = ms < 0.f ? -1.f : ms * 1000.f;
    }
    s.profiled = false;
  }
  const int32_t* stv = static_cast<const int32_t*>(s.pin_status.p);
  s.pending = false;
  bool handoff = false;
  for (int i = 0; i < s.n && !handoff; i++) handoff = stv[i] == SPDL_HJ_ERR_HANDOFF;
  std::vector<int32_t> fixed;
  if (handoff && !s.retry.items.empty()) {
    // re-decode each image whose hand-off gave up in one workgroup (its
    // output lands where the batch's would have; the spare slot, statuses
    // copied first all the same)
    fixed.assign(stv, stv + s.n);
    Slot::Retry r = std::move(s.retry);
    s.retry = Slot::Retry{};
    for (const Slot::Retry::Item& it : r.items)
      if (fixed[it.idx] == SPDL_HJ_ERR_HANDOFF) fixed[it.idx] = retry_image(ctx, r, it);
    stv = fixed.data();
  }
  const int n = fixed.empty() ? s.n : (int)fixed.size();
  int first_bad = -1;
  for (int i = 0; i < n; i++) {
    if (status) status[i] = stv[i];
    if (stv[i] != SPDL_HJ_OK && first_bad < 0) first_bad = i;
  }
  if (first_bad >= 0) {
    set_err(err, errlen, "Failed to decode an image. (image %d: %s)", first_bad,
            status_str(stv[first_bad]));
    return stv[first_bad];
  }
  return SPDL_HJ_OK;
}

// The entropy launch as the knobs have it, "by schedule" defaults resolved:
// what run_pipeline launches with and spdl_hj_get_param reports as in effect.
EntropyParams entropy_schedule(const spdl_hj_ctx* c, int* threads) {
  const int t = *threads = c->entropy_threads ? c->entropy_threads : (c->lanes > 1 ? 256 : 512);
  EntropyParams ep{};
  ep.sub_bits = c->sub_bits;
  ep.warm_slots = c->warm_slots >= 0 ? c->warm_slots : (t <= 256 ? 6 : 12);
  ep.min_run_slots = c->min_run_slots;
  ep.chain_after = c->chain_after >= 0 ? c->chain_after : (t >= 512 ? 1 : 2);
  ep.prio = c->entropy_prio;
  ep.ablate = c->debug_mask & kAblEntropy;  // the kernel tests the same names
  ep.handoff_ticks = c->handoff_wait_us * 100;
  return ep;
}

// Size the lane's workspace (stream-ordered growth) for the batch of layout L,
// whose files end at max_end of d_bytes; its buffers, typed, for the launchers.
template <class T>
hipError_t grow(DevBuf& d, size_t bytes, hipStream_t st, T** p) {
  const hipError_t e = d.ensure(bytes, st, true);
  *p = static_cast<T*>(d.p);
  return e;
}
int workspace_buffers(Workspace& W, const Layout& L, int n, const uint8_t* d_bytes,
                      int64_t max_end, hipStream_t st, BatchBuffers* b, char* err, size_t errlen) {
  b->bytes = d_bytes;
  b->n = n;
  b->ndesc = (int)L.desc.size();  // (+ the view descriptors of a views submission)
  b->nwork = (int)L.work.size();
  HJ_HIP(grow(W.clean, (size_t)max_end + 512, st, &b->clean));
  HJ_HIP(grow(W.segs, (size_t)L.total_segs * 4 + 64, st, &b->segs));
  HJ_HIP(grow(W.dschunks, (size_t)L.total_ds * sizeof(DsChunk) + 64, st, &b->dschunks));
  // (the work list follows the descriptors, a flipped submission's flags the work list)
  HJ_HIP(grow(W.desc,
              sizeof(ImageDesc) * b->ndesc + sizeof(uint32_t) * b->nwork + L.flips.size() +
                  L.lowres.size(),
              st, &b->desc));
  b->work = reinterpret_cast<uint32_t*>(b->desc + b->ndesc);
  b->flips = L.flips.empty() ? nullptr : reinterpret_cast<const uint8_t*>(b->work + b->nwork);
  b->transposed = L.transposed;
  // (... and a reduced-size submission's levels the flags)
  b->lowres = L.lowres.empty()
                  ? nullptr
                  : reinterpret_cast<const uint8_t*>(b->work + b->nwork) + L.flips.size();
  HJ_HIP(grow(W.chain, (size_t)(kChainHead + L.chain_granules) * 8 + 64, st, &b->chain));
  HJ_HIP(grow(W.maps, (size_t)(L.ds_wgs + L.idct_wgs + L.hs_wgs + L.sws_wgs) * 4 + 64, st,
              &b->ds_map));
  b->idct_map = b->ds_map + L.ds_wgs;
  b->hs_map = b->idct_map + L.idct_wgs;
  b->sws_map = b->hs_map + L.hs_wgs;
  HJ_HIP(grow(W.hbuf, (size_t)L.total_hbuf * 2 + 64, st, &b->hbuf));
  HJ_HIP(grow(W.info, sizeof(ImageInfo) * n, st, &b->infos));
  HJ_HIP(grow(W.luts, sizeof(HuffTable) * 8 * n, st, &b->luts));
  HJ_HIP(grow(W.ents, (size_t)L.total_blocks * 256 + 256, st, &b->ents));
  HJ_HIP(grow(W.bdesc, (size_t)L.total_blocks * 8 + 64, st, &b->bdesc));
  HJ_HIP(grow(W.planes, (size_t)L.total_planes + 256, st, &b->planes));
  HJ_HIP(grow(W.recs, (size_t)L.total_recs * 4 + 256, st, &b->recs));
  HJ_HIP(grow(W.wts, L.tables.size() * 4 + 256, st, &b->wts));
  return SPDL_HJ_OK;
}

// What a batch runs with besides its layout: its n images' bytes in HBM, the
// output and the execution stream (exec_stream()).
struct Submission {
  const uint8_t* d_bytes;
  size_t bytes_len;
  int n;
  const spdl_hj_output* out;
  void* out_dev;
  size_t out_bytes;
  hipStream_t st;
  int sync;
  int32_t* status;
  bool planes_only = false;             // stop at the planes (no output stage)
  const spdl_hj_rect* crops = nullptr;  // the batch's source crops, for the retry record
  const uint8_t* flips = nullptr;       // ... and its output flips (one per image)
  bool oriented = false;                // (they are orientation codes)
  const int64_t* ragged = nullptr;      // a ragged submission's byte offsets (the planner checked them)
};

// An output chain's share of the output kernels' parameters: the batch's
// spec and size, or a view group's
void set_chain(BatchParams& p, const spdl_hj_output& o, int w, int h) {
  p.pix_fmt = o.pix_fmt;
  p.dtype = o.dtype;
  p.resize = o.resize;
  p.filter = o.filter;
  p.out_w = w;
  p.out_h = h;
  memcpy(p.mean, o.mean, sizeof(p.mean));
  memcpy(p.std, o.std, sizeof(p.std));
}

// device pipeline over bytes already in HBM; `slot` provides the descriptor
// and status staging and is marked done on the stream at the end; the
// workspace is the slot's lane.
int run_pipeline(spdl_hj_ctx* ctx, Slot& slot, const Layout& L, const Submission& sub, char* err,
                 size_t errlen) {
  const int n = sub.n;
  const spdl_hj_output* const out = sub.out;
  const hipStream_t st = sub.st;
  const size_t esz = out->dtype == SPDL_HJ_DTYPE_U8 ? 1 : 2;
  const bool by_views = !L.groups.empty();  // (build_layout checked every group's buffer)
  if (!sub.planes_only && !by_views && !L.ragged &&
      (size_t)L.out_elems_per_image * n * esz > sub.out_bytes) {
    set_err(err, errlen, "output buffer too small: need %lld bytes, have %zu",
            (long long)(L.out_elems_per_image * n * esz), sub.out_bytes);
    return SPDL_HJ_ERR_INVALID_ARG;
  }
  int64_t max_end = 0;
  for (int i = 0; i < n; i++) {
    if (L.desc[i].in_off % 256) {
      set_err(err, errlen, "image %d offset %lld is not 256-byte aligned", i,
              (long long)L.desc[i].in_off);
      return SPDL_HJ_ERR_INVALID_ARG;
    }
    int64_t e = L.desc[i].in_off + L.desc[i].in_size;
    if (L.desc[i].in_off < 0 || L.desc[i].in_size < 0 || (size_t)e > sub.bytes_len) {
      set_err(err, errlen, "image %d extends past the input buffer", i);
      return SPDL_HJ_ERR_INVALID_ARG;
    }
    if (e > max_end) max_end = e;
  }
  Workspace& W = ctx->ws[slot.ticket % ctx->lanes];
  // the previous batch may still be using the workspace (async call, maybe on
  // another stream; on the same stream, stream order already covers it)
  if (!(ctx->lean_waits && W.used && W.last_st == st)) HJ_HIP(hipStreamWaitEvent(st, W.done, 0));
  W.last_st = st;
  W.used = true;
  BatchBuffers B;
  if (int rc = workspace_buffers(W, L, n, sub.d_bytes, max_end, st, &B, err, errlen)) return rc;
  // A grid is flat (one workgroup per image tile, through the map) when the
  // (max tiles) x images grid would be mostly empty; a batch of similar
  // images keeps the 2-D grid, whose workgroups need no map lookup
  auto use_flat = [&](int64_t flat_wgs, int64_t max_tiles) {
    return (double)max_tiles * n > 1.25 * (double)flat_wgs;
  };
  const bool ds_flat = use_flat(L.ds_wgs, L.max_chunks);
  // (idct_lowres_kernel has the flat grid alone)
  const bool idct_flat = B.lowres != nullptr ||
                         use_flat(L.idct_wgs, (L.max_blocks + kIdctThreads - 1) / kIdctThreads);
  const bool sws_flat = use_flat(L.sws_wgs, (int64_t)L.sws_bands * L.sws_chunks);
  // + work list, + the flags of a flipped submission (one byte per descriptor)
  const size_t work_end = sizeof(ImageDesc) * B.ndesc + sizeof(uint32_t) * B.nwork;
  const size_t desc_bytes = work_end + L.flips.size() + L.lowres.size();
  HJ_HIP(slot.pin_desc.ensure(desc_bytes));
  HJ_HIP(slot.pin_status.ensure(sizeof(int32_t) * n));
  slot.n = n;
  memcpy(slot.pin_desc.p, L.desc.data(), sizeof(ImageDesc) * B.ndesc);
  memcpy(static_cast<ImageDesc*>(slot.pin_desc.p) + B.ndesc, L.work.data(),
         sizeof(uint32_t) * B.nwork);
  if (B.flips)
    memcpy(static_cast<uint8_t*>(slot.pin_desc.p) + work_end, L.flips.data(), L.flips.size());
  if (B.lowres)
    memcpy(static_cast<uint8_t*>(slot.pin_desc.p) + work_end + L.flips.size(), L.lowres.data(),
           L.lowres.size());
  // the batch's swscale tables travel with the descriptors
  const bool swscale = !sub.planes_only && out->csc == SPDL_HJ_CSC_SWSCALE;
  const size_t tb = swscale ? L.tables.size() * 4 : 0;
  HJ_HIP(slot.pin_tables.ensure(tb + 16));
  if (tb) memcpy(slot.pin_tables.p, L.tables.data(), tb);
  const bool hs = ctx->host_staging != 0;  // parse_kernel pulls them from the pinned pages
  if (!hs) {
    HJ_HIP(hipMemcpyAsync(B.desc, slot.pin_desc.p, desc_bytes, hipMemcpyHostToDevice, st));
    if (tb) HJ_HIP(hipMemcpyAsync(B.wts, slot.pin_tables.p, tb, hipMemcpyHostToDevice, st));
  } else if (B.flips || B.lowres) {
    // (parse_kernel brings over the descriptors and the work list alone: the
    // flags and levels behind them take one small copy from the same pinned pages)
    HJ_HIP(hipMemcpyAsync(reinterpret_cast<uint8_t*>(B.work + B.nwork),
                          static_cast<const uint8_t*>(slot.pin_desc.p) + work_end,
                          desc_bytes - work_end, hipMemcpyHostToDevice, st));
  }
  mark(ctx, slot, 1, st);
  HJ_HIP(launch_parse(B, hs ? static_cast<const ImageDesc*>(slot.pin_desc.dev) : nullptr,
                      hs ? slot.pin_tables.dev : nullptr, hs ? (int64_t)tb : 0,
                      ctx->parse_threads, st));
  mark(ctx, slot, 2, st);
  const int abl = ctx->debug_mask;  // timing ablations (hj_common.h Ablate)
  const bool ms_side = L.ms_side && !(abl & kAblNoMultiscan) && side_streams_fit(ctx);
  if (ms_side) {
    if (!W.side) HJ_HIP(create_stream(&W.side, -1));
    if (!W.ev_parsed) HJ_HIP(hipEventCreateWithFlags(&W.ev_parsed, hipEventDisableTiming));
    if (!W.ev_ms) HJ_HIP(hipEventCreateWithFlags(&W.ev_ms, hipEventDisableTiming));
    HJ_HIP(hipEventRecord(W.ev_parsed, st));
    HJ_HIP(hipStreamWaitEvent(W.side, W.ev_parsed, 0));
    HJ_HIP(launch_multiscan(B, W.side));
    HJ_HIP(hipEventRecord(W.ev_ms, W.side));
  }
  // If a launch below fails and returns early, the lane's stream still joins
  // the side stream and re-records W.done, so the next batch on this
  // workspace cannot reuse clean / ents / bdesc while multiscan writes them.
  struct SideJoin {
    hipStream_t st = nullptr;
    Workspace* w = nullptr;
    ~SideJoin() {
      if (!w) return;
      (void)hipStreamWaitEvent(st, w->ev_ms, 0);
      (void)hipEventRecord(w->done, st);
    }
  } side_join{st, ms_side ? &W : nullptr};
  HJ_HIP(launch_destuff(B, ds_flat, (int)L.ds_wgs, L.max_chunks, st));
  mark(ctx, slot, 3, st);
  int ent_threads;
  const EntropyParams ep = entropy_schedule(ctx, &ent_threads);
  HJ_HIP(launch_entropy(B, ep, ent_threads, ctx->entropy_lds_pad, st));
  // (the entropy stage ends here: the multiscan launch or the wait for the
  // side stream counts to the IDCT stage)
  mark(ctx, slot, 4, st);
  // progressive / non-interleaved images (the kernels above skipped them)
  if (ms_side) {
    side_join.w = nullptr;
    HJ_HIP(hipStreamWaitEvent(st, W.ev_ms, 0));
  } else if (!(abl & kAblNoMultiscan) && !(ctx->ms_skip_empty && L.ms_known && !L.ms_side))
    HJ_HIP(launch_multiscan(B, st));
  // full resolution u8 through swscale's unscaled converter: IDCT and
  // conversion in one kernel (output_path 1: the generic sws_kernel, 2:
  // separate IDCT + rgb_unscaled_kernel)
  // (csc = TURBO is libjpeg-turbo's default decoder: islow, whatever the spec's idct says)
  const bool turbo = !sub.planes_only && out->csc == SPDL_HJ_CSC_TURBO;
  const int idct_kind = (abl & kAblIdctNone) ? 2 : turbo ? SPDL_HJ_IDCT_ISLOW : out->idct;
  // (the planar output, SPDL_HJ_FMT_YUV, has one kernel of its own)
  const bool yuv = swscale && out->pix_fmt == SPDL_HJ_FMT_YUV;
  const bool fast_rgb = swscale && !yuv && L.all_special && out->dtype == SPDL_HJ_DTYPE_U8 &&
                        ctx->output_path != 1;
  const bool fused = fast_rgb && L.fuse_ok && L.fused_tiles > 0 && ctx->output_path != 2;
  // A ragged submission chose per image (the planner: Layout::ragged): the
  // fused kernel over the first part of the flat sws grid, the generic kernel
  // over the rest, idct_kernel for the latter's images alone.  (The fused
  // grid is flat for a uniform batch as well: measured against the (tile,
  // image) grid there, it costs nothing -- profiles/r18/ragged)
  const int ragged_fused = L.ragged ? (int)L.fused_wgs : 0;
  ctx->idct_workgroups = ctx->fused_workgroups = ctx->generic_workgroups = 0;
  ctx->turbo_workgroups = 0;
  ctx->entropy_workgroups = B.nwork;
  ctx->lowres_images = L.lowres_images;
  ctx->planes_bytes = L.total_planes;
  // (a views submission whose views were all refused has no block to transform)
  if (!(abl & kAblNoIdct) && (L.ragged || !fused) && L.max_blocks > 0) {
    if (B.lowres) HJ_HIP(launch_idct_lowres(B, idct_kind, (int)L.idct_wgs, st));
    else
      HJ_HIP(launch_idct(B, idct_kind, idct_flat, (int)L.idct_wgs, L.max_blocks,
                         (ctx->xcd_order >> 1) & 1, st));
    ctx->idct_workgroups =
        idct_flat ? L.idct_wgs : (int64_t)((L.max_blocks + kIdctThreads - 1) / kIdctThreads) * n;
  }
  // 4-component frames: FFmpeg's K transform on the planes (not on the raw
  // planes surface, which returns the IDCT output as the oracle does)
  if (!sub.planes_only && L.cmyk_px > 0) HJ_HIP(launch_cmyk(B, L.cmyk_px, st));
  mark(ctx, slot, 5, st);
  BatchParams bp{};
  bp.n = n;
  bp.idct = out->idct;
  set_chain(bp, *out, L.ow, L.oh);
  bp.sub_bits = ctx->sub_bits;
  bp.debug_mask = abl;
  bp.xcd_order = ctx->xcd_order;
  bp.csc = sws_csc();
  // the output kernel writes each image's status into the pinned array itself
  // (not with views: their descriptors are no images; the statuses are copied below)
  int32_t* hstat =
      hs && !sub.planes_only && !by_views ? static_cast<int32_t*>(slot.pin_status.dev) : nullptr;
  mark(ctx, slot, 6, st);
  if (!sub.planes_only && !(abl & kAblNoOutput)) {
    const int sws_wgs = (int)L.sws_wgs, hs_wgs = (int)L.hs_wgs;
    if (turbo) {
      // one flat launch over every image's own tiles, plain and ragged alike
      // (an image's box and offset are its descriptor's).  Every image has at
      // least one tile -- a box is 1 x 1 or larger, a refused image has the one
      // workgroup of refuse() -- so sws_wgs >= n > 0 and tile 0 of each image
      // writes its status into hstat, as in the ragged swscale launch below
      if (sws_wgs > 0) HJ_HIP(launch_turbo_rgb(B, sub.out_dev, bp, sws_wgs, hstat, st));
      ctx->turbo_workgroups = sws_wgs;
    } else if (by_views) {
      // once per group: its chain's parameters, its buffer, its slice of the
      // flat sws grid (hscale_kernel, which takes no parameters of the chain,
      // runs once over every group's pre-pass rows)
      bool first = true;
      for (const Layout::Group& G : L.groups) {
        BatchParams gp = bp;
        set_chain(gp, G.out, G.ow, G.oh);
        HJ_HIP(launch_sws(B, G.out_dev, gp, true, G.sws_wgs, 1, 1, G.sws_lds,
                          first ? hs_wgs : 0, nullptr, st, G.sws_wg0));
        first = false;
      }
    } else if (L.ragged) {
      // (each image has one writer of its status: tile 0 of its own kernel)
      if (ragged_fused)
        HJ_HIP(launch_idct_rgb_flat(B, sub.out_dev, bp, idct_kind, ragged_fused, hstat, st));
      if (sws_wgs > ragged_fused)
        HJ_HIP(launch_sws(B, sub.out_dev, bp, true, sws_wgs - ragged_fused, 1, 1, L.sws_lds, hs_wgs,
                          hstat, st, ragged_fused));
      ctx->fused_workgroups = ragged_fused;
      ctx->generic_workgroups = sws_wgs - ragged_fused;
    } else if (yuv)
      HJ_HIP(launch_yuv_planes(B, sub.out_dev, sws_wgs, L.sws_lds, hs_wgs, hstat, st));
    else if (fused)
      HJ_HIP(launch_idct_rgb(B, sub.out_dev, bp, idct_kind, L.fused_tiles, hstat, st));
    else if (fast_rgb)  // swscale's unscaled converter needs no scaling passes
      HJ_HIP(launch_rgb_unscaled(B, sub.out_dev, bp, L.max_px, hstat, st));
    else if (swscale)
      HJ_HIP(launch_sws(B, sub.out_dev, bp, sws_flat, sws_wgs, L.sws_bands, L.sws_chunks, L.sws_lds,
                        hs_wgs, hstat, st));
    else
      HJ_HIP(launch_csc(B, sub.out_dev, bp, L.max_px, hstat, st));
  }
  mark(ctx, slot, 7, st);
  // per-image status: strided D2H of ImageInfo::status
  if (!hstat)
    HJ_HIP(hipMemcpy2DAsync(slot.pin_status.p, sizeof(int32_t), B.infos, sizeof(ImageInfo),
                            sizeof(int32_t), n, hipMemcpyDeviceToHost, st));
  mark(ctx, slot, 8, st);
  HJ_HIP(hipEventRecord(W.done, st));
  HJ_HIP(hipEventRecord(slot.done, st));
  Slot::Retry& R = slot.retry;
  R.items.clear();
  if (!sub.planes_only) {
    R.has_rects = sub.crops != nullptr;
    R.has_flips = sub.flips != nullptr;
    R.oriented = sub.oriented;
    const size_t img_bytes = (size_t)L.out_elems_per_image * esz;
    for (const auto& m : L.multi) {
      const ImageDesc& d = L.desc[m.first];
      R.items.push_back({m.first, sub.ragged ? (size_t)sub.ragged[m.first] : m.first * img_bytes,
                         sub.ragged ? (size_t)d.ow * d.oh * 3 * esz : img_bytes,
                         d.in_off, d.in_size, m.second,
                         sub.crops ? sub.crops[m.first] : spdl_hj_rect{},
                         sub.flips ? sub.flips[m.first] : (uint8_t)0,
                         L.lowres.empty() ? (uint8_t)0 : L.lowres[m.first]});
    }
    R.ticket = slot.ticket;
    R.bytes = sub.d_bytes;
    R.len = sub.bytes_len;
    R.out = *out;
    R.out_dev = static_cast<uint8_t*>(sub.out_dev);
  }
  slot.pending = true;
  slot.profiled = ctx->profiling;
  slot.profiled_stages = ctx->profile_stages;
  ctx->last_ticket = slot.ticket;
  if (!sub.sync) return SPDL_HJ_OK;
  HJ_HIP(hipEventSynchronize(slot.done));
  const int rc = collect_status(ctx, slot, sub.status, err, errlen);
  if (!rc && L.view_refused) {  // as a refused image fails a synchronous crop submission
    set_err(err, errlen, "Failed to decode an image. (group %d, view %d: %s)",
            L.view_refused_group, L.view_refused_index, status_str(L.view_refused));
    return L.view_refused;
  }
  return rc;
}

// Stream the batch of `slot` executes on: the caller's stream with one lane;
// otherwise its lane's own stream, ordered after everything the caller's
// stream has queued so far (its output allocation, say).  Completion is then
// observed through the ticket (spdl_hj_wait / spdl_hj_stream_wait), not by
// the caller's stream.
int exec_stream(spdl_hj_ctx* ctx, Slot& slot, hipStream_t st, hipStream_t* xs, char* err,
                size_t errlen) {
  if (ctx->lanes <= 1) {
    *xs = st;
    return SPDL_HJ_OK;
  }
  Workspace& W = ctx->ws[slot.ticket % ctx->lanes];
  // (a caller stream with nothing pending orders nothing: no cross-queue wait.
  // Not asked of the null / per-thread default streams: a query of the
  // legacy null stream waits for the device's other blocking streams -- a
  // test with a GEMM loop on a torch side stream saw every decode wait for it)
  const bool special = st == nullptr || st == hipStreamPerThread;
  if (!(ctx->lean_waits && !special && hipStreamQuery(st) == hipSuccess)) {
    HJ_HIP(hipEventRecord(slot.submitted, st));
    HJ_HIP(hipStreamWaitEvent(W.stream, slot.submitted, 0));
  }
  *xs = W.stream;
  return SPDL_HJ_OK;
}

// One image of a finished batch again, as a one-image batch decoded by
// one entropy workgroup (no piece hand-off), synchronously, into its place in
// the batch's output.  Returns its status.
int retry_image(spdl_hj_ctx* ctx, const Slot::Retry& r, const Slot::Retry::Item& item) {
  char err[256];
  const size_t errlen = sizeof(err);
  Layout L;
  int32_t st1 = SPDL_HJ_OK;
  LayoutRequest rq{&item.off, &item.size, &item.info, 1, &r.out, 0, &ctx->plans};
  rq.crops = r.has_rects ? &item.rect : nullptr;
  if (r.has_flips && r.oriented) {
    rq.orients = &item.flip;
    rq.norients = 1;
  } else if (r.has_flips) {
    rq.flips = &item.flip;
    rq.nflips = 1;
  }
  if (item.lowres) {
    rq.lowres = &item.lowres;
    rq.nlowres = 1;
  }
  int rc = plan_batch(rq, L, &st1, err, errlen);
  if (rc) return rc;
  // the spare slot, on the failed batch's lane (its workspace is free: the
  // batch has finished); the caller's last ticket is left as it was
  Slot* s = &ctx->slots[kSlots];
  if (s->ticket && hipEventSynchronize(s->done) != hipSuccess) return SPDL_HJ_ERR_HIP;
  s->ticket = r.ticket;
  s->pending = false;
  const int64_t last = ctx->last_ticket;
  hipStream_t xs;
  rc = exec_stream(ctx, *s, nullptr, &xs, err, errlen);
  if (rc) return rc;
  ctx->handoff_retries++;
  const int64_t idct_wgs = ctx->idct_workgroups;  // (the batch's, not this re-decode's)
  const int64_t ent_wgs = ctx->entropy_workgroups;
  const int64_t fused_wgs = ctx->fused_workgroups, generic_wgs = ctx->generic_workgroups;
  const int64_t turbo_wgs = ctx->turbo_workgroups;
  const int64_t lowres_images = ctx->lowres_images, planes_bytes = ctx->planes_bytes;
  rc = run_pipeline(ctx, *s, L,
                    {r.bytes, r.len, 1, &r.out, r.out_dev + item.out_off, item.out_bytes, xs, 1,
                     &st1},
                    err, errlen);
  ctx->idct_workgroups = idct_wgs;
  ctx->entropy_workgroups = ent_wgs;
  ctx->fused_workgroups = fused_wgs;
  ctx->generic_workgroups = generic_wgs;
  ctx->turbo_workgroups = turbo_wgs;
  ctx->lowres_images = lowres_images;
  ctx->planes_bytes = planes_bytes;
  ctx->last_ticket = last;
  return rc ? rc : st1;
}

// H2D of the slot's staged bytes on the copy stream; `st` waits for it.
int stage_h2d(spdl_hj_ctx* ctx, Slot& s, size_t total, hipStream_t st, char* err, size_t errlen) {
  // (created on first use: device-resident batches never take its queue)
  if (!ctx->copy) HJ_HIP(hipStreamCreateWithFlags(&ctx->copy, hipStreamNonBlocking));
  // (the slot's previous batch has finished: acquire_slot waited for it)
  HJ_HIP(s.bytes.ensure(total + 512, ctx->copy, true));
  mark(ctx, s, 0, ctx->copy);
  HJ_HIP(hipMemcpyAsync(s.bytes.p, s.pin_in.p, total, hipMemcpyHostToDevice, ctx->copy));
  HJ_HIP(hipEventRecord(s.h2d_done, ctx->copy));
  HJ_HIP(hipStreamWaitEvent(st, s.h2d_done, 0));
  return SPDL_HJ_OK;
}

// The rectangles spdl_hj_set_crops left for this submission of n images:
// taken whatever becomes of the call.  nullptr in *rects: none.
int take_crops(spdl_hj_ctx* ctx, int n, const spdl_hj_output* out, std::vector<spdl_hj_rect>* held,
               const spdl_hj_rect** rects, char* err, size_t errlen) {
  held->clear();
  held->swap(ctx->crops);
  *rects = nullptr;
  if (held->empty()) return SPDL_HJ_OK;
  if ((int64_t)held->size() != n) {
    set_err(err, errlen, "spdl_hj_set_crops gave %zu rectangles for a batch of %d images",
            held->size(), n);
    return SPDL_HJ_ERR_INVALID_ARG;
  }
  if (out && out->csc != SPDL_HJ_CSC_SWSCALE) {
    set_err(err, errlen, "a source crop needs csc = swscale");
    return SPDL_HJ_ERR_INVALID_ARG;
  }
  *rects = held->data();
  return SPDL_HJ_OK;
}

// The views spdl_hj_set_views left for this submission of n images: taken
// whatever becomes of the call, and held against the contract's limits
// (spdl_hipjpeg.h "views").  *hv stays null when there are none.
int take_views(spdl_hj_ctx* ctx, int n, const spdl_hj_output* out, const void* out_dev,
               size_t out_bytes, bool with_crops, HeldViews* held, const HeldViews** hv, char* err,
               size_t errlen) {
  *held = HeldViews{};
  std::swap(*held, ctx->views);
  *hv = nullptr;
  if (!held->any()) return SPDL_HJ_OK;
  auto bad = [&](const char* what) {
    set_err(err, errlen, "spdl_hj_set_views: %s", what);
    return SPDL_HJ_ERR_INVALID_ARG;
  };
  if (held->bad || held->groups.empty() || (int)held->groups.size() > views::kMaxGroups)
    return bad("1 to 4 groups, each with at least one view");
  if (with_crops) return bad("views and spdl_hj_set_crops on one submission");
  if (!valid_output(out) || out->csc != SPDL_HJ_CSC_SWSCALE)
    return bad("the call's output spec must be valid, with csc = swscale");
  if (out_dev || out_bytes) return bad("the call's out_dev must be NULL and out_bytes 0");
  for (const HeldViews::Group& g : held->groups) {
    if (!valid_output(&g.out) || g.out.pix_fmt == SPDL_HJ_FMT_YUV ||
        g.out.csc != SPDL_HJ_CSC_SWSCALE)
      return bad("a group's output must be RGB / BGR with csc = swscale");
    if (g.out.idct != out->idct) return bad("every group's idct must equal the call's");
    if (!g.out_dev) return bad("a group without an output buffer");
    for (const spdl_hj_view& v : g.views)
      if (v.image < 0 || v.image >= n) return bad("a view's image index lies outside the batch");
  }
  *hv = held;
  return SPDL_HJ_OK;
}

// The prologue of the three batch entry points: the crops and views set for
// this submission come off the context at once, whatever becomes of the call.
struct Held {
  std::vector<spdl_hj_rect> rects;
  HeldViews views;
  std::vector<uint8_t> flipv, orientv, lowresv;
  std::vector<int64_t> raggedv;
  const int64_t* ragged = nullptr;      // null: a plain submission
  const spdl_hj_rect* crops = nullptr;  // null: none
  const HeldViews* hv = nullptr;
  // (their count, values and chain are the planner's to check: build_layout)
  const uint8_t* flips = nullptr;
  int64_t nflips = 0;
  const uint8_t* orients = nullptr;
  int64_t norients = 0;
  const uint8_t* lowres = nullptr;  // reduced-size levels (the planner's to check as well)
  int64_t nlowres = 0;
  int crc = 0, vrc = 0;
  Held(spdl_hj_ctx* ctx, int n, const spdl_hj_output* out, const void* out_dev, size_t out_bytes,
       char* err, size_t errlen) {
    if (!ctx) return;
    flipv.swap(ctx->flips);
    ctx->flips.clear();
    if (!flipv.empty()) {
      flips = flipv.data();
      nflips = (int64_t)flipv.size();
    }
    orientv.swap(ctx->orients);
    ctx->orients.clear();
    if (!orientv.empty()) {
      orients = orientv.data();
      norients = (int64_t)orientv.size();
    }
    lowresv.swap(ctx->lowres);
    ctx->lowres.clear();
    if (!lowresv.empty()) {
      lowres = lowresv.data();
      nlowres = (int64_t)lowresv.size();
    }
    raggedv.swap(ctx->ragged);
    ctx->ragged.clear();
    crc = take_crops(ctx, n, out, &rects, &crops, err, errlen);
    vrc = take_views(ctx, n, out, out_dev, out_bytes, !rects.empty(), &views, &hv, err, errlen);
    if (!raggedv.empty()) ragged = raggedv.data();  // (check() holds its count against n)
  }
  // The submission's first error: the views', then the call's own arguments
  // (args_ok: the entry point's pointers and sizes), then the crops'
  int check(bool args_ok, int n, const spdl_hj_output* out, const void* out_dev, char* err,
            size_t errlen) const {
    if (vrc) return vrc;
    if (!args_ok || n <= 0 || !valid_output(out) || (!out_dev && !hv)) {
      set_err(err, errlen, n <= 0 ? "the batch is empty" : "invalid argument");
      return SPDL_HJ_ERR_INVALID_ARG;
    }
    if (crc) return crc;  // (its text is still in err)
    if (!raggedv.empty() && (int64_t)raggedv.size() != n) {
      set_err(err, errlen, "spdl_hj_set_ragged gave %zu offsets for a batch of %d images",
              raggedv.size(), n);
      return SPDL_HJ_ERR_INVALID_ARG;
    }
    return SPDL_HJ_OK;
  }
};

// An acquired slot is released (ticket 0) if its call ends before
// run_pipeline has taken it: its `done` event is never recorded for the ticket
struct SlotRelease {
  Slot* s = nullptr;
  ~SlotRelease() {
    if (s) s->ticket = 0;
  }
  Slot& pass() {  // (the slot is the pipeline's from here)
    Slot* p = s;
    s = nullptr;
    return *p;
  }
};

// A batch submission, its arguments checked and its bytes located: image i is
// sizes[i] bytes at offsets[i] of `len` bytes that lie in one of three places.
struct Batch {
  const int64_t* offsets;
  const int64_t* sizes;
  int n;
  const spdl_hj_output* out;
  void* out_dev;
  size_t out_bytes;
  hipStream_t st;
  int sync;
  int32_t* status;
  size_t len;        // (an image reaching past it is refused)
  size_t bytes_len;  // what the pipeline may read: len, and the tail slack when staged
  const uint8_t* const* data = nullptr;       // host: image i at data[i] (packed by `fill`)
  const uint8_t* host = nullptr;              // a staged slot's pinned bytes
  const uint8_t* dev = nullptr;               // HBM, probed by the caller:
  const spdl_hj_image_info* infos = nullptr;  // ... its probes
};

// From there to run_pipeline, for the three batch entry points.  Host bytes
// are probed here.  Planning comes before a slot is taken (`slot` holds the
// staged entry point's), so a probe or planning failure takes no ticket;
// `fill(slot)` then completes the slot's pinned staging.
template <class Fill>
int submit(spdl_hj_ctx* ctx, const Held& held, const Batch& b, SlotRelease& slot, Fill fill,
           char* err, size_t errlen) {
  DeviceGuard g(ctx->device);
  std::vector<spdl_hj_image_info> probed;
  const spdl_hj_image_info* infos = b.infos;
  if (!b.dev) {
    probed.resize(b.n);
    infos = probed.data();
    for (int i = 0; i < b.n; i++) {
      int rc = SPDL_HJ_ERR_INVALID_ARG;
      if (b.offsets[i] >= 0 && b.sizes[i] >= 0 && (size_t)(b.offsets[i] + b.sizes[i]) <= b.len)
        rc = probe(b.data ? b.data[i] : b.host + b.offsets[i], (size_t)b.sizes[i], &probed[i]);
      if (b.status) b.status[i] = rc;
      if (rc) {
        set_err(err, errlen, "Failed to decode an image. (image %d: %s)", i, status_str(rc));
        return rc;
      }
    }
  }
  Layout L;
  // (views: one entropy workgroup per image, so no hand-off can give up)
  int rc = plan_batch({b.offsets, b.sizes, infos, b.n, b.out, held.hv ? 0 : ctx->piece_bytes,
                       &ctx->plans, held.crops, held.hv, held.flips, held.nflips, held.orients,
                       held.norients, held.ragged, (int64_t)b.out_bytes, ctx->output_path,
                       held.lowres, held.nlowres},
                      L, b.status, err, errlen);
  if (rc) return rc;
  // the probes (the caller's own with device bytes, ABI 5) say which files
  // take the multi-scan path
  for (int i = 0; i < b.n; i++) L.ms_side = L.ms_side || infos[i].multiscan != 0;
  L.ms_known = true;
  if (!slot.s && (rc = acquire_slot(ctx, &slot.s, err, errlen))) return rc;
  if ((rc = fill(*slot.s))) return rc;
  hipStream_t xs;
  rc = exec_stream(ctx, *slot.s, b.st, &xs, err, errlen);
  if (rc) return rc;
  if (b.dev) mark(ctx, *slot.s, 0, xs);
  else if ((rc = stage_h2d(ctx, *slot.s, b.bytes_len, xs, err, errlen))) return rc;
  const uint8_t* bytes = b.dev ? b.dev : static_cast<const uint8_t*>(slot.s->bytes.p);
  return run_pipeline(ctx, slot.pass(), L,
                      {bytes, b.bytes_len, b.n, b.out, b.out_dev, b.out_bytes, xs, b.sync, b.status,
                       false, held.crops,
                       held.hv ? nullptr : held.orients ? held.orients : held.flips,
                       held.orients != nullptr, held.ragged},
                      err, errlen);
}

// One host image, planes only, synchronous (spdl_hj_decode_planes,
// spdl_hj_debug_entropy): what the caller reads the results with.
struct OneImage {
  Layout L;
  Slot* slot = nullptr;
  hipStream_t xs = nullptr;
  bool ran = false;  // the pipeline was entered: the return code is its own
};

int decode_one(spdl_hj_ctx* ctx, const uint8_t* data, size_t size, const spdl_hj_image_info& info,
               const spdl_hj_output& o, int64_t piece_bytes, hipStream_t st, OneImage* r, char* err,
               size_t errlen, uint8_t lowres = 0) {
  const int64_t off = 0, sz = (int64_t)size, total = round_up(sz + 64, 256);
  r->L = Layout{};
  r->ran = false;
  LayoutRequest rq{&off, &sz, &info, 1, &o, piece_bytes, nullptr};
  if (lowres) {
    rq.lowres = &lowres;
    rq.nlowres = 1;
  }
  int rc = plan_batch(rq, r->L, nullptr, err, errlen);
  if (rc) return rc;
  SlotRelease slot;
  if ((rc = acquire_slot(ctx, &slot.s, err, errlen))) return rc;
  r->slot = slot.s;
  HJ_HIP(slot.s->pin_in.ensure((size_t)total));
  memcpy(slot.s->pin_in.p, data, size);
  memset(static_cast<uint8_t*>(slot.s->pin_in.p) + size, 0, (size_t)(total - sz));
  rc = exec_stream(ctx, *slot.s, st, &r->xs, err, errlen);
  if (!rc) rc = stage_h2d(ctx, *slot.s, (size_t)total, r->xs, err, errlen);
  if (rc) return rc;
  r->ran = true;
  return run_pipeline(ctx, slot.pass(), r->L,
                      {static_cast<const uint8_t*>(r->slot->bytes.p), (size_t)total, 1, &o, nullptr,
                       0, r->xs, 1, nullptr, true},
                      err, errlen);
}

}  // namespace

extern "C" {

int spdl_hj_abi_version(void) { return SPDL_HJ_ABI_VERSION; }

int spdl_hj_get_image_info(const uint8_t* data, size_t size, spdl_hj_image_info* info) {
  if (!info) return SPDL_HJ_ERR_INVALID_ARG;
  return probe(data, size, info);
}

int spdl_hj_output_size(int32_t w, int32_t h, const spdl_hj_output* out, int32_t* out_w,
                        int32_t* out_h) {
  if (!valid_output(out) || !out_w || !out_h) return SPDL_HJ_ERR_INVALID_ARG;
  Geom g;
  int rc = geometry(w, h, out, &g);
  if (rc) return rc;
  *out_w = g.ow;
  *out_h = g.oh;
  return SPDL_HJ_OK;
}

int spdl_hj_crop_rect(const spdl_hj_image_info* info, const spdl_hj_rect* in, spdl_hj_rect* out) {
  if (!info || !in || !out || (info->ncomp != 1 && info->ncomp != 3 && info->ncomp != 4))
    return SPDL_HJ_ERR_INVALID_ARG;
  for (int c = 0; c < info->ncomp; c++)
    if (info->h_samp[c] < 1 || info->h_samp[c] > 4 || info->v_samp[c] < 1 || info->v_samp[c] > 4)
      return SPDL_HJ_ERR_INVALID_ARG;
  return crop_resolve(*info, *in, out);
}

int spdl_hj_set_views(spdl_hj_ctx* ctx, const spdl_hj_view_group* groups, int32_t ngroups) {
  if (!ctx || ngroups < 0) return SPDL_HJ_ERR_INVALID_ARG;
  ctx->views = HeldViews{};
  if (!groups || ngroups == 0) return SPDL_HJ_OK;
  // (a broken limit is the consuming call's to report: spdl_hipjpeg.h)
  ctx->views.bad = ngroups > views::kMaxGroups;
  for (int g = 0; g < ngroups && !ctx->views.bad; g++) {
    const spdl_hj_view_group& in = groups[g];
    if (!in.views || in.nviews < 1) {
      ctx->views.bad = true;
      break;
    }
    ctx->views.groups.push_back({in.out, in.out_dev, in.out_bytes,
                                 std::vector<spdl_hj_view>(in.views, in.views + in.nviews),
                                 in.status});
  }
  return SPDL_HJ_OK;
}

int spdl_hj_set_crops(spdl_hj_ctx* ctx, const spdl_hj_rect* rects, int32_t n) {
  if (!ctx || n < 0) return SPDL_HJ_ERR_INVALID_ARG;
  ctx->crops.clear();
  if (rects && n > 0) ctx->crops.assign(rects, rects + n);
  return SPDL_HJ_OK;
}

int spdl_hj_ragged_layout(const spdl_hj_image_info* infos, int32_t n, const spdl_hj_output* out,
                          const spdl_hj_rect* crops, const uint8_t* orients, int64_t align_bytes,
                          int64_t* offsets, int32_t* ow, int32_t* oh, int32_t* status) {
  return ragged_layout(infos, n, out, crops, orients, align_bytes, offsets, ow, oh, status);
}

int spdl_hj_set_ragged(spdl_hj_ctx* ctx, const int64_t* offsets, int32_t n) {
  if (!ctx || n < 0) return SPDL_HJ_ERR_INVALID_ARG;
  ctx->ragged.clear();
  if (offsets && n > 0) ctx->ragged.assign(offsets, offsets + n);
  return SPDL_HJ_OK;
}

int spdl_hj_set_flips(spdl_hj_ctx* ctx, const uint8_t* flips, int32_t n) {
  if (!ctx || n < 0) return SPDL_HJ_ERR_INVALID_ARG;
  ctx->flips.clear();
  if (flips && n > 0) ctx->flips.assign(flips, flips + n);
  return SPDL_HJ_OK;
}

int spdl_hj_set_lowres(spdl_hj_ctx* ctx, const uint8_t* levels, int32_t n) {
  if (!ctx || n < 0) return SPDL_HJ_ERR_INVALID_ARG;
  ctx->lowres.clear();
  if (levels && n > 0) ctx->lowres.assign(levels, levels + n);
  return SPDL_HJ_OK;
}

int spdl_hj_set_orients(spdl_hj_ctx* ctx, const uint8_t* orients, int32_t n) {
  if (!ctx || n < 0) return SPDL_HJ_ERR_INVALID_ARG;
  ctx->orients.clear();
  if (orients && n > 0) ctx->orients.assign(orients, orients + n);
  return SPDL_HJ_OK;
}

spdl_hj_ctx* spdl_hj_create(int device, char* err, size_t errlen) {
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    set_err(err, errlen, "no HIP device available (%s)", hipGetErrorString(e));
    return nullptr;
  }
  if (device < 0 || device >= count) {
    set_err(err, errlen, "device index %d out of range (%d devices)", device, count);
    return nullptr;
  }
  DeviceGuard g(device);
  auto* c = new spdl_hj_ctx();
  c->device = device;
  if (const char* q = getenv("GPU_MAX_HW_QUEUES")) c->hw_queues = atoi(q) > 0 ? atoi(q) : 4;
  bool ok = ensure_lanes(c, 1);
  for (int i = 0; ok && i <= kSlots; i++)
    ok = hipEventCreateWithFlags(&c->slots[i].h2d_done, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&c->slots[i].done, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&c->slots[i].submitted, hipEventDisableTiming) == hipSuccess;
  for (int i = 0; ok && i <= kSlots; i++)
    for (int k = 0; ok && k <= kStages; k++) ok = hipEventCreate(&c->slots[i].ev[k]) == hipSuccess;
  if (!ok) {
    set_err(err, errlen, "hipEventCreate / hipStreamCreate failed");
    spdl_hj_destroy(c);
    return nullptr;
  }
  return c;
}

void spdl_hj_destroy(spdl_hj_ctx* c) {
  if (!c) return;
  DeviceGuard g(c->device);
  for (Slot& s : c->slots)
    if (s.ticket && s.done) (void)hipEventSynchronize(s.done);
  for (Workspace& w : c->ws) {
    if (w.done) (void)hipEventSynchronize(w.done);
    if (w.stream) (void)hipStreamSynchronize(w.stream);
  }
  if (c->copy) (void)hipStreamSynchronize(c->copy);
  for (Workspace& w : c->ws) {
    DevBuf* bufs[] = {&w.clean, &w.segs, &w.desc, &w.info, &w.luts, &w.ents, &w.bdesc,
                      &w.planes, &w.wts, &w.recs, &w.dschunks};
    for (DevBuf* b : bufs) b->release();
    if (w.done) (void)hipEventDestroy(w.done);
    if (w.stream) (void)hipStreamDestroy(w.stream);
    if (w.ev_parsed) (void)hipEventDestroy(w.ev_parsed);
    if (w.ev_ms) (void)hipEventDestroy(w.ev_ms);
    if (w.side) (void)hipStreamDestroy(w.side);
  }
  for (Slot& s : c->slots) {
    s.bytes.release();
    s.pin_in.release();
    s.pin_desc.release();
    s.pin_status.release();
    s.pin_tables.release();
    if (s.h2d_done) (void)hipEventDestroy(s.h2d_done);
    if (s.done) (void)hipEventDestroy(s.done);
    if (s.submitted) (void)hipEventDestroy(s.submitted);
    for (int k = 0; k <= kStages; k++)
      if (s.ev[k]) (void)hipEventDestroy(s.ev[k]);
  }
  if (c->copy) (void)hipStreamDestroy(c->copy);
  delete c->pool;
  delete c;
}

int spdl_hj_decode_batch(spdl_hj_ctx* ctx, const uint8_t* const* data, const size_t* sizes,
                         int32_t n, const spdl_hj_output* out, void* out_dev, size_t out_bytes,
                         void* stream, int32_t sync, int32_t* status, char* err, size_t errlen) {
  const Held held(ctx, n, out, out_dev, out_bytes, err, errlen);
  if (int rc = held.check(ctx && data && sizes, n, out, out_dev, err, errlen)) return rc;
  // the files, each with 64 bytes of slack, on 256-byte boundaries of the staging
  std::vector<int64_t> offs(n), szs(n);
  std::vector<CopyItem> items(n);
  int64_t total = 0;
  for (int i = 0; i < n; i++) {
    offs[i] = total;
    szs[i] = (int64_t)sizes[i];
    const int64_t padded = round_up((int64_t)sizes[i] + 64, 256);
    items[i] = {total, data[i], (int64_t)sizes[i], padded};
    total += padded;
  }
  Batch b{offs.data(), szs.data(), n, out, out_dev, out_bytes, static_cast<hipStream_t>(stream),
          sync, status, (size_t)total, (size_t)total};
  b.data = data;
  SlotRelease slot;
  return submit(
      ctx, held, b, slot,
      [&](Slot& s) -> int {
        HJ_HIP(s.pin_in.ensure((size_t)total));
        parallel_pack(copy_pool(ctx), static_cast<uint8_t*>(s.pin_in.p), items);
        return SPDL_HJ_OK;
      },
      err, errlen);
}

int spdl_hj_decode_batch_device(spdl_hj_ctx* ctx, const uint8_t* dev_data, size_t dev_bytes,
                                const int64_t* offsets, const int64_t* sizes,
                                const spdl_hj_image_info* infos, int32_t n,
                                const spdl_hj_output* out, void* out_dev, size_t out_bytes,
                                void* stream, int32_t sync, int32_t* status, char* err,
                                size_t errlen) {
  const Held held(ctx, n, out, out_dev, out_bytes, err, errlen);
  if (int rc = held.check(ctx && dev_data && offsets && sizes && infos, n, out, out_dev, err, errlen))
    return rc;
  Batch b{offsets, sizes, n, out, out_dev, out_bytes, static_cast<hipStream_t>(stream), sync,
          status, dev_bytes, dev_bytes};
  b.dev = dev_data;
  b.infos = infos;
  SlotRelease slot;
  return submit(ctx, held, b, slot, [](Slot&) { return 0; }, err, errlen);
}

int64_t spdl_hj_last_ticket(spdl_hj_ctx* ctx) { return ctx ? ctx->last_ticket : 0; }

int spdl_hj_wait(spdl_hj_ctx* ctx, int64_t ticket, int32_t* status, int32_t n, char* err,
                 size_t errlen) {
  if (!ctx) return SPDL_HJ_ERR_INVALID_ARG;
  Slot* s = find_slot(ctx, ticket);
  if (!s || !s->pending) {
    set_err(err, errlen, "unknown, already waited or overwritten ticket %lld", (long long)ticket);
    return SPDL_HJ_ERR_INVALID_ARG;
  }
  if (status && n < s->n) {
    set_err(err, errlen, "status array too small (%d < %d)", n, s->n);
    return SPDL_HJ_ERR_INVALID_ARG;
  }
  DeviceGuard g(ctx->device);
  HJ_HIP(hipEventSynchronize(s->done));
  return collect_status(ctx, *s, status, err, errlen);
}

int spdl_hj_stream_wait(spdl_hj_ctx* ctx, int64_t ticket, void* stream, char* err,
                        size_t errlen) {
  Slot* s = ctx ? find_slot(ctx, ticket) : nullptr;
  if (!s) {
    set_err(err, errlen, "unknown or overwritten ticket %lld", (long long)ticket);
    return SPDL_HJ_ERR_INVALID_ARG;
  }
  DeviceGuard g(ctx->device);
  HJ_HIP(hipStreamWaitEvent(static_cast<hipStream_t>(stream), s->done, 0));
  return SPDL_HJ_OK;
}

int spdl_hj_staging_acquire(spdl_hj_ctx* ctx, size_t bytes, uint8_t** host_ptr, int64_t* ticket,
                            char* err, size_t errlen) {
  if (!ctx || !host_ptr || !ticket) {
    set_err(err, errlen, "invalid argument");
    return SPDL_HJ_ERR_INVALID_ARG;
  }
  DeviceGuard g(ctx->device);
  Slot* s = nullptr;
  int rc = acquire_slot(ctx, &s, err, errlen);
  if (rc) return rc;
  HJ_HIP(s->pin_in.ensure(bytes + 512));
  s->staged = true;
  *host_ptr = static_cast<uint8_t*>(s->pin_in.p);
  *ticket = s->ticket;
  return SPDL_HJ_OK;
}

int spdl_hj_staging_fill(spdl_hj_ctx* ctx, int64_t ticket, size_t dst_off, const uint8_t* src,
                         size_t len, char* err, size_t errlen) {
  Slot* s = ctx ? find_slot(ctx, ticket) : nullptr;
  if (!s || !s->staged || !src || dst_off + len > s->pin_in.cap) {
    set_err(err, errlen, "invalid staging fill (ticket %lld)", (long long)ticket);
    return SPDL_HJ_ERR_INVALID_ARG;
  }
  std::vector<CopyItem> items(1, CopyItem{(int64_t)dst_off, src, (int64_t)len, (int64_t)len});
  parallel_pack(copy_pool(ctx), static_cast<uint8_t*>(s->pin_in.p), items);
  return SPDL_HJ_OK;
}

int spdl_hj_staging_read(spdl_hj_ctx* ctx, int64_t ticket, size_t dst_off, int fd,
                         int64_t file_off, size_t len, char* err, size_t errlen) {
  Slot* s = ctx ? find_slot(ctx, ticket) : nullptr;
  if (!s || !s->staged || fd < 0 || file_off < 0 || dst_off + len > s->pin_in.cap) {
    set_err(err, errlen, "invalid staging read (ticket %lld)", (long long)ticket);
    return SPDL_HJ_ERR_INVALID_ARG;
  }
  // (a small read is one thread's: it does not create the pool)
  if (!parallel_pread(len < (4u << 20) ? nullptr : copy_pool(ctx), fd, file_off,
                      static_cast<uint8_t*>(s->pin_in.p) + dst_off, len)) {
    set_err(err, errlen, "pread failed or hit end of file (offset %lld, %zu bytes)",
            (long long)file_off, len);
    return SPDL_HJ_ERR_INVALID_ARG;
  }
  return SPDL_HJ_OK;
}

int spdl_hj_decode_staged(spdl_hj_ctx* ctx, int64_t ticket, size_t len, const int64_t* offsets,
                          const int64_t* sizes, int32_t n, const spdl_hj_output* out,
                          void* out_dev, size_t out_bytes, void* stream, int32_t sync,
                          int32_t* status, char* err, size_t errlen) {
  const Held held(ctx, n, out, out_dev, out_bytes, err, errlen);
  Slot* s = ctx ? find_slot(ctx, ticket) : nullptr;
  if (!s || !s->staged) {
    set_err(err, errlen, "ticket %lld does not name an acquired staging slot", (long long)ticket);
    return SPDL_HJ_ERR_INVALID_ARG;
  }
  s->staged = false;  // the slot is consumed whatever happens below
  SlotRelease slot{s};
  if (int rc = held.check(offsets && sizes && len + 512 <= s->pin_in.cap, n, out, out_dev, err,
                          errlen))
    return rc;
  Batch b{offsets, sizes, n, out, out_dev, out_bytes, static_cast<hipStream_t>(stream), sync,
          status, len, len + 512};
  b.host = static_cast<const uint8_t*>(s->pin_in.p);
  return submit(
      ctx, held, b, slot,
      [len](Slot& s) {
        memset(static_cast<uint8_t*>(s.pin_in.p) + len, 0, 512);  // tail read slack
        return 0;
      },
      err, errlen);
}

int spdl_hj_tar_index(const uint8_t* data, size_t size, size_t start, int32_t max_entries,
                      int64_t* offsets, int64_t* sizes, int64_t* name_offs, char* names,
                      size_t names_cap, int32_t* n_out, size_t* next_pos) {
  if (!data || !offsets || !sizes || !n_out || !next_pos || max_entries < 0)
    return SPDL_HJ_ERR_INVALID_ARG;
  tar_index(data, size, start, max_entries, offsets, sizes, name_offs, names, names_cap, n_out,
            next_pos);
  return SPDL_HJ_OK;
}

int spdl_hj_decode_planes(spdl_hj_ctx* ctx, const uint8_t* data, size_t size, int32_t idct,
                          uint8_t* const* planes, void* stream, char* err, size_t errlen) {
  if (!ctx || !data || !planes || (idct != 0 && idct != 1)) {
    set_err(err, errlen, "invalid argument");
    return SPDL_HJ_ERR_INVALID_ARG;
  }
  // (a one-element spdl_hj_set_lowres: consumed whatever becomes of the call)
  std::vector<uint8_t> levels;
  levels.swap(ctx->lowres);
  if (levels.size() > 1 || (levels.size() == 1 && levels[0] > 3)) {
    set_err(err, errlen, "spdl_hj_set_lowres: one level, 0 to 3, for spdl_hj_decode_planes");
    return SPDL_HJ_ERR_INVALID_ARG;
  }
  const int lv = levels.empty() ? 0 : levels[0];
  DeviceGuard g(ctx->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  spdl_hj_image_info info;
  int rc = probe(data, size, &info);
  if (rc) {
    set_err(err, errlen, "Failed to decode an image. (%s)", status_str(rc));
    return rc;
  }
  spdl_hj_output o{};
  o.idct = idct;
  OneImage one;
  // (a piece hand-off that gave up: once more in one entropy workgroup)
  for (int64_t piece_bytes : {ctx->piece_bytes, (int64_t)0}) {
    rc = decode_one(ctx, data, size, info, o, piece_bytes, st, &one, err, errlen, (uint8_t)lv);
    if (rc != SPDL_HJ_ERR_HANDOFF || !one.ran || piece_bytes == 0) break;
    ctx->handoff_retries++;
  }
  if (rc) return rc;
  Workspace& W = ctx->ws[one.slot->ticket % ctx->lanes];
  st = one.xs;
  const ImageDesc& d = one.L.desc[0];
  FrameBlocks fb;
  (void)frame_blocks(info, &fb);  // (the layout was built: the frame is supported)
  const int hmax = fb.grid.hmax, vmax = fb.grid.vmax;
  for (int c = 0; c < info.ncomp; c++) {
    // (the reduced frame's component sizes at a level above 0)
    const int fw = lowres_side(info.width, lv), fh = lowres_side(info.height, lv);
    int w = info.ncomp == 1 ? fw : (fw * info.h_samp[c] + hmax - 1) / hmax;
    int h = info.ncomp == 1 ? fh : (fh * info.v_samp[c] + vmax - 1) / vmax;
    HJ_HIP(hipMemcpy2DAsync(planes[c], (size_t)w,
                            static_cast<const uint8_t*>(W.planes.p) + d.plane_off[c],
                            (size_t)d.plane_stride[c], (size_t)w, (size_t)h,
                            hipMemcpyDeviceToHost, st));
  }
  HJ_HIP(hipStreamSynchronize(st));
  return SPDL_HJ_OK;
}

int spdl_hj_debug_entropy(spdl_hj_ctx* ctx, const uint8_t* data, size_t size, int16_t* coefs,
                          size_t coef_cap, uint8_t* clean, size_t clean_cap, int32_t* diag,
                          char* err, size_t errlen) {
  if (!ctx || !data || !diag) {
    set_err(err, errlen, "invalid argument");
    return SPDL_HJ_ERR_INVALID_ARG;
  }
  DeviceGuard g(ctx->device);
  spdl_hj_image_info info;
  int rc = probe(data, size, &info);
  if (rc) {
    set_err(err, errlen, "probe failed (%s)", status_str(rc));
    return rc;
  }
  spdl_hj_output o{};
  OneImage one;
  rc = decode_one(ctx, data, size, info, o, ctx->piece_bytes, nullptr, &one, err, errlen);
  if (rc && !one.ran) return rc;  // (the pipeline's own code is not looked at: diag[0] says)
  const Layout& L = one.L;
  Workspace& W = ctx->ws[one.slot->ticket % ctx->lanes];
  ImageInfo hi;
  HJ_HIP(hipMemcpy(&hi, W.info.p, sizeof(ImageInfo), hipMemcpyDeviceToHost));
  diag[0] = hi.status;
  diag[1] = hi.clean_len;
  diag[2] = hi.nseg;
  diag[3] = hi.sync_rounds;
  for (int i = 0; i < 4; i++) diag[4 + i] = (int32_t)hi.tphase[i];
  for (int i = 0; i < 4; i++) diag[8 + i] = (int32_t)hi.dbg[i];
  for (int i = 0; i < 48; i++) diag[12 + i] = hi.sdiag[i];
  // expand the coefficient lists (see BlockOut in hj_kernels.hip: entries
  // level << 16 | zig-zag index, dequantised as the IDCT does) to the dense
  // natural-order blocks the IDCT consumes
  const size_t nbk = (size_t)L.desc[0].nblocks;
  if (coefs && hi.status == SPDL_HJ_OK) {
    static const uint8_t kNatural[64] = {
        0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    std::vector<uint2> bd(nbk);
    std::vector<uint32_t> ents(nbk * 64);
    HJ_HIP(hipMemcpy(bd.data(), W.bdesc.p, nbk * sizeof(uint2), hipMemcpyDeviceToHost));
    HJ_HIP(hipMemcpy(ents.data(), W.ents.p, nbk * 256, hipMemcpyDeviceToHost));
    std::vector<int16_t> dense(nbk * 64, 0);
    for (size_t j = 0; j < nbk; j++) {
      const int c = hi.mcu_comp[j % (size_t)hi.bpm];
      dense[j * 64] = (int16_t)(bd[j].y >> 16);
      const uint32_t cnt = bd[j].y & 0xFFFFu;
      for (uint32_t i = 0; i < cnt && bd[j].x + i < nbk * 64; i++) {
        const uint32_t e = ents[bd[j].x + i];
        const uint32_t zz = e & 63u;
        dense[j * 64 + kNatural[zz]] = (int16_t)(uint16_t)((e >> 16) * hi.qt[c][zz]);
      }
    }
    memcpy(coefs, dense.data(), 2 * (dense.size() < coef_cap ? dense.size() : coef_cap));
  }
  if (clean && hi.clean_len > 0) {
    size_t n = (size_t)hi.clean_len < clean_cap ? (size_t)hi.clean_len : clean_cap;
    HJ_HIP(hipMemcpy(clean, W.clean.p, n, hipMemcpyDeviceToHost));
  }
  return SPDL_HJ_OK;
}

int spdl_hj_debug_sws_plan(int32_t width, int32_t height, int32_t hsub, int32_t vsub, int32_t mode,
                           int32_t planar, const spdl_hj_output* out, int32_t prepass,
                           int32_t max_cols, int32_t* info, int32_t* vmode, int32_t* const* pos,
                           int16_t* const* coef) {
  if (!out || !info || mode < kPlanYuv || mode > kPlanGbr || (planar && mode == kPlanGbr) ||
      hsub < 0 || hsub > 2 || vsub < 0 || vsub > 2 || prepass < -1 || prepass > 1 ||
      max_cols < 16 || max_cols > kSwsMaxCols)
    return SPDL_HJ_ERR_INVALID_ARG;
  memset(info, 0, sizeof(int32_t) * 40);
  // the key build_layout makes of an image of this size and sampling
  Geom g;
  int rc = planar ? geometry(width, height, out, &g, 1 << hsub, 1 << vsub)
                  : geometry(width, height, out, &g);
  if (rc) return rc;
  const PlanKey key{width, height, hsub, vsub, mode | (planar ? kPlanPlanar : 0),
                    out->resize ? out->filter : 0, g.sw, g.sh, g.dx, g.dy, g.ow, g.oh};
  const int32_t geo[6] = {g.sw, g.sh, g.dx, g.dy, g.ow, g.oh};
  memcpy(info + 5, geo, sizeof(geo));
  auto pp = PlanCache::build(key, &rc, prepass, max_cols);
  if (!pp) return rc;
  const SwsDesc& d = pp->d;
  const int32_t head[5] = {pp->special, d.full, d.gray, d.gbr, d.pre};
  memcpy(info, head, sizeof(head));
  const int32_t taps[4] = {d.hl_taps, d.hc_taps, d.vl_taps, d.vc_taps};
  const int32_t sizes[4] = {d.hl_size, d.hc_size, d.vl_size, d.vc_size};
  memcpy(info + 11, taps, sizeof(taps));
  memcpy(info + 15, sizes, sizeof(sizes));
  memcpy(info + 19, pp->axis_n, sizeof(pp->axis_n));
  const int32_t tile[9] = {d.rb, d.col_chunk, pp->bands, pp->chunks, pp->lds,
                           d.pre_rl, d.pre_rc, d.chr_w, d.chr_h};
  memcpy(info + 23, tile, sizeof(tile));
  // the tables as the device gets them: the blob's sections
  const int32_t* blob = pp->blob.data();
  for (int i = 0; i < 4; i++) {
    if (pos && pos[i]) memcpy(pos[i], blob + d.off[2 * i], sizeof(int32_t) * pp->axis_n[i]);
    if (coef && coef[i])
      memcpy(coef[i], blob + d.off[2 * i + 1], sizeof(int16_t) * (size_t)pp->axis_n[i] * sizes[i]);
  }
  if (vmode && !planar) memcpy(vmode, blob + d.off[kVmode], sizeof(int32_t) * g.sh);
  return SPDL_HJ_OK;
}

int spdl_hj_nv12_to_planar_rgb(const uint8_t* src_dev, int32_t num_frames, int32_t h2,
                               int32_t width, int32_t bgr, int32_t matrix_coeff, uint8_t* dst_dev,
                               size_t dst_bytes, int device, void* stream, int32_t sync, char* err,
                               size_t errlen) {
  if (!src_dev || !dst_dev || num_frames < 0 || width <= 0 || h2 <= 0) {
    set_err(err, errlen, "invalid argument");
    return SPDL_HJ_ERR_INVALID_ARG;
  }
  if (h2 % 3 != 0) {  // reference: src/libspdl/cuda/color_conversion.cpp:45-50
    set_err(err, errlen,
            "The height of NV12 image (h*1.5) must be divisible by 3. Found: %d", (int)h2);
    return SPDL_HJ_ERR_INVALID_ARG;
  }
  const int32_t height = h2 / 3 * 2;
  if ((size_t)num_frames * 3 * height * width > dst_bytes) {
    set_err(err, errlen, "output buffer too small");
    return SPDL_HJ_ERR_INVALID_ARG;
  }
  if (matrix_coeff <= 0 || matrix_coeff > 10) matrix_coeff = 1;  // silently BT.709
  DeviceGuard g(device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  HJ_HIP(launch_nv12(src_dev, dst_dev, num_frames, height, width, bgr != 0, matrix_coeff, st));
  if (sync) HJ_HIP(hipStreamSynchronize(st));
  return SPDL_HJ_OK;
}

int spdl_hj_copy(void* dst, const void* src, size_t bytes, int32_t kind, int device, void* stream,
                 int32_t pinned, char* err, size_t errlen) {
  if ((!dst || !src) && bytes) {
    set_err(err, errlen, "invalid argument");
    return SPDL_HJ_ERR_INVALID_ARG;
  }
  if (kind != 0 && kind != 1) {
    set_err(err, errlen, "invalid copy kind %d", (int)kind);
    return SPDL_HJ_ERR_INVALID_ARG;
  }
  if (!bytes) return SPDL_HJ_OK;
  DeviceGuard g(device);
  const hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
  if (pinned) {  // reference transfer_buffer_impl: async on the stream + sync
    hipStream_t st = static_cast<hipStream_t>(stream);
    HJ_HIP(hipMemcpyAsync(dst, src, bytes, k, st));
    HJ_HIP(hipStreamSynchronize(st));
  } else {
    HJ_HIP(hipMemcpy(dst, src, bytes, k));
  }
  return SPDL_HJ_OK;
}

int spdl_hj_set_profiling(spdl_hj_ctx* ctx, int32_t enable) {
  if (!ctx) return SPDL_HJ_ERR_INVALID_ARG;
  ctx->profiling = enable != 0;
  return SPDL_HJ_OK;
}

int spdl_hj_last_timings(spdl_hj_ctx* ctx, float* us, int32_t cap, int32_t* n_out) {
  if (!ctx || !us || !n_out) return SPDL_HJ_ERR_INVALID_ARG;
  int k = ctx->ntimings < cap ? ctx->ntimings : cap;
  for (int i = 0; i < k; i++) us[i] = ctx->timings[i];
  *n_out = k;
  return SPDL_HJ_OK;
}

const char* spdl_hj_stage_name(int32_t i) {
  return (i >= 0 && i < kStages) ? kStageNames[i] : "";
}

int spdl_hj_set_param(spdl_hj_ctx* ctx, const char* name, int64_t value) {
  if (!ctx || !name) return SPDL_HJ_ERR_INVALID_ARG;
  if (!strcmp(name, "sub_bits")) {
    if (value < 32 || value > (1 << 24) || value % 32) return SPDL_HJ_ERR_INVALID_ARG;
    ctx->sub_bits = (int)value;
    return SPDL_HJ_OK;
  }
  if (!strcmp(name, "entropy_threads")) {  // workgroup size of the Huffman kernel
    if (value != 0 && value != 128 && value != 256 && value != 512 && value != 1024)
      return SPDL_HJ_ERR_INVALID_ARG;
    ctx->entropy_threads = (int)value;
    return SPDL_HJ_OK;
  }
  if (!strcmp(name, "warmup_slots")) {  // entropy round-0 warm-up before each run
    if (value < 0 || value > 64) return SPDL_HJ_ERR_INVALID_ARG;
    ctx->warm_slots = (int)value;
    return SPDL_HJ_OK;
  }
  if (!strcmp(name, "entropy_piece_bytes")) {  // size-adaptive entropy decode; 0 = off
    if (value < 0 || (value > 0 && value < 16 * 1024)) return SPDL_HJ_ERR_INVALID_ARG;
    ctx->piece_bytes = value;
    return SPDL_HJ_OK;
  }
  if (!strcmp(name, "min_run_slots")) {  // entropy: fewest slots per run (0 = off)
    if (value < 0 || value > 64) return SPDL_HJ_ERR_INVALID_ARG;
    ctx->min_run_slots = (int)value;
    return SPDL_HJ_OK;
  }
  if (!strcmp(name, "chain_after")) {  // entropy chain rounds after this many sync rounds
    if (value < -1 || value > 15) return SPDL_HJ_ERR_INVALID_ARG;
    ctx->chain_after = (int)value;
    return SPDL_HJ_OK;
  }
  if (!strcmp(name, "parse_threads")) {
    if (value != 64 && value != 128 && value != 256) return SPDL_HJ_ERR_INVALID_ARG;
    ctx->parse_threads = (int)value;
    return SPDL_HJ_OK;
  }
  if (!strcmp(name, "entropy_prio")) {
    if (value < 0 || value > 3) return SPDL_HJ_ERR_INVALID_ARG;
    ctx->entropy_prio = (int)value;
    return SPDL_HJ_OK;
  }
  if (!strcmp(name, "sws_cols")) {  // widest swscale tile (16-256 columns; A/B knob)
    if (value < 16 || value > kSwsMaxCols) return SPDL_HJ_ERR_INVALID_ARG;
    ctx->plans.set_max_cols((int)value);
    return SPDL_HJ_OK;
  }
  if (!strcmp(name, "sws_prepass")) {  // -1 auto, 0 never, 1 always (identical outputs)
    if (value < -1 || value > 1) return SPDL_HJ_ERR_INVALID_ARG;
    ctx->plans.set_pre_mode((int)value);
    return SPDL_HJ_OK;
  }
  if (!strcmp(name, "entropy_lds_pad")) {  // bytes; > ~26 KB leaves one entropy WG per CU
    if (value < 0 || value > 64 * 1024) return SPDL_HJ_ERR_INVALID_ARG;
    ctx->entropy_lds_pad = (int)value;
    return SPDL_HJ_OK;
  }
  if (!strcmp(name, "lanes")) {  // concurrent pipelines (workspaces + streams)
    if (value < 0 || value > kMaxLanes) return SPDL_HJ_ERR_INVALID_ARG;
    // 0: automatic -- four lanes, fewer only with fewer hardware queues
    // (r04 sweep, 4-lane bench: 3 lanes 447k img/s, 4 479k, 5 431k, 8 471k)
    if (value == 0) value = std::max(1, std::min(4, ctx->hw_queues));
    // lanes beyond the hardware queues of their priority's pool would share
    // queues and serialise: clamp (spdl_hj_get_param reports the lanes in effect)
    const int lanes = std::min((int)value, std::max(1, ctx->hw_queues));
    if (!ensure_lanes(ctx, lanes)) return SPDL_HJ_ERR_HIP;
    ctx->lanes = lanes;
    return SPDL_HJ_OK;
  }
  if (!strcmp(name, "lane_priority")) {  // 1 low (own queue pool), 0 normal, -1 high
    if (value < -1 || value > 1) return SPDL_HJ_ERR_INVALID_ARG;
    if (value == ctx->lane_priority) return SPDL_HJ_OK;
    // the lanes' streams are re-created at the new priority (after their
    // work): every stream is drained first, so a failure leaves all of them
    // in place (none destroyed while lanes_ready still counts it)
    DeviceGuard g(ctx->device);
    for (Workspace& w : ctx->ws)
      if (w.stream && hipStreamSynchronize(w.stream) != hipSuccess) return SPDL_HJ_ERR_HIP;
    for (Workspace& w : ctx->ws)
      if (w.stream) {
        (void)hipStreamDestroy(w.stream);
        w.stream = nullptr;
      }
    ctx->lane_priority = (int)value;
    ctx->lanes_ready = 0;
    return ensure_lanes(ctx, std::max(1, ctx->lanes)) ? SPDL_HJ_OK : SPDL_HJ_ERR_HIP;
  }
  if (!strcmp(name, "hw_queues")) {  // the caller knows HIP initialised with another value
    if (value < 1 || value > 32) return SPDL_HJ_ERR_INVALID_ARG;
    ctx->hw_queues = (int)value;
    if (ctx->lanes > ctx->hw_queues) ctx->lanes = ctx->hw_queues;
    return SPDL_HJ_OK;
  }
  if (!strcmp(name, "output_path")) {  // equivalent output kernels (A/B and tests)
    if (value < 0 || value > 2) return SPDL_HJ_ERR_INVALID_ARG;
    ctx->output_path = (int)value;
    return SPDL_HJ_OK;
  }
  if (!strcmp(name, "ms_skip_empty")) {
    ctx->ms_skip_empty = value != 0;
    return SPDL_HJ_OK;
  }
  if (!strcmp(name, "xcd_order")) {
    if (value < 0 || value > 3) return SPDL_HJ_ERR_INVALID_ARG;
    ctx->xcd_order = (int)value;
    return SPDL_HJ_OK;
  }
  if (!strcmp(name, "lean_waits")) {
    ctx->lean_waits = value != 0;
    return SPDL_HJ_OK;
  }
  if (!strcmp(name, "profile_stages")) {  // bitmask over spdl_hj_stage_name indices
    if (value < 0 || value >= (1 << kStages)) return SPDL_HJ_ERR_INVALID_ARG;
    ctx->profile_stages = (uint32_t)value;
    return SPDL_HJ_OK;
  }
  if (!strcmp(name, "handoff_wait_us")) {  // piece hand-off wait bound (0: give up at once)
    if (value < 0 || value > 60 * 1000 * 1000) return SPDL_HJ_ERR_INVALID_ARG;
    ctx->handoff_wait_us = value;
    return SPDL_HJ_OK;
  }
  if (!strcmp(name, "host_staging")) {  // 1: kernels move descriptors / statuses; 0: DMA copies
    ctx->host_staging = value != 0;
    return SPDL_HJ_OK;
  }
#if HJ_ABLATIONS
  if (!strcmp(name, "debug_mask")) {  // timing ablations only: output is wrong
    ctx->debug_mask = (int)value;
    return SPDL_HJ_OK;
  }
#endif
  return SPDL_HJ_ERR_INVALID_ARG;
}

int spdl_hj_get_param(spdl_hj_ctx* ctx, const char* name, int64_t* value) {
  if (!ctx || !name || !value) return SPDL_HJ_ERR_INVALID_ARG;
  int ent_threads;
  const EntropyParams ep = entropy_schedule(ctx, &ent_threads);
  const struct {
    const char* n;
    int64_t v;
  } tab[] = {
      {"sub_bits", ctx->sub_bits},
      {"entropy_threads", ent_threads},
      {"warmup_slots", ep.warm_slots},
      {"lanes", ctx->lanes},
      {"entropy_piece_bytes", ctx->piece_bytes},
      {"sws_prepass", ctx->plans.pre_mode()},
      {"entropy_prio", ctx->entropy_prio},
      {"min_run_slots", ctx->min_run_slots},
      {"chain_after", ep.chain_after},
      {"parse_threads", ctx->parse_threads},
      {"sws_cols", ctx->plans.max_cols()},
      {"hw_queues", ctx->hw_queues},
      // streams a batch holding a progressive image may use: one per lane, a
      // multiscan side stream per lane when the queues allow it, the copy stream
      {"streams", ctx->lanes * (side_streams_fit(ctx) ? 2 : 1) + 1},
      {"lane_priority", ctx->lane_priority},
      {"output_path", ctx->output_path},
      {"host_staging", ctx->host_staging},
      {"copy_threads", ctx->pool ? ctx->pool->workers() : copy_workers() + 1},
      {"device", ctx->device},
      {"handoff_wait_us", ctx->handoff_wait_us},
      {"profile_stages", ctx->profile_stages},
      {"lean_waits", ctx->lean_waits},
      {"ms_skip_empty", ctx->ms_skip_empty},
      {"xcd_order", ctx->xcd_order},
      {"handoff_retries", ctx->handoff_retries},
      {"idct_workgroups", ctx->idct_workgroups},
      {"lowres_images", ctx->lowres_images},
      {"planes_bytes", ctx->planes_bytes},
      {"fused_workgroups", ctx->fused_workgroups},
      {"generic_workgroups", ctx->generic_workgroups},
      {"turbo_workgroups", ctx->turbo_workgroups},
      {"entropy_workgroups", ctx->entropy_workgroups},
  };
  for (const auto& t : tab)
    if (!strcmp(name, t.n)) {
      *value = t.v;
      return SPDL_HJ_OK;
    }
  return SPDL_HJ_ERR_INVALID_ARG;
}

}  // extern "C"
