// hj_kernels.hip -- gfx950 kernels of the JPEG -> RGB decode stage.
//
// Pipeline (one launch each, all on the caller's stream):
//   parse_kernel    one workgroup per image: marker walk (T.81 B.2) and the
//                   10-bit Huffman lookup tables (code+value fused entries).
//   destuff_kernel  one workgroup per image: removes 0xFF00 stuffing, splits
//                   restart segments (RSTn), block-wide prefix sums.
//   entropy_kernel  one workgroup per image: self-synchronising parallel
//                   Huffman decode.  The segment bitstream is cut into
//                   subsequences ("slots"); each thread owns a contiguous run
//                   of slots, decodes it from a guessed state, and runs are
//                   re-decoded from their left neighbour's end state until
//                   every slot start state is consistent (slot boundaries are
//                   checkpoints: a re-decode stops where it merges with the
//                   previous trajectory).  A segmented prefix sum over runs
//                   then gives every run its absolute block index and DC
//                   predictors, and a final pass writes dequantised
//                   coefficients.
//   idct_kernel     8x8 IDCT (FFmpeg simple_idct or IJG islow), block -> plane.
//   output kernels  planes -> RGB / planar YUV (DESIGN.md section 3 lists them).
// The launchers (hj_launch.h) are at the end of the file.
//
// Semantics follow oracle/jpeg_oracle.c line for line (the CPU restatement of
// SPDL's FFmpeg path); the two are compared bit-exactly by tests/.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "hj_common.h"
#include "hj_destuff.h"
#include "hj_idct.h"
#include "hj_launch.h"
#include "hj_sws_tile.h"
#include "hj_upsample.h"

namespace hj {

// a wave-uniform value into an SGPR
__device__ __forceinline__ uint32_t rfl(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// ---------------------------------------------------------------------------
// parse_kernel
// ---------------------------------------------------------------------------

struct ParseScratch {
  ImageInfo info;
  uint16_t qt[4][64];
  uint8_t bits[8][17];   // 0..3 DC, 4..7 AC
  uint8_t vals[8][256];
  int32_t have[8];
  int32_t qhave[4];
  int32_t maxcode[8][18];
  int32_t valoff[8][17];
  // table payloads in effect at SOS (file offsets), copied by all threads
  int32_t dqt_off[4], dqt_pq[4];
  int32_t dht_off[8], dht_n[8];
  int32_t qtsel[kMaxComp];
  // the SOF's component ids and quantiser selectors, the SOS's component
  // order (LDS: as private arrays indexed at run time they lived in scratch)
  int32_t comp_id[kMaxComp], comp_tq[kMaxComp], order[kMaxComp];
};

// Header bytes: the first kHdrBytes of the file are staged in LDS by the
// whole workgroup (one coalesced pass); the serial marker walk reads them
// from there and only reaches into HBM for headers past that window.
constexpr int kHdrBytes = 4096;

typedef __attribute__((address_space(3))) const uint8_t lds_u8;  // an LDS byte

// a header byte past the LDS window (rare): out of line, so the compiler
// cannot speculate the HBM load beside every LDS read of the serial walk
// (it did: each byte of the marker walk waited for an HBM load it then threw
// away -- 31 of the parse kernel's 47 us for a bench image, r06)
__device__ __forceinline__ uint8_t bytes_far(const uint8_t* g, int i) { return g[i]; }

struct Bytes {
  const uint8_t* g;  // file in HBM
  lds_u8* l;         // its first nl bytes in LDS (typed so: a generic pointer
                     // would make every header read a flat load)
  int nl;
  __device__ uint8_t operator[](int i) const {
    if (__builtin_expect(i < nl, 1)) return l[i];
    return bytes_far(g, i);
  }
};

// (the Bytes by value: a pointer to the walk's local Bytes put it in scratch
// memory, and every header byte read first loaded its fields from there)
struct BPtr {
  Bytes b;
  int o;
  __device__ uint8_t operator[](int k) const { return b[o + k]; }
  __device__ BPtr operator+(int k) const { return BPtr{b, o + k}; }
  __device__ BPtr& operator+=(int k) {
    o += k;
    return *this;
  }
};

__device__ static int be16(BPtr p) { return (p[0] << 8) | p[1]; }

__device__ static int parse_headers(const Bytes& d, int size, ParseScratch& s) {
  ImageInfo& in = s.info;
  if (size < 4 || d[0] != 0xFF || d[1] != 0xD8) return kErrNotJpeg;
  int have_sof = 0, prog = 0;
  int32_t* comp_id = s.comp_id;  // (zeroed with the scratch)
  int32_t* comp_tq = s.comp_tq;
  int adobe = -1;
  int pos = 2;
  for (;;) {
    while (pos < size && d[pos] != 0xFF) pos++;
    while (pos < size && d[pos] == 0xFF) pos++;
    if (pos >= size) return kErrBadHeader;
    int m = d[pos++];
    if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
    if (m == 0xD9) return kErrBadHeader;
    if (pos + 2 > size) return kErrBadHeader;
    int len = be16(BPtr{d, pos});
    if (len < 2 || pos + len > size) return kErrBadHeader;
    BPtr p{d, pos + 2};
    int n = len - 2;
    pos += len;
    if (m == 0xDB) {
      while (n > 0) {
        int pq = p[0] >> 4, tq = p[0] & 15;
        if (tq > 3 || pq > 1) return kErrBadHeader;
        int need = 1 + 64 * (pq + 1);
        if (n < need) return kErrBadHeader;
        s.dqt_off[tq] = p.o + 1;
        s.dqt_pq[tq] = pq;
        s.qhave[tq] = 1;
        p += need;
        n -= need;
      }
    } else if (m == 0xC4) {
      while (n > 0) {
        if (n < 17) return kErrBadHeader;
        int tc = p[0] >> 4, th = p[0] & 15;
        if (tc > 1 || th > 3) return kErrBadHeader;
        int slot = tc * 4 + th, total = 0, code = 0;
        s.bits[slot][0] = 0;
        for (int l = 1; l <= 16; l++) {
          s.bits[slot][l] = p[l];
          total += p[l];
          code += p[l];
          if (code > (1 << l)) return kErrBadHeader;
          code <<= 1;
        }
        if (total > 256 || n < 17 + total) return kErrBadHeader;
        s.dht_off[slot] = p.o + 17;
        s.dht_n[slot] = total;
        s.have[slot] = 1;
        p += 17 + total;
        n -= 17 + total;
      }
    } else if (m == 0xC0 || m == 0xC1 || m == 0xC2) {
      prog = m == 0xC2;
      if (n < 6) return kErrBadHeader;
      if (p[0] != 8) return kErrUnsupported;
      in.height = be16(p + 1);
      in.width = be16(p + 3);
      int nf = p[5];
      if (in.height == 0) return kErrUnsupported;
      if (in.width == 0) return kErrBadHeader;
      if (nf != 1 && nf != 3 && nf != 4) return kErrUnsupported;
      if (n < 6 + 3 * nf) return kErrBadHeader;
      in.ncomp = nf;
      for (int c = 0; c < nf; c++) {
        comp_id[c] = p[6 + 3 * c];
        in.comp_h[c] = p[7 + 3 * c] >> 4;
        in.comp_v[c] = p[7 + 3 * c] & 15;
        comp_tq[c] = p[8 + 3 * c];
        if (in.comp_h[c] < 1 || in.comp_h[c] > 4 || in.comp_v[c] < 1 || in.comp_v[c] > 4 ||
            comp_tq[c] > 3)
          return kErrBadHeader;
      }
      if (!frame_color(nf, in.comp_h, in.comp_v, comp_id, adobe, &in.color)) return kErrUnsupported;
      have_sof = 1;
    } else if (m == 0xC3 || (m >= 0xC5 && m <= 0xC7) || (m >= 0xC9 && m <= 0xCB) ||
               (m >= 0xCD && m <= 0xCF)) {
      return kErrUnsupported;
    } else if (m == 0xEE) {  // APP14 "Adobe": the transform flag, for the next SOF
      if (n >= 12 && p[0] == 'A' && p[1] == 'd' && p[2] == 'o' && p[3] == 'b' && p[4] == 'e')
        adobe = p[11];
    } else if (m == 0xDD) {
      if (n < 2) return kErrBadHeader;
      in.ri = be16(p);
    } else if (m == 0xDA) {
      if (!have_sof) return kErrBadHeader;
      if (n < 1) return kErrBadHeader;  // (Ns itself would lie past the segment)
      int ns = p[0];
      if (ns < 1 || ns > in.ncomp) return kErrBadHeader;
      // progressive, or sequential with non-interleaved scans: multiscan_kernel
      // walks every scan; the MCU holds the components in frame order
      in.multiscan = prog || ns != in.ncomp;
      in.progressive = prog;
      if (n < 1 + 2 * ns + 3) return kErrBadHeader;
      int32_t* order = s.order;
      for (int i = 0; i < kMaxComp; i++) order[i] = 0;
      for (int i = 0; i < ns; i++) {
        int cs = p[1 + 2 * i], c = -1;
        for (int k = 0; k < in.ncomp; k++)
          if (comp_id[k] == cs) c = k;
        if (c < 0) return kErrBadHeader;
        order[i] = c;
        in.dc_tab[c] = p[2 + 2 * i] >> 4;
        in.ac_tab[c] = p[2 + 2 * i] & 15;
        if (in.dc_tab[c] > 3 || in.ac_tab[c] > 3) return kErrBadHeader;
      }
      int ss = p[1 + 2 * ns], se = p[2 + 2 * ns], ahal = p[3 + 2 * ns];
      if (!in.multiscan && (ss != 0 || se != 63 || ahal != 0)) return kErrUnsupported;
      in.scan_start = pos;
      if (in.multiscan)
        for (int i = 0; i < in.ncomp; i++) order[i] = i;
      int hmax = 1, vmax = 1;
      for (int c = 0; c < in.ncomp; c++) {
        hmax = max(hmax, in.comp_h[c]);
        vmax = max(vmax, in.comp_v[c]);
      }
      in.hmax = hmax;
      in.vmax = vmax;
      for (int c = 0; c < in.ncomp; c++) {
        if (hmax % in.comp_h[c] || vmax % in.comp_v[c]) return kErrUnsupported;
        if (!s.qhave[comp_tq[c]] ||
            (!in.multiscan && (!s.have[in.dc_tab[c]] || !s.have[4 + in.ac_tab[c]])))
          return kErrBadHeader;
        in.comp_w[c] = (in.width * in.comp_h[c] + hmax - 1) / hmax;
        in.comp_hpx[c] = (in.height * in.comp_v[c] + vmax - 1) / vmax;
        s.qtsel[c] = comp_tq[c];
      }
      if (in.ncomp == 1) {
        in.comp_bw[0] = (in.comp_w[0] + 7) / 8;
        in.comp_bh[0] = (in.comp_hpx[0] + 7) / 8;
        in.mcux = in.comp_bw[0];
        in.mcuy = in.comp_bh[0];
        in.bpm = 1;
        in.mcu_comp[0] = 0;
        in.mcu_dx[0] = in.mcu_dy[0] = 0;
      } else {
        in.mcux = (in.width + 8 * hmax - 1) / (8 * hmax);
        in.mcuy = (in.height + 8 * vmax - 1) / (8 * vmax);
        int b = 0;
        for (int i = 0; i < (in.multiscan ? in.ncomp : ns); i++) {
          int c = order[i];
          in.comp_bw[c] = in.mcux * in.comp_h[c];
          in.comp_bh[c] = in.mcuy * in.comp_v[c];
          for (int y = 0; y < in.comp_v[c]; y++)
            for (int x = 0; x < in.comp_h[c]; x++) {
              if (b >= kMaxBpm) return kErrUnsupported;
              in.mcu_comp[b] = c;
              in.mcu_dx[b] = x;
              in.mcu_dy[b] = y;
              b++;
            }
        }
        in.bpm = b;
      }
      in.nblocks = in.mcux * in.mcuy * in.bpm;
      in.bpm_magic = idct_div_magic((uint32_t)in.bpm);
      in.mcux_magic = idct_div_magic((uint32_t)in.mcux);
      return kOk;
    }
  }
}

// The batch's host-built inputs arrive with the first kernel: each
// workgroup pulls its image's descriptor, and all of them the swscale table
// pool, straight from the slot's pinned staging (mapped host memory) into the
// workspace -- no DMA-engine copy and no cross-queue sync ahead of the batch.
__global__ void __launch_bounds__(256, 8) parse_kernel(const uint8_t* __restrict__ bytes,
                                                    const ImageDesc* __restrict__ host_desc,
                                                    ImageDesc* __restrict__ desc,
                                                    ImageInfo* __restrict__ infos,
                                                    HuffTable* __restrict__ luts,
                                                    const uint4* __restrict__ host_tables,
                                                    uint4* __restrict__ tables, int64_t ntab16,
                                                    const uint32_t* __restrict__ host_work,
                                                    uint32_t* __restrict__ work, int nwork,
                                                    uint64_t* __restrict__ chain,
                                                    uint32_t* __restrict__ ds_map,
                                                    uint32_t* __restrict__ idct_map,
                                                    uint32_t* __restrict__ hs_map,
                                                    uint32_t* __restrict__ sws_map,
                                                    const int ndesc) {
  __shared__ ParseScratch s;
  __shared__ int st;
  __shared__ __attribute__((aligned(16))) uint8_t hdr[kHdrBytes];
  const int img = blockIdx.x, tid = threadIdx.x;
#if HJ_PARSE_PROF  // phase timers (variant builds): ImageInfo::sdiag[40..46]
  int64_t pt[8];
  int npt = 0;
  pt[npt++] = wall_clock64();
#define HJ_PT() (pt[npt++] = wall_clock64())
#else
#define HJ_PT() ((void)0)
#endif
  // the descriptor in LDS (a private copy, indexed at run time, lived in
  // scratch memory)
  __shared__ __attribute__((aligned(16))) ImageDesc sdd;
  {
    static_assert(sizeof(ImageDesc) % 8 == 0, "descriptor copied in 8-byte words");
    const uint64_t* src = reinterpret_cast<const uint64_t*>((host_desc ? host_desc : desc) + img);
    uint64_t* dst = reinterpret_cast<uint64_t*>(desc + img);
    uint64_t* sdst = reinterpret_cast<uint64_t*>(&sdd);
    for (int i = tid; i < (int)(sizeof(ImageDesc) / 8); i += blockDim.x) {
      const uint64_t v = src[i];
      if (host_desc) dst[i] = v;
      sdst[i] = v;
    }
  }
  if (host_desc) {
    for (int64_t i = (int64_t)img * blockDim.x + tid; i < ntab16;
         i += (int64_t)gridDim.x * blockDim.x)
      tables[i] = host_tables[i];
    for (int i = img * blockDim.x + tid; i < nwork; i += gridDim.x * blockDim.x)
      work[i] = host_work[i];
  }
  // A views submission: descriptors [n, ndesc) are the views' (ImageDesc::src),
  // which no workgroup parses.  The images' workgroups bring them over in turn
  // and map their output workgroups.
  for (int v = (int)gridDim.x + img; v < ndesc; v += (int)gridDim.x) {
    const ImageDesc* sv = (host_desc ? host_desc : desc) + v;
    if (host_desc) {
      const uint64_t* src = reinterpret_cast<const uint64_t*>(sv);
      uint64_t* dst = reinterpret_cast<uint64_t*>(desc + v);
      for (int i = tid; i < (int)(sizeof(ImageDesc) / 8); i += blockDim.x) dst[i] = src[i];
    }
    const int hs0 = sv->hs_wg0, hsn = sv->hs_wgs, sw0 = sv->sws_wg0,
              swn = sv->sws_bands * sv->sws_chunks;
    for (int i = tid; i < hsn; i += blockDim.x) hs_map[hs0 + i] = (uint32_t)v;
    for (int i = tid; i < swn; i += blockDim.x) sws_map[sw0 + i] = (uint32_t)v;
  }
  __syncthreads();
  const ImageDesc& dd = sdd;
  // the flat grids' dispatch maps: this image's destuff-chunk and IDCT
  // workgroups (written whatever the status: those kernels look it up)
  for (int i = tid; i < dd.ds_cap; i += blockDim.x) ds_map[dd.ds_wg0 + i] = (uint32_t)img;
  for (int i = tid; i < (dd.idct_blocks + kIdctThreads - 1) / kIdctThreads; i += blockDim.x)
    idct_map[dd.idct_wg0 + i] = (uint32_t)img;
  for (int i = tid; i < dd.hs_wgs; i += blockDim.x) hs_map[dd.hs_wg0 + i] = (uint32_t)img;
  for (int i = tid; i < dd.sws_bands * dd.sws_chunks; i += blockDim.x)
    sws_map[dd.sws_wg0 + i] = (uint32_t)img;
  // the entropy kernel's ticket counter and this image's piece records
  if (img == 0 && tid == 0) chain[0] = 0ull;
  if (dd.pieces > 1)
    for (int i = tid; i < dd.pieces * kChainGranules; i += blockDim.x)
      chain[kChainHead + dd.chain_off + i] = 0ull;
  {
    int* z = reinterpret_cast<int*>(&s);
    for (int i = tid; i < (int)(sizeof(ParseScratch) / 4); i += blockDim.x) z[i] = 0;
  }
  const int nh = (int)min(dd.in_size, (int64_t)kHdrBytes) & ~15;  // whole 16-byte groups
  for (int i = tid; i < nh / 16; i += blockDim.x)
    reinterpret_cast<uint4*>(hdr)[i] = reinterpret_cast<const uint4*>(bytes + dd.in_off)[i];
  __syncthreads();
  HJ_PT();
  if (tid == 0) {
    const Bytes file{bytes + dd.in_off, (lds_u8*)hdr, nh};
    int rc = parse_headers(file, (int)dd.in_size, s);
    if (rc == kOk) {
      // the host probe sized every buffer; it must agree with the device parse
      if (s.info.width != dd.width || s.info.height != dd.height || s.info.ncomp != dd.ncomp ||
          s.info.nblocks != dd.nblocks || s.info.color != dd.color)
        rc = kErrBadHeader;
      for (int c = 0; c < s.info.ncomp && rc == kOk; c++)
        if (s.info.comp_h[c] != dd.h_samp[c] || s.info.comp_v[c] != dd.v_samp[c])
          rc = kErrBadHeader;
      if (rc == kOk && s.info.ri > 0 &&
          (s.info.mcux * s.info.mcuy + s.info.ri - 1) / s.info.ri > dd.seg_cap)
        rc = kErrBadRestart;
    }
    if (rc == kOk && dd.refuse) rc = dd.refuse;  // the host refused this image alone
    s.info.status = rc;
    st = rc;
  }
  __syncthreads();
  HJ_PT();
  // canonical-code decode arrays (T.81 F.2.2.3 / libjpeg jdhuff.c), one
  // thread per table slot
  if (tid < 8 && st == kOk && s.have[tid]) {
    const int t = tid;
    {
      int code = 0, k = 0;
      for (int l = 1; l <= 16; l++) {
        if (s.bits[t][l]) {
          s.valoff[t][l] = k - code;
          code += s.bits[t][l];
          k += s.bits[t][l];
          s.maxcode[t][l] = code - 1;
        } else {
          s.maxcode[t][l] = -1;
          s.valoff[t][l] = 0;
        }
        code <<= 1;
      }
      s.maxcode[t][17] = 0x7FFFFFFF;
    }
  }
  __syncthreads();
  HJ_PT();
  if (st != kOk) {
    if (tid == 0) infos[img] = s.info;
    return;
  }
  {
    // table payloads: every thread copies a share
    const Bytes file{bytes + dd.in_off, (lds_u8*)hdr, nh};
    for (int i = tid; i < 8 * 256; i += blockDim.x) {
      const int t = i >> 8, k = i & 255;
      if (s.have[t]) s.vals[t][k] = k < s.dht_n[t] ? file[s.dht_off[t] + k] : 0;
    }
    for (int i = tid; i < 4 * 64; i += blockDim.x) {
      const int t = i >> 6, k = i & 63;
      if (s.qhave[t])
        s.qt[t][k] = s.dqt_pq[t] ? (uint16_t)((file[s.dqt_off[t] + 2 * k] << 8) |
                                              file[s.dqt_off[t] + 2 * k + 1])
                                 : file[s.dqt_off[t] + k];
    }
  }
  __syncthreads();
  HJ_PT();
  // the image's quantisation tables by component
  for (int i = tid; i < s.info.ncomp * 64; i += blockDim.x)
    s.info.qt[i / 64][i % 64] = s.qt[s.qtsel[i / 64]][i % 64];
  __syncthreads();
  if (s.info.multiscan) {  // tables are built per scan later
    if (tid == 0) infos[img] = s.info;
    return;
  }
  // The tables themselves are built by lut_kernel, once per distinct table of
  // the batch; here: their identity (offset, size, FNV-1a hash of the 16
  // lengths + symbols) and the sub-table count the entropy instance choice
  // needs.  One thread per table slot.
  __shared__ int tab_nsub[8], tab_slow;
  if (tid == 0) tab_slow = 0;
  __syncthreads();
  if (tid < 8) {
    const int t = tid;
    int nsub = 0;
    if (s.have[t]) {
      uint32_t h = 2166136261u;
      for (int l = 1; l <= 16; l++) h = (h ^ s.bits[t][l]) * 16777619u;
      for (int k = 0; k < s.dht_n[t]; k++) h = (h ^ s.vals[t][k]) * 16777619u;
      s.info.tab_off[t] = s.dht_off[t] - 16;
      s.info.tab_n[t] = s.dht_n[t];
      s.info.tab_hash[t] = h;
      // canonical codes are consecutive: the 10-bit prefixes of all codes
      // longer than kLutBits form one contiguous range
      int p_lo = kLutSize, p_hi = -1;
      for (int l = kLutBits + 1; l <= 16; l++) {
        if (s.bits[t][l] == 0) continue;
        const int first = s.maxcode[t][l] - s.bits[t][l] + 1;
        p_lo = min(p_lo, first >> (l - kLutBits));
        p_hi = max(p_hi, s.maxcode[t][l] >> (l - kLutBits));
      }
      nsub = p_hi >= p_lo ? p_hi - p_lo + 1 : 0;
      if (nsub > kMaxSub) {
        atomicOr(&tab_slow, 1 << t);
        nsub = 0;
      }
    } else {
      s.info.tab_off[t] = 0;
      s.info.tab_n[t] = 0;
      s.info.tab_hash[t] = 0;
    }
    s.info.lut_ref[t] = img * 8 + t;
    tab_nsub[t] = nsub;
  }
  __syncthreads();
  if (tid == 0) {
    // Which entropy instance decodes this scan: NTAB = 4 takes <= 4 distinct
    // tables whose long codes all fit the LDS sub-table pool, each table its
    // slot's share of it (no canonical fallback); the wide path takes the
    // rest.  Decided once here, so the entropy
    // kernels test one flag instead of walking the tables in HBM.
    int ns = 0, seen = 0, subs = 0, slow = 0;
    for (int c = 0; c < s.info.ncomp; c++)
      for (int k = 0; k < 2; k++) {
        const int slot = k == 0 ? s.info.dc_tab[c] : 4 + s.info.ac_tab[c];
        if (!(seen & (1 << slot))) {
          ns++;
          subs += tab_nsub[slot];
          slow |= (tab_slow >> slot) & 1;
          // (the LDS-only loops give every table slot kSubShare entries)
          slow |= tab_nsub[slot] > (kSubShare >> kSubBits);
        }
        seen |= 1 << slot;
      }
    s.info.ent_wide = !(ns <= 4 && (subs << kSubBits) <= kSubPool && !slow);
  }
  __syncthreads();
  HJ_PT();
#if HJ_PARSE_PROF
  if (tid == 0)
    for (int i = 1; i < npt && i < 8; i++) s.info.sdiag[39 + i] = (int32_t)(pt[i] - pt[0]);
#endif
  static_assert(sizeof(ImageInfo) % 4 == 0, "ImageInfo copied in words");
  {  // the parse result out, a word per thread
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&s.info);
    uint32_t* dst = reinterpret_cast<uint32_t*>(infos + img);
    for (int i = tid; i < (int)(sizeof(ImageInfo) / 4); i += blockDim.x) dst[i] = src[i];
  }
}

// ---------------------------------------------------------------------------
// lut_kernel: the Huffman LUTs, once per distinct table of the batch.  One
// workgroup per (table slot, image): the table is looked for among the
// earlier images' tables of the same slot (hash, then the bytes); the first
// image holding these bytes builds it into its own LUT slot, the others only
// point there (ImageInfo::lut_ref).  A batch of one encoder's files (shared
// standard or per-quality tables) builds a handful of tables instead of
// eight per image.
// ---------------------------------------------------------------------------

__global__ void __launch_bounds__(256) lut_kernel(const uint8_t* __restrict__ bytes,
                                                  const ImageDesc* __restrict__ desc,
                                                  ImageInfo* __restrict__ infos,
                                                  HuffTable* __restrict__ luts) {
  __shared__ int first, same, maxcode[18], valoff[17];
  __shared__ uint8_t bits[17], vals[256];
  const int t = blockIdx.x, img = blockIdx.y, tid = threadIdx.x;
  const ImageInfo& in = infos[img];
  if (in.status != kOk || in.multiscan || in.tab_n[t] == 0) return;
  const uint32_t h = in.tab_hash[t];
  const int n = in.tab_n[t];
  const uint8_t* d = bytes + desc[img].in_off + in.tab_off[t];
  if (tid == 0) first = img;
  __syncthreads();
  for (int j = tid; j < img; j += blockDim.x) {
    const ImageInfo& o = infos[j];
    if (o.status == kOk && !o.multiscan && o.tab_n[t] == n && o.tab_hash[t] == h)
      atomicMin(&first, j);
  }
  __syncthreads();
  const int j = first;
  if (j < img) {  // the same bytes? (a hash match is only a candidate)
    if (tid == 0) same = 1;
    __syncthreads();
    const uint8_t* e = bytes + desc[j].in_off + infos[j].tab_off[t];
    for (int k = tid; k < 16 + n; k += blockDim.x)
      if (d[k] != e[k]) same = 0;
    __syncthreads();
    if (same) {
      if (tid == 0) infos[img].lut_ref[t] = j * 8 + t;
      return;
    }
  }
  // build: canonical arrays (T.81 F.2.2.3 / libjpeg jdhuff.c), then the LUT
  if (tid < 16) bits[tid + 1] = d[tid];
  for (int k = tid; k < 256; k += blockDim.x) vals[k] = k < n ? d[16 + k] : 0;
  __syncthreads();
  if (tid == 0) {
    int code = 0, k = 0;
    for (int l = 1; l <= 16; l++) {
      if (bits[l]) {
        valoff[l] = k - code;
        code += bits[l];
        k += bits[l];
        maxcode[l] = code - 1;
      } else {
        maxcode[l] = -1;
        valoff[l] = 0;
      }
      code <<= 1;
    }
    maxcode[17] = 0x7FFFFFFF;
  }
  __syncthreads();
  HuffTable& T = luts[(size_t)img * 8 + t];
  const bool is_dc = t < 4;
  int p_lo = kLutSize, p_hi = -1;
  for (int l = kLutBits + 1; l <= 16; l++) {
    if (bits[l] == 0) continue;
    const int fc = maxcode[l] - bits[l] + 1;
    p_lo = min(p_lo, fc >> (l - kLutBits));
    p_hi = max(p_hi, maxcode[l] >> (l - kLutBits));
  }
  const int nsub = p_hi >= p_lo ? p_hi - p_lo + 1 : 0;
  const bool sub_ok = nsub <= kMaxSub;
  // one 16-bit window -> entry (levels share this): codes up to max_len
  // bits; the value is folded in (Full) when code + value fit full_max bits
  // (level 1: |v| < 2^9; sub-tables: codes >= 11 bits, |v| < 2^5 -- both
  // fit the entry's int11 field)
  auto entry16 = [&](uint32_t w16, int max_len, int full_max) -> uint32_t {
    for (int l = 1; l <= max_len; l++) {
      const int code = (int)(w16 >> (16 - l));
      if (code <= maxcode[l]) {
        const int sym = vals[valoff[l] + code];
        const int sz = is_dc ? sym : (sym & 15);
        if (is_dc && sym > 15) return 0u;  // invalid size (stored as 1: see below)
        if (l + sz <= full_max) {
          int v = 0;
          if (sz) {
            const int raw = (int)((w16 >> (16 - l - sz)) & ((1u << sz) - 1));
            v = raw < (1 << (sz - 1)) ? raw - ((1 << sz) - 1) : raw;
          }
          return hj_entry(kKindFull, l + sz, sym, is_dc, v);
        }
        return hj_entry(kKindCode, l, sym, is_dc, 0);
      }
    }
    return 0u;
  };
  for (int idx = tid; idx < kLutSize; idx += blockDim.x) {
    // level 1 resolves codes (and code+value) that fit in kLutBits
    uint32_t e = entry16((uint32_t)idx << kSubBits, kLutBits, kLutBits);
    if (e == 0u && idx >= p_lo && idx <= p_hi)
      e = sub_ok ? ((kKindSub << 5) | ((uint32_t)(idx - p_lo) << kEntHiShift)) : 0u;
    T.lut[idx] = e ? e : 1u;  // invalid: kind Slow, one bit (the decode loops' step)
  }
  if (sub_ok)
    for (int i = tid; i < nsub << kSubBits; i += blockDim.x)
      T.sub[i] = max(entry16(((uint32_t)(p_lo + (i >> kSubBits)) << kSubBits) |
                                 (uint32_t)(i & ((1 << kSubBits) - 1)),
                             16, 16),
                     1u);
  if (tid == 0) {
    T.nsub = sub_ok ? nsub : 0;
    T.long_slow = sub_ok ? 0 : 1;  // long codes left to the canonical path
    T.sub_lo = sub_ok ? p_lo : 0;
  }
  if (tid < 18) T.maxcode[tid] = maxcode[tid];
  if (tid < 17) T.valoff[tid] = valoff[tid];
  for (int i = tid; i < 256; i += blockDim.x) T.vals[i] = vals[i];
}

// ---------------------------------------------------------------------------
// destuff_kernel
// ---------------------------------------------------------------------------

constexpr int kDsThreads = 256;
constexpr int kDsPer = kDsChunk / kDsThreads;

__device__ __forceinline__ int wave_incl_scan(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}

// Workgroup exclusive scan of two counters (256 threads = 4 waves); also
// returns the totals.
__device__ __forceinline__ void wg_scan2(int a, int b, int& ea, int& eb, int& ta, int& tb,
                                        int* sh /* 8 ints */) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int ia = wave_incl_scan(a), ib = wave_incl_scan(b);
  if (lane == 63) {
    sh[wid] = ia;
    sh[4 + wid] = ib;
  }
  __syncthreads();
  ea = ia - a;
  eb = ib - b;
  ta = tb = 0;
#pragma unroll
  for (int w = 0; w < 4; w++) {
    if (w < wid) {
      ea += sh[w];
      eb += sh[4 + w];
    }
    ta += sh[w];
    tb += sh[4 + w];
  }
}

// Wave inclusive scan in six DPP adds: Hillis-Steele inside each row of 16
// lanes (a shift past the row's start reads 0), then the rows' totals handed
// on by row_bcast:15 into rows 1 and 3 and row_bcast:31 into rows 2 and 3.
// Every lane of the wave must be active.
__device__ __forceinline__ int wave_incl_scan_dpp(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);  // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);  // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);  // row_bcast:15
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);  // row_bcast:31
  return v;
}

// Workgroup exclusive scan of one word (the destuff kernels pack two counters
// in it: rst << 16 | keep, a chunk holds at most 2048 / 4096); also the total.
__device__ __forceinline__ void wg_scan1(int v, int& ex, int& tot, int* sh /* 4 ints */) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int iv = wave_incl_scan_dpp(v);
  if (lane == 63) sh[wid] = iv;
  __syncthreads();
  ex = iv - v;
  tot = 0;
#pragma unroll
  for (int w = 0; w < 4; w++) {
    if (w < wid) ex += sh[w];
    tot += sh[w];
  }
}

// A thread's group for hj_destuff.h: the 16 bytes [j0, j0 + 16) of file `d` as
// words, the byte before (0 where there is none) and the byte after; bytes
// past the file read as 0xD9 (EOI).
__device__ __forceinline__ void ds_load(const uint8_t* __restrict__ d, int size, int j0,
                                        uint32_t (&w)[4], uint32_t& prev, uint32_t& next) {
  prev = ds_prev_byte(d, size, j0);
  if (j0 + 16 <= size) {
    const uint4 q = *reinterpret_cast<const uint4*>(d + j0);
    w[0] = q.x;
    w[1] = q.y;
    w[2] = q.z;
    w[3] = q.w;
  } else {
    ds_load_bytes(d, size, j0, w);
  }
  next = ds_next_byte(d, size, j0);
}

// destuff_write_kernel's LDS stage: a chunk's kept bytes at the destination's
// offset within 16 bytes, so that the copy-out moves 16 bytes at a time
// (yuv_planes_kernel stages its tiles the same way).  16 bytes of slack in
// front (a group is stored below its first kept byte by up to 15 zero bytes),
// 15 of offset and 32 behind.
constexpr int kDsStageWords = (16 + 16 + kDsChunk + 32) / 4;

// Copy the `n` staged bytes to `dst` (staged from byte 16 + (dst & 15) on):
// head bytes singly, 16-byte LDS loads and global stores, tail bytes singly.
__device__ __forceinline__ void stage_to_global(uint8_t* __restrict__ dst, const uint32_t* stage,
                                                int n, int tid) {
  const int a = (int)((uintptr_t)dst & 15);
  const uint8_t* src = reinterpret_cast<const uint8_t*>(stage) + 16 + a;
  const int head = min(n, (16 - a) & 15);
  if (tid < head) dst[tid] = src[tid];
  const int nv = (n - head) >> 4;
  const uint4* s4 = reinterpret_cast<const uint4*>(src + head);
  uint4* d4 = reinterpret_cast<uint4*>(dst + head);
  for (int i = tid; i < nv; i += kDsThreads) d4[i] = s4[i];
  const int t0 = head + 16 * nv;
  if (t0 + tid < n) dst[t0 + tid] = src[t0 + tid];
}

// Destuffing runs as count -> per-image prefix -> write over 4 KB chunks of
// every image at once (chunk k of image i starts at (scan_start & ~15) + 4096 k).
__global__ void __launch_bounds__(kDsThreads) destuff_count_kernel(
    const uint8_t* __restrict__ bytes, const ImageDesc* __restrict__ desc,
    const ImageInfo* __restrict__ infos, DsChunk* __restrict__ chunks,
    const uint32_t* __restrict__ ds_map) {
  __shared__ int shsum, shterm;
  // (chunk, image) grid, or a flat grid over every image's chunks (ds_map:
  // workgroup -> image) when the batch's sizes differ widely
  const bool flat = ds_map != nullptr;
  const int img = flat ? (int)ds_map[blockIdx.x] : (int)blockIdx.y;
  const int k = flat ? (int)blockIdx.x - desc[img].ds_wg0 : (int)blockIdx.x, tid = threadIdx.x;
  if (infos[img].status != kOk || infos[img].multiscan) return;
  const ImageDesc& dd = desc[img];
  const int size = (int)dd.in_size, start = infos[img].scan_start;
  const int cbase = (start & ~15) + k * kDsChunk;
  if (cbase >= size || k >= dd.ds_cap) return;
  if (tid == 0) {
    shsum = 0;
    shterm = 0x7FFFFFFF;
  }
  __syncthreads();
  const uint8_t* d = bytes + dd.in_off;
  const int j0 = cbase + tid * kDsPer;
  uint32_t w[4], prev, next;
  ds_load(d, size, j0, w, prev, next);
  uint32_t slow;
  int cnt = ds_count_words(w, prev, next, j0, start, size, slow);
  if (slow) {  // a marker: rare, at most one per image besides RSTn
    uint32_t rst;
    int term;
    ds_resolve(d, size, j0, slow, rst, term);
    cnt += __popc(rst) << 16;
    if (term != 0x7FFFFFFF) atomicMin(&shterm, term);
  }
  // rst << 16 | keep: at most 2048 and 4096 per chunk
  const int wsum = wave_incl_scan_dpp(cnt);
  if ((tid & 63) == 63) atomicAdd(&shsum, wsum);
  __syncthreads();
  if (tid == 0) {
    DsChunk& c = chunks[dd.ds_off + k];
    c.keep = shsum & 0xFFFF;
    c.rst = shsum >> 16;
    c.term = shterm;
  }
}

// One workgroup per image: exclusive prefix of the chunk counts up to the
// first terminating marker; records the scan end (terminator or file end).
__global__ void __launch_bounds__(kDsThreads) destuff_prefix_kernel(
    const ImageDesc* __restrict__ desc, ImageInfo* __restrict__ infos,
    DsChunk* __restrict__ chunks) {
  __shared__ int sh[8];
  __shared__ int shterm;
  const int img = blockIdx.x, tid = threadIdx.x;
  if (infos[img].status != kOk || infos[img].multiscan) return;
  const ImageDesc& dd = desc[img];
  const int size = (int)dd.in_size, start = infos[img].scan_start;
  const int base = start & ~15;
  const int nch = min(dd.ds_cap, (size - base + kDsChunk - 1) / kDsChunk);
  if (tid == 0) shterm = 0x7FFFFFFF;
  __syncthreads();
  for (int k = tid; k < nch; k += kDsThreads) atomicMin(&shterm, chunks[dd.ds_off + k].term);
  __syncthreads();
  const int end = min(shterm, size);
  int ck = 0, cr = 0;
  for (int k0 = 0; k0 < nch; k0 += kDsThreads) {
    const int k = k0 + tid;
    const bool v = k < nch && base + k * kDsChunk < end;
    const int kk = v ? chunks[dd.ds_off + k].keep : 0, rr = v ? chunks[dd.ds_off + k].rst : 0;
    int ek, er, tk, tr;
    wg_scan2(kk, rr, ek, er, tk, tr, sh);
    if (k < nch) {
      chunks[dd.ds_off + k].keep_pre = ck + ek;
      chunks[dd.ds_off + k].rst_pre = cr + er;
    }
    ck += tk;
    cr += tr;
    __syncthreads();
  }
  if (tid == 0) infos[img].scan_end = end;
}

__global__ void __launch_bounds__(kDsThreads) destuff_write_kernel(
    const uint8_t* __restrict__ bytes, const ImageDesc* __restrict__ desc,
    ImageInfo* __restrict__ infos, const DsChunk* __restrict__ chunks, uint8_t* __restrict__ clean,
    uint32_t* __restrict__ segs, const uint32_t* __restrict__ ds_map) {
  __shared__ int sh[4];
  __shared__ __attribute__((aligned(16))) uint32_t stage[kDsStageWords];
  const bool flat = ds_map != nullptr;
  const int img = flat ? (int)ds_map[blockIdx.x] : (int)blockIdx.y;
  const int k = flat ? (int)blockIdx.x - desc[img].ds_wg0 : (int)blockIdx.x, tid = threadIdx.x;
  if (infos[img].status != kOk || infos[img].multiscan) return;
  const ImageDesc& dd = desc[img];
  const int size = (int)dd.in_size, start = infos[img].scan_start, end = infos[img].scan_end;
  const int base = start & ~15;
  const int cbase = base + k * kDsChunk;
  // the chunk holding the last scan byte also finishes the image
  const int last = (max(end - 1, start) - base) / kDsChunk;
  if (k > last || k >= dd.ds_cap) return;
  for (int i = tid; i < kDsStageWords / 4; i += kDsThreads)
    reinterpret_cast<uint4*>(stage)[i] = make_uint4(0, 0, 0, 0);
  const uint8_t* d = bytes + dd.in_off;
  const int j0 = cbase + tid * kDsPer;
  uint32_t w[4], prev, next;
  ds_load(d, size, j0, w, prev, next);
  // bytes at or past the scan end are not part of it
  const DsMasks m = ds_classify_words(w, prev, next, j0, start, end);
  const uint32_t keep = m.keep;
  uint32_t rst = 0;
  if (m.slow) {
    int term;
    ds_resolve(d, size, j0, m.slow, rst, term);
  }
  int ex, tot;
  wg_scan1((int)(__popc(rst) << 16 | __popc(keep)), ex, tot, sh);  // syncs: the stage is zero
  const int ek = ex & 0xFFFF, er = ex >> 16, tk = tot & 0xFFFF, tr = tot >> 16;
  const DsChunk& c = chunks[dd.ds_off + k];
  uint32_t* sg = segs + dd.seg_off;
  if (rst) {  // RSTn markers record segment starts
    int r = c.rst_pre + er;
    bool overflow = false;
    for (uint32_t q = rst; q; q &= q - 1) {
      const int i = ds_ctz(q);
      r++;
      if (r < dd.seg_cap) sg[r] = (uint32_t)(c.keep_pre + ek + __popc(keep & ((1u << i) - 1u)));
      else overflow = true;
    }
    if (overflow) infos[img].status = kErrBadRestart;
  }
  uint8_t* out = clean + dd.in_off + c.keep_pre;
  // compact the kept bytes in registers: one step per dropped byte, as many
  // steps as the wave's worst group needs (one or two on ordinary scans)
  uint32_t drop;
  ds_compact_begin(w, keep, drop);
  while (__any(drop != 0u)) ds_compact_step(w, drop);
  if (keep) {
    // the kept bytes start at register byte ctz(keep), zeros below and above:
    // shift the group to its byte offset in the stage and OR the five words in
    const int p = 16 + (int)((uintptr_t)out & 15) + ek - ds_ctz(keep);
    uint32_t x[5];
    ds_shift_words(w, (uint32_t)(p & 3), x);
    uint32_t* q = stage + (p >> 2);
#pragma unroll
    for (int i = 0; i < 5; i++) atomicOr(q + i, x[i]);
  }
  __syncthreads();
  stage_to_global(out, stage, tk, tid);
  if (k == last) {
    const int clen = c.keep_pre + tk;
    if (tid < 64) out[tk + tid] = 0;  // zero padding past the data
    if (tid == 0) {
      infos[img].clean_len = clen;
      infos[img].nseg = min(c.rst_pre + tr + 1, dd.seg_cap);
      sg[0] = 0;
    }
  }
}

// ---------------------------------------------------------------------------
// entropy_kernel
// ---------------------------------------------------------------------------

constexpr int kMaxTabs = 2 * kMaxComp;  // distinct (DC, AC) tables of a scan
// The coefficient lists' index field: a coefficient's slot in the IDCT's
// LDS block, not its natural index: each row stored as the pairs (x0, x2),
// (x4, x6), (x1, x3), (x5, x7), so the row pass reads its even and odd
// halves as ready-packed int16 pairs for v_dot2 (slot = row * 8 +
// ((c >> 1) | (c & 1) << 2) for natural index row * 8 + c).  Per zig-zag
// position:
__constant__ uint8_t kSlotOrder[64] = {
    0,  4,  8,  16, 12, 1,  5,  9,  20, 24, 32, 28, 17, 13, 2,  6,  10, 21, 25, 36, 40, 48,
    44, 33, 29, 18, 14, 3,  7,  11, 22, 26, 37, 41, 52, 56, 60, 49, 45, 34, 30, 19, 15, 23,
    27, 38, 42, 53, 57, 61, 50, 46, 35, 31, 39, 43, 54, 58, 62, 51, 47, 55, 59, 63};
// bit-reader window per thread (words): 12 restages a lane every ~8-11 words
// (r04 A/B, 4-lane bench: 8 words 507.5k img/s, 12 515.1k, 16 514.1k)
constexpr int kWinWords = 12;

// NTAB = distinct Huffman tables the workgroup holds in LDS: 4 covers luma +
// chroma DC/AC (gray: 2) and keeps three entropy workgroups per CU; a scan
// with 5-6 distinct tables reads the extra ones from their HBM copies.
template <int NT, int NTAB>
struct EntShared {
  static constexpr int kTabs = NTAB;
  uint32_t lut[NTAB][kLutSize];
  uint32_t sub[kSubPool];
  int32_t maxcode[NTAB][18];
  int32_t valoff[NTAB][17];
  uint8_t vals[NTAB][256];
  uint32_t run_pos[NT];
  uint32_t run_zb[NT];
  uint32_t qdc[kMaxComp];  // DC quantiser per component
  // The bit-reader windows are dead outside round 0 / the sync rounds, so the
  // reduction and scan scratch share their storage (keeps the workgroup at
  // <= 80 KiB of LDS: two entropy workgroups -- e.g. of two concurrent
  // batches -- fit one CU and fill each other's barrier stalls).
  union {
    uint32_t win[kWinWords][NT];  // bit-reader windows
    struct {
      int32_t scan_flag[NT];
      int32_t scan_v[NT][kMaxComp];  // block totals (0), or the DC sums per component
      int32_t red[NT];
    } sc;
  };
  int32_t flag;
  int32_t err;
  // chain rounds: runs to re-decode, and the chains' heads (bit per run)
  uint64_t cmask[NT / 64], hmask[NT / 64];
  uint32_t chain_bits;  // bits the chain rounds decoded (diagnostics)
#if HJ_OWN_CHECK
  uint32_t own_viol;    // write-pass descriptor stores outside the storing run's scan range
#endif
  uint32_t chain_sweeps;  // chains they decoded (diagnostics)
  // the left neighbour of run 0 (a piece's first run: the previous piece's
  // end state once known; zb 0xFFFFFFFF = none) and a piece's hand-off results
  uint32_t left_pos, left_zb;
  int32_t lb_ok, lb_blocks;
  int32_t lb_dc[kMaxComp];
  // tables past the NTAB LDS slots (5-6 distinct tables, rare): read from
  // the parse kernel's HBM copy
  const HuffTable* gtab;
  int32_t gslot[kMaxTabs];
};
static_assert(sizeof(EntShared<512, 4>) <= 160 * 1024 / 2,
              "entropy LDS must allow 2 workgroups per CU");
static_assert(sizeof(EntShared<256, 4>) <= 160 * 1024 / 3,
              "entropy LDS must allow 3 workgroups per CU at 256 threads");

// Per-thread bit reader over the destuffed stream (big-endian bytes read as
// 32-bit words).  Words come from a kWinWords LDS window per thread
// ([word][thread], conflict-free), restaged from HBM once every 8-11 words:
// the decode loop itself issues no global load, so its coefficient stores
// never stall it (on gfx9 a vmcnt wait for a load also waits for older
// stores).
//
// The state is the bit position alone; each step reads the two window words
// holding bits [pos, pos + 32) (one ds_read2st64) and shifts them -- no bit
// buffer to refill, no branch.  (A 64-bit register bit buffer refilled from
// the window one word ahead takes the window read off the symbol's
// dependency chain, but its refill selects cost more issue than the read's
// latency: round 0 +11 %, r04 A/B.)  The decode loops are issue-bound as much
// as latency-bound, so the step is written for instruction count: the
// window position as a bit offset from the window's first bit (`wbit`), the
// table of a step from one packed map per symbol class (TabMap).
struct Dec {
  uint32_t wbit;  // absolute bit position of the window's first word
  uint32_t pos;   // absolute bit position of the next symbol
  uint32_t z;     // next coefficient index (0 = DC)
  uint32_t bs;    // 3 * block-in-MCU
};

// The Huffman table slots and component of each block of the MCU, packed
// 3 bits per block-in-MCU b at bit 3b (Dec::bs), and the MCU's end.
struct TabMap {
  uint32_t dmap;    // LDS table slot of b's DC table
  uint32_t amap;    // ... of its AC table
  uint32_t cmap;    // its component
  uint32_t bs_end;  // 3 * blocks per MCU
  uint32_t rdmap, ramap;  // dmap / amap packed in reverse: block b at bit bs_end - 3 - 3b
  uint64_t unused_;       // unused (always 0): without it the chain walk's scalar copies reorder
};

template <int NT>
__device__ __forceinline__ void win_stage(uint32_t* win, const uint32_t* words, uint32_t wb) {
  static_assert(kWinWords % 4 == 0, "window is staged in uint4 units");
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4), aligned(4)));
  const u32x4* src = reinterpret_cast<const u32x4*>(words + wb);  // dword-aligned 16-B loads
  u32x4 q[kWinWords / 4];
#pragma unroll
  for (int i = 0; i < kWinWords / 4; i++) q[i] = src[i];
  // stored MSB-first (byte-swapped once here instead of at every read)
#pragma unroll
  for (int i = 0; i < kWinWords / 4; i++) {
    win[(kWinWords - 1 - 4 * i) * NT] = __builtin_bswap32(q[i].x);
    win[(kWinWords - 2 - 4 * i) * NT] = __builtin_bswap32(q[i].y);
    win[(kWinWords - 3 - 4 * i) * NT] = __builtin_bswap32(q[i].z);
    win[(kWinWords - 4 - 4 * i) * NT] = __builtin_bswap32(q[i].w);
  }
}

template <int NT>
__device__ __forceinline__ void dec_init(Dec& d, uint32_t* win, const uint32_t* words, uint32_t p,
                                         uint32_t z, uint32_t bs) {
  d.wbit = p & ~31u;  // the word holding the position: a full window of runway
  win_stage<NT>(win, words, p >> 5);
  d.pos = p;
  d.z = z;
  d.bs = bs;
}

// The 32 bits at d.pos, MSB-first.  Wave-uniform window restage: when any
// active lane is about to read past its window, every active lane restages
// from its own position, so the global load and its vmcnt wait happen once
// per ~25 symbol steps of the wave.
template <int NT>
__device__ __forceinline__ uint32_t dec_peek(Dec& d, uint32_t* win, const uint32_t* words) {
  uint32_t rel = d.pos - d.wbit;
  if (__any(rel >= 32u * (kWinWords - 1))) {
    d.wbit = d.pos & ~31u;
    win_stage<NT>(win, words, d.pos >> 5);
    rel = d.pos - d.wbit;
  }
  // (the window is stored in reverse word order, so the pair lands in a
  // register pair as (lo, hi) = (word w + 1, word w), ready for one shift)
  const uint32_t* pw = win + (kWinWords - 2 - (int)(rel >> 5)) * NT;
  const uint64_t lohi = (uint64_t)pw[0] | ((uint64_t)pw[NT] << 32);
  return (uint32_t)((lohi << (rel & 31u)) >> 32);
}

__device__ __forceinline__ void dec_skip(Dec& d, uint32_t nbits) { d.pos += nbits; }

// Three window words from the one holding d.pos, as the pairs (w0, w1) and
// (w1, w2) (hi word first): bits [pos, pos + 64) for two symbol steps from one
// window read.  Returns the bit offset of pos in w0.
template <int NT>
__device__ __forceinline__ uint32_t dec_peek3(Dec& d, uint32_t* win, const uint32_t* words,
                                              uint64_t& p01, uint64_t& p12) {
  uint32_t rel = d.pos - d.wbit;
  if (__any(rel >= 32u * (kWinWords - 2))) {
    d.wbit = d.pos & ~31u;
    win_stage<NT>(win, words, d.pos >> 5);
    rel = d.pos - d.wbit;
  }
  const uint32_t* pw = win + (kWinWords - 3 - (int)(rel >> 5)) * NT;
  const uint32_t w2 = pw[0], w1 = pw[NT], w0 = pw[2 * NT];
  p01 = (uint64_t)w1 | ((uint64_t)w0 << 32);
  p12 = (uint64_t)w2 | ((uint64_t)w1 << 32);
  return rel & 31u;
}

// The second step's 32 bits: (hi, lo) are the 64 bits at pos, the first step
// took nbits of them -- every entry takes 1..31 bits (an invalid code's one),
// so the funnel shift's count 32 - nbits is in 1..31.
__device__ __forceinline__ uint32_t win_next(uint32_t hi, uint32_t lo, uint32_t nbits) {
  return __builtin_amdgcn_alignbit(hi, lo, 32u - nbits);
}

// the LDS table of the next symbol, and the block-in-MCU advance at a block end
__device__ __forceinline__ uint32_t tab_slot(const TabMap& m, const Dec& d, bool is_dc) {
  return __builtin_amdgcn_ubfe(is_dc ? m.dmap : m.amap, d.bs, 3);
}
__device__ __forceinline__ uint32_t next_bs(const TabMap& m, uint32_t bs) {
  return bs + 3u == m.bs_end ? 0u : bs + 3u;
}
// decode_state and decode_write count the block-in-MCU downwards while they
// run (Dec::bs = bs_end - 3 - 3b there, flipped on entry and on return; the
// maps packed in reverse): the advance is a subtract and an unsigned min --
// below 0 it wraps past every bound, to the MCU's first block.
__device__ __forceinline__ void hot_flip(const TabMap& m, Dec& d) { d.bs = m.bs_end - 3u - d.bs; }
__device__ __forceinline__ uint32_t hot_tab(const TabMap& m, const Dec& d, bool is_dc) {
  return __builtin_amdgcn_ubfe(is_dc ? m.rdmap : m.ramap, d.bs, 3);
}
__device__ __forceinline__ uint32_t hot_next(const TabMap& m, uint32_t bs) {
  return min(bs - 3u, m.bs_end - 3u);
}

// Canonical decode of a code that is not fully resolved by the LUT (longer
// than kLutBits, or a DC size > 15): returns a kKindCode entry, 0 if invalid.
template <class SH>
__device__ __attribute__((noinline)) uint32_t slow_symbol(const SH& S, int t, uint32_t hi,
                                                          bool is_dc) {
  const bool g = t >= SH::kTabs;
  const HuffTable* G = g ? S.gtab + S.gslot[t] : nullptr;
  const int tl = g ? 0 : t;
  const uint32_t w16 = hi >> 16;
  for (int l = 1; l <= 16; l++) {
    const int code = (int)(w16 >> (16 - l));
    if (code <= (g ? G->maxcode[l] : S.maxcode[tl][l])) {
      const int sym = g ? G->vals[G->valoff[l] + code] : S.vals[tl][S.valoff[tl][l] + code];
      if (is_dc && sym > 15) return 1;
      return hj_entry(kKindCode, l, sym, is_dc, 0);
    }
  }
  return 1;
}

// The entry of the symbol at the head of `hi` in table slot t (two-level LUT,
// canonical fallback); 0 = invalid code.
// SLOW = false: every table's long codes are in LDS sub-tables, so a Slow
// entry is 0 (invalid code) and the canonical fallback is not needed.
template <bool SLOW, class SH>
__device__ __forceinline__ uint32_t lookup(const SH& S, uint32_t t, uint32_t hi, bool is_dc) {
  if constexpr (SLOW) {
    if (t >= (uint32_t)SH::kTabs) {  // a table past the LDS slots: its HBM copy
      const HuffTable& G = S.gtab[S.gslot[t]];
      uint32_t e = G.lut[hi >> (32 - kLutBits)];
      if (((e >> 5) & 3) == kKindSub)
        e = G.sub[((e >> kEntHiShift) << kSubBits) |
                  ((hi >> (32 - kLutBits - kSubBits)) & ((1u << kSubBits) - 1))];
      if (((e >> 5) & 3) == kKindSlow) e = slow_symbol(S, (int)t, hi, is_dc);
      return e;
    }
  }
  uint32_t e = S.lut[t][hi >> (32 - kLutBits)];
  if constexpr (!SLOW) {
    // both levels read back to back (the second address from the bits and
    // the slot, not from the first entry), one LDS latency per symbol
    // instead of two whenever any lane of the wave has a long code:
    // slot t's share of the pool, the sub-table at its level-1 index modulo
    // the share (entropy_image's table load): slot bits above nine stream bits
    const uint32_t a2 = (t << kSubShareBits) | ((hi >> 16) & (uint32_t)(kSubShare - 1));
    const uint32_t e2 = S.sub[a2];
    return e == kSubMark ? e2 : e;
  }
  if (((e >> 5) & 3) == kKindSub)
    e = S.sub[((e >> kEntHiShift) << kSubBits) |
              ((hi >> (32 - kLutBits - kSubBits)) & ((1u << kSubBits) - 1))];
  if constexpr (SLOW) {
    if (((e >> 5) & 3) == kKindSlow) e = slow_symbol(S, (int)t, hi, is_dc);
  }
  return e;
}

// lookup() without the canonical fallback: an entry of kind Slow comes back
// as it is (the chain walk's lane lookups decode every bit offset of a
// window, most of them no symbol start, and leave the rare Slow symbol that
// the walk actually meets to one uniform lookup())
template <bool SLOW, class SH>
__device__ __forceinline__ uint32_t lookup_fast(const SH& S, uint32_t t, uint32_t hi) {
  if constexpr (SLOW) {
    if (t >= (uint32_t)SH::kTabs) {
      const HuffTable& G = S.gtab[S.gslot[t]];
      uint32_t e = G.lut[hi >> (32 - kLutBits)];
      if (((e >> 5) & 3) == kKindSub)
        e = G.sub[((e >> kEntHiShift) << kSubBits) |
                  ((hi >> (32 - kLutBits - kSubBits)) & ((1u << kSubBits) - 1))];
      return e;
    }
    uint32_t e = S.lut[t][hi >> (32 - kLutBits)];
    if (((e >> 5) & 3) == kKindSub)
      e = S.sub[((e >> kEntHiShift) << kSubBits) |
                ((hi >> (32 - kLutBits - kSubBits)) & ((1u << kSubBits) - 1))];
    return e;
  } else {
    return lookup<false>(S, t, hi, false);
  }
}

// State-only decode of every symbol that starts in [d.pos, end): bit
// position, z and block-in-MCU advance and the number of blocks started --
// no stores and no coefficient values (DC predictors are resolved after the
// write pass), so the loop carries no memory traffic besides the bit window.
// Total over any bit position: an invalid code (entry 0) consumes one bit, a
// run past coefficient 63 ends the block, so every start state has one
// trajectory.  One path for DC and AC (selects, not branches: the 64 lanes of
// a wave decode 64 unrelated streams).  Returns the blocks started.
template <int NT, bool SLOW, class SH>
__device__ int decode_state(const SH& S, Dec& d, uint32_t* win, const uint32_t* words,
                            const TabMap& m, const uint32_t end) {
  // blocks started = blocks ended + (a block open at the end) - (one open at
  // the start): counting ends is one add per step
  int nend = 0;
  const int open0 = d.z != 0u;
  hot_flip(m, d);
  // two symbol steps per window read (a step takes <= 31 bits, so both lie in
  // the three words from the one holding pos): the second step's LUT read
  // waits for the first entry only, not for another window read
  while (d.pos < end) {
    uint64_t p01, p12;
    const uint32_t r = dec_peek3<NT>(d, win, words, p01, p12);
    uint32_t nbits;
    const uint32_t hi0 = (uint32_t)((p01 << r) >> 32), lo0 = (uint32_t)((p12 << r) >> 32);
    {
      const uint32_t z = d.z;
      const uint32_t t = hot_tab(m, d, z == 0u);
      const uint32_t e = lookup<SLOW>(S, t, hi0, z == 0u);
      // an invalid code's entry (1) takes one bit, advances nothing and
      // starts no block
      nbits = e & 31u;  // code + value bits, <= 31
      dec_skip(d, nbits);
      const uint32_t zn = z + __builtin_amdgcn_ubfe(e, 12, 7);
      const bool bend = zn >= 64u;
      nend += bend ? 1 : 0;
      const uint32_t bsn = hot_next(m, d.bs);
      d.z = bend ? 0u : zn;
      d.bs = bend ? bsn : d.bs;
    }
    {
      const bool more = d.pos < end;
      const uint32_t hi = win_next(hi0, lo0, nbits);
      const uint32_t z = d.z;
      const uint32_t t = hot_tab(m, d, z == 0u);
      // past the end: the null entry (no bits, no advance, so no block end)
      // in place of the symbol's -- one select instead of three masked results
      const uint32_t es = lookup<SLOW>(S, t, hi, z == 0u);
      const uint32_t e = more ? es : 0u;
      dec_skip(d, e & 31u);
      const uint32_t zn = z + __builtin_amdgcn_ubfe(e, 12, 7);
      const bool bend = zn >= 64u;
      nend += bend ? 1 : 0;
      const uint32_t bsn = hot_next(m, d.bs);
      d.z = bend ? 0u : zn;
      d.bs = bend ? bsn : d.bs;
    }
  }
  hot_flip(m, d);
  return nend + (d.z != 0u ? 1 : 0) - open0;
}

// The block in progress at a run's synchronised start belongs to the run
// its DC symbol lies in (that run finishes it past its own slots): skip the
// rest of it, state only, bounded by the segment end.
template <int NT, bool SLOW, class SH>
__device__ void skip_open_block(const SH& S, Dec& d, uint32_t* win, const uint32_t* words,
                                const TabMap& m, const uint32_t seg_end) {
  while (d.z != 0u && d.pos < seg_end) {
    const uint32_t hi = dec_peek<NT>(d, win, words);
    const uint32_t z = d.z;
    const uint32_t e = lookup<SLOW>(S, tab_slot(m, d, false), hi, false);
    const uint32_t nbits = e & 31u;
    dec_skip(d, nbits);
    const uint32_t zn = z + __builtin_amdgcn_ubfe(e, 12, 7);
    const bool bend = zn >= 64u;
    const uint32_t bsn = next_bs(m, d.bs);
    d.z = bend ? 0u : zn;
    d.bs = bend ? bsn : d.bs;
  }
}

// Coefficient lists, the write pass's output (read by idct_kernel): block j
// of an image keeps its non-zero AC coefficients, dequantised (the int16
// product the sequential decoder stores), as u32 entries (value << 16 |
// IDCT slot, kSlotOrder) in ents[bd.x, bd.x + (bd.y & 0xFFFF)), bd = bdesc[j];
// bd.y >> 16 holds the block's raw DC difference until the DC pass replaces
// it by the final dequantised DC.  Each block is written by the one run its DC
// symbol lies in, entries appended from that run's region start (first block
// * 64; a block has at most 63 AC entries; the run's lists follow each other back to back),
// so no buffer needs clearing and nothing is scattered: HBM sees ~4 bytes per
// non-zero coefficient.

// The symbol's value: the entry's own (Full) plus the sz value bits that
// follow the code (Code), JPEG EXTEND -- a field whose top bit is clear is
// negative, raw - (2^sz - 1).  (sz = 0: the top-bit extract reads bit 31 of
// raw, which is 0, and the mask is empty.)
__device__ __forceinline__ int sym_value(uint32_t e, uint32_t hi, uint32_t nbits, uint32_t sz) {
  const uint32_t raw = __builtin_amdgcn_ubfe(hi, 32u - nbits, sz);
  const uint32_t top = (uint32_t)__builtin_amdgcn_sbfe((int)raw, sz - 1u, 1);  // ~0: positive
  const uint32_t neg = ~top & ((1u << sz) - 1u);
  return ((int32_t)e >> kEntHiShift) + (int)(raw - neg);
}

struct BlockOut {
  uint32_t* ents;
  uint2* bdesc;
  uint32_t cur;   // next entry
  uint32_t last;  // the image's last entry (a clamp that keeps a failed scan's stores in place)
  uint32_t nblk;  // the image's blocks: descriptor stores past them are dropped
  uint32_t bstart;  // first entry of the open block
  int dcv;          // its DC difference
  bool open;        // a block of this run is being decoded
  uint32_t pk[4];   // the last four entries (a shift register: pk[3] the newest)
#if HJ_OWN_CHECK
  int lo, hi;       // the run's blocks by the block scan, [lo, hi)
  uint32_t viol;    // descriptor stores outside them
#endif
#if HJ_ABLATIONS
  bool no_list, no_desc;  // store-site ablations (write-traffic accounting)
#endif
};

// entry e at o.cur when `put` (the caller advances o.cur): shifted into pk,
// and the group of four leaves as one 16-byte store when it completes
__device__ __forceinline__ void put_entry(BlockOut& o, uint32_t e, bool put) {
  o.pk[0] = put ? o.pk[1] : o.pk[0];
  o.pk[1] = put ? o.pk[2] : o.pk[1];
  o.pk[2] = put ? o.pk[3] : o.pk[2];
  o.pk[3] = put ? e : o.pk[3];
#if HJ_ABLATIONS
  if (o.no_list) return;
#endif
  if (put && (o.cur & 3u) == 3u) {
    const uint32_t base = min(o.cur & ~3u, o.last & ~3u);
    *reinterpret_cast<uint4*>(o.ents + base) = make_uint4(o.pk[0], o.pk[1], o.pk[2], o.pk[3]);
  }
}

// a run's lists go back to back: the next list continues the current group,
// so a block end stores nothing but its descriptor (the run's last, partial
// group leaves in flush_tail)
// (a block index past the image -- a run counting blocks in trailing garbage
// or a failed scan -- is dropped: the next image's descriptors follow)
__device__ __forceinline__ void close_block(BlockOut& o, int blk) {
#if HJ_ABLATIONS
  if (o.no_desc) blk = -1;
#endif
  if ((uint32_t)blk < o.nblk) {
#if HJ_OWN_CHECK
    o.viol += (blk < o.lo || blk >= o.hi) ? 1u : 0u;
#endif
    o.bdesc[blk] = make_uint2(o.bstart, (o.cur - o.bstart) | ((uint32_t)o.dcv << 16));
  }
  o.open = false;
}

// the run's last r = cur & 3 entries, pk[4 - r .. 3], to the group at cur & ~3
__device__ __forceinline__ void flush_tail(BlockOut& o) {
  const uint32_t r = o.cur & 3u;
  if (r == 0u) return;
#if HJ_ABLATIONS
  if (o.no_list) return;
#endif
  const uint32_t base = min(o.cur & ~3u, o.last & ~3u);
  // (masks, not selects: a select chain over pk becomes a dynamic index
  // and puts the BlockOut in scratch)
  const uint32_t m1 = 0u - (uint32_t)(r == 1u), m2 = 0u - (uint32_t)(r == 2u);
  const uint32_t m3 = ~(m1 | m2);
  uint4 q;
  q.x = (o.pk[3] & m1) | (o.pk[2] & m2) | (o.pk[1] & m3);
  q.y = (o.pk[3] & m2) | (o.pk[2] & m3);
  q.z = o.pk[3];
  q.w = 0u;
  *reinterpret_cast<uint4*>(o.ents + base) = q;
}

// Full decode from a synchronised state (z == 0: at a block start) of the
// blocks whose DC symbol starts before `end`, each to its end (past `end` if
// needed); the sequential decoder's stop / error rules of the segment (blocks
// [.., seg_end_blk), scan bits [.., seg_end)) -- oracle jo_decode_coefs.  nb =
// blocks started so far (absolute).  Returns the status; sets `done` once the
// segment's last block is complete.
template <int NT, bool SLOW, class SH>
__device__ int decode_write(const SH& S, Dec& d, uint32_t* win, const uint32_t* words,
                            const TabMap& m, const uint32_t end, const uint32_t seg_end,
                            const int seg_end_blk, BlockOut& o, int& nb, bool& done) {
  int rc = kOk;
  hot_flip(m, d);
  // Fast path, straight-line: a symbol that can trigger none of the rules
  // below -- a valid code, no run past coefficient 63, not within 32 bits of
  // the segment end, not a DC symbol once the segment's last block started
  // -- is decoded without them.  A lane leaves at the first symbol that
  // could, before consuming it, and the careful loop continues from that
  // state.  (In the fast path a block is open exactly while z != 0.)
  const int nb_entry = nb;
  // one fast-path step on the 32 bits `hi` at d.pos: false (nothing
  // consumed) when the symbol could trigger a rule
  auto fast_step = [&](const uint32_t hi) -> bool {
    const uint32_t z = d.z;
    const bool is_dc = z == 0;
    const uint32_t e = lookup<SLOW>(S, hot_tab(m, d, is_dc), hi, is_dc);
    const uint32_t sz = __builtin_amdgcn_ubfe(e, 7, 5);
    const uint32_t nbits = e & 31u;
    const uint32_t zn = z + __builtin_amdgcn_ubfe(e, 12, 7);
    // One unsigned test for the three rules: the entry's flag bits bound the
    // z its symbol may reach (hj_common.h) -- 64 a coefficient (none past
    // 63), 128 an EOB / ZRL (zn <= 127: any), 0 an invalid code or an AC
    // size-0 symbol other than these (zn - 1 wraps for the invalid code at z
    // = 0, which advances nothing).
    const uint32_t lim = (e >> 13) & 0xC0u;
    const bool coef = lim == 64u;
    if (zn - 1u >= lim) return false;
    const int v = sym_value(e, hi, nbits, sz);
    dec_skip(d, nbits);
    const bool ac = coef & !is_dc;
    put_entry(o, (uint32_t)v << 16 | (zn - 1u), ac);  // (zn <= 64 for a coefficient)
    o.cur += ac ? 1u : 0u;
    o.bstart = is_dc ? o.cur : o.bstart;
    o.dcv = is_dc ? v : o.dcv;
    nb += is_dc ? 1 : 0;
    const bool bend = zn >= 64u;
    if (bend) close_block(o, nb - 1);
    const uint32_t bsn = hot_next(m, d.bs);
    d.z = bend ? 0u : zn;
    d.bs = bend ? bsn : d.bs;
    return true;
  };
  // (pos + 32 > seg_end as one compare with a bound made once: pos >= seg_end - 31)
  const uint32_t near_end = seg_end >= 31u ? seg_end - 31u : 0u;
  auto fast_stop = [&]() -> bool {
    const bool is_dc = d.z == 0u;
    return (is_dc & ((d.pos >= end) | (nb >= seg_end_blk))) | (d.pos >= near_end);
  };
  // two steps per window read (as decode_state)
  for (;;) {
    if (fast_stop()) break;
    uint64_t p01, p12;
    const uint32_t r = dec_peek3<NT>(d, win, words, p01, p12);
    const uint32_t pos0 = d.pos;
    const uint32_t hi0 = (uint32_t)((p01 << r) >> 32), lo0 = (uint32_t)((p12 << r) >> 32);
    if (!fast_step(hi0)) break;
    if (fast_stop()) break;
    if (!fast_step(win_next(hi0, lo0, d.pos - pos0))) break;  // (a step taken took >= 1 bit)
  }
  // a block in progress is this run's only if the fast path started it (a
  // run that entered inside the previous run's block -- skip_open_block
  // stopped at the segment end -- owns nothing yet)
  o.open = d.z != 0u && nb > nb_entry;
  while (!done && rc == kOk && !(d.z == 0u && d.pos >= end)) {
    const uint32_t hi = dec_peek<NT>(d, win, words);
    const uint32_t z = d.z;
    const bool is_dc = z == 0;
    const uint32_t e = lookup<SLOW>(S, hot_tab(m, d, is_dc), hi, is_dc);
    const bool valid = (e & 0x60u) != 0u;
    const uint32_t sz = __builtin_amdgcn_ubfe(e, 7, 5);
    const uint32_t nbits = e & 31u;
    const int v = sym_value(e, hi, nbits, sz);
    dec_skip(d, nbits);
    const uint32_t zinc = __builtin_amdgcn_ubfe(e, 12, 7);
    const bool coef = valid && ((e >> 19) & 1u);
    // (the rejected AC size-0 symbol: valid with neither flag bit, hj_common.h)
    const bool refused = (e & 0x180000u) == 0u;
    const bool bad = !valid || (coef && z + zinc > 64u) || refused;
    // The sequential decoder's rules, branch-free (the lanes of a wave sit
    // at unrelated symbols): it stops at the segment's last block and never
    // reads what follows; anything else that is invalid is an error.
    const bool past_a = nb > seg_end_blk || (nb == seg_end_blk && z == 0u);
    const bool good = coef && !bad;
    const bool stop = good && (is_dc ? nb : nb - 1) >= seg_end_blk;
    const bool wr = good && !stop;
    const uint32_t zn = valid ? z + zinc : z;
    if (wr && is_dc) {
      o.bstart = o.cur;
      o.dcv = v;
      o.open = true;
    }
    const bool put = wr && !is_dc;
    put_entry(o, (uint32_t)v << 16 | ((zn - 1u) & 63u), put);
    o.cur += put ? 1u : 0u;
    nb += (wr && is_dc) ? 1 : 0;
    // a symbol running past the segment end (after the rule above)
    const bool trunc = !bad && !stop && d.pos > seg_end;
    const bool past_b = nb > seg_end_blk || (nb == seg_end_blk && z == 0u);
    done = (bad && past_a) || stop || (trunc && past_b);
    rc = (bad && !past_a) ? kErrBadHuffman : ((trunc && !past_b) ? kErrTruncated : kOk);
    const bool bend = zn >= 64u;
    if (bend && !stop && o.open) close_block(o, nb - 1);
    const uint32_t bsn = hot_next(m, d.bs);
    d.z = bend ? 0u : zn;
    d.bs = bend ? bsn : d.bs;
  }
  // the segment ended (or failed) inside a block: keep what it decoded
  if (o.open && d.z != 0u) close_block(o, nb - 1);
  hot_flip(m, d);
  return rc;
}

// Segmented inclusive scan over the workgroup's runs (Hillis-Steele): a run
// with `flag` set restarts the sums.  Results in S.sc.scan_v[tid][0, NV).
template <int NT, int NV, class SH>
__device__ void seg_scan(SH& S, int tid, int flag, const int (&v)[kMaxComp]) {
  S.sc.scan_flag[tid] = flag;
#pragma unroll
  for (int i = 0; i < NV; i++) S.sc.scan_v[tid][i] = v[i];
  __syncthreads();
  for (int off = 1; off < NT; off <<= 1) {
    int pf = 0, pv[NV];
    const bool take = tid >= off;
#pragma unroll
    for (int i = 0; i < NV; i++) pv[i] = take ? S.sc.scan_v[tid - off][i] : 0;
    if (take) pf = S.sc.scan_flag[tid - off];
    __syncthreads();
    if (take && !S.sc.scan_flag[tid]) {
#pragma unroll
      for (int i = 0; i < NV; i++) S.sc.scan_v[tid][i] += pv[i];
      S.sc.scan_flag[tid] = pf;
    }
    __syncthreads();
  }
}

// ---- piece hand-off (hj_common.h EntChain): 8-byte {tag, value} granules,
// each written by ONE agent-scope relaxed (sc1, write-through) store and read
// by agent-scope relaxed (sc1) loads, so a granule is its own flag -- no
// fences (MI355X_MICROARCH.md, hand-off R2).  Every wait is bounded.
typedef __attribute__((address_space(1))) unsigned long long hj_gu64;
__device__ __forceinline__ void gran_put(uint64_t* c, int i, uint32_t tag, uint32_t v) {
  __hip_atomic_store((hj_gu64*)(c + i), ((unsigned long long)tag << 32) | v, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t gran_get(const uint64_t* c, int i) {
  return __hip_atomic_load((hj_gu64*)(c + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Bounded waits, counted in polling time without progress (wall_clock64
// ticks, 100 MHz).  The clock runs on while the queue's waves are switched
// out (CWSR: the GPU shared with another process), so a gap between two polls
// longer than kPollGapTicks is not waiting time; and any new granule among
// those awaited restarts the count.  So only a wait that polled `limit`
// ticks with nothing arriving gives up -- never a slow or preempted
// predecessor (pieces take tickets in order: every awaited piece is running,
// and piece 0 waits for nobody).  A wait that gives up fails its image with
// kErrHandoff, which the host re-decodes in one workgroup (no hand-off).
constexpr int64_t kPollGapTicks = 100000;  // 1 ms
struct WaitBound {
  int64_t last, idle;
  int sig;
};
__device__ __forceinline__ WaitBound wait_begin() { return WaitBound{wall_clock64(), 0, -1}; }
// sig: a wave-uniform count of the awaited granules present (grows with progress)
__device__ __forceinline__ bool wait_expired(WaitBound& w, int sig, int64_t limit) {
  const int64_t now = wall_clock64(), dt = now - w.last;
  w.last = now;
  if (sig != w.sig) {
    w.sig = sig;
    w.idle = 0;
    return false;
  }
  if (dt < kPollGapTicks) w.idle += dt;
  return w.idle >= limit;
}

// A piece that cannot take part (failed image, bad restart count, a hand-off
// that gave up): every granule it would publish carries kTagFail, so the
// pieces waiting for it stop waiting and fail the image too.
__device__ __forceinline__ void chain_fail(uint64_t* rec, int tid) {
  if (tid < kChainGranules) gran_put(rec, tid, kTagFail, 0u);
}

// Look-back of piece p (> 0), wave 0: the end state and block count of piece
// p - 1 as the sequential decoder sees them.  Lane l reads piece q = p-1-l.
// The base is the nearest piece with its final record (rec2; piece 0 posts
// one at once); from it the fold walks up through the pieces' own records
// (rec1) while each one's guessed start equals the state handed to it (an
// empty piece passes the state on); a piece whose guess was wrong has to post
// its own rec2 first.  -> S.left_pos / left_zb / lb_blocks, S.lb_ok.
template <class SH>
__device__ void chain_lookback(SH& S, const uint64_t* chain, int p, int lane, int64_t limit) {
  const uint64_t* rec = chain + (int64_t)(p - 1 - lane) * kChainGranules;
  const bool mine = lane < p;
  WaitBound wb = wait_begin();
  for (;;) {
    uint64_t r[8] = {};
    if (mine) {
#pragma unroll
      for (int i = 0; i < 8; i++) r[i] = gran_get(rec, i);
    }
    bool fail = false, has1 = mine, has2 = mine;
    int present = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint32_t tag = (uint32_t)(r[i] >> 32);
      fail |= tag == kTagFail;
      present += __popcll(__ballot(tag != 0u));
      if (i < 5) has1 = has1 && tag == kTagRec1;
      else has2 = has2 && tag == kTagRec2;
    }
    if (__any(fail)) {
      if (lane == 0) S.lb_ok = -1;
      return;
    }
    const uint64_t m2 = __ballot(has2), m1 = __ballot(has1);
    if (m2 != 0) {
      const int lb = __builtin_ctzll(m2);
      const uint64_t below = (1ull << lb) - 1ull;
      if ((m1 & below) == below) {
        uint32_t e0 = __shfl((uint32_t)r[kChE0], lb), e1 = __shfl((uint32_t)r[kChE1], lb);
        int32_t b = (int32_t)__shfl((uint32_t)r[kChB], lb);
        bool ok = true;
        for (int l = lb - 1; l >= 0; l--) {  // wave-uniform fold
          const uint32_t g0 = __shfl((uint32_t)r[kChG0], l), g1 = __shfl((uint32_t)r[kChG1], l);
          if (g1 == 0xFFFFFFFFu) continue;  // an empty piece
          if (g0 != e0 || g1 != e1) {
            ok = false;  // started from a wrong guess: wait for its final record
            break;
          }
          e0 = __shfl((uint32_t)r[kChL0], l);
          e1 = __shfl((uint32_t)r[kChL1], l);
          b += (int32_t)__shfl((uint32_t)r[kChT], l);
        }
        if (ok) {
          if (lane == 0) {
            S.left_pos = e0;
            S.left_zb = e1;
            S.lb_blocks = b;
            S.lb_ok = 1;
          }
          return;
        }
      }
    }
    if (wait_expired(wb, present, limit)) {
      if (lane == 0) S.lb_ok = -2;  // gave up
      return;
    }
    __builtin_amdgcn_s_sleep(4);
  }
}

// DC predictors entering piece p: the sum of the DC-difference sums of
// pieces 0 .. p-1 (one restart-free segment: no resets), wave 0.
template <class SH>
__device__ void chain_dc(SH& S, const uint64_t* chain, int p, int lane, int64_t limit) {
  const uint64_t* rec = chain + (int64_t)lane * kChainGranules + kChDc;
  const bool mine = lane < p;
  WaitBound wb = wait_begin();
  for (;;) {
    uint64_t r[kMaxComp] = {};
    bool fail = false, have = true;
    int got = 0;
    if (mine) {
#pragma unroll
      for (int i = 0; i < kMaxComp; i++) {
        r[i] = gran_get(rec, i);
        const uint32_t tag = (uint32_t)(r[i] >> 32);
        fail |= tag == kTagFail;
        have = have && tag == kTagDc;
        got += tag != 0u ? 1 : 0;
      }
    }
    if (__any(fail)) {
      if (lane == 0) S.lb_ok = -1;
      return;
    }
    if (__all(have)) {
#pragma unroll
      for (int i = 0; i < kMaxComp; i++) {
        int32_t v = (int32_t)(uint32_t)r[i];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) S.lb_dc[i] = v;
      }
      if (lane == 0) S.lb_ok = 1;
      return;
    }
    int present = got;
    for (int o = 32; o > 0; o >>= 1) present += __shfl_xor(present, o);
    if (wait_expired(wb, present, limit)) {
      if (lane == 0) S.lb_ok = -2;  // gave up
      return;
    }
    __builtin_amdgcn_s_sleep(4);
  }
}

// Slot geometry of one chunk of restart segments (entropy_image's slot_*
// lambdas, for code outside it)
struct SlotGeo {
  const uint32_t* sg;  // segment start bytes
  int seg_lo, cmax, nseg_found;
  uint32_t N, clean_len;
  __device__ uint32_t seg_start(int s) const { return sg[s] * 8u; }
  __device__ uint32_t seg_end(int s) const {
    return (s + 1 < nseg_found ? sg[s + 1] : clean_len) * 8u;
  }
  __device__ int seg(int k) const { return seg_lo + k / cmax; }
  __device__ int j(int k) const { return k % cmax; }
  __device__ uint32_t start(int k) const { return seg_start(seg(k)) + (uint32_t)j(k) * N; }
  __device__ uint32_t end(int k) const {
    const uint32_t a = start(k) + N, e = seg_end(seg(k));
    return a < e ? a : e;
  }
  __device__ bool empty(int k) const { return j(k) > 0 && start(k) >= seg_end(seg(k)); }
  __device__ bool known(int k) const { return j(k) == 0; }
};

// One chain of a chain round (entropy_image's chain_round): the wave decodes
// from the true end state of run h - 1 through the slots of runs h, h + 1,
// ... until the trajectory meets a recorded slot state, a segment start, or
// the next head nh's first slot, rewriting the slot records (sst) and run end
// states it passes -- decode_state's semantics symbol for symbol.  Lane l
// looks up the symbol at bit l of a 64-bit window (the current block's AC
// table; lane 0 the DC table at a block start); the wave walks the symbols
// with v_readlane.  (Out of line: the rare path keeps its registers out of
// the decode loops' budget.)
template <int NT, bool kSlow, class SH>
__device__ __forceinline__ void chain_sweep(SH& S, uint4* sst, const uint32_t* __restrict__ words,
                                         TabMap tm, SlotGeo geo, int K, int pc, int nslots,
                                         int h, int nh, const int lane, const int wave) {
  // every scalar in SGPRs (a value the compiler cannot prove uniform would
  // make the whole walk divergent in its eyes)
  auto rfli = [](int v) { return (int)rfl((uint32_t)v); };
  auto rflp = [](const uint32_t* p) {
    const uint64_t a = (uint64_t)(uintptr_t)p;
    return (const uint32_t*)(uintptr_t)((uint64_t)rfl((uint32_t)a) |
                                        (uint64_t)rfl((uint32_t)(a >> 32)) << 32);
  };
  K = rfli(K);
  pc = rfli(pc);
  nslots = rfli(nslots);
  h = rfli(h);
  nh = rfli(nh);
  tm.dmap = rfl(tm.dmap);
  tm.amap = rfl(tm.amap);
  tm.bs_end = rfl(tm.bs_end);
  geo.sg = rflp(geo.sg);
  geo.seg_lo = rfli(geo.seg_lo);
  geo.cmax = rfli(geo.cmax);
  geo.nseg_found = rfli(geo.nseg_found);
  geo.N = rfl(geo.N);
  geo.clean_len = rfl(geo.clean_len);
  words = rflp(words);
  auto run_first = [&](int u) { return min((pc * NT + u) * K, nslots); };
  uint32_t* cw = &S.win[0][0] + wave * (kWinWords * 64);  // this wave's chunk of the stream
  constexpr uint32_t kChunkBits = kWinWords * 64 * 32;
  const uint32_t nwords = (geo.clean_len + 3u) / 4u;
  const int kstop = run_first(nh);  // (nh == NT: the end of this workgroup's slots)
  const int kh = run_first(h);
  uint32_t pos = __builtin_amdgcn_readfirstlane(h > 0 ? S.run_pos[h - 1] : S.left_pos);
  const uint32_t zb_in = __builtin_amdgcn_readfirstlane(h > 0 ? S.run_zb[h - 1] : S.left_zb);
  uint32_t z = zb_in & 0xFFu, bs = zb_in >> 8;
  uint32_t cbit = 0xFFFFFFFFu;  // first bit of the staged chunk (none yet)
  // lane l, for the symbol at window bit l: the window bit of the next
  // symbol (nx) and the coefficient-index advance (zi); the walk's
  // dependency chain is one v_readlane of nx per symbol
  uint32_t nx = 0, zi = 0;
  uint32_t wb = 0;  // the window's first bit
  uint32_t o = 64;  // pos's bit in the window (>= 64: refill)
  // lane lookups of the window starting at pos: the AC table of block-in-MCU
  // bs, but lane 0 takes the DC table when the block's DC symbol is next
  // (z == 0): a window is refilled at every block start
  auto fill = [&]() {
    if (cbit == 0xFFFFFFFFu || pos - cbit + 96u > kChunkBits) {
      cbit = pos & ~31u;
      const uint32_t w0 = cbit >> 5;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      // (four words in flight per lane: this rare path must not raise the
      // kernel's register count)
#pragma unroll 1
      for (int i = 0; i < kWinWords; i += 4) {
        uint32_t q[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint32_t wi = w0 + (uint32_t)((i + j) * 64 + lane);
          q[j] = words[min(wi, nwords + 1u)];
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint32_t wi = w0 + (uint32_t)((i + j) * 64 + lane);
          cw[(i + j) * 64 + lane] = wi < nwords + 2u ? __builtin_bswap32(q[j]) : 0u;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    const uint32_t r = pos - cbit + (uint32_t)lane;
    const uint64_t pr = ((uint64_t)cw[r >> 5] << 32) | cw[(r >> 5) + 1];
    const uint32_t hi = (uint32_t)((pr << (r & 31u)) >> 32);
    const bool dc = lane == 0 && z == 0u;
    const uint32_t e =
        lookup_fast<kSlow>(S, __builtin_amdgcn_ubfe(dc ? tm.dmap : tm.amap, bs, 3), hi);
    // a Slow entry (a code the LDS tables do not resolve): nx = 128 + l makes
    // the walk stop there with o >= 128, and the symbol takes lookup()
    const bool slow = ((e >> 5) & 3u) == kKindSlow;
    nx = slow ? 128u + (uint32_t)lane : (uint32_t)lane + (e & 31u);
    zi = slow ? 0u : __builtin_amdgcn_ubfe(e, 12, 7);
    wb = pos;
    o = 0;
  };
  pos = rfl(pos);
  z = rfl(z);
  bs = rfl(bs);
  const uint32_t pos_in = pos;
  int u = h;  // the run whose slots are being decoded
  int cseg = -1;
  uint32_t seg_s = 0, seg_e = 0;
  // slot k + 1's recorded state, loaded a slot ahead (the merge test)
  uint4 qn = kh + 1 < kstop ? sst[kh + 1] : make_uint4(0u, 0u, 0u, 0u);
  for (int k = kh; k < kstop; k++) {
    const int sk = geo.seg(k), jk = geo.j(k);
    if (jk == 0) break;  // a segment start: its state is known
    if (sk != cseg) {
      cseg = sk;
      seg_s = rfl(geo.seg_start(sk));
      seg_e = rfl(geo.seg_end(sk));
    }
    const uint32_t st = seg_s + (uint32_t)jk * geo.N;
    if (st >= seg_e) break;  // an empty slot past the segment's bits
    const uint32_t zb0 = z | (bs << 8);
    const uint4 q = qn;
    if (k + 1 < kstop) qn = sst[k + 1];
    if (k > kh && rfl(q.x) == pos && rfl(q.y) == zb0) break;  // met the recorded trajectory
    const uint32_t p0 = pos, end = rfl(min(st + geo.N, seg_e));
    int nend = 0;
    while (pos < end) {
      if (o >= 64u) fill();
      // symbols until a block ends, the slot ends or the window runs out:
      // o <- nx[o] (one v_readlane on the chain), z += zi[o] beside it
      const uint32_t lim = rfl(min(end - wb, 64u));
      uint32_t be, t;
      asm volatile(
          "s_nop 4\n\t"  // (o may come from a VALU write: lane-select hazard)
          "s_mov_b32 %[be], 0\n"
          "1:\n\t"
          "v_readlane_b32 %[t], %[zi], %[o]\n\t"
          "v_readlane_b32 %[o], %[nx], %[o]\n\t"
          "s_add_u32 %[z], %[z], %[t]\n\t"
          "s_cmp_gt_u32 %[z], 63\n\t"
          "s_cbranch_scc1 3f\n\t"
          "s_cmp_lt_u32 %[o], %[lim]\n\t"
          "s_cbranch_scc1 1b\n\t"
          "s_branch 2f\n"
          "3:\n\t"
          "s_mov_b32 %[be], 1\n"
          "2:"
          : [o] "+s"(o), [z] "+s"(z), [be] "=&s"(be), [t] "=&s"(t)
          : [nx] "v"(nx), [zi] "v"(zi), [lim] "s"(lim)
          : "scc");
      if (o >= 128u) {  // a Slow symbol at window bit o - 128: the full lookup
        pos = wb + (o - 128u);
        const uint32_t r = pos - cbit;
        const uint64_t pr = ((uint64_t)cw[r >> 5] << 32) | cw[(r >> 5) + 1];
        const uint32_t hi = (uint32_t)((pr << (r & 31u)) >> 32);
        const bool isdc = z == 0u;
        const uint32_t e =
            rfl(lookup<kSlow>(S, __builtin_amdgcn_ubfe(isdc ? tm.dmap : tm.amap, bs, 3), hi, isdc));
        pos += e & 31u;
        const uint32_t zn = z + __builtin_amdgcn_ubfe(e, 12, 7);
        if (zn >= 64u) {
          nend++;
          bs = next_bs(tm, bs);
          z = 0u;
        } else {
          z = zn;
        }
        o = 64u;  // refill at the next symbol
        continue;
      }
      pos = wb + o;
      if (be) {  // a block ended: the next one's tables
        nend++;
        bs = next_bs(tm, bs);
        z = 0u;
        o = 64u;
      }
    }
    if (lane == 0)
      sst[k] = make_uint4(p0, zb0,
                          (uint32_t)(nend + (z != 0u ? 1 : 0) - ((zb0 & 0xFFu) != 0u ? 1 : 0)), z);
    if (k + 1 == min(run_first(u) + K, nslots)) {  // the end of run u
      if (lane == 0) {
        S.run_pos[u] = pos;
        S.run_zb[u] = z | (bs << 8);
      }
      u++;
    }
  }
  if (lane == 0) {
    atomicAdd(&S.chain_bits, pos - pos_in);
    atomicAdd(&S.chain_sweeps, 1u);
  }
}

// One image's scan, decoded by the whole workgroup.  kSlow: the scan has
// more distinct tables than LDS slots, or long codes outside the LDS
// sub-table pool (parse_kernel's ent_wide): lookups may go to HBM copies
// and the canonical fallback.
// (always inlined: as a real call the kernel takes the call ABI's register
// budget -- 248 VGPRs and scratch instead of ~100)
template <int NT, int NTAB, bool kSlow>
__device__ __forceinline__ void entropy_image(EntShared<NT, NTAB>& S, const int img,
                              const uint8_t* __restrict__ clean, const uint32_t* __restrict__ segs,
                              const ImageDesc* __restrict__ desc, ImageInfo* __restrict__ infos,
                              const HuffTable* __restrict__ luts, uint32_t* __restrict__ ents,
                              uint2* __restrict__ bdesc, uint32_t* __restrict__ recs,
                              uint64_t* __restrict__ chain, const int piece,
                              const EntropyParams ep) {
  const int tid = threadIdx.x;
  const int ablate = HJ_ABLATIONS ? ep.ablate : 0;  // (release builds: no tests, no live SGPR)
  uint32_t* win = &S.win[0][tid];
  const ImageDesc dd = desc[img];
  const ImageInfo& in = infos[img];
  // pieces of this image (hj_common.h): crec = piece 0's hand-off record
  const int P = max(1, dd.pieces);
  uint64_t* crec = chain + kChainHead + dd.chain_off;
  uint64_t* myrec = crec + (int64_t)piece * kChainGranules;
  // (the status is read once, by one lane: another piece of this image may
  // write it while this one starts)
  if (tid == 0) S.flag = (in.status != kOk || in.multiscan) ? 1 : 0;
  __syncthreads();
  if (S.flag) {
    if (P > 1) chain_fail(myrec, tid);
    return;
  }
  // The NTAB = 4 instance takes the images whose scan uses <= 4 distinct
  // tables with every long code in sub-tables that fit the LDS pool (no
  // canonical fallback in its loops); the NTAB = 6 instance takes the rest.
  const int bpm = in.bpm, ri = in.ri, nmcu = in.mcux * in.mcuy;
  const int nblocks = in.nblocks;
  const uint32_t* words = reinterpret_cast<const uint32_t*>(clean + dd.in_off);
  const uint32_t* sg = segs + dd.seg_off;
  const int clean_len = in.clean_len;
  const int nseg_found = in.nseg;
  const int nseg = ri > 0 ? (nmcu + ri - 1) / ri : 1;

  // ---- tables into LDS (dedup table slots per component) ----
  // table slots and components per block-in-MCU (TabMap); the DC pass
  // keeps a 2-bit component map
  uint32_t bcomp = 0;  // 2-bit component per block-in-MCU (DC pass)
  TabMap tm{};
  {
    int slots[kMaxTabs], ns = 0, ldc[kMaxComp] = {}, lac[kMaxComp] = {};
    for (int c = 0; c < in.ncomp; c++) {
      const int want[2] = {in.dc_tab[c], 4 + in.ac_tab[c]};
      for (int k = 0; k < 2; k++) {
        int f = -1;
        for (int i = 0; i < ns; i++)
          if (slots[i] == want[k]) f = i;
        if (f < 0) {
          f = ns;
          slots[ns++] = want[k];
        }
        (k == 0 ? ldc : lac)[c] = f;
      }
    }
    if (tid == 0) S.gtab = luts;
    int pool = 0;  // in units of 64-entry sub-tables
    for (int i = 0; i < ns; i++) {
      const int ref = in.lut_ref[slots[i]];  // the batch's build of this table (lut_kernel)
      if (i >= NTAB) {  // kept in HBM (kSlow images only)
        if (tid == 0) S.gslot[i] = ref;
        continue;
      }
      const HuffTable& T = luts[ref];
      const int nsub = T.nsub;
      // the LDS-only loops (lookup<false>): slot i's sub-tables in its share
      // of the pool, each at its level-1 index modulo the share -- they are
      // consecutive level-1 cells and parse_kernel sent a table with more of
      // them than the share holds to the wide path, so no two collide
      constexpr bool kShared = !kSlow;
      const bool fits = kShared ? nsub << kSubBits <= kSubShare
                                : (pool + nsub) << kSubBits <= kSubPool;
      const int base = pool;
      if (fits && !kShared) pool += nsub;
      for (int k = tid; k < kLutSize; k += NT) {
        uint32_t e = T.lut[k];
        if ((e >> 5 & 3) == kKindSub) {
          if (!fits) e = 1u;
          else if (kShared) e = kSubMark;
          else e += (uint32_t)base << kEntHiShift;
        }
        S.lut[i][k] = e;
      }
      if (fits && kShared) {
        for (int k = tid; k < nsub << kSubBits; k += NT)
          S.sub[(i << kSubShareBits) + (((T.sub_lo << kSubBits) + k) & (kSubShare - 1))] = T.sub[k];
      } else if (fits) {
        for (int k = tid; k < nsub << kSubBits; k += NT)
          S.sub[(base << kSubBits) + k] = T.sub[k];
      }
      if (tid < 18) S.maxcode[i][tid] = T.maxcode[tid];
      if (tid < 17) S.valoff[i][tid] = T.valoff[tid];
      for (int k = tid; k < 256; k += NT) S.vals[i][k] = T.vals[k];
    }
    if (tid < kMaxComp) S.qdc[tid] = in.qt[tid][0];
    for (int b = 0; b < bpm; b++) {
      const int c = in.mcu_comp[b];
      bcomp |= (uint32_t)c << (2 * b);
      tm.dmap |= (uint32_t)ldc[c] << (3 * b);
      tm.amap |= (uint32_t)lac[c] << (3 * b);
      tm.cmap |= (uint32_t)c << (3 * b);
      tm.rdmap |= (uint32_t)ldc[c] << (3 * (bpm - 1 - b));
      tm.ramap |= (uint32_t)lac[c] << (3 * (bpm - 1 - b));
    }
    tm.bs_end = 3u * (uint32_t)bpm;
    if (tid == 0) {
      S.err = kOk;
      S.chain_bits = 0;
      S.chain_sweeps = 0;
#if HJ_OWN_CHECK
      S.own_viol = 0;
#endif
    }
  }
  if (nseg_found < nseg) {
    if (tid == 0) infos[img].status = kErrBadRestart;
    if (P > 1) chain_fail(myrec, tid);
    return;
  }
  __syncthreads();

  // ---- the image's pieces: restart segments split over P workgroups, or
  // one restart-free segment decoded as one workgroup of P x NT runs, its
  // run states, block counts and DC sums handed across pieces ----
  const bool chained = P > 1 && ri == 0;
  const int seg_a = (P > 1 && !chained) ? (int)((int64_t)piece * nseg / P) : 0;
  const int seg_b = (P > 1 && !chained) ? (int)((int64_t)(piece + 1) * nseg / P) : nseg;
  const int pc = chained ? piece : 0;  // this workgroup's share of the run space
  const int nruns = chained ? P * NT : NT;
  const uint32_t budget = (uint32_t)kMaxSlots * (chained ? P : 1);

  auto seg_start_bits = [&](int s) -> uint32_t { return sg[s] * 8u; };
  auto seg_end_bits = [&](int s) -> uint32_t {
    return (s + 1 < nseg_found ? sg[s + 1] : (uint32_t)clean_len) * 8u;
  };

  // ---- subsequence size: keep every segment within kMaxSlots slots ----
  uint32_t maxbits = 0;
  for (int s = tid; s < nseg; s += NT) {
    const uint32_t a = seg_start_bits(s), e = seg_end_bits(s);
    maxbits = max(maxbits, e > a ? e - a : 0u);
  }
  S.sc.red[tid] = (int32_t)maxbits;
  __syncthreads();
  for (int off = NT / 2; off > 0; off >>= 1) {
    if (tid < off) S.sc.red[tid] = max(S.sc.red[tid], S.sc.red[tid + off]);
    __syncthreads();
  }
  maxbits = (uint32_t)S.sc.red[0];
  __syncthreads();
  const uint32_t N = slot_bits(maxbits, ep.sub_bits, budget);
  if ((int64_t)kMaxSlots * 8 * P > dd.rec_cap) {  // host-sized slot state
    if (tid == 0) infos[img].status = kErrBadGeometry;
    if (P > 1) chain_fail(myrec, tid);
    return;
  }
  const int cmax = max(1, (int)((maxbits + N - 1) / N));
  const int seg_per_chunk = max(1, (int)(budget / (uint32_t)cmax));
  uint32_t* ents_img = ents + (size_t)dd.coef_off * 64;
  uint2* bdesc_img = bdesc + dd.coef_off;
  // per-slot state, one uint4 per slot: {start pos, start z | bs << 8, blocks
  // started, end z}; each slot is only ever touched by the thread that owns it
  uint4* sst = reinterpret_cast<uint4*>(recs + dd.rec_off) +
              (chained ? 0 : (size_t)piece * kMaxSlots * 2);
  auto seg_first_blk = [&](int s) { return ri > 0 ? s * ri * bpm : 0; };
  auto seg_end_blk = [&](int s) { return ri > 0 ? min((s + 1) * ri, nmcu) * bpm : nblocks; };
  int rounds_total = 0;
  int64_t tph[4] = {0, 0, 0, 0}, dcfix = 0, chain_ticks = 0;
  int64_t tstamp = wall_clock64();

  for (int seg_lo = seg_a; seg_lo < seg_b; seg_lo += seg_per_chunk) {
    const int nsc = min(seg_per_chunk, seg_b - seg_lo);
    const int nslots = nsc * cmax;
    const int K = max((nslots + nruns - 1) / nruns, ep.min_run_slots);
    const int r0 = min((pc * NT + tid) * K, nslots), r1 = min(r0 + K, nslots);
    auto slot_seg = [&](int k) { return seg_lo + k / cmax; };
    auto slot_j = [&](int k) { return k % cmax; };
    auto slot_start = [&](int k) { return seg_start_bits(slot_seg(k)) + (uint32_t)slot_j(k) * N; };
    auto slot_end = [&](int k) {
      const uint32_t a = slot_start(k) + N, e = seg_end_bits(slot_seg(k));
      return a < e ? a : e;
    };
    auto slot_empty = [&](int k) {
      return slot_j(k) > 0 && slot_start(k) >= seg_end_bits(slot_seg(k));
    };
    auto slot_known = [&](int k) { return slot_j(k) == 0; };
    auto decode_k = [&](Dec& d, int k) {
      const uint32_t p0 = d.pos, zb0 = d.z | (d.bs << 8);
      const int nblk = decode_state<NT, kSlow>(S, d, win, words, tm, slot_end(k));
      sst[k] = make_uint4(p0, zb0, (uint32_t)nblk, d.z);
    };

    // ---- round 0: every run from a guess at its first slot ----
    {
      Dec d;
      d.pos = 0;
      d.z = d.bs = 0;
      bool have = false;
      // the run's slots, one segment piece at a time: [k, k2] = its slots
      // in segment s that hold bits
      for (int k = r0; k < r1;) {
        const int s = slot_seg(k);
        const uint32_t s0 = seg_start_bits(s), se = seg_end_bits(s);
        const int jlast = se > s0 ? (int)((se - s0 - 1) / N) : 0;
        const int k2 = min(r1 - 1, (s - seg_lo) * cmax + jlast);
        if (k > k2) {  // past the segment's bits: empty slots
          have = false;
          k = min(r1, (s - seg_lo + 1) * cmax);
          continue;
        }
        const uint32_t ss = s0 + (uint32_t)slot_j(k) * N;
        if (slot_known(k)) {
          dec_init<NT>(d, win, words, ss, 0, 0);
        } else if (!have) {
          // warm-up: guess a state warm_slots slots earlier (or take the
          // segment start, which is exact) and decode up to the slot, so the
          // run's first state is usually already synchronised and the sync
          // rounds below have short chains to settle
          const uint32_t wb = (uint32_t)ep.warm_slots * N;
          dec_init<NT>(d, win, words, ss - s0 > wb ? ss - wb : s0, 0, 0);
          decode_state<NT, kSlow>(S, d, win, words, tm, ss);
        }
        // one decode_state call per slot (measured: a single loop over the
        // piece that records each slot as it crosses the boundary ran 20 %
        // slower than these per-slot loops), the slot ends precomputed
        for (uint32_t kk = k, be = ss + N; (int)kk <= k2; kk++, be += N) {
          const uint32_t p0 = d.pos, zb0 = d.z | (d.bs << 8);
          const int nblk = decode_state<NT, kSlow>(S, d, win, words, tm, min(be, se));
          sst[kk] = make_uint4(p0, zb0, (uint32_t)nblk, d.z);
        }
        have = true;
        k = k2 + 1;
      }
      S.run_pos[tid] = d.pos;
      S.run_zb[tid] = (have && r0 < r1) ? (d.z | (d.bs << 8)) : 0xFFFFFFFFu;
    }
    __syncthreads();
    {
      const int64_t t = wall_clock64();
      tph[0] += t - tstamp;
      tstamp = t;
    }
    // ---- sync rounds: re-decode a run from its left neighbour's end state
    // until the trajectory merges with the stored one at a slot boundary.
    // Run 0's left neighbour is S.left (none, except for a later piece once
    // the previous piece's end state is known) ----
    if (tid == 0) {
      S.left_pos = 0;
      S.left_zb = 0xFFFFFFFFu;
    }
    // ---- chain rounds.  A run whose recorded start state disagrees with its
    // left neighbour's end state is re-decoded by the sync rounds; when the
    // guessed trajectories stay out of phase for many runs (high-quality
    // scans with optimised tables: the block-in-MCU phase is lost for tens of
    // kbit), the true state walks one run per round, each round one run's
    // decode long.  A chain round instead decodes each chain serially from its
    // head (a run to re-decode whose left neighbour is not), through the
    // following runs' slots -- rewriting their slot records and end states --
    // until the trajectory meets a recorded slot state or the next head.  One
    // wave decodes a chain cooperatively: lane l looks up the symbol at bit
    // offset l of a 64-bit window (the current block's DC and AC tables), and
    // the wave walks the symbol chain with v_readlane, so a symbol costs a
    // readlane and a few scalar operations instead of a lane's full step;
    // a block end or the window's end refills the lookups.  The semantics are
    // decode_state's, symbol for symbol; the sync round that follows checks
    // every run again.
    auto chain_round = [&]() {
      const int64_t tc0 = wall_clock64();
      // (wave-uniform in the compiler's eyes too: the chain decode keeps its
      // state in SGPRs)
      const int lane = tid & 63, wave = (int)rfl((uint32_t)(tid >> 6));
      constexpr int kNW = NT / 64;
      bool redo = false;
      if ((tid > 0 || S.left_zb != 0xFFFFFFFFu) && r0 < r1 && !slot_known(r0) &&
          !slot_empty(r0)) {
        const uint32_t npos = tid > 0 ? S.run_pos[tid - 1] : S.left_pos;
        const uint32_t nzb = tid > 0 ? S.run_zb[tid - 1] : S.left_zb;
        if (nzb != 0xFFFFFFFFu) {
          const uint4 q = sst[r0];
          redo = npos != q.x || nzb != q.y;
        }
      }
      const uint64_t rm = __ballot(redo);
      if (lane == 0) S.cmask[wave] = rm;
      __syncthreads();
      if (lane == 0) {
        const uint64_t carry = wave > 0 ? S.cmask[wave - 1] >> 63 : 0ull;
        S.hmask[wave] = rm & ~((rm << 1) | carry);
      }
      __syncthreads();
      const SlotGeo geo{sg, seg_lo, cmax, nseg_found, N, (uint32_t)clean_len};
      int ord = 0;  // heads are dealt to the waves in order
      for (int w = 0; w < kNW; w++) {
        uint64_t hm = S.hmask[w];
        hm = (uint64_t)rfl((uint32_t)hm) | (uint64_t)rfl((uint32_t)(hm >> 32)) << 32;
        while (hm) {
          const int h = w * 64 + __builtin_ctzll(hm);
          hm &= hm - 1ull;
          if (ord++ % kNW != wave) continue;
          // the next head: where this chain's decode stops at the latest
          int nh = NT;
          {
            uint64_t rest = hm;
            for (int w2 = w; w2 < kNW && nh == NT; w2++) {
              if (w2 > w) {
                rest = S.hmask[w2];
                rest = (uint64_t)rfl((uint32_t)rest) | (uint64_t)rfl((uint32_t)(rest >> 32)) << 32;
              }
              if (rest) nh = w2 * 64 + __builtin_ctzll(rest);
            }
          }
          chain_sweep<NT, kSlow>(S, sst, words, tm, geo, K, pc, nslots, h, nh, lane, wave);
        }
      }
      __syncthreads();
      chain_ticks += wall_clock64() - tc0;
    };
    auto sync_rounds = [&]() -> int {
      int rounds = 0;
      for (; !(ablate & kAblEntSync);) {
        if (ep.chain_after > 0 && rounds >= ep.chain_after) chain_round();
        if (tid == 0) S.flag = 0;
        __syncthreads();
        bool redo = false;
        uint32_t npos = 0, nzb = 0;
        if ((tid > 0 || S.left_zb != 0xFFFFFFFFu) && r0 < r1 && !slot_known(r0) &&
            !slot_empty(r0)) {
          npos = tid > 0 ? S.run_pos[tid - 1] : S.left_pos;
          nzb = tid > 0 ? S.run_zb[tid - 1] : S.left_zb;
          if (nzb != 0xFFFFFFFFu) {
            const uint4 q = sst[r0];
            redo = npos != q.x || nzb != q.y;
          }
        }
        __syncthreads();
        if (redo) {
          Dec d;
          dec_init<NT>(d, win, words, npos, nzb & 0xFF, nzb >> 8);
          bool merged = false;
          for (int k = r0; k < r1; k++) {
            if (slot_empty(k) || slot_known(k)) {
              merged = true;
              break;
            }
            const uint32_t zb = d.z | (d.bs << 8);
            if (k > r0) {
              const uint4 q = sst[k];
              if (q.x == d.pos && q.y == zb) {
                merged = true;
                break;
              }
            }
            decode_k(d, k);
          }
          if (!merged) {
            const uint32_t zb = d.z | (d.bs << 8);
            if (S.run_pos[tid] != d.pos || S.run_zb[tid] != zb) {
              S.run_pos[tid] = d.pos;
              S.run_zb[tid] = zb;
              S.flag = 1;
            }
          }
        }
        __syncthreads();
        const int again = S.flag;
        rounds++;
        __syncthreads();
        if (!again || rounds > NT + 2) break;
      }
      return rounds;
    };
    // ---- per-run block totals, then a segmented inclusive scan over runs:
    // the block index before (nb) and after (run_end_blk) each run, and the
    // workgroup's total ----
    int nb = 0, run_end_blk = 0, blk_total = 0;
    auto block_scan = [&]() {
      int flag = 0, v[kMaxComp] = {};
      for (int k = r0; k < r1; k++) {
        if (slot_empty(k)) continue;
        if (slot_known(k)) {
          flag = 1;
          v[0] = seg_first_blk(slot_seg(k));
        }
        v[0] += (int)sst[k].z;
      }
      seg_scan<NT, 1>(S, tid, flag, v);
      // the scan scratch shares LDS with the bit windows: take this thread's
      // values before anything restages windows
      nb = tid > 0 ? S.sc.scan_v[tid - 1][0] : 0;
      run_end_blk = S.sc.scan_v[tid][0];
      blk_total = S.sc.scan_v[NT - 1][0];
      __syncthreads();
    };
    // Chained pieces: pass 0 decodes from this piece's own guess and posts
    // it (rec1); a later piece then looks back for the previous piece's end
    // state and, if its first run guessed wrong, runs pass 1 from the handed
    // state.  (One call site each for the sync rounds and the block scan: the
    // loops are inlined once.)
    const int busy_runs = (int)(((int64_t)nslots + K - 1) / K);  // runs holding slots
    const int t_last = min(NT - 1, busy_runs - 1 - pc * NT);     // < 0: an empty piece
    for (int pass = 0;; pass++) {
      rounds_total += sync_rounds();
      if (pass == 0) {
        const int64_t t = wall_clock64();
        tph[1] += t - tstamp;
        tstamp = t;
      }
      block_scan();
      if (!chained || pass > 0) break;
      if (tid == 0) {
        uint32_t g0 = 0u, g1 = 0xFFFFFFFFu, l0 = 0u, l1 = 0u;
        if (t_last >= 0) {
          const uint4 q = sst[r0];
          g0 = q.x;
          g1 = q.y;
          l0 = S.run_pos[t_last];
          l1 = S.run_zb[t_last];
        }
        gran_put(myrec, kChG0, kTagRec1, g0);
        gran_put(myrec, kChG1, kTagRec1, g1);
        gran_put(myrec, kChL0, kTagRec1, l0);
        gran_put(myrec, kChL1, kTagRec1, l1);
        gran_put(myrec, kChT, kTagRec1, (uint32_t)blk_total);
        if (pc == 0) {  // the first piece starts at the segment start: final at once
          gran_put(myrec, kChE0, kTagRec2, l0);
          gran_put(myrec, kChE1, kTagRec2, l1);
          gran_put(myrec, kChB, kTagRec2, (uint32_t)blk_total);
        }
        S.lb_ok = 1;
        S.lb_blocks = 0;
      }
      if (pc == 0) break;
      // the previous piece's end state and block count as the sequential
      // decoder sees them
      if (tid < 64) chain_lookback(S, crec, pc, tid, ep.handoff_ticks);
      __syncthreads();
      const int ok = S.lb_ok;
      if (ok < 0) {
        if (tid == 0 && ok == -2) infos[img].status = kErrHandoff;
        chain_fail(myrec, tid);
        return;
      }
      // run 0 started from a wrong guess: the sync rounds again from the
      // handed state (usually a short re-decode until it merges)
      if (tid == 0) {
        bool wrong = false;
        if (t_last >= 0) {
          const uint4 q = sst[r0];
          wrong = q.x != S.left_pos || q.y != S.left_zb;
        }
        S.flag = wrong ? 1 : 0;
      }
      __syncthreads();
      const bool resync = S.flag != 0;
      __syncthreads();  // (sync_rounds rewrites S.flag)
      if (!resync) break;
    }
    if (chained) {
      if (pc > 0 && tid == 0) {  // rec2: final
        const bool empty = t_last < 0;
        gran_put(myrec, kChE0, kTagRec2, empty ? S.left_pos : S.run_pos[t_last]);
        gran_put(myrec, kChE1, kTagRec2, empty ? S.left_zb : S.run_zb[t_last]);
        gran_put(myrec, kChB, kTagRec2, (uint32_t)(S.lb_blocks + blk_total));
      }
      __syncthreads();
      nb += S.lb_blocks;
      run_end_blk += S.lb_blocks;
    }
    {
      const int64_t t = wall_clock64();
      tph[2] += t - tstamp;
      tstamp = t;
    }
    // This run's blocks [b0, b1): those whose DC symbol lies in the run --
    // from its first slot's segment start (or the predecessor's end) to its
    // count end, clamped to its last segment's end (symbols decoded from the
    // fill bits after a segment's last block are not blocks).  The ranges of
    // the runs are disjoint and cover every block of a well-formed scan.
    int b0 = 0, b1 = 0;
    {
      int k0 = r0;
      while (k0 < r1 && slot_empty(k0)) k0++;
      if (k0 < r1) {
        b0 = max(0, slot_known(k0) ? seg_first_blk(slot_seg(k0)) : nb);
        b1 = min(min(run_end_blk, seg_end_blk(slot_seg(r1 - 1))), nblocks);
      }
    }
    // (timing ablations: a later piece still needs this one's DC record)
    if ((ablate & (kAblEntWrite | kAblEntDc)) && chained && tid < kMaxComp)
      gran_put(myrec, kChDc + tid, kTagDc, 0u);
    if (ablate & kAblEntWrite) continue;
    // ---- write pass: decode each run once more from its synchronised
    // start, appending its blocks' coefficient lists; the sequential decoder's
    // stop and error rules per segment ----
    {
      int rc = kOk;
      bool done = false;  // the segment's last block is complete
      bool have = false;  // the decoder holds this run's state
      BlockOut o;
      o.ents = ents_img;
      o.bdesc = bdesc_img;
      o.cur = (uint32_t)b0 * 64u;
      o.last = (uint32_t)nblocks * 64u - 1u;
      o.nblk = (uint32_t)nblocks;
      // The store bases and bounds are uniform, and the kernel has no scalar
      // register left for them: kept there, each store of the write step
      // fetched them back from spill lanes (v_readlane + wait states).  As
      // vector registers they cost the step nothing.
      asm volatile("" : "+v"(o.ents), "+v"(o.bdesc), "+v"(o.last), "+v"(o.nblk));
#if HJ_ABLATIONS
      o.no_list = (ablate & kAblEntList) != 0;
      o.no_desc = (ablate & kAblEntDesc) != 0;
#endif
      o.bstart = o.cur;
      o.dcv = 0;
      o.open = false;
#if HJ_OWN_CHECK
      o.lo = b0;
      o.hi = b1;
      o.viol = 0u;
#endif
#pragma unroll
      for (uint32_t i = 0; i < 4; i++) o.pk[i] = 0u;
      Dec d;
      // one decode_write call per segment piece of the run (its slots [k,
      // k2] in segment s that hold bits), to the piece's end
      for (int k = r0; k < r1 && rc == kOk;) {
        const int s = slot_seg(k);
        const uint32_t s0 = seg_start_bits(s), se = seg_end_bits(s);
        const int jlast = se > s0 ? (int)((se - s0 - 1) / N) : 0;
        const int k2 = min(r1 - 1, (s - seg_lo) * cmax + jlast);
        if (k > k2) {  // past the segment's bits: empty slots
          have = false;
          k = min(r1, (s - seg_lo + 1) * cmax);
          continue;
        }
        if (slot_known(k)) {
          nb = seg_first_blk(s);
          done = false;
          dec_init<NT>(d, win, words, s0, 0, 0);
          have = true;
        } else if (!have) {
          const uint4 q = sst[k];
          dec_init<NT>(d, win, words, q.x, q.y & 0xFF, q.y >> 8);
          skip_open_block<NT, kSlow>(S, d, win, words, tm, se);
          have = true;
        }
        if (!done) {
          const int seb = seg_end_blk(s);
          const uint32_t pend = min(s0 + (uint32_t)(slot_j(k2) + 1) * N, se);
          rc = decode_write<NT, kSlow>(S, d, win, words, tm, pend, se, seb, o, nb, done);
          // the piece ends its segment: every block of the segment must be done
          const bool last = (k2 + 1 >= nslots) || slot_j(k2 + 1) == 0 || pend >= se;
          if (rc == kOk && !done && last && (nb < seb || (nb == seb && d.z != 0)))
            rc = kErrTruncated;
        }
        k = k2 + 1;
      }
      flush_tail(o);
#if HJ_OWN_CHECK
      if (o.viol) atomicAdd(&S.own_viol, o.viol);
#endif
      if (rc != kOk) atomicCAS(&S.err, kOk, rc);
    }
    __syncthreads();
    {
      const int64_t t = wall_clock64();
      tph[3] += t - tstamp;
      tstamp = t;
    }
    if (ablate & kAblEntDc) continue;
    // ---- DC predictors: the write pass stored raw DC differences.  Sum them
    // per component over this run's blocks, segmented-scan the sums over the
    // runs (predictors restart at each restart segment), then replace each
    // difference by clip(bias + q * predictor) -- oracle jo_decode_coefs ----
    {
      const int rblk = ri > 0 ? ri * bpm : 0x7FFFFFFF;
      const int first_reset = ri > 0 ? (b0 + rblk - 1) / rblk * rblk : 0x7FFFFFFF;
      const int bs0 = b0 % bpm;
      // (selects over the components, not a dynamically indexed array: that
      // would live in scratch)
      int v[kMaxComp] = {}, flag = 0;
      // (blocks in groups of kG: the group's descriptor loads are issued
      // back to back, so one memory latency is exposed per group)
      constexpr int kG = 8;
      {
        int bs = bs0, reset = first_reset;
        for (int b = b0; b < b1; b += kG) {
          uint32_t ys[kG];
#pragma unroll
          for (int g = 0; g < kG; g++) ys[g] = bdesc_img[min(b + g, b1 - 1)].y;
#pragma unroll
          for (int g = 0; g < kG; g++) {
            if (b + g >= b1) break;
            if (b + g == reset) {
              flag = 1;
#pragma unroll
              for (int i = 0; i < kMaxComp; i++) v[i] = 0;
              reset += rblk;
            }
            const uint32_t c = __builtin_amdgcn_ubfe(bcomp, 2u * (uint32_t)bs, 2);
            const int dv = (int32_t)ys[g] >> 16;
#pragma unroll
            for (int i = 0; i < kMaxComp; i++) v[i] += c == (uint32_t)i ? dv : 0;
            bs = bs + 1 == bpm ? 0 : bs + 1;
          }
        }
      }
      seg_scan<NT, kMaxComp>(S, tid, flag, v);
      int pr[kMaxComp] = {};
      if (tid > 0) {
#pragma unroll
        for (int i = 0; i < kMaxComp; i++) pr[i] = S.sc.scan_v[tid - 1][i];
      }
      if (chained && tid < kMaxComp)  // this piece's DC sums (no restarts: no resets)
        gran_put(myrec, kChDc + tid, kTagDc, (uint32_t)S.sc.scan_v[NT - 1][tid]);
      __syncthreads();
      if (chained && pc > 0) {
        // the predictors entering this piece: the sums of all earlier pieces
        if (tid < 64) chain_dc(S, crec, pc, tid, ep.handoff_ticks);
        __syncthreads();
        const int ok = S.lb_ok;
        if (ok < 0) {
          if (tid == 0 && ok == -2) infos[img].status = kErrHandoff;
          return;  // (this piece's records are all posted)
        }
#pragma unroll
        for (int i = 0; i < kMaxComp; i++) pr[i] += S.lb_dc[i];
      }
      int bs = bs0, reset = first_reset;
      for (int b = b0; b < b1; b += kG) {
        uint32_t ys[kG];
#pragma unroll
        for (int g = 0; g < kG; g++) ys[g] = bdesc_img[min(b + g, b1 - 1)].y;
#pragma unroll
        for (int g = 0; g < kG; g++) {
          if (b + g >= b1) break;
          if (b + g == reset) {
#pragma unroll
            for (int i = 0; i < kMaxComp; i++) pr[i] = 0;
            reset += rblk;
          }
          const uint32_t c = __builtin_amdgcn_ubfe(bcomp, 2u * (uint32_t)bs, 2);
          const uint32_t by = ys[g];
          int cur = (int32_t)by >> 16;
#pragma unroll
          for (int i = 0; i < kMaxComp; i++) cur += c == (uint32_t)i ? pr[i] : 0;
#pragma unroll
          for (int i = 0; i < kMaxComp; i++) pr[i] = c == (uint32_t)i ? cur : pr[i];
          const uint32_t q = S.qdc[c];
          const int32_t dqi = (int32_t)((uint32_t)kDcBias + q * (uint32_t)cur);
          const int32_t dc = dqi < -32768 ? -32768 : (dqi > 32767 ? 32767 : dqi);
          bdesc_img[b + g].y = (by & 0xFFFFu) | ((uint32_t)dc << 16);
          bs = bs + 1 == bpm ? 0 : bs + 1;
        }
      }
    }
    {
      const int64_t t = wall_clock64();
      dcfix += t - tstamp;
      tstamp = t;
    }
  }
  if (tid == 0 && S.err != kOk && !ablate) infos[img].status = S.err;
  if (tid == 0 && piece == 0) {
    infos[img].sync_rounds = rounds_total;
    for (int i = 0; i < 4; i++) infos[img].tphase[i] = tph[i];
    for (int i = 0; i < 4; i++) infos[img].dbg[i] = 0;
    infos[img].dbg[0] = dcfix;  // DC predictor pass (ticks)
    // chain rounds (ticks, inside the sync phase) | chains decoded << 24
    infos[img].dbg[1] = chain_ticks | ((int64_t)S.chain_sweeps << 24);
    infos[img].dbg[2] = S.chain_bits;  // bits they decoded (summed over the chains)
#if HJ_OWN_CHECK
    infos[img].dbg[3] = S.own_viol;
#endif
  }
}

// One workgroup per work item: an image, or a piece of a large one
// (hj_common.h).  Items are taken in ticket order (a device-scope counter
// that parse_kernel zeroed), so a piece waits only for pieces of lower
// tickets, which are already running: no dependence on dispatch order.  The
// common scan (<= 4 distinct tables, every long code in the LDS sub-table
// pool) runs the LDS-only decode loops; a wide one (parse_kernel's ent_wide)
// the loops that may read HBM table copies and the canonical fallback.
template <int NT, int NTAB>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(NT >= 256 ? 4 : 1)))
entropy_kernel(const uint8_t* __restrict__ clean, const uint32_t* __restrict__ segs,
               const ImageDesc* __restrict__ desc, ImageInfo* __restrict__ infos,
               const HuffTable* __restrict__ luts, uint32_t* __restrict__ ents,
               uint2* __restrict__ bdesc, uint32_t* __restrict__ recs,
               const uint32_t* __restrict__ work, uint64_t* __restrict__ chain,
               const EntropyParams ep, const int nwork) {
  __shared__ EntShared<NT, NTAB> S;
  __shared__ uint32_t item;
  if (ep.prio == 3) __builtin_amdgcn_s_setprio(3);  // (the instruction takes an immediate)
  else if (ep.prio == 2) __builtin_amdgcn_s_setprio(2);
  else if (ep.prio == 1) __builtin_amdgcn_s_setprio(1);
  if (threadIdx.x == 0) {
    const uint32_t t = __hip_atomic_fetch_add((__attribute__((address_space(1))) uint32_t*)chain,
                                              1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    item = t < (uint32_t)nwork ? work[t] : 0xFFFFFFFFu;
  }
  __syncthreads();
  const uint32_t w = item;
  if (w == 0xFFFFFFFFu) return;
  const int img = (int)(w & 0xFFFFFFu), piece = (int)(w >> 24);
  if (infos[img].ent_wide)
    entropy_image<NT, NTAB, true>(S, img, clean, segs, desc, infos, luts, ents, bdesc, recs, chain,
                                  piece, ep);
  else
    entropy_image<NT, NTAB, false>(S, img, clean, segs, desc, infos, luts, ents, bdesc, recs,
                                   chain, piece, ep);
}

// ---------------------------------------------------------------------------
// multiscan_kernel: progressive (SOF2) and sequential non-interleaved JPEGs.
// One workgroup per image.  The whole workgroup finds the marker candidates
// (one coalesced pass over the file), thread 0 walks the segments and records
// every scan with its dependencies, then every wave of the workgroup is a
// scan decoder: it takes the next ready scan and decodes it wave-uniformly (a
// progressive scan's meaning depends on every earlier scan of its blocks, so
// each scan is one sequential pass; independent scans run at once; images
// run in parallel, one per CU).  Levels accumulate as int32 in the image's
// coefficient-list region, which the final pass turns into the lists
// idct_kernel reads.  Arithmetic: oracle ms_decode (jpeg_oracle.c), libjpeg
// jdphuff.c semantics, FFmpeg-style dequantisation.
//
// The decoder keeps its whole working set in registers, so that the serial
// bit chain never waits on LDS:
//   - state (bit buffer, positions, predictors, EOB run) in SGPRs;
//   - the file's bytes through scalar loads (constant address space), the
//     next dword prefetched one refill ahead;
//   - Huffman tables as VGPRs read with v_readlane at a uniform lane
//     (RTab: a 6-bit first level, the canonical limits for the rest);
//   - a block's coefficients gathered in the lanes of one VGPR (v_writelane)
//     and stored in one instruction (an AC first scan: the coded lanes);
//   - AC refinement: 64-block chunks, the blocks' non-zero masks in VGPR
//     lanes (prefetched a chunk ahead), the correction / new-coefficient
//     records written to the lanes of the decoding block, and applied by
//     the lanes (one block each) at the chunk end to levels loaded at the
//     chunk start.
// ---------------------------------------------------------------------------

constexpr int kMsPrio = 3;  // multiscan_kernel's wave priority (the A/B: where it is set)
constexpr int kMsMaxScans = 64;
constexpr int kMsMaxMarks = 512;

struct MsScan {
  int32_t ns, comp[kMaxComp], td[kMaxComp], ta[kMaxComp];
  int32_t ss, se, ah, al, ri;
  int32_t start, end;  // entropy-coded bytes [start, end) of the file
  int32_t dht[8];      // file offset of the DHT entry in effect per slot (-1: none)
};

struct MsShared {
  MsScan scan[kMsMaxScans];
  uint64_t deps[kMsMaxScans];  // earlier scans a scan must wait for (to finish)
  uint64_t soft[kMsMaxScans];  // ... or only to run ahead of it (trailing, below)
  int32_t prog[kMsMaxScans];   // blocks a scan has finished, in scan order
  int32_t prio[kMsMaxScans];   // claim priority (bytes of its heaviest dependent chain)
  int32_t dlen[kMsMaxScans];   // destuffed bytes in `clean` (-1: the stuffed reader)
  int32_t dbase[kMsMaxScans];  // their offset from the image's start (a multiple of 4)
  int32_t wtot[4], dodd;       // destuff scratch
  uint64_t claimed, done;      // scans taken by a decoder wave / finished
  int64_t tkind[4];            // diagnostics: decode ticks by scan kind
  int32_t marks[kMsMaxMarks];
  int32_t sdiag[48];                  // diagnostics (ImageInfo::sdiag)
  int32_t dht[8], comp_id[kMaxComp];  // segment walk state (thread 0)
  int32_t nmarks, nscans, err;
};

// Wave-uniform values: every LDS / global read of the decoder's inputs goes
// through readfirstlane; stores and atomics of one value come from lane 0.
__device__ __forceinline__ uint32_t ms_u(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int ms_i(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t ms_u64(uint64_t v) {
  return (uint64_t)ms_u((uint32_t)(v >> 32)) << 32 | ms_u((uint32_t)v);
}
__device__ __forceinline__ bool ms_lane0() { return __lane_id() == 0; }
// lane i of v (i uniform): v_readlane; v with lane i set to x
__device__ __forceinline__ uint32_t ms_rl(uint32_t v, int i) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, i);
}
__device__ __forceinline__ uint32_t ms_wl(uint32_t v, uint32_t x, int i) {
  return (int)__lane_id() == i ? x : v;  // v_cmp + v_cndmask
}

// An SGPR value the compiler may not re-derive (it would turn a sign test of
// the bit buffer's top word back into a 64-bit compare, which only the VALU
// has).  No instruction.
__device__ __forceinline__ void ms_opaque(uint32_t& v) { asm("" : "+s"(v)); }
__device__ __forceinline__ void ms_opaque(int& v) { asm("" : "+s"(v)); }

// The file's bytes as dwords in the constant address space: uniform loads of
// them are scalar loads (the bytes are never written while the kernel runs).
typedef const uint32_t __attribute__((address_space(4)))* MsWords;

// Bit reader over stuffed entropy data: 0xFF00 -> 0xFF; any other marker (or
// the scan end) stops the data, zeros follow (oracle bitrd_t).  Four plain
// bytes (no 0xFF among them) enter the buffer at once from two prefetched
// dwords; `fake` counts the zero bits appended past the data (the
// truncation test: more bits used than the data held).
struct MsBits {
  MsWords w;
  int size, pos, end;
  uint64_t buf;  // left-justified
  int cnt, fake;
  uint32_t n0, n1;  // dwords pos >> 2 and (pos >> 2) + 1
  bool marker;
  int lastw;  // last dword holding a byte of the file
  // dword i (clamped: never a byte past the file is used)
  __device__ __forceinline__ uint32_t word(int i) const {
    // (an unsigned 32-bit index: no 64-bit sign extension in the address)
    return w[(uint32_t)(i < lastw ? i : lastw)];
  }
  __device__ __forceinline__ uint32_t byte(int i) const {
    return (word(i >> 2) >> (8 * (i & 3))) & 0xFFu;
  }
  // dwords i, i + 1: two scalar loads, each clamped as above (and so not
  // merged into one 8-byte load, which would need 8-byte alignment to be
  // a scalar load)
  __device__ __forceinline__ void pair(int i) {
    n0 = word(i);
    n1 = word(i + 1);
  }
  __device__ __forceinline__ void start(int p, int e) {
    pos = p;
    end = e;
    buf = 0;
    cnt = 0;
    fake = 0;
    marker = false;
    pair(p >> 2);
  }
  // tops the buffer up to >= 32 bits (every step needs at most 32).  The
  // next refill's 8 bytes are loaded right after each 4-byte step, so the
  // scalar load has a few symbols' time to land.
  __device__ __forceinline__ void fill() {
    while (cnt < 32) {
      if (!marker && pos + 4 <= end) {
        const uint32_t x = (uint32_t)((((uint64_t)n1 << 32) | n0) >> (8 * (pos & 3)));
        if (((~x - 0x01010101u) & x & 0x80808080u) == 0u) {  // no 0xFF byte
          // (bswap is a VALU v_perm: back to an SGPR at once, or the whole bit
          // buffer would follow it onto the vector unit)
          buf |= (uint64_t)ms_u(__builtin_bswap32(x)) << (32 - cnt);
          cnt += 32;
          pos += 4;
          pair(pos >> 2);
          continue;
        }
      }
      uint32_t b = 0;
      if (!marker) {
        if (pos >= end) {
          marker = true;
        } else {
          const uint32_t c = byte(pos);
          if (c == 0xFFu) {
            const uint32_t nb = pos + 1 < end ? byte(pos + 1) : 0xD9u;
            if (nb == 0u) {
              pos += 2;
              b = 0xFFu;
            } else {
              marker = true;
            }
          } else {
            pos++;
            b = c;
          }
        }
        pair(pos >> 2);
      }
      if (marker) fake += 8;
      buf |= (uint64_t)b << (56 - cnt);
      cnt += 8;
    }
  }
  __device__ __forceinline__ void need();
  __device__ __forceinline__ uint32_t hi32() const { return (uint32_t)(buf >> 32); }
  __device__ __forceinline__ uint32_t peek16() const { return hi32() >> 16; }
  // the next s bits (1..16) as a JPEG signed value (F.2.2.1 EXTEND), taken;
  // the sign test on the 32-bit top word (SALU has no 64-bit signed
  // compare: a 64-bit one is a VALU v_cmp, ~40 cycles back to the scalar unit)
  __device__ __forceinline__ int take_ext(int s) {
    uint32_t h = hi32();
    ms_opaque(h);
    const int v = (int)(h >> (32 - s));
    skip(s);
    return (int32_t)h < 0 ? v : v + 1 - (1 << s);
  }
  // one bit, taken
  __device__ __forceinline__ uint32_t take_bit() {
    uint32_t h = hi32();
    ms_opaque(h);
    skip(1);
    return h >> 31;
  }
  __device__ __forceinline__ void skip(int n) {
    buf <<= n;
    cnt -= n;
  }
  // n in 1..32 bits already in the buffer
  __device__ __forceinline__ uint32_t take(int n) {
    const uint32_t v = hi32() >> (32 - n);
    skip(n);
    return v;
  }
  __device__ __forceinline__ uint32_t get(int n) {  // n in 0..32
    if (n == 0) return 0u;
    need();
    return take(n);
  }
  __device__ __forceinline__ bool truncated() const { return fake > cnt; }
};

// The bit reader's slow refill (an 0xFF byte, a marker, the scan's last
// bytes: ~2 % of refills), out of line so that the decode loops keep only
// the 4-byte step: fewer branches and register copies on the symbol path.
// (Arguments of a non-kernel function live in VGPRs: the fields come back
// through readfirstlane.)
struct MsFillState {
  uint64_t buf;
  int cnt, pos, fake, marker;
  uint32_t n0, n1;
};
__device__ __noinline__ MsFillState ms_fill_slow(MsWords w, int size, int end, int lastw,
                                                 MsFillState f) {
  MsBits b;
  b.w = w;
  b.size = size;
  b.end = end;
  b.lastw = lastw;
  b.buf = f.buf;
  b.cnt = f.cnt;
  b.pos = f.pos;
  b.fake = f.fake;
  b.marker = f.marker != 0;
  b.n0 = f.n0;
  b.n1 = f.n1;
  b.fill();
  return MsFillState{b.buf, b.cnt, b.pos, b.fake, b.marker ? 1 : 0, b.n0, b.n1};
}

__device__ __forceinline__ void MsBits::need() {
  if (__builtin_expect(cnt < 32, 0)) {
    // the common step inline (one 4-byte step always tops the buffer up)
    const uint32_t x = (uint32_t)((((uint64_t)n1 << 32) | n0) >> (8 * (pos & 3)));
    if (__builtin_expect(!marker && pos + 4 <= end && ((~x - 0x01010101u) & x & 0x80808080u) == 0u, 1)) {
      buf |= (uint64_t)ms_u(__builtin_bswap32(x)) << (32 - cnt);
      cnt += 32;
      pos += 4;
      pair(pos >> 2);
    } else {
      const MsFillState f =
          ms_fill_slow(w, size, end, lastw, MsFillState{buf, cnt, pos, fake, marker ? 1 : 0, n0, n1});
      buf = ms_u64(f.buf);
      cnt = ms_i(f.cnt);
      pos = ms_i(f.pos);
      fake = ms_i(f.fake);
      marker = ms_i(f.marker) != 0;
      n0 = ms_u(f.n0);
      n1 = ms_u(f.n1);
    }
  }
}

// Bit reader over a scan's pre-destuffed data (multiscan_kernel writes it to
// `clean` as big-endian dwords before any decoder wave starts): a refill is
// one aligned dword, loaded one refill ahead by a scalar load, with no 0xFF
// test, marker or byte swap.  Past the data it reads zeros, as the stuffed
// reader feeds zeros after a marker.  (The copy is read through the scalar
// cache, which starts each dispatch empty, only after the kernel wrote it
// and fenced: the stuffed reader's file bytes take the same path.)
struct MsWBits {
  MsWords w;
  uint64_t buf;  // left-justified
  int cnt;
  int wi, lastw;  // next dword to enter the buffer; last dword holding data
  uint32_t nxm;   // ~0 while wi <= lastw
  uint32_t nx;    // dword wi (prefetched)
  int nbits;      // bits of data
  __device__ __forceinline__ void init(const uint8_t* p, int len) {
    // (readfirstlane: the pointer is uniform, but the compiler cannot see
    // it through the destuff pass's stores and would load through VGPRs)
    w = (MsWords)(const void*)(uintptr_t)ms_u64((uint64_t)(uintptr_t)p);
    nbits = 8 * len;
    lastw = len > 0 ? (len - 1) >> 2 : 0;
    wi = 0;
    nxm = len > 0 ? ~0u : 0u;
    nx = w[0];
    buf = 0;
    cnt = 0;
  }
  __device__ __forceinline__ void need() {
    if (__builtin_expect(cnt < 32, 0)) {
      buf |= (uint64_t)(nx & nxm) << (32 - cnt);
      cnt += 32;
      wi++;
      int past = lastw - wi;  // (< 0: past the data; a sign, not a compare
      ms_opaque(past);        // result, which would go through the VALU)
      nxm = ~(uint32_t)(past >> 31);
      nx = w[(uint32_t)min(wi, lastw)];
    }
  }
  __device__ __forceinline__ uint32_t hi32() const { return (uint32_t)(buf >> 32); }
  __device__ __forceinline__ uint32_t peek16() const { return hi32() >> 16; }
  __device__ __forceinline__ int take_ext(int s) {
    uint32_t h = hi32();
    ms_opaque(h);
    const int v = (int)(h >> (32 - s));
    skip(s);
    return (int32_t)h < 0 ? v : v + 1 - (1 << s);
  }
  __device__ __forceinline__ uint32_t take_bit() {
    uint32_t h = hi32();
    ms_opaque(h);
    skip(1);
    return h >> 31;
  }
  __device__ __forceinline__ void skip(int n) {
    buf <<= n;
    cnt -= n;
  }
  __device__ __forceinline__ uint32_t take(int n) {
    const uint32_t v = hi32() >> (32 - n);
    skip(n);
    return v;
  }
  __device__ __forceinline__ uint32_t get(int n) {
    if (n == 0) return 0u;
    need();
    return take(n);
  }
  __device__ __forceinline__ bool truncated() const { return 32 * wi - cnt > nbits; }
};

template <class A, class B>
struct ms_same {
  static constexpr bool value = false;
};
template <class A>
struct ms_same<A, A> {
  static constexpr bool value = true;
};

// A Huffman table held in four VGPRs (one entry per lane):
//   l1   lane p: the code starting with the 6-bit prefix p, len | symbol << 8
//        (0: the code is longer than 6 bits)
//   lim  lane l in 1..16: sum over i <= l of bits[i] << (16 - i), i.e. the
//        first left-justified 16-bit word past the codes of length <= l
//        (monotone; ~0 on the other lanes): a word w has the code length
//        1 + #{l : lim[l] <= w} (17: invalid)
//   voff lane l: (symbols of length < l) - (first code of length l)
//   vals lane i: symbols 4i .. 4i + 3
struct RTab {
  uint32_t l1, lim, voff, vals;
};

// Builds the table of the DHT entry at file offset o (uniform); all lanes.
// Sets bad for an over-subscribed code (oracle: code > 1 << l).
__device__ __noinline__ RTab rt_build(const uint8_t* __restrict__ d, int o, int lane, bool& bad) {
  RTab t;
  const bool len_lane = lane >= 1 && lane <= 16;
  const int nb = len_lane ? d[o + lane] : 0;
  const uint32_t lim = (uint32_t)wave_incl_scan(len_lane ? nb << (16 - lane) : 0);
  const int kc = wave_incl_scan(nb);
  const int total = (int)ms_rl((uint32_t)kc, 16);
  bad = ms_rl(lim, 16) > 65536u;
  const uint32_t limp = (uint32_t)__shfl_up((int)lim, 1, 64);
  const int kp = __shfl_up(kc, 1, 64);
  t.lim = len_lane ? lim : ~0u;
  t.voff = len_lane ? (uint32_t)kp - (lane == 1 ? 0u : (limp >> (16 - lane))) : 0u;
  uint32_t v = 0;
#pragma unroll
  for (int b = 0; b < 4; b++) {
    const int i = 4 * lane + b;
    if (i < total) v |= (uint32_t)d[o + 17 + i] << (8 * b);
  }
  t.vals = v;
  // first level: lane p decodes the word p << 10
  const uint32_t w = (uint32_t)lane << 10;
  int L = 1;
#pragma unroll
  for (int l = 1; l <= 6; l++) L += ms_rl(lim, l) <= w ? 1 : 0;
  uint32_t e = 0;
  const uint32_t vo = (uint32_t)__shfl((int)t.voff, L, 64);
  if (L <= 6) {
    const uint32_t idx = vo + (w >> (16 - L));
    e = (uint32_t)L | ((uint32_t)d[o + 17 + idx] << 8);
  }
  t.l1 = e;
  return t;
}

// symbol of the code at the top of w16 (uniform), or -1; len: its length
__device__ __forceinline__ int rt_decode(const RTab& t, uint32_t w16, int& len) {
  const uint32_t e = ms_rl(t.l1, (int)(w16 >> 10));
  if (e) {
    len = (int)(e & 31u);
    return (int)(e >> 8);
  }
  int L = __popcll(__builtin_amdgcn_ballot_w64(t.lim <= w16));
  ms_opaque(L);  // (a 32-bit count, not a 64-bit compare)
  L += 1;
  if (L > 16) {
    len = 0;
    return -1;
  }
  len = L;
  const uint32_t idx = ms_rl(t.voff, L) + (w16 >> (16 - L));
  return (int)((ms_rl(t.vals, (int)(idx >> 2)) >> (8 * (idx & 3u))) & 0xFFu);
}

// The same as one packed entry, len | symbol << 8 (0xFFFFFF00: a bad code,
// len 0, symbol -1), with a single branch for the codes longer than 6 bits.
__device__ __forceinline__ uint32_t rt_entry(const RTab& t, uint32_t w16) {
  uint32_t e = ms_rl(t.l1, (int)(w16 >> 10));
  if (__builtin_expect(e == 0u, 0)) {
    int L = __popcll(__builtin_amdgcn_ballot_w64(t.lim <= w16));
    ms_opaque(L);
    L += 1;
    const int Lc = L > 16 ? 16 : L;
    const uint32_t idx = ms_rl(t.voff, Lc) + (w16 >> (16 - Lc));
    const uint32_t sym = (ms_rl(t.vals, (int)((idx >> 2) & 63u)) >> (8 * (idx & 3u))) & 0xFFu;
    e = L > 16 ? 0xFFFFFF00u : ((uint32_t)L | sym << 8);
  }
  return e;
}

// AC refinement entries: the symbol's fields the symbol loop needs, unpacked
// once per table instead of once per symbol:
//   bits 0-5   the code length: a 64-bit shift by the entry itself skips
//              the code
//   bit 6      stop: EOBr, or s > 1 (an error), or a bad code
//   bit 7      s == 1 (a new coefficient)
//   bits 8-11  r;  bits 12-15  s;  bits 16-20  the code length (0: bad)
//   bit 31     not a new-coefficient symbol (stop or ZRL) -- every entry the
//              fast loop's common step takes is > 0
__device__ __forceinline__ uint32_t ms_ref_pack(uint32_t L, int sym) {
  const int s = sym & 15, r = sym >> 4;
  const bool zrl = s == 0 && r == 15;
  const uint32_t stop = (s > 1 || (s == 0 && !zrl)) ? 1u : 0u;
  return L | stop << 6 | (s == 1 ? 1u : 0u) << 7 | (uint32_t)r << 8 | (uint32_t)s << 12 |
         L << 16 | (s != 1 ? 1u : 0u) << 31;
}
constexpr uint32_t kRefBad = 0x8000F040u;  // bad code: length 0, stop, s 15
// (per lane, on a built table's first level)
__device__ __forceinline__ uint32_t ms_ref_l1(uint32_t e) {
  return e ? ms_ref_pack(e & 31u, (int)(e >> 8)) : 0u;
}
__device__ __forceinline__ uint32_t rt_entry_ref(const RTab& t, uint32_t w16) {
  uint32_t e = ms_rl(t.l1, (int)(w16 >> 10));
  if (__builtin_expect(e == 0u, 0)) {
    int L = __popcll(__builtin_amdgcn_ballot_w64(t.lim <= w16));
    ms_opaque(L);
    L += 1;
    const int Lc = L > 16 ? 16 : L;
    const uint32_t idx = ms_rl(t.voff, Lc) + (w16 >> (16 - Lc));
    const uint32_t sym = (ms_rl(t.vals, (int)((idx >> 2) & 63u)) >> (8 * (idx & 3u))) & 0xFFu;
    e = L > 16 ? kRefBad : ms_ref_pack((uint32_t)L, (int)sym);
  }
  return e;
}

// The refinement symbol loop in straight scalar code (MsWBits reader):
// new-coefficient symbols that do not run past the band's zeros and take
// <= 15 correction bits, codes of <= 6 bits from the lane table, longer ones
// by the canonical limits (one ballot); ZRL and the EOBr that ends a block on
// side paths.  A symbol is two v_readlane (entry, zero place), ~27 scalar
// instructions and two conditional branches, two symbols per taken branch;
// the compiled loop of the same step took ~78 instructions, with register
// copies at its join points and a wait for the refill's prefetch on every
// symbol.  The
// buffer carries a marker bit right below its valid bits (>= 32 valid bits
// <=> a non-zero low word), so the loop keeps no bit count.  It returns
// BEFORE a symbol it does not take (the general step in ms_decode_scan
// decodes that one), or after the symbol that ends the band (ended = 1) or
// an EOBr (ended = 2, eobrun set); state in/out as MsWBits / the symbol loop
// keep it.  zpos lanes >= nzero hold a sentinel > 63 + 15 + 15, so a run past
// the band's zeros fails the <= 15 test (a zero index >= 64 reads lane
// t - 64, a zero before k: the difference is negative, and fails it too).
// Entry: >= 32 bits in the buffer.  The refill's scalar load is waited for
// before the return (the compiler does not count the statement's loads).
#define HJ_REF_BODY(EXIT)                                               \
  /* the new coefficient's place: the (zi + r)-th zero */               \
  "s_bfe_u32 %[r], %[e], 0x40008\n\t"                                   \
  "s_add_i32 %[t], %[zi], %[r]\n\t"                                     \
  "v_readlane_b32 %[p], %[zpos], %[t]\n\t"                              \
  /* correction bits: the history coefficients passed; leave if > 15 */ \
  /* or the entry is a stop or a long code (<= 0) */                    \
  "s_sub_i32 %[c], %[p], %[k]\n\t"                                      \
  "s_sub_i32 %[c], %[c], %[r]\n\t"                                      \
  "s_cmp_lt_i32 %[e], 1\n\t"                                            \
  "s_cselect_b32 %[c], 64, %[c]\n\t"                                    \
  "s_cmp_gt_u32 %[c], 15\n\t"                                           \
  "s_cbranch_scc1 " EXIT "\n\t"                                         \
  /* past the code: the sign bit on top (1: positive), then c bits; */ \
  /* a positive coefficient sets the sign mask's bit 0 (never a place */ \
  /* of an AC band) */                                                  \
  "s_lshl_b64 s[42:43], s[40:41], %[e]\n\t"                             \
  "s_bitset1_b64 %[nm], %[p]\n\t"                                       \
  "s_cmp_lt_i32 s43, 0\n\t"                                             \
  "s_cselect_b32 %[u], 0, %[p]\n\t"                                     \
  "s_bitset1_b64 %[nsg], %[u]\n\t"                                      \
  "s_sub_i32 %[o], 63, %[c]\n\t"                                        \
  "s_pack_ll_b32_b16 %[o], %[o], %[c]\n\t"                              \
  "s_bfe_u64 %[x], s[42:43], %[o]\n\t"                                  \
  "s_lshl_b64 %[corr], %[corr], %[c]\n\t"                               \
  "s_or_b64 %[corr], %[corr], %[x]\n\t"                                 \
  "s_add_i32 %[u], %[c], 1\n\t"                                         \
  "s_lshl_b64 s[40:41], s[42:43], %[u]\n\t"                             \
  "s_add_i32 %[k], %[p], 1\n\t"                                         \
  "s_add_i32 %[zi], %[t], 1\n\t"                                        \
  /* on while the band goes on and >= 32 bits are left */              \
  "s_cmp_ge_i32 %[p], %[se]\n\t"                                        \
  "s_cselect_b32 %[u], 0, s40\n\t"                                      \
  "s_cmp_lg_u32 %[u], 0\n\t"
#define HJ_REF_SYM                                                      \
  /* entry of the code at the top 6 bits (0: a longer code) */          \
  "s_lshr_b32 %[i], s41, 26\n\t"                                        \
  "v_readlane_b32 %[e], %[l1], %[i]\n\t"                                \
  HJ_REF_BODY("6f")

__device__ __forceinline__ void ms_ref_fast(uint64_t& buf, int& cnt, int& wi, uint32_t& nxm,
                                            uint32_t& nx, MsWords w, int lastw, int& k, int& zi,
                                            uint64_t& corr, uint64_t& nm, uint64_t& nsg,
                                            int& nsym, int se, const RTab& tab, uint32_t zpos,
                                            int& eobrun, int& ended) {
  uint32_t i, e, r, t, p, c, o, u;
  uint64_t x;
  // (all uniform; readfirstlane where the compiler's divergence analysis
  // cannot see it -- no instruction for values already in SGPRs)
  buf = ms_u64(buf);
  cnt = ms_i(cnt);
  wi = ms_i(wi);
  nxm = ms_u(nxm);
  nx = ms_u(nx);
  k = ms_i(k);
  zi = ms_i(zi);
  corr = ms_u64(corr);
  nm = ms_u64(nm);
  nsg = ms_u64(nsg);
  nsym = ms_i(nsym);
  eobrun = ms_i(eobrun);
  se = ms_i(se);
  lastw = ms_i(lastw);
  w = (MsWords)(const void*)(uintptr_t)ms_u64((uint64_t)(uintptr_t)(const void*)w);
  asm volatile(
      "s_mov_b32 %[ended], 0\n\t"
      // the marker below the valid bits
      "s_sub_i32 %[o], 63, %[cnt]\n\t"
      "s_bitset1_b64 s[40:41], %[o]\n"
      "1:\n\t"
      HJ_REF_SYM
      "s_cbranch_scc0 7f\n\t"
      HJ_REF_SYM
      "s_cbranch_scc1 1b\n"
      // the band's end, or a refill (MsWBits::need): the prefetched dword
      // enters the buffer right below the valid bits, the marker below it
      "7:\n\t"
      "s_cmp_ge_i32 %[p], %[se]\n\t"
      "s_cbranch_scc1 8f\n\t"
      "s_waitcnt lgkmcnt(0)\n\t"
      "s_ff1_i32_b64 %[o], s[40:41]\n\t"
      "s_bitset0_b64 s[40:41], %[o]\n\t"
      "s_sub_i32 %[o], 63, %[o]\n\t"
      "s_and_b32 s43, %[nx], %[nxm]\n\t"
      "s_brev_b32 s42, 1\n\t"
      "s_lshr_b64 s[42:43], s[42:43], %[o]\n\t"
      "s_or_b64 s[40:41], s[40:41], s[42:43]\n\t"
      "s_add_i32 %[wi], %[wi], 1\n\t"
      "s_sub_i32 %[o], %[lastw], %[wi]\n\t"
      "s_ashr_i32 %[o], %[o], 31\n\t"
      "s_not_b32 %[nxm], %[o]\n\t"
      "s_min_i32 %[o], %[wi], %[lastw]\n\t"
      "s_lshl_b32 %[o], %[o], 2\n\t"
      "s_load_dword %[nx], %[w], %[o]\n\t"
      "s_branch 1b\n"
      // not taken: a code longer than 6 bits (e = 0) by the canonical
      // limits -- length 1 + #{l : lim[l] <= w16} -- and its symbol; a
      // plain (s = 1) symbol goes on in line, the rest is the general step's
      "6:\n\t"
      "s_cmp_eq_u32 %[e], 0\n\t"
      "s_cbranch_scc0 5f\n\t"
      "s_lshr_b32 %[i], s41, 16\n\t"
      "v_cmp_ge_u32_e32 vcc, %[i], %[lim]\n\t"
      "s_bcnt1_i32_b64 %[t], vcc\n\t"
      "s_add_i32 %[t], %[t], 1\n\t"
      "s_cmp_gt_u32 %[t], 16\n\t"
      "s_cbranch_scc1 9f\n\t"
      "v_readlane_b32 %[o], %[voff], %[t]\n\t"
      "s_sub_i32 %[u], 16, %[t]\n\t"
      "s_lshr_b32 %[i], %[i], %[u]\n\t"
      "s_add_i32 %[i], %[i], %[o]\n\t"
      "s_lshr_b32 %[u], %[i], 2\n\t"
      "v_readlane_b32 %[o], %[vals], %[u]\n\t"
      "s_and_b32 %[i], %[i], 3\n\t"
      "s_lshl_b32 %[i], %[i], 3\n\t"
      "s_lshr_b32 %[o], %[o], %[i]\n\t"
      "s_and_b32 %[u], %[o], 15\n\t"
      "s_cmp_eq_u32 %[u], 1\n\t"
      "s_cbranch_scc0 9f\n\t"
      "s_bfe_u32 %[e], %[o], 0x40004\n\t"
      "s_lshl_b32 %[e], %[e], 8\n\t"
      "s_or_b32 %[e], %[e], %[t]\n\t"
      "s_or_b32 %[e], %[e], 0x80\n\t"
      HJ_REF_BODY("6b")
      "s_cbranch_scc1 1b\n\t"
      "s_branch 7b\n"
      // an entry <= 0 from the lane table: stop or ZRL
      "5:\n\t"
      "s_bitcmp1_b32 %[e], 6\n\t"
      "s_cbranch_scc1 3f\n\t"
      // not a stop: a new-coefficient symbol with > 15 correction bits (the
      // general step's), or ZRL: the 16th zero from k, its correction bits
      "s_cmp_gt_i32 %[e], -1\n\t"
      "s_cbranch_scc1 9f\n\t"
      "s_add_i32 %[t], %[zi], 15\n\t"
      "v_readlane_b32 %[p], %[zpos], %[t]\n\t"
      "s_sub_i32 %[c], %[p], %[k]\n\t"
      "s_sub_i32 %[c], %[c], 15\n\t"
      "s_cmp_gt_u32 %[c], 15\n\t"
      "s_cbranch_scc1 9f\n\t"
      "s_lshl_b64 s[42:43], s[40:41], %[e]\n\t"
      "s_sub_i32 %[o], 64, %[c]\n\t"
      "s_pack_ll_b32_b16 %[o], %[o], %[c]\n\t"
      "s_bfe_u64 %[x], s[42:43], %[o]\n\t"
      "s_lshl_b64 %[corr], %[corr], %[c]\n\t"
      "s_or_b64 %[corr], %[corr], %[x]\n\t"
      "s_lshl_b64 s[40:41], s[42:43], %[c]\n\t"
      "s_add_i32 %[k], %[p], 1\n\t"
      "s_add_i32 %[zi], %[t], 1\n\t"
      "s_cmp_ge_i32 %[p], %[se]\n\t"
      "s_cselect_b32 %[u], 0, s40\n\t"
      "s_cmp_lg_u32 %[u], 0\n\t"
      "s_cbranch_scc1 1b\n\t"
      "s_branch 7b\n"
      // a stop: EOBr (s = 0) ends the block with an EOB run of 2^r + r
      // more bits (r <= 14: the code is <= 6 bits, so >= 26 bits are in the
      // buffer); anything else is the general step's
      "3:\n\t"
      "s_bfe_u32 %[u], %[e], 0x4000c\n\t"
      "s_cmp_lg_u32 %[u], 0\n\t"
      "s_cbranch_scc1 9f\n\t"
      "s_lshl_b64 s[40:41], s[40:41], %[e]\n\t"
      "s_lshl_b32 %[eob], 1, %[r]\n\t"
      "s_sub_i32 %[o], 64, %[r]\n\t"
      "s_pack_ll_b32_b16 %[o], %[o], %[r]\n\t"
      "s_bfe_u64 s[42:43], s[40:41], %[o]\n\t"
      "s_add_i32 %[eob], %[eob], s42\n\t"
      "s_lshl_b64 s[40:41], s[40:41], %[r]\n\t"
      "s_add_i32 %[nsym], %[nsym], 1\n\t"
      "s_mov_b32 %[ended], 2\n\t"
      "s_branch 9f\n"
      "8:\n\t"
      "s_mov_b32 %[ended], 1\n"
      "9:\n\t"
      // the bit count back from the marker
      "s_ff1_i32_b64 %[o], s[40:41]\n\t"
      "s_bitset0_b64 s[40:41], %[o]\n\t"
      "s_sub_i32 %[cnt], 63, %[o]\n\t"
      "s_waitcnt lgkmcnt(0)\n\t"
      : "+{s[40:41]}"(buf), [cnt] "+s"(cnt), [wi] "+s"(wi), [nxm] "+s"(nxm), [nx] "+s"(nx),
        [k] "+s"(k), [zi] "+s"(zi), [corr] "+s"(corr), [nm] "+s"(nm), [nsg] "+s"(nsg),
        [nsym] "+s"(nsym), [eob] "+s"(eobrun), [ended] "=&s"(ended), [i] "=&s"(i), [e] "=&s"(e),
        [r] "=&s"(r), [t] "=&s"(t), [p] "=&s"(p), [c] "=&s"(c), [o] "=&s"(o), [u] "=&s"(u),
        [x] "=&s"(x)
      : [l1] "v"(tab.l1), [lim] "v"(tab.lim), [voff] "v"(tab.voff), [vals] "v"(tab.vals),
        [zpos] "v"(zpos), [se] "s"(se), [lastw] "s"(lastw), [w] "s"(w)
      : "s42", "s43", "vcc", "scc", "memory");
}
#undef HJ_REF_SYM
#undef HJ_REF_BODY

// bits k .. e (inclusive) of a coefficient mask; 0 when k > e
__device__ __forceinline__ uint64_t ms_range(int k, int e) {
  return k > e ? 0ull : ((~0ull) >> (63 - e)) & ((~0ull) << k);
}

// The image geometry the scan decoder needs (uniform copies).
// (sampling factors packed 3 bits each: a local array with a dynamic index
// would live in scratch memory)
struct MsGeo {
  int ncomp, mcux, bpm;
  uint32_t hv;  // comp_h[c] at bit 6c, comp_v[c] at bit 6c + 3
  __device__ __forceinline__ int h(int c) const { return (int)((hv >> (6 * c)) & 7u); }
  __device__ __forceinline__ int v(int c) const { return (int)((hv >> (6 * c + 3)) & 7u); }
};

__device__ __forceinline__ MsGeo ms_geo(const ImageInfo& in) {
  MsGeo g;
  g.ncomp = ms_i(in.ncomp);
  g.mcux = ms_i(in.mcux);
  g.bpm = ms_i(in.bpm);
  g.hv = 0;
  for (int c = 0; c < kMaxComp; c++)
    g.hv |= (uint32_t)ms_i(in.comp_h[c]) << (6 * c) | (uint32_t)ms_i(in.comp_v[c]) << (6 * c + 3);
  return g;
}

// The scalar fields of a scan record, uniform.
struct MsBand {
  int ns, ss, se, ah, al, ri, start, end;
};

__device__ __forceinline__ MsBand ms_band(const MsScan& sc) {
  return MsBand{ms_i(sc.ns), ms_i(sc.ss), ms_i(sc.se), ms_i(sc.ah), ms_i(sc.al), ms_i(sc.ri),
                ms_i(sc.start), ms_i(sc.end)};
}

// MCU-order block index of component c's block (bx, by)
__device__ __forceinline__ int ms_block(const MsGeo& g, int c, int bx, int by) {
  if (g.ncomp == 1) return by * g.mcux + bx;
  int b0 = 0;
  for (int k = 0; k < c; k++) b0 += g.h(k) * g.v(k);
  const int hc = g.h(c), vc = g.v(c);
  return ((by / vc) * g.mcux + bx / hc) * g.bpm + b0 + (by % vc) * hc + (bx % hc);
}

// x / d for a sampling factor d in 1..4 (no division instruction)
__device__ __forceinline__ int ms_div(int x, int d) {
  return d == 1 ? x : (d == 2 ? x >> 1 : (d == 4 ? x >> 2 : (int)(((uint32_t)x * 0xAAABu) >> 17)));
}

// c correction bits appended MSB-first to corr (bit order of the stream:
// the block's i-th non-zero history coefficient of n takes bit n - 1 - i)
template <class Rd>
__device__ __forceinline__ void ms_take_corr(Rd& br, int c, uint64_t& corr) {
  while (c > 0) {
    const int t = c < 32 ? c : 32;
    corr = (corr << t) | br.get(t);
    c -= t;
  }
}

// The same for a long run of correction bits (> 15), out of line: the
// symbol loop's registers stay put on its common path.
struct MsCorrState {
  MsFillState f;
  uint64_t corr;
};
__device__ __noinline__ MsCorrState ms_take_corr_slow(MsWords w, int size, int end, int lastw,
                                                      MsCorrState st, int c) {
  MsBits b;
  b.w = w;
  b.size = size;
  b.end = end;
  b.lastw = lastw;
  b.buf = st.f.buf;
  b.cnt = st.f.cnt;
  b.pos = st.f.pos;
  b.fake = st.f.fake;
  b.marker = st.f.marker != 0;
  b.n0 = st.f.n0;
  b.n1 = st.f.n1;
  ms_take_corr(b, c, st.corr);
  st.f = MsFillState{b.buf, b.cnt, b.pos, b.fake, b.marker ? 1 : 0, b.n0, b.n1};
  return st;
}
__device__ __forceinline__ void ms_take_corr_long(MsBits& br, int c, uint64_t& corr) {
  const MsCorrState st = ms_take_corr_slow(
      br.w, br.size, br.end, br.lastw,
      MsCorrState{MsFillState{br.buf, br.cnt, br.pos, br.fake, br.marker ? 1 : 0, br.n0, br.n1}, corr},
      c);
  br.buf = ms_u64(st.f.buf);
  br.cnt = ms_i(st.f.cnt);
  br.pos = ms_i(st.f.pos);
  br.fake = ms_i(st.f.fake);
  br.marker = ms_i(st.f.marker) != 0;
  br.n0 = ms_u(st.f.n0);
  br.n1 = ms_u(st.f.n1);
  corr = ms_u64(st.corr);
}

__device__ __forceinline__ void ms_take_corr_long(MsWBits& br, int c, uint64_t& corr) {
  ms_take_corr(br, c, corr);
}

enum { kScanSeq = 0, kScanDcFirst, kScanDcRefine, kScanAcFirst, kScanAcRefine };
constexpr int kMsChunk = 64;  // AC refinement blocks per chunk (one per lane)

// AC refinement chunk: the lanes' blocks (lane j = block m0 + j of the scan)
struct MsChunk {
  int32_t lv[64];          // the lane's block levels (zig-zag), loaded at the chunk start
  uint32_t mlo, mhi;       // the lane's block non-zero mask (all bands)
  uint32_t nlo, nhi;       // the same for the next chunk (prefetched)
  uint32_t clo, chi, wlo, whi, slo, shi;  // records: correction bits, new coefficients, signs
  int blk, nblk;           // the lane's block index (-1: none) / the next chunk's
};

// block index of scan position m of a one-component scan (per lane; -1 past the end)
__device__ __forceinline__ int ms_lane_block(const MsGeo& g, int c1, int bw1, int nmcu, int m) {
  return m < nmcu ? ms_block(g, c1, m % bw1, m / bw1) : -1;
}

__device__ __forceinline__ void ms_chunk_load(MsChunk& ch, const int32_t* __restrict__ lv,
                                              int blk) {
  ch.blk = blk;
  if (blk >= 0) {
    const uint4* src = reinterpret_cast<const uint4*>(lv + (size_t)blk * 64);
#pragma unroll
    for (int q = 0; q < 16; q++) {
      const uint4 x = src[q];
      ch.lv[4 * q] = (int32_t)x.x;
      ch.lv[4 * q + 1] = (int32_t)x.y;
      ch.lv[4 * q + 2] = (int32_t)x.z;
      ch.lv[4 * q + 3] = (int32_t)x.w;
    }
  }
}

// Apply the chunk's records (libjpeg decode_mcu_AC_refine: a correction bit
// adds +-p1 to a coefficient whose bit al is clear; a new coefficient is
// +-p1), store the band's levels and the updated non-zero mask.
__device__ __forceinline__ void ms_chunk_apply(MsChunk& ch, int32_t* __restrict__ lv,
                                               uint64_t* __restrict__ masks, int ss, int se,
                                               int al) {
  if (ch.blk < 0) return;
  const uint64_t band = ms_range(ss, se);
  const uint64_t m = (uint64_t)ch.mhi << 32 | ch.mlo;
  const uint64_t h = m & band;
  const uint64_t corr = (uint64_t)ch.chi << 32 | ch.clo;
  const uint64_t nm = (uint64_t)ch.whi << 32 | ch.wlo;
  const uint64_t sg = (uint64_t)ch.shi << 32 | ch.slo;
  const int32_t p1 = 1 << al, m1 = -p1;
  int rem = __popcll(h);  // one correction bit per non-zero history coefficient, MSB-first
#pragma unroll
  for (int k = 1; k < 64; k++) {
    if ((h >> k) & 1u) {
      rem--;
      if ((corr >> rem) & 1u) {
        const int32_t c = ch.lv[k];
        if ((c & p1) == 0) ch.lv[k] = c + (c >= 0 ? p1 : m1);
      }
    }
    if ((nm >> k) & 1u) ch.lv[k] = ((sg >> k) & 1u) ? m1 : p1;
  }
  int32_t* dst = lv + (size_t)ch.blk * 64;
#pragma unroll
  for (int q = 0; q < 16; q++) {
    if (4 * q >= ss && 4 * q + 3 <= se) {
      reinterpret_cast<uint4*>(dst)[q] = make_uint4((uint32_t)ch.lv[4 * q], (uint32_t)ch.lv[4 * q + 1],
                                                    (uint32_t)ch.lv[4 * q + 2],
                                                    (uint32_t)ch.lv[4 * q + 3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; e++)
        if (4 * q + e >= ss && 4 * q + e <= se) dst[4 * q + e] = ch.lv[4 * q + e];
    }
  }
  // (atomic: a first scan of another band of the component may run at once)
  if (nm) atomicOr(reinterpret_cast<unsigned long long*>(masks + ch.blk), nm);
}

// Trailing scans: a one-component AC scan may run while the earlier AC scans
// of its component that it depends on are still decoding, one chunk of
// kMsChunk blocks behind them (all of them visit the component's blocks in
// the same raster order).  Every AC scan publishes how many blocks it has
// finished (S.prog, after its level and mask stores for them); a trailing
// scan waits at each chunk start until its producers are past the chunk.
// The scans of a progressive image's component then overlap instead of
// running one after another (the default script's luma chain: two AC-first
// bands, then two refinement scans).
__device__ __forceinline__ void ms_publish(MsShared& S, int si, int n) {
  __threadfence_block();  // (the blocks' level / mask stores before the count)
  if (ms_lane0()) __hip_atomic_store(&S.prog[si], n, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// every scan in `soft` has finished `need` blocks (false: a scan failed)
__device__ __forceinline__ bool ms_reached(MsShared& S, uint64_t soft, int need) {
  for (; soft; soft &= soft - 1) {
    const int t = __builtin_ctzll(soft);
    if (ms_i(__hip_atomic_load(&S.prog[t], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) < need)
      return false;
  }
  return true;
}
__device__ __forceinline__ bool ms_wait(MsShared& S, uint64_t soft, int need) {
  while (!ms_reached(S, soft, need)) {
    if (ms_i(__hip_atomic_load(&S.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != kOk)
      return false;
    __builtin_amdgcn_s_sleep(1);
  }
  return true;
}

// t[i] for a uniform i (selects, not a dynamically indexed register array)
__device__ __forceinline__ RTab rt_pick(int i, const RTab (&t)[kMaxComp]) {
  RTab r = t[0];
  if (i == 1) r = t[1];
  if (i == 2) r = t[2];
  if (i == 3) r = t[3];
  return r;
}
__device__ __forceinline__ int32_t ms_pick(int i, const int32_t (&v)[kMaxComp]) {
  return i == 0 ? v[0] : (i == 1 ? v[1] : (i == 2 ? v[2] : v[3]));
}
__device__ __forceinline__ void ms_put(int i, int32_t (&v)[kMaxComp], int32_t x) {
  v[0] = i == 0 ? x : v[0];
  v[1] = i == 1 ? x : v[1];
  v[2] = i == 2 ? x : v[2];
  v[3] = i == 3 ? x : v[3];
}

// One block of an AC refinement scan against its history mask (lane j of
// the chunk): the symbols, the correction bits, the records of lane j.
template <class Rd>
__device__ __forceinline__ int ms_refine_block(Rd& br, MsChunk& ch, const int j,
                                               const uint64_t band, const int ss, const int se,
                                               const int lane, const RTab& atr, int& eobrun,
                                               int& nsym, int64_t (&prof)[3]) {
  constexpr bool kWord = ms_same<Rd, MsWBits>::value;
  int rc = kOk;
  // against the block's non-zero mask (lane j of the chunk)
#ifdef HJ_MS_PROF
  const int64_t pt0 = (int64_t)__builtin_amdgcn_s_memtime();
  int64_t pt1 = pt0;
#endif
  const uint64_t hist = ((uint64_t)ms_rl(ch.mhi, j) << 32 | ms_rl(ch.mlo, j)) & band;
  const int htot = __popcll(hist);
  uint64_t corr = 0, nm = 0, nsg = 0;
  int cb = 0;  // correction bits taken (non-zero history coefficients passed)
  if (eobrun <= 0) {
    // zpos lane i: the place of the band's i-th coefficient that was
    // zero before the scan (a lane permutation: the others go after)
    const uint64_t hz = ~hist & band;
    const int nzero = __popcll(hz);
    const int below = (int)__builtin_amdgcn_mbcnt_hi(
        (uint32_t)(hz >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)hz, 0u));
    const bool isz = (hz >> lane) & 1ull;
    uint32_t zpos = (uint32_t)__builtin_amdgcn_ds_permute(
        (isz ? below : nzero + lane - below) << 2, lane);
    zpos = lane < nzero ? zpos : 127u;  // (past the zeros: ms_ref_fast's sentinel)
    // One exit, at the bottom: the rare ends (EOBr, a run past se, a
    // bad code) only clear `live` and are sorted out after the loop,
    // so the symbol step is straight-line scalar code (flags as 0/1
    // integers, not compare results).
    int k = ss, zi = 0;  // next coefficient; zeros before it
    uint32_t e;
    int t, cont;
    constexpr uint32_t kRefDone = 15u << 8;  // (s = 0, r = 15: no EOBr, no error)
    // zpos is waited for here, once: in the loop the LDS and scalar
    // load counters are one, and a wait for it there would also wait
    // for the bit reader's prefetch
    asm volatile("" ::"s"(ms_rl(zpos, 0)));
#ifdef HJ_MS_PROF
    pt1 = (int64_t)__builtin_amdgcn_s_memtime();
#endif
    // (the refill at the bottom: the common path falls through)
    br.need();
    do {
      if constexpr (kWord) {
        // the common symbols in ms_ref_fast; it returns before one it
        // does not take, or after the one that ends the band
        const int k0 = k;
        const uint64_t nm0 = nm;
        int ended;
        ms_ref_fast(br.buf, br.cnt, br.wi, br.nxm, br.nx, br.w, br.lastw, k, zi, corr, nm,
                    nsg, nsym, se, atr, zpos, eobrun, ended);
#ifdef HJ_MS_COUNT2
        prof[0] += 0;
#elif defined(HJ_MS_COUNT)
        prof[0] += 256;  // (count build: fast-loop calls, blocks, general steps)
#endif
        cb += __popcll(hist & ms_range(k0, k - 1));
        // (symbols: the loop counts only EOBr; its new coefficients
        // here, its ZRL not at all)
        nsym += __popcll(nm) - __popcll(nm0);
        if (ended) {  // (1: the band's end; 2: an EOBr, eobrun set)
          e = kRefDone;
          t = 0;
          break;
        }
      }
      e = rt_entry_ref(atr, br.peek16());
      nsym++;
#ifdef HJ_MS_COUNT2
      // (second count build: general steps by kind -- long code / ZRL /
      // other)
      if (((e >> 16) & 31u) > 6u) prof[0] += 256;
      else if (((e >> 8) & 15u) == 15u && ((e >> 12) & 15u) == 0u) prof[1] += 256;
      else prof[2] += 256;
#elif defined(HJ_MS_COUNT)
      prof[2] += 256;
#endif
      br.skip((int)((e >> 16) & 31u));
      const int s1 = (int)((e >> 7) & 1u);
      int stop = (int)((e >> 6) & 1u);
      ms_opaque(stop);  // (as a compare result it went through the VALU: illegal copy)
      const int r = (int)((e >> 8) & 15u);
      // the new coefficient's sign (bit 1: positive)
      uint32_t h = br.hi32();
      ms_opaque(h);
      const uint32_t neg = (~h >> 31) & (uint32_t)s1;
      br.skip(s1);
      // the (r + 1)-th coefficient from k that was zero before the
      // scan is the new coefficient's place (ZRL: the 16th, left
      // zero); each non-zero one passed on the way takes a
      // correction bit
      t = zi + r;
      // (sign bits, not compares: a compare result the loop keeps
      // would become a lane mask and go through the VALU)
      uint32_t dz = (uint32_t)(t - nzero);
      ms_opaque(dz);
      const int live = (int)(dz >> 31) & (stop ^ 1);
      const int lm = -live;
      const int p = (int)ms_rl(zpos, t & lm);
      const int c = (p - k - r) & lm;
      if (__builtin_expect(c <= 15, 1)) {  // (>= 15 bits are left after a code and a sign)
        uint32_t hc = br.hi32();
        ms_opaque(hc);
        corr = (corr << c) | ((hc >> 1) >> (31 - c));
        br.skip(c);
      } else {
        ms_take_corr_long(br, c, corr);
      }
      cb += c;
      const uint32_t m1 = (uint32_t)(s1 & live);
      nm |= (uint64_t)m1 << p;
      nsg |= (uint64_t)(m1 & neg) << p;
      k = p + 1;
      zi = t + 1;
      // (k <= se, i.e. p < se: a sign bit)
      uint32_t dk = (uint32_t)(p - se);
      ms_opaque(dk);
      cont = live & (int)(dk >> 31);
      ms_opaque(cont);
      br.need();
    } while (__builtin_expect(cont, 1));
    const int r = (int)((e >> 8) & 15u), s = (int)((e >> 12) & 15u);
    if (s > 1 || (s == 1 && t >= nzero)) {
      rc = kErrBadHuffman;  // (a bad code, a value other than +-1, a new coefficient past se)
    } else if (s == 0 && r != 15) {  // EOBr
      eobrun = 1 << r;
      if (r) eobrun += (int)br.take(r);
    }
  }
#ifdef HJ_MS_PROF
  const int64_t pt2 = (int64_t)__builtin_amdgcn_s_memtime();
#endif
  if (rc != kOk) return rc;
  // the history coefficients after the last symbol (an EOB run, or a
  // run past se) take their correction bits
  ms_take_corr(br, htot - cb, corr);
  if (eobrun > 0) eobrun--;
  ch.clo = ms_wl(ch.clo, (uint32_t)corr, j);
  ch.chi = ms_wl(ch.chi, (uint32_t)(corr >> 32), j);
  ch.wlo = ms_wl(ch.wlo, (uint32_t)nm, j);
  ch.whi = ms_wl(ch.whi, (uint32_t)(nm >> 32), j);
  ch.slo = ms_wl(ch.slo, (uint32_t)nsg, j);
  ch.shi = ms_wl(ch.shi, (uint32_t)(nsg >> 32), j);
#ifdef HJ_MS_COUNT
#ifndef HJ_MS_COUNT2
  prof[1] += 256;
#endif
#elif defined(HJ_MS_PROF)
  const int64_t pt3 = (int64_t)__builtin_amdgcn_s_memtime();
  prof[0] += pt1 - pt0;
  prof[1] += pt2 - pt1;
  prof[2] += pt3 - pt2;
#endif
  return rc;
}

// Decode one scan (a whole decoder wave, uniform control flow).
// lv: the image's levels (64 int32 per block, zig-zag); masks: per block the
// coefficients non-zero so far (AC bands of progressive images); soft: the
// running scans this one trails (AC scans).
template <int kind, class Rd>
__device__ __forceinline__ int ms_decode_scan(MsShared& S, int si, uint64_t soft, const MsGeo& g,
                                              const ImageInfo& in, const uint8_t* __restrict__ d,
                                              const uint8_t* cl, int size, int32_t* __restrict__ lv,
                                              uint64_t* __restrict__ masks, int lane, int& nsym,
                                              int64_t (&prof)[3]) {
  const MsScan& scl = S.scan[si];
  const MsBand sc = ms_band(scl);
  // AC scans of a progressive image have one component
  constexpr bool kAc = kind == kScanAcFirst || kind == kScanAcRefine;
  constexpr int kComp = kAc ? 1 : kMaxComp;
  constexpr bool need_dc = kind == kScanSeq || kind == kScanDcFirst;
  constexpr bool need_ac = kind == kScanSeq || kAc;
  int rc = kOk;
  // tables per scan component, as the scan reads them
  RTab tdc[kMaxComp], tac[kMaxComp];
#pragma unroll
  for (int i = 0; i < kComp; i++) {
    if (i < sc.ns) {
      bool bad = false, bad2 = false;
      if (need_dc) {
        const int o = ms_i(scl.dht[ms_i(scl.td[i])]);
        if (o < 0) rc = kErrBadHeader;
        else tdc[i] = rt_build(d, o, lane, bad);
      }
      if (need_ac) {
        const int o = ms_i(scl.dht[4 + ms_i(scl.ta[i])]);
        if (o < 0) rc = kErrBadHeader;
        else tac[i] = rt_build(d, o, lane, bad2);
      }
      if (bad || bad2) rc = kErrBadHeader;
    }
  }
  if (rc != kOk) return rc;
  int nmcu = ms_i(in.mcux) * ms_i(in.mcuy), bw1 = 1;
  const int c1 = ms_i(scl.comp[0]);  // the component of a one-component scan
  if (sc.ns == 1) {
    bw1 = g.ncomp == 1 ? g.mcux : (ms_i(in.comp_w[c1]) + 7) / 8;
    nmcu = bw1 * (g.ncomp == 1 ? ms_i(in.mcuy) : (ms_i(in.comp_hpx[c1]) + 7) / 8);
  }
  const int hc1 = g.ncomp == 1 ? 1 : g.h(c1), vc1 = g.ncomp == 1 ? 1 : g.v(c1);
  int b01 = 0;  // blocks of the components before c1 in an MCU
  for (int k = 0; k < c1; k++) b01 += g.h(k) * g.v(k);
  constexpr bool kWord = ms_same<Rd, MsWBits>::value;
  Rd br;
  if constexpr (kWord) {
    br.init(cl + ms_i(S.dbase[si]), ms_i(S.dlen[si]));
  } else {
    br.w = (MsWords)(const void*)d;
    br.size = size;
    br.lastw = (size - 1) >> 2;
    br.start(sc.start, sc.end);
  }
  int32_t pred[kMaxComp] = {0, 0, 0, 0};
  int eobrun = 0;
  const int al = sc.al, ss = sc.ss, se = sc.se;
  const uint64_t band = ms_range(ss, se);
  uint32_t vblk = 0;  // the block being decoded, lane k = coefficient k
  RTab atr;  // AC refinement: the table with packed first-level entries
  if constexpr (kind == kScanAcRefine) {
    atr = tac[0];
    atr.l1 = ms_ref_l1(atr.l1);
  }
  MsChunk ch;
  bool have_next = false;
  if constexpr (kind == kScanAcRefine) ch.blk = -1;
  int bx = 0, by = 0, rpos = 0;
  // a one-component scan's block index, kept incrementally: rowb (the row's
  // first block) + colq (whole MCUs along the row) + colr (the block within
  // the MCU's width)
  const int bpm1 = g.ncomp == 1 ? 1 : g.bpm;
  const auto row_base = [&](int y) {
    return g.ncomp == 1 ? y * g.mcux
                        : ms_div(y, vc1) * g.mcux * g.bpm + b01 + (y - ms_div(y, vc1) * vc1) * hc1;
  };
  int rowb = row_base(0), colq = 0, colr = 0;
  for (int mcu = 0;; mcu++) {
    if constexpr (kind == kScanAcRefine) {
      if ((mcu & (kMsChunk - 1)) == 0 || mcu >= nmcu) {
        // chunk boundary: apply the finished chunk, load the next one's
        // levels and masks once the scans this one trails are past it
        ms_chunk_apply(ch, lv, masks, ss, se, al);
        if (mcu) ms_publish(S, si, mcu);
        if (mcu >= nmcu) break;
        const int nxt = min(mcu + kMsChunk, nmcu);
        if (!have_next) {
          if (!ms_wait(S, soft, nxt)) {
            rc = kErrBadHuffman;  // (another scan failed; its status is the image's)
            break;
          }
          ch.nblk = ms_lane_block(g, c1, bw1, nmcu, mcu + lane);
          const uint64_t m = ch.nblk >= 0 ? masks[ch.nblk] : 0ull;
          ch.nlo = (uint32_t)m;
          ch.nhi = (uint32_t)(m >> 32);
        }
        ch.mlo = ch.nlo;
        ch.mhi = ch.nhi;
        ms_chunk_load(ch, lv, ch.nblk);
        ch.clo = ch.chi = ch.wlo = ch.whi = ch.slo = ch.shi = 0;
        // the next chunk's masks now, if its producers are already past it
        have_next = nxt < nmcu && ms_reached(S, soft, min(nxt + kMsChunk, nmcu));
        if (have_next) {
          ch.nblk = ms_lane_block(g, c1, bw1, nmcu, nxt + lane);
          const uint64_t m = ch.nblk >= 0 ? masks[ch.nblk] : 0ull;
          ch.nlo = (uint32_t)m;
          ch.nhi = (uint32_t)(m >> 32);
        }
      }
    } else {
      if (mcu >= nmcu) break;
    }
    if constexpr (!kWord)  // (the word reader takes scans without restart markers)
    if (sc.ri && mcu && rpos == 0) {
      if (br.truncated()) {
        rc = kErrTruncated;
        break;
      }
      // the next marker must be RSTn (found in the file itself: once per interval)
      int p = br.pos;
      for (;;) {
        if (p >= sc.end) {
          rc = kErrBadRestart;
          break;
        }
        const uint32_t c = br.byte(p);
        if (c == 0xFFu && p + 1 < size && br.byte(p + 1) == 0u) {
          p += 2;
          continue;
        }
        if (c == 0xFFu) break;
        p++;
      }
      if (rc != kOk) break;
      while (p < size && br.byte(p) == 0xFFu) p++;
      if (p >= size || br.byte(p) < 0xD0u || br.byte(p) > 0xD7u) {
        rc = kErrBadRestart;
        break;
      }
      br.start(p + 1, sc.end);
      pred[0] = pred[1] = pred[2] = pred[3] = 0;
      eobrun = 0;
    }
#pragma unroll 1
    for (int i = 0; i < (kAc ? 1 : sc.ns) && rc == kOk; i++) {
      // the MCU's blocks of scan component i (one block for a one-component scan)
      int b, nb = 1;
      if (!kAc && sc.ns > 1) {
        const int c = ms_i(scl.comp[i]);
        nb = g.h(c) * g.v(c);
        b = mcu * g.bpm;
        for (int k = 0; k < c; k++) b += g.h(k) * g.v(k);
      } else {
        b = rowb + colq + colr;
      }
      RTab dt, at;
      if constexpr (need_dc) dt = kComp == 1 ? tdc[0] : rt_pick(i, tdc);
      if constexpr (need_ac) at = kComp == 1 ? tac[0] : rt_pick(i, tac);
      int32_t pr = ms_pick(i, pred);
      for (int u = 0; u < nb; u++, b++) {
        int32_t* blev = lv + (size_t)b * 64;
        if constexpr (kind == kScanDcFirst) {
          br.need();
          int len;
          const int s = rt_decode(dt, br.peek16(), len);
          nsym++;
          if (s < 0 || s > 15) {
            rc = kErrBadHuffman;
            break;
          }
          br.skip(len);
          pr += s ? br.take_ext(s) : 0;
          if (ms_lane0()) blev[0] = (int32_t)((uint32_t)pr << al);
        } else if constexpr (kind == kScanDcRefine) {
          br.need();
          const uint32_t bit = br.take_bit();
          if (bit) {  // (uniform; then lane 0)
            if (ms_lane0()) atomicOr(reinterpret_cast<unsigned int*>(blev), 1u << al);
          }
        } else if constexpr (kind == kScanAcFirst) {
          if (eobrun > 0) {
            eobrun--;
          } else {
            // one exit, at the bottom (as the refinement loop below)
            uint64_t nz = 0;
            int k = ss, rs, r, s;
            bool eob, bad, cont;
            br.need();
            do {
              const uint32_t e = rt_entry(at, br.peek16());  // (len 0, -1: bad code)
              nsym++;
              br.skip((int)(e & 31u));
              rs = (int)e >> 8;
              r = rs >> 4;
              s = rs & 15;
              eob = s == 0 && r != 15;
              k += r;  // (ZRL: 15)
              bad = rs < 0 || (s != 0 && k > se);
              // the value (F.2.2.1 EXTEND; 0 for s = 0), branch-free
              uint32_t h = br.hi32();
              ms_opaque(h);
              const int v = (int)((h >> 1) >> (31 - s));
              const int x = (int32_t)h < 0 ? v : v + 1 - (1 << s);
              br.skip(s);
              const bool put = s != 0 && !bad;
              vblk = ms_wl(vblk, (uint32_t)x << al, put ? k : 64);
              nz |= put ? 1ull << k : 0ull;
              k++;
              cont = !eob && !bad && k <= se;
              br.need();
            } while (cont);
            if (bad) {
              rc = kErrBadHuffman;
            } else if (eob) {
              eobrun = (1 << r) - 1;
              if (r) eobrun += (int)br.take(r);
            }
            if (rc != kOk) break;
            if (nz) {
              // only the coefficients the scan codes (oracle ms_block_decode,
              // libjpeg decode_mcu_AC_first): a first scan whose band overlaps
              // an earlier one's leaves that scan's other values alone
              if ((nz >> lane) & 1ull) blev[lane] = (int32_t)vblk;
              vblk = 0;
              if (ms_lane0()) atomicOr(reinterpret_cast<unsigned long long*>(masks + b), nz);
            }
          }
          if ((mcu & (kMsChunk - 1)) == kMsChunk - 1) ms_publish(S, si, mcu + 1);
        } else if constexpr (kind == kScanAcRefine) {
          rc = ms_refine_block(br, ch, mcu & (kMsChunk - 1), band, ss, se, lane, atr, eobrun,
                               nsym, prof);
          if (rc != kOk) break;
        } else {  // sequential: the whole block
          br.need();
          int len;
          int s = rt_decode(dt, br.peek16(), len);
          nsym++;
          if (s < 0 || s > 15) {
            rc = kErrBadHuffman;
            break;
          }
          br.skip(len);
          pr += s ? br.take_ext(s) : 0;
          vblk = ms_wl(vblk, (uint32_t)pr, 0);
          for (int k = 1; k < 64;) {
            br.need();
            const int rs = rt_decode(at, br.peek16(), len);
            nsym++;
            if (rs < 0) {
              rc = kErrBadHuffman;
              break;
            }
            br.skip(len);
            const int r = rs >> 4;
            s = rs & 15;
            if (s == 0) {
              if (r == 15) {
                k += 16;
                continue;
              }
              if (r != 0) rc = kErrBadHuffman;
              break;
            }
            k += r;
            if (k > 63) {
              rc = kErrBadHuffman;
              break;
            }
            vblk = ms_wl(vblk, (uint32_t)br.take_ext(s), k);
            k++;
          }
          blev[lane] = (int32_t)vblk;
          vblk = 0;
        }
      }
      ms_put(i, pred, pr);
    }
    if (rc != kOk) break;
    if (++bx == bw1) {
      bx = 0;
      by++;
      rowb = row_base(by);
      colq = colr = 0;
    } else {
      const bool wrap = colr + 1 == hc1;
      colr = wrap ? 0 : colr + 1;
      colq += wrap ? bpm1 : 0;
    }
    if (sc.ri && ++rpos == sc.ri) rpos = 0;
  }
  if (rc == kOk) rc = br.truncated() ? kErrTruncated : kOk;
  return rc;
}

// An AC refinement scan over the destuffed copy (no restart markers): the
// block loop of ms_decode_scan without its per-MCU bookkeeping (block
// coordinates, predictors, restart intervals, scan components) -- a chunk of
// kMsChunk blocks is loaded, decoded block by block, applied and published.
__device__ __forceinline__ int ms_refine_word(MsShared& S, const int si, const uint64_t soft,
                                              const MsGeo& g, const ImageInfo& in,
                                              const uint8_t* __restrict__ d, const uint8_t* cl,
                                              int32_t* __restrict__ lv,
                                              uint64_t* __restrict__ masks, const int lane,
                                              int& nsym, int64_t (&prof)[3]) {
  const MsScan& scl = S.scan[si];
  const MsBand sc = ms_band(scl);
  const int o = ms_i(scl.dht[4 + ms_i(scl.ta[0])]);
  if (o < 0) return kErrBadHeader;
  bool bad = false;
  RTab atr = rt_build(d, o, lane, bad);
  if (bad) return kErrBadHeader;
  atr.l1 = ms_ref_l1(atr.l1);
  const int c1 = ms_i(scl.comp[0]);
  const int bw1 = g.ncomp == 1 ? g.mcux : (ms_i(in.comp_w[c1]) + 7) / 8;
  const int nmcu = bw1 * (g.ncomp == 1 ? ms_i(in.mcuy) : (ms_i(in.comp_hpx[c1]) + 7) / 8);
  MsWBits br;
  br.init(cl + ms_i(S.dbase[si]), ms_i(S.dlen[si]));
  const int al = sc.al, ss = sc.ss, se = sc.se;
  const uint64_t band = ms_range(ss, se);
  int eobrun = 0, rc = kOk;
  MsChunk ch;
  ch.blk = -1;
  bool have_next = false;
  for (int m0 = 0; m0 < nmcu; m0 += kMsChunk) {
    const int nxt = min(m0 + kMsChunk, nmcu);
    // levels and masks of the chunk once the scans this one trails are past it
    if (!have_next) {
      if (!ms_wait(S, soft, nxt)) return kErrBadHuffman;  // (another scan failed)
      ch.nblk = ms_lane_block(g, c1, bw1, nmcu, m0 + lane);
      const uint64_t m = ch.nblk >= 0 ? masks[ch.nblk] : 0ull;
      ch.nlo = (uint32_t)m;
      ch.nhi = (uint32_t)(m >> 32);
    }
    ch.mlo = ch.nlo;
    ch.mhi = ch.nhi;
    ms_chunk_load(ch, lv, ch.nblk);
    ch.clo = ch.chi = ch.wlo = ch.whi = ch.slo = ch.shi = 0;
    // the next chunk's masks now, if its producers are already past it
    have_next = nxt < nmcu && ms_reached(S, soft, min(nxt + kMsChunk, nmcu));
    if (have_next) {
      ch.nblk = ms_lane_block(g, c1, bw1, nmcu, nxt + lane);
      const uint64_t m = ch.nblk >= 0 ? masks[ch.nblk] : 0ull;
      ch.nlo = (uint32_t)m;
      ch.nhi = (uint32_t)(m >> 32);
    }
    const int nb = nxt - m0;
    for (int j = 0; j < nb; j++) {
      rc = ms_refine_block(br, ch, j, band, ss, se, lane, atr, eobrun, nsym, prof);
      if (rc != kOk) return rc;
    }
    ms_chunk_apply(ch, lv, masks, ss, se, al);
    ms_publish(S, si, nxt);
  }
  return br.truncated() ? kErrTruncated : kOk;
}

// The AC refinement scan decoder as a function of its own: inlined into the
// kernel it shares the SGPR budget with every other scan kind and the
// kernel's state (104 SGPRs, spilled to VGPR lanes around the symbol loop);
// called, it gets the registers to itself (arguments arrive in VGPRs:
// readfirstlane).  Returns {status, symbols}.
template <class Rd>
__device__ __noinline__ int2 ms_decode_refine(MsShared& S, int si, uint64_t soft, MsGeo g,
                                              const ImageInfo& in, const uint8_t* d,
                                              const uint8_t* cl, int size, int32_t* lv,
                                              uint64_t* masks, int lane) {
  g.ncomp = ms_i(g.ncomp);
  g.mcux = ms_i(g.mcux);
  g.bpm = ms_i(g.bpm);
  g.hv = ms_u(g.hv);
  const auto up = [](auto* q) {
    return reinterpret_cast<decltype(q)>(ms_u64((uint64_t)(uintptr_t)q));
  };
  int nsym = 0;
  int64_t prof[3] = {0, 0, 0};
  if constexpr (ms_same<Rd, MsWBits>::value) {
    const int rc = ms_refine_word(S, ms_i(si), ms_u64(soft), g, *up(&in), up(d), up(cl), up(lv),
                                  up(masks), lane, nsym, prof);
    return make_int2(rc, nsym);
  }
  const int rc = ms_decode_scan<kScanAcRefine, Rd>(S, ms_i(si), ms_u64(soft), g, *up(&in), up(d),
                                                   up(cl), ms_i(size), up(lv), up(masks), lane,
                                                   nsym, prof);
  return make_int2(rc, nsym);
}

__global__ void __launch_bounds__(256) multiscan_kernel(const uint8_t* __restrict__ bytes,
                                                        uint8_t* __restrict__ clean,
                                                        const ImageDesc* __restrict__ desc,
                                                        ImageInfo* __restrict__ infos,
                                                        uint32_t* __restrict__ ents,
                                                        uint2* __restrict__ bdesc) {
  __shared__ MsShared S;
  const int img = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  ImageInfo& in = infos[img];
  if (in.status != kOk || !in.multiscan) return;
  // the scan decoders' waves (one serial bit chain each) ahead of the CU's
  // other waves -- the other lanes' kernels take the issue cycles they leave
  // (r05 A/B, one progressive image per pipelined batch: 3.71 -> 3.61 ms per
  // batch, profiles/r05/ab/multiscan_prio.txt)
  __builtin_amdgcn_s_setprio(kMsPrio);
  const ImageDesc& dd = desc[img];
  const uint8_t* d = bytes + dd.in_off;
  const int size = (int)dd.in_size;
  const bool prog = in.progressive != 0;
  int32_t* lv = reinterpret_cast<int32_t*>(ents + (size_t)dd.coef_off * 64);
  // per block non-zero coefficient masks while the scans decode (bdesc is
  // written only by the final pass)
  uint64_t* masks = reinterpret_cast<uint64_t*>(bdesc + dd.coef_off);
  const int nblocks = in.nblocks;
  int64_t t0 = wall_clock64(), tph[4] = {0, 0, 0, 0}, tdbg[4] = {0, 0, 0, 0};
  const MsGeo geo = ms_geo(in);
  if (tid == 0) {
    S.nmarks = 0;
    S.nscans = 0;
    S.err = kOk;
  }
  __syncthreads();
  // ---- marker candidates: 0xFF followed by neither 0x00, 0xFF nor RSTn,
  // from the first scan's data on (APPn payloads before it -- ICC profiles,
  // EXIF, thumbnails -- are skipped by length and never end a scan) ----
  for (int g = (in.scan_start >> 4) + tid; g * 16 < size; g += nt) {
    const int b = g * 16;
    uint32_t w[5];
    if (b + 20 <= size) {
      const uint4 q = *reinterpret_cast<const uint4*>(d + b);
      w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
      w[4] = *reinterpret_cast<const uint32_t*>(d + b + 16);
    } else {
      for (int i = 0; i < 5; i++) w[i] = 0;
      for (int i = 0; i < 20 && b + i < size; i++) w[i >> 2] |= (uint32_t)d[b + i] << (8 * (i & 3));
    }
    for (int i = 0; i < 16 && b + i + 1 < size; i++) {
      const uint32_t c = (w[i >> 2] >> (8 * (i & 3))) & 0xFFu;
      const uint32_t nx = (w[(i + 1) >> 2] >> (8 * ((i + 1) & 3))) & 0xFFu;
      if (c == 0xFFu && nx != 0u && nx != 0xFFu && (nx < 0xD0u || nx > 0xD7u)) {
        const int k = atomicAdd(&S.nmarks, 1);
        if (k < kMsMaxMarks) S.marks[k] = b + i;
      }
    }
  }
  for (int i = tid; i < nblocks * 16; i += nt)
    reinterpret_cast<uint4*>(lv)[i] = make_uint4(0u, 0u, 0u, 0u);
  for (int i = tid; i < nblocks; i += nt) masks[i] = 0ull;
  __syncthreads();
  // ---- thread 0: sort the candidates, walk the segments, record the scans ----
  if (tid == 0) {
    const int nm = min(S.nmarks, kMsMaxMarks);
    for (int i = 1; i < nm; i++) {
      const int v = S.marks[i];
      int j = i - 1;
      while (j >= 0 && S.marks[j] > v) {
        S.marks[j + 1] = S.marks[j];
        j--;
      }
      S.marks[j + 1] = v;
    }
    // more candidates than the list holds: find each scan's end by a forward
    // search from its start instead
    const bool overflow = S.nmarks > kMsMaxMarks;
    int err = kOk;
    int* dht = S.dht;
    int* comp_id = S.comp_id;
    for (int t = 0; t < 8; t++) dht[t] = -1;
    for (int c = 0; c < kMaxComp; c++) comp_id[c] = 0;
    int ri = 0, ns = 0;
    int pos = 2;
    while (err == kOk) {
      while (pos < size && d[pos] != 0xFF) pos++;
      while (pos < size && d[pos] == 0xFF) pos++;
      if (pos >= size) break;
      const int m = d[pos++];
      if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
      if (m == 0xD9) break;
      if (pos + 2 > size) {
        err = kErrBadHeader;
        break;
      }
      const int len = (d[pos] << 8) | d[pos + 1];
      if (len < 2 || pos + len > size) {
        err = kErrBadHeader;
        break;
      }
      int p = pos + 2;
      const int seg_end = pos + len;
      pos = seg_end;
      if (m == 0xC4) {
        while (p + 17 <= seg_end) {
          const int tc = d[p] >> 4, th = d[p] & 15;
          int total = 0;
          for (int l = 1; l <= 16; l++) total += d[p + l];
          if (tc > 1 || th > 3 || total > 256 || p + 17 + total > seg_end) {
            err = kErrBadHeader;
            break;
          }
          dht[tc * 4 + th] = p;
          p += 17 + total;
        }
      } else if (m == 0xC0 || m == 0xC1 || m == 0xC2) {
        for (int c = 0; c < in.ncomp && p + 6 + 3 * c < seg_end; c++) comp_id[c] = d[p + 6 + 3 * c];
      } else if (m == 0xDD) {
        if (len >= 4) ri = (d[p] << 8) | d[p + 1];
      } else if (m == 0xDA) {
        if (ns >= kMsMaxScans) {
          err = kErrUnsupported;
          break;
        }
        MsScan& sc = S.scan[ns];
        sc.ns = p < seg_end ? d[p] : 0;  // (an empty SOS: Ns would lie past the segment)
        if (sc.ns < 1 || sc.ns > in.ncomp || p + 1 + 2 * sc.ns + 3 > seg_end) {
          err = kErrBadHeader;
          break;
        }
        for (int i = 0; i < sc.ns; i++) {
          const int cs = d[p + 1 + 2 * i];
          int c = -1;
          for (int k = 0; k < in.ncomp; k++)
            if (comp_id[k] == cs) c = k;
          sc.comp[i] = c;
          sc.td[i] = d[p + 2 + 2 * i] >> 4;
          sc.ta[i] = d[p + 2 + 2 * i] & 15;
          if (c < 0 || sc.td[i] > 3 || sc.ta[i] > 3) err = kErrBadHeader;
        }
        if (err != kOk) break;
        sc.ss = d[p + 1 + 2 * sc.ns];
        sc.se = d[p + 2 + 2 * sc.ns];
        sc.ah = d[p + 3 + 2 * sc.ns] >> 4;
        sc.al = d[p + 3 + 2 * sc.ns] & 15;
        if (prog ? (sc.ss > sc.se || sc.se > 63 || sc.al > 13 || (sc.ss == 0 && sc.se != 0) ||
                    (sc.ss > 0 && sc.ns != 1))
                 : (sc.ss != 0 || sc.se != 63 || sc.ah || sc.al)) {
          err = kErrBadHeader;
          break;
        }
        sc.ri = ri;
        for (int t = 0; t < 8; t++) sc.dht[t] = dht[t];
        sc.start = seg_end;
        int e = size;  // the scan's data ends at the first marker past its start
        if (!overflow) {
          for (int i = 0; i < nm; i++)
            if (S.marks[i] >= seg_end) {
              e = S.marks[i];
              break;
            }
        } else {
          for (int i = seg_end; i + 1 < size; i++) {
            const int nx = d[i + 1];
            if (d[i] == 0xFF && nx != 0 && nx != 0xFF && (nx < 0xD0 || nx > 0xD7)) {
              e = i;
              break;
            }
          }
        }
        sc.end = e;
        pos = e;
        ns++;
      }
    }
    if (err == kOk && ns == 0) err = kErrBadHeader;
    S.nscans = ns;
    S.err = err;
  }
  __syncthreads();
  // ---- each scan without restart markers destuffed into `clean` (the
  // image's offsets; the scan's start rounded down to 4, so the scans' copies
  // never overlap: headers >= 10 bytes lie between them), bytes reversed in
  // each dword so that a dword load is the big-endian bit order.  Each thread
  // takes a contiguous slice: count the kept bytes (a 0x00 after 0xFF is
  // dropped), scan the counts, write.  A 0xFF followed by anything but 0x00
  // inside the scan (fill bytes before the marker, a stray marker) leaves
  // the scan to the stuffed reader, which stops there. ----
  uint8_t* cl = clean + dd.in_off;
  const int lane0 = tid & 63, wid = tid >> 6;
  for (int i = 0; i < S.nscans && S.err == kOk; i++) {
    const int s0 = S.scan[i].start, e0 = S.scan[i].end;
    if (S.scan[i].ri != 0) {
      if (tid == 0) S.dlen[i] = -1;
      continue;
    }
    if (tid == 0) S.dodd = 0;
    const int per = ((e0 - s0 + nt - 1) / nt + 15) & ~15;
    const int cs = min(s0 + tid * per, e0), ce = min(cs + per, e0);
    // The copy's dwords stay inside the image's own bytes (a tightly packed
    // next image may follow at in_size while its destuff / entropy run on
    // another stream): base = the scan start rounded down to 4, lowered
    // further when the last (byte-reversed) dword would pass in_size.  It
    // stays past the previous scan's copy: >= 10 header bytes separate them.
    uint8_t* out = cl;
    int base = 0;
    int kept = 0, off = 0;
    bool odd = false;
    for (int pass = 0; pass < 2; pass++) {
      uint32_t prev = cs > s0 ? d[cs - 1] : 0u;
      int o = off;
      for (int a = cs & ~15; a < ce; a += 16) {
        uint32_t w4[4];
        if (a + 16 <= size) {
          const uint4 q = *reinterpret_cast<const uint4*>(d + a);
          w4[0] = q.x, w4[1] = q.y, w4[2] = q.z, w4[3] = q.w;
        } else {
          for (int k = 0; k < 4; k++) w4[k] = 0;
          for (int k = 0; k < 16 && a + k < size; k++) w4[k >> 2] |= (uint32_t)d[a + k] << (8 * (k & 3));
        }
#pragma unroll
        for (int k = 0; k < 16; k++) {
          const int p = a + k;
          const uint32_t c = (w4[k >> 2] >> (8 * (k & 3))) & 0xFFu;
          if (p >= cs && p < ce) {
            const bool ff = prev == 0xFFu;
            if (ff && c != 0u) odd = true;
            if (!(ff && c == 0u)) {
              if (pass) out[o ^ 3] = (uint8_t)c;
              o++;
            }
            prev = c;
          }
        }
      }
      if (ce == e0 && ce > cs && prev == 0xFFu) odd = true;  // (0xFF as the scan's last byte)
      if (pass == 0) {
        kept = o;
        // exclusive scan of the slices' counts
        const int inc = wave_incl_scan(kept);
        if (lane0 == 63) S.wtot[wid] = inc;
        if (odd) S.dodd = 1;
        __syncthreads();
        int wb = 0;
        for (int k = 0; k < wid; k++) wb += S.wtot[k];
        off = wb + inc - kept;
        if (S.dodd) break;  // (uniform: every thread read it after the barrier)
        const int tot = S.wtot[0] + S.wtot[1] + S.wtot[2] + S.wtot[3];
        base = min(s0 & ~3, ((int)dd.in_size - ((tot + 3) & ~3)) & ~3);
        out = cl + base;
        if (base < 0) break;  // (cannot happen: total <= e0 - s0; uniform)
      }
    }
    const int total = S.wtot[0] + S.wtot[1] + S.wtot[2] + S.wtot[3];
    __syncthreads();
    if (tid == 0) {
      if (S.dodd || base < 0) {
        S.dlen[i] = -1;
      } else {
        for (int k = total; k & 3; k++) out[k ^ 3] = 0;  // (the last dword's tail)
        S.dlen[i] = total;
        S.dbase[i] = base;
      }
    }
    __syncthreads();
  }
  __threadfence();  // (the copies before any decoder wave reads them)
  __syncthreads();
  tph[0] = wall_clock64() - t0;  // marker candidates + segment walk
  // ---- scan dependencies: a scan waits for every earlier scan that shares
  // a component and overlaps its coefficient band -- to finish, or, when
  // both are one-component AC scans of a progressive image, only to stay
  // ahead of it (soft: the later scan trails it chunk by chunk) ----
  for (int i = tid; i < S.nscans; i += nt) {
    const MsScan& x = S.scan[i];
    int cx = 0;
    for (int k = 0; k < x.ns; k++) cx |= 1 << x.comp[k];
    const int lx = prog ? x.ss : 0, hx = prog ? x.se : 63;
    const bool xac = prog && x.ss > 0;
    uint64_t m = 0, sm = 0;
    for (int j = 0; j < i; j++) {
      const MsScan& y = S.scan[j];
      int cy = 0;
      for (int k = 0; k < y.ns; k++) cy |= 1 << y.comp[k];
      const int ly = prog ? y.ss : 0, hy = prog ? y.se : 63;
      if ((cx & cy) && !(hy < lx || hx < ly)) {
        // (AC scans have one component; only a refinement scan trails: a
        // first scan does not wait on its way, so one whose band overlaps an
        // earlier AC scan's -- no legal progression -- starts after it)
        if (xac && x.ah != 0 && y.ss > 0) sm |= 1ull << j;
        else m |= 1ull << j;
      }
    }
    S.deps[i] = m;
    S.soft[i] = sm;
    S.prog[i] = 0;
  }
  if (tid < 48) S.sdiag[tid] = 0;
  __syncthreads();
  if (tid == 0) {
    // claim priority: a scan's bytes plus the heaviest chain of scans that
    // wait for it (hard or trailing), so the chain that bounds the image --
    // for the libjpeg script the luma AC bands and the two refinement scans
    // trailing them -- takes the waves first
    // (a scan's cost: its bytes plus a byte per block it visits -- the DC
    // scans' per-block work is most of theirs: the DC chain, ~1 KB of bits
    // over every block of the image, then starts before the chroma chains
    // instead of after the luma AC bands)
    for (int i = S.nscans - 1; i >= 0; i--) {
      int down = 0;
      for (int j = i + 1; j < S.nscans; j++)
        if (((S.deps[j] | S.soft[j]) >> i) & 1ull) down = max(down, S.prio[j]);
      const MsScan& x = S.scan[i];
      const int c0 = x.comp[0];
      const int blocks = x.ns > 1 || in.ncomp == 1
                             ? nblocks
                             : ((in.comp_w[c0] + 7) / 8) * ((in.comp_hpx[c0] + 7) / 8);
      S.prio[i] = x.end - x.start + blocks + down;
    }
    S.claimed = 0;
    S.done = 0;
    for (int k = 0; k < 4; k++) S.tkind[k] = 0;
  }
  __syncthreads();
  const int64_t tdec = wall_clock64();
  const int64_t cdec = (int64_t)__builtin_amdgcn_s_memtime();
  // ---- decoder waves: each takes the first ready scan, decodes it and marks
  // it done ----
  const int lane = tid & 63;
  // (four of them; one wave, the scans one after another, decoded the
  // dominant scan no faster: profiles/r05/prog/)
  constexpr int kMsWaves = 4;
  if ((__builtin_amdgcn_readfirstlane(tid) >> 6) < kMsWaves) {
    __builtin_amdgcn_s_setprio(2);  // the serial bit chains: first in issue
    const bool progu = ms_i(prog) != 0;
    const int sizeu = ms_i(size);
    for (;;) {
      // claim (lane 0 does the LDS atomic; its result is broadcast)
      int si = -1;
      for (;;) {
        const int nsc = ms_i(S.nscans);
        const uint64_t full = nsc >= 64 ? ~0ull : ((1ull << nsc) - 1ull);
        const uint64_t done = ms_u64(__hip_atomic_load(&S.done, __ATOMIC_ACQUIRE,
                                                        __HIP_MEMORY_SCOPE_WORKGROUP));
        const uint64_t claimed = ms_u64(__hip_atomic_load(&S.claimed, __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_WORKGROUP));
        if (ms_i(__hip_atomic_load(&S.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) !=
                kOk ||
            (claimed & full) == full)
          break;
        // the claimable scan of the heaviest chain first (S.prio)
        int cand = -1, cprio = -1;
        for (int i = 0; i < nsc; i++)
          if (!((claimed >> i) & 1ull) && (ms_u64(S.deps[i]) & ~done) == 0ull &&
              (ms_u64(S.soft[i]) & ~(done | claimed)) == 0ull) {
            const int pr = ms_i(S.prio[i]);
            if (pr > cprio) {
              cand = i;
              cprio = pr;
            }
          }
        if (cand < 0) {
          __builtin_amdgcn_s_sleep(2);
          continue;
        }
        uint64_t old = 0;
        if (ms_lane0()) old = atomicOr(reinterpret_cast<unsigned long long*>(&S.claimed),
                                       1ull << cand);
        if (!((ms_u64(old) >> cand) & 1ull)) {
          si = cand;
          break;
        }
      }
      if (si < 0) break;
      __threadfence_block();  // (acquire: the stores of the scans it waited for are visible)
      const int64_t ts = wall_clock64();
      const MsScan& sc = S.scan[si];
      const MsBand bd = ms_band(sc);
      const uint64_t soft = ms_u64(S.soft[si]);
      int rc, nsym = 0;
      int64_t prof[3] = {0, 0, 0};
      const bool wr = ms_i(S.dlen[si]) >= 0;  // destuffed copy (else the stuffed reader)
#define HJ_MS_SCAN(K)                                                                      \
  (wr ? ms_decode_scan<K, MsWBits>(S, si, soft, geo, in, d, cl, sizeu, lv, masks, lane, nsym, \
                                   prof)                                                     \
      : ms_decode_scan<K, MsBits>(S, si, soft, geo, in, d, cl, sizeu, lv, masks, lane, nsym, prof))
      if (!progu)
        rc = HJ_MS_SCAN(kScanSeq);
      else if (bd.ss == 0 && bd.ah == 0)
        rc = HJ_MS_SCAN(kScanDcFirst);
      else if (bd.ss == 0)
        rc = HJ_MS_SCAN(kScanDcRefine);
      else if (bd.ah == 0)
        rc = HJ_MS_SCAN(kScanAcFirst);
      else
#ifdef HJ_MS_PROF
        // (the profile reads prof[])
        rc = wr ? ms_refine_word(S, si, soft, geo, in, d, cl, lv, masks, lane, nsym, prof)
                : HJ_MS_SCAN(kScanAcRefine);
#else
      {
        const int2 rn = wr ? ms_decode_refine<MsWBits>(S, si, soft, geo, in, d, cl, sizeu, lv,
                                                       masks, lane)
                           : ms_decode_refine<MsBits>(S, si, soft, geo, in, d, cl, sizeu, lv,
                                                      masks, lane);
        rc = ms_i(rn.x);
        nsym = ms_i(rn.y);
      }
#endif
#undef HJ_MS_SCAN
      // the scan's stores are visible before it counts as done
      ms_publish(S, si, 1 << 30);
      if (ms_lane0() && si < 16) {
        S.sdiag[3 * si] = (int32_t)(ts - tdec);
        S.sdiag[3 * si + 1] = (int32_t)(wall_clock64() - tdec);
        S.sdiag[3 * si + 2] = nsym;
#ifdef HJ_MS_PROF
        // (profile build: cycles / 256 of the refinement blocks' setup, symbol
        // loops and ends in place of the start / end times)
        if (prof[1]) {
          S.sdiag[3 * si] = (int32_t)(prof[0] >> 8);
          S.sdiag[3 * si + 1] = (int32_t)(prof[1] >> 8);
          S.sdiag[3 * si + 2] = (int32_t)(prof[2] >> 8);
        }
#endif
      }
      if (ms_lane0()) {
        if (rc != kOk) atomicCAS(&S.err, kOk, rc);
        const int sss = ms_i(sc.ss), sah = ms_i(sc.ah);
        const int kind = !progu ? 3 : (sss == 0 ? 0 : (sah == 0 ? 1 : 2));
        atomicAdd(reinterpret_cast<unsigned long long*>(&S.tkind[kind]),
                  (unsigned long long)(wall_clock64() - ts));
        __hip_atomic_fetch_or(&S.done, 1ull << si, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
    __builtin_amdgcn_s_setprio(0);
  }
  __syncthreads();
  tph[2] = wall_clock64() - tdec;  // decode (tables included)
#pragma unroll
  for (int i = 0; i < 4; i++) tdbg[i] = S.tkind[i];
  tdbg[3] = (int64_t)__builtin_amdgcn_s_memtime() - cdec;  // shader clocks of the decode
  tph[1] = 0;
  if (S.err != kOk) {
    if (tid == 0) in.status = S.err;
    return;
  }
  // ---- levels -> coefficient lists (BlockOut layout; dequantised by the IDCT) ----
  for (int j = tid; j < nblocks; j += nt) {
    const int c = in.mcu_comp[j % in.bpm];
    uint4 q[16];
    const uint4* src = reinterpret_cast<const uint4*>(lv + (size_t)j * 64);
#pragma unroll
    for (int i = 0; i < 16; i++) q[i] = src[i];
    int32_t l[64];
#pragma unroll
    for (int i = 0; i < 16; i++) {
      l[4 * i] = (int32_t)q[i].x;
      l[4 * i + 1] = (int32_t)q[i].y;
      l[4 * i + 2] = (int32_t)q[i].z;
      l[4 * i + 3] = (int32_t)q[i].w;
    }
    uint32_t* out = ents + ((size_t)dd.coef_off + j) * 64;
    uint32_t n = 0;
#pragma unroll
    for (int k = 1; k < 64; k++) {
      if (l[k] != 0) {
        out[n++] = ((uint32_t)l[k] << 16) | (uint32_t)k;
      }
    }
    const int32_t dc = (int32_t)(int16_t)(uint16_t)((uint32_t)kDcBias + (uint32_t)l[0] * in.qt[c][0]);
    bdesc[(size_t)dd.coef_off + j] = make_uint2((uint32_t)j * 64u, n | ((uint32_t)dc << 16));
  }
  __syncthreads();
  if (tid == 0) {
    tph[3] = wall_clock64() - t0 - tph[0] - tph[1] - tph[2];  // lists
    for (int i = 0; i < 4; i++) in.tphase[i] = tph[i];
    for (int i = 0; i < 4; i++) in.dbg[i] = tdbg[i];
    for (int i = 0; i < 48; i++) in.sdiag[i] = S.sdiag[i];
    in.sync_rounds = S.nscans;
  }
}

// ---------------------------------------------------------------------------
// idct_kernel
// ---------------------------------------------------------------------------

// Per-thread dense block in LDS, word-major: word w of thread t's block at
// [w][t] (32 words of int16 pairs in the IDCT slot order, kSlotOrder), so any
// access of a wave in which each lane touches its own block -- the scatter of
// a list entry into an arbitrary slot included -- falls on 64 distinct banks
// (a block-major layout took ~4 bank-conflict cycles per LDS instruction in
// the scatter).  Word kBlkWords is a per-thread dummy that takes the
// scatter's stores past the end of a list.
constexpr int kBlkWords = 32;

// (a coefficient's int16 store into the block words: may_alias, or the
// compiler may forward the zeroing word stores to the transform's word loads)
typedef int16_t __attribute__((may_alias)) hj_i16_alias;
typedef __attribute__((address_space(3))) hj_i16_alias hj_lds_i16;
typedef __attribute__((address_space(3))) uint32_t hj_lds_u32;

// idct_kernel<simple> is written for instruction count.  Each of these was
// measured against the form it replaced, which is gone from the tree; the
// numbers are in profiles/r09/idct (ab.txt, counters_summary_no_<NAME>.txt):
//   SEED     the first dot2 of a chain takes its bias as the third operand
//   DCBIAS   the DC-only row shortcut as a bias of the full sums
//   PACK     column sums shifted, clipped and packed two at a time
//   SCATTER  half-word operand selects in the list scatter
//   GATHER   a group's 16 dequantisation-table reads ahead of its 16 stores
//   INDEX    block -> (MCU, block of MCU, MCU column, row) by multiplication
//            (idct_divmod, hj_common.h)

// byte offset of IDCT slot s (kSlotOrder) in the word-major block of NT threads
template <int NT>
__device__ __forceinline__ uint32_t slot_byte(uint32_t s) {
  return (s >> 1) * (uint32_t)NT * 4u + ((s & 1u) << 1);
}

// The IDCT kernels' dequantisation table, per component and zig-zag index:
// the coefficient's byte offset in the word-major block (its IDCT slot,
// kSlotOrder) | quantiser << 16.  Filled by the workgroup before its blocks.
template <int NT>
__device__ __forceinline__ void load_dequant(uint32_t (&sq)[kMaxComp][64], const ImageInfo& in,
                                             int tid) {
  for (int k = tid; k < kMaxComp * 64; k += NT)
    sq[k >> 6][k & 63] = slot_byte<NT>(kSlotOrder[k & 63]) | ((uint32_t)in.qt[k >> 6][k & 63] << 16);
}

// One block's coefficient list (see BlockOut: DC final in bd; AC entries
// level << 16 | zig-zag index) into the thread's word-major block (b32: its
// word 0; zeroed here), dequantised on the way (sqc: the component's row of
// the dequantisation table).  (A list may start inside a 16-byte group: a
// run's lists are packed back to back; entries [lo, lo + count) of the groups
// from `start`.)
template <int NT>
__device__ __forceinline__ void list_block(const uint32_t* __restrict__ ents, const uint2 bd,
                                           const int64_t coef_off, const int nblocks,
                                           const uint32_t* sqc, uint32_t* b32) {
#pragma unroll
  for (int w = 0; w < kBlkWords; w++) b32[w * NT] = w == 0 ? (bd.y >> 16) : 0u;
  // (b32 points into the kernel's LDS: 32-bit LDS addresses)
  const uint32_t blk_a = (uint32_t)(uintptr_t)(hj_lds_u32*)b32;
  const uint32_t dummy_a = blk_a + (uint32_t)(kBlkWords * NT * 4);
  const uint32_t cap = (uint32_t)nblocks * 64u;
  const uint32_t lo = bd.x & 3u, start = bd.x & ~3u;
  uint32_t count = min(bd.y & 0xFFFFu, 63u);
  if (start > cap - 64u) count = 0;  // only an unwritten list (a failed scan)
  const uint4* e4 = reinterpret_cast<const uint4*>(ents + (size_t)coef_off * 64 + start);
  const uint32_t n4 = (lo + count + 3u) >> 2;
  for (uint32_t i = 0; i < n4; i += 4) {
    // unconditional loads (index clamped into the list), then the scatter
    uint4 q[4];
#pragma unroll
    for (int u = 0; u < 4; u++) q[u] = e4[min(i + u, n4 - 1u)];
    // the 16 table words ahead of the 16 stores: a store may alias the table
    // for all the compiler knows, so read entry by entry each table read
    // waits for the store before it and each store for its read -- 16 LDS
    // round trips in a row
    uint32_t qsv[16];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      qsv[4 * u] = sqc[q[u].x & 63u];
      qsv[4 * u + 1] = sqc[q[u].y & 63u];
      qsv[4 * u + 2] = sqc[q[u].z & 63u];
      qsv[4 * u + 3] = sqc[q[u].w & 63u];
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const uint32_t w[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
#pragma unroll
      for (int h = 0; h < 4; h++) {  // (outside the list: into the dummy word)
        const uint32_t k = 4u * (i + u) + h;
        const uint32_t qs = qsv[4 * u + h];
        // the entry's and the table word's halves picked by the instructions
        // themselves (SDWA): level x quantiser from the high halves, block
        // address + slot offset from the low half; k in [lo, lo + count) as
        // one unsigned compare
        uint32_t in_a, prod;
        asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD "
            "src1_sel:WORD_0"
            : "=v"(in_a)
            : "v"(blk_a), "v"(qs));
        asm("v_mul_lo_u16_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 "
            "src1_sel:WORD_1"
            : "=v"(prod)
            : "v"(w[h]), "v"(qs));
        const uint32_t a32 = k - lo < count ? in_a : dummy_a;
        *reinterpret_cast<hj_lds_i16*>(a32) = (int16_t)prod;
      }
    }
  }
}

// FFmpeg simple_idct (8-bit) on packed int16 pairs with v_dot2_i32_i16: a
// row of the slot block is (x0, x2), (x4, x6), (x1, x3), (x5, x7), so each
// even / odd partial sum of a pass is two dot2 steps.  The products and
// 32-bit sums are the C code's exactly (oracle simple_row / simple_col_put;
// the C code's unsigned wrap-around equals the dot2's modular int32 sum).
typedef short hj_s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int32_t dot2(uint32_t a, uint32_t w, int32_t c) {
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(hj_s16x2, a), __builtin_bit_cast(hj_s16x2, w),
                                c, false);
}
constexpr uint32_t pk16(int lo, int hi) {
  return (uint32_t)(uint16_t)(int16_t)lo | ((uint32_t)(uint16_t)(int16_t)hi << 16);
}
// low halves of lo and hi as one pair (v_perm)
__device__ __forceinline__ uint32_t pack_lo16(uint32_t lo, uint32_t hi) {
  return __builtin_amdgcn_perm(hi, lo, 0x05040100u);
}
// The first dot2 of a chain.  The builtin becomes the two-operand
// v_dot2c_i32_i16, which accumulates in place and so costs a v_mov of the bias
// (or of 0) per chain; the three-operand form reads the bias where it is.  Its
// weight is an SGPR (VOP3: one constant-bus operand, no literal).
__device__ __forceinline__ int32_t dot2_seed(uint32_t a, uint32_t w, int32_t c) {
  int32_t d;
  asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "s"(w), "v"(c));
  return d;
}
__device__ __forceinline__ int32_t dot2_seed0(uint32_t a, uint32_t w) {
  int32_t d;
  asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(d) : "v"(a), "s"(w));
  return d;
}
// an 8-point pass: a[k] even sums (+ bias), b[k] odd sums
__device__ __forceinline__ void sidct8(uint32_t e0, uint32_t e1, uint32_t o0, uint32_t o1,
                                       int32_t bias, int32_t (&a)[4], int32_t (&b)[4]) {
  a[0] = dot2(e1, pk16(kW4, kW6), dot2_seed(e0, pk16(kW4, kW2), bias));
  a[1] = dot2(e1, pk16(-kW4, -kW2), dot2_seed(e0, pk16(kW4, kW6), bias));
  a[2] = dot2(e1, pk16(-kW4, kW2), dot2_seed(e0, pk16(kW4, -kW6), bias));
  a[3] = dot2(e1, pk16(kW4, -kW6), dot2_seed(e0, pk16(kW4, -kW2), bias));
  b[0] = dot2(o1, pk16(kW5, kW7), dot2_seed0(o0, pk16(kW1, kW3)));
  b[1] = dot2(o1, pk16(-kW1, -kW5), dot2_seed0(o0, pk16(kW3, -kW7)));
  b[2] = dot2(o1, pk16(kW7, kW3), dot2_seed0(o0, pk16(kW5, -kW1)));
  b[3] = dot2(o1, pk16(kW3, -kW1), dot2_seed0(o0, pk16(kW7, -kW5)));
}
// row i of the word-major block: words 4i..4i+3
template <int NT>
__device__ __forceinline__ uint4 blk_row(const uint32_t* b32, int i) {
  return make_uint4(b32[(4 * i) * NT], b32[(4 * i + 1) * NT], b32[(4 * i + 2) * NT],
                    b32[(4 * i + 3) * NT]);
}
// The row pass.  b32: the thread's word 0 of the word-major block; r[i][k]:
// row i's output k, truncated to int16 by the column pass's packing (FFmpeg
// keeps the rows in the int16 block; only the low halves are used).
// DC-only rows (x1..x7 zero) are x0 << 3 in all eight places
// (idctRowCondDC).  As a bias: with 1024 + x0 every even sum is
// kW4 x0 + x0 + 1024 = 16384 x0 + 1024 and every odd sum 0, so >> 11 leaves
// 8 x0 exactly, the int16 truncation being the shortcut's.  (The plain full
// path differs from the shortcut wherever |x0| > 1024.)
template <int NT>
__device__ __forceinline__ void simple_idct_rows(const uint32_t* b32, uint32_t (&r)[8][8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint4 q = blk_row<NT>(b32, i);
    int32_t a[4], b[4];
    const bool dc_only = ((q.x >> 16) | q.y | q.z | q.w) == 0u;
    sidct8(q.x, q.y, q.z, q.w, (1 << 10) + (dc_only ? sext16(q.x) : 0), a, b);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      r[i][k] = (uint32_t)((int32_t)((uint32_t)a[k] + (uint32_t)b[k]) >> 11);
      r[i][7 - k] = (uint32_t)((int32_t)((uint32_t)a[k] - (uint32_t)b[k]) >> 11);
    }
  }
}
// column k of the row pass's output: s[j] = the sum of row j before >> 20.
// (c0 + 32) W4 = c0 W4 + 32 W4
__device__ __forceinline__ void simple_idct_col(const uint32_t (&r)[8][8], int k,
                                                int32_t (&s)[8]) {
  int32_t a[4], b[4];
  sidct8(pack_lo16(r[0][k], r[2][k]), pack_lo16(r[4][k], r[6][k]), pack_lo16(r[1][k], r[3][k]),
         pack_lo16(r[5][k], r[7][k]), kW4 * ((1 << 19) / kW4), a, b);
#pragma unroll
  for (int u = 0; u < 4; u++) {
    s[u] = (int32_t)((uint32_t)a[u] + (uint32_t)b[u]);
    s[7 - u] = (int32_t)((uint32_t)a[u] - (uint32_t)b[u]);
  }
}

// four column sums -> clip_u8(s >> 20) as the bytes of a word, a first.
// v_ashr_pk_u8_i32 shifts two sums and saturates them to bytes 0 and 1 of
// its result; what it leaves in bytes 2..3 is not relied on (see
// clip_u8_opaque, hj_idct.h: the compiler's own use of it assumes zero there,
// which the hardware does not give), the v_perm takes the low halves only.
// 3 instructions per 4 pixels (11 as shifts, v_med3 and ors; 7 through the
// high halves, a packed 16-bit shift and v_sat_pk_u8_i16:
// profiles/r09/idct/not_kept.txt).
__device__ __forceinline__ uint32_t clip_pair(int32_t a, int32_t b) {
  uint32_t u;
  asm("v_ashr_pk_u8_i32 %0, %1, %2, 20" : "=v"(u) : "v"(a), "v"(b));
  return u;
}
__device__ __forceinline__ uint32_t clip_pack4(int32_t a, int32_t b, int32_t c, int32_t d) {
  return __builtin_amdgcn_perm(clip_pair(c, d), clip_pair(a, b), 0x05040100u);
}
// rows: the block's 8 pixel rows as the words the kernels store
template <int NT>
__device__ __forceinline__ void simple_idct_packed(const uint32_t* b32, uint2 (&rows)[8]) {
  uint32_t r[8][8];
  simple_idct_rows<NT>(b32, r);
  int32_t s[8][8];  // [column][row]
#pragma unroll
  for (int k = 0; k < 8; k++) simple_idct_col(r, k, s[k]);
#pragma unroll
  for (int j = 0; j < 8; j++) {
    rows[j].x = clip_pack4(s[0][j], s[1][j], s[2][j], s[3][j]);
    rows[j].y = clip_pack4(s[4][j], s[5][j], s[6][j], s[7][j]);
  }
}

// The thread's LDS block (b32: its word 0) -> 8x8 pixels (u8 values in
// int32), row-major: the islow transform (IDCT 1) or none (2).
template <int NT, int IDCT>
__device__ __forceinline__ void idct_block(const uint32_t* b32, int32_t (&px)[64]) {
  static_assert(IDCT == 1 || IDCT == 2, "the simple IDCT packs its own rows (simple_idct_packed)");
  // natural order from the slot layout (a compile-time permutation)
  int32_t blk[64];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint4 q = blk_row<NT>(b32, i);
    blk[8 * i + 0] = sext16(q.x);
    blk[8 * i + 2] = sext16(q.x >> 16);
    blk[8 * i + 4] = sext16(q.y);
    blk[8 * i + 6] = sext16(q.y >> 16);
    blk[8 * i + 1] = sext16(q.z);
    blk[8 * i + 3] = sext16(q.z >> 16);
    blk[8 * i + 5] = sext16(q.w);
    blk[8 * i + 7] = sext16(q.w >> 16);
  }
  if (IDCT == 2) {
#pragma unroll
    for (int i = 0; i < 64; i++) px[i] = blk[i] & 255;
  } else {
    islow_block(blk, px);
  }
}

// The same as the 8 pixel rows a kernel stores (bytes in x order).
template <int NT, int IDCT>
__device__ __forceinline__ void idct_block_rows(const uint32_t* b32, uint2 (&rows)[8]) {
  if constexpr (IDCT == 0) {
    simple_idct_packed<NT>(b32, rows);
  } else {
    int32_t px[64];
    idct_block<NT, IDCT>(b32, px);
#pragma unroll
    for (int r = 0; r < 8; r++) {
      rows[r].x = (uint32_t)px[8 * r] | ((uint32_t)px[8 * r + 1] << 8) |
                  ((uint32_t)px[8 * r + 2] << 16) | ((uint32_t)px[8 * r + 3] << 24);
      rows[r].y = (uint32_t)px[8 * r + 4] | ((uint32_t)px[8 * r + 5] << 8) |
                  ((uint32_t)px[8 * r + 6] << 16) | ((uint32_t)px[8 * r + 7] << 24);
    }
  }
}

// XCD-aware workgroup order: workgroups b and b + 8 share an XCD (observed
// round-robin dispatch, MI355X_MICROARCH.md -- speed only, never
// correctness), so the grid's linear index b is taken as tile
// (b % 8) * Q + b / 8: each XCD gets a contiguous range of tiles in dispatch
// order (a tail of fewer than 8 keeps its place).  (bx, by, bz) in and out.
__device__ __forceinline__ void xcd_order(uint32_t& bx, uint32_t& by, uint32_t& bz) {
  const uint32_t n_wg = gridDim.x * gridDim.y * gridDim.z, full = n_wg & ~7u;
  uint32_t lin = bx + gridDim.x * (by + gridDim.y * bz);
  if (lin < full) lin = (lin & 7u) * (full >> 3) + (lin >> 3);
  bx = lin % gridDim.x;
  by = (lin / gridDim.x) % gridDim.y;
  bz = lin / (gridDim.x * gridDim.y);
}

template <int IDCT>
__global__ void __launch_bounds__(kIdctThreads) idct_kernel(const uint32_t* __restrict__ ents,
                                                            const uint2* __restrict__ bdesc,
                                                            const ImageDesc* __restrict__ desc,
                                                            const ImageInfo* __restrict__ infos,
                                                            uint8_t* __restrict__ planes,
                                                            const uint32_t* __restrict__ idct_map,
                                                            const int xcd) {
  __shared__ __attribute__((aligned(16))) uint32_t sblk[kBlkWords + 1][kIdctThreads];
  __shared__ uint32_t sq[kMaxComp][64];
  // (tile, image) grid, or a flat grid over every image's block tiles
  // (idct_map: workgroup -> image) when the batch's sizes differ widely;
  // xcd: XCD-aware order ("xcd_order" bit 1: neighbouring tiles of one plane
  // row share their edge lines in one L2)
  uint32_t gx = blockIdx.x, gy = blockIdx.y, gz = blockIdx.z;
  if (xcd) xcd_order(gx, gy, gz);
  const bool flat = idct_map != nullptr;
  const int img = flat ? (int)idct_map[gx] : (int)gy;
  const int tile = flat ? (int)gx - desc[img].idct_wg0 : (int)gx;
  int j = tile * kIdctThreads + threadIdx.x;
  const ImageInfo& in = infos[img];
  const ImageDesc& dd = desc[img];
  // (nblocks, or the blocks of the MCU rectangle a source crop touches)
  const int nb = dd.idct_blocks;
  if (in.status != kOk || tile * kIdctThreads >= nb) return;
  load_dequant<kIdctThreads>(sq, in, threadIdx.x);
  __syncthreads();
  if (j >= nb) return;
  if (dd.reg_mw)
    j = (int)idct_region_block(in, dd.reg_mx0, dd.reg_my0, dd.reg_mw, dd.reg_mw_magic, (uint32_t)j);
  const IdctBlockPos bp = idct_block_pos(in, (uint32_t)j);
  const int c = bp.c;
  uint32_t* b32 = &sblk[0][threadIdx.x];
  list_block<kIdctThreads>(ents, bdesc[(size_t)dd.coef_off + j], dd.coef_off, in.nblocks, sq[c],
                           b32);
  uint2 rows[8];
  idct_block_rows<kIdctThreads, IDCT>(b32, rows);
  const int stride = dd.plane_stride[c];
  uint8_t* dst = planes + dd.plane_off[c] + (size_t)bp.by * 8 * stride + bp.bx * 8;
#pragma unroll
  for (int r = 0; r < 8; r++) *reinterpret_cast<uint2*>(dst + (size_t)r * stride) = rows[r];
}

// ---------------------------------------------------------------------------
// idct_lowres_kernel: the IDCT stage of a submission with reduced-size images
// (spdl_hj_set_lowres; FFmpeg's lowres 1..3, hj_idct.h lowres_idct4 / 2 / 1)
// ---------------------------------------------------------------------------
//
// A block yields P x P samples, P = 8 >> L, so one thread per block would
// store 4, 2 or 1 bytes a row.  The levels are organised by output instead: a
// lane owns 8 consecutive bytes of each of the P plane rows of one block row
// and fetches the 2^L blocks under them, so every store of every level is 8
// bytes (uint2) at an 8-byte aligned address, P of them per lane -- the store
// width of idct_kernel.  A plane's stride is 8 bytes a lane
// (hj_layout.h lowres_lanes_row): the lanes of a block row tile the stride
// exactly, blocks past the component's last one are written as zeros, and so
// the stage writes every byte of every plane it lays out.
//
// Read set per block: L = 3 its descriptor alone (the DC is final there);
// L = 2 / 1 the list entries up to the first whose zig-zag index is above 4 /
// 24 -- the last index of the 2x2 / 4x4 corner; the lists are in zig-zag order
// -- of which those in the 4x4 corner are dequantised and scattered into the
// lane's corner in LDS (word-major like idct_kernel's block: word w of lane t
// at [w][t], word 16 a dummy for the entries outside the corner).
//
// The level is per image, so workgroup-uniform (the flat grid's idct_map).
// An image of level 0 is transformed as idct_kernel transforms it.

// sq for the reduced levels, per component and zig-zag index: the
// coefficient's corner word (row * 4 + column; 16 outside the 4x4 corner) |
// quantiser << 16
__device__ __forceinline__ void load_dequant_corner(uint32_t (&sq)[kMaxComp][64], const ImageInfo& in,
                                                    int tid) {
  for (int k = tid; k < kMaxComp * 64; k += kIdctThreads) {
    const uint32_t slot = kSlotOrder[k & 63], r = slot >> 3, s = slot & 7u;
    const uint32_t col = ((s & 3u) << 1) | (s >> 2);  // (kSlotOrder's pairing undone)
    const uint32_t word = r < 4u && col < 4u ? r * 4u + col : 16u;
    sq[k >> 6][k & 63] = word | ((uint32_t)in.qt[k >> 6][k & 63] << 16);
  }
}

// A block's list as the corner walk reads it: the 16-byte groups from the
// one its first entry lies in (a run's lists are packed back to back, so a
// list may start inside a group: entries [lo, lo + count) of the groups), the
// first NQ of them loaded here -- ahead of any use, so that a lane's blocks
// have their loads in flight together.
template <int NQ>
struct CornerList {
  const uint4* e4;
  uint32_t lo, count, n4;
  uint4 q[NQ];
};
template <int NQ>
__device__ __forceinline__ CornerList<NQ> corner_list(const uint32_t* __restrict__ ents,
                                                      const uint2 bd, const int64_t coef_off,
                                                      const int nblocks) {
  CornerList<NQ> l;
  const uint32_t cap = (uint32_t)nblocks * 64u, start = bd.x & ~3u;
  l.lo = bd.x & 3u;
  l.count = min(bd.y & 0xFFFFu, 63u);
  l.e4 = reinterpret_cast<const uint4*>(ents + (size_t)coef_off * 64 + start);
  l.n4 = (l.lo + l.count + 3u) >> 2;
  if (start > cap - 64u) l.count = l.n4 = 0;  // only an unwritten list (a failed scan)
#pragma unroll
  for (int u = 0; u < NQ; u++)
    l.q[u] = l.n4 ? l.e4[min((uint32_t)u, l.n4 - 1u)] : make_uint4(0u, 0u, 0u, 0u);
  return l;
}

// The corner's AC coefficients of list `l` into the lane's LDS words (col: the
// lane's word 0; stride kIdctThreads words), zeroed first.  ZMAX: the corner's
// last zig-zag index.  The entries are in zig-zag order, so one test per entry
// (in the list, index <= ZMAX) leaves out what lies behind the corner, and a
// trip whose last entry is past ZMAX is the last: most blocks take one trip of
// NQ groups, every load of it unconditional and issued together.
template <int ZMAX, int NQ>
__device__ __forceinline__ void corner_scatter(const CornerList<NQ>& l, const uint32_t* sqc,
                                               uint32_t* col) {
#pragma unroll
  for (int w = 1; w < 16; w++)
    if (ZMAX > 4 || w == 1 || w == 4 || w == 5) col[w * kIdctThreads] = 0u;
  for (uint32_t i = 0; i < l.n4; i += NQ) {
    uint4 q[NQ];
#pragma unroll
    for (int u = 0; u < NQ; u++) q[u] = i == 0 ? l.q[u] : l.e4[min(i + u, l.n4 - 1u)];
#pragma unroll
    for (int u = 0; u < NQ; u++) {
      const uint32_t w[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
#pragma unroll
      for (int h = 0; h < 4; h++) {
        const uint32_t k = 4u * (i + u) + h, zz = w[h] & 63u;
        const uint32_t qs = sqc[zz];
        const bool take = k - l.lo < l.count && zz <= (uint32_t)ZMAX;
        // (the int16 product the sequential decoder stores; outside: the dummy word)
        col[(take ? (qs & 0xFFFFu) : 16u) * kIdctThreads] = (uint32_t)sext16((w[h] >> 16) * (qs >> 16));
      }
    }
    if ((q[NQ - 1].w & 63u) > (uint32_t)ZMAX) break;
  }
}

// One lane of level LV: lane `j` of the image's lanes, components in order,
// each plane's block rows top to bottom, ceil(bw / 2^LV) lanes to a block row.
template <int LV>
__device__ __forceinline__ void lowres_lane(const uint32_t* __restrict__ ents,
                                            const uint2* __restrict__ bdesc, const ImageDesc& dd,
                                            const ImageInfo& in, uint8_t* __restrict__ planes,
                                            const uint32_t (&sq)[kMaxComp][64], uint32_t* col, int j) {
  constexpr int NB = 1 << LV, P = 8 >> LV;
  int c = 0, base = 0, lr = 0;
  for (; c < in.ncomp; c++) {
    lr = (in.comp_bw[c] + NB - 1) >> LV;
    const int cnt = lr * in.comp_bh[c];
    if (j < cnt) break;
    j -= cnt;
    base += in.comp_h[c] * in.comp_v[c];
  }
  if (c >= in.ncomp) return;  // (the planner counted the same lanes: never)
  const int by = j / lr, gx = j - by * lr;
  const int bw = in.comp_bw[c], hc = in.comp_h[c], vc = in.comp_v[c];
  uint32_t lo[P], hi[P];
#pragma unroll
  for (int r = 0; r < P; r++) lo[r] = hi[r] = 0u;
  // the lane's descriptors, then (levels 1 and 2) the head of every list, all
  // ahead of the first transform: 16 / 8 entries cover most corners
  constexpr int ZMAX = LV == 1 ? 24 : 4, NQ = LV == 1 ? 4 : 2;
  uint2 bd[NB];
#pragma unroll
  for (int k = 0; k < NB; k++) {
    const int bx = min(gx * NB + k, bw - 1);  // (past the last block: its neighbour, unused)
    // block (bx, by) of component c in the image's MCU order
    const int jb = in.ncomp == 1 ? by * in.mcux + bx
                                 : ((by / vc) * in.mcux + bx / hc) * in.bpm + base + (by % vc) * hc +
                                       bx % hc;
    bd[k] = bdesc[(size_t)dd.coef_off + jb];
  }
  CornerList<NQ> lists[LV == 3 ? 1 : NB];
  if constexpr (LV != 3) {
#pragma unroll
    for (int k = 0; k < NB; k++) lists[k] = corner_list<NQ>(ents, bd[k], dd.coef_off, in.nblocks);
  }
#pragma unroll
  for (int k = 0; k < NB; k++) {
    if (gx * NB + k >= bw) continue;  // (past the component's last block: zeros)
    int32_t px[P * P];
    if constexpr (LV == 3) {
      px[0] = lowres_idct1(sext16(bd[k].y >> 16));
    } else {
      corner_scatter<ZMAX, NQ>(lists[k], sq[c], col);
      int32_t b[16];
      b[0] = sext16(bd[k].y >> 16);
#pragma unroll
      for (int w = 1; w < 16; w++)
        b[w] = (LV == 1 || w == 1 || w == 4 || w == 5) ? (int32_t)col[w * kIdctThreads] : 0;
      if constexpr (LV == 1) lowres_idct4(b, 4, px, 4);
      else lowres_idct2(b, 4, px, 2);
    }
    // its P bytes of each row: bytes [k P, k P + P) of the lane's eight
#pragma unroll
    for (int r = 0; r < P; r++)
#pragma unroll
      for (int x = 0; x < P; x++) {
        const int byte = k * P + x;
        const uint32_t v = (uint32_t)px[r * P + x] << (8 * (byte & 3));
        if (byte < 4) lo[r] |= v;
        else hi[r] |= v;
      }
  }
  const int stride = dd.plane_stride[c];
  uint8_t* dst = planes + dd.plane_off[c] + (size_t)by * P * stride + gx * 8;
#pragma unroll
  for (int r = 0; r < P; r++)
    *reinterpret_cast<uint2*>(dst + (size_t)r * stride) = make_uint2(lo[r], hi[r]);
}

template <int IDCT>
__global__ void __launch_bounds__(kIdctThreads) idct_lowres_kernel(
    const uint32_t* __restrict__ ents, const uint2* __restrict__ bdesc,
    const ImageDesc* __restrict__ desc, const ImageInfo* __restrict__ infos,
    uint8_t* __restrict__ planes, const uint32_t* __restrict__ idct_map,
    const uint8_t* __restrict__ levels) {
  __shared__ __attribute__((aligned(16))) uint32_t sblk[kBlkWords + 1][kIdctThreads];
  __shared__ uint32_t sq[kMaxComp][64];
  const int img = (int)idct_map[blockIdx.x];
  const ImageInfo& in = infos[img];
  const ImageDesc& dd = desc[img];
  const int tile = (int)blockIdx.x - dd.idct_wg0;
  const int nb = dd.idct_blocks;  // (the image's lanes: hj_layout.h Layout::lowres)
  const int lv = levels[img];
  if (in.status != kOk || tile * kIdctThreads >= nb) return;
  const int j = tile * kIdctThreads + threadIdx.x;
  uint32_t* b32 = &sblk[0][threadIdx.x];
  if (lv == 0) {
    load_dequant<kIdctThreads>(sq, in, threadIdx.x);
    __syncthreads();
    if (j >= nb) return;
    const IdctBlockPos bp = idct_block_pos(in, (uint32_t)j);
    const int c = bp.c;
    list_block<kIdctThreads>(ents, bdesc[(size_t)dd.coef_off + j], dd.coef_off, in.nblocks, sq[c],
                             b32);
    uint2 rows[8];
    idct_block_rows<kIdctThreads, IDCT>(b32, rows);
    const int stride = dd.plane_stride[c];
    uint8_t* dst = planes + dd.plane_off[c] + (size_t)bp.by * 8 * stride + bp.bx * 8;
#pragma unroll
    for (int r = 0; r < 8; r++) *reinterpret_cast<uint2*>(dst + (size_t)r * stride) = rows[r];
    return;
  }
  if (lv < 3) {  // (level 3 reads no list: no table)
    load_dequant_corner(sq, in, threadIdx.x);
    __syncthreads();
  }
  if (j >= nb) return;
  if (lv == 1) lowres_lane<1>(ents, bdesc, dd, in, planes, sq, b32, j);
  else if (lv == 2) lowres_lane<2>(ents, bdesc, dd, in, planes, sq, b32, j);
  else lowres_lane<3>(ents, bdesc, dd, in, planes, sq, b32, j);
}

// ---------------------------------------------------------------------------
// colour conversion (IJG jdcolor.c / jdmerge.c integer tables, SCALEBITS 16)
// ---------------------------------------------------------------------------

constexpr int32_t kFix1402 = 91881, kFix1772 = 116130, kFix0714 = 46802, kFix0344 = 22553;

__device__ __forceinline__ void ycc_rgb(int y, int cb, int cr, int* rgb) {
  const int32_t x_cb = cb - 128, x_cr = cr - 128;
  const int32_t cr_r = (kFix1402 * x_cr + 32768) >> 16;
  const int32_t cb_b = (kFix1772 * x_cb + 32768) >> 16;
  const int32_t g = ((-kFix0344 * x_cb + 32768) + (-kFix0714 * x_cr)) >> 16;
  rgb[0] = clip_u8(y + cr_r);
  rgb[1] = clip_u8(y + g);
  rgb[2] = clip_u8(y + cb_b);
}

// fp32 -> 16-bit output: dtype 1 = IEEE half (RNE), 2 = bfloat16 (RNE, as
// torch's Tensor.to(torch.bfloat16) after the reference's fp32 normalisation,
// examples/imagenet_classification.py:95-106,162-163).
__device__ __forceinline__ uint16_t to_f16_bits(float f, int dtype) {
  if (dtype == 1) return __half_as_ushort(__float2half_rn(f));
  uint32_t x = __float_as_uint(f);
  if ((x & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((x >> 16) | 0x40u);
  x += 0x7FFFu + ((x >> 16) & 1u);
  return (uint16_t)(x >> 16);
}

__device__ __forceinline__ void store_rgb(void* out, int64_t base, int fmt, int dtype, int ow,
                                          int oh, int x, int y, const int* rgb,
                                          const BatchParams& p) {
  const bool planar = fmt == 0 || fmt == 1;
  const bool swap = fmt == 1 || fmt == 3;
  const int64_t pl = (int64_t)ow * oh;
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    const int v = rgb[swap ? 2 - ch : ch];
    const int64_t oi = base + (planar ? ch * pl + (int64_t)y * ow + x : ((int64_t)y * ow + x) * 3 + ch);
    if (dtype == 0) {
      static_cast<uint8_t*>(out)[oi] = (uint8_t)v;
    } else {
      float f = __fdiv_rn((float)v, 255.0f);
      f = __fsub_rn(f, p.mean[ch]);
      f = __fdiv_rn(f, p.std[ch]);
      static_cast<uint16_t*>(out)[oi] = to_f16_bits(f, dtype);
    }
  }
}

__global__ void __launch_bounds__(256) csc_kernel(const uint8_t* __restrict__ planes,
                                                  const ImageDesc* __restrict__ desc,
                                                  const ImageInfo* __restrict__ infos,
                                                  void* __restrict__ out, const BatchParams p,
                                                  int32_t* __restrict__ host_status) {
  const int img = blockIdx.y;
  const ImageInfo& in = infos[img];
  if (host_status && blockIdx.x == 0 && threadIdx.x == 0) host_status[img] = in.status;
  if (in.status != kOk) return;
  const ImageDesc& dd = desc[img];
  const int W = in.width, H = in.height;
  const int64_t npx = (int64_t)W * H;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npx;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
    // (the first component from its own grid too: luma sampled below chroma
    // is legal for libjpeg, whose plain upsampler replicates)
    const int lx = x * in.comp_h[0] / in.hmax, ly = y * in.comp_v[0] / in.vmax;
    const int yv = planes[dd.plane_off[0] + (int64_t)ly * dd.plane_stride[0] + lx];
    int rgb[3];
    if (in.ncomp == 1) {
      rgb[0] = rgb[1] = rgb[2] = yv;
    } else {
      const int cx1 = x * in.comp_h[1] / in.hmax, cy1 = y * in.comp_v[1] / in.vmax;
      const int cx2 = x * in.comp_h[2] / in.hmax, cy2 = y * in.comp_v[2] / in.vmax;
      const int cb = planes[dd.plane_off[1] + (int64_t)cy1 * dd.plane_stride[1] + cx1];
      const int cr = planes[dd.plane_off[2] + (int64_t)cy2 * dd.plane_stride[2] + cx2];
      if (in.color == kColorRgb) {  // libjpeg's RGB-coded frame: a copy (1x1)
        rgb[0] = yv;
        rgb[1] = cb;
        rgb[2] = cr;
      } else {
        ycc_rgb(yv, cb, cr, rgb);
      }
    }
    store_rgb(out, dd.out_off, p.pix_fmt, p.dtype, W, H, x, y, rgb, p);
  }
}

// ---------------------------------------------------------------------------
// sws_kernel: the reference CPU path's swscale conversion -- scale to the
// content size + yuvj -> rgb24 in one pass (the graph's scale filter outputs
// rgb24 itself, src/libspdl/core/detail/ffmpeg/filter_graph.cpp:280-313) --
// then pad (black) / crop, optional (x/255 - mean)/std, stores in the
// caller's layout.  Workgroup = (band of output rows, chunk of output
// columns, image).  The band's source rows are scaled horizontally into LDS
// (hScale8To15: one thread per column, taps in registers as lo / hi bytes,
// v_dot4 on the source bytes), then each output pixel runs the vertical taps
// and the RGB24 writer swscale picks for its row (yuv2rgb_{X,2,1}_c table
// path, a pixel pair per work item, or the _full_ path, libswscale/output.c).  Tables come from the host plan (hj_sws.cpp);
// arithmetic: oracle/sws_oracle.c.
// ---------------------------------------------------------------------------

typedef short hj_short2 __attribute__((ext_vector_type(2)));
// 16-byte vector load from a 4-byte aligned address (gfx950 global loads
// allow it): one global_load_dwordx4 instead of four dword loads
typedef uint32_t hj_u32x4a __attribute__((ext_vector_type(4), aligned(4)));

// NW dwords (NW % 4 == 0) from a 4-byte aligned address, 16 bytes at a time
template <int NW>
__device__ __forceinline__ void load_words(const uint8_t* p, uint32_t (&w)[NW]) {
  static_assert(NW % 4 == 0, "whole 16-byte loads");
#pragma unroll
  for (int i = 0; i < NW; i += 4) {
    const hj_u32x4a v = *reinterpret_cast<const hj_u32x4a*>(p + 4 * i);
    w[i] = v.x;
    w[i + 1] = v.y;
    w[i + 2] = v.z;
    w[i + 3] = v.w;
  }
}

// sum over t < 4*NQ of byte (sh + t) of w times tap t: realign (v_alignbyte),
// widen to int16 pairs (v_perm), accumulate with v_dot2 against packed taps
template <int NQ, int NW>
__device__ __forceinline__ int32_t hdot(const uint32_t (&w)[NW], uint32_t sh, const uint32_t* wp) {
  int32_t h = 0;
#pragma unroll
  for (int i = 0; i < NQ; i++) {
    const uint32_t u = __builtin_amdgcn_alignbyte(w[i + 1], w[i], sh);
    const uint32_t lo = __builtin_amdgcn_perm(0u, u, 0x0C010C00u);  // bytes 0,1 -> int16 x2
    const uint32_t hi = __builtin_amdgcn_perm(0u, u, 0x0C030C02u);  // bytes 2,3
    h = __builtin_amdgcn_sdot2(__builtin_bit_cast(hj_short2, lo),
                               __builtin_bit_cast(hj_short2, wp[2 * i]), h, false);
    h = __builtin_amdgcn_sdot2(__builtin_bit_cast(hj_short2, hi),
                               __builtin_bit_cast(hj_short2, wp[2 * i + 1]), h, false);
  }
  return h;
}

// The same sum with v_dot4 on the bytes themselves, no widening: a tap splits
// as 256 * hi + lo (lo 0..255, hi -128..127: any int16 tap), and with
// p' = p ^ 0x80 = p - 128 as a signed byte
//   sum p * tap = udot4(p, lo) + 256 * (sdot4(p', hi) + 128 * sum hi)
// modulo 2^32, which is what the v_dot2 sum is too.  wp[2i] holds the lo
// bytes of taps 4i .. 4i + 3, wp[2i + 1] the hi bytes; k0 = 128 * sum hi.
// 4 taps: 1 align + 1 xor + 2 dot4 against 1 align + 2 perm + 2 dot2.
template <int NQ, int NW>
__device__ __forceinline__ int32_t hdot4(const uint32_t (&w)[NW], uint32_t sh, const uint32_t* wp,
                                         int32_t k0) {
  uint32_t a = 0;
  int32_t b = k0;
#pragma unroll
  for (int i = 0; i < NQ; i++) {
    const uint32_t u = __builtin_amdgcn_alignbyte(w[i + 1], w[i], sh);
    a = __builtin_amdgcn_udot4(u, wp[2 * i], a, false);
    b = __builtin_amdgcn_sdot4((int32_t)(u ^ 0x80808080u), (int32_t)wp[2 * i + 1], b, false);
  }
  return (int32_t)(a + ((uint32_t)b << 8));
}

// the taps 4k .. 4k + 3 of a table row (int16 x4) as hdot4's lo and hi words;
// returns the sum of the four hi bytes
__device__ __forceinline__ int32_t split_taps(uint2 t, uint32_t& lo, uint32_t& hi, int32_t sum) {
  lo = __builtin_amdgcn_perm(t.y, t.x, 0x06040200u);
  hi = __builtin_amdgcn_perm(t.y, t.x, 0x07050301u);
  return __builtin_amdgcn_sdot4((int32_t)hi, 0x01010101, sum, false);
}

__device__ __forceinline__ int16_t h15(int32_t h) {  // hScale8To15: (sum >> 7), capped
  return (int16_t)min(h >> 7, (1 << 15) - 1);
}

// (Inlined: through a call the plane and LDS pointers turn generic and the
// loads / stores into flat ones.)
// Horizontal pass of one plane: scaled columns [c0, c0 + ncols) for source
// rows [r0, r1) into lds[(c - c0) * cst + (r - r0)] (column-major).  One thread per
// column, its taps in registers (rows of the tap table are padded to a
// multiple of 4 taps, `cstride` int16 apart), one or two 16-byte loads per
// source row, the next row's load issued before the current row's taps.
// Rows past the plane (reached by zero taps only) read its last row.  `plane`
// is the source window's first row at the plane's column 0 (4-byte aligned),
// `x0` the window's first column there and `ph` its rows: a source crop's
// origin has any alignment, the word loads keep the plane's.
template <int NQ>
__device__ __forceinline__ void hpass_cols(const uint8_t* plane, int stride, int ph, int x0,
                           const int32_t* pos, const int16_t* coef, int cstride, int c0,
                           int ncols, int r0, int r1,
                           int16_t* lds, int cst, int tid, int nthreads, int rst = 1) {
  constexpr int NW = (NQ + 1 + 3) / 4 * 4;
  for (int c = tid; c < ncols; c += nthreads) {
    const int x = c0 + c;
    const int p = x0 + pos[x];  // (the origin first: the split below is of the plane's column)
    const uint32_t sh = (uint32_t)(p & 3);
    uint32_t wp[2 * NQ];
    const uint2* cp = reinterpret_cast<const uint2*>(coef + (int64_t)x * cstride);
    int32_t k0 = 0;  // 128 * the sum of the taps' hi bytes (hdot4)
#pragma unroll
    for (int k = 0; k < NQ; k++) k0 = split_taps(cp[k], wp[2 * k], wp[2 * k + 1], k0);
    k0 <<= 7;
    const uint8_t* base = plane + (p & ~3);
    int16_t* out = lds + c * cst;
    // rows in groups of G: the G loads are issued back to back, so one
    // memory latency is exposed per group instead of per row
    constexpr int G = NW <= 4 ? 12 : (NW <= 8 ? 4 : 1);
    for (int r = r0; r < r1; r += G) {
      uint32_t w[G][NW];
#pragma unroll
      for (int g = 0; g < G; g++)
        if (r + g < r1) load_words<NW>(base + (int64_t)min(r + g, ph - 1) * stride, w[g]);
#pragma unroll
      for (int g = 0; g < G; g++)
        if (r + g < r1) out[(r + g - r0) * rst] = h15(hdot4<NQ>(w[g], sh, wp, k0));
    }
  }
}

// taps beyond 64: a plain loop over the table
__device__ __forceinline__ void hpass_cols_long(const uint8_t* plane, int stride, int ph, int x0,
                                const int32_t* pos, const int16_t* coef, int cstride, int taps,
                                int c0, int ncols,
                                int r0, int r1, int16_t* lds, int cst, int tid, int nthreads,
                                int rst = 1) {
  for (int c = tid; c < ncols; c += nthreads) {
    const int x = c0 + c;
    const int p = x0 + pos[x];
    const int16_t* cf = coef + (int64_t)x * cstride;
    for (int r = r0; r < r1; r++) {
      const uint8_t* row = plane + (int64_t)min(r, ph - 1) * stride + p;
      int32_t v = 0;
      for (int t = 0; t < taps; t++) v += (int32_t)row[t] * cf[t];
      lds[c * cst + (r - r0) * rst] = h15(v);
    }
  }
}

// (dst column c, row r at dst[c * cst + (r - r0) * rst]: column-major LDS by
// default, row-major HBM for hscale_kernel)
__device__ __forceinline__ void hpass(const uint8_t* plane, int stride, int ph, int x0,
                      const int32_t* pos, const int16_t* coef, int cstride, int taps, int c0,
                      int ncols, int r0, int r1,
                      int16_t* lds, int cst, int tid, int nthreads, int rst = 1) {
  const int nq = (taps + 3) >> 2;
#define HJ_HP(N) \
  hpass_cols<N>(plane, stride, ph, x0, pos, coef, cstride, c0, ncols, r0, r1, lds, cst, tid, \
                nthreads, rst)
  if (nq <= 1) HJ_HP(1);
  else if (nq <= 2) HJ_HP(2);
  else if (nq <= 3) HJ_HP(3);
  else if (nq <= 4) HJ_HP(4);
  else if (nq <= 6) HJ_HP(6);
  else if (nq <= 8) HJ_HP(8);
  else if (nq <= 12) HJ_HP(12);
  else if (nq <= 16) HJ_HP(16);
  else hpass_cols_long(plane, stride, ph, x0, pos, coef, cstride, taps, c0, ncols, r0, r1, lds, cst,
                       tid, nthreads, rst);
#undef HJ_HP
}

// Vertical taps over an LDS column (column-major int16 words): the tap
// pairs (row p + 2i, p + 2i + 1) realigned from the column's words
// (v_alignbit by 16 when p is odd) against packed tap pairs, v_dot2 4 taps a
// step (tap rows are padded to a multiple of 4 with zeros; the 4 slack rows
// keep the padded reads inside the column).
__device__ __forceinline__ int32_t vdot_pairs(const uint32_t* col, int p, const uint32_t* f,
                                              int np) {
  const uint32_t* c = col + (p >> 1);
  const uint32_t sh = (uint32_t)(p & 1) * 16u;
  int32_t acc = 0;
  uint32_t w0 = c[0];
  for (int i = 0; i < np; i += 2) {
    const uint32_t w1 = c[i + 1], w2 = c[i + 2];
    const uint2 ff = *reinterpret_cast<const uint2*>(f + i);
    acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(hj_short2, __builtin_amdgcn_alignbit(w1, w0, sh)),
                                 __builtin_bit_cast(hj_short2, ff.x), acc, false);
    acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(hj_short2, __builtin_amdgcn_alignbit(w2, w1, sh)),
                                 __builtin_bit_cast(hj_short2, ff.y), acc, false);
    w0 = w2;
  }
  return acc;
}

// two columns against the same taps (the two pixels of a pair, or U and V):
// each tap pair is read once
__device__ __forceinline__ void vdot_pairs2(const uint32_t* col0, const uint32_t* col1, int p,
                                            const uint32_t* f, int np, int32_t& acc0,
                                            int32_t& acc1) {
  const uint32_t* c0 = col0 + (p >> 1);
  const uint32_t* c1 = col1 + (p >> 1);
  const uint32_t sh = (uint32_t)(p & 1) * 16u;
  int32_t a0 = 0, a1 = 0;
  uint32_t x0 = c0[0], y0 = c1[0];
  for (int i = 0; i < np; i += 2) {
    const uint32_t x1 = c0[i + 1], x2 = c0[i + 2], y1 = c1[i + 1], y2 = c1[i + 2];
    const uint2 ff = *reinterpret_cast<const uint2*>(f + i);
    a0 = __builtin_amdgcn_sdot2(__builtin_bit_cast(hj_short2, __builtin_amdgcn_alignbit(x1, x0, sh)),
                                __builtin_bit_cast(hj_short2, ff.x), a0, false);
    a1 = __builtin_amdgcn_sdot2(__builtin_bit_cast(hj_short2, __builtin_amdgcn_alignbit(y1, y0, sh)),
                                __builtin_bit_cast(hj_short2, ff.x), a1, false);
    a0 = __builtin_amdgcn_sdot2(__builtin_bit_cast(hj_short2, __builtin_amdgcn_alignbit(x2, x1, sh)),
                                __builtin_bit_cast(hj_short2, ff.y), a0, false);
    a1 = __builtin_amdgcn_sdot2(__builtin_bit_cast(hj_short2, __builtin_amdgcn_alignbit(y2, y1, sh)),
                                __builtin_bit_cast(hj_short2, ff.y), a1, false);
    x0 = x2;
    y0 = y2;
  }
  acc0 = a0;
  acc1 = a1;
}

// rows p and p + 1 of a column as (lo, hi) int16
__device__ __forceinline__ void vpair(const uint32_t* col, int p, int& a, int& b) {
  const uint32_t* c = col + (p >> 1);
  const uint32_t w = __builtin_amdgcn_alignbit(c[1], c[0], (uint32_t)(p & 1) * 16u);
  a = (int32_t)(int16_t)(w & 0xFFFFu);
  b = (int32_t)w >> 16;
}

__device__ __forceinline__ int clip_i8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// yuv2rgb.c fill_table / fill_gv_table: the luma-index offset a chroma value
// adds through the clipping table (the chroma index saturates to [0, 255])
__device__ __forceinline__ int tab_off(int32_t inc, int c) {
  return ((clip_i8(c) * inc) >> 16) - (inc >> 9);
}

// output.c yuv2rgb_write_full (RGB24): 2^22-scaled sums, 30-bit clip
__device__ __forceinline__ void full_rgb(const BatchParams& p, int Y, int U, int V, int* rgb) {
  Y -= p.csc.y_offset;
  Y *= p.csc.y_coeff;
  Y += 1 << 21;
  int R = (int)((uint32_t)Y + (uint32_t)V * (uint32_t)p.csc.v2r);
  int G = (int)((uint32_t)Y + (uint32_t)V * (uint32_t)p.csc.v2g + (uint32_t)U * (uint32_t)p.csc.u2g);
  int B = (int)((uint32_t)Y + (uint32_t)U * (uint32_t)p.csc.u2b);
  if ((R | G | B) & 0xC0000000) {
    auto c30 = [](int a) { return (a & ~((1 << 30) - 1)) ? ((~a) >> 31) & ((1 << 30) - 1) : a; };
    R = c30(R);
    G = c30(G);
    B = c30(B);
  }
  rgb[0] = R >> 22;
  rgb[1] = G >> 22;
  rgb[2] = B >> 22;
}

// component c's source window (ImageDesc::win_*): its first row, at the
// plane's column 0
__device__ __forceinline__ const uint8_t* win_rows(const uint8_t* planes, const ImageDesc& dd,
                                                   int c) {
  return planes + dd.plane_off[c] + (int64_t)dd.win_y[c] * dd.plane_stride[c];
}

// hscale_kernel: swscale's horizontal pass (hScale8To15) of every source row
// a large downscale reads, once, into a row-major int16 buffer (per image:
// luma pre_rl x sw, then the two chroma planes pre_rc x chr_w -- gbr: three
// planes through the luma filters; hj_sws_tile.h hs_tiles / hs_plane).  The
// output kernels then stage their bands from there (hbuf_stage) instead of
// re-filtering the rows their bands share: with a 17.9x
// bicubic downscale (12 MP -> 224) each band's 72-tap window overlaps its
// neighbours' 4x.  Flat grid (hs_map: workgroup -> image), kHsRows rows of
// one plane per workgroup.  Arithmetic: hpass (oracle sws_oracle.c hscale).
__global__ void __launch_bounds__(256) hscale_kernel(const uint8_t* __restrict__ planes,
                                                     const ImageDesc* __restrict__ desc,
                                                     const ImageInfo* __restrict__ infos,
                                                     const int32_t* __restrict__ pool,
                                                     const uint32_t* __restrict__ hs_map,
                                                     int16_t* __restrict__ hbuf) {
  const int img = (int)hs_map[blockIdx.x];
  const ImageDesc& dd = desc[img];
  // (a view's descriptor: the status is its image's, ImageDesc::src)
  const ImageInfo& in = infos[dd.src];
  if (in.status != kOk) return;
  const SwsDesc& s = dd.sws;
  const int32_t* T = pool + dd.wt_off;
  const HsTiles ht = hs_tiles(s);
  int t = (int)blockIdx.x - dd.hs_wg0;
  int c = 0;
  if (t >= ht.tl) {
    t -= ht.tl;
    c = 1 + t / ht.tc;
    t %= ht.tc;
  }
  // (a gbr plan is a gray one -- luma filters only -- applied to three planes)
  const bool lumaf = c == 0 || s.gbr;
  const HsPlane hp = hs_plane(s, c);
  const int rows = hp.rows, w = hp.w;
  const int r0 = t * kHsRows, r1 = min(r0 + kHsRows, rows);
  const int stride = dd.plane_stride[c], ph = dd.win_h[c], wx = dd.win_x[c];
  const uint8_t* plane = win_rows(planes, dd, c);
  const int32_t* pos = T + s.off[lumaf ? kHlPos : kHcPos];
  const int16_t* coef = reinterpret_cast<const int16_t*>(T + s.off[lumaf ? kHlCoef : kHcCoef]);
  const int cstride = lumaf ? s.hl_size : s.hc_size, taps = lumaf ? s.hl_taps : s.hc_taps;
  int16_t* dst = hbuf + dd.hbuf_off + hp.off + (int64_t)r0 * w;
  if (taps <= 64) {  // the register-bucket kernels of sws_kernel's own pass
    hpass(plane, stride, ph, wx, pos, coef, cstride, taps, 0, w, r0, r1, dst, 1, threadIdx.x,
          blockDim.x, w);
    return;
  }
  // longer filters (downscales past ~16x): 64-tap chunks, the chunk's taps in
  // registers, every row of the tile accumulated in registers across chunks
  const int nch = (taps + 63) / 64;
  for (int x = threadIdx.x; x < w; x += blockDim.x) {
    const int p0 = wx + pos[x];
    const uint32_t sh = (uint32_t)(p0 & 3);
    const uint8_t* base = plane + (p0 & ~3);
    int32_t acc[kHsRows];
#pragma unroll
    for (int g = 0; g < kHsRows; g++) acc[g] = 0;
    for (int k = 0; k < nch; k++) {
      // taps [64k, 64k + 64): rows of the table are padded to a multiple of 4
      // taps and the chunk past them reads zero taps of the next row's
      // padding -- masked: a quad past `taps` is zeroed
      uint32_t wp[32];
      const uint2* cp = reinterpret_cast<const uint2*>(coef + (int64_t)x * cstride + 64 * k);
#pragma unroll
      for (int q = 0; q < 16; q++) {
        const bool in_row = 64 * k + 4 * q < taps;
        const uint2 t = in_row ? cp[q] : make_uint2(0u, 0u);
        wp[2 * q] = t.x;
        wp[2 * q + 1] = t.y;
      }
#pragma unroll
      for (int g = 0; g < kHsRows; g++) {
        if (r0 + g >= r1) break;
        uint32_t wv[20];
        load_words<20>(base + (int64_t)min(r0 + g, ph - 1) * stride + 64 * k, wv);
        acc[g] += hdot<16>(wv, sh, wp);
      }
    }
#pragma unroll
    for (int g = 0; g < kHsRows; g++)
      if (r0 + g < r1) dst[(int64_t)g * w + x] = h15(acc[g]);
  }
}

// hscale_kernel's row-major rows [r0, r1) x [c0, c0 + ncols) of a `rows` x `w`
// plane into an output kernel's column-major LDS (rows past the last one read
// it: zero taps only); 4 elements per thread and step, the loads issued together
__device__ __forceinline__ void hbuf_stage(const int16_t* __restrict__ src, int w, int rows, int c0,
                                           int ncols, int r0, int r1, int16_t* dst, int cst,
                                           int tid, int nt) {
  const int nr = r1 - r0, ne = ncols * nr;
  for (int i0 = tid; i0 < ne; i0 += 4 * nt) {
    int16_t v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int i = min(i0 + u * nt, ne - 1);
      const int r = i / ncols, c = i - r * ncols;
      v[u] = src[(int64_t)min(r0 + r, rows - 1) * w + c0 + c];
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int i = i0 + u * nt;
      if (i < ne) {
        const int r = i / ncols, c = i - r * ncols;
        dst[c * cst + r] = v[u];
      }
    }
  }
}

// kOrient: the instantiation a submission with a transposed descriptor
// launches (spdl_hj_set_orients, a code with bit 2).  Its tile lands in the
// final box (hj_sws_tile.h tile_orient), the u8 tile in LDS is in landed
// layout, and the store below takes row segments of any width.  Without it
// the kernel is the one before orientations, flips included.
template <bool kOrient>
__global__ void __launch_bounds__(256) sws_kernel(const uint8_t* __restrict__ planes,
                                                  const ImageDesc* __restrict__ desc,
                                                  const ImageInfo* __restrict__ infos,
                                                  const int32_t* __restrict__ pool,
                                                  void* __restrict__ out, const BatchParams p,
                                                  int32_t* __restrict__ host_status,
                                                  const int16_t* __restrict__ hbuf,
                                                  const uint32_t* __restrict__ sws_map,
                                                  const int wg0,
                                                  const uint8_t* __restrict__ flips) {
  extern __shared__ __attribute__((aligned(16))) int16_t sws_lds[];
  // (band, chunk, image) grid, or a flat grid over every image's own tiles
  // (sws_map: workgroup -> image) when the batch's plans differ widely
  const bool flat = sws_map != nullptr;
  // XCD-aware order ("xcd_order" bit 0): neighbouring bands of one image,
  // whose source rows overlap, run on one XCD at about the same time
  uint32_t bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (p.xcd_order & 1) xcd_order(bx, by, bz);
  // (wg0: a views submission launches once per group, over that group's part
  // of the map; 0 otherwise)
  if (flat) bx += (uint32_t)wg0;
  const int img = flat ? (int)sws_map[bx] : (int)bz, tid = threadIdx.x, nt = blockDim.x;
  const ImageDesc& dd = desc[img];
  const int t = flat ? (int)bx - dd.sws_wg0 : (int)(bx * dd.sws_chunks + by);
  const int band = flat ? t / dd.sws_chunks : (int)bx;
  const int chunk = flat ? t - band * dd.sws_chunks : (int)by;
  // (a view's descriptor reads its image's status, ImageDesc::src; an image's
  // own names itself)
  const ImageInfo& in = infos[dd.src];
  // the image's final status, straight into the slot's pinned status array
  if (host_status && t == 0 && tid == 0) host_status[img] = in.status;
  // (a view the host refused alone: nothing to do, its image's status stays clean)
  if (in.status != kOk || dd.refuse) return;
  const SwsDesc& s = dd.sws;
  const int yo0 = band * s.rb, xo0 = chunk * s.col_chunk;
  if (yo0 >= dd.oh || xo0 >= dd.ow) return;
  // the tile's end and its content in scaled coordinates
  const SwsWindow win =
      sws_window(yo0, xo0, s.rb, s.col_chunk, dd.dx, dd.dy, dd.ow, dd.oh, s.sw, s.sh);
  const int yo1 = win.yo1, xo1 = win.xo1, th = yo1 - yo0, tw = xo1 - xo0;
  const int ys0 = win.ys0, ys1 = win.ys1, xs0 = win.xs0, xs1 = win.xs1;
  const bool content = win.content;
  // the output flip of this image or view (spdl_hj_set_flips), one byte per
  // descriptor and uniform over the workgroup; null: the submission has none.
  // It changes where the tile lands and where a pixel sits in it, nothing
  // else (hj_sws_tile.h tile_flip)
  const int flip = flips ? __builtin_amdgcn_readfirstlane((int)flips[img]) : 0;
  const TileFlip tf = tile_flip(xo0, xo1, yo0, yo1, dd.ow, dd.oh, flip);
  // (kOrient: codes 0..7; the landed tile lw x lh at (mx0, my0) of the final
  // box, whose rows are fw apart)
  TileOrient to{};  // (sws_kernel<false> never computes it: tf is all it has)
  int lw = 0, lh = 0, fw = 0, mx0 = 0, my0 = 0;  // (of sws_kernel<true> alone)
  if constexpr (kOrient) {
    to = tile_orient(xo0, xo1, yo0, yo1, dd.ow, dd.oh, flip);
    lw = to.lw;
    lh = to.lh;
    fw = to.fw;
    mx0 = to.mx0();
    my0 = to.my0();
  }
  const bool planar = p.pix_fmt == 0 || p.pix_fmt == 1;
  const bool swap = p.pix_fmt == 1 || p.pix_fmt == 3;
  const bool u8 = p.dtype == 0;
  const int64_t pl = (int64_t)dd.ow * dd.oh;
  const int32_t* T = pool + dd.wt_off;
  const int32_t* vl_pos = T + s.off[kVlPos];
  const int32_t* vc_pos = T + s.off[kVcPos];
  int lr0 = 0, lr1 = 0, cr0 = 0, cr1 = 0;
  SwsChromaCols ccols = {0, 0};
  const int ncl = content ? xs1 - xs0 : 0;
  if (content) {
    lr0 = vl_pos[ys0];
    lr1 = vl_pos[ys1 - 1] + s.vl_taps;
    if (!s.gray) {
      cr0 = vc_pos[ys0];
      cr1 = vc_pos[ys1 - 1] + s.vc_taps;
      ccols = sws_chroma_cols(xs0, xs1, s.full);
    }
  }
  const int cx0 = ccols.cx0, ncc = ccols.ncc;
  // LDS (sws_lds_layout): the horizontal-pass output, column-major (gbr: the
  // R, G, B planes all through the luma filters: hl, hu, hv), then the u8 tile
  // in output layout for wide stores, then the band's vertical tables
  const SwsLds lay = sws_lds_layout(ncl, ncc, lr1 - lr0, cr1 - cr0, s.gbr, s.gray, s.rb,
                                    s.col_chunk, s.vl_size, s.vc_size);
  const int lst = lay.lst, cst = lay.cst, vrw = lay.vrw;
  int16_t *hl = sws_lds, *hu = hl + lay.hu, *hv = hl + lay.hv;
  uint8_t* tile = reinterpret_cast<uint8_t*>(sws_lds) + lay.tile;
  // the vertical tables are staged once (the per-row loads of the V pass are
  // then LDS broadcasts); their first rows are band-relative
  uint32_t* vt = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(sws_lds) + lay.vt);
  if (content) {
    const int32_t* vmode = T + s.off[kVmode];
    const uint32_t* vlw = reinterpret_cast<const uint32_t*>(T + s.off[kVlCoef]);
    const uint32_t* vcw = reinterpret_cast<const uint32_t*>(T + s.off[kVcCoef]);
    const int nl = s.vl_size / 2, nc = s.vc_size / 2;
    for (int i = tid; i < (ys1 - ys0) * vrw; i += nt) {
      const int r = i / vrw, w = i - r * vrw, ys = ys0 + r;
      uint32_t v = 0;
      if (w == 0) v = (uint32_t)vmode[ys];
      else if (w == 1) v = (uint32_t)(vl_pos[ys] - lr0);
      else if (w == 2) v = s.gray ? 0u : (uint32_t)(vc_pos[ys] - cr0);
      else if (w >= 4 && w < 4 + nl) v = vlw[(int64_t)ys * nl + (w - 4)];
      else if (w >= 4 + nl) v = vcw[(int64_t)ys * nc + (w - 4 - nl)];
      vt[i] = v;
    }
  }
  // one pixel, its three values in the output's channel order
  auto putc = [&](int xo, int yo, int c0v, int c1v, int c2v) {
    const int cv[3] = {c0v, c1v, c2v};
    // (in the mirrored tile; kOrient: in the landed one)
    int tx, ty;
    if constexpr (kOrient) {
      tx = to.lx(xo, yo);
      ty = to.ly(xo, yo);
    } else {
      tx = tf.tx(xo);
      ty = tf.ty(yo);
    }
    if (u8) {
#pragma unroll
      for (int ch = 0; ch < 3; ch++) {
        const int v = cv[ch];
        int ti;
        if constexpr (kOrient) ti = planar ? (ch * lh + ty) * lw + tx : (ty * lw + tx) * 3 + ch;
        else ti = planar ? (ch * th + ty) * tw + tx : (ty * tw + tx) * 3 + ch;
        tile[ti] = (uint8_t)v;
      }
      return;
    }
    // (in the flipped output; kOrient: in the final one, whose rows are fw apart)
    const int mx = (kOrient ? mx0 : tf.mx0) + tx, my = (kOrient ? my0 : tf.my0) + ty;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const int v = cv[ch];
      int64_t oi;
      if constexpr (kOrient)
        oi = dd.out_off + (planar ? ch * pl + (int64_t)my * fw + mx : ((int64_t)my * fw + mx) * 3 + ch);
      else
        oi = dd.out_off + (planar ? ch * pl + (int64_t)my * dd.ow + mx : ((int64_t)my * dd.ow + mx) * 3 + ch);
      float f = __fdiv_rn((float)v, 255.0f);
      f = __fsub_rn(f, p.mean[ch]);
      f = __fdiv_rn(f, p.std[ch]);
      static_cast<uint16_t*>(out)[oi] = to_f16_bits(f, p.dtype);
    }
  };
  auto put = [&](int xo, int yo, const int* rgb) {
    // (selects, not a dynamically indexed array: that would live in scratch)
    putc(xo, yo, swap ? rgb[2] : rgb[0], rgb[1], swap ? rgb[0] : rgb[2]);
  };
  // pad: tile pixels outside the scaled image are black
  {
    // the content's rows and columns in output coordinates (no content: every
    // row of the tile counts as above it).  A tile of content alone has
    // nothing to fill; otherwise the pad is at most four rectangles: the rows
    // above and below, the columns left and right of the content rows.
    const int cy0 = content ? ys0 + dd.dy : yo1, cy1 = content ? ys1 + dd.dy : yo1;
    const int cxa = xs0 + dd.dx, cxb = xs1 + dd.dx;
    if (cy0 > yo0 || cy1 < yo1 || cxa > xo0 || cxb < xo1) {
      const int lane = tid & 63, nw = nt >> 6;
      const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
      // bytes [off, off + n) of the u8 tile, thread t of nth: words where
      // the run is aligned, single bytes at its ends
      auto zrun = [&](int off, int n, int t, int nth) {
        const int head = min(n, -off & 3), words = (n - head) >> 2;
        const int tail = n - head - 4 * words;
        uint8_t* q = tile + off + head;
        if (t < head) tile[off + t] = 0;
        for (int i = t; i < words; i += nth) reinterpret_cast<uint32_t*>(q)[i] = 0u;
        if (t < tail) q[4 * words + t] = 0;
      };
      // rows [ya, yb) x columns [xa, xb)
      auto fill = [&](int ya, int yb, int xa, int xb) {
        if (ya >= yb || xa >= xb) return;
        if (!u8) {  // straight to the output: a row per wave at a time
          for (int yo = ya + wave; yo < yb; yo += nw)
            for (int xo = xa + lane; xo < xb; xo += 64) putc(xo, yo, 0, 0, 0);
          return;
        }
        const int bpp = planar ? 1 : 3, np_ = planar ? 3 : 1;
        const int ps = th * tw;  // bytes of a planar tile's plane
        if constexpr (kOrient) {
          // the rectangle in the landed tile, kw x rh at (k0, r0): a pad row
          // of a transposed descriptor is a column there
          const int k0 = min(to.lx(xa, ya), to.lx(xb - 1, yb - 1));
          const int r0 = min(to.ly(xa, ya), to.ly(xb - 1, yb - 1));
          const int kw = to.t ? yb - ya : xb - xa, rh = to.t ? xb - xa : yb - ya;
          if (kw == lw) {  // whole rows: one run per plane
            for (int pc = 0; pc < np_; pc++) zrun((pc * ps + r0 * lw) * bpp, rh * lw * bpp, tid, nt);
            return;
          }
          for (int r = r0 + wave; r < r0 + rh; r += nw)
            for (int pc = 0; pc < np_; pc++) zrun((pc * ps + r * lw + k0) * bpp, kw * bpp, lane, 64);
          return;
        }
        // the rectangle's first row and column in the mirrored tile
        const int r0 = min(tf.ty(ya), tf.ty(yb - 1)), k0 = min(tf.tx(xa), tf.tx(xb - 1));
        if (xb - xa == tw) {     // whole rows: one run per plane
          for (int pc = 0; pc < np_; pc++)
            zrun((pc * ps + r0 * tw) * bpp, (yb - ya) * tw * bpp, tid, nt);
          return;
        }
        for (int yo = ya + wave; yo < yb; yo += nw)
          for (int pc = 0; pc < np_; pc++)
            zrun((pc * ps + tf.ty(yo) * tw + k0) * bpp, (xb - xa) * bpp, lane, 64);
      };
      fill(yo0, cy0, xo0, xo1);
      fill(cy1, yo1, xo0, xo1);
      fill(cy0, cy1, xo0, cxa);
      fill(cy0, cy1, cxb, xo1);
    }
  }
  if (content && s.pre) {
    // the horizontal pass was run once per source row by hscale_kernel
    // (large downscales): copy the band's rows into the column-major LDS
    const int16_t* hb = hbuf + dd.hbuf_off;
    hbuf_stage(hb, s.sw, s.pre_rl, xs0, ncl, lr0, lr1, hl, lst, tid, nt);
    if (s.gbr || !s.gray) {  // G and B through the luma window, or U and V
      const HsPlane p1 = hs_plane(s, 1), p2 = hs_plane(s, 2);
      const int c0 = s.gbr ? xs0 : cx0, nc = s.gbr ? ncl : ncc;
      const int q0 = s.gbr ? lr0 : cr0, q1 = s.gbr ? lr1 : cr1, st = s.gbr ? lst : cst;
      hbuf_stage(hb + p1.off, p1.w, p1.rows, c0, nc, q0, q1, hu, st, tid, nt);
      hbuf_stage(hb + p2.off, p2.w, p2.rows, c0, nc, q0, q1, hv, st, tid, nt);
    }
  } else if (content && s.gbr) {
    // three planes, a third of the threads each
    const int third = nt / 3, c = min(tid / third, 2), t3 = tid - c * third;
    if (tid < 3 * third)
      hpass(win_rows(planes, dd, c), dd.plane_stride[c], dd.win_h[c], dd.win_x[c],
            T + s.off[kHlPos],
            reinterpret_cast<const int16_t*>(T + s.off[kHlCoef]), s.hl_size, s.hl_taps, xs0, ncl,
            lr0, lr1, c == 0 ? hl : c == 1 ? hu : hv, lst, t3, third);
  } else if (content && !(p.debug_mask & kAblSwsHpass)) {
    hpass(win_rows(planes, dd, 0), dd.plane_stride[0], dd.win_h[0], dd.win_x[0],
          T + s.off[kHlPos],
          reinterpret_cast<const int16_t*>(T + s.off[kHlCoef]), s.hl_size, s.hl_taps, xs0, ncl,
          lr0, lr1, hl, lst, tid, nt);
    if (!s.gray) {
      // the two chroma planes share the tables: half the threads each
      const int half = nt >> 1, t2 = tid < half ? tid : tid - half;
      const int c = tid < half ? 1 : 2;
      hpass(win_rows(planes, dd, c), dd.plane_stride[c], dd.win_h[c], dd.win_x[c],
            T + s.off[kHcPos],
            reinterpret_cast<const int16_t*>(T + s.off[kHcCoef]), s.hc_size, s.hc_taps, cx0, ncc,
            cr0, cr1, c == 1 ? hu : hv, cst, t2, half);
    }
  }
  __syncthreads();
  const bool pairs = !s.full && !s.gbr && !s.gray;
  if (content && pairs && !(p.debug_mask & kAblSwsVpass)) {
    // The table writers (yuv2rgb_{X,2,1}_c) share one U, V between the two
    // pixels of a chroma column: a work item owns chroma column cx0 + cc and
    // those of luma columns 2 (cx0 + cc), + 1 that lie in [xs0, xs1) -- a
    // tile may begin or end in the middle of a pair.  U, V and their four
    // table offsets once, Y and the clips per pixel.  A wave works on one
    // output row at a time (its header is wave-uniform: scalar mode tests
    // and row offsets); the (row, 64 pairs) units go round the waves.
    const int npl = s.vl_size / 2, npc = s.vc_size / 2;  // tap pairs per row
    const int lane = tid & 63, nw = nt >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nch = (ncc + 63) >> 6, nrows = ys1 - ys0;
    int r = 0, chk = wave;
    while (chk >= nch) {
      chk -= nch;
      r++;
    }
    while (r < nrows) {
      const uint32_t* row = vt + r * vrw;
      const uint4 hdr = *reinterpret_cast<const uint4*>(row);
      const int m = (int)hdr.x;
      const int lp = (int)hdr.y, cp = (int)hdr.z;
      const int mode = m & 15, ya = (m >> 4) & 8191, ua = (m >> 17) & 8191;
      const uint32_t* lf = row + 4;  // luma tap pairs, then chroma
      const uint32_t* cf = lf + npl;
      const int cc = chk * 64 + lane;
      if (cc < ncc) {
        const int xe = 2 * (cx0 + cc) - xs0;  // the even pixel's column in the tile, -1: not ours
        const bool h0 = xe >= 0, h1 = xe + 1 < ncl;
        const uint32_t* l0 = reinterpret_cast<const uint32_t*>(hl + max(xe, 0) * lst);
        const uint32_t* l1 = reinterpret_cast<const uint32_t*>(hl + min(xe + 1, ncl - 1) * lst);
        const uint32_t* ucol = reinterpret_cast<const uint32_t*>(hu + cc * cst);
        const uint32_t* vcol = reinterpret_cast<const uint32_t*>(hv + cc * cst);
        int Y0, Y1, U, V;
        if (mode == kSwsX) {
          int32_t a0, a1;
          vdot_pairs2(l0, l1, lp, lf, npl, a0, a1);
          Y0 = ((1 << 18) + a0) >> 19;
          Y1 = ((1 << 18) + a1) >> 19;
          vdot_pairs2(ucol, vcol, cp, cf, npc, a0, a1);
          U = ((1 << 18) + a0) >> 19;
          V = ((1 << 18) + a1) >> 19;
        } else {
          int y00, y01, y10, y11, u0, u1, v0, v1;
          vpair(l0, lp, y00, y01);
          vpair(l1, lp, y10, y11);
          vpair(ucol, cp, u0, u1);
          vpair(vcol, cp, v0, v1);
          if (mode == kSwsTwo) {
            Y0 = (y00 * (4096 - ya) + y01 * ya) >> 19;
            Y1 = (y10 * (4096 - ya) + y11 * ya) >> 19;
            U = (u0 * (4096 - ua) + u1 * ua) >> 19;
            V = (v0 * (4096 - ua) + v1 * ua) >> 19;
          } else {
            if (!ua) {
              u1 = u0;
              v1 = v0;
            }
            Y0 = (y00 + 64) >> 7;
            Y1 = (y10 + 64) >> 7;
            U = (u0 * (4096 - ua) + u1 * ua + (128 << 11)) >> 19;
            V = (v0 * (4096 - ua) + v1 * ua + (128 << 11)) >> 19;
          }
        }
        // the chroma terms of the first and last channel swap with the channels
        const int tr = tab_off(p.csc.crv, V), tb = tab_off(p.csc.cbu, U);
        const int t0 = swap ? tb : tr, t2 = swap ? tr : tb;
        const int t1 = tab_off(p.csc.cgu, U) + tab_off(p.csc.cgv, V);
        const int yo = ys0 + r + dd.dy, xo = xs0 + xe + dd.dx;
        if (h0) putc(xo, yo, clip_i8(Y0 + t0), clip_i8(Y0 + t1), clip_i8(Y0 + t2));
        if (h1) putc(xo + 1, yo, clip_i8(Y1 + t0), clip_i8(Y1 + t1), clip_i8(Y1 + t2));
      }
      chk += nw;
      while (chk >= nch) {
        chk -= nch;
        r++;
      }
    }
  } else if (content && !(p.debug_mask & kAblSwsVpass)) {
    // vertical taps + RGB24 writer, one scaled column per thread
    const int npl = s.vl_size / 2, npc = s.vc_size / 2;  // tap pairs per row
    for (int cl = tid; cl < ncl; cl += nt) {
      const int xs = xs0 + cl;
      const int cc = (s.full ? xs : xs >> 1) - cx0;
      const uint32_t* lcol = reinterpret_cast<const uint32_t*>(hl + cl * lst);
      const uint32_t* ucol = reinterpret_cast<const uint32_t*>(hu + cc * cst);
      const uint32_t* vcol = reinterpret_cast<const uint32_t*>(hv + cc * cst);
      for (int ys = ys0; ys < ys1; ys++) {
        const uint32_t* row = vt + (ys - ys0) * vrw;
        const uint4 hdr = *reinterpret_cast<const uint4*>(row);
        const int m = (int)hdr.x;
        const int mode = m & 15, ya = (m >> 4) & 8191, ua = (m >> 17) & 8191;
        const uint32_t* lf = row + 4;  // luma tap pairs, then chroma
        const uint32_t* cf = lf + npl;
        const int lp = (int)hdr.y, cp = (int)hdr.z;
        int rgb[3];
        int Y, U = 0, V = 0;
        if (s.gbr) {
          // swscale's 8-bit planar writers per plane (oracle sws_scale_gbr)
          const uint32_t* cols[3] = {lcol, lcol + (hu - hl) / 2, lcol + (hv - hl) / 2};
#pragma unroll
          for (int c = 0; c < 3; c++) {
            int v;
            if (mode == kSwsX) {
              v = ((1 << 18) + vdot_pairs(cols[c], lp, lf, npl)) >> 19;
            } else {
              int a, b;
              vpair(cols[c], lp, a, b);
              v = mode == kSwsTwo ? (a * (4096 - ya) + b * ya) >> 19 : (a + 64) >> 7;
            }
            rgb[c] = clip_i8(v);
          }
        } else if (s.full) {
          if (mode == kSwsTwo) {
            int a, b;
            vpair(lcol, lp, a, b);
            Y = (a * (4096 - ya) + b * ya) >> 10;
          } else if (mode == kSwsOne) {
            int a, b;
            vpair(lcol, lp, a, b);
            Y = a * 4;
          } else {
            Y = ((1 << 9) + vdot_pairs(lcol, lp, lf, npl)) >> 10;
          }
          if (!s.gray) {
            if (mode == kSwsX) {
              U = ((1 << 9) - (128 << 19) + vdot_pairs(ucol, cp, cf, npc)) >> 10;
              V = ((1 << 9) - (128 << 19) + vdot_pairs(vcol, cp, cf, npc)) >> 10;
            } else {
              int u0, u1, v0, v1;
              vpair(ucol, cp, u0, u1);
              vpair(vcol, cp, v0, v1);
              if (!ua) {
                u1 = u0;
                v1 = v0;
              }
              U = (u0 * (4096 - ua) + u1 * ua - (128 << 19)) >> 10;
              V = (v0 * (4096 - ua) + v1 * ua - (128 << 19)) >> 10;
            }
          }
          full_rgb(p, Y, U, V, rgb);
        } else {
          if (mode == kSwsX) {
            Y = ((1 << 18) + vdot_pairs(lcol, lp, lf, npl)) >> 19;
            U = ((1 << 18) + vdot_pairs(ucol, cp, cf, npc)) >> 19;
            V = ((1 << 18) + vdot_pairs(vcol, cp, cf, npc)) >> 19;
          } else {
            int y0, y1, u0, u1, v0, v1;
            vpair(lcol, lp, y0, y1);
            vpair(ucol, cp, u0, u1);
            vpair(vcol, cp, v0, v1);
            if (mode == kSwsTwo) {
              Y = (y0 * (4096 - ya) + y1 * ya) >> 19;
              U = (u0 * (4096 - ua) + u1 * ua) >> 19;
              V = (v0 * (4096 - ua) + v1 * ua) >> 19;
            } else {
              if (!ua) {
                u1 = u0;
                v1 = v0;
              }
              Y = (y0 + 64) >> 7;
              U = (u0 * (4096 - ua) + u1 * ua + (128 << 11)) >> 19;
              V = (v0 * (4096 - ua) + v1 * ua + (128 << 11)) >> 19;
            }
          }
          rgb[0] = clip_i8(Y + tab_off(p.csc.crv, V));
          rgb[1] = clip_i8(Y + tab_off(p.csc.cgu, U) + tab_off(p.csc.cgv, V));
          rgb[2] = clip_i8(Y + tab_off(p.csc.cbu, U));
        }
        put(xs + dd.dx, ys + dd.dy, rgb);
      }
    }
  }
  if (!u8 || (p.debug_mask & kAblSwsStore)) return;
  __syncthreads();
  // the u8 tile out with wide stores: whole rows of an interleaved image are
  // one contiguous run, planar ones three (a flipped output: the same tile at
  // its mirrored origin)
  const int nplane = planar ? 3 : 1;
  const int run = planar ? th * tw : th * tw * 3;  // bytes per plane run
  if constexpr (kOrient) {
    // The landed tile leaves as row segments, lh per plane, rowb bytes each
    // and ostride apart in the final box.  A segment is cut at the 4-byte
    // words of its DESTINATION: a word that lies inside the segment is one
    // dword store, assembled from the two aligned LDS words its bytes straddle
    // (the LDS side is at another offset within 4 bytes: no unaligned access);
    // the words at a segment's two ends hold one to three of its bytes, which
    // leave one by one -- the byte head and the byte tail.  The work items are
    // (segment, word): a segment shorter than the wave wastes no lanes.
    const int rowb = planar ? lw : lw * 3;
    const int64_t ostride = planar ? fw : (int64_t)fw * 3;
    uint8_t* dst0 = static_cast<uint8_t*>(out) + dd.out_off +
                    (planar ? (int64_t)my0 * fw + mx0 : ((int64_t)my0 * fw + mx0) * 3);
    if (lw == fw && ((uintptr_t)dst0 & 15) == 0 && (run & 15) == 0 && (!planar || (pl & 15) == 0)) {
      // (whole rows of the final box: one aligned run per plane, as below)
      for (int pc = 0; pc < nplane; pc++)
        for (int i = tid; i < run / 16; i += nt)
          reinterpret_cast<uint4*>(dst0 + pc * pl)[i] =
              reinterpret_cast<const uint4*>(tile + pc * run)[i];
      return;
    }
    const int wps = (rowb + 6) >> 2;  // the most destination words a segment touches
    const int nseg = nplane * lh;
    const uint32_t* tw32 = reinterpret_cast<const uint32_t*>(tile);  // (16-byte aligned)
    for (int i = tid; i < nseg * wps; i += nt) {
      const int seg = i / wps, j = i - seg * wps;
      const int pc = seg / lh, r = seg - pc * lh;
      const int so = pc * run + r * rowb;  // the segment in the LDS tile
      uint8_t* d = dst0 + pc * pl + r * ostride;
      const int k0 = 4 * j - (int)((uintptr_t)d & 3);  // this word's first byte in the segment
      if (k0 >= rowb) continue;
      if (k0 >= 0 && k0 + 4 <= rowb) {
        const int o = so + k0;
        // (an aligned word needs no second one: the last word of the tile is
        // then never followed by a read past the tile's region)
        const uint32_t lo = tw32[o >> 2], hi = (o & 3) ? tw32[(o >> 2) + 1] : 0u;
        *reinterpret_cast<uint32_t*>(d + k0) = __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)(o & 3));
      } else {
        for (int k = max(k0, 0); k < min(k0 + 4, rowb); k++) d[k] = tile[so + k];
      }
    }
    return;
  }
  for (int pc = 0; pc < nplane; pc++) {
    const uint8_t* src = tile + pc * run;
    uint8_t* dst = static_cast<uint8_t*>(out) + dd.out_off + pc * pl +
                   (planar ? (int64_t)tf.my0 * dd.ow + tf.mx0
                           : ((int64_t)tf.my0 * dd.ow + tf.mx0) * 3);
    if (tw == dd.ow && ((uintptr_t)dst & 15) == 0 && (run & 15) == 0) {
      for (int i = tid; i < run / 16; i += nt)
        reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
    } else {
      const int rowb = planar ? tw : tw * 3;
      const int64_t ostride = planar ? dd.ow : (int64_t)dd.ow * 3;
      for (int i = tid; i < run; i += nt) {
        const int r = i / rowb, k = i - r * rowb;
        dst[r * ostride + k] = src[i];
      }
    }
  }
}

// yuv_planes_kernel: the planar destination (SPDL_HJ_FMT_YUV) -- the scale
// chain on the frame's own format, yuvj4xxp -> yuvj4xxp or gray8 -> gray8
// (hj_sws.h sws_plan_planar).  A sibling of sws_kernel without the colour
// arithmetic: every plane goes through its own filters (luma hl / vl, chroma
// hc / vc, chroma plane to chroma plane) and swscale's 8-bit planar writer
//   clip8((2^18 + sum tap x) >> 19)          (yuv2planeX_8_c; a size-1 filter
//   holds the tap 4096, which makes it yuv2plane1_8_c's clip8((x + 64) >> 7))
// as the gbr branch of sws_kernel does per RGB plane.  One workgroup per
// (plane, row band, column chunk) tile of one image, flat grid through
// sws_map; an image's tiles are its luma tiles, then U's, then V's, bands of
// SwsDesc::rb rows and chunks of SwsDesc::col_chunk columns of the plane.
// Horizontal pass (hpass, or hscale_kernel's rows for a large downscale) into
// column-major LDS, vertical pass one column per thread into a u8 tile in
// LDS, pad region filled with the plane's pad byte (Y 0, U = V 128; gray8
// 16), then the tile out.  Plane rows are ow or cw bytes, not 4-aligned in
// general: a run of the tile (the whole tile when it spans the plane's
// width, else one row) sits in LDS at its destination's offset within 16
// bytes, so after a head of single bytes both sides are 16-byte aligned for
// dwordx4 stores, and a tail of single bytes ends it.  A flipped image
// (spdl_hj_set_flips) has that destination, and so that offset, from the
// tile's mirrored origin.
__global__ void __launch_bounds__(256) yuv_planes_kernel(const uint8_t* __restrict__ planes,
                                                         const ImageDesc* __restrict__ desc,
                                                         const ImageInfo* __restrict__ infos,
                                                         const int32_t* __restrict__ pool,
                                                         uint8_t* __restrict__ out,
                                                         int32_t* __restrict__ host_status,
                                                         const int16_t* __restrict__ hbuf,
                                                         const uint32_t* __restrict__ sws_map,
                                                         const uint8_t* __restrict__ flips) {
  extern __shared__ __attribute__((aligned(16))) int16_t yuv_lds[];
  const int img = (int)sws_map[blockIdx.x], tid = threadIdx.x, nt = blockDim.x;
  const ImageDesc& dd = desc[img];
  int t = (int)blockIdx.x - dd.sws_wg0;
  const ImageInfo& in = infos[img];
  // the image's final status, straight into the slot's pinned status array
  // (an image the host refused has this one workgroup)
  if (host_status && t == 0 && tid == 0) host_status[img] = in.status;
  if (in.status != kOk) return;
  const SwsDesc& s = dd.sws;
  // the tile's plane: its box (W x H), the scaled content (psw x psh) and
  // where that sits in the box (the chroma offsets are exact shifts: the host
  // keeps pad and crop on the chroma grid)
  const PlanarTiles pt = planar_tiles(dd.ow, dd.oh, s.hsub, s.vsub, s.rb, s.col_chunk, s.gray);
  const int cw = pt.cw, ch = pt.ch;
  int c = 0;
  if (t >= pt.ltiles) {
    t -= pt.ltiles;
    c = 1 + t / pt.ctiles;
    t -= (c - 1) * pt.ctiles;
    if (s.gray || c > 2) return;
  }
  const bool luma = c == 0;
  const int W = luma ? dd.ow : cw, H = luma ? dd.oh : ch;
  const int psw = luma ? s.sw : s.chr_w, psh = luma ? s.sh : s.chr_h;
  const int pdx = luma ? dd.dx : dd.dx >> s.hsub, pdy = luma ? dd.dy : dd.dy >> s.vsub;
  const int padv = luma ? (s.gray ? 16 : 0) : 128;
  const int chunks = luma ? pt.lchunks : pt.cchunks;
  const int band = t / chunks, chunk = t - band * chunks;
  const int yo0 = band * s.rb, xo0 = chunk * s.col_chunk;
  if (yo0 >= H || xo0 >= W) return;
  const SwsWindow win = sws_window(yo0, xo0, s.rb, s.col_chunk, pdx, pdy, W, H, psw, psh);
  const int yo1 = win.yo1, xo1 = win.xo1, th = yo1 - yo0, tw = xo1 - xo0;
  const int ys0 = win.ys0, ys1 = win.ys1, xs0 = win.xs0, xs1 = win.xs1;
  const bool content = win.content;
  const int ncl = content ? xs1 - xs0 : 0;
  // the image's output flip (as in sws_kernel): every plane is mirrored by its
  // own width and height, so the tile of this plane lands at its mirrored
  // origin in the plane and its pixels at their mirrored tile coordinates
  const int flip = flips ? __builtin_amdgcn_readfirstlane((int)flips[img]) : 0;
  const TileFlip tf = tile_flip(xo0, xo1, yo0, yo1, W, H, flip);
  const int32_t* T = pool + dd.wt_off;
  const int32_t* vpos = T + s.off[luma ? kVlPos : kVcPos];
  const uint32_t* vco = reinterpret_cast<const uint32_t*>(T + s.off[luma ? kVlCoef : kVcCoef]);
  const int vnp = (luma ? s.vl_size : s.vc_size) / 2, vtaps = luma ? s.vl_taps : s.vc_taps;
  int r0 = 0, r1 = 0;
  if (content) {
    r0 = vpos[ys0];
    r1 = vpos[ys1 - 1] + vtaps;
  }
  // LDS (planar_lds_layout): the horizontal-pass columns, then the u8 tile
  const PlanarLds lay = planar_lds_layout(ncl, r1 - r0, th, tw);
  const int cst = lay.cst;
  int16_t* hcol = yuv_lds;
  uint8_t* tile = reinterpret_cast<uint8_t*>(yuv_lds) + lay.tile;
  // the tile's destination: one run when the tile spans the plane's width
  const int64_t pbase = dd.out_off + (luma ? 0 : (int64_t)dd.ow * dd.oh + (int64_t)(c - 1) * cw * ch);
  uint8_t* dst = out + pbase + (int64_t)tf.my0 * W + tf.mx0;
  const bool whole = tw == W;
  const int nrun = whole ? 1 : th, runlen = whole ? th * W : tw;
  const int pitch = lay.pitch;  // LDS bytes between the runs of a chunked tile
  const uint32_t g0 = (uint32_t)(uintptr_t)dst;
  auto tpos = [&](int r, int k) {  // tile byte of row r, column k
    return whole ? (int)(g0 & 15u) + r * W + k : r * pitch + (int)((g0 + (uint32_t)(r * W)) & 15u) + k;
  };
  // pad: tile pixels outside the scaled content
  for (int i = tid; i < th * tw; i += nt) {
    const int r = i / tw, k = i - r * tw;
    const int ys = tf.sy(r) - pdy, xs = tf.sx(k) - pdx;
    if (ys < 0 || ys >= psh || xs < 0 || xs >= psw) tile[tpos(r, k)] = (uint8_t)padv;
  }
  if (content && s.pre) {
    const HsPlane hp = hs_plane(s, c);
    hbuf_stage(hbuf + dd.hbuf_off + hp.off, hp.w, hp.rows, xs0, ncl, r0, r1, hcol, cst, tid, nt);
  } else if (content) {
    hpass(win_rows(planes, dd, c), dd.plane_stride[c], dd.win_h[c], dd.win_x[c],
          T + s.off[luma ? kHlPos : kHcPos],
          reinterpret_cast<const int16_t*>(T + s.off[luma ? kHlCoef : kHcCoef]),
          luma ? s.hl_size : s.hc_size, luma ? s.hl_taps : s.hc_taps, xs0, ncl, r0, r1, hcol, cst,
          tid, nt);
  }
  __syncthreads();
  if (content) {
    // vertical taps + the planar writer, one scaled column per thread (the
    // row's first source row and taps are uniform: scalar loads)
    for (int cl = tid; cl < ncl; cl += nt) {
      const uint32_t* col = reinterpret_cast<const uint32_t*>(hcol + cl * cst);
      const int k = tf.tx(xs0 + cl + pdx);
      for (int ys = ys0; ys < ys1; ys++) {
        const int v = ((1 << 18) + vdot_pairs(col, vpos[ys] - r0, vco + (int64_t)ys * vnp, vnp)) >> 19;
        tile[tpos(tf.ty(ys + pdy), k)] = (uint8_t)clip_i8(v);
      }
    }
  }
  __syncthreads();
  // the tile out: per run up to 15 head bytes, 16-byte vectors, up to 15 tail
  // bytes; a thread takes one of these items at a time
  const int items = 30 + runlen / 16 + 1;
  for (int i = tid; i < nrun * items; i += nt) {
    const int r = i / items, j = i - r * items;
    uint8_t* g = dst + (int64_t)r * W;
    const uint8_t* l = tile + tpos(r, 0);
    const int head = min(runlen, (int)((16u - ((uint32_t)(uintptr_t)g & 15u)) & 15u));
    const int nvec = (runlen - head) >> 4, tail = runlen - head - 16 * nvec;
    if (j < 15) {
      if (j < head) g[j] = l[j];
    } else if (j < 30) {
      const int o = head + 16 * nvec + (j - 15);
      if (j - 15 < tail) g[o] = l[o];
    } else if (j - 30 < nvec) {
      const int o = head + 16 * (j - 30);
      *reinterpret_cast<uint4*>(g + o) = *reinterpret_cast<const uint4*>(l + o);
    }
  }
}

// swscale's unscaled special converter (ff_get_unscaled_swscale ->
// yuv2rgb_c_24_rgb: yuvj420p with even height / yuvj422p, even width ->
// rgb24) for full-resolution output: nearest chroma and the same table
// arithmetic as sws_kernel's one-tap writer with identity filters (Y, U, V
// are the plane bytes; oracle sws_oracle.c), but one thread per
// kRgbPx pixels of a row -- no horizontal / vertical passes and no LDS.  u8
// only.  HBM-bound: 1.5 B in + 3 B out per pixel.
constexpr int kRgbPx = 8;  // 8 or 16

template <int N>  // N words from a pointer aligned to 4 N bytes
__device__ __forceinline__ void rgbu_load(const uint8_t* p, uint32_t (&w)[N]) {
  if constexpr (N == 1) {
    w[0] = *reinterpret_cast<const uint32_t*>(p);
  } else if constexpr (N == 2) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    w[0] = v.x, w[1] = v.y;
  } else {
    static_assert(N == 4, "rgbu_load: 1, 2 or 4 words");
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
  }
}

template <int N>  // N words (2 or 4) as one store
__device__ __forceinline__ void rgbu_store(uint8_t* p, const uint32_t* w) {
  if constexpr (N == 2) {
    *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
  } else {
    static_assert(N == 4, "rgbu_store: 2 or 4 words");
    *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// One group of PX pixels of output row y (columns x0 .. x0 + npx) from its
// luma words yw and chroma words uw / vw (x0 / 2 onwards): the table
// arithmetic of yuv2rgb_c_24_rgb, then vector stores where aligned.
template <int PX>
__device__ __forceinline__ void rgbu_group(const uint32_t (&yw)[PX / 4], const uint32_t (&uw)[PX / 8],
                                           const uint32_t (&vw)[PX / 8], uint8_t* __restrict__ base,
                                           const int64_t pl, const int w, const int y, const int x0,
                                           const int npx, const BatchParams& p, const bool planar,
                                           const bool swap) {
  constexpr int SW = PX / 4;  // words per vector store
  uint32_t c0[PX], c1[PX], c2[PX];
#pragma unroll
  for (int i = 0; i < PX; i++) {
    const int Y = (int)((yw[i >> 2] >> (8 * (i & 3))) & 0xFFu);
    const int U = (int)((uw[i >> 3] >> (8 * ((i >> 1) & 3))) & 0xFFu);
    const int V = (int)((vw[i >> 3] >> (8 * ((i >> 1) & 3))) & 0xFFu);
    const int r = clip_i8(Y + tab_off(p.csc.crv, V));
    const int gg = clip_i8(Y + tab_off(p.csc.cgu, U) + tab_off(p.csc.cgv, V));
    const int b = clip_i8(Y + tab_off(p.csc.cbu, U));
    c0[i] = (uint32_t)(swap ? b : r);
    c1[i] = (uint32_t)gg;
    c2[i] = (uint32_t)(swap ? r : b);
  }
  if (!planar) {
    uint8_t* o = base + ((int64_t)y * w + x0) * 3;
    if (npx == PX && ((uintptr_t)o & (4u * SW - 1u)) == 0u) {  // 3 PX bytes: three stores
      uint32_t wv[3 * PX / 4];
#pragma unroll
      for (int k = 0; k < 3 * PX / 4; k++) {
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int q = 4 * k + j, i = q / 3, c = q % 3;
          v |= (c == 0 ? c0[i] : c == 1 ? c1[i] : c2[i]) << (8 * j);
        }
        wv[k] = v;
      }
#pragma unroll
      for (int s3 = 0; s3 < 3; s3++) rgbu_store<SW>(o + 4 * SW * s3, wv + SW * s3);
    } else {
      for (int i = 0; i < npx; i++) {
        o[3 * i] = (uint8_t)c0[i];
        o[3 * i + 1] = (uint8_t)c1[i];
        o[3 * i + 2] = (uint8_t)c2[i];
      }
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const uint32_t* cv = c == 0 ? c0 : c == 1 ? c1 : c2;
      uint8_t* o = base + c * pl + (int64_t)y * w + x0;
      if (npx == PX && ((uintptr_t)o & (4u * SW - 1u)) == 0u) {
        uint32_t wv[SW];
#pragma unroll
        for (int k = 0; k < SW; k++)
          wv[k] = cv[4 * k] | cv[4 * k + 1] << 8 | cv[4 * k + 2] << 16 | cv[4 * k + 3] << 24;
        rgbu_store<SW>(o, wv);
      } else {
        for (int i = 0; i < npx; i++) o[i] = (uint8_t)cv[i];
      }
    }
  }
}

__global__ void __launch_bounds__(256) rgb_unscaled_kernel(const uint8_t* __restrict__ planes,
                                                           const ImageDesc* __restrict__ desc,
                                                           const ImageInfo* __restrict__ infos,
                                                           uint8_t* __restrict__ out,
                                                           const BatchParams p,
                                                           int32_t* __restrict__ host_status) {
  constexpr int PX = kRgbPx, YW = PX / 4, CW = PX / 8;
  const int img = blockIdx.y;
  const ImageInfo& in = infos[img];
  if (host_status && blockIdx.x == 0 && threadIdx.x == 0) host_status[img] = in.status;
  if (in.status != kOk) return;
  const ImageDesc& dd = desc[img];
  const int w = dd.ow, h = dd.oh;  // w is even: a row's last group may hold 2..PX-2 px
  const uint32_t ngr = (uint32_t)(w + PX - 1) / PX;
  const uint32_t total = ngr * (uint32_t)h;  // < 2^27 (nblocks < 2^24)
  const int vsub = in.comp_v[0] > in.comp_v[1] ? 1 : 0;
  const bool planar = p.pix_fmt == 0 || p.pix_fmt == 1;
  const bool swap = p.pix_fmt == 1 || p.pix_fmt == 3;
  const int64_t pl = (int64_t)w * h;
  const uint8_t* y_pl = planes + dd.plane_off[0];
  const uint8_t* u_pl = planes + dd.plane_off[1];
  const uint8_t* v_pl = planes + dd.plane_off[2];
  uint8_t* base = out + dd.out_off;
  for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < total; g += gridDim.x * blockDim.x) {
    const int y = (int)(g / ngr), x0 = (int)(g - (uint32_t)y * ngr) * PX;
    const int npx = x0 + PX <= w ? PX : w - x0;
    // planes are padded to whole blocks (luma rows to 16 px for 4:2:x): PX luma
    // and PX/2 chroma bytes are readable and aligned
    uint32_t yw[YW], uw[CW], vw[CW];
    rgbu_load<YW>(y_pl + (int64_t)y * dd.plane_stride[0] + x0, yw);
    rgbu_load<CW>(u_pl + (int64_t)(y >> vsub) * dd.plane_stride[1] + (x0 >> 1), uw);
    rgbu_load<CW>(v_pl + (int64_t)(y >> vsub) * dd.plane_stride[2] + (x0 >> 1), vw);
    rgbu_group<PX>(yw, uw, vw, base, pl, w, y, x0, npx, p, planar, swap);
  }
}

// Full resolution, fused: one workgroup transforms a run of MCUs of one MCU
// row into LDS (list_block + idct_block, the blocks' LDS then reused as the plane
// tile) and converts it with swscale's unscaled converter straight from LDS
// (rgbu_group) -- the planes never go through HBM.  Standard 4:2:0 / 4:2:2
// MCUs only (Y 2x2 or 2x1 blocks, then U, V 1x1: bpm 6 or 4); the host checks
// the sampling (Layout::fuse_ok).  u8 output.
//
// Grid: (tile, image) for a batch whose images all take this path and have
// one size.  With the trailing sws_map argument (Map: one pointer) it is the
// flat grid over the fused-eligible images of a ragged submission
// (spdl_hj_set_ragged): workgroup g is tile g - sws_wg0 of image sws_map[g],
// the map's first part (Layout::fused_wgs entries; hj_layout.h) -- no empty
// workgroup, whatever the images' sizes.  The argument is a pack so that the
// instantiation without it is the kernel as it was, signature and code.  A
// tile shares nothing with its neighbours (its coefficients in, its rows
// out), so the order the flat grid's workgroups take over the XCDs is left as
// the dispatcher has it.
template <class T, class... R>
__device__ __forceinline__ T first_arg(T a, R...) {
  return a;
}
template <int IDCT, class... Map>
__global__ void __launch_bounds__(kFusedThreads) idct_rgb_kernel(const uint32_t* __restrict__ ents,
                                                       const uint2* __restrict__ bdesc,
                                                       const ImageDesc* __restrict__ desc,
                                                       const ImageInfo* __restrict__ infos,
                                                       uint8_t* __restrict__ out,
                                                       const BatchParams p,
                                                       int32_t* __restrict__ host_status,
                                                       const Map... sws_map) {
  __shared__ __attribute__((aligned(16))) uint32_t sblk[kBlkWords + 1][kFusedThreads];
  __shared__ uint32_t sq[kMaxComp][64];
  constexpr bool flat = sizeof...(Map) != 0;
  int img = blockIdx.y, bx = blockIdx.x;
  const int tid = threadIdx.x;
  if constexpr (flat) {
    img = (int)first_arg(sws_map...)[blockIdx.x];
    bx -= desc[img].sws_wg0;
  }
  const ImageInfo& in = infos[img];
  if (host_status && bx == 0 && tid == 0) host_status[img] = in.status;
  if (in.status != kOk) return;
  const ImageDesc& dd = desc[img];
  const int bpm = in.bpm;   // 6 or 4
  const int tw = kFusedThreads / bpm;  // MCUs per tile
  const int tiles_x = (in.mcux + tw - 1) / tw;
  if (bx >= tiles_x * in.mcuy) return;
  const int my = bx / tiles_x, mx0 = (bx - my * tiles_x) * tw;
  const int nm = min(tw, in.mcux - mx0);
  const int hy = 8 * in.comp_v[0];                    // luma rows of the MCU row: 16 or 8
  const int ys = tw * 16, cs = tw * 8;                 // tile row strides (bytes)
  const bool act = tid < nm * bpm;
  const int m = tid / bpm, b = tid - m * bpm;
  load_dequant<kFusedThreads>(sq, in, tid);
  __syncthreads();
  uint2 px[8];
  if (act) {
    const int j = (my * in.mcux + mx0 + m) * bpm + b;
    list_block<kFusedThreads>(ents, bdesc[(size_t)dd.coef_off + j], dd.coef_off, in.nblocks,
                              sq[in.mcu_comp[b]], &sblk[0][tid]);
    idct_block_rows<kFusedThreads, IDCT>(&sblk[0][tid], px);
  }
  __syncthreads();  // every slot read: the tile takes their place
  uint8_t* tl = reinterpret_cast<uint8_t*>(&sblk[0][0]);  // hy x ys luma, then 8 x cs U, V
  uint8_t* tu = tl + hy * ys;
  uint8_t* tv = tu + 8 * cs;
  if (act) {
    const int c = in.mcu_comp[b];
    uint8_t* dst = c == 0 ? tl + in.mcu_dy[b] * 8 * ys + m * 16 + in.mcu_dx[b] * 8
                          : (c == 1 ? tu : tv) + m * 8;
    const int st = c == 0 ? ys : cs;
#pragma unroll
    for (int r = 0; r < 8; r++) *reinterpret_cast<uint2*>(dst + r * st) = px[r];
  }
  __syncthreads();
  const int w = dd.ow, h = dd.oh;
  const int x_base = mx0 * 16, y_base = my * hy;
  const int cols = min(nm * 16, w - x_base), rows = min(hy, h - y_base);
  const int ngr = (cols + 7) >> 3;
  const int vsub = hy == 16 ? 1 : 0;
  const bool planar = p.pix_fmt == 0 || p.pix_fmt == 1;
  const bool swap = p.pix_fmt == 1 || p.pix_fmt == 3;
  const int64_t pl = (int64_t)w * h;
  uint8_t* base = out + dd.out_off;
  for (int g = tid; g < ngr * rows; g += kFusedThreads) {
    const int r = g / ngr, xl = (g - r * ngr) * 8;
    const uint2 yq = *reinterpret_cast<const uint2*>(tl + r * ys + xl);
    const uint32_t yw[2] = {yq.x, yq.y};
    const uint32_t uw[1] = {*reinterpret_cast<const uint32_t*>(tu + (r >> vsub) * cs + (xl >> 1))};
    const uint32_t vw[1] = {*reinterpret_cast<const uint32_t*>(tv + (r >> vsub) * cs + (xl >> 1))};
    rgbu_group<8>(yw, uw, vw, base, pl, w, y_base + r, x_base + xl, min(8, cols - xl), p, planar,
                  swap);
  }
}

// FFmpeg mjpeg's in-decoder conversion of a 4-component frame (oracle
// jo_cmyk_transform; parity unpinned), in place on the IDCT planes:
//   Adobe 0 (GBRAP): inverted CMYK -> RGB, R = c k 257 >> 16 ...
//   Adobe 2 (YUVA444P): YCCK -> YCbCr, Y = (255 - y) k 257 >> 16,
//                       Cb = ((128 - cb) k 257 >> 16) + 128, Cr likewise
// Adobe 1, another transform or no Adobe marker: YCbCr + K (frame_color
// kColorYcbcrk; K dropped, this kernel skips the image).  The colour models
// are restated from mjpegdec as recalled: parity unpinned (no fixture the
// reference holds covers them).  Four pixels per thread: one
// 32-bit load from each plane, three stores (HBM-bound: 4 B in, 3 B out per
// pixel); the planes are 1x1-sampled, so one stride serves all four.
__global__ void __launch_bounds__(256) cmyk_kernel(const ImageDesc* __restrict__ desc,
                                                   const ImageInfo* __restrict__ infos,
                                                   uint8_t* __restrict__ planes) {
  const int img = blockIdx.y;
  const ImageInfo& in = infos[img];
  if (in.status != kOk || (in.color != kColorCmyk && in.color != kColorYcck)) return;
  const ImageDesc& dd = desc[img];
  const int wq = (in.width + 3) >> 2, stride = dd.plane_stride[0];
  const bool ycck = in.color == kColorYcck;
  const int64_t nq = (int64_t)wq * in.height;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nq;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / wq), x = 4 * (int)(i - (int64_t)y * wq);
    const int64_t o = (int64_t)y * stride + x;
    uint32_t* p0 = reinterpret_cast<uint32_t*>(planes + dd.plane_off[0] + o);
    uint32_t* p1 = reinterpret_cast<uint32_t*>(planes + dd.plane_off[1] + o);
    uint32_t* p2 = reinterpret_cast<uint32_t*>(planes + dd.plane_off[2] + o);
    const uint32_t k4 = *reinterpret_cast<const uint32_t*>(planes + dd.plane_off[3] + o);
    const uint32_t a = *p0, b = *p1, c = *p2;
    uint32_t ra = 0, rb = 0, rc = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int k = (int)((k4 >> (8 * j)) & 255u);
      const int va = (int)((a >> (8 * j)) & 255u), vb = (int)((b >> (8 * j)) & 255u),
                vc = (int)((c >> (8 * j)) & 255u);
      int oa, ob, oc;
      if (ycck) {
        oa = ((255 - va) * k * 257) >> 16;
        ob = ((((128 - vb) * k) * 257) >> 16) + 128;
        oc = ((((128 - vc) * k) * 257) >> 16) + 128;
      } else {
        oa = (va * k * 257) >> 16;
        ob = (vb * k * 257) >> 16;
        oc = (vc * k * 257) >> 16;
      }
      ra |= (uint32_t)(oa & 255) << (8 * j);
      rb |= (uint32_t)(ob & 255) << (8 * j);
      rc |= (uint32_t)(oc & 255) << (8 * j);
    }
    *p0 = ra;
    *p1 = rb;
    *p2 = rc;
  }
}

// ---------------------------------------------------------------------------
// NV12 -> planar RGB/BGR (the video path's colour conversion; reference
// src/libspdl/cuda/detail/color_conversion.cu:90-138).  One thread per 2x2
// luma quad, x fastest so the 2-byte loads and stores of a wave are
// contiguous.  Arithmetic: oracle jo_nv12_to_rgb (explicit fma order).
// ---------------------------------------------------------------------------
__constant__ float kYuv2Rgb[10][3][3] = {
    {{1.1644f, 0.0000f, 1.8337f}, {1.1644f, -0.2181f, -0.5451f}, {1.1644f, 2.1606f, 0.0000f}},
    {{1.1644f, 0.0000f, 1.8337f}, {1.1644f, -0.2181f, -0.5451f}, {1.1644f, 2.1606f, 0.0000f}},
    {{1.1644f, 0.0000f, 1.8337f}, {1.1644f, -0.2181f, -0.5451f}, {1.1644f, 2.1606f, 0.0000f}},
    {{1.1644f, 0.0000f, 1.6301f}, {1.1644f, -0.3864f, -0.8289f}, {1.1644f, 2.0726f, 0.0000f}},
    {{1.1644f, 0.0000f, 1.6325f}, {1.1644f, -0.4007f, -0.8315f}, {1.1644f, 2.0633f, 0.0000f}},
    {{1.1644f, 0.0000f, 1.6325f}, {1.1644f, -0.4007f, -0.8315f}, {1.1644f, 2.0633f, 0.0000f}},
    {{1.1644f, 0.0000f, 1.8351f}, {1.1644f, -0.2639f, -0.5550f}, {1.1644f, 2.1262f, 0.0000f}},
    {{1.1644f, 0.0000f, 1.8337f}, {1.1644f, -0.2181f, -0.5451f}, {1.1644f, 2.1606f, 0.0000f}},
    {{1.1689f, 0.0000f, 1.7237f}, {1.1689f, -0.1924f, -0.6679f}, {1.1689f, 2.1992f, 0.0000f}},
    {{1.1689f, 0.0000f, 1.7237f}, {1.1689f, -0.1924f, -0.6679f}, {1.1689f, 2.1992f, 0.0000f}},
};

__device__ __forceinline__ uint8_t clamp8f(float x) {
  return x < 0.0f ? 0 : (x > 255.0f ? 255 : (uint8_t)x);
}

__global__ void __launch_bounds__(256) nv12_kernel(const uint8_t* __restrict__ src,
                                                   uint8_t* __restrict__ dst, int height,
                                                   int width, int bgr, int coeff) {
  const int qx = blockIdx.x * 256 + threadIdx.x, qy = blockIdx.y, f = blockIdx.z;
  const int x = 2 * qx, y = 2 * qy;
  if (x + 1 >= width || y + 1 >= height) return;
  const float(*m)[3] = kYuv2Rgb[coeff - 1];
  const uint8_t* yuv = src + (size_t)f * (height + height / 2) * width;
  uint8_t* rgb = dst + (size_t)f * 3 * height * width;
  const uint8_t* uv = yuv + (size_t)(height + qy) * width + x;
  const float fu = (float)((int)uv[0] - 128), fv = (float)((int)uv[1] - 128);
  const size_t plane = (size_t)height * width;
#pragma unroll
  for (int dy = 0; dy < 2; dy++) {
    const uint8_t* yr = yuv + (size_t)(y + dy) * width + x;
    const float y0 = (float)((int)yr[0] - 16), y1 = (float)((int)yr[1] - 16);
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const float t = m[ch][1] * fu;
      const uint8_t a = clamp8f(__fmaf_rn(m[ch][2], fv, __fmaf_rn(m[ch][0], y0, t)));
      const uint8_t b = clamp8f(__fmaf_rn(m[ch][2], fv, __fmaf_rn(m[ch][0], y1, t)));
      uint8_t* o = rgb + (size_t)(bgr ? 2 - ch : ch) * plane + (size_t)(y + dy) * width + x;
      o[0] = a;
      o[1] = b;
    }
  }
}

hipError_t launch_nv12(const uint8_t* src, uint8_t* dst, int frames, int height, int width,
                       int bgr, int coeff, hipStream_t st) {
  const int qx = width / 2, qy = height / 2;
  if (frames <= 0 || qx <= 0 || qy <= 0) return hipSuccess;
  hipLaunchKernelGGL(nv12_kernel, dim3((qx + 255) / 256, qy, frames), dim3(256), 0, st, src, dst,
                     height, width, bgr, coeff);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// turbo_rgb_kernel: csc = TURBO (spdl_hipjpeg.h "Pillow-exact decode") -- the
// islow planes through libjpeg-turbo's per-component upsampling and 6b colour
// tables (hj_upsample.h) into the caller's layout, at full resolution.
//
// Grid: flat over (image, tile) through sws_map (workgroup g is tile
// g - sws_wg0 of image sws_map[g]; the planner counts an image's tiles from its
// own size, ImageDesc::sws_bands x sws_chunks of kTurboTileW x kTurboTileH
// pixels), so a plain and a ragged submission are one launch each.  A thread
// owns 8 consecutive pixels of two output rows -- one chroma row under a
// vertical ratio of 2, whose triple products serve both rows.  Planes are read
// as aligned words (a neighbour sample from the neighbouring word, clamped at
// the plane's true edge); a row segment leaves as dwords from the first
// 4-byte boundary on, with byte stores for the head and tail: a row of odd
// width and a ragged offset start anywhere, and a ragged neighbour may start
// at the next byte, so no byte outside the segment is written.  Each
// component's rule is uniform over the image (a scalar branch).
// ---------------------------------------------------------------------------

typedef uint32_t hj_u32x2a __attribute__((ext_vector_type(2), aligned(4)));

// N dwords to a 4-byte aligned address, 16 bytes at a time
template <int N>
__device__ __forceinline__ void store_words(uint8_t* q, const uint32_t (&w)[N]) {
#pragma unroll
  for (int i = 0; i + 4 <= N; i += 4) {
    hj_u32x4a v;
    v.x = w[i];
    v.y = w[i + 1];
    v.z = w[i + 2];
    v.w = w[i + 3];
    *reinterpret_cast<hj_u32x4a*>(q + 4 * i) = v;
  }
  if constexpr (N % 4 >= 2) {
    constexpr int j = N / 4 * 4;
    hj_u32x2a v;
    v.x = w[j];
    v.y = w[j + 1];
    *reinterpret_cast<hj_u32x2a*>(q + 4 * j) = v;
  }
  if constexpr (N % 2 == 1) *reinterpret_cast<uint32_t*>(q + 4 * (N - 1)) = w[N - 1];
}

// Bytes [K, nbytes) of the byte stream b, one store each (every index a
// constant: the words stay in registers)
template <int K, int NW>
__device__ __forceinline__ void store_bytes(uint8_t* dst, const uint32_t (&b)[NW], int nbytes) {
  if constexpr (K < 4 * NW) {
    if (K < nbytes) dst[K] = (uint8_t)(b[K >> 2] >> (8 * (K & 3)));
    store_bytes<K + 1, NW>(dst, b, nbytes);
  }
}

// The first nbytes (<= 4 NW) of the byte stream b to dst, of any alignment,
// and nothing else.  A whole segment: the bytes up to the first 4-byte
// boundary, NW - 1 (or NW) realigned dwords, the bytes behind them.  A partial
// one (the last of a row whose width is no multiple of 8): bytes.
template <int NW>
__device__ __forceinline__ void store_run(uint8_t* dst, const uint32_t (&b)[NW], int nbytes) {
  const uint32_t mis = (uint32_t)reinterpret_cast<uintptr_t>(dst) & 3u;
  if (nbytes == 4 * NW) {
    if (mis == 0) {
      store_words<NW>(dst, b);
      return;
    }
    const uint32_t head = 4u - mis;
#pragma unroll
    for (uint32_t k = 0; k < 3; k++)
      if (k < head) dst[k] = (uint8_t)(b[0] >> (8 * k));
    uint32_t m[NW - 1];
#pragma unroll
    for (int j = 0; j < NW - 1; j++) m[j] = __builtin_amdgcn_alignbyte(b[j + 1], b[j], head);
    store_words<NW - 1>(dst + head, m);
    const uint32_t tail = b[NW - 1] >> (8 * head);
    uint8_t* q = dst + head + 4 * (NW - 1);
#pragma unroll
    for (uint32_t k = 0; k < 3; k++)
      if (k < mis) q[k] = (uint8_t)(tail >> (8 * k));
    return;
  }
  store_bytes<0, NW>(dst, b, nbytes);
}

// (x / 255 - mean) / std as store_rgb has it, to f16 / bf16 bits
__device__ __forceinline__ uint32_t turbo_norm(int v, float mean, float sd, int dtype) {
  float f = __fdiv_rn((float)v, 255.0f);
  f = __fsub_rn(f, mean);
  f = __fdiv_rn(f, sd);
  return to_f16_bits(f, dtype);
}

// One row segment of a thread: 8 pixels, c0 / c1 / c2 in the output's channel
// order, npx of them inside the frame, to row y from column x0 of an image
// whose first element is `base`
__device__ __forceinline__ void turbo_store_row(void* out, int64_t base, const BatchParams& p,
                                                int W, int H, int x0, int y, int npx,
                                                const int (&c0)[8], const int (&c1)[8],
                                                const int (&c2)[8]) {
  const bool planar = p.pix_fmt == 0 || p.pix_fmt == 1;
  const int64_t pl = (int64_t)W * H, at = (int64_t)y * W + x0;
  if (p.dtype == 0) {
    uint8_t* o = static_cast<uint8_t*>(out) + base;
    if (planar) {
      uint32_t b[3][2];
#pragma unroll
      for (int h = 0; h < 2; h++) {
        b[0][h] = (uint32_t)c0[4 * h] | (uint32_t)c0[4 * h + 1] << 8 | (uint32_t)c0[4 * h + 2] << 16 |
                  (uint32_t)c0[4 * h + 3] << 24;
        b[1][h] = (uint32_t)c1[4 * h] | (uint32_t)c1[4 * h + 1] << 8 | (uint32_t)c1[4 * h + 2] << 16 |
                  (uint32_t)c1[4 * h + 3] << 24;
        b[2][h] = (uint32_t)c2[4 * h] | (uint32_t)c2[4 * h + 1] << 8 | (uint32_t)c2[4 * h + 2] << 16 |
                  (uint32_t)c2[4 * h + 3] << 24;
      }
#pragma unroll
      for (int ch = 0; ch < 3; ch++) store_run<2>(o + ch * pl + at, b[ch], npx);
    } else {
      // 8 pixels x 3 bytes: four pixels make three dwords
      uint32_t b[6];
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int k = 4 * h;
        b[3 * h] = (uint32_t)c0[k] | (uint32_t)c1[k] << 8 | (uint32_t)c2[k] << 16 |
                   (uint32_t)c0[k + 1] << 24;
        b[3 * h + 1] = (uint32_t)c1[k + 1] | (uint32_t)c2[k + 1] << 8 | (uint32_t)c0[k + 2] << 16 |
                       (uint32_t)c1[k + 2] << 24;
        b[3 * h + 2] = (uint32_t)c2[k + 2] | (uint32_t)c0[k + 3] << 8 | (uint32_t)c1[k + 3] << 16 |
                       (uint32_t)c2[k + 3] << 24;
      }
      store_run<6>(o + at * 3, b, npx * 3);
    }
    return;
  }
  uint8_t* o = static_cast<uint8_t*>(out) + base * 2;
  if (planar) {
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      uint32_t b[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int va = ch == 0 ? c0[2 * k] : ch == 1 ? c1[2 * k] : c2[2 * k];
        const int vb = ch == 0 ? c0[2 * k + 1] : ch == 1 ? c1[2 * k + 1] : c2[2 * k + 1];
        b[k] = turbo_norm(va, p.mean[ch], p.std[ch], p.dtype) |
               turbo_norm(vb, p.mean[ch], p.std[ch], p.dtype) << 16;
      }
      store_run<4>(o + (ch * pl + at) * 2, b, npx * 2);
    }
  } else {
    // 8 pixels x 3 halves: two pixels make three dwords
    uint32_t b[12];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      uint32_t e[6];
      e[0] = turbo_norm(c0[2 * k], p.mean[0], p.std[0], p.dtype);
      e[1] = turbo_norm(c1[2 * k], p.mean[1], p.std[1], p.dtype);
      e[2] = turbo_norm(c2[2 * k], p.mean[2], p.std[2], p.dtype);
      e[3] = turbo_norm(c0[2 * k + 1], p.mean[0], p.std[0], p.dtype);
      e[4] = turbo_norm(c1[2 * k + 1], p.mean[1], p.std[1], p.dtype);
      e[5] = turbo_norm(c2[2 * k + 1], p.mean[2], p.std[2], p.dtype);
      b[3 * k] = e[0] | e[1] << 16;
      b[3 * k + 1] = e[2] | e[3] << 16;
      b[3 * k + 2] = e[4] | e[5] << 16;
    }
    store_run<12>(o + at * 6, b, npx * 6);
  }
}

// One output row of a thread from its three components' samples: the colour
// model, the channel order, the store
__device__ __forceinline__ void turbo_row(void* out, const ImageDesc& dd, const BatchParams& p,
                                          int x0, int y, const int (&v0)[8], const int (&v1)[8],
                                          const int (&v2)[8]) {
  const bool swap = p.pix_fmt == 1 || p.pix_fmt == 3;
  int c0[8], c1[8], c2[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    int rgb[3];
    if (dd.ncomp == 1) {
      rgb[0] = rgb[1] = rgb[2] = v0[k];
    } else if (dd.color == kColorRgb) {  // an RGB-coded frame: a copy of its planes
      rgb[0] = v0[k];
      rgb[1] = v1[k];
      rgb[2] = v2[k];
    } else {
      up::ycc_rgb(v0[k], v1[k], v2[k], rgb);
    }
    c0[k] = swap ? rgb[2] : rgb[0];
    c1[k] = rgb[1];
    c2[k] = swap ? rgb[0] : rgb[2];
  }
  turbo_store_row(out, dd.out_off, p, dd.ow, dd.oh, x0, y, min(8, dd.ow - x0), c0, c1, c2);
}

__global__ void __launch_bounds__(256) turbo_rgb_kernel(const uint8_t* __restrict__ planes,
                                                        const ImageDesc* __restrict__ desc,
                                                        const ImageInfo* __restrict__ infos,
                                                        void* __restrict__ out, const BatchParams p,
                                                        int32_t* __restrict__ host_status,
                                                        const uint32_t* __restrict__ sws_map) {
  const int img = (int)sws_map[blockIdx.x], tid = threadIdx.x;
  const ImageDesc& dd = desc[img];
  const int t = (int)blockIdx.x - dd.sws_wg0;
  const ImageInfo& in = infos[img];
  if (host_status && t == 0 && tid == 0) host_status[img] = in.status;
  if (in.status != kOk || dd.refuse) return;
  const int W = dd.ow, H = dd.oh;
  const int ty = t / dd.sws_chunks, tx = t - ty * dd.sws_chunks;
  const int x0 = tx * kTurboTileW + (tid & 15) * 8;
  const int y0 = ty * kTurboTileH + (tid >> 4) * 2;
  if (x0 >= W || y0 >= H) return;
  // the ratios, from the sampling factors the planner laid the planes out by
  int hmax = 1, vmax = 1;
  if (dd.ncomp > 1) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      hmax = max(hmax, dd.h_samp[c]);
      vmax = max(vmax, dd.v_samp[c]);
    }
  }
  int v[3][2][8];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    if (c < dd.ncomp) {
      const int hr = dd.ncomp > 1 ? hmax / dd.h_samp[c] : 1;
      const int vr = dd.ncomp > 1 ? vmax / dd.v_samp[c] : 1;
      const int cw = dd.win_w[c], ch = dd.win_h[c];
      up::run8x2(planes + dd.plane_off[c], dd.plane_stride[c], cw, ch, up::mode_of(hr, vr, cw), hr,
                 vr, x0, y0, v[c][0], v[c][1]);
    } else {  // (gray: every channel is Y)
#pragma unroll
      for (int k = 0; k < 8; k++) {
        v[c][0][k] = v[0][0][k];
        v[c][1][k] = v[0][1][k];
      }
    }
  }
  turbo_row(out, dd, p, x0, y0, v[0][0], v[1][0], v[2][0]);
  if (y0 + 1 < H) turbo_row(out, dd, p, x0, y0 + 1, v[0][1], v[1][1], v[2][1]);
}

// ---------------------------------------------------------------------------
// launchers (host side, same TU; declared in hj_launch.h)
// ---------------------------------------------------------------------------

hipError_t launch_parse(const BatchBuffers& b, const ImageDesc* host_desc, const void* host_tables,
                        int64_t table_bytes, int threads, hipStream_t st) {
  const auto* host_work =
      host_desc ? reinterpret_cast<const uint32_t*>(host_desc + b.ndesc) : nullptr;
  hipLaunchKernelGGL(parse_kernel, dim3(b.n), dim3(threads), 0, st, b.bytes, host_desc, b.desc,
                     b.infos, b.luts, static_cast<const uint4*>(host_tables),
                     reinterpret_cast<uint4*>(b.wts), (table_bytes + 15) / 16, host_work, b.work,
                     b.nwork, b.chain, b.ds_map, b.idct_map, b.hs_map, b.sws_map, b.ndesc);
  hipLaunchKernelGGL(lut_kernel, dim3(8, b.n), dim3(256), 0, st, b.bytes, b.desc, b.infos, b.luts);
  return hipGetLastError();
}
hipError_t launch_destuff(const BatchBuffers& b, bool flat, int ds_wgs, int max_chunks,
                          hipStream_t st) {
  // not flat: the (max chunks, image) grid of a batch of similar sizes
  const dim3 grid = flat ? dim3(ds_wgs) : dim3(max_chunks, b.n);
  const uint32_t* map = flat ? b.ds_map : nullptr;
  hipLaunchKernelGGL(destuff_count_kernel, grid, dim3(kDsThreads), 0, st, b.bytes, b.desc, b.infos,
                     b.dschunks, map);
  hipLaunchKernelGGL(destuff_prefix_kernel, dim3(b.n), dim3(kDsThreads), 0, st, b.desc, b.infos,
                     b.dschunks);
  hipLaunchKernelGGL(destuff_write_kernel, grid, dim3(kDsThreads), 0, st, b.bytes, b.desc, b.infos,
                     b.dschunks, b.clean, b.segs, map);
  return hipGetLastError();
}
hipError_t launch_entropy(const BatchBuffers& b, const EntropyParams& ep, int threads, int lds_pad,
                          hipStream_t st) {
  // one workgroup per work item (image or piece)
#define HJ_ENT(T, NTAB)                                                                        \
  hipLaunchKernelGGL((entropy_kernel<T, NTAB>), dim3(b.nwork), dim3(T), lds_pad, st, b.clean,  \
                     b.segs, b.desc, b.infos, b.luts, b.ents, b.bdesc, b.recs, b.work, b.chain, \
                     ep, b.nwork)
  switch (threads) {
    case 1024: HJ_ENT(1024, 4); break;
    case 512: HJ_ENT(512, 4); break;
    case 128: HJ_ENT(128, 4); break;
    default: HJ_ENT(256, 4);
  }
#undef HJ_ENT
  return hipGetLastError();
}
hipError_t launch_multiscan(const BatchBuffers& b, hipStream_t st) {
  hipLaunchKernelGGL(multiscan_kernel, dim3(b.n), dim3(256), 0, st, b.bytes, b.clean, b.desc,
                     b.infos, b.ents, b.bdesc);
  return hipGetLastError();
}
// kernel K's instance for an IDCT kind: 0 simple, 1 islow, 2 none (kAblIdctNone)
#define HJ_IDCT_KIND(K, kind, ...)                               \
  do {                                                           \
    if ((kind) == 2) hipLaunchKernelGGL(K<2>, __VA_ARGS__);      \
    else if ((kind) == 1) hipLaunchKernelGGL(K<1>, __VA_ARGS__); \
    else hipLaunchKernelGGL(K<0>, __VA_ARGS__);                  \
  } while (0)
hipError_t launch_idct(const BatchBuffers& b, int idct, bool flat, int idct_wgs, int max_blocks,
                       int xcd, hipStream_t st) {
  // flat: every image's tiles, no empty workgroups; else (max tiles, image)
  const int max_tiles = (max_blocks + kIdctThreads - 1) / kIdctThreads;
  const dim3 grid = flat ? dim3(idct_wgs) : dim3(max_tiles, b.n);
  HJ_IDCT_KIND(idct_kernel, idct, grid, dim3(kIdctThreads), 0, st, b.ents, b.bdesc, b.desc, b.infos,
               b.planes, flat ? b.idct_map : nullptr, xcd);
  return hipGetLastError();
}
hipError_t launch_idct_lowres(const BatchBuffers& b, int idct, int idct_wgs, hipStream_t st) {
  HJ_IDCT_KIND(idct_lowres_kernel, idct, dim3(idct_wgs), dim3(kIdctThreads), 0, st, b.ents, b.bdesc,
               b.desc, b.infos, b.planes, b.idct_map, b.lowres);
  return hipGetLastError();
}
hipError_t launch_idct_rgb(const BatchBuffers& b, void* out, const BatchParams& p, int idct,
                           int tiles, int32_t* host_status, hipStream_t st) {
  HJ_IDCT_KIND(idct_rgb_kernel, idct, dim3(tiles, b.n), dim3(kFusedThreads), 0, st, b.ents, b.bdesc,
               b.desc, b.infos, static_cast<uint8_t*>(out), p, host_status);
  return hipGetLastError();
}
hipError_t launch_idct_rgb_flat(const BatchBuffers& b, void* out, const BatchParams& p, int idct,
                                int fused_wgs, int32_t* host_status, hipStream_t st) {
  const uint32_t* map = b.sws_map;
  const dim3 grid(fused_wgs), wg(kFusedThreads);
  uint8_t* o = static_cast<uint8_t*>(out);
  // (HJ_IDCT_KIND takes a kernel with one template argument)
  if (idct == 2)
    hipLaunchKernelGGL((idct_rgb_kernel<2, const uint32_t*>), grid, wg, 0, st, b.ents, b.bdesc,
                       b.desc, b.infos, o, p, host_status, map);
  else if (idct == 1)
    hipLaunchKernelGGL((idct_rgb_kernel<1, const uint32_t*>), grid, wg, 0, st, b.ents, b.bdesc,
                       b.desc, b.infos, o, p, host_status, map);
  else
    hipLaunchKernelGGL((idct_rgb_kernel<0, const uint32_t*>), grid, wg, 0, st, b.ents, b.bdesc,
                       b.desc, b.infos, o, p, host_status, map);
  return hipGetLastError();
}
#undef HJ_IDCT_KIND
hipError_t launch_cmyk(const BatchBuffers& b, int64_t max_px, hipStream_t st) {
  // max_px: the largest 4-component image of the batch (grid-stride beyond)
  const int gx = (int)std::min<int64_t>((max_px / 4 + 255) / 256 + 1, 1024);
  hipLaunchKernelGGL(cmyk_kernel, dim3(gx, b.n), dim3(256), 0, st, b.desc, b.infos, b.planes);
  return hipGetLastError();
}
hipError_t launch_csc(const BatchBuffers& b, void* out, const BatchParams& p, int64_t max_px,
                      int32_t* host_status, hipStream_t st) {
  const int gx = (int)std::min<int64_t>((max_px + 255) / 256, 4096);
  hipLaunchKernelGGL(csc_kernel, dim3(gx, b.n), dim3(256), 0, st, b.planes, b.desc, b.infos, out, p,
                     host_status);
  return hipGetLastError();
}
hipError_t launch_turbo_rgb(const BatchBuffers& b, void* out, const BatchParams& p, int turbo_wgs,
                            int32_t* host_status, hipStream_t st) {
  hipLaunchKernelGGL(turbo_rgb_kernel, dim3(turbo_wgs), dim3(256), 0, st, b.planes, b.desc, b.infos,
                     out, p, host_status, b.sws_map);
  return hipGetLastError();
}
hipError_t launch_rgb_unscaled(const BatchBuffers& b, void* out, const BatchParams& p,
                               int64_t max_px, int32_t* host_status, hipStream_t st) {
  const int64_t groups = (max_px + kRgbPx - 1) / kRgbPx + 64;
  const int gx = (int)std::min<int64_t>((groups + 255) / 256, 1024);
  hipLaunchKernelGGL(rgb_unscaled_kernel, dim3(gx, b.n), dim3(256), 0, st, b.planes, b.desc,
                     b.infos, static_cast<uint8_t*>(out), p, host_status);
  return hipGetLastError();
}
static void launch_hscale(const BatchBuffers& b, int hs_wgs, hipStream_t st) {
  if (hs_wgs > 0)
    hipLaunchKernelGGL(hscale_kernel, dim3(hs_wgs), dim3(256), 0, st, b.planes, b.desc, b.infos,
                       b.wts, b.hs_map, b.hbuf);
}
hipError_t launch_sws(const BatchBuffers& b, void* out, const BatchParams& p, bool flat,
                      int sws_wgs, int bands, int chunks, int lds_bytes, int hs_wgs,
                      int32_t* host_status, hipStream_t st, int wg0) {
  launch_hscale(b, hs_wgs, st);
  const dim3 grid = flat ? dim3(sws_wgs) : dim3(bands, chunks, b.n);
  // (a submission with a transposed descriptor: the orienting instantiation)
  hipLaunchKernelGGL(b.transposed ? sws_kernel<true> : sws_kernel<false>, grid, dim3(256), lds_bytes,
                     st, b.planes, b.desc, b.infos, b.wts, out, p, host_status, b.hbuf,
                     flat ? b.sws_map : nullptr, wg0, b.flips);
  return hipGetLastError();
}
hipError_t launch_yuv_planes(const BatchBuffers& b, void* out, int sws_wgs, int lds_bytes,
                             int hs_wgs, int32_t* host_status, hipStream_t st) {
  launch_hscale(b, hs_wgs, st);
  // (always the flat grid: every image's own tiles, three planes each)
  hipLaunchKernelGGL(yuv_planes_kernel, dim3(sws_wgs), dim3(256), lds_bytes, st, b.planes, b.desc,
                     b.infos, b.wts, static_cast<uint8_t*>(out), host_status, b.hbuf, b.sws_map,
                     b.flips);
  return hipGetLastError();
}

}  // namespace hj
