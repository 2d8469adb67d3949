// hj_sws.cpp -- host-side plan of the swscale conversion (see hj_sws.h).
//
// The algorithm is libswscale's (third-party FFmpeg, CI pin conda-forge
// ffmpeg 8.0, .github/workflows/_build_linux.yml:127), x86-64 build:
//   sws_init_context   (libswscale/utils.c)  chroma sizes, xInc, forced full
//                                            chroma, get_local_pos siting
//   initFilter         (utils.c)             taps per axis
//   packed_vscale      (vscale.c)            writer per output row
//   ff_yuv2rgb_c_init_tables (yuv2rgb.c)     BT.601 full-range coefficients
//   ff_get_unscaled_swscale                  yuv2rgb_c_24_rgb special case
// The test oracle restates the same algorithm separately
// (oracle/sws_oracle.c); the GPU parity tests compare the two end to end.
#include "hj_sws.h"

#include <math.h>
#include <string.h>

#include <algorithm>

#include "../../include/spdl_hipjpeg.h"
#include "hj_sws_tile.h"

namespace hj {
namespace {

constexpr double kReduceCutoff = 0.002;  // SWS_MAX_REDUCE_CUTOFF
constexpr int kMaxFilterSize = 256;      // SWS_MAX_FILTER_SIZE (longer -> cascade)

inline int64_t c_div(int64_t a, int64_t b) { return a / b; }  // C: truncates
inline int64_t rounded_div(int64_t a, int64_t b) { return (a >= 0 ? a + (b >> 1) : a - (b >> 1)) / b; }
inline int ilog2(unsigned v) { return v ? 31 - __builtin_clz(v) : 0; }  // av_log2

// The fixed-point kernel value at distance d (2^30 = one source sample after
// the downscale widening) for swscale's SWS_BICUBIC / SWS_BILINEAR /
// SWS_LANCZOS, in units of `fone`.
int64_t kernel_tap(int kind, int64_t d, int64_t fone) {
  if (kind == SPDL_HJ_FILTER_BILINEAR) {
    int64_t c = (1 << 30) - d;
    return (c < 0 ? 0 : c) * (fone >> 30);
  }
  if (kind == SPDL_HJ_FILTER_LANCZOS) {
    const double p = 3.0, x = d * (1.0 / (1 << 30));
    int64_t c = (int64_t)((d ? sin(x * M_PI) * sin(x * M_PI / p) / (x * x * M_PI * M_PI / p) : 1.0) *
                          fone);
    return x > p ? 0 : c;
  }
  // Mitchell-Netravali with swscale's defaults B = 0, C = 0.6 in Q24
  const int64_t B = 0, C = (int64_t)(0.6 * (1 << 24));
  int64_t c = 0;
  if (d < 1LL << 31) {
    const int64_t d2 = (d * d) >> 30, d3 = (d2 * d) >> 30;
    if (d < 1LL << 30)
      c = (12 * (1 << 24) - 9 * B - 6 * C) * d3 + (-18 * (1 << 24) + 12 * B + 6 * C) * d2 +
          (6 * (1 << 24) - 2 * B) * (1 << 30);
    else
      c = (-B - 6 * C) * d3 + (6 * B + 30 * C) * d2 + (-12 * B - 48 * C) * d +
          (8 * B + 24 * C) * (1 << 30);
  }
  return c / ((1LL << 54) / fone);
}

class FilterBuilder {
 public:
  FilterBuilder(int xInc, int src, int dst, int align, int one, int kind, int src_pos, int dst_pos)
      : xinc_(xInc), src_(src), dst_(dst), align_(align), one_(one), kind_(kind), sp_(src_pos),
        dp_(dst_pos) {
    const int r = ilog2((unsigned)(src / dst));
    fone_ = 1LL << (54 - (r < 8 ? r : 8));
  }

  bool build(SwsAxis* out) {
    sample();
    const int fs = reduce();
    if (fs >= kMaxFilterSize) return false;
    fold_borders(fs);
    normalise(fs, out);
    return true;
  }

 private:
  // initial taps: identity when unscaled, else the kernel over a window of
  // `size_` samples starting at the truncated (C division) window origin
  void sample() {
    pos_.assign(dst_, 0);
    if (llabs((int64_t)xinc_ - 0x10000) < 10 && sp_ == dp_) {
      size_ = 1;
      taps_.assign(dst_, fone_);
      for (int i = 0; i < dst_; i++) pos_[i] = i;
      return;
    }
    const int factor = kind_ == SPDL_HJ_FILTER_BILINEAR ? 2 : kind_ == SPDL_HJ_FILTER_LANCZOS ? 6 : 4;
    size_ = xinc_ <= (1 << 16) ? 1 + factor : 1 + (factor * src_ + dst_ - 1) / dst_;
    size_ = std::max(1, std::min(size_, src_ - 2));
    taps_.assign((size_t)dst_ * size_, 0);
    int64_t center = ((dp_ * (int64_t)xinc_) >> 7) - ((sp_ * 0x10000LL) >> 7);  // Q17
    for (int i = 0; i < dst_; i++, center += 2LL * xinc_) {
      int xx = (int)c_div(center - (size_ - 2) * (1LL << 16), 1 << 17);
      pos_[i] = xx;
      for (int j = 0; j < size_; j++, xx++) {
        int64_t d = llabs((int64_t)xx * (1 << 17) - center) << 13;
        if (xinc_ > 1 << 16) d = d * dst_ / src_;
        taps_[(size_t)i * size_ + j] = kernel_tap(kind_, d, fone_);
      }
    }
  }

  // drop near-zero taps (cumulative |tap| <= 0.002) from the left of every
  // row while positions stay monotonic, measure the widest row's right
  // trim, align the size
  int reduce() {
    const double cut = kReduceCutoff * fone_;
    int widest = 0;
    for (int i = dst_ - 1; i >= 0; i--) {
      int64_t* row = &taps_[(size_t)i * size_];
      int64_t acc = 0;
      for (int j = 0; j < size_; j++) {
        acc += llabs(row[0]);
        if (acc > cut) break;
        if (i < dst_ - 1 && pos_[i] >= pos_[i + 1]) break;
        std::copy(row + 1, row + size_, row);
        row[size_ - 1] = 0;
        pos_[i]++;
      }
      int keep = size_;
      acc = 0;
      for (int j = size_ - 1; j > 0; j--) {
        acc += llabs(row[j]);
        if (acc > cut) break;
        keep--;
      }
      widest = std::max(widest, keep);
    }
    int align = align_;
    if (widest == 1 && align == 2) align = 1;  // x86: unscaled vertical stays 1
    const int fs = (widest + align - 1) & ~(align - 1);
    std::vector<int64_t> t((size_t)dst_ * fs, 0);
    for (int i = 0; i < dst_; i++)
      for (int j = 0; j < fs && j < size_; j++) t[(size_t)i * fs + j] = taps_[(size_t)i * size_ + j];
    taps_.swap(t);
    size_ = fs;
    return fs;
  }

  // taps left of sample 0 / right of src-1 fold into the edge sample
  void fold_borders(int fs) {
    for (int i = 0; i < dst_; i++) {
      int64_t* row = &taps_[(size_t)i * fs];
      if (pos_[i] < 0) {
        for (int j = 1; j < fs; j++) {
          const int to = std::max(j + pos_[i], 0);
          row[to] += row[j];
          row[j] = 0;
        }
        pos_[i] = 0;
      }
      if (pos_[i] + fs > src_) {
        const int shift = pos_[i] + std::min(fs - src_, 0);
        int64_t spill = 0;
        for (int j = fs - 1; j >= 0; j--)
          if (pos_[i] + j >= src_) {
            spill += row[j];
            row[j] = 0;
          }
        for (int j = fs - 1; j >= 0; j--) row[j] = j < shift ? 0 : row[j - shift];
        pos_[i] -= shift;
        row[src_ - 1 - pos_[i]] += spill;
      }
    }
  }

  void normalise(int fs, SwsAxis* out) {
    out->size = fs;
    out->n = dst_;
    out->pos = pos_;
    out->coef.assign((size_t)dst_ * fs, 0);
    out->eff = 1;
    for (int i = 0; i < dst_; i++) {
      const int64_t* row = &taps_[(size_t)i * fs];
      int64_t sum = 0, err = 0;
      for (int j = 0; j < fs; j++) sum += row[j];
      sum = (sum + one_ / 2) / one_;
      if (!sum) sum = 1;
      for (int j = 0; j < fs; j++) {
        const int64_t v = row[j] + err;
        const int q = (int)rounded_div(v, sum);
        out->coef[(size_t)i * fs + j] = (int16_t)q;
        err = v - (int64_t)q * sum;
        if (q) out->eff = std::max(out->eff, j + 1);
      }
    }
  }

  int xinc_, src_, dst_, align_, one_, kind_, sp_, dp_;
  int64_t fone_;
  int size_ = 0;
  std::vector<int32_t> pos_;
  std::vector<int64_t> taps_;
};

// One axis, memoised per thread (a context is one thread's): initFilter's
// result depends on these seven numbers alone, and a stream of source crops --
// one new geometry per image -- repeats its axes long before it repeats a
// geometry (RandomResizedCrop of 480x640 frames to 224x224: 300,000 sizes,
// about 1,100 axes).  Bounded: cleared at kAxisMemo entries (~5 KB each at 224
// outputs).  A filter too long for swscale (false) is not kept.
int64_t xinc(int src, int dst) { return (((int64_t)src << 16) + (dst >> 1)) / dst; }

constexpr size_t kAxisMemo = 2048;
bool build_axis(int src, int dst, int align, int one, int kind, int src_pos, int dst_pos,
                SwsAxis* out) {
  using Key = std::tuple<int, int, int, int, int, int, int>;
  thread_local std::map<Key, std::shared_ptr<const SwsAxis>> memo;
  const Key key{src, dst, align, one, kind, src_pos, dst_pos};
  // swscale keeps xInc in an int: a ratio of 32768 or more does not fit, and
  // what the wrapped value would select (an upscale's few taps) is nothing to
  // pin.  Refused, like every filter swscale would cascade.
  if (xinc(src, dst) > INT32_MAX) return false;
  auto it = memo.find(key);
  if (it == memo.end()) {
    auto a = std::make_shared<SwsAxis>();
    FilterBuilder fb((int)xinc(src, dst), src, dst, align, one, kind, src_pos, dst_pos);
    if (!fb.build(a.get())) return false;
    if (memo.size() >= kAxisMemo) memo.clear();
    it = memo.emplace(key, std::move(a)).first;
  }
  *out = *it->second;
  return true;
}

// utils.c get_local_pos: -513 (unset) means centred
int local_pos(int sub, int pos) {
  if (pos == -1 || pos <= -513) pos = (128 << sub) - 128;
  return (pos + 128) >> sub;
}

int ceil_rshift(int a, int b) { return -((-a) >> b); }

void identity(SwsAxis* a, int n, int one, int shift) {
  a->size = a->eff = 1;
  a->n = n;
  a->pos.resize(n);
  a->coef.assign(n, (int16_t)one);
  for (int i = 0; i < n; i++) a->pos[i] = i >> shift;
}

int16_t round_to_int16(int64_t f) {  // utils.c roundToInt16
  const int r = (int)((f + (1 << 15)) >> 16);
  return (int16_t)(r < -0x7FFF ? -0x8000 : r > 0x7FFF ? 0x7FFF : r);
}

}  // namespace

SwsCsc sws_csc() {
  // ff_yuv2rgb_coeffs[SWS_CS_ITU601]; contrast = saturation = 1 << 16,
  // brightness 0; full range (yuvj: srcRange 1) scales the chroma terms
  int64_t crv = 104597, cbu = 132201, cgu = -25675, cgv = -53279;
  const int64_t cy = 1 << 16, oy = 0;
  crv = crv * 224 / 255;
  cbu = cbu * 224 / 255;
  cgu = cgu * 224 / 255;
  cgv = cgv * 224 / 255;
  SwsCsc c;
  c.y_coeff = round_to_int16(cy * (1 << 13));
  c.y_offset = round_to_int16(oy * (1 << 9));
  c.v2r = round_to_int16(crv * (1 << 13));
  c.v2g = round_to_int16(cgv * (1 << 13));
  c.u2g = round_to_int16(cgu * (1 << 13));
  c.u2b = round_to_int16(cbu * (1 << 13));
  c.crv = (int32_t)((crv * (1 << 16) + 0x8000) / cy);
  c.cbu = (int32_t)((cbu * (1 << 16) + 0x8000) / cy);
  c.cgu = (int32_t)((cgu * (1 << 16) + 0x8000) / cy);
  c.cgv = (int32_t)((cgv * (1 << 16) + 0x8000) / cy);
  return c;
}

int sws_plan(int srcW, int srcH, int hsub, int vsub, bool gray, int dstW, int dstH, int kind,
             SwsPlan* p) {
  *p = SwsPlan{};
  p->srcW = srcW;
  p->srcH = srcH;
  p->dstW = dstW;
  p->dstH = dstH;
  p->gray = gray;
  p->hsub = gray ? 0 : hsub;
  p->vsub = gray ? 0 : vsub;
  p->vmode.assign(dstH, kSwsX);
  const bool same = srcW == dstW && srcH == dstH;
  if (same && !gray && hsub == 1 && (vsub == 0 || (vsub == 1 && !(dstH & 1))) && !(dstW & 1)) {
    // yuv2rgb_c_24_rgb: nearest chroma (rows y >> vsub, pairs of columns)
    p->special = true;
    p->chrSrcW = p->chrDstW = ceil_rshift(srcW, hsub);
    p->chrSrcH = ceil_rshift(srcH, vsub);
    p->chrDstH = dstH;
    identity(&p->hl, dstW, 1 << 14, 0);
    identity(&p->vl, dstH, 1 << 12, 0);
    identity(&p->hc, p->chrDstW, 1 << 14, 0);
    identity(&p->vc, dstH, 1 << 12, vsub);
    p->vmode.assign(dstH, kSwsOne);
    return SPDL_HJ_OK;
  }
  p->full = (dstW & 1) || (p->hsub == 0 && p->vsub == 0);
  const int dst_hsub = p->full ? 0 : 1;
  p->chrSrcW = ceil_rshift(srcW, p->hsub);
  p->chrSrcH = ceil_rshift(srcH, p->vsub);
  p->chrDstW = ceil_rshift(dstW, dst_hsub);
  p->chrDstH = dstH;
  const int lp = local_pos(0, 0);
  if (!build_axis(srcW, dstW, 4, 1 << 14, kind, lp, lp, &p->hl) ||
      !build_axis(srcH, dstH, 2, 1 << 12, kind, lp, lp, &p->vl))
    return SPDL_HJ_ERR_BAD_GEOMETRY;
  if (!gray) {
    if (!build_axis(p->chrSrcW, p->chrDstW, 4, 1 << 14, kind, local_pos(p->hsub, -513),
                    local_pos(dst_hsub, -513), &p->hc) ||
        !build_axis(p->chrSrcH, p->chrDstH, 2, 1 << 12, kind, local_pos(p->vsub, -513),
                    local_pos(0, -513), &p->vc))
      return SPDL_HJ_ERR_BAD_GEOMETRY;
  }
  // packed_vscale's choice per output row
  const int lfs = p->vl.size, cfs = gray ? 1 : p->vc.size;
  for (int y = 0; y < dstH; y++) {
    const int16_t* lf = &p->vl.coef[(size_t)y * lfs];
    const int16_t* cf = gray ? nullptr : &p->vc.coef[(size_t)y * cfs];
    auto bilin = [](const int16_t* f) { return f[0] + f[1] == 4096 && (unsigned)f[1] <= 4096u; };
    int32_t m = kSwsX;
    if (gray) {
      if (lfs == 1) m = kSwsOne;
      else if (lfs == 2 && bilin(lf)) m = kSwsTwo | (lf[1] << 4);
    } else if (lfs == 1 && cfs == 1) {
      m = kSwsOne;
    } else if (lfs == 1 && cfs == 2 && bilin(cf)) {
      m = kSwsOne | (cf[1] << 17);
    } else if (lfs == 2 && cfs == 2 && bilin(lf) && bilin(cf)) {
      m = kSwsTwo | (lf[1] << 4) | (cf[1] << 17);
    }
    p->vmode[y] = m;
  }
  return SPDL_HJ_OK;
}

int sws_plan_planar(int srcW, int srcH, int hsub, int vsub, bool gray, int dstW, int dstH, int kind,
                    SwsPlan* p) {
  *p = SwsPlan{};
  p->srcW = srcW;
  p->srcH = srcH;
  p->dstW = dstW;
  p->dstH = dstH;
  p->gray = gray;
  p->hsub = gray ? 0 : hsub;
  p->vsub = gray ? 0 : vsub;
  p->chrSrcW = ceil_rshift(srcW, p->hsub);
  p->chrSrcH = ceil_rshift(srcH, p->vsub);
  p->chrDstW = ceil_rshift(dstW, p->hsub);
  p->chrDstH = ceil_rshift(dstH, p->vsub);
  const int lp = local_pos(0, 0);
  if (!build_axis(srcW, dstW, 4, 1 << 14, kind, lp, lp, &p->hl) ||
      !build_axis(srcH, dstH, 2, 1 << 12, kind, lp, lp, &p->vl))
    return SPDL_HJ_ERR_BAD_GEOMETRY;
  if (!gray) {
    const int hp = local_pos(p->hsub, -513), vp = local_pos(p->vsub, -513);
    if (!build_axis(p->chrSrcW, p->chrDstW, 4, 1 << 14, kind, hp, hp, &p->hc) ||
        !build_axis(p->chrSrcH, p->chrDstH, 2, 1 << 12, kind, vp, vp, &p->vc))
      return SPDL_HJ_ERR_BAD_GEOMETRY;
  }
  // yuv2plane1 ignores its tap (see hj_sws.h)
  for (SwsAxis* a : {&p->vl, &p->vc})
    if (a->size == 1) std::fill(a->coef.begin(), a->coef.end(), (int16_t)(1 << 12));
  return SPDL_HJ_OK;
}

// ---- the packer and the tiler ----------------------------------------------
namespace {

void put(std::vector<int32_t>& blob, int32_t* off, const void* data, size_t bytes) {
  *off = (int32_t)blob.size();
  const size_t words = (bytes + 3) / 4;
  blob.resize(blob.size() + ((words + 3) & ~(size_t)3), 0);
  if (bytes) memcpy(blob.data() + *off, data, bytes);
}

// source rows a vertical filter reaches (first tap + taps, max over rows)
int reach(const SwsAxis& a) {
  int r = 0;
  for (int y = 0; y < a.n; y++) r = std::max(r, a.pos[y] + a.eff);
  return r;
}

// What both destinations share: the sizes, the tables of the plan into the
// blob, and the pre-pass switch and its rows.
void pack_tables(const PlanKey& k, const SwsPlan& pl, int pre_mode, PackedPlan* pp) {
  SwsDesc& d = pp->d;
  d.sw = k.sw;
  d.sh = k.sh;
  d.chr_w = pl.chrDstW;
  d.gray = pl.gray;
  const SwsAxis* ax[4] = {&pl.hl, &pl.hc, &pl.vl, &pl.vc};
  int32_t* taps[4] = {&d.hl_taps, &d.hc_taps, &d.vl_taps, &d.vc_taps};
  int32_t* sizes[4] = {&d.hl_size, &d.hc_size, &d.vl_size, &d.vc_size};
  for (int i = 0; i < 4; i++) {
    // rows cut to the taps that are ever non-zero, padded to a multiple
    // of 4 (the kernel reads taps 4 at a time); horizontal rows to the
    // kernel's register bucket of taps (hpass: 4, 8, 12, 16, 24, 32, 48, 64;
    // longer rows use a plain loop)
    const SwsAxis& a = *ax[i];
    pp->axis_n[i] = a.n;
    const int eff = a.eff;
    int q = (eff + 3) / 4;
    if (i < 2) q = q <= 4 ? q : q <= 6 ? 6 : q <= 8 ? 8 : q <= 12 ? 12 : q <= 16 ? 16 : q;
    const int stride = 4 * q;
    *taps[i] = eff;
    *sizes[i] = stride;
    std::vector<int16_t> rows((size_t)a.n * stride, 0);
    for (int r = 0; r < a.n; r++)
      for (int t = 0; t < eff; t++) rows[(size_t)r * stride + t] = a.coef[(size_t)r * a.size + t];
    put(pp->blob, &d.off[2 * i], a.pos.data(), a.pos.size() * 4);
    put(pp->blob, &d.off[2 * i + 1], rows.data(), rows.size() * 2);
  }
  put(pp->blob, &d.off[kVmode], pl.vmode.data(), pl.vmode.size() * 4);  // (planar: none)
  d.pre = pre_mode > 0 || (pre_mode < 0 && !pp->special &&
                           (k.h >= PlanCache::kPreRatio * k.sh || pl.hl.eff > 64));
  d.pre_rl = d.pre ? reach(pl.vl) : 0;
  d.pre_rc = d.pre && !pl.gray ? reach(pl.vc) : 0;
}

// Tiling: the widest column chunk, then the tallest band, whose largest tile's
// LDS (lds_of(rb, chunk), bytes) fits the budget.  The launch's LDS is the
// batch's largest plan's, so a plan over the budget slows every image's tiles:
// only a one-row band of a plan without the hscale pre-pass may exceed it.
template <class LdsOf>
bool pick_tile(int ow, int max_cols, PackedPlan* pp, LdsOf lds_of) {
  SwsDesc& d = pp->d;
  for (int cols = std::min(max_cols, kSwsMaxCols); cols >= 16; cols /= 2) {
    const int chunk = ow < cols ? ow : cols;
    for (int rb : {32, 24, 16, 12, 8, 6, 4, 3, 2, 1}) {
      const int lds = lds_of(rb, chunk);
      if (lds <= kSwsLdsBudget || (!d.pre && rb == 1 && lds <= 64 * 1024)) {
        d.rb = rb;
        d.col_chunk = chunk;
        pp->lds = lds;
        return true;
      }
    }
  }
  return false;
}

int build_rgb(const PlanKey& k, int pre_mode, int max_cols, PackedPlan* pp) {
  SwsPlan pl;
  // gbr: the luma plan (gray) applied to each of the three RGB planes
  if (int rc = sws_plan(k.w, k.h, k.hsub, k.vsub, k.mode != kPlanYuv, k.sw, k.sh, k.filter, &pl))
    return rc;
  pp->special = pl.special && k.dx == 0 && k.dy == 0 && k.ow == k.sw && k.oh == k.sh;
  SwsDesc& d = pp->d;
  d.full = pl.full;
  d.gbr = k.mode == kPlanGbr;
  pack_tables(k, pl, pre_mode, pp);
  const auto lds_of = [&](int rb, int chunk) {
    int lds = sws_lds_layout(0, 0, 0, 0, d.gbr, pl.gray, rb, chunk, d.vl_size, d.vc_size).end;
    for (int yo0 = 0; yo0 < k.oh; yo0 += rb)
      for (int xo0 = 0; xo0 < k.ow; xo0 += chunk) {
        // (whole bands and chunks: a short last one is sized as a whole one)
        const SwsWindow w =
            sws_window(yo0, xo0, rb, chunk, k.dx, k.dy, xo0 + chunk, yo0 + rb, k.sw, k.sh);
        if (!w.content) continue;
        const int lrows = pl.vl.pos[w.ys1 - 1] + pl.vl.eff - pl.vl.pos[w.ys0];
        const int crows = pl.gray ? 0 : pl.vc.pos[w.ys1 - 1] + pl.vc.eff - pl.vc.pos[w.ys0];
        const int ncc = pl.gray ? 0 : sws_chroma_cols(w.xs0, w.xs1, pl.full).ncc;
        lds = std::max(lds, sws_lds_layout(w.xs1 - w.xs0, ncc, lrows, crows, d.gbr, pl.gray, rb, chunk,
                                           d.vl_size, d.vc_size).end);
      }
    return lds;
  };
  if (!pick_tile(k.ow, max_cols, pp, lds_of)) return SPDL_HJ_ERR_BAD_GEOMETRY;
  pp->bands = tile_div_up(k.oh, d.rb);
  pp->chunks = tile_div_up(k.ow, d.col_chunk);
  return SPDL_HJ_OK;
}

// The planar destination (hj_sws.h sws_plan_planar): the same tables (no row
// writers), one band height and column chunk for the luma and the chroma tiles
int build_planar(const PlanKey& k, int pre_mode, int max_cols, PackedPlan* pp) {
  SwsPlan pl;
  const bool gray = (k.mode & ~kPlanPlanar) == kPlanGray;
  if (int rc = sws_plan_planar(k.w, k.h, k.hsub, k.vsub, gray, k.sw, k.sh, k.filter, &pl)) return rc;
  SwsDesc& d = pp->d;
  d.chr_h = pl.chrDstH;
  d.yuv = 1;
  d.hsub = pl.hsub;
  d.vsub = pl.vsub;
  pack_tables(k, pl, pre_mode, pp);
  // the planes' placement: luma as the key says, chroma at the shifted
  // offset (a multiple of the ratio: geometry()) in a ceil-shifted box
  const SwsAxis* pv[2] = {&pl.vl, &pl.vc};
  const int psw[2] = {k.sw, pl.chrDstW}, psh[2] = {k.sh, pl.chrDstH};
  const int pdy[2] = {k.dy, k.dy >> pl.vsub};
  const int poh[2] = {k.oh, planar_tiles(k.ow, k.oh, pl.hsub, pl.vsub, 1, 1, pl.gray).ch};
  const auto lds_of = [&](int rb, int chunk) {
    int lds = planar_lds_layout(0, 0, rb, chunk).bound;
    for (int c = 0; c < (pl.gray ? 1 : 2); c++)
      for (int yo0 = 0; yo0 < poh[c]; yo0 += rb) {
        // (a whole band: a short last one is sized as a whole one)
        const SwsWindow w = sws_window(yo0, 0, rb, chunk, 0, pdy[c], chunk, yo0 + rb, psw[c], psh[c]);
        if (w.ys0 >= w.ys1) continue;
        const int rows = pv[c]->pos[w.ys1 - 1] + pv[c]->eff - pv[c]->pos[w.ys0];
        lds = std::max(lds, planar_lds_layout(std::min(chunk, psw[c]), rows, rb, chunk).bound);
      }
    return lds;
  };
  if (!pick_tile(k.ow, max_cols, pp, lds_of)) return SPDL_HJ_ERR_BAD_GEOMETRY;
  pp->bands = planar_tiles(k.ow, k.oh, pl.hsub, pl.vsub, d.rb, d.col_chunk, pl.gray).total;
  pp->chunks = 1;
  return SPDL_HJ_OK;
}

}  // namespace

std::shared_ptr<const PackedPlan> PlanCache::build(const PlanKey& k, int* rc, int pre_mode,
                                                   int max_cols) {
  auto pp = std::make_shared<PackedPlan>();
  *rc = (k.mode & kPlanPlanar ? build_planar : build_rgb)(k, pre_mode, max_cols, pp.get());
  return *rc ? nullptr : pp;
}

std::shared_ptr<const PackedPlan> PlanCache::get(const PlanKey& k, int* rc) {
  auto it = map_.find(k);
  if (it != map_.end()) return it->second;
  auto p = build(k, rc, pre_mode_, max_cols_);
  if (!p) return nullptr;
  if (map_.size() >= 512) map_.clear();  // bounded: a stream of odd sizes replans
  map_.emplace(k, p);
  return p;
}

}  // namespace hj
