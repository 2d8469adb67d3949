// hj_resample.cpp -- the coefficient rule, the axis cache and the tiler of the
// Pillow-exact resize (hj_resample.h).  Built with -ffp-contract=off: the
// rule's doubles are evaluated in the order written, nothing fused.
#include "hj_resample.h"

#include <math.h>

#include <algorithm>

namespace hj {
namespace rs {
namespace {

double f_bilinear(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}
double f_bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
double sinc(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}
double f_lanczos(double x) { return -3.0 <= x && x < 3.0 ? sinc(x) * sinc(x / 3) : 0.0; }

struct Filter {
  double (*f)(double);
  double support;
};
bool filter_of(int filter, Filter* out) {
  switch (filter) {
    case SPDL_HJ_FILTER_BILINEAR: *out = {f_bilinear, 1.0}; return true;
    case SPDL_HJ_FILTER_BICUBIC: *out = {f_bicubic, 2.0}; return true;
    case SPDL_HJ_FILTER_LANCZOS: *out = {f_lanczos, 3.0}; return true;
  }
  return false;
}

// Output xx's sample range [xmin, xmax) and its centre
struct Span {
  int xmin, xmax;
  double center;
};
Span span_of(int xx, int in, double in0, double scale, double support) {
  const double center = in0 + (xx + 0.5) * scale;
  Span s;
  s.center = center;
  s.xmin = std::max((int)(center - support + 0.5), 0);
  s.xmax = std::min((int)(center + support + 0.5), in);
  return s;
}
bool sizes_ok(int in, int out) { return in >= 1 && in <= 65535 && out >= 1 && out <= 65535; }
// Pillow takes a box in single precision and subtracts its ends there; an
// integer box (0, inSize) is exact in it
double box_scale(double* in0, double in1, int out) {
  const float lo = (float)*in0, hi = (float)in1;
  *in0 = (double)lo;
  return (double)(hi - lo) / out;
}

}  // namespace

int axis_taps(int in, double in0, double in1, int out, int filter) {
  Filter flt;
  if (!sizes_ok(in, out) || !filter_of(filter, &flt)) return 0;
  const double scale = box_scale(&in0, in1, out);
  const double support = flt.support * std::max(scale, 1.0);
  int taps = 0;
  for (int xx = 0; xx < out; xx++) {
    const Span s = span_of(xx, in, in0, scale, support);
    taps = std::max(taps, s.xmax - s.xmin);
  }
  return taps;
}

std::shared_ptr<const Axis> make_axis(int in, double in0, double in1, int out, int filter,
                                      int* rc) {
  Filter flt;
  if (!sizes_ok(in, out) || !filter_of(filter, &flt) ||
      !(in0 >= 0 && (float)in0 < (float)in1 && in1 <= in)) {  // (not empty in single precision)
    *rc = SPDL_HJ_ERR_INVALID_ARG;
    return nullptr;
  }
  const int ksize = axis_taps(in, in0, in1, out, filter);
  if (ksize < 1 || ksize > kMaxTaps) {
    *rc = SPDL_HJ_ERR_BAD_GEOMETRY;
    return nullptr;
  }
  auto a = std::make_shared<Axis>();
  a->in = in;
  a->out = out;
  a->filter = filter;
  a->ksize = ksize;
  a->in0 = in0;
  a->in1 = in1;
  a->blob.assign(2 * (size_t)out + (size_t)out * ksize, 0);
  int32_t* xmin = a->blob.data();
  int32_t* n = xmin + out;
  int32_t* K = n + out;
  const double scale = box_scale(&in0, in1, out);
  const double filterscale = std::max(scale, 1.0);
  const double support = flt.support * filterscale;
  const double ss = 1.0 / filterscale;
  std::vector<double> w(ksize);
  for (int xx = 0; xx < out; xx++) {
    const Span s = span_of(xx, in, in0, scale, support);
    const int cnt = s.xmax - s.xmin;
    double ww = 0.0;
    for (int x = 0; x < cnt; x++) {
      w[x] = flt.f((x + s.xmin - s.center + 0.5) * ss);
      ww += w[x];
    }
    xmin[xx] = s.xmin;
    n[xx] = cnt;
    for (int x = 0; x < cnt; x++) {
      const double k = ww != 0.0 ? w[x] / ww : w[x];
      K[(size_t)xx * ksize + x] = k < 0 ? (int)(-0.5 + k * (double)(1 << kCoefBits))
                                        : (int)(0.5 + k * (double)(1 << kCoefBits));
    }
  }
  *rc = SPDL_HJ_OK;
  return a;
}

std::shared_ptr<const Axis> AxisCache::get(int in, double in0, double in1, int out, int filter,
                                           int* rc) {
  const auto key = std::make_tuple(in, (double)(float)in0, (double)(float)in1, out, filter);
  auto it = held.find(key);
  if (it != held.end()) {
    *rc = SPDL_HJ_OK;
    return it->second;
  }
  auto a = make_axis(in, in0, in1, out, filter, rc);
  if (!a) return nullptr;
  if (held.size() >= kCap) held.clear();
  held.emplace(key, a);
  return a;
}

int resolve(const spdl_hj_resample_item* it, int W, int H, int out_w, int out_h, Geo* g) {
  *g = Geo{0, 0, W, H, out_w, out_h, 0, 0};
  if (!it) return SPDL_HJ_OK;
  if (it->box.w != 0) {
    const spdl_hj_rect& b = it->box;
    if (b.x < 0 || b.y < 0 || b.w < 1 || b.h < 1 || b.x > W - b.w || b.y > H - b.h)
      return SPDL_HJ_ERR_BAD_GEOMETRY;
    g->bx = b.x;
    g->by = b.y;
    g->bw = b.w;
    g->bh = b.h;
  }
  if (it->rw) g->rw = it->rw;
  if (it->rh) g->rh = it->rh;
  g->ox = it->ox;
  g->oy = it->oy;
  if (g->rw < 1 || g->rw > 65535 || g->rh < 1 || g->rh > 65535 || g->ox < 0 || g->oy < 0 ||
      g->ox > g->rw - out_w || g->oy > g->rh - out_h)
    return SPDL_HJ_ERR_BAD_GEOMETRY;
  return SPDL_HJ_OK;
}

namespace {
// tile() for either kernel.  reduce: resample_reduce_kernel's -- windows
// unaligned, the LDS with the second sums' plane.  aligned: the windows start
// on the producer's 8 x 2 units (tile()'s, not tile_oriented()'s)
int tile_for(bool reduce, bool aligned, int nch, const Axis& H, const Axis& V, const Geo& g,
             int out_w, int out_h, ResampleDesc* d, int* bands, int* chunks) {
  const int tile_w = nch == 1 ? kTileW1 : kTileW;
  const int sum_planes = nch == 1 ? 0 : 1;  // (planes of sums beside the strip)
  const int ax = aligned ? 8 : 1, ay = aligned ? 2 : 1;
  ResampleDesc t{};
  t.bx = g.bx;
  t.by = g.by;
  t.ox = g.ox;
  t.oy = g.oy;
  t.kh = H.ksize;
  t.kv = V.ksize;
  t.tw = 8;  // (8, 16, 32, 64 or 128: halving keeps it a multiple of the store's 8 columns)
  while (t.tw < tile_w && t.tw < out_w) t.tw *= 2;
  t.th = kTileH;
  while (t.th > 1 && t.th / 2 >= out_h) t.th /= 2;
  t.sr = kStripRows;
  for (;;) {
    // the widest and the tallest source window of a tile of this size
    const int nx = (out_w + t.tw - 1) / t.tw, ny = (out_h + t.th - 1) / t.th;
    int cols = 0, rows = 0;
    for (int i = 0; i < nx; i++) {
      const Window w = tile_window(H.xmin(), H.n(), g.bx, g.ox, out_w, t.tw, i, ax);
      cols = std::max(cols, w.hi - w.lo);
    }
    for (int j = 0; j < ny; j++) {
      const Window w = tile_window(V.xmin(), V.n(), g.by, g.oy, out_h, t.th, j, ay);
      rows = std::max(rows, w.hi - w.lo);
    }
    while (t.sr > 2 && t.sr / 2 >= rows) t.sr /= 2;  // (no strip taller than the window)
    // (one channel, no sums: a strip row of bytes, 8 columns are two words)
    t.pitch = nch == 1 && !reduce ? (((cols + 7) >> 3) << 1) | 1 : ((cols + 7) & ~7) | 1;
    t.rows = rows;
    LdsLayout l = lds_layout(t, nch);
    if (reduce) l.words = reduce_lds_words(t, nch);
    if (l.words * 4 <= kLdsBudget) {
      *d = t;
      *bands = ny;
      *chunks = nx;
      return SPDL_HJ_OK;
    }
    // shrink what takes the most: the strip by its rows (down to 16: a wave's
    // lanes run along them) and then by the tile's columns, the intermediate
    // and the coefficient rows by the tile's rows first
    const int strip = (reduce ? 1 + sum_planes : 1) * t.sr * t.pitch, rest = l.words - strip;
    if (strip >= rest) {
      if (t.sr > 16) t.sr /= 2;
      else if (t.tw > 8) t.tw /= 2;
      else if (t.sr > 2) t.sr /= 2;
      else if (t.th > 1) t.th /= 2;
      else break;
    } else {
      if (t.th > 1) t.th /= 2;
      else if (t.tw > 8) t.tw /= 2;
      else if (t.sr > 2) t.sr /= 2;
      else break;
    }
  }
  *d = ResampleDesc{};
  *bands = *chunks = 0;
  return SPDL_HJ_ERR_BAD_GEOMETRY;
}
}  // namespace

int tile(const Axis& H, const Axis& V, const Geo& g, int out_w, int out_h, ResampleDesc* d,
         int* bands, int* chunks, int nch) {
  return tile_for(false, true, nch, H, V, g, out_w, out_h, d, bands, chunks);
}
int tile_oriented(const Axis& H, const Axis& V, const Geo& g, int out_w, int out_h, ResampleDesc* d,
                  int* bands, int* chunks) {
  return tile_for(false, false, 3, H, V, g, out_w, out_h, d, bands, chunks);
}
int tile_reduce(const Axis& H, const Axis& V, const Geo& g, int out_w, int out_h, ResampleDesc* d,
                int* bands, int* chunks, int nch) {
  return tile_for(true, false, nch, H, V, g, out_w, out_h, d, bands, chunks);
}

int place(AxisCache& cache, int filter, const spdl_hj_resample_item* it, int W, int H, int out_w,
          int out_h, Placed* out) {
  Geo g;
  int rc = resolve(it, W, H, out_w, out_h, &g);
  if (rc) return rc;
  out->H = cache.get(g.bw, g.rw, filter, &rc);
  if (!out->H) return rc;
  out->V = cache.get(g.bh, g.rh, filter, &rc);
  if (!out->V) return rc;
  return tile(*out->H, *out->V, g, out_w, out_h, &out->d, &out->bands, &out->chunks, cache.channels);
}

namespace {
// A placed image's two axes into the submission's table pool, each once
int pool_tables(const Placed& pl, std::vector<int32_t>& tables, ResamplePool& pool, ResampleDesc* d,
                int* bands, int* chunks) {
  int64_t at[2];
  const std::shared_ptr<const Axis> axes[2] = {pl.H, pl.V};
  for (int k = 0; k < 2; k++) {
    auto f = pool.placed.find(axes[k].get());
    if (f == pool.placed.end()) {
      f = pool.placed.emplace(axes[k].get(), (int64_t)tables.size()).first;
      pool.alive.push_back(axes[k]);  // (the cache may let go of it before the submission ends)
      tables.insert(tables.end(), axes[k]->blob.begin(), axes[k]->blob.end());
    }
    at[k] = f->second;
  }
  if ((int64_t)tables.size() > INT32_MAX) return SPDL_HJ_ERR_BAD_GEOMETRY;
  *d = pl.d;
  d->hx = (int32_t)at[0];
  d->hn = d->hx + pl.H->out;
  d->hk = d->hn + pl.H->out;
  d->vx = (int32_t)at[1];
  d->vn = d->vx + pl.V->out;
  d->vk = d->vn + pl.V->out;
  *bands = pl.bands;
  *chunks = pl.chunks;
  return SPDL_HJ_OK;
}
}  // namespace

int place_into(void* cache, int filter, const spdl_hj_resample_item* it, int W, int H, int out_w,
               int out_h, std::vector<int32_t>& tables, ResamplePool& pool, ResampleDesc* d,
               int* bands, int* chunks) {
  Placed pl;
  if (const int rc = place(*static_cast<AxisCache*>(cache), filter, it, W, H, out_w, out_h, &pl))
    return rc;
  return pool_tables(pl, tables, pool, d, bands, chunks);
}

int resolve_box(const spdl_hj_resample_box_item* it, int W, int H, int out_w, int out_h, int filter,
                double gap, BoxGeo* g) {
  Filter flt;
  if (!filter_of(filter, &flt)) return SPDL_HJ_ERR_INVALID_ARG;
  if (W < 1 || H < 1) return SPDL_HJ_ERR_BAD_GEOMETRY;
  if (!(gap == 0.0 || (gap >= 1.0 && gap <= 65536.0))) return SPDL_HJ_ERR_INVALID_ARG;
  double x0 = 0, y0 = 0, x1 = W, y1 = H;
  *g = BoxGeo{};
  g->rw = out_w;
  g->rh = out_h;
  if (it) {
    if (it->x0 != 0 || it->y0 != 0 || it->x1 != 0 || it->y1 != 0) {
      x0 = it->x0, y0 = it->y0, x1 = it->x1, y1 = it->y1;
      if (!(x0 >= 0 && y0 >= 0 && x0 < x1 && y0 < y1 && x1 <= W && y1 <= H))
        return SPDL_HJ_ERR_INVALID_ARG;
    }
    if (it->rw) g->rw = it->rw;
    if (it->rh) g->rh = it->rh;
    g->ox = it->ox;
    g->oy = it->oy;
  }
  if (g->rw < 1 || g->rw > 65535 || g->rh < 1 || g->rh > 65535 || g->ox < 0 || g->oy < 0 ||
      g->ox > g->rw - out_w || g->oy > g->rh - out_h)
    return SPDL_HJ_ERR_BAD_GEOMETRY;
  // (Pillow resizes such a frame in the other order: not restated)
  if ((int64_t)H > 100 * (int64_t)W && g->rh < y1 - y0) return SPDL_HJ_ERR_BAD_GEOMETRY;
  g->fx = g->fy = 1;
  if (gap != 0.0) {
    g->fx = (int)((x1 - x0) / g->rw / gap);
    g->fy = (int)((y1 - y0) / g->rh / gap);
    if (g->fx < 1) g->fx = 1;
    if (g->fy < 1) g->fy = 1;
  }
  g->q[2] = W;
  g->q[3] = H;
  if (g->fx > 1 || g->fy > 1) {
    if ((int64_t)g->fx * g->fy > kReduceMaxCell) return SPDL_HJ_ERR_BAD_GEOMETRY;
    const double s = flt.support - 0.5;
    const double sx = s * (x1 - x0) / g->rw, sy = s * (y1 - y0) / g->rh;
    g->q[0] = std::max(0, (int)(x0 - sx));
    g->q[1] = std::max(0, (int)(y0 - sy));
    g->q[2] = std::min(W, (int)ceil(x1 + sx));
    g->q[3] = std::min(H, (int)ceil(y1 + sy));
    x0 = (x0 - g->q[0]) / g->fx;
    y0 = (y0 - g->q[1]) / g->fy;
    x1 = (x1 - g->q[0]) / g->fx;
    y1 = (y1 - g->q[1]) / g->fy;
  }
  const int qw = g->q[2] - g->q[0], qh = g->q[3] - g->q[1];
  g->cw = (qw + g->fx - 1) / g->fx;
  g->ch = (qh + g->fy - 1) / g->fy;
  if ((int64_t)g->ch > 100 * (int64_t)g->cw && g->rh < y1 - y0) return SPDL_HJ_ERR_BAD_GEOMETRY;
  g->box[0] = x0, g->box[1] = y0, g->box[2] = x1, g->box[3] = y1;
  const int ex = qw % g->fx ? qw % g->fx : g->fx, ey = qh % g->fy ? qh % g->fy : g->fy;
  g->div[0] = g->fx * g->fy;
  g->div[1] = ex * g->fy;
  g->div[2] = g->fx * ey;
  g->div[3] = ex * ey;
  for (int k = 0; k < 4; k++) g->mult[k] = (1u << 24) / (uint32_t)g->div[k];
  return SPDL_HJ_OK;
}

int probe_box(int filter, double gap, const spdl_hj_resample_box_item* it, int W, int H, int out_w,
              int out_h, int* reduces) {
  BoxGeo g;
  const int rc = resolve_box(it, W, H, out_w, out_h, filter, gap, &g);
  *reduces = !rc && (g.fx > 1 || g.fy > 1);
  return rc;
}

int place_box_into(void* cache, int filter, double gap, const spdl_hj_resample_box_item* it, int W,
                   int H, int out_w, int out_h, std::vector<int32_t>& tables, ResamplePool& pool,
                   ResampleDesc* d, ReduceDesc* red, int* bands, int* chunks) {
  BoxGeo b;
  int rc = resolve_box(it, W, H, out_w, out_h, filter, gap, &b);
  if (rc) return rc;
  if (!red && (b.fx > 1 || b.fy > 1)) return SPDL_HJ_ERR_INVALID_ARG;  // (the planner probed)
  AxisCache& ac = *static_cast<AxisCache*>(cache);
  Placed pl;
  pl.H = ac.get(b.cw, b.box[0], b.box[2], b.rw, filter, &rc);
  if (!pl.H) return rc;
  pl.V = ac.get(b.ch, b.box[1], b.box[3], b.rh, filter, &rc);
  if (!pl.V) return rc;
  // (the tables' xmin is absolute in the picture: the kernels' box origin is 0)
  const Geo g{0, 0, b.cw, b.ch, b.rw, b.rh, b.ox, b.oy};
  rc = red ? tile_reduce(*pl.H, *pl.V, g, out_w, out_h, &pl.d, &pl.bands, &pl.chunks, ac.channels)
           : tile(*pl.H, *pl.V, g, out_w, out_h, &pl.d, &pl.bands, &pl.chunks, ac.channels);
  if (rc) return rc;
  if (red) {
    *red = ReduceDesc{b.q[0], b.q[1], b.q[2] - b.q[0], b.q[3] - b.q[1], b.fx, b.fy, b.cw, b.ch, {}, {}};
    for (int k = 0; k < 4; k++) {
      red->amend[k] = (uint32_t)b.div[k] / 2;
      red->mult[k] = b.mult[k];
    }
  }
  return pool_tables(pl, tables, pool, d, bands, chunks);
}

int resolve_item(const spdl_hj_resample_items_item* it, int W, int H, int filter, double gap,
                 ItemGeo* g) {
  *g = ItemGeo{};
  if (it->orient < 0 || it->orient > 7) return SPDL_HJ_ERR_INVALID_ARG;
  if (it->orient & 4) std::swap(W, H);  // (the displayed frame: everything below is in it)
  if (it->flip < 0 || it->flip > 3 || it->out_w < 1 || it->out_w > 65535 || it->out_h < 1 ||
      it->out_h > 65535)
    return SPDL_HJ_ERR_INVALID_ARG;
  spdl_hj_resample_box_item b{it->x0, it->y0, it->x1, it->y1, it->rw, it->rh, it->ox, it->oy};
  if (!it->clamp) return resolve_box(&b, W, H, it->out_w, it->out_h, filter, gap, &g->b);
  int fw = W, fh = H;
  if (b.x0 != 0 || b.y0 != 0 || b.x1 != 0 || b.y1 != 0) {
    const double v[4] = {b.x0, b.y0, b.x1, b.y1};
    for (double x : v)
      if (!(x >= -65536.0 && x <= 65536.0) || x != floor(x)) return SPDL_HJ_ERR_INVALID_ARG;
    if (b.x0 < 0 || b.y0 < 0 || b.x1 <= b.x0 || b.y1 <= b.y0 || b.x1 > W || b.y1 > H)
      return SPDL_HJ_ERR_BAD_GEOMETRY;
    g->bx = (int)b.x0;
    g->by = (int)b.y0;
    fw = (int)b.x1 - g->bx;
    fh = (int)b.y1 - g->by;
    b.x0 = b.y0 = b.x1 = b.y1 = 0;
  }
  return resolve_box(&b, fw, fh, it->out_w, it->out_h, filter, gap, &g->b);
}

int probe_item(int filter, double gap, const spdl_hj_resample_items_item* it, int W, int H,
               int* reduces) {
  ItemGeo g;
  const int rc = resolve_item(it, W, H, filter, gap, &g);
  *reduces = !rc && (g.b.fx > 1 || g.b.fy > 1);
  return rc;
}

int place_item_into(void* cache, int filter, double gap, const spdl_hj_resample_items_item* it,
                    int W, int H, bool sum, std::vector<int32_t>& tables, ResamplePool& pool,
                    ItemDesc* rec, int* bands, int* chunks) {
  ItemGeo ig;
  int rc = resolve_item(it, W, H, filter, gap, &ig);
  if (rc) return rc;
  const BoxGeo& b = ig.b;
  if (!sum && (b.fx > 1 || b.fy > 1)) return SPDL_HJ_ERR_INVALID_ARG;  // (the planner probed)
  AxisCache& ac = *static_cast<AxisCache*>(cache);
  Placed pl;
  pl.H = ac.get(b.cw, b.box[0], b.box[2], b.rw, filter, &rc);
  if (!pl.H) return rc;
  pl.V = ac.get(b.ch, b.box[1], b.box[3], b.rh, filter, &rc);
  if (!pl.V) return rc;
  // (with sums the cells count from rr.qx / qy, which hold the clamped box's
  // origin; without, the producer reads the frame at the box's origin + xmin)
  const Geo g{sum ? 0 : ig.bx, sum ? 0 : ig.by, b.cw, b.ch, b.rw, b.rh, b.ox, b.oy};
  if (sum)
    rc = tile_reduce(*pl.H, *pl.V, g, it->out_w, it->out_h, &pl.d, &pl.bands, &pl.chunks,
                     ac.channels);
  else if (it->orient)
    rc = tile_oriented(*pl.H, *pl.V, g, it->out_w, it->out_h, &pl.d, &pl.bands, &pl.chunks);
  else
    rc = tile(*pl.H, *pl.V, g, it->out_w, it->out_h, &pl.d, &pl.bands, &pl.chunks, ac.channels);
  if (rc) return rc;
  rec->orient = it->orient;
  rec->dw = it->orient & 4 ? H : W;
  rec->dh = it->orient & 4 ? W : H;
  rec->rr = ReduceDesc{ig.bx + b.q[0], ig.by + b.q[1], b.q[2] - b.q[0], b.q[3] - b.q[1],
                       b.fx,           b.fy,           b.cw,            b.ch,
                       {},             {}};
  for (int k = 0; k < 4; k++) {
    rec->rr.amend[k] = (uint32_t)b.div[k] / 2;
    rec->rr.mult[k] = b.mult[k];
  }
  rec->ow = it->out_w;
  rec->oh = it->out_h;
  return pool_tables(pl, tables, pool, &rec->rd, bands, chunks);
}

}  // namespace rs
}  // namespace hj
