// hj_sws_tile.h -- the tile and LDS geometry of the output stage, defined once
// for both sides of the launch: the host tiler (hj_sws.cpp PlanCache) sizes a
// launch's dynamic LDS and its grids from these functions, and sws_kernel,
// yuv_planes_kernel and hscale_kernel take their windows, pointers and tile
// counts from the same ones.  Integers only, no HIP types: builds with -DHJ_HD=.
#pragma once
#include "hj_common.h"

namespace hj {

inline HJ_HD int tile_min(int a, int b) { return a < b ? a : b; }
inline HJ_HD int tile_max(int a, int b) { return a > b ? a : b; }
inline HJ_HD int tile_div_up(int a, int b) { return (a + b - 1) / b; }
inline HJ_HD int tile_align16(int v) { return (v + 15) & ~15; }

// The tile at (xo0, yo0) of an ow x oh output box that holds the sw x sh
// scaled content at (dx, dy): its end in the box (xo1, yo1) and its content in
// scaled coordinates, columns [xs0, xs1) and rows [ys0, ys1); `content`: the
// tile holds any (else it is all pad).
struct SwsWindow {
  int yo1, xo1, ys0, ys1, xs0, xs1;
  bool content;
};
inline HJ_HD SwsWindow sws_window(int yo0, int xo0, int rb, int col_chunk, int dx, int dy, int ow,
                                  int oh, int sw, int sh) {
  const int yo1 = tile_min(yo0 + rb, oh), xo1 = tile_min(xo0 + col_chunk, ow);
  const int ys0 = tile_max(yo0 - dy, 0), ys1 = tile_min(yo1 - dy, sh);
  const int xs0 = tile_max(xo0 - dx, 0), xs1 = tile_min(xo1 - dx, sw);
  return {yo1, xo1, ys0, ys1, xs0, xs1, ys0 < ys1 && xs0 < xs1};
}

// Output flips (spdl_hj_set_flips; bit 0 horizontal, bit 1 vertical): the
// flip is the last node of the chain, so it changes no pixel, only where the
// tile and each pixel in it land.  The tile [xo0, xo1) x [yo0, yo1) of the
// unflipped W x H box is the tile at (mx0, my0), of the same size, of the
// flipped one: mx0 = W - xo1, my0 = H - yo1 for a set bit.  Output pixel
// (xo, yo) of the unflipped box has the tile coordinate (tx(xo), ty(yo)) there
// -- (v ^ mask) + base: mask 0 and base -xo0 without the flip, mask -1 and base
// xo1 with it, which is xo1 - 1 - xo -- and the box coordinate mx0 + tx(xo).
// The inverse, from a tile coordinate back to the unflipped box, is sx / sy.
struct TileFlip {
  int mx0, my0;  // the mirrored tile's origin in the box
  int xm, xb, ym, yb;
  HJ_HD int tx(int xo) const { return (xo ^ xm) + xb; }
  HJ_HD int ty(int yo) const { return (yo ^ ym) + yb; }
  HJ_HD int sx(int k) const { return (k - xb) ^ xm; }
  HJ_HD int sy(int r) const { return (r - yb) ^ ym; }
};
inline HJ_HD TileFlip tile_flip(int xo0, int xo1, int yo0, int yo1, int W, int H, int flip) {
  const bool fh = flip & 1, fv = flip & 2;
  return {fh ? W - xo1 : xo0, fv ? H - yo1 : yo0, fh ? -1 : 0, fh ? xo1 : -xo0,
          fv ? -1 : 0,        fv ? yo1 : -yo0};
}

// Output orientation (spdl_hj_set_orients; bits 0 and 1 as the flips, bit 2 a
// transpose ahead of them): with C the chain's ow x oh box, A(x, y) = C(y, x)
// for a transposed descriptor (else A = C), and the final box is A mirrored.
// The final box is fw x fh (oh x ow when transposed), its row pitch fw.  The
// tile [xo0, xo1) x [yo0, yo1) of the chain's box lands as the lw x lh tile at
// (mx0, my0) of the final box -- th x tw when transposed -- and chain pixel
// (xo, yo) at (lx, ly) of the landed tile; cx / cy lead from a landed
// coordinate back to the chain's box.  It is tile_flip over the final box's
// axes: the final x axis is the chain's y axis when transposed.
struct TileOrient {
  TileFlip f;  // over (u, v): the chain coordinates that run along final x and y
  bool t;
  int fw, fh;  // the final box
  int lw, lh;  // the landed tile
  HJ_HD int mx0() const { return f.mx0; }
  HJ_HD int my0() const { return f.my0; }
  HJ_HD int lx(int xo, int yo) const { return f.tx(t ? yo : xo); }
  HJ_HD int ly(int xo, int yo) const { return f.ty(t ? xo : yo); }
  HJ_HD int cx(int kx, int ky) const { return t ? f.sy(ky) : f.sx(kx); }
  HJ_HD int cy(int kx, int ky) const { return t ? f.sx(kx) : f.sy(ky); }
};
inline HJ_HD TileOrient tile_orient(int xo0, int xo1, int yo0, int yo1, int ow, int oh, int code) {
  const bool t = code & 4;
  const int fw = t ? oh : ow, fh = t ? ow : oh;
  const TileFlip f = t ? tile_flip(yo0, yo1, xo0, xo1, fw, fh, code & 3)
                       : tile_flip(xo0, xo1, yo0, yo1, fw, fh, code & 3);
  return {f, t, fw, fh, t ? yo1 - yo0 : xo1 - xo0, t ? xo1 - xo0 : yo1 - yo0};
}

// The chroma columns under the luma columns [xs0, xs1) (xs0 < xs1): one per
// column with SWS_FULL_CHR_H_INT, else one per pixel pair.
struct SwsChromaCols {
  int cx0, ncc;
};
inline HJ_HD SwsChromaCols sws_chroma_cols(int xs0, int xs1, bool full) {
  const int cx0 = full ? xs0 : xs0 >> 1;
  return {cx0, (full ? xs1 - 1 : (xs1 - 1) >> 1) + 1 - cx0};
}

// sws_kernel's dynamic LDS for a tile of ncl luma and ncc chroma columns whose
// vertical filters reach lrows / crows source rows: the int16 columns (lst /
// cst apart) of luma at 0, of the two chroma planes (none: gray; gbr: the G and
// B planes through the luma filters) at hu and hv; `tile`, the u8 output tile
// of rb x col_chunk pixels; `vt`, the band's vertical tables, rb rows of vrw
// words: {mode, first luma row, first chroma row, 0}, the luma tap pairs, the
// chroma ones.  hu, hv in int16 units; tile, vt, end in bytes.
struct SwsLds {
  int lst, cst, hu, hv, tile, vt, vrw, end;
};
inline HJ_HD SwsLds sws_lds_layout(int ncl, int ncc, int lrows, int crows, bool gbr, bool gray,
                                   int rb, int col_chunk, int vl_size, int vc_size) {
  const int lst = sws_col_stride(lrows), cst = sws_col_stride(crows);
  const int side = gbr ? ncl * lst : gray ? 0 : ncc * cst;  // hu's and hv's columns
  const int hu = ncl * lst, hv = hu + side, tile = tile_align16(2 * (hv + side));
  const int vt = tile + tile_align16(rb * col_chunk * 3), vrw = 4 + (vl_size + vc_size) / 2;
  return {lst, cst, hu, hv, tile, vt, vrw, vt + rb * vrw * 4};
}

// yuv_planes_kernel's dynamic LDS for a tile of rb rows x chunk columns with
// ncols content columns of `rows` source rows: the int16 columns at 0, then
// the u8 tile, whose runs (rows, `pitch` bytes apart) sit at their
// destination's offset within 16 bytes.  `bound`: bytes that hold any such
// tile -- a run starts up to 15 bytes in and pitch >= chunk + 15.
struct PlanarLds {
  int cst, tile, pitch, bound;
};
inline HJ_HD PlanarLds planar_lds_layout(int ncols, int rows, int rb, int chunk) {
  const int cst = sws_col_stride(rows), tile = tile_align16(2 * ncols * cst);
  const int pitch = (chunk + 30) & ~15;
  return {cst, tile, pitch, tile + rb * pitch + 16};
}

// hscale_kernel's tiles of one image (SwsDesc::pre): kHsRows rows of one plane
// per workgroup, tl luma tiles, then tc for each of the two other planes (chroma
// through the chroma filters; gbr: G and B through the luma ones; gray: none).
struct HsTiles {
  int tl, tc, wgs;
};
inline HJ_HD HsTiles hs_tiles(const SwsDesc& s) {
  const int tl = tile_div_up(s.pre_rl, kHsRows);
  const int tc = s.gbr ? tl : s.gray ? 0 : tile_div_up(s.pre_rc, kHsRows);
  return {tl, tc, tl + 2 * tc};
}
// Plane c (0..2) of an image's hbuf region: row-major int16, `rows` x `w`,
// `off` elements in; hs_hbuf_size: the region, through its last plane.
struct HsPlane {
  int64_t off;
  int rows, w;
};
inline HJ_HD HsPlane hs_plane(const SwsDesc& s, int c) {
  const bool lumaf = c == 0 || s.gbr;  // luma filters
  const int64_t side = s.gbr ? (int64_t)s.pre_rl * s.sw : (int64_t)s.pre_rc * s.chr_w;
  return {c == 0 ? 0 : (int64_t)s.pre_rl * s.sw + (c - 1) * side, lumaf ? s.pre_rl : s.pre_rc,
          lumaf ? s.sw : s.chr_w};
}
inline HJ_HD int64_t hs_hbuf_size(const SwsDesc& s) {
  const HsPlane last = hs_plane(s, hs_tiles(s).tc ? 2 : 0);
  return last.off + (int64_t)last.rows * last.w;
}

// yuv_planes_kernel's tiles of one image: bands of rb rows x chunks of
// col_chunk columns of every plane, the luma plane's (ow x oh) first, then
// U's and V's (cw x ch, the ceil-shifted box).
struct PlanarTiles {
  int cw, ch, lchunks, cchunks, ltiles, ctiles, total;  // (chunks: per band of a plane)
};
inline HJ_HD PlanarTiles planar_tiles(int ow, int oh, int hsub, int vsub, int rb, int col_chunk,
                                      bool gray) {
  const int cw = (ow + (1 << hsub) - 1) >> hsub, ch = (oh + (1 << vsub) - 1) >> vsub;
  const int lchunks = tile_div_up(ow, col_chunk), cchunks = tile_div_up(cw, col_chunk);
  const int ltiles = tile_div_up(oh, rb) * lchunks, ctiles = tile_div_up(ch, rb) * cchunks;
  return {cw, ch, lchunks, cchunks, ltiles, ctiles, ltiles + (gray ? 0 : 2 * ctiles)};
}

}  // namespace hj
