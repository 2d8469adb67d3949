// items_sweep.cpp -- stand-alone, self-checking sweep of the planner's item
// path (hj::place_items, spdl_amd/csrc/hj_layout.h) for a sanitizer build on the
// CPU, built and run by tests/test_resample_items.py with hj_layout.cpp,
// hj_sws.cpp and hj_resample.cpp.  Random item lists over a few frame sizes:
// every workgroup of the map lands in exactly one item's tile range, one
// image's items are adjacent, the tables lie inside the pool, the LDS inside
// the budget and every item inside the buffer.  Prints one line per failed
// expectation and a count; exit status 1 when any failed.
#include "../../spdl_amd/csrc/hj_resample.h"

#include <stdio.h>

#include <random>

namespace {

using namespace hj;

int failures = 0, checks = 0;

#define EXPECT(cond, ...)                   \
  do {                                      \
    checks++;                               \
    if (!(cond) && failures++ < 40) {       \
      printf("FAIL %s: ", #cond);           \
      printf(__VA_ARGS__);                  \
      printf("\n");                         \
    }                                       \
  } while (0)

void sweep(rs::AxisCache& cache, std::mt19937& rng, int filter, double gap) {
  static const int sides[] = {1, 8, 33, 101, 227, 640};
  auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
  const int n = pick(1, 5);
  std::vector<int> fw(n), fh(n);
  for (int i = 0; i < n; i++) {
    fw[i] = sides[pick(0, 5)];
    fh[i] = sides[pick(0, 5)];
  }
  std::vector<spdl_hj_resample_items_item> items((size_t)pick(0, 12));
  int64_t end = 0;
  for (auto& it : items) {
    it = spdl_hj_resample_items_item{};
    it.image = pick(0, n - 1);
    it.clamp = pick(0, 1);
    const int W = fw[it.image], H = fh[it.image];
    if (pick(0, 2) && W > 2 && H > 2) {  // a box: integral when clamped, else fractional
      it.x0 = pick(0, W / 2), it.y0 = pick(0, H / 2);
      it.x1 = pick((int)it.x0 + 1, W), it.y1 = pick((int)it.y0 + 1, H);
      if (!it.clamp) it.x0 += 0.25, it.y1 -= 0.5;
    }
    it.out_w = pick(1, 90), it.out_h = pick(1, 90);
    it.ox = pick(0, 3), it.oy = pick(0, 3);
    it.rw = it.out_w + it.ox + pick(0, 2), it.rh = it.out_h + it.oy;
    it.flip = pick(0, 3);
    it.offset = end;
    end += (int64_t)it.out_w * it.out_h * 3 + pick(0, 7);
  }
  ResampleRequest r{filter, 0, 0, nullptr, 0, &cache, nullptr};
  r.gap = gap;
  r.list = items.data();
  r.n_items = (int64_t)items.size();
  r.place_item = &rs::place_item_into;
  r.probe_item = &rs::probe_item;
  Layout L;
  ResamplePool pool;
  std::vector<int32_t> st;
  const char* what = place_items(r, fw, fh, 1, end, L, pool, st);
  EXPECT(!what, "%s", what ? what : "");
  if (what) return;
  size_t placed = 0;
  for (int32_t s : st) {
    EXPECT(s == SPDL_HJ_OK || s == SPDL_HJ_ERR_BAD_GEOMETRY, "status %d", s);
    placed += s == SPDL_HJ_OK;
  }
  EXPECT(L.items.size() == placed && L.by_items, "%zu records for %zu placed items", L.items.size(), placed);
  EXPECT(L.resample_lds <= rs::kLdsBudget, "LDS %d", L.resample_lds);
  const size_t status_wgs = (size_t)(n + 255) / 256;
  size_t wg = 0;
  int last_image = -1;
  for (size_t k = 0; k < L.items.size(); k++) {
    const rs::ItemDesc& it = L.items[k];
    const rs::ResampleDesc& d = it.rd;
    const int bands = (it.oh + d.th - 1) / d.th, chunks = (it.ow + d.tw - 1) / d.tw;
    EXPECT(it.image >= last_image && it.image < n, "image order: %d after %d", it.image, last_image);
    last_image = it.image;
    EXPECT((size_t)it.wg0 == wg && it.chunks == chunks, "item %zu: first workgroup %d, expected %zu", k, it.wg0, wg);
    for (int t = 0; t < bands * chunks; t++, wg++)
      EXPECT(wg < L.item_map.size() && L.item_map[wg] == k, "workgroup %zu is not item %zu's", wg, k);
    const int64_t tsz = (int64_t)L.tables.size();
    EXPECT(d.hx >= 0 && d.hk + (int64_t)(d.ox + it.ow) * d.kh <= tsz && d.vx >= 0 &&
               d.vk + (int64_t)(d.oy + it.oh) * d.kv <= tsz,
           "item %zu: tables outside the pool of %lld", k, (long long)tsz);
    const int words = L.items_sum ? rs::reduce_lds_words(d) : rs::lds_layout(d).words;
    EXPECT(words * 4 <= L.resample_lds, "item %zu: %d LDS words above the launch's", k, words);
    const int64_t off = (int64_t)((uint64_t)it.off_hi << 32 | it.off_lo);
    EXPECT(off >= 0 && off + (int64_t)it.ow * it.oh * 3 <= end, "item %zu past the buffer", k);
    EXPECT(it.rr.qx >= 0 && it.rr.qy >= 0 && it.rr.qx + it.rr.qw <= fw[it.image] &&
               it.rr.qy + it.rr.qh <= fh[it.image] && it.rr.fx >= 1 && it.rr.fy >= 1 &&
               (L.items_sum || (it.rr.fx == 1 && it.rr.fy == 1)),
           "item %zu: source rectangle outside its frame", k);
  }
  EXPECT(L.item_map.size() == wg + status_wgs, "%zu map entries for %zu tiles", L.item_map.size(), wg);
  for (; wg < L.item_map.size(); wg++) EXPECT(L.item_map[wg] == rs::kItemNone, "status workgroup %zu", wg);
}

}  // namespace

int main() {
  rs::AxisCache cache;
  std::mt19937 rng(24);
  for (int round = 0; round < 400; round++)
    for (int filter = 0; filter < 3; filter++)
      for (double gap : {0.0, 1.0, 2.0}) sweep(cache, rng, filter, gap);
  printf("%d checks, %d failed expectations\n", checks, failures);
  return failures != 0;
}
