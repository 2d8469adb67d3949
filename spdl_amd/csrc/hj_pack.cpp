// hj_pack.cpp -- see hj_pack.h.
#include "hj_pack.h"

#include <sched.h>
#include <unistd.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace hj {

CopyPool::CopyPool(int n) {
  for (int i = 0; i < n; i++) th_.emplace_back([this, i] { loop(i + 1); });
}

CopyPool::~CopyPool() {
  {
    std::lock_guard<std::mutex> g(m_);
    stop_ = true;
  }
  cv_.notify_all();
  for (auto& t : th_) t.join();
}

void CopyPool::run(const std::function<void(int, int)>& fn) {
  const int np = workers();
  {
    std::lock_guard<std::mutex> g(m_);
    fn_ = &fn;
    pending_ = np - 1;
    gen_++;
  }
  cv_.notify_all();
  fn(0, np);
  std::unique_lock<std::mutex> lk(m_);
  done_cv_.wait(lk, [this] { return pending_ == 0; });
  fn_ = nullptr;
}

void CopyPool::loop(int part) {
  uint64_t seen = 0;
  for (;;) {
    const std::function<void(int, int)>* fn;
    {
      std::unique_lock<std::mutex> lk(m_);
      cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
      if (stop_) return;
      seen = gen_;
      fn = fn_;
    }
    (*fn)(part, workers());
    std::lock_guard<std::mutex> g(m_);
    if (--pending_ == 0) done_cv_.notify_all();
  }
}

int copy_workers() {
  if (const char* e = getenv("SPDL_HJ_COPY_THREADS")) {
    const int v = atoi(e);
    return v < 1 ? 0 : (v > 16 ? 15 : v - 1);
  }
  int cores = (int)sysconf(_SC_NPROCESSORS_ONLN);
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof(set), &set) == 0) cores = CPU_COUNT(&set);
  if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[32] = {0};
    long long per = 0;
    if (fscanf(f, "%31s %lld", q, &per) == 2 && strcmp(q, "max") != 0 && per > 0) {
      const long long c = atoll(q) / per;
      if (c >= 1 && c < cores) cores = (int)c;
    }
    fclose(f);
  }
  int ranks = 1;
  if (const char* e = getenv("LOCAL_WORLD_SIZE")) ranks = atoi(e) > 0 ? atoi(e) : 1;
  const int share = cores / ranks;
  return share <= 1 ? 0 : (share - 1 > 7 ? 7 : share - 1);
}

void parallel_pack(CopyPool* pool, uint8_t* base, const std::vector<CopyItem>& items) {
  int64_t total = 0;
  for (const CopyItem& it : items) total += it.padded;
  auto body = [&](int part, int np) {
    // byte range [lo, hi) of the concatenated padded items
    const int64_t lo = total * part / np, hi = total * (part + 1) / np;
    int64_t acc = 0;
    for (const CopyItem& it : items) {
      const int64_t a = acc, b = acc + it.padded;
      acc = b;
      if (b <= lo) continue;
      if (a >= hi) break;
      const int64_t s = lo > a ? lo - a : 0, e = (hi < b ? hi : b) - a;
      const int64_t cs = s, ce = e < it.len ? e : it.len;
      if (ce > cs) memcpy(base + it.dst_off + cs, it.src + cs, (size_t)(ce - cs));
      const int64_t zs = s > it.len ? s : it.len;
      if (e > zs) memset(base + it.dst_off + zs, 0, (size_t)(e - zs));
    }
  };
  if (!pool || pool->workers() < 2 || total < (4 << 20)) body(0, 1);
  else pool->run(body);
}

bool parallel_pread(CopyPool* pool, int fd, int64_t file_off, uint8_t* base, size_t len) {
  std::atomic<int> bad{0};
  auto body = [&](int part, int np) {
    // 64 KiB-aligned split so the page-cache copies stay sequential per thread
    const size_t unit = 1 << 16, nu = (len + unit - 1) / unit;
    size_t lo = nu * part / np * unit, hi = nu * (part + 1) / np * unit;
    if (hi > len) hi = len;
    while (lo < hi) {
      const ssize_t r = pread(fd, base + lo, hi - lo, (off_t)(file_off + (int64_t)lo));
      if (r <= 0) {
        bad = 1;
        return;
      }
      lo += (size_t)r;
    }
  };
  if (!pool || pool->workers() < 2 || len < (4u << 20)) body(0, 1);
  else pool->run(body);
  return !bad;
}

}  // namespace hj
