// hj_pack.h -- the host threads that fill pinned staging: the copier pool,
// the split copy of a batch's files and the split read of a file range.
// Host only: no HIP include, so tests/native/pack_sweep.cpp runs the pool
// alone under ASan / UBSan and under TSan.
#pragma once

#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace hj {

// Persistent host workers for the pinned-staging copies.  A 256-image batch
// is ~28 MB; one core copies that at ~6-10 GB/s, slower than the GPU decodes
// it, so the copy into pinned memory is split over a few threads.
class CopyPool {
 public:
  explicit CopyPool(int n);  // n threads beside the caller
  ~CopyPool();
  int workers() const { return (int)th_.size() + 1; }
  // fn(part, nparts) runs for part = 0..nparts-1 (part 0 on the caller).
  void run(const std::function<void(int, int)>& fn);

 private:
  void loop(int part);
  std::vector<std::thread> th_;
  std::mutex m_;
  std::condition_variable cv_, done_cv_;
  const std::function<void(int, int)>* fn_ = nullptr;
  int pending_ = 0;
  uint64_t gen_ = 0;
  bool stop_ = false;
};

// Copier threads per context: the host cores this process may use (affinity,
// capped by a cgroup v2 CPU quota) shared among the ranks of this node
// (LOCAL_WORLD_SIZE), at most 8 with the caller; SPDL_HJ_COPY_THREADS
// overrides.  8 ranks x 8 copiers would oversubscribe a 16-core share.
int copy_workers();

// Copy n items of (dst_off, src, len) into `base`, zero-filling each item's
// tail [len, padded) -- split by bytes over the pool when the total is large.
struct CopyItem {
  int64_t dst_off;
  const uint8_t* src;
  int64_t len, padded;
};
void parallel_pack(CopyPool* pool, uint8_t* base, const std::vector<CopyItem>& items);

// pread of [file_off, file_off + len) of fd into base, split over the pool
// when large (no pool: one thread).  False: a read failed or hit end of file.
bool parallel_pread(CopyPool* pool, int fd, int64_t file_off, uint8_t* base, size_t len);

}  // namespace hj
