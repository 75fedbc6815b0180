// Size-class free lists in front of an allocator: the device work-buffer pool and the page-locked block pool of memory.hip.  No HIP
// header: tests/test_host_pool.py builds it on the host against stand-ins for the allocator.
// A request is served with a block of cls(bytes) bytes: an idle one of the same key (device) and class, else a fresh one.  A block handed
// back stays idle while the pool is enabled, the block is at most block_max bytes and the idle ones stay within cap; anything else goes
// straight back to the allocator.  Callers hand a block back only when nothing in flight uses it any more.
#pragma once
#include <cstddef>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

struct SizeClassRule {
  size_t granule_above;   // classes: powers of two from 4 KiB up to this (0: all the way), then multiples of `granule`
  size_t granule;
  size_t block_max;       // larger blocks are never kept
  size_t cap;             // idle bytes kept at most
  size_t cls(size_t bytes) const {
    size_t c = 4096;
    while (c < bytes) c <<= 1;
    if (granule_above && c > granule_above) c = (bytes + granule - 1) / granule * granule;
    return c;
  }
};
static const SizeClassRule DEVICE_POOL_RULE = {(size_t)64 << 20, (size_t)16 << 20, (size_t)256 << 20, (size_t)1 << 30};
static const SizeClassRule PINNED_POOL_RULE = {0, 0, (size_t)4 << 20, (size_t)32 << 20};

class SizeClassPool {
 public:
  using AllocFn = int (*)(void** out, size_t bytes);   // 0, or the allocator's error code
  using FreeFn = void (*)(void* p);
  SizeClassPool(const SizeClassRule& rule, AllocFn alloc, FreeFn release, int oom_code)
      : rule_(rule), alloc_(alloc), free_(release), oom_(oom_code) {}

  size_t cls(size_t bytes) const { return rule_.cls(bytes > 0 ? bytes : 1); }

  // 0, or the allocator's error code.  Out of memory: the idle blocks go back to the allocator and it is asked once more.
  int alloc(int key, size_t bytes, void** out) {
    const std::pair<int, size_t> k{key, cls(bytes)};
    std::unique_lock<std::mutex> lk(mu_);
    auto it = idle_.find(k);
    if (it != idle_.end()) {
      *out = it->second;
      idle_.erase(it);
      cached_ -= k.second;
      live_[*out] = k;
      return 0;
    }
    lk.unlock();
    *out = nullptr;
    int e = alloc_(out, k.second);
    if (e == oom_) { drain(); e = alloc_(out, k.second); }
    if (e) return e;
    lk.lock();
    live_[*out] = k;
    return 0;
  }

  // a block of this pool, or any block of the allocator (it goes straight back)
  void free(void* p) {
    if (!p) return;
    std::unique_lock<std::mutex> lk(mu_);
    auto it = live_.find(p);
    if (it != live_.end()) {
      const std::pair<int, size_t> k = it->second;
      live_.erase(it);
      if (enabled_ && k.second <= rule_.block_max && cached_ + k.second <= rule_.cap) {
        idle_.insert({k, p});
        cached_ += k.second;
        return;
      }
    }
    lk.unlock();
    free_(p);
  }

  void drain() {   // every idle block back to the allocator
    std::vector<void*> blocks;
    std::unique_lock<std::mutex> lk(mu_);
    for (auto& kv : idle_) blocks.push_back(kv.second);
    idle_.clear();
    cached_ = 0;
    lk.unlock();
    for (void* p : blocks) free_(p);
  }

  void set_enabled(bool on) {   // off: what is idle goes back now, every block handed back follows
    { std::lock_guard<std::mutex> lk(mu_); enabled_ = on; }
    if (!on) drain();
  }

  size_t cached() { std::lock_guard<std::mutex> lk(mu_); return cached_; }

 private:
  const SizeClassRule rule_;
  const AllocFn alloc_;
  const FreeFn free_;
  const int oom_;
  std::mutex mu_;
  std::multimap<std::pair<int, size_t>, void*> idle_;   // (key, class bytes) -> block
  std::map<void*, std::pair<int, size_t>> live_;        // block -> (key, class bytes)
  size_t cached_ = 0;
  bool enabled_ = true;
};
