// The library's memory and transfer layer: the device work-buffer pool and the page-locked block pool (size_class_pool.h), the idle
// work sets, the host worker threads, the huge-page host blocks, and the staged, sum-checked host <-> device copies.
#include "glx_internal.h"
#include "size_class_pool.h"
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <thread>
#include <sys/mman.h>
#include <unistd.h>

// ---- device work-buffer pool and page-locked block pool ---------------------------------------------------------------------------
// hipMalloc / hipFree cost 0.1-1 ms each (hipFree synchronises the device): a kNN build makes thirty of them for 4 ms of
// kernels.  Work buffers of the one-shot entry points (knn.hip, assemble.hip) come from size-class free lists instead;
// at most 1 GiB stays cached per process, blocks above 256 MiB go straight back to the runtime.
// Small page-locked blocks (the stop-value mirrors of a sweep object, the projector's image): hipHostMalloc 0.03-0.13 ms, hipHostFree
// 0.25 ms each -- two of each per model on a fresh graph.  Power-of-two classes, blocks up to 4 MiB kept, at most 32 MiB idle.
// The contract of both: callers release a block only after the stream that used it has been synchronised.
// (never destroyed: they outlive the HIP runtime's teardown; a failed allocation leaves no error behind for a later hipGetLastError)
static SizeClassPool& device_pool() {
  static SizeClassPool* p = new SizeClassPool(
      DEVICE_POOL_RULE, [](void** out, size_t bytes) { const hipError_t e = hipMalloc(out, bytes); if (e) (void)hipGetLastError(); return (int)e; },
      [](void* q) { hipFree(q); }, (int)hipErrorOutOfMemory);
  return *p;
}
static SizeClassPool& pinned_pool() {
  static SizeClassPool* p = new SizeClassPool(
      PINNED_POOL_RULE, [](void** out, size_t bytes) { const hipError_t e = hipHostMalloc(out, bytes, hipHostMallocDefault); if (e) (void)hipGetLastError(); return (int)e; },
      [](void* q) { hipHostFree(q); }, (int)hipErrorOutOfMemory);
  return *p;
}
// glx_pool_set_enabled(0): every block straight from / back to the runtime and no idle work sets -- the ablation switch of the
// randomised soak (a result that changes with it names a buffer handed on while still in use) and of tests/test_gpu_switches.py
static std::atomic<bool> g_pool_enabled{true};
// glx_pool_set_poison(b): every block handed out is first filled with the byte b (-1: off, the default) -- a debugging aid: a kernel
// that reads a work buffer before anything wrote it then computes from the pattern instead of from whatever an earlier call left there
static std::atomic<int> g_pool_poison{-1};

int glx_pool_alloc(void** out, size_t bytes) {
  int dev = 0;
  GLX_HIP(hipGetDevice(&dev));
  GLX_HIP((hipError_t)device_pool().alloc(dev, bytes, out));
  const int poison = g_pool_poison.load();
  if (poison >= 0 && *out) {
    GLX_HIP(hipDeviceSynchronize());
    GLX_HIP(hipMemset(*out, poison, device_pool().cls(bytes)));
    GLX_HIP(hipDeviceSynchronize());
  }
  return GLX_OK;
}
void glx_pool_free(void* p) { device_pool().free(p); }

int glx_pinned_alloc(void** out, size_t bytes) {
  GLX_HIP((hipError_t)pinned_pool().alloc(0, bytes, out));
  return GLX_OK;
}
void glx_pinned_free(void* p) { pinned_pool().free(p); }

namespace {
// per device, objects nobody holds (never destroyed: HIP objects must not be torn down after the runtime at exit)
template <typename T> struct IdleByDevice { std::mutex mu; std::map<int, std::vector<T*>> idle; };
IdleByDevice<glx_work>* const g_idle_work = new IdleByDevice<glx_work>();
void work_destroy(glx_work* w) {
  for (int i = 0; i < 4; ++i)
    if (w->ev[i]) hipEventDestroy(w->ev[i]);
  if (w->ev_side) hipEventDestroy(w->ev_side);
  if (w->side) hipStreamDestroy(w->side);
  if (w->stream) hipStreamDestroy(w->stream);
  if (w->stage) hipHostFree(w->stage);
  delete w;
}
}  // namespace

// the page-locked block *p of *have bytes, replaced by one of `want` bytes when smaller (contents not kept)
static int pinned_grow(void** p, size_t* have, size_t want) {
  if (*have >= want) return GLX_OK;
  if (*p) hipHostFree(*p);
  *p = nullptr;
  *have = 0;
  GLX_HIP(hipHostMalloc(p, want, hipHostMallocDefault));
  *have = want;
  return GLX_OK;
}

int glx_work_stage(glx_work* w, size_t bytes, void** out) {
  size_t want = (size_t)1 << 16;
  while (want < bytes) want <<= 1;
  GLX_UP(pinned_grow(&w->stage, &w->stage_bytes, want));
  *out = w->stage;
  return GLX_OK;
}

int glx_work_acquire(int device, glx_work** out) {
  auto& wc = *g_idle_work;
  {
    std::lock_guard<std::mutex> lk(wc.mu);
    auto& v = wc.idle[device];
    if (!v.empty()) {
      *out = v.back();
      v.pop_back();
      return GLX_OK;
    }
  }
  glx_work* w = new glx_work;
  w->device = device;
  hipError_t e = hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&w->side, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&w->ev_side, hipEventDisableTiming);
  for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipEventCreate(&w->ev[i]);
  if (e != hipSuccess) {
    glx_set_error("glx_work_acquire: %s", hipGetErrorString(e));
    work_destroy(w);
    return GLX_EHIP;
  }
  // The FIRST work set of a device starts the copy engines: the runtime creates a copy queue the first time an engine is picked
  // (7.7 ms each, measured with rocprofv3 --hip-trace: the first host-to-device copy, the first device-to-host copy, and one more
  // device-to-host copy when a second engine is drawn), which otherwise lands in the middle of the first graph builds.  Two
  // transfers per direction in flight at once, through page-locked memory, draw them now -- next to the 150 ms of runtime start-up.
  {
    static std::mutex mu;
    static std::vector<int> warmed;
    std::lock_guard<std::mutex> lk(mu);
    if (std::find(warmed.begin(), warmed.end(), device) == warmed.end()) {
      warmed.push_back(device);
      // (two more streams than the set owns: a solver object's own stream is the third or fourth the process creates, and its first
      // device-to-host copy drew one more engine -- 10 ms inside the first fit of a process, scripts/first_fit_probe.py)
      const size_t half = (size_t)1 << 20;
      void *d = nullptr, *h = nullptr;
      hipStream_t extra[2] = {nullptr, nullptr};
      for (int q = 0; q < 2; ++q)
        if (hipStreamCreateWithFlags(&extra[q], hipStreamNonBlocking) != hipSuccess) extra[q] = nullptr;
      if (hipMalloc(&d, 8 * half) == hipSuccess && hipHostMalloc(&h, 8 * half, hipHostMallocDefault) == hipSuccess) {
        hipStream_t sts[4] = {w->stream, w->side, extra[0], extra[1]};
        for (int rep = 0; rep < 2; ++rep)
          for (int q = 0; q < 4; ++q) {
            if (!sts[q]) continue;
            hipMemcpyAsync((char*)h + (2 * q) * half, (char*)d + (2 * q) * half, half, hipMemcpyDeviceToHost, sts[q]);
            hipMemcpyAsync((char*)d + (2 * q + 1) * half, (char*)h + (2 * q + 1) * half, half, hipMemcpyHostToDevice, sts[q]);
          }
        for (int q = 0; q < 4; ++q)
          if (sts[q]) hipStreamSynchronize(sts[q]);
      }
      for (int q = 0; q < 2; ++q)
        if (extra[q]) hipStreamDestroy(extra[q]);
      if (h) hipHostFree(h);
      if (d) hipFree(d);
      (void)hipGetLastError();
    }
  }
  *out = w;
  return GLX_OK;
}

// the holder has synchronised the stream (nothing of its work is left on it)
void glx_work_release(glx_work* w) {
  if (!w) return;
  auto& wc = *g_idle_work;
  {
    std::lock_guard<std::mutex> lk(wc.mu);
    auto& v = wc.idle[w->device];
    if (g_pool_enabled.load() && v.size() < 8) {
      v.push_back(w);
      return;
    }
  }
  work_destroy(w);
}

extern "C" int glx_pool_set_enabled(int enabled) {
  g_pool_enabled = enabled != 0;
  device_pool().set_enabled(enabled != 0);       // (disabled: what is idle now goes back to the runtime; blocks in use follow when released)
  if (!enabled) {
    std::unique_lock<std::mutex> lk(g_idle_work->mu);
    std::vector<glx_work*> sets;
    for (auto& kv : g_idle_work->idle) { sets.insert(sets.end(), kv.second.begin(), kv.second.end()); kv.second.clear(); }
    lk.unlock();
    for (glx_work* w : sets) work_destroy(w);
  }
  pinned_pool().set_enabled(enabled != 0);
  return GLX_OK;
}

extern "C" int glx_pool_set_poison(int byte) {
  g_pool_poison = byte < 0 ? -1 : (byte & 0xff);
  return GLX_OK;
}

// A few host worker threads that stay around (spawning eight std::threads costs ~0.3 ms: as much as hashing 25 MB).  run() executes
// fn(t) for t in [0, nt) on the workers and the caller, and returns when all are done.  One job at a time; a process forked from one
// that had workers starts its own (threads do not survive fork).
namespace {
struct HostPool {
  std::mutex mu, job_mu;
  std::condition_variable cv, done;
  std::vector<std::thread>* workers = nullptr;
  const std::function<void(int)>* fn = nullptr;
  int next = 0, total = 0, pending = 0;
  unsigned long gen = 0;
  pid_t pid = 0;
  void loop() {
    unsigned long seen = 0;
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv.wait(lk, [&] { return gen != seen; });
      seen = gen;
      while (next < total) {
        const int t = next++;
        lk.unlock();
        (*fn)(t);
        lk.lock();
        if (--pending == 0) done.notify_all();
      }
    }
  }
  void run(int nt, const std::function<void(int)>& f) {
    std::lock_guard<std::mutex> one(job_mu);
    if (nt <= 1) { for (int t = 0; t < nt; ++t) f(t); return; }
    {
      std::unique_lock<std::mutex> lk(mu);
      if (pid != getpid()) {            // first use, or a forked child: the parent's workers are not here (their handles are left alone)
        workers = new std::vector<std::thread>();
        pid = getpid();
      }
      const int want = std::min(7, nt - 1);
      while ((int)workers->size() < want) workers->emplace_back([this] { loop(); });
      fn = &f;
      next = 0;
      total = nt;
      pending = nt;
      ++gen;
    }
    cv.notify_all();
    std::unique_lock<std::mutex> lk(mu);
    while (next < total) {               // the caller works too
      const int t = next++;
      lk.unlock();
      f(t);
      lk.lock();
      --pending;
    }
    done.wait(lk, [&] { return pending == 0; });
  }
};
HostPool* const g_host_pool = new HostPool();   // never destroyed: its workers may outlive static destruction
}  // namespace

void glx_host_parallel(int nt, const std::function<void(int)>& fn) { g_host_pool->run(nt, fn); }

// Page-locked, device-visible host memory for result arrays.  From 1 MiB on: anonymous memory aligned to 2 MiB with transparent huge
// pages asked for, faulted in by a few threads, then registered with the runtime -- 1.1 ms for 19 MB (one huge-page fault zeroes
// 2 MiB at memory speed) where hipHostMalloc takes 2.7-3.2 ms (1.7 ms with any explicit flag; scripts/probes/pin_probe.hip): fresh
// result arrays were most of what the first graph build of a new size paid.  Smaller blocks: hipHostMalloc.
namespace {
struct HostBlocks {
  std::mutex mu;
  std::map<void*, std::pair<void*, size_t>> mapped;      // user pointer -> (mmap base, mmap length)
};
HostBlocks& host_blocks() {
  static HostBlocks* h = new HostBlocks();
  return *h;
}
}  // namespace

extern "C" int glx_host_alloc(size_t bytes, void** out) {
  GLX_CHECK(out, GLX_EINVAL, "glx_host_alloc: null output");
  *out = nullptr;
  const size_t HUGE = (size_t)2 << 20;
  if (bytes >= ((size_t)1 << 20)) {
    const size_t len = (bytes + HUGE - 1) / HUGE * HUGE;
    void* base = mmap(nullptr, len + HUGE, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (base != MAP_FAILED) {
      char* a = (char*)(((uintptr_t)base + HUGE - 1) & ~(uintptr_t)(HUGE - 1));
      madvise(a, len, MADV_HUGEPAGE);
      const int64_t npages = (int64_t)(len / HUGE);
      const int nt = (int)std::min<int64_t>(4, npages);
      g_host_pool->run(nt, [&](int t) {               // one store per 4 KiB: faults the range in whether or not huge pages are granted
        for (size_t off = (size_t)(npages * t / nt) * HUGE, end = (size_t)(npages * (t + 1) / nt) * HUGE; off < end; off += 4096)
          *(volatile char*)(a + off) = 0;
      });
      if (hipHostRegister(a, len, hipHostRegisterDefault) == hipSuccess) {
        std::lock_guard<std::mutex> lk(host_blocks().mu);
        host_blocks().mapped[a] = {base, len + HUGE};
        *out = a;
        return GLX_OK;
      }
      (void)hipGetLastError();
      munmap(base, len + HUGE);
    }
  }
  GLX_HIP(hipHostMalloc(out, bytes > 0 ? bytes : 1, hipHostMallocPortable | hipHostMallocMapped));
  return GLX_OK;
}

extern "C" int glx_host_free(void* p) {
  if (!p) return GLX_OK;
  std::pair<void*, size_t> m{nullptr, 0};
  {
    std::lock_guard<std::mutex> lk(host_blocks().mu);
    auto it = host_blocks().mapped.find(p);
    if (it != host_blocks().mapped.end()) {
      m = it->second;
      host_blocks().mapped.erase(it);
    }
  }
  if (m.first) {
    hipError_t e = hipHostUnregister(p);
    munmap(m.first, m.second);
    GLX_HIP(e);
    return GLX_OK;
  }
  GLX_HIP(hipHostFree(p));
  return GLX_OK;
}

// copy `len` bytes (a multiple of 8 when a sum is asked for) and add the 64-bit words up (wrapping)
static unsigned long long copy_and_sum(char* dst, const char* src, size_t len, bool want_sum) {
  if (!want_sum) { memcpy(dst, src, len); return 0ull; }
  const unsigned long long* s8 = (const unsigned long long*)src;
  unsigned long long* d8 = (unsigned long long*)dst;
  unsigned long long a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  const size_t nw = len / 8;
  size_t i = 0;
  for (; i + 4 <= nw; i += 4) {
    const unsigned long long v0 = s8[i], v1 = s8[i + 1], v2 = s8[i + 2], v3 = s8[i + 3];
    d8[i] = v0; d8[i + 1] = v1; d8[i + 2] = v2; d8[i + 3] = v3;
    a0 += v0; a1 += v1; a2 += v2; a3 += v3;
  }
  for (; i < nw; ++i) { d8[i] = s8[i]; a0 += s8[i]; }
  return a0 + a1 + a2 + a3;
}
// ... on `nt` (at most 8) host threads, each a part of whole 64-byte lines
static unsigned long long copy_and_sum_parallel(char* dst, const char* src, size_t len, bool want_sum, int nt) {
  if (nt <= 1) return copy_and_sum(dst, src, len, want_sum);
  unsigned long long part[8] = {0, 0, 0, 0, 0, 0, 0, 0}, total = 0;
  g_host_pool->run(nt, [&](int t) {
    const size_t a = len * (size_t)t / nt / 64 * 64, b = t + 1 == nt ? len : len * (size_t)(t + 1) / nt / 64 * 64;
    part[t] = copy_and_sum(dst + a, src + a, b - a, want_sum);
  });
  for (int t = 0; t < 8; ++t) total += part[t];
  return total;
}

namespace {
// The staging area of a thread that uploads or downloads, one per device.  HIP objects are never destroyed (they must not outlive the
// runtime's teardown): when its thread exits, a thread's Uploaders go to a list of spares that the next new thread takes from, so that
// the page-locked memory they hold is bounded by the threads that transfer at the same time, not by those that ever did.
struct Uploader {
  void* stage = nullptr;          // page-locked: two halves that take turns
  size_t bytes = 0;
  hipEvent_t ev[2] = {nullptr, nullptr};
  unsigned long long* sum = nullptr;        // device word of the check
  unsigned long long* sum_host = nullptr;   // its page-locked mirror
};
IdleByDevice<Uploader>* const g_spares = new IdleByDevice<Uploader>();     // the Uploaders of threads that have exited
struct ThreadUploaders {
  std::map<int, Uploader*> per_device;
  ~ThreadUploaders() {          // (every call ended with its copies complete: nothing in flight uses these any more)
    std::lock_guard<std::mutex> lk(g_spares->mu);
    for (auto& kv : per_device) g_spares->idle[kv.first].push_back(kv.second);
  }
};
Uploader* my_uploader() {
  static thread_local ThreadUploaders mine;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
  Uploader*& u = mine.per_device[dev];
  if (!u) {
    std::lock_guard<std::mutex> lk(g_spares->mu);
    auto& v = g_spares->idle[dev];
    if (v.empty()) v.push_back(new Uploader());
    u = v.back();
    v.pop_back();
  }
  return u;
}
}  // namespace

// the staging area: two halves of 256 KiB .. 16 MiB, the smallest that holds `need` bytes (or the largest), grown when too small
static int stage_reserve(Uploader* w, size_t need) {
  const size_t HALF_MAX = (size_t)16 << 20;
  size_t half = (size_t)1 << 18;
  while (half < need && half < HALF_MAX) half <<= 1;
  return pinned_grow(&w->stage, &w->bytes, 2 * half);     // (nothing reads the old area any more: every call ends behind its last copy)
}

// the staged copy: returns the wrapping sum of the 64-bit words (a zero-padded last word for a length that is no multiple of 8) when asked
static int upload_staged(Uploader* w, void* dst, const void* src, size_t bytes, hipStream_t st, unsigned long long* sum_out, size_t stage_shift) {
  if (sum_out) *sum_out = 0ull;
  if (bytes == 0) return GLX_OK;
  GLX_UP(stage_reserve(w, bytes + stage_shift));
  const size_t h = w->bytes / 2;
  GLX_CHECK(stage_shift % 64 == 0 && stage_shift < h / 2, GLX_EINVAL, "glx_upload: bad staging shift");
  // bytes of a half in use per piece (a multiple of 64: whole words); big uploads go in pieces of 4 MB so that the host threads fill one half
  // while the copy engine empties the other
  const size_t room = std::min<size_t>((h - stage_shift) / 64 * 64, bytes > ((size_t)6 << 20) ? ((size_t)4 << 20) : (size_t)-1);
  for (int i = 0; i < 2; ++i)
    if (!w->ev[i]) GLX_HIP(hipEventCreateWithFlags(&w->ev[i], hipEventDisableTiming));
  int turn = 0;
  unsigned long long total = 0;
  for (size_t off = 0; off < bytes; off += room, turn ^= 1) {
    const size_t len = std::min(room, bytes - off);
    const size_t whole = len / 8 * 8;
    char* stage = (char*)w->stage + (size_t)turn * h + stage_shift;
    // the copy of THIS call that last read this half.  Never an event of an earlier call: the runtime's hipEventSynchronize looks at the
    // stream the event was last recorded on, and that stream may be gone by now (a work set's stream destroyed with its set: the pool
    // switched off) -- "operation not permitted on an event last recorded in a capturing stream" out of freed memory, in the first
    // upload after such a stream's address was reused (round 6, tests/test_gpu_switches.py).  Every call therefore ends with its
    // copies complete (the checked path waits for its sum, the unchecked one for the stream) and starts with both halves free.
    if (off >= 2 * room) GLX_HIP(hipEventSynchronize(w->ev[turn]));
    total += copy_and_sum_parallel(stage, (const char*)src + off, whole, sum_out != nullptr, (int)std::min<size_t>(8, std::max<size_t>(1, whole >> 19)));
    if (len > whole) {                                   // the last bytes of the upload: a word padded with zeros for the sum
      unsigned long long tail = 0;
      memcpy(&tail, (const char*)src + off + whole, len - whole);
      memcpy(stage + whole, (const char*)src + off + whole, len - whole);
      total += tail;
    }
    GLX_HIP(hipMemcpyAsync((char*)dst + off, stage, len, hipMemcpyHostToDevice, st));
    GLX_HIP(hipEventRecord(w->ev[turn], st));
  }
  if (sum_out) *sum_out = total;
  else GLX_HIP(hipStreamSynchronize(st));             // (the checked caller synchronises behind its sum kernel)
  return GLX_OK;
}

// (one atomic per workgroup and at most UPLOAD_SUM_BLOCKS of them: 8192 wavefronts adding to ONE address took 100 us for 11 MB, the
// additions themselves 5)
#define UPLOAD_SUM_BLOCKS 512
__global__ __launch_bounds__(256) void upload_sum_kernel(const unsigned long long* __restrict__ p, int64_t nwords, int tail_bytes,
                                                         unsigned long long* __restrict__ out) {
  unsigned long long a = 0;
  const int64_t step = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * step < nwords; i += 4 * step) {          // four loads in flight per thread
    const unsigned long long v0 = p[i], v1 = p[i + step], v2 = p[i + 2 * step], v3 = p[i + 3 * step];
    a += v0 + v1 + v2 + v3;
  }
  for (; i < nwords; i += step) a += p[i];
  if (tail_bytes && blockIdx.x == 0 && threadIdx.x == 0) {
    const unsigned char* t = (const unsigned char*)(p + nwords);
    unsigned long long v = 0;
    for (int q = 0; q < tail_bytes; ++q) v |= (unsigned long long)t[q] << (8 * q);
    a += v;
  }
  for (int off = 32; off >= 1; off >>= 1) a += (unsigned long long)__shfl_xor((long long)a, off);
  __shared__ unsigned long long sh[4];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long t = sh[0] + sh[1] + sh[2] + sh[3];
    if (t) atomicAdd(out, t);
  }
}

// enqueue on `st` the device's wrapping sum of the 64-bit words of `src_dev` (a zero-padded last word for a length that is no multiple of
// 8): it is in *w->sum_host once `st` has reached this point
static int enqueue_device_sum(Uploader* w, const void* src_dev, size_t bytes, hipStream_t st) {
  if (!w->sum) GLX_HIP(hipMalloc((void**)&w->sum, 64));
  if (!w->sum_host) GLX_HIP(hipHostMalloc((void**)&w->sum_host, 64, hipHostMallocDefault));
  GLX_HIP(hipMemsetAsync(w->sum, 0, 8, st));
  const int64_t nw = (int64_t)(bytes / 8);
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(UPLOAD_SUM_BLOCKS, (nw + 1023) / 1024));
  hipLaunchKernelGGL(upload_sum_kernel, dim3(grid), dim3(256), 0, st, (const unsigned long long*)src_dev, nw, (int)(bytes % 8), w->sum);
  GLX_HIP(hipGetLastError());
  GLX_HIP(hipMemcpyAsync(w->sum_host, w->sum, 8, hipMemcpyDeviceToHost, st));
  return GLX_OK;
}

int glx_compare_readback(const void* host, const void* dev, size_t bytes, GlxReadbackDiff* diff, unsigned long long* back) {
  *diff = GlxReadbackDiff();
  unsigned long long* own = nullptr;
  if (!back) {
    GLX_HIP(hipHostMalloc((void**)&own, std::max<size_t>(bytes, 64), hipHostMallocDefault));
    back = own;
  }
  const hipError_t e = hipMemcpy(back, dev, bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) {
    const unsigned long long* s8 = (const unsigned long long*)host;
    for (size_t i = 0; i < bytes / 8; ++i)
      if (back[i] != s8[i]) { if (!diff->bad) diff->first = i; diff->last = i; ++diff->bad; diff->zeros += back[i] == 0; }
  }
  if (own) hipHostFree(own);
  GLX_HIP(e);
  return GLX_OK;
}

static std::atomic<unsigned long long> g_upload_stats[4];       // uploads checked, sums that differed, uploads repeated successfully, given up
extern "C" int glx_upload_stats(unsigned long long out[4]) {
  GLX_CHECK(out, GLX_EINVAL, "glx_upload_stats: null output");
  for (int q = 0; q < 4; ++q) out[q] = g_upload_stats[q].load();
  return GLX_OK;
}
static std::atomic<int> g_upload_mode{0};      // glx_upload_set_mode: 0 staged + checked (default), 1 staged, 2 hipMemcpyAsync from the caller's memory (rounds 1-5)
extern "C" int glx_upload_set_mode(int mode) {
  GLX_CHECK(mode >= 0 && mode <= 2, GLX_EINVAL, "glx_upload_set_mode: 0 (staged + checked), 1 (staged) or 2 (direct)");
  g_upload_mode = mode;
  return GLX_OK;
}

int glx_upload(void* dst, const void* src, size_t bytes, hipStream_t st, const char* what) {
  if (bytes == 0) return GLX_OK;
  GLX_CHECK(dst && src, GLX_EINVAL, "%s: null pointer in an upload of %zu bytes", what, bytes);
  const int mode = g_upload_mode.load();
  if (bytes < ((size_t)128 << 10) || mode == 2) {
    GLX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
    return GLX_OK;
  }
  Uploader* w = my_uploader();
  const bool aligned = ((uintptr_t)dst % 8 == 0) && ((uintptr_t)src % 8 == 0);
  // (word sums need 8-byte aligned ends; the staging alone is what keeps the transfer off the runtime's pageable path)
  if (!aligned || mode == 1) return upload_staged(w, dst, src, bytes, st, nullptr, 0);
  ++g_upload_stats[0];
  for (int attempt = 0; attempt < 4; ++attempt) {
    unsigned long long want = 0;
    // (a repeat goes through another part of the staging area)
    GLX_UP(upload_staged(w, dst, src, bytes, st, &want, (size_t)attempt * 12288));
    GLX_UP(enqueue_device_sum(w, dst, bytes, st));
    GLX_HIP(hipStreamSynchronize(st));
    if (*w->sum_host == want) {
      if (attempt) ++g_upload_stats[2];
      return GLX_OK;
    }
    ++g_upload_stats[1];
    // what went wrong where: the staging area against the caller's array (single-piece uploads: the area still holds the whole array), and
    // the device copy, read back THROUGH PAGE-LOCKED MEMORY (a read-back into pageable memory can show the same holes), against it
    size_t stage_bad = 0;
    const unsigned long long* s8 = (const unsigned long long*)src;
    if (bytes <= ((size_t)6 << 20) && bytes + (size_t)attempt * 12288 <= w->bytes / 2) {      // (one piece: the area still holds the whole array)
      const unsigned long long* g8 = (const unsigned long long*)((const char*)w->stage + (size_t)attempt * 12288);
      for (size_t i = 0; i < bytes / 8; ++i) stage_bad += g8[i] != s8[i];
    }
    GlxReadbackDiff dev;
    (void)glx_compare_readback(src, dst, bytes, &dev);
    (void)hipGetLastError();
    fprintf(stderr, "[glx] upload check (%s, pid %d, attempt %d): %zu bytes arrived with sum %016llx instead of %016llx -- the staging area differs from "
                    "the caller's array in %zu words, the device copy in %zu (bytes %zu .. %zu of the upload, %zu of them zero); repeating the upload\n",
            what, (int)getpid(), attempt, bytes, *w->sum_host, want, stage_bad, dev.bad, dev.first * 8, dev.last * 8 + 7, dev.zeros);
  }
  ++g_upload_stats[3];
  glx_set_error("%s: the upload of %zu bytes did not arrive intact in four attempts", what, bytes);
  return GLX_EHIP;
}

int glx_download(void* dst, const void* src, size_t bytes, hipStream_t st, const char* what) {
  if (bytes == 0) return GLX_OK;
  GLX_CHECK(dst && src, GLX_EINVAL, "%s: null pointer in a download of %zu bytes", what, bytes);
  const int mode = g_upload_mode.load();
  bool direct = bytes < ((size_t)128 << 10) || mode == 2;
  if (!direct) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, dst) == hipSuccess && (at.type == hipMemoryTypeHost || at.type == hipMemoryTypeManaged)) direct = true;   // page-locked
    (void)hipGetLastError();
  }
  if (direct) {
    GLX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
    return GLX_OK;
  }
  Uploader* w = my_uploader();
  const bool check = mode == 0 && ((uintptr_t)dst % 8 == 0) && ((uintptr_t)src % 8 == 0) && bytes % 8 == 0;
  if (check) ++g_upload_stats[0];
  for (int attempt = 0; attempt < 4; ++attempt) {
    const size_t shift = (size_t)attempt * 12288;
    // the staging area is the uploads' own: one half of it is used here, piece by piece.  (No upload of this thread still reads the area --
    // every one ended with its copies complete -- and no event of an earlier call is waited for here either: the stream it was recorded on
    // may be gone, and the runtime's hipEventSynchronize looks at that stream; see upload_staged)
    GLX_UP(stage_reserve(w, bytes + shift));
    const size_t room = (w->bytes / 2 - shift) / 64 * 64;
    unsigned long long got = 0;
    if (check) GLX_UP(enqueue_device_sum(w, src, bytes, st));
    char* stage = (char*)w->stage + shift;
    for (size_t off = 0; off < bytes; off += room) {
      const size_t len = std::min(room, bytes - off);
      GLX_HIP(hipMemcpyAsync(stage, (const char*)src + off, len, hipMemcpyDeviceToHost, st));
      GLX_HIP(hipStreamSynchronize(st));
      got += copy_and_sum_parallel((char*)dst + off, stage, len, check, (int)std::min<size_t>(4, std::max<size_t>(1, len >> 20)));
    }
    if (!check) return GLX_OK;
    const unsigned long long want = *w->sum_host;
    if (got == want) {
      if (attempt) ++g_upload_stats[2];
      return GLX_OK;
    }
    ++g_upload_stats[1];
    fprintf(stderr, "[glx] download check (%s, pid %d, attempt %d): %zu bytes came down with sum %016llx instead of %016llx; repeating the download\n", what,
            (int)getpid(), attempt, bytes, got, want);
  }
  ++g_upload_stats[3];
  glx_set_error("%s: the download of %zu bytes did not arrive intact in four attempts", what, bytes);
  return GLX_EHIP;
}

int glx_download_sync(void* dst, const void* src, size_t bytes, const char* what) {
  GLX_UP(glx_download(dst, src, bytes, nullptr, what));
  GLX_HIP(hipStreamSynchronize(nullptr));
  return GLX_OK;
}

int glx_upload_sync(void* dst, const void* src, size_t bytes, const char* what) {
  GLX_UP(glx_upload(dst, src, bytes, nullptr, what));
  GLX_HIP(hipStreamSynchronize(nullptr));
  return GLX_OK;
}
