// Host driver of graphlearning_amd/csrc/size_class_pool.h for tests/test_host_pool.py: the pool in front of counting stand-ins for the
// allocator (malloc / free of a token block; the size asked for is recorded).  Built with -fsanitize=thread.
//   classes SIZE...   one line per size: "SIZE <device class> <bytes the device allocator was asked for> <pinned class> <pinned asked>"
//   caps | disabled | oom | stress   the checks of that name; exit status 0 when they hold
#include "size_class_pool.h"
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

static const int OOM = 2, OTHER_ERROR = 3;
static std::atomic<long> g_allocs{0}, g_frees{0};
static std::atomic<size_t> g_asked{0};
static std::atomic<int> g_fail{0};   // the next allocation fails with this code (0: none)

static int stand_in_alloc(void** out, size_t bytes) {
  const int f = g_fail.exchange(0);
  if (f) return f;
  g_asked = bytes;
  *out = malloc(16);
  ++g_allocs;
  return 0;
}
static void stand_in_free(void* p) {
  free(p);
  ++g_frees;
}

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "check failed at line %d: %s\n", __LINE__, #cond); \
      return 1;                                                      \
    }                                                                \
  } while (0)

static int classes(int argc, char** argv) {
  for (int i = 2; i < argc; ++i) {
    const size_t bytes = strtoull(argv[i], nullptr, 10);
    size_t cls[2], asked[2];
    const SizeClassRule* rules[2] = {&DEVICE_POOL_RULE, &PINNED_POOL_RULE};
    for (int r = 0; r < 2; ++r) {
      SizeClassPool pool(*rules[r], stand_in_alloc, stand_in_free, OOM);
      void* p = nullptr;
      g_asked = 0;
      CHECK(pool.alloc(0, bytes, &p) == 0 && p);
      asked[r] = g_asked;
      cls[r] = pool.cls(bytes > 0 ? bytes : 1);
      pool.free(p);
      pool.drain();
    }
    printf("%zu %zu %zu %zu %zu\n", bytes, cls[0], asked[0], cls[1], asked[1]);
  }
  return 0;
}

// free `blocks` blocks of `bytes` each; the idle bytes never exceed the rule's cap; returns how many reached the allocator
static long free_many(SizeClassPool& pool, const SizeClassRule& rule, size_t bytes, int blocks, int* bad) {
  std::vector<void*> ps(blocks);
  for (auto& p : ps)
    if (pool.alloc(0, bytes, &p)) ++*bad;
  const long f0 = g_frees;
  for (void* p : ps) {
    pool.free(p);
    if (pool.cached() > rule.cap) ++*bad;
  }
  return g_frees - f0;
}

static int caps() {
  int bad = 0;
  {
    SizeClassPool pool(DEVICE_POOL_RULE, stand_in_alloc, stand_in_free, OOM);
    CHECK(free_many(pool, DEVICE_POOL_RULE, (size_t)64 << 20, 20, &bad) == 4);        // 16 of 64 MiB fill the 1 GiB
    CHECK(pool.cached() == ((size_t)1 << 30));
    pool.drain();
    CHECK(free_many(pool, DEVICE_POOL_RULE, (size_t)256 << 20, 1, &bad) == 0);        // the largest block that is kept
    CHECK(free_many(pool, DEVICE_POOL_RULE, ((size_t)256 << 20) + 1, 1, &bad) == 1);  // above the block cap: straight back
    pool.drain();
    CHECK(pool.cached() == 0);
  }
  {
    SizeClassPool pool(PINNED_POOL_RULE, stand_in_alloc, stand_in_free, OOM);
    CHECK(free_many(pool, PINNED_POOL_RULE, (size_t)4 << 20, 9, &bad) == 1);          // 8 of 4 MiB fill the 32 MiB
    CHECK(pool.cached() == ((size_t)32 << 20));
    pool.drain();
    CHECK(free_many(pool, PINNED_POOL_RULE, ((size_t)4 << 20) + 1, 1, &bad) == 1);
    CHECK(free_many(pool, PINNED_POOL_RULE, 1000, 3, &bad) == 0);
    const long a0 = g_allocs;
    void* p = nullptr;
    CHECK(pool.alloc(0, 4000, &p) == 0 && g_allocs == a0);                            // same class: an idle block, no allocation
    pool.free(p);
    pool.drain();
  }
  CHECK(bad == 0);
  CHECK(g_allocs == g_frees);
  return 0;
}

static int disabled() {
  SizeClassPool pool(DEVICE_POOL_RULE, stand_in_alloc, stand_in_free, OOM);
  int bad = 0;
  CHECK(free_many(pool, DEVICE_POOL_RULE, 5000, 4, &bad) == 0);
  const long f0 = g_frees;
  pool.set_enabled(false);                                       // what is idle goes at once
  CHECK(g_frees - f0 == 4 && pool.cached() == 0);
  for (size_t bytes : {(size_t)1, (size_t)5000, (size_t)1 << 20, (size_t)100 << 20}) {
    const long f1 = g_frees;
    void* p = nullptr;
    CHECK(pool.alloc(0, bytes, &p) == 0);
    pool.free(p);
    CHECK(g_frees - f1 == 1 && pool.cached() == 0);              // every free reaches the allocator
  }
  pool.set_enabled(true);
  CHECK(free_many(pool, DEVICE_POOL_RULE, 5000, 2, &bad) == 0);
  pool.drain();
  CHECK(bad == 0 && g_allocs == g_frees);
  return 0;
}

static int oom() {
  SizeClassPool pool(DEVICE_POOL_RULE, stand_in_alloc, stand_in_free, OOM);
  int bad = 0;
  CHECK(free_many(pool, DEVICE_POOL_RULE, 5000, 3, &bad) == 0);
  const long f0 = g_frees;
  void* p = nullptr;
  g_fail = OOM;                                                   // out of memory once: the idle blocks go back, the retry succeeds
  CHECK(pool.alloc(0, 1 << 20, &p) == 0 && p);
  CHECK(g_frees - f0 == 3 && pool.cached() == 0);
  pool.free(p);
  g_fail = OTHER_ERROR;                                           // any other error: returned as it is, nothing drained
  void* q = nullptr;
  CHECK(pool.alloc(0, 3 << 20, &q) == OTHER_ERROR);
  CHECK(pool.cached() == ((size_t)1 << 20));
  pool.drain();
  CHECK(bad == 0 && g_allocs == g_frees);
  return 0;
}

static int stress() {
  SizeClassPool pool(DEVICE_POOL_RULE, stand_in_alloc, stand_in_free, OOM);
  std::atomic<bool> stop{false};
  std::atomic<int> bad{0};
  std::vector<std::thread> th;
  for (int t = 0; t < 8; ++t)
    th.emplace_back([&, t] {
      std::mt19937_64 rng(t);
      void* held[4] = {nullptr, nullptr, nullptr, nullptr};
      for (int i = 0; i < 100000; ++i) {
        void*& slot = held[i & 3];
        if (slot) pool.free(slot);
        slot = nullptr;
        if (pool.alloc(t & 1, (size_t)1 << (rng() % 28), &slot) || !slot) ++bad;
      }
      for (void* p : held) pool.free(p);
    });
  std::thread toggler([&] {
    for (bool on = false; !stop; on = !on) pool.set_enabled(on);
  });
  for (auto& t : th) t.join();
  stop = true;
  toggler.join();
  pool.set_enabled(true);
  pool.drain();
  CHECK(bad == 0);
  CHECK(pool.cached() == 0);
  CHECK(g_allocs == g_frees);
  printf("%ld allocations, %ld frees\n", (long)g_allocs, (long)g_frees);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "classes")) return classes(argc, argv);
  if (!strcmp(argv[1], "caps")) return caps();
  if (!strcmp(argv[1], "disabled")) return disabled();
  if (!strcmp(argv[1], "oom")) return oom();
  if (!strcmp(argv[1], "stress")) return stress();
  return 2;
}
