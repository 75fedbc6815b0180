// Host build of the grow-loop schedule of INCRES clustering (csrc/incres_plan.h) for tests/test_incres_host.py: the chunked loop with its
// per-slot flags and label buffers, plain loops standing in for the kernels of incres.hip -- the product adds a row's entries in stored
// order, the census tests the k real columns for a zero and takes the row-wise first maximum.  The chunk length is an argument, so that a
// stop on a chunk's last slot, on its first slot and in slot 0 are all exercised.  Compile with -ffp-contract=off.
#include "incres_plan.h"
#include <cstddef>
#include <limits>
#include <vector>

namespace {
struct Host {
  int64_t n;
  int k;
  std::vector<int32_t> ptr, col;
  std::vector<double> val;
  std::vector<double> buf[2];
  std::vector<int32_t> flags, labels;      // [INCRES_MAX_CHUNK + 1], [INCRES_MAX_CHUNK + 1][n]
  IncresPlan plan;
};

struct HostOps {
  Host* h;
  int cur = 0;
  int64_t chunks = 0, enqueued = 0;
  int begin_chunk(int, int) {
    for (auto& f : h->flags) f = 0;
    return 0;
  }
  int census(int slot) {
    const std::vector<double>& F = h->buf[cur];
    int zero = 0;
    for (int64_t i = h->n - 1; i >= 0; --i) {      // (backwards: the order inside a census must not matter)
      int arg = 0;
      for (int c = 0; c < h->k; ++c) {
        const double v = F[i * h->k + c];
        if (v == 0.0) zero = 1;
        if (v > F[i * h->k + arg]) arg = c;
      }
      h->labels[(int64_t)slot * h->n + i] = arg;
    }
    h->flags[slot] = zero;
    return 0;
  }
  int sweep() {
    const std::vector<double>& in = h->buf[cur];
    std::vector<double>& out = h->buf[cur ^ 1];
    for (int64_t i = 0; i < h->n; ++i)
      for (int c = 0; c < h->k; ++c) {
        double s = 0.0;
        for (int64_t e = h->ptr[i]; e < h->ptr[i + 1]; ++e) s = s + h->val[e] * in[(int64_t)h->col[e] * h->k + c];
        out[i * h->k + c] = s;
      }
    cur ^= 1;
    return 0;
  }
  int read_flags(int, int len, const int32_t** flags) {
    ++chunks;
    enqueued += len;
    *flags = h->flags.data();
    return 0;
  }
};
}  // namespace

extern "C" void incres_host_constants(int64_t* out) {
  out[0] = INCRES_MAX_COLS;
  out[1] = INCRES_MAX_CHUNK;
  out[2] = INCRES_FIRST_CHUNK;
  out[3] = INCRES_MARGIN;
  out[4] = INCRES_NEXT_CHUNK;
}

extern "C" int incres_host_chunk_len2(int margin, int next, int64_t prev, int64_t done, int64_t max_grow, int64_t nth) {
  IncresPlan p;
  p.margin = margin;
  p.next = next;
  p.prev = prev;
  return p.chunk_len(done, max_grow, nth);
}

extern "C" int incres_host_chunk_len(int forced, int64_t prev, int64_t done, int64_t max_grow, int64_t nth) {
  IncresPlan p;
  p.forced = forced;
  p.prev = prev;
  return p.chunk_len(done, max_grow, nth);
}

extern "C" void* incres_host_create(int64_t n, const int32_t* ptr, const int32_t* col, const double* val, int k) {
  Host* h = new Host;
  h->n = n;
  h->k = k;
  h->ptr.assign(ptr, ptr + n + 1);
  h->col.assign(col, col + ptr[n]);
  h->val.assign(val, val + ptr[n]);
  const double poison = std::numeric_limits<double>::quiet_NaN();
  h->buf[0].assign((size_t)n * k, poison);
  h->buf[1].assign((size_t)n * k, poison);
  h->flags.assign(INCRES_MAX_CHUNK + 1, -1);
  h->labels.assign((size_t)(INCRES_MAX_CHUNK + 1) * n, -1);
  return h;
}

extern "C" void incres_host_destroy(void* p) { delete (Host*)p; }

// seeds (k, m); info: the slot, the chunks of this loop, the sweeps enqueued in it
extern "C" int incres_host_step(void* p, const int32_t* seeds, int64_t m, int64_t max_grow, int chunk, int32_t* labels_out, int64_t* sweeps_out,
                                double* info) {
  Host* h = (Host*)p;
  for (auto& v : h->buf[0]) v = 0.0;
  for (int r = 0; r < h->k; ++r)
    for (int64_t q = 0; q < m; ++q) h->buf[0][(int64_t)seeds[r * m + q] * h->k + r] = 1.0;
  HostOps ops{h};
  h->plan.forced = chunk;
  int slot = -1;
  const int rc = incres_grow(h->plan, max_grow, ops, sweeps_out, &slot);
  info[0] = slot;
  info[1] = (double)ops.chunks;
  info[2] = (double)ops.enqueued;
  if (rc) return rc;
  for (int64_t i = 0; i < h->n; ++i) labels_out[i] = h->labels[(int64_t)slot * h->n + i];
  return 0;
}
