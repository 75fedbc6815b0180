// INCRES clustering (Bresson et al., incremental reseeding; reference graphlearning/clustering.py:325-371), the device half of one
// outer iteration: plant the seeds, grow `while np.min(F) == 0: F = P*F`, harvest the row-wise argmax.  The contract is DESIGN.md 4.15.
//
// The product is the sweep engine's, as it is (glx_launch_spmm on device records: no bias, no stop column, one sweep per launch): a
// row's entries are added in stored order with separate multiply and add roundings, which is scipy's csr_matvecs bit for bit.  P is
// handed over with the entry order scipy's `W*D` left it in (reversed rows) and kept that way.  New here: the plant kernels, the
// census-and-harvest kernel that runs behind every sweep, and the driver around incres_plan.h.
#include "glx_internal.h"
#include "incres_plan.h"
#include <string.h>
#include <algorithm>
#include <vector>

// the calling thread's plan override (glx_incres_set_options; chunk = 0: the library decides)
static thread_local glx_incres_options g_incres_opt = {0, 0, 0};
extern "C" int glx_incres_set_options(const glx_incres_options* opt) {
  if (!opt) { g_incres_opt = glx_incres_options{0, 0, 0}; return GLX_OK; }
  GLX_CHECK(opt->chunk >= 0 && opt->chunk <= INCRES_MAX_CHUNK && opt->margin >= 0 && opt->margin <= INCRES_MAX_CHUNK && opt->next >= 0 &&
                opt->next <= INCRES_MAX_CHUNK,
            GLX_EINVAL, "glx_incres_set_options: chunk %d, margin %d or next %d outside [0, %d]", opt->chunk, opt->margin, opt->next, INCRES_MAX_CHUNK);
  g_incres_opt = *opt;
  return GLX_OK;
}

struct glx_incres {
  glx_graph* P = nullptr;
  int64_t n = 0;
  int k = 0, device = 0;
  RecLayout L;
  SellPlan* plan = nullptr;
  double* buf[2] = {nullptr, nullptr};      // state records, two iterates
  int32_t* d_flags = nullptr;               // [INCRES_MAX_CHUNK + 2]
  int32_t* d_labels = nullptr;              // [INCRES_MAX_CHUNK + 1][n], the caller's vertex order
  int32_t* d_seeds = nullptr;               // [seed_cap]
  int64_t seed_cap = 0;
  IncresPlan sched;
  std::mutex mu;
};

static const int INCRES_FLAG_WORDS = INCRES_MAX_CHUNK + 2;      // (an even count: cleared in 8-byte words)

// ---- plant: F.fill(0), then F[seeds of cluster r, r] = 1 (clustering.py:350-354) -----------------------------------------------------
__global__ __launch_bounds__(256) void incres_clear_kernel(double* __restrict__ rec, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < total) rec[i] = 0.0;
}

// seeds (k, m) in the caller's numbering (checked on the host); duplicates store the same value twice
__global__ __launch_bounds__(256) void incres_scatter_kernel(double* __restrict__ rec, int ld, const int32_t* __restrict__ seeds,
                                                             const int32_t* __restrict__ inv, int k, int64_t m) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)k * m) return;
  const int r = (int)(i / m);
  const int32_t v = seeds[i];
  const int64_t row = inv ? inv[v] : v;
  rec[row * ld + r] = 1.0;
}

// ---- census and harvest of one iterate ---------------------------------------------------------------------------------------------
// G lanes per record (the layout's G: a power of two, 4 .. 64, at least nvec), lane t holds columns 4 t .. 4 t + 3.  Per record: is one
// of the k REAL columns 0.0 (the padding up to 4 nvec is zero by construction and must not count), and np.argmax of the row: the first
// index of the largest value, a NaN being larger than any number (F holds none; numpy's rule all the same).  The zero test is on the bit
// pattern: a denormal is not zero whatever the float mode.  One flag store per wavefront that saw a zero.
template <int G>
__global__ __launch_bounds__(256) void incres_census_kernel(const double* __restrict__ rec, int ld, int nvec, int k, int64_t n,
                                                            const int32_t* __restrict__ perm, int32_t* __restrict__ flag,
                                                            int32_t* __restrict__ labels) {
  const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
  const int t = (int)(threadIdx.x % G);
  bool zero = false;
  double best = 0.0;
  int arg = 0x7fffffff;             // no column: loses against every real one
  if (row < n && t < nvec) {
    const double4 v = *(const double4*)(rec + row * ld + 4 * t);
    const double x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = 4 * t + j;
      if (c < k) {
        zero |= ((unsigned long long)__double_as_longlong(x[j]) << 1) == 0ull;
        const bool better = arg == 0x7fffffff || x[j] > best || (x[j] != x[j] && best == best);
        if (better) { best = x[j]; arg = c; }
      }
    }
  }
#pragma unroll
  for (int off = 1; off < G; off <<= 1) {
    const double ob = __shfl_xor(best, off, G);
    const int oa = __shfl_xor(arg, off, G);
    // the other lane's column wins if it is larger, or equal (or both NaN) and earlier
    bool take;
    if (oa == 0x7fffffff) take = false;
    else if (arg == 0x7fffffff) take = true;
    else if (ob != ob || best != best) take = (ob != ob) && (best == best || oa < arg);
    else take = ob > best || (ob == best && oa < arg);
    if (take) { best = ob; arg = oa; }
  }
  if (row < n && t == 0) labels[perm ? perm[row] : row] = arg;
  if (__any(zero) && (threadIdx.x & 63) == 0) *flag = 1;
}

static int incres_census(const glx_incres* h, const double* rec, int slot, hipStream_t st) {
  const int G = h->L.G;
  const int64_t threads = h->n * G;
  const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  int32_t* flag = h->d_flags + slot;
  int32_t* labels = h->d_labels + (int64_t)slot * h->n;
  const int32_t* perm = h->P->d_perm;
#define INCRES_CENSUS(GG) \
  hipLaunchKernelGGL(incres_census_kernel<GG>, grid, block, 0, st, rec, h->L.ld, h->L.nvec, h->k, h->n, perm, flag, labels)
  switch (G) {
    case 4: INCRES_CENSUS(4); break;
    case 8: INCRES_CENSUS(8); break;
    case 16: INCRES_CENSUS(16); break;
    case 32: INCRES_CENSUS(32); break;
    case 64: INCRES_CENSUS(64); break;
    default: glx_set_error("incres: unsupported lanes-per-row %d", G); return GLX_EUNSUPPORTED;
  }
#undef INCRES_CENSUS
  GLX_HIP(hipGetLastError());
  return GLX_OK;
}

static void incres_free(glx_incres* h) {
  hipSetDevice(h->device);
  if (h->P) glx_graph_destroy(h->P);        // (waits for the device: nothing in flight uses the blocks below)
  glx_pool_free(h->buf[0]);
  glx_pool_free(h->buf[1]);
  glx_pool_free(h->d_flags);
  glx_pool_free(h->d_labels);
  glx_pool_free(h->d_seeds);
  delete h;
}

extern "C" int glx_incres_create(int64_t n, const int32_t* row_ptr, const int32_t* col, const double* val, int k, int device, glx_incres** out) {
  GLX_CHECK(out, GLX_EINVAL, "glx_incres_create: null output");
  *out = nullptr;
  GLX_CHECK(row_ptr && n >= 1 && n < (1ll << 31) && (row_ptr[n] <= 0 || (col && val)), GLX_EINVAL, "glx_incres_create: null argument or n < 1");
  GLX_CHECK(k >= 1 && k <= INCRES_MAX_COLS, GLX_EUNSUPPORTED, "glx_incres_create: %d clusters outside [1, %d] (the record layout's column cap)", k,
            INCRES_MAX_COLS);
  GLX_CHECK((INCRES_MAX_CHUNK + 1) * n < (1ll << 40), GLX_EUNSUPPORTED, "glx_incres_create: n = %lld too large", (long long)n);
  glx_incres* h = new glx_incres;
  h->n = n;
  h->k = k;
  h->device = device;
  int rc = glx_graph_create(n, n, row_ptr[n], row_ptr, col, val, GLX_F64, device, &h->P);      // keeps a row's stored order
  if (!rc) rc = glx_make_layout(k, GLX_F64, false, &h->L);
  if (!rc) rc = glx_graph_plan(h->P, h->L.G, &h->plan);
  GlxCall call;
  if (!rc) rc = call.begin(device);
  const bool begun = rc == GLX_OK;
  const size_t recs = begun ? std::max<size_t>((size_t)n * h->L.ld, 8) : 8;      // (at least 64 bytes, like the sweep objects of solver.hip)
  if (!rc) rc = glx_pool_alloc((void**)&h->buf[0], recs * 8);
  if (!rc) rc = glx_pool_alloc((void**)&h->buf[1], recs * 8);
  if (!rc) rc = glx_pool_alloc((void**)&h->d_flags, (size_t)INCRES_FLAG_WORDS * 4);
  if (!rc) rc = glx_pool_alloc((void**)&h->d_labels, (size_t)(INCRES_MAX_CHUNK + 1) * n * 4);
  // both iterates start as zeros: a sweep writes the column vectors of a record, the padding behind them is read by nobody but must
  // not hold whatever the block held before
  if (!rc) rc = glx_zero_async(h->buf[0], recs * 8, call.stream());
  if (!rc) rc = glx_zero_async(h->buf[1], recs * 8, call.stream());
  if (!rc && hipStreamSynchronize(call.stream()) != hipSuccess) {
    glx_set_error("glx_incres_create: clearing the state did not complete");
    rc = GLX_EHIP;
  }
  if (rc) {
    if (begun) (void)hipStreamSynchronize(call.stream());
    incres_free(h);
    return rc;
  }
  *out = h;
  return GLX_OK;
}

extern "C" int glx_incres_destroy(glx_incres* h) {
  if (!h) return GLX_OK;
  incres_free(h);
  return GLX_OK;
}

namespace {
// the kernels behind incres_grow (incres_plan.h)
struct IncresOps {
  glx_incres* h;
  hipStream_t st;
  int32_t* h_flags;      // page-locked, INCRES_FLAG_WORDS
  int cur = 0;
  int begin_chunk(int, int) { return glx_zero_async(h->d_flags, (size_t)INCRES_FLAG_WORDS * 4, st); }      // a kernel, not a memset
  int census(int slot) { return incres_census(h, h->buf[cur], slot, st); }
  int sweep() {
    SweepArgs a;
    memset(&a, 0, sizeof(a));
    a.plan = h->plan;
    a.L = h->L;
    a.dtype = GLX_F64;
    a.xin = h->buf[cur];
    a.xout = h->buf[cur ^ 1];
    a.n_rows = h->n;
    GLX_UP(glx_launch_spmm(a, st));
    cur ^= 1;
    return GLX_OK;
  }
  int read_flags(int first, int len, const int32_t** flags) {
    GLX_HIP(hipMemcpyAsync(h_flags + first, h->d_flags + first, (size_t)(len - first + 1) * 4, hipMemcpyDeviceToHost, st));
    GLX_HIP(hipStreamSynchronize(st));
    *flags = h_flags;
    return GLX_OK;
  }
};
}  // namespace

extern "C" int glx_incres_step(glx_incres* h, const int32_t* seeds, int64_t m, int64_t max_grow, int32_t* labels_out, int64_t* sweeps_out) {
  GLX_CHECK(h && seeds && labels_out && sweeps_out, GLX_EINVAL, "glx_incres_step: null argument");
  GLX_CHECK(m >= 1 && m * h->k < (1ll << 31), GLX_EINVAL, "glx_incres_step: m = %lld seeds per cluster", (long long)m);
  GLX_CHECK(max_grow >= 1, GLX_EINVAL, "glx_incres_step: max_grow = %lld below 1", (long long)max_grow);
  const int64_t ns = m * h->k;
  for (int64_t i = 0; i < ns; ++i)
    GLX_CHECK(seeds[i] >= 0 && seeds[i] < h->n, GLX_EINVAL, "glx_incres_step: seed %d outside [0, %lld)", seeds[i], (long long)h->n);
  std::lock_guard<std::mutex> lock(h->mu);
  GlxCall call;
  GLX_UP(call.begin(h->device));
  hipStream_t st = call.stream();
  if (h->seed_cap < ns) {
    glx_pool_free(h->d_seeds);      // (every step ends with its stream drained: nothing reads the old block)
    h->d_seeds = nullptr;
    h->seed_cap = 0;
    GLX_UP(glx_pool_alloc((void**)&h->d_seeds, (size_t)ns * 2 * 4));
    h->seed_cap = ns * 2;
  }
  // seeds and flags through the work set's page-locked staging area
  char* stage = nullptr;
  GLX_UP(call.stage(&stage, (size_t)INCRES_FLAG_WORDS * 4 + (size_t)ns * 4));
  int32_t* h_flags = (int32_t*)stage;
  int32_t* h_seeds = h_flags + INCRES_FLAG_WORDS;
  memcpy(h_seeds, seeds, (size_t)ns * 4);
  GLX_HIP(hipMemcpyAsync(h->d_seeds, h_seeds, (size_t)ns * 4, hipMemcpyHostToDevice, st));
  // plant
  const int64_t total = h->n * h->L.ld;
  hipLaunchKernelGGL(incres_clear_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, h->buf[0], total);
  GLX_HIP(hipGetLastError());
  hipLaunchKernelGGL(incres_scatter_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, st, h->buf[0], h->L.ld, (const int32_t*)h->d_seeds,
                     (const int32_t*)h->P->d_inv, h->k, m);
  GLX_HIP(hipGetLastError());
  // grow
  IncresOps ops{h, st, h_flags};
  h->sched.forced = g_incres_opt.chunk;
  h->sched.margin = g_incres_opt.margin;
  h->sched.next = g_incres_opt.next;
  int64_t sweeps = 0;
  int slot = -1;
  const int rc = incres_grow(h->sched, max_grow, ops, &sweeps, &slot);
  *sweeps_out = sweeps;
  if (rc < 0) return rc;
  GLX_CHECK(rc != INCRES_CAPPED, GLX_EUNSUPPORTED,
            "glx_incres_step: the iterate still holds a zero after max_grow = %lld sweeps: the graph is disconnected, or bipartite (a path "
            "without self loops), or so long that values underflow to 0 before they arrive",
            (long long)max_grow);
  // harvest
  GLX_UP(glx_download(labels_out, h->d_labels + (int64_t)slot * h->n, (size_t)h->n * 4, st, __func__));
  GLX_HIP(hipStreamSynchronize(st));
  return GLX_OK;
}

// out: 0 the chunk cap, 1 the first guess, 2 the margin, 3 the length of a loop's second chunk, 4 grow loops so far, 5 chunks read, 6 sweeps
// enqueued, 7 sweeps counted, 8 lanes per record, 9 elements per record, 10: 1 if the graph's locality renumbering is in use, 11 slices
extern "C" int glx_incres_stats(glx_incres* h, int64_t out[12]) {
  GLX_CHECK(h && out, GLX_EINVAL, "glx_incres_stats: null argument");
  std::lock_guard<std::mutex> lock(h->mu);
  out[0] = INCRES_MAX_CHUNK;
  out[1] = INCRES_FIRST_CHUNK;
  out[2] = INCRES_MARGIN;
  out[3] = INCRES_NEXT_CHUNK;
  out[4] = h->sched.loops;
  out[5] = h->sched.chunks;
  out[6] = h->sched.enqueued;
  out[7] = h->sched.counted;
  out[8] = h->L.G;
  out[9] = h->L.ld;
  out[10] = h->P->d_perm ? 1 : 0;
  out[11] = h->plan->nslices;
  return GLX_OK;
}

// The plant's host side draws the seeds of cluster r among `J[u == r]` (clustering.py:352-354): all k member lists in one counting sort
// instead of k passes over the labels (at 70 000 vertices and 10 clusters those passes cost more than the device's whole iteration).
extern "C" int glx_host_group_by_label(int64_t n, const int32_t* labels, int k, int64_t* counts, int32_t* order) {
  GLX_CHECK(n >= 0 && n < (1ll << 31) && k >= 1 && (n == 0 || (labels && order)) && counts, GLX_EINVAL, "glx_host_group_by_label: bad argument");
  for (int r = 0; r < k; ++r) counts[r] = 0;
  for (int64_t i = 0; i < n; ++i) {
    GLX_CHECK(labels[i] >= 0 && labels[i] < k, GLX_EINVAL, "glx_host_group_by_label: label %d of vertex %lld outside [0, %d)", labels[i], (long long)i, k);
    ++counts[labels[i]];
  }
  std::vector<int64_t> next((size_t)k);
  int64_t at = 0;
  for (int r = 0; r < k; ++r) { next[r] = at; at += counts[r]; }
  for (int64_t i = 0; i < n; ++i) order[next[labels[i]]++] = (int32_t)i;
  return GLX_OK;
}
