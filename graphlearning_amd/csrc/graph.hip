// Sparse operator residency: CSR (host copy, entry order preserved) -> sliced-ELL plans in HBM.
// Replaces utils.torch_sparse (reference graphlearning/utils.py:288-317).
#include "glx_internal.h"
#include <cstring>
#include <stdarg.h>
#include <algorithm>
#include <numeric>
#include <chrono>
#include <thread>
#include <string.h>
#include <stdlib.h>

static thread_local std::string g_err;

void glx_set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}

extern "C" const char* glx_last_error(void) { return g_err.c_str(); }
extern "C" int glx_version(void) { return 100; }

extern "C" int glx_device_count(int* n) {
  GLX_CHECK(n != nullptr, GLX_EINVAL, "glx_device_count: null output");
  GLX_HIP(hipGetDeviceCount(n));
  return GLX_OK;
}

extern "C" int glx_device_synchronize(void) {
  GLX_HIP(hipDeviceSynchronize());
  return GLX_OK;
}

extern "C" void glx_free(void* p) { free(p); }

#define GLX_POOL(call) do { int rc_ = (call); if (rc_) return rc_; } while (0)

// 128-bit content fingerprint (host): 4 MiB chunks hashed independently by a few threads -- two 64-bit multiply-mix lanes per
// chunk over 16-byte blocks -- and the chunk digests folded in order.  Not cryptographic: it tells an edited matrix from an
// unedited one (utils.matrix_fingerprint), 25 MB in ~0.2 ms instead of ~1 ms on one core.
static inline uint64_t fp_mix(uint64_t a, uint64_t b) {
  const __uint128_t m = (__uint128_t)(a ^ 0x9e3779b97f4a7c15ull) * (b ^ 0xc2b2ae3d27d4eb4full);
  return (uint64_t)m ^ (uint64_t)(m >> 64);
}
static void fp_chunk(const unsigned char* p, size_t len, uint64_t seed, uint64_t out[2]) {
  uint64_t h0 = seed ^ 0x243f6a8885a308d3ull ^ len, h1 = seed ^ 0x13198a2e03707344ull;
  size_t i = 0;
  for (; i + 32 <= len; i += 32) {
    uint64_t w[4];
    memcpy(w, p + i, 32);
    h0 = fp_mix(h0 ^ w[0], w[1]) + (h0 << 1);
    h1 = fp_mix(h1 ^ w[2], w[3]) + (h1 << 1);
  }
  uint64_t tail[4] = {0, 0, 0, 0};
  memcpy(tail, p + i, len - i);
  h0 = fp_mix(h0 ^ tail[0], tail[1] + 0x5851f42d4c957f2dull);
  h1 = fp_mix(h1 ^ tail[2], tail[3] + 0x14057b7ef767814full);
  out[0] = fp_mix(h0, h1 + len);
  out[1] = fp_mix(h1, h0 ^ (len * 0x9fb21c651e98df25ull));
}
extern "C" int glx_host_fingerprint(const void* data, size_t bytes, uint64_t seed, uint64_t out[2]) {
  GLX_CHECK(out && (data || bytes == 0), GLX_EINVAL, "glx_host_fingerprint: null argument");
  const size_t CH = (size_t)1 << 20;
  const size_t nch = std::max<size_t>(1, (bytes + CH - 1) / CH);
  std::vector<uint64_t> dig(2 * nch);
  const unsigned char* p = (const unsigned char*)data;
  auto work = [&](size_t c0, size_t c1) {
    for (size_t c = c0; c < c1; ++c) fp_chunk(p + c * CH, std::min(CH, bytes - std::min(bytes, c * CH)), seed + c, &dig[2 * c]);
  };
  const int nt = (int)std::min<size_t>(8, nch);
  glx_host_parallel(nt, [&](int t) { work(nch * t / nt, nch * (t + 1) / nt); });
  uint64_t a = seed ^ bytes, b = ~seed;
  for (size_t c = 0; c < nch; ++c) {
    a = fp_mix(a ^ dig[2 * c], b + dig[2 * c + 1]);
    b = fp_mix(b ^ dig[2 * c + 1], a);
  }
  out[0] = a;
  out[1] = b;
  return GLX_OK;
}

int glx_make_layout(int C, int dtype, bool has_w, RecLayout* L) {
  GLX_CHECK(C >= 1, GLX_EINVAL, "layout: C must be >= 1 (got %d)", C);
  GLX_CHECK(dtype == GLX_F32 || dtype == GLX_F64, GLX_EINVAL, "layout: bad dtype %d", dtype);
  const int es = dtype == GLX_F32 ? 4 : 8;
  const int nvec = (C + 3) / 4;
  const int lanes = nvec + (has_w ? 1 : 0);
  GLX_CHECK(lanes <= 64, GLX_EUNSUPPORTED, "layout: C=%d needs %d lanes per row (max 64 -> C <= %d)", C, lanes,
            has_w ? 252 : 256);
  int G = 4;
  while (G < lanes) G *= 2;
  int bytes = lanes * 4 * es;   // the stop value gets a full 4-wide slot so every lane issues the same gather
  int rb = 32;
  while (rb < bytes && rb < 128) rb *= 2;      // 32 / 64 / 128-byte records stay line-aligned
  if (rb < bytes) rb = (bytes + 63) / 64 * 64; // larger records: multiple of 64 bytes
  L->C = C;
  L->nvec = nvec;
  L->ld = rb / es;
  L->woff = has_w ? nvec * 4 * es : -1;
  L->G = G;
  L->esize = es;
  L->ngroups = 1;
  L->nstop = has_w ? 1 : 0;
  return GLX_OK;
}

int glx_make_layout_groups(int C, int B, int dtype, RecLayout* L) {
  GLX_CHECK(C >= 1 && B >= 1 && B <= 32, GLX_EINVAL, "layout: %d groups of %d columns (1 .. 32 groups)", B, C);
  GLX_CHECK(dtype == GLX_F32 || dtype == GLX_F64, GLX_EINVAL, "layout: bad dtype %d", dtype);
  if (B == 1) return glx_make_layout(C, dtype, true, L);
  const int es = dtype == GLX_F32 ? 4 : 8;
  const int nvec = (C * B + 3) / 4;
  const int nstop = (B * 8 + 4 * es - 1) / (4 * es);     // fp64 stop values packed behind the columns: 4 (fp64 state) / 2 (fp32) per lane
  const int lanes = nvec + nstop;
  GLX_CHECK(lanes <= 64, GLX_EUNSUPPORTED, "layout: %d groups of %d columns need %d lanes per row (max 64)", B, C, lanes);
  int G = 8;
  while (G < lanes) G *= 2;
  const int bytes = lanes * 4 * es;
  const int rb = (bytes + 127) / 128 * 128;              // whole 128-byte lines: a gather never shares a line with another record
  L->C = C * B;
  L->nvec = nvec;
  L->ld = rb / es;
  L->woff = nvec * 4 * es;
  L->G = G;
  L->esize = es;
  L->ngroups = B;
  L->nstop = nstop;
  return GLX_OK;
}

static int graph_keep_order(glx_graph* g) {
  GLX_CHECK(g->plans.empty() && !g->order_ready, GLX_EINVAL, "glx_graph_set_order: call before the operator is first used");
  g->keep_order = true;
  return GLX_OK;
}

extern "C" int glx_graph_create(int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t* rowptr,
                                const int32_t* col, const double* val, int state_dtype, int device,
                                glx_graph** out) {
  GLX_CHECK(out != nullptr, GLX_EINVAL, "glx_graph_create: null output");
  *out = nullptr;
  GLX_CHECK(n_rows >= 0 && n_cols >= 0 && nnz >= 0, GLX_EINVAL, "glx_graph_create: negative size");
  GLX_CHECK(n_rows < (1ll << 31) && n_cols < (1ll << 31), GLX_EINVAL, "glx_graph_create: n must fit int32");
  GLX_CHECK(rowptr && (nnz == 0 || (col && val)), GLX_EINVAL, "glx_graph_create: null CSR array");
  GLX_CHECK(state_dtype == GLX_F32 || state_dtype == GLX_F64, GLX_EINVAL, "glx_graph_create: bad dtype %d", state_dtype);
  GLX_CHECK(rowptr[0] == 0 && rowptr[n_rows] == nnz, GLX_EINVAL, "glx_graph_create: rowptr[0]=%d rowptr[n]=%d nnz=%lld",
            rowptr[0], rowptr[n_rows], (long long)nnz);
  int ndev = 0;
  GLX_HIP(hipGetDeviceCount(&ndev));
  GLX_CHECK(device >= 0 && device < ndev, GLX_EINVAL, "glx_graph_create: device %d of %d", device, ndev);
  int max_row = 0;
  for (int64_t i = 0; i < n_rows; ++i) {
    const int len = rowptr[i + 1] - rowptr[i];
    GLX_CHECK(len >= 0, GLX_EINVAL, "glx_graph_create: rowptr not monotone at row %lld", (long long)i);
    max_row = std::max(max_row, len);
  }
  for (int64_t e = 0; e < nnz; ++e)
    GLX_CHECK(col[e] >= 0 && col[e] < n_cols, GLX_EINVAL, "glx_graph_create: column %d out of range at entry %lld", col[e], (long long)e);
  glx_graph* g = new glx_graph();
  g->n_rows = n_rows;
  g->n_cols = n_cols;
  g->nnz = nnz;
  g->dtype = state_dtype;
  g->device = device;
  g->max_row = max_row;
  g->h_rowptr.assign(rowptr, rowptr + n_rows + 1);
  g->h_col.assign(col, col + nnz);
  g->h_val.assign(val, val + nnz);
  g->plans.reserve(8);   // plan pointers handed out stay valid
  *out = g;
  return GLX_OK;
}

// The same operator object from CSR arrays that stay on the DEVICE: nothing but the row pointers is kept on the host, plans are
// filled straight from the resident arrays.  rowsum_out (may be NULL): the row sums `A * ones` as scipy's csr_matvec forms them
// (sequentially, in stored order) -- the degree vector of reference graph.py:108-122 -- computed on the device.  What a fresh
// ssl.poisson fit does with weightmatrix.knn's matrix (1.3 ms of host passes and two copies of the 14 MB operator otherwise).
__global__ __launch_bounds__(256) void csr_check_rowsum_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                               const double* __restrict__ val, int64_t n_rows, int64_t n_cols,
                                                               double* __restrict__ rowsum, int* __restrict__ bad) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_rows) return;
  double s = 0.0;
  int b = 0;
  for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
    const int32_t c = col[e];
    if (c < 0 || c >= n_cols) b = 1;
    s = s + val[e] * 1.0;
  }
  if (rowsum) rowsum[i] = s;
  if (b) *bad = 1;
}

extern "C" int glx_graph_create_resident(int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t* rowptr, const int32_t* col,
                                         const double* val, int state_dtype, int device, double* rowsum_out, glx_graph** out) {
  GLX_CHECK(out != nullptr, GLX_EINVAL, "glx_graph_create_resident: null output");
  *out = nullptr;
  GLX_CHECK(n_rows >= 0 && n_cols >= 0 && nnz >= 0, GLX_EINVAL, "glx_graph_create_resident: negative size");
  GLX_CHECK(n_rows < (1ll << 31) && n_cols < (1ll << 31), GLX_EINVAL, "glx_graph_create_resident: n must fit int32");
  GLX_CHECK(rowptr && (nnz == 0 || (col && val)), GLX_EINVAL, "glx_graph_create_resident: null CSR array");
  GLX_CHECK(state_dtype == GLX_F32 || state_dtype == GLX_F64, GLX_EINVAL, "glx_graph_create_resident: bad dtype %d", state_dtype);
  GLX_CHECK(rowptr[0] == 0 && rowptr[n_rows] == nnz, GLX_EINVAL, "glx_graph_create_resident: rowptr[0]=%d rowptr[n]=%d nnz=%lld",
            rowptr[0], rowptr[n_rows], (long long)nnz);
  int ndev = 0;
  GLX_HIP(hipGetDeviceCount(&ndev));
  GLX_CHECK(device >= 0 && device < ndev, GLX_EINVAL, "glx_graph_create_resident: device %d of %d", device, ndev);
  int max_row = 0;
  for (int64_t i = 0; i < n_rows; ++i) {
    const int len = rowptr[i + 1] - rowptr[i];
    GLX_CHECK(len >= 0, GLX_EINVAL, "glx_graph_create_resident: rowptr not monotone at row %lld", (long long)i);
    max_row = std::max(max_row, len);
  }
  GLX_HIP(hipSetDevice(device));
  glx_graph* g = new glx_graph();
  g->n_rows = n_rows;
  g->n_cols = n_cols;
  g->nnz = nnz;
  g->dtype = state_dtype;
  g->device = device;
  g->max_row = max_row;
  g->h_rowptr.assign(rowptr, rowptr + n_rows + 1);
  g->plans.reserve(8);
  struct Guard { glx_graph* g; ~Guard() { if (g) glx_graph_destroy(g); } } guard{g};
  GlxCall call;
  GLX_UP(call.begin(device));
  hipStream_t st = call.stream();
  GLX_POOL(glx_pool_alloc((void**)&g->d_src_rowptr, (size_t)(n_rows + 1) * 4));
  GLX_POOL(glx_pool_alloc((void**)&g->d_src_col, std::max<size_t>((size_t)nnz * 4, 4)));
  GLX_POOL(glx_pool_alloc((void**)&g->d_src_val, std::max<size_t>((size_t)nnz * 8, 8)));
  GLX_UP(glx_upload(g->d_src_rowptr, rowptr, (size_t)(n_rows + 1) * 4, st, __func__));
  if (nnz > 0) {
    GLX_UP(glx_upload(g->d_src_col, col, (size_t)nnz * 4, st, __func__));
    GLX_UP(glx_upload(g->d_src_val, val, (size_t)nnz * 8, st, __func__));
  }
  // column range check (+ the row sums) on the device; results through the work set's page-locked staging area
  char* stage = nullptr;
  GLX_UP(call.stage(&stage, (size_t)n_rows * 8 + 64));
  double* d_sum = nullptr;
  int* d_bad = nullptr;
  GLX_UP(call.alloc(&d_sum, (size_t)n_rows));
  GLX_UP(call.alloc(&d_bad, 16));
  GLX_HIP(hipMemsetAsync(d_bad, 0, 4, st));
  if (n_rows > 0) {
    hipLaunchKernelGGL(csr_check_rowsum_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, (const int32_t*)g->d_src_rowptr,
                       (const int32_t*)g->d_src_col, (const double*)g->d_src_val, n_rows, n_cols, rowsum_out ? d_sum : nullptr, d_bad);
    GLX_HIP(hipGetLastError());
  }
  int* h_bad = (int*)(stage + (size_t)n_rows * 8);
  GLX_HIP(hipMemcpyAsync(h_bad, d_bad, 4, hipMemcpyDeviceToHost, st));
  if (rowsum_out && n_rows > 0) GLX_HIP(hipMemcpyAsync(stage, d_sum, (size_t)n_rows * 8, hipMemcpyDeviceToHost, st));
  GLX_HIP(hipStreamSynchronize(st));
  GLX_CHECK(*h_bad == 0, GLX_EINVAL, "glx_graph_create_resident: column index out of range");
  if (rowsum_out && n_rows > 0) memcpy(rowsum_out, stage, (size_t)n_rows * 8);
  guard.g = nullptr;
  *out = g;
  return GLX_OK;
}

// Row i of the operator = row i of the resident source with its entries in reverse order (reverse_rows != 0) and multiplied by
// row_scale[i] (NULL: as they are).  Before the operator is first used.  reverse + D^-1: P = D^-1 W^T of a symmetric W exactly as
// scipy writes it down (`D * W.transpose()`: csr_matmat emits every row in reverse, reference ssl.py:634-635).
extern "C" int glx_graph_set_row_transform(glx_graph* g, const double* row_scale, int reverse_rows) {
  GLX_CHECK(g, GLX_EINVAL, "glx_graph_set_row_transform: null graph");
  GLX_CHECK(g->d_src_col != nullptr, GLX_EINVAL, "glx_graph_set_row_transform: not a resident graph (glx_graph_create_resident)");
  GLX_CHECK(g->plans.empty(), GLX_EINVAL, "glx_graph_set_row_transform: call before the operator is first used");
  GLX_HIP(hipSetDevice(g->device));
  g->reverse_rows = reverse_rows != 0;
  glx_pool_free(g->d_row_scale);
  g->d_row_scale = nullptr;
  if (row_scale && g->n_rows > 0) {
    GLX_POOL(glx_pool_alloc((void**)&g->d_row_scale, (size_t)g->n_rows * 8));
    GlxCall call;                      // (a work set's stream, not a blocking copy on the NULL stream: see glx_graph_set_order)
    GLX_UP(call.begin(g->device));
    GLX_UP(glx_upload(g->d_row_scale, row_scale, (size_t)g->n_rows * 8, call.stream(), __func__));
    GLX_HIP(hipStreamSynchronize(call.stream()));
  }
  return GLX_OK;
}

static void free_plan(SellPlan& p) {      // (callers: glx_graph_destroy behind its device synchronisation)
  glx_pool_free(p.d_slot_row);
  glx_pool_free(p.d_slot_len);
  glx_pool_free(p.d_slice_hdr);
  glx_pool_free(p.d_col);
  glx_pool_free(p.d_val);
  p = SellPlan();
}

extern "C" int glx_graph_destroy(glx_graph* g) {
  if (!g) return GLX_OK;
  hipSetDevice(g->device);
  // the operator's buffers go back to the size-class pool (hipFree of a block of megabytes costs 0.23 ms and there were ten of them: a
  // third of a first fit on a fresh graph, profiles/r06_fresh_path.txt).  hipFree waited for the device; the pool's contract is that nothing
  // in flight still uses a block that is handed back -- so wait here, once.
  hipDeviceSynchronize();
  for (auto& p : g->plans) free_plan(p);
  if (g->cg_ws) glx_cg_ws_destroy(g->cg_ws);
  glx_pool_free(g->d_perm);
  glx_pool_free(g->d_inv);
  glx_pool_free(g->d_src_rowptr);
  glx_pool_free(g->d_src_col);
  glx_pool_free(g->d_src_val);
  glx_pool_free(g->d_row_scale);
  delete g;
  return GLX_OK;
}

extern "C" int glx_graph_info(const glx_graph* g, int64_t info[8]) {
  GLX_CHECK(g && info, GLX_EINVAL, "glx_graph_info: null argument");
  for (int i = 0; i < 8; ++i) info[i] = 0;
  info[0] = g->n_rows;
  info[1] = g->n_cols;
  info[2] = g->nnz;
  if (!g->plans.empty()) {
    info[3] = g->plans[0].stored;
    info[4] = g->plans[0].nslices;
    info[5] = g->plans[0].R;
  }
  info[6] = g->max_row;
  info[7] = g->h_perm.empty() ? 0 : 1;
  return GLX_OK;
}

// Reverse Cuthill-McKee on the symmetrised pattern: neighbours get nearby ids, so the
// contiguous id range an XCD works on mostly gathers records of that same range (its own L2).
static void rcm_order_arrays(int64_t n, const int32_t* h_rowptr, const int32_t* h_col, std::vector<int32_t>& perm, bool sort_children);

static void rcm_order(const glx_graph* g, std::vector<int32_t>& perm, bool sort_children = true) {
  rcm_order_arrays(g->n_rows, g->h_rowptr.data(), g->h_col.data(), perm, sort_children);   // (resident sources: glx_graph_ensure_order fetched the pattern)
}

static void rcm_order_arrays(int64_t n, const int32_t* h_rowptr, const int32_t* h_col, std::vector<int32_t>& perm, bool sort_children) {
  // The order is a locality heuristic: any permutation is correct.  When every vertex has as many
  // stored entries in its row as in its column the pattern is (almost certainly) symmetric --
  // P = D^-1 W^T, Laplacians -- and the rows themselves serve as adjacency lists; otherwise the
  // pattern is symmetrised first.
  std::vector<int64_t> indeg(n, 0);
  for (int64_t e = 0; e < h_rowptr[n]; ++e) indeg[h_col[e]]++;
  bool balanced = true;
  for (int64_t i = 0; i < n && balanced; ++i) balanced = indeg[i] == (int64_t)(h_rowptr[i + 1] - h_rowptr[i]);
  std::vector<int64_t> ptr_own;
  std::vector<int32_t> adj_own;
  const int32_t* adj;
  const int64_t* ptr;
  std::vector<int64_t> ptr64;
  if (balanced) {
    ptr64.assign(h_rowptr, h_rowptr + n + 1);
    ptr = ptr64.data();
    adj = h_col;
  } else {
    ptr_own.assign(n + 1, 0);
    for (int64_t i = 0; i < n; ++i)
      for (int64_t e = h_rowptr[i]; e < h_rowptr[i + 1]; ++e) {
        ptr_own[i + 1]++;
        ptr_own[h_col[e] + 1]++;
      }
    for (int64_t i = 0; i < n; ++i) ptr_own[i + 1] += ptr_own[i];
    adj_own.resize(ptr_own[n]);
    std::vector<int64_t> fill(ptr_own.begin(), ptr_own.end() - 1);
    for (int64_t i = 0; i < n; ++i)
      for (int64_t e = h_rowptr[i]; e < h_rowptr[i + 1]; ++e) {
        const int32_t j = h_col[e];
        adj_own[fill[i]++] = j;
        adj_own[fill[j]++] = (int32_t)i;
      }
    ptr = ptr_own.data();
    adj = adj_own.data();
  }
  auto degree = [&](int32_t v) { return ptr[v + 1] - ptr[v]; };
  // vertices by ascending degree, ties by index (a counting sort: degrees are small integers)
  std::vector<int32_t> by_deg(n);
  {
    int64_t dmax = 0;
    for (int64_t v = 0; v < n; ++v) dmax = std::max<int64_t>(dmax, degree((int32_t)v));
    std::vector<int64_t> first(dmax + 2, 0);
    for (int64_t v = 0; v < n; ++v) first[degree((int32_t)v) + 1]++;
    for (int64_t q = 0; q <= dmax; ++q) first[q + 1] += first[q];
    for (int64_t v = 0; v < n; ++v) by_deg[first[degree((int32_t)v)]++] = (int32_t)v;
  }
  std::vector<char> seen(n, 0);
  perm.clear();
  perm.reserve(n);
  std::vector<int32_t> nb;
  for (int32_t start : by_deg) {
    if (seen[start]) continue;
    seen[start] = 1;
    size_t head = perm.size();
    perm.push_back(start);
    while (head < perm.size()) {
      const int32_t v = perm[head++];
      nb.clear();
      for (int64_t e = ptr[v]; e < ptr[v + 1]; ++e) {
        const int32_t u = adj[e];
        if (!seen[u]) { seen[u] = 1; nb.push_back(u); }
      }
      if (sort_children) std::sort(nb.begin(), nb.end(), [&](int32_t a, int32_t b) { return degree(a) < degree(b) || (degree(a) == degree(b) && a < b); });
      perm.insert(perm.end(), nb.begin(), nb.end());
    }
  }
  std::reverse(perm.begin(), perm.end());
}

// Vertex renumbering used by every plan of this operator (square operators only):
// d_perm[new] = old, d_inv[old] = new.  Dense operands live on the device in the NEW order;
// pack/unpack translate.  The entry order inside a row never changes.
int glx_graph_ensure_order(glx_graph* g) {
  if (g->order_ready) return GLX_OK;
  g->order_ready = true;
  const int64_t n = g->n_rows;
  if (g->keep_order || g->n_rows != g->n_cols || n < 4096) return GLX_OK;
  if (g->d_src_col && g->h_col.empty() && g->nnz > 0) {      // a resident source: the pass below reads the pattern on the host
    g->h_col.resize(g->nnz);
    GLX_HIP(hipSetDevice(g->device));
    GLX_UP(glx_download_sync(g->h_col.data(), g->d_src_col, (size_t)g->nnz * 4, __func__));
  }
  const auto t_rcm0 = std::chrono::steady_clock::now();
  rcm_order(g, g->h_perm, true);
  if (getenv("GLX_TIMING")) fprintf(stderr, "[glx] locality order of %lld vertices: %.1f ms\n", (long long)n,
                                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_rcm0).count());
  g->h_inv.assign(n, 0);
  for (int64_t i = 0; i < n; ++i) g->h_inv[g->h_perm[i]] = (int32_t)i;
  GLX_HIP(hipSetDevice(g->device));
  GLX_POOL(glx_pool_alloc((void**)&g->d_perm, n * 4));
  GLX_POOL(glx_pool_alloc((void**)&g->d_inv, n * 4));
  GLX_UP(glx_upload_sync(g->d_perm, g->h_perm.data(), n * 4, __func__));
  GLX_UP(glx_upload_sync(g->d_inv, g->h_inv.data(), n * 4, __func__));
  return GLX_OK;
}

// Host helper of ssl.poisson's operator set-up for a symmetric W: row i of P = D^-1 W^T is row i of W scaled by
// scale[i] = 1/deg_i, with the entries in REVERSE order (the order scipy's csr_matmat leaves them in, which the sweep's
// bit-exactness depends on); deg_out[i] = the row sum in stored order from 0.0 (scipy's csr_matvec with a vector of ones).
// Plain loops over the CSR arrays: the numpy formulation of the same thing cost 8 ms at 70 000 vertices.
extern "C" int glx_host_row_sums(int64_t n, const int32_t* rowptr, const double* val, double* sum_out) {
#pragma clang fp contract(off)
  GLX_CHECK(rowptr && val && sum_out, GLX_EINVAL, "glx_host_row_sums: null argument");
  for (int64_t i = 0; i < n; ++i) {
    double s = 0.0;
    for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) s = s + val[e] * 1.0;
    sum_out[i] = s;
  }
  return GLX_OK;
}

// The nonzero rows of -L[:, cols] * F (ssl.laplace's right-hand side, reference ssl.py:1236) from the CSC image of L: scipy forms the
// CSR matrix -L[:, cols] and csr_matvecs adds a row's products one after another from 0, i.e. for canonical L and distinct cols the
// terms (-l_ij) * F[pos(j), :] in ascending j.  Rows listed in `cols` themselves are left out (they are not part of the Dirichlet
// system), every other row comes out times row_scale[row] (M*b, ssl.py:1249).  *count_out = -1: duplicate columns, the caller falls
// back to the literal expression.
extern "C" int glx_host_neg_columns_rows(int64_t n, const int32_t* cptr, const int32_t* crow, const double* cval, int64_t m, const int64_t* cols,
                                         const double* F, int k, const double* row_scale, int64_t cap, int32_t* rows_out, double* vals_out,
                                         int64_t* count_out) {
#pragma clang fp contract(off)
  GLX_CHECK(cptr && crow && cval && F && rows_out && vals_out && count_out && (cols || m == 0), GLX_EINVAL, "glx_host_neg_columns_rows: null argument");
  GLX_CHECK(n >= 0 && m >= 0 && k > 0, GLX_EINVAL, "glx_host_neg_columns_rows: bad size");
  for (int64_t q = 0; q < m; ++q) GLX_CHECK(cols[q] >= 0 && cols[q] < n, GLX_EINVAL, "glx_host_neg_columns_rows: column %lld out of range", (long long)cols[q]);
  std::vector<int64_t> pos((size_t)m);
  for (int64_t q = 0; q < m; ++q) pos[q] = q;
  std::stable_sort(pos.begin(), pos.end(), [&](int64_t a, int64_t b) { return cols[a] < cols[b]; });
  for (int64_t q = 1; q < m; ++q)
    if (cols[pos[q]] == cols[pos[q - 1]]) { *count_out = -1; return GLX_OK; }
  static thread_local std::vector<int32_t> slot;       // row -> slot of this call, -1 elsewhere (only touched entries are reset)
  if ((int64_t)slot.size() < n) slot.assign((size_t)n, -1);
  std::vector<int32_t> touched;
  std::vector<double> acc;
  for (int64_t q = 0; q < m; ++q) {
    const int64_t j = cols[pos[q]];
    const double* f = F + (size_t)pos[q] * k;
    for (int64_t e = cptr[j]; e < cptr[j + 1]; ++e) {
      const int32_t row = crow[e];
      int32_t sl = slot[row];
      if (sl < 0) {
        sl = (int32_t)touched.size();
        slot[row] = sl;
        touched.push_back(row);
        acc.resize(acc.size() + (size_t)k, 0.0);
      }
      const double nv = -cval[e];
      double* a = acc.data() + (size_t)sl * k;
      for (int c = 0; c < k; ++c) a[c] = a[c] + nv * f[c];
    }
  }
  std::vector<int32_t> ord(touched);
  std::sort(ord.begin(), ord.end());
  for (int64_t q = 0; q < m; ++q) {                    // the labelled rows themselves are not part of the system
    const int32_t sl = slot[cols[q]];
    if (sl >= 0) slot[cols[q]] = -2 - sl;
  }
  int64_t cnt = 0;
  int rc = GLX_OK;
  for (int32_t row : ord) {
    const int32_t sl = slot[row];
    if (sl < 0) continue;
    if (cnt >= cap) { rc = GLX_EINVAL; glx_set_error("glx_host_neg_columns_rows: more than %lld rows", (long long)cap); break; }
    const double sc = row_scale ? row_scale[row] : 1.0;
    const double* a = acc.data() + (size_t)sl * k;
    rows_out[cnt] = row;
    for (int c = 0; c < k; ++c) vals_out[(size_t)cnt * k + c] = row_scale ? sc * a[c] : a[c];
    ++cnt;
  }
  for (int32_t row : touched) slot[row] = -1;
  *count_out = cnt;
  return rc;
}

extern "C" int glx_host_reverse_scale_rows(int64_t n, const int32_t* rowptr, const int32_t* col, const double* val, const double* scale,
                                           int32_t* col_out, double* val_out) {
#pragma clang fp contract(off)
  GLX_CHECK(rowptr && col && val && scale && col_out && val_out, GLX_EINVAL, "glx_host_reverse_scale_rows: null argument");
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(8, n / 16384));
  auto work = [&](int64_t lo, int64_t hi) {
    for (int64_t i = lo; i < hi; ++i) {
      const int64_t a = rowptr[i], b = rowptr[i + 1];
      const double sc = scale[i];
      for (int64_t e = a; e < b; ++e) {
        const int64_t src = a + (b - 1 - e);
        col_out[e] = col[src];
        val_out[e] = sc * val[src];
      }
    }
  };
  if (nt == 1) {
    work(0, n);
  } else {
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t) th.emplace_back(work, n * t / nt, n * (t + 1) / nt);
    for (auto& x : th) x.join();
  }
  return GLX_OK;
}

// The library's locality order (the breadth-first / reverse Cuthill-McKee pass of rcm_order) for a pattern the caller holds on the
// host, restricted to the columns [col_lo, col_lo + n): a rank of the vertex-partitioned sweep orders ITS rows by their links
// among themselves (halo columns ignored) -- the rectangular rank-local operator is never renumbered by the library.
// perm_out[new] = old.
extern "C" int glx_host_locality_order(int64_t n, const int32_t* rowptr, const int32_t* col, int64_t col_lo, int32_t* perm_out) {
  GLX_CHECK(n >= 0 && rowptr && col && perm_out, GLX_EINVAL, "glx_host_locality_order: null argument");
  std::vector<int32_t> rp(n + 1, 0), cc;
  cc.reserve((size_t)rowptr[n]);
  for (int64_t i = 0; i < n; ++i) {
    for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
      const int64_t j = (int64_t)col[e] - col_lo;
      if (j >= 0 && j < n) cc.push_back((int32_t)j);
    }
    rp[i + 1] = (int32_t)cc.size();
  }
  std::vector<int32_t> perm;
  rcm_order_arrays(n, rp.data(), cc.data(), perm, true);
  GLX_CHECK((int64_t)perm.size() == n, GLX_EINVAL, "glx_host_locality_order: internal error");
  memcpy(perm_out, perm.data(), (size_t)n * 4);
  return GLX_OK;
}

// rows of a CSR matrix in another order (row i of the result = row perm[i] of the input, entries in their stored order), on host
// threads: scipy's fancy row indexing takes seconds at 2 x 10^8 entries
extern "C" int glx_host_permute_rows(int64_t n, const int32_t* rowptr, const int32_t* col, const double* val, const int64_t* perm,
                                     int32_t* rowptr_out, int32_t* col_out, double* val_out) {
  GLX_CHECK(n >= 0 && rowptr && col && val && perm && rowptr_out && col_out && val_out, GLX_EINVAL, "glx_host_permute_rows: null argument");
  rowptr_out[0] = 0;
  for (int64_t i = 0; i < n; ++i) {
    GLX_CHECK(perm[i] >= 0 && perm[i] < n, GLX_EINVAL, "glx_host_permute_rows: row %lld out of range", (long long)perm[i]);
    const int64_t len = rowptr[perm[i] + 1] - rowptr[perm[i]];
    GLX_CHECK((int64_t)rowptr_out[i] + len < (1ll << 31), GLX_EUNSUPPORTED, "glx_host_permute_rows: more than 2^31 entries");
    rowptr_out[i + 1] = rowptr_out[i] + (int32_t)len;
  }
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(16, n / 65536));
  auto work = [&](int64_t lo, int64_t hi) {
    for (int64_t i = lo; i < hi; ++i) {
      const int64_t a = rowptr[perm[i]], len = rowptr[perm[i] + 1] - a, o = rowptr_out[i];
      memcpy(col_out + o, col + a, (size_t)len * 4);
      memcpy(val_out + o, val + a, (size_t)len * 8);
    }
  };
  if (nt == 1) {
    work(0, n);
  } else {
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t) th.emplace_back(work, n * t / nt, n * (t + 1) / nt);
    for (auto& x : th) x.join();
  }
  return GLX_OK;
}

// The caller's own vertex order (perm[new] = old) instead of the library's reverse Cuthill-McKee pass: whoever built the graph
// may know a better one -- weightmatrix.knn has the FEATURES in hand, and an order by a tree over feature space keeps
// neighbours close without looking at the graph at all.  Before the operator is first used.
extern "C" int glx_graph_set_order(glx_graph* g, const int32_t* perm) {
  GLX_CHECK(g, GLX_EINVAL, "glx_graph_set_order: null graph");
  if (!perm) return graph_keep_order(g);      // the caller's order as it is: no renumbering at all
  GLX_CHECK(g->plans.empty() && !g->order_ready, GLX_EINVAL, "glx_graph_set_order: call before the operator is first used");
  GLX_CHECK(g->n_rows == g->n_cols, GLX_EINVAL, "glx_graph_set_order: operator must be square");
  const int64_t n = g->n_rows;
  std::vector<int32_t> inv(n, -1);
  for (int64_t i = 0; i < n; ++i) {
    GLX_CHECK(perm[i] >= 0 && perm[i] < n && inv[perm[i]] < 0, GLX_EINVAL, "glx_graph_set_order: not a permutation at position %lld", (long long)i);
    inv[perm[i]] = (int32_t)i;
  }
  g->h_perm.assign(perm, perm + n);
  g->h_inv.swap(inv);
  g->order_ready = true;
  GLX_HIP(hipSetDevice(g->device));
  GLX_POOL(glx_pool_alloc((void**)&g->d_perm, std::max<size_t>(n * 4, 4)));
  GLX_POOL(glx_pool_alloc((void**)&g->d_inv, std::max<size_t>(n * 4, 4)));
  // through a work set's stream and its page-locked staging: a blocking hipMemcpy runs on the NULL stream, whose copy queue the first
  // such call of a process creates (9 ms of a fresh model's first fit_predict)
  GlxCall call;
  GLX_UP(call.begin(g->device));
  GLX_UP(glx_upload(g->d_perm, g->h_perm.data(), (size_t)n * 4, call.stream(), __func__));
  GLX_UP(glx_upload(g->d_inv, g->h_inv.data(), (size_t)n * 4, call.stream(), __func__));
  GLX_HIP(hipStreamSynchronize(call.stream()));
  return GLX_OK;
}

extern "C" int glx_graph_order(glx_graph* g, int32_t* perm_out) {
  GLX_CHECK(g && perm_out, GLX_EINVAL, "glx_graph_order: null argument");
  int rc = glx_graph_ensure_order(g);
  if (rc) return rc;
  for (int64_t i = 0; i < g->n_rows; ++i) perm_out[i] = g->h_perm.empty() ? (int32_t)i : g->h_perm[i];
  return GLX_OK;
}


// The sliced-ELL image is assembled ON THE DEVICE (round 3): the CSR arrays go up as they are and one wavefront per slice
// writes the slice's chunks -- image position (chunk k, lane w) holds entry jj = (k S + seg) 4 + t of the row in slot w / 4
// (G = 4: seg = slot within the row's S slots, t = w % 4; wider rows: jj = k G + w % G), or a zero for positions past the end
// of the row -- so nothing needs a memset and the host never touches the 1.3 M (... 2 x 10^8) entries: the host fill took 6 ms at
// 70 000 vertices with 16 threads (300 ms at 18 M entries), more than everything else of the plan together.
template <typename T>
__global__ __launch_bounds__(256) void sell_fill_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ ccol,
                                                        const double* __restrict__ cval, const int32_t* __restrict__ perm,
                                                        const int32_t* __restrict__ inv, const int32_t* __restrict__ slot_row,
                                                        const int32_t* __restrict__ slot_len, const SliceHdr* __restrict__ hdr,
                                                        int64_t nslices, int64_t head, int G, int32_t* __restrict__ col, T* __restrict__ val,
                                                        const double* __restrict__ row_scale, int reverse) {
#pragma clang fp contract(off)
  // row_scale / reverse (resident sources, glx_graph_set_row_transform): entry jj of the operator's row is entry len - 1 - jj of
  // the source row, times row_scale[row] -- one rounding, the host expression `scale[i] * w` of the reference's D^-1 W^T
  const int lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= nslices) return;
  const SliceHdr h = hdr[s];
  const int S = h.S & 0xff, R = 64 / G;
  const int slot = lane / G, t = lane % G;
  const int32_t row = slot_row[s * R + slot];
  const int len = slot_len[s * R + slot];
  const int seg = slot & (S - 1);
  const int32_t orow = row >= 0 ? (perm ? perm[row] : row) : 0;
  const int64_t b = row >= 0 ? rowptr[orow] : 0;
  const double sc = (row >= 0 && row_scale) ? row_scale[orow] : 1.0;
  for (int k = 0; k < h.nchunks || k == 0; ++k) {          // chunk 0 always exists (the dense head region)
    const int jj = G == 4 ? (k * S + seg) * 4 + t : k * G + t;
    int32_t c = 0;
    double v = 0.0;
    if (row >= 0 && jj < len) {
      const int64_t src = reverse ? b + (len - 1 - jj) : b + jj;
      c = ccol[src];
      if (inv) c = inv[c];
      v = cval[src];
      if (row_scale) v = sc * v;
    }
    const int64_t idx = k == 0 ? s * 64 + lane : head + h.ptr + (int64_t)(k - 1) * 64 + lane;
    col[idx] = c;
    val[idx] = (T)v;
  }
}

// Build (once per G) the sliced-ELL image of the operator.  The (renumbered) rows are cut
// into 8 contiguous id ranges, one per XCD; inside a range rows are handed to wavefront slices
// in order of decreasing length (longest first: LPT balance, little padding inside a slice);
// the ENTRY order inside a row is untouched.  G = 4 plans split rows longer than L1 entries
// over S = 4 slots and rows longer than L4 over S = 16 slots.  Every range
// is padded with empty slices to the same number of 4-slice blocks, so block b serves range
// b % 8 -- the XCD the dispatcher is observed to place it on.
int glx_graph_plan(glx_graph* g, int G, SellPlan** out, bool relaxed) {
  if (G != 4) relaxed = false;      // (segments exist in G = 4 plans only)
  for (auto& p : g->plans)
    if (p.G == G && p.relaxed == relaxed) {
      *out = &p;
      return GLX_OK;
    }
  int rc = glx_graph_ensure_order(g);
  if (rc) return rc;
  GLX_HIP(hipSetDevice(g->device));
  const auto t_plan0 = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (getenv("GLX_TIMING")) fprintf(stderr, "[glx] plan G=%d, %s: %.1f ms since the plan started\n", G, what,
                                      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_plan0).count());
  };
  const int R = 64 / G;
  const int64_t n = g->n_rows;
  const bool renum = !g->h_perm.empty();
  int L1 = 24, L4 = 96;   // measured on the 70k k=10 graph (fp64): 24/96 13.3 us, 32/128 15.2 us, 16/64 15.4 us
  // Round 3: once the vertex records no longer fit the L2s (8 x 4 MB) the balance tips the other way -- every gather is a trip to
  // the Infinity Cache / HBM whatever the slice shape, and what counts is fewer, longer slices (a row of 25 entries should not take
  // four quarter-filled slots) and less padding: n = 1e6 (d = 64): 277.1 us with 24/96, 258.5 with 40/160, 248.6 with 64/256
  // (-10 %), 250.9 with 96/384; n = 1e7: 4020 -> 3887 us; at 70 000 vertices 64/256 costs 18.1 us against 13.1
  // (profiles/r03_slot_thresholds.txt).
  // Relaxed plans (tolerance-mode CG: a row's entries may be added in any fixed order, its segments sum independently and are
  // combined once behind the chunk loop): what counts is the number of wavefronts, every one of which pays its header loads, its
  // epilogue and its share of the column dots -- fewer, longer slices win.  Config 3 (60 000 vertices, rows of 21..660 entries),
  // SpMM + dots per launch: 8/64 37.6 us, 24/96 32.2, 32/128 27.3, 64/256 26.5, 96/384 32.6 (profiles/r04_cg_slot_thresholds.txt)
  if (relaxed) { L1 = 64; L4 = 256; }
#ifndef GLX_SELL_WINDOW_MIN_MB
#define GLX_SELL_WINDOW_MIN_MB 32      // records beyond the eight L2s (32 MB)
#endif
  const bool big_state = (double)g->n_cols * G * 4.0 * (g->dtype == GLX_F64 ? 8.0 : 4.0) >= (double)GLX_SELL_WINDOW_MIN_MB * 1024 * 1024;
  if (big_state) { L1 = 64; L4 = 256; }
  const bool window_state = big_state;
  const int64_t sigma_big = 32768;      // measured at n = 10^6 (fp64, us per sweep): whole range 255, 8192: 255, 16384: 252, 32768: 229, 65536: 239, 131072: 253
  bool windowed = false;
  if (G != 4) { L1 = 1 << 30; L4 = 1 << 30; }
  auto old_of = [&](int64_t nid) -> int64_t { return renum ? g->h_perm[nid] : nid; };
  // (row lengths in the new numbering, looked up ~6 times per row below: one pass through the permutation instead of six)
  std::vector<int32_t> len_new((size_t)n);
  for (int64_t nid = 0; nid < n; ++nid) { const int64_t o = old_of(nid); len_new[nid] = (int32_t)(g->h_rowptr[o + 1] - g->h_rowptr[o]); }
  auto rowlen = [&](int64_t nid) -> int { return len_new[nid]; };
  auto klass = [&](int len) { return len > L4 ? 16 : (len > L1 ? 4 : 1); };

  const int NX = 8;
  std::vector<std::vector<SliceHdr>> ghdr(NX);
  std::vector<std::vector<int32_t>> grow(NX), glen(NX);
  // the eight id ranges carry equal WORK, not equal row counts (equal rows, the round-2 rule: 13.69 -> 13.10 us per sweep at config 2, profiles/r03_xcd_balance.txt): the launch ends
  // when the slowest XCD does, and under a locality order the rows' lengths drift along the order (a cluster's dense core
  // first, its fringe last).  Work of a row = its entries + XCD_ROW_COST (header, epilogue, store).
  std::vector<int64_t> xb(NX + 1, 0);
  {
    const bool by_work = n >= NX;
    const int64_t row_cost = 3;
    int64_t total = 0;
    if (by_work) for (int64_t i = 0; i < n; ++i) total += rowlen(i) + row_cost;
    int64_t acc = 0, i = 0;
    for (int x = 1; x < NX; ++x) {
      if (!by_work) { xb[x] = n * x / NX; continue; }
      const int64_t want = total * x / NX;
      while (i < n && acc < want) { acc += rowlen(i) + row_cost; ++i; }
      xb[x] = i;
    }
    xb[NX] = n;
  }
  for (int x = 0; x < NX; ++x) {
    const int64_t b0 = xb[x], b1 = xb[x + 1];
    const int64_t m = b1 - b0;
    std::vector<int32_t> order(m);
    grow[x].reserve((size_t)m + m / 4 + 4 * R);
    glen[x].reserve((size_t)m + m / 4 + 4 * R);
    ghdr[x].reserve((size_t)m / (R > 0 ? R : 1) + 16);
    // sort by decreasing length inside windows of `sigma` consecutive ids (SELL-C-sigma): small
    // windows keep rows that share neighbours in the same wavefronts/CUs (L1 reuse), large ones
    // minimise padding.  The whole XCD range is one window.
    // Round 5: once the records no longer fit the L2s the window must be SMALL.  The wavefronts resident on an XCD at one time cover
    // ~10^4 consecutive rows of the slice order; sorted by length over the whole range those rows come from all over the XCD's share
    // of the vertex order (16 MB of records at 10^6 vertices against a 4 MB L2) and their gathers miss -- counters at n = 10^6:
    // 1.82 GB per sweep against 0.57 GB for the distinct records of the eight ranges (profiles/r05_scale_1e6_pmc.txt).  Sorted inside
    // windows of `sigma` consecutive rows the resident wavefronts work on one stretch of the locality order at a time: -10 % at 32768
    // rows per window.  (Smaller windows gain nothing: inside a cluster of the blob data the kNN graph is an expander -- a window's
    // neighbours are spread over its whole cluster, 13 MB of records, whatever the window's size.)
    int64_t sigma = window_state ? sigma_big : m;
    if (sigma < m) windowed = true;
    // With windows the LONG rows (those split over 4 or 16 slots: chains of dependent round trips) still come first, longest first,
    // whatever their window: they are few and they are what a launch's tail consists of (without this the windows cost 20 % at
    // 3 x 10^5 vertices, where an XCD's range is hardly more than one window).
    int64_t nlong = 0;
    std::vector<int32_t> rest;
    if (sigma < m) {
      std::vector<int32_t> lng;
      rest.reserve(m);
      for (int64_t i = 0; i < m; ++i) (klass(rowlen(b0 + i)) > 1 ? lng : rest).push_back((int32_t)(b0 + i));
      std::stable_sort(lng.begin(), lng.end(), [&](int32_t a, int32_t b) { return rowlen(a) > rowlen(b); });
      nlong = (int64_t)lng.size();
      std::copy(lng.begin(), lng.end(), order.begin());
    }
    for (int64_t w0 = 0; w0 < m - nlong; w0 += sigma) {
      const int64_t w1 = std::min(m - nlong, w0 + sigma);
      auto rowat = [&](int64_t i) -> int64_t { return nlong || sigma < m ? (int64_t)rest[i] : b0 + i; };
      std::vector<int64_t> cnt(g->max_row + 2, 0);
      for (int64_t i = w0; i < w1; ++i) cnt[g->max_row - rowlen(rowat(i)) + 1]++;
      for (size_t b = 1; b < cnt.size(); ++b) cnt[b] += cnt[b - 1];
      for (int64_t i = w0; i < w1; ++i) order[nlong + w0 + cnt[g->max_row - rowlen(rowat(i))]++] = (int32_t)rowat(i);
    }
    int64_t pos = 0;
    while (pos < m) {
      const int S = klass(rowlen(order[pos]));
      SliceHdr h;
      h.ptr = 0;
      h.S = S;
      int width = 0, narrow = 1 << 30;
      for (int r = 0; r < R / S; ++r) {
        int32_t row = -1;
        int len = 0;
        if (pos < m && klass(rowlen(order[pos])) == S) {
          row = order[pos];
          len = rowlen(row);
          ++pos;
        }
        for (int sgm = 0; sgm < S; ++sgm) { grow[x].push_back(row); glen[x].push_back(len); }
        width = std::max(width, len);
        narrow = std::min(narrow, len);      // (an empty slot has len 0)
      }
      h.nchunks = G == 4 ? (width + 4 * S - 1) / (4 * S) : (width + G - 1) / G;
      // G = 4: chunks k < full hold four real entries in EVERY slot of the slice -- the kernel gathers them without predicates
      // (rows are sorted by length, so a slice's rows are nearly equally long and most chunks are full); bits 8.. of S
      if (G == 4) h.S = S | ((narrow / (4 * S)) << 8);
      ghdr[x].push_back(h);
    }
    // longest-running slices first (the launch ends when the last wavefront does): a slice's time is its gather rounds times the
    // cost of a round in its class -- measured per chunk at config 3: 1.25 / 2.5 / 3.6 us for S = 1 / 4 / 16 when the running sum
    // hops between segments, one price for all when it does not (relaxed).  Not with windows: the order of the windows IS the point
    // (and with thousands of slices per XCD the tail of a launch does not matter).
    if (!windowed) {
      const size_t ns = ghdr[x].size();
      std::vector<int32_t> idx(ns);
      for (size_t q = 0; q < ns; ++q) idx[q] = (int32_t)q;
      auto cost = [&](const SliceHdr& h) {
        const int S = h.S & 0xff;
        return (int64_t)h.nchunks * (relaxed ? 4 : (S == 1 ? 4 : (S == 4 ? 8 : 12)));
      };
      std::stable_sort(idx.begin(), idx.end(), [&](int32_t a, int32_t b) { return cost(ghdr[x][a]) > cost(ghdr[x][b]); });
      std::vector<SliceHdr> h2(ns);
      std::vector<int32_t> r2(ns * R), l2(ns * R);
      for (size_t q = 0; q < ns; ++q) {
        h2[q] = ghdr[x][idx[q]];
        for (int r = 0; r < R; ++r) {
          r2[q * R + r] = grow[x][(size_t)idx[q] * R + r];
          l2[q * R + r] = glen[x][(size_t)idx[q] * R + r];
        }
      }
      ghdr[x].swap(h2);
      grow[x].swap(r2);
      glen[x].swap(l2);
    }
  }
  lap("slices formed");
  int64_t bpx = 0;   // blocks (GLX_WPB slices) per XCD range
  for (int x = 0; x < NX; ++x) bpx = std::max<int64_t>(bpx, ((int64_t)ghdr[x].size() + GLX_WPB - 1) / GLX_WPB);
  const int64_t spx = bpx * GLX_WPB;
  const int64_t nslices = spx * NX;
  std::vector<SliceHdr> hdr(nslices);
  std::vector<int32_t> slot_row(nslices * R, -1), slot_len(nslices * R, 0);
  int64_t stored = 0;
  for (int x = 0; x < NX; ++x)
    for (int64_t s = 0; s < spx; ++s) {
      SliceHdr h;
      h.ptr = stored;
      h.nchunks = 0;
      h.S = 1;
      if (s < (int64_t)ghdr[x].size()) {
        h = ghdr[x][s];
        h.ptr = stored;
        for (int r = 0; r < R; ++r) {
          slot_row[(x * spx + s) * R + r] = grow[x][s * R + r];
          slot_len[(x * spx + s) * R + r] = glen[x][s * R + r];
        }
      }
      stored += (int64_t)(h.nchunks > 0 ? h.nchunks - 1 : 0) * 64;   // chunk 0 lives in the dense head arrays
      hdr[x * spx + s] = h;
    }
  // image = [head: chunk 0 of every slice, nslices*64 entries][tail: chunks 1.. at hdr.ptr], filled by sell_fill_kernel
  const int64_t head = nslices * 64;
  SellPlan p;
  p.G = G;
  p.R = R;
  p.relaxed = relaxed;
  p.nslices = nslices;
  p.stored = head + stored;
  p.head = head;
  const size_t es = g->dtype == GLX_F64 ? 8 : 4;
  GLX_POOL(glx_pool_alloc((void**)&p.d_slot_row, std::max<size_t>(4, slot_row.size() * 4)));
  GLX_POOL(glx_pool_alloc((void**)&p.d_slot_len, std::max<size_t>(4, slot_len.size() * 4)));
  GLX_POOL(glx_pool_alloc((void**)&p.d_slice_hdr, std::max<size_t>(16, hdr.size() * sizeof(SliceHdr))));
  GLX_POOL(glx_pool_alloc((void**)&p.d_col, std::max<size_t>(4, (head + stored) * 4)));
  GLX_POOL(glx_pool_alloc((void**)&p.d_val, std::max<size_t>(8, (head + stored) * es)));
  GlxCall call;                        // uploads and the fill run in a work set's stream (no blocking copies on the NULL stream)
  GLX_UP(call.begin(g->device));
  hipStream_t pst = call.stream();
  GLX_UP(glx_upload(p.d_slot_row, slot_row.data(), slot_row.size() * 4, pst, __func__));
  GLX_UP(glx_upload(p.d_slot_len, slot_len.data(), slot_len.size() * 4, pst, __func__));
  GLX_UP(glx_upload(p.d_slice_hdr, hdr.data(), hdr.size() * sizeof(SliceHdr), pst, __func__));
  if (nslices > 0) {
    // the CSR arrays as they are: resident on the device already (glx_graph_create_resident), or uploaded into work buffers of
    // this call
    int32_t *d_rp = g->d_src_rowptr, *d_cc = g->d_src_col;
    double* d_cv = g->d_src_val;
    if (!d_cc) {
      GLX_UP(call.alloc(&d_rp, (size_t)(n + 1)));
      GLX_UP(call.alloc(&d_cc, (size_t)g->nnz));
      GLX_UP(call.alloc(&d_cv, (size_t)g->nnz));
      GLX_UP(glx_upload(d_rp, g->h_rowptr.data(), (size_t)(n + 1) * 4, pst, __func__));
      if (g->nnz > 0) {
        GLX_UP(glx_upload(d_cc, g->h_col.data(), (size_t)g->nnz * 4, pst, __func__));
        GLX_UP(glx_upload(d_cv, g->h_val.data(), (size_t)g->nnz * 8, pst, __func__));
      }
    }
    const unsigned grid = (unsigned)((nslices + 3) / 4);
    if (g->dtype == GLX_F64)
      hipLaunchKernelGGL(sell_fill_kernel<double>, dim3(grid), dim3(256), 0, pst, (const int32_t*)d_rp, (const int32_t*)d_cc, (const double*)d_cv,
                         (const int32_t*)(renum ? g->d_perm : nullptr), (const int32_t*)(renum ? g->d_inv : nullptr), (const int32_t*)p.d_slot_row,
                         (const int32_t*)p.d_slot_len, (const SliceHdr*)p.d_slice_hdr, nslices, head, G, p.d_col, (double*)p.d_val,
                         (const double*)g->d_row_scale, g->reverse_rows ? 1 : 0);
    else
      hipLaunchKernelGGL(sell_fill_kernel<float>, dim3(grid), dim3(256), 0, pst, (const int32_t*)d_rp, (const int32_t*)d_cc, (const double*)d_cv,
                         (const int32_t*)(renum ? g->d_perm : nullptr), (const int32_t*)(renum ? g->d_inv : nullptr), (const int32_t*)p.d_slot_row,
                         (const int32_t*)p.d_slot_len, (const SliceHdr*)p.d_slice_hdr, nslices, head, G, p.d_col, (float*)p.d_val,
                         (const double*)g->d_row_scale, g->reverse_rows ? 1 : 0);
    GLX_HIP(hipGetLastError());
  }
  GLX_HIP(hipStreamSynchronize(pst));         // the host vectors of the plan may go; the pooled CSR copies go back when `call` ends
  lap("uploaded");
  g->plans.push_back(p);
  *out = &g->plans.back();
  return GLX_OK;
}
