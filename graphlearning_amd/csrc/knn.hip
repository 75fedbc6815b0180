// Exact k-nearest-neighbour search on the MI355X: weightmatrix.knnsearch of the reference
// (graphlearning/weightmatrix.py:297-429; kdtree branch :349-352 is the exact answer we
// reproduce).  Three stages:
//   1. candidate filter -- brute-force tiled pairwise squared distances as an (n x d) @ (d x n) contraction on the matrix
//      cores, refs staged through LDS: split-bf16 operands (knn_tile_bf16.h; d <= 128) or fp32 operands with the norms folded
//      in as two extra features (knn_tile_f32.h); every lane owns one query column and keeps the KP best of its half of the
//      refs of its range in a list (unsorted, maximum tracked);
//   2. exact re-rank (knn_rerank.hip) -- fp64 direct-difference distances (the accumulation pattern of scipy cKDTree's
//      sqeuclidean_distance_double) of the candidates, sorted by (distance, index); a row is accepted only if every candidate
//      list's threshold exceeds the exact k-th distance by twice a bound on the filter's error;
//   3. fallback -- rows that fail the check are redone by an exact fp64 scan.
// This file: one pass of the search (knn_pass: the stages of KnnPass in order, planned by knn_plan.h), the escalation to long lists,
// the C-ABI entry points.
#include "knn_internal.h"
#include <array>
#include <atomic>
#include <chrono>
#include <stdlib.h>
#include <unistd.h>
#include <vector>

// statistics of the calling thread's last search (glx_knn_stats)
static thread_local double g_knn_stats[KS_COUNT];
extern "C" int glx_knn_stats(double stats[16]) {
  GLX_CHECK(stats, GLX_EINVAL, "glx_knn_stats: null output");
  for (int i = 0; i < KS_COUNT; ++i) stats[i] = g_knn_stats[i];
  return GLX_OK;
}

// the calling thread's plan overrides (glx_knn_set_options; all zero / -1 = the library decides)
static thread_local glx_knn_options g_knn_opt = {0, 0, 0, -1};
extern "C" int glx_knn_set_options(const glx_knn_options* opt) {
  if (!opt) { g_knn_opt = {0, 0, 0, -1}; return GLX_OK; }
  GLX_CHECK(opt->filter >= 0 && opt->filter <= 2 && opt->lists >= 0 && opt->lists <= 2 && opt->nsplit >= 0 && opt->nsplit <= 32 &&
            opt->concat >= -1 && opt->concat <= 2, GLX_EINVAL, "glx_knn_set_options: value out of range");
  g_knn_opt = *opt;
  return GLX_OK;
}

// ---- debugging aid: is the device copy of X the caller's X? ------------------------------------------------------------------------
// glx_debug_set(flags): bit 0 (1) = after the upload of a search's features the device copy is read back TWICE -- by the copy engine, and through a
// kernel (i.e. through the L2s) -- and compared with the caller's array; differences are counted (glx_debug_counters) and described
// on stderr.  Round 6: the one parity failure of the randomised soak that left evidence was a search whose device copy of ONE row of X
// was not the caller's (EXPERIMENTS.md round 6, section 2).
static std::atomic<int> g_debug_flags{0};
static std::atomic<unsigned long long> g_debug_counts[4];   // uploads checked, uploads whose engine read-back differed, whose kernel read-back differed, bytes differing
extern "C" int glx_debug_set(int flags) { g_debug_flags = flags; return GLX_OK; }
extern "C" int glx_debug_counters(unsigned long long out[4]) {
  GLX_CHECK(out, GLX_EINVAL, "glx_debug_counters: null output");
  for (int q = 0; q < 4; ++q) out[q] = g_debug_counts[q].load();
  return GLX_OK;
}
__global__ __launch_bounds__(256) void knn_copy_u64_kernel(const unsigned long long* __restrict__ src, unsigned long long* __restrict__ dst, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = src[i];
}
static int knn_verify_upload(const double* X_host, const double* X_dev, int64_t n, int d, hipStream_t st, const char* what) {
  const size_t bytes = (size_t)n * d * 8;
  GLX_HIP(hipStreamSynchronize(st));
  // (read back INTO PAGE-LOCKED MEMORY: a copy into pageable memory can show the very holes this check looks for)
  unsigned long long* back = nullptr;
  GLX_HIP(hipHostMalloc((void**)&back, std::max<size_t>(bytes, 64), hipHostMallocDefault));
  struct Free { unsigned long long* p; ~Free() { hipHostFree(p); } } free_back{back};
  ++g_debug_counts[0];
  for (int pass = 0; pass < 2; ++pass) {
    GlxReadbackDiff diff;
    if (pass == 0) {
      GLX_UP(glx_compare_readback(X_host, X_dev, bytes, &diff, back));
    } else {
      void* tmp = nullptr;
      GLX_HIP(hipMalloc(&tmp, bytes));                  // (a fresh allocation, not a pooled block)
      hipLaunchKernelGGL(knn_copy_u64_kernel, dim3(1024), dim3(256), 0, st, (const unsigned long long*)X_dev, (unsigned long long*)tmp, (int64_t)(bytes / 8));
      hipError_t e = hipStreamSynchronize(st);
      const int rc = e == hipSuccess ? glx_compare_readback(X_host, tmp, bytes, &diff, back) : GLX_OK;
      hipFree(tmp);
      GLX_HIP(e);
      if (rc) return rc;
    }
    const unsigned long long* src = (const unsigned long long*)X_host;
    const size_t nbad = diff.bad, first = diff.first, last = diff.last;
    if (nbad) {
      ++g_debug_counts[1 + pass];
      g_debug_counts[3] += nbad * 8;
      fprintf(stderr, "[glx] knn DEBUG (%s, pid %d): the device copy of X read back by %s differs from the caller's array in %zu of %zu words: words %zu .. %zu "
                      "(rows %zu .. %zu of %lld, d = %d; byte offsets %zu .. %zu; device address %p; source address %p)\n", what, (int)getpid(),
              pass == 0 ? "the copy engine" : "a kernel (through the L2s)", nbad, bytes / 8, first, last, first / d, last / d, (long long)n, d, first * 8, last * 8 + 7,
              (const void*)X_dev, (const void*)X_host);
      if (pass == 0) {
        // what the wrong words hold: words of the SAME array from another place (a shifted or repeated piece), or nothing of it
        size_t shown = 0;
        for (size_t i = first; i <= last && shown < 6; ++i) {
          if (back[i] == src[i] || back[i] == 0) continue;
          long long at = -1;
          for (size_t j = 0; j < bytes / 8; ++j)
            if (src[j] == back[i]) { at = (long long)j; break; }
          fprintf(stderr, "[glx] knn DEBUG   word %zu: got %016llx (as a double %.6g), expected %016llx (%.6g); the value got %s%lld\n", i, back[i],
                  __builtin_bit_cast(double, back[i]), src[i], __builtin_bit_cast(double, src[i]),
                  at >= 0 ? "is word " : "occurs nowhere in the caller's array ", at);
          ++shown;
        }
        fprintf(stderr, "[glx] knn DEBUG   %zu of the wrong words are zero\n", diff.zeros);
      }
    }
  }
  return GLX_OK;
}

static const int KNN_ESCALATE = 1;    // knn_pass: too many rows failed the acceptance test of the short lists -- search again with long ones

// GLX_TIMING: the host's stage stamps on stderr
struct KnnStamp {
  bool on;
  std::chrono::steady_clock::time_point t0;
  void operator()(const char* what) const {
    if (on) fprintf(stderr, "[glx] knn: %-28s %.2f ms since the call\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
};

static int knn_check_args(const double* X, int64_t n, int d, int k, int64_t q0, int64_t q1, const int64_t* ind_out, const double* dist_out,
                          const glx_knn_result* capture) {
  GLX_CHECK(X && ((ind_out && dist_out) || capture), GLX_EINVAL, "glx_knn_bruteforce: null argument");
  GLX_CHECK(!capture || (q0 == 0 && q1 == n), GLX_EINVAL, "glx_knn_search: a result object holds a full search");
  GLX_CHECK(n >= 1 && d >= 1 && k >= 1, GLX_EINVAL, "glx_knn_bruteforce: need n, d, k >= 1 (n=%lld d=%d k=%d)", (long long)n, d, k);
  GLX_CHECK(k <= n, GLX_EINVAL, "glx_knn_bruteforce: k=%d exceeds the number of points %lld", k, (long long)n);
  GLX_CHECK(n < (1ll << 31) - BR_MAX, GLX_EINVAL, "glx_knn_bruteforce: n must fit int32");
  GLX_CHECK(0 <= q0 && q0 <= q1 && q1 <= n, GLX_EINVAL, "glx_knn_bruteforce: bad query range");
  GLX_CHECK(k <= KNN_K_MAX, GLX_EUNSUPPORTED, "glx_knn_search: k=%d (incl. self) above the supported %d", k, KNN_K_MAX);
  GLX_CHECK(d <= 16382, GLX_EUNSUPPORTED, "glx_knn_bruteforce: d=%d above the supported 16382", d);
  return GLX_OK;
}

// One pass of the search: the request, its plan, what it works on, and what a stage leaves for the next.  The stages run in the
// order of their declarations (knn_pass); each returns the library's status.
struct KnnPass {
  const double* X;
  int64_t n;
  int d, k;
  int64_t q0, q1, nq;
  int64_t* ind_out;
  double* dist_out;
  int device;
  bool long_lists;
  glx_knn_result* capture;
  const int64_t* cell_starts;   // the cells the rows come in: the caller's, or the ones form_cells made (b.own_starts)
  int ncells;
  KnnPlan p;
  KnnStamp stamp;
  KnnBufs b;
  hipStream_t st = nullptr;
  bool on_host = true;          // X is a host array (else a device pointer)
  bool perm_pending = false;    // b.orig goes to the result object
  // the host look at the device's counts (members: the copies into them are asynchronous)
  float h_rmax[2] = {0.f, 0.f};
  int h_nbad = 0;
  unsigned long long h_visited = 0;
  size_t nbad = 0;              // rows that failed the acceptance test (the list itself is on the device: b.rows)

  int launch_tile(int64_t c0, int64_t c1) {
    return p.use_bf16 ? knn_launch_tile_bf16(p.KP, p.NKB, b, n, c0, c1, p.nsplit, st, p.cat, false)
                      : knn_launch_tile_f32(p.KP, p.DH, p.nkb, b, n, c0, c1, p.nsplit, st);
  }

  // the work set (stream, events) and the features on the device
  int upload_features() {
    GLX_UP(glx_work_acquire(device, &b.work));
    b.stream = b.work->stream;
    b.e0 = b.work->ev[0]; b.e1 = b.work->ev[1]; b.e2 = b.work->ev[2]; b.e3 = b.work->ev[3];
    st = b.stream;
    GLX_POOL(glx_pool_alloc((void**)&b.X, (size_t)n * d * 8));
    GLX_POOL(glx_pool_alloc((void**)&b.mean, d * 8));
    stamp("stream, events, buffers");
    // (hipMemcpyDefault: X may also be a DEVICE pointer -- glx_knn_bruteforce_range / glx_knn_cells_range of the sharded build, whose
    // features are generated, ordered and kept on the GPU; the library-formed cells read sample rows on the host and need a host X)
    {
      hipPointerAttribute_t at;
      on_host = hipPointerGetAttributes(&at, X) != hipSuccess || (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged);
      (void)hipGetLastError();
    }
    if (on_host) {
      // the caller's (pageable) array goes up through the library's page-locked staging area, checked (glx_internal.h: why)
      GLX_UP(glx_upload(b.X, X, (size_t)n * d * 8, st, "features of a search"));
    } else {
      GLX_HIP(hipMemcpyAsync(b.X, X, (size_t)n * d * 8, hipMemcpyDefault, st));
    }
    stamp("X enqueued");
    if ((g_debug_flags & 1) && on_host) GLX_UP(knn_verify_upload(X, b.X, n, d, st, "after the upload"));
    return GLX_OK;
  }

  // Cells formed by the library (auto_cells).  > 1: that many cells (nearest of evenly spaced sample rows), the rows reordered by
  // cell and searched with the cell pruning of glx_knn_cells_range; the re-rank ranks by and returns the caller's indices.
  // < -1 (below the size where pruning pays): the rows ARE reordered by -auto_cells chained cells on the device and then searched
  // all pairs.  The 32 queries of a wavefront then come from one corner of feature space, a ref tile holds candidates for many of
  // them or for none, and fewer wave-tiles leave the tile kernel's fast path: config 2 2.06 -> 1.83 ms of search wall time, config
  // 3's shape 3.06 -> 2.63 ms, data without clusters unchanged (profiles/r03_knn_cells_midsize.txt).
  // Either way the cells are put in a chain of nearest centres (knn_chain_places), then the rows by cell (counting sort, ascending
  // caller index inside a cell).
  int form_cells(int auto_cells) {
    const bool reorder_only = auto_cells < -1;
    if (auto_cells < -1) auto_cells = -auto_cells;
    if (!(auto_cells > 1 && q0 == 0 && q1 == n && !long_lists && d <= 128 && n >= 4 * (int64_t)auto_cells)) return GLX_OK;
    const int m = auto_cells;
    b.oc_sample.resize(m);
    for (int c = 0; c < m; ++c) b.oc_sample[c] = (int)(((2 * (int64_t)c + 1) * n) / (2 * (int64_t)m));     // evenly spaced rows
    GLX_POOL(glx_pool_alloc((void**)&b.cen, (size_t)m * d * 8));
    GLX_POOL(glx_pool_alloc((void**)&b.cell_id, (size_t)std::max<int64_t>(n, m) * 4));
    GLX_UP(glx_upload(b.cell_id, b.oc_sample.data(), (size_t)m * 4, st, "knn_pass"));
    hipLaunchKernelGGL(knn_gather_rows_kernel, dim3((unsigned)(((int64_t)m * d + 255) / 256)), dim3(256), 0, st, (const double*)b.X, (const int*)b.cell_id,
                       (int64_t)m, d, b.cen);
    hipLaunchKernelGGL(knn_assign_kernel, dim3((unsigned)((4 * n + 255) / 256)), dim3(256), (size_t)16 * d * 8, st, (const double*)b.X, d, n, (const double*)b.cen, m,
                       b.cell_id, (d + 31) / 32);
    GLX_HIP(hipGetLastError());
    GLX_POOL(glx_pool_alloc((void**)&b.orig, (size_t)n * 4));
    GLX_UP(reorder_only ? order_cells_on_device(m) : order_cells_on_host(m));
    b.Xraw = b.X;
    b.X = nullptr;
    GLX_POOL(glx_pool_alloc((void**)&b.X, (size_t)n * d * 8));
    hipLaunchKernelGGL(knn_gather_rows_kernel, dim3((unsigned)((n * d + 255) / 256)), dim3(256), 0, st, (const double*)b.Xraw, (const int*)b.orig, n, d, b.X);
    GLX_HIP(hipGetLastError());
    stamp("rows reordered by cell");
    return GLX_OK;
  }

  // reorder only: the chain of the cells from the caller's copy of the sample rows (the same doubles the device gathered), the rows
  // into cell order by the three knn_cellrank kernels: nothing here waits for the device
  int order_cells_on_device(int m) {
    b.oc_cen.resize((size_t)m * d);
    for (int c = 0; c < m; ++c) memcpy(&b.oc_cen[(size_t)c * d], X + (size_t)b.oc_sample[c] * d, (size_t)d * 8);
    b.oc_place = knn_chain_places(b.oc_cen, m, d);
    const int nb = (int)((n + 255) / 256);
    GLX_POOL(glx_pool_alloc((void**)&b.place, (size_t)m * 4));
    GLX_POOL(glx_pool_alloc((void**)&b.bh, (size_t)(nb + 1) * m * 4));     // (+ one row: the keys' totals / starting positions)
    GLX_UP(glx_upload(b.place, b.oc_place.data(), (size_t)m * 4, st, "knn_pass"));
    hipLaunchKernelGGL(knn_cellrank_hist_kernel, dim3((unsigned)nb), dim3(256), (size_t)m * 4, st, b.cell_id, (const int*)b.place, n, m, b.bh);
    hipLaunchKernelGGL(knn_cellrank_scan_kernel, dim3((unsigned)m), dim3(256), 0, st, b.bh, nb, m);
    hipLaunchKernelGGL(knn_cellrank_base_kernel, dim3(1), dim3(256), 0, st, b.bh, nb, m);
    hipLaunchKernelGGL(knn_cellrank_scatter_kernel, dim3((unsigned)nb), dim3(256), 0, st, (const int*)b.cell_id, n, m, (const int*)b.bh, nb, b.orig);
    perm_pending = capture != nullptr;               // the permutation comes back with the results (glx_knn_result_order)
    return GLX_OK;
  }

  // the pruned search needs the cells' extents on the host: cell ids and centres come back, the rows are counted into chained
  // cells here (stable: ascending caller index inside a cell)
  int order_cells_on_host(int m) {
    b.oc_cid.resize(n);
    b.oc_cen.resize((size_t)m * d);
    GLX_UP(glx_download(b.oc_cid.data(), b.cell_id, (size_t)n * 4, st, "knn_pass"));
    GLX_UP(glx_download(b.oc_cen.data(), b.cen, (size_t)m * d * 8, st, "knn_pass"));
    GLX_HIP(hipStreamSynchronize(st));
    b.oc_place = knn_chain_places(b.oc_cen, m, d);
    std::vector<int64_t> fill(m + 1, 0);
    for (int64_t i = 0; i < n; ++i) { b.oc_cid[i] = b.oc_place[b.oc_cid[i]]; ++fill[b.oc_cid[i] + 1]; }
    for (int c = 0; c < m; ++c) fill[c + 1] += fill[c];
    b.own_starts.assign(fill.begin(), fill.begin() + m);
    b.oc_perm.resize(n);
    for (int64_t i = 0; i < n; ++i) b.oc_perm[fill[b.oc_cid[i]]++] = (int)i;
    GLX_UP(glx_upload(b.orig, b.oc_perm.data(), (size_t)n * 4, st, "knn_pass"));   // (no synchronisation behind it: b.oc_perm outlives the stream's work)
    if (capture) capture->order.assign(b.oc_perm.begin(), b.oc_perm.end());
    glx_pool_free(b.cen);                          // the cell pass allocates its own
    b.cen = nullptr;
    cell_starts = b.own_starts.data();
    ncells = m;
    return GLX_OK;
  }

  // centring in fp64 (distances are translation invariant; small norms keep the filter sharp), all of it on the device; then the
  // buffers of the lists
  int centre_and_alloc_lists() {
    const int64_t nb_sum = (n + CENTRE_ROWS - 1) / CENTRE_ROWS, nb_max = (n + 255) / 256;
    GLX_POOL(glx_pool_alloc((void**)&b.part, (size_t)std::max<int64_t>(nb_sum * d, nb_max) * 8));
    GLX_POOL(glx_pool_alloc((void**)&b.rmax, 64));
    int dt = 1;
    while (dt < d && dt < 256) dt *= 2;
    hipLaunchKernelGGL(knn_colsum_kernel, dim3((unsigned)nb_sum), dim3(256), 0, st, (const double*)b.X, n, d, dt, b.part);
    GLX_HIP(hipGetLastError());
    hipLaunchKernelGGL(knn_mean_kernel, dim3(1), dim3(256), 0, st, (const double*)b.part, nb_sum, d, n, b.mean);
    hipLaunchKernelGGL(knn_maxnorm_kernel, dim3((unsigned)nb_max), dim3(256), 0, st, (const double*)b.X, (const double*)b.mean, n, d, b.part);
    hipLaunchKernelGGL(knn_rmax_kernel, dim3(1), dim3(256), 0, st, (const double*)b.part, nb_max, b.rmax);
    GLX_HIP(hipGetLastError());
    // the candidate lists of a chunk of queries, the flags and thresholds of all, the lists that are returned
    GLX_POOL(glx_pool_alloc((void**)&b.qnorm, (size_t)n * 4));
    GLX_POOL(glx_pool_alloc((void**)&b.cand_d, (size_t)p.chunk * p.ncand * 4));
    GLX_POOL(glx_pool_alloc((void**)&b.cand_i, (size_t)p.chunk * p.ncand * 4));
    GLX_POOL(glx_pool_alloc((void**)&b.flags, (size_t)nq * 4));
    GLX_POOL(glx_pool_alloc((void**)&b.dk2, (size_t)nq * 8));
    GLX_POOL(glx_pool_alloc((void**)&b.nbad, 4));
    GLX_HIP(hipMemsetAsync(b.nbad, 0, 4, st));
    GLX_POOL(glx_pool_alloc((void**)&b.gtau, (size_t)nq * 4));
    GLX_HIP(hipMemsetD32Async((hipDeviceptr_t)b.gtau, 0x7f800000, (size_t)nq, st));   // +inf: nothing published yet
    GLX_POOL(glx_pool_alloc((void**)&b.rows, (size_t)nq * 4));
    GLX_POOL(glx_pool_alloc((void**)&b.ind, (size_t)nq * k * 8));
    GLX_POOL(glx_pool_alloc((void**)&b.dist, (size_t)nq * k * 8));
    stamp("centred, norms bounded");
    GLX_HIP(hipEventRecord(b.e0, st));
    return GLX_OK;
  }

  // the filter's operand images; for rows that come in cells (bf16 filter, lists that can hold k: knn_seed_plan) the cell pruning
  int prepare_operands() {
    g_knn_stats[KS_CONCAT] = (double)p.cat;      // (0 on the fp32 filter, which has no concatenated form: not the previous search's value)
    if (!p.use_bf16) {
      GLX_POOL(glx_pool_alloc((void**)&b.Rf, (size_t)n * p.dpa * 4));
      GLX_POOL(glx_pool_alloc((void**)&b.Qf, (size_t)n * p.dpa * 4));
      hipLaunchKernelGGL(knn_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const double*)b.X, (const double*)b.mean,
                         (const float*)b.rmax, n, d, p.dpa, b.Rf, b.Qf, b.qnorm);
      GLX_HIP(hipGetLastError());
      return GLX_OK;
    }
    GLX_POOL(glx_pool_alloc((void**)&b.Xb, (size_t)(n + KNN_PAD_ROWS) * 2 * p.dpa * 2));
    GLX_POOL(glx_pool_alloc((void**)&b.nrm, (size_t)(n + KNN_PAD_ROWS) * 4));
    if (p.cat) {
      GLX_POOL(glx_pool_alloc((void**)&b.Xq, (size_t)(n + KNN_PAD_ROWS) * 64 * 2));
      hipLaunchKernelGGL(knn_prep_bf16_cat_kernel, dim3((unsigned)((n + KNN_PAD_ROWS + 255) / 256)), dim3(256), 0, st, (const double*)b.X,
                         (const double*)b.mean, (const float*)b.rmax, n, d, b.Xb, b.Xq, b.nrm, b.qnorm, p.cat == 2 ? 1 : 0);
    } else {
      hipLaunchKernelGGL(knn_prep_bf16_kernel, dim3((unsigned)((n + KNN_PAD_ROWS + 255) / 256)), dim3(256), 0, st, (const double*)b.X, (const double*)b.mean,
                         (const float*)b.rmax, n, d, p.dpa, b.Xb, b.nrm, b.qnorm);
    }
    GLX_HIP(hipGetLastError());
    const KnnSeedPlan seed = knn_seed_plan(p, k, cell_starts ? ncells : 0);
    g_knn_stats[KS_SEED_SAMPLE] = seed.seeded ? (double)seed.sub : 0.0;
    g_knn_stats[KS_VISITED_SHARE] = 0.0;
    g_knn_stats[KS_CELLS] = 0.0;
    return seed.seeded ? seed_from_cells(seed.sub) : GLX_OK;
  }

  // the cell-pruned search: centres and radii of the cells, the seeding pre-pass over every seed_sub-th tile of a query block's own
  // cells, the cells each block has to visit (knn_cellmask_kernel) as runs of tiles
  int seed_from_cells(int seed_sub) {
    const int64_t nqb = p.nqb;
    GLX_POOL(glx_pool_alloc((void**)&b.cell_starts, (size_t)ncells * 8));
    GLX_POOL(glx_pool_alloc((void**)&b.cen, (size_t)ncells * d * 8));
    GLX_POOL(glx_pool_alloc((void**)&b.rad, (size_t)ncells * 8));
    GLX_POOL(glx_pool_alloc((void**)&b.ub2, (size_t)nq * 8));
    GLX_POOL(glx_pool_alloc((void**)&b.mask, (size_t)nqb * ncells));
    GLX_POOL(glx_pool_alloc((void**)&b.nruns, (size_t)nqb * 4));
    b.maxruns = ncells;
    GLX_POOL(glx_pool_alloc((void**)&b.runs, (size_t)nqb * 2 * ncells * 4));   // (from here on the tile launches follow the runs)
    GLX_UP(glx_upload(b.cell_starts, cell_starts, (size_t)ncells * 8, st, "knn_pass"));
    // centres and radii of the cells
    GLX_POOL(glx_pool_alloc((void**)&b.cpart, (size_t)ncells * CELL_SPLIT * (d + 1) * 8));
    double* prad = b.cpart + (size_t)ncells * CELL_SPLIT * d;
    hipLaunchKernelGGL(knn_cell_sum_kernel, dim3((unsigned)ncells, CELL_SPLIT), dim3(256), 0, st, (const double*)b.X, d, (const int64_t*)b.cell_starts, n,
                       ncells, b.cpart);
    hipLaunchKernelGGL(knn_cell_centre_kernel, dim3((unsigned)ncells), dim3(256), 0, st, (const double*)b.cpart, d, (const int64_t*)b.cell_starts, n, ncells,
                       b.cen);
    hipLaunchKernelGGL(knn_cell_rad_kernel, dim3((unsigned)ncells, CELL_SPLIT), dim3(256), (size_t)(d + 256) * 8, st, (const double*)b.X, d,
                       (const int64_t*)b.cell_starts, n, ncells, (const double*)b.cen, prad);
    hipLaunchKernelGGL(knn_cell_radfin_kernel, dim3((unsigned)((ncells + 255) / 256)), dim3(256), 0, st, (const double*)prad,
                       (const int64_t*)b.cell_starts, n, ncells, b.rad);
    hipLaunchKernelGGL(knn_runs_kernel, dim3((unsigned)((nqb + 255) / 256)), dim3(256), 0, st, (const unsigned char*)nullptr,
                       (const int64_t*)b.cell_starts, n, ncells, p.BR, q0, q1, nqb, b.maxruns, b.runs, b.nruns, (unsigned long long*)nullptr);
    GLX_HIP(hipGetLastError());
    GLX_POOL(glx_pool_alloc((void**)&b.pre_d, (size_t)nq * 2 * p.KP * 4));
    GLX_POOL(glx_pool_alloc((void**)&b.pre_i, (size_t)nq * 2 * p.KP * 4));
    GLX_UP(knn_launch_tile_bf16(p.KP, p.NKB, b, n, q0, q1, seed_sub, st, p.cat, true));
    GLX_UP(knn_launch_seed(p.KP, b, nq, q0, k, p.cerr, st));
    hipLaunchKernelGGL(knn_cellmask_kernel, dim3((unsigned)nqb), dim3(256), (size_t)16 * d * 8, st, (const double*)b.X, d, q0, q1, (const double*)b.cen,
                       (const double*)b.rad, ncells, (const double*)b.ub2, b.mask);
    GLX_POOL(glx_pool_alloc((void**)&b.visited, 8));
    GLX_HIP(hipMemsetAsync(b.visited, 0, 8, st));
    hipLaunchKernelGGL(knn_runs_kernel, dim3((unsigned)((nqb + 255) / 256)), dim3(256), 0, st, (const unsigned char*)b.mask,
                       (const int64_t*)b.cell_starts, n, ncells, p.BR, q0, q1, nqb, b.maxruns, b.runs, b.nruns, b.visited);
    GLX_HIP(hipGetLastError());
    g_knn_stats[KS_CELLS] = (double)ncells;
    return GLX_OK;
  }

  // filter + re-rank, in one go or (wide) chunk by chunk
  int filter_and_rerank() {
    if (!p.wide) {
      GLX_UP(launch_tile(q0, q1));
      GLX_HIP(hipEventRecord(b.e1, st));
      GLX_UP(knn_launch_rerank(b, n, d, k, q0, nq, p.lists, p.KP, p.M, p.cerr, st));
      GLX_HIP(hipEventRecord(b.e2, st));
      return GLX_OK;
    }
    // chunk by chunk: filter, re-rank (flags, dk2 and the flagged rows are numbered within the pass, the lists go to their final rows).
    // Every chunk's stage boundaries have events of their own, read once the stream has drained: the host never waits between chunks.
    hipEvent_t start = b.e0;
    for (int64_t c0 = q0; c0 < q1; c0 += p.chunk) {
      const int64_t c1 = std::min(q1, c0 + p.chunk);
      if (c0 > q0) GLX_HIP(hipMemsetD32Async((hipDeviceptr_t)b.gtau, 0x7f800000, (size_t)(c1 - c0), st));   // (the filter's thresholds are per chunk row)
      GLX_UP(launch_tile(c0, c1));
      hipEvent_t et = b.e1, er = b.e2;                 // (the last chunk ends on the pass's own events: the fallback is timed from e2)
      if (c1 < q1) {
        GLX_HIP(hipEventCreate(&et));
        b.chunk_ev.push_back(et);
        GLX_HIP(hipEventCreate(&er));
        b.chunk_ev.push_back(er);
      }
      GLX_HIP(hipEventRecord(et, st));
      GLX_UP(knn_launch_rerank_wide(b, n, d, k, q0, c0, c1 - c0, p.lists, p.KP, p.M, p.cerr, st));
      GLX_HIP(hipEventRecord(er, st));
      b.chunk_marks.push_back({start, et, er});
      start = er;
    }
    return GLX_OK;
  }

  // the host's look at the pass: rows that failed the acceptance test, the centring pass's verdict on the input, the pruning's share;
  // KNN_ESCALATE if repairing the failed rows one by one would cost more than searching again with the long lists
  int host_look() {
    GLX_HIP(hipMemcpyAsync(&h_nbad, b.nbad, 4, hipMemcpyDeviceToHost, st));
    GLX_HIP(hipMemcpyAsync(h_rmax, b.rmax, 8, hipMemcpyDeviceToHost, st));
    if (b.visited) GLX_HIP(hipMemcpyAsync(&h_visited, b.visited, 8, hipMemcpyDeviceToHost, st));
    GLX_HIP(hipStreamSynchronize(st));
    if (b.visited) {
      g_knn_stats[KS_VISITED_SHARE] = (double)h_visited / ((double)p.nqb * (double)p.ntiles);
      if (stamp.on) fprintf(stderr, "[glx] knn: cell pruning, %d cells: %.1f %% of the (query block, ref tile) pairs visited\n", ncells, 100.0 * g_knn_stats[KS_VISITED_SHARE]);
    }
    stamp("tile + re-rank done, flags on the host");
    GLX_CHECK(h_rmax[1] == 1.0f, GLX_EINVAL, "glx_knn_bruteforce: non-finite input");   // (the first host look at the centring pass)
    nbad = (size_t)h_nbad;
    if (knn_should_escalate(p, n, d, k, nq, nbad, b.visited ? g_knn_stats[KS_VISITED_SHARE] : 1.0)) {
      g_knn_stats[KS_FALLBACK_ROWS] = (double)nbad;
      return KNN_ESCALATE;
    }
    return GLX_OK;
  }

  // the rows that failed the acceptance test redone exactly
  int fallback() {
    const size_t nr = nbad;
    if (nr && p.wide) {
      const KnnWideFallbackPlan f = knn_wide_fallback_plan(k, nr);
      GLX_POOL(glx_pool_alloc((void**)&b.fb_pd, f.batch * FB_SPLIT * k * 8));
      GLX_POOL(glx_pool_alloc((void**)&b.fb_pi, f.batch * FB_SPLIT * k * 4));
      GLX_POOL(glx_pool_alloc((void**)&b.fb_cnt, f.batch * 2 * 4));
      GLX_POOL(glx_pool_alloc((void**)&b.fb_bd, f.batch * f.cap * 8));
      GLX_POOL(glx_pool_alloc((void**)&b.fb_bi, f.batch * f.cap * 4));
      for (size_t r0 = 0; r0 < nr; r0 += f.batch) GLX_UP(knn_launch_fallback_wide(b, n, d, k, q0, b.rows + r0, std::min(f.batch, nr - r0), f.cap, st));
    } else if (nr) {
      GLX_POOL(glx_pool_alloc((void**)&b.fb_pd, nr * FB_SPLIT * k * 8));
      GLX_POOL(glx_pool_alloc((void**)&b.fb_pi, nr * FB_SPLIT * k * 4));
      GLX_POOL(glx_pool_alloc((void**)&b.fb_cnt, nr * 2 * 4));            // [nr] counts, [nr] redo marks
      GLX_POOL(glx_pool_alloc((void**)&b.fb_bd, nr * FB_CAP * 8));
      GLX_POOL(glx_pool_alloc((void**)&b.fb_bi, nr * FB_CAP * 4));
      GLX_HIP(hipMemsetAsync(b.fb_cnt, 0, nr * 2 * 4, st));
      const int* fb_runs = (const int*)(b.visited ? b.runs : nullptr);   // (b.runs: the main pass's runs when the search was cell-pruned -- the pre-pass's were overwritten by them)
      GLX_UP(knn_launch_fallback(b, n, d, k, q0, nr, fb_runs, p.BR, st));
    }
    GLX_HIP(hipEventRecord(b.e3, st));
    return GLX_OK;
  }

  // the lists to the caller's arrays, or (capture) handed to the result object together with the cell order; the statistics
  int finish() {
    if (ind_out) GLX_UP(glx_download(ind_out, b.ind, (size_t)nq * k * 8, st, "knn_pass"));
    if (dist_out) GLX_UP(glx_download(dist_out, b.dist, (size_t)nq * k * 8, st, "knn_pass"));
    GLX_HIP(hipStreamSynchronize(st));
    stamp("results on the host");
    if (perm_pending) {    // the permutation stays on the device with the result (glx_knn_result_order copies it into the caller's --
      glx_pool_free(capture->order_dev);      // page-locked -- array: a synchronous copy into fresh pageable memory cost 8 ms here)
      capture->order_dev = b.orig;
      b.orig = nullptr;
    }
    if (capture) {         // the lists stay on the device with the caller's result object (everything that writes them has finished)
      glx_pool_free(capture->ind);
      glx_pool_free(capture->dist);
      capture->ind = b.ind;
      capture->dist = b.dist;
      capture->n = n;
      capture->k = k;
      capture->device = device;
      b.ind = nullptr;
      b.dist = nullptr;
    }
    float ms_tile = 0, ms_rr = 0, ms_fb = 0;
    GLX_HIP(hipEventElapsedTime(&ms_tile, b.e0, b.e1));
    GLX_HIP(hipEventElapsedTime(&ms_rr, b.e1, b.e2));
    GLX_HIP(hipEventElapsedTime(&ms_fb, b.e2, b.e3));
    if (p.wide) {                // (the sum over the chunks; a later chunk's filter time includes the reset of the thresholds)
      ms_tile = ms_rr = 0;
      for (const auto& m : b.chunk_marks) {
        float t = 0, r = 0;
        GLX_HIP(hipEventElapsedTime(&t, m[0], m[1]));
        GLX_HIP(hipEventElapsedTime(&r, m[1], m[2]));
        ms_tile += t;
        ms_rr += r;
      }
    }
    g_knn_stats[KS_TILE_MS] = ms_tile;
    g_knn_stats[KS_RERANK_MS] = ms_rr;
    g_knn_stats[KS_FALLBACK_ROWS] = (double)nbad;
    g_knn_stats[KS_TOTAL_MS] = ms_tile + ms_rr + ms_fb;
    g_knn_stats[KS_FALLBACK_MS] = ms_fb;
    g_knn_stats[KS_DPA] = (double)p.dpa;
    g_knn_stats[KS_NSPLIT] = (double)p.nsplit;
    g_knn_stats[KS_KP] = p.use_bf16 ? -(double)p.KP : (double)p.KP;
    g_knn_stats[KS_CHUNKS] = (double)p.nchunks;
    g_knn_stats[KS_WIDE] = p.wide ? 1.0 : 0.0;
    g_knn_stats[KS_CANDIDATES] = (double)p.ncand;
    return GLX_OK;
  }
};
// One pass of the search.  long_lists = false: the default (short lists where they apply); if then so many query rows fail
// the acceptance test that repairing them row by row -- each streams the whole data set -- would take longer than
// searching again, KNN_ESCALATE is returned: the caller repeats the search with the long lists (one list
// holds all k neighbours of a query, whatever their arrangement in the data).  It takes data whose k nearest neighbours
// sit in the same 16 of 32 consecutive points to get there (tight groups stored one after another); interleaving the ref tiles
// over the ranges already spreads anything coarser.
// capture (full searches: glx_knn_search): the lists stay on the device with this result object, together with the cell order
// the pass worked out (if it did), instead of being copied out.
static int knn_pass(const double* X, int64_t n, int d, int k, int64_t q0, int64_t q1, int64_t* ind_out, double* dist_out, int device,
                    bool long_lists, glx_knn_result* capture, const int64_t* cell_starts = nullptr, int ncells = 0, int auto_cells = 0) {
  GLX_UP(knn_check_args(X, n, d, k, q0, q1, ind_out, dist_out, capture));
  const int64_t nq = q1 - q0;
  if (nq == 0) return GLX_OK;
  const KnnStamp stamp = {getenv("GLX_TIMING") != nullptr, std::chrono::steady_clock::now()};
  GLX_HIP(hipSetDevice(device));
  KnnPass s = {X, n, d, k, q0, q1, nq, ind_out, dist_out, device, long_lists, capture, cell_starts, ncells,
               knn_make_plan(n, d, k, nq, long_lists, g_knn_opt), stamp};
  GLX_UP(s.upload_features());
  GLX_UP(s.form_cells(auto_cells));
  GLX_UP(s.centre_and_alloc_lists());
  GLX_UP(s.prepare_operands());
  GLX_UP(s.filter_and_rerank());
  GLX_UP(s.host_look());             // (KNN_ESCALATE included)
  GLX_UP(s.fallback());
  return s.finish();
}

static int knn_run(const double* X, int64_t n, int d, int k, int64_t q0, int64_t q1, int64_t* ind_out, double* dist_out, int device,
                   glx_knn_result* capture = nullptr, const int64_t* cell_starts = nullptr, int ncells = 0, int auto_cells = 0) {
  g_knn_stats[KS_ESCALATED_ROWS] = 0.0;
  g_knn_stats[KS_SEED_SAMPLE] = g_knn_stats[KS_VISITED_SHARE] = g_knn_stats[KS_CELLS] = 0.0;
  int rc = knn_pass(X, n, d, k, q0, q1, ind_out, dist_out, device, false, capture, cell_starts, ncells, auto_cells);
  if (rc != KNN_ESCALATE) return rc;
  const double flagged = g_knn_stats[KS_FALLBACK_ROWS];
  g_knn_stats[KS_SEED_SAMPLE] = g_knn_stats[KS_VISITED_SHARE] = g_knn_stats[KS_CELLS] = 0.0;
  if (capture) { capture->order.clear(); glx_pool_free(capture->order_dev); capture->order_dev = nullptr; }
  rc = knn_pass(X, n, d, k, q0, q1, ind_out, dist_out, device, true, capture);     // (long lists: the fp32-input kernel, all refs)
  g_knn_stats[KS_ESCALATED_ROWS] = flagged;            // rows the first (short-list) pass could not accept
  return rc;
}

extern "C" int glx_knn_bruteforce(const double* X, int64_t n, int d, int k, int similarity, int64_t* ind_out, double* dist_out,
                                  int device) {
  GLX_CHECK(similarity == 0, GLX_EINVAL,
            "glx_knn_bruteforce: similarity %d; only euclidean (0) -- normalise rows on the host for angular", similarity);
  GLX_CHECK(k <= KNN_K_NARROW, GLX_EUNSUPPORTED, "glx_knn_bruteforce: k=%d (incl. self) above the supported %d (glx_knn_search takes up to %d)", k,
            KNN_K_NARROW, KNN_K_MAX);
  return knn_run(X, n, d, k, 0, n, ind_out, dist_out, device);
}

extern "C" int glx_knn_bruteforce_range(const double* X, int64_t n, int d, int k, int64_t q_begin, int64_t q_end,
                                        int64_t* ind_out, double* dist_out, int device) {
  GLX_CHECK(k <= KNN_K_NARROW, GLX_EUNSUPPORTED, "glx_knn_bruteforce_range: k=%d (incl. self) above the supported %d", k, KNN_K_NARROW);
  return knn_run(X, n, d, k, q_begin, q_end, ind_out, dist_out, device);
}

// The same search -- the same lists, bit for bit -- for rows that come in a coarse geometric order: cell c = the rows
// [cell_starts[c], cell_starts[c + 1]) (the last cell ends at n; empty cells allowed).  Per query block only the cells that can hold
// one of its k nearest are visited (bounds from the cells' centres and radii against the k-th distance within a sample of the
// block's own cells); everything skipped is strictly farther than the k-th neighbour.  Takes the place of the tree the reference
// searches with (scipy cKDTree / annoy, graphlearning/weightmatrix.py:297-429) at sizes where all pairs are too many.
extern "C" int glx_knn_cells_range(const double* X, int64_t n, int d, int k, const int64_t* cell_starts, int ncells, int64_t q_begin,
                                   int64_t q_end, int64_t* ind_out, double* dist_out, int device) {
  GLX_CHECK(cell_starts && ncells >= 1, GLX_EINVAL, "glx_knn_cells_range: null argument");
  GLX_CHECK(k <= KNN_K_NARROW, GLX_EUNSUPPORTED, "glx_knn_cells_range: k=%d (incl. self) above the supported %d", k, KNN_K_NARROW);
  GLX_CHECK(ncells <= 4096, GLX_EUNSUPPORTED, "glx_knn_cells_range: %d cells above the supported 4096", ncells);
  GLX_CHECK(cell_starts[0] == 0, GLX_EINVAL, "glx_knn_cells_range: the first cell must start at row 0");
  for (int c = 1; c < ncells; ++c)
    GLX_CHECK(cell_starts[c] >= cell_starts[c - 1] && cell_starts[c] <= n, GLX_EINVAL, "glx_knn_cells_range: cell starts must ascend within [0, n]");
  return knn_run(X, n, d, k, q_begin, q_end, ind_out, dist_out, device, nullptr, cell_starts, ncells);
}

// All n rows in the caller's order, the cells formed here: ncells evenly spaced rows serve as centres, every row joins the
// nearest one, the rows are reordered by cell on the device and searched with the pruning of glx_knn_cells_range; indices and
// output rows are the caller's, ties between equal distances go to the lower caller index -- the lists of glx_knn_bruteforce,
// bit for bit.  On data without cluster structure every cell stays in play and the extra passes cost a few per cent.
// ncells < -1: the rows reordered by -ncells chained cells, then all pairs (coherent wavefronts below the size where pruning pays).
extern "C" int glx_knn_clustered(const double* X, int64_t n, int d, int k, int ncells, int64_t* ind_out, double* dist_out, int device) {
  GLX_CHECK(ncells >= -4096 && ncells <= 4096, GLX_EINVAL, "glx_knn_clustered: ncells=%d outside [-4096, 4096]", ncells);
  GLX_CHECK(k <= KNN_K_NARROW, GLX_EUNSUPPORTED, "glx_knn_clustered: k=%d (incl. self) above the supported %d", k, KNN_K_NARROW);
  return knn_run(X, n, d, k, 0, n, ind_out, dist_out, device, nullptr, nullptr, 0, ncells);
}

// ---- search results as objects -------------------------------------------------------------------------------------------------
// glx_knn_search runs the full search (every row a query) and leaves the lists ON THE DEVICE in a result object the caller owns:
// glx_knn_result_to_csr (assemble.hip) builds the weight matrix from them without a host round trip, glx_knn_result_lists copies
// them out, glx_knn_result_order returns the cell order the search worked out (if it did: contiguous, chained cells of feature
// space -- on clustered data as good a locality order for the graph's operators as the library's own pass over the graph,
// glx_graph_set_order, and free), glx_knn_result_destroy releases everything.  Nothing is handed from one call to the next through
// hidden state.
extern "C" int glx_knn_search(const double* X, int64_t n, int d, int k, int ncells, int device, glx_knn_result** out) {
  GLX_CHECK(out, GLX_EINVAL, "glx_knn_search: null output");
  *out = nullptr;
  GLX_CHECK(ncells >= -4096 && ncells <= 4096, GLX_EINVAL, "glx_knn_search: ncells=%d outside [-4096, 4096]", ncells);
  GLX_CHECK(k <= KNN_K_MAX, GLX_EUNSUPPORTED, "glx_knn_search: k=%d (incl. self) above the supported %d", k, KNN_K_MAX);
  glx_knn_result* res = new glx_knn_result();
  const auto t_call = std::chrono::steady_clock::now();
  const int rc = knn_run(X, n, d, k, 0, n, nullptr, nullptr, device, res, nullptr, 0, (ncells > 1 || ncells < -1) ? ncells : 0);
  if (getenv("GLX_TIMING"))
    fprintf(stderr, "[glx] knn: search returns after %.2f ms (work buffers released)\n",
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count());
  if (rc || !res->ind) {
    glx_knn_result_destroy(res);
    if (!rc) glx_set_error("glx_knn_search: the search left no lists behind");
    return rc ? rc : GLX_EINVAL;
  }
  *out = res;
  return GLX_OK;
}

extern "C" int glx_knn_result_lists(const glx_knn_result* res, int64_t* ind_out, double* dist_out) {
  GLX_CHECK(res && res->ind && res->dist, GLX_EINVAL, "glx_knn_result_lists: empty result");
  GLX_HIP(hipSetDevice(res->device));
  const size_t bytes = (size_t)res->n * res->k * 8;
  if (ind_out) GLX_UP(glx_download_sync(ind_out, res->ind, bytes, __func__));
  if (dist_out) GLX_UP(glx_download_sync(dist_out, res->dist, bytes, __func__));
  return GLX_OK;
}

__global__ __launch_bounds__(256) void knn_copy_i32_kernel(const int32_t* __restrict__ src, int32_t* __restrict__ dst, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

extern "C" int glx_knn_result_order(const glx_knn_result* res, int32_t* perm_out) {
  GLX_CHECK(res && perm_out, GLX_EINVAL, "glx_knn_result_order: null argument");
  if (res->order_dev) {
    GLX_HIP(hipSetDevice(res->device));
    // Page-locked destinations (what _hip.KnnResult.order passes) are written by a kernel: the first copy-engine transfer after the
    // search's allocations took 8 ms (measured: hipMemcpy and hipMemcpyAsync alike, 0.02 ms on every later call), a kernel's
    // stores into mapped host memory 0.03 ms.
    glx_work* w = nullptr;
    int rcw = glx_work_acquire(res->device, &w);
    if (rcw) return rcw;
    void* dev_view = nullptr;
    hipError_t e;
    if (hipHostGetDevicePointer(&dev_view, perm_out, 0) == hipSuccess && dev_view) {
      hipLaunchKernelGGL(knn_copy_i32_kernel, dim3((unsigned)((res->n + 255) / 256)), dim3(256), 0, w->stream, (const int32_t*)res->order_dev,
                         (int32_t*)dev_view, res->n);
      e = hipGetLastError();
    } else {
      (void)hipGetLastError();
      e = hipMemcpyAsync(perm_out, res->order_dev, (size_t)res->n * 4, hipMemcpyDeviceToHost, w->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(w->stream);
    glx_work_release(w);
    GLX_HIP(e);
    return GLX_OK;
  }
  GLX_CHECK((int64_t)res->order.size() == res->n && res->n > 0, GLX_EINVAL, "glx_knn_result_order: this search worked out no cell order");
  memcpy(perm_out, res->order.data(), (size_t)res->n * 4);
  return GLX_OK;
}

extern "C" int glx_knn_result_destroy(glx_knn_result* res) {
  if (!res) return GLX_OK;
  glx_pool_free(res->ind);
  glx_pool_free(res->dist);
  glx_pool_free(res->order_dev);
  delete res;
  return GLX_OK;
}

