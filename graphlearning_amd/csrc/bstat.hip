// utils.boundary_statistic on the device (glx_boundary_stat): the boundary test of Calder, Park and Slepcev over the rows of a
// canonical CSR pattern with unit weights -- the ball graph of weightmatrix.epsilon_ball or the directed kNN graph of weightmatrix.knn.
// The arithmetic is that of bstat_plan.h, operation by operation, and the host restatement there (bstat_host) IS the result.
//
// Stages, one launch each, nothing between them but the kernel boundary:
//   recip     a_j = 1.0 / deg_j                                                             a thread per vertex
//   dp        dp_i, the chain of step 2 (descending columns) or 3                           a thread per vertex
//   raw       y[i, c], the sequential chain of steps 2 / 3                                  a thread per (vertex, coordinate)
//   unit      norm_i = sqrt(np.sum(y_i * y_i)), nu[i, :] = y[i, :] / norm_i, in place;      a thread per vertex
//             the lowest vertex whose norm is zero or not finite goes into a flag word (an integer atomicMin)
// unit and stat exist in two instantiations: up to 128 coordinates numpy's row sum is one leaf of eight accumulators, above it the
// split walked with a stack (bstat_rowsum); the narrow form carries no stack and no scratch memory.
//   stat      T_i: a group of lanes per row, the lanes striding the row's members (step 5 is independent per member), the maximum
//             reduced across the group with shuffles, steps 6 - 8 in lane 0.  Two launches at most: the rows of the short class
//             (BSTAT_SHORT_LANES lanes each, four rows to a wavefront) and the rows that take a wavefront.
// The host reads the flag word before it downloads anything: a bad norm is GLX_EINVAL naming the vertex, nothing else happened.
//
// What the code guarantees.
// 1. A pure function of the inputs.  The chains run in the order the contract names, one thread each; the sums over coordinates are
//    npsum_terms; the only cross-lane operation is the maximum (and the farthest member of a full row, a maximum under a total
//    order), which does not depend on the order of its operands; NaN and the sign of zero are settled after it (bstat_finish).  No
//    floating-point atomic, no grid-wide wait.
// 2. No out-of-range access.  bstat_check (host) walks the pattern and the lists before the first upload: row pointers from 0 to nnz
//    and ascending, every column and list index in [0, n), no empty row.  Every offset a kernel forms is 64-bit.
// 3. Buffers come from the pools (GlxCall), transfers go through glx_upload / glx_download.
#include "glx_internal.h"
#include "bstat_plan.h"
#include <chrono>
#include <new>
#include <vector>

namespace {
thread_local int t_wave_row = 0;          // glx_boundary_stat_set_wave_row: 0 = BSTAT_WAVE_ROW
}

__global__ __launch_bounds__(256) void bstat_recip_kernel(const int32_t* __restrict__ indptr, int64_t n, double* __restrict__ a) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < n) a[j] = 1.0 / (double)(indptr[j + 1] - indptr[j]);
}

__global__ __launch_bounds__(256) void bstat_dp_kernel(const int32_t* __restrict__ indptr, const int32_t* __restrict__ col,
                                                       const double* __restrict__ a, int64_t n, int second_order, double* __restrict__ dp) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dp[i] = bstat_dp(col, indptr[i], indptr[i + 1], a, second_order);
}

__global__ __launch_bounds__(256) void bstat_raw_kernel(const double* __restrict__ X, int d, const int32_t* __restrict__ indptr,
                                                        const int32_t* __restrict__ col, const double* __restrict__ a,
                                                        const double* __restrict__ dp, int64_t n, int second_order, double* __restrict__ y) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n * d) return;
  const int64_t i = t / d;
  const int c = (int)(t - i * d);
  y[t] = bstat_raw(X, d, col, indptr[i], indptr[i + 1], a, (int32_t)i, c, dp[i], second_order);
}

// WIDE: d > 128, the row sums walk numpy's split with a stack; otherwise they are one leaf (bstat_rowsum)
template <bool WIDE>
__global__ __launch_bounds__(256) void bstat_unit_kernel(double* __restrict__ y, int d, int64_t n, unsigned long long* first_bad) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double* row = y + (size_t)i * d;
  const double norm = sqrt(bstat_norm2<WIDE>(row, d));
  if (!(norm > 0.0) || !(norm < __builtin_inf())) atomicMin(first_bad, (unsigned long long)i);
  for (int c = 0; c < d; ++c) row[c] = row[c] / norm;
}

// G lanes per listed row.  indptr null: the kNN mode, the members of vertex i are J[i * k .. i * k + k).
template <int G, bool WIDE>
__global__ __launch_bounds__(256) void bstat_stat_kernel(const double* __restrict__ X, const double* __restrict__ nu, int d,
                                                         const int32_t* __restrict__ indptr, const int32_t* __restrict__ members, int k,
                                                         int64_t maxdeg, int flags, const int32_t* __restrict__ rows, int64_t nrows,
                                                         double* __restrict__ T) {
  const int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
  const int lane = threadIdx.x % G;
  const bool live = g < nrows;
  int32_t i = 0;
  const int32_t* mem = members;
  int64_t len = 0;
  if (live) {
    i = rows[g];
    if (indptr) {
      mem = members + indptr[i];
      len = indptr[i + 1] - indptr[i];
    } else {
      mem = members + (size_t)i * k;
      len = k;
    }
  }
  const bool full = indptr && len == maxdeg;        // (uniform in the group)
  int32_t drop = -1;
  double best = -1.0;                               // (a squared distance is never below 0)
  if (full) {
    for (int64_t e = lane; e < len; e += G) {
      const int32_t j = mem[e];
      const double sq = sqdist_exact(X + (size_t)i * d, X + (size_t)j * d, d);
      if (bstat_farther(sq, j, best, drop)) {
        best = sq;
        drop = j;
      }
    }
  }
  // every lane of the wavefront takes part in the shuffles; a group never reads outside itself
  if (__any(full)) {
#pragma unroll
    for (int s = G / 2; s >= 1; s >>= 1) {
      const double o_sq = __shfl_xor(best, s, G);
      const int32_t o_j = __shfl_xor(drop, s, G);
      if (bstat_farther(o_sq, o_j, best, drop)) {
        best = o_sq;
        drop = o_j;
      }
    }
    if (!full) drop = -1;
  }
  double mx = -__builtin_inf();
  int nan = 0;
  for (int64_t e = lane; e < len; e += G) {
    const int32_t j = mem[e];
    if (j != drop) bstat_max_in(bstat_term<WIDE>(X, nu, d, i, j, flags), &mx, &nan);
  }
#pragma unroll
  for (int s = G / 2; s >= 1; s >>= 1) {
    const double o = __shfl_xor(mx, s, G);
    nan |= __shfl_xor(nan, s, G);
    if (o > mx) mx = o;
  }
  if (live && lane == 0) T[i] = bstat_finish(mx, nan, bstat_adds_zero(len, maxdeg, indptr != nullptr));
}

extern "C" int glx_boundary_stat_set_wave_row(int min_members) {
  GLX_CHECK(min_members >= 0, GLX_EINVAL, "glx_boundary_stat_set_wave_row: %d is negative", min_members);
  t_wave_row = min_members;
  return GLX_OK;
}

// (the host vectors of the checks and of the row lists may throw: the entry point below catches)
static int bstat_run(int64_t n, int d, const double* X, int64_t nnz, const int32_t* indptr, const int32_t* indices, int k, const int32_t* J,
                     int flags, double* T, double* nu, double* stats_out, int device) {
  GLX_CHECK(X && indptr && indices && T && nu, GLX_EINVAL, "glx_boundary_stat: null argument");
  GLX_CHECK((flags & ~(BSTAT_SECOND_ORDER | BSTAT_CUTOFF)) == 0, GLX_EINVAL, "glx_boundary_stat: unknown flags %d", flags);
  auto ms_since = [](std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  };
  double ms[4] = {0, 0, 0, 0};      // checks, upload, kernels, download
  auto t0 = std::chrono::steady_clock::now();
  char why[200];
  int64_t maxdeg = 0;
  GLX_CHECK(bstat_check(n, d, indptr, indices, nnz, k, J, &maxdeg, why, sizeof why) == 0, GLX_EINVAL, "glx_boundary_stat: %s", why);
  // the rows by class: the short ones first, then those that take a wavefront
  const int wave_row = t_wave_row > 0 ? t_wave_row : BSTAT_WAVE_ROW;
  std::vector<int32_t> rows((size_t)n);
  int64_t nshort = 0, nfull = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t len = J ? k : indptr[i + 1] - indptr[i];
    nshort += bstat_row_lanes(len, wave_row) != 64;
    nfull += !J && len == maxdeg;
  }
  {
    int64_t s = 0, w = nshort;
    for (int64_t i = 0; i < n; ++i) {
      const int64_t len = J ? k : indptr[i + 1] - indptr[i];
      rows[bstat_row_lanes(len, wave_row) != 64 ? s++ : w++] = (int32_t)i;
    }
  }
  ms[0] = ms_since(t0);

  GlxCall call;
  GLX_UP(call.begin(device));
  hipStream_t st = call.stream();
  t0 = std::chrono::steady_clock::now();
  const size_t nd = (size_t)n * d;
  double *d_X = nullptr, *d_a = nullptr, *d_dp = nullptr, *d_nu = nullptr, *d_T = nullptr;
  int32_t *d_indptr = nullptr, *d_indices = nullptr, *d_J = nullptr, *d_rows = nullptr;
  unsigned long long *d_flag = nullptr, *h_flag = nullptr;
  GLX_UP(call.put(&d_X, X, nd, __func__));
  GLX_UP(call.put(&d_indptr, indptr, (size_t)n + 1, __func__));
  GLX_UP(call.put(&d_indices, indices, (size_t)nnz, __func__));
  if (J) GLX_UP(call.put(&d_J, J, (size_t)n * k, __func__));
  GLX_UP(call.put(&d_rows, (const int32_t*)rows.data(), (size_t)n, __func__));
  GLX_UP(call.alloc(&d_a, (size_t)n));
  GLX_UP(call.alloc(&d_dp, (size_t)n));
  GLX_UP(call.alloc(&d_nu, nd));
  GLX_UP(call.alloc(&d_T, (size_t)n));
  GLX_UP(call.alloc(&d_flag, 1));
  GLX_UP(call.stage(&h_flag, 1));
  h_flag[0] = ~0ull;
  GLX_HIP(hipMemcpyAsync(d_flag, h_flag, 8, hipMemcpyHostToDevice, st));
  GLX_HIP(hipStreamSynchronize(st));
  ms[1] = ms_since(t0);

  t0 = std::chrono::steady_clock::now();
  int launches = 0;
  const unsigned grid_n = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(bstat_recip_kernel, dim3(grid_n), dim3(256), 0, st, (const int32_t*)d_indptr, n, d_a);
  GLX_HIP(hipGetLastError());
  hipLaunchKernelGGL(bstat_dp_kernel, dim3(grid_n), dim3(256), 0, st, (const int32_t*)d_indptr, (const int32_t*)d_indices, (const double*)d_a, n,
                     flags & BSTAT_SECOND_ORDER, d_dp);
  GLX_HIP(hipGetLastError());
  hipLaunchKernelGGL(bstat_raw_kernel, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, st, (const double*)d_X, d, (const int32_t*)d_indptr,
                     (const int32_t*)d_indices, (const double*)d_a, (const double*)d_dp, n, flags & BSTAT_SECOND_ORDER, d_nu);
  GLX_HIP(hipGetLastError());
  const bool wide = d > 128;
  if (wide)
    hipLaunchKernelGGL(bstat_unit_kernel<true>, dim3(grid_n), dim3(256), 0, st, d_nu, d, n, d_flag);
  else
    hipLaunchKernelGGL(bstat_unit_kernel<false>, dim3(grid_n), dim3(256), 0, st, d_nu, d, n, d_flag);
  GLX_HIP(hipGetLastError());
  launches += 4;
  const int32_t* d_ptr_or_null = J ? nullptr : d_indptr;
  const int32_t* d_members = J ? d_J : d_indices;
  if (nshort > 0) {
    constexpr int per_block = 256 / BSTAT_SHORT_LANES;
    auto kernel = wide ? bstat_stat_kernel<BSTAT_SHORT_LANES, true> : bstat_stat_kernel<BSTAT_SHORT_LANES, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((nshort + per_block - 1) / per_block)), dim3(256), 0, st, (const double*)d_X,
                       (const double*)d_nu, d, d_ptr_or_null, d_members, k, maxdeg, flags, (const int32_t*)d_rows, nshort, d_T);
    GLX_HIP(hipGetLastError());
    ++launches;
  }
  if (n - nshort > 0) {
    auto kernel = wide ? bstat_stat_kernel<64, true> : bstat_stat_kernel<64, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n - nshort + 3) / 4)), dim3(256), 0, st, (const double*)d_X, (const double*)d_nu, d,
                       d_ptr_or_null, d_members, k, maxdeg, flags, (const int32_t*)d_rows + nshort, n - nshort, d_T);
    GLX_HIP(hipGetLastError());
    ++launches;
  }
  // (the flag word: 8 bytes from and to the work set's page-locked staging area -- far below the 128 KB from which glx_upload and
  // glx_download stage and check a transfer, and what they would do with it themselves)
  GLX_HIP(hipMemcpyAsync(h_flag, d_flag, 8, hipMemcpyDeviceToHost, st));
  GLX_HIP(hipStreamSynchronize(st));
  ms[2] = ms_since(t0);
  GLX_CHECK(h_flag[0] == ~0ull, GLX_EINVAL,
            "glx_boundary_stat: the normal of vertex %llu has norm zero or not finite (its neighbours balance, as on a lattice)", h_flag[0]);

  t0 = std::chrono::steady_clock::now();
  GLX_UP(glx_download(T, d_T, (size_t)n * 8, st, __func__));
  GLX_UP(glx_download(nu, d_nu, nd * 8, st, __func__));
  GLX_HIP(hipStreamSynchronize(st));
  ms[3] = ms_since(t0);
  if (stats_out) {
    stats_out[0] = launches;
    stats_out[1] = (double)nshort;
    stats_out[2] = (double)(n - nshort);
    stats_out[3] = (double)nfull;
    for (int q = 0; q < 4; ++q) stats_out[4 + q] = ms[q];
  }
  return GLX_OK;
}

extern "C" int glx_boundary_stat(int64_t n, int d, const double* X, int64_t nnz, const int32_t* indptr, const int32_t* indices, int k,
                                 const int32_t* J, int flags, double* T, double* nu, double* stats_out, int device) {
  try {
    return bstat_run(n, d, X, nnz, indptr, indices, k, J, flags, T, nu, stats_out, device);
  } catch (const std::bad_alloc&) {            // no exception crosses the C boundary
    glx_set_error("glx_boundary_stat: out of host memory (n=%lld nnz=%lld)", (long long)n, (long long)nnz);
    return GLX_ENOMEM;
  }
}
