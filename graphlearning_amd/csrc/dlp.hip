// Dynamic label propagation (Wang, Tu and Tsotsos, ICCV 2013; the reference's ssl.dynamic_label_propagation, ssl.py:1263-1343) without
// the dense n x n array, in one device call, reached through ssl.dynamic_label_propagation / _hip.dlp_solve.  The contract -- the
// unrolled recursion Pt_t X = P (Pt_{t-1} (P^T X)) + alpha v_{t-1} (v_{t-1}^T X) + lam X, every operation rounded on its own, the order
// of every sum -- is written down in dlp_plan.h and DESIGN.md 4.17 and walked on the host by dlp_host_reference; this file is that
// order on the device, bit for bit.
//
// Three kernels.  The sparse pass serves P and P^T alike: one thread per (vertex, column), columns fastest, a workgroup = FS_ROWS rows
// times one tile of at most DLP_TILE columns; a thread walks its row's entries alone and in stored order (a row of 3 000 entries is
// 3 000 dependent additions of one thread: the chain is the contract), the lanes of a row read consecutive doubles of each gathered
// record.  With an epilogue it reads the finished Gram G (k * k doubles) into LDS and leaves (s + alpha * g) + lam * X; on the last pass
// of a step it sets the training rows back to val.  The Gram pass leaves the (partials, k * k) array: a workgroup holds the FS_ROWS rows
// of one partial of X (all k columns) and of one column tile of V in LDS, column by column, and every wavefront adds DLP_GRAM_U products
// side by side across its 64 lanes by fs_wave_tree64.  The finishing kernel adds the partials of FS_FIN_COLS entries per workgroup in
// the order of fs_finish (fs_finish_cols).  No floating-point atomic, nothing depends on which workgroup ends first, the kernel
// boundary is the only synchronisation, and the host reads nothing back between the steps.
#include "glx_internal.h"
#include "dlp_plan.h"
#include "fixed_sum_device.h"
#include <vector>

#define DLP_GRAM_THREADS 256
#define DLP_GRAM_U 8                       // trees side by side per wavefront
#define DLP_GRAM_LD (FS_ROWS + 1)          // doubles between two columns of a tile in LDS: no two columns of a row on one bank

// out = spmm(A, X) for the tile's columns; EPI: out = (spmm + alpha * (v G)) + lam * Xe with G (k, k) finished by the kernel before.
// lab (or null): rows with lab[i] >= 0 are set to val[lab[i]] instead; raw (or null) receives the value before that.
template <bool EPI>
__global__ __launch_bounds__(FS_ROWS * DLP_TILE) void dlp_pass_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ col,
                                                                       const double* __restrict__ A, const double* __restrict__ X,
                                                                       double* __restrict__ out, double* __restrict__ raw,
                                                                       const double* __restrict__ v, const double* __restrict__ G,
                                                                       const double* __restrict__ Xe, double alpha, double lam,
                                                                       const int32_t* __restrict__ lab, const double* __restrict__ val,
                                                                       int64_t n, int k, int ct, int tbase, int textra) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double s_G[];          // EPI: k * k doubles
  if constexpr (EPI) {
    for (int q = threadIdx.x; q < k * k; q += blockDim.x) s_G[q] = G[q];
    __syncthreads();
  }
  const int r = (int)threadIdx.x / ct, c = (int)threadIdx.x - r * ct;
  const ColTile tl = col_tile_at((int)blockIdx.y, tbase, textra);
  const int c0 = tl.c0, cols = tl.cols;
  const int64_t i = (int64_t)blockIdx.x * FS_ROWS + r;
  if (i >= n || c >= cols) return;
  const int b = c0 + c;
  double s = 0.0;
  const int64_t e1 = ptr[i + 1];
  for (int64_t e = ptr[i]; e < e1; ++e) {
    const double pr = A[e] * X[(int64_t)col[e] * k + b];
    s = s + pr;
  }
  if constexpr (EPI) {
    double g = 0.0;
    for (int cc = 0; cc < k; ++cc) {
      const double pr = v[i * k + cc] * s_G[cc * k + b];
      g = g + pr;
    }
    const double ag = alpha * g;
    const double s1 = s + ag;
    const double lx = lam * Xe[i * k + b];
    s = s1 + lx;
  }
  if (raw) raw[i * k + b] = s;
  if (lab) {
    const int32_t q = lab[i];
    if (q >= 0) s = val[(int64_t)q * k + b];
  }
  out[i * k + b] = s;
}

// part[p, c * k + b] = the tree over the rows of partial p of V[i, c] * X[i, b], for the columns c of the tile blockIdx.y
__global__ __launch_bounds__(DLP_GRAM_THREADS) void dlp_gram_kernel(const double* __restrict__ V, const double* __restrict__ X,
                                                                     double* __restrict__ part, int64_t n, int k, int ct, int tbase,
                                                                     int textra) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double s_t[];          // X: k columns, then V: ct columns, DLP_GRAM_LD doubles each
  double* s_x = s_t;
  double* s_v = s_t + (size_t)k * DLP_GRAM_LD;
  const ColTile tl = col_tile_at((int)blockIdx.y, tbase, textra);
  const int c0 = tl.c0, cols = tl.cols;
  const int64_t p = blockIdx.x, i0 = p * FS_ROWS;
  // rows past n count as +0.0
  for (int q = threadIdx.x; q < FS_ROWS * k; q += DLP_GRAM_THREADS) {
    const int r = q / k, b = q - r * k;
    s_x[b * DLP_GRAM_LD + r] = i0 + r < n ? X[(i0 + r) * k + b] : 0.0;
  }
  for (int q = threadIdx.x; q < FS_ROWS * cols; q += DLP_GRAM_THREADS) {
    const int r = q / cols, c = q - r * cols;
    s_v[c * DLP_GRAM_LD + r] = i0 + r < n ? V[(i0 + r) * k + c0 + c] : 0.0;
  }
  __syncthreads();
  const int lane = (int)threadIdx.x % FS_ROWS, wave = (int)threadIdx.x / FS_ROWS;
  for (int c = wave; c < cols; c += DLP_GRAM_THREADS / FS_ROWS) {
    const double vc = s_v[c * DLP_GRAM_LD + lane];
    for (int b0 = 0; b0 < k; b0 += DLP_GRAM_U) {
      double a[DLP_GRAM_U];
#pragma unroll
      for (int q = 0; q < DLP_GRAM_U; ++q) a[q] = b0 + q < k ? vc * s_x[(b0 + q) * DLP_GRAM_LD + lane] : 0.0;
      fs_wave_tree64(a);
      if (lane == 0) {
#pragma unroll
        for (int q = 0; q < DLP_GRAM_U; ++q)
          if (b0 + q < k) part[p * k * k + (int64_t)(c0 + c) * k + b0 + q] = a[q];
      }
    }
  }
}

// G[j] = fs_finish of entry j of part (P, nq), FS_FIN_COLS entries per workgroup
__global__ __launch_bounds__(FS_FIN_THREADS) void dlp_gram_finish_kernel(const double* __restrict__ part, int64_t P, int nq,
                                                                          double* __restrict__ G) {
#pragma clang fp contract(off)
  __shared__ double s_a[FS_FIN_THREADS];
  const int j0 = blockIdx.x * FS_FIN_COLS, j = j0 + (int)threadIdx.x % FS_FIN_COLS;
  const double s = fs_finish_cols(part, P, nq, j0, s_a);
  if ((int)threadIdx.x < FS_FIN_COLS && j < nq) G[j] = s;
}

// u0: val on the training rows, zero elsewhere
__global__ __launch_bounds__(256) void dlp_start_kernel(double* __restrict__ u, const int32_t* __restrict__ lab, const double* __restrict__ val,
                                                        int64_t n, int k) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n * k) return;
  const int64_t i = t / k;
  const int32_t q = lab[i];
  u[t] = q >= 0 ? val[(int64_t)q * k + (t - i * k)] : 0.0;
}

extern "C" int glx_dlp_solve(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* col, const double* P, int k, int64_t m,
                             const int32_t* ind, const double* val, double alpha, double lam, int64_t T, double* u, double* hist,
                             int64_t* plan_out, int device) {
  GLX_CHECK(row_ptr && (M <= 0 || (col && P)) && (m <= 0 || (ind && val)) && u, GLX_EINVAL, "glx_dlp_solve: null argument");
  {
    char msg[256];
    const int bad = dlp_validate(n, M, row_ptr, col, P, k, m, ind, alpha, lam, T, msg, sizeof msg);
    GLX_CHECK(!bad, bad == 9 ? GLX_EUNSUPPORTED : GLX_EINVAL, "glx_dlp_solve: %s", msg);
  }
  DlpPlan plan;
  dlp_make_plan(n, M, row_ptr, col, P, k, m, ind, T, &plan);
  const size_t nk = (size_t)n * k;
  const int kk = k * k;

  GlxCall call;
  GLX_UP(call.begin(device));
  hipStream_t st = call.stream();
  int64_t *d_ptr = nullptr, *d_tptr = nullptr;
  int32_t *d_col = nullptr, *d_tcol = nullptr, *d_lab = nullptr;
  double *d_p = nullptr, *d_tp = nullptr, *d_val = nullptr, *d_work = nullptr, *d_hist = nullptr, *d_part = nullptr, *d_G = nullptr;
  GLX_UP(call.put(&d_ptr, row_ptr, (size_t)(n + 1), __func__));
  GLX_UP(call.put(&d_col, col, (size_t)M, __func__));
  GLX_UP(call.put(&d_p, P, (size_t)M, __func__));
  GLX_UP(call.put(&d_tptr, (const int64_t*)plan.tptr.data(), (size_t)(n + 1), __func__));
  GLX_UP(call.put(&d_tcol, (const int32_t*)plan.tcol.data(), (size_t)M, __func__));
  GLX_UP(call.put(&d_tp, (const double*)plan.tval.data(), (size_t)M, __func__));
  GLX_UP(call.put(&d_lab, (const int32_t*)plan.lab.data(), (size_t)n, __func__));
  GLX_UP(call.put(&d_val, val, (size_t)m * k, __func__));
  // the workspace, (2 T + 2) blocks of n k values: two iterates (with hist: u_0 only, the others live in the history), v_0 .. v_{T-2},
  // Y_1 .. Y_{T-1}, and the two buffers R_s alternates between
  GLX_UP(call.alloc(&d_work, (size_t)plan.work));
  if (hist) GLX_UP(call.alloc(&d_hist, (size_t)T * nk));
  GLX_UP(call.alloc(&d_part, (size_t)plan.P * kk));
  GLX_UP(call.alloc(&d_G, (size_t)kk));
  double* const d_V = d_work + 2 * nk;
  double* const d_Y = d_V + (size_t)(T - 1) * nk;           // Y_j at d_Y + (j - 1) n k
  double* const d_R = d_Y + (size_t)(T - 1) * nk;
  auto iterate = [&](int64_t t) { return t > 0 && d_hist ? d_hist + (size_t)(t - 1) * nk : d_work + (size_t)(t & 1) * nk; };

  const int tbase = k / plan.ntiles, textra = k % plan.ntiles;          // what col_tile_at (csr_plan.h) takes
  const dim3 grid((unsigned)plan.P, (unsigned)plan.ntiles), blk((unsigned)(FS_ROWS * plan.ct));
  const size_t gram_lds = (size_t)(k + plan.ct) * DLP_GRAM_LD * 8;
  int64_t launches = 0, sparse = 0, grams = 0;
  // out = spmm(A, X), training rows reset when `reset`, the value before the reset to `raw` (or null)
  auto product = [&](bool transposed, const double* X, double* out, double* raw, bool reset) -> int {
    hipLaunchKernelGGL(dlp_pass_kernel<false>, grid, blk, 0, st, (const int64_t*)(transposed ? d_tptr : d_ptr),
                       (const int32_t*)(transposed ? d_tcol : d_col), (const double*)(transposed ? d_tp : d_p), X, out, raw,
                       (const double*)nullptr, (const double*)nullptr, (const double*)nullptr, alpha, lam,
                       (const int32_t*)(reset ? d_lab : nullptr), (const double*)d_val, n, k, plan.ct, tbase, textra);
    GLX_HIP(hipGetLastError());
    ++launches;
    ++sparse;
    return GLX_OK;
  };

  hipLaunchKernelGGL(dlp_start_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st, iterate(0), (const int32_t*)d_lab,
                     (const double*)d_val, n, k);
  GLX_HIP(hipGetLastError());
  ++launches;
  for (int64_t t = 0; t < T; ++t) {
    const double* ut = iterate(t);
    double* unext = iterate(t + 1);
    if (t == 0) {          // R_0 = v_0, computed once: u_1 is its copy with the training rows reset
      GLX_UP(product(false, ut, unext, T >= 2 ? d_V : nullptr, true));
      continue;
    }
    if (t <= T - 2) GLX_UP(product(false, ut, d_V + (size_t)t * nk, nullptr, false));
    for (int64_t j = 1; j <= t; ++j) GLX_UP(product(true, j == 1 ? ut : d_Y + (size_t)(j - 2) * nk, d_Y + (size_t)(j - 1) * nk, nullptr, false));
    GLX_UP(product(false, d_Y + (size_t)(t - 1) * nk, d_R, nullptr, false));
    for (int64_t s = 0; s < t; ++s) {
      const int64_t j = t - 1 - s;
      const double* X = j == 0 ? ut : d_Y + (size_t)(j - 1) * nk;
      const double* v = d_V + (size_t)s * nk;
      const double* Rs = d_R + (size_t)(s & 1) * nk;
      const bool last = s == t - 1;
      double* Rn = last ? unext : d_R + (size_t)((s + 1) & 1) * nk;
      hipLaunchKernelGGL(dlp_gram_kernel, grid, dim3(DLP_GRAM_THREADS), gram_lds, st, v, X, d_part, n, k, plan.ct, tbase, textra);
      GLX_HIP(hipGetLastError());
      hipLaunchKernelGGL(dlp_gram_finish_kernel, dim3((unsigned)((kk + FS_FIN_COLS - 1) / FS_FIN_COLS)), dim3(FS_FIN_THREADS), 0, st,
                         (const double*)d_part, plan.P, kk, d_G);
      GLX_HIP(hipGetLastError());
      hipLaunchKernelGGL(dlp_pass_kernel<true>, grid, blk, (size_t)kk * 8, st, (const int64_t*)d_ptr, (const int32_t*)d_col,
                         (const double*)d_p, Rs, Rn, (double*)nullptr, v, (const double*)d_G, X, alpha, lam,
                         (const int32_t*)(last ? d_lab : nullptr), (const double*)d_val, n, k, plan.ct, tbase, textra);
      GLX_HIP(hipGetLastError());
      launches += 3;
      ++sparse;
      ++grams;
    }
  }
  GLX_UP(glx_download(u, iterate(T), nk * 8, st, __func__));
  if (hist) GLX_UP(glx_download(hist, d_hist, (size_t)T * nk * 8, st, __func__));
  GLX_HIP(hipStreamSynchronize(st));
  if (plan_out) {
    plan_out[0] = launches;
    plan_out[1] = sparse;
    plan_out[2] = grams;
    plan_out[3] = plan.P;
  }
  return GLX_OK;
}
