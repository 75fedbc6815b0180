// The centered-kernel learner of Mai and Couillet (ICML 2018) in one device call: the power iteration for the largest eigenvalue of
// C W C and the fixed-point iteration u <- u + ((1 / alpha) C W C u - u) off the training rows, the loop of the reference's
// ssl.centered_kernel (ssl.py:1346-1426), reached through ssl.centered_kernel / _hip.ck_solve.  The contract -- the one-pass form
// C W C u = W u - d (x) m - 1 (x) yb, every operation rounded on its own, the stop -- is written down in ck_plan.h and DESIGN.md 4.11,
// the reduction order in fixed_sum.h, and both are walked on the host by ck_host_reference; this file is that loop on the device,
// bit for bit.
//
// Two kernels per iteration with an ordinary kernel boundary between them (1.5-1.9 us; a cooperative grid-wide wait costs 26 us or
// more, so there is none).  The pass: one thread per (vertex, column), columns fastest, a workgroup = the FS_ROWS rows of one partial
// times one tile of at most CK_TILE columns.  A thread walks its row's entries alone and in stored order, the lanes of a row read
// consecutive doubles of each gathered record; the iterate goes into the other of two buffers because the gathers read other rows.
// The workgroup adds its rows' u' and c u' by the tree of fs_tree64 in LDS (ck_tree) and leaves one partial per column, and the
// maximum of |w| as a bit pattern.  The finishing kernel, ONE workgroup, adds the partials in the order of fs_finish (fs_finish_cols
// of fixed_sum_device.h) and leaves m, yb and the iteration's err slot -- no workgroup of the pass reads all partials, no
// floating-point atomic anywhere, nothing depends on which workgroup ends first.  The power iteration is the same pair of kernels
// with one column and five sums.
//
// The host enqueues chunks of CK_CHUNK iterations, reads the chunk's err slots once and decides (CkStops).  Both kernels first look at
// the slot of the iteration before theirs, so whatever was enqueued behind the stop changes nothing.  Buffers come from the pool and
// are written before they are read; no launch sequence is captured.
#include "glx_internal.h"
#include "ck_plan.h"
#include "fixed_sum_device.h"
#include <algorithm>
#include <vector>

// the workgroup's NQ sums over its FS_ROWS rows, thread (r, c) of a tile `ct` columns wide holding v[]: the tree of fs_tree64
// (fixed_sum.h) in this kernel's own LDS layout.  s: NQ * FS_ROWS * ct doubles of LDS.  The result is valid in the threads of row 0.
template <int NQ>
__device__ __forceinline__ void ck_tree(double* v, double* s, int r, int c, int ct) {
#pragma clang fp contract(off)
  const int at = r * ct + c, plane = FS_ROWS * ct;
#pragma unroll
  for (int j = 0; j < NQ; ++j) s[j * plane + at] = v[j];
  for (int h = FS_ROWS / 2; h >= 1; h >>= 1) {
    __syncthreads();
    if (r < h) {
#pragma unroll
      for (int j = 0; j < NQ; ++j) s[j * plane + at] = s[j * plane + at] + s[j * plane + at + h * ct];
    }
  }
  if (r == 0) {
#pragma unroll
    for (int j = 0; j < NQ; ++j) v[j] = s[j * plane + at];
  }
}

// pst: nrm, m, yb of the vector x (read), l and 1 / alpha (written by the finishing kernel); part (P, 5): e.w, e.e, w.w, 1.w, c.w
__global__ __launch_bounds__(FS_ROWS) void ck_power_pass_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                                 const double* __restrict__ W, const double* __restrict__ d,
                                                                 const double* __restrict__ cs, const double* __restrict__ x,
                                                                 double* __restrict__ xout, const double* __restrict__ pst,
                                                                 double* __restrict__ part, int64_t n) {
#pragma clang fp contract(off)
  __shared__ double s_t[5 * FS_ROWS];
  const int r = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * FS_ROWS + r;
  double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (i < n) {
    const double nrm = pst[0], mean = pst[1], yb = pst[2];
    double s = 0.0;
    const int64_t e1 = row_ptr[i + 1];
    for (int64_t e = row_ptr[i]; e < e1; ++e) {
      const double ej = x[col[e]] / nrm;
      const double pr = W[e] * ej;
      s = s + pr;
    }
    const double ei = x[i] / nrm;
    const double t1 = d[i] * mean;
    const double y1 = s - t1;
    const double w = y1 - yb;
    xout[i] = w;
    v[0] = ei * w;
    v[1] = ei * ei;
    v[2] = w * w;
    v[3] = w;
    v[4] = cs[i] * w;
  }
  ck_tree<5>(v, s_t, r, 0, 1);
  if (r == 0) {
#pragma unroll
    for (int j = 0; j < 5; ++j) part[(int64_t)blockIdx.x * 5 + j] = v[j];
  }
}

// iteration of slot r: reads uin, mst = m[k], yb[k]; writes uout, part (P, 2 k) and perr (P, ntiles)
__global__ __launch_bounds__(FS_ROWS * CK_TILE) void ck_pass_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                                     const double* __restrict__ W, const double* __restrict__ d,
                                                                     const double* __restrict__ cs, const int32_t* __restrict__ lab,
                                                                     const double* __restrict__ uin, double* __restrict__ uout,
                                                                     const double* __restrict__ mst, const double* __restrict__ pst,
                                                                     double* __restrict__ part, unsigned long long* __restrict__ perr,
                                                                     int64_t n, int k, int ct, int tbase, int textra,
                                                                     const double* __restrict__ slots, int r_slot, double tol) {
#pragma clang fp contract(off)
  extern __shared__ double s_dyn[];          // 2 * FS_ROWS * ct doubles
  __shared__ unsigned long long s_e;
  if (ck_stopped(slots[r_slot - 1], tol)) return;          // the iteration before was the last one
  const int r = (int)threadIdx.x / ct, c = (int)threadIdx.x - r * ct;
  const int tile = blockIdx.y;
  const ColTile tl = col_tile_at(tile, tbase, textra);
  const int c0 = tl.c0, cols = tl.cols;
  const int64_t i = (int64_t)blockIdx.x * FS_ROWS + r;
  if (threadIdx.x == 0) s_e = 0ull;
  double v[2] = {0.0, 0.0};
  unsigned long long eb = 0ull;
  const bool live = i < n && c < cols;
  const int b = c0 + c;
  if (live) {
    double s = 0.0;
    const int64_t e1 = row_ptr[i + 1];
    for (int64_t e = row_ptr[i]; e < e1; ++e) {
      const double pr = W[e] * uin[(int64_t)col[e] * k + b];
      s = s + pr;
    }
    const double ui = uin[i * k + b];
    const double t1 = d[i] * mst[b];
    const double y1 = s - t1;
    const double y2 = y1 - mst[k + b];
    const double sv = pst[4] * y2;
    double w = sv - ui;
    if (lab[i] >= 0) w = 0.0;
    const double un = ui + w;
    uout[i * k + b] = un;
    v[0] = un;
    v[1] = cs[i] * un;
    eb = (unsigned long long)__double_as_longlong(fabs(w));
  }
  ck_tree<2>(v, s_dyn, r, c, ct);            // (its first barrier also orders s_e = 0 before the maxima)
  if (eb) atomicMax(&s_e, eb);
  if (r == 0 && c < cols) {
    part[(int64_t)blockIdx.x * 2 * k + b] = v[0];
    part[(int64_t)blockIdx.x * 2 * k + k + b] = v[1];
  }
  __syncthreads();
  if (threadIdx.x == 0) perr[(int64_t)blockIdx.x * gridDim.y + tile] = s_e;
}

// the sums of the nq columns of part (P, nq) into s_sum, FS_FIN_COLS of them per round; s_sum may be read when it returns
__device__ __forceinline__ void ck_finish_sums(const double* __restrict__ part, int64_t P, int nq, double* s_a, double* s_sum) {
#pragma clang fp contract(off)
  for (int j0 = 0; j0 < nq; j0 += FS_FIN_COLS) {
    const int j = j0 + (int)threadIdx.x % FS_FIN_COLS;
    const double s = fs_finish_cols(part, P, nq, j0, s_a);
    if ((int)threadIdx.x < FS_FIN_COLS && j < nq) s_sum[j] = s;
    __syncthreads();          // s_a may be written again and s_sum read
  }
}

__global__ __launch_bounds__(FS_FIN_THREADS) void ck_power_finish_kernel(const double* __restrict__ part, int64_t P, double* pst, double sc,
                                                                          double invn, int last, double alpha_frac) {
#pragma clang fp contract(off)
  __shared__ double s_a[FS_FIN_THREADS];
  __shared__ double s_sum[8];
  ck_finish_sums(part, P, 5, s_a, s_sum);
  if (threadIdx.x == 0) {
    const double l = fabs(s_sum[0] / s_sum[1]);
    const double nrm = sqrt(s_sum[2]);
    const double s1 = s_sum[3] / nrm, s2 = s_sum[4] / nrm;
    const double m = invn * s1;
    const double t = sc * m;
    const double y = s2 - t;
    pst[0] = nrm;
    pst[1] = m;
    pst[2] = invn * y;
    pst[3] = l;
    if (last) {
      const double alpha = alpha_frac * l;
      pst[4] = 1.0 / alpha;
    }
  }
}

// closes the iteration of slot r: m, yb of the new iterate and err; r_slot = 0: the start (the partials of u0, no err)
__global__ __launch_bounds__(FS_FIN_THREADS) void ck_finish_kernel(const double* __restrict__ part, int64_t P, int k,
                                                                    const unsigned long long* __restrict__ perr, int64_t nerr, double* mst,
                                                                    double sc, double invn, double* slots, int r_slot, double tol) {
#pragma clang fp contract(off)
  __shared__ double s_a[FS_FIN_THREADS];
  __shared__ double s_sum[2 * CK_MAX_COLS];
  __shared__ unsigned long long s_e;
  if (r_slot > 0 && ck_stopped(slots[r_slot - 1], tol)) return;
  if (threadIdx.x == 0) s_e = 0ull;
  ck_finish_sums(part, P, 2 * k, s_a, s_sum);
  if ((int)threadIdx.x < k) {
    const int c = threadIdx.x;
    const double m = invn * s_sum[c];
    const double t = sc * m;
    const double y = s_sum[k + c] - t;
    mst[c] = m;
    mst[k + c] = invn * y;
  }
  if (r_slot > 0) {
    unsigned long long e = 0ull;
    for (int64_t q = threadIdx.x; q < nerr; q += FS_FIN_THREADS) e = perr[q] > e ? perr[q] : e;
    if (e) atomicMax(&s_e, e);
    __syncthreads();
    if (threadIdx.x == 0) slots[r_slot] = __longlong_as_double((long long)s_e);
  }
}

// u0: val on the training rows, zero elsewhere
__global__ __launch_bounds__(256) void ck_start_kernel(double* __restrict__ u, const int32_t* __restrict__ lab, const double* __restrict__ val,
                                                       int64_t n, int k) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n * k) return;
  const int64_t i = t / k;
  const int32_t q = lab[i];
  u[t] = q >= 0 ? val[(int64_t)q * k + (t - i * k)] : 0.0;
}

// ck_slots_next on the device (one workgroup, chunk + 1 <= 256 slots)
__global__ __launch_bounds__(256) void ck_slots_kernel(double* slots, int chunk, int prev_len, int first) {
  const double carry = first ? 1.0 : slots[prev_len];
  __syncthreads();
  const int r = threadIdx.x;
  if (r == 0) slots[0] = carry;
  else if (r <= chunk) slots[r] = __longlong_as_double(0x7ff8000000000000ll);
}

extern "C" int glx_ck_solve(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* col, const double* W, int k, int64_t m,
                            const int32_t* ind, const double* val, const double* e, int64_t power_it, double alpha_frac, double tol,
                            int64_t max_it, double* u, double* l_out, int64_t* T_out, double* err_hist, int64_t err_cap,
                            glx_ck_iterate_fn on_iterate, void* user, int64_t* plan_out, int device) {
  GLX_CHECK(row_ptr && (M <= 0 || (col && W)) && (m <= 0 || (ind && val)) && e && u && l_out && T_out, GLX_EINVAL,
            "glx_ck_solve: null argument");
  {
    char msg[256];
    const int bad = ck_validate(n, M, row_ptr, col, W, k, m, ind, power_it, alpha_frac, max_it, msg, sizeof msg);
    GLX_CHECK(!bad, bad == 9 ? GLX_EUNSUPPORTED : GLX_EINVAL, "glx_ck_solve: %s", msg);
  }
  GLX_CHECK(err_cap >= 0, GLX_EINVAL, "glx_ck_solve: err_cap=%lld", (long long)err_cap);
  CkPlan plan;
  ck_make_plan(n, row_ptr, col, W, k, m, ind, &plan);
  const int64_t P = plan.P;
  const int chunk = on_iterate ? 1 : CK_CHUNK;
  double pst0[8] = {1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  ck_power_start(plan, n, e, &pst0[1], &pst0[2]);
  std::vector<double> part0((size_t)P * 2 * k);
  ck_start_partials(plan, n, k, val, part0.data());

  GlxCall call;
  GLX_UP(call.begin(device));
  hipStream_t st = call.stream();
  int64_t* d_ptr = nullptr;
  int32_t *d_col = nullptr, *d_lab = nullptr;
  double *d_w = nullptr, *d_d = nullptr, *d_c = nullptr, *d_val = nullptr, *d_xa = nullptr, *d_xb = nullptr, *d_ua = nullptr, *d_ub = nullptr,
         *d_pst = nullptr, *d_mst = nullptr, *d_part = nullptr, *d_slots = nullptr, *stage = nullptr;
  unsigned long long* d_perr = nullptr;
  const int64_t nerr = P * plan.ntiles;
  GLX_UP(call.put(&d_ptr, row_ptr, (size_t)(n + 1), __func__));
  GLX_UP(call.put(&d_col, col, (size_t)M, __func__));
  GLX_UP(call.put(&d_w, W, (size_t)M, __func__));
  GLX_UP(call.put(&d_d, (const double*)plan.d.data(), (size_t)n, __func__));
  GLX_UP(call.put(&d_c, (const double*)plan.c.data(), (size_t)n, __func__));
  GLX_UP(call.put(&d_lab, (const int32_t*)plan.lab.data(), (size_t)n, __func__));
  GLX_UP(call.put(&d_val, val, (size_t)m * k, __func__));
  GLX_UP(call.put(&d_xa, e, (size_t)n, __func__));
  GLX_UP(call.alloc(&d_xb, (size_t)n));
  GLX_UP(call.alloc(&d_ua, (size_t)n * k));
  GLX_UP(call.alloc(&d_ub, (size_t)n * k));
  GLX_UP(call.put(&d_pst, (const double*)pst0, 8, __func__));
  GLX_UP(call.alloc(&d_mst, (size_t)2 * k));
  GLX_UP(call.alloc(&d_part, (size_t)P * std::max(2 * k, 5)));
  GLX_UP(call.alloc(&d_perr, (size_t)nerr));
  GLX_UP(call.alloc(&d_slots, (size_t)CK_CHUNK + 1));
  GLX_UP(call.stage(&stage, (size_t)CK_CHUNK + 8));
  int64_t launches = 0;

  // power iteration: pass p reads one of the two vectors and writes the other
  for (int64_t p = 0; p < power_it; ++p) {
    const double* x = (p & 1) ? d_xb : d_xa;
    double* xout = (p & 1) ? d_xa : d_xb;
    hipLaunchKernelGGL(ck_power_pass_kernel, dim3((unsigned)P), dim3(FS_ROWS), 0, st, (const int64_t*)d_ptr, (const int32_t*)d_col,
                       (const double*)d_w, (const double*)d_d, (const double*)d_c, x, xout, (const double*)d_pst, d_part, n);
    GLX_HIP(hipGetLastError());
    hipLaunchKernelGGL(ck_power_finish_kernel, dim3(1), dim3(FS_FIN_THREADS), 0, st, (const double*)d_part, P, d_pst, plan.sc, plan.invn,
                       p + 1 == power_it ? 1 : 0, alpha_frac);
    GLX_HIP(hipGetLastError());
    launches += 2;
  }
  // the start of the fixed-point iteration and its means (the partials of u0 come from the host: u0 is zero off the m training rows)
  hipLaunchKernelGGL(ck_start_kernel, dim3((unsigned)((n * k + 255) / 256)), dim3(256), 0, st, d_ua, (const int32_t*)d_lab,
                     (const double*)d_val, n, k);
  GLX_HIP(hipGetLastError());
  GLX_UP(glx_upload(d_part, part0.data(), (size_t)P * 2 * k * 8, st, __func__));
  hipLaunchKernelGGL(ck_finish_kernel, dim3(1), dim3(FS_FIN_THREADS), 0, st, (const double*)d_part, P, k, (const unsigned long long*)d_perr,
                     nerr, d_mst, plan.sc, plan.invn, d_slots, 0, tol);
  GLX_HIP(hipGetLastError());
  launches += 2;

  const int tbase = k / plan.ntiles, textra = k % plan.ntiles;          // what col_tile_at (csr_plan.h) takes
  const dim3 grid((unsigned)P, (unsigned)plan.ntiles), blk((unsigned)(FS_ROWS * plan.ct));
  const size_t lds = (size_t)2 * FS_ROWS * plan.ct * 8;
  std::vector<double> iterate;
  if (on_iterate) iterate.resize((size_t)n * k);
  CkStops stops(tol, max_it);
  bool first = true;
  for (int len; (len = stops.next_len(chunk)) > 0;) {
    hipLaunchKernelGGL(ck_slots_kernel, dim3(1), dim3(256), 0, st, d_slots, CK_CHUNK, stops.prev_len, first ? 1 : 0);
    GLX_HIP(hipGetLastError());
    first = false;
    for (int r = 1; r <= len; ++r) {
      const int64_t q = stops.it + r;
      const double* uin = ((q - 1) & 1) ? d_ub : d_ua;
      double* uout = (q & 1) ? d_ub : d_ua;
      hipLaunchKernelGGL(ck_pass_kernel, grid, blk, lds, st, (const int64_t*)d_ptr, (const int32_t*)d_col, (const double*)d_w,
                         (const double*)d_d, (const double*)d_c, (const int32_t*)d_lab, uin, uout, (const double*)d_mst, (const double*)d_pst,
                         d_part, d_perr, n, k, plan.ct, tbase, textra, (const double*)d_slots, r, tol);
      GLX_HIP(hipGetLastError());
      hipLaunchKernelGGL(ck_finish_kernel, dim3(1), dim3(FS_FIN_THREADS), 0, st, (const double*)d_part, P, k,
                         (const unsigned long long*)d_perr, nerr, d_mst, plan.sc, plan.invn, d_slots, r, tol);
      GLX_HIP(hipGetLastError());
      launches += 2;
    }
    GLX_HIP(hipMemcpyAsync(stage, d_slots + 1, (size_t)len * 8, hipMemcpyDeviceToHost, st));
    GLX_HIP(hipStreamSynchronize(st));
    const int64_t q = stops.it + 1;
    stops.decide(stage, len, err_hist, err_cap);
    if (on_iterate) {          // chunk = 1: the iterate this iteration wrote, handed to the caller while the solve runs
      GLX_UP(glx_download(iterate.data(), (q & 1) ? d_ub : d_ua, (size_t)n * k * 8, st, __func__));
      GLX_HIP(hipStreamSynchronize(st));
      GLX_CHECK(on_iterate(q, iterate.data(), stage[0], user) == 0, GLX_EINVAL, "glx_ck_solve: on_iterate asked to end the call at iteration %lld",
                (long long)q);
    }
  }
  GLX_HIP(hipMemcpyAsync(stage, d_pst, 8 * 8, hipMemcpyDeviceToHost, st));
  GLX_HIP(hipStreamSynchronize(st));
  *l_out = stage[3];
  GLX_CHECK(!stops.capped(), GLX_EUNSUPPORTED, "glx_ck_solve: no stop within max_it=%lld iterations (last err above tol=%g)", (long long)max_it,
            tol);
  *T_out = stops.T;
  GLX_UP(glx_download(u, (stops.T & 1) ? d_ub : d_ua, (size_t)n * k * 8, st, __func__));
  GLX_HIP(hipStreamSynchronize(st));
  if (plan_out) {
    plan_out[0] = 2;
    plan_out[1] = launches;
    plan_out[2] = chunk;
    plan_out[3] = P;
  }
  return GLX_OK;
}
