// Game-theoretic p-Laplace equation, Jacobi iteration of the upper and lower barrier functions: lp_iterate_main of the reference's C
// extension (c_code/lp_iterate.cpp:35-125), reached through graph.plaplace(..., fast=False) (graphlearning/graph.py:1262-1278).
//
// ONE kernel serves both entry points.  glx_lp_iterate_batch runs B problems that share the boundary vertices as the columns of one
// launch per iteration, and glx_lp_iterate is the same driver with B = 1 and the caller's (uu, ul) as the start.  One thread per
// (vertex, column), columns fastest; the state is (n, B) row-major records (uu, ul), so a neighbour's B records are one contiguous
// 16 B-byte gather and the indices and weights are streamed once for all columns.  A thread walks its vertex's stored entries in the
// caller's order, left to right (min / max / sequential sum of w_ij (u_j - u_i), separate multiply and add roundings) for both
// barriers at once; no row is reduced across lanes.
//
// All iterations are enqueued from the host in chunks of LP_BATCH_CHUNK.  Every column stops on its own: the per-chunk error slots,
// why a stopped column stays frozen in both buffers -- so that both iterates of the stopping step survive exactly as they do behind
// the reference's swapped pointers -- and which iterate the first buffer then holds are in lp_plan.h.  Every buffer comes from the
// library's pool and is written before it is read (the slots are cleared by a kernel); device memory does not grow with T.
#include "glx_internal.h"
#include "lp_plan.h"
#include <algorithm>
#include <vector>

// iteration `it`, slot r of the chunk (slot r - 1 is the iteration before: slot 0 carries it over from the chunk before)
__global__ __launch_bounds__(LP_BLOCK) void lp_batch_sweep_kernel(const double2* __restrict__ xin, double2* __restrict__ xout,
                                                                  const int64_t* __restrict__ start, const int32_t* __restrict__ nbr,
                                                                  const double* __restrict__ W, const double* __restrict__ invdeg,
                                                                  const int32_t* __restrict__ bdy, const double* __restrict__ val,
                                                                  double dt, double delta, int64_t n, int B, int it, int r, double tol,
                                                                  unsigned long long* err) {
#pragma clang fp contract(off)
  __shared__ unsigned long long s_e[LP_LDS_COLS];
  const bool lds = B <= LP_LDS_COLS;
  if (lds) {
    if ((int)threadIdx.x < B) s_e[threadIdx.x] = 0ull;
    __syncthreads();
  }
  const int64_t t = (int64_t)blockIdx.x * LP_BLOCK + threadIdx.x;
  if (t < n * B) {
    const int64_t i = t / B;
    const int b = (int)(t - i * B);
    if (!lp_frozen(it, err[(int64_t)(r - 1) * B + b], tol)) {      // a stopped column is written in neither buffer
      const double2 me = xin[t];
      double minu = 0, maxu = 0, sumu = 0, minl = 0, maxl = 0, suml = 0;
      const int64_t j1 = start[i + 1];
      for (int64_t j = start[i]; j < j1; ++j) {     // lp_iterate.cpp:82-97
        const double2 x = xin[(int64_t)nbr[j] * B + b];
        const double w = W[j];
        const double du = x.x - me.x;
        const double tu = w * du;
        minu = (tu < minu) ? tu : minu;              // MIN / MAX of vector_operations.h: NaN leaves the bound alone
        maxu = (tu > maxu) ? tu : maxu;
        sumu = sumu + tu;
        const double dl = x.y - me.y;
        const double tl = w * dl;
        minl = (tl < minl) ? tl : minl;
        maxl = (tl > maxl) ? tl : maxl;
        suml = suml + tl;
      }
      const double id = invdeg[i];
      double2 out;
      {
        const double a1 = id * sumu, a2 = minu + maxu, a3 = delta * a2, a4 = a1 + a3, a5 = dt * a4;
        out.x = me.x + a5;
      }
      {
        const double a1 = id * suml, a2 = minl + maxl, a3 = delta * a2, a4 = a1 + a3, a5 = dt * a4;
        out.y = me.y + a5;
      }
      const int32_t bj = bdy[i];                     // Dirichlet values overwrite the update (:105-110)
      if (bj >= 0) { out.x = val[(int64_t)bj * B + b]; out.y = out.x; }
      xout[t] = out;
      const double gap = me.x - me.y;
      if (gap > 0.0) {                               // err = MAX(uu[i] - ul[i], err) from 0: a NaN or negative gap leaves it alone
        const unsigned long long e = (unsigned long long)__double_as_longlong(gap);
        if (lds) atomicMax(&s_e[b], e);
        else atomicMax(&err[(int64_t)r * B + b], e);
      }
    }
  }
  if (lds) {
    __syncthreads();
    if ((int)threadIdx.x < B && s_e[threadIdx.x]) atomicMax(&err[(int64_t)r * B + threadIdx.x], s_e[threadIdx.x]);
  }
}

// the start: boundary rows take val, the others the column's largest / smallest boundary value
__global__ __launch_bounds__(256) void lp_batch_init_kernel(double2* x, const int32_t* __restrict__ bdy, const double* __restrict__ val,
                                                            const double* __restrict__ hi, const double* __restrict__ lo, int64_t n, int B) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n * B) return;
  const int64_t i = t / B;
  const int b = (int)(t - i * B);
  const int32_t q = bdy[i];
  double2 v;
  if (q >= 0) { v.x = val[(int64_t)q * B + b]; v.y = v.x; }
  else { v.x = hi[b]; v.y = lo[b]; }
  x[t] = v;
}

namespace {
// B columns from the iterate lp_batch_init_kernel forms, or (start) from the caller's uu, ul as they are
int lp_run(const char* who, int64_t n, int64_t M, const int32_t* nbr, const int32_t* row, const double* W, int B, int64_t m,
           const int32_t* ind, const double* val, double p, int64_t T, double tol, bool start, double* uu, double* ul, int64_t* iters_out,
           int device) {
  LpPlan plan;
  {
    char msg[200];
    const int bad = lp_make_plan(n, M, nbr, row, W, B, m, ind, val, p, T, &plan, msg, sizeof msg);
    GLX_CHECK(!bad, bad == 2 ? GLX_EUNSUPPORTED : GLX_EINVAL, "%s: %s", who, msg);
  }
  GlxCall call;
  GLX_UP(call.begin(device));
  hipStream_t st = call.stream();
  const int64_t total = n * B;
  std::vector<double2> x((size_t)total);
  double2 *d_a = nullptr, *d_b = nullptr;
  int64_t* d_start = nullptr;
  int32_t *d_nbr = nullptr, *d_bdy = nullptr;
  double *d_w = nullptr, *d_invdeg = nullptr, *d_val = nullptr, *d_hi = nullptr, *d_lo = nullptr;
  unsigned long long *d_err = nullptr, *stage = nullptr;
  if (start) {
    for (int64_t q = 0; q < total; ++q) { x[q].x = uu[q]; x[q].y = ul[q]; }
    GLX_UP(call.put(&d_a, (const double2*)x.data(), (size_t)total, who));
  } else {
    GLX_UP(call.alloc(&d_a, (size_t)total));
  }
  GLX_UP(call.alloc(&d_b, (size_t)total));
  GLX_UP(call.put(&d_start, (const int64_t*)plan.start.data(), (size_t)(n + 1), who));
  GLX_UP(call.put(&d_nbr, nbr, (size_t)M, who));
  GLX_UP(call.put(&d_w, W, (size_t)M, who));
  GLX_UP(call.put(&d_invdeg, (const double*)plan.invdeg.data(), (size_t)n, who));
  GLX_UP(call.put(&d_bdy, (const int32_t*)plan.bdy.data(), (size_t)n, who));
  GLX_UP(call.put(&d_val, val, (size_t)m * B, who));
  if (!start) {
    GLX_UP(call.put(&d_hi, (const double*)plan.hi.data(), (size_t)B, who));
    GLX_UP(call.put(&d_lo, (const double*)plan.lo.data(), (size_t)B, who));
  }
  GLX_UP(call.alloc(&d_err, (size_t)(LP_BATCH_CHUNK + 1) * B));
  GLX_UP(call.stage(&stage, (size_t)LP_BATCH_CHUNK * B));
  if (!start) {
    hipLaunchKernelGGL(lp_batch_init_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d_a, (const int32_t*)d_bdy,
                       (const double*)d_val, (const double*)d_hi, (const double*)d_lo, n, B);
    GLX_HIP(hipGetLastError());
  }

  const unsigned grid = (unsigned)((total + LP_BLOCK - 1) / LP_BLOCK);
  LpStops stops(B, T, tol);
  for (int len; (len = stops.next_len(LP_BATCH_CHUNK)) > 0;) {
    GLX_UP(glx_slots_next_async(d_err, B, LP_BATCH_CHUNK, stops.prev_len, st));
    for (int r = 1; r <= len; ++r) {
      const int64_t it = stops.it + r - 1;
      const double2* xin = (it & 1) ? d_b : d_a;
      double2* xout = (it & 1) ? d_a : d_b;
      hipLaunchKernelGGL(lp_batch_sweep_kernel, dim3(grid), dim3(LP_BLOCK), 0, st, xin, xout, (const int64_t*)d_start, (const int32_t*)d_nbr,
                         (const double*)d_w, (const double*)d_invdeg, (const int32_t*)d_bdy, (const double*)d_val, plan.dt, plan.delta, n, B,
                         (int)it, r, tol, d_err);
      GLX_HIP(hipGetLastError());
    }
    GLX_HIP(hipMemcpyAsync(stage, d_err + B, (size_t)len * B * 8, hipMemcpyDeviceToHost, st));
    GLX_HIP(hipStreamSynchronize(st));
    stops.decide(stage, len);
  }
  // the caller's arrays are the first buffer: whatever iterate of a column last lived there (lp_result_iterate)
  GLX_UP(glx_download(x.data(), d_a, (size_t)total * 16, st, who));
  GLX_HIP(hipStreamSynchronize(st));
  for (int64_t q = 0; q < total; ++q) { uu[q] = x[q].x; ul[q] = x[q].y; }
  if (iters_out)
    for (int b = 0; b < B; ++b) iters_out[b] = stops.iters(b);
  return GLX_OK;
}
}  // namespace

extern "C" int glx_lp_iterate(double* uu, double* ul, const int32_t* nbr, const int32_t* row, const double* W, const int32_t* ind,
                              const double* val, double p, int64_t T, double tol, int64_t n, int64_t M, int64_t m,
                              int64_t* iters_out, int device) {
  GLX_CHECK(uu && ul && (M <= 0 || (nbr && row && W)) && (m <= 0 || (ind && val)), GLX_EINVAL, "glx_lp_iterate: null argument");
  return lp_run("glx_lp_iterate", n, M, nbr, row, W, 1, m, ind, val, p, T, tol, true, uu, ul, iters_out, device);
}

extern "C" int glx_lp_iterate_batch(int64_t n, int64_t M, const int32_t* nbr, const int32_t* row, const double* W, int B, int64_t m,
                                    const int32_t* ind, const double* val, double p, int64_t T, double tol, double* uu, double* ul,
                                    int64_t* iters_out, int device) {
  GLX_CHECK(uu && ul && (M <= 0 || (nbr && row && W)) && (m <= 0 || (ind && val)), GLX_EINVAL, "glx_lp_iterate_batch: null argument");
  return lp_run("glx_lp_iterate_batch", n, M, nbr, row, W, B, m, ind, val, p, T, tol, false, uu, ul, iters_out, device);
}
