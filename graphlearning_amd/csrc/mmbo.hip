// The multiclass MBO learner of Garcia-Cardona et al. (2014) in one device call: T * Ns diffusion steps in the basis X (n, m) with a
// projection onto the classes after every Ns of them, the loop of the reference's ssl.multiclass_mbo (ssl.py:989-996), reached
// through ssl.multiclass_mbo / _hip.mmbo_solve.  The contract -- the order of operations of a step, every operation rounded on its
// own, the reduction order, the tie rule of the projection -- is written down in mmbo_plan.h and DESIGN.md 4.13 and walked on the
// host by mmbo_host_reference; this file is that loop on the device, bit for bit.
//
// Two kernels per step with an ordinary kernel boundary between them.  The only per-vertex state is the label: u (k, n) never exists
// in memory.  The pass: one workgroup per partial of MMBO_ROWS rows, Z (k m doubles, rows padded to an odd length) in LDS, the rows
// taken up to 64 at a time (mmbo_sub_rows: as many as 48 KiB of LDS hold, at least 8) -- their X into LDS, u = Z x per (row, class)
// by one thread each in the order of j, the label decided and recorded where the step follows a projection, the fidelity term, X
// scaled by the eigenvalue factors in place -- and then every thread adds b[r, c] * y[r, j] for the (c, j) it owns, row after row,
// into registers: the chain of mmbo_plan.h.  The finishing kernel adds the partials of 16 values per workgroup in the fixed order of
// fs_finish (fixed_sum.h; fs_finish_cols of fixed_sum_device.h) and leaves the next Z.  No floating-point atomic, no grid-wide wait,
// nothing depends on which workgroup ends first.  One last pass decides the final labels.
//
// Buffers come from the pool and are written before they are read; no launch sequence is captured.
#include "glx_internal.h"
#include "mmbo_plan.h"
#include "fixed_sum_device.h"
#include <vector>

#define MMBO_OWN (MMBO_CAP / MMBO_THREADS)          // (c, j) pairs a thread of the pass owns at most

// lab_in: read by MMBO_START; lab_out: written by MMBO_PROJECT and MMBO_LABELS; part (P, k m): not written by MMBO_LABELS
__global__ __launch_bounds__(MMBO_THREADS) void mmbo_pass_kernel(const double* __restrict__ X, const double* __restrict__ d,
                                                                 const int32_t* __restrict__ tl, const int32_t* __restrict__ lab_in,
                                                                 int32_t* __restrict__ lab_out, const double* __restrict__ Z,
                                                                 double* __restrict__ part, int64_t n, int m, int k, int sub, int mode, double c0) {
#pragma clang fp contract(off)
  extern __shared__ double s_dyn[];          // zs k * mp, xs sub * m, us sub * k (mmbo_lds_doubles)
  __shared__ int s_lab[MMBO_ROWS], s_tl[MMBO_ROWS];
  const int mp = m | 1, km = k * m, t = threadIdx.x;
  double* zs = s_dyn;
  double* xs = zs + k * mp;
  double* us = xs + sub * m;
  const int64_t i0 = (int64_t)blockIdx.x * MMBO_ROWS;
  const int rows = (int)(n - i0 < MMBO_ROWS ? n - i0 : MMBO_ROWS);
  if (mode != MMBO_START)
    for (int q = t; q < km; q += MMBO_THREADS) {
      const int c = q / m;
      zs[c * mp + (q - c * m)] = Z[q];
    }
  double acc[MMBO_OWN];
#pragma unroll
  for (int s = 0; s < MMBO_OWN; ++s) acc[s] = 0.0;
  for (int r0 = 0; r0 < rows; r0 += sub) {
    const int nr = rows - r0 < sub ? rows - r0 : sub;
    const int64_t ib = i0 + r0;
    __syncthreads();          // the rows before are added up (and, the first time, zs is written)
    for (int q = t; q < nr * m; q += MMBO_THREADS) xs[q] = X[ib * m + q];
    if (t < nr) {
      s_tl[t] = tl[ib + t];
      if (mode == MMBO_START) s_lab[t] = lab_in[ib + t];
    }
    __syncthreads();
    if (mode != MMBO_START) {
      for (int q = t; q < nr * k; q += MMBO_THREADS) {
        const int r = q / k, c = q - r * k;
        double s = 0.0;
        for (int j = 0; j < m; ++j) {
          const double pr = zs[c * mp + j] * xs[r * m + j];
          s = s + pr;
        }
        us[q] = s;
      }
      __syncthreads();
      if (mode != MMBO_PLAIN && t < nr) {
        int best = 0;
        double ub = us[t * k];
        for (int c = 1; c < k; ++c) {
          const double v = us[t * k + c];
          if (v > ub) {
            ub = v;
            best = c;
          }
        }
        s_lab[t] = best;
        lab_out[ib + t] = best;
      }
      __syncthreads();
    }
    if (mode == MMBO_LABELS) continue;          // (the same in every thread)
    for (int q = t; q < nr * k; q += MMBO_THREADS) {
      const int r = q / k, c = q - r * k;
      double u = mode == MMBO_PLAIN ? us[q] : (s_lab[r] == c ? 1.0 : 0.0);
      const int tr = s_tl[r];
      if (tr >= 0) {
        const double K = c == tr ? 1.0 : 0.0;
        const double t1 = u - K;
        const double t2 = c0 * t1;
        u = u - t2;
      }
      us[q] = u;
    }
    for (int q = t; q < nr * m; q += MMBO_THREADS) xs[q] = xs[q] * d[q % m];
    __syncthreads();
#pragma unroll
    for (int s = 0; s < MMBO_OWN; ++s) {
      const int q = t + MMBO_THREADS * s;
      if (q < km) {
        const int c = q / m, j = q - c * m;
        double a = acc[s];
        for (int r = 0; r < nr; ++r) {
          const double pr = us[r * k + c] * xs[r * m + j];
          a = a + pr;
        }
        acc[s] = a;
      }
    }
  }
  if (mode != MMBO_LABELS) {
#pragma unroll
    for (int s = 0; s < MMBO_OWN; ++s) {
      const int q = t + MMBO_THREADS * s;
      if (q < km) part[(int64_t)blockIdx.x * km + q] = acc[s];
    }
  }
}

// Z[j] for the FS_FIN_COLS values of this workgroup, in the order of fs_finish
__global__ __launch_bounds__(FS_FIN_THREADS) void mmbo_finish_kernel(const double* __restrict__ part, int64_t P, int km, double* __restrict__ Z) {
#pragma clang fp contract(off)
  __shared__ double s_a[FS_FIN_THREADS];
  const int j = (int)blockIdx.x * FS_FIN_COLS + (int)threadIdx.x;          // (of the threads of chain 0)
  const double s = fs_finish_cols(part, P, km, (int)blockIdx.x * FS_FIN_COLS, s_a);
  if ((int)threadIdx.x < FS_FIN_COLS && j < km) Z[j] = s;
}

extern "C" int glx_mmbo_solve(int64_t n, int m, const double* X, const double* vals, const int32_t* lab0, int64_t ntrain, const int32_t* ind,
                              const int32_t* lab, int k, int64_t Ns, int64_t T, double dt, double mu, int32_t* hist, double* Zlast,
                              int64_t* plan_out, int device) {
  GLX_CHECK(X && vals && lab0 && (ntrain <= 0 || (ind && lab)) && hist && Zlast, GLX_EINVAL, "glx_mmbo_solve: null argument");
  {
    char msg[256];
    const int bad = mmbo_validate(n, m, X, vals, lab0, ntrain, ind, lab, k, Ns, T, dt, mu, msg, sizeof msg);
    GLX_CHECK(!bad, bad == 8 ? GLX_EUNSUPPORTED : GLX_EINVAL, "glx_mmbo_solve: %s", msg);
  }
  MmboPlan plan;
  mmbo_make_plan(n, m, vals, ntrain, ind, lab, Ns, dt, mu, &plan);
  const int64_t P = plan.P;
  const int km = k * m;

  GlxCall call;
  GLX_UP(call.begin(device));
  hipStream_t st = call.stream();
  double *d_x = nullptr, *d_d = nullptr, *d_z = nullptr, *d_part = nullptr;
  int32_t *d_tl = nullptr, *d_lab0 = nullptr, *d_hist = nullptr;
  GLX_UP(call.put(&d_x, X, (size_t)n * m, __func__));
  GLX_UP(call.put(&d_d, (const double*)plan.d.data(), (size_t)m, __func__));
  GLX_UP(call.put(&d_tl, (const int32_t*)plan.tl.data(), (size_t)n, __func__));
  GLX_UP(call.put(&d_lab0, lab0, (size_t)n, __func__));
  GLX_UP(call.alloc(&d_hist, (size_t)T * n));
  GLX_UP(call.alloc(&d_z, (size_t)km));
  GLX_UP(call.alloc(&d_part, (size_t)P * km));

  const int sub = mmbo_sub_rows(k, m);
  const size_t lds = mmbo_lds_doubles(k, m, sub) * 8;          // 52 KiB at the most
  const unsigned fin_blocks = (unsigned)((km + FS_FIN_COLS - 1) / FS_FIN_COLS);
  int64_t launches = 0;
  for (int64_t g = 0; g < T * Ns; ++g) {
    const int mode = mmbo_mode(g, Ns);
    int32_t* out = mode == MMBO_PROJECT ? d_hist + (g / Ns - 1) * n : nullptr;
    hipLaunchKernelGGL(mmbo_pass_kernel, dim3((unsigned)P), dim3(MMBO_THREADS), lds, st, (const double*)d_x, (const double*)d_d,
                       (const int32_t*)d_tl, (const int32_t*)d_lab0, out, (const double*)d_z, d_part, n, m, k, sub, mode, plan.c0);
    GLX_HIP(hipGetLastError());
    hipLaunchKernelGGL(mmbo_finish_kernel, dim3(fin_blocks), dim3(FS_FIN_THREADS), 0, st, (const double*)d_part, P, km, d_z);
    GLX_HIP(hipGetLastError());
    launches += 2;
  }
  hipLaunchKernelGGL(mmbo_pass_kernel, dim3((unsigned)P), dim3(MMBO_THREADS), lds, st, (const double*)d_x, (const double*)d_d,
                     (const int32_t*)d_tl, (const int32_t*)d_lab0, d_hist + (T - 1) * n, (const double*)d_z, d_part, n, m, k, sub,
                     (int)MMBO_LABELS, plan.c0);
  GLX_HIP(hipGetLastError());
  launches += 1;
  GLX_UP(glx_download(hist, d_hist, (size_t)T * n * 4, st, __func__));
  GLX_UP(glx_download(Zlast, d_z, (size_t)km * 8, st, __func__));
  GLX_HIP(hipStreamSynchronize(st));
  if (plan_out) {
    plan_out[0] = 2;
    plan_out[1] = MMBO_ROWS;
    plan_out[2] = P;
    plan_out[3] = MMBO_CAP;
    plan_out[4] = MMBO_MAX_K;
    plan_out[5] = MMBO_MAX_M;
    plan_out[6] = launches;
  }
  return GLX_OK;
}
