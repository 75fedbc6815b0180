// In-order Gauss-Seidel sweeps on the device, bit for bit: lip_iterate_main and lip_iterate_weighted_main of the reference's C
// extension (c_code/lp_iterate.cpp:129-187, :190-259), reached through graph.amle / ssl.amle (and, with alpha != 0, the arguments of
// graph.plaplace(fast=True)).
//
// The reference visits the vertices in index order and overwrites u in place.  The level plan (lip_plan.h, where the argument is)
// orders the non-boundary vertices so that the vertices of one level are never adjacent: a launch per level -- or one workgroup
// walking a run of small levels with a barrier between them -- runs them concurrently on the in-place array, and every one of
// them reads exactly the values the sequential loop would read.  No grid-wide wait, no persistent kernel.
//
// One thread per (vertex of the level, column), columns fastest: u is (n, B) row-major, a neighbour's B values are contiguous.  A
// thread walks its vertex's stored entries in the caller's order, diagonal included, folding left to right with the reference's
// MIN / MAX / ABS (vector_operations.h: `(a<b)?a:b`, `(a>b)?a:b`, `(a<0)?-a:a`) and separately rounded operations; no row is
// reduced across lanes.
//
// Errors and stops.  err = MAX(ABS(u_i - ne), err) from 0 over a sweep is the largest non-NaN |u_i - ne| or +0: non-negative doubles
// order like their bit patterns, so an integer atomicMax per (sweep, column) gives the same value whatever the order.  A column
// stops after the sweep `it` with err < tol && it > 20 (:184, :256).  The host enqueues LIP_CHUNK sweeps, reads their error slots once
// and decides; on the device a thread of sweep `it` finds its column stopped when the slot of sweep it - 1 holds a value below
// tol (and it - 1 > 20): a stopped column's later slots stay zero, which is below any tol that can stop at all, so the column
// stays frozen through the chunk.  Slot 0 of a chunk carries the last slot of the chunk before.  The slots are per chunk:
// device memory does not grow with T.  Every buffer comes from the library's pool and is written before it is read (the slots are
// cleared by a kernel).
#include "glx_internal.h"
#include "lip_plan.h"
#include "glx_stops.h"
#include <algorithm>
#include <vector>

static const int LIP_REG_ROW = 32;         // weighted form: rows of up to this many entries are held in registers through the bisection
static const int LIP_STOP_AFTER = 20;       // no column stops after a sweep <= this one (lp_iterate.cpp:184, :256)
static const int LIP_LDS_COLS = 64;        // up to this many columns a workgroup folds its errors in LDS before it touches the slots

// The weighted update of a row of at most CAP entries: its values and weights stay in registers through the 30 passes (same entries,
// same order, same operations).  Every index is a compile-time constant and an entry beyond deg is masked out: a loop that leaves
// early on `deg` is not unrolled, and x[k] then becomes an indexed register read behind a waterfall loop (measured on four inputs in
// EXPERIMENTS.md, "AMLE by levels": 1.1 to 4.8 times slower than this form).
template <int CAP>
__device__ __forceinline__ double lip_bisect(const double* u, const int32_t* __restrict__ nbr, const double* __restrict__ W, int64_t e0,
                                             int deg, int B, int b, double first) {
#pragma clang fp contract(off)
  double x[CAP], w[CAP];
#pragma unroll
  for (int k = 0; k < CAP; ++k) {
    const bool in = k < deg;
    x[k] = in ? u[(int64_t)nbr[e0 + k] * B + b] : 0.0;
    w[k] = in ? W[e0 + k] : 0.0;
  }
  double minu = first, maxu = first;
#pragma unroll
  for (int k = 0; k < CAP; ++k) {                      // lp_iterate.cpp:225-228
    const bool lo = (k < deg) & (x[k] < minu), hi = (k < deg) & (x[k] > maxu);
    minu = lo ? x[k] : minu;
    maxu = hi ? x[k] : maxu;
  }
  double a = minu, bb = maxu;
#pragma unroll 1                                       // (code size; no effect on the time was measured)
  for (int pass = 0; pass < 30; ++pass) {              // :231-243
    double minw = 0, maxw = 0;
    const double s = a + bb;
    const double t = s / 2.0;
#pragma unroll
    for (int k = 0; k < CAP; ++k) {
      const double d = t - x[k];
      const double v = w[k] * d;
      const bool lo = (k < deg) & (v < minw), hi = (k < deg) & (v > maxw);
      minw = lo ? v : minw;
      maxw = hi ? v : maxw;
    }
    const double inflap = minw + maxw;
    if (inflap > 0) bb = t; else a = t;
  }
  const double s = a + bb;
  return s / 2.0;
}

template <bool WEIGHTED>
__device__ __forceinline__ double lip_new_value(const double* u, const int32_t* __restrict__ nbr, const double* __restrict__ W, int64_t e0,
                                                int64_t e1, int B, int b, double alpha, double beta) {
#pragma clang fp contract(off)
  const double first = u[(int64_t)nbr[e0] * B + b];
  double minu = first, maxu = first;
  if (!WEIGHTED) {
    double sumu = 0.0, deg = 0.0;
    for (int64_t e = e0; e < e1; ++e) {                // lp_iterate.cpp:166-171
      const double x = u[(int64_t)nbr[e] * B + b];
      const double w = W[e];
      const double wx = w * x;
      sumu = sumu + wx;
      deg = deg + w;
      minu = (x < minu) ? x : minu;
      maxu = (x > maxu) ? x : maxu;
    }
    // `alpha*sumu/deg + beta*(minu + maxu)/2`: evaluated as written (with alpha == 0 the first term still decides +0 / -0)
    const double a1 = alpha * sumu, a2 = a1 / deg, b1 = minu + maxu, b2 = beta * b1, b3 = b2 / 2;
    return a2 + b3;
  }
  const int64_t deg = e1 - e0;
  if (deg <= 4) return lip_bisect<4>(u, nbr, W, e0, (int)deg, B, b, first);
  if (deg <= 8) return lip_bisect<8>(u, nbr, W, e0, (int)deg, B, b, first);
  if (deg <= 16) return lip_bisect<16>(u, nbr, W, e0, (int)deg, B, b, first);
  if (deg <= LIP_REG_ROW) return lip_bisect<LIP_REG_ROW>(u, nbr, W, e0, (int)deg, B, b, first);
  for (int64_t e = e0; e < e1; ++e) {                  // a longer row: from memory (it stays in cache)
    const double x = u[(int64_t)nbr[e] * B + b];
    minu = (x < minu) ? x : minu;
    maxu = (x > maxu) ? x : maxu;
  }
  double a = minu, bb = maxu;
#pragma unroll 1
  for (int k = 0; k < 30; ++k) {
    double minw = 0, maxw = 0;
    const double s = a + bb;
    const double t = s / 2.0;
    for (int64_t e = e0; e < e1; ++e) {
      const double d = t - u[(int64_t)nbr[e] * B + b];
      const double v = W[e] * d;
      minw = (v < minw) ? v : minw;
      maxw = (v > maxw) ? v : maxw;
    }
    const double inflap = minw + maxw;
    if (inflap > 0) bb = t; else a = t;
  }
  const double s = a + bb;
  return s / 2.0;
}

// one (vertex, column) of sweep `it` (slot r of the chunk): returns the bit pattern of |u_i - ne| where that is > 0, else 0
template <bool WEIGHTED>
__device__ __forceinline__ unsigned long long lip_visit(double* u, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ nbr,
                                                        const double* __restrict__ W, int32_t v, int B, int b, double alpha, double beta,
                                                        int it, int r, double tol, const unsigned long long* err) {
#pragma clang fp contract(off)
  if (it >= 1 && it - 1 > LIP_STOP_AFTER && __longlong_as_double((long long)err[(int64_t)(r - 1) * B + b]) < tol) return 0ull;      // the column has stopped
  const double ne = lip_new_value<WEIGHTED>(u, nbr, W, row_ptr[v], row_ptr[v + 1], B, b, alpha, beta);
  const int64_t at = (int64_t)v * B + b;
  const double d = u[at] - ne;
  const double ad = (d < 0) ? -d : d;
  u[at] = ne;
  return (ad > 0) ? (unsigned long long)__double_as_longlong(ad) : 0ull;
}

// A level of its own: order[0 .. count) are its vertices.
template <bool WEIGHTED>
__global__ __launch_bounds__(LIP_BLOCK) void lip_level_kernel(double* u, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ nbr,
                                                              const double* __restrict__ W, const int32_t* __restrict__ order, int64_t count,
                                                              int B, double alpha, double beta, int it, int r, double tol,
                                                              unsigned long long* err) {
  __shared__ unsigned long long s_e[LIP_LDS_COLS];
  const bool lds = B <= LIP_LDS_COLS;
  if (lds) {
    if ((int)threadIdx.x < B) s_e[threadIdx.x] = 0ull;
    __syncthreads();
  }
  const int64_t t = (int64_t)blockIdx.x * LIP_BLOCK + threadIdx.x;
  if (t < count * B) {
    const int64_t q = t / B;
    const int b = (int)(t - q * B);
    const unsigned long long e = lip_visit<WEIGHTED>(u, row_ptr, nbr, W, order[q], B, b, alpha, beta, it, r, tol, err);
    if (e) {
      if (lds) atomicMax(&s_e[b], e);
      else atomicMax(&err[(int64_t)r * B + b], e);
    }
  }
  if (lds) {
    __syncthreads();
    if ((int)threadIdx.x < B && s_e[threadIdx.x]) atomicMax(&err[(int64_t)r * B + threadIdx.x], s_e[threadIdx.x]);
  }
}

// A run of small levels [lvl0, lvl1): ONE workgroup walks them, a barrier between two levels.
template <bool WEIGHTED>
__global__ __launch_bounds__(LIP_BLOCK) void lip_merged_kernel(double* u, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ nbr,
                                                               const double* __restrict__ W, const int32_t* __restrict__ order,
                                                               const int64_t* __restrict__ lvl_ptr, int lvl0, int lvl1, int B, double alpha,
                                                               double beta, int it, int r, double tol, unsigned long long* err) {
  __shared__ unsigned long long s_e[LIP_LDS_COLS];
  const bool lds = B <= LIP_LDS_COLS;
  if (lds) {
    if ((int)threadIdx.x < B) s_e[threadIdx.x] = 0ull;
    __syncthreads();
  }
  for (int l = lvl0; l < lvl1; ++l) {
    const int64_t o0 = lvl_ptr[l];
    const int64_t items = (lvl_ptr[l + 1] - o0) * B;
    for (int64_t t = threadIdx.x; t < items; t += LIP_BLOCK) {
      const int64_t q = t / B;
      const int b = (int)(t - q * B);
      const unsigned long long e = lip_visit<WEIGHTED>(u, row_ptr, nbr, W, order[o0 + q], B, b, alpha, beta, it, r, tol, err);
      if (e) {
        if (lds) atomicMax(&s_e[b], e);
        else atomicMax(&err[(int64_t)r * B + b], e);
      }
    }
    __syncthreads();        // the level's values are written before the next level reads them (one workgroup: workgroup scope suffices)
  }
  if (lds && (int)threadIdx.x < B && s_e[threadIdx.x]) atomicMax(&err[(int64_t)r * B + threadIdx.x], s_e[threadIdx.x]);
}

// u = 0, boundary vertices take their values: bdy_q[i] = the row of `val` (m, B) vertex i takes, -1 off the boundary
__global__ __launch_bounds__(256) void lip_init_kernel(double* u, const int32_t* __restrict__ bdy_q, const double* __restrict__ val, int64_t n,
                                                       int B) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n * B) return;
  const int64_t i = t / B;
  const int32_t q = bdy_q[i];
  u[t] = q >= 0 ? val[(int64_t)q * B + (t - i * B)] : 0.0;
}

namespace {
template <bool WEIGHTED>
int lip_run(int64_t n, int64_t M, const std::vector<int64_t>& row_ptr, const int32_t* nbr, const double* W, const LipPlan& plan, int B,
            int64_t m, const std::vector<int32_t>& bdy_q, const double* val, double alpha, double beta, int64_t T, double tol, double* u,
            int64_t* iters_out, double* hist, int64_t* launches_out, int device) {
  GlxCall call;
  GLX_UP(call.begin(device));
  hipStream_t st = call.stream();
  const int64_t total = n * B, nlv = plan.nlevels, nord = (int64_t)plan.order.size();
  double *d_u = nullptr, *d_w = nullptr, *d_val = nullptr;
  int64_t *d_ptr = nullptr, *d_lvl = nullptr;
  int32_t *d_nbr = nullptr, *d_order = nullptr, *d_bq = nullptr;
  unsigned long long *d_err = nullptr, *stage = nullptr;
  GLX_UP(call.alloc(&d_u, (size_t)total));
  GLX_UP(call.put(&d_ptr, row_ptr.data(), (size_t)(n + 1), __func__));
  GLX_UP(call.put(&d_nbr, nbr, (size_t)M, __func__));
  GLX_UP(call.put(&d_w, W, (size_t)M, __func__));
  GLX_UP(call.put(&d_order, plan.order.data(), (size_t)nord, __func__));
  GLX_UP(call.put(&d_lvl, plan.lvl_ptr.data(), (size_t)(nlv + 1), __func__));
  GLX_UP(call.put(&d_bq, bdy_q.data(), (size_t)n, __func__));
  GLX_UP(call.put(&d_val, val, (size_t)m * B, __func__));
  GLX_UP(call.alloc(&d_err, (size_t)(LIP_CHUNK + 1) * B));
  GLX_UP(call.stage(&stage, (size_t)LIP_CHUNK * B));
  hipLaunchKernelGGL(lip_init_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d_u, (const int32_t*)d_bq,
                     (const double*)d_val, n, B);
  GLX_HIP(hipGetLastError());

  GlxStops stops(B, T, tol, LIP_STOP_AFTER, hist);
  if (nord == 0) stops.running = 0;
  int64_t launches = 0;
  for (int len; (len = stops.next_len(LIP_CHUNK)) > 0;) {
    GLX_UP(glx_slots_next_async(d_err, B, LIP_CHUNK, stops.prev_len, st));
    for (int r = 1; r <= len; ++r) {
      const int sweep = (int)(stops.it + r - 1);
      for (const LipLaunch& L : plan.launches) {
        if (L.merged) {
          hipLaunchKernelGGL((lip_merged_kernel<WEIGHTED>), dim3(1), dim3(LIP_BLOCK), 0, st, d_u, (const int64_t*)d_ptr, (const int32_t*)d_nbr,
                             (const double*)d_w, (const int32_t*)d_order, (const int64_t*)d_lvl, (int)L.lvl0, (int)L.lvl1, B, alpha, beta,
                             sweep, r, tol, d_err);
        } else {
          const int64_t o0 = plan.lvl_ptr[L.lvl0], count = plan.lvl_ptr[L.lvl1] - o0;
          hipLaunchKernelGGL((lip_level_kernel<WEIGHTED>), dim3((unsigned)((count * B + LIP_BLOCK - 1) / LIP_BLOCK)), dim3(LIP_BLOCK), 0, st,
                             d_u, (const int64_t*)d_ptr, (const int32_t*)d_nbr, (const double*)d_w, (const int32_t*)d_order + o0, count, B,
                             alpha, beta, sweep, r, tol, d_err);
        }
        GLX_HIP(hipGetLastError());
        ++launches;
      }
    }
    GLX_HIP(hipMemcpyAsync(stage, d_err + B, (size_t)len * B * 8, hipMemcpyDeviceToHost, st));
    GLX_HIP(hipStreamSynchronize(st));
    stops.decide(stage, len);
  }
  // sweeps done by a column: the stopping sweep counts.  With no vertex to update the reference still walks its T sweeps (err = 0
  // throughout) and stops after sweep 21
  std::vector<int64_t> iters((size_t)B);
  for (int c = 0; c < B; ++c) {
    if (nord == 0) {
      const int64_t done = (T > LIP_STOP_AFTER + 2 && 0.0 < tol) ? LIP_STOP_AFTER + 2 : T;
      if (hist)
        for (int64_t s = 0; s < done; ++s) hist[s * B + c] = 0.0;
      iters[c] = done;
    } else {
      iters[c] = stops.stop[c] >= 0 ? stops.stop[c] + 1 : T;
    }
  }
  GLX_UP(glx_download(u, d_u, (size_t)total * 8, st, __func__));
  GLX_HIP(hipStreamSynchronize(st));
  if (iters_out)
    for (int c = 0; c < B; ++c) iters_out[c] = iters[c];
  if (launches_out) *launches_out = launches;
  return GLX_OK;
}
}  // namespace

extern "C" int glx_lip_iterate(int64_t n, int64_t M, const int32_t* nbr, const int32_t* row, const double* W, int B, int64_t m,
                               const int32_t* ind, const double* val, int weighted, double alpha, double beta, int64_t T, double tol,
                               double* u, int64_t* iters_out, int64_t* plan_out, double* err_hist, int small_level, int device) {
  GLX_CHECK(u && (M == 0 || (nbr && row && W)) && (m == 0 || (ind && val)), GLX_EINVAL, "glx_lip_iterate: null argument");
  GLX_CHECK(B >= 1, GLX_EINVAL, "glx_lip_iterate: B=%d columns", B);
  GLX_CHECK(n >= 1 && M >= 0 && m >= 0 && T >= 0, GLX_EINVAL, "glx_lip_iterate: bad sizes (n=%lld M=%lld m=%lld T=%lld)", (long long)n,
            (long long)M, (long long)m, (long long)T);
  GLX_CHECK(T <= (1ll << 24), GLX_EUNSUPPORTED, "glx_lip_iterate: T=%lld above the supported 2^24 sweeps", (long long)T);
  GLX_CHECK(tol == tol && alpha == alpha && beta == beta, GLX_EINVAL, "glx_lip_iterate: tol, alpha or beta is NaN");
  GLX_CHECK(n <= 0x7fffffff && n * (int64_t)B <= (1ll << 31), GLX_EUNSUPPORTED,
            "glx_lip_iterate: n * B = %lld values above the supported 2^31 (split the columns into several calls)", (long long)(n * (int64_t)B));
  // vertex blocks of the row-sorted entry list (lp_iterate.cpp:138-145)
  std::vector<int64_t> row_ptr((size_t)n + 1, 0);
  for (int64_t e = 0; e < M; ++e) {
    GLX_CHECK(row[e] >= 0 && row[e] < n, GLX_EINVAL, "glx_lip_iterate: vertex index %d of entry %lld out of range", row[e], (long long)e);
    GLX_CHECK(e == 0 || row[e - 1] <= row[e], GLX_EINVAL, "glx_lip_iterate: the entries are not sorted by vertex (entry %lld)", (long long)e);
    GLX_CHECK(nbr[e] >= 0 && nbr[e] < n, GLX_EINVAL, "glx_lip_iterate: neighbour index %d of entry %lld out of range", nbr[e], (long long)e);
    GLX_CHECK(W[e] >= 0, GLX_EINVAL, "glx_lip_iterate: weight %g of entry %lld is negative or NaN", W[e], (long long)e);
    ++row_ptr[(size_t)row[e] + 1];
  }
  for (int64_t i = 0; i < n; ++i) row_ptr[i + 1] += row_ptr[i];
  std::vector<int32_t> bdy_q((size_t)n, -1);
  std::vector<unsigned char> bdy((size_t)n, 0);
  for (int64_t q = 0; q < m; ++q) {
    GLX_CHECK(ind[q] >= 0 && ind[q] < n, GLX_EINVAL, "glx_lip_iterate: boundary index %d out of range", ind[q]);
    bdy_q[ind[q]] = (int32_t)q;      // a vertex listed twice takes its last value, like the loop at :148-151
    bdy[ind[q]] = 1;
  }
  for (int64_t i = 0; i < n; ++i)
    GLX_CHECK(bdy[i] || row_ptr[i + 1] > row_ptr[i], GLX_EINVAL,
              "glx_lip_iterate: vertex %lld is not on the boundary and has no stored entry (the reference reads another vertex's entry there)",
              (long long)i);
  const LipPlan plan = lip_make_plan(n, row_ptr.data(), nbr, bdy.data(), small_level);      // (< 0: LIP_SMALL; 0: every level a launch of its own)
  int64_t launches = 0;
  const int rc = weighted ? lip_run<true>(n, M, row_ptr, nbr, W, plan, B, m, bdy_q, val, alpha, beta, T, tol, u, iters_out, err_hist, &launches, device)
                          : lip_run<false>(n, M, row_ptr, nbr, W, plan, B, m, bdy_q, val, alpha, beta, T, tol, u, iters_out, err_hist, &launches, device);
  if (plan_out) {
    plan_out[0] = plan.nlevels;
    plan_out[1] = (int64_t)plan.launches.size();
    plan_out[2] = launches;
  }
  return rc;
}
