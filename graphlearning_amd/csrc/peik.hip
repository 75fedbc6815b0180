// The p-eikonal equation of graph.peikonal / ssl.peikonal: peikonal_fmm_main of the reference's C extension (c_code/hjsolvers.cpp:
// 342-420) WITHOUT a heap, as synchronous fixed-point rounds.  The arithmetic, the argument for the fixed point and the host form the
// device must equal head csrc/peik_plan.h; the local solves are the header's own functions, compiled here for the device.
//
// Rounds.  One launch per round (no grid-wide wait, no persistent kernel); one thread per (vertex, problem), problems fastest, so
// that the B values of a neighbour are contiguous.  Two value buffers take turns: round r reads the one round r - 1 wrote and writes
// every value of the other, lowered or not.  A workgroup in which a value was lowered votes in LDS and one thread stores the round's
// flag (a plain store of the same 1 from every such workgroup).  The host enqueues PEIK_CHUNK rounds, reads the chunk's flags once and
// stops at the first round that lowered nothing; rounds behind it see their predecessor's flag at zero and return at once -- the idle
// round wrote a copy, so both buffers hold the result and nothing depends on the chunk length.  More than peik_round_cap rounds (2 n + 2
// for p == 1) are refused (GLX_EUNSUPPORTED).  No floating-point atomics, no fused multiply-add: a result is a pure function of the arguments.
#include "glx_internal.h"
#include "peik_plan.h"
#include <algorithm>
#include <chrono>

static const int PEIK_CHUNK = 32;
static_assert(PEIK_CHUNK % 2 == 0, "the two value buffers take turns by the parity of the round");

// flags[r] != 0: round r lowered something.  flags[0] is 1 (the round before a chunk always did).
template <bool FAST>
__global__ __launch_bounds__(256) void peik_round_kernel(const double* __restrict__ u_old, double* __restrict__ u_new,
                                                         const unsigned char* __restrict__ fixed, const int64_t* __restrict__ ptr,
                                                         const int32_t* __restrict__ nbr, const double* __restrict__ W,
                                                         const double* __restrict__ f, int64_t n, int B, double p, int nbis, int r,
                                                         unsigned long long* flags) {
  if (flags[r - 1] == 0) return;     // uniform over the grid: the iteration ended at an earlier round
  __shared__ int vote;
  if (threadIdx.x == 0) vote = 0;
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < n * B) {
    double v = u_old[t];
    if (!fixed[t]) {
      const int64_t j = t / B;
      const int64_t b = t - j * B;
      double s;
      const bool any = FAST ? peik_solve_fast(u_old, nbr, W, ptr[j], ptr[j + 1], j, B, b, f[j], &s)
                            : peik_solve_bisect(u_old, nbr, W, ptr[j], ptr[j + 1], j, B, b, f[j], p, nbis, &s);
      if (any && s < v) {
        v = s;
        vote = 1;
      }
    }
    u_new[t] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0 && vote) flags[r] = 1ull;
}

__global__ __launch_bounds__(256) void peik_fill_kernel(double* u, unsigned char* fixed, int64_t total) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  u[t] = std::numeric_limits<double>::infinity();
  fixed[t] = 0;
}

// entry q: boundary vertex vert[q] of problem prob[q] with the value val[q]; no (vertex, problem) is listed twice (peik_make_boundary)
__global__ __launch_bounds__(256) void peik_boundary_kernel(double* u, unsigned char* fixed, const int32_t* __restrict__ vert,
                                                            const int32_t* __restrict__ prob, const double* __restrict__ val, int64_t m,
                                                            int B) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= m) return;
  const int64_t t = (int64_t)vert[q] * B + prob[q];
  u[t] = val[q];
  fixed[t] = 1;
}

// what no boundary reached takes the start value of its vertex
__global__ __launch_bounds__(256) void peik_finish_kernel(double* u, const double* __restrict__ u0, int64_t total, int B) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < total && !(u[t] < std::numeric_limits<double>::infinity())) u[t] = u0[t / B];
}

extern "C" int glx_peikonal(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* nbr, const double* W, const double* f, int B,
                            const int64_t* bdy_ptr, const int32_t* bdy_idx, const double* bdy_val, double p, int num_bisection_it,
                            const double* u0, int64_t max_rounds, double* u, int64_t* rounds_out, double* ms_out, int device) {
  GLX_CHECK(row_ptr && (M <= 0 || (nbr && W)) && f && bdy_ptr && bdy_idx && bdy_val && u0 && u, GLX_EINVAL, "glx_peikonal: null argument");
  {
    char msg[256];
    const int bad = peik_validate(n, M, row_ptr, nbr, W, f, B, bdy_ptr, bdy_idx, bdy_val, p, num_bisection_it, u0, msg, sizeof msg);
    GLX_CHECK(!bad, bad >= 9 ? GLX_EUNSUPPORTED : GLX_EINVAL, "glx_peikonal: %s", msg);
  }
  GLX_CHECK(max_rounds >= 0, GLX_EINVAL, "glx_peikonal: max_rounds=%lld is negative", (long long)max_rounds);
  PeikBoundary bd;
  peik_make_boundary(n, B, bdy_ptr, bdy_idx, bdy_val, &bd);
  const int64_t m = (int64_t)bd.vert.size();
  int64_t cap = peik_round_cap(n, p, num_bisection_it);
  if (max_rounds > 0 && max_rounds < cap) cap = max_rounds;

  GlxCall call;
  GLX_UP(call.begin(device));
  hipStream_t st = call.stream();
  auto ms_since = [](std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  };
  auto t0 = std::chrono::steady_clock::now();
  const int64_t total = n * B;
  double *d_u[2] = {nullptr, nullptr}, *d_W = nullptr, *d_f = nullptr, *d_u0 = nullptr, *d_val = nullptr;
  unsigned char* d_fixed = nullptr;
  int64_t* d_ptr = nullptr;
  int32_t *d_nbr = nullptr, *d_vert = nullptr, *d_prob = nullptr;
  unsigned long long *d_flags = nullptr, *stage = nullptr;
  GLX_UP(call.alloc(&d_u[0], (size_t)total));
  GLX_UP(call.alloc(&d_u[1], (size_t)total));
  GLX_UP(call.alloc(&d_fixed, (size_t)total));
  GLX_UP(call.alloc(&d_flags, (size_t)PEIK_CHUNK + 1));
  GLX_UP(call.stage(&stage, (size_t)PEIK_CHUNK));
  GLX_UP(call.put(&d_ptr, row_ptr, (size_t)(n + 1), __func__));
  GLX_UP(call.put(&d_nbr, nbr, (size_t)M, __func__));
  GLX_UP(call.put(&d_W, W, (size_t)M, __func__));
  GLX_UP(call.put(&d_f, f, (size_t)n, __func__));
  GLX_UP(call.put(&d_u0, u0, (size_t)n, __func__));
  GLX_UP(call.put(&d_vert, (const int32_t*)bd.vert.data(), (size_t)m, __func__));
  GLX_UP(call.put(&d_prob, (const int32_t*)bd.prob.data(), (size_t)m, __func__));
  GLX_UP(call.put(&d_val, (const double*)bd.val.data(), (size_t)m, __func__));
  const unsigned long long one = 1;
  GLX_HIP(hipMemcpyAsync(d_flags, &one, 8, hipMemcpyHostToDevice, st));
  GLX_HIP(hipStreamSynchronize(st));            // (`one` and the boundary lists live on this frame)
  double ms[3] = {ms_since(t0), 0, 0};          // uploads, rounds, download

  t0 = std::chrono::steady_clock::now();
  const unsigned grid = (unsigned)((total + 255) / 256), grid_m = (unsigned)((m + 255) / 256);
  hipLaunchKernelGGL(peik_fill_kernel, dim3(grid), dim3(256), 0, st, d_u[0], d_fixed, total);
  GLX_HIP(hipGetLastError());
  hipLaunchKernelGGL(peik_boundary_kernel, dim3(grid_m), dim3(256), 0, st, d_u[0], d_fixed, (const int32_t*)d_vert, (const int32_t*)d_prob,
                     (const double*)d_val, m, B);
  GLX_HIP(hipGetLastError());
  // round r of a chunk reads buffer (r + 1) & 1 and writes buffer r & 1: r & 1 is the parity of the round overall
  const bool fast = p == 1;
  int64_t done = 0, rounds = 0;
  while (rounds == 0) {
    GLX_CHECK(done < cap, GLX_EUNSUPPORTED, "glx_peikonal: values still fall after %lld rounds (the cap is %lld)", (long long)done,
              (long long)cap);
    const int len = (int)std::min<int64_t>(PEIK_CHUNK, cap - done);
    GLX_UP(glx_zero_async(d_flags + 1, (size_t)PEIK_CHUNK * 8, st));
    for (int r = 1; r <= len; ++r) {
      const double* src = d_u[(r + 1) & 1];
      double* dst = d_u[r & 1];
      if (fast)
        hipLaunchKernelGGL(peik_round_kernel<true>, dim3(grid), dim3(256), 0, st, src, dst, (const unsigned char*)d_fixed,
                           (const int64_t*)d_ptr, (const int32_t*)d_nbr, (const double*)d_W, (const double*)d_f, n, B, p, num_bisection_it, r,
                           d_flags);
      else
        hipLaunchKernelGGL(peik_round_kernel<false>, dim3(grid), dim3(256), 0, st, src, dst, (const unsigned char*)d_fixed,
                           (const int64_t*)d_ptr, (const int32_t*)d_nbr, (const double*)d_W, (const double*)d_f, n, B, p, num_bisection_it, r,
                           d_flags);
      GLX_HIP(hipGetLastError());
    }
    GLX_HIP(hipMemcpyAsync(stage, d_flags + 1, (size_t)len * 8, hipMemcpyDeviceToHost, st));
    GLX_HIP(hipStreamSynchronize(st));
    for (int r = 1; r <= len && rounds == 0; ++r)
      if (stage[r - 1] == 0) rounds = done + r;
    if (rounds == 0) done += len;          // every round lowered something: flags[0] = 1 holds for the next chunk too
  }
  // the idle round copied its input: both buffers hold the result
  hipLaunchKernelGGL(peik_finish_kernel, dim3(grid), dim3(256), 0, st, d_u[0], (const double*)d_u0, total, B);
  GLX_HIP(hipGetLastError());
  GLX_HIP(hipStreamSynchronize(st));
  ms[1] = ms_since(t0);
  t0 = std::chrono::steady_clock::now();
  GLX_UP(glx_download(u, d_u[0], (size_t)total * 8, st, __func__));
  GLX_HIP(hipStreamSynchronize(st));
  ms[2] = ms_since(t0);
  if (rounds_out) *rounds_out = rounds;
  if (ms_out)
    for (int q = 0; q < 3; ++q) ms_out[q] = ms[q];
  return GLX_OK;
}
