// Shortest-path distances and closest source of graph.dijkstra / graph.dijkstra_hl: dijkstra_main and dijkstra_hl_main of the
// reference's C extension (c_code/hjsolvers.cpp:117-227) WITHOUT a priority queue, bit for bit.
//
// Why a label-correcting iteration gives the heap's bits.  The reference relaxes d[j] = relax(d[i], c_ij) under a strict `<`, with
// c_ij = fl(W[i,j] * f[i]) >= 0 and
//     plain      relax(a, c) = fl(a + c)                                                         (hjsolvers.cpp:210)
//     Hopf-Lax   relax(a, c) = fl(fl(c + sqrt(fl(fl(c*c) + fl(fl(4*a)*a)))) / 2.0)               (hjsolvers.cpp:153-154)
// In IEEE arithmetic both maps are monotone in a (every step is a correctly rounded monotone operation) and inflationary
// (relax(a, c) >= a: fl(a + c) >= a for c >= 0, and sqrt(fl(x*x)) = |x| away from under- and overflow).  Those are the two
// properties Dijkstra's correctness proof uses, so its output is the minimum, over paths from the sources, of the cost folded
// left to right along the path -- a quantity that does not depend on the order in which anybody relaxes.  Any iteration
//     u_j <- min(u_j, min over edges i->j of relax(u_i, c_ij)),     u = g on the sources, +inf elsewhere
// reaches exactly these values: every intermediate value is the folded cost of a real path (so it never undershoots), and
// monotonicity carries the optimum along the prefixes of an optimal path (so a round in which nothing moves is the fixed point).
// That holds for synchronous rounds and for IN-PLACE rounds alike: a thread that reads a neighbour's value while another thread
// lowers it sees the old or the new value -- aligned 8-byte loads and stores are single accesses -- and both are folded costs of
// real paths.  A value is written by the thread that owns it and by nobody else.  A round reads nothing older than the values at its
// launch, so it lowers at least what a synchronous round would: at most n - 1 rounds lower something, and the first that lowers
// nothing ends the iteration.
//
// Rounds.  One launch per round (no grid-wide wait, no persistent kernel); one thread per (vertex, problem), problems fastest, so
// that the B values of a neighbour are contiguous.  A round that lowers a value raises its flag; the host enqueues SSSP_CHUNK rounds,
// reads the chunk's flags once and stops at the first round that changed nothing (rounds behind it see the lowered flag of their
// predecessor and return at once).  More than n + 1 rounds cannot happen; the host refuses to go on beyond (GLX_EUNSUPPORTED).
//
// Active values.  With the graph's OUT-edge lists at hand a round only looks at the values marked for it: a value that is lowered marks
// the values its out-edges lead to for the next round (two byte maps that take turns; the first round looks at everything).  A value
// nobody marked has no in-neighbour that moved since it was last looked at, so looking at it would change nothing: the same fixed
// point, the same bound on the rounds, a round's work proportional to the frontier instead of the graph.  Without out-edge lists every
// round looks at every value (kept for measurement: EXPERIMENTS.md).
//
// max_dist.  A vertex relaxes from i only if u_i <= max_dist (the reference never expands a vertex popped above max_dist); when the
// distances have converged, values above max_dist become +inf, as the reference's documentation says (its code leaves tentative
// heap values there).
//
// Closest point, a second fixed point on the converged distances.  A source s attains its own value if u_s == g_s (and
// g_s <= max_dist); an edge i->j is tight if u_i <= max_dist, u_j < inf and relax(u_i, c_ij) == u_j; cp[j] is the smallest source
// index that reaches j along tight edges (-1: none), found by the same kind of rounds with an integer minimum.  Deterministic and
// schedule-independent; equal to the reference's closest point wherever the closest source is unique.
#include "glx_internal.h"
#include <algorithm>
#include <chrono>
#include <limits>
#include <vector>

static const int SSSP_CHUNK = 32;
static const int32_t SSSP_NO_CP = 0x7fffffff;

template <int FORM>
__device__ __forceinline__ double sssp_relax(double a, double c) {
#pragma clang fp contract(off)
  if (FORM == GLX_SSSP_PLAIN) return a + c;
  const double cc = c * c;
  const double a4 = 4 * a;          // `4*d[i]*d[i]` is (4*d[i])*d[i]
  const double aa = a4 * a;
  const double s = cc + aa;
  const double t = c + sqrt(s);
  return t / 2.0;
}

// flags[r] != 0: round r lowered something.  flags[0] is 1 (the round before a chunk always did).
// ACT: only the values marked in act_cur are looked at (and unmarked); a value that is lowered marks the values its out-edges lead to
// in act_nxt (the two byte maps take turns).
template <int FORM, bool ACT>
__global__ __launch_bounds__(256) void sssp_dist_round_kernel(double* u, const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                                                              const double* __restrict__ cost, int64_t n, int B, double max_dist, int r,
                                                              unsigned long long* flags, const int64_t* __restrict__ out_ptr,
                                                              const int32_t* __restrict__ out_idx, unsigned char* act_cur,
                                                              unsigned char* act_nxt) {
  if (flags[r - 1] == 0) return;     // uniform over the grid: the iteration ended at an earlier round
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int lowered = 0;
  if (t < n * B) {
    bool look = true;
    if (ACT) {
      look = act_cur[t] != 0;
      if (look) act_cur[t] = 0;
    }
    if (look) {
      const int64_t j = t / B;
      const int64_t b = t - j * B;
      const double mine = u[t];
      double best = mine;
      const int64_t e1 = ptr[j + 1];
      for (int64_t e = ptr[j]; e < e1; ++e) {
        const double a = u[(int64_t)idx[e] * B + b];
        if (a <= max_dist) {
          const double v = sssp_relax<FORM>(a, cost[e]);
          best = (v < best) ? v : best;
        }
      }
      if (best < mine) {
        u[t] = best;
        lowered = 1;
        if (ACT) {
          const int64_t o1 = out_ptr[j + 1];
          for (int64_t e = out_ptr[j]; e < o1; ++e) act_nxt[(int64_t)out_idx[e] * B + b] = 1;
        }
      }
    }
  }
  if (__syncthreads_or(lowered) && threadIdx.x == 0) atomicOr(&flags[r], 1ull);
}

template <int FORM, bool ACT>
__global__ __launch_bounds__(256) void sssp_cp_round_kernel(int32_t* cp, const double* __restrict__ u, const int64_t* __restrict__ ptr,
                                                            const int32_t* __restrict__ idx, const double* __restrict__ cost, int64_t n,
                                                            int B, double max_dist, int r, unsigned long long* flags,
                                                            const int64_t* __restrict__ out_ptr, const int32_t* __restrict__ out_idx,
                                                            unsigned char* act_cur, unsigned char* act_nxt) {
  if (flags[r - 1] == 0) return;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int lowered = 0;
  if (t < n * B) {
    const int64_t j = t / B;
    const int64_t b = t - j * B;
    bool look = true;
    if (ACT) {
      look = act_cur[t] != 0;
      if (look) act_cur[t] = 0;
    }
    const double uj = look ? u[t] : std::numeric_limits<double>::infinity();
    if (uj < std::numeric_limits<double>::infinity()) {
      const int32_t mine = cp[t];
      int32_t best = mine;
      const int64_t e1 = ptr[j + 1];
      for (int64_t e = ptr[j]; e < e1; ++e) {
        const int64_t s = (int64_t)idx[e] * B + b;
        const double a = u[s];
        if (a <= max_dist && sssp_relax<FORM>(a, cost[e]) == uj) {
          const int32_t c = cp[s];
          best = (c < best) ? c : best;
        }
      }
      if (best < mine) {
        cp[t] = best;
        lowered = 1;
        if (ACT) {
          const int64_t o1 = out_ptr[j + 1];
          for (int64_t e = out_ptr[j]; e < o1; ++e) act_nxt[(int64_t)out_idx[e] * B + b] = 1;
        }
      }
    }
  }
  if (__syncthreads_or(lowered) && threadIdx.x == 0) atomicOr(&flags[r], 1ull);
}

__global__ __launch_bounds__(256) void sssp_fill_kernel(double* u, int32_t* cp, int64_t total) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  if (u) u[t] = std::numeric_limits<double>::infinity();
  if (cp) cp[t] = SSSP_NO_CP;
}

// entry q: source vertex src[q] of problem prob[q] with boundary value val[q]
__global__ __launch_bounds__(256) void sssp_sources_kernel(double* u, const int32_t* __restrict__ src, const int32_t* __restrict__ prob,
                                                           const double* __restrict__ val, int64_t m, int B) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q < m) u[(int64_t)src[q] * B + prob[q]] = val[q];
}

__global__ __launch_bounds__(256) void sssp_cp_sources_kernel(int32_t* cp, const double* __restrict__ u, const int32_t* __restrict__ src,
                                                              const int32_t* __restrict__ prob, const double* __restrict__ val, int64_t m,
                                                              int B, double max_dist) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= m) return;
  const int64_t t = (int64_t)src[q] * B + prob[q];
  if (val[q] <= max_dist && u[t] == val[q]) cp[t] = src[q];
}

// every value is looked at in the first round: map 1 (odd rounds) all ones, map 0 clear
__global__ __launch_bounds__(256) void sssp_act_reset_kernel(unsigned char* act, int64_t total) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  act[t] = 0;
  act[total + t] = 1;
}

__global__ __launch_bounds__(256) void sssp_clip_kernel(double* u, int64_t total, double max_dist) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < total && u[t] > max_dist) u[t] = std::numeric_limits<double>::infinity();
}

__global__ __launch_bounds__(256) void sssp_cp_finish_kernel(int32_t* cp, int64_t total) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < total && cp[t] == SSSP_NO_CP) cp[t] = -1;
}

namespace {
// Rounds until one changes nothing.  launch(r) enqueues round r of a chunk (r = 1 .. SSSP_CHUNK).  rounds_out: rounds run, the
// idle last one included.
template <class F>
int sssp_iterate(F&& launch, unsigned long long* flags, unsigned long long* stage, int64_t cap, hipStream_t st, int64_t* rounds_out,
                 const char* what) {
  const unsigned long long one = 1;
  GLX_HIP(hipMemcpyAsync(flags, &one, 8, hipMemcpyHostToDevice, st));
  GLX_HIP(hipStreamSynchronize(st));            // (`one` lives on this frame)
  int64_t done = 0;
  for (;;) {
    GLX_CHECK(done < cap, GLX_EUNSUPPORTED, "glx_sssp: %s still change after %lld rounds (more than vertices + 1)", what, (long long)done);
    const int len = (int)std::min<int64_t>(SSSP_CHUNK, cap - done);
    GLX_UP(glx_zero_async(flags + 1, (size_t)SSSP_CHUNK * 8, st));
    for (int r = 1; r <= len; ++r) {
      launch(r);
      GLX_HIP(hipGetLastError());
    }
    GLX_HIP(hipMemcpyAsync(stage, flags + 1, (size_t)len * 8, hipMemcpyDeviceToHost, st));
    GLX_HIP(hipStreamSynchronize(st));
    for (int r = 1; r <= len; ++r)
      if (stage[r - 1] == 0) {
        *rounds_out = done + r;
        return GLX_OK;
      }
    done += len;
  }
}

template <int FORM, bool ACT>
int sssp_run(int64_t n, int64_t nnz, const int64_t* in_ptr, const int32_t* in_idx, const double* in_cost, const int64_t* out_ptr,
             const int32_t* out_idx, int B, int64_t m, const int32_t* src, const int32_t* prob, const double* val, double max_dist,
             double* dist, int32_t* cp, int64_t* rounds_out, double* ms_out, int device) {
  GlxCall call;
  GLX_UP(call.begin(device));
  hipStream_t st = call.stream();
  const auto t_start = std::chrono::steady_clock::now();
  auto ms_since = [](std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  };
  const int64_t total = n * B;
  double* d_u = nullptr;
  int32_t* d_cp = nullptr;
  int64_t *d_ptr = nullptr, *d_optr = nullptr;
  int32_t *d_idx = nullptr, *d_oidx = nullptr, *d_src = nullptr, *d_prob = nullptr;
  double *d_cost = nullptr, *d_val = nullptr;
  unsigned char* d_act = nullptr;
  unsigned long long *d_flags = nullptr, *stage = nullptr;
  GLX_UP(call.alloc(&d_u, (size_t)total));
  if (cp) GLX_UP(call.alloc(&d_cp, (size_t)total));
  GLX_UP(call.alloc(&d_ptr, (size_t)(n + 1)));
  GLX_UP(call.alloc(&d_idx, (size_t)nnz));
  GLX_UP(call.alloc(&d_cost, (size_t)nnz));
  GLX_UP(call.alloc(&d_src, (size_t)m));
  GLX_UP(call.alloc(&d_prob, (size_t)m));
  GLX_UP(call.alloc(&d_val, (size_t)m));
  GLX_UP(call.alloc(&d_flags, (size_t)SSSP_CHUNK + 1));
  if (ACT) {
    GLX_UP(call.alloc(&d_optr, (size_t)(n + 1)));
    GLX_UP(call.alloc(&d_oidx, (size_t)nnz));
    GLX_UP(call.alloc(&d_act, (size_t)total * 2));
  }
  GLX_UP(call.stage(&stage, (size_t)SSSP_CHUNK));
  GLX_UP(glx_upload(d_ptr, in_ptr, (size_t)(n + 1) * 8, st, __func__));
  if (ACT) GLX_UP(glx_upload(d_optr, out_ptr, (size_t)(n + 1) * 8, st, __func__));
  if (nnz > 0) {
    GLX_UP(glx_upload(d_idx, in_idx, (size_t)nnz * 4, st, __func__));
    GLX_UP(glx_upload(d_cost, in_cost, (size_t)nnz * 8, st, __func__));
    if (ACT) GLX_UP(glx_upload(d_oidx, out_idx, (size_t)nnz * 4, st, __func__));
  }
  if (m > 0) {
    GLX_UP(glx_upload(d_src, src, (size_t)m * 4, st, __func__));
    GLX_UP(glx_upload(d_prob, prob, (size_t)m * 4, st, __func__));
    GLX_UP(glx_upload(d_val, val, (size_t)m * 8, st, __func__));
  }
  GLX_HIP(hipStreamSynchronize(st));
  double ms[4] = {ms_since(t_start), 0, 0, 0};      // uploads, distance rounds, closest-point rounds, downloads

  const unsigned grid = (unsigned)((total + 255) / 256), grid_m = (unsigned)((m + 255) / 256);
  auto t0 = std::chrono::steady_clock::now();
  hipLaunchKernelGGL(sssp_fill_kernel, dim3(grid), dim3(256), 0, st, d_u, d_cp, total);
  GLX_HIP(hipGetLastError());
  if (m > 0) {
    hipLaunchKernelGGL(sssp_sources_kernel, dim3(grid_m), dim3(256), 0, st, d_u, (const int32_t*)d_src, (const int32_t*)d_prob,
                       (const double*)d_val, m, B);
    GLX_HIP(hipGetLastError());
  }
  if (ACT) {
    hipLaunchKernelGGL(sssp_act_reset_kernel, dim3(grid), dim3(256), 0, st, d_act, total);
    GLX_HIP(hipGetLastError());
  }
  // round r of a chunk looks at map r & 1 and marks the other one (SSSP_CHUNK is even: r & 1 is the parity of the round overall)
  static_assert(SSSP_CHUNK % 2 == 0, "the two activity maps take turns by the parity of the round");
  int64_t rounds[2] = {0, 0};
  GLX_UP(sssp_iterate(
      [&](int r) {
        hipLaunchKernelGGL((sssp_dist_round_kernel<FORM, ACT>), dim3(grid), dim3(256), 0, st, d_u, (const int64_t*)d_ptr,
                           (const int32_t*)d_idx, (const double*)d_cost, n, B, max_dist, r, d_flags, (const int64_t*)d_optr,
                           (const int32_t*)d_oidx, ACT ? d_act + (size_t)(r & 1) * total : nullptr, ACT ? d_act + (size_t)((r + 1) & 1) * total : nullptr);
      },
      d_flags, stage, n + 1, st, &rounds[0], "the distances"));
  hipLaunchKernelGGL(sssp_clip_kernel, dim3(grid), dim3(256), 0, st, d_u, total, max_dist);
  GLX_HIP(hipGetLastError());
  ms[1] = ms_since(t0);
  if (cp) {
    t0 = std::chrono::steady_clock::now();
    if (m > 0) {
      hipLaunchKernelGGL(sssp_cp_sources_kernel, dim3(grid_m), dim3(256), 0, st, d_cp, (const double*)d_u, (const int32_t*)d_src,
                         (const int32_t*)d_prob, (const double*)d_val, m, B, max_dist);
      GLX_HIP(hipGetLastError());
    }
    if (ACT) {
      hipLaunchKernelGGL(sssp_act_reset_kernel, dim3(grid), dim3(256), 0, st, d_act, total);
      GLX_HIP(hipGetLastError());
    }
    GLX_UP(sssp_iterate(
        [&](int r) {
          hipLaunchKernelGGL((sssp_cp_round_kernel<FORM, ACT>), dim3(grid), dim3(256), 0, st, d_cp, (const double*)d_u,
                             (const int64_t*)d_ptr, (const int32_t*)d_idx, (const double*)d_cost, n, B, max_dist, r, d_flags,
                             (const int64_t*)d_optr, (const int32_t*)d_oidx, ACT ? d_act + (size_t)(r & 1) * total : nullptr,
                             ACT ? d_act + (size_t)((r + 1) & 1) * total : nullptr);
        },
        d_flags, stage, n + 1, st, &rounds[1], "the closest points"));
    hipLaunchKernelGGL(sssp_cp_finish_kernel, dim3(grid), dim3(256), 0, st, d_cp, total);
    GLX_HIP(hipGetLastError());
    GLX_HIP(hipStreamSynchronize(st));
    ms[2] = ms_since(t0);
  }
  t0 = std::chrono::steady_clock::now();
  if (cp) GLX_UP(glx_download(cp, d_cp, (size_t)total * 4, st, __func__));
  GLX_UP(glx_download(dist, d_u, (size_t)total * 8, st, __func__));
  GLX_HIP(hipStreamSynchronize(st));
  ms[3] = ms_since(t0);
  if (rounds_out) {
    rounds_out[0] = rounds[0];
    rounds_out[1] = rounds[1];
  }
  if (ms_out)
    for (int q = 0; q < 4; ++q) ms_out[q] = ms[q];
  return GLX_OK;
}

// the stored entries of a CSR pattern: pointers span them, indices in range
int sssp_check_pattern(const char* which, int64_t n, int64_t nnz, const int64_t* ptr, const int32_t* idx) {
  GLX_CHECK(ptr[0] == 0 && ptr[n] == nnz, GLX_EINVAL, "glx_sssp: the %s-edge pointers do not span the %lld entries", which, (long long)nnz);
  for (int64_t j = 0; j < n; ++j)
    GLX_CHECK(ptr[j] <= ptr[j + 1], GLX_EINVAL, "glx_sssp: the %s-edge pointers decrease at vertex %lld", which, (long long)j);
  for (int64_t e = 0; e < nnz; ++e)
    GLX_CHECK(idx[e] >= 0 && idx[e] < n, GLX_EINVAL, "glx_sssp: vertex index %d of an %s-edge out of range", idx[e], which);
  return GLX_OK;
}
}  // namespace

extern "C" int glx_sssp(int64_t n, int64_t nnz, const int64_t* in_ptr, const int32_t* in_idx, const double* in_cost,
                        const int64_t* out_ptr, const int32_t* out_idx, int B, const int64_t* src_ptr, const int32_t* src_idx,
                        const double* src_val, double max_dist, int form, double* dist, int32_t* cp, int64_t* rounds_out, double* ms_out,
                        int device) {
  GLX_CHECK(in_ptr && src_ptr && dist && (nnz == 0 || (in_idx && in_cost)), GLX_EINVAL, "glx_sssp: null argument");
  GLX_CHECK(n >= 1 && nnz >= 0 && B >= 1, GLX_EINVAL, "glx_sssp: bad sizes (n=%lld nnz=%lld B=%d)", (long long)n, (long long)nnz, B);
  GLX_CHECK(form == GLX_SSSP_PLAIN || form == GLX_SSSP_HOPF_LAX, GLX_EINVAL, "glx_sssp: unknown relaxation %d", form);
  GLX_CHECK(max_dist == max_dist, GLX_EINVAL, "glx_sssp: max_dist is NaN");
  GLX_CHECK(n <= 0x7fffffff && n * (int64_t)B <= (1ll << 31), GLX_EUNSUPPORTED,
            "glx_sssp: n * B = %lld values above the supported 2^31 (split the problems into several calls)", (long long)(n * (int64_t)B));
  GLX_UP(sssp_check_pattern("in", n, nnz, in_ptr, in_idx));
  for (int64_t e = 0; e < nnz; ++e)
    GLX_CHECK(in_cost[e] >= 0, GLX_EINVAL, "glx_sssp: edge cost %g at entry %lld is negative or NaN", in_cost[e], (long long)e);
  const bool act = out_ptr != nullptr;
  if (act) {
    GLX_CHECK(nnz == 0 || out_idx, GLX_EINVAL, "glx_sssp: out-edge pointers without out-edge indices");
    GLX_UP(sssp_check_pattern("out", n, nnz, out_ptr, out_idx));
  }
  const int64_t m = src_ptr[B];
  GLX_CHECK(src_ptr[0] == 0 && m >= 0 && (m == 0 || (src_idx && src_val)), GLX_EINVAL, "glx_sssp: bad source lists");
  std::vector<int32_t> prob((size_t)std::max<int64_t>(m, 1));
  std::vector<int32_t> seen((size_t)n, 0);         // problem (1-based) that last listed the vertex: a vertex listed twice in one problem is refused
  for (int b = 0; b < B; ++b) {
    GLX_CHECK(src_ptr[b] <= src_ptr[b + 1] && src_ptr[b + 1] <= m, GLX_EINVAL, "glx_sssp: source pointers decrease at problem %d", b);
    for (int64_t q = src_ptr[b]; q < src_ptr[b + 1]; ++q) {
      const int32_t s = src_idx[q];
      GLX_CHECK(s >= 0 && s < n, GLX_EINVAL, "glx_sssp: source index %d out of range", s);
      GLX_CHECK(src_val[q] >= 0, GLX_EINVAL, "glx_sssp: boundary value %g of source %d is negative or NaN", src_val[q], s);
      GLX_CHECK(seen[s] != b + 1, GLX_EINVAL, "glx_sssp: source %d listed twice in problem %d", s, b);
      seen[s] = b + 1;
      prob[q] = b;
    }
  }
#define SSSP_RUN(F, A) \
  sssp_run<F, A>(n, nnz, in_ptr, in_idx, in_cost, out_ptr, out_idx, B, m, src_idx, prob.data(), src_val, max_dist, dist, cp, rounds_out, ms_out, device)
  if (form == GLX_SSSP_PLAIN) return act ? SSSP_RUN(GLX_SSSP_PLAIN, true) : SSSP_RUN(GLX_SSSP_PLAIN, false);
  return act ? SSSP_RUN(GLX_SSSP_HOPF_LAX, true) : SSSP_RUN(GLX_SSSP_HOPF_LAX, false);
#undef SSSP_RUN
}
