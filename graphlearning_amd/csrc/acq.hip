// Acquisition functions of active learning in the truncated eigenbasis (reference graphlearning/active_learning.py:237-575: var_opt,
// sigma_opt, model_change, model_change_var_opt), reached through graphlearning_amd.active_learning / _hip.Acq.  The handle keeps the
// eigenvectors V (n, M) and the covariance C (M, M) on the device.  The contract -- the order of every sum, every operation rounded on
// its own, the tie rule of the greedy design -- is written down in acq_plan.h and DESIGN.md 4.19 and walked on the host by
// acq_host_compute / acq_host_update / acq_host_greedy; this file is the same arithmetic on the device, bit for bit.
//
// The pass: one workgroup of 256 threads per tile of R = acq_tile_rows(M) candidates (64 at M = 50, 8 at M = 256), G = 256 / R threads
// per candidate.  The tile's rows of V are gathered into LDS, padded to an odd length so that the threads of different candidates read
// different banks.  Thread g of a candidate forms w[a] = (C v)[a] for the rows a = g, g + G, ... of C, each the chain over b, and
// leaves them in LDS; then one thread per candidate walks a in ascending order and d, s1 and s2 each take their next term.  With one
// thread per candidate the M * M dependent additions of a candidate were the whole run time (116 us at M = 50 whatever n, 10 ms at
// M = 256: profiles/active_learning.txt); split this way M * M / G + M remain.  C is read from global memory at addresses that the
// threads of a wavefront share (R = 64) or share in groups (R < 64); V is read once.  No fp64 matrix core: an MFMA's order of
// accumulation would have to be restated on the host for nothing.
// The rank-one step runs in ONE workgroup: thread a forms w[a], one thread the chain of v.w, then all of them update C.  A batch of
// queries is one launch with C in LDS between the queries (rows padded to an odd length) up to M = ACQ_UPD_LDS_M, and in the
// device's L2 beyond, where 64 KiB of LDS do not hold it; the arithmetic is the same code either way.
// The greedy design: per round the pass leaves every workgroup's best (value, position), and a finishing workgroup takes the best of
// those by the same total order, records it, strikes the vertex and applies the rank-one step to the scratch copy of C -- two launches
// per round in stream order, no floating-point atomic, no grid-wide wait, nothing read back between the rounds.
#include "glx_internal.h"
#include "acq_plan.h"
#include <mutex>
#include <vector>

struct glx_acq {
  int64_t n = 0;
  int M = 0, device = 0;
  double gamma2 = 0;
  double* d_V = nullptr;      // (n, M)
  double* d_C = nullptr;      // (M, M)
  int64_t pass_launches = 0, update_launches = 0, greedy_launches = 0;
  std::mutex mu;
};

// vals (or null): the value of every position of cand.  bval / bpos (or null): per workgroup the best position whose vertex is not
// struck in `removed`, by acq_better (bpos -1: none).  err (or null): a nonzero word ends the launch at once (a greedy round failed).
// R = acq_tile_rows(M) candidates per workgroup, G = ACQ_THREADS / R threads per candidate.
__global__ __launch_bounds__(ACQ_THREADS) void acq_pass_kernel(const double* __restrict__ V, const double* __restrict__ C,
                                                               const int32_t* __restrict__ cand, int64_t nc, const double* __restrict__ unc,
                                                               const int32_t* __restrict__ removed, const int32_t* __restrict__ err, int M, int R,
                                                               int kind, double gamma2, double* __restrict__ vals, double* __restrict__ bval,
                                                               int32_t* __restrict__ bpos) {
#pragma clang fp contract(off)
  extern __shared__ double s_dyn[];        // the tile's rows of V, then its rows of w = C v: R rows of M | 1 each
  if (err && *err) return;                 // (the same in every thread)
  const int mp = M | 1, t = threadIdx.x, G = ACQ_THREADS / R;
  const int r = t % R, q = t / R;          // candidate of the tile, and which of its G threads
  double* s_v = s_dyn;
  double* s_w = s_dyn + R * mp;
  const int64_t p0 = (int64_t)blockIdx.x * R;
  const int rows = (int)(nc - p0 < R ? nc - p0 : R);
  for (int i = t; i < rows * M; i += ACQ_THREADS) {
    const int rr = i / M, b = i - rr * M;
    s_v[rr * mp + b] = V[(int64_t)cand[p0 + rr] * M + b];
  }
  __syncthreads();
  // w[a] for the rows a = q, q + G, ... of C, each a chain over b; the threads behind the tile repeat candidate 0 into their own row
  const bool mine = r < rows;
  const double* x = s_v + (mine ? r : 0) * mp;
  double* wr = s_w + r * mp;
  for (int a = q; a < M; a += G) {
    const double* c = C + a * M;
    double w = 0.0;
    for (int b = 0; b < M; ++b) {
      const double pr = c[b] * x[b];
      w = w + pr;
    }
    wr[a] = w;
  }
  __syncthreads();
  if (t >= 64) return;                     // the first wavefront holds thread 0 of every candidate (R <= 64): the three chains over a
  const bool first = t < R && mine;
  double d = 0.0, s1 = 0.0, s2 = 0.0;
  if (first)
    for (int a = 0; a < M; ++a) {
      const double w = wr[a];
      const double pd = x[a] * w;
      d = d + pd;
      s1 = s1 + w;
      const double pq = w * w;
      s2 = s2 + pq;
    }
  const int64_t p = p0 + t;
  const double val = acq_value(kind, gamma2, d, s1, s2, (first && unc) ? unc[p] : 0.0);
  if (vals && first) vals[p] = val;
  if (bval) {
    double best = val;
    int32_t pos = (first && removed[cand[p]] == 0) ? (int32_t)p : -1;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double ov = __shfl_xor(best, off, 64);
      const int32_t op = __shfl_xor(pos, off, 64);
      if (acq_better(ov, op, best, pos)) {
        best = ov;
        pos = op;
      }
    }
    if (t == 0) {
      bval[blockIdx.x] = best;
      bpos[blockIdx.x] = pos;
    }
  }
}

// C <- C - (w w^T) / (gamma2 + v.w), w = C v, by the whole workgroup; cs has the leading dimension ld and lies in LDS or in global
// memory (only this workgroup touches it).  s_x, s_w: ACQ_MAX_M doubles each.
__device__ __forceinline__ void acq_rank_one(const double* __restrict__ v, double* cs, int ld, int M, double gamma2, double* s_x, double* s_w,
                                             double* s_den) {
#pragma clang fp contract(off)
  const int t = threadIdx.x;
  __syncthreads();          // the step before is written, s_x and s_w are free
  for (int b = t; b < M; b += ACQ_UPD_THREADS) s_x[b] = v[b];
  __syncthreads();
  for (int a = t; a < M; a += ACQ_UPD_THREADS) {
    const double* c = cs + a * ld;
    double w = 0.0;
    for (int b = 0; b < M; ++b) {
      const double pr = c[b] * s_x[b];
      w = w + pr;
    }
    s_w[a] = w;
  }
  __syncthreads();
  if (t == 0) {
    double ip = 0.0;
    for (int a = 0; a < M; ++a) {
      const double pr = s_x[a] * s_w[a];
      ip = ip + pr;
    }
    *s_den = gamma2 + ip;
  }
  __syncthreads();
  const double den = *s_den;
  for (int q = t; q < M * M; q += ACQ_UPD_THREADS) {
    const int a = q / M, b = q - a * M;
    const double pr = s_w[a] * s_w[b];
    const double qt = pr / den;
    cs[a * ld + b] = cs[a * ld + b] - qt;
  }
  __syncthreads();
}

// one workgroup: the rank-one steps of query[0 .. nq) in order
__global__ __launch_bounds__(ACQ_UPD_THREADS) void acq_update_kernel(const double* __restrict__ V, double* C, const int32_t* __restrict__ query,
                                                                     int64_t nq, int M, double gamma2, int in_lds) {
  extern __shared__ double s_c[];          // M rows of M | 1 when in_lds
  __shared__ double s_x[ACQ_MAX_M], s_w[ACQ_MAX_M], s_den;
  const int mp = M | 1, t = threadIdx.x;
  double* cs = in_lds ? s_c : C;
  const int ld = in_lds ? mp : M;
  if (in_lds)
    for (int q = t; q < M * M; q += ACQ_UPD_THREADS) {
      const int a = q / M;
      s_c[a * mp + (q - a * M)] = C[q];
    }
  for (int64_t i = 0; i < nq; ++i) acq_rank_one(V + (int64_t)query[i] * M, cs, ld, M, gamma2, s_x, s_w, &s_den);
  if (in_lds)
    for (int q = t; q < M * M; q += ACQ_UPD_THREADS) {
      const int a = q / M;
      C[q] = s_c[a * mp + (q - a * M)];
    }
}

// one workgroup: the best of the workgroups' bests of round `round`, recorded and struck, then its rank-one step on the scratch copy Cs
__global__ __launch_bounds__(ACQ_UPD_THREADS) void acq_pick_kernel(const double* __restrict__ V, double* Cs, const int32_t* __restrict__ cand,
                                                                   const double* __restrict__ bval, const int32_t* __restrict__ bpos,
                                                                   int64_t nblocks, int M, double gamma2, int round, int32_t* removed,
                                                                   int32_t* err, int32_t* __restrict__ q_out, double* __restrict__ qv_out) {
  __shared__ double s_val[ACQ_UPD_THREADS];
  __shared__ int32_t s_pos[ACQ_UPD_THREADS];
  __shared__ double s_x[ACQ_MAX_M], s_w[ACQ_MAX_M], s_den;
  __shared__ int32_t s_row;
  const int t = threadIdx.x;
  if (t == 0) s_row = *err ? -1 : 0;
  __syncthreads();
  if (s_row < 0) return;
  double best = 0.0;
  int32_t pos = -1;
  for (int64_t i = t; i < nblocks; i += ACQ_UPD_THREADS)
    if (acq_better(bval[i], bpos[i], best, pos)) {
      best = bval[i];
      pos = bpos[i];
    }
  s_val[t] = best;
  s_pos[t] = pos;
  __syncthreads();
  for (int half = ACQ_UPD_THREADS / 2; half > 0; half >>= 1) {
    if (t < half && acq_better(s_val[t + half], s_pos[t + half], s_val[t], s_pos[t])) {
      s_val[t] = s_val[t + half];
      s_pos[t] = s_pos[t + half];
    }
    __syncthreads();
  }
  if (t == 0) {
    best = s_val[0];
    pos = s_pos[0];
    if (pos < 0 || !isfinite(best)) {
      err[0] = round + 1;
      s_row = -1;
    } else {
      q_out[round] = pos;
      qv_out[round] = best;
      s_row = cand[pos];
      removed[s_row] = 1;
    }
  }
  __syncthreads();
  if (s_row < 0) return;
  acq_rank_one(V + (int64_t)s_row * M, Cs, M, M, gamma2, s_x, s_w, &s_den);
}

static void acq_free(glx_acq* h) {
  hipSetDevice(h->device);
  glx_pool_free(h->d_V);
  glx_pool_free(h->d_C);
  delete h;
}

extern "C" int glx_acq_create(int64_t n, int M, const double* V, const double* C, double gamma2, int device, glx_acq** out) {
  GLX_CHECK(out, GLX_EINVAL, "glx_acq_create: null output");
  *out = nullptr;
  GLX_CHECK(V && C, GLX_EINVAL, "glx_acq_create: null argument");
  {
    char msg[256];
    const int bad = acq_validate_state(n, M, V, C, gamma2, msg, sizeof msg);
    GLX_CHECK(!bad, bad == 8 ? GLX_EUNSUPPORTED : GLX_EINVAL, "glx_acq_create: %s", msg);
  }
  glx_acq* h = new glx_acq;
  h->n = n;
  h->M = M;
  h->device = device;
  h->gamma2 = gamma2;
  GlxCall call;
  int rc = call.begin(device);
  const bool begun = rc == GLX_OK;
  if (!rc) rc = glx_pool_alloc((void**)&h->d_V, (size_t)n * M * 8);
  if (!rc) rc = glx_pool_alloc((void**)&h->d_C, (size_t)M * M * 8);
  if (!rc) rc = glx_upload(h->d_V, V, (size_t)n * M * 8, call.stream(), __func__);
  if (!rc) rc = glx_upload(h->d_C, C, (size_t)M * M * 8, call.stream(), __func__);
  if (!rc && hipStreamSynchronize(call.stream()) != hipSuccess) {
    glx_set_error("glx_acq_create: the uploads did not complete");
    rc = GLX_EHIP;
  }
  if (rc) {
    if (begun) (void)hipStreamSynchronize(call.stream());
    acq_free(h);
    return rc;
  }
  *out = h;
  return GLX_OK;
}

extern "C" int glx_acq_destroy(glx_acq* h) {
  if (!h) return GLX_OK;
  acq_free(h);
  return GLX_OK;
}

static int acq_check_cand(const glx_acq* h, int kind, bool greedy, const int32_t* cand, int64_t nc, const char* who) {
  GLX_CHECK(nc <= 0 || cand, GLX_EINVAL, "%s: null candidates", who);
  char msg[256];
  const int bad = acq_validate_cand(h->n, kind, greedy, cand, nc, msg, sizeof msg);
  GLX_CHECK(!bad, GLX_EINVAL, "%s: %s", who, msg);
  return GLX_OK;
}

static unsigned acq_pass_blocks(int64_t nc, int R) { return (unsigned)((nc + R - 1) / R); }

extern "C" int glx_acq_compute(glx_acq* h, int kind, const int32_t* cand, int64_t nc, const double* unc, double* vals_out) {
  GLX_CHECK(h && (nc <= 0 || vals_out), GLX_EINVAL, "glx_acq_compute: null argument");
  GLX_UP(acq_check_cand(h, kind, false, cand, nc, "glx_acq_compute"));
  GLX_CHECK(unc || kind == ACQ_VAR || kind == ACQ_SIGMA, GLX_EINVAL, "glx_acq_compute: kind %d needs the multiplier unc", kind);
  if (nc == 0) return GLX_OK;
  std::lock_guard<std::mutex> lock(h->mu);
  GlxCall call;
  GLX_UP(call.begin(h->device));
  hipStream_t st = call.stream();
  int32_t* d_cand = nullptr;
  double *d_unc = nullptr, *d_vals = nullptr;
  GLX_UP(call.put(&d_cand, cand, (size_t)nc, __func__));
  if (unc) GLX_UP(call.put(&d_unc, unc, (size_t)nc, __func__));
  GLX_UP(call.alloc(&d_vals, (size_t)nc));
  const int R = acq_tile_rows(h->M);
  hipLaunchKernelGGL(acq_pass_kernel, dim3(acq_pass_blocks(nc, R)), dim3(ACQ_THREADS), acq_pass_lds_bytes(h->M), st, (const double*)h->d_V,
                     (const double*)h->d_C, (const int32_t*)d_cand, nc, (const double*)d_unc, (const int32_t*)nullptr, (const int32_t*)nullptr,
                     h->M, R, kind, h->gamma2, d_vals, (double*)nullptr, (int32_t*)nullptr);
  GLX_HIP(hipGetLastError());
  ++h->pass_launches;
  GLX_UP(glx_download(vals_out, d_vals, (size_t)nc * 8, st, __func__));
  GLX_HIP(hipStreamSynchronize(st));
  return GLX_OK;
}

extern "C" int glx_acq_update(glx_acq* h, const int32_t* query, int64_t nq) {
  GLX_CHECK(h, GLX_EINVAL, "glx_acq_update: null argument");
  GLX_UP(acq_check_cand(h, ACQ_VAR, false, query, nq, "glx_acq_update"));
  if (nq == 0) return GLX_OK;
  std::lock_guard<std::mutex> lock(h->mu);
  GlxCall call;
  GLX_UP(call.begin(h->device));
  hipStream_t st = call.stream();
  int32_t* d_q = nullptr;
  GLX_UP(call.put(&d_q, query, (size_t)nq, __func__));
  hipLaunchKernelGGL(acq_update_kernel, dim3(1), dim3(ACQ_UPD_THREADS), acq_update_lds_bytes(h->M), st, (const double*)h->d_V, h->d_C,
                     (const int32_t*)d_q, nq, h->M, h->gamma2, acq_update_in_lds(h->M) ? 1 : 0);
  GLX_HIP(hipGetLastError());
  ++h->update_launches;
  GLX_HIP(hipStreamSynchronize(st));
  return GLX_OK;
}

extern "C" int glx_acq_greedy(glx_acq* h, int kind, const int32_t* cand, int64_t nc, int64_t b, int32_t* queries_out, double* vals_out) {
  GLX_CHECK(h && (b <= 0 || (queries_out && vals_out)), GLX_EINVAL, "glx_acq_greedy: null argument");
  GLX_UP(acq_check_cand(h, kind, true, cand, nc, "glx_acq_greedy"));
  GLX_CHECK(b >= 0 && b <= nc, GLX_EINVAL, "glx_acq_greedy: %lld rounds for %lld candidates", (long long)b, (long long)nc);
  {
    const int64_t distinct = acq_distinct(cand, nc);
    GLX_CHECK(b <= distinct, GLX_EINVAL, "glx_acq_greedy: %lld rounds, but the %lld candidates name only %lld vertices", (long long)b,
              (long long)nc, (long long)distinct);
  }
  if (b == 0) return GLX_OK;
  std::lock_guard<std::mutex> lock(h->mu);
  GlxCall call;
  GLX_UP(call.begin(h->device));
  hipStream_t st = call.stream();
  const int M = h->M, R = acq_tile_rows(M);
  const unsigned nblocks = acq_pass_blocks(nc, R);
  const size_t flag_words = ((size_t)h->n + 2 + 1) & ~(size_t)1;          // removed (n), err (1), cleared in 8-byte words
  int32_t *d_cand = nullptr, *d_flags = nullptr, *d_bpos = nullptr, *d_q = nullptr;
  double *d_cs = nullptr, *d_bval = nullptr, *d_qv = nullptr;
  GLX_UP(call.put(&d_cand, cand, (size_t)nc, __func__));
  GLX_UP(call.alloc(&d_flags, flag_words));
  GLX_UP(call.alloc(&d_bpos, (size_t)nblocks));
  GLX_UP(call.alloc(&d_bval, (size_t)nblocks));
  GLX_UP(call.alloc(&d_q, (size_t)b));
  GLX_UP(call.alloc(&d_qv, (size_t)b));
  GLX_UP(call.alloc(&d_cs, (size_t)M * M));
  GLX_UP(glx_zero_async(d_flags, flag_words * 4, st));
  GLX_HIP(hipMemcpyAsync(d_cs, h->d_C, (size_t)M * M * 8, hipMemcpyDeviceToDevice, st));
  int32_t* d_removed = d_flags;
  int32_t* d_err = d_flags + h->n;
  for (int64_t r = 0; r < b; ++r) {
    hipLaunchKernelGGL(acq_pass_kernel, dim3(nblocks), dim3(ACQ_THREADS), acq_pass_lds_bytes(M), st, (const double*)h->d_V, (const double*)d_cs,
                       (const int32_t*)d_cand, nc, (const double*)nullptr, (const int32_t*)d_removed, (const int32_t*)d_err, M, R, kind,
                       h->gamma2, (double*)nullptr, d_bval, d_bpos);
    GLX_HIP(hipGetLastError());
    hipLaunchKernelGGL(acq_pick_kernel, dim3(1), dim3(ACQ_UPD_THREADS), 0, st, (const double*)h->d_V, d_cs, (const int32_t*)d_cand,
                       (const double*)d_bval, (const int32_t*)d_bpos, (int64_t)nblocks, M, h->gamma2, (int)r, d_removed, d_err, d_q, d_qv);
    GLX_HIP(hipGetLastError());
    h->greedy_launches += 2;
  }
  int32_t* h_err = nullptr;
  GLX_UP(call.stage(&h_err, (size_t)2));
  GLX_HIP(hipMemcpyAsync(h_err, d_err, 4, hipMemcpyDeviceToHost, st));
  GLX_UP(glx_download(queries_out, d_q, (size_t)b * 4, st, __func__));
  GLX_UP(glx_download(vals_out, d_qv, (size_t)b * 8, st, __func__));
  GLX_HIP(hipStreamSynchronize(st));
  GLX_CHECK(h_err[0] == 0, GLX_EINVAL, "glx_acq_greedy: round %d (0-based) has no finite maximum among its candidates", h_err[0] - 1);
  return GLX_OK;
}

extern "C" int glx_acq_get_c(glx_acq* h, double* C_out) {
  GLX_CHECK(h && C_out, GLX_EINVAL, "glx_acq_get_c: null argument");
  std::lock_guard<std::mutex> lock(h->mu);
  GlxCall call;
  GLX_UP(call.begin(h->device));
  GLX_UP(glx_download(C_out, h->d_C, (size_t)h->M * h->M * 8, call.stream(), __func__));
  GLX_HIP(hipStreamSynchronize(call.stream()));
  return GLX_OK;
}

// out: 0 launches of the pass by glx_acq_compute, 1 launches of the update, 2 launches of the greedy design (two per round), 3 candidates
// per workgroup of the pass, 4 bytes of LDS of the pass, 5 bytes of LDS of the update (0: C stays in L2), 6 n, 7 M
extern "C" int glx_acq_stats(glx_acq* h, int64_t out[8]) {
  GLX_CHECK(h && out, GLX_EINVAL, "glx_acq_stats: null argument");
  std::lock_guard<std::mutex> lock(h->mu);
  out[0] = h->pass_launches;
  out[1] = h->update_launches;
  out[2] = h->greedy_launches;
  out[3] = acq_tile_rows(h->M);
  out[4] = (int64_t)acq_pass_lds_bytes(h->M);
  out[5] = (int64_t)acq_update_lds_bytes(h->M);
  out[6] = h->n;
  out[7] = h->M;
  return GLX_OK;
}
