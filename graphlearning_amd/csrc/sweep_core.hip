// The driver the single Poisson sweep (glx_sweep, solver.hip) and the stacked one (glx_sweep_groups, groups.hip) share: the buffers
// of a prepared sweep, the upload helpers of a training set, the launch of one sweep, and the host loop of the stop test (reference
// graphlearning/ssl.py:631-670).  The kernel is sweep.hip's; what decides where a run stops is StopWalk (sweep_stop_plan.h), and this
// file only feeds it: every row of stop values the walk sees is one this loop has read back.
#include "glx_internal.h"
#include <string.h>
#include <algorithm>

int glx_sweep_core_create(SweepCore* c, glx_graph* P, const RecLayout& L, int C, int B, int shards, int min_iter, int max_iter, bool stop) {
  c->P = P;
  c->device = P->device;
  c->C = C;
  c->B = B;
  c->shards = shards;
  c->min_iter = min_iter;
  c->max_iter = max_iter;
  c->has_w = stop;
  c->L = L;
  c->n_rows = P->n_rows;
  c->n_cols = P->n_cols;
  c->thresh = 1.0 / (double)c->n_rows;
  GLX_UP(glx_graph_plan(P, L.G, &c->plan));
  GLX_UP(glx_work_acquire(P->device, &c->work));
  c->stream = c->work->stream;
  c->ev0 = c->work->ev[0];
  c->ev1 = c->work->ev[1];
  // (work buffers from the size-class pool of memory.hip: a dozen hipMalloc / hipFree pairs per sweep object cost milliseconds)
  const size_t xb = std::max<size_t>((size_t)c->n_cols * c->rec_bytes(), 128), bb = std::max<size_t>((size_t)c->n_rows * c->rec_bytes(), 128);
  GLX_UP(glx_pool_alloc(&c->buf[0], xb));
  GLX_UP(glx_pool_alloc(&c->buf[1], xb));
  GLX_UP(glx_pool_alloc(&c->bias, bb));
  // (on the sweep's own stream: it is non-blocking, so a null-stream memset -- asynchronous to the host --
  // would not be ordered against the first pack / upload and could land after it)
  GLX_HIP(hipMemsetAsync(c->buf[0], 0, xb, c->stream));
  GLX_HIP(hipMemsetAsync(c->buf[1], 0, xb, c->stream));
  GLX_HIP(hipMemsetAsync(c->bias, 0, bb, c->stream));
  GLX_UP(glx_pool_alloc((void**)&c->slot_has_bias, std::max<size_t>((size_t)c->nslots(), 64)));
  // (n, C) of the state dtype, and never less than two fp64 vectors (glx_sweep_set_vectors_core)
  GLX_UP(glx_pool_alloc(&c->dense, std::max<size_t>((size_t)std::max(c->n_rows, c->n_cols) * std::max(C * L.esize, 16), 64)));
  if (stop) {
    GLX_UP(glx_pool_alloc((void**)&c->deg, std::max<size_t>((size_t)c->n_rows * 8, 64)));
    GLX_UP(glx_pool_alloc((void**)&c->vinf, std::max<size_t>((size_t)c->n_rows * 8, 64)));
    GLX_UP(glx_pool_alloc((void**)&c->w0, std::max<size_t>((size_t)c->n_cols * 8 * B, 64)));
    const size_t eb = (size_t)(max_iter + 1) * c->err_row() * 8;
    GLX_UP(glx_pool_alloc((void**)&c->err, eb));
    GLX_UP(glx_pinned_alloc((void**)&c->h_err, eb));
  }
  c->walk.start(B, 0, min_iter, max_iter, c->thresh);
  return GLX_OK;
}

void glx_sweep_core_destroy(SweepCore* c) {
  glx_pool_free(c->buf[0]);
  glx_pool_free(c->buf[1]);
  glx_pool_free(c->bias);
  glx_pool_free(c->slot_has_bias);
  glx_pool_free(c->deg);
  glx_pool_free(c->vinf);
  glx_pool_free(c->w0);
  glx_pool_free(c->err);
  glx_pinned_free(c->h_err);
  glx_pool_free(c->dense);
  glx_pool_free(c->stage);
  glx_projector_destroy(c->proj);
  glx_work_release(c->work);
}

int glx_sweep_reserve(SweepCore* c, void** block, size_t* cap, size_t need) {
  if (*cap >= need) return GLX_OK;
  GLX_HIP(hipStreamSynchronize(c->stream));
  glx_pool_free(*block);
  *block = nullptr;
  *cap = 0;
  GLX_UP(glx_pool_alloc(block, 2 * need));
  *cap = 2 * need;
  return GLX_OK;
}

__global__ void permute_f64_kernel(const double* __restrict__ src, double* __restrict__ dst, const int32_t* __restrict__ perm, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[perm ? perm[i] : i];
}

// the graph's own vectors of the stop test (ssl.py:642-643): the kernel indexes them by record
int glx_sweep_set_vectors_core(SweepCore* c, const double* deg, const double* vinf) {
  const int64_t n = c->n_rows;
  if (n == 0) return GLX_OK;
  double* tmp = (double*)c->dense;
  const unsigned grid = (unsigned)((n + 255) / 256);
  GLX_UP(glx_upload(tmp, deg, (size_t)n * 8, c->stream, __func__));
  GLX_UP(glx_upload(tmp + n, vinf, (size_t)n * 8, c->stream, __func__));
  hipLaunchKernelGGL(permute_f64_kernel, dim3(grid), dim3(256), 0, c->stream, (const double*)tmp, c->deg, (const int32_t*)c->P->d_perm, n);
  hipLaunchKernelGGL(permute_f64_kernel, dim3(grid), dim3(256), 0, c->stream, (const double*)(tmp + n), c->vinf, (const int32_t*)c->P->d_perm, n);
  GLX_HIP(hipGetLastError());
  GLX_HIP(hipStreamSynchronize(c->stream));
  return GLX_OK;
}

// per-slot flag: does the row's bias record hold any nonzero, in any group?  (Poisson's Db = D^-1 b is
// nonzero on the m labelled rows only, ssl.py:620-622,636: the sweep then skips reading it.)
__global__ void glx_bias_flags_kernel(const int32_t* __restrict__ slot_row, uint8_t* __restrict__ flags, int64_t nslots,
                                      const char* __restrict__ bias, int rec_bytes) {
  const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= nslots) return;
  const int row = slot_row[slot];
  uint8_t f = 0;
  if (row >= 0) {
    const unsigned long long* r = (const unsigned long long*)(bias + (size_t)row * rec_bytes);
    for (int i = 0; i < rec_bytes / 8; ++i) f |= (r[i] << 1) != 0;   // -0.0 counts as zero
  }
  flags[slot] = f;
}

int glx_bias_flags_async(const SellPlan* plan, const void* bias, int rec_bytes, uint8_t* flags, hipStream_t st) {
  const int64_t nslots = plan->nslices * plan->R;
  if (nslots == 0) return GLX_OK;
  hipLaunchKernelGGL(glx_bias_flags_kernel, dim3((unsigned)((nslots + 255) / 256)), dim3(256), 0, st, (const int32_t*)plan->d_slot_row, flags,
                     nslots, (const char*)bias, rec_bytes);
  GLX_HIP(hipGetLastError());
  return GLX_OK;
}

template <typename T>
__global__ void scatter_rows_kernel(char* __restrict__ bias, int rec_bytes, const int32_t* __restrict__ inv, const int64_t* __restrict__ rows,
                                    const T* __restrict__ vals, const double* __restrict__ w0_rows, double* __restrict__ w0_b, int64_t m, int C,
                                    int col0) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m * C) return;
  const int64_t q = i / C;
  const int c = (int)(i % C);
  const int64_t row = rows[q];
  const int32_t rec = inv ? inv[row] : (int32_t)row;
  ((T*)(bias + (size_t)rec * rec_bytes))[col0 + c] = vals ? vals[i] : (T)0;
  if (c == 0 && w0_b) w0_b[row] = w0_rows ? w0_rows[q] : 0.0;
}

int glx_sweep_scatter_rows(SweepCore* c, const int64_t* rows, const void* vals, const double* w0_rows, double* w0_b, int64_t m, int col0) {
  const int64_t tot = m * c->C;
  if (tot == 0) return GLX_OK;
  const dim3 grid((unsigned)((tot + 255) / 256));
  if (c->P->dtype == GLX_F32)
    hipLaunchKernelGGL(scatter_rows_kernel<float>, grid, dim3(256), 0, c->stream, (char*)c->bias, (int)c->rec_bytes(), (const int32_t*)c->P->d_inv,
                       rows, (const float*)vals, w0_rows, w0_b, m, c->C, col0);
  else
    hipLaunchKernelGGL(scatter_rows_kernel<double>, grid, dim3(256), 0, c->stream, (char*)c->bias, (int)c->rec_bytes(), (const int32_t*)c->P->d_inv,
                       rows, (const double*)vals, w0_rows, w0_b, m, c->C, col0);
  GLX_HIP(hipGetLastError());
  return GLX_OK;
}

int glx_sweep_launch(SweepCore* c, int t, bool with_stop, unsigned used_mask) {
  SweepArgs a;
  memset(&a, 0, sizeof(a));
  a.plan = c->plan;
  a.L = c->L;
  a.dtype = c->P->dtype;
  a.xin = c->buf[c->cur];
  a.xout = c->buf[c->cur ^ 1];
  a.bias = c->bias_set ? c->bias : nullptr;
  a.slot_has_bias = c->bias_set ? c->slot_has_bias : nullptr;
  a.has_w = c->has_w;
  a.n_rows = c->n_rows;
  if (c->B > 1) {   // (selects the grouped kernel)
    a.ngroups = c->B;
    a.used_mask = used_mask;
  }
  if (with_stop) {
    a.deg = c->deg;
    a.vinf = c->vinf;
    a.thresh = c->thresh;
    a.err_prev = t >= c->min_iter ? c->err + (size_t)t * c->err_row() : nullptr;
    a.err_next = t + 1 >= c->min_iter ? c->err + (size_t)(t + 1) * c->err_row() : nullptr;
  }
  GLX_UP(glx_launch_spmm(a, c->stream));
  c->cur ^= 1;
  c->launches++;
  return GLX_OK;
}

int glx_sweep_capture(SweepCore* c, const std::function<int()>& enqueue, hipGraphExec_t* exec) {
  hipGraph_t graph;
  const int cur0 = c->cur;
  const int64_t launches0 = c->launches;
  GLX_HIP(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  const int rc = enqueue();
  const hipError_t e = hipStreamEndCapture(c->stream, &graph);
  c->cur = cur0;
  c->launches = launches0;
  if (rc) return rc;
  GLX_HIP(e);
  GLX_HIP(hipGraphInstantiate(exec, graph, nullptr, nullptr, 0));
  GLX_HIP(hipGraphDestroy(graph));
  return GLX_OK;
}

void glx_sweep_put_err0(SweepCore* c, const double* err0) {
  if (c->min_iter != 0) return;
  memset(c->h_err, 0, c->err_row() * 8);
  for (int b = 0; b < c->B; ++b) c->h_err[(size_t)b * c->shards] = stop_bits(err0[b]);
}

// The start of a run of the single form in ONE kernel (before: glx_zero_async + pack_kernel + write_w_kernel, 14.7 us of kernels per
// step at config 2, profiles/sweep_head.txt): every record of the start iterate written whole in 16-byte pieces -- u = 0
// (ssl.py:645) and the padding as zeros, the fp64 stop value w[perm[row]] in the first half of piece woff / 16 -- and, by the first
// workgroup, the `nerr` words of the stop row the head's last sweep does its atomic maxima into.  The bytes are those of
// glx_pack_records(nullptr, ..., w, perm), in either state dtype.
__global__ __launch_bounds__(256) void sweep_start_kernel(ulonglong2* __restrict__ rec, int64_t npieces, int pieces_per_rec, int w_piece,
                                                          const double* __restrict__ w, const int32_t* __restrict__ perm,
                                                          unsigned long long* __restrict__ err_row, int nerr) {
  if (blockIdx.x == 0)
    for (int j = threadIdx.x; j < nerr; j += 256) err_row[j] = 0ull;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npieces) return;
  const int64_t row = i / pieces_per_rec;
  ulonglong2 v = make_ulonglong2(0ull, 0ull);
  if ((int)(i - row * pieces_per_rec) == w_piece) v.x = (unsigned long long)__double_as_longlong(w[perm ? perm[row] : row]);
  rec[i] = v;
}

// The stop values the head's sweeps write are row min_iter (written by sweep min_iter - 1) and, for min_iter = 0, row 0; the rows of
// a tail chunk are cleared in front of that chunk (glx_sweep_tail) -- not all max_iter + 1 rows on every run (512 KB, 6.6 us of a
// 620 us step at config 2).  Invariant: the cleared row is zero before the sweep that does its atomic maxima into it -- stream order
// behind the kernel that clears it; for min_iter = 0 row 0 then comes from the mirror, behind that kernel in the stream.
// The stacked form (start_iterate = false) clears the row alone and resets its iterate itself (groups.hip).  The single form
// (start_iterate = true) gets its whole reset from the one start kernel: buf[0] = (u = 0, stop value w0 through perm), the row
// cleared by that kernel's first workgroup, cur = 0.
int glx_sweep_head_rows(SweepCore* c, bool start_iterate) {
  const size_t er = c->err_row(), rb = c->rec_bytes();
  unsigned long long* row = c->err + (size_t)std::min(c->min_iter, c->max_iter) * er;
  if (start_iterate) {
    GLX_CHECK(c->B == 1 && c->L.woff >= 0 && c->L.woff % 16 == 0 && rb % 16 == 0 && c->L.woff + 8 <= (int)rb, GLX_EINVAL,
              "sweep start: record of %zu bytes with its stop value at %d", rb, c->L.woff);
    const int64_t npieces = c->n_cols * (int64_t)(rb / 16);
    const unsigned grid = (unsigned)std::max<int64_t>(1, (npieces + 255) / 256);      // (an empty operator still clears its stop row)
    hipLaunchKernelGGL(sweep_start_kernel, dim3(grid), dim3(256), 0, c->stream, (ulonglong2*)c->buf[0], npieces, (int)(rb / 16), c->L.woff / 16,
                       (const double*)c->w0, (const int32_t*)c->P->d_perm, row, (int)er);
    GLX_HIP(hipGetLastError());
    c->cur = 0;
  } else {
    // (a kernel, not a memset node: this sequence is captured and replayed -- glx_zero_async, glx_internal.h)
    GLX_UP(glx_zero_async(row, er * 8, c->stream));
  }
  if (c->min_iter == 0) GLX_HIP(hipMemcpyAsync(c->err, c->h_err, er * 8, hipMemcpyHostToDevice, c->stream));
  return GLX_OK;
}

// Tail: conditional sweeps in chunks.  Every kernel decides per group from the previous sweep's maxima -- a stopped group is copied
// forward, a launch behind the last group's stop returns at once --, so over-launching is harmless and the host only reads the maxima
// back: row t in front of a chunk, rows t + 1 .. end behind it (which of the chunk's sweeps really ran?).  Ends with the run
// complete: c->walk finished, c->cur on the buffer that holds u_T.
// A run that stops at its head (the usual one: min_iter sweeps suffice) costs ONE host wait: ev1 is recorded behind the read-back of
// row `head`, and the wait for that row is the wait for the run.  A walk that goes on records ev1 again at its end.
int glx_sweep_tail(SweepCore* c, const std::function<int(int)>& launch, float* device_ms_out) {
  StopWalk& w = c->walk;
  const size_t er = c->err_row();
  int t = w.head;
  bool ended = false;      // ev1 stands behind everything enqueued, and the host has waited for it
  while (t < w.max_iter && w.running()) {
    GLX_HIP(hipMemcpyAsync(c->h_err + (size_t)t * er, c->err + (size_t)t * er, er * 8, hipMemcpyDeviceToHost, c->stream));
    const bool at_head = t == w.head;
    if (at_head) GLX_HIP(hipEventRecord(c->ev1, c->stream));
    GLX_HIP(hipStreamSynchronize(c->stream));
    w.test(t, c->h_err + (size_t)t * er, c->shards);
    if (!w.running()) {
      ended = at_head;
      break;
    }
    const int end = w.chunk_end(t), t0 = t;
    // rows t0 + 1 .. end: what this chunk's sweeps write (atomic maxima: they must start from 0)
    GLX_HIP(hipMemsetAsync(c->err + (size_t)(t0 + 1) * er, 0, (size_t)(end - t0) * er * 8, c->stream));
    for (; t < end; ++t) GLX_UP(launch(t));
    GLX_HIP(hipMemcpyAsync(c->h_err + (size_t)(t0 + 1) * er, c->err + (size_t)(t0 + 1) * er, (size_t)(end - t0) * er * 8, hipMemcpyDeviceToHost,
                           c->stream));
    GLX_HIP(hipStreamSynchronize(c->stream));
    for (int q = t0 + 1; q < end; ++q) w.test(q, c->h_err + (size_t)q * er, c->shards);   // (row `end` opens the next round)
  }
  c->cur = StopWalk::parity(w.finish());
  if (!ended) {
    GLX_HIP(hipEventRecord(c->ev1, c->stream));
    GLX_HIP(hipStreamSynchronize(c->stream));
  }
  if (device_ms_out) GLX_HIP(hipEventElapsedTime(device_ms_out, c->ev0, c->ev1));
  return GLX_OK;
}

// The stop values group b's last run compared with 1/n: vals[i] = max|v_t - v_inf| at t = *first + i, the last one being the value
// at t = T.  They are computed as deg*(P w) (the fused column), not as the reference's separate product RW*v (ssl.py:669): equal
// up to rounding.  The caller (ssl.poisson) uses them to recognise the one case in which the two roundings could decide
// differently -- a value within a few ulps of 1/n -- and settles that case with the reference's own recurrence.
int glx_sweep_stop_values_core(const SweepCore* c, int b, int64_t cap, double* vals, int* first, int* count) {
  *first = c->walk.head;
  *count = c->walk.tested_count(b);
  if (!vals) return GLX_OK;
  GLX_CHECK(cap >= *count, GLX_EINVAL, "stop values: %d values, room for %lld", *count, (long long)cap);
  for (int i = 0; i < *count; ++i) vals[i] = stop_value(c->h_err + (size_t)(*first + i) * c->err_row() + (size_t)b * c->shards, c->shards);
  return GLX_OK;
}

int glx_sweep_project_target(SweepCore* c, void** prob) {
  *prob = c->dense;
  if (c->P->dtype != GLX_F64) return GLX_OK;
  double* scores = nullptr;
  GLX_UP(glx_project_scores(&c->proj, c->n_rows, c->C, c->stream, &scores));
  *prob = scores;
  return GLX_OK;
}
