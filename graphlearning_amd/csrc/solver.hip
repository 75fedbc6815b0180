// Iteration drivers on top of the sliced-ELL SpMM: the Poisson sweep with its fused stop
// column (reference graphlearning/ssl.py:631-670), the PoissonMBO heat loop (ssl.py:826-827)
// and the one-shot glx_spmm_bias.  All iterations run on the device; the host only reads
// back the per-iteration stop-test maxima in small chunks.  The buffers of a prepared sweep and the loop of the stop test
// are sweep_core.hip's, shared with the stacked trials (groups.hip); this file adds the single form's head (eager first run,
// then one captured graph), its dense and row-wise problem uploads, and the heat loop.
#include "glx_internal.h"
#include <string.h>
#include <map>
#include <math.h>
#include <vector>
#include <algorithm>

static const int ERR_SHARDS = 64;

struct glx_sweep : SweepCore {
  bool use_graph = false;
  hipGraphExec_t head_exec = nullptr;       // captured: reset + min_iter unconditional sweeps
  int64_t runs = 0;                         // glx_sweep_run calls so far (the first one launches eagerly)
  std::map<long, hipGraphExec_t> iter_exec; // heat loop graphs keyed by (iters, parity)
  double err0 = 0.0;
  // sparse right-hand side (glx_sweep_set_problem_rows): the rows set by the previous call.  Pooled blocks like the core's.
  int32_t* row_slot = nullptr;              // [n_rows] record index -> its (first) slot in the plan
  void* prev = nullptr;                     // [cap] rows in the caller's numbering (for w0), then [cap] their record indices
  size_t prev_bytes = 0;                    // cap = prev_bytes / 12
  int64_t prev_m = 0;
  bool vectors_set = false;
  int64_t* prev_row() const { return (int64_t*)prev; }
  int32_t* prev_rec() const { return (int32_t*)(prev_row() + prev_bytes / 12); }
};

static size_t rec_bytes(const glx_sweep* s, int64_t rows) { return (size_t)rows * s->rec_bytes(); }

extern "C" int glx_sweep_destroy(glx_sweep* s) {
  if (!s) return GLX_OK;
  hipSetDevice(s->device);
  if (s->stream) hipStreamSynchronize(s->stream);
  if (s->head_exec) hipGraphExecDestroy(s->head_exec);
  for (auto& kv : s->iter_exec) hipGraphExecDestroy(kv.second);
  glx_pool_free(s->row_slot);
  glx_pool_free(s->prev);
  glx_sweep_core_destroy(s);
  delete s;
  return GLX_OK;
}

extern "C" int glx_sweep_create(glx_graph* P, int C, int min_iter, int max_iter, int use_hipgraph, glx_sweep** out) {
  GLX_CHECK(P && out, GLX_EINVAL, "glx_sweep_create: null argument");
  *out = nullptr;
  GLX_CHECK(min_iter >= 0 && max_iter >= 0, GLX_EINVAL, "glx_sweep_create: negative iteration bound");
  GLX_HIP(hipSetDevice(P->device));
  RecLayout L;
  GLX_UP(glx_make_layout(C, P->dtype, max_iter > 0, &L));
  glx_sweep* s = new glx_sweep();
  s->use_graph = use_hipgraph != 0;
  int rc = glx_sweep_core_create(s, P, L, C, 1, ERR_SHARDS, min_iter, max_iter, max_iter > 0);
  if (rc) { glx_sweep_destroy(s); return rc; }
  *out = s;
  return GLX_OK;
}

// captured launch sequences bake in whether a bias is read: drop them when that changes
static void drop_graphs_if_bias_changes(glx_sweep* s, bool will_have_bias) {
  if (s->bias_set == will_have_bias) return;
  if (s->head_exec) { hipGraphExecDestroy(s->head_exec); s->head_exec = nullptr; }
  for (auto& kv : s->iter_exec) hipGraphExecDestroy(kv.second);
  s->iter_exec.clear();
}

static int zero_bias(glx_sweep* s) {
  GLX_HIP(hipMemsetAsync(s->bias, 0, rec_bytes(s, s->n_rows), s->stream));
  GLX_HIP(hipMemsetAsync(s->slot_has_bias, 0, std::max<int64_t>(s->nslots(), 1), s->stream));
  return GLX_OK;
}

static int upload_bias(glx_sweep* s, const void* Db) {
  drop_graphs_if_bias_changes(s, Db != nullptr);
  s->bias_set = Db != nullptr;
  if (!Db) return zero_bias(s);
  GLX_UP(glx_upload(s->dense, Db, (size_t)s->n_rows * s->C * s->L.esize, s->stream, __func__));
  GLX_UP(glx_pack_records(s->dense, s->bias, s->n_rows, s->L, s->P->dtype, nullptr, s->stream, s->P->d_perm));
  return glx_bias_flags_async(s->plan, s->bias, (int)s->rec_bytes(), s->slot_has_bias, s->stream);
}

extern "C" int glx_sweep_set_problem(glx_sweep* s, const void* Db, const double* w0, const double* deg, const double* vinf) {
  GLX_CHECK(s, GLX_EINVAL, "glx_sweep_set_problem: null sweep");
  GLX_CHECK(s->has_w, GLX_EINVAL, "glx_sweep_set_problem: sweep was created without a stop column (max_iter = 0)");
  GLX_CHECK(w0 && deg && vinf, GLX_EINVAL, "glx_sweep_set_problem: null vector");
  GLX_CHECK(s->n_rows == s->n_cols, GLX_EINVAL, "glx_sweep_set_problem: operator must be square");
  GLX_HIP(hipSetDevice(s->P->device));
  if (s->row_slot) {   // a later sparse problem starts from scratch
    GLX_HIP(hipStreamSynchronize(s->stream));   // (nothing in flight may still read a block the pool hands on)
    glx_pool_free(s->row_slot);
    s->row_slot = nullptr;
    s->prev_m = 0;
  }
  GLX_UP(upload_bias(s, Db));
  s->vectors_set = true;
  GLX_UP(glx_upload(s->w0, w0, s->n_cols * 8, s->stream, __func__));   // caller order; packed through perm
  std::vector<double> degp, vinfp;
  if (!s->P->h_perm.empty()) {   // the kernel indexes deg / vinf by renumbered row
    degp.resize(s->n_rows);
    vinfp.resize(s->n_rows);
    for (int64_t i = 0; i < s->n_rows; ++i) { degp[i] = deg[s->P->h_perm[i]]; vinfp[i] = vinf[s->P->h_perm[i]]; }
  }
  GLX_UP(glx_upload(s->deg, degp.empty() ? deg : degp.data(), s->n_rows * 8, s->stream, __func__));
  GLX_UP(glx_upload(s->vinf, vinfp.empty() ? vinf : vinfp.data(), s->n_rows * 8, s->stream, __func__));
  double e0 = 0.0;
  for (int64_t i = 0; i < s->n_rows; ++i) {
    const double e = fabs(deg[i] * w0[i] - vinf[i]);
    if (e > e0 || e != e) e0 = e;
    if (e != e) break;   // np.max keeps the NaN
  }
  s->err0 = e0;
  GLX_HIP(hipStreamSynchronize(s->stream));
  return GLX_OK;
}

// ---- sparse problem upload -------------------------------------------------------------------------
// Poisson's right-hand side Db = D^-1 b and the initial stop vector v0 are nonzero on the m labelled rows only
// (ssl.py:620-622, 639-641): a new training set on a resident graph then costs a few KB of upload instead of a
// dense (n, C) array, and the graph's own vectors (deg, vinf) are uploaded once.
extern "C" int glx_sweep_set_vectors(glx_sweep* s, const double* deg, const double* vinf) {
  GLX_CHECK(s && deg && vinf, GLX_EINVAL, "glx_sweep_set_vectors: null argument");
  GLX_CHECK(s->has_w, GLX_EINVAL, "glx_sweep_set_vectors: sweep was created without a stop column (max_iter = 0)");
  GLX_CHECK(s->n_rows == s->n_cols, GLX_EINVAL, "glx_sweep_set_vectors: operator must be square");
  GLX_HIP(hipSetDevice(s->device));
  GLX_UP(glx_sweep_set_vectors_core(s, deg, vinf));
  s->vectors_set = true;
  return GLX_OK;
}

__global__ void row_slot_kernel(const int32_t* __restrict__ slot_row, int32_t* __restrict__ row_slot, int64_t nslots) {
  const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= nslots) return;
  const int row = slot_row[slot];
  // the first of a long row's S consecutive slots is the one whose lanes store (and read the bias flag)
  if (row >= 0 && (slot == 0 || slot_row[slot - 1] != row)) row_slot[row] = (int32_t)slot;
}

template <typename T>
__global__ void clear_rows_kernel(char* __restrict__ bias, int rec_bytes, uint8_t* __restrict__ flags, const int32_t* __restrict__ row_slot,
                                  double* __restrict__ w0, const int32_t* __restrict__ prev_rec, const int64_t* __restrict__ prev_row,
                                  int64_t m, int ld) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m * ld) return;
  const int64_t q = i / ld;
  const int c = (int)(i % ld);
  const int32_t rec = prev_rec[q];
  ((T*)(bias + (size_t)rec * rec_bytes))[c] = 0;
  if (c == 0) {
    flags[row_slot[rec]] = 0;
    w0[prev_row[q]] = 0.0;
  }
}

template <typename T>
__global__ void set_rows_kernel(char* __restrict__ bias, int rec_bytes, uint8_t* __restrict__ flags, const int32_t* __restrict__ row_slot,
                                double* __restrict__ w0, const int64_t* __restrict__ rows, const int32_t* __restrict__ inv,
                                const T* __restrict__ Db_rows, const double* __restrict__ w0_rows, int64_t m, int C,
                                int32_t* __restrict__ prev_rec, int64_t* __restrict__ prev_row) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m * C) return;
  const int64_t q = i / C;
  const int c = (int)(i % C);
  const int64_t row = rows[q];
  const int32_t rec = inv ? inv[row] : (int32_t)row;
  const T v = Db_rows[i];
  ((T*)(bias + (size_t)rec * rec_bytes))[c] = v;
  // flag: any nonzero in the record (-0.0 counts as zero, like glx_bias_flags_kernel); benign race: every writer stores 1
  bool nz;
  if constexpr (sizeof(T) == 8) nz = ((unsigned long long)__double_as_longlong((double)v) << 1) != 0;
  else nz = ((unsigned)__float_as_int((float)v) << 1) != 0;
  if (nz) flags[row_slot[rec]] = 1;
  if (c == 0) {
    w0[row] = w0_rows[q];
    prev_rec[q] = rec;
    prev_row[q] = row;
  }
}

extern "C" int glx_sweep_set_problem_rows(glx_sweep* s, int64_t m, const int64_t* rows, const void* Db_rows, const double* w0_rows,
                                          double err0) {
  GLX_CHECK(s, GLX_EINVAL, "glx_sweep_set_problem_rows: null sweep");
  GLX_CHECK(s->has_w, GLX_EINVAL, "glx_sweep_set_problem_rows: sweep was created without a stop column (max_iter = 0)");
  GLX_CHECK(s->vectors_set, GLX_EINVAL, "glx_sweep_set_problem_rows: call glx_sweep_set_vectors first");
  GLX_CHECK(m >= 0 && (m == 0 || (rows && Db_rows && w0_rows)), GLX_EINVAL, "glx_sweep_set_problem_rows: null array");
  for (int64_t q = 0; q < m; ++q)
    GLX_CHECK(rows[q] >= 0 && rows[q] < s->n_rows, GLX_EINVAL, "glx_sweep_set_problem_rows: row %lld out of range", (long long)rows[q]);
  GLX_HIP(hipSetDevice(s->device));
  const int64_t nslots = s->nslots();
  const int rb = (int)s->rec_bytes();
  const bool f32 = s->P->dtype == GLX_F32;
  if (!s->row_slot) {
    GLX_UP(glx_pool_alloc((void**)&s->row_slot, std::max<size_t>((size_t)s->n_rows * 4, 64)));
    if (nslots > 0) {
      hipLaunchKernelGGL(row_slot_kernel, dim3((unsigned)((nslots + 255) / 256)), dim3(256), 0, s->stream, (const int32_t*)s->plan->d_slot_row,
                         s->row_slot, nslots);
      GLX_HIP(hipGetLastError());
    }
    // from a dense problem to sparse ones: start from an all-zero bias
    GLX_UP(zero_bias(s));
    GLX_HIP(hipMemsetAsync(s->w0, 0, std::max<size_t>(s->n_cols * 8, 8), s->stream));
    s->prev_m = 0;
  }
  drop_graphs_if_bias_changes(s, true);
  if (s->prev_m > 0) {
    const dim3 grid((unsigned)((s->prev_m * s->L.ld + 255) / 256));
    auto* clear = f32 ? clear_rows_kernel<float> : clear_rows_kernel<double>;
    hipLaunchKernelGGL(clear, grid, dim3(256), 0, s->stream, (char*)s->bias, rb, s->slot_has_bias, (const int32_t*)s->row_slot, s->w0,
                       (const int32_t*)s->prev_rec(), (const int64_t*)s->prev_row(), s->prev_m, s->L.ld);
    GLX_HIP(hipGetLastError());
    s->prev_m = 0;
  }
  if (m > 0) {
    GLX_UP(glx_sweep_reserve(s, &s->prev, &s->prev_bytes, (size_t)m * 12));   // (the clear above may still be reading the old block)
    const size_t es = s->L.esize;
    const size_t b_rows = (size_t)m * 8, b_db = ((size_t)m * s->C * es + 7) / 8 * 8, b_w = (size_t)m * 8;
    GLX_UP(glx_sweep_reserve(s, &s->stage, &s->stage_cap, b_rows + b_db + b_w));
    char* st = (char*)s->stage;
    GLX_UP(glx_upload(st, rows, b_rows, s->stream, __func__));
    GLX_UP(glx_upload(st + b_rows, Db_rows, (size_t)m * s->C * es, s->stream, __func__));
    GLX_UP(glx_upload(st + b_rows + b_db, w0_rows, b_w, s->stream, __func__));
    const dim3 grid((unsigned)((m * s->C + 255) / 256));
    if (f32)
      hipLaunchKernelGGL(set_rows_kernel<float>, grid, dim3(256), 0, s->stream, (char*)s->bias, rb, s->slot_has_bias, (const int32_t*)s->row_slot,
                         s->w0, (const int64_t*)st, (const int32_t*)s->P->d_inv, (const float*)(st + b_rows), (const double*)(st + b_rows + b_db), m,
                         s->C, s->prev_rec(), s->prev_row());
    else
      hipLaunchKernelGGL(set_rows_kernel<double>, grid, dim3(256), 0, s->stream, (char*)s->bias, rb, s->slot_has_bias, (const int32_t*)s->row_slot,
                         s->w0, (const int64_t*)st, (const int32_t*)s->P->d_inv, (const double*)(st + b_rows), (const double*)(st + b_rows + b_db), m,
                         s->C, s->prev_rec(), s->prev_row());
    GLX_HIP(hipGetLastError());
    s->prev_m = m;
  }
  s->bias_set = true;
  s->err0 = err0;
  GLX_HIP(hipStreamSynchronize(s->stream));   // the host arrays may go; the staging is reused by the next call
  return GLX_OK;
}

static int enqueue_iterate(glx_sweep* s, int iters);

// reset state (one kernel: u = 0 (ssl.py:645), w = w0, the head's stop row cleared) + the min_iter unconditional sweeps; identical
// every run -> capturable
static int enqueue_head(glx_sweep* s) {
  GLX_UP(glx_sweep_head_rows(s, true));
  for (int t = 0; t < s->walk.head; ++t) GLX_UP(glx_sweep_launch(s, t, true, 0));
  return GLX_OK;
}

extern "C" int glx_sweep_run(glx_sweep* s, int* T_out, float* device_ms_out) {
  GLX_CHECK(s && s->has_w, GLX_EINVAL, "glx_sweep_run: sweep has no stop column");
  GLX_HIP(hipSetDevice(s->P->device));
  const int64_t launches0 = s->launches;
  s->walk.start(1, 1, s->min_iter, s->max_iter, s->thresh);
  GLX_HIP(hipEventRecord(s->ev0, s->stream));
  glx_sweep_put_err0(s, &s->err0);
  // A model that is fitted once never earns its launch graph back: capture + instantiate + the first launch of a fresh executable graph +
  // its destruction cost 1.1-1.4 ms against 0.35 ms of launching the same 50 sweeps one by one (they run behind each other either way:
  // 0.62 ms of device time; profiles/r06_fresh_path.txt).  The first run of a sweep object therefore launches eagerly; the graph is captured
  // on the second run and replayed from then on.  Same kernels, same order: the iterates do not depend on the form.
  // The graph is the start kernel (sweep_start_kernel, sweep_core.hip: the whole reset in one node) and the min_iter sweeps -- 51 kernel
  // nodes at config 2 -- plus, for min_iter = 0 only, the upload of stop row 0 behind the start kernel.  Launching the start kernel and
  // sweep 0 directly and replaying sweeps 1 .. only ("primed replay") was measured and is not done: 0.618 against 0.616 ms per step
  // (profiles/sweep_head.txt).
  const bool replay = s->use_graph && (s->runs > 0 || s->head_exec);
  ++s->runs;
  if (replay) {
    if (!s->head_exec) GLX_UP(glx_sweep_capture(s, [&]() { return enqueue_head(s); }, &s->head_exec));
    GLX_HIP(hipGraphLaunch(s->head_exec, s->stream));
    s->cur = s->walk.head & 1;
  } else {
    GLX_UP(enqueue_head(s));
  }
  GLX_UP(glx_sweep_tail(s, [&](int t) { return glx_sweep_launch(s, t, true, 0); }, device_ms_out));
  if (T_out) *T_out = s->walk.T[0];
  // count the sweeps that really ran: kernels of a tail chunk launched past the stop test exit at once
  s->launches = launches0 + s->walk.T[0];
  return GLX_OK;
}

extern "C" int glx_sweep_stop_values(const glx_sweep* s, int64_t cap, double* vals, int* first, int* count) {
  GLX_CHECK(s && first && count, GLX_EINVAL, "glx_sweep_stop_values: null argument");
  return glx_sweep_stop_values_core(s, 0, cap, vals, first, count);
}

extern "C" int glx_sweep_fetch(glx_sweep* s, void* u_out) {
  GLX_CHECK(s && u_out, GLX_EINVAL, "glx_sweep_fetch: null argument");
  GLX_HIP(hipSetDevice(s->P->device));
  int rc = glx_unpack_records(s->buf[s->cur], s->dense, s->n_rows, s->L, s->P->dtype, s->stream, s->P->d_perm);
  if (rc) return rc;
  GLX_UP(glx_download(u_out, s->dense, (size_t)s->n_rows * s->C * s->L.esize, s->stream, __func__));
  GLX_HIP(hipStreamSynchronize(s->stream));
  return GLX_OK;
}

// ssl.predict / ssl.volume_label_projection (ssl.py:230-266, 172-209) on the sweep's current state
// without a host round trip; with to_onehot the state is then replaced by onehot(labels), which is
// the hand-over between the heat sweeps and the thresholding of PoissonMBO (ssl.py:826-832).
// then_iterate > 0 (needs to_onehot): that many sweeps are enqueued behind the one-hot state before the host has even seen the
// decision -- PoissonMBO's next heat chunk (ssl.py:826-832) starts where the thresholding ends instead of two host round trips later
// (~75 us of idle device per outer step at config 5, profiles/r04_mbo_step.txt).
extern "C" int glx_sweep_project_iterate(glx_sweep* s, const double* priors, double* weights_inout, int64_t* labels_out, double* err_out,
                                         int* steps_out, int max_steps, int similarity, int to_onehot, int then_iterate) {
  GLX_CHECK(s && weights_inout, GLX_EINVAL, "glx_sweep_project: null argument");
  GLX_CHECK(!s->has_w || !to_onehot, GLX_EINVAL, "glx_sweep_project: to_onehot needs a sweep created with max_iter = 0");
  GLX_CHECK(then_iterate >= 0 && (then_iterate == 0 || (to_onehot && s->n_rows == s->n_cols)), GLX_EINVAL,
            "glx_sweep_project: then_iterate needs to_onehot and a square operator");
  GLX_HIP(hipSetDevice(s->device));
  const int dtype = s->P->dtype;
  void* prob = nullptr;
  GLX_UP(glx_sweep_project_target(s, &prob));
  GLX_UP(glx_unpack_records(s->buf[s->cur], prob, s->n_rows, s->L, dtype, s->stream, s->P->d_perm));
  const long long* d_labels = nullptr;
  // what goes with the decision (the labels, waited for) and what follows it (the one-hot state, the next sweeps: enqueued, not
  // awaited -- the next call on this sweep is ordered behind them in its stream)
  const std::function<int(bool)> hook = [&](bool after) -> int {
    if (!after) {
      if (labels_out) GLX_UP(glx_download(labels_out, d_labels, (size_t)s->n_rows * 8, s->stream, __func__));
      return GLX_OK;
    }
    if (to_onehot) {
      int rh = glx_onehot_records(d_labels, s->buf[s->cur], dtype, s->n_cols, s->L, s->P->d_perm, s->stream);
      if (rh) return rh;
    }
    return then_iterate > 0 ? enqueue_iterate(s, then_iterate) : GLX_OK;
  };
  return glx_project_device(&s->proj, prob, dtype, s->n_rows, s->C, priors, weights_inout, err_out, steps_out, max_steps, similarity,
                            s->stream, &d_labels, &hook);
}

extern "C" int glx_sweep_launches(const glx_sweep* s, int64_t* n) {
  GLX_CHECK(s && n, GLX_EINVAL, "glx_sweep_launches: null argument");
  *n = s->launches;
  return GLX_OK;
}

extern "C" int glx_sweep_set_state(glx_sweep* s, const void* u0, const void* Db) {
  GLX_CHECK(s, GLX_EINVAL, "glx_sweep_set_state: null sweep");
  GLX_CHECK(!s->has_w, GLX_EINVAL, "glx_sweep_set_state: only for sweeps created with max_iter = 0");
  GLX_HIP(hipSetDevice(s->P->device));
  int rc = upload_bias(s, Db);
  if (rc) return rc;
  GLX_HIP(hipStreamSynchronize(s->stream));   // `dense` staging is reused below
  if (u0) {
    GLX_UP(glx_upload(s->dense, u0, (size_t)s->n_cols * s->C * s->L.esize, s->stream, __func__));
    rc = glx_pack_records(s->dense, s->buf[0], s->n_cols, s->L, s->P->dtype, nullptr, s->stream, s->P->d_perm);
  } else {
    rc = glx_pack_records(nullptr, s->buf[0], s->n_cols, s->L, s->P->dtype, nullptr, s->stream);
  }
  if (rc) return rc;
  s->cur = 0;
  GLX_HIP(hipStreamSynchronize(s->stream));
  return GLX_OK;
}

extern "C" int glx_sweep_set_state_labels(glx_sweep* s, const int64_t* labels, int64_t m, const int64_t* rows, const void* Db_rows) {
  GLX_CHECK(s && labels, GLX_EINVAL, "glx_sweep_set_state_labels: null argument");
  GLX_CHECK(!s->has_w, GLX_EINVAL, "glx_sweep_set_state_labels: only for sweeps created with max_iter = 0");
  GLX_CHECK(s->n_rows == s->n_cols, GLX_EINVAL, "glx_sweep_set_state_labels: operator must be square");
  GLX_CHECK(m >= 0 && (m == 0 || (rows && Db_rows)), GLX_EINVAL, "glx_sweep_set_state_labels: null array");
  for (int64_t q = 0; q < m; ++q)
    GLX_CHECK(rows[q] >= 0 && rows[q] < s->n_rows, GLX_EINVAL, "glx_sweep_set_state_labels: row %lld out of range", (long long)rows[q]);
  GLX_HIP(hipSetDevice(s->P->device));
  const size_t es = s->L.esize;
  const size_t b_lab = (size_t)s->n_rows * 8, b_rows = (size_t)m * 8, b_db = ((size_t)m * s->C * es + 7) / 8 * 8;
  GLX_UP(glx_sweep_reserve(s, &s->stage, &s->stage_cap, b_lab + b_rows + b_db));
  char* st = (char*)s->stage;
  drop_graphs_if_bias_changes(s, m > 0);
  GLX_UP(glx_upload(st, labels, b_lab, s->stream, __func__));
  GLX_UP(glx_onehot_records((const long long*)st, s->buf[0], s->P->dtype, s->n_rows, s->L, s->P->d_perm, s->stream));   // u = onehot(labels)
  GLX_UP(zero_bias(s));
  if (m > 0) {   // (heat sweeps: no stop column, and no flags per row beyond glx_bias_flags_kernel's pass)
    GLX_UP(glx_upload(st + b_lab, rows, b_rows, s->stream, __func__));
    GLX_UP(glx_upload(st + b_lab + b_rows, Db_rows, (size_t)m * s->C * es, s->stream, __func__));
    GLX_UP(glx_sweep_scatter_rows(s, (const int64_t*)(st + b_lab), st + b_lab + b_rows, nullptr, nullptr, m, 0));
    GLX_UP(glx_bias_flags_async(s->plan, s->bias, (int)s->rec_bytes(), s->slot_has_bias, s->stream));
  }
  s->bias_set = m > 0;
  s->cur = 0;
  GLX_HIP(hipStreamSynchronize(s->stream));   // the host arrays may go
  return GLX_OK;
}

static int enqueue_iterate(glx_sweep* s, int iters) {
  const auto sweeps = [&]() -> int {
    for (int t = 0; t < iters; ++t) GLX_UP(glx_sweep_launch(s, t, false, 0));
    return GLX_OK;
  };
  if (!s->use_graph || iters <= 1) return sweeps();
  const long key = (long)iters * 4 + s->cur * 2 + (s->bias_set ? 1 : 0);
  auto it = s->iter_exec.find(key);
  if (it == s->iter_exec.end()) {
    hipGraphExec_t exec;
    GLX_UP(glx_sweep_capture(s, sweeps, &exec));
    it = s->iter_exec.emplace(key, exec).first;
  }
  GLX_HIP(hipGraphLaunch(it->second, s->stream));
  s->cur ^= (iters & 1);
  s->launches += iters;
  return GLX_OK;
}

extern "C" int glx_sweep_iterate(glx_sweep* s, int iters) {
  GLX_CHECK(s && iters >= 0, GLX_EINVAL, "glx_sweep_iterate: bad argument");
  GLX_CHECK(!s->has_w, GLX_EINVAL, "glx_sweep_iterate: only for sweeps created with max_iter = 0");
  GLX_CHECK(s->n_rows == s->n_cols, GLX_EINVAL, "glx_sweep_iterate: operator must be square");
  GLX_HIP(hipSetDevice(s->P->device));
  // (enqueued, not awaited: whatever reads the state next -- glx_sweep_project, glx_sweep_fetch, another glx_sweep_iterate -- runs
  // in this sweep's stream behind it; PoissonMBO's 20 outer steps each saved a host round trip)
  return enqueue_iterate(s, iters);
}

extern "C" int glx_spmm_bias(glx_graph* A, const void* Db, const void* u_in, void* u_out, int C, int iters) {
  GLX_CHECK(A && u_in && u_out, GLX_EINVAL, "glx_spmm_bias: null argument");
  GLX_CHECK(iters >= 0, GLX_EINVAL, "glx_spmm_bias: negative iters");
  GLX_CHECK(A->n_rows == A->n_cols || iters <= 1, GLX_EINVAL, "glx_spmm_bias: iterating needs a square operator");
  glx_sweep* s = nullptr;
  int rc = glx_sweep_create(A, C, 0, 0, 0, &s);
  if (rc) return rc;
  rc = glx_sweep_set_state(s, u_in, Db);
  if (!rc) {
    for (int t = 0; t < iters && !rc; ++t) rc = glx_sweep_launch(s, t, false, 0);
    if (!rc && hipStreamSynchronize(s->stream) != hipSuccess) { glx_set_error("glx_spmm_bias: sync failed"); rc = GLX_EHIP; }
  }
  if (!rc) rc = glx_sweep_fetch(s, u_out);
  glx_sweep_destroy(s);
  return rc;
}

// ---- affine fixed-point iteration with a sup-norm stop ---------------------------------------
// u <- A u + b until max |u_new - u_old| <= tol: the power iteration of graph.page_rank
// (graphlearning/graph.py:1405-1410: `w = alpha*P@u + (1-alpha)*v ; err = np.max(np.absolute(w-u))`,
// `while err > tol`).  The records of both iterates are compared element by element (padding is 0
// in both); NaN bit patterns order above +inf, so a NaN difference ends the loop like `nan > tol`.
template <typename T>
__global__ __launch_bounds__(256) void absdiff_max_kernel(const T* __restrict__ a, const T* __restrict__ b, int64_t total,
                                                          unsigned long long* __restrict__ out) {
  unsigned long long m = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const T d = a[i] - b[i];                  // the subtraction in the array dtype, like numpy
    const double ad = fabs((double)d);
    const unsigned long long u = (unsigned long long)__double_as_longlong(ad);
    m = u > m ? u : m;
  }
  __shared__ unsigned long long s_m[256];
  s_m[threadIdx.x] = m;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off && s_m[threadIdx.x + off] > s_m[threadIdx.x]) s_m[threadIdx.x] = s_m[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0 && s_m[0] != 0) atomicMax(out, s_m[0]);
}

extern "C" int glx_affine_iterate(glx_graph* A, const void* b, const void* u0, void* u_out, int C, double tol, int64_t max_iter,
                                  int64_t* iters_out, double* err_out) {
  GLX_CHECK(A && u0 && u_out, GLX_EINVAL, "glx_affine_iterate: null argument");
  GLX_CHECK(A->n_rows == A->n_cols, GLX_EINVAL, "glx_affine_iterate: operator must be square");
  GLX_CHECK(max_iter >= 0, GLX_EINVAL, "glx_affine_iterate: negative max_iter");
  glx_sweep* s = nullptr;
  int rc = glx_sweep_create(A, C, 0, 0, 0, &s);
  if (rc) return rc;
  rc = glx_sweep_set_state(s, u0, b);
  unsigned long long* d_err = nullptr;
  unsigned long long* h_err = nullptr;
  int64_t it = 0;
  double err = tol + 1.0;                      // graph.py:1404
  if (!rc && hipMalloc(&d_err, 8) != hipSuccess) { glx_set_error("glx_affine_iterate: hipMalloc failed"); rc = GLX_EHIP; }
  if (!rc && hipHostMalloc((void**)&h_err, 8, hipHostMallocDefault) != hipSuccess) { glx_set_error("glx_affine_iterate: hipHostMalloc failed"); rc = GLX_EHIP; }
  const int64_t total = s ? (int64_t)s->n_rows * s->L.ld : 0;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(1024, (total + 255) / 256));
  while (!rc && err > tol && it < max_iter) {
    hipError_t e = hipMemsetAsync(d_err, 0, 8, s->stream);
    if (e == hipSuccess) {
      rc = glx_sweep_launch(s, (int)(it & 1), false, 0);
      if (rc) break;
      if (A->dtype == GLX_F32)
        hipLaunchKernelGGL(absdiff_max_kernel<float>, dim3(grid), dim3(256), 0, s->stream, (const float*)s->buf[0], (const float*)s->buf[1], total, d_err);
      else
        hipLaunchKernelGGL(absdiff_max_kernel<double>, dim3(grid), dim3(256), 0, s->stream, (const double*)s->buf[0], (const double*)s->buf[1], total, d_err);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_err, d_err, 8, hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) { glx_set_error("glx_affine_iterate: %s", hipGetErrorString(e)); rc = GLX_EHIP; break; }
    err = __builtin_bit_cast(double, *h_err);
    ++it;
  }
  if (!rc) rc = glx_sweep_fetch(s, u_out);
  if (iters_out) *iters_out = it;
  if (err_out) *err_out = err;
  hipFree(d_err);
  if (h_err) hipHostFree(h_err);
  glx_sweep_destroy(s);
  return rc;
}

extern "C" int glx_poisson_sweep(glx_graph* P, const void* Db, const double* w0, const double* deg, const double* vinf,
                                 int C, int min_iter, int max_iter, void* u_out, int* T_out) {
  GLX_CHECK(P && u_out, GLX_EINVAL, "glx_poisson_sweep: null argument");
  if (max_iter == 0) {   // zero sweeps: u = 0
    memset(u_out, 0, (size_t)P->n_rows * C * (P->dtype == GLX_F32 ? 4 : 8));
    if (T_out) *T_out = 0;
    return GLX_OK;
  }
  glx_sweep* s = nullptr;
  int rc = glx_sweep_create(P, C, min_iter, max_iter, 0, &s);
  if (rc) return rc;
  rc = glx_sweep_set_problem(s, Db, w0, deg, vinf);
  if (!rc) rc = glx_sweep_run(s, T_out, nullptr);
  if (!rc) rc = glx_sweep_fetch(s, u_out);
  glx_sweep_destroy(s);
  return rc;
}

// ---- device-pointer entry points (rank-local sweeps of the vertex-partitioned solver) --------
// The caller (graphlearning_amd/dist.py) owns the buffers -- torch tensors in the record layout
// of glx_record_layout -- and the stream; nothing here synchronises.

extern "C" int glx_record_layout(int C, int dtype, int has_w, int32_t out[6]) {
  GLX_CHECK(out, GLX_EINVAL, "glx_record_layout: null output");
  RecLayout L;
  int rc = glx_make_layout(C, dtype, has_w != 0, &L);
  if (rc) return rc;
  out[0] = L.ld;
  out[1] = L.woff;
  out[2] = L.ld * L.esize;
  out[3] = L.G;
  out[4] = L.nvec;
  out[5] = L.esize;
  return GLX_OK;
}

static int require_caller_order(glx_graph* P, const char* who) {
  int rc = glx_graph_ensure_order(P);
  if (rc) return rc;
  GLX_CHECK(P->h_perm.empty(), GLX_EINVAL, "%s: the operator was renumbered internally; create it with glx_graph_set_order(g, NULL) "
            "to use caller-ordered device records", who);
  return GLX_OK;
}

extern "C" int glx_graph_slots(glx_graph* P, int C, int has_w, int64_t* nslots) {
  GLX_CHECK(P && nslots, GLX_EINVAL, "glx_graph_slots: null argument");
  RecLayout L;
  int rc = glx_make_layout(C, P->dtype, has_w != 0, &L);
  if (rc) return rc;
  SellPlan* plan = nullptr;
  rc = glx_graph_plan(P, L.G, &plan);
  if (rc) return rc;
  *nslots = plan->nslices * plan->R;
  return GLX_OK;
}

extern "C" int glx_bias_flags_dev(glx_graph* P, int C, int has_w, const void* bias_rec, uint8_t* flags, void* stream) {
  GLX_CHECK(P && bias_rec && flags, GLX_EINVAL, "glx_bias_flags_dev: null argument");
  RecLayout L;
  int rc = glx_make_layout(C, P->dtype, has_w != 0, &L);
  if (rc) return rc;
  SellPlan* plan = nullptr;
  rc = glx_graph_plan(P, L.G, &plan);
  if (rc) return rc;
  return glx_bias_flags_async(plan, bias_rec, L.ld * L.esize, flags, (hipStream_t)stream);
}

extern "C" int glx_sweep_step_dev(glx_graph* P, int C, int has_w, const void* xin, void* xout, const void* bias_rec,
                                  const uint8_t* slot_flags, const double* deg, const double* vinf, void* err_next,
                                  void* stream) {
  GLX_CHECK(P && xin && xout, GLX_EINVAL, "glx_sweep_step_dev: null argument");
  SweepArgs a;
  memset(&a, 0, sizeof(a));
  int rc = require_caller_order(P, "glx_sweep_step_dev");
  if (rc) return rc;
  rc = glx_make_layout(C, P->dtype, has_w != 0, &a.L);
  if (rc) return rc;
  SellPlan* plan = nullptr;
  rc = glx_graph_plan(P, a.L.G, &plan);
  if (rc) return rc;
  a.plan = plan;
  a.dtype = P->dtype;
  a.xin = xin;
  a.xout = xout;
  a.bias = bias_rec;
  a.slot_has_bias = bias_rec ? slot_flags : nullptr;
  a.has_w = has_w != 0;
  a.n_rows = P->n_rows;
  a.deg = deg;
  a.vinf = vinf;
  a.err_next = (unsigned long long*)err_next;   // 64 fp64-bit-pattern maxima, caller zeroes them
  GLX_CHECK(!err_next || (has_w && deg && vinf), GLX_EINVAL, "glx_sweep_step_dev: the stop test needs the stop column, deg and vinf");
  return glx_launch_spmm(a, (hipStream_t)stream);
}

extern "C" int glx_pack_records_dev(const void* dense, void* rec, int64_t n, int C, int dtype, int has_w, const double* w,
                                    void* stream) {
  GLX_CHECK(rec, GLX_EINVAL, "glx_pack_records_dev: null output");
  RecLayout L;
  int rc = glx_make_layout(C, dtype, has_w != 0, &L);
  if (rc) return rc;
  return glx_pack_records(dense, rec, n, L, dtype, w, (hipStream_t)stream);
}

extern "C" int glx_unpack_records_dev(const void* rec, void* dense, int64_t n, int C, int dtype, int has_w, void* stream) {
  GLX_CHECK(rec && dense, GLX_EINVAL, "glx_unpack_records_dev: null argument");
  RecLayout L;
  int rc = glx_make_layout(C, dtype, has_w != 0, &L);
  if (rc) return rc;
  return glx_unpack_records(rec, dense, n, L, dtype, (hipStream_t)stream);
}
