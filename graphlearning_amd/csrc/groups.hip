// Several training sets of ssl.poisson(solver='gradient_descent') as ONE sweep (SURVEY 8 f-1 for the headline kernel; reference
// graphlearning/ssl.py:292-396 runs one `_fit` per training set, each the loop of ssl.py:631-670).  The B trials' label matrices
// are B column groups of the same vertex record -- columns b C .. b C + C - 1 belong to trial b --, each group with its own fp64 stop
// value w_b = D^-1 v_b riding along (its training set decides v_0, ssl.py:639-641) and its own stop test: group b runs sweep t iff
// t < min_iter or max|deg w_b - vinf| > 1/n held after sweep t - 1, exactly the `while` of ssl.py:667.  A group that has stopped
// neither gathers nor changes (its elements are copied forward), so every trial's iterate u_T and its T are those of its own fit,
// bit for bit: the arithmetic of a column never depends on which other columns share its record.
// What is gained: the index / value stream of the operator, the launch and the prologue are paid once per B trials, and a gather
// fetches whole 128-byte lines of useful columns (10 fp64 columns alone fill 80 of 128 bytes).
// The buffers, the uploads and the loop of the stop test are sweep_core.hip's; this file adds the head of a stacked run and its graphs.
#include "glx_internal.h"
#include <algorithm>
#include <map>
#include <vector>

struct glx_sweep_groups : SweepCore {
  std::map<unsigned, hipGraphExec_t> head_exec;   // keyed by the mask of groups in use
  bool vectors_set = false, flags_stale = true;
  std::vector<std::vector<int64_t>> rows;      // per group: the labelled rows of its current training set (cleared by the next one)
  std::vector<double> err0;                    // per group: max|v_0 - vinf| (the test before the first sweep, min_iter = 0)
};

extern "C" int glx_sweep_groups_destroy(glx_sweep_groups* s) {
  if (!s) return GLX_OK;
  hipSetDevice(s->device);
  if (s->stream) hipStreamSynchronize(s->stream);
  for (auto& kv : s->head_exec) hipGraphExecDestroy(kv.second);
  glx_sweep_core_destroy(s);
  delete s;
  return GLX_OK;
}

extern "C" int glx_sweep_groups_create(glx_graph* P, int C, int B, int min_iter, int max_iter, glx_sweep_groups** out) {
  GLX_CHECK(P && out, GLX_EINVAL, "glx_sweep_groups_create: null argument");
  *out = nullptr;
  GLX_CHECK(P->n_rows == P->n_cols, GLX_EINVAL, "glx_sweep_groups_create: operator must be square");
  GLX_CHECK(B >= 2 && B <= SWEEP_MAX_GROUPS, GLX_EINVAL, "glx_sweep_groups_create: %d groups (2 .. 32; one training set is glx_sweep_create)", B);
  GLX_CHECK(min_iter >= 0 && max_iter >= 1, GLX_EINVAL, "glx_sweep_groups_create: bad iteration bounds (%d, %d)", min_iter, max_iter);
  GLX_HIP(hipSetDevice(P->device));
  RecLayout L;
  GLX_UP(glx_make_layout_groups(C, B, P->dtype, &L));
  glx_sweep_groups* s = new glx_sweep_groups();
  const auto rest = [&]() -> int {
    GLX_UP(glx_sweep_core_create(s, P, L, C, B, GLX_GRP_SHARDS, min_iter, max_iter, true));
    s->bias_set = true;      // every launch reads the bias through the flags
    GLX_HIP(hipMemsetAsync(s->slot_has_bias, 0, std::max<size_t>((size_t)s->nslots(), 64), s->stream));
    GLX_HIP(hipMemsetAsync(s->w0, 0, std::max<size_t>((size_t)s->n_rows * 8 * B, 64), s->stream));
    GLX_HIP(hipStreamSynchronize(s->stream));
    return GLX_OK;
  };
  const int rc = rest();
  if (rc) { glx_sweep_groups_destroy(s); return rc; }
  s->rows.resize(B);
  s->err0.assign(B, 0.0);
  *out = s;
  return GLX_OK;
}

extern "C" int glx_sweep_groups_set_vectors(glx_sweep_groups* s, const double* deg, const double* vinf) {
  GLX_CHECK(s && deg && vinf, GLX_EINVAL, "glx_sweep_groups_set_vectors: null argument");
  GLX_HIP(hipSetDevice(s->device));
  GLX_UP(glx_sweep_set_vectors_core(s, deg, vinf));
  s->vectors_set = true;
  return GLX_OK;
}

// Training set of group b: its m labelled rows, their rows of Db = D^-1 b (m x C, state dtype) and of w0 = v_0 / deg, and
// err0 = max|v_0 - vinf| (ssl.py:620-622, 636, 639-641, 667).  m = 0 leaves the group without a problem (u stays 0).
extern "C" int glx_sweep_groups_set_problem_rows(glx_sweep_groups* s, int b, int64_t m, const int64_t* rows, const void* Db_rows,
                                                 const double* w0_rows, double err0) {
  GLX_CHECK(s, GLX_EINVAL, "glx_sweep_groups_set_problem_rows: null sweep");
  GLX_CHECK(b >= 0 && b < s->B, GLX_EINVAL, "glx_sweep_groups_set_problem_rows: group %d of %d", b, s->B);
  GLX_CHECK(s->vectors_set, GLX_EINVAL, "glx_sweep_groups_set_problem_rows: call glx_sweep_groups_set_vectors first");
  GLX_CHECK(m >= 0 && (m == 0 || (rows && Db_rows && w0_rows)), GLX_EINVAL, "glx_sweep_groups_set_problem_rows: null array");
  for (int64_t q = 0; q < m; ++q)
    GLX_CHECK(rows[q] >= 0 && rows[q] < s->n_rows, GLX_EINVAL, "glx_sweep_groups_set_problem_rows: row %lld out of range", (long long)rows[q]);
  GLX_HIP(hipSetDevice(s->device));
  const size_t es = s->L.esize;
  const int64_t mp = (int64_t)s->rows[b].size();
  const size_t b_prev = (size_t)mp * 8, b_rows = (size_t)m * 8, b_db = ((size_t)m * s->C * es + 7) / 8 * 8, b_w = (size_t)m * 8;
  GLX_UP(glx_sweep_reserve(s, &s->stage, &s->stage_cap, b_prev + b_rows + b_db + b_w + 64));
  char* st = (char*)s->stage;
  double* w0_b = s->w0 + (size_t)b * s->n_rows;
  if (mp > 0) {      // the previous training set of this group: its bias rows and start values back to zero
    GLX_UP(glx_upload(st, s->rows[b].data(), b_prev, s->stream, __func__));
    GLX_UP(glx_sweep_scatter_rows(s, (const int64_t*)st, nullptr, nullptr, w0_b, mp, b * s->C));
  }
  if (m > 0) {
    char* q0 = st + b_prev;
    GLX_UP(glx_upload(q0, rows, b_rows, s->stream, __func__));
    GLX_UP(glx_upload(q0 + b_rows, Db_rows, (size_t)m * s->C * es, s->stream, __func__));
    GLX_UP(glx_upload(q0 + b_rows + b_db, w0_rows, b_w, s->stream, __func__));
    GLX_UP(glx_sweep_scatter_rows(s, (const int64_t*)q0, q0 + b_rows, (const double*)(q0 + b_rows + b_db), w0_b, m, b * s->C));
  }
  GLX_HIP(hipStreamSynchronize(s->stream));      // the host arrays may go; the staging is reused by the next call
  s->rows[b].assign(rows, rows + m);
  s->err0[b] = err0;
  s->flags_stale = true;
  return GLX_OK;
}

// the start of every run: u = 0 (ssl.py:645), stop value of group b = w0_b (record order through perm)
__global__ void grp_init_stop_kernel(char* __restrict__ rec, int rec_bytes, int woff, const double* __restrict__ w0, const int32_t* __restrict__ perm,
                                     int64_t n, int B) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * B) return;
  const int64_t row = i / B;
  const int b = (int)(i % B);
  *(double*)(rec + (size_t)row * rec_bytes + woff + 8 * b) = w0[(size_t)b * n + (perm ? perm[row] : row)];
}

// reset + the min_iter unconditional sweeps: identical for every run with the same groups in use -> captured once
static int grp_enqueue_head(glx_sweep_groups* s, unsigned used_mask) {
  GLX_UP(glx_sweep_head_rows(s));
  s->cur = 0;
  // (a kernel, not a memset node: this sequence is captured and replayed -- glx_zero_async, glx_internal.h)
  GLX_UP(glx_zero_async(s->buf[0], (size_t)s->n_rows * s->rec_bytes(), s->stream));
  if (s->n_rows > 0) {
    const int64_t tot = s->n_rows * s->B;
    hipLaunchKernelGGL(grp_init_stop_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s->stream, (char*)s->buf[0], (int)s->rec_bytes(),
                       s->L.woff, (const double*)s->w0, (const int32_t*)s->P->d_perm, s->n_rows, s->B);
    GLX_HIP(hipGetLastError());
  }
  for (int t = 0; t < s->walk.head; ++t) GLX_UP(glx_sweep_launch(s, t, true, used_mask));
  return GLX_OK;
}

// Run the groups 0 .. used - 1 (the others stay idle).  T_out[b] = sweeps of group b, exactly the T of its own fit.
extern "C" int glx_sweep_groups_run(glx_sweep_groups* s, int used, int* T_out, float* device_ms_out) {
  GLX_CHECK(s && T_out, GLX_EINVAL, "glx_sweep_groups_run: null argument");
  GLX_CHECK(used >= 1 && used <= s->B, GLX_EINVAL, "glx_sweep_groups_run: %d of %d groups", used, s->B);
  GLX_HIP(hipSetDevice(s->device));
  const unsigned used_mask = used >= 32 ? 0xffffffffu : ((1u << used) - 1u);
  s->walk.start(s->B, used, s->min_iter, s->max_iter, s->thresh);
  if (s->flags_stale) {
    GLX_UP(glx_bias_flags_async(s->plan, s->bias, (int)s->rec_bytes(), s->slot_has_bias, s->stream));
    s->flags_stale = false;
  }
  GLX_HIP(hipEventRecord(s->ev0, s->stream));
  glx_sweep_put_err0(s, s->err0.data());
  auto it = s->head_exec.find(used_mask);
  if (it == s->head_exec.end()) {
    hipGraphExec_t exec;
    GLX_UP(glx_sweep_capture(s, [&]() { return grp_enqueue_head(s, used_mask); }, &exec));
    it = s->head_exec.emplace(used_mask, exec).first;
  }
  GLX_HIP(hipGraphLaunch(it->second, s->stream));
  s->cur = s->walk.head & 1;
  s->launches += s->walk.head;
  GLX_UP(glx_sweep_tail(s, [&](int t) { return glx_sweep_launch(s, t, true, used_mask); }, device_ms_out));
  for (int b = 0; b < s->B; ++b) T_out[b] = s->walk.T[b];
  return GLX_OK;
}

// The stop values group b's last run compared with 1/n (see glx_sweep_stop_values_core): t = *first .. *first + *count - 1.
extern "C" int glx_sweep_groups_stop_values(const glx_sweep_groups* s, int b, int64_t cap, double* vals, int* first, int* count) {
  GLX_CHECK(s && first && count, GLX_EINVAL, "glx_sweep_groups_stop_values: null argument");
  GLX_CHECK(b >= 0 && b < s->B, GLX_EINVAL, "glx_sweep_groups_stop_values: group %d of %d", b, s->B);
  return glx_sweep_stop_values_core(s, b, cap, vals, first, count);
}

template <typename T>
__global__ void grp_unpack_kernel(const T* __restrict__ rec, T* __restrict__ dense, int64_t n, int C, int ld, int col0,
                                  const int32_t* __restrict__ perm) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * C) return;
  const int64_t row = i / C;
  const int c = (int)(i % C);
  dense[(perm ? (int64_t)perm[row] : row) * C + c] = rec[row * ld + col0 + c];
}

static int grp_unpack(glx_sweep_groups* s, int b, void* dense_dev) {
  const int64_t tot = s->n_rows * s->C;
  if (tot == 0) return GLX_OK;
  const unsigned grid = (unsigned)((tot + 255) / 256);
  if (s->P->dtype == GLX_F32)
    hipLaunchKernelGGL(grp_unpack_kernel<float>, dim3(grid), dim3(256), 0, s->stream, (const float*)s->buf[s->cur], (float*)dense_dev, s->n_rows,
                       s->C, s->L.ld, b * s->C, (const int32_t*)s->P->d_perm);
  else
    hipLaunchKernelGGL(grp_unpack_kernel<double>, dim3(grid), dim3(256), 0, s->stream, (const double*)s->buf[s->cur], (double*)dense_dev, s->n_rows,
                       s->C, s->L.ld, b * s->C, (const int32_t*)s->P->d_perm);
  GLX_HIP(hipGetLastError());
  return GLX_OK;
}

// group b's (n, C) iterate of the last run, caller order, state dtype
extern "C" int glx_sweep_groups_fetch(glx_sweep_groups* s, int b, void* u_out) {
  GLX_CHECK(s && u_out, GLX_EINVAL, "glx_sweep_groups_fetch: null argument");
  GLX_CHECK(b >= 0 && b < s->B, GLX_EINVAL, "glx_sweep_groups_fetch: group %d of %d", b, s->B);
  GLX_HIP(hipSetDevice(s->device));
  GLX_UP(grp_unpack(s, b, s->dense));
  GLX_UP(glx_download(u_out, s->dense, (size_t)s->n_rows * s->C * s->L.esize, s->stream, __func__));
  GLX_HIP(hipStreamSynchronize(s->stream));
  return GLX_OK;
}

// ssl.predict / ssl.volume_label_projection (ssl.py:230-266, 172-209) on group b's iterate without a host round trip
extern "C" int glx_sweep_groups_project(glx_sweep_groups* s, int b, const double* priors, double* weights_inout, int64_t* labels_out,
                                        double* err_out, int* steps_out, int max_steps, int similarity) {
  GLX_CHECK(s && weights_inout, GLX_EINVAL, "glx_sweep_groups_project: null argument");
  GLX_CHECK(b >= 0 && b < s->B, GLX_EINVAL, "glx_sweep_groups_project: group %d of %d", b, s->B);
  GLX_HIP(hipSetDevice(s->device));
  void* prob = nullptr;
  GLX_UP(glx_sweep_project_target(s, &prob));
  GLX_UP(grp_unpack(s, b, prob));
  const long long* d_labels = nullptr;
  const std::function<int(bool)> hook = [&](bool after) -> int {
    if (!after && labels_out) GLX_UP(glx_download(labels_out, d_labels, (size_t)s->n_rows * 8, s->stream, __func__));
    return GLX_OK;
  };
  return glx_project_device(&s->proj, prob, s->P->dtype, s->n_rows, s->C, priors, weights_inout, err_out, steps_out, max_steps, similarity,
                            s->stream, &d_labels, &hook);
}

extern "C" int glx_sweep_groups_launches(const glx_sweep_groups* s, int64_t* n) {
  GLX_CHECK(s && n, GLX_EINVAL, "glx_sweep_groups_launches: null argument");
  *n = s->launches;
  return GLX_OK;
}
