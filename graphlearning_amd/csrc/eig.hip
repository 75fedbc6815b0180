// Thick-restart Lanczos with full reorthogonalisation on B = A A, the device half: graph.eigen_decomp and ssl.poisson(solver=
// 'spectral') reach it through _hip.Eig and the driver of graphlearning_amd/_eig.py.  The contract -- the order of every sum, every
// operation rounded on its own -- is written down in eig_plan.h, fixed_sum.h and DESIGN.md 4.12 and walked on the host by EigHost;
// this file is those operations on the device, bit for bit.  The host owns every decision (the projected matrix, the stop, the
// restart, the probe); the device owns the basis, which never leaves it before the end.
//
// The basis is column-major, so projection and update stream (j + 1) n doubles with consecutive lanes on consecutive rows.  A
// wavefront owns the 64 rows of one partial: the halving tree of fs_tree64 runs across its lanes (fs_wave_tree64 of
// fixed_sum_device.h); a workgroup holds EIG_WG_PARTIALS wavefronts -- one, which spreads the 1 094 partials of 70 000 rows most
// evenly over the SIMDs (EXPERIMENTS.md "Eigensolver").  The partials of a column are finished by one workgroup per 16 columns in the
// order of fs_finish (fs_finish_cols): no floating-point atomic anywhere, nothing depends on which workgroup ends first.  The SpMV is
// a CSR row pass, one thread per row.  One step is eleven launches with ordinary kernel boundaries between them; all steps of a run
// are enqueued without a host wait and alpha, beta come back once per run.  The rotation of a restart reads EIG_ROT_ROWS rows of the
// basis into LDS and writes them back in place, each element summed in ascending column order -- which is why it is no MFMA product.
#include "glx_internal.h"
#include "eig_plan.h"
#include "fixed_sum_device.h"
#include <mutex>
#include <vector>

#define EIG_WG (FS_ROWS * EIG_WG_PARTIALS)

struct glx_eig {
  int64_t n = 0, nnz = 0, P = 0;
  int m = 0, device = 0;
  int64_t* d_ptr = nullptr;
  int32_t* d_col = nullptr;
  double *d_val = nullptr, *d_V = nullptr, *d_w = nullptr, *d_t = nullptr, *d_part = nullptr, *d_h = nullptr, *d_ab = nullptr, *d_Y = nullptr;
  std::mutex mu;          // one call at a time per object (ctypes releases the GIL)
};

__global__ __launch_bounds__(256) void eig_spmv_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                        const double* __restrict__ val, const double* __restrict__ x,
                                                        double* __restrict__ y, int64_t n) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  const int64_t e1 = row_ptr[i + 1];
  for (int64_t e = row_ptr[i]; e < e1; ++e) {
    const double pr = val[e] * x[col[e]];
    s = s + pr;
  }
  y[i] = s;
}

// part[p][c] = the tree over the rows of partial p of v_c[i] * w[i], c < count.  Four columns at a time (fs_wave_tree64 of four): their
// trees are independent, and with one wavefront per SIMD at 70 000 rows it is the latency of the six dependent cross-lane steps that
// has to be hidden.
__global__ __launch_bounds__(EIG_WG) void eig_dots_kernel(const double* __restrict__ V, int count, const double* __restrict__ w,
                                                           double* __restrict__ part, int64_t n, int64_t P) {
#pragma clang fp contract(off)
  const int64_t p = (int64_t)blockIdx.x * ((int)blockDim.x / FS_ROWS) + (int)threadIdx.x / FS_ROWS;
  if (p >= P) return;                                   // (the same for every lane of the wavefront)
  const int r = (int)threadIdx.x % FS_ROWS;
  const int64_t i = p * FS_ROWS + r;
  const bool live = i < n;
  const double wi = live ? w[i] : 0.0;
  const double* v = V + (live ? i : 0);
  int c = 0;
  for (; c + 4 <= count; c += 4) {
    double a[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double pr = v[(int64_t)(c + u) * n] * wi;
      a[u] = live ? pr : 0.0;
    }
    fs_wave_tree64(a);
    if (r == 0) {
#pragma unroll
      for (int u = 0; u < 4; ++u) part[p * count + c + u] = a[u];
    }
  }
  for (; c < count; ++c) {
    const double pr = v[(int64_t)c * n] * wi;
    const double s = fs_wave_tree64(live ? pr : 0.0);
    if (r == 0) part[p * count + c] = s;
  }
}

// w_i <- w_i - h[c] * v_c[i], c ascending; part_ww (or null): part_ww[p] = the tree of the new w_i * w_i
__global__ __launch_bounds__(EIG_WG) void eig_update_kernel(const double* __restrict__ V, int count, const double* __restrict__ h,
                                                             double* __restrict__ w, double* __restrict__ part_ww, int64_t n, int64_t P) {
#pragma clang fp contract(off)
  const int64_t p = (int64_t)blockIdx.x * ((int)blockDim.x / FS_ROWS) + (int)threadIdx.x / FS_ROWS;
  if (p >= P) return;
  const int r = (int)threadIdx.x % FS_ROWS;
  const int64_t i = p * FS_ROWS + r;
  const bool live = i < n;
  double wi = live ? w[i] : 0.0;
  const double* v = V + (live ? i : 0);
#pragma unroll 4
  for (int c = 0; c < count; ++c) {
    const double pr = h[c] * v[(int64_t)c * n];
    wi = wi - pr;
  }
  if (live) w[i] = wi;
  if (part_ww) {
    const double sq = wi * wi;
    const double s = fs_wave_tree64(live ? sq : 0.0);
    if (r == 0) part_ww[p] = s;
  }
}

// fs_finish on the device: workgroup b owns the columns [16 b, 16 b + 16) of part (P, nq) and leaves out[j] = the sum of column j;
// no workgroup depends on another.  mode 1: also *slot = prev[nq - 1] + out[nq - 1] (alpha); mode 2 (nq = 1): out[0] = *slot =
// sqrt(sum) (beta)
__global__ __launch_bounds__(FS_FIN_THREADS) void eig_finish_kernel(const double* __restrict__ part, int64_t P, int nq, double* __restrict__ out,
                                                                      int mode, const double* __restrict__ prev, double* __restrict__ slot) {
#pragma clang fp contract(off)
  __shared__ double s_a[FS_FIN_THREADS];
  const int j = (int)blockIdx.x * FS_FIN_COLS + (int)threadIdx.x;          // (of the threads of chain 0)
  const double s = fs_finish_cols(part, P, nq, (int)blockIdx.x * FS_FIN_COLS, s_a);
  if ((int)threadIdx.x < FS_FIN_COLS && j < nq) {
    if (mode == 2) {
      const double b = sqrt(s);
      out[j] = b;
      *slot = b;
    } else {
      out[j] = s;
      if (mode == 1 && j == nq - 1) *slot = prev[j] + s;
    }
  }
}

__global__ __launch_bounds__(256) void eig_scale_kernel(const double* __restrict__ w, const double* __restrict__ beta, double* __restrict__ out,
                                                         int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = w[i] / beta[0];
}

__global__ __launch_bounds__(256) void eig_copy_kernel(const double* __restrict__ src, double* __restrict__ dst, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

// V[i, q] <- sum over c < rows, ascending from +0.0, of V[i, c] * Y[c, q] for q < keep, in place: a workgroup first holds its
// EIG_ROT_ROWS rows in LDS.  Thread t works on row t % 8 and the columns t / 8, t / 8 + 32, ..: a wavefront writes 64 contiguous bytes
// of eight columns and reads eight consecutive doubles of a row of Y.
__global__ __launch_bounds__(256) void eig_rotate_kernel(double* __restrict__ V, int64_t n, const double* __restrict__ Y, int rows, int keep) {
#pragma clang fp contract(off)
  __shared__ double s_v[EIG_ROT_ROWS * EIG_MAX_M];
  const int64_t i0 = (int64_t)blockIdx.x * EIG_ROT_ROWS;
  for (int idx = threadIdx.x; idx < rows * EIG_ROT_ROWS; idx += 256) {
    const int c = idx / EIG_ROT_ROWS, r = idx % EIG_ROT_ROWS;
    const int64_t i = i0 + r;
    s_v[r * EIG_MAX_M + c] = i < n ? V[(int64_t)c * n + i] : 0.0;
  }
  __syncthreads();
  const int r = (int)threadIdx.x % EIG_ROT_ROWS;
  const int64_t i = i0 + r;
  if (i >= n) return;
  const double* row = s_v + r * EIG_MAX_M;
  for (int q = (int)threadIdx.x / EIG_ROT_ROWS; q < keep; q += 256 / EIG_ROT_ROWS) {
    double s = 0.0;
    for (int c = 0; c < rows; ++c) {
      const double pr = row[c] * Y[(int64_t)c * keep + q];
      s = s + pr;
    }
    V[(int64_t)q * n + i] = s;
  }
}

static void eig_free(glx_eig* e) {
  glx_pool_free(e->d_ptr);
  glx_pool_free(e->d_col);
  glx_pool_free(e->d_val);
  glx_pool_free(e->d_V);
  glx_pool_free(e->d_w);
  glx_pool_free(e->d_t);
  glx_pool_free(e->d_part);
  glx_pool_free(e->d_h);
  glx_pool_free(e->d_ab);
  glx_pool_free(e->d_Y);
  delete e;
}

static unsigned eig_blocks(int64_t count, int per) { return (unsigned)((count + per - 1) / per); }

// items 2 - 4 on d_w against the columns [0, count); the new column goes to column dst; alpha_slot (or null) and beta_slot: where the
// two scalars are left on the device
static int eig_orthogonalise(glx_eig* e, int count, int dst, double* alpha_slot, double* beta_slot, hipStream_t st) {
  const unsigned gw = eig_blocks(e->P, EIG_WG_PARTIALS), wg = EIG_WG;
  double* h = e->d_h;
  double* g = e->d_h + (e->m + 1);
  for (int pass = 0; pass < 2; ++pass) {
    double* out = pass ? g : h;
    if (count > 0) {
      hipLaunchKernelGGL(eig_dots_kernel, dim3(gw), dim3(wg), 0, st, (const double*)e->d_V, count, (const double*)e->d_w, e->d_part, e->n, e->P);
      GLX_HIP(hipGetLastError());
      hipLaunchKernelGGL(eig_finish_kernel, dim3(eig_blocks(count, FS_FIN_COLS)), dim3(FS_FIN_THREADS), 0, st, (const double*)e->d_part, e->P, count, out,
                         pass && alpha_slot ? 1 : 0, (const double*)h, alpha_slot);
      GLX_HIP(hipGetLastError());
    }
    if (count > 0 || pass) {
      hipLaunchKernelGGL(eig_update_kernel, dim3(gw), dim3(wg), 0, st, (const double*)e->d_V, count, (const double*)out, e->d_w,
                         pass ? e->d_part : (double*)nullptr, e->n, e->P);
      GLX_HIP(hipGetLastError());
    }
  }
  hipLaunchKernelGGL(eig_finish_kernel, dim3(1), dim3(FS_FIN_THREADS), 0, st, (const double*)e->d_part, e->P, 1, h, 2, (const double*)nullptr, beta_slot);
  GLX_HIP(hipGetLastError());
  hipLaunchKernelGGL(eig_scale_kernel, dim3(eig_blocks(e->n, 256)), dim3(256), 0, st, (const double*)e->d_w, (const double*)beta_slot,
                     e->d_V + (int64_t)dst * e->n, e->n);
  GLX_HIP(hipGetLastError());
  return GLX_OK;
}

template <class T> static int eig_block(T** out, size_t count) {
  void* p = nullptr;
  GLX_UP(glx_pool_alloc(&p, count * sizeof(T) > 8 ? (count * sizeof(T) + 7) & ~(size_t)7 : 8));
  *out = (T*)p;
  return GLX_OK;
}

extern "C" int glx_eig_create(int64_t n, const int64_t* row_ptr, const int32_t* col, const double* val, int m, int device, glx_eig** out) {
  GLX_CHECK(row_ptr && out && n >= 1 && (row_ptr[n] <= 0 || (col && val)), GLX_EINVAL, "glx_eig_create: null argument or n < 1");
  {
    char msg[256];
    const int bad = eig_validate(n, row_ptr, col, val, m, msg, sizeof msg);
    GLX_CHECK(!bad, GLX_EINVAL, "glx_eig_create: %s", msg);
  }
  const int64_t nnz = row_ptr[n];
  GlxCall call;
  GLX_UP(call.begin(device));
  size_t mem_free = 0, mem_total = 0;
  GLX_HIP(hipMemGetInfo(&mem_free, &mem_total));
  const int64_t need = eig_device_bytes(n, nnz, m);
  GLX_CHECK((uint64_t)need <= (uint64_t)mem_total, GLX_ENOMEM, "glx_eig_create: %lld bytes for a basis of %d + 1 columns of %lld rows, the device has %llu",
            (long long)need, m, (long long)n, (unsigned long long)mem_total);
  glx_eig* e = new glx_eig;
  e->n = n;
  e->nnz = nnz;
  e->m = m;
  e->device = device;
  e->P = fs_partials(n);
  hipStream_t st = call.stream();
  int rc = GLX_OK;
  do {
    if ((rc = eig_block(&e->d_ptr, (size_t)n + 1))) break;
    if ((rc = eig_block(&e->d_col, (size_t)nnz))) break;
    if ((rc = eig_block(&e->d_val, (size_t)nnz))) break;
    if ((rc = eig_block(&e->d_V, (size_t)(m + 1) * n))) break;
    if ((rc = eig_block(&e->d_w, (size_t)n))) break;
    if ((rc = eig_block(&e->d_t, (size_t)n))) break;
    if ((rc = eig_block(&e->d_part, (size_t)e->P * (m + 1)))) break;
    if ((rc = eig_block(&e->d_h, (size_t)2 * (m + 1)))) break;
    if ((rc = eig_block(&e->d_ab, (size_t)2 * (m + 1)))) break;
    if ((rc = eig_block(&e->d_Y, (size_t)EIG_MAX_M * EIG_MAX_M))) break;
    if ((rc = glx_upload(e->d_ptr, row_ptr, (size_t)(n + 1) * 8, st, __func__))) break;
    if (nnz > 0) {
      if ((rc = glx_upload(e->d_col, col, (size_t)nnz * 4, st, __func__))) break;
      if ((rc = glx_upload(e->d_val, val, (size_t)nnz * 8, st, __func__))) break;
    }
    if (hipStreamSynchronize(st) != hipSuccess) {
      glx_set_error("glx_eig_create: the uploads did not complete");
      rc = GLX_EHIP;
    }
  } while (0);
  if (rc) {
    (void)hipStreamSynchronize(st);
    eig_free(e);
    return rc;
  }
  *out = e;
  return GLX_OK;
}

extern "C" int glx_eig_destroy(glx_eig* e) {
  if (!e) return GLX_OK;
  eig_free(e);
  return GLX_OK;
}

extern "C" int glx_eig_set_column(glx_eig* e, int j, const double* host_vector) {
  GLX_CHECK(e && host_vector, GLX_EINVAL, "glx_eig_set_column: null argument");
  GLX_CHECK(j >= 0 && j <= e->m, GLX_EINVAL, "glx_eig_set_column: column %d outside [0, %d]", j, e->m);
  std::lock_guard<std::mutex> lock(e->mu);
  GlxCall call;
  GLX_UP(call.begin(e->device));
  GLX_UP(glx_upload(e->d_V + (int64_t)j * e->n, host_vector, (size_t)e->n * 8, call.stream(), __func__));
  GLX_HIP(hipStreamSynchronize(call.stream()));
  return GLX_OK;
}

extern "C" int glx_eig_orthonormalize(glx_eig* e, int j, double* norm_out) {
  GLX_CHECK(e && norm_out, GLX_EINVAL, "glx_eig_orthonormalize: null argument");
  GLX_CHECK(j >= 0 && j <= e->m, GLX_EINVAL, "glx_eig_orthonormalize: column %d outside [0, %d]", j, e->m);
  std::lock_guard<std::mutex> lock(e->mu);
  GlxCall call;
  GLX_UP(call.begin(e->device));
  hipStream_t st = call.stream();
  double* stage = nullptr;
  GLX_UP(call.stage(&stage, 1));
  hipLaunchKernelGGL(eig_copy_kernel, dim3(eig_blocks(e->n, 256)), dim3(256), 0, st, (const double*)(e->d_V + (int64_t)j * e->n), e->d_w, e->n);
  GLX_HIP(hipGetLastError());
  GLX_UP(eig_orthogonalise(e, j, j, nullptr, e->d_ab, st));
  GLX_HIP(hipMemcpyAsync(stage, e->d_ab, 8, hipMemcpyDeviceToHost, st));
  GLX_HIP(hipStreamSynchronize(st));
  *norm_out = stage[0];
  return GLX_OK;
}

extern "C" int glx_eig_run(glx_eig* e, int j0, int j1, double* alpha_out, double* beta_out) {
  GLX_CHECK(e && alpha_out && beta_out, GLX_EINVAL, "glx_eig_run: null argument");
  GLX_CHECK(j0 >= 0 && j0 < j1 && j1 <= e->m, GLX_EINVAL, "glx_eig_run: steps [%d, %d) outside [0, %d]", j0, j1, e->m);
  std::lock_guard<std::mutex> lock(e->mu);
  GlxCall call;
  GLX_UP(call.begin(e->device));
  hipStream_t st = call.stream();
  const int len = j1 - j0;
  double* stage = nullptr;
  GLX_UP(call.stage(&stage, (size_t)2 * len));
  double* alpha = e->d_ab;
  double* beta = e->d_ab + (e->m + 1);
  const unsigned gn = eig_blocks(e->n, 256);
  for (int j = j0; j < j1; ++j) {
    hipLaunchKernelGGL(eig_spmv_kernel, dim3(gn), dim3(256), 0, st, (const int64_t*)e->d_ptr, (const int32_t*)e->d_col, (const double*)e->d_val,
                       (const double*)(e->d_V + (int64_t)j * e->n), e->d_t, e->n);
    GLX_HIP(hipGetLastError());
    hipLaunchKernelGGL(eig_spmv_kernel, dim3(gn), dim3(256), 0, st, (const int64_t*)e->d_ptr, (const int32_t*)e->d_col, (const double*)e->d_val,
                       (const double*)e->d_t, e->d_w, e->n);
    GLX_HIP(hipGetLastError());
    GLX_UP(eig_orthogonalise(e, j + 1, j + 1, alpha + j, beta + j, st));
  }
  GLX_HIP(hipMemcpyAsync(stage, alpha + j0, (size_t)len * 8, hipMemcpyDeviceToHost, st));
  GLX_HIP(hipMemcpyAsync(stage + len, beta + j0, (size_t)len * 8, hipMemcpyDeviceToHost, st));
  GLX_HIP(hipStreamSynchronize(st));
  for (int q = 0; q < len; ++q) {
    alpha_out[q] = stage[q];
    beta_out[q] = stage[len + q];
  }
  return GLX_OK;
}

extern "C" int glx_eig_rotate(glx_eig* e, const double* Y, int rows, int keep) {
  GLX_CHECK(e && Y, GLX_EINVAL, "glx_eig_rotate: null argument");
  GLX_CHECK(rows >= 1 && rows <= e->m && keep >= 1 && keep <= rows, GLX_EINVAL, "glx_eig_rotate: rows=%d keep=%d outside 1 <= keep <= rows <= %d",
            rows, keep, e->m);
  std::lock_guard<std::mutex> lock(e->mu);
  GlxCall call;
  GLX_UP(call.begin(e->device));
  hipStream_t st = call.stream();
  GLX_UP(glx_upload(e->d_Y, Y, (size_t)rows * keep * 8, st, __func__));
  hipLaunchKernelGGL(eig_rotate_kernel, dim3(eig_blocks(e->n, EIG_ROT_ROWS)), dim3(256), 0, st, e->d_V, e->n, (const double*)e->d_Y, rows, keep);
  GLX_HIP(hipGetLastError());
  if (keep != rows) {
    hipLaunchKernelGGL(eig_copy_kernel, dim3(eig_blocks(e->n, 256)), dim3(256), 0, st, (const double*)(e->d_V + (int64_t)rows * e->n),
                       e->d_V + (int64_t)keep * e->n, e->n);
    GLX_HIP(hipGetLastError());
  }
  GLX_HIP(hipStreamSynchronize(st));
  return GLX_OK;
}

extern "C" int glx_eig_get_columns(glx_eig* e, int j0, int j1, double* out) {
  GLX_CHECK(e && out, GLX_EINVAL, "glx_eig_get_columns: null argument");
  GLX_CHECK(j0 >= 0 && j0 < j1 && j1 <= e->m + 1, GLX_EINVAL, "glx_eig_get_columns: columns [%d, %d) outside [0, %d]", j0, j1, e->m + 1);
  GLX_CHECK(j1 - j0 <= EIG_MAX_K, GLX_EUNSUPPORTED, "glx_eig_get_columns: %d columns (at most %d eigenpairs are handed out)", j1 - j0, EIG_MAX_K);
  std::lock_guard<std::mutex> lock(e->mu);
  GlxCall call;
  GLX_UP(call.begin(e->device));
  GLX_UP(glx_download(out, e->d_V + (int64_t)j0 * e->n, (size_t)(j1 - j0) * e->n * 8, call.stream(), __func__));
  GLX_HIP(hipStreamSynchronize(call.stream()));
  return GLX_OK;
}
