// Sparse label propagation on the device, bit for bit: the primal-dual total-variation sweeps of the reference's
// ssl.sparse_label_propagation (ssl.py:1429-1508), reached through ssl.sparse_label_propagation / _hip.slp_iterate.  The contract --
// every operation rounded on its own, the row sums in ascending column order from +0.0 -- is written down in DESIGN.md 4.9 and walked
// on the host by slp_host_reference (slp_plan.h); this file is that loop on the device.
//
// Two kernels per iteration with an ordinary kernel boundary between them: the edge phase reads ut[j] of OTHER rows, so every ut must be
// written before any Y moves, and the next vertex phase reads Y[rev[e]] of other rows.  A dependent boundary costs 1.5-1.9 us; a
// cooperative grid-wide wait costs 26 us or more at 256 workgroups, so there is none.  Full chunks of SLP_CHUNK iterations are replayed from
// a captured launch sequence (no memset node in it: the state is cleared by a kernel before the first chunk); the rest is enqueued eagerly.
//
// State: Y (M, cpad) on the entries, u and ut (n, cpad) on the vertices, class columns contiguous (slp_plan.h: one line per gathered
// record).  One thread per (row, column) in both kernels, columns fastest: a thread walks its row's entries alone and in order -- the
// sequential chain the contract demands, whatever the row's length --, the lanes of a row read consecutive doubles of each record, and
// the edge kernel loads ut[i] once per row.  u is updated in place (only its own thread reads u[i]); ut is a second array because the
// edge phase reads it across rows.
#include "glx_internal.h"
#include "slp_plan.h"
#include <algorithm>
#include <vector>

// vertex phase of iteration (base[0] + r): u, ut of the tile's columns; hist (or null): the iterates (T, n, C) of ALL columns
__global__ __launch_bounds__(SLP_BLOCK) void slp_vertex_kernel(const int64_t* __restrict__ row_ptr, const double* __restrict__ W,
                                                               const int32_t* __restrict__ rev, const double* __restrict__ gamma,
                                                               const int32_t* __restrict__ lab, const double* __restrict__ val,
                                                               const double* __restrict__ Y, double* __restrict__ u, double* __restrict__ ut,
                                                               int64_t n, int C, int c0, int cols, int cpad, double* hist,
                                                               const int64_t* __restrict__ base, int r) {
#pragma clang fp contract(off)
  const int64_t t = (int64_t)blockIdx.x * SLP_BLOCK + threadIdx.x;
  if (t >= n * cols) return;
  const int64_t i = t / cols;
  const int c = (int)(t - i * cols);
  double s = 0.0;
  const int64_t e1 = row_ptr[i + 1];
  for (int64_t e = row_ptr[i]; e < e1; ++e) {
    const int32_t re = rev[e];
    const double y = Y[e * cpad + c];
    const double back = re >= 0 ? Y[(int64_t)re * cpad + c] : 0.0;
    const double d = y - back;
    const double p = d * W[e];
    s = s + p;
  }
  const double h = s / 2.0;
  const double div = 2.0 * h;
  const double g = gamma[i] * div;
  const double z = 0.0 + g;                    // scipy's matvec accumulator: it decides the sign of a zero
  const int64_t at = i * cpad + c;
  const double uo = u[at];
  double un = uo - z;
  const int32_t q = lab[i];
  if (q >= 0) un = val[(int64_t)q * C + c0 + c];
  const double tw = 2.0 * un;
  ut[at] = tw - uo;
  u[at] = un;
  if (hist) hist[((base[0] + r) * n + i) * C + c0 + c] = un;
}

// edge phase: Y of the tile's columns, by row
__global__ __launch_bounds__(SLP_BLOCK) void slp_edge_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                             const double* __restrict__ W, const double* __restrict__ lam,
                                                             const double* __restrict__ ut, double* __restrict__ Y, int64_t n, int cols,
                                                             int cpad) {
#pragma clang fp contract(off)
  const int64_t t = (int64_t)blockIdx.x * SLP_BLOCK + threadIdx.x;
  if (t >= n * cols) return;
  const int64_t i = t / cols;
  const int c = (int)(t - i * cols);
  const double ui = ut[i * cpad + c];
  const int64_t e1 = row_ptr[i + 1];
  for (int64_t e = row_ptr[i]; e < e1; ++e) {
    const double d = ut[(int64_t)col[e] * cpad + c] - ui;
    const double p = W[e] * d;
    const double q = -p;
    const double m = q * lam[e];
    const double y = Y[e * cpad + c] + m;
    Y[e * cpad + c] = y > 1.0 ? 1.0 : (y < -1.0 ? -1.0 : y);      // sign(y) where |y| > 1; a NaN stays
  }
}

// the tile's columns of the state u into the result (n, C)
__global__ __launch_bounds__(SLP_BLOCK) void slp_export_kernel(const double* __restrict__ u, double* __restrict__ out, int64_t n, int C, int c0,
                                                               int cols, int cpad) {
  const int64_t t = (int64_t)blockIdx.x * SLP_BLOCK + threadIdx.x;
  if (t >= n * cols) return;
  const int64_t i = t / cols;
  const int c = (int)(t - i * cols);
  out[i * C + c0 + c] = u[i * cpad + c];
}

// the iteration a chunk starts at (a replayed launch sequence carries its kernel arguments with it; this one value is what changes)
__global__ void slp_base_kernel(int64_t* base, int64_t it) {
  if (threadIdx.x == 0 && blockIdx.x == 0) base[0] = it;
}

extern "C" int glx_slp_iterate(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* col, const double* W, const double* lam,
                               const double* gamma, int C, int64_t m, const int32_t* ind, const double* val, int64_t T, double* u,
                               double* u_hist, int64_t* plan_out, int device) {
  GLX_CHECK(row_ptr && col && W && lam && gamma && u && (m == 0 || (ind && val)), GLX_EINVAL, "glx_slp_iterate: null argument");
  GLX_CHECK(C >= 1, GLX_EINVAL, "glx_slp_iterate: C=%d columns", C);
  GLX_CHECK(T >= 0 && T <= (1ll << 24), GLX_EINVAL, "glx_slp_iterate: T=%lld outside [0, 2^24]", (long long)T);
  {
    char msg[256];
    const int bad = slp_validate(n, M, row_ptr, col, W, lam, gamma, C, m, ind, msg, sizeof msg);
    GLX_CHECK(!bad, GLX_EINVAL, "glx_slp_iterate: %s", msg);
  }
  GLX_CHECK(n * (int64_t)C <= (1ll << 40) / 8, GLX_EUNSUPPORTED, "glx_slp_iterate: a result of n * C = %lld values", (long long)(n * (int64_t)C));
  std::vector<int32_t> rev((size_t)M);
  slp_reverse_index(n, row_ptr, col, rev.data());
  const std::vector<int32_t> lab = csr_label_rows(n, m, ind);
  const std::vector<SlpTile> tiles = slp_tiles(C);
  const int cpad_max = tiles[0].cpad;               // the first tile is the widest

  GlxCall call;
  GLX_UP(call.begin(device));
  hipStream_t st = call.stream();
  int64_t *d_ptr = nullptr, *d_base = nullptr;
  int32_t *d_col = nullptr, *d_rev = nullptr, *d_lab = nullptr;
  double *d_w = nullptr, *d_lam = nullptr, *d_gamma = nullptr, *d_val = nullptr, *d_Y = nullptr, *d_u = nullptr, *d_ut = nullptr,
         *d_out = nullptr, *d_hist = nullptr;
  const size_t hist_bytes = u_hist ? (size_t)T * n * C * 8 : 0;
  GLX_UP(call.put(&d_ptr, row_ptr, (size_t)(n + 1), __func__));
  GLX_UP(call.put(&d_col, col, (size_t)M, __func__));
  GLX_UP(call.put(&d_rev, (const int32_t*)rev.data(), (size_t)M, __func__));
  GLX_UP(call.put(&d_lab, lab.data(), (size_t)n, __func__));
  GLX_UP(call.put(&d_w, W, (size_t)M, __func__));
  GLX_UP(call.put(&d_lam, lam, (size_t)M, __func__));
  GLX_UP(call.put(&d_gamma, gamma, (size_t)n, __func__));
  GLX_UP(call.alloc(&d_val, (size_t)std::max<int64_t>(m, 1) * C));
  if (m > 0) GLX_UP(glx_upload(d_val, val, (size_t)m * C * 8, st, __func__));
  GLX_UP(call.alloc(&d_Y, (size_t)M * cpad_max));
  GLX_UP(call.alloc(&d_u, (size_t)n * cpad_max));
  GLX_UP(call.alloc(&d_ut, (size_t)n * cpad_max));
  GLX_UP(call.alloc(&d_out, (size_t)n * C));
  GLX_UP(call.alloc(&d_base, 1));
  if (hist_bytes) GLX_UP(call.alloc(&d_hist, hist_bytes / 8));

  int64_t launches = 0;
  for (const SlpTile& tile : tiles) {
    const int cols = tile.cols, cpad = tile.cpad, c0 = tile.c0;
    const dim3 grid((unsigned)((n * cols + SLP_BLOCK - 1) / SLP_BLOCK)), blk(SLP_BLOCK);
    GLX_CHECK(n * (int64_t)cols + SLP_BLOCK - 1 < (int64_t)SLP_BLOCK * 0x7fffffffll, GLX_EUNSUPPORTED, "glx_slp_iterate: grid too large");
    GLX_UP(glx_zero_async(d_Y, (size_t)M * cpad * 8, st));
    GLX_UP(glx_zero_async(d_u, (size_t)n * cpad * 8, st));
    auto enqueue = [&](int r) -> int {
      hipLaunchKernelGGL(slp_vertex_kernel, grid, blk, 0, st, (const int64_t*)d_ptr, (const double*)d_w, (const int32_t*)d_rev,
                         (const double*)d_gamma, (const int32_t*)d_lab, (const double*)d_val, (const double*)d_Y, d_u, d_ut, n, C, c0, cols,
                         cpad, d_hist, (const int64_t*)d_base, r);
      GLX_HIP(hipGetLastError());
      hipLaunchKernelGGL(slp_edge_kernel, grid, blk, 0, st, (const int64_t*)d_ptr, (const int32_t*)d_col, (const double*)d_w,
                         (const double*)d_lam, (const double*)d_ut, d_Y, n, cols, cpad);
      GLX_HIP(hipGetLastError());
      launches += 2;
      return GLX_OK;
    };
    // a captured sequence pays for itself from the second replay on
    const bool replay = T >= 2 * (int64_t)SLP_CHUNK;
    call.drop_exec();
    for (int64_t it = 0; it < T;) {
      const int len = (int)std::min<int64_t>(SLP_CHUNK, T - it);
      if (d_hist) {
        hipLaunchKernelGGL(slp_base_kernel, dim3(1), dim3(1), 0, st, d_base, it);
        GLX_HIP(hipGetLastError());
      }
      if (replay && len == SLP_CHUNK) {
        if (!call.exec) {
          hipGraph_t graph = nullptr;
          const int64_t before = launches;
          GLX_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
          int rc2 = GLX_OK;
          for (int r = 0; r < SLP_CHUNK && !rc2; ++r) rc2 = enqueue(r);
          const hipError_t e = hipStreamEndCapture(st, &graph);
          launches = before;
          if (rc2) { if (graph) hipGraphDestroy(graph); return rc2; }
          GLX_HIP(e);
          const hipError_t e2 = hipGraphInstantiate(&call.exec, graph, nullptr, nullptr, 0);
          hipGraphDestroy(graph);
          GLX_HIP(e2);
        }
        GLX_HIP(hipGraphLaunch(call.exec, st));
        launches += 2 * SLP_CHUNK;
      } else {
        for (int r = 0; r < len; ++r) GLX_UP(enqueue(r));
      }
      it += len;
    }
    hipLaunchKernelGGL(slp_export_kernel, grid, blk, 0, st, (const double*)d_u, d_out, n, C, c0, cols, cpad);
    GLX_HIP(hipGetLastError());
    GLX_HIP(hipStreamSynchronize(st));      // this tile's captured sequence is destroyed before the next tile captures its own
  }
  GLX_UP(glx_download(u, d_out, (size_t)n * C * 8, st, __func__));
  if (hist_bytes) GLX_UP(glx_download(u_hist, d_hist, hist_bytes, st, __func__));
  GLX_HIP(hipStreamSynchronize(st));
  if (plan_out) {
    plan_out[0] = 2;
    plan_out[1] = launches;
    plan_out[2] = tiles[0].cols;
  }
  return GLX_OK;
}
