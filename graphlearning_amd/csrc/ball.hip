// Exact radius graphs on the device: weightmatrix.epsilon_ball of the reference (graphlearning/weightmatrix.py:189-294).
//
// The rows of such a graph have no fixed length (0 .. n - 1 entries), so nothing of the kNN list machinery applies; the search is
// count / scan / fill over a grid of cells (ball_plan.h: the plan and the argument why the grid never hides a pair):
//   grid     a cell id per point, a histogram of the cells (integer atomics, one per POINT), its scan, the rows reordered by cell
//            (order inside a cell is arbitrary -- nothing below depends on it);
//   count    one wavefront owns 64 consecutive sorted rows, one per lane.  With the last grid axis running fastest in the cell id,
//            the neighbour cells of the block's cells are 3^(g-1) contiguous ROW ranges (merged where they overlap); the ranges are
//            staged through LDS 64 rows at a time (d <= 3, the query in registers) or read in place (larger d), and every lane
//            tests its query against every candidate with the tree's own expression: sqdist_exact(x, y) <= fl(epsilon * epsilon),
//            fp64, difference form, no pre-filter.  The count goes to the row's ORIGINAL position;
//   scan     n counters -> int64 offsets; the total is checked against int32 and sizes the result exactly;
//   fill     the same traversal writes the original column ids at the row's offset.  A lane owns its row, so it keeps its own
//            cursor: no atomics, no cross-lane compaction;
//   sort     one wavefront per row sorts the columns in LDS (a bitonic network whose merges all run upwards, so a row of any
//            length sorts in place: the missing tail behaves as +infinity and never moves); rows above BALL_SORT_CAP get a
//            workgroup each and sort in place in global memory.
// glx_ball_result_to_csr then walks the finished structure: per entry the distance in numpy's summation order (npsum_exact.h: what
// the reference's weights see -- not the tree's order, the two differ from 8 coordinates on), the feature distance, the kernel,
// operation by operation; entries whose weight is exactly zero are dropped by a second scan and a stable compaction.
// A pair is tested from both sides; the differences negate exactly and the squares agree, so both sides decide and weigh alike
// and the matrix is symmetric bit for bit.
#include "glx_internal.h"
#include "ball_plan.h"
#include "sqdist_tree.h"
#include "npsum_exact.h"
#include "exp_cr.h"
#include <algorithm>
#include <cmath>
#include <vector>
#define GLX_POOL(call) do { int rc_ = (call); if (rc_) return rc_; } while (0)

enum { BK_GIVEN = 0, BK_UNIFORM = 1, BK_GAUSSIAN = 2, BK_DISTANCE = 4, BK_SINGULAR = 5 };   // the ids of the kNN assembly
enum { BS_TESTED = 0, BS_ACCEPTED, BS_CELLS, BS_GRID_MS, BS_COUNT_MS, BS_FILL_MS, BS_SORT_MS, BS_WEIGHTS_MS, BS_COUNT };

static thread_local double g_ball_stats[BS_COUNT];
extern "C" int glx_ball_stats(double stats[8]) {
  GLX_CHECK(stats, GLX_EINVAL, "glx_ball_stats: null output");
  for (int i = 0; i < BS_COUNT; ++i) stats[i] = g_ball_stats[i];
  return GLX_OK;
}

struct glx_ball_result {
  int64_t n = 0, nnz = 0;
  int d = 0, mf = 0, device = 0;
  double epsilon = 0.0;
  double* X = nullptr;          // [n][d] the caller's rows (pooled)
  double* F = nullptr;          // [n][mf] features or null
  long long* off = nullptr;     // [n + 1] row offsets
  int* col = nullptr;           // [nnz] columns, ascending inside a row
};

// the grid as the kernels see it
struct BallGrid {
  int g;
  int axis[3];
  double lo[3], h[3];
  long long nc[3], stride[3];
  long long ncells;
};

__device__ __forceinline__ int ball_cell_of(const BallGrid& G, const double* __restrict__ x) {
  long long id = 0;
  for (int a = 0; a < G.g; ++a) {
    const double t = floor((x[G.axis[a]] - G.lo[a]) / G.h[a]);
    long long c = 0;
    if (t > 0.0) c = t >= (double)(G.nc[a] - 1) ? G.nc[a] - 1 : (long long)t;
    id += c * G.stride[a];
  }
  return (int)id;
}

__global__ void ball_cellid_kernel(const double* __restrict__ X, int64_t n, int d, BallGrid G, int* __restrict__ cid,
                                   int* __restrict__ cell_cnt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int c = ball_cell_of(G, X + i * d);
  cid[i] = c;
  atomicAdd(&cell_cnt[c], 1);
}

// out[i] = cnt[0] + ... + cnt[i-1] for i = 0 .. n (one workgroup of 1024 threads walks the array in pieces of 8192).  At 10^6
// counters a pass takes 0.3 ms and the search makes three (profiles/epsball.txt: the largest single item of its kernel time);
// a version in pieces scanned by many workgroups is the obvious next step.
static const int SCAN_ITEMS = 8;
__global__ __launch_bounds__(1024) void ball_scan_kernel(const int* __restrict__ cnt, int64_t n, long long* __restrict__ out) {
  __shared__ long long s_wave[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long carry = 0;
  for (int64_t base = 0; base < n; base += 1024 * SCAN_ITEMS) {
    const int64_t i0 = base + (int64_t)tid * SCAN_ITEMS;
    int v[SCAN_ITEMS];
    long long mine = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
      v[j] = i0 + j < n ? cnt[i0 + j] : 0;
      mine += v[j];
    }
    long long incl = mine;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const long long up = __shfl_up(incl, s);
      if (lane >= s) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    long long before = 0, total = 0;
    for (int w = 0; w < 16; ++w) {
      if (w < wave) before += s_wave[w];
      total += s_wave[w];
    }
    long long run = carry + before + incl - mine;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
      if (i0 + j < n) out[i0 + j] = run;
      run += v[j];
    }
    carry += total;
    __syncthreads();
  }
  if (tid == 0) out[n] = carry;
}

// rows into cell order: orig[position] = the caller's row.  The histogram doubles as the cursor (counted down to zero).
__global__ void ball_scatter_kernel(const double* __restrict__ X, int64_t n, int d, const int* __restrict__ cid,
                                    const long long* __restrict__ cell_start, int* __restrict__ cell_cnt, int* __restrict__ orig,
                                    int* __restrict__ scell, double* __restrict__ Xs) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int c = cid[i];
  const int64_t pos = cell_start[c] + (atomicSub(&cell_cnt[c], 1) - 1);
  if (pos < 0 || pos >= n) return;   // (cannot happen: the histogram counted this very point)
  orig[pos] = (int)i;
  scell[pos] = c;
  for (int f = 0; f < d; ++f) Xs[pos * d + f] = X[i * d + f];
}

// count (FILL = false) and fill (FILL = true): see the head of the file.  D = 1, 2, 3: d = D, query in registers, candidates
// staged in LDS; D = 0: any d, both rows read in place (the candidate's address is the same in every lane).
template <int D, bool FILL>
__global__ __launch_bounds__(BALL_BQ) void ball_pairs_kernel(const double* __restrict__ Xs, const int* __restrict__ orig,
                                                             const int* __restrict__ scell, const long long* __restrict__ cell_start,
                                                             int64_t n, int d, BallGrid G, double eps2, int* __restrict__ cnt,
                                                             const long long* __restrict__ off, int* __restrict__ col,
                                                             unsigned long long* __restrict__ tested) {
  __shared__ long long s_lo[9], s_hi[9], s_tlo[9], s_thi[9];
  __shared__ int s_nr;
  __shared__ double s_x[BALL_TILE * (D > 0 ? D : 1)];
  __shared__ int s_id[BALL_TILE];
  const int lane = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x * BALL_BQ;
  const int64_t q = q0 + lane;
  const bool valid = q < n;
  if (lane == 0) {
    const long long c_lo = scell[q0], c_hi = scell[q0 + BALL_BQ - 1 < n ? q0 + BALL_BQ - 1 : n - 1];
    const long long sA = G.g == 3 ? G.stride[0] : 0, sB = G.g == 3 ? G.stride[1] : (G.g == 2 ? G.stride[0] : 0);
    const int ra = G.g == 3 ? 1 : 0, rb = G.g >= 2 ? 1 : 0;
    long long* lo = s_tlo;   // (in LDS: nine pairs of registers in every lane for the sake of one would cost a wave of occupancy)
    long long* hi = s_thi;
    int m = 0;
    for (int da = -ra; da <= ra; ++da) {
      for (int db = -rb; db <= rb; ++db) {
        long long a = c_lo + da * sA + db * sB - 1, b = c_hi + da * sA + db * sB + 1;
        if (b < 0 || a > G.ncells - 1) continue;
        if (a < 0) a = 0;
        if (b > G.ncells - 1) b = G.ncells - 1;
        const long long r0 = cell_start[a], r1 = cell_start[b + 1];
        if (r0 >= r1) continue;
        // insertion by first row (the offsets are not monotone when a slow axis has a single cell)
        int p = m++;
        while (p > 0 && lo[p - 1] > r0) {
          lo[p] = lo[p - 1];
          hi[p] = hi[p - 1];
          --p;
        }
        lo[p] = r0;
        hi[p] = r1;
      }
    }
    int nr = 0;
    for (int p = 0; p < m; ++p) {
      if (nr > 0 && lo[p] <= s_hi[nr - 1]) {
        if (hi[p] > s_hi[nr - 1]) s_hi[nr - 1] = hi[p];
      } else {
        s_lo[nr] = lo[p];
        s_hi[nr] = hi[p];
        ++nr;
      }
    }
    s_nr = nr;
  }
  __syncthreads();
  const int nr = s_nr;
  const int64_t qs = valid ? q : 0;        // (a lane without a row computes on row 0 and writes nothing)
  const int me = orig[qs];
  const double* xq = Xs + qs * d;
  double xr[D > 0 ? D : 1];
  if constexpr (D > 0) {
#pragma unroll
    for (int f = 0; f < D; ++f) xr[f] = xq[f];
  }
  int count = 0;
  int room = 0;
  int64_t pos = 0;
  if constexpr (FILL) {
    pos = off[me];
    room = (int)(off[me + 1] - pos);      // what the count pass found: the traversal is the same, this only guards the stores
  }
  unsigned long long cand = 0;
  for (int r = 0; r < nr; ++r) {
    const long long r0 = s_lo[r], r1 = s_hi[r];
    cand += (unsigned long long)(r1 - r0);
    for (long long base = r0; base < r1; base += BALL_TILE) {
      const int m = (int)(r1 - base < BALL_TILE ? r1 - base : BALL_TILE);
      if constexpr (D > 0) {
        __syncthreads();
        if (lane < m) {
#pragma unroll
          for (int f = 0; f < D; ++f) s_x[lane * D + f] = Xs[(base + lane) * D + f];
          if constexpr (FILL) s_id[lane] = orig[base + lane];
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < m; ++j) {
          const double d2 = sqdist_exact(xr, &s_x[j * D], D);
          if (valid && d2 <= eps2 && base + j != q) {
            if constexpr (FILL) {
              if (count < room) col[pos + count] = s_id[j];
            }
            ++count;
          }
        }
      } else {
        for (int j = 0; j < m; ++j) {
          const double d2 = sqdist_exact(xq, Xs + (base + j) * d, d);
          if (valid && d2 <= eps2 && base + j != q) {
            if constexpr (FILL) {
              if (count < room) col[pos + count] = orig[base + j];
            }
            ++count;
          }
        }
      }
    }
  }
  if constexpr (!FILL) {
    if (valid) cnt[me] = count;
    if (lane == 0) {
      const int64_t rows = n - q0 < BALL_BQ ? n - q0 : BALL_BQ;
      atomicAdd(tested, cand * (unsigned long long)rows);
    }
  }
}

__global__ void ball_hubs_kernel(const int* __restrict__ cnt, int64_t n, int* __restrict__ nhub, int* __restrict__ hubs) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (cnt[i] > BALL_SORT_CAP) hubs[atomicAdd(nhub, 1)] = (int)i;
}

// ascending sort of a[0 .. L) by the nt threads of a workgroup (a in LDS or in global memory).  Every merge of the network
// compares upwards (its first step pairs i with the mirror position of its block), so slots at L and beyond act as +infinity
// and are never touched.
__device__ __forceinline__ void ball_sort_inplace(int* a, int L, int tid, int nt) {
  int P = 1;
  while (P < L) P <<= 1;
  const int half = P >> 1;
  for (int k = 2; k <= P; k <<= 1) {
    const int hk = k >> 1;
    for (int t = tid; t < half; t += nt) {
      const int blk = t / hk, o = t % hk;
      const int i = blk * k + o, j = blk * k + k - 1 - o;
      if (j < L) {
        const int x = a[i], y = a[j];
        if (x > y) { a[i] = y; a[j] = x; }
      }
    }
    __syncthreads();
    for (int jj = hk >> 1; jj > 0; jj >>= 1) {
      for (int t = tid; t < half; t += nt) {
        const int i = 2 * jj * (t / jj) + t % jj, j = i + jj;
        if (j < L) {
          const int x = a[i], y = a[j];
          if (x > y) { a[i] = y; a[j] = x; }
        }
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(64) void ball_sort_rows_kernel(const long long* __restrict__ off, int64_t n, int* __restrict__ col) {
  __shared__ int s[BALL_SORT_CAP];
  const int lane = threadIdx.x;
  for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
    const long long b = off[row];
    const int L = (int)(off[row + 1] - b);
    if (L < 2 || L > BALL_SORT_CAP) continue;     // (the same in every lane; hubs: ball_sort_hub_kernel)
    for (int e = lane; e < L; e += 64) s[e] = col[b + e];
    __syncthreads();
    ball_sort_inplace(s, L, lane, 64);
    for (int e = lane; e < L; e += 64) col[b + e] = s[e];
    __syncthreads();
  }
}

__global__ __launch_bounds__(1024) void ball_sort_hub_kernel(const long long* __restrict__ off, const int* __restrict__ hubs,
                                                             int* __restrict__ col) {
  const int row = hubs[blockIdx.x];
  const long long b = off[row];
  ball_sort_inplace(col + b, (int)(off[row + 1] - b), threadIdx.x, 1024);
}

// one kernel of the reference's __weights__ (weightmatrix.py:268-294), operation by operation.  Not inlined, like ball_npsum
// below: the weights kernel calls each twice (points and features), and two inlined copies of the double-double exponential
// and of the summation stack cost it every register and all but one wave per SIMD.
__device__ __noinline__ double ball_weight(int kernel, double dd, double e2) {
#pragma clang fp contract(off)
  if (kernel == BK_GAUSSIAN) {
    const double a = -4.0 * dd;
    return exp_cr(a / e2);
  }
  if (kernel == BK_DISTANCE) return sqrt(dd);
  if (kernel == BK_SINGULAR) {
    double s = sqrt(dd);
    if (dd == 0.0) s = 1.0;
    return 1.0 / s;
  }
  return 1.0;
}

__device__ __noinline__ double ball_npsum(const double* u, const double* v, int d) { return npsum_sqdiff(u, v, d); }

// 16 lanes per row: distances in numpy's order, weights, and the number of entries whose weight is not exactly zero
static const int BALL_ROW_LANES = 16;
__global__ __launch_bounds__(256) void ball_weights_kernel(const double* __restrict__ X, const double* __restrict__ F, int64_t n, int d,
                                                           int mf, const long long* __restrict__ off, const int* __restrict__ col,
                                                           int kernel, double eps2, double epsf2, double* __restrict__ val,
                                                           double* __restrict__ dists, double* __restrict__ fdists,
                                                           int* __restrict__ kept) {
#pragma clang fp contract(off)
  const int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BALL_ROW_LANES;
  const int sub = threadIdx.x % BALL_ROW_LANES;
  int k = 0;
  if (row < n) {
    const long long b = off[row], e1 = off[row + 1];
    for (long long e = b + sub; e < e1; e += BALL_ROW_LANES) {
      const int64_t j = col[e];
      const double dd = ball_npsum(X + row * d, X + j * d, d);
      double w = kernel == BK_GIVEN ? 1.0 : ball_weight(kernel, dd, eps2);
      if (dists) dists[e] = dd;
      if (F) {
        const double fd = ball_npsum(F + row * mf, F + j * mf, mf);
        if (kernel != BK_GIVEN) w = w * ball_weight(kernel, fd, epsf2);
        if (fdists) fdists[e] = fd;
      }
      val[e] = w;
      k += w != 0.0;
    }
  }
  for (int m = BALL_ROW_LANES / 2; m > 0; m >>= 1) k += __shfl_xor(k, m, BALL_ROW_LANES);
  if (row < n && sub == 0) kept[row] = k;
}

// the entries with a weight other than zero, in order, at the offsets of the second scan
__global__ __launch_bounds__(256) void ball_compact_kernel(int64_t n, const long long* __restrict__ off, const int* __restrict__ col,
                                                           const double* __restrict__ val, const long long* __restrict__ off2,
                                                           int* __restrict__ col2, double* __restrict__ val2) {
  const int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BALL_ROW_LANES;
  const int sub = threadIdx.x % BALL_ROW_LANES;
  const int shift = (threadIdx.x & 63) & ~(BALL_ROW_LANES - 1);
  if (row >= n) return;
  const long long b = off[row], L = off[row + 1] - b, b2 = off2[row], room = off2[row + 1] - b2;
  long long done = 0;
  for (long long base = 0; base < L; base += BALL_ROW_LANES) {
    const bool has = base + sub < L;
    const double w = has ? val[b + base + sub] : 0.0;
    const bool keep = has && w != 0.0;
    const unsigned gm = (unsigned)((__ballot(keep) >> shift) & 0xFFFFull);
    const long long p = done + __popc(gm & ((1u << sub) - 1u));
    if (keep && p < room) {
      col2[b2 + p] = col[b + base + sub];
      val2[b2 + p] = w;
    }
    done += __popc(gm);
  }
}

__global__ void ball_rowptr_kernel(const long long* __restrict__ off, int64_t n, int* __restrict__ rowptr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= n) rowptr[i] = (int)off[i];
}

extern "C" int glx_ball_result_destroy(glx_ball_result* res) {
  if (!res) return GLX_OK;
  glx_pool_free(res->X);
  glx_pool_free(res->F);
  glx_pool_free(res->off);
  glx_pool_free(res->col);
  delete res;
  return GLX_OK;
}

extern "C" int glx_ball_result_nnz(const glx_ball_result* res, int64_t* nnz_out) {
  GLX_CHECK(res && nnz_out, GLX_EINVAL, "glx_ball_result_nnz: null argument");
  *nnz_out = res->nnz;
  return GLX_OK;
}

namespace {
template <bool FILL>
int launch_pairs(int d, unsigned grid, hipStream_t st, const double* Xs, const int* orig, const int* scell, const long long* cell_start,
                 int64_t n, const BallGrid& G, double eps2, int* cnt, const long long* off, int* col, unsigned long long* tested) {
  switch (d <= BALL_REG_D ? d : 0) {
    case 1: hipLaunchKernelGGL((ball_pairs_kernel<1, FILL>), dim3(grid), dim3(BALL_BQ), 0, st, Xs, orig, scell, cell_start, n, d, G, eps2, cnt, off, col, tested); break;
    case 2: hipLaunchKernelGGL((ball_pairs_kernel<2, FILL>), dim3(grid), dim3(BALL_BQ), 0, st, Xs, orig, scell, cell_start, n, d, G, eps2, cnt, off, col, tested); break;
    case 3: hipLaunchKernelGGL((ball_pairs_kernel<3, FILL>), dim3(grid), dim3(BALL_BQ), 0, st, Xs, orig, scell, cell_start, n, d, G, eps2, cnt, off, col, tested); break;
    default: hipLaunchKernelGGL((ball_pairs_kernel<0, FILL>), dim3(grid), dim3(BALL_BQ), 0, st, Xs, orig, scell, cell_start, n, d, G, eps2, cnt, off, col, tested); break;
  }
  GLX_HIP(hipGetLastError());
  return GLX_OK;
}

int ball_search_impl(const double* X, int64_t n, int d, double epsilon, const double* F, int mf, int device, glx_ball_result* res) {
  GlxCall call;
  GLX_UP(call.begin(device));
  hipStream_t st = call.stream();
  for (int i = 0; i < BS_COUNT; ++i) g_ball_stats[i] = 0.0;
  // the bounding box, on the host's threads, BEFORE anything travels: the plan and the finiteness refusal need it, and a checked
  // upload (glx_upload) ends in a stream synchronisation of its own, so there is nothing to overlap it with
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(8, n / 65536));
  std::vector<double> lo((size_t)nt * d), hi((size_t)nt * d);
  glx_host_parallel(nt, [&](int t) {
    double* l = lo.data() + (size_t)t * d;
    double* h = hi.data() + (size_t)t * d;
    const int64_t r0 = n * t / nt, r1 = n * (t + 1) / nt;
    for (int f = 0; f < d; ++f) l[f] = h[f] = X[r0 * d + f];
    for (int64_t i = r0; i < r1; ++i)
      for (int f = 0; f < d; ++f) {
        const double v = X[i * d + f];
        if (v < l[f]) l[f] = v;
        if (v > h[f]) h[f] = v;
      }
  });
  for (int t = 1; t < nt; ++t)
    for (int f = 0; f < d; ++f) {
      lo[f] = std::min(lo[f], lo[(size_t)t * d + f]);
      hi[f] = std::max(hi[f], hi[(size_t)t * d + f]);
    }
  for (int f = 0; f < d; ++f)
    GLX_CHECK(std::isfinite(lo[f]) && std::isfinite(hi[f]), GLX_EINVAL, "glx_ball_search: coordinate %d is not finite", f);
  const BallPlan plan = ball_make_plan(n, d, epsilon, lo.data(), hi.data());
  BallGrid G;
  G.g = plan.g;
  G.ncells = plan.ncells;
  for (int a = 0; a < 3; ++a) {
    G.axis[a] = plan.axis[a];
    G.lo[a] = plan.lo[a];
    G.h[a] = plan.h[a];
    G.nc[a] = plan.nc[a];
    G.stride[a] = plan.stride[a];
  }
  const double eps2 = epsilon * epsilon;

  GLX_POOL(glx_pool_alloc((void**)&res->X, std::max<size_t>((size_t)n * d * 8, 8)));
  GLX_UP(glx_upload(res->X, X, (size_t)n * d * 8, st, __func__));
  if (F) {
    GLX_POOL(glx_pool_alloc((void**)&res->F, std::max<size_t>((size_t)n * mf * 8, 8)));
    GLX_UP(glx_upload(res->F, F, (size_t)n * mf * 8, st, __func__));
  }
  GLX_POOL(glx_pool_alloc((void**)&res->off, (size_t)(n + 1) * 8));
  int *cid, *cell_cnt, *orig, *scell, *cnt, *hubs;
  long long* cell_start;
  double* Xs;
  unsigned long long* counters;    // [0] pairs tested, [1] (int) hub rows
  GLX_POOL(call.alloc(&cid, (size_t)n));
  GLX_POOL(call.alloc(&cell_cnt, (size_t)plan.ncells));
  GLX_POOL(call.alloc(&cell_start, (size_t)(plan.ncells + 1)));
  GLX_POOL(call.alloc(&orig, (size_t)n));
  GLX_POOL(call.alloc(&scell, (size_t)n));
  GLX_POOL(call.alloc(&Xs, (size_t)n * d));
  GLX_POOL(call.alloc(&cnt, (size_t)n));
  GLX_POOL(call.alloc(&hubs, (size_t)n));
  GLX_POOL(call.alloc(&counters, 2));
  GLX_UP(glx_zero_async(cell_cnt, ((size_t)plan.ncells * 4 + 7) & ~(size_t)7, st));
  GLX_UP(glx_zero_async(counters, 16, st));
  hipEvent_t* ev = call.work()->ev;
  const unsigned gn = (unsigned)((n + 255) / 256);
  GLX_HIP(hipEventRecord(ev[0], st));
  hipLaunchKernelGGL(ball_cellid_kernel, dim3(gn), dim3(256), 0, st, (const double*)res->X, n, d, G, cid, cell_cnt);
  GLX_HIP(hipGetLastError());
  hipLaunchKernelGGL(ball_scan_kernel, dim3(1), dim3(1024), 0, st, (const int*)cell_cnt, (int64_t)plan.ncells, cell_start);
  GLX_HIP(hipGetLastError());
  hipLaunchKernelGGL(ball_scatter_kernel, dim3(gn), dim3(256), 0, st, (const double*)res->X, n, d, (const int*)cid,
                     (const long long*)cell_start, cell_cnt, orig, scell, Xs);
  GLX_HIP(hipGetLastError());
  GLX_HIP(hipEventRecord(ev[1], st));
  GLX_UP(launch_pairs<false>(d, (unsigned)plan.nqb, st, Xs, orig, scell, cell_start, n, G, eps2, cnt, nullptr, nullptr, counters));
  hipLaunchKernelGGL(ball_scan_kernel, dim3(1), dim3(1024), 0, st, (const int*)cnt, n, res->off);
  GLX_HIP(hipGetLastError());
  hipLaunchKernelGGL(ball_hubs_kernel, dim3(gn), dim3(256), 0, st, (const int*)cnt, n, (int*)(counters + 1), hubs);
  GLX_HIP(hipGetLastError());
  GLX_HIP(hipEventRecord(ev[2], st));
  // the total, the hub rows and the tested pairs land in the work set's page-locked staging area
  unsigned long long* stage = nullptr;
  GLX_POOL(call.stage(&stage, 8));
  // (24 bytes into page-locked memory: far below the size from which glx_download stages and checks a transfer, so a plain copy)
  GLX_HIP(hipMemcpyAsync(stage, counters, 16, hipMemcpyDeviceToHost, st));
  GLX_HIP(hipMemcpyAsync(stage + 2, res->off + n, 8, hipMemcpyDeviceToHost, st));
  GLX_HIP(hipStreamSynchronize(st));
  const long long total = (long long)stage[2];
  const int nhub = (int)(stage[1] & 0xffffffffull);
  float ms = 0.f;
  GLX_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
  g_ball_stats[BS_GRID_MS] = ms;
  GLX_HIP(hipEventElapsedTime(&ms, ev[1], ev[2]));
  g_ball_stats[BS_COUNT_MS] = ms;
  g_ball_stats[BS_TESTED] = (double)stage[0];
  g_ball_stats[BS_ACCEPTED] = (double)total;
  g_ball_stats[BS_CELLS] = (double)plan.ncells;
  GLX_CHECK(total >= 0 && total <= BALL_NNZ_MAX, GLX_EUNSUPPORTED,
            "glx_ball_search: the graph has %lld entries, more than the %lld an int32 CSR matrix holds", total, (long long)BALL_NNZ_MAX);
  res->nnz = total;
  if (total == 0) return GLX_OK;
  GLX_POOL(glx_pool_alloc((void**)&res->col, (size_t)total * 4));
  GLX_HIP(hipEventRecord(ev[0], st));
  GLX_UP(launch_pairs<true>(d, (unsigned)plan.nqb, st, Xs, orig, scell, cell_start, n, G, eps2, nullptr, res->off, res->col, nullptr));
  GLX_HIP(hipEventRecord(ev[1], st));
  hipLaunchKernelGGL(ball_sort_rows_kernel, dim3((unsigned)std::min<int64_t>(n, 1 << 16)), dim3(64), 0, st, (const long long*)res->off, n,
                     res->col);
  GLX_HIP(hipGetLastError());
  if (nhub > 0) {
    hipLaunchKernelGGL(ball_sort_hub_kernel, dim3((unsigned)nhub), dim3(1024), 0, st, (const long long*)res->off, (const int*)hubs, res->col);
    GLX_HIP(hipGetLastError());
  }
  GLX_HIP(hipEventRecord(ev[2], st));
  GLX_HIP(hipStreamSynchronize(st));
  GLX_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
  g_ball_stats[BS_FILL_MS] = ms;
  GLX_HIP(hipEventElapsedTime(&ms, ev[1], ev[2]));
  g_ball_stats[BS_SORT_MS] = ms;
  return GLX_OK;
}
}  // namespace

// X (n, d) and optional features F (n, m_f), host arrays, finite; epsilon >= 0.  The structure of the graph stays on the device in *out.
extern "C" int glx_ball_search(const double* X, int64_t n, int d, double epsilon, const double* F, int m_f, int device,
                               glx_ball_result** out) {
  GLX_CHECK(out, GLX_EINVAL, "glx_ball_search: null output");
  *out = nullptr;
  GLX_CHECK(X && n >= 1 && d >= 1, GLX_EINVAL, "glx_ball_search: need n >= 1 points of d >= 1 coordinates (n=%lld d=%d)", (long long)n, d);
  GLX_CHECK(epsilon >= 0.0, GLX_EINVAL, "glx_ball_search: epsilon must not be negative or NaN");
  GLX_CHECK(n <= BALL_NNZ_MAX, GLX_EUNSUPPORTED, "glx_ball_search: n=%lld does not fit int32", (long long)n);
  GLX_CHECK(!F || m_f >= 1, GLX_EINVAL, "glx_ball_search: features need m_f >= 1 (m_f=%d)", m_f);
  glx_ball_result* res = new glx_ball_result();
  res->n = n;
  res->d = d;
  res->mf = F ? m_f : 0;
  res->device = device;
  res->epsilon = epsilon;
  const int rc = ball_search_impl(X, n, d, epsilon, F, m_f, device, res);
  if (rc) {
    glx_ball_result_destroy(res);
    return rc;
  }
  *out = res;
  return GLX_OK;
}

// kernel: 0 structure and distances only (val = 1 everywhere, nothing dropped: the caller weighs on the host), 1 uniform,
// 2 gaussian, 4 distance, 5 singular.  rowptr [n + 1], col / val / dists_out / fdists_out [glx_ball_result_nnz]; val and either
// distance output may be NULL.  *nnz_out = entries written (fewer than the result's where zero weights were dropped).
extern "C" int glx_ball_result_to_csr(const glx_ball_result* res, int kernel, double epsilon_f, int32_t* rowptr, int32_t* col, double* val,
                                      double* dists_out, double* fdists_out, int64_t* nnz_out) {
  GLX_CHECK(res && res->off, GLX_EINVAL, "glx_ball_result_to_csr: empty result");
  GLX_CHECK(rowptr && nnz_out && (col || res->nnz == 0), GLX_EINVAL, "glx_ball_result_to_csr: null buffer");
  GLX_CHECK(kernel == BK_GIVEN || kernel == BK_UNIFORM || kernel == BK_GAUSSIAN || kernel == BK_DISTANCE || kernel == BK_SINGULAR, GLX_EINVAL,
            "glx_ball_result_to_csr: bad kernel id %d", kernel);
  GLX_CHECK(!fdists_out || res->F, GLX_EINVAL, "glx_ball_result_to_csr: feature distances asked of a search without features");
  *nnz_out = 0;
  const int64_t n = res->n, nnz = res->nnz;
  if (nnz == 0) {
    for (int64_t i = 0; i <= n; ++i) rowptr[i] = 0;
    return GLX_OK;
  }
  GlxCall call;
  GLX_UP(call.begin(res->device));
  hipStream_t st = call.stream();
  double *dval, *dd = nullptr, *dfd = nullptr;
  int *kept, *rp32;
  long long* off2;
  GLX_POOL(call.alloc(&dval, (size_t)nnz));
  if (dists_out) GLX_POOL(call.alloc(&dd, (size_t)nnz));
  if (fdists_out) GLX_POOL(call.alloc(&dfd, (size_t)nnz));
  GLX_POOL(call.alloc(&kept, (size_t)n));
  GLX_POOL(call.alloc(&off2, (size_t)(n + 1)));
  GLX_POOL(call.alloc(&rp32, (size_t)(n + 1)));
  hipEvent_t* ev = call.work()->ev;
  const unsigned gr = (unsigned)((n * BALL_ROW_LANES + 255) / 256);
  GLX_HIP(hipEventRecord(ev[0], st));
  hipLaunchKernelGGL(ball_weights_kernel, dim3(gr), dim3(256), 0, st, (const double*)res->X, (const double*)res->F, n, res->d, res->mf,
                     (const long long*)res->off, (const int*)res->col, kernel, res->epsilon * res->epsilon, epsilon_f * epsilon_f, dval, dd,
                     dfd, kept);
  GLX_HIP(hipGetLastError());
  hipLaunchKernelGGL(ball_scan_kernel, dim3(1), dim3(1024), 0, st, (const int*)kept, n, off2);
  GLX_HIP(hipGetLastError());
  GLX_HIP(hipEventRecord(ev[1], st));
  unsigned long long* stage = nullptr;
  GLX_POOL(call.stage(&stage, 8));
  GLX_HIP(hipMemcpyAsync(stage, off2 + n, 8, hipMemcpyDeviceToHost, st));   // (8 bytes into page-locked memory: a plain copy, as above)
  GLX_HIP(hipStreamSynchronize(st));
  const int64_t nkeep = (int64_t)stage[0];
  float ms = 0.f;
  GLX_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
  g_ball_stats[BS_WEIGHTS_MS] = ms;
  GLX_CHECK(nkeep >= 0 && nkeep <= nnz, GLX_EHIP, "glx_ball_result_to_csr: %lld of %lld entries kept", (long long)nkeep, (long long)nnz);
  const unsigned gp = (unsigned)((n + 1 + 255) / 256);
  const int* out_col = res->col;
  const double* out_val = dval;
  const long long* out_off = res->off;
  if (nkeep < nnz) {
    // (the distance outputs belong to the weigh-on-the-host mode, which drops nothing here)
    GLX_CHECK(!dists_out && !fdists_out, GLX_EINVAL, "glx_ball_result_to_csr: distances of a matrix with dropped entries");
    int* col2;
    double* val2;
    GLX_POOL(call.alloc(&col2, (size_t)nkeep));
    GLX_POOL(call.alloc(&val2, (size_t)nkeep));
    hipLaunchKernelGGL(ball_compact_kernel, dim3(gr), dim3(256), 0, st, n, (const long long*)res->off, (const int*)res->col,
                       (const double*)dval, (const long long*)off2, col2, val2);
    GLX_HIP(hipGetLastError());
    out_col = col2;
    out_val = val2;
    out_off = off2;
  }
  hipLaunchKernelGGL(ball_rowptr_kernel, dim3(gp), dim3(256), 0, st, out_off, n, rp32);
  GLX_HIP(hipGetLastError());
  GLX_UP(glx_download(rowptr, rp32, (size_t)(n + 1) * 4, st, __func__));
  if (nkeep > 0) {
    GLX_UP(glx_download(col, out_col, (size_t)nkeep * 4, st, __func__));
    if (val) GLX_UP(glx_download(val, out_val, (size_t)nkeep * 8, st, __func__));
    if (dists_out) GLX_UP(glx_download(dists_out, dd, (size_t)nkeep * 8, st, __func__));
    if (fdists_out) GLX_UP(glx_download(fdists_out, dfd, (size_t)nkeep * 8, st, __func__));
  }
  GLX_HIP(hipStreamSynchronize(st));
  *nnz_out = nkeep;
  return GLX_OK;
}
