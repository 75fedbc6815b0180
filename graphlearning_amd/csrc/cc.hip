// Connected components of the pattern of a CSR matrix: graph.connected_components / largest_connected_component (glx_components).
// Every stored entry (i, j) with i != j joins i and j; direction and value are ignored.  The labels are those of
// scipy.sparse.csgraph.connected_components(W, directed=False) -- and of its default weak form -- on every vertex: components are
// numbered by their smallest vertex, ascending.  No floating point anywhere.
//
// The algorithm is the lock-free union-find of Jaiganesh and Burtscher (ECL-CC, HPDC 2018) in one pass, no rounds, no host loop:
//   init      parent[i] = the first smaller neighbour among the first entries of row i, else i          (cc_first_parent, cc_plan.h)
//   union     every stored entry: find both roots, hook the LARGER root under the SMALLER with a compare-and-swap; a failed
//             compare-and-swap continues from the value it returned; find halves the path it walks       (cc_union, cc_find, cc_plan.h)
//   flatten   behind the kernel boundary: root[i] = find(i); the workgroup counts its roots
//   number    flag[i] = (root[i] == i); exclusive prefix sum of the flags by tiles of CC_SCAN_TILE vertices (tile totals, one
//             workgroup scans the totals, every tile scans itself from its offset); labels[i] = rank[root[i]]; ncomp = the total
// cc_find and cc_union are the templates of cc_plan.h, which the host test runs with plain memory; here they run on CcAtomicParent.
//
// What the code guarantees, and why.
//
// 1. Every root is its component's smallest vertex, so the partition AND the labels are a pure function of the input.
//    Invariant: parent[x] <= x at all times.  init writes a smaller neighbour or x; a hook writes lo < hi into parent[hi]; halving
//    writes an ancestor of x, and every ancestor of x is below x by the invariant.  A vertex with parent[x] < x never becomes a root
//    again (nobody writes x into parent[x]; the hook's compare-and-swap expects parent[hi] == hi), so the set of ancestors of a vertex
//    only grows, and there is no cycle (indices fall strictly along parent[]).  A tree's root is therefore below every other member.
//    A hook joins two trees that hold the two ends of a stored entry, or of entries already processed: trees never span two
//    components.  When the union kernel has ended, every stored entry has been through cc_union, which returns only after a
//    compare-and-swap joined the two trees or both finds met at one root: the trees ARE the components, each root the minimum of
//    its component.  flatten and number are functions of that forest: rank[r] = number of roots below r.  The interleaving of the
//    threads decides the shape of the trees on the way, never the roots.
//
// 2. Every loop is bounded and nothing waits on another thread.  cc_find walks strictly decreasing indices (x -> parent[parent[x]]
//    < x), at most x steps.  In cc_union a failed compare-and-swap means the root was hooked meanwhile, i.e. moved strictly down:
//    max(ru, rv) falls with every failure, at most max(u, v) failures.  No spin-wait, no grid-wide barrier, no cooperative launch: a
//    thread's progress needs nobody else's, so the divergence of a wavefront's lanes in these loops cannot lock up.
//
// 3. Visibility across the XCDs.  Inside the union kernel (and in flatten, which halves too) EVERY read and write of parent[] is a
//    relaxed agent-scope atomic: __hip_atomic_load, __hip_atomic_compare_exchange_strong, and __hip_atomic_store for the halving
//    write.  A plain load could be served from the CU's L1 or from another XCD's L2 long after the word changed.  Even a stale value
//    would be harmless: what parent[x] held at any earlier time is x itself or an ancestor of x, and ancestors stay ancestors (1.); a
//    stale "x is a root" only leads to a compare-and-swap, which is decided at the memory side on the current value and fails.  The
//    code does not rely on that -- it reads nothing stale.  init writes with plain stores: a kernel boundary lies between it and the
//    first atomic.  number's kernels read root[] and rank[] of EARLIER launches with plain loads.
//
// 4. Row classes (cc_plan.h): rows below CC_WAVE_ROW stored entries take a thread per row, rows at or above it a wavefront per row,
//    lanes striding the entries.  The thread-per-row kernel runs over all rows and skips the long ones; the host lists the long ones.
//
// 5. No out-of-range access.  Before anything is launched the host checks rowptr (rowptr[0] == 0, monotone, rowptr[n] == nnz: every
//    entry offset a kernel forms lies in [0, nnz)).  A device pass then checks every column index against [0, n) and the host reads
//    its result BEFORE init and union are launched; a bad index is GLX_EINVAL, never a fault.  Entry offsets are 64-bit in the
//    kernels (a lane's e + 64 may pass 2^31).
//
// 6. Device buffers come from the library's pools (GlxCall), transfers of 128 KB or more go through the checked upload and download
//    (glx_upload / glx_download).  Only rowptr and col go up, the values never.
#include "glx_internal.h"
#include "cc_plan.h"
#include <chrono>
#include <vector>

namespace {
thread_local int t_wave_row = 0;          // glx_components_set_wave_row: 0 = CC_WAVE_ROW
thread_local int64_t t_last_long = 0;     // long rows of the calling thread's last call

// parent[] of the device: relaxed agent-scope atomics, every access
struct CcAtomicParent {
  int32_t* p;
  __device__ __forceinline__ int32_t load(int32_t i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ void store(int32_t i, int32_t v) const { __hip_atomic_store(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ int32_t cas(int32_t i, int32_t expected, int32_t desired) const {
    __hip_atomic_compare_exchange_strong(p + i, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expected;          // (on failure the builtin stores what it found there)
  }
};
}  // namespace

// *first_bad <- the lowest entry offset whose column index lies outside [0, n) (left at ~0: none)
__global__ __launch_bounds__(256) void cc_check_cols_kernel(const int32_t* __restrict__ col, int64_t nnz, int64_t n,
                                                            unsigned long long* first_bad) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  unsigned long long mine = ~0ull;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < nnz; e += stride) {
    const int32_t j = col[e];
    if ((j < 0 || j >= n) && (unsigned long long)e < mine) mine = (unsigned long long)e;
  }
  if (mine != ~0ull) atomicMin(first_bad, mine);
}

__global__ __launch_bounds__(256) void cc_init_kernel(int32_t* parent, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                      int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) parent[i] = cc_first_parent((int32_t)i, col, rowptr[i], rowptr[i + 1]);
}

// a thread per row; rows of the wavefront class are left to cc_union_long_kernel
__global__ __launch_bounds__(256) void cc_union_rows_kernel(int32_t* parent_, const int32_t* __restrict__ rowptr,
                                                            const int32_t* __restrict__ col, int64_t n, int wave_row) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t e0 = rowptr[i], e1 = rowptr[i + 1];
  if (e1 - e0 >= wave_row) return;
  const CcAtomicParent parent{parent_};
  for (int64_t e = e0; e < e1; ++e) {
    const int32_t j = col[e];
    if (j != (int32_t)i) cc_union(parent, (int32_t)i, j);
  }
}

// a wavefront per listed row, its lanes striding the entries
__global__ __launch_bounds__(256) void cc_union_long_kernel(int32_t* parent_, const int32_t* __restrict__ rowptr,
                                                            const int32_t* __restrict__ col, const int32_t* __restrict__ rows,
                                                            int64_t nrows) {
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= nrows) return;
  const int32_t i = rows[w];
  const int64_t e1 = rowptr[i + 1];
  const CcAtomicParent parent{parent_};
  for (int64_t e = (int64_t)rowptr[i] + (threadIdx.x & 63); e < e1; e += 64) {
    const int32_t j = col[e];
    if (j != i) cc_union(parent, i, j);
  }
}

// root[i] = find(i) for the CC_SCAN_TILE vertices of the workgroup's tile; tile_cnt[tile] = how many of them are roots
__global__ __launch_bounds__(256) void cc_flatten_kernel(int32_t* parent_, int32_t* __restrict__ root, int64_t n,
                                                         int32_t* __restrict__ tile_cnt) {
  __shared__ int s_cnt[4];
  const CcAtomicParent parent{parent_};
  const int64_t base = (int64_t)blockIdx.x * CC_SCAN_TILE;
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < CC_SCAN_TILE / 256; ++k) {
    const int64_t i = base + k * 256 + threadIdx.x;
    if (i < n) {
      const int32_t r = cc_find(parent, (int32_t)i);
      root[i] = r;
      cnt += r == (int32_t)i;
    }
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) cnt += __shfl_down(cnt, s);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// exclusive prefix sum over the 256 values the workgroup's threads hold (v), in thread order; *total_out <- their sum (all threads).
// s_wave: 4 ints of LDS, free again on return.
__device__ __forceinline__ int cc_block_exclusive(int v, int* s_wave, int* total_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const int up = __shfl_up(incl, s);
    if (lane >= s) incl += up;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (w < wave) before += s_wave[w];
    total += s_wave[w];
  }
  __syncthreads();
  *total_out = total;
  return before + incl - v;
}

// tile_cnt[0 .. ntiles) <- its exclusive prefix sum, in place; *total <- the sum: one workgroup walks the totals in pieces of 256
__global__ __launch_bounds__(256) void cc_scan_tiles_kernel(int32_t* tile_cnt, int64_t ntiles, int32_t* total) {
  __shared__ int s_wave[4];
  int carry = 0;
  for (int64_t base = 0; base < ntiles; base += 256) {
    const int64_t t = base + threadIdx.x;
    const int v = t < ntiles ? tile_cnt[t] : 0;
    int sum;
    const int ex = cc_block_exclusive(v, s_wave, &sum);
    if (t < ntiles) tile_cnt[t] = carry + ex;
    carry += sum;
  }
  if (threadIdx.x == 0) *total = carry;
}

// rank[i] = number of roots below i, for the vertices of the workgroup's tile: thread t holds the vertices base + 4 t .. base + 4 t + 3
__global__ __launch_bounds__(256) void cc_rank_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ tile_off, int64_t n,
                                                      int32_t* __restrict__ rank) {
  __shared__ int s_wave[4];
  constexpr int ITEMS = CC_SCAN_TILE / 256;
  const int64_t i0 = (int64_t)blockIdx.x * CC_SCAN_TILE + (int64_t)threadIdx.x * ITEMS;
  int flag[ITEMS], mine = 0;
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    flag[j] = (i0 + j < n && root[i0 + j] == (int32_t)(i0 + j)) ? 1 : 0;
    mine += flag[j];
  }
  int sum;
  int run = tile_off[blockIdx.x] + cc_block_exclusive(mine, s_wave, &sum);
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    if (i0 + j < n) rank[i0 + j] = run;
    run += flag[j];
  }
}

__global__ __launch_bounds__(256) void cc_label_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ rank, int64_t n,
                                                       int32_t* __restrict__ labels) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) labels[i] = rank[root[i]];
}

extern "C" int glx_components_set_wave_row(int min_entries) {
  GLX_CHECK(min_entries >= 0, GLX_EINVAL, "glx_components_set_wave_row: %d is negative", min_entries);
  t_wave_row = min_entries;
  return GLX_OK;
}

extern "C" int glx_components_plan(int64_t out[4]) {
  GLX_CHECK(out, GLX_EINVAL, "glx_components_plan: null argument");
  out[0] = t_wave_row > 0 ? t_wave_row : CC_WAVE_ROW;
  out[1] = CC_WAVE_ROW;
  out[2] = CC_SCAN_TILE;
  out[3] = t_last_long;
  return GLX_OK;
}

extern "C" int glx_components(int64_t n, int64_t nnz, const int32_t* rowptr, const int32_t* col, int32_t* labels, int64_t* ncomp_out,
                              double* ms_out, int device) {
  GLX_CHECK(rowptr && labels && ncomp_out && (nnz == 0 || col), GLX_EINVAL, "glx_components: null argument");
  GLX_CHECK(n >= 1 && nnz >= 0, GLX_EINVAL, "glx_components: bad sizes (n=%lld nnz=%lld)", (long long)n, (long long)nnz);
  GLX_CHECK(n <= 0x7fffffff && nnz <= 0x7fffffff, GLX_EUNSUPPORTED, "glx_components: n=%lld or nnz=%lld above 2^31 - 1", (long long)n,
            (long long)nnz);
  auto ms_since = [](std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  };
  double ms[4] = {0, 0, 0, 0};      // upload, checks, kernels, download
  auto t0 = std::chrono::steady_clock::now();
  const int64_t bad_row = cc_check_rowptr(n, nnz, rowptr);
  GLX_CHECK(bad_row != n + 2, GLX_EINVAL, "glx_components: the row pointers do not span the %lld entries (first %d, last %d)", (long long)nnz,
            rowptr[0], rowptr[n]);
  GLX_CHECK(bad_row == 0, GLX_EINVAL, "glx_components: the row pointers decrease at row %lld", (long long)(bad_row - 1));
  const int wave_row = t_wave_row > 0 ? t_wave_row : CC_WAVE_ROW;
  std::vector<int32_t> lng;
  cc_long_rows(n, rowptr, wave_row, &lng);
  t_last_long = (int64_t)lng.size();
  ms[1] = ms_since(t0);

  GlxCall call;
  GLX_UP(call.begin(device));
  hipStream_t st = call.stream();
  t0 = std::chrono::steady_clock::now();
  const int64_t ntiles = (n + CC_SCAN_TILE - 1) / CC_SCAN_TILE;
  int32_t *d_rowptr = nullptr, *d_col = nullptr, *d_long = nullptr, *d_parent = nullptr, *d_root = nullptr, *d_rank = nullptr,
          *d_labels = nullptr, *d_tiles = nullptr;
  unsigned long long *d_flag = nullptr, *h_flag = nullptr;      // [0] first bad entry offset, [1] (low word) the component count
  GLX_UP(call.put(&d_rowptr, rowptr, (size_t)(n + 1), __func__));
  GLX_UP(call.put(&d_col, col, (size_t)nnz, __func__));
  GLX_UP(call.put(&d_long, lng.data(), lng.size(), __func__));
  GLX_UP(call.alloc(&d_parent, (size_t)n));
  GLX_UP(call.alloc(&d_root, (size_t)n));
  GLX_UP(call.alloc(&d_rank, (size_t)n));
  GLX_UP(call.alloc(&d_labels, (size_t)n));
  GLX_UP(call.alloc(&d_tiles, (size_t)ntiles));
  GLX_UP(call.alloc(&d_flag, 2));
  GLX_UP(call.stage(&h_flag, 2));
  GLX_HIP(hipStreamSynchronize(st));
  ms[0] = ms_since(t0);

  // the column check, read by the host before any kernel follows an index
  t0 = std::chrono::steady_clock::now();
  h_flag[0] = ~0ull;
  h_flag[1] = 0;
  GLX_HIP(hipMemcpyAsync(d_flag, h_flag, 16, hipMemcpyHostToDevice, st));
  if (nnz > 0) {
    const unsigned grid = (unsigned)std::min<int64_t>((nnz + 255) / 256, 1 << 16);
    hipLaunchKernelGGL(cc_check_cols_kernel, dim3(grid), dim3(256), 0, st, (const int32_t*)d_col, nnz, n, d_flag);
    GLX_HIP(hipGetLastError());
  }
  GLX_HIP(hipMemcpyAsync(h_flag, d_flag, 8, hipMemcpyDeviceToHost, st));
  GLX_HIP(hipStreamSynchronize(st));
  ms[1] += ms_since(t0);
  GLX_CHECK(h_flag[0] == ~0ull, GLX_EINVAL, "glx_components: column index %d at entry %llu outside [0, %lld)", col[h_flag[0]], h_flag[0],
            (long long)n);

  t0 = std::chrono::steady_clock::now();
  const unsigned grid_n = (unsigned)((n + 255) / 256), grid_t = (unsigned)ntiles;
  hipLaunchKernelGGL(cc_init_kernel, dim3(grid_n), dim3(256), 0, st, d_parent, (const int32_t*)d_rowptr, (const int32_t*)d_col, n);
  GLX_HIP(hipGetLastError());
  hipLaunchKernelGGL(cc_union_rows_kernel, dim3(grid_n), dim3(256), 0, st, d_parent, (const int32_t*)d_rowptr, (const int32_t*)d_col, n,
                     wave_row);
  GLX_HIP(hipGetLastError());
  if (!lng.empty()) {
    hipLaunchKernelGGL(cc_union_long_kernel, dim3((unsigned)((lng.size() + 3) / 4)), dim3(256), 0, st, d_parent, (const int32_t*)d_rowptr,
                       (const int32_t*)d_col, (const int32_t*)d_long, (int64_t)lng.size());
    GLX_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(grid_t), dim3(256), 0, st, d_parent, d_root, n, d_tiles);
  GLX_HIP(hipGetLastError());
  hipLaunchKernelGGL(cc_scan_tiles_kernel, dim3(1), dim3(256), 0, st, d_tiles, ntiles, (int32_t*)(d_flag + 1));
  GLX_HIP(hipGetLastError());
  hipLaunchKernelGGL(cc_rank_kernel, dim3(grid_t), dim3(256), 0, st, (const int32_t*)d_root, (const int32_t*)d_tiles, n, d_rank);
  GLX_HIP(hipGetLastError());
  hipLaunchKernelGGL(cc_label_kernel, dim3(grid_n), dim3(256), 0, st, (const int32_t*)d_root, (const int32_t*)d_rank, n, d_labels);
  GLX_HIP(hipGetLastError());
  GLX_HIP(hipStreamSynchronize(st));
  ms[2] = ms_since(t0);

  t0 = std::chrono::steady_clock::now();
  GLX_HIP(hipMemcpyAsync(h_flag + 1, d_flag + 1, 8, hipMemcpyDeviceToHost, st));
  GLX_UP(glx_download(labels, d_labels, (size_t)n * 4, st, __func__));
  GLX_HIP(hipStreamSynchronize(st));
  ms[3] = ms_since(t0);
  *ncomp_out = (int64_t)(h_flag[1] & 0xffffffffull);
  if (ms_out)
    for (int q = 0; q < 4; ++q) ms_out[q] = ms[q];
  return GLX_OK;
}
