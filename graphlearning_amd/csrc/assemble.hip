// kNN data -> symmetric sparse weight matrix on the device: weightmatrix.knn of the reference
// given knn_data (graphlearning/weightmatrix.py:134-187): kernel weights (:140-164), COO->CSR
// with duplicates summed (:171-175), symmetrisation (:177-183), zero diagonal + drop zeros
// (:185-186).  No global sort: every row of A has exactly k entries, so A^T is built by
// counting reverse neighbours (atomics) + a host scan of n counters, then one wavefront per
// row merges its forward and reverse lists with a bitonic sort in LDS and applies the
// symmetrisation rule per column; a hub vertex (more entries than one wavefront's LDS share holds)
// gets a whole workgroup that sorts in a global scratch.  Output: canonical CSR (sorted, no duplicates, no zeros).
// Which kernel a row belongs to, the sort key and the per-column rule are assemble_plan.h's; the whole matrix (glx_knn_to_csr*) and a
// block of its rows (glx_knn_rows_to_csr) differ in where the reverse entries come from and run ONE merge pipeline (asm_merge_rows).
#include "glx_internal.h"
#include "assemble_plan.h"
#include "exp_cr.h"
#include <algorithm>
#include <vector>

enum { K_GIVEN = 0, K_UNIFORM = 1, K_GAUSSIAN = 2, K_SYMGAUSSIAN = 3, K_DISTANCE = 4, K_SINGULAR = 5 };

// weights exactly as numpy forms them, operation by operation (weightmatrix.py:140-156); the exponential is the correctly
// rounded one of exp_cr.h (numpy's is the host libm's or its own SIMD kernel: within an ulp of this, host by host)
__global__ void knn_weights_kernel(const int64_t* __restrict__ ind, const double* __restrict__ dist, int64_t n, int kk, int k,
                                   int kernel, const double* __restrict__ given, double* __restrict__ w) {
#pragma clang fp contract(off)
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * k) return;
  const int64_t i = e / k;
  const int t = (int)(e % k);
  const double d = dist ? dist[i * kk + t] : 0.0;
  double v = 1.0;
  if (kernel == K_GIVEN) {
    v = given[i * k + t];
  } else if (kernel == K_GAUSSIAN) {
    const double dk = dist[i * kk + k - 1];
    const double D = d * d, eps = dk * dk;
    const double a = -4.0 * D;
    v = exp_cr(a / eps);
  } else if (kernel == K_SYMGAUSSIAN) {
    const double ei = dist[i * kk + k - 1];
    // (an index outside [0, n) is reported by count_reverse_kernel, which runs behind this kernel: here it must not become an
    // out-of-bounds read -- user-supplied knn_data reaches this kernel unchecked)
    const int64_t jn = ind[i * kk + t];
    const double ej = dist[(jn >= 0 && jn < n ? jn : i) * kk + k - 1];
    const double a = -4.0 * d;
    const double b = a * d;
    const double c = b / ei;
    v = exp_cr(c / ej);
  } else if (kernel == K_DISTANCE) {
    v = d;
  } else if (kernel == K_SINGULAR) {
    v = 1.0 / (d == 0.0 ? 1.0 : d);
  }
  w[e] = v;
}

__global__ void count_reverse_kernel(const int64_t* __restrict__ ind, int64_t n, int kk, int k, int* __restrict__ rcnt,
                                     int* __restrict__ bad) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * k) return;
  const int64_t j = ind[(e / k) * kk + (e % k)];
  if (j < 0 || j >= n) { *bad = 1; return; }
  atomicAdd(&rcnt[j], 1);
}

__global__ void fill_reverse_kernel(const int64_t* __restrict__ ind, const double* __restrict__ w, int64_t n, int kk, int k,
                                    const int64_t* __restrict__ roff, int* __restrict__ cursor, int* __restrict__ rsrc,
                                    unsigned short* __restrict__ rpos, double* __restrict__ rw) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * k) return;
  const int64_t i = e / k;
  const int64_t j = ind[i * kk + (e % k)];
  const int64_t pos = roff[j] + atomicAdd(&cursor[j], 1);
  rsrc[pos] = (int)i;
  rpos[pos] = (unsigned short)(e % k);   // duplicates of one source row are summed in the order the row lists them
  rw[pos] = w[e];
}

// one wavefront per row of at most ROW_CAP entries: forward and reverse entries sorted by key in LDS, asm_segment per column.  ONE
// pass -- the kept entries go to the row's slot in a scratch image (asm_row_slot) and compact_rows_kernel moves them to their place
// once the row pointers exist; sorting every row twice (count, then write) cost a fifth of weightmatrix.knn's assembly.
// rowlist: only these rows (merge_rows_small_kernel has the others).  A hub row is marked (rowcnt -1, *overflow) for merge_hub_kernel.
__global__ __launch_bounds__(256) void merge_rows_kernel(const int64_t* __restrict__ ind, const double* __restrict__ w, int64_t n, int kk,
                                                         int k, const int64_t* __restrict__ roff, const int* __restrict__ rsrc,
                                                         const unsigned short* __restrict__ rpos, const double* __restrict__ rw, int sym,
                                                         int* __restrict__ rowcnt, int* __restrict__ col_out, double* __restrict__ val_out,
                                                         int* __restrict__ overflow, int64_t row_base, const int* __restrict__ rowlist,
                                                         int nlist) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char sm[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long* key = (unsigned long long*)sm + (size_t)wave * ROW_CAP;
  double* val = (double*)(sm + (size_t)4 * ROW_CAP * 8) + (size_t)wave * ROW_CAP;
  int64_t i = (int64_t)blockIdx.x * 4 + wave;
  if (rowlist) {
    if (i >= nlist) return;
    i = rowlist[i];
  }
  if (i >= n) return;
  const int rc = sym == SYM_NONE ? 0 : (int)(roff[i + 1] - roff[i]);
  const int M = k + rc;
  const int cls = asm_row_class(k, M);
  if (cls == ASM_ROW_REGISTER) return;
  if (cls == ASM_ROW_HUB) {
    if (lane == 0) { rowcnt[i] = -1; *overflow = 1; }
    return;
  }
  int P = 64;
  while (P < M) P <<= 1;
  for (int e = lane; e < P; e += 64) {
    unsigned long long kx = ~0ull;
    double v = 0.0;
    if (e < k) {
      kx = asm_key((unsigned)ind[i * kk + e], ASM_KIND_FORWARD, (unsigned)e);
      v = w[i * k + e];
    } else if (e < M) {
      const int64_t p = roff[i] + (e - k);
      kx = asm_key((unsigned)rsrc[p], ASM_KIND_REVERSE, rpos[p]);
      v = rw[p];
    }
    key[e] = kx;
    val[e] = v;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = lane; t < P / 2; t += 64) {
        const int lo = (t / stride) * stride * 2 + (t % stride);
        const int hi = lo + stride;
        const bool up = ((lo & size) == 0);
        const unsigned long long kl = key[lo], kh = key[hi];
        // (one comparison of selected operands: as `up ? kh < kl : kl < kh` the two comparisons become two branches in this loop)
        if ((up ? kh : kl) < (up ? kl : kh)) {
          key[lo] = kh;
          key[hi] = kl;
          const double vl = val[lo];
          val[lo] = val[hi];
          val[hi] = vl;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
  int kept_before = 0;   // running count of kept entries (uniform across the wave)
  const int64_t obase = asm_row_slot(i, k, sym, roff[i]);
  for (int e0 = 0; e0 < M; e0 += 64) {
    const int e = e0 + lane;
    int c = 0;
    double v = 0.0;
    const bool keep = e < M && asm_segment(key, val, e, M, (int)(i + row_base), sym, &c, &v);
    const unsigned long long mask = __ballot(keep);
    if (keep) {
      const int pos = kept_before + __popcll(mask & ((1ull << lane) - 1ull));
      col_out[obase + pos] = c;
      val_out[obase + pos] = v;
    }
    kept_before += __popcll(mask);
  }
  if (lane == 0) rowcnt[i] = kept_before;
}

// The same merge for rows of at most REG_CAP entries (forward + reverse) -- all of them unless the graph has popular vertices --: one
// entry per lane, sorted by a bitonic network over the wavefront in REGISTERS (keys only: the source lane rides in the key's free
// bits and the value is fetched from it afterwards), 4 KB of LDS per workgroup for the segment pass instead of the 64 KB
// the general kernel sizes for ROW_CAP entries (two workgroups per CU, 21 LDS passes with a barrier each: 0.24 ms of the 1.2 ms
// assembly at config 2).  Longer rows are left to merge_rows_kernel.
__global__ __launch_bounds__(256) void merge_rows_small_kernel(const int64_t* __restrict__ ind, const double* __restrict__ w, int64_t n, int kk,
                                                               int k, const int64_t* __restrict__ roff, const int* __restrict__ rsrc,
                                                               const unsigned short* __restrict__ rpos, const double* __restrict__ rw, int sym,
                                                               int* __restrict__ rowcnt, int* __restrict__ col_out,
                                                               double* __restrict__ val_out, int64_t row_base) {
#pragma clang fp contract(off)
  __shared__ unsigned long long s_key[4][64];
  __shared__ double s_val[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 4 + wave;
  if (i >= n) return;
  const int rc = sym == SYM_NONE ? 0 : (int)(roff[i + 1] - roff[i]);
  const int M = k + rc;
  if (asm_row_class(k, M) != ASM_ROW_REGISTER) return;
  unsigned long long kx = ~0ull;
  double v = 0.0;
  if (lane < k) {
    kx = asm_key((unsigned)ind[i * kk + lane], ASM_KIND_FORWARD, (unsigned)lane, (unsigned)lane);
    v = w[i * k + lane];
  } else if (lane < M) {
    const int64_t p = roff[i] + (lane - k);
    kx = asm_key((unsigned)rsrc[p], ASM_KIND_REVERSE, rpos[p], (unsigned)lane);
    v = rw[p];
  }
#pragma unroll
  for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      const unsigned lo = __shfl_xor((unsigned)(kx & 0xffffffffull), stride), hi = __shfl_xor((unsigned)(kx >> 32), stride);
      const unsigned long long o = ((unsigned long long)hi << 32) | lo;
      const bool up = (lane & size) == 0, lower = (lane & stride) == 0;
      const bool take_min = lower == up;
      kx = (take_min == (o < kx)) ? o : kx;
    }
  }
  {
    const int src = (int)asm_key_lane(kx);            // (padding keys point at lane 63: its value is 0 and never read)
    const int vlo = __shfl(__double2loint(v), src), vhi = __shfl(__double2hiint(v), src);
    s_key[wave][lane] = kx;
    s_val[wave][lane] = __hiloint2double(vhi, vlo);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int64_t obase = asm_row_slot(i, k, sym, roff[i]);
  int c = 0;
  double vv = 0.0;
  const bool keep = lane < M && asm_segment(s_key[wave], s_val[wave], lane, M, (int)(i + row_base), sym, &c, &vv);
  const unsigned long long mask = __ballot(keep);
  if (keep) {
    const int pos = __popcll(mask & ((1ull << lane) - 1ull));
    col_out[obase + pos] = c;
    val_out[obase + pos] = vv;
  }
  if (lane == 0) rowcnt[i] = __popcll(mask);
}

// rows of the scratch image of the row merges to their place in the CSR arrays (hub rows, rowcnt < 0, are written by
// merge_hub_kernel); four rows per workgroup
__global__ __launch_bounds__(256) void compact_rows_kernel(const int* __restrict__ rowcnt, const int64_t* __restrict__ roff, int64_t n, int k, int sym,
                                                           const int64_t* __restrict__ rowptr, const int* __restrict__ tcol,
                                                           const double* __restrict__ tval, int* __restrict__ col_out, double* __restrict__ val_out) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int cnt = rowcnt[i];
  if (cnt <= 0) return;
  const int64_t src = asm_row_slot(i, k, sym, roff[i]), dst = rowptr[i];
  for (int e = lane; e < cnt; e += 64) {
    col_out[dst + e] = tcol[src + e];
    val_out[dst + e] = tval[src + e];
  }
}

// hub vertices (more than ROW_CAP forward + reverse entries; high-dimensional data has them): one workgroup per hub,
// the same keys sorted by the same bitonic network in a global scratch of P entries (P = asm_hub_scratch(M)), then the
// same segment rule.  mode 0 sorts and counts, mode 1 writes from the scratch mode 0 left sorted.
__global__ __launch_bounds__(1024) void merge_hub_kernel(const int64_t* __restrict__ ind, const double* __restrict__ w, int kk, int k,
                                                         const int64_t* __restrict__ roff, const int* __restrict__ rsrc,
                                                         const unsigned short* __restrict__ rpos, const double* __restrict__ rw, int sym,
                                                         int mode, const int64_t* __restrict__ hub_row, const int64_t* __restrict__ hub_off,
                                                         unsigned long long* __restrict__ skey, double* __restrict__ sval,
                                                         int* __restrict__ hub_cnt, const int64_t* __restrict__ rowptr,
                                                         int* __restrict__ col_out, double* __restrict__ val_out, int64_t row_base) {
#pragma clang fp contract(off)
  __shared__ int wcnt[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t i = hub_row[blockIdx.x];
  const int64_t P = hub_off[blockIdx.x + 1] - hub_off[blockIdx.x];
  unsigned long long* key = skey + hub_off[blockIdx.x];
  double* val = sval + hub_off[blockIdx.x];
  const int64_t rc = roff[i + 1] - roff[i];
  const int64_t M = k + rc;
  if (!mode) {
    for (int64_t e = tid; e < P; e += 1024) {
      unsigned long long kx = ~0ull;
      double v = 0.0;
      if (e < k) {
        kx = asm_key((unsigned)ind[i * kk + e], ASM_KIND_FORWARD, (unsigned)e);
        v = w[i * k + e];
      } else if (e < M) {
        const int64_t p = roff[i] + (e - k);
        kx = asm_key((unsigned)rsrc[p], ASM_KIND_REVERSE, rpos[p]);
        v = rw[p];
      }
      key[e] = kx;
      val[e] = v;
    }
    __syncthreads();
    for (int64_t size = 2; size <= P; size <<= 1) {
      for (int64_t stride = size >> 1; stride > 0; stride >>= 1) {
        for (int64_t t = tid; t < P / 2; t += 1024) {
          const int64_t lo = (t / stride) * stride * 2 + (t % stride);
          const int64_t hi = lo + stride;
          const bool up = ((lo & size) == 0);
          const unsigned long long kl = key[lo], kh = key[hi];
          if (up ? (kh < kl) : (kl < kh)) {
            key[lo] = kh;
            key[hi] = kl;
            const double vl = val[lo];
            val[lo] = val[hi];
            val[hi] = vl;
          }
        }
        __syncthreads();
      }
    }
  }
  int kept_before = 0;   // uniform across the workgroup
  const int64_t obase = mode ? rowptr[i] : 0;
  for (int64_t e0 = 0; e0 < M; e0 += 1024) {
    const int64_t e = e0 + tid;
    int c = 0;
    double v = 0.0;
    const bool keep = e < M && asm_segment(key, val, e, M, (int)(i + row_base), sym, &c, &v);
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) wcnt[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
    for (int q = 0; q < 16; ++q) {
      if (q < wave) before += wcnt[q];
      total += wcnt[q];
    }
    if (keep && mode) {
      const int64_t pos = obase + kept_before + before + __popcll(mask & ((1ull << lane) - 1ull));
      col_out[pos] = c;
      val_out[pos] = v;
    }
    kept_before += total;
    __syncthreads();
  }
  if (!mode && tid == 0) hub_cnt[blockIdx.x] = kept_before;
}

// ---- host: one merge pipeline ----------------------------------------------------------------------------------------------------------
// The rows one call assembles, as the pipeline sees them: lists and weights on the device and the reverse entries (source row,
// position in the source's list, weight) grouped by row.  Counting and filling the reverse entries is the entry point's own -- from
// the lists themselves, or from the tuples a block received --; asm_rows_alloc and asm_reverse_offsets serve both.
struct AsmRows {
  int64_t n = 0;                   // rows
  int kk = 0, k = 0;               // stride of the lists, entries per list
  int64_t row_base = 0;            // global id of row 0: the diagonal of row i is column row_base + i
  int sym = SYM_NONE;
  const int64_t* ind = nullptr;    // [n][kk]
  double* w = nullptr;             // [n][k]
  int *rcnt = nullptr, *cursor = nullptr;     // [n] reverse entries of a row, and how many of them are filled in
  int64_t* roff = nullptr;         // [n + 1] their scan
  int* rsrc = nullptr;
  unsigned short* rpos = nullptr;
  double* rw = nullptr;
  int* flag = nullptr;             // [0]: an index out of range, [1]: hub rows among the merged
  int *h_rcnt = nullptr, *h_rowcnt = nullptr;    // page-locked: the counts the host scans (reverse entries, kept entries)
  std::vector<int64_t> h_roff;
};

static int asm_rows_alloc(GlxCall& call, AsmRows& r, int64_t n_rev) {
  hipStream_t st = call.stream();
  GLX_UP(call.alloc(&r.rcnt, (size_t)r.n + 1));
  GLX_UP(call.alloc(&r.cursor, (size_t)r.n + 1));
  GLX_UP(call.alloc(&r.roff, (size_t)r.n + 1));
  GLX_UP(call.alloc(&r.rsrc, (size_t)n_rev));
  GLX_UP(call.alloc(&r.rpos, (size_t)n_rev));
  GLX_UP(call.alloc(&r.rw, (size_t)n_rev));
  GLX_UP(call.alloc(&r.flag, 2));
  GLX_HIP(hipMemsetAsync(r.rcnt, 0, (r.n + 1) * 4, st));
  GLX_HIP(hipMemsetAsync(r.cursor, 0, (r.n + 1) * 4, st));
  GLX_HIP(hipMemsetAsync(r.flag, 0, 8, st));
  GLX_UP(call.stage(&r.h_rcnt, (size_t)2 * r.n + 16));
  r.h_rowcnt = r.h_rcnt + r.n;
  return GLX_OK;
}

// the counts come down, their scan goes up; `bad`: what to say if a kernel met an index out of range
static int asm_reverse_offsets(GlxCall& call, AsmRows& r, const char* bad) {
  hipStream_t st = call.stream();
  int flags[2] = {0, 0};
  GLX_HIP(hipMemcpyAsync(r.h_rcnt, r.rcnt, r.n * 4, hipMemcpyDeviceToHost, st));
  GLX_HIP(hipMemcpyAsync(flags, r.flag, 8, hipMemcpyDeviceToHost, st));
  GLX_HIP(hipStreamSynchronize(st));
  GLX_CHECK(!flags[0], GLX_EINVAL, "%s", bad);
  r.h_roff.assign(r.n + 1, 0);
  for (int64_t i = 0; i < r.n; ++i) r.h_roff[i + 1] = r.h_roff[i] + r.h_rcnt[i];
  return glx_upload(r.roff, r.h_roff.data(), (r.n + 1) * 8, st, __func__);
}

struct AsmMerge {                  // what the stages hand on
  int* rowcnt = nullptr;           // [n] kept entries of a row; -1: a hub, until its first pass has counted
  int* tcol = nullptr;             // scratch image of the one-pass merges (asm_row_slot)
  double* tval = nullptr;
  std::vector<int> big;            // rows above REG_CAP entries of a graph with k <= REG_CAP (popular vertices); their upload may
                                   // be a plain asynchronous copy: the list lives until asm_hub_count has synchronised the stream
  int64_t nh = 0;                  // hubs
  int64_t *hub_row = nullptr, *hub_off = nullptr;
  int* hub_cnt = nullptr;
  unsigned long long* skey = nullptr;
  double* sval = nullptr;
  int64_t* rowptr = nullptr;
};

// stage 1: every row that is not a hub merged into the scratch image -- the register kernel when the lists are short enough for
// it, the wavefront kernel for all rows otherwise and for the rows the register kernel leaves (the host has the counts)
static int asm_merge_launch(GlxCall& call, const AsmRows& r, int64_t image, AsmMerge& m) {
  hipStream_t st = call.stream();
  const size_t shm = (size_t)4 * ROW_CAP * 16;
  GLX_HIP(hipFuncSetAttribute((const void*)merge_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
  GLX_UP(call.alloc(&m.rowcnt, (size_t)r.n + 1));
  GLX_UP(call.alloc(&m.tcol, (size_t)image));
  GLX_UP(call.alloc(&m.tval, (size_t)image));
  const unsigned gr = (unsigned)((r.n + 3) / 4);
  if (r.k > REG_CAP) {
    hipLaunchKernelGGL(merge_rows_kernel, dim3(gr), dim3(256), shm, st, r.ind, (const double*)r.w, r.n, r.kk, r.k, (const int64_t*)r.roff,
                       (const int*)r.rsrc, (const unsigned short*)r.rpos, (const double*)r.rw, r.sym, m.rowcnt, m.tcol, m.tval, r.flag + 1,
                       r.row_base, (const int*)nullptr, 0);
    GLX_HIP(hipGetLastError());
    return GLX_OK;
  }
  hipLaunchKernelGGL(merge_rows_small_kernel, dim3(gr), dim3(256), 0, st, r.ind, (const double*)r.w, r.n, r.kk, r.k, (const int64_t*)r.roff,
                     (const int*)r.rsrc, (const unsigned short*)r.rpos, (const double*)r.rw, r.sym, m.rowcnt, m.tcol, m.tval, r.row_base);
  GLX_HIP(hipGetLastError());
  if (r.sym != SYM_NONE)
    for (int64_t i = 0; i < r.n; ++i)
      if (asm_row_class(r.k, r.k + (int64_t)r.h_rcnt[i]) != ASM_ROW_REGISTER) m.big.push_back((int)i);
  if (m.big.empty()) return GLX_OK;
  int* d_big = nullptr;
  GLX_UP(call.put(&d_big, (const int*)m.big.data(), m.big.size(), __func__));
  hipLaunchKernelGGL(merge_rows_kernel, dim3((unsigned)((m.big.size() + 3) / 4)), dim3(256), shm, st, r.ind, (const double*)r.w, r.n, r.kk, r.k,
                     (const int64_t*)r.roff, (const int*)r.rsrc, (const unsigned short*)r.rpos, (const double*)r.rw, r.sym, m.rowcnt, m.tcol,
                     m.tval, r.flag + 1, r.row_base, (const int*)d_big, (int)m.big.size());
  GLX_HIP(hipGetLastError());
  return GLX_OK;
}

// stage 2: the rows' counts come down; the hubs among them (marked by the wavefront kernel) get a workgroup each, which sorts in a
// global scratch and counts (merge_hub_kernel, first pass)
static int asm_hub_count(GlxCall& call, const AsmRows& r, AsmMerge& m) {
  hipStream_t st = call.stream();
  int flags[2] = {0, 0};
  GLX_HIP(hipMemcpyAsync(r.h_rowcnt, m.rowcnt, r.n * 4, hipMemcpyDeviceToHost, st));
  GLX_HIP(hipMemcpyAsync(flags, r.flag, 8, hipMemcpyDeviceToHost, st));
  GLX_HIP(hipStreamSynchronize(st));
  if (!flags[1]) return GLX_OK;
  std::vector<int64_t> hrow, hoff(1, 0);
  for (int64_t i = 0; i < r.n; ++i) {
    if (r.h_rowcnt[i] >= 0) continue;
    hrow.push_back(i);
    hoff.push_back(hoff.back() + asm_hub_scratch(r.k + (r.h_roff[i + 1] - r.h_roff[i])));
  }
  m.nh = (int64_t)hrow.size();
  GLX_UP(call.put(&m.hub_row, (const int64_t*)hrow.data(), (size_t)m.nh, __func__));
  GLX_UP(call.put(&m.hub_off, (const int64_t*)hoff.data(), (size_t)m.nh + 1, __func__));
  GLX_UP(call.alloc(&m.hub_cnt, (size_t)m.nh));
  GLX_UP(call.alloc(&m.skey, (size_t)hoff.back()));
  GLX_UP(call.alloc(&m.sval, (size_t)hoff.back()));
  hipLaunchKernelGGL(merge_hub_kernel, dim3((unsigned)m.nh), dim3(1024), 0, st, r.ind, (const double*)r.w, r.kk, r.k, (const int64_t*)r.roff,
                     (const int*)r.rsrc, (const unsigned short*)r.rpos, (const double*)r.rw, r.sym, 0, (const int64_t*)m.hub_row,
                     (const int64_t*)m.hub_off, m.skey, m.sval, m.hub_cnt, (const int64_t*)nullptr, (int*)nullptr, (double*)nullptr, r.row_base);
  GLX_HIP(hipGetLastError());
  std::vector<int> hcnt(m.nh);
  GLX_HIP(hipMemcpyAsync(hcnt.data(), m.hub_cnt, m.nh * 4, hipMemcpyDeviceToHost, st));
  GLX_HIP(hipStreamSynchronize(st));
  for (int64_t h = 0; h < m.nh; ++h) r.h_rowcnt[hrow[h]] = hcnt[h];
  return GLX_OK;
}

// stage 3: row pointers from the counts; cap < 0: the caller has no limit of its own
static int asm_row_pointers(GlxCall& call, const AsmRows& r, int64_t cap, const char* who, AsmMerge& m, std::vector<int64_t>& rp) {
  rp.assign(r.n + 1, 0);
  for (int64_t i = 0; i < r.n; ++i) rp[i + 1] = rp[i] + r.h_rowcnt[i];
  const int64_t nnz = rp[r.n];
  GLX_CHECK(nnz < (1ll << 31), GLX_EUNSUPPORTED, "%s: nnz %lld does not fit the int32 CSR of the reference", who, (long long)nnz);
  GLX_CHECK(cap < 0 || nnz <= cap, GLX_EINVAL, "%s: %lld entries, room for %lld", who, (long long)nnz, (long long)cap);
  return call.put(&m.rowptr, (const int64_t*)rp.data(), (size_t)r.n + 1, who);
}

// stages 4 and 5: the rows of the scratch image move to their place, the hubs write theirs from the scratch their first pass sorted
static int asm_compact(GlxCall& call, const AsmRows& r, const AsmMerge& m, int32_t* col, double* val) {
  hipLaunchKernelGGL(compact_rows_kernel, dim3((unsigned)((r.n + 3) / 4)), dim3(256), 0, call.stream(), (const int*)m.rowcnt, (const int64_t*)r.roff,
                     r.n, r.k, r.sym, (const int64_t*)m.rowptr, (const int*)m.tcol, (const double*)m.tval, col, val);
  GLX_HIP(hipGetLastError());
  return GLX_OK;
}

static int asm_hub_write(GlxCall& call, const AsmRows& r, const AsmMerge& m, int32_t* col, double* val) {
  if (!m.nh) return GLX_OK;
  hipLaunchKernelGGL(merge_hub_kernel, dim3((unsigned)m.nh), dim3(1024), 0, call.stream(), r.ind, (const double*)r.w, r.kk, r.k,
                     (const int64_t*)r.roff, (const int*)r.rsrc, (const unsigned short*)r.rpos, (const double*)r.rw, r.sym, 1,
                     (const int64_t*)m.hub_row, (const int64_t*)m.hub_off, m.skey, m.sval, m.hub_cnt, (const int64_t*)m.rowptr, col, val,
                     r.row_base);
  GLX_HIP(hipGetLastError());
  return GLX_OK;
}

// Rows whose reverse entries are in place -> CSR: rp (n + 1 row pointers, the caller's: their upload may still be in flight) and the
// entries at *col / *val on the device -- the caller's destination, or where null pooled blocks of the call -- when the stream has
// drained.  image: entries of the scratch image (every row's candidates); cap, who: asm_row_pointers.
static int asm_merge_rows(GlxCall& call, const AsmRows& r, int64_t image, int64_t cap, const char* who, int32_t** col, double** val,
                          std::vector<int64_t>& rp) {
  AsmMerge m;
  GLX_UP(asm_merge_launch(call, r, image, m));
  GLX_UP(asm_hub_count(call, r, m));
  GLX_UP(asm_row_pointers(call, r, cap, who, m, rp));
  if (!*col) {
    GLX_UP(call.alloc(col, (size_t)rp[r.n]));
    GLX_UP(call.alloc(val, (size_t)rp[r.n]));
  }
  GLX_UP(asm_compact(call, r, m, *col, *val));
  return asm_hub_write(call, r, m, *col, *val);
}

// ---- the whole matrix ------------------------------------------------------------------------------------------------------------------
// the host arrays glx_knn_to_csr allocates (glx_free releases them): freed here unless the call succeeds
struct HostCsr {
  int32_t *rowptr = nullptr, *col = nullptr;
  double* val = nullptr;
  ~HostCsr() { free(rowptr); free(col); free(val); }
  void release() { rowptr = col = nullptr; val = nullptr; }
};

// cap < 0: the CSR arrays are allocated here (malloc; glx_free releases them); cap >= 0: *rowptr_out / *col_out / *val_out
// are the caller's buffers with room for n + 1 row pointers and cap entries
static int knn_to_csr_impl(const int64_t* ind, const double* dist, const double* weights, int64_t n, int kk, int k, int kernel,
                           int sym, int64_t cap, int32_t** rowptr_out, int32_t** col_out, double** val_out, int64_t* nnz_out, int device,
                           const glx_knn_result* res = nullptr) {
  // res: the lists are the device-resident ones of a search result (borrowed: glx_knn_result_to_csr), not blocks of this call
  GLX_CHECK(rowptr_out && col_out && val_out && nnz_out, GLX_EINVAL, "glx_knn_to_csr: null argument");
  GLX_CHECK(ind || res, GLX_EINVAL, "glx_knn_to_csr: null neighbour indices");
  GLX_CHECK(n >= 1 && k >= 1 && kk >= k, GLX_EINVAL, "glx_knn_to_csr: need n >= 1 and 1 <= k <= columns (n=%lld k=%d columns=%d)", (long long)n, k, kk);
  GLX_CHECK(kernel >= K_GIVEN && kernel <= K_SINGULAR, GLX_EINVAL, "glx_knn_to_csr: bad kernel id %d", kernel);
  GLX_CHECK(sym >= SYM_NONE && sym <= SYM_SYMGAUSS, GLX_EINVAL, "glx_knn_to_csr: bad symmetrisation id %d", sym);
  GLX_CHECK(kernel == K_GIVEN ? weights != nullptr : (kernel == K_UNIFORM || dist != nullptr || res), GLX_EINVAL, "glx_knn_to_csr: missing weights / distances");
  GLX_CHECK(n < (1ll << 31) && n * k < (1ll << 31), GLX_EUNSUPPORTED, "glx_knn_to_csr: n*k must fit int32");
  GLX_CHECK(k <= 65535, GLX_EUNSUPPORTED, "glx_knn_to_csr: at most 65535 neighbours per row (k=%d)", k);
  const bool own = cap < 0;
  if (own) { *rowptr_out = nullptr; *col_out = nullptr; *val_out = nullptr; }
  *nnz_out = 0;
  GlxCall call;
  GLX_UP(call.begin(device));
  hipStream_t st = call.stream();
  const int64_t ne = n * k;
  AsmRows r;
  r.n = n; r.kk = kk; r.k = k; r.sym = sym;
  int64_t* d_ind = res ? res->ind : nullptr;
  double *d_dist = res ? res->dist : nullptr, *d_given = nullptr;
  if (!res) GLX_UP(call.put(&d_ind, ind, (size_t)n * kk, __func__));
  if (!res && dist) GLX_UP(call.put(&d_dist, dist, (size_t)n * kk, __func__));
  if (kernel == K_GIVEN) GLX_UP(call.put(&d_given, weights, (size_t)ne, __func__));
  r.ind = d_ind;
  GLX_UP(call.alloc(&r.w, (size_t)ne));
  GLX_UP(asm_rows_alloc(call, r, ne));
  const unsigned ge = (unsigned)((ne + 255) / 256);
  hipLaunchKernelGGL(knn_weights_kernel, dim3(ge), dim3(256), 0, st, r.ind, (const double*)d_dist, n, kk, k, kernel, (const double*)d_given, r.w);
  GLX_HIP(hipGetLastError());
  hipLaunchKernelGGL(count_reverse_kernel, dim3(ge), dim3(256), 0, st, r.ind, n, kk, k, r.rcnt, r.flag);
  GLX_HIP(hipGetLastError());
  GLX_UP(asm_reverse_offsets(call, r, "glx_knn_to_csr: neighbour index out of range"));
  hipLaunchKernelGGL(fill_reverse_kernel, dim3(ge), dim3(256), 0, st, r.ind, (const double*)r.w, n, kk, k, (const int64_t*)r.roff, r.cursor, r.rsrc,
                     r.rpos, r.rw);
  GLX_HIP(hipGetLastError());
  // Page-locked destinations (the arrays _hip hands in) are written by the compaction kernels themselves through their device
  // view: no device copy of the result, no copy-engine transfer behind it (whose first use after fresh allocations cost 8 ms).
  void *v_col = nullptr, *v_val = nullptr;
  const bool direct = !own && hipHostGetDevicePointer(&v_col, *col_out, 0) == hipSuccess && v_col &&
                      hipHostGetDevicePointer(&v_val, *val_out, 0) == hipSuccess && v_val;
  (void)hipGetLastError();
  int32_t* d_col = direct ? (int32_t*)v_col : nullptr;
  double* d_val = direct ? (double*)v_val : nullptr;
  std::vector<int64_t> rp;
  GLX_UP(asm_merge_rows(call, r, 2 * ne, cap, own ? "glx_knn_to_csr" : "glx_knn_to_csr_into", &d_col, &d_val, rp));
  const int64_t nnz = rp[n];
  HostCsr mine;
  if (own) {
    mine.rowptr = (int32_t*)malloc((n + 1) * 4);
    mine.col = (int32_t*)malloc(std::max<size_t>(nnz * 4, 4));
    mine.val = (double*)malloc(std::max<size_t>(nnz * 8, 8));
    GLX_CHECK(mine.rowptr && mine.col && mine.val, GLX_ENOMEM, "glx_knn_to_csr: host allocation failed");
  }
  int32_t *h_rp = own ? mine.rowptr : *rowptr_out, *h_col = own ? mine.col : *col_out;
  double* h_val = own ? mine.val : *val_out;
  for (int64_t i = 0; i <= n; ++i) h_rp[i] = (int32_t)rp[i];
  if (!direct) {       // (into memory that may be ordinary: through the checked download)
    GLX_UP(glx_download(h_col, d_col, nnz * 4, st, "glx_knn_to_csr"));
    GLX_UP(glx_download(h_val, d_val, nnz * 8, st, "glx_knn_to_csr"));
  }
  GLX_HIP(hipStreamSynchronize(st));
  *rowptr_out = h_rp;
  *col_out = h_col;
  *val_out = h_val;
  *nnz_out = nnz;
  mine.release();
  return GLX_OK;
}

extern "C" int glx_knn_to_csr(const int64_t* ind, const double* dist, const double* weights, int64_t n, int kk, int k, int kernel,
                              int sym, int32_t** rowptr_out, int32_t** col_out, double** val_out, int64_t* nnz_out, int device) {
  return knn_to_csr_impl(ind, dist, weights, n, kk, k, kernel, sym, -1, rowptr_out, col_out, val_out, nnz_out, device);
}

// the same with the CSR written into the caller's arrays (rowptr: n + 1, col / val: cap entries; 2 n k always suffices,
// n k without symmetrisation): page-locked ones make the copy back run at PCIe speed and save the copy out of
// library-owned memory
extern "C" int glx_knn_to_csr_into(const int64_t* ind, const double* dist, const double* weights, int64_t n, int kk, int k, int kernel,
                                   int sym, int64_t cap, int32_t* rowptr, int32_t* col, double* val, int64_t* nnz_out, int device) {
  GLX_CHECK(cap >= 0 && rowptr && col && val, GLX_EINVAL, "glx_knn_to_csr_into: null buffer or negative capacity");
  return knn_to_csr_impl(ind, dist, weights, n, kk, k, kernel, sym, cap, &rowptr, &col, &val, nnz_out, device);
}

// the weight matrix of a search result (glx_knn_search): the lists never leave the device.  k <= the result's columns; weights
// (n, k) only for kernel = given.  Caller's buffers as in glx_knn_to_csr_into.
extern "C" int glx_knn_result_to_csr(const glx_knn_result* res, int k, int kernel, int sym, const double* weights, int64_t cap,
                                     int32_t* rowptr, int32_t* col, double* val, int64_t* nnz_out) {
  GLX_CHECK(res && res->ind && res->dist, GLX_EINVAL, "glx_knn_result_to_csr: empty result");
  GLX_CHECK(rowptr && col && val && cap >= 0, GLX_EINVAL, "glx_knn_result_to_csr: null buffer");
  return knn_to_csr_impl(nullptr, nullptr, weights, res->n, res->k, k, kernel, sym, cap, &rowptr, &col, &val, nnz_out, res->device, res);
}

// ---- a BLOCK of rows of the weight matrix (sharded build, SURVEY.md 8e "symmetrisation by owner rank") ----------------------
// Rows [row_base, row_base + m) of weightmatrix.knn's result from the block's own lists (ind_own / w_own: m x k, weights given)
// and the reverse entries the other rows' owners sent: (rev_row = j in the block, rev_src = i, rev_pos = position of j in row
// i's list, rev_w = w_ij).  From there on it is asm_merge_rows, as for the whole matrix -- forward and reverse entries of a row
// sorted by (column, kind, position), duplicates summed in list order, the symmetrisation rule per column, diagonal and zeros
// dropped -- so the rows are bit-identical to the rows of the whole matrix.  Columns are global ids (< n_cols).
__global__ void count_rev_rows_kernel(const int64_t* __restrict__ rev_row, int64_t n_rev, int64_t row_base, int64_t m, int* __restrict__ rcnt,
                                      int* __restrict__ bad) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_rev) return;
  const int64_t j = rev_row[e] - row_base;
  if (j < 0 || j >= m) { *bad = 1; return; }
  atomicAdd(&rcnt[j], 1);
}

__global__ void fill_rev_rows_kernel(const int64_t* __restrict__ rev_row, const int64_t* __restrict__ rev_src, const int64_t* __restrict__ rev_pos,
                                     const double* __restrict__ rev_w, int64_t n_rev, int64_t row_base, const int64_t* __restrict__ roff,
                                     int* __restrict__ cursor, int* __restrict__ rsrc, unsigned short* __restrict__ rpos, double* __restrict__ rw) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_rev) return;
  const int64_t j = rev_row[e] - row_base;
  const int64_t pos = roff[j] + atomicAdd(&cursor[j], 1);
  rsrc[pos] = (int)rev_src[e];
  rpos[pos] = (unsigned short)rev_pos[e];
  rw[pos] = rev_w[e];
}

__global__ void check_cols_kernel(const int64_t* __restrict__ ind, int64_t total, int64_t n_cols, int* __restrict__ bad) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < total && (ind[e] < 0 || ind[e] >= n_cols)) *bad = 1;
}

extern "C" int glx_knn_rows_to_csr(const int64_t* ind_own, const double* w_own, int64_t m, int k, int64_t n_cols, int64_t row_base,
                                   const int64_t* rev_row, const int64_t* rev_src, const int64_t* rev_pos, const double* rev_w, int64_t n_rev,
                                   int sym, int64_t cap, int32_t* rowptr_out, int32_t* col_out, double* val_out, int64_t* nnz_out, int device) {
  GLX_CHECK(ind_own && w_own && rowptr_out && col_out && val_out && nnz_out, GLX_EINVAL, "glx_knn_rows_to_csr: null argument");
  GLX_CHECK(m >= 0 && k >= 1 && n_cols >= 1 && row_base >= 0 && row_base + m <= n_cols, GLX_EINVAL, "glx_knn_rows_to_csr: bad sizes");
  GLX_CHECK(n_rev >= 0 && (n_rev == 0 || (rev_row && rev_src && rev_pos && rev_w)), GLX_EINVAL, "glx_knn_rows_to_csr: null reverse arrays");
  GLX_CHECK(sym == SYM_NONE || sym == SYM_MEAN || sym == SYM_MAX, GLX_EINVAL, "glx_knn_rows_to_csr: symmetrisation %d needs other rows' data", sym);
  GLX_CHECK(n_cols < (1ll << 31) && m * k < (1ll << 31) && n_rev < (1ll << 31), GLX_EUNSUPPORTED, "glx_knn_rows_to_csr: sizes must fit int32");
  GLX_CHECK(k <= 65535, GLX_EUNSUPPORTED, "glx_knn_rows_to_csr: at most 65535 neighbours per row (k=%d)", k);
  GLX_CHECK(cap >= 0, GLX_EINVAL, "glx_knn_rows_to_csr: negative capacity");
  *nnz_out = 0;
  rowptr_out[0] = 0;
  if (m == 0) return GLX_OK;
  GlxCall call;
  GLX_UP(call.begin(device));
  hipStream_t st = call.stream();
  const int64_t ne = m * k, nr = sym == SYM_NONE ? 0 : n_rev;
  AsmRows r;
  r.n = m; r.kk = k; r.k = k; r.row_base = row_base; r.sym = sym;
  int64_t* d_ind = nullptr;
  GLX_UP(call.put(&d_ind, ind_own, (size_t)ne, __func__));
  GLX_UP(call.put(&r.w, w_own, (size_t)ne, __func__));
  r.ind = d_ind;
  GLX_UP(asm_rows_alloc(call, r, nr));
  hipLaunchKernelGGL(check_cols_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, r.ind, ne, n_cols, r.flag);
  int64_t *d_rrow = nullptr, *d_rsrc = nullptr, *d_rpos = nullptr;      // the received tuples as they came
  double* d_rw = nullptr;
  const unsigned gv = (unsigned)((nr + 255) / 256);
  if (nr > 0) {
    GLX_UP(call.put(&d_rrow, rev_row, (size_t)nr, __func__));
    GLX_UP(call.put(&d_rsrc, rev_src, (size_t)nr, __func__));
    GLX_UP(call.put(&d_rpos, rev_pos, (size_t)nr, __func__));
    GLX_UP(call.put(&d_rw, rev_w, (size_t)nr, __func__));
    hipLaunchKernelGGL(count_rev_rows_kernel, dim3(gv), dim3(256), 0, st, (const int64_t*)d_rrow, nr, row_base, m, r.rcnt, r.flag);
    hipLaunchKernelGGL(check_cols_kernel, dim3(gv), dim3(256), 0, st, (const int64_t*)d_rsrc, nr, n_cols, r.flag);
  }
  GLX_HIP(hipGetLastError());
  GLX_UP(asm_reverse_offsets(call, r, "glx_knn_rows_to_csr: index out of range (a neighbour id, or a reverse entry outside the block)"));
  if (nr > 0) {
    hipLaunchKernelGGL(fill_rev_rows_kernel, dim3(gv), dim3(256), 0, st, (const int64_t*)d_rrow, (const int64_t*)d_rsrc, (const int64_t*)d_rpos,
                       (const double*)d_rw, nr, row_base, (const int64_t*)r.roff, r.cursor, r.rsrc, r.rpos, r.rw);
    GLX_HIP(hipGetLastError());
  }
  int32_t* d_col = nullptr;
  double* d_val = nullptr;
  std::vector<int64_t> rp;
  GLX_UP(asm_merge_rows(call, r, ne + n_rev, cap, "glx_knn_rows_to_csr", &d_col, &d_val, rp));
  const int64_t nnz = rp[m];
  for (int64_t i = 0; i <= m; ++i) rowptr_out[i] = (int32_t)rp[i];
  GLX_UP(glx_download(col_out, d_col, nnz * 4, st, __func__));
  GLX_UP(glx_download(val_out, d_val, nnz * 8, st, __func__));
  GLX_HIP(hipStreamSynchronize(st));
  *nnz_out = nnz;
  return GLX_OK;
}
