/* glx_experimental.h -- the entry points of libglx.so that are NOT part of the drop-in boundary (include/glx.h): host helpers of the
 * Python boundary, diagnostics and plan overrides for tests and A/B measurements, the device-pointer calls of the torch fallback
 * engine of the multi-GPU path, and the stepwise form of the distributed sweep with which multi-rank jobs are tested on ONE GPU.
 * Same conventions as glx.h (status codes, glx_last_error, borrowed host pointers); no stability promise. */
#ifndef GLX_EXPERIMENTAL_H
#define GLX_EXPERIMENTAL_H
#include "glx.h"
#ifdef __cplusplus
extern "C" {
#endif

int glx_version(void);
int glx_device_synchronize(void);
/* sweep kernels enqueued so far by a prepared sweep (the bench derives a per-launch time from it) */
int glx_sweep_launches(const glx_sweep* s, int64_t* sweep_kernel_launches);
int glx_sweep_groups_launches(const glx_sweep_groups* s, int64_t* sweep_kernel_launches);

/* Host helpers of ssl.poisson's operator set-up (graphlearning/ssl.py:634-635, 642) for a W that is symmetric bit for bit:
 * row sums in stored order (= scipy's W * ones), and the rows of P = D^-1 W^T written down without a transpose -- row i of W
 * scaled by scale[i] with its entries in reverse order, the arrays scipy's `D * W.transpose()` yields.  No device involved. */
int glx_host_row_sums(int64_t n, const int32_t* rowptr, const double* val, double* sum_out);
int glx_host_reverse_scale_rows(int64_t n, const int32_t* rowptr, const int32_t* col, const double* val,
                                const double* scale, int32_t* col_out, double* val_out);
/* Host: the nonzero rows of -L[:, cols] * F from the CSC image (cptr, crow, cval) of a canonical L -- ssl.laplace's right-hand side,
 * reference ssl.py:1236, a row's terms added in ascending column order from 0 as scipy's csr_matvecs does --, without the rows listed
 * in cols, every row times row_scale[row] when given (M*b, ssl.py:1249).  rows_out ascending, vals_out (count, k); cap = room in both.
 * *count_out = -1 (and GLX_OK): cols has duplicates, use the literal expression. */
int glx_host_neg_columns_rows(int64_t n, const int32_t* cptr, const int32_t* crow, const double* cval, int64_t m, const int64_t* cols,
                              const double* F, int k, const double* row_scale, int64_t cap, int32_t* rows_out, double* vals_out,
                              int64_t* count_out);

/* host helpers of the sharded build: the library's locality order (perm_out[new] = old, the breadth-first pass glx_graph uses for
 * square operators) of an n-row pattern restricted to the columns [col_lo, col_lo + n) -- a rank orders its own rows by their links
 * among themselves --, and the rows of a CSR matrix in another order (row i of the result = row perm[i], entry order kept). */
int glx_host_locality_order(int64_t n, const int32_t* rowptr, const int32_t* col, int64_t col_lo, int32_t* perm_out);
int glx_host_permute_rows(int64_t n, const int32_t* rowptr, const int32_t* col, const double* val, const int64_t* perm,
                          int32_t* rowptr_out, int32_t* col_out, double* val_out);

/* 128-bit content fingerprint of `bytes` bytes (chunks hashed on a few host threads, then combined): what the learners key
 * their device-resident operators by, so that a weight matrix edited in place between two fits is seen as a new graph. */
int glx_host_fingerprint(const void* data, size_t bytes, uint64_t seed, uint64_t out[2]);

/* info[0]=n_rows,[1]=n_cols,[2]=nnz,[3]=stored entries incl. padding,[4]=slices,[5]=rows per slice,[6]=max row nnz,[7]=1 if renumbered */
int glx_graph_info(const glx_graph* g, int64_t info[8]);
/* the internal vertex order: perm_out[new] = caller's row (n_rows entries; the identity when the operator
 * was not renumbered).  Forces the order to be computed if it has not been yet. */
int glx_graph_order(glx_graph* g, int32_t* perm_out);

/* ---- device-pointer entry points: rank-local sweeps of the vertex-partitioned solver -------
 * Buffers are DEVICE memory in the vertex-record layout (torch tensors' data_ptr()); `stream`
 * is a hipStream_t; nothing synchronises.  Record layout: `ld` elements per vertex, columns
 * 0..C-1, zero padding to a multiple of 4, then (has_w) the fp64 stop value at byte `woff`.
 * out = {ld, woff, record bytes, lanes per row, 4-wide column vectors, element size}. */
int glx_record_layout(int C, int dtype, int has_w, int32_t out[6]);
int glx_graph_slots(glx_graph* P, int C, int has_w, int64_t* nslots);
/* flags[slot] = 1 where the slot's row has a nonzero bias record (sparse Db: ssl.py:620-622) */
int glx_bias_flags_dev(glx_graph* P, int C, int has_w, const void* bias_rec, uint8_t* flags, void* stream);
/* one sweep xout[0:n_rows] = bias + P xin[0:n_cols]; err_next (64 x uint64, caller-zeroed) receives
 * max |deg*w - vinf| as fp64 bit patterns when non-NULL (the rank-local part of ssl.py:667) */
int glx_sweep_step_dev(glx_graph* P, int C, int has_w, const void* xin, void* xout, const void* bias_rec,
                       const uint8_t* slot_flags, const double* deg, const double* vinf, void* err_next,
                       void* stream);
int glx_pack_records_dev(const void* dense, void* rec, int64_t n, int C, int dtype, int has_w, const double* w,
                         void* stream);
int glx_unpack_records_dev(const void* rec, void* dense, int64_t n, int C, int dtype, int has_w, void* stream);

/* Dense vector kernels of utils.conjgrad (graphlearning/utils.py:483-532) on device records, for the vertex-partitioned
 * conjugate-gradient solve (dist.py: cg_distributed): out[c] = sum_i a[i,c] b[i,c] in fp64 with a fixed order inside the
 * rank (partial: device scratch of glx_rec_dots_scratch(n, C) doubles); x += alpha p, r -= alpha Ap; p = r + beta p --
 * alpha, beta: device fp64[C].  The ranks add their column sums with one all-reduce each (tolerance mode). */
int64_t glx_rec_dots_scratch(int64_t n, int C);
int glx_rec_dots_dev(const void* a, const void* b, int64_t n, int C, int dtype, int has_w, double* partial, double* out, void* stream);
int glx_rec_axpy2_dev(void* x, void* r, const void* p, const void* Ap, const double* alpha, int64_t n, int C, int dtype, int has_w,
                      void* stream);
int glx_rec_xpby_dev(void* p, const void* r, const double* beta, int64_t n, int C, int dtype, int has_w, void* stream);

int glx_dist_comm_info(const glx_comm* c, int32_t info[4]);   /* rank, nranks, device, 1 if it has an RCCL communicator */

int glx_dist_sweep_stats(const glx_dist_sweep* s, int64_t out[4]);      /* sweeps run, exchanges enqueued, graphs, 1 if it exchanges */
/* what the object decided: out[0] 1 if it exchanges, [1] exchanging sweeps captured (1) / eager (0) / undecided (-1),
 * [2] self-test 0 not run / 1 passed / 2 failed, [3] exchange on a second stream beside the interior rows, [4] one
 * launch per sweep (GLX_DIST_FUSE), [5] boundary rows scattered into the send buffer by the SpMM (no pack kernel),
 * [6] records sent per sweep, [7] halo records */
int glx_dist_sweep_info(const glx_dist_sweep* s, int64_t out[8]);
/* device microseconds of the rank-local pieces of a sweep, each timed alone over `reps` launches: [0] boundary rows
 * (incl. the scatter), [1] interior rows, [2] the stand-alone pack kernel, [3] boundary + interior back to back */
int glx_dist_sweep_time_parts(glx_dist_sweep* s, int reps, float us_out[4]);

/* the same pieces one at a time with the transport left to the caller (eager, synchronous): multi-rank tests on one
 * GPU move the packed records between ranks through a host-side backend */
int glx_dist_sweep_begin(glx_dist_sweep* s);                                    /* state <- initial records; packs them */
int glx_dist_sweep_boundary(glx_dist_sweep* s, int want_err);                   /* boundary rows of the next iterate; packs them */
int glx_dist_sweep_get_send(glx_dist_sweep* s, void* host_out);                 /* the packed records (sum of send_counts) */
int glx_dist_sweep_put_halo(glx_dist_sweep* s, const void* host_in, int next);  /* received records -> halo of the current / next iterate */
int glx_dist_sweep_interior(glx_dist_sweep* s, int want_err, double* err_local_out);   /* interior rows; next becomes current */

/* all n rows in the caller's order, the cells formed by the library: ncells (<= 4096; 0 / 1 = plain all-pairs search) evenly
 * spaced rows serve as centres, every row joins the nearest, the rows are reordered by cell on the device and searched with the
 * pruning of glx_knn_cells_range.  Indices and output rows are the caller's, equal distances go to the lower caller index: the
 * lists of glx_knn_bruteforce bit for bit.  ncells < -1: the rows reordered by -ncells chained cells on the device, then ALL PAIRS
 * (no pruning: a wavefront's queries share a corner of feature space, which is worth 10-14 % of the search on clustered data
 * below the size where pruning pays, and nothing elsewhere).  glx_knn_search hands that order out with its result. */
int glx_knn_clustered(const double* X, int64_t n, int d, int k, int ncells, int64_t* ind_out, double* dist_out, int device);
/* Plan overrides of the calling thread's searches (tests and A/B measurements; NULL or all-default values = the library decides):
 * filter 0 auto | 1 split-bf16 | 2 fp32 operands; lists 0 auto | 1 short | 2 long (one list holds all k neighbours of a query);
 * nsplit 0 auto | 1..8 ref ranges per query block (1..32 for the wide search, k > 60, never fewer than k candidates); concat -1 auto | 0 blocks of 16 features | 1 concatenated split operands
 * (d <= 21) | 2 with the norm folded in (d <= 20).  Every plan returns the same exact lists. */
typedef struct { int filter, lists, nsplit, concat; } glx_knn_options;
int glx_knn_set_options(const glx_knn_options* opt);

/* 0: the device work-buffer pool and the idle work sets (streams, events, staging) are bypassed -- every buffer comes from hipMalloc and
 * goes back with hipFree; 1 (default): size-class free lists in front of the runtime.  Results are identical either way
 * (tests/test_gpu_switches.py); the switch exists for ablation runs of the randomised soak. */
int glx_pool_set_enabled(int enabled);
/* debugging aid: every work buffer the pool hands out is first filled with `byte` (0 .. 255; -1 = off, the default), so that a kernel reading
 * a buffer before anything wrote it computes from the pattern instead of from what an earlier call left there */
int glx_pool_set_poison(int byte);
/* debugging aid of the search: flags bit 0 = after the upload of a search's features read the device copy back (by the copy engine and through a
 * kernel) and compare it with the caller's array; counters: uploads checked, uploads whose engine / kernel read-back differed, bytes differing */
int glx_debug_set(int flags);
/* how uploads of 128 KB or more travel: 0 (default) through the library's page-locked staging area and CHECKED (word sums of the source and of
 * what arrived; a difference is described on stderr and the upload repeated), 1 staged without the check, 2 hipMemcpyAsync straight from the caller's
 * pageable memory as rounds 1-5 did -- the path on which round 6 found holes of 256 zero bytes.  For A/B runs. */
int glx_upload_set_mode(int mode);
/* the checked uploads of this process (csrc/glx_internal.h glx_upload): uploads checked, sums that differed, uploads that arrived intact on
 * a repeat, uploads given up */
int glx_upload_stats(unsigned long long out[4]);
int glx_debug_counters(unsigned long long out[4]);

/* out[i] = exp(x[i]) correctly rounded (csrc/exp_cr.h: the exponential of the Gaussian weights), host arrays; a test hook */
int glx_exp_cr(const double* x, double* out, int64_t n, int device);

int glx_knn_stats(double stats[16]);  /* of the calling thread's last search: [0] tile-kernel ms, [1] re-rank ms, [2] fallback rows, [3] total device ms,
                                        [4] fallback ms, [5] padded feature count, [6] ref ranges, [7] list length (negative: bf16 filter),
                                        [8] rows the short lists could not accept when the search was repeated with long ones (else 0);
                                        [9] concatenated operands (d <= 21): 0 no, 1 yes, 2 with the norm folded in (d <= 20),
                                        [10] tile stride of the sample the seeding pre-pass looked at (0: no pre-pass; tile-kernel ms
                                        include it and the cell passes), [11] share of the (query block, ref tile) pairs visited and
                                        [12] number of cells of a cell-pruned search (0: all pairs); [13] query chunks of the
                                        pass (1 unless the wide plan's candidates exceed 1 GiB), [14] 1 if the wide plan ran
                                        (k > 60), [15] candidates per query (lists x list length) */

/* the smallest relative distance from `tol` of the residual norms that decided the stops of the last tolerance-mode (GLX_CG_TREE)
 * solve on this operator; +inf when there was none.  ssl.laplace / ssl.randomwalk (reduce='auto') hand a solve whose stop hung on less
 * than ssl.AUTO_STOP_BAND back to the reference-order reductions. */
int glx_cg_last_stop_margin(glx_graph* A, double* margin_out);
/* how the last reference-order solve on this operator walked numpy's reduction chains (csrc/seqsum_exact.h): out4 = blocks of 256 rows
 * applied as plain integer sums, through their record (rows added exactly between integer segments), row by row -- summed over
 * the solve's reductions --, and which kinds of reduction were still in block form at its end (bit 0: p.Ap, bit 1: r.r; the solve
 * moves a kind whose products cancel to the chain form, see GLX_CG_BLOCKS); all -1: the chain form throughout (GLX_CG_CHAIN, fewer
 * than 8192 rows, a 1-D right-hand side) or no solve yet. */
int glx_cg_last_block_stats(glx_graph* A, int* out4);

/* ---- exact radius graphs: weightmatrix.epsilon_ball (csrc/ball.hip) -------------------------------------------------------
 * The unordered pair {i, j}, i != j, is an edge iff the squared distance in the accumulation order of scipy's cKDTree
 * (csrc/sqdist_tree.h) is <= fl(epsilon * epsilon).  glx_ball_search finds the structure (X (n, d) and the optional features
 * F (n, m_f) are host arrays, finite; epsilon >= 0) and keeps it on the device: rows of ascending columns, no diagonal.
 * GLX_EUNSUPPORTED (with the count in the message) when the graph has more than 2^31 - 1 entries.  OWNERSHIP: the caller owns
 * *out and releases it with glx_ball_result_destroy; the other calls borrow it.
 * glx_ball_result_to_csr weighs the entries -- distances summed in numpy's order (csrc/npsum_exact.h), times the same kernel of
 * the feature distance with epsilon_f when the search had features -- and drops those whose weight is exactly zero.  kernel:
 * 1 uniform, 2 gaussian (correctly rounded exp), 4 distance, 5 singular, or 0: structure and distances only (val = 1, nothing
 * dropped; the caller weighs on the host).  rowptr [n + 1]; col, val, dists_out, fdists_out [glx_ball_result_nnz] (val and
 * either distance output may be NULL; distances only where nothing is dropped); *nnz_out = entries written.
 * glx_ball_stats, of the calling thread's last search: [0] pairs tested, [1] pairs accepted (= entries), [2] cells, device ms of
 * [3] the grid passes, [4] count + scan, [5] fill, [6] the row sorts, [7] weights + second scan of the last glx_ball_result_to_csr. */
typedef struct glx_ball_result glx_ball_result;
int glx_ball_search(const double* X, int64_t n, int d, double epsilon, const double* F, int m_f, int device, glx_ball_result** out);
int glx_ball_result_nnz(const glx_ball_result* res, int64_t* nnz_out);
int glx_ball_result_to_csr(const glx_ball_result* res, int kernel, double epsilon_f, int32_t* rowptr, int32_t* col, double* val,
                           double* dists_out, double* fdists_out, int64_t* nnz_out);
int glx_ball_result_destroy(glx_ball_result* res);
int glx_ball_stats(double stats[8]);

/* ---- shortest paths: graph.dijkstra / graph.dijkstra_hl (csrc/sssp.hip) ------------------------------------------------------------
 * Replaces dijkstra_main / dijkstra_hl_main of the reference's C extension (c_code/hjsolvers.cpp:117-227) by label-correcting rounds
 * on the device whose fixed point is the heap's result bit for bit (the argument heads csrc/sssp.hip).
 * The graph arrives as its IN-edge lists: vertex j's entries in_idx[in_ptr[j] .. in_ptr[j+1]) are the vertices i with an edge i -> j,
 * in_cost the costs c_ij = fl(W[i,j] * f[i]) >= 0 (self entries and explicit zeros of W already removed; +inf allowed).
 * B >= 1 independent problems on that graph: problem b's sources are src_idx[src_ptr[b] .. src_ptr[b+1]) with boundary values
 * src_val >= 0; a vertex listed twice in one problem is refused.  form: the relaxation, GLX_SSSP_PLAIN fl(a + c) or
 * GLX_SSSP_HOPF_LAX (c + sqrt(c*c + 4*a*a))/2.  A vertex is relaxed from i only while u_i <= max_dist.
 * dist (n, B) fp64, vertex-major: the distances, +inf where they exceed max_dist or nothing is reached.  cp (n, B) int32 or NULL: the
 * smallest source index reaching the vertex along tight edges, -1 where dist is +inf.  rounds_out[2] (or NULL): rounds of the distance
 * and of the closest-point iteration, the idle last round included.  n * B <= 2^31.  All pointers are host pointers.
 * out_ptr / out_idx (or NULL): the same edges listed by the vertex they LEAVE (out_idx[out_ptr[i] .. out_ptr[i+1]) = the vertices j
 * with an edge i -> j).  With them a round only looks at values one of whose in-neighbours was lowered in the round before; without
 * them every round looks at every value (same results, for measurement).  ms_out[4] (or NULL): host milliseconds of the uploads, the
 * distance rounds, the closest-point rounds and the downloads. */
#define GLX_SSSP_PLAIN 0
#define GLX_SSSP_HOPF_LAX 1
int glx_sssp(int64_t n, int64_t nnz, const int64_t* in_ptr, const int32_t* in_idx, const double* in_cost,
             const int64_t* out_ptr, const int32_t* out_idx, int B, const int64_t* src_ptr, const int32_t* src_idx,
             const double* src_val, double max_dist, int form, double* dist, int32_t* cp, int64_t* rounds_out, double* ms_out,
             int device);

/* ---- connected components: graph.connected_components / largest_connected_component (csrc/cc.hip, csrc/cc_plan.h) -----------------
 * The components of the PATTERN of a CSR matrix: every stored entry (i, j) with i != j joins i and j, whatever its direction and value
 * (a stored zero is an entry; rows may be unsorted and hold duplicates; a graph with no entries has n components).  Lock-free
 * union-find in one pass (the argument heads csrc/cc.hip); labels (n) <- the component of every vertex, components numbered by their
 * smallest vertex in ascending order: the labels of scipy.sparse.csgraph.connected_components(W, directed=False), and of its default
 * weak form, on every vertex.  *ncomp_out <- the number of components.  ms_out[4] (or NULL): host milliseconds of the uploads, the
 * checks (row pointers on the host, column indices on the device), the kernels and the downloads.  n >= 1, nnz >= 0, both at most
 * 2^31 - 1 (GLX_EUNSUPPORTED beyond).  All pointers are host pointers; the caller owns the buffers.  GLX_EINVAL, before any kernel
 * follows an index: a null argument, rowptr[0] != 0, rowptr[n] != nnz, row pointers that decrease, a column index outside [0, n).
 * glx_components_set_wave_row: a plan override of the calling thread for measurements -- rows of at least that many stored entries
 * take a wavefront, shorter ones a thread (0: the library's CC_WAVE_ROW).  No result depends on it.
 * glx_components_plan: out[4] <- the threshold in effect, the library's own, the vertices per tile of the numbering's prefix sum, the
 * rows that took a wavefront in the calling thread's last glx_components. */
int glx_components(int64_t n, int64_t nnz, const int32_t* rowptr, const int32_t* col, int32_t* labels, int64_t* ncomp_out,
                   double* ms_out, int device);
int glx_components_set_wave_row(int min_entries);
int glx_components_plan(int64_t out[4]);

/* ---- in-order Gauss-Seidel sweeps: graph.amle / ssl.amle (csrc/lip.hip, csrc/lip_plan.h) ---------------------------------------------
 * lip_iterate_main (weighted = 0) and lip_iterate_weighted_main (weighted != 0) of the reference's C extension
 * (c_code/lp_iterate.cpp:129-259) bit for bit: the sequential sweep in vertex order runs as the levels of its dependence pattern,
 * a launch per level or one workgroup over a run of small levels.
 * The graph arrives as the reference hands it over: M stored entries sorted by vertex, row[e] the vertex, nbr[e] its neighbour, W[e] >= 0
 * the weight, the order inside a vertex's block the caller's (it decides the rounding).  B >= 1 columns share the m boundary vertices
 * ind (a vertex listed twice takes its last value); val (m, B) row-major are their values per column.  u starts at zero off the boundary.
 * Unweighted: ne = alpha*sumu/deg + beta*(minu + maxu)/2 (graph.amle: alpha 0, beta 1; graph.plaplace(fast=True): alpha 1/(p-1),
 * beta 1-alpha); weighted: 30 bisection passes per vertex, alpha and beta unused.  At most T <= 2^24 sweeps; a column stops on its own
 * after the sweep `it` with err < tol && it > 20 and is frozen from then on.
 * u (n, B) row-major: the result.  iters_out[B] (or NULL): sweeps done per column.  plan_out[3] (or NULL): levels, launches per
 * sweep, launches enqueued in all.  err_hist (T, B) or NULL: err of sweep `it`, column b at [it * B + b] for the sweeps the column
 * ran (other entries are left alone).  small_level: a plan override for measurements -- levels of at most that many vertices are merged
 * into single-workgroup launches (0: none are, every level is a launch of its own; < 0: the library's constant).  The result does not
 * depend on it.  All pointers are host pointers.
 * GLX_EINVAL: a null argument, B < 1, an index out of range, entries not sorted by vertex, a negative or NaN weight, a vertex that is
 * not on the boundary and has no stored entry (the reference reads another vertex's entry, or past the arrays, there). */
int glx_lip_iterate(int64_t n, int64_t M, const int32_t* nbr, const int32_t* row, const double* W, int B, int64_t m, const int32_t* ind,
                    const double* val, int weighted, double alpha, double beta, int64_t T, double tol, double* u, int64_t* iters_out,
                    int64_t* plan_out, double* err_hist, int small_level, int device);

/* ---- sparse label propagation: ssl.sparse_label_propagation (csrc/slp.hip, csrc/slp_plan.h) ----------------------------------------
 * The primal-dual total-variation sweeps of the reference's ssl.sparse_label_propagation (ssl.py:1429-1508) bit for bit; the contract,
 * every operation rounded on its own, is DESIGN.md 4.9.  W arrives as canonical CSR: n rows, M entries, row_ptr (n + 1), col ascending
 * inside a row without duplicates, W finite and > 0, no empty row.  lam (M) per entry and gamma (n) per vertex are the caller's (the
 * host's expm1 / log1p and degree ** -1).  C >= 1 class columns share the m labelled vertices ind (a vertex listed twice takes its
 * last row); val (m, C) row-major are the rows they are set to in every iteration.  u and the edge state start at zero; T iterations
 * of two launches each (vertex phase, edge phase), full chunks replayed from a captured launch sequence; more than 16 columns run as
 * tiles of at most 16, one after another, and the result does not depend on the tiling.
 * u (n, C) row-major: the result (zeros for T = 0, also on the labelled vertices).  u_hist (T, n, C) or NULL: u after every iteration.
 * plan_out[3] (or NULL): launches per iteration, sweep launches enqueued in all, columns of the widest tile.  All pointers are host
 * pointers.  GLX_EINVAL: a null argument, C < 1, rows that are not canonical, an index out of range, a weight that is not finite and
 * > 0, a non-finite lam or gamma, an empty row. */
int glx_slp_iterate(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* col, const double* W, const double* lam,
                    const double* gamma, int C, int64_t m, const int32_t* ind, const double* val, int64_t T, double* u, double* u_hist,
                    int64_t* plan_out, int device);

/* ---- p-Laplace Jacobi iteration, all columns in one call: ssl.plaplace(fast=False) (csrc/plaplace.hip, csrc/lp_plan.h) -------------
 * B problems of glx_lp_iterate (glx.h) on one graph that share the m boundary vertices ind (a vertex listed twice takes its last
 * row); val (m, B) row-major are their values, one problem per column.  Column b starts from uu = max(val[:, b]), ul = min(val[:, b])
 * off the boundary (NaN if the column holds one; -inf / +inf for m = 0) and val on it.  nbr / row / W (M): the stored entries sorted by
 * vertex, as glx_lp_iterate takes them.  Every column equals, bit for bit, what glx_lp_iterate returns for that column alone: uu, ul
 * (the content of the first of the two iterate buffers: U_S for a stop at an even iteration S, U_{S+1} at an odd one) and the
 * stopping iteration.  A column stops on its own at the first `it` with err < tol && it > 10 and is written by no later iteration.
 * uu, ul (n, B) row-major: the results.  iters_out[B] (or NULL): the stopping iteration per column (T if never).  1 <= B <= 256,
 * T <= 2^24, n * B <= 2^31 (GLX_EUNSUPPORTED beyond).  All pointers are host pointers.  GLX_EINVAL: a null argument, bad sizes, an
 * index out of range. */
int glx_lp_iterate_batch(int64_t n, int64_t M, const int32_t* nbr, const int32_t* row, const double* W, int B, int64_t m,
                         const int32_t* ind, const double* val, double p, int64_t T, double tol, double* uu, double* ul,
                         int64_t* iters_out, int device);

/* ---- centered-kernel learner: ssl.centered_kernel (csrc/ck.hip, csrc/ck_plan.h) ---------------------------------------------------
 * The loop of the reference's ssl.centered_kernel (ssl.py:1346-1426; Mai and Couillet, ICML 2018) in one blocking call: power_it
 * steps of the power iteration e <- C W C e / |C W C e| from the caller's start vector e (n) for l = |e.w / e.e|, alpha =
 * alpha_frac * l, then u <- u + w with w = (1 / alpha) C W C u - u, w = 0 on the training rows, until !(max|w| > tol): iteration q
 * (1-based) is the last one iff !(err_q > tol), with err_0 = 1 (tol >= 1 or NaN: no iteration, u is the start).  C x = x - mean(x)
 * column by column; the products use the one-pass form and the fixed reduction order of DESIGN.md 4.11, so the result is a pure
 * function of the arguments (no floating-point atomics) and equals ck_host_reference (csrc/ck_plan.h) bit for bit.  W arrives as
 * canonical CSR WITHOUT its diagonal: n rows, M entries, row_ptr (n + 1), col ascending inside a row; weights finite, of either sign;
 * empty rows are legal.  1 <= k <= 256 columns; u starts from val (m, k) row-major on the m training vertices ind (a vertex listed
 * twice takes its last row) and from zero elsewhere.  Two launches per iteration; the host reads the err slots once per chunk.
 * u (n, k) row-major: the iterate that includes the stopping iteration's update.  *l_out: the eigenvalue estimate.  *T_out: the
 * iterations that ran.  err_hist (or NULL): err_q at err_hist[q - 1] for q <= min(T, err_cap); nothing behind it is written.
 * on_iterate (or NULL): called after every iteration with (q, the iterate (n, k), err_q, user) -- the call then runs one iteration
 * per chunk and downloads every iterate, which is slow; a nonzero return ends the call with GLX_EINVAL.  plan_out[4] (or NULL):
 * kernels per iteration, launches enqueued, iterations per chunk, partial sums per column.  All pointers are host pointers.
 * GLX_EINVAL: a null argument, bad sizes, rows that are not canonical or store a diagonal entry, an index out of range, a weight that is
 * not finite, power_it or max_it outside [1, 2^24].  GLX_EUNSUPPORTED: k > 256, n * k > 2^31, or max_it iterations without a stop
 * (the reference has no cap; *l_out is set). */
typedef int (*glx_ck_iterate_fn)(int64_t q, const double* u, double err, void* user);
int glx_ck_solve(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* col, const double* W, int k, int64_t m, const int32_t* ind,
                 const double* val, const double* e, int64_t power_it, double alpha_frac, double tol, int64_t max_it, double* u,
                 double* l_out, int64_t* T_out, double* err_hist, int64_t err_cap, glx_ck_iterate_fn on_iterate, void* user,
                 int64_t* plan_out, int device);

/* ---- multiclass MBO learner: ssl.multiclass_mbo (csrc/mmbo.hip, csrc/mmbo_plan.h) ------------------------------------------------
 * The loop of the reference's ssl.multiclass_mbo (ssl.py:989-996; Garcia-Cardona et al. 2014) in one blocking call: T outer
 * iterations of Ns diffusion steps Z = (u - c0 J (u - K)) (X diag(d)), u = Z X^T with c0 = (dt / Ns) mu and d[j] = 1 / (1 + (dt / Ns)
 * vals[j]), each followed by the projection of every vertex onto its first largest class.  X (n, m) row-major and vals (m) are any
 * finite arrays (the learner hands in eigenpairs of the normalised Laplacian); lab0 (n) are the start labels in [0, k), used as they
 * are; the ntrain training vertices ind carry the labels lab in [0, k) (a vertex listed twice takes its last label; ntrain = 0 is
 * legal).  The order of operations and of every sum is that of DESIGN.md 4.13, so the result is a pure function of the arguments (no
 * floating-point atomics, no fused multiply-add) and equals mmbo_host_reference (csrc/mmbo_plan.h) bit for bit.  Two launches per
 * step and one last pass for the labels; u is never stored.  hist (T, n): the labels after every outer iteration, the last row is the
 * result.  Zlast (k, m): the Z of the last step.  plan_out[7] (or NULL): launches per step, rows per partial sum, partial sums, the
 * caps on k * m, k and m, launches enqueued.  All pointers are host pointers.
 * GLX_EINVAL: a null argument, bad sizes, Ns or T below 1 or T * Ns above 2^24, dt or mu not finite, a training vertex or a label out
 * of range, X, vals or a factor d[j] not finite.  GLX_EUNSUPPORTED, before anything is touched: k > 256, m > 256, k * m > 4096 (Z is
 * held in LDS), n * m, T * n or partial sums * k * m above 2^31. */
int glx_mmbo_solve(int64_t n, int m, const double* X, const double* vals, const int32_t* lab0, int64_t ntrain, const int32_t* ind,
                   const int32_t* lab, int k, int64_t Ns, int64_t T, double dt, double mu, int32_t* hist, double* Zlast, int64_t* plan_out,
                   int device);

/* ---- thick-restart Lanczos eigensolver: graph.eigen_decomp, ssl.poisson(solver='spectral') (csrc/eig.hip, csrc/eig_plan.h) --------
 * The device half of the solver for the k largest singular values of a symmetric matrix A (the method works on B = A A): a basis of
 * m + 1 column-major Lanczos vectors that stays on the device, and the operations on it.  The host half -- the projected matrix, the
 * stop, the restart, the probe for a missed multiple eigenvalue -- is graphlearning_amd/_eig.py.  Every operation is a pure function of
 * its arguments in the order of DESIGN.md 4.12 (no fused multiply-add, no floating-point atomics) and equals EigHost of csrc/eig_plan.h
 * bit for bit.  A arrives as canonical CSR: n rows, row_ptr (n + 1), col strictly ascending inside a row, val finite; a stored
 * diagonal and empty rows are legal; symmetry is the caller's business.  1 <= m <= min(n, 513).  OWNERSHIP: the caller owns *out and
 * releases it with glx_eig_destroy.  All pointers are host pointers; every call returns with its work complete.
 * glx_eig_set_column: column j (0 .. m) <- host_vector (n).
 * glx_eig_orthonormalize: column j (0 .. m) is made orthogonal to the columns before it (two passes of projection and update) and
 *   scaled to length one; *norm_out = its length before the scaling.
 * glx_eig_run: the Lanczos steps j0 <= j < j1 <= m, each reading the columns 0 .. j and writing column j + 1, enqueued without a
 *   host wait in between; alpha_out, beta_out (j1 - j0): the coefficients of the steps.
 * glx_eig_rotate: V[:, :keep] <- V[:, :rows] Y with Y (rows, keep) row-major, 1 <= keep <= rows <= m, every element summed in ascending
 *   column order; then V[:, keep] <- V[:, rows].
 * glx_eig_get_columns: out (j1 - j0, n) <- the columns j0 <= j < j1 <= m + 1, column j0 first.
 * GLX_EINVAL: a null argument, rows that are not canonical, an index out of range, a value that is not finite, m or a column outside its
 * range.  GLX_EUNSUPPORTED: more than 256 columns asked of glx_eig_get_columns.  GLX_ENOMEM: the (m + 3) n doubles of the basis and
 * its two work vectors, the matrix and the partial sums exceed the device's memory. */
typedef struct glx_eig glx_eig;
int glx_eig_create(int64_t n, const int64_t* row_ptr, const int32_t* col, const double* val, int m, int device, glx_eig** out);
int glx_eig_set_column(glx_eig* e, int j, const double* host_vector);
int glx_eig_orthonormalize(glx_eig* e, int j, double* norm_out);
int glx_eig_run(glx_eig* e, int j0, int j1, double* alpha_out, double* beta_out);
int glx_eig_rotate(glx_eig* e, const double* Y, int rows, int keep);
int glx_eig_get_columns(glx_eig* e, int j0, int j1, double* out);
int glx_eig_destroy(glx_eig* e);

/* ---- INCRES clustering: clustering.incres (csrc/incres.hip, csrc/incres_plan.h) -----------------------------------------------------
 * The device half of one outer iteration of the reference's clustering.incres (clustering.py:348-361; Bresson et al. 2016): plant,
 * grow `while np.min(F) == 0: F = P*F`, harvest `np.argmax(F, axis=1)`.  The handle holds P (n x n, CSR with int32 row pointers; a
 * row's STORED entry order is kept and is the order of every sum: hand over scipy's `W*D` as it is, unsorted) and the state of k <= 256
 * columns across the iterations.  The product is the sweep engine's, bit for bit scipy's csr_matvecs; the census behind every sweep
 * tests the k real columns for an entry equal to 0.0 (a denormal is not zero) and takes the row-wise first-maximum index.  The contract
 * is DESIGN.md 4.15.  OWNERSHIP: the caller owns *out and releases it with glx_incres_destroy.  All pointers are host pointers; every
 * call returns with its work complete.
 * glx_incres_step: seeds (k, m) row-major, vertex ids in the caller's numbering, duplicates allowed: F <- 0, F[seeds[r][:], r] <- 1;
 *   then sweeps until no entry is zero; labels_out (n) <- the argmax, *sweeps_out <- the number of sweeps (0: the planted state had no
 *   zero).  At most max_grow sweeps: GLX_EUNSUPPORTED if the iterate behind max_grow sweeps still holds a zero (*sweeps_out = max_grow;
 *   the graph is disconnected, bipartite, or so long that values underflow) -- an error return, the handle stays usable.
 * glx_incres_stats: out[12] <- the chunk cap, the first guess, the margin, the length of a loop's second chunk, grow loops so far, chunks read,
 *   sweeps enqueued, sweeps counted, lanes per record, elements per record, 1 if the locality renumbering is in use, slices.
 * glx_host_group_by_label (host only, no device): the vertices grouped by label for the plant's draws -- counts (k) <- members per label,
 *   order (n) <- the vertex ids sorted by label, ascending inside a label (a counting sort): the members of cluster r in ascending
 *   order are order[counts[0] + .. + counts[r-1] ..][:counts[r]].  GLX_EINVAL: a label outside [0, k).
 * glx_incres_set_options: the calling thread's schedule -- chunk: every chunk has this length; margin: the first chunk of a loop is the
 *   count before plus this; next: the length of a loop's second chunk, every further one twice the one before (each 1 .. 64; 0, or
 *   NULL for all: the library decides).  No result
 *   depends on them.
 * GLX_EINVAL: a null argument, n < 1, an index or a seed out of range, m or max_grow below 1.  GLX_EUNSUPPORTED: k outside 1 .. 256. */
typedef struct glx_incres glx_incres;
typedef struct { int chunk, margin, next; } glx_incres_options;
int glx_incres_set_options(const glx_incres_options* opt);
int glx_incres_create(int64_t n, const int32_t* row_ptr, const int32_t* col, const double* val, int k, int device, glx_incres** out);
int glx_incres_step(glx_incres* h, const int32_t* seeds, int64_t m, int64_t max_grow, int32_t* labels_out, int64_t* sweeps_out);
int glx_incres_stats(glx_incres* h, int64_t* out);
int glx_incres_destroy(glx_incres* h);
int glx_host_group_by_label(int64_t n, const int32_t* labels, int k, int64_t* counts, int32_t* order);

/* ---- dynamic label propagation: ssl.dynamic_label_propagation (csrc/dlp.hip, csrc/dlp_plan.h) -------------------------------------
 * The loop of the reference's ssl.dynamic_label_propagation (ssl.py:1328-1332; Wang, Tu and Tsotsos, ICCV 2013) in one blocking call
 * and without its dense n x n array: T steps of v = P u; u = Pt u; u[ind] = val; Pt = P Pt P^T + alpha v v^T + lam I (Pt = P at
 * first), with Pt applied through the unrolled recursion Pt_t X = P (Pt_{t-1} (P^T X)) + alpha v_{t-1} (v_{t-1}^T X) + lam X --
 * T^2 + max(T - 2, 0) sparse products of (n, k) blocks and T (T - 1) / 2 Gram matrices of size k x k per call, (2 T + 2) n k values
 * of workspace.  The order of operations and of every sum is that of DESIGN.md 4.17, so the result is a pure function of the
 * arguments (no floating-point atomics, no fused multiply-add) and equals dlp_host_reference (csrc/dlp_plan.h) bit for bit; alpha == 0
 * and lam == 0 take no shortcut.  P arrives as canonical CSR: n rows, M entries, row_ptr (n + 1), col strictly ascending inside a row,
 * values finite, of either sign; empty rows and a stored diagonal are legal; P^T is built inside the call.  u starts from val (m, k)
 * row-major on the m training vertices ind (a vertex listed twice takes its last row) and from zero elsewhere, and the training rows
 * are set back to val after every step.  u (n, k) row-major: u_T.  hist (or NULL), (T, n, k): u_1 .. u_T.  plan_out[4] (or NULL): the
 * launches enqueued, the sparse passes, the Gram passes, the partial sums per Gram entry.  The host reads nothing back between the
 * steps.  All pointers are host pointers.
 * GLX_EINVAL: a null argument, bad sizes, rows that are not canonical, an index out of range, a value that is not finite, T < 1, alpha or
 * lam not finite.  GLX_EUNSUPPORTED: k > 64 (the Gram is held in LDS), T > 64, (2 T + 2) n k > 2^30. */
int glx_dlp_solve(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* col, const double* P, int k, int64_t m,
                  const int32_t* ind, const double* val, double alpha, double lam, int64_t T, double* u, double* hist,
                  int64_t* plan_out, int device);

/* ---- acquisition functions of active learning: graphlearning_amd.active_learning (csrc/acq.hip, csrc/acq_plan.h) ------------------
 * var_opt, sigma_opt, model_change and model_change_var_opt of the reference (active_learning.py:237-575) in the truncated eigenbasis.
 * The handle keeps V (n, M) row-major -- vertex i is the row v_i -- and the covariance C (M, M) row-major on the device; gamma2 is fixed
 * at creation.  The order of every sum and operation is that of DESIGN.md 4.19 (chains in ascending index, no fused multiply-add, no
 * floating-point atomics), so every result is a pure function of the arguments and equals acq_host_compute / acq_host_update /
 * acq_host_greedy of csrc/acq_plan.h bit for bit.  OWNERSHIP: the caller owns *out and releases it with glx_acq_destroy.  All pointers
 * are host pointers; every call returns with its work complete.
 * glx_acq_compute: vals_out (nc) <- the value of `kind` at the rows cand[0 .. nc) of V (positions may repeat, in any order; nc = 0
 *   launches nothing), with w = C v, d = v.w: VAR (sqrt(sum w^2))^2 / (gamma2 + d); SIGMA (sum w)^2 / (gamma2 + d); MC unc sqrt(sum w^2)
 *   / (gamma2 + d); MCVAR unc (sqrt(sum w^2))^2 / (gamma2 + d).  unc (nc): the multiplier of MC and MCVAR (required there, ignored
 *   otherwise).  Values that are not finite are returned as they are.
 * glx_acq_update: for each query in order w = C v, ip = v.w, C[a, b] <- C[a, b] - (w[a] w[b]) / (gamma2 + ip): numpy's
 *   C -= np.outer(w, w) / (gamma2 + ip).  One launch for the batch; repeated indices are legal.
 * glx_acq_greedy (VAR and SIGMA): b rounds on a scratch copy of C -- evaluate, take the first maximum (equal values go to the smallest
 *   position in cand), strike the chosen vertex from the candidates, apply its rank-one step.  queries_out (b) <- the chosen POSITIONS
 *   in cand, vals_out (b) <- their values.  The handle's C is left as it was; nothing is read back between the rounds.
 * glx_acq_get_c: C_out (M, M) <- the current covariance.
 * glx_acq_stats: out[8] <- launches of the pass by glx_acq_compute, of the update, of the greedy design (two per round), candidates per
 *   workgroup of the pass, bytes of LDS of the pass, bytes of LDS of the update (0: C stays in L2 between the queries), n, M.
 * GLX_EINVAL: a null argument, n or M below 1, an entry of V or C or gamma2 not finite, a kind outside the table (for the greedy design
 *   outside VAR and SIGMA), a position outside [0, n), MC or MCVAR without unc, b above the number of distinct vertices in cand, a
 *   greedy round whose maximum is not finite (the message names the round; the outputs hold the rounds before it).
 * GLX_EUNSUPPORTED: M > 256, n > 2^31 - 1. */
#define GLX_ACQ_VAR 0
#define GLX_ACQ_SIGMA 1
#define GLX_ACQ_MC 2
#define GLX_ACQ_MCVAR 3
typedef struct glx_acq glx_acq;
int glx_acq_create(int64_t n, int M, const double* V, const double* C, double gamma2, int device, glx_acq** out);
int glx_acq_compute(glx_acq* h, int kind, const int32_t* cand, int64_t nc, const double* unc, double* vals_out);
int glx_acq_update(glx_acq* h, const int32_t* query, int64_t nq);
int glx_acq_greedy(glx_acq* h, int kind, const int32_t* cand, int64_t nc, int64_t b, int32_t* queries_out, double* vals_out);
int glx_acq_get_c(glx_acq* h, double* C_out);
int glx_acq_stats(glx_acq* h, int64_t* out);
int glx_acq_destroy(glx_acq* h);

/* ---- boundary test of a point cloud: utils.boundary_statistic (csrc/bstat.hip, csrc/bstat_plan.h) ----------------------------------
 * The boundary statistic of Calder, Park and Slepcev (reference utils.py:18-114) over the rows of a canonical CSR pattern whose
 * weights are all 1 (only the pattern arrives): the ball graph of weightmatrix.epsilon_ball in the radius mode, the directed kNN graph
 * of weightmatrix.knn(symmetrize=False) in the kNN mode.  The arithmetic, operation by operation, heads csrc/bstat_plan.h; the
 * normals equal the reference's bit for bit, the statistic as numbers (a zero is +0.0).
 * X (n, d) row-major; indptr (n + 1) / indices (nnz) the pattern; J (n, k) the neighbour lists of the kNN mode (self included) or NULL
 * with k = 0: the radius mode, whose lists are the rows of the pattern, a row of the largest length L without its farthest entry and
 * every row of fewer than L - 1 entries with a 0 among its terms (a row of exactly L - 1 entries: its entries, no 0).  flags: GLX_BSTAT_SECOND_ORDER | GLX_BSTAT_CUTOFF.
 * T (n) <- the statistic, nu (n, d) <- the unit normals.  stats_out[8] (or NULL): launches, rows of the short class, rows that took a
 * wavefront, rows of the largest length (radius mode), host milliseconds of the checks, the uploads, the kernels and the downloads.
 * All pointers are host pointers.  GLX_EINVAL, before anything is launched: a null argument, sizes below 1 or above 2^31 - 1, k above
 * min(n, 1024), row pointers that do not run from 0 to nnz ascending, a column or list index outside [0, n), a row whose columns
 * are not strictly ascending, an empty row.  GLX_EINVAL behind the kernels: a vertex whose raw normal has norm zero or not finite (the
 * message names the lowest such vertex; T and nu are left untouched).
 * glx_boundary_stat_set_wave_row: a plan override of the calling thread for measurements -- rows of at least that many members take
 * a wavefront, shorter ones a group of 16 lanes (0: the library's BSTAT_WAVE_ROW).  No result depends on it. */
#define GLX_BSTAT_SECOND_ORDER 1
#define GLX_BSTAT_CUTOFF 2
int glx_boundary_stat(int64_t n, int d, const double* X, int64_t nnz, const int32_t* indptr, const int32_t* indices, int k,
                      const int32_t* J, int flags, double* T, double* nu, double* stats_out, int device);
int glx_boundary_stat_set_wave_row(int min_members);

/* ---- p-eikonal equation: graph.peikonal / ssl.peikonal (csrc/peik.hip, csrc/peik_plan.h) --------------------------------------------
 * sum_j w_ij (u_i - u_j)_+^p = f_i off the boundary, u = g on it: peikonal_fmm_main of the reference's C extension
 * (c_code/hjsolvers.cpp:342-420) as synchronous fixed-point rounds u_j <- min(u_j, S_j(u)) from +inf, neighbours at +inf left out;
 * the arithmetic, operation by operation, heads csrc/peik_plan.h.  For p == 1 the result equals peik_host_reference (and the
 * reference's marching solver) bit for bit; for p != 1 the local solve is num_bisection_it halvings with the device's pow.
 * The graph arrives as the reference hands it over: M stored entries sorted by vertex, row_ptr (n + 1) their blocks, nbr the
 * neighbour, W the weight (finite, > 0); a stored self loop is skipped.  f (n) >= 0.  B problems on that graph: problem b's boundary
 * vertices are bdy_idx[bdy_ptr[b] .. bdy_ptr[b + 1]) with the values bdy_val (a vertex listed twice takes its last value; a list may
 * not be empty).  u0 (n): the value of a vertex no boundary reaches.  max_rounds: 0, or a cap below the library's (2 n + 2 rounds,
 * and 8 more per halving for p != 1: csrc/peik_plan.h; a test hook).
 * u (n, B) row-major: the result.  *rounds_out (or NULL): the rounds run, the idle last one included.  ms_out[3] (or NULL): host
 * milliseconds of the uploads, the rounds and the download.  One launch per round, the flags of 32 rounds read at once; no result
 * depends on that length.  All pointers are host pointers.
 * GLX_EINVAL: a null argument, bad sizes or row pointers, an index out of range, an empty boundary list, a weight that is not finite
 * and > 0, an f that is negative or not finite, a g or u0 that is not finite, p not finite or <= 0, num_bisection_it outside 1 .. 128.
 * GLX_EUNSUPPORTED: B outside 1 .. 256, n * B > 2^31, or values that still fall after the cap on the rounds. */
int glx_peikonal(int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* nbr, const double* W, const double* f, int B,
                 const int64_t* bdy_ptr, const int32_t* bdy_idx, const double* bdy_val, double p, int num_bisection_it, const double* u0,
                 int64_t max_rounds, double* u, int64_t* rounds_out, double* ms_out, int device);

#ifdef __cplusplus
}
#endif
#endif
