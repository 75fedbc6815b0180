"""Host restatement of the stop-column sweeps (glx_sweep_run, csrc/solver.hip; glx_sweep_groups_run, csrc/groups.hip; their shared
loop glx_sweep_tail, csrc/sweep_core.hip) in plain
numpy / scipy, and the fixtures tests/test_sweep_ref_host.py and tests/test_gpu_sweep_stop.py share.  No GPU, no library call.

What the two entry points promise, and what `poisson_sweeps` states:

    A_dt = A's entries rounded to the state's dtype, in stored order;  A_w = A_dt widened to float64
    u = 0 (dtype), w = w0 (float64), t = 0
    while t < max_iter:
        if t >= min_iter:  e = max|deg * w - vinf| (two roundings, NaN propagates); record e; stop when not (e > 1 / n)
        u = Db + A_dt u      every row summed entry by entry in stored order, product and sum rounded separately in dtype
        w = A_w w            the same order in float64: a float32 state's stop value uses the float32-rounded weights
        t += 1

The products may be scipy's (`A @ x` walks a row's entries in stored order with separate roundings: csr_matvec / csr_matvecs); the
explicit entry-order loop is `loop_product`, and `prove_products` shows the two equal on a matrix before anything relies on scipy."""
import functools
import numpy as np
from scipy import sparse

LENGTHS = [0, 1, 3, 4, 5, 23, 24, 25, 63, 64, 65, 95, 96, 97, 255, 256, 257, 300]
N = 640
MIN_ITER = 3
MAX_ITER = 60
# Fixture A: w0 = 2^k * w_unit -> the sweep count T the stop test yields (w halves per sweep; found on the CPU, held by
# tests/test_sweep_ref_host.py in both dtypes; every k sits in the middle of its T's interval).  With min_iter = 3, T - 3 lands on
# 0, 1, 2 and 15, 16, 17 -- both parities inside a 16-sweep tail chunk and both sides of the chunk edge -- and on 33, in the third chunk.
K_T = [(-10.0, 3), (-5.625, 4), (-4.625, 5), (9.375, 18), (10.375, 19), (11.5, 20), (28.625, 36)]
POSITIONS = [0, 1, 2, 15, 16, 17, 33]
# the stacked groups: group b starts from k = GROUP_K[b % 10], so that two groups already stop in different chunks; at k = -14 the start
# value is below 1 / n (T = 0 with min_iter = 0)
GROUP_K_T = [(10.375, 19), (-14.0, 3), (28.625, 36), (-5.625, 4), (11.5, 20), (-0.25, 9), (9.375, 18), (25.375, 33), (16.875, 25), (3.0, 12)]
# the same ladder at 4608 rows, where the library renumbers the vertices by itself (it does so from 4096 rows on): one stop inside the
# first chunk, one on either side of the chunk edge
N_BIG = 4608
BIG_K_T = [(-8.5, 4), (7.75, 19), (8.75, 20)]


def as_dtype(A, dtype):
    """A with its entries rounded to `dtype`, in A's stored order (astype may sort a row, and the order inside a row is the order
    of its sum)."""
    A = sparse.csr_matrix(A)
    B = sparse.csr_matrix((A.data.astype(dtype), A.indices, A.indptr), shape=A.shape)
    B.has_sorted_indices = A.has_sorted_indices
    return B


def loop_product(A, x):
    """A x with every row summed entry by entry in stored order, product and sum rounded separately in the dtype A and x share.
    (Entry j of all rows that have one is added in one numpy statement: the order inside every row is that of a loop over its
    entries.)  x: (n,) or (n, C)."""
    dtype = A.data.dtype
    assert x.dtype == dtype, (x.dtype, dtype)
    indptr, indices, data = A.indptr.astype(np.int64), A.indices, A.data
    lengths = np.diff(indptr)
    acc = np.zeros((A.shape[0],) + x.shape[1:], dtype=dtype)
    for j in range(int(lengths.max()) if len(lengths) else 0):
        rows = np.nonzero(lengths > j)[0]
        at = indptr[rows] + j
        v = data[at] if x.ndim == 1 else data[at][:, None]
        prod = x[indices[at]] * v
        acc[rows] = acc[rows] + prod
    assert acc.dtype == dtype
    return acc


def host_sweep(A, u, Db, dtype):
    """Db + A u by the entry-order loop in `dtype` (Db None: the plain product)."""
    acc = loop_product(as_dtype(A, dtype), np.asarray(u).astype(dtype))
    return acc if Db is None else np.asarray(Db).astype(dtype) + acc


def prove_products(A, C=5, seed=0):
    """loop == scipy on A: the (n, C) product in float64 and float32, and the float64 stop-column product with the weights of
    either state."""
    rng = np.random.default_rng(seed)
    n = A.shape[1]
    u, w = rng.normal(size=(n, C)), rng.normal(size=n) * 3.0
    for dtype in (np.float64, np.float32):
        A_dt = as_dtype(A, dtype)
        ud = u.astype(dtype)
        got = A_dt @ ud
        assert got.dtype == dtype and np.array_equal(got, loop_product(A_dt, ud)), np.dtype(dtype).name
        A_w = as_dtype(A_dt, np.float64)
        assert np.array_equal(A_w.data, A_dt.data)
        assert np.array_equal(A_w @ w, loop_product(A_w, w)), np.dtype(dtype).name
    return True


def poisson_sweeps(A, Db, w0, deg, vinf, min_iter, max_iter, dtype, products='scipy'):
    """(u_T, T, first, stop_values) of one training set: see the module's docstring."""
    dtype = np.dtype(dtype).type
    A_dt = as_dtype(A, dtype)
    A_w = as_dtype(A_dt, np.float64)
    mul = (lambda M, x: M @ x) if products == 'scipy' else loop_product
    n = A.shape[0]
    Db = np.asarray(Db).astype(dtype)
    deg, vinf = np.asarray(deg, dtype=np.float64), np.asarray(vinf, dtype=np.float64)
    u = np.zeros(Db.shape, dtype=dtype)
    w = np.array(w0, dtype=np.float64)
    first = min(min_iter, max_iter)
    values = []
    t = 0
    while t < max_iter:
        if t >= min_iter:
            e = np.max(np.abs(deg * w - vinf))
            values.append(e)
            if not (e > 1 / n):
                break
        u = Db + mul(A_dt, u)
        w = mul(A_w, w)
        assert u.dtype == dtype and w.dtype == np.float64
        t += 1
    assert len(values) == t - first + (1 if t < max_iter else 0)
    return u, t, first, np.array(values, dtype=np.float64)


def groups(A, problems, deg, vinf, min_iter, max_iter, dtype):
    """Stacked training sets: the same function once per (Db_b, w0_b) -- a group's result does not depend on its neighbours."""
    return [poisson_sweeps(A, Db_b, w0_b, deg, vinf, min_iter, max_iter, dtype) for Db_b, w0_b in problems]


# ---- fixture A: the contraction ladder ---------------------------------------------------------------------------------------------
def ladder(seed=21, lengths=LENGTHS, n=N):
    """n rows whose lengths cycle through `lengths`; distinct columns in unsorted stored order; positive weights, every row scaled
    to sum 0.5 (w then halves per sweep)."""
    rng = np.random.default_rng(seed)
    lens = np.array([lengths[i % len(lengths)] for i in range(n)])
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = np.empty(indptr[-1], dtype=np.int32)
    data = np.empty(indptr[-1], dtype=np.float64)
    for i in range(n):
        indices[indptr[i]:indptr[i + 1]] = rng.choice(n, size=lens[i], replace=False)
        v = rng.random(lens[i]) + 0.25
        data[indptr[i]:indptr[i + 1]] = 0.5 * v / v.sum() if lens[i] else v
    A = sparse.csr_matrix((data, indices, indptr), shape=(n, n))
    A.has_sorted_indices = False
    return A, lens


def check_ladder(A, lens, lengths=LENGTHS):
    n = A.shape[0]
    assert set(lens.tolist()) == set(lengths) and np.array_equal(np.diff(A.indptr), lens)
    last = A.indices[A.indptr[-2]:A.indptr[-1]]
    assert len(last) > 1 and not np.all(np.diff(last) > 0)                          # stored order: unsorted
    assert all(len(set(A.indices[A.indptr[i]:A.indptr[i + 1]].tolist())) == lens[i] for i in range(n))
    assert A.data.min() > 0
    sums = np.asarray(A.sum(axis=1)).ravel()
    assert np.allclose(sums[lens > 0], 0.5, rtol=1e-12, atol=0) and np.all(sums[lens == 0] == 0)


def stop_vectors(n=N, seed=22):
    """(deg, vinf, w_unit): w0 = scale * w_unit."""
    rng = np.random.default_rng(seed)
    deg = rng.random(n) + 0.5
    vinf = 0.2 * rng.random(n) / n
    w_unit = rng.random(n) + 0.1
    return deg, vinf, w_unit


def bias(C, n=N, seed=23):
    """(n, C) of both signs, nonzero on about 30 % of the rows."""
    rng = np.random.default_rng(seed)
    Db = rng.normal(size=(n, C))
    Db[rng.random(n) >= 0.3] = 0.0
    return Db


@functools.lru_cache(maxsize=None)
def fixture_a(lengths=tuple(LENGTHS), n=N):
    """(A, deg, vinf, w_unit) of the ladder with the given row lengths, checked, loop == scipy proved; read-only."""
    A, lens = ladder(lengths=list(lengths), n=n)
    check_ladder(A, lens, list(lengths))
    assert prove_products(A)
    deg, vinf, w_unit = stop_vectors(n)
    for a in (A.data, A.indices, A.indptr, deg, vinf, w_unit):
        a.setflags(write=False)
    return A, deg, vinf, w_unit


@functools.lru_cache(maxsize=None)
def ladder_run(C, db_seed, k, min_iter, max_iter, dtype_name, n=N):
    """The reference run of fixture A with Db = bias(C, seed=db_seed) and w0 = 2^k w_unit: computed once, shared, read-only."""
    A, deg, vinf, w_unit = fixture_a(tuple(LENGTHS), n)
    u, T, first, vals = poisson_sweeps(A, bias(C, n=n, seed=db_seed), 2.0 ** k * w_unit, deg, vinf, min_iter, max_iter,
                                       np.dtype(dtype_name))
    u.setflags(write=False)
    vals.setflags(write=False)
    return u, T, first, vals


def group_k(b):
    return GROUP_K_T[b % len(GROUP_K_T)][0]


def group_db_seed(b):
    return 40 + b


def err0(deg, vinf, w0):
    """The stop value in front of the first sweep (what set_problem_rows is handed)."""
    return float(np.max(np.abs(deg * w0 - vinf)))


# ---- fixture B: the decision at 1 / n ----------------------------------------------------------------------------------------------
NB = 1024


def half_identity(n=NB):
    """P = I / 2 with deg = 1, vinf = 0: stop values w0 2^-t, exact in both dtypes; 1 / n = 2^-10."""
    return sparse.identity(n, dtype=np.float64, format='csr') * 0.5, np.ones(n), np.zeros(n)


REBOUND = (5, 700)


def half_identity_rebound(n=NB):
    """(P, deg, vinf, w0): P = I / 2 except two vertices a, b that feed each other, w_a <- 4 w_b and w_b <- w_a / 16, from
    w0 = 1 (a, b: 1 / 2).  The stop values are 2^-t at even t and 2^(2 - t) at odd t: the value at t = 10 EQUALS 1 / n and the run
    stops there, while the value a sweep later, 2^-9, is above 1 / n again -- a kernel that runs on at equality overwrites u_10."""
    a, b = REBOUND
    col, val = np.arange(n, dtype=np.int32), np.full(n, 0.5)
    col[a], val[a] = b, 4.0
    col[b], val[b] = a, 1.0 / 16
    P = sparse.csr_matrix((val, col, np.arange(n + 1, dtype=np.int32)), shape=(n, n))
    w0 = np.ones(n)
    w0[[a, b]] = 0.5
    return P, np.ones(n), np.zeros(n), w0


def bias_b(C, n=NB, seed=31):
    """Small integers on a third of the rows."""
    rng = np.random.default_rng(seed)
    Db = rng.integers(-3, 4, size=(n, C)).astype(np.float64)
    Db[rng.random(n) >= 0.35] = 0.0
    return Db
