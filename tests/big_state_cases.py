"""The fixtures tests/test_gpu_big_state.py runs on the device and tests/test_sell_plan_host.py holds, without one, to what they
claim: operators whose plans are the ones glx_graph_plan builds for states beyond 32 MB (tests/sell_plan_ref.py).

Both are built without a Python loop over rows: entry j of row i sits in column (a i + b + j P) mod n_cols with P a large prime that
does not divide n_cols -- the columns of a row are distinct (n_cols > the longest row) and their stored order is unsorted.

Fixture A (`rect`): 640 rows of the lengths sweep_ref.LENGTHS over n_cols columns, n_cols on either side of the flip of the row
classes; weights of both signs; the last column is used.
Fixture B (`square`): n rows, every 64th of them a hub of LENGTHS[(i // 64) % 18] entries, the others of (0, 1, 2, 3, 4, 7)[i % 6]:
at 300 000 rows every XCD range holds more than one window of 32 768 rows and some 260 rows split over 4 or 16 slots."""
import functools
import numpy as np
from scipy import sparse
import sweep_ref

P = 1000003
LENGTHS = sweep_ref.LENGTHS
SHORT = (0, 1, 2, 3, 4, 7)
N_A = 640
N_B = 300000
N_B32 = 600000
NNZ_B = 1265289
# the first column count of the big state at 4 lanes per row: n_cols * 4 * 4 * esize >= 32 MiB
FLIP = {'f64': 262144, 'f32': 524288}
ESIZE = {'f64': 8, 'f32': 4}
DT = {'f64': np.float64, 'f32': np.float32}
# stop-column runs on fixture B: w0 = 2^k w_unit -> sweeps (min_iter 3, max_iter 6); found on the CPU, held by test_sell_plan_host.py
STOP_MIN, STOP_MAX = 3, 6
STOP_K_T = [(-15.0, 4), (4.0, 6)]


def lengths_a():
    return np.array(LENGTHS, dtype=np.int64)[np.arange(N_A) % len(LENGTHS)]


def lengths_b(n=N_B):
    i = np.arange(n, dtype=np.int64)
    return np.where(i % 64 == 0, np.array(LENGTHS, dtype=np.int64)[(i // 64) % len(LENGTHS)], np.array(SHORT, dtype=np.int64)[i % 6])


def pattern(lens, n_cols, a, b):
    """(indptr, indices) of the rule above"""
    assert n_cols % P != 0 and P % n_cols != 0 and np.gcd(P, n_cols) == 1 and n_cols > lens.max()
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    row = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    j = np.arange(indptr[-1], dtype=np.int64) - indptr[row]
    indices = (a * row + b + j * P) % n_cols
    assert indptr[-1] < 2 ** 31
    return indptr.astype(np.int32), indices.astype(np.int32), row


def check_pattern(A, lens, rows):
    """the lengths, and on a sample of rows: distinct columns in unsorted stored order"""
    assert np.array_equal(np.diff(A.indptr), lens)
    unsorted = 0
    for i in rows:
        c = A.indices[A.indptr[i]:A.indptr[i + 1]]
        assert len(set(c.tolist())) == lens[i], i
        if len(c) > 2 and not np.all(np.diff(c) > 0):
            unsorted += 1
    assert unsorted >= sum(lens[i] > 7 for i in rows) > 0
    assert A.indices.min() >= 0 and A.indices.max() < A.shape[1]


def _freeze(A):
    A.has_sorted_indices = False
    for arr in (A.data, A.indices, A.indptr):
        arr.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def rect(n_cols):
    """fixture A over n_cols columns (checked, loop == scipy proved, read-only)"""
    lens = lengths_a()
    a = n_cols // N_A + 1
    indptr, indices, _ = pattern(lens, n_cols, a, n_cols - 1 - a)      # row 1's only entry: the last column
    rng = np.random.default_rng(61)
    A = sparse.csr_matrix((rng.normal(size=indptr[-1]), indices, indptr), shape=(N_A, n_cols))
    _freeze(A)
    check_pattern(A, lens, range(N_A))
    assert A.indices[A.indptr[1]] == n_cols - 1 and A.indices.min() < n_cols // 100
    assert len(np.unique(A.indices // (n_cols // 16))) >= 16               # spread over the whole column range
    assert A.data.min() < 0 < A.data.max()
    assert sweep_ref.prove_products(A)
    return A


def _sample(n):
    hubs = np.arange(0, 64 * 18 * 3, 64)
    return np.concatenate([hubs, np.arange(1, 40), np.arange(n - 70, n), (n // 128) * 64 + np.arange(0, 64 * 18, 64)])


@functools.lru_cache(maxsize=None)
def square(n=N_B, positive=False):
    """fixture B (checked, loop == scipy proved, read-only).  positive: weights > 0, every row summing to 0.5 (sweep_ref.ladder's
    rule), for the stop-column forms; otherwise normal weights of both signs."""
    lens = lengths_b(n)
    indptr, indices, row = pattern(lens, n, 7919, 12345)
    rng = np.random.default_rng(62)
    if positive:
        v = rng.random(indptr[-1]) + 0.25
        data = 0.5 * v / np.bincount(row, weights=v, minlength=n)[row]
    else:
        data = rng.normal(size=indptr[-1])
    A = sparse.csr_matrix((data, indices, indptr), shape=(n, n))
    _freeze(A)
    if n == N_B:
        assert A.nnz == NNZ_B
    check_pattern(A, lens, _sample(n))
    if positive:
        sums = np.asarray(A.sum(axis=1)).ravel()
        assert A.data.min() > 0 and np.allclose(sums[lens > 0], 0.5, rtol=1e-12, atol=0) and np.all(sums[lens == 0] == 0)
    else:
        assert A.data.min() < 0 < A.data.max()
    assert sweep_ref.prove_products(A, C=2)
    return A


def operands(n_rows, n_cols, C, dtype, seed=63):
    """(u, Db) in `dtype`"""
    rng = np.random.default_rng([seed, C])
    u = rng.standard_normal(size=(n_cols, C), dtype=np.float32).astype(dtype)
    Db = rng.standard_normal(size=(n_rows, C), dtype=np.float32).astype(dtype)
    return u, Db


# ---- the stop-column runs on fixture B ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def stop_fixture():
    A = square(N_B, True)
    deg, vinf, w_unit = sweep_ref.stop_vectors(N_B)
    for arr in (deg, vinf, w_unit):
        arr.setflags(write=False)
    return A, deg, vinf, w_unit


def stop_db_seed(b):
    return 70 + b


@functools.lru_cache(maxsize=None)
def stop_run(C, b, k):
    """the restatement's run of fixture B with Db = sweep_ref.bias(C, seed = stop_db_seed(b)) and w0 = 2^k w_unit, in fp64"""
    A, deg, vinf, w_unit = stop_fixture()
    Db = sweep_ref.bias(C, n=N_B, seed=stop_db_seed(b))
    out = sweep_ref.poisson_sweeps(A, Db, 2.0 ** k * w_unit, deg, vinf, STOP_MIN, STOP_MAX, np.float64)
    out[0].setflags(write=False)
    return out
