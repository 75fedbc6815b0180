"""utils.conjgrad of the reference (graphlearning/utils.py:483-532) restated in plain numpy, in fp64, fp32 or long double, and the
operators the conjugate-gradient tests solve with.  Independent of the library AND of oracle/ (tests/test_cg_ref_host.py pins the
fp64 form to oracle.gl_oracle.conjgrad bit for bit); the long-double form is what the tolerance mode is measured against.

Order of the additions: the operator is applied from the CSR arrays in entry order (scipy's csr_matvecs adds a row's entries in
that order, starting from zero), the column sums run down the rows one after the other (numpy's axis-0 reduction of an (n, C) array with C > 1).  A
single column is summed the same way here (`_colsum` pads it): the pairwise rule numpy applies to one contiguous column is the
oracle's business, not this file's.
"""
import numpy as np
from scipy import sparse

DTYPES = {'f64': np.float64, 'f32': np.float32, 'ld': np.longdouble}
EPS = {'f64': 2.0 ** -52, 'f32': 2.0 ** -23}


def _colsum(v):
    """sum over the rows, one row after the other (also for one column, which numpy alone would sum pairwise)"""
    if v.shape[1] == 1:
        return np.sum(np.concatenate([v, np.zeros_like(v)], axis=1), axis=0)[:1]
    return np.sum(v, axis=0)


class Operator:
    """A CSR matrix applied in entry order in any of the three number formats: y[i] = (((0 + a_i0 p_j0) + a_i1 p_j1) + ...), the order
    of scipy's csr_matvecs.  (np.add.reduceat over data[:, None] * p[indices] takes long double too, but it does not add a run's
    entries one after the other: its results differ from scipy's in the last bits.)  The k-th entries of all rows go in one step."""

    def __init__(self, A, dtype):
        A = sparse.csr_matrix(A)
        self.n = A.shape[0]
        self.dtype = dtype
        indptr = A.indptr.astype(np.int64)
        length = np.diff(indptr)
        data = A.data.astype(dtype)
        self.steps = []
        for k in range(int(length.max()) if self.n else 0):
            rows = np.flatnonzero(length > k)
            at = indptr[rows] + k
            self.steps.append((None if len(rows) == self.n else rows, data[at][:, None], A.indices[at].astype(np.int64)))

    def __call__(self, p):
        out = np.zeros(p.shape, dtype=self.dtype)
        for rows, a, cols in self.steps:
            if rows is None:
                out += a * p[cols]
            else:
                out[rows] += a * p[cols]
        return out


def conjgrad(A, b, x0=None, tol=1e-10, max_iter=1e5, dtype=np.float64, hold=None, r0=False):
    """-> (x, iterations, history): history[k] is the residual norm iteration k + 1 left (the reference's `err`; its last entry is
    what the reference returns, 1 when no iteration ran).  `b` is the right-hand side also when x0 is given (r = b - A x0), unless
    r0 says that `b` already IS that residual (what DeviceGraph.cg takes beside an x0).
    hold: rows on which A p is held at zero (Dirichlet rows of DeviceGraph.cg_groups; b must be zero there)."""
    op = A if isinstance(A, Operator) else Operator(A, dtype)
    b = np.asarray(b).astype(dtype)
    if b.ndim == 1:
        x, it, hist = conjgrad(op, b[:, None], None if x0 is None else np.asarray(x0)[:, None], tol, max_iter, dtype, hold, r0)
        return x[:, 0], it, hist

    def apply(v):
        y = op(v)
        if hold is not None:
            y[hold] = 0
        return y
    with np.errstate(all='ignore'):
        if x0 is None:
            x = np.zeros_like(b)
            r = b.copy()
        else:
            x = np.asarray(x0).astype(dtype).copy()
            r = b.copy() if r0 else b - apply(x)
        p = r.copy()
        rsold = _colsum(r ** 2)
        err = 1
        it = 0
        hist = []
        while (err > tol) and (it < max_iter):
            it += 1
            Ap = apply(p)
            alpha = rsold / _colsum(p * Ap)
            x += alpha * p
            r -= alpha * Ap
            rsnew = _colsum(r ** 2)
            err = np.sqrt(np.sum(rsnew))
            hist.append(err)
            p = r + (rsnew / rsold) * p
            rsold = rsnew
    return x, it, hist


def conjgrad_groups(A, B, group_cols, masks=None, x0=None, tol=1e-10, max_iter=1e5, dtype=np.float64):
    """Every group of `group_cols` columns solved as a system of its own (DeviceGraph.cg_groups): on its Dirichlet rows `masks[g]`
    B is zeroed and A p held at zero.  -> (X, iterations per group, history per group)."""
    op = A if isinstance(A, Operator) else Operator(A, dtype)
    B = np.asarray(B).astype(dtype)
    ng = B.shape[1] // group_cols
    assert ng * group_cols == B.shape[1]
    X = np.empty_like(B)
    its, hists = [], []
    for g in range(ng):
        cols = slice(g * group_cols, (g + 1) * group_cols)
        bg = B[:, cols].copy()
        hold = None
        if masks is not None and len(masks[g]):
            hold = np.asarray(masks[g], dtype=np.int64)
            bg[hold] = 0
        x, it, hist = conjgrad(op, bg, None if x0 is None else np.asarray(x0)[:, cols], tol, max_iter, dtype, hold)
        X[:, cols] = x
        its.append(it)
        hists.append(hist)
    return X, its, hists


def laplacian_plus(n, seed, tau=1.0):
    """diag(W 1 + tau) - W for a random symmetric W >= 0 with zero diagonal: eigenvalues in [tau, tau + 2 dmax]."""
    W = sparse.random(n, n, density=min(1.0, 8.0 / n), random_state=seed, format='csr')
    W = sparse.csr_matrix(W + W.T)
    W.setdiag(0)
    W.eliminate_zeros()
    d = np.asarray(W.sum(axis=1)).ravel() + tau
    A = sparse.csr_matrix(sparse.diags(d) - W)
    A.sort_indices()
    return A


def banded(n):
    """diagonals 4, -1, -1 and 0.5 at offsets +-997: strictly diagonally dominant"""
    off = 997
    parts = [np.full(n, 4.0), np.full(n - 1, -1.0), np.full(n - 1, -1.0)]
    where = [0, 1, -1]
    if n > off:
        parts += [np.full(n - off, 0.5), np.full(n - off, 0.5)]
        where += [off, -off]
    return sparse.csr_matrix(sparse.diags(parts, where))


HUB_EVERY, HUB_SHORT, HUB_LONG, HUB_WEIGHT = 4096, 70, 300, -0.001


def banded_hubs(n):
    """banded(n) plus symmetric couplings of -0.001 from every 4096th row h (as long as h + 4096 < n) to the rows h + 1500 + 7 j,
    j < 70 (even hubs) or j < 300 (odd hubs): far from the band, inside the hub's own stretch, so that no row is coupled to two
    hubs.  Hub rows have 75 / 305 entries (the first: 73), their partners 6; still strictly diagonally dominant (4 > 3 + 0.3)."""
    hubs = np.arange(0, n - HUB_EVERY, HUB_EVERY)
    count = np.where((hubs // HUB_EVERY) % 2 == 0, HUB_SHORT, HUB_LONG)
    h = np.repeat(hubs, count)
    j = np.arange(len(h)) - np.repeat(np.cumsum(count) - count, count)
    p = h + 1500 + 7 * j
    assert p.max() < n and (p - h).max() < HUB_EVERY
    H = sparse.csr_matrix((np.full(len(h), HUB_WEIGHT), (h, p)), shape=(n, n))
    A = sparse.csr_matrix(banded(n) + H + H.T)
    A.sort_indices()
    return A


def in_format(A, dtype):
    """the operator with every entry rounded to `dtype` (what a DeviceGraph of that dtype holds), as an fp64 CSR matrix"""
    A = sparse.csr_matrix(A).copy()
    A.data = A.data.astype(dtype).astype(np.float64)
    return A
