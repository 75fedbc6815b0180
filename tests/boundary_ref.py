"""utils.boundary_statistic restated in numpy (reference utils.py:18-114): one walk over the rows of a canonical CSR pattern with unit
weights, the contract that heads graphlearning_amd/csrc/bstat_plan.h operation by operation.  Two forms of the same arithmetic:
`statistic_rows`, one readable loop per vertex, and `statistic`, vectorised over the vertices (what the speed figures use as the CPU
baseline).  tests/test_boundary_host.py holds both to the reference's golden vectors and to each other; the GPU tests and the
stand-alone host program of the header are compared with them bit for bit.

The graphs are built here without a GPU: the ball graph by tests/epsball_ref.py, the kNN lists by scipy's cKDTree (the reference's
method='kdtree'), the directed kNN graph from the lists as weightmatrix.knn(kernel='uniform', symmetrize=False) leaves it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epsball_ref  # noqa: E402

ORDERS = ((False, True), (True, True), (True, False))      # (second_order, cutoff): first order, second with and without cutoff


class ZeroNormal(ValueError):
    """the raw normal of `vertex` has norm zero or not finite"""

    def __init__(self, vertex):
        ValueError.__init__(self, 'the normal of vertex %d has norm zero or not finite' % vertex)
        self.vertex = vertex


# ---- the graphs ---------------------------------------------------------------------------------------------------------------------

def ball_pattern(X, r):
    """(indptr, indices) int32 of weightmatrix.epsilon_ball(X, r, kernel='uniform')"""
    W = epsball_ref.epsilon_ball(np.ascontiguousarray(X, dtype=np.float64), r, kernel='uniform')
    return W.indptr.astype(np.int32), W.indices.astype(np.int32)


def knn_lists(X, k):
    """(J, D) of the reference's knnsearch(X, k, method='kdtree')"""
    from scipy.spatial import cKDTree
    D, J = cKDTree(X).query(X, k=k)
    return J.reshape(len(X), k), D.reshape(len(X), k)


def knn_pattern(J, k):
    """(indptr, indices) int32 of weightmatrix.knn(X, k, kernel='uniform', symmetrize=False, knn_data=(J, D)): row i holds the first k
    members of J[i] without i itself, ascending.  A member named twice would be a weight of 2: ValueError."""
    J = np.asarray(J)[:, :k]
    n = J.shape[0]
    rows = []
    for i in range(n):
        m = np.sort(J[i][J[i] != i])
        if (m[1:] == m[:-1]).any():
            raise ValueError('list %d names a vertex twice' % i)
        rows.append(m)
    indptr = np.concatenate(([0], np.cumsum([len(m) for m in rows])))
    return indptr.astype(np.int32), np.concatenate(rows).astype(np.int32)


# ---- one vertex at a time -----------------------------------------------------------------------------------------------------------

def _normals_rows(X, indptr, indices, second_order):
    n, d = X.shape
    deg = np.diff(indptr).astype(np.float64)
    a = 1.0 / deg                                                   # step 1
    nu = np.empty((n, d))
    for i in range(n):
        cols = indices[indptr[i]:indptr[i + 1]]
        dp = np.float64(0.0)
        y = np.zeros(d)
        if second_order:                                            # step 2
            for j in cols[::-1]:
                dp = dp + a[j]
            for j in cols:
                y = y + a[j] * X[j]
            y = y + (-dp) * X[i]
        else:                                                       # step 3
            for j in cols:
                dp = dp + 1.0
            placed = False
            for j in cols:
                if not placed and j > i:
                    y = y + (-dp) * X[i]
                    placed = True
                y = y + 1.0 * X[j]
            if not placed:
                y = y + (-dp) * X[i]
        norm = np.sqrt(np.sum(y * y))                               # step 4
        if not (norm > 0 and np.isfinite(norm)):
            raise ZeroNormal(i)
        nu[i] = y / norm
    return nu


def _term(X, nu, i, j, second_order, cutoff):
    V = X[i] - X[j]                                                 # step 5
    if not second_order:
        return np.sum(V * nu[i])
    h = (nu[i] + nu[j]) / 2
    if cutoff and not np.sum(nu[i] * nu[j]) > 0:
        h = nu[i]
    return np.sum(V * h)


def statistic_rows(X, indptr, indices, J=None, second_order=True, cutoff=True):
    """(T, nu) by the contract, vertex by vertex.  J (n, k): the lists of the kNN mode; None: the radius mode."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    n = X.shape[0]
    nu = _normals_rows(X, indptr, indices, second_order)
    maxdeg = int(np.diff(indptr).max())
    T = np.empty(n)
    for i in range(n):
        members = list(J[i]) if J is not None else list(indices[indptr[i]:indptr[i + 1]])
        full = J is None and len(members) == maxdeg
        if full:                                                    # step 7: without the farthest, the largest index among equals
            sq = epsball_ref.d2_tree(X[i], X[members])
            far = max(range(len(members)), key=lambda q: (sq[q], members[q]))
            del members[far]
        xd = [_term(X, nu, i, j, second_order, cutoff) for j in members]
        if J is None and len(members) < maxdeg - 1:                 # a masked-out member of the reference's maxdeg - 1 nearest
            xd.append(0.0)
        T[i] = np.max(xd) if xd else -np.inf                        # steps 6, 7
    return T + 0.0, nu                                              # step 8: -0.0 + 0.0 = +0.0


# ---- all vertices at once -----------------------------------------------------------------------------------------------------------

def _normals(X, indptr, indices, second_order):
    n, d = X.shape
    lens = np.diff(indptr).astype(np.int64)
    a = 1.0 / lens.astype(np.float64)
    rows = np.repeat(np.arange(n), lens)
    pos = np.arange(len(indices)) - np.repeat(indptr[:-1].astype(np.int64), lens)
    maxdeg = int(lens.max())
    # the chain of every row as (coefficient, vertex) by position: the neighbours ascending and the diagonal term where it belongs
    coef = np.zeros((n, maxdeg + 1))
    vert = np.zeros((n, maxdeg + 1), dtype=np.int64)
    used = np.zeros((n, maxdeg + 1), dtype=bool)
    dp = np.zeros(n)
    if second_order:
        for p in range(maxdeg - 1, -1, -1):                          # descending columns
            live = np.flatnonzero(lens > p)
            dp[live] = dp[live] + a[indices[indptr[live] + p]]
        slot = pos
        at = lens
    else:
        for p in range(maxdeg):
            live = np.flatnonzero(lens > p)
            dp[live] = dp[live] + 1.0
        at = np.bincount(rows, weights=(indices < rows), minlength=n).astype(np.int64)      # neighbours below i
        slot = pos + (pos >= at[rows])
    coef[rows, slot] = a[indices] if second_order else 1.0
    vert[rows, slot] = indices
    used[rows, slot] = True
    coef[np.arange(n), at] = -dp
    vert[np.arange(n), at] = np.arange(n)
    used[np.arange(n), at] = True
    y = np.zeros((n, d))
    for p in range(maxdeg + 1):
        live = np.flatnonzero(used[:, p])
        y[live] = y[live] + coef[live, p][:, None] * X[vert[live, p]]
    norms = np.sqrt(np.sum(y * y, axis=1))
    bad = np.flatnonzero(~((norms > 0) & np.isfinite(norms)))
    if len(bad):
        raise ZeroNormal(int(bad[0]))
    return y / norms[:, None]


def statistic(X, indptr, indices, J=None, second_order=True, cutoff=True, chunk=400000):
    """(T, nu): the same arithmetic as statistic_rows, vectorised over the vertices and the pairs"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    n = X.shape[0]
    indptr = np.asarray(indptr).astype(np.int64)
    indices = np.asarray(indices).astype(np.int64)
    nu = _normals(X, indptr, indices, second_order)
    if J is not None:
        k = J.shape[1]
        I, M = np.repeat(np.arange(n), k), np.asarray(J).reshape(-1).astype(np.int64)
        starts, lens = np.arange(n) * k, np.full(n, k)
        full = np.zeros(n, dtype=bool)
    else:
        lens = np.diff(indptr)
        I, M, starts = np.repeat(np.arange(n), lens), indices, indptr[:-1]
        full = lens == lens.max()
    xd = np.empty(len(I))
    for lo in range(0, len(I), chunk):
        i, j = I[lo:lo + chunk], M[lo:lo + chunk]
        V = X[i] - X[j]
        if second_order:
            nu2 = (nu[i] + nu[j]) / 2
            if cutoff:
                m = np.sum(nu[i] * nu[j], axis=1) > 0
                nu2 = np.where(m[:, None], nu2, nu[i])
        else:
            nu2 = nu[i]
        xd[lo:lo + chunk] = np.sum(V * nu2, axis=1)
    for i in np.flatnonzero(full):                                  # a full row goes without its farthest entry
        e0, e1 = starts[i], starts[i] + lens[i]
        sq = epsball_ref.d2_tree(X[i], X[M[e0:e1]])
        far = e1 - 1 - int(np.argmax(sq[::-1]))                     # the last of the equals: the largest column index
        xd[far] = -np.inf
    T = np.maximum.reduceat(xd, starts)
    if J is None:
        T = np.where(lens < lens.max() - 1, np.maximum(T, 0.0), T)  # a 0 only where the reference's list reaches outside the ball
    return T + 0.0, nu
