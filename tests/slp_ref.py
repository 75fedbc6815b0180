"""Sparse label propagation restated from its contract, for the tests of ssl.sparse_label_propagation and
glx_slp_iterate: the primal-dual sweeps once entry by entry in Python floats and once vectorised in numpy, the set-up both share,
the names of the golden graphs and cases, and the seeded problems of the device tests.

The contract.  W canonical CSR (indices ascending, no duplicates, no stored zero), n rows, M entries e = (i, j, w).  Per entry
lam = expm1(-log1p(2 w - (1 - 1e-10))) + 1, per vertex gamma = degree ** -1, rev[e] = the entry (j, i) or -1.  u (n, k) and Y (M, k)
start at zero; every class column is on its own.  One iteration:

    vertex i:   s = +0.0; over row i in ascending column order: s = s + (Y[e] - (Y[rev[e]] if rev[e] >= 0 else 0.0)) * w[e]
                div = 2 * (s / 2);  u_new = u - (0.0 + gamma * div);  a labelled vertex takes its one-hot row (listed twice: the last)
                ut = 2 * u_new - u
    entry e:    y = Y[e] + (-(w * (ut[j] - ut[i]))) * lam;  Y[e] = sign(y) if |y| > 1 else y        (after ALL ut are written)

Every operation is rounded on its own (no fused multiply-add)."""
import os
import subprocess
import ctypes
import numpy as np
from scipy import sparse

GOLDEN_FILES = ('g16_slp.npz', 'g16_slp_2.npz')
GOLDEN_GRAPHS = ('blobs', 'blobs_dir', 'wide17', 'hub_diag', 'ball')
# case -> (graph, classes, T)
GOLDEN_CASES = {
    'blobs': ('blobs', 3, 100),
    'blobs_T1': ('blobs', 3, 1),
    'blobs_T0': ('blobs', 3, 0),
    'blobs_dir': ('blobs_dir', 3, 100),
    'wide17': ('wide17', 17, 40),
    'oneclass': ('blobs', 1, 10),
    'hub_diag': ('hub_diag', 3, 60),
    'ball': ('ball', 2, 100),
}


def canonical(W):
    """W as canonical CSR float64: duplicates summed, stored zeros removed, indices ascending."""
    W = sparse.csr_matrix(W, dtype=np.float64, copy=True)
    W.sum_duplicates()
    W.eliminate_zeros()
    W.sort_indices()
    return W


def reverse_index(indptr, indices):
    """rev[e] = the index of entry (j, i) for e = (i, j), -1 where W has none: a lookup of the key j * n + i among the (sorted) keys."""
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    cols = indices.astype(np.int64)
    keys = rows * n + cols
    want = cols * n + rows
    at = np.searchsorted(keys, want)
    at[at >= len(keys)] = 0
    found = keys[at] == want if len(keys) else np.zeros(0, dtype=bool)
    return np.where(found, at, -1).astype(np.int64)


def setup(W):
    """(indptr int64, indices int32, w, lam, gamma, rev) of a canonical W, by the element-wise calls of the contract."""
    W = canonical(W)
    n = W.shape[0]
    w = np.ascontiguousarray(W.data, dtype=np.float64)
    lam = np.expm1(-np.log1p(2 * w - (1 - 1e-10))) + 1.0
    gamma = (W * np.ones(n)) ** -1
    indptr = W.indptr.astype(np.int64)
    indices = W.indices.astype(np.int32)
    return indptr, indices, w, lam, gamma, reverse_index(indptr, indices)


def onehot_rows(n, ind, labels, k):
    """lab[i] = the label vertex i takes (-1: none); a vertex listed twice takes its last label."""
    lab = np.full(n, -1, dtype=np.int64)
    for q in range(len(ind)):
        lab[int(ind[q])] = int(labels[q])
    assert k < 1 or lab.max() < k
    return lab


def slp_python(W, ind, labels, T, k=None, cols=None):
    """Entry by entry, in Python floats.  Returns u (n, k), or its columns `cols` only (the class columns are independent)."""
    indptr, indices, w, lam, gamma, rev = setup(W)
    n, M = len(indptr) - 1, len(w)
    k = len(np.unique(labels)) if k is None else k
    lab = onehot_rows(n, ind, labels, k)
    indptr, indices, rev = indptr.tolist(), indices.tolist(), rev.tolist()
    w, lam, gamma = w.tolist(), lam.tolist(), gamma.tolist()
    cols = list(range(k)) if cols is None else list(cols)
    out = np.zeros((n, len(cols)))
    for at, c in enumerate(cols):
        u = [0.0] * n
        ut = [0.0] * n
        Y = [0.0] * M
        for _ in range(T):
            for i in range(n):
                s = 0.0
                for e in range(indptr[i], indptr[i + 1]):
                    r = rev[e]
                    s = s + (Y[e] - (Y[r] if r >= 0 else 0.0)) * w[e]
                div = 2 * (s / 2)
                new = u[i] - (0.0 + gamma[i] * div)
                if lab[i] >= 0:
                    new = 1.0 if lab[i] == c else 0.0
                ut[i] = 2 * new - u[i]
                u[i] = new
            for i in range(n):
                for e in range(indptr[i], indptr[i + 1]):
                    y = Y[e] + (-(w[e] * (ut[indices[e]] - ut[i]))) * lam[e]
                    if y > 1:
                        y = 1.0
                    elif y < -1:
                        y = -1.0
                    Y[e] = y
        out[:, at] = u
    return out


def slp_numpy(W, ind, labels, T, k=None, history=False, clamped=False, cols=None):
    """Vectorised: the rows padded to the longest and summed slot after slot.  Returns u (n, k); with `history` also the
    iterates (T, n, k); with `clamped` also the share of entries with |y| > 1 in the last iteration (nan for T = 0).  cols: these
    class columns only (the columns are independent)."""
    indptr, indices, w, lam, gamma, rev = setup(W)
    n, M = len(indptr) - 1, len(w)
    k = len(np.unique(labels)) if k is None else k
    lab = onehot_rows(n, ind, labels, k)
    deg = np.diff(indptr)
    rows = np.repeat(np.arange(n, dtype=np.int64), deg)
    slot_of = np.arange(M, dtype=np.int64) - indptr[rows]
    nbrs = indices.astype(np.int64)
    labelled = np.where(lab >= 0)[0]
    onehot = (lab[labelled, None] == np.arange(k)[None, :]).astype(np.float64)
    if cols is not None:
        onehot = np.ascontiguousarray(onehot[:, list(cols)])
        k = onehot.shape[1]
    slots = [np.where(slot_of == d)[0] for d in range(int(deg.max()) if M else 0)]
    has_rev = rev >= 0
    rev_at = np.where(has_rev, rev, 0)
    u = np.zeros((n, k))
    Y = np.zeros((M, k))
    hist = np.zeros((T, n, k)) if history else None
    share = float('nan')
    wc, lc, gc = w[:, None], lam[:, None], gamma[:, None]
    for t in range(T):
        term = (Y - np.where(has_rev[:, None], Y[rev_at], 0.0)) * wc
        s = np.zeros((n, k))
        for es in slots:
            s[rows[es]] = s[rows[es]] + term[es]
        div = 2 * (s / 2)
        new = u - (0.0 + gc * div)
        new[labelled] = onehot
        ut = 2 * new - u
        u = new
        y = Y + (-(wc * (ut[nbrs] - ut[rows]))) * lc
        big = np.abs(y) > 1
        Y = np.where(big, np.sign(y), y)
        share = float(big.mean()) if M else float('nan')
        if history:
            hist[t] = u
    res = (u,)
    if history:
        res += (hist,)
    if clamped:
        res += (share,)
    return res if len(res) > 1 else u


# ---- seeded problems of the device tests ---------------------------------------------------------------------------------------------

def _knn_weights(X, k, rng):
    """k nearest neighbours by all pairs (self excluded), weights in (0.05, 1]: a directed CSR matrix."""
    n = X.shape[0]
    D = ((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(D, np.inf)
    J = np.argsort(D, axis=1, kind='stable')[:, :k]
    I = np.repeat(np.arange(n), k)
    V = 0.05 + 0.95 * rng.random(n * k)
    return sparse.csr_matrix((V, (I, J.ravel())), shape=(n, n))


def _labels(rng, n, k, per_class=2):
    ind = rng.choice(n, size=k * per_class, replace=False)
    labels = np.tile(np.arange(k), per_class)
    return ind.astype(np.int64), labels.astype(np.int64)


_RANDOM = [(50, 1, 1), (400, 20, 30), (123, 3, 7), (257, 17, 16), (64, 10, 17), (333, 2, 25)]      # (n, classes, T) by seed


def random_problem(seed):
    """(W canonical CSR, train_ind, train_labels, classes, T): n 50 .. 400, symmetric for even seeds and directed for odd ones,
    diagonal entries when seed % 3 == 0, a training vertex listed twice (other label last) when seed % 2 == 1 and classes > 1."""
    n, k, T = _RANDOM[seed % len(_RANDOM)]
    rng = np.random.default_rng(1000 + seed)
    W = _knn_weights(rng.random((n, 2)), 4 + seed % 4, rng)
    if seed % 2 == 0:
        W = W.maximum(W.T)
    if seed % 3 == 0:
        d = np.zeros(n)
        d[::3] = 0.7
        W = W + sparse.diags(d)
    ind, labels = _labels(rng, n, k)
    if seed % 2 == 1 and k > 1:
        ind = np.concatenate([ind, ind[:1]])
        labels = np.concatenate([labels, [(labels[0] + 1) % k]])
    return canonical(W), ind, labels, k, T


def hub_problem(h):
    """300 vertices, symmetric 5-nearest-neighbour base graph; row 0 replaced by exactly h entries (columns 1 .. h).  3 classes, T 12."""
    n = 300
    rng = np.random.default_rng(77)
    W = _knn_weights(rng.random((n, 2)), 5, rng)
    W = W.maximum(W.T).tolil()
    W[0, :] = 0
    W[0, 1:h + 1] = 0.1 + 0.4 * rng.random(h)
    ind, labels = _labels(rng, n, 3)
    W = canonical(W.tocsr())
    assert W.indptr[1] == h
    return W, ind, labels, 3, 12


# ---- the host restatement behind csrc/slp_plan.h (tests/slp_plan_host.cpp) -------------------------------------------------------------

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_host_lib(tmp):
    """csrc/slp_plan.h compiled for the host: `g++ -O2 -ffp-contract=off` behind tests/slp_plan_host.cpp."""
    so = os.path.join(str(tmp), 'libslp_plan_host.so')
    subprocess.run(['g++', '-O2', '-ffp-contract=off', '-std=c++17', '-fPIC', '-shared', '-I' + os.path.join(ROOT, 'graphlearning_amd', 'csrc'),
                    '-o', so, os.path.join(ROOT, 'tests', 'slp_plan_host.cpp')], check=True)
    lib = ctypes.CDLL(so)
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    lib.slp_host_validate.argtypes = [i64, i64, vp, vp, vp, vp, vp, ctypes.c_int, i64, vp]
    lib.slp_host_validate.restype = ctypes.c_int
    lib.slp_host_reverse.argtypes = [i64, vp, vp, vp]
    lib.slp_host_reverse.restype = ctypes.c_int
    lib.slp_host_tiles.argtypes = [ctypes.c_int, vp, ctypes.c_int]
    lib.slp_host_tiles.restype = ctypes.c_int
    lib.slp_host_iterate.argtypes = [i64, i64, vp, vp, vp, vp, vp, ctypes.c_int, i64, vp, vp, i64, vp]
    lib.slp_host_iterate.restype = ctypes.c_int
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_validate(lib, indptr, indices, w, lam, gamma, C, ind):
    n, M = len(indptr) - 1, len(indices)
    return lib.slp_host_validate(n, M, _p(indptr), _p(indices), _p(w), _p(lam), _p(gamma), C, len(ind), _p(ind))


def host_reverse(lib, indptr, indices):
    rev = np.empty(len(indices), dtype=np.int32)
    rc = lib.slp_host_reverse(len(indptr) - 1, _p(indptr), _p(indices), _p(rev))
    assert rc == 0
    return rev


def host_tiles(lib, C):
    out = np.zeros(3 * 64, dtype=np.int32)
    nt = lib.slp_host_tiles(C, _p(out), 64)
    return out[:3 * nt].reshape(nt, 3)      # (first column, columns, padded record width)


def host_iterate(lib, W, ind, labels, T, k):
    indptr, indices, w, lam, gamma, _ = setup(W)
    n = len(indptr) - 1
    ind32 = np.ascontiguousarray(ind, dtype=np.int32)
    val = np.ascontiguousarray((np.asarray(labels)[:, None] == np.arange(k)[None, :]).astype(np.float64))
    u = np.empty((n, k))
    rc = lib.slp_host_iterate(n, len(w), _p(indptr), _p(indices), _p(w), _p(lam), _p(gamma), k, len(ind32), _p(ind32), _p(val), T, _p(u))
    assert rc == 0, rc
    return u
