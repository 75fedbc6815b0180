"""Dynamic label propagation restated in numpy, twice, for tests/test_dlp_host.py, tests/test_gpu_dlp.py and the fixture generator
tests/golden/make_golden_dlp.py.

`dense_loop` is the independent check: the reference's formula with the dense n x n array Pt (ssl.py:1328-1332).

`dlp_device_order` is the order the device documents (csrc/dlp_plan.h), vectorised: the unrolled recursion, every
operation rounded on its own, row sums entry by entry in stored order, the Gram matrices by the fixed-order sum of fixed_sum.h.  It
equals dlp_host_reference (csrc/dlp_plan.h, built on the host behind tests/dlp_plan_host.cpp) and the device bit for bit."""
import ctypes
import os
import subprocess
import numpy as np
from scipy import sparse

from ck_ref import _Rows, _partials, _finish, canonical, without_diagonal, predict      # noqa: F401  (shared with the centered kernel)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_FILE = 'g22_dlp.npz'
GRAPH_FILE = 'g18_ck.npz'           # the graphs are read from the centered-kernel fixture and not stored again
# case -> (graph of g18_ck.npz, seed of the training set, parameters that differ from the defaults)
GOLDEN_CASES = {
    'blobs': ('blobs', 0, {}), 'blobs_T6': ('blobs', 0, {'T': 6}), 'blobs_T4': ('blobs', 0, {'T': 4, 'alpha': 0.5, 'lam': 0.01}),
    'directed_T2': ('directed', 0, {'T': 2}), 'directed_T3': ('directed', 0, {'T': 3}), 'directed_T6': ('directed', 0, {'T': 6}),
    'ten_T2': ('ten', 0, {'T': 2}), 'ten_T6': ('ten', 0, {'T': 6}), 'tiny_T2': ('tiny', 0, {'T': 2}), 'tiny_T3': ('tiny', 0, {'T': 3})}
LINES_CASES = ('blobs_T6', 'tiny_T3')          # cases with the lines of an all_labels fit
MIN_GAP = 1e-6                                 # smallest top-two gap of a row, as a fraction of the largest entry
DEFAULTS = {'alpha': 0.05, 'lam': 0.1, 'T': 2}


def case_params(name):
    return dict(DEFAULTS, **GOLDEN_CASES[name][2])


def load_graphs():
    with np.load(os.path.join(ROOT, 'tests', 'golden', GRAPH_FILE)) as z:
        return {k: z[k] for k in z.files if k.startswith('graph_')}


def golden_graph(graphs, g):
    ip, ix, d = graphs['graph_%s_indptr' % g], graphs['graph_%s_indices' % g], graphs['graph_%s_data' % g]
    n = len(ip) - 1
    return sparse.csr_matrix((d, ix, ip), shape=(n, n)), graphs['graph_%s_truth' % g]


def training_set(truth, seed):
    """5 labels per class from np.random.default_rng(100 + seed)"""
    rng = np.random.default_rng(100 + seed)
    ind = np.concatenate([rng.choice(np.where(truth == c)[0], size=5, replace=False) for c in np.unique(truth)])
    return ind, truth[ind]


def onehot(labels, k):
    return (np.asarray(labels).astype(np.int64)[:, None] == np.arange(k)[None, :]).astype(np.float64)


def transition(W):
    """P = D^-1 W of W without its diagonal, by the reference's expressions, as canonical CSR: what the learner hands to the device"""
    W = without_diagonal(W)
    n = W.shape[0]
    d = W * np.ones(n)
    P = sparse.csr_matrix(sparse.spdiags(d ** -1, 0, n, n).tocsr() * W)
    P.sort_indices()
    return P


# ---- the reference's formula ---------------------------------------------------------------------------------------------------------

def dense_loop(P, ind, val, alpha=0.05, lam=0.1, T=2):
    """(u_T, [u_1 .. u_T]) with the dense n x n array"""
    P = np.array(sparse.csr_matrix(P).todense())
    n = P.shape[0]
    u = np.zeros((n, val.shape[1]))
    u[ind, :] = val
    Pt = np.copy(P)
    Id = np.identity(n)
    hist = []
    with np.errstate(all='ignore'):
        for _ in range(T):
            v = P @ u
            u = Pt @ u
            u[ind, :] = val
            Pt = P @ Pt @ np.transpose(P) + alpha * v @ np.transpose(v) + lam * Id
            hist.append(np.array(u))
    return np.array(u), hist


# ---- the device's documented order ---------------------------------------------------------------------------------------------------

def _gram(V, X):
    n, k = V.shape
    return _finish(_partials((V[:, :, None] * X[:, None, :]).reshape(n, k * k))).reshape(k, k)


def dlp_device_order(indptr, indices, data, ind, val, alpha=0.05, lam=0.1, T=2):
    """(u_T, hist (T, n, k)).  The CSR arrays are P; val (m, k) the training rows' values."""
    indptr, indices, data = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64), np.asarray(data, dtype=np.float64)
    n, k = len(indptr) - 1, val.shape[1]
    alpha, lam = np.float64(alpha), np.float64(lam)
    Pt = sparse.csr_matrix((data, indices, indptr), shape=(n, n)).T.tocsr()       # scipy's transpose lists ascending rows, as the plan's
    Pt.sort_indices()
    rows, trows = _Rows(indptr, indices, data), _Rows(Pt.indptr.astype(np.int64), Pt.indices.astype(np.int64), Pt.data)
    lab = np.full(n, -1, dtype=np.int64)
    lab[np.asarray(ind, dtype=np.int64)] = np.arange(len(ind))
    train = lab >= 0
    u = np.zeros((n, k))
    u[train] = val[lab[train]]
    V, hist = [], np.zeros((T, n, k))
    with np.errstate(all='ignore'):
        for t in range(T):
            if t <= T - 2:
                V.append(rows.product(u))
            Y = [u]
            for j in range(1, t + 1):
                Y.append(trows.product(Y[j - 1]))
            R = V[0] if (t == 0 and T >= 2) else rows.product(Y[t])
            for s in range(t):
                X = Y[t - 1 - s]
                G = _gram(V[s], X)
                g = np.zeros((n, k))
                for c in range(k):
                    g = g + V[s][:, c:c + 1] * G[c][None, :]
                R = (rows.product(R) + alpha * g) + lam * X
            u = np.array(R)
            u[train] = val[lab[train]]
            hist[t] = u
    return np.ascontiguousarray(u), hist


def row_gaps(u):
    """(rows that are exactly zero, the smallest top-two gap of the other rows as a fraction of the largest entry)"""
    zero = ~np.any(u != 0, axis=1)
    if u.shape[1] < 2 or zero.all():
        return zero, np.inf
    srt = np.sort(u[~zero], axis=1)
    return zero, float((srt[:, -1] - srt[:, -2]).min() / np.abs(u).max())


# ---- seeded problems -----------------------------------------------------------------------------------------------------------------

def random_problem(seed, n, k, deg=6, symmetric=False, hub=0, empty_rows=0, negative=0.1, exact=False, all_train=False):
    """(P as canonical CSR, ind, val (m, k)): a seeded random matrix without diagonal, 1 .. 2 deg - 1 entries per row (`exact`: deg in
    every row), values of about 1 / deg, a share `negative` of them below zero; `hub` > 0: row n // 2 stores exactly `hub` entries;
    the first `empty_rows` rows store none; `symmetric`: P + P^T."""
    rng = np.random.default_rng(2200 + seed)
    top = max(1, min(n - 1, deg if exact else 2 * deg - 1))
    cnt = np.full(n, min(deg, top)) if exact else rng.integers(1, top + 1, size=n)
    cnt = np.minimum(cnt, n - 1)
    cnt[:empty_rows] = 0
    gaps = rng.integers(1, max(2, (n - 1) // top + 1), size=(n, top))
    off = np.cumsum(gaps, axis=1)                                  # distinct offsets in [1, n - 1]: no diagonal, no duplicate
    keep = np.arange(top)[None, :] < cnt[:, None]
    r = np.broadcast_to(np.arange(n)[:, None], (n, top))[keep]
    c = ((np.arange(n)[:, None] + off) % max(n, 1))[keep]
    if hub:
        h = n // 2
        r, c = r[r != h], c[r != h]
        others = np.delete(np.arange(n), h)
        r = np.concatenate([r, np.full(hub, h)])
        c = np.concatenate([c, rng.choice(others, size=hub, replace=False)])
    data = (rng.random(len(r)) + 0.05) / deg
    data[rng.random(len(r)) < negative] *= -0.5
    P = sparse.csr_matrix((data, (r, c)), shape=(n, n))
    if symmetric:
        P = P + P.T
    P = without_diagonal(P)
    m = n if all_train else min(n, max(k, min(n // 3 + 1, 2 * k)))
    ind = rng.permutation(n)[:m]
    val = onehot(np.arange(m) % k, k)
    return P, ind.astype(np.int64), val


# ---- csrc/dlp_plan.h on the host -----------------------------------------------------------------------------------------------------

HOST_FLAGS = ['g++', '-O2', '-ffp-contract=off', '-std=c++17', '-I' + os.path.join(ROOT, 'graphlearning_amd', 'csrc')]
HOST_SOURCE = os.path.join(ROOT, 'tests', 'dlp_plan_host.cpp')


def build_host_lib(tmp):
    """csrc/dlp_plan.h compiled for the host: `g++ -O2 -ffp-contract=off` behind tests/dlp_plan_host.cpp."""
    so = os.path.join(str(tmp), 'libdlp_plan_host.so')
    subprocess.run(HOST_FLAGS + ['-fPIC', '-shared', '-o', so, HOST_SOURCE], check=True)
    lib = ctypes.CDLL(so)
    vp, i64, f64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
    lib.dlp_host_validate.argtypes = [i64, i64, vp, vp, vp, ctypes.c_int, i64, vp, f64, f64, i64]
    lib.dlp_host_validate.restype = ctypes.c_int
    lib.dlp_host_plan.argtypes = [i64, i64, vp, vp, vp, ctypes.c_int, i64, vp, i64, vp, vp, vp, vp, vp]
    lib.dlp_host_plan.restype = None
    lib.dlp_host_solve.argtypes = [i64, i64, vp, vp, vp, ctypes.c_int, i64, vp, vp, f64, f64, i64, vp, vp]
    lib.dlp_host_solve.restype = ctypes.c_int
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _arrays(indptr, indices, data, ind):
    return (np.ascontiguousarray(indptr, dtype=np.int64), np.ascontiguousarray(indices, dtype=np.int32),
            np.ascontiguousarray(data, dtype=np.float64), np.ascontiguousarray(ind, dtype=np.int32))


def host_validate(lib, indptr, indices, data, k, ind, alpha=0.05, lam=0.1, T=2):
    indptr, indices, data, ind = _arrays(indptr, indices, data, ind)
    return lib.dlp_host_validate(len(indptr) - 1, len(indices), _p(indptr), _p(indices), _p(data), k, len(ind), _p(ind), alpha, lam, T)


def host_plan(lib, indptr, indices, data, k, ind, T=2):
    """(P^T as a scipy CSR matrix built from the plan's arrays, lab, sizes)"""
    indptr, indices, data, ind = _arrays(indptr, indices, data, ind)
    n, M = len(indptr) - 1, len(indices)
    tptr, tcol, tval = np.zeros(n + 1, dtype=np.int64), np.zeros(M, dtype=np.int32), np.zeros(M)
    lab, sizes = np.zeros(n, dtype=np.int32), np.zeros(6, dtype=np.int64)
    lib.dlp_host_plan(n, M, _p(indptr), _p(indices), _p(data), k, len(ind), _p(ind), T, _p(tptr), _p(tcol), _p(tval), _p(lab), _p(sizes))
    return sparse.csr_matrix((tval, tcol, tptr), shape=(n, n)), lab, sizes


def host_solve(lib, indptr, indices, data, ind, val, alpha=0.05, lam=0.1, T=2, want_history=True):
    """dlp_host_reference: (u_T, hist (T, n, k) or None); ValueError if dlp_validate refuses"""
    indptr, indices, data, ind = _arrays(indptr, indices, data, ind)
    val = np.ascontiguousarray(val, dtype=np.float64)
    n, k = len(indptr) - 1, val.shape[1]
    u = np.empty((n, k))
    hist = np.empty((T, n, k)) if want_history else None
    rc = lib.dlp_host_solve(n, len(indices), _p(indptr), _p(indices), _p(data), k, len(ind), _p(ind), _p(val), alpha, lam, T, _p(u), _p(hist))
    if rc:
        raise ValueError('dlp_validate refused the arrays: %d' % -rc)
    return u, hist
