"""Helpers of the eigensolver's tests: csrc/eig_plan.h compiled for the host as a backend of graphlearning_amd._eig.thick_restart
(the same driver the device runs), seeded graphs, scipy's svds as the independent reference, and the quantities the tests bound."""
import ctypes
import os
import subprocess

import numpy as np
from scipy import sparse, spatial
from scipy.sparse import linalg as splinalg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_FILE = 'g19_eig.npz'
CK_GOLDEN_FILE = 'g18_ck.npz'                  # the 600-vertex `blobs` graph is read from there, not stored twice
GRAPHS = ('blobs', 'moons')
DECOMPS = (('normalized', 50), ('randomwalk', 11), ('combinatorial', 10))
# (n, k) of the whole solves: n = m without restart and probe; m = 23; negative eigenvalues of large modulus at (64, 30) and (257, 100);
# m = 513, the widest basis; the fixture's size
SHAPES = [(20, 5), (25, 11), (64, 30), (257, 100), (1000, 256), (600, 11)]
NORMALIZATIONS = ('normalized', 'randomwalk', 'combinatorial')
QUANTITIES = ('vals', 'overlap', 'subspace', 'residual')


def build_host_lib(tmp):
    """csrc/eig_plan.h compiled for the host: `g++ -O2 -ffp-contract=off` behind tests/eig_plan_host.cpp."""
    so = os.path.join(str(tmp), 'libeig_plan_host.so')
    subprocess.run(['g++', '-O2', '-ffp-contract=off', '-std=c++17', '-fPIC', '-shared', '-I' + os.path.join(ROOT, 'graphlearning_amd', 'csrc'),
                    '-o', so, os.path.join(ROOT, 'tests', 'eig_plan_host.cpp')], check=True)
    lib = ctypes.CDLL(so)
    vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.eig_host_validate.argtypes = [i64, vp, vp, vp, i64]
    lib.eig_host_basis_size.argtypes = [i64, i64]
    lib.eig_host_basis_size.restype = i64
    lib.eig_host_device_bytes.argtypes = [i64, i64, i64]
    lib.eig_host_device_bytes.restype = i64
    lib.eig_host_create.argtypes = [i64, vp, vp, vp, ci, ctypes.POINTER(vp)]
    lib.eig_host_set_column.argtypes = [vp, ci, vp]
    lib.eig_host_orthonormalize.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_double)]
    lib.eig_host_run.argtypes = [vp, ci, ci, vp, vp]
    lib.eig_host_rotate.argtypes = [vp, vp, ci, ci]
    lib.eig_host_get_columns.argtypes = [vp, ci, ci, vp]
    lib.eig_host_destroy.argtypes = [vp]
    lib.eig_host_destroy.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def csr_arrays(A):
    return (np.ascontiguousarray(A.indptr, dtype=np.int64), np.ascontiguousarray(A.indices, dtype=np.int32),
            np.ascontiguousarray(A.data, dtype=np.float64))


def host_validate(lib, indptr, indices, data, m):
    indptr, indices, data = (np.ascontiguousarray(indptr, dtype=np.int64), np.ascontiguousarray(indices, dtype=np.int32),
                             np.ascontiguousarray(data, dtype=np.float64))
    return lib.eig_host_validate(len(indptr) - 1, _p(indptr), _p(indices), _p(data), m)


class HostBackend:
    """EigHost of csrc/eig_plan.h behind the backend interface of _eig.thick_restart; a refusal raises ValueError with its code."""

    def __init__(self, lib, A, m):
        self.lib, self.n, self.m = lib, A.shape[0], int(m)
        self._arrays = csr_arrays(A)
        self._h = ctypes.c_void_p()
        self._check(lib.eig_host_create(self.n, _p(self._arrays[0]), _p(self._arrays[1]), _p(self._arrays[2]), self.m, ctypes.byref(self._h)))
        self.calls = {'run': 0, 'rotate': 0}

    @staticmethod
    def _check(rc):
        if rc:
            raise ValueError(rc)

    def set_column(self, j, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.shape == (self.n,)
        self._check(self.lib.eig_host_set_column(self._h, j, _p(x)))

    def orthonormalize(self, j):
        norm = ctypes.c_double(0.0)
        self._check(self.lib.eig_host_orthonormalize(self._h, j, ctypes.byref(norm)))
        return norm.value

    def run(self, j0, j1):
        self.calls['run'] += 1
        alpha, beta = np.empty(max(j1 - j0, 1)), np.empty(max(j1 - j0, 1))
        self._check(self.lib.eig_host_run(self._h, j0, j1, _p(alpha), _p(beta)))
        return alpha, beta

    def rotate(self, Y, rows, keep):
        self.calls['rotate'] += 1
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        assert Y.shape == (rows, keep)
        self._check(self.lib.eig_host_rotate(self._h, _p(Y), rows, keep))

    def get_columns(self, j0, j1):
        out = np.empty((max(j1 - j0, 1), self.n))
        self._check(self.lib.eig_host_get_columns(self._h, j0, j1, _p(out)))
        return np.ascontiguousarray(out.T)

    def close(self):
        if self._h:
            self.lib.eig_host_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def host_decomp(lib, W, normalization, k, tol=0, m=None):
    """graph.eigen_decomp with the host backend in the device's place: (vals ascending, vecs (n, k), steps, restarts, probe)"""
    from graphlearning_amd import _eig
    _eig.check_weights(W, normalization, k)
    A, D, M = _eig.operator(W, normalization)
    n = W.shape[0]
    with HostBackend(lib, A, _eig.basis_size(n, k) if m is None else m) as backend:
        theta, steps, restarts, probe = _eig.thick_restart(backend, n, k, tol=tol, m=m)
        vecs = backend.get_columns(0, k)
    s = np.sqrt(np.maximum(theta, 0.0))
    vals = (1 - s) if M is None else (M - s)
    ind = np.argsort(vals, kind='stable')
    vals, vecs = vals[ind], vecs[:, ind]
    if normalization == 'randomwalk':
        vecs = D @ vecs
    return vals, vecs, steps, restarts, probe


# ---- graphs ----------------------------------------------------------------------------------------------------------------------------

def knn_graph(X, k):
    """a symmetric Gaussian kNN weight matrix (bit for bit symmetric, no diagonal), canonical CSR"""
    n = X.shape[0]
    dist, idx = spatial.cKDTree(X).query(X, k=k + 1)
    eps = dist[:, -1]
    rows = np.repeat(np.arange(n), k)
    cols = idx[:, 1:].ravel()
    w = np.exp(-4 * dist[:, 1:].ravel() ** 2 / np.repeat(eps, k) ** 2)
    W = sparse.coo_matrix((w, (rows, cols)), shape=(n, n)).tocsr()
    W = W.maximum(W.T).tocsr()                  # max(a, b) is the same number on both sides
    W.setdiag(0)
    W.eliminate_zeros()
    W.sort_indices()
    return W


def seeded_graph(n, seed=0, k=None):
    rng = np.random.default_rng(1000 + seed + n)
    X = rng.normal(size=(n, 3))
    return knn_graph(X, min(10, n - 2) if k is None else k)


def components_graph(parts, per, seed=0):
    """`parts` connected components of `per` vertices each: the eigenvalue 1 of D^-1/2 W D^-1/2 `parts`-fold"""
    rng = np.random.default_rng(2000 + seed)
    return sparse.block_diag([knn_graph(rng.normal(size=(per, 3)), 10) for _ in range(parts)]).tocsr()


def path_graph(n):
    """bipartite: the eigenvalues of A come in pairs +-lambda, which doubles every eigenvalue of A A"""
    W = sparse.diags([np.ones(n - 1), np.ones(n - 1)], [1, -1]).tocsr()
    W.sort_indices()
    return W


def complete_graph(n):
    return sparse.csr_matrix(np.ones((n, n)) - np.eye(n))


def two_moons(n, seed, noise=0.1):
    """sklearn's make_moons without sklearn"""
    rng = np.random.default_rng(seed)
    half = n // 2
    t1, t2 = np.linspace(0, np.pi, half), np.linspace(0, np.pi, n - half)
    X = np.vstack([np.column_stack([np.cos(t1), np.sin(t1)]), np.column_stack([1 - np.cos(t2), 1 - np.sin(t2) - 0.5])])
    return X + rng.normal(scale=noise, size=X.shape), np.concatenate([np.zeros(half, dtype=np.int64), np.ones(n - half, dtype=np.int64)])


# ---- the independent reference and the quantities that are bounded ------------------------------------------------------------------

def svds_reference(A, k):
    """(s descending, u (n, k)) of scipy.sparse.linalg.svds(A, k, tol=0): what the reference's eigen_decomp calls"""
    u, s, vt = splinalg.svds(A, k=k, tol=0)
    order = np.argsort(-s, kind='stable')
    return s[order], u[:, order]


def orthonormality(V):
    return float(np.abs(V.T @ V - np.eye(V.shape[1])).max())


def overlap_defect(V, Vref):
    """1 - |<v, v_ref>| per column, the largest"""
    return float((1 - np.abs(np.sum(V * Vref, axis=0)) / (np.linalg.norm(V, axis=0) * np.linalg.norm(Vref, axis=0))).max())


def subspace_defect(V, Uref):
    """|| U U^T V - V ||_2 with U an orthonormal basis of the reference's columns"""
    Q, _ = np.linalg.qr(Uref)
    Vn = V / np.linalg.norm(V, axis=0)
    return float(np.linalg.norm(Q @ (Q.T @ Vn) - Vn, 2))


def residual(A, s, V):
    """the largest of min(||A v - s v||, ||A v + s v||) over the columns, v scaled to length one: an eigenvalue of A is s or -s"""
    Vn = V / np.linalg.norm(V, axis=0)
    AV = A @ Vn
    return float(np.minimum(np.linalg.norm(AV - Vn * s, axis=0), np.linalg.norm(AV + Vn * s, axis=0)).max())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def load_golden():
    out = {}
    with np.load(os.path.join(ROOT, 'tests', 'golden', GOLDEN_FILE)) as z:
        out.update({k: z[k] for k in z.files})
    with np.load(os.path.join(ROOT, 'tests', 'golden', CK_GOLDEN_FILE)) as z:
        for part in ('indptr', 'indices', 'data', 'truth'):
            out['graph_blobs_' + part] = z['graph_blobs_' + part]
    return out


def golden_graph(gold, g):
    ip, ix, d = gold['graph_%s_indptr' % g], gold['graph_%s_indices' % g], gold['graph_%s_data' % g]
    n = len(ip) - 1
    return sparse.csr_matrix((d, ix.astype(np.int32), ip.astype(np.int32)), shape=(n, n))


def a_vectors(W, normalization, vecs):
    """the eigenvectors of A behind what eigen_decomp returns: 'randomwalk' hands out D^-1/2 v"""
    if normalization != 'randomwalk':
        return vecs
    return (W * np.ones(W.shape[0]))[:, None] ** 0.5 * vecs


def measure(W, normalization, vals, vecs, ref_vals, ref_vecs):
    """the four bounded quantities of one decomposition against the reference's: |vals - ref|, the overlap defect per column, the
    subspace defect and the residual || A v - lambda v ||"""
    from graphlearning_amd import _eig
    A, D, M = _eig.operator(W, normalization)
    V, U = a_vectors(W, normalization, vecs), a_vectors(W, normalization, ref_vecs)
    s = (1 - vals) if M is None else (M - vals)
    return {'vals': float(np.abs(vals - ref_vals).max()), 'overlap': overlap_defect(V, U), 'subspace': subspace_defect(V, U),
            'residual': residual(A, s, V)}


def without_diagonal(W):
    n = W.shape[0]
    return sparse.csr_matrix(W - sparse.spdiags(W.diagonal(), 0, n, n))


def poisson_spectral(vals, vecs, n, ind, labels, p=1, cutoff=10):
    """reference ssl.py:619-622, 682-688 on a finished decomposition"""
    k = len(np.unique(labels))
    onehot = np.zeros((len(labels), k))
    onehot[np.arange(len(labels)), labels] = 1
    source = np.zeros((n, k))
    source[ind] = onehot - np.mean(onehot, axis=0)
    V, lam = vecs[:, 1:], vals[1:]
    if p != 1:
        lam = lam ** p
    L = sparse.spdiags(1 / lam, 0, cutoff, cutoff)
    return V @ (L @ (V.T @ source))


def top_two_gap(prob):
    srt = np.sort(prob, axis=1)
    return float((srt[:, -1] - srt[:, -2]).min())


def prob_difference(prob, ref_prob):
    """max |prob - ref| over max |ref|: prob = V L^-p V^T source grows like lambda_2^-p (4.5e5 on two moons at p = 2), its error with it"""
    return float(np.abs(prob - ref_prob).max() / np.abs(ref_prob).max())
