"""The numpy restatement of INCRES clustering (reference clustering.py:325-371) that the golden fixture, the host plan driver
(tests/incres_plan_host.cpp: csrc/incres_plan.h with plain loops in the kernels' place) and the device are compared with, the golden
cases, and the small graphs of the shape tests.  Every random number comes from numpy's global stream, every product is scipy's `P*F`."""
import ctypes
import os
import subprocess
import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_FILE = 'g21_incres.npz'
# name -> (graph, clusters, seed, keyword arguments).  A case that cannot be made to pass is replaced by another seed, not waived.
GOLDEN_CASES = {
    'blobs3': ('blobs', 3, 11, {}),
    'blobs3_fast': ('blobs', 3, 12, {'speed': 50, 'T': 20}),
    'blobs5': ('blobs', 5, 13, {}),
    'moons2': ('moons', 2, 14, {}),
}
LINES_CASE = 'blobs3_fast'
DENORMAL_MIN_NORMAL = 2.2250738585072014e-308


def transition(W):
    """P = W D^-1 exactly as the reference writes it: degree_matrix(p=-1), then the sparse product, rows left as csr_matmat stores them"""
    W = sparse.csr_matrix(W)
    n = W.shape[0]
    d = W * np.ones(n)
    D = sparse.spdiags(d ** -1, 0, n, n).tocsr()
    return W * D


def plant(n, k, seeds):
    F = np.zeros((n, k))
    for r in range(k):
        F[seeds[r], r] = 1
    return F


def grow(P, F, max_grow=None):
    """(F, sweeps) of `while np.min(F) == 0: F = P*F`; None for F when max_grow sweeps leave a zero"""
    sweeps = 0
    while np.min(F) == 0:
        if max_grow is not None and sweeps >= max_grow:
            return None, sweeps
        F = P * F
        sweeps += 1
    return F, sweeps


def step(P, k, seeds, max_grow=None):
    """one outer iteration from given seeds (k, m): (labels int64 or None at the cap, sweeps, the grown F)"""
    F, sweeps = grow(P, plant(P.shape[0], k, np.asarray(seeds)), max_grow)
    return (None if F is None else np.argmax(F, axis=1)), sweeps, F


def draw_seeds(u, k, m):
    """the reference's draws for one plant, cluster by cluster: (k, m) vertex indices"""
    seeds = np.empty((k, m), dtype=np.int64)
    J = np.arange(len(u))
    for r in range(k):
        I = u == r
        seeds[r] = J[I][np.random.choice(np.sum(I), m)]
    return seeds


def fit(W, k, speed=5, T=200, stepper=None):
    """the whole fit from numpy's global stream: (labels (T, n), sweeps (T), seeds per iteration).  stepper(seeds) -> (labels, sweeps)
    stands in for the numpy step (the host plan driver, the device)."""
    n = W.shape[0]
    Dm = max(int(speed * 1e-4 * n / k), 1)
    u = np.random.randint(0, k, size=n)
    P = transition(W)
    hist, counts, planted = [], [], []
    m = 1
    for _ in range(T):
        seeds = draw_seeds(u, k, m)
        if stepper is None:
            u, sweeps, _ = step(P, k, seeds)
        else:
            u, sweeps = stepper(seeds)
            u = np.asarray(u).astype(np.int64)
        hist.append(u)
        counts.append(sweeps)
        planted.append(seeds)
        m += Dm
    return np.array(hist), np.array(counts, dtype=np.int64), planted


# ---- graphs ------------------------------------------------------------------------------------------------------------------------------
def load_golden():
    import eig_ref
    out = eig_ref.load_golden()
    with np.load(os.path.join(ROOT, 'tests', 'golden', GOLDEN_FILE)) as z:
        out.update({key: z[key] for key in z.files})
    return out


def golden_graph(gold, g):
    import eig_ref
    return eig_ref.golden_graph(gold, g)


def ring_graph(n, seed=0, extra=2):
    """connected, with self loops (so not bipartite), symmetric, positive weights: a ring plus `extra` random chords per vertex"""
    rng = np.random.default_rng(500 + seed + n)
    rows, cols = [np.arange(n)], [np.arange(n)]
    if n > 1:
        rows.append(np.arange(n))
        cols.append((np.arange(n) + 1) % n)
        for _ in range(extra):
            rows.append(np.arange(n))
            cols.append(rng.integers(0, n, n))
    A = sparse.coo_matrix((rng.uniform(0.5, 1.5, sum(len(r) for r in rows)), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    W = sparse.csr_matrix(A.maximum(A.T))
    W.sort_indices()
    return W


def path_graph(n, loops=True):
    """the path 0 - 1 - .. - n-1 with unit weights; with self loops W is tridiagonal ones, without them the graph is bipartite"""
    diags = [np.ones(n - 1), np.ones(n - 1)] + ([np.ones(n)] if loops else [])
    W = sparse.diags(diags, [1, -1] + ([0] if loops else [])).tocsr()
    W.sort_indices()
    return W


def star_graph(n):
    """vertex 0 joined to everyone and to itself (a row of n entries; the loop makes the graph non-bipartite), the leaves' rows hold
    one entry"""
    A = sparse.lil_matrix((n, n))
    A[0, :] = 1
    A[:, 0] = 1
    W = A.tocsr()
    W.sort_indices()
    return W


# ---- the host build of csrc/incres_plan.h (tests/incres_plan_host.cpp) --------------------------------------------------------------------
def build_host_lib(tmp):
    so = os.path.join(str(tmp), 'libincres_plan_host.so')
    subprocess.run(['g++', '-O2', '-ffp-contract=off', '-std=c++17', '-fPIC', '-shared', '-I' + os.path.join(ROOT, 'graphlearning_amd', 'csrc'),
                    '-o', so, os.path.join(ROOT, 'tests', 'incres_plan_host.cpp')], check=True)
    lib = ctypes.CDLL(so)
    vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.incres_host_create.argtypes = [i64, vp, vp, vp, ci]
    lib.incres_host_create.restype = vp
    lib.incres_host_step.argtypes = [vp, vp, i64, i64, ci, vp, vp, vp]
    lib.incres_host_destroy.argtypes = [vp]
    lib.incres_host_destroy.restype = None
    lib.incres_host_constants.argtypes = [vp]
    lib.incres_host_constants.restype = None
    lib.incres_host_chunk_len.argtypes = [ci, i64, i64, i64, i64]
    lib.incres_host_chunk_len2.argtypes = [ci, ci, i64, i64, i64, i64]
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class HostIncres:
    """the plan driver with plain loops behind the interface of _hip.Incres.step; chunk = 0: the plan decides"""

    def __init__(self, lib, P, k, chunk=0):
        self.lib, self.n, self.k, self.chunk = lib, P.shape[0], k, chunk
        self.arrays = (np.ascontiguousarray(P.indptr, dtype=np.int32), np.ascontiguousarray(P.indices, dtype=np.int32),
                       np.ascontiguousarray(P.data, dtype=np.float64))
        self.h = lib.incres_host_create(self.n, *[_p(a) for a in self.arrays], k)
        self.last = None          # (slot, chunks of the last loop, sweeps enqueued in it)

    def step(self, seeds, max_grow=None):
        seeds = np.ascontiguousarray(seeds, dtype=np.int32)
        labels = np.full(self.n, -7, dtype=np.int32)
        sweeps = np.zeros(1, dtype=np.int64)
        info = np.zeros(4, dtype=np.float64)
        rc = self.lib.incres_host_step(self.h, _p(seeds), seeds.shape[1], 2 * self.n + 2 if max_grow is None else max_grow, self.chunk,
                                       _p(labels), _p(sweeps), _p(info))
        self.last = (int(info[0]), int(info[1]), int(info[2]))
        if rc:
            raise RuntimeError('capped after %d sweeps' % int(sweeps[0]))
        return labels, int(sweeps[0])

    def close(self):
        if self.h:
            self.lib.incres_host_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
