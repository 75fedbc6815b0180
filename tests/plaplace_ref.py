"""What the p-Laplace learner's tests share: the description of the fixtures tests/golden/g17_plaplace*.npz
(tests/golden/make_golden_plaplace.py), the oracle's C restatement of lp_iterate_main called on GIVEN entry lists (one column), the
host build of csrc/lp_plan.h with its chunked two-buffer schedule (tests/lp_plan_host.cpp), and the small problems whose columns stop at
different iterations."""
import ctypes
import os
import subprocess
import sys

import numpy as np
from scipy import sparse

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# name -> how the generator builds the graph and the training set (the fixtures hold the result)
GOLDEN_GRAPHS = {
    'blobs3': dict(n=2000, d=5, C=3, seed=19, k=8, symmetrize=True, per_class=4),
    'blobs10_dir': dict(n=1500, d=20, C=10, seed=20, k=6, symmetrize=False, per_class=2),
}

# name -> (graph, fast, p, tol, max_num_it)
GOLDEN_CASES = {
    'b3_fast_p10': ('blobs3', True, 10, 1e-1, 1e6),
    'b3_fast_p3': ('blobs3', True, 3, 1e-1, 1e6),
    'b3_jac_p10': ('blobs3', False, 10, 1e-1, 1e6),
    'b3_jac_p10_tol2': ('blobs3', False, 10, 1e-2, 1e6),
    'b3_jac_p3': ('blobs3', False, 3, 1e-1, 1e6),
    'b3_jac_T57': ('blobs3', False, 10, 1e-1, 57),
    'b3_jac_T200': ('blobs3', False, 10, 1e-1, 200),
    'b3_jac_T0': ('blobs3', False, 10, 1e-1, 0),
    'b10_fast_p10': ('blobs10_dir', True, 10, 1e-1, 1e6),
    'b10_jac_p10': ('blobs10_dir', False, 10, 1e-1, 1e6),
}
PRIORS_CASE = 'b3_jac_p10'          # also fitted with class_priors: `<case>_priors_pred`


def load_golden():
    gdir = os.path.join(HERE, 'golden')
    g = dict(np.load(os.path.join(gdir, 'g17_plaplace.npz'), allow_pickle=False))
    for fn in sorted(set(g['entry_files'].tolist())):
        if fn != 'g17_plaplace.npz':
            g.update(dict(np.load(os.path.join(gdir, fn), allow_pickle=False)))
    return g


def golden_graph(g, gname):
    n = len(g['graph_%s_indptr' % gname]) - 1
    return sparse.csr_matrix((g['graph_%s_data' % gname], g['graph_%s_indices' % gname], g['graph_%s_indptr' % gname]), shape=(n, n))


def golden_entries(g, gname):
    """(I, J, V) of the capturing host's __ccode_init__."""
    return (np.ascontiguousarray(g['graph_%s_I' % gname], dtype=np.int32), np.ascontiguousarray(g['graph_%s_J' % gname], dtype=np.int32),
            np.ascontiguousarray(g['graph_%s_V' % gname], dtype=np.float64))


def class_columns(train_labels):
    classes = np.unique(train_labels)
    return (train_labels[:, None] == classes[None, :]).astype(np.float64)


# ---- the oracle's restatement (oracle/csr_ref.c: ref_lp_iterate) on given entry lists ------------------------------------------------
def _oracle_lib():
    from oracle import gl_oracle as orc
    lib = orc._c_lib()
    lib.ref_lp_iterate.restype = ctypes.c_int64
    return lib


def start_values(n, ind, val):
    """(uu, ul) as graph.plaplace sets them up; without boundary vertices the fold's identity."""
    val = np.asarray(val, dtype=np.float64)
    hi, lo = (np.max(val), np.min(val)) if len(val) else (-np.inf, np.inf)
    uu = hi * np.ones(n)
    ul = lo * np.ones(n)
    uu[ind] = val
    ul[ind] = val
    return np.ascontiguousarray(uu), np.ascontiguousarray(ul)


def oracle_from(uu, ul, n, I, J, V, ind, val, p, T, tol):
    """(uu, ul, stopping iteration) of one column from the given start (copied, not written)."""
    vp = ctypes.c_void_p
    I = np.ascontiguousarray(I, dtype=np.int32)
    J = np.ascontiguousarray(J, dtype=np.int32)
    V = np.ascontiguousarray(V, dtype=np.float64)
    ind = np.ascontiguousarray(ind, dtype=np.int32)
    val = np.ascontiguousarray(val, dtype=np.float64)
    uu, ul = np.array(uu, dtype=np.float64), np.array(ul, dtype=np.float64)
    with np.errstate(all='ignore'):
        it = _oracle_lib().ref_lp_iterate(uu.ctypes.data_as(vp), ul.ctypes.data_as(vp), J.ctypes.data_as(vp), I.ctypes.data_as(vp),
                                          V.ctypes.data_as(vp), ind.ctypes.data_as(vp), val.ctypes.data_as(vp), ctypes.c_double(p),
                                          ctypes.c_int64(int(T)), ctypes.c_double(float(tol)), ctypes.c_int64(n), ctypes.c_int64(len(V)),
                                          ctypes.c_int64(len(ind)))
    return uu, ul, int(it)


def oracle_column(n, I, J, V, ind, val, p, T, tol):
    """(uu, ul, stopping iteration) of one column from the start graph.plaplace sets up."""
    uu, ul = start_values(n, ind, val)
    return oracle_from(uu, ul, n, I, J, V, ind, val, p, T, tol)


def oracle_batch(n, I, J, V, ind, vals, p, T, tol):
    cols = [oracle_column(n, I, J, V, ind, vals[:, b], p, T, tol) for b in range(vals.shape[1])]
    return (np.stack([c[0] for c in cols], axis=1), np.stack([c[1] for c in cols], axis=1), np.array([c[2] for c in cols], dtype=np.int64))


def same(a, b):
    """Bit for bit, NaN positions equal (a NaN's payload is not compared)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.where(na, 0.0, a).tobytes() == np.where(nb, 0.0, b).tobytes())


# ---- the host build of csrc/lp_plan.h (tests/lp_plan_host.cpp) -------------------------------------------------------------------------
def build_host_lib(outdir):
    out = os.path.join(str(outdir), 'liblpb.so')
    subprocess.run(['g++', '-O2', '-ffp-contract=off', '-shared', '-fPIC', '-o', out, os.path.join(HERE, 'lp_plan_host.cpp')], check=True)
    lib = ctypes.CDLL(out)
    vp, i64, dbl, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_int
    lib.lpb_constants.argtypes = [vp]
    lib.lpb_constants.restype = None
    lib.lpb_result_iterate.argtypes = [i64, i64]
    lib.lpb_result_iterate.restype = i64
    lib.lpb_plan.argtypes = [i64, i64, vp, vp, vp, ci, i64, vp, vp, dbl, i64, vp, vp, vp, vp, vp, vp]
    lib.lpb_run.argtypes = [i64, i64, vp, vp, vp, ci, i64, vp, vp, dbl, i64, dbl, ci, vp, vp, vp]
    return lib


def _p(a):
    return a.ctypes.data


def _args(I, J, V, ind, vals):
    return (np.ascontiguousarray(I, dtype=np.int32), np.ascontiguousarray(J, dtype=np.int32), np.ascontiguousarray(V, dtype=np.float64),
            np.ascontiguousarray(ind, dtype=np.int32), np.ascontiguousarray(vals, dtype=np.float64))


def host_constants(lib):
    out = np.zeros(4, dtype=np.int64)
    lib.lpb_constants(_p(out))
    return dict(block=int(out[0]), chunk=int(out[1]), lds_cols=int(out[2]), max_cols=int(out[3]))


def host_plan(lib, n, I, J, V, ind, vals, p, T=100):
    I, J, V, ind, vals = _args(I, J, V, ind, vals)
    B = vals.shape[1]
    start, invdeg, bdy = np.zeros(n + 1, dtype=np.int64), np.zeros(n), np.zeros(n, dtype=np.int32)
    hi, lo, scal = np.zeros(B), np.zeros(B), np.zeros(3)
    rc = lib.lpb_plan(n, len(V), _p(J), _p(I), _p(V), B, len(ind), _p(ind), _p(vals), float(p), int(T), _p(start), _p(invdeg), _p(bdy),
                      _p(hi), _p(lo), _p(scal))
    return rc, dict(start=start, invdeg=invdeg, bdy=bdy, hi=hi, lo=lo, alpha=scal[0], delta=scal[1], dt=scal[2])


def host_run(lib, n, I, J, V, ind, vals, p, T, tol, chunk=None):
    """(uu (n, B), ul (n, B), iters (B,)) of the chunked schedule on the host; chunk None: the library's constant."""
    I, J, V, ind, vals = _args(I, J, V, ind, vals)
    B = vals.shape[1]
    uu, ul, iters = np.zeros((n, B)), np.zeros((n, B)), np.zeros(B, dtype=np.int64)
    chunk = host_constants(lib)['chunk'] if chunk is None else int(chunk)
    rc = lib.lpb_run(n, len(V), _p(J), _p(I), _p(V), B, len(ind), _p(ind), _p(vals), float(p), int(T), float(tol), chunk, _p(uu), _p(ul),
                     _p(iters))
    assert rc == 0, rc
    return uu, ul, iters


# ---- small problems -----------------------------------------------------------------------------------------------------------------
def entries(W):
    """(I, J, V): the expressions of the reference's __ccode_init__ (graph.py:69-84)."""
    I, J, V = sparse.find(sparse.csr_matrix(W))
    o = np.argsort(I)
    return (np.ascontiguousarray(I[o], dtype=np.int32), np.ascontiguousarray(J[o], dtype=np.int32), np.ascontiguousarray(V[o], dtype=np.float64))


def random_graph(n, seed, dens=None):
    """Symmetric, connected along a ring, uneven weights."""
    A = sparse.random(n, n, density=dens if dens is not None else min(1.0, 6.0 / n), random_state=seed, format='csr')
    A = A + sparse.diags(np.full(n - 1, 0.5), 1, format='csr')
    A = sparse.csr_matrix(A + A.T)
    A.setdiag(0)
    A.eliminate_zeros()
    return A


def scaled_columns(rng, m, B):
    """One boundary vector scaled by 1, 1e-1, 1e-2, ...: the stop test is absolute, so the columns stop at different iterations."""
    base = rng.normal(size=m)
    return base[:, None] * (10.0 ** -(np.arange(B) % 6))[None, :]


def scaled_problem(B, n=400, seed=31):
    rng = np.random.default_rng(seed + B)
    W = random_graph(n, seed)
    ind = np.sort(rng.choice(n, size=n // 12, replace=False))
    return W, ind, scaled_columns(rng, len(ind), B)


def constant_problem(B, n=300, seed=32):
    """Every column constant on the boundary (column b: the value b + 0.5): the gap is zero from the start, the stop comes at
    iteration 11 exactly."""
    rng = np.random.default_rng(seed)
    W = random_graph(n, seed)
    ind = np.sort(rng.choice(n, size=20, replace=False))
    return W, ind, np.tile(np.arange(B) + 0.5, (len(ind), 1))
