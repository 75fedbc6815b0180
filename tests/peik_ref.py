"""Shared by the p-eikonal tests and the golden maker: the fixture tests/golden/g26_peikonal.npz with the graphs it borrows from
g18_ck.npz (`blobs`, 600 vertices) and g19_eig.npz (`moons`, 500 vertices), the entry arrays the reference hands to its C extension,
its host preprocessing of a non-local boundary, and csrc/peik_plan.h compiled for the host (tests/peik_plan_host.cpp): the
restatement of the synchronous rounds that the device must equal."""
import ctypes
import os
import subprocess
import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_FILE = 'g26_peikonal.npz'
BORROWED = {'blobs': 'g18_ck.npz', 'moons': 'g19_eig.npz'}       # read from there, not stored again
ECAP = 12                                                        # PEIK_ECAP of csrc/peik_plan.h
HOST_FLAGS = ['g++', '-O2', '-ffp-contract=off', '-std=c++17']


def load_golden():
    out = {}
    for g, fn in BORROWED.items():
        with np.load(os.path.join(ROOT, 'tests', 'golden', fn)) as z:
            for k in ('indptr', 'indices', 'data', 'truth'):
                out['graph_%s_%s' % (g, k)] = z['graph_%s_%s' % (g, k)]
    path = os.path.join(ROOT, 'tests', 'golden', GOLDEN_FILE)
    if os.path.exists(path):
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    return out


def graph(gold, name):
    indptr = gold['graph_%s_indptr' % name]
    n = len(indptr) - 1
    return sparse.csr_matrix((gold['graph_%s_data' % name].astype(np.float64), gold['graph_%s_indices' % name], indptr), shape=(n, n))


def entries(W):
    """(row_ptr, neighbour, weight): the arrays of the reference's __ccode_init__ (graph.py:69-84, the same expressions), with row
    pointers that are right also where a vertex has no entry"""
    I, J, V = sparse.find(W)
    ind = np.argsort(I)
    I, J, V = I[ind], J[ind], V[ind]
    row_ptr = np.concatenate(([0], np.cumsum(np.bincount(I, minlength=W.shape[0])))).astype(np.int64)
    return row_ptr, np.ascontiguousarray(J, dtype=np.int32), np.ascontiguousarray(V, dtype=np.float64)


def dilate(W, bdy_set, bdy_val):
    """the reference's nl_bdy preprocessing (graph.py:891-901), the same scipy expressions"""
    n = W.shape[0]
    d = W * np.ones(n)
    D = sparse.spdiags(d ** (-1.0), 0, n, n).tocsr()
    bdy_mask = np.zeros(n)
    bdy_mask[bdy_set] = 1
    bdy_dilate = (D * W * bdy_mask) > 0
    new_set = np.where(bdy_dilate)[0]
    bdy_val_all = np.zeros(n)
    bdy_val_all[bdy_mask == 1] = bdy_val
    return new_set, (D * W * bdy_val_all)[new_set]


def case_names(gold):
    return [str(s) for s in gold['case_names']]


def case(gold, name):
    """the inputs and the recorded results of a golden case"""
    c = {k: gold['case_%s_%s' % (name, k)] for k in ('bdy', 'g', 'f', 'u', 'u0')}
    c.update(graph=str(gold['case_%s_graph' % name]), p=float(gold['case_%s_p' % name]), nbis=int(gold['case_%s_nbis' % name]),
             nl_bdy=bool(gold['case_%s_nl_bdy' % name]), rounds=int(gold['case_%s_rounds' % name]),
             has_u0=bool(gold['case_%s_has_u0' % name]), exact=bool(gold['case_%s_exact' % name]))
    return c


def bound(gold, p, nbis):
    """16 x the recorded distance between the restatement and the reference, relative to max |u|, of the (p, num_bisection_it) class"""
    for q in range(len(gold['class_p'])):
        if float(gold['class_p'][q]) == float(p) and int(gold['class_nbis'][q]) == int(nbis):
            return float(gold['class_bound'][q])
    raise KeyError((p, nbis))


def build_host_lib(tmp):
    """csrc/peik_plan.h compiled for the host: `g++ -O2 -ffp-contract=off` behind tests/peik_plan_host.cpp."""
    so = os.path.join(str(tmp), 'libpeik_plan_host.so')
    subprocess.run(HOST_FLAGS + ['-fPIC', '-shared', '-o', so, os.path.join(ROOT, 'tests', 'peik_plan_host.cpp')], check=True)
    lib = ctypes.CDLL(so)
    vp, i64, f64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_int
    lib.peik_host_validate.argtypes = [i64, i64, vp, vp, vp, vp, ci, vp, vp, vp, f64, ci, vp]
    lib.peik_host_validate.restype = ci
    lib.peik_host_solve.argtypes = [i64, i64, vp, vp, vp, vp, ci, vp, vp, vp, f64, ci, vp, i64, vp, vp]
    lib.peik_host_solve.restype = ci
    lib.peik_host_constants.argtypes = [vp]
    lib.peik_host_constants.restype = None
    return lib


def build_host_exe(tmp, name, extra=()):
    exe = os.path.join(str(tmp), name)
    subprocess.run(HOST_FLAGS + list(extra) + ['-DPEIK_PLAN_MAIN', '-o', exe, os.path.join(ROOT, 'tests', 'peik_plan_host.cpp')], check=True)
    return exe


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def boundary_lists(bdy_sets, bdy_vals):
    ptr = np.concatenate(([0], np.cumsum([len(s) for s in bdy_sets]))).astype(np.int64)
    idx = np.ascontiguousarray(np.concatenate([np.asarray(s) for s in bdy_sets]), dtype=np.int32)
    val = np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=np.float64) * np.ones(len(s)) for s, v in zip(bdy_sets, bdy_vals)]))
    return ptr, idx, val


def host_arrays(n, row_ptr, nbr, V, f, bdy_sets, bdy_vals, u0):
    f = np.ascontiguousarray(np.ones(n) * f, dtype=np.float64)
    u0 = np.zeros(n) if u0 is None else np.ascontiguousarray(u0, dtype=np.float64)
    ptr, idx, val = boundary_lists(bdy_sets, bdy_vals)
    return (np.ascontiguousarray(row_ptr, dtype=np.int64), np.ascontiguousarray(nbr, dtype=np.int32),
            np.ascontiguousarray(V, dtype=np.float64), f, ptr, idx, val, u0)


def host_validate(lib, n, row_ptr, nbr, V, f, bdy_sets, bdy_vals, p, nbis, u0=None, B=None, M=None):
    row_ptr, nbr, V, f, ptr, idx, val, u0 = host_arrays(n, row_ptr, nbr, V, f, bdy_sets, bdy_vals, u0)
    return lib.peik_host_validate(n, len(nbr) if M is None else M, _p(row_ptr), _p(nbr), _p(V), _p(f), len(bdy_sets) if B is None else B,
                                  _p(ptr), _p(idx), _p(val), float(p), int(nbis), _p(u0))


def host_solve(lib, W, f, bdy_sets, bdy_vals, p, nbis, u0=None, max_rounds=0):
    """the rounds of csrc/peik_plan.h on the host: (status, u (n, B), rounds)"""
    n = W.shape[0]
    row_ptr, nbr, V, f, ptr, idx, val, u0 = host_arrays(n, *entries(W), f, bdy_sets, bdy_vals, u0)
    u = np.empty((n, len(bdy_sets)))
    rounds = ctypes.c_int64(0)
    rc = lib.peik_host_solve(n, len(nbr), _p(row_ptr), _p(nbr), _p(V), _p(f), len(bdy_sets), _p(ptr), _p(idx), _p(val), float(p), int(nbis),
                             _p(u0), int(max_rounds), _p(u), ctypes.byref(rounds))
    return rc, u, int(rounds.value)


def case_problem(gold, name):
    """(W, boundary set, boundary values, f, u0 or None) as the solver sees them: a non-local boundary already dilated"""
    c = case(gold, name)
    W = graph(gold, c['graph'])
    bdy, g = c['bdy'].astype(np.int64), c['g']
    if c['nl_bdy']:
        bdy, g = dilate(W, bdy, g)
    f = c['f'] if c['f'].ndim else float(c['f'])
    return c, W, bdy, g, f, (c['u0'] if c['has_u0'] else None)
