"""Helpers of the multiclass MBO learner's tests: csrc/mmbo_plan.h compiled for the host, a plain-numpy form of the reference's loop
(ssl.py:989-996), the golden cases of tests/golden/g20_mmbo.npz with the graphs and eigenpairs they borrow from g18_ck.npz and
g19_eig.npz, and seeded problems for the device call."""
import ctypes
import os
import subprocess

import numpy as np

import eig_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_FILE = 'g20_mmbo.npz'
DEFAULTS = dict(Ns=6, T=10, dt=0.15, mu=50, num_eig=50)
# name -> (graph, seed, what differs from the defaults); the seed gives the training set and, in the maker, np.random.seed before fit
GOLDEN_CASES = {}
for _g in eig_ref.GRAPHS:
    for _s in (0, 1, 2):
        GOLDEN_CASES['%s_s%d' % (_g, _s)] = (_g, _s, {})
    GOLDEN_CASES['%s_short' % _g] = (_g, 3, dict(Ns=3, T=4, dt=0.3, mu=10))
    GOLDEN_CASES['%s_eig20' % _g] = (_g, 4, dict(num_eig=20))
LINES_CASES = ('blobs_s0', 'moons_s0')           # the cases whose all_labels lines are recorded
MIN_GAP = 1e-6
CAP = 4096


def case_params(name):
    return dict(DEFAULTS, **GOLDEN_CASES[name][2])


def load_golden():
    """g20_mmbo.npz with the graphs and the ('normalized', 50) eigenpairs of g19_eig.npz / g18_ck.npz beside it"""
    out = eig_ref.load_golden()
    with np.load(os.path.join(ROOT, 'tests', 'golden', GOLDEN_FILE)) as z:
        out.update({k: z[k] for k in z.files})
    return out


def golden_eigenpairs(gold, name):
    """the stored eigenpairs of the case's graph: the lowest num_eig of the 50 of g19_eig.npz"""
    g = GOLDEN_CASES[name][0]
    m = case_params(name)['num_eig']
    return gold['dec_%s_normalized_vals' % g][:m].copy(), np.ascontiguousarray(gold['dec_%s_normalized_vecs' % g][:, :m])


def numpy_state(gold, name):
    """numpy's global state at the reference's draw of the random labelling, for np.random.set_state"""
    return ('MT19937', gold['case_%s_key' % name].astype(np.uint32), int(gold['case_%s_pos' % name]), int(gold['case_%s_has_gauss' % name]),
            float(gold['case_%s_cached_gaussian' % name]))


def start_labels(u, ind, labels):
    """the learner's start: argmax over the classes of ONE rand(k, n), the training vertices overwritten"""
    lab0 = np.argmax(u, axis=0).astype(np.int32)
    lab0[ind] = labels
    return lab0


def build_host_lib(tmp):
    """csrc/mmbo_plan.h compiled for the host: `g++ -O2 -ffp-contract=off` behind tests/mmbo_plan_host.cpp."""
    so = os.path.join(str(tmp), 'libmmbo_plan_host.so')
    subprocess.run(['g++', '-O2', '-ffp-contract=off', '-std=c++17', '-fPIC', '-shared', '-I' + os.path.join(ROOT, 'graphlearning_amd', 'csrc'),
                    '-o', so, os.path.join(ROOT, 'tests', 'mmbo_plan_host.cpp')], check=True)
    lib = ctypes.CDLL(so)
    vp, i64, f64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_int
    lib.mmbo_host_validate.argtypes = [i64, ci, vp, vp, vp, i64, vp, vp, ci, i64, i64, f64, f64]
    lib.mmbo_host_validate.restype = ci
    lib.mmbo_host_solve.argtypes = [i64, ci, vp, vp, vp, i64, vp, vp, ci, i64, i64, f64, f64, vp, vp, vp]
    lib.mmbo_host_solve.restype = ci
    lib.mmbo_host_partials.argtypes = [i64, vp, i64]
    lib.mmbo_host_partials.restype = i64
    lib.mmbo_host_sub_rows.argtypes = [ci, ci, vp]
    lib.mmbo_host_sub_rows.restype = ci
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _arrays(X, vals, lab0, ind, lab):
    return (np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(vals, dtype=np.float64), np.ascontiguousarray(lab0, dtype=np.int32),
            np.ascontiguousarray(ind, dtype=np.int32), np.ascontiguousarray(lab, dtype=np.int32))


def host_validate(lib, X, vals, lab0, ind, lab, k, Ns=6, T=10, dt=0.15, mu=50.0, n=None, m=None):
    X, vals, lab0, ind, lab = _arrays(X, vals, lab0, ind, lab)
    return lib.mmbo_host_validate(X.shape[0] if n is None else n, X.shape[1] if m is None else m, _p(X), _p(vals), _p(lab0), len(ind), _p(ind),
                                  _p(lab), k, Ns, T, dt, mu)


def host_solve(lib, X, vals, lab0, ind, lab, k, Ns=6, T=10, dt=0.15, mu=50.0):
    """mmbo_host_reference: (labels (T, n) int32, the last Z (k, m), the smallest top-two gap of all projections); ValueError if
    mmbo_validate refuses"""
    X, vals, lab0, ind, lab = _arrays(X, vals, lab0, ind, lab)
    n, m = X.shape
    hist = np.empty((T, n), dtype=np.int32)
    Z = np.empty((k, m))
    gap = np.zeros(1)
    rc = lib.mmbo_host_solve(n, m, _p(X), _p(vals), _p(lab0), len(ind), _p(ind), _p(lab), k, Ns, T, dt, mu, _p(hist), _p(Z), _p(gap))
    if rc:
        raise ValueError('mmbo_validate refused the arrays: %d' % -rc)
    return hist, Z, float(gap[0])


def host_sub_rows(lib, k, m):
    """(rows of a partial the pass holds in LDS at a time, the bytes of LDS of that pass)"""
    lds = np.zeros(1, dtype=np.int64)
    return lib.mmbo_host_sub_rows(k, m, _p(lds)), int(lds[0])


def onehot(labels, k):
    return (np.asarray(labels)[:, None] == np.arange(k)[None, :]).astype(np.float64)


def numpy_loop(vals, X, lab0, ind, labels, k, Ns=6, T=10, dt=0.15, mu=50):
    """The reference's loop (ssl.py:972-996) in plain numpy from a given start labelling: (labels (T, n), the smallest top-two gap)."""
    n = X.shape[0]
    Y = X @ np.diag(1 / (1 + (dt / Ns) * vals))
    Xt = np.transpose(X)
    u = onehot(lab0, k).T
    J = np.zeros(n)
    K = np.zeros(n)
    J[ind] = 1
    K[ind] = labels
    K = onehot(K, k).T
    hist, gap = np.empty((T, n), dtype=np.int32), np.inf
    for i in range(T):
        for s in range(Ns):
            Z = (u - (dt / Ns) * mu * J * (u - K)) @ Y
            u = Z @ Xt
        if k >= 2:
            top = np.sort(u, axis=0)
            gap = min(gap, float((top[-1] - top[-2]).min()))
        hist[i] = np.argmax(u, axis=0)
        u = onehot(hist[i], k).T
    return hist, gap


def random_problem(seed, n, m, k, ntrain=None, zero_column=False, empty_class=False, tied_classes=False):
    """A seeded problem for the device call: X (n, m) of order 1 / sqrt(n) like eigenvectors, vals ascending in [0, 2), start labels,
    a training set.  tied_classes: classes 0 and 1 start and stay identical (the same start label never, the same training labels
    never: neither class is used at all), so u[0] == u[1] exactly wherever both are largest."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, m)) / np.sqrt(n)
    vals = np.sort(rng.random(m) * 2.0)
    if zero_column:
        X[:, m // 2] = 0.0
    lo = 2 if tied_classes else 0
    lab0 = rng.integers(lo, k, size=n).astype(np.int32) if k > lo else np.zeros(n, dtype=np.int32)
    if empty_class and k - lo >= 2:
        lab0[lab0 == k - 1] = lo
    ntrain = min(n, max(1, n // 10)) if ntrain is None else ntrain
    ind = rng.choice(n, size=ntrain, replace=False).astype(np.int32)
    lab = (rng.integers(lo, k, size=ntrain) if k > lo else np.zeros(ntrain)).astype(np.int32)
    return X, vals, lab0, ind, lab
