"""Helpers of the active-learning tests: csrc/acq_plan.h compiled for the host, a plain-numpy restatement of its documented order, the
golden cases of tests/golden/g23_al.npz with the graphs and eigenpairs they borrow from g18_ck.npz and g19_eig.npz, and seeded
problems for the device calls."""
import ctypes
import os
import subprocess

import numpy as np

import eig_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_FILE = 'g23_al.npz'
VAR, SIGMA, MC, MCVAR = 0, 1, 2, 3
KINDS = {'var_opt': VAR, 'sigma_opt': SIGMA, 'model_change': MC, 'model_change_var_opt': MCVAR}
CONDITIONINGS = {'e11': 1e-11, 'e2': 1e-2}          # C = diag(1 / (evals + shift)): the documented one, and a tame one
ROUNDS = 10
FULL_ROUNDS = (0, 4, 9)          # rounds whose whole value vector and u are stored; every round stores its best TOP values
TOP = 6
GAMMA2 = 0.1 ** 2.               # the reference's default, not 0.01
# name -> graph, criterion, conditioning, batch size, candidates ('full' or a subset size), policy, seed of the first labels
GOLDEN_CASES = {}
for _g in eig_ref.GRAPHS:
    for _a in KINDS:
        for _c in CONDITIONINGS:
            GOLDEN_CASES['%s_%s_%s' % (_g, _a, _c)] = dict(graph=_g, acq=_a, cond=_c, batch=1, cand='full', policy='max', seed=0)
GOLDEN_CASES['blobs_var_opt_e2_batch5'] = dict(graph='blobs', acq='var_opt', cond='e2', batch=5, cand='full', policy='max', seed=1)
GOLDEN_CASES['moons_sigma_opt_e2_subset'] = dict(graph='moons', acq='sigma_opt', cond='e2', batch=1, cand=200, policy='max', seed=2)
GOLDEN_CASES['moons_var_opt_e2_prop'] = dict(graph='moons', acq='var_opt', cond='e2', batch=1, cand='full', policy='prop', seed=3)
UNC_CASE = 'moons_model_change_e2'          # the case whose u of round 0 the six methods of unc_sampling are recorded on
UNC_METHODS = ('norm', 'entropy', 'least_confidence', 'smallest_margin', 'largest_margin', 'unc_2norm')
FULL_N = 40                                # vertices of the full-storage cases
FULL_QUERIES = np.array([3, 17, 3])
SHAPE_M = (1, 2, 3, 63, 64, 65, 256)
SHAPE_N = (1, 63, 64, 65, 129)


def unc_candidates(n):
    return np.arange(0, n, 5)


def full_C(n):
    """a dense symmetric positive definite covariance that elementwise arithmetic defines: 1 / (1 + |i - j|), 2 on the diagonal"""
    i = np.arange(n)
    return 1. / (1. + np.abs(i[:, None] - i[None, :])) + np.eye(n)


def load_golden():
    out = eig_ref.load_golden()
    with np.load(os.path.join(ROOT, 'tests', 'golden', GOLDEN_FILE)) as z:
        out.update({k: z[k] for k in z.files})
    return out


def case_state(gold, name):
    """(W, truth, V, the start C, the first labelled vertices, their labels, the candidate subset or None) of a golden case"""
    case = GOLDEN_CASES[name]
    g = case['graph']
    W, truth = eig_ref.golden_graph(gold, g), gold['graph_%s_truth' % g]
    vals = gold['dec_%s_normalized_vals' % g]
    V = np.ascontiguousarray(gold['dec_%s_normalized_vecs' % g])
    C = np.diag(1. / (vals + CONDITIONINGS[case['cond']]))
    ind = first_labels(truth, case['seed'])
    subset = None
    if case['cand'] != 'full':
        rng = np.random.default_rng(300 + case['seed'])
        subset = np.sort(rng.choice(np.setdiff1d(np.arange(len(truth)), ind), size=case['cand'], replace=False))
    return W, truth, V, C, ind, truth[ind], subset


def first_labels(truth, seed):
    """one labelled vertex per class"""
    rng = np.random.default_rng(200 + seed)
    return np.array([rng.choice(np.where(truth == c)[0]) for c in np.unique(truth)])


def numpy_state(gold, name, r):
    key = 'case_%s_r%d_' % (name, r)
    return ('MT19937', gold[key + 'key'].astype(np.uint32), int(gold[key + 'pos']), int(gold[key + 'has_gauss']), float(gold[key + 'cached_gaussian']))


def reference_C(C, w, ip, gamma2=GAMMA2):
    """the reference's rank-one steps from its recorded C v (rows of w) and v.C v (ip): elementwise numpy, the same bits everywhere"""
    C = C.copy()
    for wk, ipk in zip(np.atleast_2d(w), np.atleast_1d(ip)):
        C -= np.outer(wk, wk) / (gamma2 + ipk)
    return C


def reference_C_sequence(gold, name):
    """[C after the first labels, C after round 0, ...] of the reference"""
    C = case_state(gold, name)[3]
    key = 'case_%s_' % name
    seq = [reference_C(C, gold[key + 'init_w'], gold[key + 'init_ip'])]
    for r in range(ROUNDS):
        seq.append(reference_C(seq[-1], gold[key + 'r%d_w' % r], gold[key + 'r%d_ip' % r]))
    return seq


def build_host_lib(tmp):
    """csrc/acq_plan.h compiled for the host: `g++ -O2 -ffp-contract=off` behind tests/acq_plan_host.cpp."""
    so = os.path.join(str(tmp), 'libacq_plan_host.so')
    subprocess.run(['g++', '-O2', '-ffp-contract=off', '-std=c++17', '-fPIC', '-shared', '-I' + os.path.join(ROOT, 'graphlearning_amd', 'csrc'),
                    '-o', so, os.path.join(ROOT, 'tests', 'acq_plan_host.cpp')], check=True)
    lib = ctypes.CDLL(so)
    vp, i64, f64, ci, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_int, ctypes.c_int32
    lib.acq_host_validate_state.argtypes = [i64, ci, vp, vp, f64]
    lib.acq_host_validate_cand.argtypes = [i64, ci, ci, vp, i64]
    lib.acq_host_tiling.argtypes = [ci, vp]
    lib.acq_host_tiling.restype = None
    lib.acq_host_compute_c.argtypes = [i64, ci, vp, vp, f64, ci, vp, i64, vp, vp]
    lib.acq_host_update_c.argtypes = [i64, ci, vp, vp, f64, vp, i64]
    lib.acq_host_greedy_c.argtypes = [i64, ci, vp, vp, f64, ci, vp, i64, i64, vp, vp]
    lib.acq_host_greedy_c.restype = i64
    lib.acq_host_better.argtypes = [f64, i32, f64, i32]
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i(a):
    return np.ascontiguousarray(a, dtype=np.int32).ravel()


def host_validate_state(lib, V, C, gamma2=GAMMA2, n=None, M=None):
    V, C = _f(V), _f(C)
    return lib.acq_host_validate_state(V.shape[0] if n is None else n, V.shape[1] if M is None else M, _p(V), _p(C), gamma2)


def host_validate_cand(lib, n, kind, cand, greedy=False):
    cand = _i(cand)
    return lib.acq_host_validate_cand(n, kind, int(greedy), _p(cand), len(cand))


def host_tiling(lib, M):
    out = np.zeros(3, dtype=np.int64)
    lib.acq_host_tiling(M, _p(out))
    return tuple(int(v) for v in out)


def host_compute(lib, V, C, kind, cand, unc=None, gamma2=GAMMA2):
    V, C, cand = _f(V), _f(C), _i(cand)
    unc = None if unc is None else _f(unc)
    vals = np.empty(len(cand))
    rc = lib.acq_host_compute_c(V.shape[0], V.shape[1], _p(V), _p(C), gamma2, kind, _p(cand), len(cand), _p(unc), _p(vals))
    if rc:
        raise ValueError('acq_plan.h refused the arrays: %d' % -rc)
    return vals


def host_update(lib, V, C, query, gamma2=GAMMA2):
    """the new C"""
    V, C, query = _f(V), _f(C).copy(), _i(query)
    rc = lib.acq_host_update_c(V.shape[0], V.shape[1], _p(V), _p(C), gamma2, _p(query), len(query))
    if rc:
        raise ValueError('acq_plan.h refused the arrays: %d' % -rc)
    return C


def host_greedy(lib, V, C, kind, cand, b, gamma2=GAMMA2):
    """(the code of acq_host_greedy_c, positions, values)"""
    V, C, cand = _f(V), _f(C), _i(cand)
    q, qv = np.full(max(b, 1), -1, dtype=np.int32), np.full(max(b, 1), np.nan)
    rc = lib.acq_host_greedy_c(V.shape[0], V.shape[1], _p(V), _p(C), gamma2, kind, _p(cand), len(cand), b, _p(q), _p(qv))
    return int(rc), q[:b], qv[:b]


# ---- the documented order in plain numpy: chains in ascending index, every operation rounded on its own ------------------------------

def numpy_terms(V, C, cand):
    X = V[np.asarray(cand, dtype=np.int64)]
    nc, M = X.shape
    w = np.zeros((nc, M))
    for b in range(M):
        w = w + C[None, :, b] * X[:, b, None]
    d, s1, s2 = np.zeros(nc), np.zeros(nc), np.zeros(nc)
    for a in range(M):
        d = d + X[:, a] * w[:, a]
        s1 = s1 + w[:, a]
        s2 = s2 + w[:, a] * w[:, a]
    return d, s1, s2


def numpy_compute(V, C, kind, cand, unc=None, gamma2=GAMMA2):
    d, s1, s2 = numpy_terms(V, C, cand)
    den = gamma2 + d
    with np.errstate(all='ignore'):
        if kind == SIGMA:
            return (s1 * s1) / den
        nrm = np.sqrt(s2)
        if kind == MC:
            return (unc * nrm) / den
        if kind == VAR:
            return (nrm * nrm) / den
        return (unc * (nrm * nrm)) / den


def numpy_update(V, C, query, gamma2=GAMMA2):
    C = C.copy()
    M = C.shape[0]
    for k in np.asarray(query, dtype=np.int64):
        v = V[k]
        w = np.zeros(M)
        for b in range(M):
            w = w + C[:, b] * v[b]
        ip = 0.0
        for a in range(M):
            ip = ip + v[a] * w[a]
        with np.errstate(all='ignore'):
            C = C - (w[:, None] * w[None, :]) / (gamma2 + ip)
    return C


def numpy_greedy(V, C, kind, cand, b, gamma2=GAMMA2):
    cand = np.asarray(cand, dtype=np.int64)
    left = np.ones(len(cand), dtype=bool)
    q, qv = [], []
    for _ in range(b):
        vals = numpy_compute(V, C, kind, cand, gamma2=gamma2)
        vals = np.where(left, vals, -np.inf)
        p = int(np.argmax(vals))          # the first maximum
        q.append(p)
        qv.append(vals[p])
        left &= cand != cand[p]
        C = numpy_update(V, C, [cand[p]], gamma2=gamma2)
    return np.array(q, dtype=np.int32), np.array(qv)


def random_problem(seed, n, M, ties=False):
    """V (n, M) of order 1 / sqrt(n) like eigenvectors, a symmetric positive C with a wide spectrum, candidates unsorted with repeats,
    a multiplier.  ties: every odd row of V repeats the row before it."""
    rng = np.random.default_rng(seed * 1000 + 7 * n + M)
    V = rng.standard_normal((n, M)) / np.sqrt(n)
    if ties:
        V[1::2] = V[0:2 * (n // 2):2]
    Q = rng.standard_normal((M, M)) * 0.1
    C = np.diag(1. / (np.sort(rng.random(M)) + 1e-3)) + Q @ Q.T
    cand = rng.integers(0, n, size=n + 3).astype(np.int32)
    unc = rng.random(len(cand))
    return V, C, cand, unc


def same_bits(a, b):
    return eig_ref.same_bits(np.asarray(a), np.asarray(b))


def rel_diff(a, b):
    """max |a - b| over max |b|"""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def top_gaps(vals, count):
    """the relative gaps between consecutive values among the best `count + 1`, relative to the largest"""
    s = np.sort(vals)[::-1][:count + 1]
    return (s[:-1] - s[1:]) / abs(s[0])
