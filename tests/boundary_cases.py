"""The cases of utils.boundary_statistic shared by tests/golden/make_golden_boundary.py, tests/test_boundary_host.py and
tests/test_gpu_boundary.py.

GOLDEN: the inputs whose reference results tests/golden/g25_boundary.npz stores.  Radius cases keep d <= 5 (above that the
reference's own second search wants a package that is not installed); kNN cases hand the reference the lists of its kdtree search.

device_cases(): the smallest shapes at which the kernels can go wrong, each a dict with X, the pattern (indptr, indices), the lists J
of the kNN mode (or None) and, where the public function can build the same graph, how to ask it (`r`, `knn`).  Results are not
stored: the restatement tests/boundary_ref.py is the reference, bit for bit."""
import os
import re

import numpy as np

import boundary_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (mode, n, d, r, seed); points uniform in the unit cube
GOLDEN = {
    'r_d1': ('radius', 300, 1, 0.03, 11),
    'r_d2': ('radius', 600, 2, 0.12, 12),
    'r_d3': ('radius', 500, 3, 0.25, 13),
    'r_d5': ('radius', 257, 5, 0.6, 14),
    # rows of exactly maxdeg - 1 entries whose terms are all negative: the reference's list is the row, no 0 joins the maximum
    'r_edge': ('radius', 14, 2, 0.45, 117),
    'k_d2': ('knn', 500, 2, 15, 21),
    'k_d3': ('knn', 400, 3, 10, 22),
    'k_d7': ('knn', 300, 7, 20, 23),
    'k_d20': ('knn', 257, 20, 30, 24),
}


def golden_points(name):
    mode, n, d, r, seed = GOLDEN[name]
    return np.random.default_rng(seed).random((n, d))


def plan_constants():
    """BSTAT_WAVE_ROW and BSTAT_SHORT_LANES as csrc/bstat_plan.h states them"""
    text = open(os.path.join(ROOT, 'graphlearning_amd', 'csrc', 'bstat_plan.h')).read()
    return tuple(int(re.search(r'static const int %s = (\d+);' % name, text).group(1)) for name in ('BSTAT_WAVE_ROW', 'BSTAT_SHORT_LANES'))


def _radius_case(X, r):
    indptr, indices = ref.ball_pattern(X, r)
    return {'X': X, 'indptr': indptr, 'indices': indices, 'J': None, 'r': r, 'knn': False}


def _knn_case(X, k):
    J, D = ref.knn_lists(X, k)
    indptr, indices = ref.knn_pattern(J, k)
    return {'X': X, 'indptr': indptr, 'indices': indices, 'J': J.astype(np.int32), 'D': D, 'r': k, 'knn': True}


def _radius_for_degree(X, deg):
    """a radius that gives about `deg` neighbours per vertex: halfway between two neighbouring pair distances"""
    import epsball_ref
    D2 = np.sort(epsball_ref.full_d2(X), axis=1)
    a, b = np.median(D2[:, deg]), np.median(D2[:, deg + 1])
    return float(np.sqrt(max((a + b) / 2, D2[:, 1].max() * 1.0001)))        # (and no vertex without a neighbour)


def clusters(sizes, seed=5, d=2, spread=1e-3):
    """Clusters of the given sizes, 1 apart, every cluster inside a ball of diameter below 4 * spread: with r = 0.01 a vertex of a
    cluster of m points has exactly m - 1 neighbours."""
    rng = np.random.default_rng(seed)
    parts = []
    for q, m in enumerate(sizes):
        P = rng.random((m, d)) * spread
        P[:, 0] += q
        parts.append(P)
    X = np.concatenate(parts)
    return X[rng.permutation(len(X))]


def hub(n=2001, seed=7, d=3):
    """A pattern no ball graph gives: row 0 holds every other vertex, every other row three vertices.  Radius-mode rules: row 0 is the
    one full row."""
    rng = np.random.default_rng(seed)
    X = rng.random((n, d))
    rows = [np.arange(1, n)]
    for i in range(1, n):
        m = rng.choice(n - 1, size=3, replace=False)
        m = np.sort(np.where(m >= i, m + 1, m))
        rows.append(m)
    indptr = np.concatenate(([0], np.cumsum([len(m) for m in rows]))).astype(np.int32)
    return {'X': X, 'indptr': indptr, 'indices': np.concatenate(rows).astype(np.int32), 'J': None, 'r': None, 'knn': False}


def no_self(n=300, d=3, k=10, seed=9):
    """kNN lists that never hold their own vertex (the k nearest OTHER points): every row of the graph has k entries.  Lists in which
    duplicate points crowd the vertex out give the same rows, but there every member sits on the vertex and the normal cancels to
    zero -- that is duplicates_knn below."""
    X = np.random.default_rng(seed).random((n, d))
    J, D = ref.knn_lists(X, k + 1)
    J, D = np.ascontiguousarray(J[:, 1:]), np.ascontiguousarray(D[:, 1:])
    indptr, indices = ref.knn_pattern(J, k)
    return {'X': X, 'indptr': indptr, 'indices': indices, 'J': J.astype(np.int32), 'D': D, 'r': k, 'knn': True}


def duplicates_knn(n=200, d=2, k=10, copies=40, seed=10):
    """`copies` points at (0.5, 0.25): more than k, so some of them are missing from their own lists, and all their neighbours sit on
    them -- the raw normal is exactly zero (every product is exact).  Returns (X, J, D, the lowest such vertex)."""
    X = np.random.default_rng(seed).random((n, d))
    X[60:60 + copies] = [0.5, 0.25][:d] + [0.125] * (d - 2)
    J, D = ref.knn_lists(X, k)
    return X, J, D, 60


def lattice(m=12):
    """an m x m grid with integer coordinates: the neighbours of an interior vertex balance exactly"""
    g = np.arange(m, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, indexing='ij'), axis=-1).reshape(-1, 2)


def device_cases():
    wave_row, _ = plan_constants()
    rng = np.random.default_rng(3)
    cases = {}
    X2 = rng.random((2, 2))
    cases['n2_radius'] = _radius_case(X2, 2.0)                       # maxdeg = 1: both rows full, nothing left, -inf
    cases['n2_knn'] = _knn_case(X2, 2)
    for n in (65, 257):
        X = rng.random((n, 2))
        cases['n%d_radius' % n] = _radius_case(X, _radius_for_degree(X, 12))
        cases['n%d_knn' % n] = _knn_case(X, 9)
    for d in (1, 7, 8, 9, 128, 129):                                 # where numpy's row sum changes its walk
        X = rng.random((301, d))
        cases['d%d_radius' % d] = _radius_case(X, _radius_for_degree(X, 20))
        cases['d%d_knn' % d] = _knn_case(X, 12)
    X = rng.random((300, 3))
    cases['k2'] = _knn_case(X, 2)
    cases['k61'] = _knn_case(X, 61)
    sizes = sorted({2, 64, 65, 66, wave_row, wave_row + 1, wave_row + 2})
    cases['lengths'] = _radius_case(clusters(sizes), 0.01)           # rows of 1, 63, 64, 65 and around the class threshold
    cases['full_rows'] = _radius_case(clusters([9, 9, 9, 5, 3]), 0.01)      # 27 full rows
    cases['hub'] = hub()
    cases['no_self'] = no_self()
    return cases
