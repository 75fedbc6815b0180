"""The graphs of the connected-components tests, shared by tests/test_components_host.py (numpy restatement against scipy) and
tests/test_gpu_components.py (device against scipy).  Every generator is seeded.  A case is (name, group, W): W a scipy CSR matrix
built from RAW arrays, so that unsorted rows, duplicates and stored zeros arrive as they were written.

Groups: 'random' (sizes around the wavefront and tile boundaries, mean degrees around the percolation threshold, eight storage
variants), 'diameter' (65 536 vertices: paths, ring, grid), 'hubs' (stars, a clique beside isolated vertices, rows around the
wavefront threshold of csrc/cc_plan.h), 'ties' (equal largest components, all isolated); 'package' graphs need the device and are
built by package_cases()."""
import os
import re

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RANDOM_N = (1, 2, 63, 64, 65, 257, 1000, 4097)
RANDOM_DEGREES = (0, 0.5, 1, 2, 4)
RANDOM_VARIANTS = ('symmetric', 'upper', 'asymmetric', 'unsorted_duplicates', 'stored_zeros', 'self_loops', 'empty_rows', 'no_entries')


def wave_row_threshold():
    """CC_WAVE_ROW of csrc/cc_plan.h: rows of at least this many stored entries take a wavefront"""
    text = open(os.path.join(ROOT, 'graphlearning_amd', 'csrc', 'cc_plan.h')).read()
    return int(re.search(r'static const int CC_WAVE_ROW = (\d+);', text).group(1))


def csr_raw(n, rows, cols, vals=None):
    """CSR from entries in the order given: a row's entries keep their order (a stable sort by row), duplicates and zeros stay"""
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    vals = np.ones(len(rows)) if vals is None else np.asarray(vals, dtype=np.float64)
    order = np.argsort(rows, kind='stable')
    indptr = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
    W = sparse.csr_matrix((vals[order], cols[order].astype(np.int32), indptr), shape=(n, n))
    assert W.nnz == len(rows)          # nothing was merged or dropped
    return W


def both_ways(a, b):
    return np.concatenate([a, b]), np.concatenate([b, a])


def random_case(n, degree, variant, seed):
    rng = np.random.default_rng(seed)
    m = int(round(degree * n / 2))
    a, b = rng.integers(0, n, m), rng.integers(0, n, m)
    if variant == 'no_entries':
        a = b = np.zeros(0, dtype=np.int64)
    vals = None
    if variant in ('symmetric', 'stored_zeros', 'self_loops', 'unsorted_duplicates'):
        rows, cols = both_ways(a, b)
    elif variant == 'upper':
        rows, cols = np.minimum(a, b), np.maximum(a, b)
    else:                                               # asymmetric, empty_rows: one direction, as drawn
        rows, cols = a, b
    if variant == 'unsorted_duplicates' and len(rows):
        again = rng.integers(0, len(rows), len(rows) // 2)         # half the entries a second time, then everything shuffled
        rows, cols = np.concatenate([rows, rows[again]]), np.concatenate([cols, cols[again]])
        p = rng.permutation(len(rows))
        rows, cols = rows[p], cols[p]
    if variant == 'stored_zeros':
        vals = np.where(rng.random(len(rows)) < 0.5, 0.0, 1.0)
    if variant == 'self_loops':
        loops = rng.integers(0, n, max(1, n // 4))
        rows, cols = np.concatenate([rows, loops]), np.concatenate([cols, loops])
    if variant == 'empty_rows' and len(rows):
        keep = ~np.isin(rows, rng.integers(0, n, max(1, n // 3)))  # a third of the vertices store nothing; others may still name them
        rows, cols = rows[keep], cols[keep]
    return csr_raw(n, rows, cols, vals)


def random_cases(n):
    out = []
    for di, degree in enumerate(RANDOM_DEGREES):
        for vi, variant in enumerate(RANDOM_VARIANTS):
            if variant == 'no_entries' and di:
                continue                                 # one matrix without entries per size
            out.append(('random_n%d_deg%s_%s' % (n, degree, variant), 'random', random_case(n, degree, variant, 1000 * n + 10 * di + vi)))
    return out


def path(n, order=None):
    i = np.arange(n - 1)
    a, b = (i, i + 1) if order is None else (order[i], order[i + 1])
    return csr_raw(n, *both_ways(a, b))


def star(n, hub):
    leaves = np.delete(np.arange(n), hub)
    return csr_raw(n, *both_ways(np.full(n - 1, hub), leaves))


def diameter_cases():
    n = 65536
    i = np.arange(n)
    r, c = np.divmod(i, 256)
    right, down = i[c < 255], i[r < 255]
    return [('path_65536', 'diameter', path(n)),
            ('path_65536_permuted', 'diameter', path(n, np.random.default_rng(7).permutation(n))),
            ('ring_65536', 'diameter', csr_raw(n, *both_ways(i, (i + 1) % n))),
            ('grid_256x256', 'diameter', csr_raw(n, *both_ways(np.concatenate([right, down]), np.concatenate([right + 1, down + 256]))))]


def threshold_rows(length):
    """three rows of `length` stored entries each, stored in ONE direction (the rows of their neighbours are empty), the three
    neighbourhoods disjoint, and five vertices nobody names: 3 components of length + 1 vertices, 5 of one"""
    n = 3 * (length + 1) + 5
    rows = np.repeat(n - 1 - np.arange(3), length)
    cols = np.arange(3 * length)
    return csr_raw(n, rows, cols)


def hub_cases():
    T = wave_row_threshold()
    k = np.arange(300)
    a, b = np.meshgrid(k, k, indexing='ij')
    off = a != b
    two = sparse.block_diag([star(700, 0), star(500, 499)]).tocsr()
    two = csr_raw(1200, *both_ways(np.concatenate([two.nonzero()[0], [3]]), np.concatenate([two.nonzero()[1], [700 + 17]])))
    return [('star_5000_hub_first', 'hubs', star(5000, 0)),
            ('star_5000_hub_last', 'hubs', star(5000, 4999)),
            ('k300_and_50_isolated', 'hubs', csr_raw(350, a[off] + 25, b[off] + 25)),
            ('two_stars_joined', 'hubs', two)] + \
           [('rows_of_%d_entries' % length, 'hubs', threshold_rows(length)) for length in (T - 1, T, T + 1)]


def tie_cases():
    # two components of 40 vertices and three single vertices: first the halves in index order, then interleaved, then with vertex 0
    # alone in FRONT of the two (the first maximum is label 1, neither 0 nor the last)
    k = np.arange(39)
    halves = csr_raw(83, *both_ways(np.concatenate([k, 40 + k]), np.concatenate([k + 1, 41 + k])))
    inter = csr_raw(83, *both_ways(np.concatenate([2 * k, 2 * k + 1]), np.concatenate([2 * k + 2, 2 * k + 3])))
    behind = csr_raw(83, *both_ways(np.concatenate([1 + k, 43 + k]), np.concatenate([2 + k, 44 + k])))
    return [('tie_two_halves', 'ties', halves), ('tie_interleaved', 'ties', inter), ('tie_behind_a_single_vertex', 'ties', behind),
            ('all_isolated', 'ties', csr_raw(100, [], []))]


def host_cases():
    """every case that needs no device"""
    out = []
    for n in RANDOM_N:
        out += random_cases(n)
    return out + diameter_cases() + hub_cases() + tie_cases()


def three_blobs():
    """300, 200 and 100 points around centres 50 units apart"""
    rng = np.random.default_rng(11)
    return np.concatenate([rng.normal(size=(m, 2)) + [50.0 * c, 0.0] for c, m in enumerate((300, 200, 100))])


def package_cases():
    """graphs built by the package itself (on the device)"""
    import graphlearning_amd as gl
    X = three_blobs()
    Y = np.random.default_rng(12).random((400, 2))
    return [('blobs_knn5', 'package', gl.weightmatrix.knn(X, 5)),
            ('blobs_knn5_unsymmetrized', 'package', gl.weightmatrix.knn(X, 5, symmetrize=False)),
            ('epsilon_ball_with_isolated_points', 'package', gl.weightmatrix.epsilon_ball(Y, 0.04))]


def scipy_components(W):
    from scipy.sparse import csgraph
    return csgraph.connected_components(W, directed=False)
