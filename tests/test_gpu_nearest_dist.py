"""_hip.nearest_dist (glx_nearest_dist, csrc/knn_rerank.hip: the distance from every row to the nearest labelled row, behind
graph.reweight(method='properly')) against scipy's cKDTree and against the tree-order squared distance of tests/epsball_ref.py, bit
for bit.  The kernel stages the labelled rows through LDS in pieces of 6144 // d rows: one piece, several, a partial last one, a
piece of one row, every remainder of d modulo 4; then what the entry point refuses."""
import os
import sys

import numpy as np
import pytest
from scipy import sparse, spatial

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epsball_ref as eref  # noqa: E402

pytestmark = pytest.mark.gpu

STAGE_ROWS = 6144       # doubles of LDS that hold the labelled rows of one piece

# (n, d, m): pieces of 6144 // d rows
SHAPES = [(1, 1, 1), (257, 1, 3), (300, 2, 300), (513, 3, 40), (300, 7, 17),
          (1000, 20, 400),      # two pieces, the second partial
          (700, 64, 97),        # pieces of 96 rows: m = piece + 1
          (300, 769, 9),        # pieces of 7 rows, d = 1 mod 4
          (260, 6144, 3),       # pieces of one row
          (2000, 5, 1500),      # two pieces
          (1100, 12, 1024),     # exactly two pieces of 512
          (400, 20, 308),       # m = piece + 1 with a piece of 307
          (300, 6, 3072)]       # exactly three pieces of 1024, m > n: every labelled row repeated


@pytest.fixture(scope='module')
def gl():
    import graphlearning_amd as gl
    from graphlearning_amd import _hip
    _hip.require_device()
    return gl


@pytest.fixture(scope='module')
def orc():
    from oracle import gl_oracle
    return gl_oracle


def make(n, d, m, offset, seed=0):
    """Points around `offset` (10: the differences cancel leading digits), one unlabelled row that duplicates a labelled one
    (distance 0), a repeated entry in idx."""
    rng = np.random.default_rng(1000 * seed + n + d + m)
    X = rng.normal(size=(n, d)) + offset
    if m <= n:
        idx = rng.permutation(n)[:m]
    else:
        idx = rng.integers(0, n, size=m)
    if m >= 2:
        idx[-1] = idx[0]
    rest = np.setdiff1d(np.arange(n), idx)
    if len(rest):
        X[rest[-1]] = X[idx[0]]
    return X, idx.astype(np.int64)


def references(X, idx):
    tree = spatial.cKDTree(X[idx]).query(X)[0]
    d2 = eref.d2_tree_matrix(X, idx)                   # (m, n): d2_tree between labelled row j and row i; (a - b)^2 == (b - a)^2 bit for bit
    return tree, np.sqrt(np.min(d2, axis=0))


@pytest.mark.parametrize('offset', [0.0, 10.0])
@pytest.mark.parametrize('n,d,m', SHAPES)
def test_nearest_dist_equals_both_references(gl, n, d, m, offset):
    from graphlearning_amd import _hip
    X, idx = make(n, d, m, offset)
    piece = max(1, min(m, STAGE_ROWS // d))
    print('pieces', -(-m // piece), 'of', piece, 'last', m - (-(-m // piece) - 1) * piece)
    tree, rows = references(X, idx)
    assert np.array_equal(tree, rows)                   # the two references agree
    got = _hip.nearest_dist(X, idx)
    assert got.dtype == np.float64 and got.shape == (n,)
    assert np.array_equal(got, tree) and np.array_equal(got, rows)
    assert (got[idx] == 0).all() and (m >= n or (got == 0).sum() > len(np.unique(idx)))


def test_shapes_cover_the_piece_loop():
    """What the shapes above are there for (host arithmetic only)."""
    pieces = {(n, d, m): (max(1, min(m, STAGE_ROWS // d)), m) for n, d, m in SHAPES}
    count = {k: -(-m // p) for k, (p, m) in pieces.items()}
    assert count[(1000, 20, 400)] == 2 and 400 % 307 != 0
    assert pieces[(700, 64, 97)][0] == 96 and pieces[(400, 20, 308)][0] == 307
    assert pieces[(300, 769, 9)][0] == 7 and count[(300, 769, 9)] == 2 and 769 % 4 == 1
    assert pieces[(260, 6144, 3)][0] == 1 and count[(260, 6144, 3)] == 3
    assert count[(2000, 5, 1500)] == 2
    assert pieces[(1100, 12, 1024)][0] == 512 and count[(1100, 12, 1024)] == 2
    assert pieces[(300, 6, 3072)][0] == 1024 and count[(300, 6, 3072)] == 3
    assert {d % 4 for _, d, _ in SHAPES} == {0, 1, 2, 3}
    assert all(count[k] == 1 for k in [(1, 1, 1), (257, 1, 3), (300, 2, 300), (513, 3, 40), (300, 7, 17)])


def test_row_form_of_the_second_reference():
    """sqrt(min_j d2_tree(x, X[idx])) row by row equals the matrix form used above."""
    X, idx = make(300, 7, 17, 10.0)
    rows = np.array([np.sqrt(np.min(eref.d2_tree(x, X[idx]))) for x in X])
    assert np.array_equal(rows, references(X, idx)[1])


def test_index_forms(gl):
    from graphlearning_amd import _hip
    X, idx = make(513, 3, 40, 10.0)
    want = spatial.cKDTree(X[idx]).query(X)[0]
    for form in (list(idx), [int(i) for i in idx], idx.astype(np.int32), idx.reshape(-1, 1), idx[::-1].copy(), np.asfortranarray(idx.reshape(-1, 1))):
        assert np.array_equal(_hip.nearest_dist(X, form), want)
    assert np.array_equal(_hip.nearest_dist(np.asfortranarray(X), idx), want)
    assert np.array_equal(_hip.nearest_dist(X.astype(np.float32), idx), spatial.cKDTree(X.astype(np.float32)[idx]).query(X.astype(np.float32))[0])


def test_refusals(gl):
    from graphlearning_amd import _hip
    X, idx = make(300, 7, 17, 0.0)
    n = X.shape[0]
    with pytest.raises(_hip.GlxError):
        _hip.nearest_dist(np.zeros((4, 6145)), [0, 1])          # a labelled row no longer fits the LDS stage
    assert np.array_equal(_hip.nearest_dist(np.zeros((4, 6144)), [0, 1]), np.zeros(4))
    for bad in ([-1], [0, n], [n], np.concatenate([idx, [-1]]), [], np.zeros(0, dtype=np.int64)):
        with pytest.raises(_hip.GlxError):
            _hip.nearest_dist(X, bad)
    with pytest.raises(_hip.GlxError):
        _hip.nearest_dist(X[:, 0], idx)                         # not (n, d)
    assert np.array_equal(_hip.nearest_dist(X, idx), spatial.cKDTree(X[idx]).query(X)[0])      # and the next call is served


@pytest.mark.parametrize('value', [np.nan, np.inf, -np.inf])
def test_non_finite_data_is_refused(gl, value):
    """The reference's cKDTree raises ValueError on it; weightmatrix.epsilon_ball refuses it too."""
    from graphlearning_amd import _hip
    X, idx = make(300, 7, 17, 0.0)
    W = sparse.random(300, 300, density=0.03, random_state=3, format='csr')
    for row in (int(idx[3]), int(np.setdiff1d(np.arange(300), idx)[0])):         # in a labelled row, in an unlabelled one
        Y = X.copy()
        Y[row, 5] = value
        with pytest.raises(ValueError):
            spatial.cKDTree(Y[idx]).query(Y)
        with pytest.raises(_hip.GlxError):
            _hip.nearest_dist(Y, idx)
        with pytest.raises(_hip.GlxError):
            gl.graph.graph(W).reweight(idx, method='properly', X=Y)


def test_reweight_properly_equals_oracle(gl, orc):
    """graph.reweight(method='properly') where the labelled rows take two pieces: indices and data of the oracle's matrix."""
    X, idx = make(1000, 20, 400, 10.0)
    W = gl.weightmatrix.knn(X, 8)
    for kw in ({}, dict(alpha=3, zeta=1e5, r=0.5)):
        got = sparse.csr_matrix(gl.graph.graph(W).reweight(idx, method='properly', X=X, **kw))
        want = sparse.csr_matrix(orc.reweight(W, idx, method='properly', X=X, **kw))
        assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
        assert np.array_equal(got.data, want.data)
