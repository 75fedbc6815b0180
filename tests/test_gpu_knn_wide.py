"""The wide search: exact kNN lists of 61 .. 1024 neighbours (self included) through glx_knn_search (_hip.KnnResult), which
weightmatrix.knnsearch and weightmatrix.knn use above 60.  Lists against cKDTree (oracle.gl_oracle), the plan's statistics,
every form of the search against the others bit for bit, weight matrices and a learner end to end, and the limits."""
import os
import numpy as np
import pytest
from conftest import blobs

pytestmark = pytest.mark.gpu


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


def _data(style, n, d, seed):
    rng = np.random.default_rng(seed)
    if style == 'iso':
        return rng.normal(size=(n, d))
    if style == 'blobs':
        return blobs(n, d, 10, seed, 4.0)[0]
    if style == 'offset':
        return rng.normal(size=(n, d)) + 1e6
    if style == 'badscale':
        return rng.normal(size=(n, d)) * np.exp(rng.normal(size=(1, d)) * 2.0)
    if style == 'repeat3':
        return np.repeat(rng.normal(size=(n // 3, d)), 3, axis=0)
    if style == 'grid':                         # integers in a small box: masses of ties
        side = max(2, int(round(n ** (1.0 / d))) + 1)
        return rng.integers(0, side, size=(n, d)).astype(np.float64)
    raise ValueError(style)


def _exact_sq(X, i):
    """Squared distances from row i to every row with the accumulation pattern of cKDTree (and of the search's re-rank):
    four partial sums over blocks of four coordinates, combined left to right, then the tail -- the same bits."""
    diff = X - X[i]
    sq = diff * diff
    d = X.shape[1]
    nb = d // 4
    acc = [np.zeros(len(X)) for _ in range(4)]
    for b in range(nb):
        for j in range(4):
            acc[j] = acc[j] + sq[:, 4 * b + j]
    s = ((acc[0] + acc[1]) + acc[2]) + acc[3]
    for f in range(4 * nb, d):
        s = s + sq[:, f]
    return s


def _check_against_ckdtree(J, D, Jo, Do, tag):
    """Identical indices except swaps between refs at the same distance to the last bit: in every row that differs from
    cKDTree, the differing columns hold bitwise equal distances, and the refs strictly below the row's k-th distance are the
    same set.  Distances within 1e-12 x scale everywhere, self at distance 0, rows ascending by (distance, index)."""
    n, k = Jo.shape
    assert J.dtype == np.int64 and D.dtype == np.float64 and J.shape == (n, k), tag
    scale = max(1.0, float(np.max(Do)))
    assert np.max(np.abs(D - Do)) <= 1e-12 * scale, tag
    assert np.all(D[:, 0] == 0.0), tag
    assert np.all((D[:, 1:] > D[:, :-1]) | ((D[:, 1:] == D[:, :-1]) & (J[:, 1:] > J[:, :-1]))), tag
    for i in np.flatnonzero(np.any(J != Jo, axis=1)):
        cols = np.flatnonzero(J[i] != Jo[i])
        assert np.array_equal(D[i, cols], Do[i, cols]), (tag, i)
        assert set(J[i][D[i] < D[i, -1]]) == set(Jo[i][Do[i] < Do[i, -1]]), (tag, i)


def _check_exact_order(X, J, D, k, rows, tag):
    """The project's own rule on the given rows, against an independent exact ordering: the k smallest (distance^2, index)
    pairs of numpy distances with cKDTree's accumulation pattern (the same bits), lowest index first among equal distances."""
    n = len(X)
    for i in rows:
        s = _exact_sq(X, i)
        top = np.lexsort((np.arange(n), s))[:k]
        assert np.array_equal(J[i], top), (tag, i)
        assert np.array_equal(D[i], np.sqrt(s[top])), (tag, i)


def _sample(n, m, seed):
    return np.arange(n) if n <= m else np.random.default_rng(seed).choice(n, size=m, replace=False)


def _angular(X):
    return X / np.linalg.norm(X, axis=1)[:, None]          # (the expression of the search's Python boundary)


# (k incl. self, d, n, data, similarity): every k and d of the issue at least once, n = k, n not a multiple of 128, up to 20 000
CASES = [
    (61, 1, 61, 'iso', 'euclidean'),
    (61, 8, 20000, 'blobs', 'euclidean'),
    (64, 20, 3001, 'blobs', 'euclidean'),
    (65, 21, 1999, 'offset', 'euclidean'),
    (100, 2, 5000, 'grid', 'euclidean'),
    (100, 33, 2500, 'badscale', 'euclidean'),
    (100, 200, 777, 'repeat3', 'angular'),
    (128, 3, 20000, 'iso', 'euclidean'),
    (128, 64, 1500, 'repeat3', 'angular'),
    (129, 128, 1000, 'blobs', 'euclidean'),
    (129, 129, 1200, 'iso', 'angular'),
    (256, 200, 1000, 'offset', 'euclidean'),
    (256, 8, 9999, 'repeat3', 'euclidean'),
    (257, 20, 257, 'blobs', 'euclidean'),
    (257, 3, 4000, 'grid', 'euclidean'),
    (512, 2, 20000, 'iso', 'angular'),
    (512, 21, 3000, 'badscale', 'euclidean'),
    (1024, 20, 5000, 'blobs', 'euclidean'),
    (1024, 3, 1024, 'grid', 'euclidean'),
    (1024, 64, 2000, 'iso', 'euclidean'),
    (1024, 200, 1500, 'blobs', 'euclidean'),             # d > 130: the fp32 filter's 64 lists of 64, 4096 candidates
]


@pytest.mark.parametrize('k,d,n,style,sim', CASES)
def test_wide_lists_match_ckdtree(gl, orc, k, d, n, style, sim):
    from graphlearning_amd import _hip
    X = _data(style, n, d, 1000 * k + d)
    J, D = gl.weightmatrix.knnsearch(X, k, similarity=sim)
    st = _hip.knn_stats()
    assert st['wide'] and st['candidates'] >= k and st['chunks'] >= 1, st
    if d > 130:
        assert st['KP'] == 64 and st['filter'] == 'f32', st
    Jo, Do = orc.knnsearch(X, k, similarity=sim)
    tag = 'k=%d d=%d n=%d %s %s' % (k, d, n, style, sim)
    _check_against_ckdtree(J, D, Jo, Do, tag)
    _check_exact_order(_angular(X) if sim == 'angular' else X, J, D, k, _sample(n, 64, k + d), tag)


@pytest.mark.parametrize('k', [101, 256])
@pytest.mark.parametrize('style', ['iso', 'blobs'])
def test_lists_do_the_work(gl, k, style):
    """The wide plan's lists hold the k nearest of almost every row: at most 1 % of the rows go to the exact fallback."""
    from graphlearning_amd import _hip
    n = 20000
    X = _data(style, n, 20, 7 + k)
    res = _hip.KnnResult(X, k)
    res.close()
    st = _hip.knn_stats()
    assert st['wide'] and st['escalated_rows'] == 0, st
    assert st['candidates'] == 2 * st['nsplit'] * st['KP'] and st['candidates'] >= 4 * k, st
    assert st['fallback_rows'] <= 0.01 * n, st


def test_escalation_to_the_long_lists(gl, orc):
    """Tight clusters laid out so that every query's 101 nearest fall into ONE ref range of the wide plan (rows whose 32-row
    tile is congruent modulo 8 form a cluster): the lists of 32 cannot hold them, the search is repeated with the fp32 filter's
    lists of 64 -- exact lists all the same."""
    from graphlearning_amd import _hip
    n, d, k = 4096, 20, 101
    rng = np.random.default_rng(17)
    cluster = (np.arange(n) // 32) % 8
    X = rng.normal(size=(8, d))[cluster] * 100.0 + rng.normal(size=(n, d))
    J, D = gl.weightmatrix.knnsearch(X, k)
    st = _hip.knn_stats()
    assert st['wide'] and st['escalated_rows'] > 64 and st['KP'] == 64 and st['filter'] == 'f32', st
    Jo, Do = orc.knnsearch(X, k)
    _check_against_ckdtree(J, D, Jo, Do, 'escalation')
    _check_exact_order(X, J, D, k, _sample(n, 64, 3), 'escalation')


def test_largest_plan_in_chunks(gl):
    """k = 1024 with the long lists (knn_options(lists='long')): 64 lists of 64 on the fp32 filter, 4096 candidates, a 64 KB
    re-rank workgroup, two query chunks -- the default plan's lists bit for bit, and the exact order on sampled rows."""
    from graphlearning_amd import _hip
    n, k = 33000, 1024
    X = _data('blobs', n, 8, 23)
    J0, D0 = _lists(X, k)
    st0 = _hip.knn_stats()
    with _hip.knn_options(lists='long'):
        J1, D1 = _lists(X, k)
    st = _hip.knn_stats()
    assert st['KP'] == 64 and st['nsplit'] == 32 and st['candidates'] == 4096 and st['chunks'] == 2 and st['filter'] == 'f32', st
    assert st0['KP'] == 32 and st0['candidates'] == 2048, st0
    assert np.array_equal(J1, J0) and np.array_equal(D1, D0)
    _check_exact_order(X, J1, D1, k, _sample(n, 24, 5), 'long lists k=1024')


def _lists(X, k, **kw):
    from graphlearning_amd import _hip
    res = _hip.KnnResult(X, k, **kw)
    try:
        return res.lists()
    finally:
        res.close()


@pytest.mark.parametrize('n,k', [(4096, 61), (9000, 101), (20000, 256), (40000, 101)])
def test_every_form_gives_the_same_lists(gl, n, k):
    X = _data('blobs', n, 16, n + k)
    J0, D0 = _lists(X, k, clustered=0)
    J1, D1 = _lists(X, k, want_order=True)
    J2, D2 = _lists(X, k, clustered=64)                     # cells formed by the library, rows reordered (all pairs for wide k)
    for J, D in ((J1, D1), (J2, D2)):
        assert np.array_equal(J, J0) and np.array_equal(D, D0)


def test_auto_cells_at_2e5_rows(gl):
    """2e5 x 16 blobs, k = 101: auto cells switch on; 300 sampled rows equal the exact lists of numpy distances to all rows."""
    from graphlearning_amd import _hip
    n, k = 200000, 101
    assert _hip.auto_cells(n, 16) > 1 or os.environ.get('GLX_KNN_CLUSTERED') is not None
    X = _data('blobs', n, 16, 5)
    J, D = _lists(X, k)
    st = _hip.knn_stats()
    assert st['wide'], st
    rows = np.random.default_rng(0).choice(n, size=300, replace=False)
    for i in rows:
        s = _exact_sq(X, i)
        top = np.lexsort((np.arange(n), s))[:k]
        assert np.array_equal(J[i], top), i
        assert np.array_equal(D[i], np.sqrt(s[top])), i


KERNELS = ['uniform', 'gaussian', 'symgaussian', 'distance', 'singular']


def test_weight_matrices_k100(gl, orc):
    X = _data('blobs', 3000, 8, 11)
    for kernel in KERNELS:
        W = gl.weightmatrix.knn(X, 100, kernel=kernel)
        Wo = orc.knn(X, 100, kernel=kernel)
        assert np.array_equal(W.indptr, Wo.indptr) and np.array_equal(W.indices, Wo.indices), kernel
        assert np.array_equal(W.data, Wo.data), kernel
    W = gl.weightmatrix.knn(X, 100, symmetrize=False)
    Wo = orc.knn(X, 100, symmetrize=False)
    assert np.array_equal(W.indptr, Wo.indptr) and np.array_equal(W.indices, Wo.indices) and np.array_equal(W.data, Wo.data)
    old = os.environ.pop('GLX_HOST_EXP', None)      # the device's correctly rounded exp: the ulp bounds of test_gpu_knn.py
    try:
        for kernel in ['gaussian', 'symgaussian']:
            W = gl.weightmatrix.knn(X, 100, kernel=kernel)
            Wo = orc.knn(X, 100, kernel=kernel)
            assert np.array_equal(W.indptr, Wo.indptr) and np.array_equal(W.indices, Wo.indices), kernel
            assert np.max(np.abs(W.data.view(np.int64) - Wo.data.view(np.int64))) <= (2 if kernel == 'gaussian' else 8), kernel
    finally:
        if old is not None:
            os.environ['GLX_HOST_EXP'] = old


def test_poisson_and_laplace_on_a_k100_graph(gl, orc):
    X, lab = blobs(5000, 8, 5, 21, 3.0)
    W = gl.weightmatrix.knn(X, 100)
    Wo = orc.knn(X, 100)
    assert np.array_equal(W.indices, Wo.indices) and np.array_equal(W.data, Wo.data)
    ti = orc.trainsets_generate(lab, rate=2, seed=3)
    u_ref, T_ref = orc.poisson_gd(Wo, ti, lab[ti], return_T=True)
    m = gl.ssl.poisson(W, solver='gradient_descent')
    u = m.fit(ti, lab[ti])
    assert m.num_iter == T_ref
    assert np.array_equal(u, u_ref)
    assert np.array_equal(m.predict(), orc.predict(u_ref))
    ml = gl.ssl.laplace(W, reduce='exact')
    pred = ml.fit_predict(ti, lab[ti])
    assert np.array_equal(pred, orc.predict(orc.laplace_fit(Wo, ti, lab[ti])))


def test_limits(gl):
    from graphlearning_amd import _hip
    rng = np.random.default_rng(3)
    X = rng.normal(size=(2000, 4))
    with pytest.raises(_hip.GlxError, match='1024'):
        gl.weightmatrix.knnsearch(X, 1025)
    with pytest.raises(_hip.GlxError, match='1024'):
        _hip.KnnResult(X, 1025)
    with pytest.raises(_hip.GlxError):
        gl.weightmatrix.knnsearch(X[:80], 81 + 20)            # k > n
    with pytest.raises(_hip.GlxError):
        _hip.knn_bruteforce(rng.normal(size=(150, 8)), 61)     # the list-returning entry points keep k <= 60
    with pytest.raises(_hip.GlxError):
        _hip.knn_bruteforce(X, 100, query_range=(0, 100))
    J, D = gl.weightmatrix.knnsearch(X, 1024)                  # the cap itself
    assert J.shape == (2000, 1024) and np.all(J[:, 0] == np.arange(2000))
