"""weightmatrix.epsilon_ball on the device: the golden vectors of the reference bit for bit, a randomised sweep against the
restatement tests/epsball_ref.py, the extremes (complete graphs, hubs beside isolated vertices, dropped zeros, the cell cap, one point), two
inputs at scale, and the learners on a GPU-built epsilon-graph against the oracle on the golden one.  The session runs with
GLX_HOST_EXP=1 (conftest.py): the Gaussian weights are then this host's numpy bits, as in the golden files; the `device_exp`
fixture switches to the correctly rounded exponential of the device."""
import os
import sys

import numpy as np
import pytest
from scipy import sparse

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epsball_ref as ref  # noqa: E402
from test_epsball_host import load_golden, golden_matrix, GOLDEN_ENTRIES  # noqa: E402

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


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def check_canonical(W, n):
    W = sparse.csr_matrix(W)
    assert W.shape == (n, n) and W.data.dtype == np.float64 and W.indices.dtype == np.int32 and W.indptr.dtype == np.int32
    rows = np.repeat(np.arange(n), np.diff(W.indptr))
    assert (W.indices != rows).all()                                        # empty diagonal
    inner = np.ones(len(W.indices), bool)
    inner[W.indptr[:-1][np.diff(W.indptr) > 0]] = False
    assert (np.diff(W.indices.astype(np.int64))[inner[1:]] > 0).all()       # sorted, no duplicates
    assert not (W.data == 0).any()                                          # no explicit zeros


def assert_same(got, want, what, nan_ok=False):
    got, want = sparse.csr_matrix(got), sparse.csr_matrix(want)
    assert got.shape == want.shape, what
    assert np.array_equal(got.indptr, want.indptr), what
    assert np.array_equal(got.indices, want.indices), what
    if nan_ok:      # 0/0: the sign and payload of a NaN are nobody's to define
        assert np.array_equal(np.isnan(got.data), np.isnan(want.data)), what
        keep = ~np.isnan(want.data)
        assert same_bits(got.data[keep], want.data[keep]), what
    else:
        assert same_bits(got.data, want.data), what


@pytest.mark.parametrize('name', sorted(GOLDEN_ENTRIES))
def test_golden_bit_for_bit(gl, name):
    """Every golden case, all four kernels: indptr, indices, data."""
    from graphlearning_amd import utils
    g = load_golden()[name]
    X, eps, F, eps_f = ref.golden_inputs()[name]
    n = X.shape[0]
    prep = ref.prepare(X, eps, F)
    for kernel in ref.KERNELS:
        with np.errstate(all='ignore'):
            W = gl.weightmatrix.epsilon_ball(X, eps, kernel=kernel, features=F, epsilon_f=eps_f)
        want = golden_matrix(g, name, kernel, n)
        if want is None:        # the file stores this case's structure and Gaussian data only: the restatement supplies the rest
            want = ref.epsilon_ball(X, eps, kernel=kernel, features=F, epsilon_f=eps_f, prep=prep)
        assert_same(W, want, (name, kernel), nan_ok=(name == 'dups0' and kernel == 'gaussian'))
        if W.nnz:
            check_canonical(W, n)
            assert utils.known_symmetric(W)
            assert (W != W.T).nnz == 0 or name == 'dups0'
        else:
            assert W.nnz == 0 and W.shape == (n, n)
    if name == 'rand2_tiny':
        assert gl.weightmatrix.epsilon_ball(X, eps).nnz == 0


def test_golden_user_kernel(gl):
    g = load_golden()['eta']
    X, eps, _, _ = ref.golden_inputs()['grid_int']
    W = gl.weightmatrix.epsilon_ball(X, eps, eta=ref.eta_hat)
    want = sparse.csr_matrix((g['eta_data'], g['eta_indices'], g['eta_indptr']), shape=(1600, 1600))
    assert_same(W, want, 'eta')
    assert W.nnz == 12324 and W.data.min() == 0.5
    # eta with features: the product of the two kernels, zeros dropped
    Xf, epsf, F, ef = ref.golden_inputs()['feat']
    assert_same(gl.weightmatrix.epsilon_ball(Xf, epsf, features=F, epsilon_f=ef, eta=ref.eta_hat),
                ref.epsilon_ball(Xf, epsf, features=F, epsilon_f=ef, eta=ref.eta_hat), 'eta with features')


def test_device_exp_within_one_ulp(gl, device_exp):
    """The default mode: same structure, every Gaussian weight within one ulp of the golden (numpy's exp is within an ulp of the
    correctly rounded one)."""
    from graphlearning_amd import utils
    gold = load_golden()
    for name in sorted(GOLDEN_ENTRIES):
        if GOLDEN_ENTRIES[name] == 0 or name == 'dups0':
            continue
        g = gold[name]
        X, eps, F, eps_f = ref.golden_inputs()[name]
        W = gl.weightmatrix.epsilon_ball(X, eps, features=F, epsilon_f=eps_f)
        want = golden_matrix(g, name, 'gaussian', X.shape[0])
        assert np.array_equal(W.indptr, want.indptr) and np.array_equal(W.indices, want.indices), name
        from weights_cr_ref import ball_matrix_cr, same_matrix
        if F is None:
            ulps = np.abs(W.data.view(np.int64) - want.data.view(np.int64))
            assert ulps.max() <= 1, (name, int(ulps.max()))
            assert same_matrix(W, ball_matrix_cr(X.shape[0], ref.prepare(X, eps), eps)), (name, 'bit for bit')
        else:
            assert same_matrix(W, ball_matrix_cr(X.shape[0], ref.prepare(X, eps, F), eps, eps_f)), (name, 'bit for bit')
            # a product of two exponentials: each factor is within one ulp of numpy's, and the product is checked for what it
            # is -- fl(exp_cr(a) * exp_cr(b)) bit for bit, the factors evaluated one by one through the library's test hook
            assert_product_of_exponentials(W, X, eps, F, eps_f, want, name)
        assert utils.known_symmetric(W)
        assert (W != W.T).nnz == 0


def assert_product_of_exponentials(W, X, eps, F, eps_f, want, what):
    """W (device exponential, features) == fl(exp_cr(-4 d / eps^2) * exp_cr(-4 f / eps_f^2)) bit for bit on the entries of `want`,
    whose zeros (a product that underflows) are dropped; each factor within one ulp of this host's numpy."""
    from graphlearning_amd import _hip
    prep = ref.prepare(X, eps, F)
    a = -4 * prep['dists'] / (eps * eps)
    b = -4 * prep['fdists'] / (eps_f * eps_f)
    ea, eb = _hip.exp_cr(a), _hip.exp_cr(b)
    for e, x in ((ea, a), (eb, b)):
        big = np.exp(x) > 1e-300          # (one ulp is a statement about normal numbers)
        assert np.abs(e[big].view(np.int64) - np.exp(x)[big].view(np.int64)).max() <= 1, what
    w = ea * eb
    keep = w != 0
    assert np.array_equal(np.bincount(prep['I'][keep], minlength=X.shape[0]), np.diff(W.indptr)), what
    assert np.array_equal(W.indices, prep['J'][keep]), what
    assert same_bits(W.data, w[keep]), what
    assert np.array_equal(W.indptr, want.indptr) and np.array_equal(W.indices, want.indices), what


# ---- the randomised sweep ------------------------------------------------------------------------------------------------------
NS = [1, 2, 63, 64, 65, 257, 1000, 5000]
DS = [1, 2, 3, 4, 7, 8, 9, 20, 64, 130]
SHAPES = ['uniform', 'blobs', 'intgrid', 'offset', 'constcoord', 'negative']
DEGREES = [0, 1, 12, 100, 'all']


def make_points(rng, n, d, shape):
    if shape == 'blobs':
        c = rng.normal(size=(4, d)) * 3
        return c[rng.integers(0, 4, n)] + rng.normal(size=(n, d))
    if shape == 'intgrid':
        m = int(np.ceil(max(n, 2) ** (1.0 / min(d, 3)))) + 1
        return rng.integers(0, m, size=(n, d)).astype(np.float64) if d <= 3 else \
            np.concatenate([rng.integers(0, m, size=(n, 3)), rng.integers(0, 2, size=(n, d - 3))], axis=1).astype(np.float64)
    X = rng.random((n, d))
    if shape == 'offset':
        X = X + 1e6
    elif shape == 'constcoord':
        X[:, rng.integers(0, d)] = 3.25
    elif shape == 'negative':
        X = X - 5.0
    return X


def pick_epsilon(rng, X, degree):
    n = X.shape[0]
    if n == 1:
        return 0.5
    rows = rng.permutation(n)[:min(n, 200)]
    D2 = ref.d2_tree_matrix(X, rows)
    D2[np.arange(len(rows)), rows] = np.inf
    if degree == 'all':
        D2[np.isinf(D2)] = 0
        return 2.1 * float(np.sqrt(D2.max())) + 1e-3
    flat = np.sort(D2[np.isfinite(D2)])
    if degree == 0:
        pos = flat[flat > 0]
        return 0.5 * float(np.sqrt(pos[0])) if len(pos) else 0.25
    q = min(len(flat) - 1, int(len(flat) * min(1.0, degree / (n - 1))))
    return float(np.sqrt(flat[q]))


def sweep_cases():
    cases = []
    t = 0
    # every n with every d once; along a row of the (n, d) table the degree moves with i + j and the feature flag with
    # i + (i + j) // 5, so that neither is a function of d (or of n) alone, and the shape with 3 i + j
    for i, n in enumerate(NS):
        for j, d in enumerate(DS):
            cases.append((n, d, SHAPES[(3 * i + j) % 6], DEGREES[(i + j) % 5], (i + (i + j) // 5) % 2 == 1, 1000 + t))
            t += 1
    # every (d, degree) at a size where a degree of 100 and 'all' mean something, features alternating along both
    for j, d in enumerate(DS):
        for k, deg in enumerate(DEGREES):
            cases.append(([257, 1000][(j + k) % 2], d, SHAPES[(j + 2 * k) % 6], deg, (j + k) % 2 == 0, 1000 + t))
            t += 1
    # and every (shape, degree) at the sizes where the grid is busiest
    for s in SHAPES:
        for k, deg in enumerate(DEGREES):
            cases.append(([1000, 5000, 257][t % 3], [2, 3, 1, 4, 9][(t + k) % 5], s, deg, t % 2 == 0, 1000 + t))
            t += 1
    return cases


def _check_sweep_coverage():
    """The sweep crosses its factors: every (d, degree) and every (n, d) pair occurs, every d and every n meets a degree other
    than 0 both with and without features (at a size that can have edges), every shape meets every degree."""
    cases = sweep_cases()
    assert {(c[1], c[3]) for c in cases} == {(d, g) for d in DS for g in DEGREES}
    assert {(c[0], c[1]) for c in cases} >= {(n, d) for n in NS for d in DS}
    assert {(c[2], c[3]) for c in cases} == {(s, g) for s in SHAPES for g in DEGREES}
    for d in DS:
        for feat in (False, True):
            degs = {c[3] for c in cases if c[1] == d and c[4] == feat and c[0] >= 63}
            assert len(degs - {0}) >= 2, (d, feat, degs)
    for n in NS[2:]:
        for feat in (False, True):
            assert {c[3] for c in cases if c[0] == n and c[4] == feat} - {0}, (n, feat)
    for d in DS:
        assert 'all' in {c[3] for c in cases if c[1] == d} and 100 in {c[3] for c in cases if c[1] == d}


_check_sweep_coverage()


@pytest.mark.parametrize('case', sweep_cases(), ids=lambda c: 'n%d_d%d_%s_deg%s_%s_s%d' % (c[0], c[1], c[2], c[3], 'feat' if c[4] else 'nofeat', c[5]))
def test_sweep_against_restatement(gl, case):
    n, d, shape, degree, with_features, seed = case
    rng = np.random.default_rng(seed)
    X = make_points(rng, n, d, shape)
    eps = pick_epsilon(rng, X, degree)
    D2 = ref.full_d2(X)
    nudges = 0
    while ref.near_boundary(X, eps, D2=D2):          # a pair within rounding of the radius: step away from it, the case still runs
        eps *= 1 + 1e-6
        nudges += 1
        assert nudges <= 8
    F = rng.random((n, int(rng.choice([1, 3, 9])))) if with_features else None
    prep = ref.prepare(X, eps, F, D2=D2)
    del D2
    for kernel in ref.KERNELS:
        with np.errstate(all='ignore'):
            W = gl.weightmatrix.epsilon_ball(X, eps, kernel=kernel, features=F, epsilon_f=0.7)
            want = ref.epsilon_ball(X, eps, kernel=kernel, features=F, epsilon_f=0.7, prep=prep)
        assert_same(W, want, (case, kernel, eps))
        if W.nnz:
            check_canonical(W, n)
    with np.errstate(all='ignore'):
        assert_same(gl.weightmatrix.epsilon_ball(X, eps, features=F, epsilon_f=0.7, eta=ref.eta_hat),
                    ref.epsilon_ball(X, eps, features=F, epsilon_f=0.7, eta=ref.eta_hat, prep=prep), (case, 'eta'))


# ---- extremes --------------------------------------------------------------------------------------------------------------------
def test_identical_points_complete_graph(gl):
    n = 3000
    X = np.tile(np.array([[0.3, -1.5, 2.0]]), (n, 1))
    for eps in (0.0, 0.1):
        W = gl.weightmatrix.epsilon_ball(X, eps, kernel='uniform')
        assert W.nnz == n * (n - 1) and (W.data == 1).all()
        check_canonical(W, n)
        assert (np.diff(W.indptr) == n - 1).all()
        S = gl.weightmatrix.epsilon_ball(X, eps, kernel='singular')
        assert S.nnz == n * (n - 1) and (S.data == 1).all()
        D = gl.weightmatrix.epsilon_ball(X, eps, kernel='distance')
        assert D.nnz == 0 and D.shape == (n, n)


def test_hub_beside_isolated_rows(gl):
    """Rows longer than one wavefront sorts (a knot of 2500 points within epsilon of each other) between rows with no entry at
    all (1500 points far from everything), interleaved in the caller's order; and a star in 199 dimensions: the centre is
    within epsilon of all n - 1 others, which are farther than epsilon from each other."""
    rng = np.random.default_rng(21)
    knot = rng.random((2500, 2)) * 1e-3
    far = np.stack([np.arange(1500) * 10.0 + 100.0, -np.arange(1500) * 7.0 - 50.0], axis=1)
    X = np.concatenate([knot, far])[rng.permutation(4000)]
    for kernel in ('distance', 'singular'):
        W = gl.weightmatrix.epsilon_ball(X, 0.01, kernel=kernel)
        assert_same(W, ref.epsilon_ball(X, 0.01, kernel=kernel), ('knot', kernel))
    deg = np.diff(W.indptr)
    assert sorted(set(deg.tolist())) == [0, 2499] and (deg == 0).sum() == 1500
    check_canonical(W, 4000)
    n = 200
    S = np.concatenate([np.zeros((1, n - 1)), np.eye(n - 1)])
    W = gl.weightmatrix.epsilon_ball(S, 1.0, kernel='singular')
    assert_same(W, ref.epsilon_ball(S, 1.0, kernel='singular'), 'star')
    deg = np.diff(W.indptr)
    assert deg[0] == n - 1 and (deg[1:] == 1).all()


def test_zero_weights_dropped_on_the_device(gl, device_exp):
    """A Gaussian feature weight that underflows to zero, and `distance` between duplicates: dropped by the device's compaction."""
    rng = np.random.default_rng(22)
    X = rng.random((3000, 2))
    F = rng.integers(0, 2, size=(3000, 1)) * 40.0            # exp(-4 * 1600) = 0 between the two feature values
    W = gl.weightmatrix.epsilon_ball(X, 0.05, features=F, epsilon_f=1.0)
    want = ref.epsilon_ball(X, 0.05, features=F, epsilon_f=1.0)
    full = ref.epsilon_ball(X, 0.05, kernel='uniform')
    assert 0 < want.nnz < full.nnz
    assert np.array_equal(W.indptr, want.indptr) and np.array_equal(W.indices, want.indices)
    # the feature factor is exp(0) = 1 on every entry that stays, so the weight is ONE exponential: within one ulp of numpy's
    assert np.abs(W.data.view(np.int64) - want.data.view(np.int64)).max() <= 1
    assert_product_of_exponentials(W, X, 0.05, F, 1.0, want, 'underflow')
    check_canonical(W, 3000)
    Xd = np.repeat(X[:1000], 3, axis=0)
    Wd = gl.weightmatrix.epsilon_ball(Xd, 0.03, kernel='distance')
    assert_same(Wd, ref.epsilon_ball(Xd, 0.03, kernel='distance'), 'duplicates')
    assert Wd.nnz < gl.weightmatrix.epsilon_ball(Xd, 0.03, kernel='uniform').nnz


def test_cell_cap_and_single_point(gl):
    from graphlearning_amd import _hip
    rng = np.random.default_rng(11)
    X = rng.random((20000, 3))
    X[:500] = X[500:1000] + 1e-9 * rng.normal(size=(500, 3))      # 500 close pairs in a cloud whose grid would need 1e24 cells
    eps = 1e-8
    W = gl.weightmatrix.epsilon_ball(X, eps, kernel='uniform')
    st = _hip.ball_stats()
    assert st['cells'] <= 4 * 20000                                 # the cap by points
    assert_same(W, ref.epsilon_ball(X, eps, kernel='uniform'), 'cell cap')
    assert W.nnz >= 900
    # tiny epsilon against a long extent: the cap per axis
    Y = np.stack([np.linspace(0, 1e9, 3000), np.zeros(3000)], axis=1)
    Y[1::2, 0] = Y[0::2, 0] + 0.5
    Wy = gl.weightmatrix.epsilon_ball(Y, 0.75, kernel='singular')
    assert_same(Wy, ref.epsilon_ball(Y, 0.75, kernel='singular'), 'long axis')
    assert Wy.nnz == 3000
    for d in (1, 3, 9):
        W1 = gl.weightmatrix.epsilon_ball(np.zeros((1, d)), 2.0)
        assert W1.shape == (1, 1) and W1.nnz == 0


# ---- scale -----------------------------------------------------------------------------------------------------------------------
def test_million_points(gl):
    """10^6 uniform points in 3-D: the entry count is the tree's own count; symmetric, sorted, no diagonal; 2000 sampled rows
    equal brute force bit for bit; and the grid prunes -- at most 0.01 n^2 pairs tested (exact 27-cell enumeration needs
    27 eps^3 n^2 = 1.4e-4 n^2; the factor of 70 is room for tile granularity)."""
    from scipy.spatial import cKDTree
    from graphlearning_amd import _hip, utils
    n, eps = 10 ** 6, 0.0174
    X = np.random.default_rng(8).random((n, 3))
    W = gl.weightmatrix.epsilon_ball(X, eps)
    st = _hip.ball_stats()
    print('ball_stats', st)
    T = cKDTree(X)
    count = int(T.count_neighbors(T, eps)) - n
    print('entries', W.nnz, 'tree count', count)
    assert count == 21638882
    assert W.nnz == count
    assert st['pairs_accepted'] == count
    assert st['pairs_tested'] <= 0.01 * n * n, st
    check_canonical(W, n)
    assert utils.known_symmetric(W)
    Wt = sparse.csr_matrix(W.T)
    Wt.sort_indices()
    assert np.array_equal(Wt.indptr, W.indptr) and np.array_equal(Wt.indices, W.indices) and same_bits(Wt.data, W.data)
    # brute force over every point whose first coordinate is within 2 epsilon of the row's (beyond that the first term of the
    # sum alone exceeds epsilon^2, by a factor of four)
    rows = np.random.default_rng(9).permutation(n)[:2000]
    order = np.argsort(X[:, 0], kind='stable')
    x0 = X[order, 0]
    for i in rows:
        cand = np.sort(order[np.searchsorted(x0, X[i, 0] - 2 * eps):np.searchsorted(x0, X[i, 0] + 2 * eps, side='right')])
        nb = cand[ref.d2_tree(X[i], X[cand]) <= eps * eps]
        nb = nb[nb != i]
        assert np.array_equal(W.indices[W.indptr[i]:W.indptr[i + 1]], nb), i
        V = X[i][None, :] - X[nb]
        want = np.exp(-4 * np.sum(V * V, axis=1) / (eps * eps))
        assert same_bits(W.data[W.indptr[i]:W.indptr[i + 1]], want), i


def test_pixel_grid_with_features(gl):
    """512 x 512 pixels, epsilon = 5, three features per pixel: 80 neighbours inside, the host's entry count."""
    from scipy.spatial import cKDTree
    m = 512
    g = np.meshgrid(np.arange(float(m)), np.arange(float(m)), indexing='ij')
    X = np.stack([g[0].ravel(), g[1].ravel()], axis=1)
    F = np.random.default_rng(12).random((m * m, 3))
    W = gl.weightmatrix.epsilon_ball(X, 5.0, features=F, epsilon_f=1.0)
    T = cKDTree(X)
    count = int(T.count_neighbors(T, 5.0)) - m * m
    assert W.nnz == count
    deg = np.diff(W.indptr).reshape(m, m)
    assert (deg[5:-5, 5:-5] == 80).all()
    check_canonical(W, m * m)
    rows = np.random.default_rng(13).permutation(m * m)[:300]
    for i in rows:
        nb = np.nonzero(ref.d2_tree(X[i], X) <= 25.0)[0]
        nb = nb[nb != i]
        assert np.array_equal(W.indices[W.indptr[i]:W.indptr[i + 1]], nb), i
        V, VF = X[i][None, :] - X[nb], F[i][None, :] - F[nb]
        want = np.exp(-4 * np.sum(V * V, axis=1) / 25.0) * np.exp(-4 * np.sum(VF * VF, axis=1) / 1.0)
        assert same_bits(W.data[W.indptr[i]:W.indptr[i + 1]], want), i


# ---- downstream ------------------------------------------------------------------------------------------------------------------
def test_learners_on_the_gpu_built_graph(gl, orc):
    """ssl.poisson (both solvers), ssl.laplace and graph.plaplace(fast=False) on the GPU-built rand2 graph (minimum degree 2)
    equal the oracle's results on the golden matrix, by the comparisons of tests/test_gpu_parity.py."""
    g = load_golden()['rand2']
    X, eps, _, _ = ref.golden_inputs()['rand2']
    Wg = golden_matrix(g, 'rand2', 'gaussian', X.shape[0])
    W = gl.weightmatrix.epsilon_ball(X, eps)
    assert_same(W, Wg, 'rand2')
    assert np.diff(W.indptr).min() == 2
    labels = (X[:, 0] + 0.3 * np.sin(6 * X[:, 1]) > 0.5).astype(np.int64)
    ti = orc.trainsets_generate(labels, rate=5, seed=2)
    m = gl.ssl.poisson(W, solver='gradient_descent')
    u = m.fit(ti, labels[ti])
    u_ref, T_ref = orc.poisson_gd(Wg, ti, labels[ti], return_T=True)
    assert m.num_iter == T_ref
    assert np.array_equal(u, u_ref)
    assert np.array_equal(m.predict(), orc.predict(u_ref))
    m = gl.ssl.poisson(W)
    u = m.fit(ti, labels[ti])
    u_ref, it_ref = orc.poisson_cg(Wg, ti, labels[ti], return_iters=True)
    assert m.num_iter == it_ref
    assert np.array_equal(u, u_ref)
    m = gl.ssl.laplace(W, reduce='exact')
    u = m.fit(ti, labels[ti])
    u_ref = orc.laplace_fit(Wg, ti, labels[ti])
    assert np.array_equal(u, u_ref)
    assert np.array_equal(m.predict(), orc.predict(u_ref))
    x, y = X[:, 0], X[:, 1]
    bdy = (x < 0.05) | (x > 0.95) | (y < 0.05) | (y > 0.95)
    val = (x - 0.5) ** 2 + (y - 0.5) ** 2
    G = gl.graph(W)
    u = G.plaplace(bdy, val[bdy], 6.0, tol=1e-1, max_num_it=301, fast=False)
    uo, it = orc.plaplace_jacobi(Wg, bdy, val[bdy], 6.0, tol=1e-1, max_num_it=301, return_iters=True)
    assert G.plaplace_iters == it
    assert np.array_equal(u, uo)


def test_int32_limit_is_reported(gl):
    """More than 2^31 - 1 entries: refused with the count in the message (66 000 points within epsilon of each other)."""
    from graphlearning_amd import _hip
    n = 66000
    X = np.random.default_rng(14).random((n, 2)) * 1e-3
    with pytest.raises(_hip.GlxError) as e:
        gl.weightmatrix.epsilon_ball(X, 1.0, kernel='uniform')
    assert str(n * (n - 1)) in str(e.value)
