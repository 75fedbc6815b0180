"""The narrow search: exact kNN lists of up to 60 neighbours (self included) through _hip.knn_bruteforce -- what every
weightmatrix.knn call and every benchmark configuration runs -- at every instantiation of the two tile kernels that knn_make_plan
can choose (tests/knn_narrow_cases.py; tests/test_knn_plan.py proves on the host that the cases reach all of them): every feature
block count and operand form of the split-bf16 filter, every width class of the fp32-input filter and its feature-blocked variant,
each with every list length, at both edges of every class.  Per case: the statistics name the intended instantiation, the lists are
cKDTree's (oracle.gl_oracle) and the project's own exact order on sampled rows, and -- on benign data -- the LISTS did the work:
the exact fallback repairs whatever the filter loses, so a broken tile kernel would otherwise only show as time."""
import numpy as np
import pytest

import knn_narrow_cases as nc
from test_gpu_knn_wide import _angular, _check_against_ckdtree, _check_exact_order, _data, _exact_sq, _sample  # noqa: F401

pytestmark = pytest.mark.gpu

STYLES = ('iso', 'blobs', 'offset', 'badscale', 'repeat3', 'grid', 'neardup', 'lohalf')


@pytest.fixture(scope='module')
def gl():
    import graphlearning_amd as gl
    from graphlearning_amd import _hip
    _hip.require_device()
    return gl


def data(style, n, d):
    seed = 7000 + 10 * d + STYLES.index(style)
    if style == 'neardup':        # 10 copies of each centre + 1e-6 noise + an offset of 1e3: far below what either filter resolves
        rng = np.random.default_rng(seed)
        m = (n + 9) // 10
        return np.ascontiguousarray((np.repeat(rng.normal(size=(m, d)) * 2.0, 10, axis=0) + rng.normal(size=(10 * m, d)) * 1e-6 + 1e3)[:n])
    if style == 'repeat3':
        return np.ascontiguousarray(_data(style, n + 2, d, seed)[:n])
    if style == 'lohalf':
        # The last 16 features are +-(4 + w), 0 <= w < 2^-4, the same in all 16: their bf16 hi parts are +-4 or +-4.03125 and everything
        # else sits in the lo parts, coherently across the block.  hi.lo + lo.hi of that block then moves a filter value by up to
        # 2 * 16 * 4 * 2^-6 = 2 between refs whose exact distances differ by at most 16 * 2^-8 in these features, against an
        # acceptance margin of 2 eps = 2 cerr (|q| + rmax)^2 of about 0.3 at d = 128 (cerr = 1.0e-4, norms of about 20): a filter
        # that drops or misplaces one of the block's split products ranks the other d - 16 (isotropic) features' neighbours wrongly.
        rng = np.random.default_rng(seed)
        X = rng.normal(size=(n, d))
        X[:, d - 16:] = (rng.integers(0, 2, size=(n, 1)) * 2.0 - 1.0) * (4.0 + rng.random((n, 1)) * 2.0 ** -4)
        return X
    return _data(style, n, d, seed)


_REF = {}


def reference(style, n, d, similarity='euclidean'):
    """(X, J, D): the data of (style, n, d) and cKDTree's lists of min(60, n) neighbours, computed once per module; a case of
    smaller k takes the prefix.  Never written to."""
    key = (style, n, d, similarity)
    if key not in _REF:
        from oracle import gl_oracle
        X = data(style, n, d)
        J, D = gl_oracle.knnsearch(X, min(60, n), similarity=similarity)
        for a in (X, J, D):
            a.setflags(write=False)
        _REF[key] = (X, J, D)
    return _REF[key]


def check_stats(st, c, tag, nq=None):
    """The instantiation the case is there for is the one that ran (the long-list repeat's, where the search escalated)."""
    p = nc.plan(c.n, c.d, c.k, nq=nq, long_lists=st['escalated_rows'] > 0, **dict(c.opts))
    got = (st['filter'], st['KP'], st['dpa'], st['concatenated'], st['nsplit'], st['wide'], st['candidates'])
    want = ('bf16x3' if p.use_bf16 else 'f32', p.KP, p.dpa, p.cat, p.nsplit, False, 2 * p.nsplit * p.KP)
    assert got == want, (tag, got, want)
    return p


def overflow_rows(Jk, p):
    """Rows of which more than KP of the k nearest (the reference's) can only enter one and the same candidate list
    (nc.list_of_ref: the mapping read from the tile kernels): no filter can hold them, the acceptance test must notice."""
    lst = nc.list_of_ref(np.asarray(Jk), p)
    counts = np.stack([(lst == i).sum(axis=1) for i in range(2 * p.nsplit)], axis=1)
    return int(np.sum(counts.max(axis=1) > p.KP))


def check_lists(X, J, D, Jo, Do, k, tag):
    J, D = np.asarray(J), np.asarray(D)
    _check_against_ckdtree(J, D, np.ascontiguousarray(Jo[:, :k]), np.ascontiguousarray(Do[:, :k]), tag)
    _check_exact_order(X, J, D, k, _sample(len(X), 64, k + X.shape[1]), tag)


def search(c, X, **kw):
    from graphlearning_amd import _hip
    with _hip.knn_options(**dict(c.opts)):
        J, D = _hip.knn_bruteforce(X, c.k, **kw)
    return np.array(J), np.array(D), _hip.knn_stats()


@pytest.mark.parametrize('c', [c for c in nc.CASES if c.group in ('main', 'f32', 'long', 'split')], ids=nc.case_id)
def test_narrow_lists_match_ckdtree(gl, c):
    """The main matrix (split-bf16 filter; the fp32-input filter from d = 129), the fp32-input filter by option, the long lists, and
    the 'lohalf' data at the full-width edge of NKB = 2, 4, 6, 8 (see `data`: the one style here that a filter without the last
    block's lo.hi product fails at every NKB; isotropic data hides that product inside the margin from d = 48 on).

    Measured on an MI355X: all 42 kernel keys of the census ran; on every benign case escalated_rows = overflow_rows = 0 and
    fallback_rows = 0, except main-d1-k12-iso with 4 of 2999 rows (cap 29.99).  That case took 1267 rows to the fallback while
    the acceptance margin was cerr (|q| + rmax)^2 for every row; knn_accept_eps (knn_plan.h) is the remedy."""
    tag = nc.case_id(c)
    X, Jo, Do = reference(c.style, c.n, c.d)
    J, D, st = search(c, X)
    p = check_stats(st, c, tag)
    first = nc.case_plan(c)
    over = overflow_rows(Jo[:, :c.k], first)
    print('%s: %s fallback_rows=%d escalated_rows=%d overflow_rows=%d' % (tag, nc.kernel_key(p), st['fallback_rows'], st['escalated_rows'], over))
    check_lists(X, J, D, Jo, Do, c.k, tag)
    if c.style in ('iso', 'blobs', 'lohalf'):
        # the lists, not the fallback, hold the neighbours: no repeat, and beyond the rows whose neighbours cannot fit a list at
        # most 1 % of the rows (the cap of test_gpu_knn_wide.py::test_lists_do_the_work) are repaired.  An overflowed row that
        # passes the acceptance test would mean the test is too lenient.  ('lohalf' is isotropic in d - 16 features and the other
        # 16 add less than 0.07 to a squared distance between points of one sign: benign for a filter that keeps its bound.)
        assert st['escalated_rows'] == 0, (tag, st)
        assert over <= st['fallback_rows'] <= over + 0.01 * c.n, (tag, over, st)


@pytest.mark.parametrize('c', [c for c in nc.CASES if c.group == 'repair'], ids=nc.case_id)
def test_forced_repair(gl, c):
    """One ref range, i.e. 2 lists of 8 for 12 neighbours: the lists cannot hold them and the search is repeated with the long lists;
    two ranges: a few rows' neighbours do not fit and the exact fallback redoes those.  The exact lists all the same, and no row
    whose neighbours overflow a list passes the acceptance test."""
    tag = nc.case_id(c)
    X, Jo, Do = reference(c.style, c.n, c.d)
    J, D, st = search(c, X)
    check_stats(st, c, tag)
    over = overflow_rows(Jo[:, :c.k], nc.case_plan(c))
    print('%s: fallback_rows=%d escalated_rows=%d overflow_rows=%d KP=%d' % (tag, st['fallback_rows'], st['escalated_rows'], over, st['KP']))
    assert st['fallback_rows'] + st['escalated_rows'] > 0, st
    assert st['fallback_rows'] + st['escalated_rows'] >= over, (st, over)
    check_lists(X, J, D, Jo, Do, c.k, tag)


@pytest.mark.parametrize('c', [c for c in nc.CASES if c.group == 'small'], ids=nc.case_id)
def test_small_n(gl, c):
    """n = k (every row lists all rows), one ragged tile, fewer tiles than ref ranges."""
    tag = nc.case_id(c)
    X, Jo, Do = reference(c.style, c.n, c.d)
    J, D, st = search(c, X)
    p = check_stats(st, c, tag)
    assert p.ntiles <= 5 and p.nsplit == min(p.ntiles, 8)
    check_lists(X, J, D, Jo, Do, c.k, tag)


FORMS = [(80, 12), (80, 29), (128, 12), (128, 29)]        # one NKB = 6, one NKB = 8; lists of 8 and of 32


@pytest.fixture(scope='module')
def forms(gl):
    """{(d, k): (X in cell order, cell starts, all-pairs J, D, statistics)} on blobs, the rows in the order of 12 cells."""
    from graphlearning_amd import _hip, dist_build
    out = {}
    for d in (80, 128):
        X0 = data('blobs', nc.N_MAIN, d)
        perm, starts = dist_build.coarse_locality_order(X0, ncells=12, seed=0, return_cells=True)
        X = np.ascontiguousarray(X0[perm])
        for k in (12, 29):
            J, D = _hip.knn_bruteforce(X, k, clustered=0)
            out[(d, k)] = (X, np.asarray(starts, dtype=np.int64), np.array(J), np.array(D), _hip.knn_stats())
    return out


@pytest.mark.parametrize('d,k', FORMS)
def test_every_form_gives_the_same_lists(gl, forms, d, k):
    """A query sub-range, the cell-pruned search (RUNS = true in the tile kernel) on given cells and on cells the library forms,
    and the result object: the lists of the all-pairs search bit for bit."""
    from graphlearning_amd import _hip
    X, starts, J0, D0, st0 = forms[(d, k)]
    p = nc.plan(nc.N_MAIN, d, k)
    assert st0['filter'] == 'bf16x3' and (st0['KP'], st0['dpa'], st0['cells']) == (p.KP, p.dpa, 0), st0
    assert st0['escalated_rows'] == 0 and st0['fallback_rows'] <= 0.01 * nc.N_MAIN, st0
    J, D = _hip.knn_bruteforce(X, k, query_range=(300, 2811))
    assert np.array_equal(J, J0[300:2811]) and np.array_equal(D, D0[300:2811])
    J, D = _hip.knn_bruteforce(X, k, cell_starts=starts)
    st = _hip.knn_stats()
    assert st['cells'] == len(starts) > 1 and (st['KP'], st['dpa']) == (p.KP, p.dpa), st
    assert np.array_equal(J, J0) and np.array_equal(D, D0)
    J, D = _hip.knn_bruteforce(X, k, cell_starts=starts, query_range=(300, 2811))
    assert np.array_equal(J, J0[300:2811]) and np.array_equal(D, D0[300:2811])
    J, D = _hip.knn_bruteforce(X, k, clustered=7)
    st = _hip.knn_stats()
    assert st['cells'] == 7 and (st['KP'], st['dpa']) == (p.KP, p.dpa), st
    assert np.array_equal(J, J0) and np.array_equal(D, D0)
    res = _hip.KnnResult(X, k)
    try:
        J, D = res.lists()
        assert np.array_equal(J, J0) and np.array_equal(D, D0)
    finally:
        res.close()


@pytest.mark.parametrize('d', [16, 32, 64, 80, 128])       # one per NKB class
def test_angular(gl, d):
    from graphlearning_amd import _hip
    X, Jo, Do = reference('iso', nc.N_MAIN, d, 'angular')
    J, D = _hip.knn_bruteforce(X, 12, similarity='angular')
    st = _hip.knn_stats()
    p = nc.plan(nc.N_MAIN, d, 12)
    assert st['filter'] == 'bf16x3' and (st['KP'], st['dpa'], st['escalated_rows']) == (p.KP, p.dpa, 0), st
    check_lists(_angular(X), J, D, Jo, Do, 12, 'angular d=%d' % d)
