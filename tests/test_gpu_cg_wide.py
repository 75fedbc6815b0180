"""Both conjugate-gradient solvers of the device against an independent reference at the widths and shapes the product uses them at.

Reference-order mode (reduce='exact': csrc/cg.hip, csrc/cg_seqsum.hip) against oracle.gl_oracle.conjgrad, bit for bit -- iterates,
iteration counts, residual norms -- at 16 ... 128 columns, on 1 ... 300 rows, in both forms of the reduction chains, as stacks of
24 x 10, 32 x 8 and 256 x 1 columns, and its refusals.

Tolerance mode (reduce='tree': csrc/cg_fused.hip with the dot-product form of the SpMM kernel) against the long-double run of
tests/cg_ref.py on every case of tests/cg_cases.py: iteration counts and NaN patterns exactly (tests/test_cg_ref_host.py shows, on
the CPU, that every case decides its stops by a margin of 1e-2 and counts the same in its own format and in long double), iterates
within F times the error the numpy run IN THE CASE'S OWN FORMAT has against long double on the same system (`d_ref`, or the
format's epsilon where that is larger), relative to max(1, max |x_ref|); the final residual norm `err` the same way: within F times
the error of the numpy run's final `err` (or epsilon), relative to max(1, |err_ref|).  F was measured on an MI355X over all cases --
EXPERIMENTS.md, "Both CG solvers at wide widths": the smallest power of two >= 4 x the worst ratio.
"""
import numpy as np
import pytest
from scipy import sparse
import cg_ref
import cg_cases

pytestmark = pytest.mark.gpu

# worst measured ratio (device error) / max(d_ref, eps) over all cases: fp64 2.08 for x (2.45 for err), fp32 1.94 (0.98); EXPERIMENTS.md
F = {'f64': 16.0, 'f32': 8.0}
_RATIOS = {'f64': [], 'f32': []}


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


@pytest.fixture
def form(monkeypatch):
    from graphlearning_amd import _hip

    def set_form(name):
        monkeypatch.setattr(_hip, 'CG_EXACT_FORM', name)
    return set_form


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    for dt, rs in _RATIOS.items():
        if rs:
            wx, we = max(rs), max(rs, key=lambda t: t[1])
            print('\ncg_wide ratios %s: %d comparisons, worst x %.3f at %s, worst err %.3f at %s' % (dt, len(rs), wx[0], wx[2], we[1], we[2]))


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ---- tolerance mode ------------------------------------------------------------------------------------------------------------
def _solve(G, case, s, reduce='tree'):
    if case['api'] == 'rows':
        X, its, errs = G.cg_groups_rows(s['rows'], s['vals'], case['group_cols'], s['masks'], out_scale=s['scale'], tol=case['tol'],
                                        max_iter=case['max_iter'], reduce=reduce)
        return np.array(X), list(its), list(errs)
    if case['api'] == 'groups':
        X, its, errs = G.cg_groups(s['B'], case['group_cols'], tol=case['tol'], max_iter=case['max_iter'], masks=s['masks'], reduce=reduce)
        return X, list(its), list(errs)
    X, it, err = G.cg(s['B'], tol=case['tol'], max_iter=case['max_iter'], x0=s['x0'], reduce=reduce)
    return X, [it], [err]


def _check(case, X, its, errs):
    """the device's answer against the long-double run: counts and NaN patterns exactly, x and the final err within F x the numpy
    run's own error (each relative to max(1, |the long-double value|), the error floored at the format's epsilon)"""
    ref = cg_cases.reference(case['id'])
    x_ld, its_ld, hist_ld = ref.ld
    x_own, _, hist_own = ref.own
    dt, gc = case['dt'], case['group_cols']
    eps = cg_ref.EPS[dt]
    assert X.dtype == cg_ref.DTYPES[dt]
    assert list(its) == list(its_ld), (case['id'], list(its), list(its_ld))
    assert np.array_equal(np.isnan(X), np.isnan(x_ld)), case['id']
    worst_x, worst_e = (0.0, -1), (0.0, -1)
    for g in range(len(its_ld)):
        cols = slice(g * gc, (g + 1) * gc)
        xl = x_ld[:, cols]
        ok = np.isfinite(xl)
        if ok.any():
            scale = max(1.0, float(np.max(np.abs(xl[ok]))))
            d_ref = float(np.max(np.abs(x_own[:, cols][ok].astype(np.longdouble) - xl[ok]))) / scale
            d_dev = float(np.max(np.abs(X[:, cols][ok].astype(np.longdouble) - xl[ok]))) / scale
            worst_x = max(worst_x, (d_dev / max(d_ref, eps), g))
        if not hist_ld[g]:
            assert errs[g] == 1.0                                                   # no iteration ran: utils.py:519
            continue
        err_ld, err_own = float(hist_ld[g][-1]), float(hist_own[g][-1])
        if err_ld != err_ld:
            assert errs[g] != errs[g], (case['id'], g, errs[g])                  # the breakdown's residual norm is NaN on the device too
            continue
        escale = max(1.0, abs(err_ld))
        e_ref = abs(err_own - err_ld) / escale
        e_dev = abs(float(errs[g]) - err_ld) / escale
        worst_e = max(worst_e, (e_dev / max(e_ref, eps), g))
    _RATIOS[dt].append((worst_x[0], worst_e[0], case['id']))
    assert worst_x[0] <= F[dt], (case['id'], 'x', worst_x)
    assert worst_e[0] <= F[dt], (case['id'], 'err', worst_e)


_SINGLE = [c for c in cg_cases.CASES if not c.get('sequence')]


@pytest.mark.parametrize('case', _SINGLE, ids=[c['id'] for c in _SINGLE])
def test_tolerance_mode_equals_the_long_double_reference(gl, case):
    from graphlearning_amd import _hip
    s = cg_cases.build(case)
    G = _hip.DeviceGraph(s['A'], dtype=cg_ref.DTYPES[case['dt']], keep_order=case['keep_order'])
    try:
        X, its, errs = _solve(G, case, s)
        margin = G.last_stop_margin()
        renumbered = G.info()['renumbered']
    finally:
        G.close()
    _check(case, X, its, errs)
    if case['id'].startswith('tol'):
        # no iteration runs (1 > tol is false, utils.py:519-521): x is 0 or x0 as given, and no residual norm was compared with tol --
        # the margin of such a solve is +inf, "nothing to hand back"
        assert its == [0] and np.array_equal(X, s['x0'] if s['x0'] is not None else np.zeros_like(X))
        assert margin == np.inf
    else:
        assert margin >= cg_cases.STOP_BAND, margin           # (the reference's margin is >= 1e-2: test_cg_ref_host.py)
    if case['id'].startswith('renum'):
        assert bool(renumbered) == (not case['keep_order'])
    if case['id'].startswith('large'):
        assert its == [6]
    if case['id'].startswith('eigenvector'):
        ref = cg_cases.reference(case['id'])
        d_ref = float(np.max(np.abs(ref.own[0].astype(np.longdouble) - ref.ld[0]))) / 10.0
        assert its == [1]
        assert np.max(np.abs(X - s['B'] / 0.5)) / 10.0 <= F[case['dt']] * max(d_ref, cg_ref.EPS[case['dt']])


def test_one_operator_through_changing_widths_systems_and_caps(gl):
    """the order of test_tree_mode_history_mirror_survives_a_change_of_layout at 17, 100 and 240 columns: max_iter, the number of
    columns and the number of systems change from solve to solve on one DeviceGraph (the history mirror's markers, the captured
    chunks' key, the work buffers' sizes), three rounds"""
    from graphlearning_amd import _hip
    seq = [c for c in cg_cases.CASES if c.get('sequence')]
    assert len(seq) == 7
    G = _hip.DeviceGraph(cg_cases.build(seq[0])['A'], keep_order=True)
    try:
        for rep in range(3):
            for case in seq:
                s = cg_cases.build(case)
                assert (s['A'] != cg_cases.build(seq[0])['A']).nnz == 0
                X, its, errs = _solve(G, case, s)
                _check(case, X, its, errs)
    finally:
        G.close()


def test_eigenvector_in_reference_order_mode(gl, orc):
    from graphlearning_amd import _hip
    case = cg_cases.BY_ID['eigenvector-f64']
    s = cg_cases.build(case)
    x_ref, it_ref, err_ref = orc.conjgrad(s['A'], s['B'], tol=case['tol'], return_iters=True)
    G = _hip.DeviceGraph(s['A'], keep_order=True)
    try:
        x, it, err = G.cg(s['B'], tol=case['tol'])
    finally:
        G.close()
    assert it == it_ref == 1 and err == err_ref and np.array_equal(x, x_ref)
    assert np.max(np.abs(x - s['B'] / 0.5)) <= F['f64'] * cg_ref.EPS['f64'] * 10.0


def test_tolerance_mode_refusals(gl):
    from graphlearning_amd import _hip
    rng = np.random.default_rng(0)
    n = 300
    A = cg_ref.laplacian_plus(n, 0)
    G = _hip.DeviceGraph(A, keep_order=True)
    try:
        with pytest.raises(_hip.GlxError):
            G.cg(rng.normal(size=(n, 257)), tol=1e-9, reduce='tree')
        with pytest.raises(_hip.GlxError):                     # 32 systems of 10 columns would be 320 columns: not a case of the table
            G.cg_groups(rng.normal(size=(n, 320)), 10, tol=1e-9, reduce='tree')
        masks = [np.array([g], dtype=np.int32) for g in range(33)]
        with pytest.raises(_hip.GlxError, match='32 systems'):
            G.cg_groups(rng.normal(size=(n, 33)), 1, tol=1e-9, masks=masks, reduce='tree')
        # 33 systems WITHOUT Dirichlet rows are fine, and the operator is still usable after the refusals
        B = rng.normal(size=(n, 33))
        X, its, errs = G.cg_groups(B, 1, tol=1e-9, reduce='tree')
        assert min(its) > 10 and np.max(np.abs(A @ X - B)) < 1e-8
    finally:
        G.close()


# ---- reference-order mode -----------------------------------------------------------------------------------------------------
def _exact_system(n, C, seed):
    rng = np.random.default_rng([seed, n, C])
    return cg_ref.laplacian_plus(n, seed), rng.normal(size=(n, C)) * np.exp(rng.normal(size=C))


@pytest.mark.parametrize('n,C', [(300, C) for C in (16, 17, 20, 21, 32, 33, 64, 65, 100, 127, 128)] +
                         [(n, C) for n in (1, 2, 63, 65, 257) for C in (17, 128)])
def test_reference_order_mode_equals_the_oracle(gl, orc, form, n, C):
    from graphlearning_amd import _hip
    A, b = _exact_system(n, C, 3)
    x_ref, it_ref, err_ref = orc.conjgrad(A, b, tol=1e-9, return_iters=True)
    G = _hip.DeviceGraph(A)
    try:
        for name in ('chain', 'blocks'):
            form(name)
            x, it, err = G.cg(b, tol=1e-9)
            assert it == it_ref, (name, it, it_ref)
            assert err == err_ref, (name, err, err_ref)
            assert np.array_equal(x, x_ref), name
            if n >= 63:
                assert (G.last_block_stats() == (-1, -1, -1)) == (name == 'chain')
    finally:
        G.close()


def _masked_reference(orc, A, B, gc, masks, tol):
    """every system alone, on the sub-matrix without its Dirichlet rows (what ssl.laplace solves in the reference)"""
    n = A.shape[0]
    X = np.zeros_like(B)
    its, errs = [], []
    for g in range(B.shape[1] // gc):
        keep = np.setdiff1d(np.arange(n), masks[g]) if masks is not None else np.arange(n)
        x, it, err = orc.conjgrad(sparse.csr_matrix(A)[keep][:, keep], B[keep, g * gc:(g + 1) * gc], tol=tol, return_iters=True)
        X[keep, g * gc:(g + 1) * gc] = x
        its.append(it)
        errs.append(err)
    return X, its, errs


@pytest.mark.parametrize('ng,gc', [(24, 10), (32, 8)])
def test_reference_order_stacks_with_dirichlet_rows(gl, orc, form, ng, gc):
    """24 x 10: the widest stack ssl.laplace's ssl_trials makes of a 10-class problem (240 columns, G = 64 plan)"""
    from graphlearning_amd import _hip
    n = 300
    rng = np.random.default_rng(ng)
    A = cg_ref.laplacian_plus(n, ng)
    B = rng.normal(size=(n, ng * gc)) * np.repeat(np.exp(3 * rng.normal(size=ng)), gc)
    masks = [np.sort(rng.choice(n, size=int(rng.integers(0, 100)), replace=False)).astype(np.int32) for _ in range(ng)]
    X_ref, its_ref, errs_ref = _masked_reference(orc, A, B, gc, masks, 1e-9)
    assert max(its_ref) - min(its_ref) >= 3
    G = _hip.DeviceGraph(A)
    try:
        for name in ('chain', 'blocks'):
            form(name)
            X, its, errs = G.cg_groups(B, gc, tol=1e-9, masks=masks)
            assert list(its) == its_ref, name
            assert list(errs) == errs_ref, name
            assert np.array_equal(X, X_ref), name
    finally:
        G.close()


def test_reference_order_stack_of_256_single_columns(gl, orc, form):
    """One-column systems of a stack are summed row after row like the columns of any (n, C) array (a lone column numpy sums pairwise:
    DeviceGraph.cg does that, cg_groups does not).  The oracle sums a column that way when it stands beside another; a copy scaled by
    1e-100 leaves `err` and the stop as they are (its r.r vanishes below the last bit)."""
    from graphlearning_amd import _hip
    n = 300
    rng = np.random.default_rng(256)
    A = cg_ref.laplacian_plus(n, 256)
    B = rng.normal(size=(n, 256)) * np.exp(3 * rng.normal(size=256))
    X_ref = np.empty_like(B)
    its_ref, errs_ref = [], []
    for j in range(256):
        x, it, err = orc.conjgrad(A, np.stack([B[:, j], 1e-100 * B[:, j]], axis=1), tol=1e-9, return_iters=True)
        X_ref[:, j] = x[:, 0]
        its_ref.append(it)
        errs_ref.append(err)
    G = _hip.DeviceGraph(A)
    try:
        for name in ('chain', 'blocks'):
            form(name)
            X, its, errs = G.cg_groups(B, 1, tol=1e-9)
            assert list(its) == its_ref and list(errs) == errs_ref and np.array_equal(X, X_ref), name
    finally:
        G.close()


def test_reference_order_refusals(gl, monkeypatch):
    """More than 128 columns per system (and more than 256 in all) are refused by the reference-order reducer, with GLX_EUNSUPPORTED
    and nothing computed.  ssl.laplace(reduce='auto') on more than 128 classes answers in tolerance mode as long as that answer
    stands; when it has to hand the solve back (here: forced by AUTO_TREE_MAX_ITER = 0) the refusal reaches the caller as GlxError --
    no tolerance-mode answer is passed off as a reference-order one."""
    from graphlearning_amd import _hip, ssl as glssl
    from conftest import blobs
    rng = np.random.default_rng(1)
    n = 300
    A = cg_ref.laplacian_plus(n, 1)
    G = _hip.DeviceGraph(A)
    try:
        with pytest.raises(_hip.GlxError, match='too wide for the reference-order reducer'):
            G.cg(rng.normal(size=(n, 129)), tol=1e-9)
        with pytest.raises(_hip.GlxError, match='too wide for the reference-order reducer'):
            G.cg_groups(rng.normal(size=(n, 129)), 129, tol=1e-9)
        with pytest.raises(_hip.GlxError):
            G.cg(rng.normal(size=(n, 257)), tol=1e-9)
        with pytest.raises(_hip.GlxError):
            G.cg_groups(rng.normal(size=(n, 258)), 2, tol=1e-9)
        b = rng.normal(size=(n, 128))
        x, it, err = G.cg(b, tol=1e-9)                         # the operator is still usable, at the limit
        assert it > 10 and np.max(np.abs(A @ x - b)) < 1e-8
    finally:
        G.close()
    k = 130
    X, _ = blobs(1000, 10, 4, 7, 1.5)
    labels = np.arange(1000) % k
    W = gl.weightmatrix.knn(X, 8)
    train = np.arange(2 * k)
    with pytest.raises(_hip.GlxError, match='too wide for the reference-order reducer'):
        gl.ssl.laplace(W, reduce='exact').fit(train, labels[train])
    u = gl.ssl.laplace(W, reduce='auto').fit(train, labels[train])          # stands as a tolerance-mode answer
    assert u.shape == (1000, k) and np.isfinite(u).all()
    monkeypatch.setattr(glssl, 'AUTO_TREE_MAX_ITER', 0)                      # every solve is handed back
    with pytest.raises(_hip.GlxError, match='too wide for the reference-order reducer'):
        gl.ssl.laplace(W, reduce='auto').fit(train, labels[train])
