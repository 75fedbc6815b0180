"""tests/cg_ref.py (the numpy restatement of utils.conjgrad the tolerance-mode tests measure against) pinned to the oracle, and the
conditions under which tests/test_gpu_cg_wide.py may compare iteration counts EXACTLY, asserted for every case of tests/cg_cases.py:
a definite operator, no residual norm of the reference run within ssl.AUTO_STOP_BAND of tol (the seeds are chosen for 1e-2), the
same iteration counts in the case's own number format and in long double.  No GPU."""
import numpy as np
import pytest
from scipy import sparse
import cg_ref
import cg_cases


@pytest.fixture(scope='module')
def orc():
    from oracle import gl_oracle
    return gl_oracle


def test_restatement_does_not_import_the_oracle():
    import sys
    import subprocess
    import os
    code = 'import sys; sys.path.insert(0, %r); import cg_ref, cg_cases; assert not any(m.split(".")[0] == "oracle" for m in sys.modules)'
    subprocess.run([sys.executable, '-c', code % os.path.dirname(os.path.abspath(__file__))], check=True)


@pytest.mark.parametrize('n,C,seed', [(65, 2, 1), (300, 3, 2), (300, 17, 3), (517, 33, 4), (700, 240, 5)])
@pytest.mark.parametrize('x0', [False, True])
@pytest.mark.parametrize('max_iter', [1e5, 7])
def test_fp64_restatement_equals_the_oracle_bit_for_bit(orc, n, C, seed, x0, max_iter):
    rng = np.random.default_rng(seed)
    A = cg_ref.laplacian_plus(n, seed)
    b = rng.normal(size=(n, C))
    start = rng.normal(size=(n, C)) if x0 else None
    x_ref, it_ref, err_ref = orc.conjgrad(A, b, x0=start, tol=1e-9, max_iter=max_iter, return_iters=True)
    x, it, hist = cg_ref.conjgrad(A, b, x0=start, tol=1e-9, max_iter=max_iter, dtype=np.float64)
    assert it == it_ref and len(hist) == it
    assert hist[-1] == err_ref
    assert np.array_equal(x, x_ref)


def test_single_column_is_summed_row_after_row(orc):
    """The restatement sums a lone column like every other (the device's stacked one-column systems do); the oracle sums it pairwise.
    Beside a copy of itself scaled by 1e-100 -- whose r.r vanishes below the last bit of the first column's in `err` -- the oracle
    sums the column row after row: the same bits."""
    rng = np.random.default_rng(8)
    A = cg_ref.laplacian_plus(300, 8)
    b = rng.normal(size=(300, 1))
    x_ref, it_ref, err_ref = orc.conjgrad(A, np.hstack([b, 1e-100 * b]), tol=1e-9, return_iters=True)
    x, it, hist = cg_ref.conjgrad(A, b, tol=1e-9, dtype=np.float64)
    assert it == it_ref and hist[-1] == err_ref and np.array_equal(x[:, 0], x_ref[:, 0])
    x1, it1, hist1 = cg_ref.conjgrad(A, b[:, 0], tol=1e-9, dtype=np.float64)
    assert it1 == it and hist1 == hist and np.array_equal(x1, x[:, 0])


@pytest.mark.parametrize('dtype', [np.float64, np.float32, np.longdouble])
def test_groups_equal_the_single_solves(dtype):
    rng = np.random.default_rng(2)
    n, gc, ng = 200, 3, 5
    A = cg_ref.laplacian_plus(n, 2)
    B = rng.normal(size=(n, gc * ng)) * np.repeat(np.exp(3 * rng.normal(size=ng)), gc)
    masks = [rng.choice(n, size=k, replace=False) for k in (0, 10, 60, 1, 199)]
    tol = 1e-3 if dtype == np.float32 else 1e-9
    X, its, hists = cg_ref.conjgrad_groups(A, B, gc, masks, tol=tol, dtype=dtype)
    assert X.dtype == dtype and len(set(its)) > 1
    for g in range(ng):
        keep = np.setdiff1d(np.arange(n), masks[g])
        sub = sparse.csr_matrix(A)[keep][:, keep]
        x, it, hist = cg_ref.conjgrad(sub, B[keep, g * gc:(g + 1) * gc], tol=tol, dtype=dtype)
        assert it == its[g] and hist == hists[g]
        assert np.array_equal(X[keep, g * gc:(g + 1) * gc], x)
        assert not X[masks[g], g * gc:(g + 1) * gc].any()


def test_the_seqsum_test_operator_is_indefinite_and_this_one_is_not():
    """why these tests bring their own operator: A + A.T + 4 I of tests/test_gpu_seqsum.py has negative eigenvalues (fine for its bit
    comparisons, useless for a tolerance)"""
    A = sparse.random(300, 300, density=8.0 / 300, random_state=300, format='csr')
    assert np.linalg.eigvalsh((A + A.T + sparse.identity(300) * 4.0).toarray())[0] < 0
    lo = np.linalg.eigvalsh(cg_ref.laplacian_plus(300, 300).toarray())
    assert 0.99 <= lo[0] and lo[-1] < 40


def test_the_table_holds_every_shape_the_issue_names():
    ids = set(cg_cases.BY_ID)
    for dt in ('f64', 'f32'):
        assert {'width-C%d-%s' % (C, dt) for C in cg_cases.WIDTHS} <= ids
        assert {'rows-n%d-C%d-%s' % (n, C, dt) for n in cg_cases.ROWS_N for C in (3, 17, 100)} <= ids
    assert {'cap-%d-f64' % c for c in cg_cases.CAPS} <= ids
    assert {'large-C3-f64', 'large-C17-f64'} <= ids


@pytest.mark.parametrize('case', cg_cases.CASES, ids=[c['id'] for c in cg_cases.CASES])
def test_case_is_definite_decided_and_counts_agree(case):
    s = cg_cases.build(case)
    A, n = s['A'], case['n']
    # definiteness (of the operator as the device holds it: entries rounded to the case's format)
    if case['op'] == 'banded':
        d = A.diagonal()
        off = np.asarray(abs(A).sum(axis=1)).ravel() - np.abs(d)
        assert np.all(d > off) and abs(A - A.T).max() == 0
    else:
        d = A.diagonal()
        off = np.asarray(abs(A).sum(axis=1)).ravel() - np.abs(d)
        assert np.min(d - off) >= 0.99 * case['tau'] and abs(A - A.T).max() == 0        # Gershgorin: every eigenvalue >= tau, nearly
        if n <= 1100:
            lo = np.linalg.eigvalsh(A.toarray())[0]
            assert lo >= 0.99 * case['tau'], lo
    ref = cg_cases.reference(case['id'])
    tol = case['tol']
    m_ld, m_own = cg_cases.margin(ref.ld[2], tol), cg_cases.margin(ref.own[2], tol)
    assert m_ld >= cg_cases.MIN_MARGIN > cg_cases.STOP_BAND and m_own >= cg_cases.MIN_MARGIN, (m_ld, m_own)
    assert ref.ld[1] == ref.own[1]
    assert np.array_equal(np.isnan(ref.ld[0]), np.isnan(ref.own[0]))
    dx, de, scale = cg_cases.d_ref(ref, cg_ref.EPS[case['dt']])
    # the restatement's own error against long double: what the device's bound is a multiple of (fp64: some 1e-16, fp32: some 1e-7)
    assert dx <= 64 * cg_ref.EPS[case['dt']], dx
    # what the case is there for
    its = ref.ld[1]
    if case['id'].startswith(('width', 'rows', 'renum', 'x0-', 'stack', 'sparse')) and n >= 63:
        assert all((1 if case['rhs'] == 'spread' else 10) <= it <= 60 for it in its), its
    if case['id'].startswith('stack') and len(its) >= 7:
        assert max(its) - min(its) >= 3, its                       # the systems stop several iterations apart
    if case['id'].startswith(('zerocol', 'zerosystem')):
        assert its[0] == 1 and np.isnan(ref.ld[0][:, case['zero_cols'][0]]).all()
    if case['id'].startswith('eigenvector'):
        assert its == [1]
    if case['id'].startswith('tol'):
        assert its == [0]
    if case['id'].startswith('large'):
        assert its == [6]
    if case['id'].startswith('cap'):
        full = cg_cases.reference('cap-36-f64').ld[1][0]
        assert 24 < full < 36 and its == [min(case['max_iter'], full)]
