"""ssl.plaplace / graph._plaplace_batch / glx_lp_iterate_batch without a GPU: the golden vectors of the compiled reference
(tests/golden/make_golden_plaplace.py) against the restatements, the host bookkeeping of csrc/lp_plan.h with its chunked two-buffer
schedule (tests/lp_plan_host.cpp: a plain loop stands in for the kernel) against the oracle column by column, and the surface: the entry
point is declared and exported, the constructor's attributes, the refusals raised before any device call."""
import os
import re
import sys

import numpy as np
import pytest
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import amle_ref                     # noqa: E402
import plaplace_ref as ref          # noqa: E402
import graphlearning_amd as gl      # noqa: E402
from graphlearning_amd import _hip  # noqa: E402

CAPS = (0, 1, 11, 12, 57, 200)


@pytest.fixture(scope='module')
def gold():
    return ref.load_golden()


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return ref.build_host_lib(tmp_path_factory.mktemp('lp_plan'))


def case_inputs(gold, name):
    gname, fast, p, tol, T = ref.GOLDEN_CASES[name]
    ti = gold['graph_%s_train_ind' % gname]
    tl = gold['graph_%s_labels' % gname][ti]
    return gname, fast, p, tol, int(T), ti, tl, ref.class_columns(tl)


def test_golden_holds_the_cases_the_feature_names(gold):
    assert set(ref.GOLDEN_CASES) <= set(gold['entry_names'].tolist())
    for gname, spec in ref.GOLDEN_GRAPHS.items():
        W = ref.golden_graph(gold, gname)
        assert W.shape[0] == spec['n'] and np.diff(W.indptr).min() >= 1 and W.data.min() > 0, gname            # no empty row
        I, J, V = ref.golden_entries(gold, gname)
        assert (np.diff(I) >= 0).all() and len(I) == W.nnz
        assert (sparse.csr_matrix((V, (I, J)), shape=W.shape) != W).nnz == 0                                   # the entry lists are the graph's
        assert len(gold['graph_%s_train_ind' % gname]) == spec['C'] * spec['per_class']
    assert (abs(ref.golden_graph(gold, 'blobs3') - ref.golden_graph(gold, 'blobs3').T) > 0).nnz == 0
    assert (abs(ref.golden_graph(gold, 'blobs10_dir') - ref.golden_graph(gold, 'blobs10_dir').T) > 0).nnz > 0     # directed
    its = gold['b3_jac_p10_iters']
    assert len(set(its.tolist())) > 1 and set((its % 2).tolist()) == {0, 1}, its          # different stops, both parities
    assert gold['b3_jac_T57_iters'].tolist() == [57] * 3 and gold['b3_jac_T200_iters'].tolist() == [200] * 3
    assert gold['b3_jac_T0_iters'].tolist() == [0] * 3
    assert gold['b10_jac_p10_prob'].shape == (1500, 10) and gold['b3_jac_p10_priors_pred'].shape == (2000,)


@pytest.mark.parametrize('name', sorted(n for n, c in ref.GOLDEN_CASES.items() if not c[1]))
def test_oracle_equals_golden_jacobi(gold, name):
    """oracle.gl_oracle's restatement of lp_iterate_main, per column on the stored entry lists: prob and iterations bit for bit."""
    gname, fast, p, tol, T, ti, tl, vals = case_inputs(gold, name)
    I, J, V = ref.golden_entries(gold, gname)
    n = len(gold['graph_%s_labels' % gname])
    uu, ul, its = ref.oracle_batch(n, I, J, V, ti, vals, p, T, tol)
    assert np.array_equal(its, gold[name + '_iters'])
    assert ((uu + ul) / 2).tobytes() == gold[name + '_prob'].tobytes()


@pytest.mark.parametrize('name', sorted(n for n, c in ref.GOLDEN_CASES.items() if c[1]))
def test_restatement_equals_golden_fast(gold, name, tmp_path):
    """amle_ref's restatements of lip_iterate_main with alpha = 1/(p-1), beta = 1-alpha, tol 1e-6: every column with the compiled
    host form, the shortest column also with the interpreted one."""
    gname, fast, p, tol, T, ti, tl, vals = case_inputs(gold, name)
    I, J, V = ref.golden_entries(gold, gname)
    n = len(gold['graph_%s_labels' % gname])
    alib = amle_ref.build_host_lib(tmp_path)
    alpha = 1 / (p - 1)
    beta = 1 - alpha
    want, its = gold[name + '_prob'], gold[name + '_iters']
    for b in range(vals.shape[1]):
        u, done, _ = amle_ref.host_sweeps(alib, n, I, J, V, ti, np.ascontiguousarray(vals[:, b]), False, alpha, beta, T, 1e-6, False)
        assert u.tobytes() == np.ascontiguousarray(want[:, b]).tobytes() and done == its[b], (name, b)
    b = int(np.argmin(its))
    if its[b] * len(J) <= 2500000:
        u, done, _ = amle_ref.sequential(n, I, J, V, ti, np.ascontiguousarray(vals[:, b]), False, alpha, beta, T, 1e-6)
        assert u.tobytes() == np.ascontiguousarray(want[:, b]).tobytes() and done == its[b], (name, b)


def test_interpreted_restatement_covers_a_fast_golden(gold):
    its = gold['b10_fast_p10_iters']
    assert its.min() * len(gold['graph_blobs10_dir_J']) <= 2500000


def check_against_oracle(lib, n, I, J, V, ind, vals, p, T, tol, chunk=None):
    uu, ul, its = ref.host_run(lib, n, I, J, V, ind, vals, p, T, tol, chunk)
    ouu, oul, oits = ref.oracle_batch(n, I, J, V, ind, vals, p, T, tol)
    what = (n, vals.shape[1], p, T, tol, chunk)
    assert np.array_equal(its, oits), (what, its, oits)
    assert ref.same(uu, ouu) and ref.same(ul, oul), what
    return its


@pytest.mark.parametrize('name', sorted(n for n, c in ref.GOLDEN_CASES.items() if not c[1] and c[0] == 'blobs3'))
def test_host_schedule_on_the_golden_jacobi_cases(gold, lib, name):
    gname, fast, p, tol, T, ti, tl, vals = case_inputs(gold, name)
    I, J, V = ref.golden_entries(gold, gname)
    its = check_against_oracle(lib, 2000, I, J, V, ti, vals, p, T, tol)
    assert np.array_equal(its, gold[name + '_iters'])
    uu, ul, _ = ref.host_run(lib, 2000, I, J, V, ti, vals, p, T, tol)
    assert ((uu + ul) / 2).tobytes() == gold[name + '_prob'].tobytes()


def test_host_schedule_caps_and_chunk_lengths(gold, lib):
    """The caps on both sides of the first possible stop (11), odd and even, on the golden graph, the scaled columns (different stops in
    one call) and the constant columns (stop at 11 exactly); chunk lengths 1 and 7 beside the library's, so that a stop lands on every
    position of a chunk and the carried slot decides the first iteration of the next."""
    gname, fast, p, tol, T, ti, tl, vals = case_inputs(gold, 'b3_jac_p10')
    problems = [(2000,) + ref.golden_entries(gold, gname) + (ti, vals, 10, 1e-1)]
    for B in (1, 7):
        W, ind, sv = ref.scaled_problem(B)
        problems.append((W.shape[0],) + ref.entries(W) + (ind, sv, 4.0, 1e-3))
    W, ind, cv = ref.constant_problem(3)
    problems.append((W.shape[0],) + ref.entries(W) + (ind, cv, 10, 1e-1))
    for n, I, J, V, ind, v, p, tol in problems:
        for T in CAPS:
            for chunk in (None, 1, 7):
                check_against_oracle(lib, n, I, J, V, ind, v, p, T, tol, chunk)
    # run to the stop: the scaled columns stop at different iterations, of both parities; the constant ones at 11
    W, ind, sv = ref.scaled_problem(7)
    I, J, V = ref.entries(W)
    for chunk in (None, 1, 7):
        its = check_against_oracle(lib, W.shape[0], I, J, V, ind, sv, 4.0, 10 ** 6, 1e-3, chunk)
    assert len(set(its.tolist())) >= 4 and set((its % 2).tolist()) == {0, 1}, its
    W, ind, cv = ref.constant_problem(3)
    I, J, V = ref.entries(W)
    for chunk in (None, 1, 7):
        its = check_against_oracle(lib, W.shape[0], I, J, V, ind, cv, 10, 10 ** 6, 1e-1, chunk)
        assert its.tolist() == [11, 11, 11]


def test_which_iterate_the_first_buffer_holds(lib):
    """lp_result_iterate: a column that stopped at S returns U_S (S even) or U_{S+1} (S odd); one that ran into the cap U_T or
    U_{T-1}: always an even iterate, which the oracle returns when it runs exactly that many iterations without a stop test."""
    W, ind, sv = ref.scaled_problem(7)
    I, J, V = ref.entries(W)
    n = W.shape[0]
    for T in (10 ** 6, 57, 200, 12, 1):
        uu, ul, its = ref.host_run(lib, n, I, J, V, ind, sv, 4.0, T, 1e-3)
        for b in range(sv.shape[1]):
            k = lib.lpb_result_iterate(int(its[b]), T)
            assert k % 2 == 0 and k in (its[b], its[b] + 1, T, T - 1)
            wu, wl, _ = ref.oracle_column(n, I, J, V, ind, sv[:, b], 4.0, k, -1.0)       # tol < 0: never stops
            assert ref.same(uu[:, b], wu) and ref.same(ul[:, b], wl), (T, b, its[b], k)
    assert [lib.lpb_result_iterate(s, 100) for s in (11, 12, 99, 100)] == [12, 12, 100, 100]
    assert [lib.lpb_result_iterate(s, 57) for s in (56, 57)] == [56, 56] and lib.lpb_result_iterate(0, 0) == 0


def test_host_plan(lib):
    """Vertex blocks, invdeg, dt, start values and the boundary map: a vertex without entries (alpha / 0), a vertex listed twice (its
    last row), a NaN value (np.max / np.min give NaN), and what is refused."""
    W = ref.random_graph(60, 5).tolil()
    W[7, :] = 0
    W[:, 7] = 0
    W = sparse.csr_matrix(W)
    W.eliminate_zeros()
    I, J, V = ref.entries(W)
    ind = np.array([3, 9, 3, 20])
    vals = np.array([[1.0, 0.5], [-2.0, np.nan], [4.0, 0.25], [0.0, 1.0]])
    rc, plan = ref.host_plan(lib, 60, I, J, V, ind, vals, 4.0)
    assert rc == 0
    assert np.array_equal(plan['start'], np.concatenate(([0], np.cumsum(np.bincount(I, minlength=60)))))
    deg = np.zeros(60)
    for i in range(60):           # the degree is summed left to right
        d = 0.0
        for w in V[plan['start'][i]:plan['start'][i + 1]]:
            d += w
        deg[i] = d
    with np.errstate(divide='ignore'):
        assert plan['invdeg'].tobytes() == ((1 / 4.0) / deg).tobytes() and np.isinf(plan['invdeg'][7])
    assert plan['alpha'] == 1 / 4.0 and plan['delta'] == 1 - 2 / 4.0 and plan['dt'] == 0.9 / (1 / 4.0 + 2 * (1 - 2 / 4.0)) / V.max()
    want = np.full(60, -1)
    want[[3, 9, 20]] = [2, 1, 3]
    assert np.array_equal(plan['bdy'], want)
    assert plan['hi'][0] == 4.0 and plan['lo'][0] == -2.0 and np.isnan(plan['hi'][1]) and np.isnan(plan['lo'][1])
    c = ref.host_constants(lib)
    assert c == dict(block=256, chunk=c['chunk'], lds_cols=c['lds_cols'], max_cols=256) and 1 <= c['chunk'] <= 1024 and 1 <= c['lds_cols'] < 67
    good = np.zeros((4, 2))
    assert ref.host_plan(lib, 60, I, J, V, np.array([3, 9, 60, 20]), good, 4.0)[0] == 1            # boundary index out of range
    assert ref.host_plan(lib, 60, I, J + 60 * (np.arange(len(J)) == 5), V, ind, good, 4.0)[0] == 1     # neighbour index out of range
    assert ref.host_plan(lib, 60, I, J, V, ind, np.zeros((4, 257)), 4.0)[0] == 2                    # wider than the cap
    assert ref.host_plan(lib, 60, I, J, V, ind, np.zeros((4, 256)), 4.0)[0] == 0
    assert ref.host_plan(lib, 60, I, J, V, ind, good, 4.0, T=(1 << 24) + 1)[0] == 2
    assert ref.host_plan(lib, 60, I, J, V, ind, good, 4.0, T=1 << 24)[0] == 0


def test_symbol_declared_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'glx_experimental.h')).read()
    assert re.search(r'\bint\s+glx_lp_iterate_batch\s*\(', hdr)
    assert 'glx_lp_iterate_batch' not in open(os.path.join(ROOT, 'include', 'glx.h')).read()
    assert 'glx_lp_iterate_batch' in _hip.EXPORTED_SYMBOLS
    assert getattr(_hip.load(), 'glx_lp_iterate_batch') is not None
    assert callable(_hip.lp_iterate_batch)
    plan_h = open(os.path.join(ROOT, 'graphlearning_amd', 'csrc', 'lp_plan.h')).read()
    assert '<hip' not in plan_h and 'glx_internal.h' not in plan_h                    # host-only


def _path_graph(n=6):
    return (sparse.diags([1.0] * (n - 1), 1) + sparse.diags([1.0] * (n - 1), -1)).tocsr()


def test_constructor():
    W = _path_graph()
    m = gl.ssl.plaplace(W)
    assert m.p == 10 and m.max_num_it == 1e6 and m.fast is True and m.tol == 1e-5 and m.onevsrest is True
    assert m.accuracy_filename == '_plaplace_p10.00' and m.name == 'p-Laplace (p=10.00)'
    assert m.get_accuracy_filename() == '_plaplace_p10.00_accuracy.csv'
    m = gl.ssl.plaplace(W, p=3, tol=1e-2, max_num_it=500, fast=False)
    assert m.p == 3 and m.max_num_it == 500 and m.fast is False and m.tol == 1e-2 and m.onevsrest is True
    assert m.accuracy_filename == '_plaplace_p3.00' and m.name == 'p-Laplace (p=3.00)'
    m = gl.ssl.plaplace(W, class_priors=np.array([1.0, 3.0]), p=2.5, tol=0.3)
    assert m.tol == 1e-5 and np.array_equal(m.class_priors, [0.25, 0.75])
    assert m.get_accuracy_filename() == '_plaplace_p2.50_classpriors_accuracy.csv'
    assert callable(gl.graph(W)._plaplace_batch)


def test_refusals_are_raised_before_any_device_call(monkeypatch):
    def reached(*a, **k):
        raise AssertionError('the device call was reached')
    monkeypatch.setattr(_hip, 'lip_iterate', reached)
    monkeypatch.setattr(_hip, 'lp_iterate_batch', reached)
    monkeypatch.setattr(_hip, 'lp_iterate', reached)
    G = gl.graph(_path_graph())
    good = np.array([[0.0, 1.0], [1.0, 0.0]])
    # fast=True: what _amle_batch refuses
    for bad in (np.array([[0.0, np.nan], [1.0, 0.0]]), np.array([[np.inf, 1.0], [1.0, 0.0]])):
        with pytest.raises(ValueError):
            G._plaplace_batch([0, 5], bad, 10)
    with pytest.raises(ValueError):
        G._plaplace_batch([0, 6], good, 10)
    with pytest.raises(ValueError):
        G._plaplace_batch([0, 5], good, 10, max_num_it=1e9)
    with pytest.raises(ValueError):
        G._plaplace_batch([0, 5], np.zeros((3, 2)), 10)
    for w in (-1.0, np.nan):
        Wn = _path_graph().tolil()
        Wn[1, 2] = w
        with pytest.raises(ValueError):
            gl.graph(Wn.tocsr())._plaplace_batch([0, 5], good, 10)
    We = _path_graph().tolil()
    We[3, 2] = 0
    We[3, 4] = 0
    We = We.tocsr()
    We.eliminate_zeros()
    with pytest.raises(ValueError):
        gl.graph(We)._plaplace_batch([0, 5], good, 10)
    with pytest.raises(AssertionError, match='device call was reached'):
        gl.graph(We)._plaplace_batch([0, 3, 5], np.zeros((3, 2)), 10)            # on the boundary it is fine
    with pytest.raises(ZeroDivisionError):
        G._plaplace_batch([0, 5], good, 1)                                         # alpha = 1/(p-1), as the reference
    # fast=False
    with pytest.raises(ValueError):
        G._plaplace_batch([0, 5], np.zeros((3, 2)), 10, fast=False)
    with pytest.raises(ValueError):
        G._plaplace_batch([0, 5], np.zeros(2), 10, fast=False)
    with pytest.raises(ValueError):
        G._plaplace_batch([0, 6], good, 10, fast=False)
    with pytest.raises(ValueError):
        G._plaplace_batch([-1, 5], good, 10, fast=False)
    with pytest.raises(ValueError):
        G._plaplace_batch([0, 5], good, 10, max_num_it=(1 << 24) + 1, fast=False)
    with pytest.raises(AssertionError, match='device call was reached'):
        gl.graph(We)._plaplace_batch([0, 5], good, 10, fast=False)                # a vertex without entries: NaN there, as the single call
    with pytest.raises(AssertionError, match='device call was reached'):
        G._plaplace_batch([0, 5], good, 10, max_num_it=1 << 24, fast=False)
    # the learner refuses the same way, in both forms, and for a single class
    for fast in (True, False):
        with pytest.raises(ValueError):
            gl.ssl.plaplace(_path_graph(), fast=fast).fit(np.array([0, 6]), np.array([0, 1]))
        with pytest.raises(ValueError):
            gl.ssl.plaplace(_path_graph(), fast=fast, max_num_it=1e9).fit(np.array([0, 5]), np.array([0, 1]))
        with pytest.raises(ValueError):
            gl.ssl.plaplace(_path_graph(), fast=fast)._fit(np.array([0, 6]), np.array([True, False]))
    with pytest.raises(ValueError):
        gl.ssl.plaplace(We).fit(np.array([0, 5]), np.array([0, 1]))
    with pytest.raises(AssertionError, match='device call was reached'):
        gl.ssl.plaplace(_path_graph()).fit(np.array([0, 5]), np.array([0, 1]))


def test_single_problem_fast_call_is_still_refused():
    G = gl.graph(_path_graph())
    with pytest.raises(NotImplementedError) as exc:
        G.plaplace(np.array([0, 5]), np.array([0.0, 1.0]), 4)
    assert 'sequential' not in str(exc.value) and 'lip_iterate' in str(exc.value)
