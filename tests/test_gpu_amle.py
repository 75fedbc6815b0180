"""graph.amle, graph._amle_batch, _hip.lip_iterate and ssl.amle on the device: the golden vectors of the compiled reference bit for
bit (u and sweeps done), a randomised sweep against the restatement, the degenerate graphs, the batched form against single calls
with columns that stop at different sweeps, the learner against the golden fits, the progress lines, and one case under the
library's off switches.

Every test runs under a time limit of its own: a test that exceeds it ends the whole session on the spot (traceback of every
thread, then exit), so nothing more is started on a device that may have hung; nothing is retried."""
import faulthandler
import os
import sys

import numpy as np
import pytest
from scipy import sparse

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import amle_ref as ref  # noqa: E402
from test_amle_host import load_golden, golden_graph, golden_entries, golden_case, random_problem  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(240, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope='module')
def gl():
    import graphlearning_amd as gl
    from graphlearning_amd import _hip
    _hip.require_device()
    return gl


@pytest.fixture(scope='module')
def gold():
    return load_golden()


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return ref.build_host_lib(tmp_path_factory.mktemp('lip_plan'))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run_case(gl, gold, name):
    """The case through the public calls where it is graph.amle's (alpha 0, beta 1), else through _hip.lip_iterate: (u (n, B), sweeps)."""
    from graphlearning_amd import _hip
    gname, ind, vals, weighted, tol, T, alpha, beta, U, sweeps, errs = golden_case(gold, name)
    W, rows, nbr, V = golden_entries(gold, gname)
    G = gl.graph(W)
    if alpha == 0.0 and beta == 1.0:
        cols, its = [], []
        for b in range(vals.shape[1]):
            cols.append(G.amle(ind, np.ascontiguousarray(vals[:, b]), tol=tol, max_num_it=T, weighted=weighted))
            its.append(G.amle_iters)
            assert cols[-1].dtype == np.float64 and cols[-1].shape == (W.shape[0],) and G.amle_levels == int(gold[name + '_levels'])
        return np.stack(cols, axis=1), np.array(its)
    G.__ccode_init__()
    assert np.array_equal(G.J, nbr) and np.array_equal(G.I, rows)
    u, its, plan, _ = _hip.lip_iterate(W.shape[0], G.J, G.I, G.V, ind.astype(np.int32), vals, weighted, alpha, beta, T, tol)
    assert plan[0] == int(gold[name + '_levels'])
    return u, its


@pytest.mark.parametrize('name', sorted(ref.GOLDEN_CASES))
def test_golden_bit_for_bit(gl, gold, name):
    U, sweeps = golden_case(gold, name)[8:10]
    u, its = run_case(gl, gold, name)
    print(name, 'sweeps', its.tolist(), 'want', sweeps.tolist(), 'differing values', int((u != U).sum()))
    assert np.array_equal(its, sweeps)
    assert same_bits(u, U)


def test_randomised_sweep_against_restatement(gl, lib):
    """40-300 vertices, symmetric and directed, with and without diagonal entries, both solvers, T on both sides of 22, alpha != 0
    (unweighted form), a boundary vertex listed twice."""
    from graphlearning_amd import _hip
    rng = np.random.default_rng(2025)
    for trial in range(48):
        n, W, ind, val, weighted, T, tol, alpha, beta = random_problem(rng, trial)
        if trial % 6 == 0:                       # listed twice: the last value counts
            ind = np.concatenate([ind, ind[:1]])
            val = np.concatenate([val, [0.75]])
        rows, nbr, V = ref.entries(W)
        want_u, want_it, want_e = ref.host_sweeps(lib, n, rows, nbr, V, ind, val, weighted, alpha, beta, T, tol, False)
        what = (trial, n, weighted, T, tol, alpha)
        G = gl.graph(W)
        if alpha == 0.0:
            u = G.amle(ind, val, tol=tol, max_num_it=T, weighted=weighted)
            assert same_bits(u, want_u) and G.amle_iters == want_it, what
        u2, its, plan, errs = _hip.lip_iterate(n, nbr, rows, V, ind.astype(np.int32), val[:, None], weighted, alpha, beta, T, tol,
                                                 want_errors=True)
        assert same_bits(np.ascontiguousarray(u2[:, 0]), want_u) and its.tolist() == [want_it], what
        assert errs[:want_it, 0].tolist() == want_e and np.isnan(errs[want_it:, 0]).all(), what
        mask, _ = ref.boundary(n, ind, val)
        assert plan[0] == int(ref.levels(n, rows, nbr, mask).max()) + 1, what


def test_python_restatement_on_the_device_too(gl):
    """A few small problems against the interpreted form itself (the other tests lean on the compiled host restatement)."""
    rng = np.random.default_rng(5)
    for trial in range(4):
        n, W, ind, val, weighted, T, tol, alpha, beta = random_problem(rng, trial)
        rows, nbr, V = ref.entries(W)
        want_u, want_it, _ = ref.sequential(n, rows, nbr, V, ind, val, weighted, 0.0, 1.0, min(T, 30), tol)
        G = gl.graph(W)
        u = G.amle(ind, val, tol=tol, max_num_it=min(T, 30), weighted=weighted)
        assert same_bits(u, want_u) and G.amle_iters == want_it, trial


def test_degenerate_graphs(gl, lib):
    for weighted in (False, True):
        # two vertices, both boundary: nothing to update; the reference still counts its sweeps (err = 0 < tol after sweep 21)
        W2 = sparse.csr_matrix(np.array([[0.0, 1.0], [1.0, 0.0]]))
        G = gl.graph(W2)
        u = G.amle([0, 1], np.array([0.25, -1.0]), weighted=weighted)
        assert np.array_equal(u, [0.25, -1.0]) and G.amle_iters == 22 and G.amle_levels == 0
        G.amle([0, 1], np.array([0.25, -1.0]), weighted=weighted, max_num_it=7)
        assert G.amle_iters == 7
        # all but one vertex boundary
        rng = np.random.default_rng(1)
        n = 50
        A = sparse.random(n, n, density=0.2, random_state=3, format='csr')
        A = A.maximum(A.T).tocsr() + sparse.diags(np.ones(n - 1), 1) + sparse.diags(np.ones(n - 1), -1)
        A = sparse.csr_matrix(A)
        ind = np.delete(np.arange(n), 17)
        val = rng.random(n - 1)
        rows, nbr, V = ref.entries(A)
        want_u, want_it, _ = ref.host_sweeps(lib, n, rows, nbr, V, ind, val, weighted, 0.0, 1.0, 1000, 1e-5, False)
        G = gl.graph(A)
        u = G.amle(ind, val, weighted=weighted)
        assert same_bits(u, want_u) and G.amle_iters == want_it and G.amle_levels == 1
        # a star: the hub between leaves that all belong to level 0 or 1
        n = 400
        hub = 123
        leaves = np.delete(np.arange(n), hub)
        S = sparse.csr_matrix((0.5 + rng.random(n - 1), (np.full(n - 1, hub), leaves)), shape=(n, n))
        S = (S + S.T).tocsr()
        ind = np.array([0, 5, 399])
        val = np.array([1.0, -2.0, 0.5])
        rows, nbr, V = ref.entries(S)
        want_u, want_it, _ = ref.host_sweeps(lib, n, rows, nbr, V, ind, val, weighted, 0.0, 1.0, 1000, 1e-5, False)
        G = gl.graph(S)
        u = G.amle(ind, val, weighted=weighted)
        assert same_bits(u, want_u) and G.amle_iters == want_it and G.amle_levels == 3
        # the path graph in index order: as many levels as free vertices, one merged launch per sweep
        n = 700
        P = (sparse.diags(np.ones(n - 1), 1) + sparse.diags(np.ones(n - 1), -1)).tocsr()
        rows, nbr, V = ref.entries(P)
        want_u, want_it, _ = ref.host_sweeps(lib, n, rows, nbr, V, [0, n - 1], [0.0, 1.0], weighted, 0.0, 1.0, 60, 1e-5, False)
        G = gl.graph(P)
        u = G.amle([0, n - 1], np.array([0.0, 1.0]), weighted=weighted, max_num_it=60)
        assert same_bits(u, want_u) and G.amle_iters == want_it == 60 and G.amle_levels == n - 2
    # T = 0: zeros with the boundary values set
    u = gl.graph(P).amle([0, n - 1], np.array([0.5, 1.0]), max_num_it=0)
    assert u[0] == 0.5 and u[-1] == 1.0 and not u[1:-1].any() and gl.graph(P).amle([3], 1.0, max_num_it=0)[3] == 1.0


@pytest.mark.parametrize('B', [1, 3, 10, 33])
def test_batch_equals_single_calls(gl, gold, B):
    """Columns with boundary values of very different size stop at different sweeps; a column frozen early is bit-identical to its own
    run, whatever the others go on doing (the largest columns run into the cap of 250 sweeps).  Both solvers; a graph whose levels get launches of their own and one of merged levels."""
    rng = np.random.default_rng(100 + B)
    for gname, weighted, tol in (('diag', False, 1e-4), ('diag', True, 1e-3), ('ball', False, 1e-4), ('ball', True, 1e-2)):
        W = golden_graph(gold, gname)
        n = W.shape[0]
        G = gl.graph(W)
        ind = np.sort(rng.choice(n, size=9, replace=False))
        vals = rng.random((9, B)) * np.array([1e-4, 10.0, 1e-2, 1.0])[np.arange(B) % 4][None, :]
        U = G._amle_batch(ind, vals, tol=tol, max_num_it=250, weighted=weighted)
        its = np.array(G.amle_iters)
        assert U.shape == (n, B) and U.dtype == np.float64 and its.shape == (B,)
        for b in range(B):
            u = G.amle(ind, np.ascontiguousarray(vals[:, b]), tol=tol, max_num_it=250, weighted=weighted)
            assert same_bits(np.ascontiguousarray(U[:, b]), u) and G.amle_iters == its[b], (gname, weighted, B, b)
        if B > 1:
            assert len(set(its.tolist())) > 1, (gname, weighted, its)          # the columns did stop at different sweeps
            assert its.min() >= 22


def test_ssl_amle_against_golden_fits(gl, gold):
    W = golden_graph(gold, 'blobs')
    lab, ti = gold['graph_blobs_labels'], gold['fit_train_ind']
    for tag, weighted in (('u', False), ('w', True)):
        want_prob, want_sweeps = gold['blobs_%s_3_u' % tag], gold['blobs_%s_3_sweeps' % tag]
        for ptag, kw in (('plain', {}), ('priors', {'class_priors': gold['fit_priors']})):
            model = gl.ssl.amle(W, weighted=weighted, **kw)
            pred = model.fit_predict(ti, lab[ti])
            assert same_bits(np.asarray(model.prob, dtype=np.float64), want_prob), (tag, ptag)
            assert model.num_iter == want_sweeps.tolist()
            assert np.array_equal(pred, gold['fit_%s_%s_pred' % (tag, ptag)]), (tag, ptag)
        # the class-by-class loop of the base class gives the same scores
        model = gl.ssl.amle(W, weighted=weighted)
        model._fit_onevsrest = lambda *a: None
        assert same_bits(np.asarray(model.fit(ti, lab[ti]), dtype=np.float64), want_prob)


def test_prog_lines_are_the_error_history(gl, gold, capfd):
    for name in ('diag_u', 'stop_T5_w'):
        gname, ind, vals, weighted, tol, T, alpha, beta, U, sweeps, errs = golden_case(gold, name)
        G = gl.graph(golden_graph(gold, gname))
        capfd.readouterr()
        u = G.amle(ind, vals[:, 0], tol=tol, max_num_it=T, weighted=weighted, prog=True)
        out = capfd.readouterr().out
        assert same_bits(u, np.ascontiguousarray(U[:, 0]))
        assert out == ''.join('Iter=%d, err=%.15f\n' % (it, errs[it, 0]) for it in range(int(sweeps[0])))


def test_identical_under_the_off_switches(gl, gold):
    """The pool bypassed, pooled blocks poisoned, transfers straight from the caller's memory: the same bits."""
    from graphlearning_amd import _hip
    name = 'blobsdir_u'
    U, sweeps = golden_case(gold, name)[8:10]

    def check():
        u, its = run_case(gl, gold, name)
        assert same_bits(u, U) and np.array_equal(its, sweeps)
    _hip.pool_set_enabled(False)
    try:
        check()
    finally:
        _hip.pool_set_enabled('nopool' not in os.environ.get('GLX_TEST_ABLATE', ''))
    _hip.upload_set_mode(2)
    try:
        check()
    finally:
        _hip.upload_set_mode(2 if 'pageableupload' in os.environ.get('GLX_TEST_ABLATE', '') else 0)
    _hip.pool_set_poison(0x7f)
    try:
        check()
    finally:
        session = [a for a in os.environ.get('GLX_TEST_ABLATE', '').split(',') if a.startswith('poison')]
        _hip.pool_set_poison(int(session[0][6:] or '255') if session else -1)


def test_more_columns_than_a_workgroup_folds_in_lds(gl, gold, lib):
    """70 columns: the errors go straight to the slots; every column against the host restatement."""
    rng = np.random.default_rng(70)
    W, rows, nbr, V = golden_entries(gold, 'diag')
    n = W.shape[0]
    ind = np.sort(rng.choice(n, size=6, replace=False))
    vals = rng.random((6, 70)) * (10.0 ** rng.integers(-3, 1, size=70))[None, :]
    for weighted, tol in ((False, 1e-3), (True, 1e-2)):
        G = gl.graph(W)
        U = G._amle_batch(ind, vals, tol=tol, max_num_it=2000, weighted=weighted)
        for b in range(70):
            want_u, want_it, _ = ref.host_sweeps(lib, n, rows, nbr, V, ind, np.ascontiguousarray(vals[:, b]), weighted, 0.0, 1.0, 2000, tol, False)
            assert same_bits(np.ascontiguousarray(U[:, b]), want_u) and G.amle_iters[b] == want_it, (weighted, b)
