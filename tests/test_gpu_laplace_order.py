"""ssl.laplace(order=2 | 3), ssl.laplace(tau=<vector>) and ssl.randomwalk(alpha=...) on the device against the oracle BIT FOR BIT
(np.array_equal on u, equality on the iteration count), on the fixtures of tests/golden/g24_laplace_order.npz.

What order >= 2 changes (reference ssl.py:1223-1228 forms L*L, L*L*L with scipy's SpGEMM): the rows of L come out UNSORTED, 100 to
450 entries long, of both signs -- the operator M L M must keep that entry order, the right-hand side -L[:, train] * F must be summed
in it (hundreds of its rows have three and more terms), the fast canonical-row routes must step aside, the solves run for 120 to
470 iterations with masked rows (every one beyond ssl.AUTO_TREE_MAX_ITER, so the default mode has to hand back to the exact
reductions), and L of order 3 is not symmetric bit for bit.  tests/test_oracle_golden.py pins the oracle at these orders to the
reference's recorded u; the combinatorial tau = 0 cases are compared with the recorded u here as well.

Every test runs under a time limit of its own: a test that exceeds it ends the whole session on the spot (traceback of every
thread, then exit), so nothing more is started on a device that may have hung; nothing is retried."""
import faulthandler

import numpy as np
import pytest

import laplace_order_ref as lo
from oracle import gl_oracle as orc

pytestmark = pytest.mark.gpu
N = 600


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)
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
    return lo.load_golden()


@pytest.fixture(scope='module')
def graphs(gl, gold):
    """n -> W from the recorded kNN lists (no vertex order comes with it: the operator is uploaded with keep_order)."""
    out = {}
    for n in lo.SIZES:
        W = gl.weightmatrix.knn(lo.points(gold, n), lo.K, knn_data=lo.knn_lists(gold, n))
        assert getattr(W, '_glx_order', None) is None
        out[n] = W
    return out


_ORACLE = {}


def oracle_fit(W, tag, gold, n, order, norm, tau, ms, trial=0):
    """The oracle's (u, iterations) of a case, computed once per module and handed out read-only."""
    key = (tag, n, order, norm, tau, ms, trial)
    if key not in _ORACLE:
        ti, lab = lo.training_set(gold, n, trial)
        u, it = orc.laplace_fit(W, ti, lab, normalization=norm, tau=lo.tau_value(gold, n, tau), mean_shift=ms, tol=lo.TOL, order=order,
                                return_iters=True)
        u.setflags(write=False)
        _ORACLE[key] = (u, it)
    return _ORACLE[key]


def model_for(gl, gold, W, n, order, norm, tau, ms, **kw):
    return gl.ssl.laplace(W, normalization=norm, tau=lo.tau_value(gold, n, tau), order=order, mean_shift=ms, tol=lo.TOL, **kw)


GRID = [c for c in lo.CASES if c[0] == N and c[1] >= 2]
assert len(GRID) == 24


@pytest.mark.parametrize('n,order,norm,tau,ms', GRID, ids=[lo.case_key(*c) for c in GRID])
def test_exact_and_default_mode_equal_the_oracle(gl, gold, graphs, n, order, norm, tau, ms):
    from graphlearning_amd import ssl as glssl
    W = graphs[n]
    ti, lab = lo.training_set(gold, n)
    u_o, it_o = oracle_fit(W, 'lists', gold, n, order, norm, tau, ms)
    assert it_o == int(gold['iters_' + lo.case_key(n, order, norm, tau, ms)])
    assert it_o > glssl.AUTO_TREE_MAX_ITER                          # the default mode must hand this solve back
    model = model_for(gl, gold, W, n, order, norm, tau, ms, reduce='exact')
    u = model.fit(ti, lab)
    print('%s: iterations %d (oracle %d), max |u - oracle| %.3e' % (lo.case_key(n, order, norm, tau, ms), model.num_iter, it_o, np.abs(u - u_o).max()))
    assert model.num_iter == it_o
    assert np.array_equal(u, u_o)
    auto = model_for(gl, gold, W, n, order, norm, tau, ms)
    assert auto.reduce == 'auto'
    ua = auto.fit(ti, lab)
    assert auto.num_iter == it_o
    assert np.array_equal(ua, u_o)
    if norm == 'combinatorial' and tau == '0':                      # the reference's own u, not only the oracle's
        assert np.array_equal(u, gold['u_' + lo.case_key(n, order, norm, tau, ms)])


@pytest.mark.parametrize('norm,tau,ms', [('combinatorial', '0', False), ('normalized', 'vec', True)])
def test_two_thousand_vertices_order_two(gl, gold, graphs, norm, tau, ms):
    from graphlearning_amd import ssl as glssl
    n = 2000
    W = graphs[n]
    ti, lab = lo.training_set(gold, n)
    u_o, it_o = oracle_fit(W, 'lists', gold, n, 2, norm, tau, ms)
    assert it_o > glssl.AUTO_TREE_MAX_ITER
    for kw in (dict(reduce='exact'), {}):
        model = model_for(gl, gold, W, n, 2, norm, tau, ms, **kw)
        u = model.fit(ti, lab)
        assert model.num_iter == it_o, kw
        assert np.array_equal(u, u_o), kw
    if (norm, tau, ms) == ('combinatorial', '0', False):
        key = lo.case_key(n, 2, norm, tau, ms)
        assert it_o == int(gold['iters_' + key]) and np.array_equal(u, gold['u_' + key])


@pytest.mark.parametrize('n,order', [(N, 2), (N, 3), (4200, 2)])
def test_graph_built_on_the_device(gl, gold, n, order):
    """W from weightmatrix.knn(X, k): searched and assembled on the device.  From 4096 vertices on the search leaves its cell order on
    W and the operator of L*L is uploaded in that order, not the caller's (n = 4200; below, the caller's order is kept)."""
    from graphlearning_amd import ssl as glssl
    if n == N:
        X, (ti, lab) = lo.points(gold, n), lo.training_set(gold, n)
    else:
        rng = np.random.default_rng(n)
        truth = rng.integers(0, lo.CLASSES, size=n)
        X = (rng.normal(size=(lo.CLASSES, lo.DIM)) * 1.5)[truth] + rng.normal(size=(n, lo.DIM))
        ti = np.concatenate([rng.choice(np.flatnonzero(truth == c), lo.PER_CLASS, replace=False) for c in range(lo.CLASSES)])
        lab = truth[ti]
    W = gl.weightmatrix.knn(X, lo.K)
    assert (getattr(W, '_glx_order', None) is not None) == (n >= 4096)
    for norm, tau in (('combinatorial', 0), ('normalized', 0.01)):
        u_o, it_o = orc.laplace_fit(W, ti, lab, normalization=norm, tau=tau, tol=lo.TOL, order=order, return_iters=True)
        assert it_o > glssl.AUTO_TREE_MAX_ITER
        for kw in (dict(reduce='exact'), {}):
            model = gl.ssl.laplace(W, normalization=norm, tau=tau, order=order, tol=lo.TOL, **kw)
            u = model.fit(ti, lab)
            assert model.num_iter == it_o, (norm, kw)
            assert np.array_equal(u, u_o), (norm, kw)
            assert model._cache[3].info()['renumbered'] == int(n >= 4096)


def _count_calls(monkeypatch):
    from graphlearning_amd import _hip
    calls = []
    for name in ('cg_groups_rows', 'cg_groups', 'cg'):
        def shim(self, *a, _orig=getattr(_hip.DeviceGraph, name), _name=name, **kw):
            calls.append((_name, kw.get('reduce'), None if kw.get('masks') is None else len(kw['masks'])))
            return _orig(self, *a, **kw)
        monkeypatch.setattr(_hip.DeviceGraph, name, shim)
    return calls


@pytest.mark.parametrize('order', [1, 2, 3])
def test_route_and_operator_rows(gl, gold, graphs, monkeypatch, order):
    """Order >= 2 goes through cg_groups with one mask (the literal right-hand side), never through cg_groups_rows; order 1 on the
    same graph the other way.  The default mode asks for the tolerance mode first and the exact reductions last.  The operator on
    the device has the rows of L: its longest row is L's."""
    W = graphs[N]
    ti, lab = lo.training_set(gold, N)
    calls = _count_calls(monkeypatch)
    model = model_for(gl, gold, W, N, order, 'combinatorial', '0', False, reduce='exact')
    u = model.fit(ti, lab)
    want = 'cg_groups_rows' if order == 1 else 'cg_groups'
    assert calls == [(want, 'exact', 1)]
    L = orc.laplace_operator(W, 'combinatorial', 0, order)
    info = model._cache[3].info()
    assert info['max_row'] == lo.longest_row(L) and info['nnz'] == L.nnz and info['n_rows'] == N
    u_o, it_o = (oracle_fit(W, 'lists', gold, N, order, 'combinatorial', '0', False) if order > 1 else
                 orc.laplace_fit(W, ti, lab, tol=lo.TOL, return_iters=True))
    assert model.num_iter == it_o and np.array_equal(u, u_o)
    if order > 1:
        del calls[:]
        auto = model_for(gl, gold, W, N, order, 'combinatorial', '0', False)
        ua = auto.fit(ti, lab)
        assert calls == [('cg_groups', 'tree', 1), ('cg_groups', 'exact', 1)]       # 'auto' never returns the tolerance mode's answer
        assert np.array_equal(ua, u_o)


@pytest.mark.parametrize('order', lo.ORDERS)
def test_tolerance_mode_is_finite_and_never_what_auto_returns(gl, gold, graphs, order):
    """reduce='tree' at these lengths is measured (EXPERIMENTS.md), not bounded: solves of more than ssl.AUTO_TREE_MAX_ITER
    iterations are what the default mode hands back."""
    for n, norm, tau in [(N, nm, t) for nm in lo.NORMS for t in ('0', '0.01')] + ([(2000, 'combinatorial', '0')] if order == 2 else []):
        W = graphs[n]
        ti, lab = lo.training_set(gold, n)
        u_o, it_o = oracle_fit(W, 'lists', gold, n, order, norm, tau, False)
        tree = model_for(gl, gold, W, n, order, norm, tau, False, reduce='tree')
        ut = tree.fit(ti, lab)
        print('tree n %d order %d %-13s tau %-4s: iterations %d (oracle %d), max |u - oracle| %.3e, labels equal %s'
              % (n, order, norm, tau, tree.num_iter, it_o, np.abs(ut - u_o).max(), np.array_equal(orc.predict(ut), orc.predict(u_o))))
        assert np.isfinite(ut).all()
        auto = model_for(gl, gold, W, n, order, norm, tau, False)
        assert np.array_equal(auto.fit(ti, lab), u_o) and auto.num_iter == it_o


def test_trials_equal_single_fits(gl, gold, graphs, capsys):
    """ssl_trials over 5 training sets at order 2: _fit_batch, _rhs and the literal right-hand side -- per set the single fit's u
    and iteration count, bit for bit, and the single fit is the oracle's."""
    W = graphs[N]
    labels = gold['labels%d' % N]
    sets = [lo.training_set(gold, N, t)[0] for t in range(lo.TRIALS)]
    model = gl.ssl.laplace(W, order=2, tol=lo.TOL, reduce='exact')
    got = []
    inner = model._fit_batch

    def spy(trials):
        out = inner(trials)
        got.append(([np.array(u, copy=True) for u in out], list(model.num_iter)))
        return out

    model._fit_batch = spy
    model.ssl_trials(sets, labels, save_results=False)
    rows = [r for r in capsys.readouterr().out.splitlines() if r.startswith('%d,' % len(sets[0]))]
    assert len(got) == 1 and len(got[0][0]) == lo.TRIALS and len(rows) == lo.TRIALS
    single = gl.ssl.laplace(W, order=2, tol=lo.TOL, reduce='exact')
    iters = []
    for t, ti in enumerate(sets):
        u = single.fit(ti, labels[ti])
        u_o, it_o = oracle_fit(W, 'lists', gold, N, 2, 'combinatorial', '0', False, trial=t)
        assert single.num_iter == it_o and np.array_equal(u, u_o), t
        assert got[0][1][t] == it_o and np.array_equal(got[0][0][t], u), t
        assert rows[t] == '%d,%.2f' % (len(ti), orc.ssl_accuracy(orc.predict(u_o), labels, ti)), t
        iters.append(it_o)
    assert len(set(iters)) > 1                          # the systems of one batch really stop at different iterations
    # the default mode of the batch hands every system back as well
    auto = gl.ssl.laplace(W, order=2, tol=lo.TOL)
    together = auto._fit_batch([(ti, labels[ti]) for ti in sets])
    assert auto.num_iter == iters and all(np.array_equal(a, b) for a, b in zip(together, got[0][0]))


@pytest.mark.parametrize('norm', lo.NORMS)
def test_reweighting_with_order(gl, gold, graphs, norm, monkeypatch):
    """reweighting='wnll', order 2: the per-fit sub-matrix route, dev.cg on an unsorted M A M."""
    W = graphs[N]
    ti, lab = lo.training_set(gold, N)
    calls = _count_calls(monkeypatch)
    model = gl.ssl.laplace(W, reweighting='wnll', normalization=norm, order=2, tol=lo.TOL, reduce='exact')
    u = model.fit(ti, lab)
    assert calls == [('cg', 'exact', None)]
    u_o, it_o = orc.laplace_fit(orc.reweight(W, ti, 'wnll', normalization=norm), ti, lab, normalization=norm, tol=lo.TOL, order=2,
                                return_iters=True)
    assert model.num_iter == it_o and np.array_equal(u, u_o)


def test_state_follows_the_attributes(gl, gold, graphs):
    """One model object, its order and tau changed between fits: every fit equals a fresh model's, the way back included; an
    unchanged model keeps its operator on the device."""
    W = graphs[N]
    ti, lab = lo.training_set(gold, N)
    tau = np.array(gold['tau%d' % N])

    def fresh(**kw):
        m = gl.ssl.laplace(W, tol=lo.TOL, reduce='exact', **kw)
        return np.array(m.fit(ti, lab), copy=True), m.num_iter

    model = gl.ssl.laplace(W, tol=lo.TOL, reduce='exact')
    first = np.array(model.fit(ti, lab), copy=True)
    it1 = model.num_iter
    dev1 = model._cache[3]
    assert np.array_equal(model.fit(ti, lab), first) and model._cache[3] is dev1            # nothing changed: nothing rebuilt
    model.order = 2
    u2 = np.array(model.fit(ti, lab), copy=True)
    dev2 = model._cache[3]
    assert dev2 is not dev1
    f2 = fresh(order=2)
    assert model.num_iter == f2[1] and np.array_equal(u2, f2[0])
    assert np.array_equal(u2, oracle_fit(W, 'lists', gold, N, 2, 'combinatorial', '0', False)[0])
    assert np.array_equal(model.fit(ti, lab), u2) and model._cache[3] is dev2
    model.tau = tau
    u3 = np.array(model.fit(ti, lab), copy=True)
    f3 = fresh(order=2, tau=tau)
    assert model._cache[3] is not dev2 and model.num_iter == f3[1] and np.array_equal(u3, f3[0])
    assert np.array_equal(u3, oracle_fit(W, 'lists', gold, N, 2, 'combinatorial', 'vec', False)[0])
    assert not np.array_equal(u3, u2)
    model.order, model.tau = 1, np.zeros(N)
    assert np.array_equal(model.fit(ti, lab), first) and model.num_iter == it1


@pytest.mark.parametrize('norm,ms', [('combinatorial', False), ('normalized', True)])
def test_vector_tau_at_order_one(gl, gold, graphs, monkeypatch, norm, ms):
    """tau as a vector on canonical rows: the fast route (cg_groups_rows), against the oracle and the reference's recorded u."""
    W = graphs[N]
    ti, lab = lo.training_set(gold, N)
    calls = _count_calls(monkeypatch)
    model = model_for(gl, gold, W, N, 1, norm, 'vec', ms, reduce='exact')
    u = model.fit(ti, lab)
    assert calls == [('cg_groups_rows', 'exact', 1)]
    u_o, it_o = orc.laplace_fit(W, ti, lab, normalization=norm, tau=gold['tau%d' % N], mean_shift=ms, tol=lo.TOL, return_iters=True)
    key = lo.case_key(N, 1, norm, 'vec', ms)
    assert model.num_iter == it_o == int(gold['iters_' + key])
    assert np.array_equal(u, u_o) and np.array_equal(u, gold['u_' + key])


def test_randomwalk_alpha(gl, gold, graphs):
    """ssl.randomwalk away from its default alpha, and alpha changed after a fit: the operator is rebuilt."""
    W = graphs[N]
    ti, lab = lo.training_set(gold, N)
    ref = {}
    for a in lo.ALPHAS:
        u_o, it_o = orc.randomwalk_fit(W, ti, lab, alpha=a, return_iters=True)
        assert it_o == int(gold['rw_alpha%s_iters' % a]) and np.array_equal(u_o, gold['rw_alpha%s_u' % a])
        model = gl.ssl.randomwalk(W, alpha=a, reduce='exact')
        u = model.fit(ti, lab)
        assert model.num_iter == it_o and np.array_equal(u, u_o), a
        ref[a] = (np.array(u, copy=True), it_o)
    assert ref[0.5][1] != ref[0.99][1]
    model = gl.ssl.randomwalk(W, alpha=0.5, reduce='exact')
    assert np.array_equal(model.fit(ti, lab), ref[0.5][0])
    dev = model._cache[2]
    model.alpha = 0.99
    assert np.array_equal(model.fit(ti, lab), ref[0.99][0]) and model.num_iter == ref[0.99][1]
    assert model._cache[2] is not dev
    dev = model._cache[2]
    assert np.array_equal(model.fit(ti, lab), ref[0.99][0]) and model._cache[2] is dev
