"""_hip.lp_iterate_batch, graph._plaplace_batch and ssl.plaplace on the device: every column of the batched Jacobi iteration against
its own _hip.lp_iterate call and against the oracle's restatement on this host (uu, ul and the stopping iteration, bit for bit), the
single call from a start of the caller's own against the oracle, the golden fits of the compiled reference through the learner, the learner against the existing single-problem paths, ssl_trials, and one
case with the library's buffer pool switched off.

Every test runs under a time limit of its own: a test that exceeds it ends the whole session on the spot (traceback of every
thread, then exit), so nothing more is started on a device that may have hung; nothing is retried."""
import faulthandler
import os
import sys

import numpy as np
import pytest
from scipy import sparse

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plaplace_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 10, 67)           # 3, 10, 67 divide neither 64 nor 256; 67 is above the columns a workgroup folds in LDS
CAPS = (0, 1, 11, 12, 57, 200, 10 ** 6)


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
    return ref.load_golden()


def _columns(rng, m, how):
    """67 columns (a narrower call takes the first B): distinct, of very different size so that they stop at different iterations."""
    if how == 'constant':
        return np.tile(np.arange(67) + 0.5, (m, 1))
    base = rng.normal(size=(m, 1)) * (1 + np.arange(67) / 64.0)[None, :] + rng.normal(size=(m, 67)) * 0.05
    return base * (10.0 ** -(np.arange(67) % 6))[None, :]


def _problems():
    """name -> (n, I, J, V, ind, vals (m, 67), p, tol, T)."""
    out = {}
    rng = np.random.default_rng(77)
    g = np.load(os.path.join(ref.HERE, 'golden', 'g12_lp_random.npz'))
    for c in range(3):                   # the three random operators of g12_lp_random (n = 300 / 800 / 150), with their own p, tol, T
        n = len(g['c%d_W_indptr' % c]) - 1
        W = sparse.csr_matrix((g['c%d_W_data' % c], g['c%d_W_indices' % c], g['c%d_W_indptr' % c]), shape=(n, n))
        p, tol, T = g['c%d_params' % c]
        vals = _columns(rng, len(g['c%d_bdy' % c]), 'scaled')
        vals[:, 0] = g['c%d_val' % c]
        out['g12_c%d' % c] = (n,) + ref.entries(W) + (g['c%d_bdy' % c], vals, float(p), float(tol), int(T))
    W, ind, _ = ref.scaled_problem(7)
    out['scaled'] = (W.shape[0],) + ref.entries(W) + (ind, _columns(rng, len(ind), 'scaled'), 4.0, 1e-3, 10 ** 6)
    W, ind, _ = ref.constant_problem(3)
    out['constant'] = (W.shape[0],) + ref.entries(W) + (ind, _columns(rng, len(ind), 'constant'), 10.0, 1e-1, 10 ** 6)
    # one vertex: on the boundary, and off it (no boundary vertex at all: the start values are the fold's identity)
    one = sparse.csr_matrix(np.array([[2.0]]))
    out['n1_on'] = (1,) + ref.entries(one) + (np.array([0]), _columns(rng, 1, 'scaled'), 3.0, 1e-2, 40)
    out['n1_off'] = (1,) + ref.entries(one) + (np.zeros(0, dtype=np.int64), np.zeros((0, 67)), 3.0, 1e-2, 40)
    for n in (255, 257):                 # one vertex short of a workgroup of single-column threads, and one over
        W = ref.random_graph(n, n)
        ind = np.sort(rng.choice(n, size=17, replace=False))
        out['n%d' % n] = (n,) + ref.entries(W) + (ind, _columns(rng, 17, 'scaled'), 6.0, 1e-2, 10 ** 6)
    n, hub = 700, 123                    # a star: one row of 699 entries
    leaves = np.delete(np.arange(n), hub)
    S = sparse.csr_matrix((0.5 + rng.random(n - 1), (np.full(n - 1, hub), leaves)), shape=(n, n))
    S = (S + S.T).tocsr()
    ind = np.array([0, 5, 399, 698])
    out['star'] = (n,) + ref.entries(S) + (ind, _columns(rng, 4, 'scaled'), 10.0, 1e-2, 300)
    # one off-boundary vertex without entries: invdeg = alpha / 0, NaN there
    E = ref.random_graph(120, 9).tolil()
    E[40, :] = 0
    E[:, 40] = 0
    E = sparse.csr_matrix(E)
    E.eliminate_zeros()
    ind = np.sort(rng.choice(np.delete(np.arange(120), 40), size=10, replace=False))
    out['empty_row'] = (120,) + ref.entries(E) + (ind, _columns(rng, 10, 'scaled'), 5.0, 1e-2, 90)
    # a boundary vertex listed twice takes its last value
    W = ref.random_graph(200, 13)
    ind = np.array([3, 50, 3, 120, 199, 50])
    out['duplicate'] = (200,) + ref.entries(W) + (ind, _columns(rng, 6, 'scaled'), 8.0, 1e-2, 10 ** 6)
    return out


PROBLEMS = sorted(['g12_c0', 'g12_c1', 'g12_c2', 'scaled', 'constant', 'n1_on', 'n1_off', 'n255', 'n257', 'star', 'empty_row', 'duplicate'])


@pytest.fixture(scope='module')
def problems():
    return _problems()


@pytest.fixture(scope='module')
def references():
    """(problem, T, column) -> (uu, ul, it) of the single device call and of the oracle, computed once and shared by the widths."""
    return {'single': {}, 'oracle': {}}


def single_column(gl, cache, name, prob, T, b):
    from graphlearning_amd import _hip
    key = (name, T, b)
    if key not in cache:
        n, I, J, V, ind, vals, p, tol, _ = prob
        val = np.ascontiguousarray(vals[:, b])
        uu, ul = ref.start_values(n, ind, val)
        it = _hip.lp_iterate(uu, ul, J, I, V, np.ascontiguousarray(ind, dtype=np.int32), val, p, T, tol)
        cache[key] = (uu, ul, it)
    return cache[key]


def oracle_column(cache, name, prob, T, b):
    key = (name, T, b)
    if key not in cache:
        n, I, J, V, ind, vals, p, tol, _ = prob
        cache[key] = ref.oracle_column(n, I, J, V, ind, np.ascontiguousarray(vals[:, b]), p, T, tol)
    return cache[key]


def run_batch(name, prob, B, T):
    from graphlearning_amd import _hip
    n, I, J, V, ind, vals, p, tol, _ = prob
    uu, ul, its = _hip.lp_iterate_batch(n, J, I, V, np.ascontiguousarray(ind, dtype=np.int32), np.ascontiguousarray(vals[:, :B]), p, T, tol)
    assert uu.shape == (n, B) and ul.shape == (n, B) and its.shape == (B,) and its.dtype == np.int64 and uu.dtype == np.float64
    return uu, ul, its


def check_columns(name, B, T, got, want_of):
    uu, ul, its = got
    for b in range(B):
        wu, wl, wit = want_of(b)
        assert its[b] == wit, (name, B, T, b, int(its[b]), wit)
        assert ref.same(uu[:, b], wu) and ref.same(ul[:, b], wl), (name, B, T, b)
    return its


@pytest.mark.parametrize('B', WIDTHS)
@pytest.mark.parametrize('name', PROBLEMS)
def test_batch_equals_single_calls_and_oracle(gl, problems, references, name, B):
    prob = problems[name]
    T = prob[8]
    got = run_batch(name, prob, B, T)
    its = check_columns(name, B, T, got, lambda b: single_column(gl, references['single'], name, prob, T, b))
    check_columns(name, B, T, got, lambda b: oracle_column(references['oracle'], name, prob, T, b))
    print(name, B, 'stops', sorted(set(its.tolist()))[:12])
    if name == 'empty_row':
        assert np.isnan(got[0][40]).all() and np.isnan(got[1][40]).all()
    if name == 'constant':
        assert its.tolist() == [11] * B
    if name in ('scaled', 'duplicate', 'n257') and B >= 10:      # different stops in one call, of both parities
        assert len(set(its.tolist())) >= 4 and set((its % 2).tolist()) == {0, 1}, its


@pytest.mark.parametrize('B', WIDTHS)
@pytest.mark.parametrize('name', ['scaled', 'constant'])
def test_caps(gl, problems, references, name, B):
    """T on both sides of the first possible stop, odd and even, and a run to the stop."""
    prob = problems[name]
    for T in CAPS:
        got = run_batch(name, prob, B, T)
        check_columns(name, B, T, got, lambda b: single_column(gl, references['single'], name, prob, T, b))
        check_columns(name, B, T, got, lambda b: oracle_column(references['oracle'], name, prob, T, b))
        if T == 0:
            n, I, J, V, ind, vals, p, tol, _ = prob
            for b in range(B):
                wu, wl = ref.start_values(n, ind, vals[:, b])
                assert ref.same(got[0][:, b], wu) and ref.same(got[1][:, b], wl)


def test_single_call_from_a_given_start(gl):
    """_hip.lp_iterate from a start the batched path never forms (off the boundary uu raised and ul lowered, vertex by vertex)
    against the oracle called with the same arrays: uu and ul bit for bit, the stopping iteration exactly.  The caps lie on both
    sides of the first possible stop (iteration 11) and return either buffer (even / odd); the run to the stop ends beyond the
    first chunk of 64 iterations, at another iteration than from the start of graph.plaplace (with this seed 66 against 61 and 63)."""
    from graphlearning_amd import _hip
    rng = np.random.default_rng(5)
    p, tol = 6.0, 1e-2
    for n in (255, 257):
        I, J, V = ref.entries(ref.random_graph(n, n))
        ind = np.sort(rng.choice(n, size=17, replace=False))
        val = rng.normal(size=17)
        uu0, ul0 = ref.start_values(n, ind, val)
        off = np.ones(n, dtype=bool)
        off[ind] = False
        uu0[off] += rng.random(n - 17)
        ul0[off] -= rng.random(n - 17)
        ind32 = np.ascontiguousarray(ind, dtype=np.int32)
        for T in (0, 11, 12, 13, 40, 41, 10 ** 6):
            wu, wl, wit = ref.oracle_from(uu0, ul0, n, I, J, V, ind, val, p, T, tol)
            uu, ul = uu0.copy(), ul0.copy()
            it = _hip.lp_iterate(uu, ul, J, I, V, ind32, val, p, T, tol)
            print(n, T, 'stop', it, 'want', wit)
            assert it == wit, (n, T, it, wit)
            assert ref.same(uu, wu) and ref.same(ul, wl), (n, T)
            assert np.isfinite(wu).all() and np.isfinite(wl).all()
        default = ref.oracle_column(n, I, J, V, ind, val, p, 10 ** 6, tol)[2]
        print(n, 'stop from the default start', default)
        assert wit > 64 and wit != default, (n, wit, default)


def test_refused_widths_and_caps(gl, problems):
    from graphlearning_amd import _hip
    n, I, J, V, ind, vals, p, tol, _ = problems['scaled']
    ind32 = np.ascontiguousarray(ind, dtype=np.int32)
    with pytest.raises(_hip.GlxError, match='columns above'):
        _hip.lp_iterate_batch(n, J, I, V, ind32, np.zeros((len(ind), 257)), p, 5, tol)
    with pytest.raises(_hip.GlxError, match='2\\^24'):
        _hip.lp_iterate_batch(n, J, I, V, ind32, vals[:, :2], p, (1 << 24) + 1, tol)
    with pytest.raises(_hip.GlxError, match='out of range'):
        _hip.lp_iterate_batch(n, J, I, V, np.array([0, n], dtype=np.int32), vals[:2, :2], p, 5, tol)
    uu, ul, its = _hip.lp_iterate_batch(n, J, I, V, ind32, np.tile(vals[:, :64], (1, 4)), p, 30, tol)        # 256 columns: the cap itself
    assert uu.shape == (n, 256) and ref.same(uu[:, :64], uu[:, 192:]) and np.array_equal(its[:64], its[192:]) and its.min() >= 11


def case_inputs(gold, name):
    gname, fast, p, tol, T = ref.GOLDEN_CASES[name]
    ti = gold['graph_%s_train_ind' % gname]
    lab = gold['graph_%s_labels' % gname]
    return gname, fast, p, tol, T, ti, lab


@pytest.mark.parametrize('name', sorted(n for n, c in ref.GOLDEN_CASES.items() if c[1]))
def test_golden_fits_fast(gl, gold, name):
    gname, fast, p, tol, T, ti, lab = case_inputs(gold, name)
    W = ref.golden_graph(gold, gname)
    model = gl.ssl.plaplace(W, p=p, max_num_it=T, tol=tol, fast=True)
    model.graph.__ccode_init__()
    I, J, V = ref.golden_entries(gold, gname)
    assert np.array_equal(model.graph.I, I) and np.array_equal(model.graph.J, J), 'this host orders the entries of a vertex differently'
    pred = model.fit_predict(ti, lab[ti])
    print(name, 'sweeps', model.num_iter, 'want', gold[name + '_iters'].tolist(), 'levels', model.graph.plaplace_levels)
    assert model.num_iter == gold[name + '_iters'].tolist()
    assert np.asarray(model.prob, dtype=np.float64).tobytes() == gold[name + '_prob'].tobytes()
    assert np.array_equal(pred, gold[name + '_pred'])
    assert model.graph.plaplace_levels >= 1 and model.graph.plaplace_plan[0] == model.graph.plaplace_levels


@pytest.mark.parametrize('name', sorted(n for n, c in ref.GOLDEN_CASES.items() if not c[1]))
def test_golden_fits_jacobi(gl, gold, name):
    """prob equals the oracle on this host's entry order bit for bit; it is within 1e-12 of the golden and num_iter within one of it
    (both exact when this host's entry order is the stored one: the rule of test_gpu_parity.py::test_plaplace_jacobi_golden)."""
    gname, fast, p, tol, T, ti, lab = case_inputs(gold, name)
    W = ref.golden_graph(gold, gname)
    model = gl.ssl.plaplace(W, p=p, max_num_it=T, tol=tol, fast=False)
    pred = model.fit_predict(ti, lab[ti])
    prob = np.asarray(model.prob, dtype=np.float64)
    I, J, V = model.graph._entries()
    ouu, oul, oit = ref.oracle_batch(W.shape[0], I, J, V, ti, ref.class_columns(lab[ti]), p, int(T), tol)
    want_it = gold[name + '_iters']
    print(name, 'iterations', model.num_iter, 'want', want_it.tolist(), 'max difference', float(np.max(np.abs(prob - gold[name + '_prob']))))
    assert model.num_iter == oit.tolist()
    assert prob.tobytes() == ((ouu + oul) / 2).tobytes()
    assert np.max(np.abs(prob - gold[name + '_prob'])) <= 1e-12
    assert np.max(np.abs(np.array(model.num_iter) - want_it)) <= 1
    if np.array_equal(J, ref.golden_entries(gold, gname)[1]):
        assert prob.tobytes() == gold[name + '_prob'].tobytes() and model.num_iter == want_it.tolist()
        assert np.array_equal(pred, gold[name + '_pred'])


def test_learner_equals_the_existing_paths(gl, gold):
    from graphlearning_amd import _hip
    gname, fast, p, tol, T, ti, lab = case_inputs(gold, 'b3_jac_p10')
    W = ref.golden_graph(gold, gname)
    tl = lab[ti]
    model = gl.ssl.plaplace(W, p=p, tol=tol, fast=False)
    prob = np.array(model.fit(ti, tl))
    G = gl.graph(W)
    for c, l in enumerate(np.unique(tl)):
        u = G.plaplace(ti, tl == l, p, tol=tol, fast=False)
        assert prob[:, c].tobytes() == u.tobytes() and model.num_iter[c] == G.plaplace_iters, c
    # one class through _fit: the same column
    assert np.asarray(model._fit(ti, tl == 1), dtype=np.float64).tobytes() == np.ascontiguousarray(prob[:, 1]).tobytes()
    model = gl.ssl.plaplace(W, p=p, fast=True)
    prob = np.array(model.fit(ti, tl))
    I, J, V = G._entries()
    for c, l in enumerate(np.unique(tl)):
        val = np.ascontiguousarray((tl == l).astype(np.float64)[:, None])
        u, its, plan, _ = _hip.lip_iterate(W.shape[0], J, I, V, ti.astype(np.int32), val, False, 1 / (p - 1), 1 - 1 / (p - 1), int(1e6), 1e-6)
        assert prob[:, c].tobytes() == u[:, 0].tobytes() and model.num_iter[c] == its[0], c
    assert np.asarray(model._fit(ti, tl == 2), dtype=np.float64).tobytes() == np.ascontiguousarray(prob[:, 2]).tobytes()


def test_trials_and_class_priors(gl, gold, tmp_path, monkeypatch):
    gname, fast, p, tol, T, ti, lab = case_inputs(gold, 'b3_jac_p10')
    W = ref.golden_graph(gold, gname)
    rng = np.random.default_rng(8)
    other = np.sort(np.concatenate([rng.choice(np.where(lab == c)[0], size=3, replace=False) for c in range(3)]))
    sets = [ti, other]
    monkeypatch.setattr(gl.ssl, 'results_dir', str(tmp_path / 'results'))
    for fast, T in ((True, 1e6), (False, 200)):
        tag = 'f%d_' % fast
        model = gl.ssl.plaplace(W, p=p, max_num_it=T, tol=tol, fast=fast)
        model.ssl_trials(sets, lab, tag=tag)
        lines = open(tmp_path / 'results' / (tag + '_plaplace_p10.00_accuracy.csv')).read().strip().split('\n')
        assert lines[0] == 'Number of labels,Accuracy' and len(lines) == 3
        for ts, line in zip(sets, lines[1:]):
            m2 = gl.ssl.plaplace(W, p=p, max_num_it=T, tol=tol, fast=fast)
            acc = gl.ssl.ssl_accuracy(m2.fit_predict(ts, lab[ts]), lab, ts)
            assert line == '%d' % len(ts) + ',%.2f' % acc
        num_train, mean, std, nt = model.trials_statistics(tag=tag)
        assert list(num_train) == [9.0, 12.0] and nt == 1 and mean.shape == (2, 1)
    # class priors: the golden fit's labels
    model = gl.ssl.plaplace(W, class_priors=gold['graph_%s_priors' % gname], p=p, tol=tol, fast=False)
    pred = model.fit_predict(ti, lab[ti])
    if np.array_equal(model.graph._entries()[1], ref.golden_entries(gold, gname)[1]):
        assert np.asarray(model.prob, dtype=np.float64).tobytes() == gold['b3_jac_p10_prob'].tobytes()
    assert np.array_equal(pred, gold['b3_jac_p10_priors_pred'])
    assert not np.array_equal(pred, gold['b3_jac_p10_pred'])          # the priors did move labels
    model.ssl_trials(sets[:1], lab, tag='p_')
    hdr = open(tmp_path / 'results' / 'p__plaplace_p10.00_classpriors_accuracy.csv').readline().strip()
    assert hdr == 'Number of labels,Accuracy,Accuracy with class priors,Class priors error'


def test_identical_with_the_pool_switched_off(gl, problems, references):
    from graphlearning_amd import _hip
    prob = problems['scaled']
    _hip.pool_set_enabled(False)
    try:
        got = run_batch('scaled', prob, 10, prob[8])
    finally:
        _hip.pool_set_enabled('nopool' not in os.environ.get('GLX_TEST_ABLATE', ''))
    check_columns('scaled', 10, prob[8], got, lambda b: oracle_column(references['oracle'], 'scaled', prob, prob[8], b))
