"""graph.amle / ssl.amle without a GPU: the restatement tests/amle_ref.py against the golden vectors of the compiled reference
(tests/golden/make_golden_amle.py), the level plan of csrc/lip_plan.h built on the host (tests/lip_plan_host.cpp), and the surface:
the entry point is declared and exported, the refusals are ValueErrors raised before any device call.

The Python forms of the restatement (`sequential`: interpreted, vertex after vertex; `levelled`: numpy, level after level) run on
every golden case they finish within a second or two (amle_ref.python_forms_fit; the longest cases are hundreds of sweeps of 30
bisection passes over 28 000 entries); EVERY golden case is reproduced by the compiled host restatement of tests/lip_plan_host.cpp in
both forms, and the Python forms are held against that one on random graphs."""
import os
import re
import sys
import numpy as np
import pytest
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import amle_ref as ref              # noqa: E402
import graphlearning_amd as gl      # noqa: E402
from graphlearning_amd import _hip  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'g15_amle.npz')


def load_golden():
    g = dict(np.load(GOLDEN, allow_pickle=False))
    for fn in sorted(set(g['entry_files'].tolist())):
        if fn != 'g15_amle.npz':
            g.update(dict(np.load(os.path.join(ROOT, 'tests', 'golden', fn), allow_pickle=False)))
    return g


def golden_graph(g, name):
    n = len(g['graph_%s_indptr' % name]) - 1
    return sparse.csr_matrix((g['graph_%s_data' % name], g['graph_%s_indices' % name], g['graph_%s_indptr' % name]), shape=(n, n))


def golden_entries(g, gname):
    """(W, rows, nbr, V) of a golden graph; the neighbour order of the entry list is the one the reference ran on."""
    W = golden_graph(g, gname)
    rows, nbr, V = ref.entries(W)
    assert np.array_equal(nbr, g['graph_%s_J' % gname]), 'np.argsort orders the entries of a vertex differently than when the goldens were made'
    return W, rows, nbr, V


def golden_case(g, name):
    """(gname, ind, vals (m, B), weighted, tol, T, alpha, beta, u (n, B), sweeps (B,), errs (max sweeps, B))."""
    gname, _, weighted, tol, T, alpha, beta = ref.GOLDEN_CASES[name]
    return (gname, g[name + '_ind'].astype(np.int64), g[name + '_vals'], weighted, tol, T, alpha, beta, g[name + '_u'], g[name + '_sweeps'],
            g[name + '_errs'])


@pytest.fixture(scope='module')
def gold():
    return load_golden()


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return ref.build_host_lib(tmp_path_factory.mktemp('lip_plan'))


def test_golden_holds_the_cases_the_feature_names(gold):
    assert set(ref.GOLDEN_CASES) <= set(gold['entry_names'].tolist())
    for gname in ref.GOLDEN_GRAPHS:
        W = golden_graph(gold, gname)
        assert np.diff(W.indptr).min() >= 1 and W.data.min() > 0, gname            # no empty row
    assert (abs(golden_graph(gold, 'blobs_dir') - golden_graph(gold, 'blobs_dir').T) > 0).nnz > 0          # directed
    assert (golden_graph(gold, 'diag').diagonal() != 0).sum() == 300
    deg = np.diff(golden_graph(gold, 'ball').indptr)
    assert deg.max() >= 4 * deg.min()                                                  # uneven degrees
    for name in ('blobs_u_3', 'blobs_u_5', 'blobs_w_3', 'blobs_w_5', 'blobsdir_u', 'blobsdir_w'):
        assert len(set(gold[name + '_sweeps'].tolist())) > 1, name                     # the classes stop at different sweeps
    assert gold['stop_T0_sweeps'].tolist() == [0] and gold['stop_T5_u_sweeps'].tolist() == [5] and gold['stop_T5_w_sweeps'].tolist() == [5]
    assert gold['stop_tol10_u_sweeps'].tolist() == [22] and gold['stop_tol10_w_sweeps'].tolist() == [22]
    assert int(gold['blobs_u_3_levels']) == 24 and int(gold['path_u_levels']) == 1498
    assert int(gold['sorted_u_levels']) == 171 and int(gold['sorted_w_levels']) == 172          # (the boundary sets of the two cases differ)
    # the inputs are what the names say
    lab, ti = gold['graph_blobs_labels'], gold['fit_train_ind']
    for name in ref.GOLDEN_CASES:
        gname, ind, vals = golden_case(gold, name)[:3]
        ind2, vals2 = ref.case_boundary(name, golden_graph(gold, gname), lab, ti)
        assert np.array_equal(ind, ind2) and vals.tobytes() == vals2.tobytes(), name


@pytest.mark.parametrize('name', sorted(ref.GOLDEN_CASES))
def test_restatement_equals_golden(gold, lib, name):
    """u, sweeps done and error history, bit for bit, column by column: the host restatement in index order and level by level on every
    case; the Python forms where they fit."""
    gname, ind, vals, weighted, tol, T, alpha, beta, U, sweeps, errs = golden_case(gold, name)
    W, rows, nbr, V = golden_entries(gold, gname)
    n = W.shape[0]
    mask, _ = ref.boundary(n, ind, vals[:, 0])
    nlevels = int(ref.levels(n, rows, nbr, mask).max()) + 1
    assert nlevels == int(gold[name + '_levels'])
    ran = set()
    for b in range(vals.shape[1]):
        val = np.ascontiguousarray(vals[:, b])
        want_u, want_errs = np.ascontiguousarray(U[:, b]), errs[:sweeps[b], b].tolist()
        for levelled in (False, True):
            u, done, e = ref.host_sweeps(lib, n, rows, nbr, V, ind, val, weighted, alpha, beta, T, tol, levelled)
            assert u.tobytes() == want_u.tobytes() and done == sweeps[b] and e == want_errs, (b, levelled)
        forms = ref.python_forms_fit(int(sweeps[b]), len(nbr), nlevels, weighted)
        for form, fn in (('sequential', ref.sequential), ('levelled', ref.levelled)):
            if form in forms:
                u, done, e = fn(n, rows, nbr, V, ind, val, weighted, alpha, beta, T, tol)
                assert u.tobytes() == want_u.tobytes() and done == sweeps[b] and e == want_errs, (b, form)
                ran.add(form)
    print(name, 'python forms run:', sorted(ran))


def test_python_forms_cover_both_solvers_on_the_goldens(gold):
    """The budget of amle_ref.python_forms_fit leaves each Python form at least one weighted and one unweighted golden case."""
    seen = set()
    for name in ref.GOLDEN_CASES:
        gname, ind, vals, weighted, tol, T, alpha, beta, U, sweeps, errs = golden_case(gold, name)
        if sweeps.max() == 0:
            continue
        for form in ref.python_forms_fit(int(sweeps.max()), len(gold['graph_%s_J' % gname]), int(gold[name + '_levels']), weighted):
            seen.add((form, bool(weighted), alpha != 0))
    assert {('sequential', False, False), ('sequential', True, False), ('levelled', False, False), ('levelled', True, False)} <= seen, seen


def random_graph(rng, n, deg, sym, diag):
    A = sparse.random(n, n, density=min(1.0, deg / n), random_state=int(rng.integers(1 << 30)), format='csr')
    A.setdiag(0)
    A.eliminate_zeros()
    A = A + sparse.diags(np.ones(n - 1) * 0.5, 1, format='csr')            # no empty row: i -> i + 1 ...
    A = (A + sparse.csr_matrix(([0.25], ([n - 1], [0])), shape=(n, n))).tocsr()      # ... and n - 1 -> 0
    if sym:
        A = A.maximum(A.T).tocsr()
    if diag:
        d = np.zeros(n)
        d[::2] = 0.1 + rng.random(len(d[::2]))
        A = (A + sparse.diags(d, 0)).tocsr()
    return A


def random_problem(rng, trial):
    n = int(rng.integers(40, 301))
    W = random_graph(rng, n, float(rng.integers(2, 9)), sym=bool(trial % 2), diag=bool(trial % 3 == 0))
    m = int(rng.integers(1, 9))
    ind = rng.choice(n, size=m, replace=False).astype(np.int64)
    val = rng.random(m) * 2 - 0.5
    weighted = bool(trial % 4 < 2)
    T = int(rng.choice([3, 21, 22, 23, 60, 400]))
    tol = float(rng.choice([1e-2, 1e-4, 10.0]))
    alpha = 0.0 if trial % 5 else float(rng.random())
    return n, W, ind, val, weighted, T, tol, alpha, 1.0 - alpha


def test_forms_agree_on_random_graphs(lib):
    """sequential (Python) == levelled (numpy) == host restatement in both forms, on symmetric and directed graphs with and without
    diagonal entries, both solvers, T on both sides of 22, alpha != 0."""
    rng = np.random.default_rng(15)
    for trial in range(6):
        n, W, ind, val, weighted, T, tol, alpha, beta = random_problem(rng, trial)
        T = min(T, 25)                      # (the interpreted form: 300 vertices x 30 passes a sweep)
        rows, nbr, V = ref.entries(W)
        a = ref.sequential(n, rows, nbr, V, ind, val, weighted, alpha, beta, T, tol)
        b = ref.levelled(n, rows, nbr, V, ind, val, weighted, alpha, beta, T, tol)
        c = ref.host_sweeps(lib, n, rows, nbr, V, ind, val, weighted, alpha, beta, T, tol, False)
        d = ref.host_sweeps(lib, n, rows, nbr, V, ind, val, weighted, alpha, beta, T, tol, True)
        for other in (b, c, d):
            assert a[0].tobytes() == other[0].tobytes() and a[1] == other[1] and a[2] == other[2], (trial, n, weighted, T, tol, alpha)


def check_plan(n, rows, nbr, mask, plan, small):
    level, order, lvl_ptr, launches = plan['level'], plan['order'], plan['lvl_ptr'], plan['launches']
    free = np.where(~mask)[0]
    assert (level[mask] == -1).all() and (level[free] >= 0).all()
    assert np.array_equal(np.sort(order), free)                                     # every non-boundary vertex exactly once
    # ordered by (level, index), the level pointers delimit the levels
    assert np.array_equal(order, free[np.lexsort((free, level[free]))])
    assert lvl_ptr[0] == 0 and lvl_ptr[-1] == len(free) and (np.diff(lvl_ptr) > 0).all()
    for l in range(plan['nlevels']):
        assert (level[order[lvl_ptr[l]:lvl_ptr[l + 1]]] == l).all()
    # every stored entry between two different non-boundary vertices: the lower index has the strictly lower level
    both = ~mask[rows] & ~mask[nbr] & (rows != nbr)
    lo, hi = np.minimum(rows[both], nbr[both]), np.maximum(rows[both], nbr[both])
    assert (level[lo] < level[hi]).all()
    # minimal: level 0 has no such lower neighbour, every other vertex has one exactly one level below
    best = np.full(n, -1, dtype=np.int64)
    np.maximum.at(best, hi, level[lo])
    assert np.array_equal(level[free], best[free] + 1)
    assert np.array_equal(level, ref.levels(n, rows, nbr, mask))
    # the launch list covers the levels in order; a merged launch is a run of two or more small levels, every other launch is one level:
    # a large one, or a small one with no small neighbour
    assert launches[0, 0] == 0 and launches[-1, 1] == plan['nlevels'] and np.array_equal(launches[1:, 0], launches[:-1, 1])
    size = np.diff(lvl_ptr)
    for l0, l1, merged in launches.tolist():
        assert l1 > l0
        if merged:
            assert l1 >= l0 + 2 and (size[l0:l1] <= small).all()
        else:
            assert l1 == l0 + 1
    is_small = size <= small
    covered = np.zeros(plan['nlevels'], dtype=bool)
    for l0, l1, merged in launches.tolist():
        if merged:
            covered[l0:l1] = True
    has_small_neighbour = np.concatenate(([False], is_small[:-1])) | np.concatenate((is_small[1:], [False]))
    assert np.array_equal(covered, is_small & has_small_neighbour)                   # maximal runs: each is ONE launch, nothing else is merged


def test_level_plan_on_the_golden_graphs(gold, lib):
    small = ref.host_constants(lib)['small']
    assert 1 <= small <= 1024
    for name in sorted(ref.GOLDEN_CASES):
        gname, ind, vals = golden_case(gold, name)[:3]
        W, rows, nbr, V = golden_entries(gold, gname)
        n = W.shape[0]
        mask, _ = ref.boundary(n, ind, vals[:, 0])
        plan = ref.host_plan(lib, n, rows, nbr, mask)
        check_plan(n, rows, nbr, mask, plan, small)
        assert plan['nlevels'] == int(gold[name + '_levels']), name
        if gname == 'path':
            assert plan['launches'].tolist() == [[0, 1498, 1]], name                      # every level small: one launch per sweep
        if gname == 'sorted':                  # all but the first two levels are small: they ride in one merged launch
            assert len(plan['launches']) <= 3 and plan['launches'][-1, 2] == 1 and plan['launches'][-1, 1] - plan['launches'][-1, 0] >= 165, name
    # nothing merged when asked so
    W, rows, nbr, V = golden_entries(gold, 'path')
    mask, _ = ref.boundary(1500, [0, 1499], [0.0, 1.0])
    plan = ref.host_plan(lib, 1500, rows, nbr, mask, small=0)
    check_plan(1500, rows, nbr, mask, plan, 0)
    assert len(plan['launches']) == 1498


def test_level_plan_on_random_directed_graphs(lib):
    rng = np.random.default_rng(21)
    for trial in range(30):
        n = int(rng.integers(2, 400))
        W = random_graph(rng, n, float(rng.integers(1, 10)), sym=bool(trial % 3 == 0), diag=bool(trial % 2))
        rows, nbr, V = ref.entries(W)
        m = int(rng.integers(0, min(n, 12) + 1)) if trial % 7 else n
        mask = np.zeros(n, dtype=bool)
        mask[rng.choice(n, size=m, replace=False)] = True
        for small in (0, 1, 3, 32, 128):
            plan = ref.host_plan(lib, n, rows, nbr, mask, small=small)
            if m == n:
                assert plan['nlevels'] == 0 and len(plan['order']) == 0 and len(plan['launches']) == 0
            else:
                check_plan(n, rows, nbr, mask, plan, small)
    # a directed pair: 0 reads 1, 1 does not read 0 -- 1 must still wait for 0
    W = sparse.csr_matrix(np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]))
    rows, nbr, V = ref.entries(W)
    plan = ref.host_plan(lib, 3, rows, nbr, np.array([False, False, True]))
    assert plan['level'].tolist() == [0, 1, -1]


def test_symbol_declared_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'glx_experimental.h')).read()
    assert re.search(r'\bint\s+glx_lip_iterate\s*\(', hdr)
    assert 'glx_lip_iterate' not in open(os.path.join(ROOT, 'include', 'glx.h')).read()
    assert 'glx_lip_iterate' in _hip.EXPORTED_SYMBOLS
    assert getattr(_hip.load(), 'glx_lip_iterate') is not None
    assert callable(_hip.lip_iterate)


def _path_graph(n=6):
    return (sparse.diags([1.0] * (n - 1), 1) + sparse.diags([1.0] * (n - 1), -1)).tocsr()


def test_entry_points_exist_and_refuse_without_a_device():
    G = gl.graph(_path_graph())
    assert callable(G.amle) and callable(G._amle_batch)
    model = gl.ssl.amle(_path_graph())
    assert model.name == 'AMLE' and model.onevsrest and model.accuracy_filename == '_amle_unweighted'
    assert model.tol == 1e-3 and model.max_num_it == 1e5 and model.weighted is False and model.prog is False
    assert model.get_accuracy_filename() == '_amle_unweighted_accuracy.csv'
    wm = gl.ssl.amle(_path_graph(), class_priors=np.array([0.5, 0.5]), weighted=True)
    assert wm.get_accuracy_filename() == '_amle_classpriors_accuracy.csv'
    # graph_nearest_neighbor keeps the class-by-class loop
    assert gl.ssl.graph_nearest_neighbor(_path_graph())._fit_onevsrest(np.array([0]), np.array([0]), np.array([0])) is None
    try:
        n_dev = _hip.device_count()
    except _hip.GlxError:
        n_dev = 0
    if n_dev > 0:
        u = G.amle([0, 5], np.array([0.0, 1.0]), weighted=False, tol=1e-12)
        assert np.allclose(u, np.arange(6) / 5, atol=1e-9)
        return
    with pytest.raises(_hip.GlxError):
        G.amle([0, 5], np.array([0.0, 1.0]))
    with pytest.raises(_hip.GlxError):
        model.fit(np.array([0, 5]), np.array([0, 1]))


def test_refusals_are_value_errors(monkeypatch):
    """The stated deviations are refused before any device call: the binding is replaced by one that fails the test when reached."""
    def reached(*a, **k):
        raise AssertionError('the device call was reached')
    monkeypatch.setattr(_hip, 'lip_iterate', reached)
    G = gl.graph(_path_graph())
    good = np.array([0.0, 1.0])
    for bad in (np.array([0.0, np.nan]), np.array([np.inf, 1.0])):
        with pytest.raises(ValueError):
            G.amle([0, 5], bad)
    for tol in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            G.amle([0, 5], good, tol=tol)
    with pytest.raises(ValueError):
        G.amle([0, 6], good)
    with pytest.raises(ValueError):
        G.amle([0, 5], good, max_num_it=1e9)
    with pytest.raises(ValueError):
        G._amle_batch([0, 5], np.zeros((3, 2)))
    for w in (-1.0, np.nan):
        Wn = _path_graph().tolil()
        Wn[1, 2] = w
        with pytest.raises(ValueError):
            gl.graph(Wn.tocsr()).amle([0, 5], good)
    # a vertex off the boundary without a stored entry; on the boundary it is fine
    We = _path_graph().tolil()
    We[3, 2] = 0
    We[3, 4] = 0
    We = We.tocsr()
    We.eliminate_zeros()
    with pytest.raises(ValueError):
        gl.graph(We).amle([0, 5], good)
    with pytest.raises(AssertionError, match='device call was reached'):
        gl.graph(We).amle([0, 3, 5], np.array([0.0, 0.5, 1.0]))
    with pytest.raises(AssertionError, match='device call was reached'):
        G.amle(np.array([True, False, False, False, False, True]), good)             # a mask as boundary set
    # the learner refuses the same way
    with pytest.raises(ValueError):
        gl.ssl.amle(We).fit(np.array([0, 5]), np.array([0, 1]))
    # plaplace(fast=True) stays refused in this form, with a message that no longer calls the sweep unparallelisable
    with pytest.raises(NotImplementedError) as exc:
        G.plaplace(np.array([0, 5]), good, 4)
    assert 'sequential' not in str(exc.value) and 'lip_iterate' in str(exc.value)
