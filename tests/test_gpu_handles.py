"""GPU: the seven device objects that had no closed-object test (DeviceGraph, Sweep, SweepGroups, Comm, DistSweep, KnnResult,
BallResult).  Of two objects of a class one is closed twice: every public method of it that reaches the library is refused with
GlxError('<Class>: the object is closed') before the library is entered, and the other object still returns what it returned before."""
import numpy as np
import pytest
from scipy import sparse
from conftest import csr_from

pytestmark = pytest.mark.gpu

N, C = 8, 2


def refused(calls):
    from graphlearning_amd import _hip
    for name, fn in calls.items():
        with pytest.raises(_hip.GlxError, match='closed'):
            fn()
            pytest.fail('%s went through on a closed object' % name)


def same(a, b):
    if isinstance(a, dict):
        return a == b
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if sparse.issparse(a):
        return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ('indptr', 'indices', 'data'))
    return np.array_equal(a, b)


def kept(v):
    """a copy of a result: page-locked result arrays are recycled"""
    if isinstance(v, (tuple, list)):
        return tuple(kept(x) for x in v)
    return v.copy() if isinstance(v, np.ndarray) or sparse.issparse(v) else v


def pair(make, result, closed_calls):
    """Two objects from make(): `result(obj)` of the second before and after the first is closed twice and refuses closed_calls(first)."""
    first, second = make(), make()
    before = kept(result(second))
    assert same(kept(result(first)), before)
    first.close()
    first.close()
    assert not first._h.value
    refused(closed_calls(first))
    assert same(kept(result(second)), before)
    return first, second


def test_closed_objects_are_refused_and_their_siblings_untouched(golden):
    from graphlearning_amd import _hip, dist as gdist
    _hip.require_device()
    rng = np.random.default_rng(5)
    A = sparse.diags([np.full(N - 1, 0.25), np.full(N, 0.5), np.full(N - 1, 0.25)], [-1, 0, 1], format='csr')
    u = rng.random((N, C))
    Db = rng.random((N, C)) - 0.5
    deg, vinf, w0 = np.ones(N), np.full(N, 1.0 / N), rng.random(N) / N
    rows, Db_rows, w0_rows = np.array([1, 6]), rng.random((2, C)) - 0.5, np.full(2, 0.5)
    labels = rng.integers(0, C, N)

    # DeviceGraph
    closed_graph, graph = pair(
        lambda: _hip.DeviceGraph(A, keep_order=True),
        lambda g: (g.spmm_bias(u, Db, 2), g.info(), g.order()),
        lambda g: {
            'set_row_transform': lambda: g.set_row_transform(np.ones(N)), 'info': g.info, 'order': g.order,
            'spmm_bias': lambda: g.spmm_bias(u, Db), 'poisson_sweep': lambda: g.poisson_sweep(Db, w0, deg, vinf, 2, 4),
            'cg': lambda: g.cg(Db), 'affine_iterate': lambda: g.affine_iterate(u, Db, max_iter=2),
            'cg_groups': lambda: g.cg_groups(Db, 1), 'cg_groups masked': lambda: g.cg_groups(Db, 1, masks=[[0], [1]]),
            'cg_groups_rows': lambda: g.cg_groups_rows(rows, Db_rows, 1, [[0], [2]]), 'last_block_stats': g.last_block_stats,
            'last_block_forms': g.last_block_forms, 'last_stop_margin': g.last_stop_margin})
    for build in (lambda: _hip.Sweep(closed_graph, C), lambda: _hip.SweepGroups(closed_graph, C, 2)):
        with pytest.raises(_hip.GlxError, match='DeviceGraph: the object is closed'):
            build()
    with _hip.DeviceGraph(A) as g:
        assert g.info()['n_rows'] == N
    assert not g._h.value
    refused({'info after with': g.info})

    # Sweep
    def make_sweep():
        sw = _hip.Sweep(graph, C, 3, 6)
        sw.set_problem(Db, w0, deg, vinf)
        return sw

    def run_sweep(sw):
        T, _ = sw.run()
        return T, sw.fetch(), sw.stop_values()[1]
    pair(make_sweep, run_sweep, lambda sw: {
        'set_problem': lambda: sw.set_problem(Db, w0, deg, vinf), 'set_vectors': lambda: sw.set_vectors(deg, vinf),
        'set_problem_rows': lambda: sw.set_problem_rows(rows, Db_rows, w0_rows, 0.0), 'run': sw.run, 'stop_values': sw.stop_values,
        'set_state': lambda: sw.set_state(u, Db), 'set_state_labels': lambda: sw.set_state_labels(labels, rows, Db_rows),
        'iterate': lambda: sw.iterate(1), 'fetch': sw.fetch, 'project': sw.project, 'launches': sw.launches})

    # SweepGroups
    def make_groups():
        gr = _hip.SweepGroups(graph, C, 2, min_iter=3, max_iter=6)
        gr.set_vectors(deg, vinf)
        for b in range(2):
            gr.set_problem_rows(b, rows[b:], Db_rows[b:], w0_rows[b:], 0.0)
        return gr

    def run_groups(gr):
        T, _ = gr.run()
        return T, gr.fetch(0), gr.view(1).fetch(), gr.stop_values(1)[1]
    pair(make_groups, run_groups, lambda gr: {
        'set_vectors': lambda: gr.set_vectors(deg, vinf), 'set_problem_rows': lambda: gr.set_problem_rows(0, rows, Db_rows, w0_rows, 0.0),
        'run': gr.run, 'stop_values': lambda: gr.stop_values(0), 'fetch': lambda: gr.fetch(0), 'project': lambda: gr.project(0),
        'launches': gr.launches, 'view.fetch': gr.view(1).fetch, 'view.project': gr.view(1).project})
    graph.close()

    # Comm
    closed_comm, comm = pair(lambda: _hip.Comm(nranks=1), lambda c: c.info(), lambda c: {'info': c.info, 'has_transport': c.has_transport})

    # DistSweep: one rank's share of the smallest operator of tests/test_gpu_dist.py
    gold = golden('g1_twomoons.npz')
    W = csr_from(gold, 'W_gaussian')
    ti, lab = gold['train_ind'], gold['labels']
    prob = gdist.poisson_problem(W, ti, lab[ti])
    plan = gdist.RankPlan(prob['P'], gdist.locality_order(prob['P']), gdist.block_bounds(W.shape[0], 1), 0)
    own = plan.own
    problem = (prob['Db'][own], prob['w0'][own], prob['deg'][own], prob['vinf'][own])

    def make_dist():
        ds = gdist.glx_dist_sweep(comm, plan, prob['k'])
        ds.set_problem(*problem)
        return ds

    def run_dist(ds):
        T, _ = ds.run(5, 10, 3, 0.0)
        return T, ds.fetch()
    _, ds = pair(make_dist, run_dist, lambda ds: {
        'set_problem': lambda: ds.set_problem(*problem), 'run': lambda: ds.run(5, 10, 3, 0.0), 'fetch': ds.fetch, 'stats': ds.stats,
        'info': ds.info, 'time_parts': lambda: ds.time_parts(1), 'begin': ds.begin, 'boundary': lambda: ds.boundary(False),
        'get_send': ds.get_send, 'put_halo': lambda: ds.put_halo(np.zeros((ds.n_halo, ds.lay['ld'])), False),
        'interior': lambda: ds.interior(False)})
    with pytest.raises(_hip.GlxError, match='Comm: the object is closed'):
        gdist.glx_dist_sweep(closed_comm, plan, prob['k'])
    ds.close()
    comm.close()

    # KnnResult
    X3 = rng.random((64, 3))
    pair(lambda: _hip.KnnResult(X3, 4), lambda r: (r.lists(), r.to_csr(4)),
         lambda r: {'lists': r.lists, 'order': r.order, 'to_csr': lambda: r.to_csr(4)})[1].close()

    # BallResult
    X2 = rng.random((64, 2))
    pair(lambda: _hip.BallResult(X2, 0.5), lambda r: (r.to_csr(), r.structure()[:3]),
         lambda r: {'to_csr': r.to_csr, 'structure': r.structure})[1].close()
