"""The sweep on the operator layout glx_graph_plan (csrc/graph.hip) builds once the vertex records no longer fit the eight L2s
(n_cols * G * 4 * sizeof(T) >= 32 MiB): row classes 64 / 256 at 4 lanes per row -- one-slot rows of up to 16 chunks, four-slot rows
of 65 .. 256 entries --, rows sorted by length inside windows of 32 768 consecutive rows only, the rows split over 4 or 16 slots
pulled out of their windows and placed first, no longest-slice-first reordering.  Everything is np.array_equal.

Fixtures (tests/big_state_cases.py; tests/test_sell_plan_host.py shows, without a device, that they reach what is claimed here):
  A  640 rows x n_cols columns, n_cols on either side of the flip of the classes: the classes alone, no windows.
  B  300 000 rows (600 000 for the fp32 state at 4 lanes per row), a hub of up to 300 entries every 64 rows: two (three) windows and
     some 260 (520) split rows in every XCD range.
References: scipy's A @ u in the state's type, proved equal to the entry-order loop on each fixture (sweep_ref.prove_products);
sweep_ref.poisson_sweeps for the stop-column forms.  That the device built the plan a test is about is read from
DeviceGraph.info() of a fresh operator after its first product -- glx_graph_info reports the first plan built -- against
tests/sell_plan_ref.py, the numpy restatement of the plan's shape, fed the row lengths in the operator's vertex order."""
import faulthandler
import numpy as np
import pytest
import sell_plan_ref as S
import big_state_cases as K
import sweep_ref as R
from test_gpu_sweep_stop import _same, _run, _group

pytestmark = pytest.mark.gpu

LANES = {1: 4, 16: 4, 17: 8, 33: 16}          # width -> lanes per row of the plain record


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope='module')
def hip():
    from graphlearning_amd import _hip
    _hip.require_device()
    return _hip


def _check_info(hip, G, lens, n_cols, C, dt, what):
    """the first plan of G against the restatement on the lengths in G's vertex order -> the restatement's plan"""
    lanes = hip.record_layout(C, K.DT[dt], False)['G']
    assert lanes == LANES[C], (C, lanes)
    perm = G.order()
    assert np.array_equal(np.sort(perm), np.arange(len(lens)))
    p = S.plan(lens[perm], n_cols, lanes, K.ESIZE[dt])
    info = G.info()
    assert info['rows_per_slice'] * lanes == 64 and info['max_row'] == lens.max()
    assert (info['slices'], info['stored']) == (p['nslices'], p['stored']), (what, info, p['nslices'], p['stored'])
    return p, perm


# ---- fixture A: the class flip alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('side', ['below', 'at'])
@pytest.mark.parametrize('C', [1, 16])
@pytest.mark.parametrize('dt', ['f64', 'f32'])
def test_class_flip_on_the_rectangular_ladder(hip, dt, C, side):
    n_cols = K.FLIP[dt] - (1 if side == 'below' else 0)
    A = K.rect(n_cols)
    dtype = K.DT[dt]
    A_dt = R.as_dtype(A, dtype)
    u, Db = K.operands(K.N_A, n_cols, C, dtype)
    G = hip.DeviceGraph(A, dtype=dtype, keep_order=True)
    try:
        got = G.spmm_bias(u, None)
        p, perm = _check_info(hip, G, K.lengths_a(), n_cols, C, dt, (dt, C, side))
        assert np.array_equal(perm, np.arange(K.N_A))
        assert p['big'] == (side == 'at') and (p['L1'], p['L4']) == ((64, 256) if side == 'at' else (24, 96)) and not p['windowed']
        assert (p['nslices'], p['stored']) == ((160, 69056) if side == 'at' else (288, 67136))
        want = A_dt @ u
        assert got.dtype == dtype and got.shape == (K.N_A, C) and np.array_equal(got, want), (dt, C, side, 'plain')
        got = G.spmm_bias(u, Db)
        assert got.dtype == dtype and np.array_equal(got, Db + want), (dt, C, side, 'bias')
    finally:
        G.close()


# ---- fixture B: windows and split rows together -------------------------------------------------------------------------------------
def _products(hip, A, n, C, dt, orders):
    dtype = K.DT[dt]
    A_dt = R.as_dtype(A, dtype)
    lens = np.diff(A.indptr).astype(np.int64)
    u, Db = K.operands(n, n, C, dtype)
    plans = {}
    graphs = {keep: hip.DeviceGraph(A, dtype=dtype, keep_order=keep) for keep in orders}
    try:
        for bias in (None, Db):
            ref = u
            for iters in (1, 2):      # (one reference at a time: at 33 fp64 columns an operand is 79 MB)
                ref = A_dt @ ref if bias is None else bias + A_dt @ ref
                assert ref.dtype == dtype
                for keep, G in graphs.items():
                    got = G.spmm_bias(u, bias, iters=iters)
                    if keep not in plans:
                        p, perm = _check_info(hip, G, lens, n, C, dt, (dt, C, keep))
                        assert np.array_equal(perm, np.arange(n)) == keep and G.info()['renumbered'] == (0 if keep else 1)
                        plans[keep] = p
                    assert got.dtype == dtype and got.shape == (n, C)
                    assert np.array_equal(got, ref), (dt, C, 'keep' if keep else 'own order', bias is not None, iters)
                    del got
    finally:
        for G in graphs.values():
            G.close()
    return plans


@pytest.mark.parametrize('dt,C', [('f64', 1), ('f64', 16), ('f64', 17), ('f64', 33), ('f32', 17), ('f32', 33)])
def test_windows_and_split_rows(hip, dt, C):
    """One and two applications, with and without Db, in the caller's order and in the library's own."""
    plans = _products(hip, K.square(), K.N_B, C, dt, (True, False))
    # the caller's order: every range has two windows and, at 4 lanes per row, split rows in front of them.  The library's own order
    # moves the hubs together: some ranges keep both, others end up below 32 768 rows -- one window, under the plan's `windowed` flag
    # that the earlier ranges have set
    for keep, p in plans.items():
        both = [r['windows'] >= 2 and (LANES[C] != 4 or (r['nlong'] > 0 and r['classes'] == {1, 4, 16} and r['max_nchunks_one_slot'] == 16))
                for r in p['ranges']]
        assert p['big'] and p['windowed'] and (all(both) if keep else any(both)), (keep, both)
    p = plans[True]
    assert (p['nslices'], p['stored']) == {4: (19584, 1854016), 8: (37600, 2822272), 16: (75168, 5201024)}[LANES[C]]


def test_control_the_same_operator_on_the_small_state_plan(hip):
    plans = _products(hip, K.square(), K.N_B, 16, 'f32', (True, False))
    for p in plans.values():
        assert not p['big'] and not p['windowed'] and (p['L1'], p['L4']) == (24, 96)
    assert (plans[True]['nslices'], plans[True]['stored']) == (20320, 1851456)


@pytest.mark.parametrize('C', [1, 16])
def test_fp32_state_at_four_lanes_per_row(hip, C):
    """600 000 rows: the only way to the fp32 plan of 4 lanes per row with windows."""
    p = _products(hip, K.square(K.N_B32), K.N_B32, C, 'f32', (True,))[True]
    assert p['big'] and p['windowed'] and (p['nslices'], p['stored']) == (39104, 3695360)
    assert all(r['windows'] == 3 and r['nlong'] > 0 and r['classes'] == {1, 4, 16} for r in p['ranges'])


# ---- the stop-column forms on fixture B ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('keep', [True, False], ids=['keep', 'own-order'])
def test_single_stop_column_form(hip, keep):
    """Sweep at 10 columns (HAS_W, 4 lanes per row): one run that stops inside, one that runs to the cap."""
    A, deg, vinf, w_unit = K.stop_fixture()
    C = 10
    assert hip.record_layout(C, np.float64, True)['G'] == 4
    Db = R.bias(C, n=K.N_B, seed=K.stop_db_seed(0))
    G = hip.DeviceGraph(A, dtype=np.float64, keep_order=keep)
    try:
        sw = hip.Sweep(G, C, min_iter=K.STOP_MIN, max_iter=K.STOP_MAX, use_hipgraph=False)
        for k, T in K.STOP_K_T:
            want = K.stop_run(C, 0, k)
            assert want[1] == T
            sw.set_problem(Db, 2.0 ** k * w_unit, deg, vinf)
            _same(_run(sw), want, (C, keep, T))
        sw.close()
        info = G.info()
        p = S.plan(np.diff(A.indptr).astype(np.int64)[G.order()], K.N_B, 4, 8)
        assert p['big'] and p['windowed'] and (info['slices'], info['stored']) == (p['nslices'], p['stored'])
    finally:
        G.close()


@pytest.mark.parametrize('C,B,lanes', [(2, 2, 8), (10, 4, 16)])
def test_grouped_stop_column_form(hip, C, B, lanes):
    """SweepGroups: the groups alternate between the run that stops inside and the one that runs to the cap."""
    A, deg, vinf, w_unit = K.stop_fixture()
    G = hip.DeviceGraph(A, dtype=np.float64, keep_order=(C == 2))
    try:
        groups = hip.SweepGroups(G, C, B, min_iter=K.STOP_MIN, max_iter=K.STOP_MAX)
        assert G.info()['rows_per_slice'] * lanes == 64
        groups.set_vectors(deg, vinf)
        rows = np.arange(K.N_B)
        want = []
        for b in range(B):
            k, T = K.STOP_K_T[b % 2]
            w0 = 2.0 ** k * w_unit
            groups.set_problem_rows(b, rows, R.bias(C, n=K.N_B, seed=K.stop_db_seed(b)), w0, R.err0(deg, vinf, w0))
            want.append(K.stop_run(C, b, k))
            assert want[-1][1] == T
        T, _ = groups.run()
        assert list(T) == [K.STOP_K_T[b % 2][1] for b in range(B)]
        for b in range(B):
            _same(_group(groups, T, b), want[b], (C, B, b))
        groups.close()
        info = G.info()
        p = S.plan(np.diff(A.indptr).astype(np.int64)[G.order()], K.N_B, lanes, 8)
        assert p['big'] and p['windowed'] and (info['slices'], info['stored']) == (p['nslices'], p['stored'])
    finally:
        G.close()
