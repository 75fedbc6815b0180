"""The stop-column forms of the sweep kernel (csrc/sweep.hip: HAS_W, what ssl.poisson(solver='gradient_descent') runs, and GRP, the
stacked trials) and the host loop around them (glx_sweep_tail, csrc/sweep_core.hip, on the walk of csrc/sweep_stop_plan.h; the heads
are glx_sweep_run's, csrc/solver.hip, and glx_sweep_groups_run's, csrc/groups.hip), bit for bit against the host restatement
tests/sweep_ref.py: the iterate u_T, the sweep count T, the first tested sweep and every stop value
max|deg w - vinf| the run compared with 1 / n.  Everything is np.array_equal; equal_nan only where a NaN is the point.

Fixture A (sweep_ref.ladder): 640 rows of lengths 0 .. 300 on both sides of every row class, positive weights, every row summing to
0.5, so that the stop column halves per sweep and the scale of w0 places T: both parities inside a 16-sweep tail chunk, both sides of
the chunk edge, the third chunk (the host's choice of ping-pong buffer).  Fixture B (sweep_ref.half_identity): P = I / 2, n = 1024,
exact in both dtypes: the decision AT 1 / n; half_identity_rebound: a value equal to 1 / n in front of a larger one, where the kernel's
own gate is what keeps u_T.  tests/test_sweep_ref_host.py holds the restatement and the fixtures' stop positions;
tests/test_sweep_stop_host.py the walk's chunked read-back, without a device."""
import numpy as np
import pytest
import sweep_ref as R

pytestmark = pytest.mark.gpu

DT = {'f64': np.float64, 'f32': np.float32}
# width -> lanes per row with the stop column: both sides of every class 4 | 8 | 16 | 32 | 64
WIDTHS = {1: 4, 12: 4, 13: 8, 28: 8, 29: 16, 60: 16, 61: 32, 124: 32, 125: 64, 252: 64}
ALL_POSITIONS = (1, 12, 13)      # the G = 4 plans (rows of S = 4 / 16 segments) and the first wide one: every stop position
# (C, B) -> lanes per row of the stacked record; (10, 8) is there for G = 32
GROUPS = {'f64': {(2, 2): 8, (3, 5): 8, (10, 4): 16, (10, 5): 16, (5, 8): 16, (5, 9): 16, (10, 8): 32, (7, 32): 64},
          'f32': {(2, 2): 8, (2, 3): 8, (3, 5): 8, (10, 4): 16, (10, 5): 16, (10, 8): 32, (6, 32): 64}}


@pytest.fixture(scope='module')
def hip():
    from graphlearning_amd import _hip
    _hip.require_device()
    return _hip


@pytest.fixture(scope='module')
def ladder(hip):
    """Fixture A and one operator per (dtype, order): the caller's order kept, and the library's locality order (at 640 rows it has to
    be handed over: the library renumbers by itself from 4096 rows on -- test_the_librarys_own_renumbering)."""
    A, deg, vinf, w_unit = R.fixture_a()
    order = hip.host_locality_order(A.indptr, A.indices)
    graphs = {}
    for name, dt in DT.items():
        graphs[name, 'keep'] = hip.DeviceGraph(A, dtype=dt, keep_order=True)
        graphs[name, 'renum'] = hip.DeviceGraph(A, dtype=dt, order=order)
        assert np.array_equal(graphs[name, 'keep'].order(), np.arange(R.N))
        perm = graphs[name, 'renum'].order()      # deg / vinf / w0 travel through it
        assert not np.array_equal(perm, np.arange(R.N)) and np.array_equal(np.sort(perm), np.arange(R.N))
    yield A, deg, vinf, w_unit, graphs
    for G in graphs.values():
        G.close()


def _same(got, want, what, equal_nan=False):
    """(u, T, first, values) of the device against the restatement's."""
    u, T, first, vals = got
    ur, Tr, firstr, valsr = want
    assert T == Tr and first == firstr, (what, T, Tr, first, firstr)
    assert vals.dtype == np.float64 and vals.shape == valsr.shape, (what, vals.shape, valsr.shape)
    assert np.array_equal(vals, valsr, equal_nan=equal_nan), (what, vals, valsr)
    u = np.asarray(u)
    assert u.dtype == ur.dtype and u.shape == ur.shape and np.array_equal(u, ur), (what, 'iterate')


def _run(sw):
    T, _ = sw.run()
    first, vals = sw.stop_values()
    return np.array(sw.fetch()), T, first, vals


def _positions(C):
    if C in ALL_POSITIONS:
        return list(range(len(R.K_T)))
    i = list(WIDTHS).index(C) % 4       # two per width: between them the other widths see every position too
    return [i, i + 3]


# ---- the single stop-column form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', list(DT))
@pytest.mark.parametrize('C', list(WIDTHS))
def test_single_form_equals_the_restatement(hip, ladder, C, dtype):
    A, deg, vinf, w_unit, graphs = ladder
    assert hip.record_layout(C, DT[dtype], True)['G'] == WIDTHS[C]
    Db = R.bias(C).astype(DT[dtype])
    for order in ('keep', 'renum'):
        G = graphs[dtype, order]
        sw = hip.Sweep(G, C, min_iter=R.MIN_ITER, max_iter=R.MAX_ITER, use_hipgraph=False)
        for i in _positions(C):
            k, T = R.K_T[i]
            want = R.ladder_run(C, 23, k, R.MIN_ITER, R.MAX_ITER, np.dtype(DT[dtype]).name)
            assert want[1] == T
            sw.set_problem(Db, 2.0 ** k * w_unit, deg, vinf)
            _same(_run(sw), want, (C, dtype, order, T))
        sw.close()
        u, T = G.poisson_sweep(Db, 2.0 ** k * w_unit, deg, vinf, min_iter=R.MIN_ITER, max_iter=R.MAX_ITER)
        assert T == want[1] and u.dtype == want[0].dtype and np.array_equal(u, want[0]), (C, dtype, order, 'poisson_sweep')


@pytest.mark.parametrize('dtype', list(DT))
def test_iteration_bounds(hip, ladder, dtype):
    A, deg, vinf, w_unit, graphs = ladder
    name = np.dtype(DT[dtype]).name
    C = 12
    Db = R.bias(C).astype(DT[dtype])
    cases = [(0, R.MAX_ITER, -14.0, 0),       # the start is already at or below 1 / n: no sweep, u = 0
             (0, R.MAX_ITER, -0.25, 9),       # no unconditional head
             (7, 7, 10.375, 7),               # min_iter = max_iter: nothing is compared
             (3, 10, 10.375, 10)]             # max_iter reached: the value at t = max_iter is never compared
    for order in ('keep', 'renum'):
        for min_iter, max_iter, k, T in cases:
            want = R.ladder_run(C, 23, k, min_iter, max_iter, name)
            assert want[1] == T
            sw = hip.Sweep(graphs[dtype, order], C, min_iter=min_iter, max_iter=max_iter, use_hipgraph=False)
            sw.set_problem(Db, 2.0 ** k * w_unit, deg, vinf)
            got = _run(sw)
            _same(got, want, (dtype, order, min_iter, max_iter, k))
            if T == 0:
                assert not got[0].any() and len(got[3]) == 1
            sw.close()


@pytest.mark.parametrize('dtype', list(DT))
@pytest.mark.parametrize('C', [12, 29])
def test_captured_head_and_sparse_problem(hip, ladder, C, dtype):
    """Three runs of one prepared sweep (the second captures its head, the third replays it), then a new problem given by rows."""
    A, deg, vinf, w_unit, graphs = ladder
    name = np.dtype(DT[dtype]).name
    Db = R.bias(C).astype(DT[dtype])
    k, T = R.K_T[4]
    want = R.ladder_run(C, 23, k, R.MIN_ITER, R.MAX_ITER, name)
    sw = hip.Sweep(graphs[dtype, 'renum'], C, min_iter=R.MIN_ITER, max_iter=R.MAX_ITER, use_hipgraph=True)
    sw.set_problem(Db, 2.0 ** k * w_unit, deg, vinf)
    for run in range(3):
        _same(_run(sw), want, (C, dtype, 'run', run))
    k2, T2 = R.K_T[2]
    want2 = R.ladder_run(C, 41, k2, R.MIN_ITER, R.MAX_ITER, name)
    assert want2[1] == T2 and not np.array_equal(want2[0], want[0][:, :C])
    w0 = 2.0 ** k2 * w_unit
    sw.set_vectors(deg, vinf)
    sw.set_problem_rows(np.arange(R.N), R.bias(C, seed=41).astype(DT[dtype]), w0, R.err0(deg, vinf, w0))
    by_rows = _run(sw)
    _same(by_rows, want2, (C, dtype, 'rows'))
    sw.set_problem(R.bias(C, seed=41).astype(DT[dtype]), w0, deg, vinf)
    _same(_run(sw), by_rows, (C, dtype, 'dense'))
    sw.close()


def _sparse_problems(C, dtype):
    """Four training sets given by rows, in the order a resident sweep meets them: a subset of the rows (a row without entries among
    them), one that keeps half of it and adds new rows, the empty one, the first again.  Each as (rows, Db_rows, w0_rows, err0, the
    restatement's run on the dense arrays that are zero outside the rows)."""
    A, deg, vinf, w_unit = R.fixture_a()
    rng = np.random.default_rng(77)
    first = np.concatenate([[0, 18], rng.choice(np.setdiff1d(np.arange(R.N), [0, 18]), size=78, replace=False)])
    new = rng.choice(np.setdiff1d(np.arange(R.N), first), size=60, replace=False)
    second = rng.permutation(np.concatenate([first[::2], new]))
    problems = []
    for rows, k, seed in ((first, R.K_T[4][0], 51), (second, R.K_T[6][0], 52), (first[:0], 0.0, 53), (first, R.K_T[4][0], 51)):
        Db_rows = R.bias(C, seed=seed)[rows]
        Db_rows[::5] = 0.0                          # labelled rows whose bias is zero: their flag stays down
        w0_rows = 2.0 ** k * w_unit[rows]
        Db, w0 = np.zeros((R.N, C)), np.zeros(R.N)
        Db[rows], w0[rows] = Db_rows, w0_rows
        want = R.poisson_sweeps(A, Db, w0, deg, vinf, R.MIN_ITER, R.MAX_ITER, DT[dtype])
        problems.append((rows.astype(np.int64), Db_rows.astype(DT[dtype]), w0_rows, R.err0(deg, vinf, w0), want))
    T = [p[4][1] for p in problems]
    assert T[0] == T[3] and len(set(T[:3])) == 3 and sum(t > R.MIN_ITER for t in T[:3]) >= 2, T      # (holds on the CPU: no device involved)
    assert problems[1][4][0].any() and not problems[2][4][0].any()
    return problems


@pytest.mark.parametrize('dtype', list(DT))
def test_sparse_problems_in_turn(hip, ladder, dtype):
    """The rows of a training set replace the previous set's rows -- bias, flags and start values of the rows that left are cleared, the
    staging and the row lists grow -- in one prepared sweep (its head eager, then captured, then replayed) and in one group of a
    stacked one, whose other groups do not move."""
    A, deg, vinf, w_unit, graphs = ladder
    dt, name = DT[dtype], np.dtype(DT[dtype]).name
    G = graphs[dtype, 'renum']
    sw = hip.Sweep(G, 12, min_iter=R.MIN_ITER, max_iter=R.MAX_ITER, use_hipgraph=True)
    sw.set_vectors(deg, vinf)
    for i, (rows, Db_rows, w0_rows, err0, want) in enumerate(_sparse_problems(12, dtype)):
        sw.set_problem_rows(rows, Db_rows, w0_rows, err0)
        _same(_run(sw), want, (dtype, 'single', i))
    sw.close()
    C, B, g = 3, 5, 2
    groups = hip.SweepGroups(G, C, B, min_iter=R.MIN_ITER, max_iter=R.MAX_ITER)
    groups.set_vectors(deg, vinf)
    _set_groups(groups, C, B, dt, deg, vinf, w_unit)
    others = None
    for i, (rows, Db_rows, w0_rows, err0, want) in enumerate(_sparse_problems(C, dtype)):
        groups.set_problem_rows(g, rows, Db_rows, w0_rows, err0)
        T, _ = groups.run()
        _same(_group(groups, T, g), want, (dtype, 'stacked', i))
        got = [_group(groups, T, b) for b in range(B) if b != g]
        if others is None:
            others = got
            for b, o in zip([b for b in range(B) if b != g], others):
                _same(o, R.ladder_run(C, R.group_db_seed(b), R.group_k(b), R.MIN_ITER, R.MAX_ITER, name), (dtype, 'stacked', 'other', b))
        for o, o0 in zip(got, others):
            _same(o, o0, (dtype, 'stacked', i, 'others moved'))
    groups.close()


@pytest.mark.parametrize('dtype', list(DT))
def test_the_librarys_own_renumbering(hip, dtype):
    """The ladder at 4608 rows: the library picks the vertex order itself, and deg / vinf / w0 / Db travel through it -- the single
    form at 4 lanes per row and three stacked groups."""
    A, deg, vinf, w_unit = R.fixture_a(tuple(R.LENGTHS), R.N_BIG)
    dt, name = DT[dtype], np.dtype(DT[dtype]).name
    C, B = 3, len(R.BIG_K_T)
    G = hip.DeviceGraph(A, dtype=dt)
    perm = G.order()
    assert G.info()['renumbered'] == 1 and not np.array_equal(perm, np.arange(R.N_BIG)) and np.array_equal(np.sort(perm), np.arange(R.N_BIG))
    want = [R.ladder_run(C, R.group_db_seed(b), k, R.MIN_ITER, R.MAX_ITER, name, R.N_BIG) for b, (k, T) in enumerate(R.BIG_K_T)]
    assert [w[1] for w in want] == [T for _, T in R.BIG_K_T]
    sw = hip.Sweep(G, C, min_iter=R.MIN_ITER, max_iter=R.MAX_ITER, use_hipgraph=False)
    groups = hip.SweepGroups(G, C, B, min_iter=R.MIN_ITER, max_iter=R.MAX_ITER)
    groups.set_vectors(deg, vinf)
    for b, (k, T) in enumerate(R.BIG_K_T):
        Db, w0 = R.bias(C, n=R.N_BIG, seed=R.group_db_seed(b)).astype(dt), 2.0 ** k * w_unit
        sw.set_problem(Db, w0, deg, vinf)
        _same(_run(sw), want[b], (dtype, 'single', b))
        groups.set_problem_rows(b, np.arange(R.N_BIG), Db, w0, R.err0(deg, vinf, w0))
    T, _ = groups.run()
    for b in range(B):
        _same(_group(groups, T, b), want[b], (dtype, 'stacked', b))
    sw.close()
    groups.close()
    G.close()


# ---- the grouped form --------------------------------------------------------------------------------------------------------------
def _set_groups(groups, C, B, dt, deg, vinf, w_unit, w0_of=None):
    rows = np.arange(R.N)
    for b in range(B):
        w0 = 2.0 ** R.group_k(b) * w_unit if w0_of is None else w0_of(b)
        groups.set_problem_rows(b, rows, R.bias(C, seed=R.group_db_seed(b)).astype(dt), w0, R.err0(deg, vinf, w0))


def _group(groups, T, b):
    first, vals = groups.stop_values(b)
    return np.array(groups.fetch(b)), T[b], first, vals


@pytest.mark.parametrize('dtype,C,B', [(d, C, B) for d in DT for (C, B) in GROUPS[d]])
def test_grouped_form_equals_the_restatement(hip, ladder, dtype, C, B):
    """Every group with its own right-hand side and its own scale of w0: the groups stop at different sweeps, in different chunks."""
    A, deg, vinf, w_unit, _ = ladder
    dt, name = DT[dtype], np.dtype(DT[dtype]).name
    G = hip.DeviceGraph(A, dtype=dt, keep_order=(B % 2 == 0))      # a graph of its own: its first plan is the stacked record's
    for min_iter in (R.MIN_ITER, 0):
        groups = hip.SweepGroups(G, C, B, min_iter=min_iter, max_iter=R.MAX_ITER)
        assert G.info()['rows_per_slice'] * GROUPS[dtype][C, B] == 64
        groups.set_vectors(deg, vinf)
        _set_groups(groups, C, B, dt, deg, vinf, w_unit)
        want = [R.ladder_run(C, R.group_db_seed(b), R.group_k(b), min_iter, R.MAX_ITER, name) for b in range(B)]
        assert len({w[1] for w in want}) == min(B, len(R.GROUP_K_T))
        T, _ = groups.run()
        assert len(T) == B
        for b in range(B):
            _same(_group(groups, T, b), want[b], (dtype, C, B, min_iter, b))
        if min_iter == 0:      # a group that never runs beside running ones
            assert T[1] == 0 and not np.array(groups.fetch(1)).any() and max(T) >= 19
        # the last group left out: the others are what they were
        T, _ = groups.run(used=B - 1)
        assert len(T) == B - 1
        for b in range(B - 1):
            _same(_group(groups, T, b), want[b], (dtype, C, B, min_iter, b, 'used'))
        assert not np.array(groups.fetch(B - 1)).any()      # idle: still the zero it started from
        groups.close()
    G.close()


def test_too_wide_a_stack_is_refused(hip, ladder):
    A = ladder[0]
    G = hip.DeviceGraph(A, dtype=np.float32, keep_order=True)
    with pytest.raises(hip.GlxError):      # 56 column lanes + 16 stop lanes
        hip.SweepGroups(G, 7, 32, min_iter=R.MIN_ITER, max_iter=R.MAX_ITER)
    G.close()


# ---- fixture B: the decision at 1 / n ----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def half(hip):
    P, deg, vinf = R.half_identity()
    assert R.prove_products(P)
    graphs = {name: hip.DeviceGraph(P, dtype=dt) for name, dt in DT.items()}
    yield P, deg, vinf, graphs
    for G in graphs.values():
        G.close()


@pytest.mark.parametrize('dtype', list(DT))
def test_decision_at_one_over_n(hip, half, dtype):
    P, deg, vinf, graphs = half
    dt = DT[dtype]
    C = 3
    Db = R.bias_b(C).astype(dt)
    one = np.ones(R.NB)
    above = one.copy()
    above[517] = 1 + 2.0 ** -52      # one ulp above: only an fp64 stop value sees it
    for min_iter, w0, T in ((0, one, 10), (10, one, 10), (11, one, 11), (0, above, 11), (10, above, 11)):
        want = R.poisson_sweeps(P, Db, w0, deg, vinf, min_iter, 64, dt)
        assert want[1] == T
        sw = hip.Sweep(graphs[dtype], C, min_iter=min_iter, max_iter=64, use_hipgraph=False)
        sw.set_problem(Db, w0, deg, vinf)
        got = _run(sw)
        _same(got, want, (dtype, min_iter, T))
        if w0 is one:
            assert np.array_equal(got[3], 2.0 ** -np.arange(min_iter, T + 1.0))
        sw.close()


@pytest.mark.parametrize('dtype', list(DT))
def test_equality_stops_the_kernel_too(hip, dtype):
    """The stop value at t = 10 equals 1 / n and the one behind it is above 1 / n again (sweep_ref.half_identity_rebound): the kernels
    launched behind sweep 9 must all have returned at their gate, or u_10 is gone by the time the host has read T."""
    P, deg, vinf, w0 = R.half_identity_rebound()
    dt = DT[dtype]
    C = 3
    Db = R.bias_b(C).astype(dt)
    G = hip.DeviceGraph(P, dtype=dt)
    for min_iter in (0, 4):
        want = R.poisson_sweeps(P, Db, w0, deg, vinf, min_iter, 64, dt)
        assert want[1] == 10 and want[3][-1] == 1 / R.NB
        sw = hip.Sweep(G, C, min_iter=min_iter, max_iter=64, use_hipgraph=False)
        sw.set_problem(Db, w0, deg, vinf)
        _same(_run(sw), want, (dtype, min_iter, 'rebound'))
        sw.close()
    G.close()


@pytest.mark.parametrize('dtype,C', [('f64', 7), ('f32', 6)])
def test_decision_at_one_over_n_grouped(hip, half, dtype, C):
    """32 groups, group b from w0 = 2^b: it stops at sweep 10 + b exactly -- over three chunks, every one frozen at its own sweep."""
    P, deg, vinf, graphs = half
    dt = DT[dtype]
    B = 32
    one = np.ones(R.NB)
    rows = np.arange(R.NB)
    groups = hip.SweepGroups(graphs[dtype], C, B, min_iter=0, max_iter=64)
    groups.set_vectors(deg, vinf)
    for b in range(B):
        groups.set_problem_rows(b, rows, R.bias_b(C, seed=31 + b).astype(dt), 2.0 ** b * one, 2.0 ** b)
    T, _ = groups.run()
    assert T == [10 + b for b in range(B)]
    want = R.groups(P, [(R.bias_b(C, seed=31 + b), 2.0 ** b * one) for b in range(B)], deg, vinf, 0, 64, dt)
    for b in range(B):
        _same(_group(groups, T, b), want[b], (dtype, b))
    groups.close()


# ---- non-finite stop columns -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,C,B', [('f64', 3, 5), ('f32', 2, 3), ('f32', 3, 5)])
def test_nan_in_one_group_stops_that_group_alone(hip, ladder, dtype, C, B):
    A, deg, vinf, w_unit, graphs = ladder
    dt, name = DT[dtype], np.dtype(DT[dtype]).name
    bad = B - 1      # f32, B odd: the stop lane it has to itself

    def w0_of(b):
        w0 = 2.0 ** R.group_k(b) * w_unit
        if b == bad:
            w0[100] = np.nan
        return w0

    groups = hip.SweepGroups(graphs[dtype, 'renum'], C, B, min_iter=5, max_iter=R.MAX_ITER)
    groups.set_vectors(deg, vinf)
    _set_groups(groups, C, B, dt, deg, vinf, w_unit)
    T, _ = groups.run()
    clean = [_group(groups, T, b) for b in range(B)]
    _set_groups(groups, C, B, dt, deg, vinf, w_unit, w0_of)
    T, _ = groups.run()
    for b in range(B):
        got = _group(groups, T, b)
        if b == bad:
            want = R.poisson_sweeps(A, R.bias(C, seed=R.group_db_seed(b)), w0_of(b), deg, vinf, 5, R.MAX_ITER, dt)
            assert want[1] == 5 and np.isnan(want[3]).tolist() == [True]
            _same(got, want, (dtype, C, B, b, 'nan'), equal_nan=True)
        else:
            _same(got, R.ladder_run(C, R.group_db_seed(b), R.group_k(b), 5, R.MAX_ITER, name), (dtype, C, B, b))
            _same(got, clean[b], (dtype, C, B, b, 'clean run'))
    groups.close()


@pytest.mark.parametrize('dtype', list(DT))
def test_infinite_stop_value_runs_on(hip, dtype):
    """inf > 1 / n: the run goes on to max_iter, and every recorded value is inf."""
    S, deg, vinf, w_unit = R.fixture_a(tuple(R.LENGTHS[1:]))      # no empty row
    dt = DT[dtype]
    C = 3
    w0 = 2.0 ** -10 * w_unit
    w0[100] = np.inf
    want = R.poisson_sweeps(S, R.bias(C), w0, deg, vinf, 3, 12, dt)
    assert want[1] == 12 and np.all(np.isposinf(want[3])) and len(want[3]) == 9
    G = hip.DeviceGraph(S, dtype=dt)
    sw = hip.Sweep(G, C, min_iter=3, max_iter=12, use_hipgraph=False)
    sw.set_problem(R.bias(C).astype(dt), w0, deg, vinf)
    _same(_run(sw), want, (dtype, 'inf'))
    sw.close()
    G.close()
