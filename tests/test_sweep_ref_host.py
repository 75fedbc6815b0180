"""CPU: the host restatement of the stop-column sweeps (tests/sweep_ref.py) -- what tests/test_gpu_sweep_stop.py holds the device to.
The entry-order loop equals scipy's products on every fixture, the restatement reproduces the project's oracle on the two-moons golden
bit for bit, and the fixtures stop where they were built to stop: a fixture that drifts fails here, not on the GPU."""
import numpy as np
import pytest
from conftest import csr_from
from oracle import gl_oracle as orc
import sweep_ref as R

DTYPES = ['float64', 'float32']
SUB_LENGTHS = tuple(R.LENGTHS[1:])


def test_loop_equals_scipy_on_every_fixture():
    for lengths in (tuple(R.LENGTHS), SUB_LENGTHS):
        A, deg, vinf, w_unit = R.fixture_a(lengths)
        assert A.shape == (R.N, R.N) and R.prove_products(A, C=7, seed=3)
    assert 57000 < R.fixture_a()[0].nnz < 59000
    P, _, _ = R.half_identity()
    assert P.nnz == R.NB and R.prove_products(P)
    # a whole run either way: same bits
    A, deg, vinf, w_unit = R.fixture_a()
    for dt in DTYPES:
        a = R.poisson_sweeps(A, R.bias(5), 2.0 ** 3 * w_unit, deg, vinf, 3, 60, dt)
        b = R.poisson_sweeps(A, R.bias(5), 2.0 ** 3 * w_unit, deg, vinf, 3, 60, dt, products='loop')
        assert a[1] == b[1] == 12 and a[2] == b[2] == 3
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3]) and a[0].dtype == np.dtype(dt)


def test_host_sweep_is_the_forms_reference():
    """host_sweep (what tests/test_gpu_sweep_forms.py compares the plain product with) against scipy, weights of both signs."""
    A, _, _, _ = R.fixture_a()
    rng = np.random.default_rng(5)
    S = R.as_dtype(A, np.float64)
    S.data = S.data * rng.choice([-1.0, 1.0], size=S.nnz)
    u, Db = rng.normal(size=(R.N, 9)), rng.normal(size=(R.N, 9))
    assert np.array_equal(R.host_sweep(S, u, None, np.float64), S @ u)
    assert np.array_equal(R.host_sweep(S, u, Db, np.float64), Db + S @ u)
    S32 = R.as_dtype(S, np.float32)
    assert np.array_equal(R.host_sweep(S, u, Db, np.float32), Db.astype(np.float32) + S32 @ u.astype(np.float32))


def test_restatement_equals_the_oracle_on_two_moons(golden):
    g = golden('g1_twomoons.npz')
    W = csr_from(g, 'W_gaussian')
    ti, lab = g['train_ind'], g['labels']
    s = orc.poisson_gd_setup(W, ti, lab[ti])
    assert R.prove_products(s['P'])
    u, T, first, vals = R.poisson_sweeps(s['P'], s['Db'], s['v0'] / s['deg'], s['deg'], s['vinf'], 50, 1000, np.float64)
    assert T == int(g['poisson_gd_T']) == 409 and first == 50 and len(vals) == T - first + 1
    assert np.array_equal(u, g['poisson_gd_prob'])
    assert np.all(vals[:-1] > 1 / W.shape[0]) and vals[-1] <= 1 / W.shape[0]


@pytest.mark.parametrize('dt', DTYPES)
def test_ladder_stops_where_it_was_built_to(dt):
    A, deg, vinf, w_unit = R.fixture_a()
    got = []
    for k, T in R.K_T:
        u, t, first, vals = R.ladder_run(3, 23, k, R.MIN_ITER, R.MAX_ITER, dt)
        assert t == T and first == R.MIN_ITER and len(vals) == T - first + 1, (k, t)
        assert np.all(vals[:-1] > 1 / R.N) and vals[-1] <= 1 / R.N
        # the decision is not a near one: a device that rounds the stop value differently fails on the value, not on T
        assert vals[-1] < 0.9 / R.N and (len(vals) < 2 or vals[-2] > 1.1 / R.N)
        got.append(t - first)
    assert got == R.POSITIONS == [0, 1, 2, 15, 16, 17, 33]
    # both values of the slot's bias flag, both signs
    Db = R.bias(3)
    nz = np.any(Db != 0, axis=1)
    assert 0.2 < nz.mean() < 0.4 and Db.min() < 0 < Db.max()
    # the stacked groups: their own table, with and without the unconditional head
    for k, T in R.GROUP_K_T:
        assert R.ladder_run(2, 40, k, R.MIN_ITER, R.MAX_ITER, dt)[1] == T
        assert R.ladder_run(2, 40, k, 0, R.MAX_ITER, dt)[1] == (0 if k == -14.0 else T)
    Ts = [T for _, T in R.GROUP_K_T]
    assert len({(T - R.MIN_ITER) // 16 for T in Ts[:3]}) == 3 and {T & 1 for T in Ts} == {0, 1}
    # the ladder large enough for the library's own renumbering
    assert R.prove_products(R.fixture_a(tuple(R.LENGTHS), R.N_BIG)[0])
    for b, (k, T) in enumerate(R.BIG_K_T):
        u, t, first, vals = R.ladder_run(3, R.group_db_seed(b), k, R.MIN_ITER, R.MAX_ITER, dt, R.N_BIG)
        assert t == T and vals[-1] < 0.9 / R.N_BIG and vals[-2] > 1.1 / R.N_BIG
    assert [T - R.MIN_ITER for _, T in R.BIG_K_T] == [1, 16, 17]
    u, t, first, vals = R.ladder_run(2, 40, -14.0, 0, R.MAX_ITER, dt)
    assert t == 0 and first == 0 and len(vals) == 1 and not u.any()
    assert vals[0] == R.err0(deg, vinf, 2.0 ** -14 * w_unit)


@pytest.mark.parametrize('dt', DTYPES)
def test_iteration_bounds_of_the_restatement(dt):
    u, t, first, vals = R.ladder_run(12, 23, 10.375, 7, 7, dt)          # min_iter = max_iter: nothing is compared
    assert (t, first, len(vals)) == (7, 7, 0)
    u, t, first, vals = R.ladder_run(12, 23, 10.375, 3, 10, dt)         # max_iter reached: the value at t = 10 is never compared
    assert (t, first, len(vals)) == (10, 3, 7) and np.all(vals > 1 / R.N)
    u, t, first, vals = R.ladder_run(12, 23, -0.25, 0, R.MAX_ITER, dt)  # no unconditional head, start above 1 / n
    assert (t, first, len(vals)) == (9, 0, 10)
    u, t, first, vals = R.ladder_run(12, 23, 10.375, 9, 5, dt)          # first = min(min_iter, max_iter)
    assert (t, first, len(vals)) == (5, 5, 0)


@pytest.mark.parametrize('dt', DTYPES)
def test_half_identity_decides_at_one_over_n(dt):
    P, deg, vinf = R.half_identity()
    Db = R.bias_b(3)
    one = np.ones(R.NB)
    for min_iter, T in ((0, 10), (10, 10), (11, 11)):
        u, t, first, vals = R.poisson_sweeps(P, Db, one, deg, vinf, min_iter, 64, dt)
        assert t == T and first == min_iter
        assert np.array_equal(vals, 2.0 ** -np.arange(min_iter, T + 1)) and (T > 10 or vals[-1] == 1 / R.NB)
    above = one.copy()
    above[517] = 1 + 2.0 ** -52
    u, t, first, vals = R.poisson_sweeps(P, Db, above, deg, vinf, 0, 64, dt)
    assert t == 11 and vals[10] == 2.0 ** -10 * (1 + 2.0 ** -52) > 1 / R.NB
    stacked = R.groups(P, [(R.bias_b(3, seed=31 + b), 2.0 ** b * one) for b in (0, 7, 31)], deg, vinf, 0, 64, dt)
    for b, (u, t, first, vals) in zip((0, 7, 31), stacked):
        assert t == 10 + b and np.array_equal(vals, 2.0 ** (b - np.arange(0, t + 1.0)))


@pytest.mark.parametrize('dt', DTYPES)
def test_non_finite_stop_columns(dt):
    A, deg, vinf, w_unit = R.fixture_a()
    w0 = 2.0 ** 10.375 * w_unit
    w0[100] = np.nan
    u, t, first, vals = R.poisson_sweeps(A, R.bias(3), w0, deg, vinf, 5, R.MAX_ITER, dt)
    assert (t, first) == (5, 5) and len(vals) == 1 and np.isnan(vals[0])
    assert np.array_equal(u, R.ladder_run(3, 23, 10.375, 5, 5, dt)[0])            # w never feeds u
    S, deg, vinf, w_unit = R.fixture_a(SUB_LENGTHS)
    w0 = 2.0 ** -10 * w_unit
    w0[100] = np.inf
    assert np.any(S.indices == 100)
    u, t, first, vals = R.poisson_sweeps(S, R.bias(3), w0, deg, vinf, 3, 12, dt)
    assert (t, first) == (12, 3) and len(vals) == 9 and np.all(np.isposinf(vals)) and np.all(np.isfinite(u))


@pytest.mark.parametrize('dt', DTYPES)
def test_rebound_stops_at_equality_below_a_larger_value(dt):
    P, deg, vinf, w0 = R.half_identity_rebound()
    assert P.nnz == R.NB and R.prove_products(P)
    Db = R.bias_b(3)
    for min_iter in (0, 4):
        u, t, first, vals = R.poisson_sweeps(P, Db, w0, deg, vinf, min_iter, 64, dt)
        ts = np.arange(min_iter, 11)
        assert t == 10 and np.array_equal(vals, np.where(ts % 2 == 0, 2.0 ** -ts, 2.0 ** (2.0 - ts))) and vals[-1] == 1 / R.NB
        on = R.poisson_sweeps(P, Db, w0, deg, vinf, 12, 12, dt)[0]      # what two sweeps more would leave behind
        assert not np.array_equal(on, u)
    w = w0.copy()
    for _ in range(11):
        w = P @ w
    assert np.max(np.abs(w)) == 2.0 ** -9 > 1 / R.NB
