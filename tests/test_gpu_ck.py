"""ssl.centered_kernel and _hip.ck_solve on the device: the reference's golden vectors within the bound measured when the fixture
was made (T equal, predict() equal on every vertex), the device against the device-order restatement of tests/ck_ref.py BIT FOR BIT on
seeded graphs at the shapes where the kernels can go wrong, the seams of the chunked schedule, repeatability with the pool on, off
and poisoned, the draws the start vector takes from numpy's global stream, the lines of an all_labels fit and ssl_trials' file.

Every test runs under a time limit of its own: a test that exceeds it ends the whole session on the spot (traceback of every
thread, then exit), so nothing more is started on a device that may have hung; nothing is retried."""
import faulthandler
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ck_ref as ref  # noqa: E402
from test_ck_host import load_golden, golden_case, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu


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
    return load_golden()


@pytest.fixture(scope='module')
def blobs(gold):
    """The `blobs` case as the device call takes it, with the device-order restatement at the default tol, computed once."""
    W, ind, labels, k, seed, e = golden_case(gold, 'blobs')
    Wd = ref.without_diagonal(W)
    val = np.ascontiguousarray(ref.start_values(W.shape[0], ind, labels, k)[ind])
    want = ref.ck_device_order(Wd.indptr, Wd.indices, Wd.data, ind, val, e)
    return Wd, ind, val, e, want


def solve(W, ind, val, e, **kw):
    from graphlearning_amd import _hip
    return _hip.ck_solve(W.indptr, W.indices, W.data, ind, val, e, **kw)


@pytest.mark.parametrize('name', sorted(ref.GOLDEN_CASES))
def test_golden_within_the_measured_bound(gl, gold, name):
    W, ind, labels, k, seed, e = golden_case(gold, name)
    prob, bound = gold['case_%s_prob' % name], float(gold['bound'])
    np.random.seed(seed)
    model = gl.ssl.centered_kernel(W)
    u = model.fit(ind, labels)
    l_ref = float(gold['case_%s_l' % name])
    print(name, 'T', model.num_iter, 'largest difference', np.abs(u - prob).max(), 'bound', bound, 'l', model.eigenvalue,
          'relative difference', abs(model.eigenvalue - l_ref) / l_ref, 'plan', model.ck_plan)
    assert model.num_iter == int(gold['case_%s_T' % name])
    assert np.abs(u - prob).max() <= bound
    assert abs(model.eigenvalue - l_ref) <= float(gold['l_bound']) * l_ref
    assert np.array_equal(model.predict(), gold['case_%s_pred' % name])
    assert model.ck_plan[0] == 2 and model.ck_plan[2] == 64 and model.ck_plan[3] == (W.shape[0] + 63) // 64
    np.random.seed(seed)
    with_priors = gl.ssl.centered_kernel(W, class_priors=gold['case_%s_priors' % name])
    assert np.array_equal(with_priors.fit_predict(ind, labels), gold['case_%s_pred_priors' % name])
    assert same_bits(np.ascontiguousarray(with_priors.prob), np.ascontiguousarray(u))
    # and the device is the device-order restatement, bit for bit
    want = ref.device_order_case(W, ind, labels, k, e)
    assert same_bits(np.ascontiguousarray(u), want[0]) and model.eigenvalue == want[1] and model.num_iter == want[2]


# seed, n, k, hub, directed, rows without entries: every n of {1, 2, 63, 64, 65, 257, 1000} (one partial exactly: 1 .. 64; n no multiple
# of the 64 rows of a partial: 65, 257, 1000), every k of {1, 2, 3, 10, 17, 64, 65, 256} (one column tile up to 16, tiles of unequal width
# at 17 and 65, sixteen tiles at 256), and n = 4097: 65 partials, so that chain 0 of the finishing kernel holds two of them, with one
# round of its 16 columns (k = 2: four sums) and three (k = 17: 34 sums); the seeds are ones whose
# problem stops within a few hundred iterations at tol = 1e-6
SHAPES = [(10, 1, 1, 0, False, 0), (11, 2, 2, 0, False, 0), (12, 63, 3, 0, False, 0), (13, 64, 10, 0, False, 0), (14, 65, 17, 0, False, 0),
          (100, 257, 64, 0, False, 2), (16, 257, 65, 0, False, 0), (40, 1000, 256, 0, False, 0), (41, 1000, 1, 0, False, 3),
          (19, 1000, 2, 0, False, 0), (100, 1000, 10, 0, False, 0), (5, 64, 10, 0, True, 0), (107, 1000, 17, 0, True, 2),
          (36, 4097, 2, 0, False, 0), (17, 4097, 17, 0, False, 0)]


@pytest.mark.parametrize('seed,n,k,hub,directed,lonely', SHAPES)
def test_seeded_shapes_bit_for_bit(gl, seed, n, k, hub, directed, lonely):
    W, ind, val, e = ref.random_problem(seed, n, k, hub=hub, directed=directed, empty_rows=lonely)
    want_u, want_l, want_T, want_errs, capped = ref.ck_device_order(W.indptr, W.indices, W.data, ind, val, e, tol=1e-6)
    assert not capped and np.all(np.isfinite(want_u))
    u, l, T, errs, plan = solve(W, ind, val, e, tol=1e-6, err_cap=want_T + 8)
    print((n, k), 'T', T, want_T, 'differing values', int((u != want_u).sum()), 'plan', plan)
    assert T == want_T and same_bits(u, want_u) and (l == want_l or (l != l and want_l != want_l))
    assert same_bits(errs[:T], want_errs) and np.all(np.isnan(errs[T:]))
    assert plan[0] == 2 and plan[1] == 2 * 100 + 2 + 2 * 64 * ((T + 63) // 64) and plan[3] == (n + 63) // 64


# seed, n, k: uneven column tiles together with a ragged last row block, the smallest shapes at which a wrong first column or width of
# a tile shows: k = 1 and 16 are one tile, 17 is 9 + 8, 33 is three tiles of 11; n = 65 and 130 leave the 64 rows of a partial with a
# remainder of one row and of two ((65, 17) is among SHAPES); the seeds are ones whose problem stops within 220 iterations at tol = 1e-6
TILE_SHAPES = [(205, 65, 1), (202, 65, 16), (202, 65, 33), (208, 130, 1), (200, 130, 16), (200, 130, 17), (200, 130, 33)]


@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    return ref.build_host_lib(tmp_path_factory.mktemp('ck_plan'))


@pytest.mark.parametrize('seed,n,k', TILE_SHAPES)
def test_uneven_tiles_on_a_ragged_row_block_bit_for_bit(gl, host_lib, seed, n, k):
    """the device against ck_host_reference (csrc/ck_plan.h built on the host)"""
    W, ind, val, e = ref.random_problem(seed, n, k)
    want_u, want_l, want_T, want_errs, capped = ref.host_solve(host_lib, W.indptr, W.indices, W.data, ind, val, e, tol=1e-6, cap=256)
    assert not capped and want_T <= 220 and np.all(np.isfinite(want_u))
    u, l, T, errs, plan = solve(W, ind, val, e, tol=1e-6, err_cap=want_T)
    print((n, k), 'T', T, want_T, 'differing values', int((u != want_u).sum()), 'plan', plan)
    assert T == want_T and same_bits(u, want_u) and l == want_l and same_bits(errs, want_errs)
    assert plan[3] == (n + 63) // 64


# hub row length -> a seed whose problem stops within a few hundred iterations
HUB_SEEDS = {63: 105, 64: 43, 65: 40, 255: 41, 256: 102, 257: 41}


@pytest.mark.parametrize('hub', sorted(HUB_SEEDS))
def test_hub_rows_bit_for_bit(gl, hub):
    W, ind, val, e = ref.random_problem(HUB_SEEDS[hub], 300, 3, hub=hub, directed=True)
    assert np.diff(W.indptr).max() == hub
    want_u, want_l, want_T, want_errs, capped = ref.ck_device_order(W.indptr, W.indices, W.data, ind, val, e, tol=1e-6)
    assert not capped and np.all(np.isfinite(want_u))
    u, l, T, errs, plan = solve(W, ind, val, e, tol=1e-6, err_cap=want_T)
    print(hub, 'T', T, want_T, 'differing values', int((u != want_u).sum()))
    assert T == want_T and same_bits(u, want_u) and l == want_l and same_bits(errs, want_errs)


def test_a_nan_err_stops_the_device_where_it_stops_the_restatement(gl):
    """A problem whose iterates overflow: err becomes NaN (inf - inf) and `nan > tol` is false, so the reference's loop ends there.
    The NaN must reach the slot -- an integer maximum that lost it would run on to max_it.  NaNs differ in sign and payload between
    hosts and the device, so they are compared by position."""
    W, ind, val, e = ref.random_problem(42, 257, 64, directed=False, empty_rows=2)
    want_u, want_l, want_T, want_errs, capped = ref.ck_device_order(W.indptr, W.indices, W.data, ind, val, e, tol=1e-6)
    assert not capped and np.isnan(want_errs[-1]) and not np.isnan(want_errs[:-1]).any()
    u, l, T, errs, plan = solve(W, ind, val, e, tol=1e-6, err_cap=want_T + 8, max_it=want_T + 200)
    assert T == want_T and l == want_l and np.isnan(errs[T - 1]) and same_bits(errs[:T - 1], want_errs[:-1])
    assert np.array_equal(np.isnan(u), np.isnan(want_u)) and np.array_equal(u[~np.isnan(u)], want_u[~np.isnan(u)])


@pytest.mark.parametrize('T', [1, 63, 64, 65, 128, 129])
def test_chunk_seams(gl, blobs, T):
    """A stop just before, at and just after the end of a chunk of 64 iterations: tol halfway between err_T and err_{T-1} leaves no
    doubt.  The iterate includes the stopping iteration's update and nothing that was enqueued behind it."""
    W, ind, val, e, full = blobs
    tol = ref.stop_tol(full[3], T)
    want = ref.ck_device_order(W.indptr, W.indices, W.data, ind, val, e, tol=tol)
    assert want[2] == T
    u, l, got_T, errs, plan = solve(W, ind, val, e, tol=tol, err_cap=200)
    assert got_T == T and same_bits(u, want[0]) and l == want[1]
    assert same_bits(errs[:T], full[3][:T]) and np.all(np.isnan(errs[T:]))
    assert plan[1] == 2 * 100 + 2 + 2 * 64 * ((T + 63) // 64)


def test_no_iteration_and_the_iteration_cap(gl, blobs):
    from graphlearning_amd import _hip
    W, ind, val, e, full = blobs
    K = np.zeros((W.shape[0], val.shape[1]))
    K[ind] = val
    for tol in (1.0, np.nan):
        u, l, T, errs, plan = solve(W, ind, val, e, tol=tol, err_cap=4)
        assert T == 0 and same_bits(u, K) and l == full[1] and np.all(np.isnan(errs)) and plan[1] == 2 * 100 + 2
    for max_it in (5, 64, 70):
        with pytest.raises(_hip.GlxError, match='no stop within max_it=%d' % max_it):
            solve(W, ind, val, e, max_it=max_it)
    u, l, T, errs, plan = solve(W, ind, val, e, max_it=full[2])          # exactly enough
    assert T == full[2] and same_bits(u, full[0])


def test_the_same_bits_with_the_pool_on_off_and_poisoned(gl, blobs):
    from graphlearning_amd import _hip
    W, ind, val, e, full = blobs
    a = solve(W, ind, val, e, err_cap=400)
    b = solve(W, ind, val, e, err_cap=400)
    assert same_bits(a[0], b[0]) and a[1:3] == b[1:3] and same_bits(a[3], b[3])
    assert same_bits(a[0], full[0]) and a[1] == full[1] and a[2] == full[2] and same_bits(a[3][:a[2]], full[3])
    _hip.pool_set_enabled(False)
    try:
        c = solve(W, ind, val, e, err_cap=400)
    finally:
        _hip.pool_set_enabled(True)
    assert same_bits(a[0], c[0]) and a[1:3] == c[1:3] and same_bits(a[3], c[3])
    for byte in (0xFF, 0x7F):                       # every pooled block filled with NaN patterns / huge numbers when it is handed out
        _hip.pool_set_poison(byte)
        try:
            d = solve(W, ind, val, e, err_cap=400)
        finally:
            session = [s for s in os.environ.get('GLX_TEST_ABLATE', '').split(',') if s.startswith('poison')]      # (an ablation run's own fill)
            _hip.pool_set_poison(int(session[0][6:] or '255') if session else -1)
        assert same_bits(a[0], d[0]) and a[1:3] == d[1:3] and same_bits(a[3], d[3]), byte


def test_the_start_vector_takes_n_draws_of_the_global_stream(gl, gold):
    W, ind, labels, k, seed, e = golden_case(gold, 'tiny')
    n = W.shape[0]
    twin = np.random.RandomState(77)
    np.random.seed(77)
    model = gl.ssl.centered_kernel(W)
    u = model.fit(ind, labels)
    drawn = twin.rand(n, 1)
    assert np.random.rand() == twin.rand()                                # the stream moved on by exactly n draws
    want = ref.device_order_case(W, ind, labels, k, drawn)
    assert same_bits(np.ascontiguousarray(u), want[0]) and model.eigenvalue == want[1]


def test_all_labels_lines(gl, gold, capsys):
    W, ind, labels, k, seed, e = golden_case(gold, 'tiny')
    truth = gold['graph_tiny_truth']
    np.random.seed(seed)
    plain = gl.ssl.centered_kernel(W).fit(ind, labels)
    capsys.readouterr()
    np.random.seed(seed)
    model = gl.ssl.centered_kernel(W)
    u = model.fit(ind, labels, all_labels=truth)
    out = capsys.readouterr().out.splitlines()
    assert out == [str(s) for s in gold['case_tiny_lines']]
    assert model.num_iter == len(out) and model.ck_plan[2] == 1          # one iteration per chunk on this path
    assert same_bits(np.ascontiguousarray(u), np.ascontiguousarray(plain))


def test_ssl_trials_writes_the_reference_format(gl, gold, tmp_path, monkeypatch):
    W, ind, labels, k, seed, e = golden_case(gold, 'blobs')
    truth = gold['graph_blobs_truth']
    rng = np.random.default_rng(3)
    other = np.concatenate([rng.choice(np.where(truth == c)[0], size=2, replace=False) for c in range(k)])
    monkeypatch.setattr(gl.ssl, 'results_dir', str(tmp_path / 'results'))
    model = gl.ssl.centered_kernel(W)
    np.random.seed(seed)
    model.ssl_trials([other, ind], truth, tag='ck_')
    path = tmp_path / 'results' / 'ck__centered_kernel_accuracy.csv'
    lines = path.read_text().splitlines()
    assert lines[0] == 'Number of labels,Accuracy' and len(lines) == 3
    counts = [int(s.split(',')[0]) for s in lines[1:]]
    assert counts == [len(other), len(ind)]
    np.random.seed(seed)
    again = gl.ssl.centered_kernel(W)
    again.fit(other, truth[other])
    acc = gl.ssl.ssl_accuracy(again.fit_predict(ind, labels), truth, ind)
    assert lines[2] == '%d,%.2f' % (len(ind), acc)
    assert model.trials_statistics(tag='ck_')[0].tolist() == sorted(counts)
