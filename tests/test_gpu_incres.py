"""clustering.incres and _hip.Incres on the device: the reference's recorded labels and sweep counts EXACTLY (tests/golden/g21_incres.npz),
the device against the numpy restatement of tests/incres_ref.py after every outer iteration at the shapes where the kernels can go
wrong, long loops whose values reach the denormal range, independence of the chunk length, the cap on the sweeps as an error return,
and repeatability with the pool off and poisoned.

Every test runs under a time limit of its own: a test that exceeds it ends the whole session on the spot (traceback of every thread,
then exit), so nothing more is started on a device that may have hung; nothing is retried."""
import faulthandler
import os
import sys

import numpy as np
import pytest
from scipy import sparse

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import incres_ref as ref  # noqa: E402

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
    return ref.load_golden()


def device(P, k):
    from graphlearning_amd import _hip
    return _hip.Incres(P.indptr, P.indices, P.data, k)


def fit_on_device(W, k, seed, **params):
    """incres_ref.fit with the device in the numpy step's place: the restatement's draws, the device's labels fed back"""
    np.random.seed(seed)
    with device(ref.transition(W), k) as dev:
        return ref.fit(W, k, stepper=lambda seeds: dev.step(seeds), **params)


def random_steps(W, k, count=3, seed=0):
    """`count` outer iterations on one handle from seeds of its own making (m = 1, 2, ..): the device against the restatement"""
    n = W.shape[0]
    rng = np.random.default_rng(seed + 31 * n + k)
    P = ref.transition(W)
    with device(P, k) as dev:
        for m in range(1, count + 1):
            seeds = rng.integers(0, n, (k, m))
            want, sweeps, _ = ref.step(P, k, seeds)
            labels, got = dev.step(seeds)
            assert got == sweeps, (n, k, m, got, sweeps)
            assert labels.dtype == np.int32 and np.array_equal(labels, want), (n, k, m, int((labels != want).sum()))


@pytest.mark.parametrize('name', list(ref.GOLDEN_CASES))
def test_golden_labels_and_sweep_counts(gl, gold, name, capsys):
    g, k, seed, params = ref.GOLDEN_CASES[name]
    W = ref.golden_graph(gold, g)
    want, counts = gold['case_%s_labels' % name], gold['case_%s_sweeps' % name]
    np.random.seed(seed)
    model = gl.clustering.incres(W, k, **params)
    got = model.fit_predict()
    print(name, 'vertices that differ', int((got != want[-1]).sum()), 'sweeps', model.grow_sweeps[:5], model.incres_plan)
    assert got.dtype == np.int64 and np.array_equal(got, want[-1])
    assert model.grow_sweeps == [int(s) for s in counts]
    plan = model.incres_plan
    assert plan['loops'] == len(counts) and plan['counted'] == int(counts.sum()) and plan['enqueued'] >= plan['counted']
    if name == ref.LINES_CASE:
        capsys.readouterr()
        np.random.seed(seed)
        again = gl.clustering.incres(W, k, **params).fit_predict(all_labels=gold['graph_%s_truth' % g])
        assert capsys.readouterr().out.splitlines() == [str(s) for s in gold['case_%s_lines' % name]]
        assert np.array_equal(again, got)


@pytest.mark.parametrize('name', ['blobs3_fast', 'moons2'])
def test_labels_after_every_outer_iteration(gl, gold, name):
    g, k, seed, params = ref.GOLDEN_CASES[name]
    params = dict(params, T=min(params.get('T', 200), 40))
    W = ref.golden_graph(gold, g)
    hist, counts, _ = fit_on_device(W, k, seed, **params)
    np.random.seed(seed)
    want, want_counts, _ = ref.fit(W, k, **params)
    assert np.array_equal(hist, want) and np.array_equal(counts, want_counts)
    assert np.array_equal(hist, gold['case_%s_labels' % name][:params['T']])


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 255, 256, 257])
def test_vertex_counts(gl, n):
    W = ref.ring_graph(n)
    for k in sorted({1, min(3, n), min(5, n)}):
        random_steps(W, k)
    # and the public class from numpy's stream (T = 3)
    k = min(2, n)
    seed = next(s for s in range(n, n + 50) if _fits(W, k, s, T=3))
    np.random.seed(seed)
    want, counts, _ = ref.fit(W, k, T=3)
    np.random.seed(seed)
    model = gl.clustering.incres(W, k, T=3)
    assert np.array_equal(model.fit_predict(), want[-1]) and model.grow_sweeps == list(counts)


@pytest.mark.parametrize('k', [1, 2, 3, 4, 5, 8, 9, 33, 256])
def test_cluster_counts(gl, k):
    """the padding columns (k = 1, 2, 3, 5, 9, 33: zeros up to a multiple of 4) must not count as zeros of the iterate, and every
    lanes-per-record form of the census runs (4, 8, 16, 64)"""
    random_steps(ref.ring_graph(300, seed=k), k)


def test_more_clusters_than_the_records_hold_are_refused(gl):
    from graphlearning_amd import _hip
    W = ref.ring_graph(300)
    with pytest.raises(ValueError, match='257'):
        gl.clustering.incres(W, 257)
    P = ref.transition(W)
    for k in (0, 257):
        with pytest.raises(_hip.GlxError, match='clusters outside'):
            _hip.Incres(P.indptr, P.indices, P.data, k)
    with device(P, 2) as dev:
        for seeds in ([[0, 300], [1, 2]], [[-1], [0]]):
            with pytest.raises(_hip.GlxError, match='seed'):
                dev.step(np.array(seeds))
        labels, sweeps = dev.step(np.array([[0], [150]]))          # usable afterwards
        want = ref.step(P, 2, [[0], [150]])
        assert sweeps == want[1] and np.array_equal(labels, want[0])


def test_more_seeds_than_a_cluster_has_members(gl):
    """speed = 5000 on 12 vertices: m = 1, 4, 7, 10 seeds drawn with replacement from clusters of about 6"""
    W = ref.ring_graph(12)
    seed = next(s for s in range(50) if _fits(W, 2, s, speed=5000, T=4))
    np.random.seed(seed)
    want, counts, planted = ref.fit(W, 2, speed=5000, T=4)
    assert [p.shape[1] for p in planted] == [1, 4, 7, 10] and any(len(set(row)) < len(row) for p in planted for row in p)
    np.random.seed(seed)
    model = gl.clustering.incres(W, 2, speed=5000, T=4)
    assert np.array_equal(model.fit_predict(), want[-1]) and model.grow_sweeps == list(counts)
    hist, got, _ = fit_on_device(W, 2, seed, speed=5000, T=4)
    assert np.array_equal(hist, want) and np.array_equal(got, counts)


def _fits(W, k, seed, **params):
    """does the restatement get through without an empty cluster?"""
    np.random.seed(seed)
    try:
        ref.fit(W, k, **params)
    except ValueError:
        return False
    return True


def test_rows_of_one_and_of_300_entries(gl):
    W = ref.star_graph(300)
    lengths = np.diff(ref.transition(W).indptr)
    assert lengths.max() == 300 and lengths.min() == 1
    for k in (1, 3, 10):
        random_steps(W, k, seed=7)


def test_the_renumbered_graph(gl):
    """from 4096 vertices on the operator is renumbered for locality: seeds go in and labels come out through the permutation"""
    W = ref.ring_graph(4100)
    with device(ref.transition(W), 3) as dev:
        assert dev.stats()['renumbered'] == 1
    random_steps(W, 3, count=2)
    random_steps(W, 10, count=1)


def test_the_long_path_ends_in_the_denormal_range(gl):
    P = ref.transition(ref.path_graph(665))
    want, sweeps, F = ref.step(P, 1, [[0]])
    assert 0 < F.min() < ref.DENORMAL_MIN_NORMAL               # first: the case is what it claims to be
    assert sweeps == 664 and not want.any()
    with device(P, 1) as dev:
        labels, got = dev.step(np.array([[0]]))
        print('sweeps', got, dev.stats())
        assert got == 664 and not labels.any()
        stats = dev.stats()
        assert stats['chunks'] > 10 and stats['enqueued'] >= 664


def test_several_chunks_per_outer_iteration(gl):
    W = ref.path_graph(300)
    seed = next(s for s in range(50) if _fits(W, 3, s, T=5))
    np.random.seed(seed)
    want, counts, _ = ref.fit(W, 3, T=5)
    assert counts.max() > 64
    np.random.seed(seed)
    model = gl.clustering.incres(W, 3, T=5)
    got = model.fit_predict()
    print('sweeps', model.grow_sweeps, model.incres_plan)
    assert np.array_equal(got, want[-1]) and model.grow_sweeps == list(counts)
    assert model.incres_plan['chunks'] > 2 * 5
    hist, got_counts, _ = fit_on_device(W, 3, seed, T=5)
    assert np.array_equal(hist, want) and np.array_equal(got_counts, counts)


def test_results_do_not_depend_on_the_chunk_length(gl, gold):
    from graphlearning_amd import _hip
    g, k, seed, params = ref.GOLDEN_CASES['moons2']
    params = dict(params, T=25)
    W = ref.golden_graph(gold, g)
    want, counts = gold['case_moons2_labels'][:25], gold['case_moons2_sweeps'][:25]
    chunks_read = {}
    for chunk in (1, 2, 7, None):
        with _hip.incres_options(chunk=chunk):
            np.random.seed(seed)
            model = gl.clustering.incres(W, k, **params)
            got = model.fit_predict()
            hist, got_counts, _ = fit_on_device(W, k, seed, **params)
        assert np.array_equal(got, want[-1]) and model.grow_sweeps == [int(s) for s in counts], chunk
        assert np.array_equal(hist, want) and np.array_equal(got_counts, counts), chunk
        chunks_read[chunk] = model.incres_plan['chunks']
    print('chunks read', chunks_read)
    assert chunks_read[1] == int(np.maximum(counts, 1).sum()) and chunks_read[1] > chunks_read[2] > chunks_read[7] >= chunks_read[None]


def test_the_cap_is_an_error_return_and_the_handle_survives(gl):
    from graphlearning_amd import _hip
    two = sparse.block_diag([ref.ring_graph(20), ref.ring_graph(23)]).tocsr()
    for W, rescue in ((two, [[0, 25]]), (ref.path_graph(40, loops=False), [[0, 1]])):
        P = ref.transition(W)
        assert ref.step(P, 1, [[0]], max_grow=50)[0] is None
        with device(P, 1) as dev:
            before = dev.stats()['enqueued']
            with pytest.raises(_hip.GlxError, match='disconnected.*bipartite.*underflow'):
                dev.step(np.array([[0]]), max_grow=50)
            assert dev.last_sweeps == 50 and dev.stats()['enqueued'] - before == 50          # exactly 50 sweeps, not one more
            want = ref.step(P, 1, rescue)                                                      # seeds on both sides: the loop ends
            labels, sweeps = dev.step(np.array(rescue))
            assert sweeps == want[1] and np.array_equal(labels, want[0])
        np.random.seed(0)
        model = gl.clustering.incres(W, 1, max_grow=50)
        with pytest.raises(gl.GlxError, match='max_grow = 50'):
            model.fit()
        assert not model.fitted and model.grow_sweeps == []
    # a loop of exactly max_grow sweeps succeeds
    P = ref.transition(ref.path_graph(30))
    with device(P, 1) as dev:
        labels, sweeps = dev.step(np.array([[0]]), max_grow=29)
        assert sweeps == 29 and not labels.any()
        with pytest.raises(_hip.GlxError):
            dev.step(np.array([[0]]), max_grow=28)
        assert dev.last_sweeps == 28


def test_the_same_labels_with_the_pool_off_and_poisoned(gl, gold):
    """every buffer is written before it is read: pooled blocks filled with 0x7f bytes when handed out, then no pool at all"""
    from graphlearning_amd import _hip
    g, k, seed, params = ref.GOLDEN_CASES['blobs3_fast']
    W = ref.golden_graph(gold, g)
    want, counts = gold['case_blobs3_fast_labels'], gold['case_blobs3_fast_sweeps']
    _hip.pool_set_poison(0x7f)
    _hip.pool_set_enabled(False)
    try:
        hist, got_counts, _ = fit_on_device(W, k, seed, **params)
        random_steps(ref.ring_graph(65), 5)
    finally:
        ablate = os.environ.get('GLX_TEST_ABLATE', '')
        session = [s for s in ablate.split(',') if s.startswith('poison')]      # (an ablation run's own fill)
        _hip.pool_set_poison(int(session[0][6:] or '255') if session else -1)
        _hip.pool_set_enabled('nopool' not in ablate)
    assert np.array_equal(hist, want) and np.array_equal(got_counts, counts)
    _hip.pool_set_poison(0xff)
    try:
        hist, got_counts, _ = fit_on_device(W, k, seed, **params)
    finally:
        _hip.pool_set_poison(int(session[0][6:] or '255') if session else -1)
    assert np.array_equal(hist, want) and np.array_equal(got_counts, counts)
