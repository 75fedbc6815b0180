"""ssl.sparse_label_propagation and _hip.slp_iterate on the device: the reference's golden vectors bit for bit, seeded problems and
hub rows against the numpy restatement, repeatability, the iterate history against shorter calls (the seam between replayed chunks and
eagerly enqueued iterations), the learner's predictions and printed lines against the fixtures, and one case with the buffer pool off.

Every test runs under a time limit of its own: a test that exceeds it ends the whole session on the spot (traceback of every
thread, then exit), so nothing more is started on a device that may have hung; nothing is retried."""
import faulthandler
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slp_ref as ref  # noqa: E402
from test_slp_host import load_golden, golden_graph, golden_case, same_bits  # noqa: E402

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
def blobs_history(gold):
    """The numpy restatement's iterates of the `blobs` case (T = 100), computed once."""
    W, ind, labels, k, T, prob = golden_case(gold, 'blobs')
    u, hist = ref.slp_numpy(W, ind, labels, T, history=True)
    assert same_bits(u, prob)
    return hist


def device_iterate(W, ind, labels, k, T, want_history=False):
    from graphlearning_amd import _hip
    indptr, indices, w, lam, gamma, _ = ref.setup(W)
    val = (np.asarray(labels)[:, None] == np.arange(k)[None, :]).astype(np.float64)
    return _hip.slp_iterate(indptr, indices, w, lam, gamma, np.asarray(ind, dtype=np.int32), val, T, want_history=want_history)


@pytest.mark.parametrize('name', sorted(ref.GOLDEN_CASES))
def test_golden_bit_for_bit(gl, gold, name):
    W, ind, labels, k, T, prob = golden_case(gold, name)
    model = gl.ssl.sparse_label_propagation(W, T=T)
    u = model.fit(ind, labels)
    print(name, 'differing values', int((u != prob).sum()), 'plan', model.slp_plan)
    assert same_bits(np.ascontiguousarray(u), prob)
    assert model.num_iter == T and model.slp_plan[0] == 2 and model.slp_plan[2] == (9 if k == 17 else k)
    assert model.slp_plan[1] == 2 * T * (2 if k > 16 else 1)
    assert np.array_equal(model.predict(), model.predict(ignore_class_priors=True))


@pytest.mark.parametrize('seed', range(6))
def test_seeded_problems_against_numpy_form(gl, seed):
    W, ind, labels, k, T = ref.random_problem(seed)
    want = ref.slp_numpy(W, ind, labels, T, k=k)
    u, _, plan = device_iterate(W, ind, labels, k, T)
    assert same_bits(u, want), (seed, int((u != want).sum()))
    if k == len(np.unique(labels)):
        assert same_bits(np.ascontiguousarray(gl.ssl.sparse_label_propagation(W, T=T).fit(ind, labels)), want)


@pytest.mark.parametrize('h', [63, 64, 65, 255, 256, 257])
def test_hub_rows_against_numpy_form(gl, h):
    W, ind, labels, k, T = ref.hub_problem(h)
    want = ref.slp_numpy(W, ind, labels, T, k=k)
    u, _, _ = device_iterate(W, ind, labels, k, T)
    assert same_bits(u, want), (h, int((u != want).sum()))


def test_two_calls_give_the_same_bits(gl, gold):
    W, ind, labels, k, T, prob = golden_case(gold, 'wide17')
    a = device_iterate(W, ind, labels, k, T)[0]
    b = device_iterate(W, ind, labels, k, T)[0]
    assert same_bits(a, b) and same_bits(a, prob)


def test_history_and_the_chunk_seam(gl, gold, blobs_history):
    """T = 100 is six replayed chunks of 16 iterations and four eager ones; u_hist[t] must be what a call of T = t + 1 returns:
    t = 15 (one iteration short of a replay: all eager), 31 (the first T that replays), 32 (a replay, a replay, one eager)."""
    W, ind, labels, k, T, prob = golden_case(gold, 'blobs')
    u, hist, plan = device_iterate(W, ind, labels, k, T, want_history=True)
    assert same_bits(u, prob) and hist.shape == (T, W.shape[0], k) and same_bits(np.ascontiguousarray(hist[-1]), u)
    assert same_bits(hist, blobs_history)
    for t in (15, 31, 32):
        assert same_bits(device_iterate(W, ind, labels, k, t + 1)[0], np.ascontiguousarray(hist[t])), t
    # the same with more columns than one tile
    W, ind, labels, k, T, prob = golden_case(gold, 'wide17')
    u, hist, _ = device_iterate(W, ind, labels, k, T, want_history=True)
    assert same_bits(u, prob) and same_bits(np.ascontiguousarray(hist[-1]), prob)
    assert same_bits(device_iterate(W, ind, labels, k, 33)[0], np.ascontiguousarray(hist[32]))


def test_learner_against_the_fixtures(gl, gold, capsys):
    W, ind, labels, k, T, prob = golden_case(gold, 'blobs')
    truth = gold['graph_blobs_truth']
    model = gl.ssl.sparse_label_propagation(W, T=100)
    assert np.array_equal(model.fit_predict(ind, labels), gold['learner_pred'])
    with_priors = gl.ssl.sparse_label_propagation(W, class_priors=gold['learner_priors'], T=100)
    assert np.array_equal(with_priors.fit_predict(ind, labels), gold['learner_pred_priors'])
    assert same_bits(np.ascontiguousarray(with_priors.prob), prob)
    capsys.readouterr()
    lines_model = gl.ssl.sparse_label_propagation(W, T=12)
    u = lines_model.fit(ind, labels, all_labels=truth)
    out = capsys.readouterr().out.splitlines()
    assert out == [str(s) for s in gold['learner_lines']]
    assert same_bits(np.ascontiguousarray(u), device_iterate(W, ind, labels, k, 12)[0]) and lines_model.num_iter == 12


def test_blobs_with_the_pool_off(gl, gold):
    from graphlearning_amd import _hip
    W, ind, labels, k, T, prob = golden_case(gold, 'blobs')
    _hip.pool_set_enabled(False)
    try:
        u = gl.ssl.sparse_label_propagation(W, T=T).fit(ind, labels)
    finally:
        _hip.pool_set_enabled(True)
    assert same_bits(np.ascontiguousarray(u), prob)
