"""ssl.multiclass_mbo and _hip.mmbo_solve on the device: the reference's golden labels on every vertex from the reference's own random
start (numpy's recorded state restored), with the device's eigen_decomp and with the stored eigenpairs; the device against
mmbo_host_reference (csrc/mmbo_plan.h on the host) BIT FOR BIT -- all T rows of labels and the last Z -- on seeded problems at the
shapes where the kernels can go wrong; the caps; repeatability with the pool on and off; the lines of an all_labels fit and ssl_trials'
file.

Every test runs under a time limit of its own: a test that exceeds it ends the whole session on the spot (traceback of every
thread, then exit), so nothing more is started on a device that may have hung; nothing is retried."""
import faulthandler
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eig_ref  # noqa: E402
import mmbo_ref as ref  # noqa: E402
from test_mmbo_host import golden_case  # noqa: E402

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


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return ref.build_host_lib(tmp_path_factory.mktemp('mmbo_plan'))


def solve(X, vals, lab0, ind, lab, k, **kw):
    from graphlearning_amd import _hip
    return _hip.mmbo_solve(X, vals, lab0, ind, lab, k, **kw)


def learner_kwargs(params):
    return {key: params[key] for key in ('Ns', 'T', 'dt', 'mu', 'num_eig')}


@pytest.mark.parametrize('name', sorted(ref.GOLDEN_CASES))
def test_golden_equal_on_every_vertex(gl, gold, name):
    W, truth, ind, labels, k, params, start = golden_case(gold, name)
    n = W.shape[0]
    want = gold['case_%s_prob_labels' % name]
    for stored in (False, True):
        graph = gl.graph(W)
        if stored:                          # the cache hit: no decomposition runs
            vals, X = ref.golden_eigenpairs(gold, name)
            graph.eigendata['normalized'].update(dict(method='exact', k=params['num_eig'], c=2 * params['num_eig'], gamma=0, tol=0, q=1,
                                                      eigenvalues=vals, eigenvectors=X))
        twin = np.random.RandomState()
        twin.set_state(ref.numpy_state(gold, name))
        np.random.set_state(ref.numpy_state(gold, name))
        model = gl.ssl.multiclass_mbo(graph, **learner_kwargs(params))
        prob = model.fit(ind, labels)
        twin.rand(k, n)
        assert np.random.rand() == twin.rand()                  # the fit consumed exactly one rand(k, n)
        got = np.argmax(prob, axis=1)
        print(name, 'stored eigenpairs' if stored else 'device eigen_decomp', 'rows that differ', int((got != want).sum()), 'plan', model.mmbo_plan)
        assert prob.shape == (n, k) and prob.dtype == np.float64 and np.array_equal(prob, ref.onehot(want, k))
        assert np.array_equal(model.predict(), gold['case_%s_pred' % name])
        assert model.num_iter == params['T'] * params['Ns']
        assert model.mmbo_plan[:6] == (2, 64, (n + 63) // 64, 4096, 256, 256) and model.mmbo_plan[6] == 2 * model.num_iter + 1
        assert (graph.eig_steps is None) == stored
        np.random.set_state(ref.numpy_state(gold, name))
        with_priors = gl.ssl.multiclass_mbo(graph, class_priors=gold['case_%s_priors' % name], **learner_kwargs(params))
        assert np.array_equal(with_priors.fit_predict(ind, labels), gold['case_%s_pred_priors' % name])
        assert np.array_equal(with_priors.prob, prob)


# seed, n, m, k, Ns, T, extras.  Rows per partial: 64.  n: 1, 2 (fewer rows than a partial), 63, 64, 65 (one partial exactly and one row
# over), 257, 1000 (no multiple of 64, several chains), 4097 (65 partials: a chain holds two).  m: 1, 2, 17, 50, 64, 65, 256.
# k: 1, 2, 3, 10, 17, 64, 256 (with m = 16).  k * m = 4096 exactly: (64, 64), (256, 16), (16, 256).  Ns = 1 (a projection after every
# step), T = 1 (none inside), both.  Rows of a partial held in LDS at a time (mmbo_sub_rows): 64 at small k * m, 32 at (4, 128), 16 at
# (8, 200), 8 at the cap.
SHAPES = [
    (0, 1, 1, 1, 1, 1, {}), (1, 2, 2, 2, 2, 2, {}), (2, 63, 17, 3, 3, 2, {}), (3, 64, 50, 10, 6, 2, {}), (4, 65, 64, 17, 2, 3, {}),
    (5, 257, 65, 3, 1, 4, {}), (6, 1000, 50, 10, 6, 3, {}), (7, 4097, 17, 10, 2, 2, {}), (8, 257, 64, 64, 2, 2, {}),
    (9, 257, 16, 256, 2, 2, {}), (10, 130, 256, 16, 3, 1, {}), (11, 1000, 256, 10, 2, 1, {}), (12, 65, 2, 1, 3, 2, {}),
    (13, 1000, 50, 10, 3, 2, dict(ntrain=1000)), (14, 1000, 50, 10, 3, 2, dict(ntrain=1)), (15, 257, 17, 5, 2, 3, dict(zero_column=True)),
    (16, 257, 17, 5, 2, 3, dict(empty_class=True)), (17, 1000, 17, 4, 2, 3, dict(tied_classes=True)), (18, 65, 1, 2, 1, 1, {}),
    (19, 130, 128, 4, 2, 2, {}), (20, 130, 200, 8, 2, 2, {}),
]


@pytest.mark.parametrize('seed,n,m,k,Ns,T,extra', SHAPES)
def test_seeded_shapes_bit_for_bit(gl, lib, seed, n, m, k, Ns, T, extra):
    X, vals, lab0, ind, lab = ref.random_problem(seed, n, m, k, **extra)
    want_hist, want_Z, gap = ref.host_solve(lib, X, vals, lab0, ind, lab, k, Ns=Ns, T=T, dt=0.15, mu=50.0)
    hist, Z, plan = solve(X, vals, lab0, ind, lab, k, Ns=Ns, T=T, dt=0.15, mu=50.0)
    print((n, m, k, Ns, T), 'labels that differ', int((hist != want_hist).sum()), 'values of Z that differ', int((Z != want_Z).sum()), 'gap', gap,
          'plan', plan)
    assert hist.dtype == np.int32 and eig_ref.same_bits(hist, want_hist) and eig_ref.same_bits(Z, want_Z)
    assert plan == (2, 64, (n + 63) // 64, 4096, 256, 256, 2 * T * Ns + 1)
    if extra.get('tied_classes'):            # classes 0 and 1 are never used: their u are equal (zero) everywhere, and 0 wins where they lead
        assert (want_hist[0] == 0).any() and not (want_hist[0] == 1).any()
    if extra.get('empty_class'):
        assert not (lab0 == k - 1).any()
    if extra.get('zero_column'):
        assert not X[:, m // 2].any()


def test_above_the_cap_is_refused_and_touches_nothing(gl):
    from graphlearning_amd import _hip
    for m, k in [(241, 17), (65, 64), (16, 257), (257, 16)]:
        X, vals, lab0, ind, lab = ref.random_problem(1, 1100, m, k)          # (an X of 128 KiB or more would go up as a checked upload)
        before = _hip.debug_counters()
        with pytest.raises(_hip.GlxError, match=r'glx_mmbo_solve failed \(-4\)'):
            solve(X, vals, lab0, ind, lab, k)
        assert _hip.debug_counters() == before
    X, vals, lab0, ind, lab = ref.random_problem(1, 70, 3, 2)
    with pytest.raises(_hip.GlxError, match=r'failed \(-1\).*start label'):
        solve(X, vals, np.full(70, 2, dtype=np.int32), ind, lab, 2)


def test_the_same_bits_twice_and_without_the_pool(gl, lib):
    from graphlearning_amd import _hip
    X, vals, lab0, ind, lab = ref.random_problem(6, 1000, 50, 10)
    want = ref.host_solve(lib, X, vals, lab0, ind, lab, 10, Ns=6, T=3, dt=0.15, mu=50.0)
    a = solve(X, vals, lab0, ind, lab, 10, Ns=6, T=3)
    b = solve(X, vals, lab0, ind, lab, 10, Ns=6, T=3)
    _hip.pool_set_enabled(False)
    try:
        c = solve(X, vals, lab0, ind, lab, 10, Ns=6, T=3)
    finally:
        _hip.pool_set_enabled(True)
    for got in (a, b, c):
        assert eig_ref.same_bits(got[0], want[0]) and eig_ref.same_bits(got[1], want[1])


@pytest.mark.parametrize('name', ref.LINES_CASES)
def test_all_labels_lines(gl, gold, capsys, name):
    W, truth, ind, labels, k, params, start = golden_case(gold, name)
    np.random.set_state(ref.numpy_state(gold, name))
    model = gl.ssl.multiclass_mbo(W, **learner_kwargs(params))
    capsys.readouterr()
    prob = model.fit(ind, labels, all_labels=truth)
    out = capsys.readouterr().out.splitlines()
    assert out == [str(s) for s in gold['case_%s_lines' % name]]
    assert np.array_equal(np.argmax(prob, axis=1), gold['case_%s_prob_labels' % name])


def test_ssl_trials_writes_the_reference_format_and_decomposes_once(gl, gold, tmp_path, monkeypatch):
    name = 'blobs_s0'
    W, truth, ind, labels, k, params, start = golden_case(gold, name)
    rng = np.random.default_rng(3)
    other = np.concatenate([rng.choice(np.where(truth == c)[0], size=2, replace=False) for c in range(k)])
    monkeypatch.setattr(gl.ssl, 'results_dir', str(tmp_path / 'results'))
    model = gl.ssl.multiclass_mbo(W)
    np.random.seed(11)
    model.fit(other, truth[other])
    steps, vecs = model.graph.eig_steps, model.graph.eigendata['normalized']['eigenvectors']
    assert steps is not None and steps > 0
    model.graph.eig_steps = -1                                   # a second decomposition would overwrite it
    np.random.seed(11)
    model.ssl_trials([other, ind], truth, tag='mmbo_')
    assert model.graph.eig_steps == -1 and model.graph.eigendata['normalized']['eigenvectors'] is vecs
    path = tmp_path / 'results' / 'mmbo__multiclass_mbo_Ns_6_T_10_dt_0.150_mu_50.00_accuracy.csv'
    lines = path.read_text().splitlines()
    assert lines[0] == 'Number of labels,Accuracy' and len(lines) == 3
    counts = [int(s.split(',')[0]) for s in lines[1:]]
    assert counts == [len(other), len(ind)]
    np.random.seed(11)
    again = gl.ssl.multiclass_mbo(model.graph)
    acc0 = gl.ssl.ssl_accuracy(again.fit_predict(other, truth[other]), truth, other)
    acc1 = gl.ssl.ssl_accuracy(again.fit_predict(ind, labels), truth, ind)
    assert lines[1] == '%d,%.2f' % (len(other), acc0) and lines[2] == '%d,%.2f' % (len(ind), acc1)
    assert model.trials_statistics(tag='mmbo_')[0].tolist() == sorted(counts)
