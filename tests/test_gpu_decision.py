"""The label decision on the device (csrc/project.hip: ssl.predict and ssl.volume_label_projection) against the numpy restatement
tests/decision_ref.py, through its three entry points -- the one-shot _hip.argmax_project, Sweep.project on the device-resident
state, SweepGroups.project on one column group -- and through the learners.  The path claims bit-identity, so every comparison is
exact: labels and class weights with np.array_equal (NaN weights in the same places), err and the step count with ==.
tests/decision_cases.py builds the inputs; tests/test_decision_host.py pins, without a GPU, how the reference run of each ends."""
import os
import sys

import numpy as np
import pytest
from scipy import sparse
from conftest import blobs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decision_ref as ref  # noqa: E402
import decision_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu
DT = sorted(dc.DTYPES)


@pytest.fixture(scope='module')
def gl():
    import graphlearning_amd as gl
    from graphlearning_amd import _hip
    _hip.require_device()
    return gl


@pytest.fixture(scope='module')
def orc():
    from oracle import gl_oracle
    return gl_oracle


def assert_same(got, want, what):
    """(labels, weights, err, steps) of the device against the restatement's."""
    print(what, 'steps', got[3], want[3], 'err', got[2], want[2])
    assert got[3] == want[3], (what, 'steps', got[3], want[3])
    assert got[2] == want[2] or (got[2] != got[2] and want[2] != want[2]), (what, 'err', got[2], want[2])
    assert np.array_equal(got[1], want[1], equal_nan=True), (what, 'weights', got[1], want[1])
    assert got[0].dtype == np.int64 and np.array_equal(got[0], want[0]), (what, 'labels', int(np.sum(got[0] != want[0])))


def one_shot(c, max_steps=None):
    from graphlearning_amd import _hip
    w = None if type(c['weights']) == int else c['weights']
    return _hip.argmax_project(c['prob'], c['priors'], w, max_steps=c['max_steps'] if max_steps is None else max_steps,
                               similarity=c['similarity'])


def some_weights(C):
    return 1 + 0.05 * ((np.arange(C) * 7) % 11)


# ---- a, b, c (first looks), d, e, f: the one-shot entry point ----------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('name', sorted(dc.CASES))
def test_one_shot_equals_restatement(gl, name, dtype):
    """Class counts 1 .. 4096 (three loops of the histogram kernel exist only for C > 256), row counts from 1 to above 2048 * 256,
    decisions of the first host look, argmin with priors, exact ties, degenerate input: the projection, and the plain decision
    under non-unit weights."""
    c, want = dc.case_and_ref(name, dtype)
    assert_same(one_shot(c), want, (name, dtype))
    C = c['prob'].shape[1]
    w = some_weights(C)
    with np.errstate(all='ignore'):
        lab = ref.predict(c['prob'], w, c['similarity'])
    got = one_shot(dict(c, weights=w), max_steps=0)
    assert_same(got, (lab, w, 1.0, 0), (name, dtype, 'plain'))


def test_one_shot_refuses_more_than_4096_classes(gl):
    from graphlearning_amd import _hip
    with pytest.raises(_hip.GlxError):
        _hip.argmax_project(np.zeros((3, 4097)), None, None, max_steps=0)
    with pytest.raises(_hip.GlxError):
        _hip.argmax_project(np.zeros((3, 4097), dtype=np.float32), np.full(4097, 1 / 4097), None, max_steps=5)


# ---- c: the step cap on and beside every host look -----------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('which', ['never', 'conv'])
def test_step_cap(gl, which, dtype):
    """The host looks at the device's `done` flag after 2, 6, 14, 30, 62, 94 ... steps and the first look carries the final
    decision: a cap on a look, one past it, and far away, on an input only the cap stops and on one that stops by itself."""
    for cap in dc.CAPS:
        c, want = dc.cap_case_and_ref(which, cap, dtype)
        got = one_shot(c)
        if which == 'never':
            assert got[3] == cap
        assert_same(got, want, (which, cap, dtype))


# ---- g: the cached per-device buffers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DT)
def test_buffers_reused_across_shapes(gl, dtype):
    """Shrinking and growing n, changing C, in one process: the buffers keep their capacity only while C stays the same."""
    for pos in range(len(dc.REUSE)):
        c, want = dc.reuse_case_and_ref(pos, dtype)
        assert_same(one_shot(c), want, (dc.REUSE[pos], dtype))


# ---- h: the device-resident state --------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def knn_operator(gl):
    """P = D^-1 W^T of a kNN graph of blobs (what ssl.poisson sweeps with), large enough (4096 vertices and more) for the library
    to renumber its vertices."""
    X, labels = blobs(4200, 6, 4, 5, 1.5)
    W = gl.weightmatrix.knn(X, 8)
    n = W.shape[0]
    deg = W * np.ones(n)
    P = sparse.csr_matrix(sparse.spdiags(deg ** (-1), 0, n, n).tocsr() * W.transpose())
    return P, deg


def resident_prob(n, C, dtype):
    return dc.draw(n, C, 80 + C).astype(dc.DTYPES[dtype])


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('C', [1, 3, 4, 5, 61, 256])
def test_resident_state_equals_restatement(gl, knn_operator, C, dtype):
    """Sweep.project on a state kept in vertex records of a renumbered operator, up to the widest record without a stop column
    (C = 256): the projection, the plain decision, and the one-hot state it leaves behind."""
    from graphlearning_amd import _hip
    P, _ = knn_operator
    n = P.shape[0]
    prob = resident_prob(n, C, dtype)
    priors = dc.priors_for(C, 80 + C)
    cap = 10000 if C == 1 else 70
    G = _hip.DeviceGraph(P, dtype=dc.DTYPES[dtype])
    S = _hip.Sweep(G, C, min_iter=0, max_iter=0, use_hipgraph=False)
    assert not np.array_equal(G.order(), np.arange(n))
    S.set_state(prob, None)
    state = np.array(S.fetch())
    assert state.dtype == prob.dtype and np.array_equal(state, prob)
    want = ref.volume_label_projection(state, priors, 1, True, cap)
    assert want[3] == 1 if C == 1 else 14 < want[3] <= cap             # past the third host look
    assert_same(S.project(priors, None, max_steps=cap), want, (C, dtype))
    assert np.array_equal(S.fetch(), prob)                                   # a decision alone leaves the state as it was
    w = some_weights(C)
    assert_same(S.project(None, w, max_steps=0, similarity=False), (ref.predict(state, w, False), w, 1.0, 0), (C, dtype, 'argmin'))
    none, w2, _, _ = S.project(None, w, max_steps=0, want_labels=False)
    assert none is None and np.array_equal(w2, w)
    assert_same(S.project(priors, w, max_steps=7, to_onehot=True), ref.volume_label_projection(state, priors, w, True, 7), (C, dtype, 'onehot'))
    onehot = S.fetch()
    assert onehot.dtype == prob.dtype
    assert np.array_equal(onehot, np.eye(C, dtype=prob.dtype)[ref.volume_label_projection(state, priors, w, True, 7)[0]])
    S.close(); G.close()


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('C', [5, 61])
def test_resident_decision_then_sweeps(gl, knn_operator, C, dtype):
    """then_iterate = 3 with a zero bias, as PoissonMBO hands its next heat sweeps to the device with the thresholding: the
    state becomes three sweeps u <- P u of onehot(labels)."""
    from graphlearning_amd import _hip
    P, _ = knn_operator
    n = P.shape[0]
    prob = resident_prob(n, C, dtype)
    priors = dc.priors_for(C, 80 + C)
    G = _hip.DeviceGraph(P, dtype=dc.DTYPES[dtype])
    S = _hip.Sweep(G, C, min_iter=0, max_iter=0, use_hipgraph=True)
    S.set_state(prob, None)
    want = ref.volume_label_projection(prob, priors, 1, True, 40)
    assert_same(S.project(priors, None, max_steps=40, to_onehot=True, then_iterate=3), want, (C, dtype))
    u = np.eye(C, dtype=prob.dtype)[want[0]]
    A = sparse.csr_matrix((P.data.astype(prob.dtype), P.indices, P.indptr), shape=P.shape)     # the stored entry order is the order of the sums
    for _ in range(3):
        u = A * u
    got = S.fetch()
    assert got.dtype == prob.dtype and np.array_equal(got, u)
    S.close(); G.close()


@pytest.mark.parametrize('dtype', DT)
def test_resident_state_with_stop_column(gl, knn_operator, dtype):
    """The widest record with a stop column (C = 252): the iterate of a short Poisson sweep, decided with priors where it lies."""
    from graphlearning_amd import _hip
    P, deg = knn_operator
    n, C = P.shape[0], 252
    rng = np.random.default_rng(91)
    Db = (rng.normal(size=(n, C)) * (rng.random((n, 1)) < 0.3)).astype(dc.DTYPES[dtype])
    v0 = np.zeros(n)
    v0[rng.choice(n, 50, replace=False)] = 1 / 50
    G = _hip.DeviceGraph(P, dtype=dc.DTYPES[dtype])
    S = _hip.Sweep(G, C, min_iter=4, max_iter=4, use_hipgraph=False)
    S.set_problem(Db, v0 / deg, deg, deg / np.sum(deg))
    T, _ = S.run()
    assert T == 4
    state = np.array(S.fetch())
    assert state.dtype == dc.DTYPES[dtype] and len(np.unique(state)) > n
    priors = dc.priors_for(C, 92)
    want = ref.volume_label_projection(state, priors, 1, True, 20)
    assert want[3] == 20
    assert_same(S.project(priors, None, max_steps=20), want, (C, dtype))
    assert np.array_equal(S.fetch(), state)
    S.close(); G.close()


def test_resident_record_limits(gl, knn_operator):
    from graphlearning_amd import _hip
    G = _hip.DeviceGraph(knn_operator[0])
    with pytest.raises(_hip.GlxError):
        _hip.Sweep(G, 253, min_iter=4, max_iter=4, use_hipgraph=False)
    with pytest.raises(_hip.GlxError):
        _hip.Sweep(G, 257, min_iter=0, max_iter=0, use_hipgraph=False)
    G.close()


# ---- i: stacked groups -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('C', [2, 10])
def test_stacked_groups_equal_restatement(gl, C, dtype):
    """Three training sets as column groups of one sweep (as ssl.poisson stacks its trials): every group's decision with its own
    priors, and a plain decision under non-unit weights, against the restatement on that group's fetched iterate."""
    from graphlearning_amd import _hip, utils
    X, labels = blobs(900, 8, C, 17 + C, 1.4)
    W = gl.weightmatrix.knn(X, 8)
    n = W.shape[0]
    model = gl.ssl.poisson(W, solver='gradient_descent', use_cuda=(dtype == 'f32'))
    dev, aux = model._operators()
    assert not aux['zero_degree']
    groups = _hip.SweepGroups(dev, C, 3, min_iter=5, max_iter=40)
    groups.set_vectors(aux['deg'], aux['vinf'])
    trials = [gl.trainsets.generate(labels, rate=1 + 2 * b, seed=b) for b in range(3)]
    for b, ti in enumerate(trials):
        onehot = utils.labels_to_onehot(labels[ti], C)
        Db_rows = aux['dinv'][ti, None] * (onehot - np.mean(onehot, axis=0))
        groups.set_problem_rows(b, ti, Db_rows, (1.0 / len(ti)) / aux['deg'][ti], 0.0)
    T, _ = groups.run()
    assert len(T) == 3 and all(5 <= t <= 40 for t in T)
    states = [np.array(groups.fetch(b)) for b in range(3)]
    assert all(s.dtype == dc.DTYPES[dtype] for s in states) and not np.array_equal(states[0], states[1])
    for b in (2, 0, 1):
        priors = dc.priors_for(C, 100 + b)
        want = ref.volume_label_projection(states[b], priors, 1, True, 60)
        assert_same(groups.project(b, priors, None, max_steps=60), want, (C, dtype, b))
        w = some_weights(C)
        assert_same(groups.project(b, None, w, max_steps=0), (ref.predict(states[b], w), w, 1.0, 0), (C, dtype, b, 'plain'))
        assert_same(groups.view(b).project(priors, w, max_steps=9, similarity=False),
                    ref.volume_label_projection(states[b], priors, w, False, 9), (C, dtype, b, 'argmin'))
    for b in range(3):
        assert np.array_equal(groups.fetch(b), states[b])
    groups.close()


# ---- j: the learners ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small_graph(gl):
    X, labels = blobs(600, 6, 3, 23, 1.2)
    W = gl.weightmatrix.knn(X, 8)
    ti = gl.trainsets.generate(labels, rate=4, seed=2)
    return W, labels, ti, gl.utils.class_priors(labels)


def model_refs(prob, priors, similarity):
    """The restatement's projection from unit weights, and the next one, which starts from the first's weights."""
    first = ref.volume_label_projection(prob, priors, 1, similarity)
    return first, ref.volume_label_projection(prob, priors, first[1], similarity)


def check_model(m, prob, resident, refs):
    """After fit: weights, error and labels of the projection from unit weights; predict() decides with those weights, twice the
    same; the next projection starts from them."""
    first, second = refs
    assert (m._device_state() is not None) == resident
    assert np.array_equal(m.weights, first[1]) and m.class_priors_error == first[2]
    for _ in range(2):
        assert np.array_equal(m.predict(), first[0])
        assert np.array_equal(m.predict(ignore_class_priors=True), ref.predict(prob, 1, m.similarity))
    assert np.array_equal(m.volume_label_projection(), second[0])
    assert np.array_equal(m.weights, second[1]) and m.class_priors_error == second[2]
    assert np.array_equal(m.predict(), second[0])
    assert (m._device_state() is not None) == resident


@pytest.mark.parametrize('dtype', DT)
def test_poisson_with_priors_resident_and_one_shot(gl, small_graph, dtype):
    W, labels, ti, priors = small_graph
    m = gl.ssl.poisson(W, class_priors=priors, solver='gradient_descent', use_cuda=(dtype == 'f32'))
    m.fit(ti, labels[ti])
    prob = np.array(m.prob)
    assert prob.dtype == dc.DTYPES[dtype]
    refs = model_refs(prob, m.class_priors, True)
    check_model(m, prob, True, refs)
    m.prob = m.prob.copy()                  # the result is the caller's array now: the one-shot entry point decides
    m.weights = 1
    m.volume_label_projection()
    check_model(m, prob, False, refs)


def test_graph_nearest_neighbor_with_priors(gl, small_graph):
    """One-vs-rest graph distances: a dissimilarity (argmin, dt = +0.1)."""
    W, labels, ti, priors = small_graph
    m = gl.ssl.graph_nearest_neighbor(W, class_priors=priors)
    m.fit(ti, labels[ti])
    assert m.similarity is False
    prob = np.array(m.prob)
    assert np.isfinite(prob).all() and prob.shape == (600, 3)
    refs = model_refs(prob, m.class_priors, False)
    check_model(m, prob, False, refs)
    m.prob = m.prob.copy()
    m.weights = 1
    m.volume_label_projection()
    check_model(m, prob, False, refs)
