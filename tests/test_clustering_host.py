"""graphlearning_amd.clustering without a GPU: the metrics against the reference's recorded outputs, the refusals, the exported surface,
and clustering.incres end to end -- its draws, its bookkeeping, its printed lines -- with the host plan driver
(tests/incres_plan_host.cpp) in the device's place."""
import os
import sys
import numpy as np
import pytest
from scipy import sparse

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import incres_ref as ref  # noqa: E402
import graphlearning_amd as gl  # noqa: E402
from graphlearning_amd import _hip  # noqa: E402


@pytest.fixture(scope='module')
def gold():
    return ref.load_golden()


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return ref.build_host_lib(tmp_path_factory.mktemp('incres_host'))


@pytest.fixture
def host_device(lib, monkeypatch):
    """_hip.Incres replaced by the host plan driver: clustering.incres runs without a GPU"""
    class Fake(ref.HostIncres):
        def __init__(self, row_ptr, col, val, k, device=None):
            n = len(row_ptr) - 1
            super().__init__(lib, sparse.csr_matrix((val, col, row_ptr), shape=(n, n)), k)
            self.arrays = tuple(np.array(a) for a in (row_ptr, col, val))

        def step(self, seeds, max_grow=None, out=None):
            try:
                return super().step(seeds, max_grow)
            except RuntimeError as e:
                raise _hip.GlxError(str(e))

        def stats(self):
            return {'chunk_cap': 64}
    monkeypatch.setattr(_hip, 'Incres', Fake)
    return Fake


def test_metrics_equal_the_reference(gold):
    pred, true = gold['metric_pred'], gold['metric_true']
    assert gl.clustering.clustering_accuracy(pred, true) == float(gold['metric_accuracy'])
    p, each = gl.clustering.purity(pred, true)
    assert p == float(gold['metric_purity']) and np.array_equal(each, gold['metric_purity_each'])
    w, m = gl.clustering.withinss(gold['metric_x'])
    assert np.array_equal(np.array([w, m]), gold['metric_withinss'])
    np.random.seed(int(gold['metric_rp1d_seed']))
    twin = np.random.RandomState(int(gold['metric_rp1d_seed']))
    got = gl.clustering.RP1D(gold['metric_X'], int(gold['metric_rp1d_T']))
    assert got.dtype == np.float64 and np.array_equal(got, gold['metric_rp1d'])
    twin.rand(int(gold['metric_rp1d_T']), gold['metric_X'].shape[1])
    assert np.random.rand() == twin.rand()                        # T * d draws, no more
    # the inputs are left alone; a predicted label beyond the number of classes is never counted as an error (the reference gives 75.0 too)
    assert np.array_equal(true, ref.load_golden()['metric_true'])
    assert gl.clustering.clustering_accuracy(np.array([0, 1, 2, 2]), np.array([5, 5, 9, 9])) == 75.0


def test_refusals_are_value_errors():
    W = ref.ring_graph(12)
    for kw in ({'num_clusters': 0}, {'num_clusters': 257}, {'num_clusters': 2.0}, {'num_clusters': 2, 'T': 0}, {'num_clusters': 2, 'max_grow': 0},
               {'num_clusters': 2, 'max_grow': -3}):
        with pytest.raises(ValueError):
            gl.clustering.incres(W, **kw)
    lonely = sparse.block_diag([ref.ring_graph(5), sparse.csr_matrix((1, 1))]).tocsr()
    with pytest.raises(ValueError, match='degree 0'):
        gl.clustering.incres(lonely, 2)
    for bad in (-1.0, np.nan, np.inf):
        V = W.copy()
        V.data[3] = bad
        with pytest.raises(ValueError, match='negative or not finite'):
            gl.clustering.incres(V, 2)
    # a parameter spoilt after the construction is caught by fit, before anything is drawn
    model = gl.clustering.incres(W, 2)
    model.T = 0
    np.random.seed(1)
    before = np.random.get_state()[1].copy()
    with pytest.raises(ValueError):
        model.fit()
    assert np.array_equal(np.random.get_state()[1], before) and not model.fitted
    assert gl.clustering.incres(W, 256).num_clusters == 256       # the cap itself is legal


def test_exports():
    assert gl.clustering.incres.__mro__[1] is gl.clustering.clustering
    for name in ('clustering', 'incres', 'clustering_accuracy', 'purity', 'withinss', 'RP1D'):
        assert hasattr(gl.clustering, name), name
    assert not hasattr(gl.clustering, 'spectral') and not hasattr(gl.clustering, 'fokker_planck')
    lib = _hip.load()
    for sym in ('glx_incres_create', 'glx_incres_step', 'glx_incres_destroy', 'glx_incres_stats', 'glx_incres_set_options'):
        assert getattr(lib, sym) is not None and sym in _hip.EXPORTED_SYMBOLS, sym
    hdr = open(os.path.join(ref.ROOT, 'include', 'glx_experimental.h')).read()
    assert all(('int %s(' % sym) in hdr for sym in ('glx_incres_create', 'glx_incres_step', 'glx_incres_destroy'))
    assert 'hip/hip_runtime.h' not in open(os.path.join(ref.ROOT, 'graphlearning_amd', 'csrc', 'incres_plan.h')).read()


def test_base_class_interface():
    class constant(gl.clustering.clustering):
        def _fit(self, all_labels=None):
            return np.zeros(self.graph.num_nodes, dtype=int)
    W = ref.ring_graph(9)
    model = constant(W, 4)
    assert model.cluster_labels is None and model.fitted is False and model.num_clusters == 4 and type(model.graph) == gl.graph
    with pytest.raises(SystemExit):
        model.predict()
    assert np.array_equal(model.fit(), np.zeros(9)) and model.fitted and model.predict() is model.cluster_labels
    assert constant(gl.graph(W), 2).fit_predict(all_labels=np.arange(9)).shape == (9,)
    with pytest.raises(NotImplementedError):
        gl.clustering.clustering(W, 2).fit()


@pytest.mark.parametrize('name', ['blobs3_fast', 'moons2'])
def test_incres_draws_and_bookkeeping_with_the_host_driver(gold, host_device, name, capsys):
    g, k, seed, params = ref.GOLDEN_CASES[name]
    W = ref.golden_graph(gold, g)
    n = W.shape[0]
    params = dict(params, T=min(params.get('T', 200), 30))
    want, counts = gold['case_%s_labels' % name], gold['case_%s_sweeps' % name]
    np.random.seed(seed)
    model = gl.clustering.incres(W, k, **params)
    got = model.fit_predict()
    assert got.dtype == np.int64 and np.array_equal(got, want[params['T'] - 1]) and got is model.cluster_labels and model.fitted
    assert model.grow_sweeps == [int(s) for s in counts[:params['T']]]
    assert model.incres_plan['max_grow'] == 2 * n + 2 and model.incres_plan['seed_step'] == max(int(params.get('speed', 5) * 1e-4 * n / k), 1)
    # the stream moved on exactly as the restatement's does
    after = np.random.rand()
    np.random.seed(seed)
    ref.fit(W, k, **params)
    assert after == np.random.rand()
    if name == ref.LINES_CASE:
        capsys.readouterr()
        np.random.seed(seed)
        again = gl.clustering.incres(W, k, **params).fit_predict(all_labels=gold['graph_%s_truth' % g])
        assert capsys.readouterr().out.splitlines() == [str(s) for s in gold['case_%s_lines' % name][:params['T']]]
        assert np.array_equal(again, got)


def test_p_goes_to_the_device_unsorted(gold, host_device, monkeypatch):
    seen = {}
    real = host_device.__init__

    def spy(self, row_ptr, col, val, k, device=None):
        seen['arrays'] = (np.array(row_ptr), np.array(col), np.array(val))
        real(self, row_ptr, col, val, k, device)
    monkeypatch.setattr(host_device, '__init__', spy)
    W = ref.golden_graph(gold, 'blobs')
    np.random.seed(0)
    gl.clustering.incres(W, 3, T=1).fit()
    P = ref.transition(W)
    for a, b in zip(seen['arrays'], (P.indptr, P.indices, P.data)):
        assert np.array_equal(a, b)
    assert not P.has_sorted_indices


def test_an_empty_cluster_is_numpys_own_error(host_device):
    W = ref.ring_graph(4)
    np.random.seed(0)
    with pytest.raises(ValueError, match='a must be greater than 0'):
        gl.clustering.incres(W, 200, T=1).fit()


def test_the_cap_is_a_glx_error(host_device):
    W = ref.path_graph(40, loops=False)
    np.random.seed(0)
    model = gl.clustering.incres(W, 1, max_grow=50)
    with pytest.raises(gl.GlxError, match='50 sweeps'):
        model.fit()
    assert not model.fitted and model.grow_sweeps == []


def test_member_lists_from_one_counting_sort():
    """_hip.host_group_by_label: the members of every cluster in ascending vertex order, as `J[u == r]` gives them"""
    rng = np.random.default_rng(4)
    for n, k in ((1, 1), (17, 3), (1000, 256), (5000, 10)):
        u = rng.integers(0, k, n)
        u[u == k // 2] = 0                                      # an empty cluster in the middle (k > 1)
        counts, order = _hip.host_group_by_label(u, k)
        assert counts.dtype == np.int64 and order.dtype == np.int32 and np.array_equal(counts, np.bincount(u, minlength=k))
        ends = np.cumsum(counts)
        for r in range(k):
            assert np.array_equal(order[ends[r] - counts[r]:ends[r]], np.flatnonzero(u == r))
    for bad in (-1, 3):
        with pytest.raises(_hip.GlxError, match='outside'):
            _hip.host_group_by_label(np.array([0, bad, 1]), 3)
