"""graph.connected_components and graph.largest_connected_component on the device against scipy, EXACTLY: the component count and the
label of every vertex (dtype included) on every case of tests/components_cases.py, a second call giving the identical array, the
largest component's mask and restricted matrix against the reference's own scipy expression, the refusal of malformed raw arrays
as an error return that leaves the device usable, and one use through the package (a Poisson fit on the largest component).

Every test runs under a time limit of its own: a test that exceeds it ends the whole session on the spot (traceback of every thread,
then exit), so nothing more is started on a device that may have hung; nothing is retried."""
import faulthandler
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

GROUPS = ['random_n%d' % n for n in cases.RANDOM_N] + ['diameter', 'hubs', 'ties', 'package']


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
def by_group(gl):
    """group -> [(name, W, scipy's ncomp, scipy's labels)]: built and solved by scipy once, shared, never written to"""
    out = {}
    every = cases.host_cases() + cases.package_cases()
    for name, group, W in every:
        key = name[:name.index('_deg')] if group == 'random' else group
        ncomp, labels = cases.scipy_components(W)
        labels.setflags(write=False)
        out.setdefault(key, []).append((name, W, ncomp, labels))
    assert sorted(out) == sorted(GROUPS)
    return out


@pytest.mark.parametrize('group', GROUPS)
def test_components_equal_scipy_on_every_vertex(gl, by_group, group):
    from graphlearning_amd import _hip
    for name, W, want_n, want in by_group[group]:
        G = gl.graph(W)
        ncomp, labels = G.connected_components()
        assert isinstance(ncomp, int) and labels.dtype == want.dtype == np.int32 and labels.shape == want.shape, name
        assert ncomp == want_n and np.array_equal(labels, want), name
        assert len(_hip.components_last_ms) == 4 and all(t >= 0 for t in _hip.components_last_ms)
        again_n, again = G.connected_components()
        assert again_n == ncomp and np.array_equal(again, labels), name


def test_both_row_classes_ran(gl, by_group):
    """the plan the library reports: rows at and above the threshold took a wavefront, the row one entry shorter did not"""
    from graphlearning_amd import _hip
    T = cases.wave_row_threshold()
    assert _hip.components_plan()[:2] == (T, T)
    took = {}
    for name, W, _, _ in by_group['hubs']:
        gl.graph(W).connected_components()
        took[name] = _hip.components_plan()[3]
        assert took[name] == int((np.diff(W.indptr) >= T).sum()), name
    assert took['rows_of_%d_entries' % (T - 1)] == 0 and took['rows_of_%d_entries' % T] == 3 == took['rows_of_%d_entries' % (T + 1)]
    assert took['star_5000_hub_first'] == took['star_5000_hub_last'] == 1


def test_the_labels_do_not_depend_on_the_row_classes(gl, by_group):
    """every row a wavefront (threshold 1) and every row a thread (threshold 2^30): the same labels"""
    from graphlearning_amd import _hip
    try:
        for threshold in (1, 1 << 30):
            _hip.components_set_wave_row(threshold)
            for group in ('random_n4097', 'hubs', 'ties'):
                for name, W, want_n, want in by_group[group]:
                    ncomp, labels = gl.graph(W).connected_components()
                    assert ncomp == want_n and np.array_equal(labels, want), (name, threshold)
    finally:
        _hip.components_set_wave_row(0)


@pytest.mark.parametrize('group', [g for g in GROUPS if g not in ('diameter', 'hubs')])
def test_largest_component_equals_the_reference_expression(gl, by_group, group):
    for name, W, want_n, want in by_group[group]:
        ind_want = want == np.argmax(np.bincount(want, minlength=want_n))
        A = W[ind_want, :][:, ind_want]
        G, ind = gl.graph(W).largest_connected_component()
        assert ind.dtype == np.bool_ and np.array_equal(ind, ind_want), name
        B = G.weight_matrix
        assert isinstance(G, gl.graph) and G.num_nodes == int(ind_want.sum()) and B.shape == A.shape, name
        assert np.array_equal(B.indptr, A.indptr) and np.array_equal(B.indices, A.indices), name
        assert B.data.dtype == A.data.dtype and np.array_equal(B.data.view(np.uint64), A.data.view(np.uint64)), name


def test_the_first_maximum_wins_a_tie(gl, by_group):
    got = {name: gl.graph(W).largest_connected_component()[1] for name, W, _, _ in by_group['ties']}
    assert np.flatnonzero(got['tie_two_halves']).tolist() == list(range(40))
    assert np.flatnonzero(got['tie_interleaved']).tolist() == list(range(0, 80, 2))
    assert np.flatnonzero(got['tie_behind_a_single_vertex']).tolist() == list(range(1, 41))
    assert np.flatnonzero(got['all_isolated']).tolist() == [0]


def test_package_graphs_have_the_components_they_were_built_with(gl, by_group):
    found = {name: (ncomp, labels) for name, _, ncomp, labels in by_group['package']}
    for name in ('blobs_knn5', 'blobs_knn5_unsymmetrized'):
        ncomp, labels = found[name]
        assert ncomp == 3 and np.bincount(labels).tolist() == [300, 200, 100]
    ncomp, labels = found['epsilon_ball_with_isolated_points']
    sizes = np.bincount(labels)
    assert (sizes == 1).any() and sizes.max() > 1


@pytest.mark.parametrize('what, indptr, indices', [
    ('a column index equal to n', [0, 2, 3, 4, 4], [1, 2, 4, 0]),
    ('a column index of -1', [0, 2, 3, 4, 4], [1, -1, 2, 0]),
    ('row pointers that decrease', [0, 3, 2, 4, 4], [1, 2, 0, 3]),
    ('a last row pointer that is not the number of entries', [0, 2, 3, 3, 3], [1, 2, 0, 3]),
])
def test_malformed_raw_arrays_are_refused_and_the_device_stays_usable(gl, what, indptr, indices):
    """stopped by the checks (host: row pointers; device pass: column indices) before a kernel follows an index"""
    from graphlearning_amd import _hip
    with pytest.raises(_hip.GlxError, match='glx_components'):
        _hip.components(np.array(indptr, dtype=np.int32), np.array(indices, dtype=np.int32), 4)
    ncomp, labels = _hip.components(np.array([0, 2, 3, 4, 4], dtype=np.int32), np.array([1, 2, 3, 0], dtype=np.int32), 4)
    assert ncomp == 1 and labels.dtype == np.int32 and labels.tolist() == [0, 0, 0, 0]


def test_a_bad_index_deep_inside_a_large_array_is_found(gl, by_group):
    """the device pass looks at every entry: one index equal to n at the far end of the grid's 261 120 entries"""
    from graphlearning_amd import _hip
    name, W, want_n, want = by_group['diameter'][3]
    indices = W.indices.copy()
    indices[-3] = W.shape[0]
    with pytest.raises(_hip.GlxError, match='column index %d at entry %d ' % (W.shape[0], len(indices) - 3)):
        _hip.components(W.indptr, indices, W.shape[0])
    ncomp, labels = _hip.components(W.indptr, W.indices, W.shape[0])
    assert ncomp == want_n and np.array_equal(labels, want)


def test_poisson_learning_on_the_largest_component(gl, by_group):
    name, W, _, _ = by_group['package'][0]
    assert name == 'blobs_knn5'
    G, ind = gl.graph(W).largest_connected_component()
    assert int(ind.sum()) == 300 and G.num_nodes == 300
    y = (cases.three_blobs()[ind, 1] > 0).astype(np.int64)          # two classes inside the one blob
    train_ind = np.concatenate([np.flatnonzero(y == 0)[:5], np.flatnonzero(y == 1)[:5]])
    pred = gl.ssl.poisson(G.weight_matrix).fit_predict(train_ind, y[train_ind])
    assert pred.shape == (300,) and set(np.unique(pred)) <= {0, 1}
