"""utils.boundary_statistic on the device: every golden vector of the reference through the public function (nu bit for bit, T equal
as numbers; both modes, the three order settings, with and without knn_data), the device against the restatement
tests/boundary_ref.py bit for bit at the smallest shapes that can go wrong (tests/boundary_cases.py), the zero-normal error and the
call after it, repeatability and the return type."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_ref as ref  # noqa: E402
import boundary_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = {(False, True): 'o1', (True, True): 'o2c', (True, False): 'o2'}


@pytest.fixture(scope='module')
def gl():
    import graphlearning_amd as gl
    from graphlearning_amd import _hip
    _hip.require_device()
    return gl


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'g25_boundary.npz'))


@pytest.fixture(scope='module')
def device_cases():
    return cases.device_cases()


@pytest.mark.parametrize('name', sorted(cases.GOLDEN))
def test_golden_vectors_through_the_public_function(gl, gold, name):
    mode, n, d, r, seed = cases.GOLDEN[name]
    X = gold[name + '_X']
    handed = [None] + ([(gold[name + '_J'].astype(np.int64), gold[name + '_D'])] if mode == 'knn' else [])
    for knn_data in handed:
        for (second, cutoff), tag in TAGS.items():
            T, nu = gl.utils.boundary_statistic(X, r, knn=mode == 'knn', return_normals=True, second_order=second, cutoff=cutoff,
                                                knn_data=knn_data)
            assert T.shape == (n,) and nu.shape == (n, d) and T.dtype == nu.dtype == np.float64
            assert nu.tobytes() == gold['%s_nu_%s' % (name, tag)].tobytes(), (name, tag)
            assert np.array_equal(T, gold['%s_T_%s' % (name, tag)]), (name, tag)
            assert not np.signbit(T[T == 0]).any()
    if mode == 'knn':       # lists wider than k, as the reference uses them: the graph from k + 1 columns, the maximum over all
        Jw, Dw = ref.knn_lists(X, r + 5)
        want_T, want_nu = ref.statistic(X, *ref.knn_pattern(Jw, r + 1), J=Jw)
        T, nu = gl.utils.boundary_statistic(X, r, knn=True, return_normals=True, knn_data=(Jw, Dw))
        assert np.array_equal(T, gold[name + '_Twide']) and T.tobytes() == want_T.tobytes() and nu.tobytes() == want_nu.tobytes()


def test_device_equals_the_restatement_bit_for_bit(gl, device_cases):
    """the library call on every device case's pattern, the three order settings"""
    from graphlearning_amd import _hip
    wave_row, _ = cases.plan_constants()
    for name, c in device_cases.items():
        for second, cutoff in ref.ORDERS:
            want_T, want_nu = ref.statistic(c['X'], c['indptr'], c['indices'], J=c['J'], second_order=second, cutoff=cutoff)
            T, nu = _hip.boundary_stat(c['X'], c['indptr'], c['indices'], second_order=second, cutoff=cutoff, J=c['J'])
            assert nu.tobytes() == want_nu.tobytes(), (name, second, cutoff)
            assert T.tobytes() == want_T.tobytes(), (name, second, cutoff)
        launches, nshort, nwave, nfull = _hip.boundary_stat_last[:4]
        lens = np.diff(c['indptr']) if c['J'] is None else np.full(len(c['X']), c['J'].shape[1])
        assert nwave == (lens >= wave_row).sum() and nshort + nwave == len(c['X']), name
        assert launches == 4 + (nshort > 0) + (nwave > 0)
        assert nfull == (0 if c['J'] is not None else (lens == lens.max()).sum())
    assert np.isneginf(_hip.boundary_stat(*[device_cases['n2_radius'][q] for q in ('X', 'indptr', 'indices')])[0]).all()


def test_public_function_builds_the_same_graphs(gl, device_cases):
    """the public function on the device cases it can ask for: its own ball graph, its own search, and lists handed in"""
    for name, c in device_cases.items():
        if c['r'] is None:
            continue
        want_T, want_nu = ref.statistic(c['X'], c['indptr'], c['indices'], J=c['J'])
        if c['knn']:
            T, nu = gl.utils.boundary_statistic(c['X'], c['r'], knn=True, return_normals=True, knn_data=(c['J'], c['D']))
        else:
            T, nu = gl.utils.boundary_statistic(c['X'], c['r'], return_normals=True)
        assert nu.tobytes() == want_nu.tobytes() and T.tobytes() == want_T.tobytes(), name
    for name in ('n65_knn', 'd7_knn', 'd128_knn', 'd129_knn', 'k2', 'k61'):       # the device's own search: the same lists as sets, no ties here
        c = device_cases[name]
        want_T, want_nu = ref.statistic(c['X'], c['indptr'], c['indices'], J=c['J'], second_order=True, cutoff=False)
        T, nu = gl.utils.boundary_statistic(c['X'], c['r'], knn=True, return_normals=True, cutoff=False)
        assert nu.tobytes() == want_nu.tobytes() and T.tobytes() == want_T.tobytes(), name


def test_class_threshold_changes_no_result(gl, device_cases):
    from graphlearning_amd import _hip
    c = device_cases['lengths']
    want_T, want_nu = ref.statistic(c['X'], c['indptr'], c['indices'])
    try:
        for wave_row in (1, 64, 65, 4096):
            _hip.boundary_stat_set_wave_row(wave_row)
            T, nu = _hip.boundary_stat(c['X'], c['indptr'], c['indices'])
            assert T.tobytes() == want_T.tobytes() and nu.tobytes() == want_nu.tobytes(), wave_row
            assert _hip.boundary_stat_last[2] == (np.diff(c['indptr']) >= wave_row).sum()
    finally:
        _hip.boundary_stat_set_wave_row(0)


def test_zero_normal_is_an_error_and_the_device_stays_usable(gl, device_cases):
    from graphlearning_amd import _hip
    X = cases.lattice()
    with pytest.raises(_hip.GlxError, match='vertex 26 '):
        gl.utils.boundary_statistic(X, 1.5)
    with pytest.raises(_hip.GlxError, match='vertex 13 '):
        gl.utils.boundary_statistic(X, 1.5, second_order=False)
    Xd, J, D, first = cases.duplicates_knn()
    with pytest.raises(_hip.GlxError, match='vertex %d ' % first):
        gl.utils.boundary_statistic(Xd, J.shape[1], knn=True, second_order=False, knn_data=(J, D))
    c = device_cases['n65_radius']
    want_T, _ = ref.statistic(c['X'], c['indptr'], c['indices'])
    assert gl.utils.boundary_statistic(c['X'], c['r']).tobytes() == want_T.tobytes()


def test_repeatable_and_return_type(gl, device_cases):
    c = device_cases['n257_radius']
    a = gl.utils.boundary_statistic(c['X'], c['r'], return_normals=True)
    b = gl.utils.boundary_statistic(c['X'], c['r'], return_normals=True)
    assert isinstance(a, tuple) and len(a) == 2
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    T = gl.utils.boundary_statistic(c['X'], c['r'])
    assert isinstance(T, np.ndarray) and T.shape == (257,) and T.tobytes() == a[0].tobytes()
    ck = device_cases['n257_knn']
    Tk = gl.utils.boundary_statistic(ck['X'], ck['r'], knn=True)
    assert isinstance(Tk, np.ndarray) and Tk.tobytes() == gl.utils.boundary_statistic(ck['X'], ck['r'], knn=True).tobytes()
