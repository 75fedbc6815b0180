"""Connected components without a GPU: the numpy restatement of union by minimum plus ranking (tests/components_ref.py) against scipy
on every case of tests/components_cases.py, the conditions on the case list that make the GPU run complete, the stand-alone host
program for csrc/cc_plan.h (tests/cc_plan_host.cpp: the kernels' own find and union on plain memory, against a breadth-first search),
and the surface: the C declaration, the export, the binding, the two graph methods and their refusals before any library call."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from scipy import sparse
from scipy.sparse import csgraph

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_cases as cases  # noqa: E402
import components_ref as ref  # noqa: E402

ROOT = cases.ROOT


@pytest.fixture(scope='module')
def host_cases():
    return cases.host_cases()


@pytest.fixture(scope='module')
def expected(host_cases):
    """name -> scipy's (ncomp, labels) with directed=False: computed once, shared, never written to"""
    out = {}
    for name, _, W in host_cases:
        ncomp, labels = cases.scipy_components(W)
        labels.setflags(write=False)
        out[name] = (ncomp, labels)
    return out


def test_restatement_equals_scipy_on_every_case(host_cases, expected):
    for name, _, W in host_cases:
        ncomp, labels = ref.components(W.indptr, W.indices, W.shape[0])
        want_n, want = expected[name]
        assert labels.dtype == np.int32 == want.dtype, name
        assert ncomp == want_n and np.array_equal(labels, want), name


def test_the_default_weak_form_gives_the_same_labels(host_cases, expected):
    """what graph.isconnected calls: connected_components(W) with directed=True, connection='weak'"""
    for name, _, W in host_cases:
        ncomp, labels = csgraph.connected_components(W)
        assert ncomp == expected[name][0] and np.array_equal(labels, expected[name][1]), name


def test_the_case_list_covers_what_the_gpu_run_needs(host_cases, expected):
    T = cases.wave_row_threshold()
    lengths = np.concatenate([np.diff(W.indptr) for _, _, W in host_cases])
    assert (lengths >= T).any() and ((lengths > 0) & (lengths < T)).any()             # both row classes
    assert {T - 1, T, T + 1} <= set(lengths.tolist())                                 # and the rows around the threshold
    tie = single_beside_giant = zeros = dups = unsorted = loops = empty = False
    for name, _, W in host_cases:
        ncomp, labels = expected[name]
        sizes = np.bincount(labels, minlength=ncomp)
        tie |= ncomp > 1 and (sizes == sizes.max()).sum() > 1 and sizes.max() > 1
        single_beside_giant |= (sizes == 1).any() and sizes.max() > W.shape[0] / 2
        zeros |= bool((W.data == 0).any())
        loops |= bool((W.nonzero()[0] == W.nonzero()[1]).any())
        empty |= bool((np.diff(W.indptr) == 0).any() and W.nnz > 0)
        for i in range(min(W.shape[0], 300)):
            row = W.indices[W.indptr[i]:W.indptr[i + 1]]
            dups |= len(np.unique(row)) < len(row)
            unsorted |= bool((np.diff(row) < 0).any())
    assert tie and single_beside_giant and zeros and dups and unsorted and loops and empty
    # a tie whose first maximum is neither the first nor the last component
    ncomp, labels = expected['tie_behind_a_single_vertex']
    sizes = np.bincount(labels, minlength=ncomp)
    assert 0 < np.argmax(sizes) < ncomp - 1 and (sizes == sizes.max()).sum() == 2
    assert expected['all_isolated'][0] == 100
    groups = {g for _, g, _ in host_cases}
    assert groups == {'random', 'diameter', 'hubs', 'ties'}
    assert max(W.shape[0] for _, _, W in host_cases) == 65536


def test_restatement_refuses_malformed_arrays():
    for indptr, indices in (([0, 2, 1, 3], [1, 2, 0]), ([0, 1, 2, 2], [1, 2, 0]), ([0, 1, 2, 3], [1, 3, 0]), ([0, 1, 2, 3], [1, -1, 0])):
        with pytest.raises(ValueError):
            ref.components(indptr, indices, 3)


def test_cc_plan_host_program_builds_and_passes(tmp_path):
    exe = str(tmp_path / 'cc_plan_host')
    subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'graphlearning_amd', 'csrc'), '-o', exe,
                    os.path.join(ROOT, 'tests', 'cc_plan_host.cpp')], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip().endswith('cc_plan_host: ok') and 'FAIL' not in res.stdout


# ---- the surface -----------------------------------------------------------------------------------------------------------------

def test_glx_components_is_declared_exported_and_bound():
    from graphlearning_amd import _hip
    hdr = open(os.path.join(ROOT, 'include', 'glx_experimental.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    decl = re.search(r'int glx_components\(([^)]*)\);', hdr)
    assert decl and [a.split()[-1].lstrip('*') for a in decl.group(1).split(',')] == \
        ['n', 'nnz', 'rowptr', 'col', 'labels', 'ncomp_out', 'ms_out', 'device']
    assert 'glx_components' in _hip.EXPORTED_SYMBOLS
    assert getattr(_hip.load(), 'glx_components') is not None
    assert list(inspect.signature(_hip.components).parameters) == ['indptr', 'indices', 'n', 'device']
    assert inspect.signature(_hip.components).parameters['device'].default is None
    assert hasattr(_hip, 'components_last_ms')
    assert _hip.components_plan()[1] == cases.wave_row_threshold()       # the header the cases read is the one the library was built from


def test_graph_methods_exist_with_device_none():
    import graphlearning_amd as gl
    for name in ('connected_components', 'largest_connected_component'):
        params = inspect.signature(getattr(gl.graph, name)).parameters
        assert list(params) == ['self', 'device'] and params['device'].default is None, name


@pytest.fixture
def no_library(monkeypatch):
    """any call into the library fails the test"""
    from graphlearning_amd import _hip

    def boom(*a, **k):
        raise AssertionError('the library was called')
    monkeypatch.setattr(_hip, 'load', boom)
    monkeypatch.setattr(_hip, 'components', boom)


def test_value_errors_fire_before_any_library_call(no_library):
    import graphlearning_amd as gl
    G = gl.graph(sparse.csr_matrix(np.ones((3, 4))))
    for call in (G.connected_components, G.largest_connected_component):
        with pytest.raises(ValueError, match='square'):
            call()
    # index arrays whose values no int32 holds (a cast would wrap 2^32 + 1 to the valid index 1)
    W = sparse.csr_matrix((np.ones(2), np.array([1, (1 << 32) + 1], dtype=np.int64), np.array([0, 1, 2, 2, 2], dtype=np.int64)), shape=(4, 4))
    assert W.indices.dtype == np.int64
    G = gl.graph(W)
    assert G.weight_matrix.indices.dtype == np.int64
    for call in (G.connected_components, G.largest_connected_component):
        with pytest.raises(ValueError, match='int32'):
            call()


def test_int64_index_arrays_with_small_values_are_accepted():
    """scipy hands out int64 index arrays for some constructions; values that fit are converted, not refused"""
    from graphlearning_amd import _hip
    a = _hip.int32_index_array(np.array([0, 1, 5], dtype=np.int64), 'a')
    assert a.dtype == np.int32 and a.tolist() == [0, 1, 5]
    with pytest.raises(ValueError):
        _hip.int32_index_array(np.array([0.0, 1.0]), 'a')
    with pytest.raises(ValueError):
        _hip.int32_index_array(np.array([0, -(1 << 31) - 1], dtype=np.int64), 'a')
