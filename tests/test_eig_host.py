"""graph.eigen_decomp and ssl.poisson(solver='spectral') without a device: csrc/eig_plan.h compiled for the host runs under the
package's own driver (graphlearning_amd/_eig.py, the code the device runs under) against scipy.sparse.linalg.svds on seeded graphs
and against the reference's golden vectors within the bounds measured when the fixture was made; the cases a single-vector Krylov
method gets wrong end in an error; every refusal is raised before any device call; numpy's global stream is left alone.

Regenerate the fixture with tests/golden/make_golden_eig.py (it needs the reference)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import eig_ref as ref               # noqa: E402
import graphlearning_amd as gl      # noqa: E402
from graphlearning_amd import _eig, _hip  # noqa: E402


@pytest.fixture(scope='module')
def gold():
    return ref.load_golden()


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return ref.build_host_lib(tmp_path_factory.mktemp('eig_plan'))


def test_the_fixture_is_what_the_tests_need(gold):
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', ref.GOLDEN_FILE)) < os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'g3_blobs5000.npz'))
    for q in ref.QUANTITIES + ('prob',):
        assert 0 < float(gold['delta_' + q]) <= 1e-9 and float(gold['bound_' + q]) == 16 * float(gold['delta_' + q])
    for g in ref.GRAPHS:
        W = ref.golden_graph(gold, g)
        assert sparse.csgraph.connected_components(W)[0] == 1 and W.shape[0] == {'blobs': 600, 'moons': 500}[g]
        for normalization, k in ref.DECOMPS:
            vals = np.concatenate([gold['dec_%s_%s_vals' % (g, normalization)], [float(gold['dec_%s_%s_next' % (g, normalization)])]])
            assert len(vals) == k + 1 and np.diff(vals).min() >= 1e-6               # no eigenvector hangs on a near-multiple eigenvalue
            assert gold['dec_%s_%s_vecs' % (g, normalization)].shape == (W.shape[0], k)
        assert len(gold['pois_%s_ind' % g]) == 5 * len(np.unique(gold['graph_%s_truth' % g]))
        for p in (1, 2):
            assert ref.top_two_gap(gold['pois_%s_p%d_prob' % (g, p)]) >= 1e-6          # no vertex's label hangs on the last bits


@pytest.mark.parametrize('normalization', ref.NORMALIZATIONS)
@pytest.mark.parametrize('n,k', ref.SHAPES)
def test_restatement_against_svds(gold, lib, n, k, normalization):
    """The host restatement in plain float64 against LAPACK/ARPACK: 1e-12 bounds an error, it is no measured margin (2e-15 measured)."""
    W = ref.seeded_graph(n)
    vals, vecs, steps, restarts, probe = ref.host_decomp(lib, W, normalization, k)
    A, D, M = _eig.operator(W, normalization)
    s_ref, u_ref = ref.svds_reference(A, k)
    s = (1 - vals) if M is None else (M - vals)
    V = ref.a_vectors(W, normalization, vecs)
    print((n, k), normalization, 'steps', steps, 'restarts', restarts, 'probe', probe, '|ds| / s_max', np.abs(s - s_ref).max() / s_ref[0],
          'orthonormality', ref.orthonormality(V), 'subspace', ref.subspace_defect(V, u_ref), 'bound', float(gold['bound_subspace']))
    assert np.all(np.diff(vals) >= 0) and vecs.shape == (n, k)
    assert np.abs(s - s_ref).max() <= 1e-12 * s_ref[0]
    assert ref.orthonormality(V) <= 1e-12
    assert ref.subspace_defect(V, u_ref) <= float(gold['bound_subspace'])
    m = _eig.basis_size(n, k)
    if n == m:
        assert (steps, restarts, probe) == (n, 0, None)                    # one run spans the space: no restart, no probe
    else:
        assert restarts >= 1 and probe is not None and steps == m + restarts * (m - (k + (m - k) // 2))
    if (n, k) == (25, 11):
        assert m == 23
    if (n, k) == (1000, 256):
        assert m == 513
    if (n, k) in ((64, 30), (257, 100)) and normalization != 'combinatorial':
        assert (np.sum(V * (A @ V), axis=0) < 0).any()                     # negative eigenvalues of large modulus are among the k


def test_missed_copies_and_breakdown_end_in_an_error(lib):
    """Ten components make the eigenvalue 1 of D^-1/2 W D^-1/2 ten-fold; a path is bipartite, so +-lambda doubles every eigenvalue of A A
    (with k = 3: at k = 5 .. 20 rounding lets the second copies converge and the result agrees with svds; at k = 2 the probe's 18 steps
    do not reach the copy and a wrong set is returned -- the probe detects, it proves nothing).  A complete graph has two distinct
    eigenvalues: the Krylov space ends at the second step."""
    with pytest.raises(_hip.GlxError, match='a multiple eigenvalue was missed'):
        ref.host_decomp(lib, ref.components_graph(10, 60), 'normalized', 11)
    with pytest.raises(_hip.GlxError, match='a multiple eigenvalue was missed'):
        ref.host_decomp(lib, ref.path_graph(101), 'normalized', 3)
    for normalization in ref.NORMALIZATIONS:
        with pytest.raises(_hip.GlxError, match='breakdown'):
            ref.host_decomp(lib, ref.complete_graph(30), normalization, 3)


@pytest.mark.parametrize('normalization', ref.NORMALIZATIONS)
def test_two_components_agree_with_svds_or_raise(lib, normalization):
    W = ref.components_graph(2, 500)
    assert W.shape[0] == 1000
    try:
        vals, vecs, steps, restarts, probe = ref.host_decomp(lib, W, normalization, 11)
    except _hip.GlxError as e:
        assert 'a multiple eigenvalue was missed' in str(e)
        return
    A, D, M = _eig.operator(W, normalization)
    s_ref, _ = ref.svds_reference(A, 11)
    s = (1 - vals) if M is None else (M - vals)
    assert np.abs(s - s_ref).max() <= 1e-12 * s_ref[0]                     # never another set


def test_refusals_of_the_plan(lib):
    W = ref.seeded_graph(65)
    indptr, indices, data = ref.csr_arrays(W)

    def changed(a, i, v):
        b = a.copy()
        b[i] = v
        return b
    assert ref.host_validate(lib, indptr, indices, data, 20) == 0
    assert ref.host_validate(lib, indptr, indices, changed(data, 7, -3.0), 20) == 0                  # negative values are legal here
    assert ref.host_validate(lib, indptr, changed(indices, 1, indices[0]), data, 20) == 4            # a duplicate
    assert ref.host_validate(lib, indptr, changed(changed(indices, 0, indices[1]), 1, indices[0]), data, 20) == 4     # descending
    assert ref.host_validate(lib, indptr, changed(indices, 3, 65), data, 20) == 3
    assert ref.host_validate(lib, indptr, changed(indices, 3, -1), data, 20) == 3
    for bad in (np.nan, np.inf, -np.inf):
        assert ref.host_validate(lib, indptr, indices, changed(data, 7, bad), 20) == 6
    assert ref.host_validate(lib, changed(indptr, 0, 1), indices, data, 20) == 2
    assert ref.host_validate(lib, changed(indptr, 5, indptr[4] - 1), indices, data, 20) == 2
    for m in (0, -1, 66, 514):
        assert ref.host_validate(lib, indptr, indices, data, m) == 8
    assert ref.host_validate(lib, indptr, indices, data, 65) == 0
    big = sparse.identity(600, format='csr')
    assert ref.host_validate(lib, *ref.csr_arrays(big), 513) == 0 and ref.host_validate(lib, *ref.csr_arrays(big), 514) == 8
    # columns and steps out of range
    with ref.HostBackend(lib, W, 20) as b:
        x = np.ones(65)
        for call in (lambda: b.set_column(-1, x), lambda: b.set_column(21, x), lambda: b.orthonormalize(21), lambda: b.run(0, 21),
                     lambda: b.run(3, 3), lambda: b.run(-1, 2), lambda: b.rotate(np.zeros((21, 2)), 21, 2), lambda: b.rotate(np.zeros((5, 6)), 5, 6),
                     lambda: b.rotate(np.zeros((5, 0)), 5, 0), lambda: b.get_columns(0, 22), lambda: b.get_columns(4, 4)):
            with pytest.raises(ValueError):
                call()
        b.set_column(20, x)                                                # the basis has m + 1 columns
    # the basis size and the memory estimate
    for n, k, m in ((20, 5, 20), (25, 11, 23), (1000, 256, 513), (70000, 10, 21), (70000, 50, 101), (15, 3, 15)):
        assert lib.eig_host_basis_size(n, k) == m == _eig.basis_size(n, k)
    assert lib.eig_host_device_bytes(70000, 1000000, 101) >= (101 + 3) * 70000 * 8 + 1000000 * 12
    assert lib.eig_host_device_bytes(70000, 1000000, 101) < 1.2 * ((101 + 3) * 70000 * 8 + 1000000 * 12) + (1 << 22)


def test_refusals_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError('the device call was reached')
    monkeypatch.setattr(_hip, 'Eig', no_device)
    W = ref.seeded_graph(120)

    def decomp(Wx, **kw):
        return gl.graph(Wx).eigen_decomp(**kw)
    for normalization in ref.NORMALIZATIONS:
        with pytest.raises(AssertionError):                      # the accepted input gets as far as the device call
            decomp(W, normalization=normalization)
    with pytest.raises(AssertionError):
        decomp(W + sparse.identity(120), k=119)                     # a stored diagonal and k = n - 1 are legal
    skew = W.copy()
    skew.data[3] = np.nextafter(skew.data[3], 2)
    with pytest.raises(ValueError, match='not symmetric bit for bit'):
        decomp(skew)
    directed = sparse.csr_matrix(sparse.triu(W))
    with pytest.raises(ValueError, match='not symmetric bit for bit'):
        decomp(directed)
    lonely = W.tolil()
    lonely[5, :] = 0
    lonely[:, 5] = 0
    lonely = lonely.tocsr()
    for normalization in ('normalized', 'randomwalk'):
        with pytest.raises(ValueError, match='degree 0'):
            decomp(lonely, normalization=normalization)
    with pytest.raises(AssertionError):
        decomp(lonely, normalization='combinatorial')               # no division there
    for bad in (np.nan, np.inf, -np.inf, -0.25):
        Wb = W.copy()
        Wb.data[:] = np.where(Wb.data == Wb.data[3], bad, Wb.data)  # (both entries of the pair)
        with pytest.raises(ValueError, match='NaN, infinite or negative'):
            decomp(Wb)
    for k in (0, -1, 120, 500):
        with pytest.raises(ValueError, match=r'outside \[1, n\)'):
            decomp(W, k=k)
    with pytest.raises(ValueError, match='above 256'):
        decomp(sparse.csr_matrix(ref.seeded_graph(300)), k=257)
    with pytest.raises(NotImplementedError, match='lowrank'):
        decomp(W, method='lowrank')
    with pytest.raises(NotImplementedError, match='gamma'):
        decomp(W, gamma=0.5)
    # the spectral solver refuses through the same checks
    with pytest.raises(ValueError, match='not symmetric bit for bit'):
        gl.ssl.poisson(skew, solver='spectral').fit(np.array([0, 5]), np.array([0, 1]))
    model = gl.ssl.poisson(W, p=2)
    assert model.solver == 'spectral' and model.accuracy_filename == '_poisson_p2.00_N10'
    with pytest.raises(AssertionError):
        model.fit(np.array([0, 5]), np.array([0, 1]))


def test_the_library_refuses_before_any_launch():
    """glx_eig_create checks the arrays on the host first: these refusals need no device."""
    W = ref.seeded_graph(65)
    indptr, indices, data = ref.csr_arrays(W)
    bad_index = indices.copy()
    bad_index[3] = 65
    swapped = indices.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    nan = data.copy()
    nan[2] = np.nan
    for args, what in (((indptr, bad_index, data, 20), 'out of range'), ((indptr, swapped, data, 20), 'not canonical'),
                       ((indptr, indices, nan, 20), 'not finite'), ((indptr, indices, data, 0), 'basis size'),
                       ((indptr, indices, data, 66), 'basis size'), ((indptr, indices, data, 514), 'basis size')):
        with pytest.raises(_hip.GlxError, match=what):
            _hip.Eig(*args)


def test_the_global_stream_is_left_alone(lib):
    np.random.seed(123)
    before = np.random.get_state()
    W = ref.seeded_graph(200)
    a = ref.host_decomp(lib, W, 'normalized', 7)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    b = ref.host_decomp(lib, W, 'normalized', 7)                            # and a solve is a pure function of its arguments
    assert ref.same_bits(a[0], b[0]) and ref.same_bits(a[1], b[1]) and a[2:] == b[2:]


def test_the_driver_decides_as_documented(lib):
    """keep = k + (m - k) // 2, one run per restart, the basis size as a keyword, the probe's length"""
    W = ref.seeded_graph(600)
    A, D, M = _eig.operator(W, 'normalized')
    for m in (None, 30):
        size = _eig.basis_size(600, 11) if m is None else m
        with ref.HostBackend(lib, A, size) as b:
            theta, steps, restarts, probe = _eig.thick_restart(b, 600, 11, m=m)
            keep = 11 + (size - 11) // 2
            assert steps == size + restarts * (size - keep) and b.calls['run'] == restarts + 2 and b.calls['rotate'] == restarts + 1
            assert np.all(np.diff(theta) <= 0) and probe < theta[-1]
            s_ref, _ = ref.svds_reference(A, 11)
            assert np.abs(np.sqrt(theta) - s_ref).max() <= 1e-12
    with pytest.raises(ValueError):
        with ref.HostBackend(lib, A, 23) as b:
            _eig.thick_restart(b, 600, 0)
    with ref.HostBackend(lib, A, 23) as b:
        with pytest.raises(_hip.GlxError, match='no convergence within 1 restarts'):
            _eig.thick_restart(b, 600, 11, max_restarts=1)


@pytest.mark.parametrize('g', ref.GRAPHS)
def test_golden_through_the_host_backend(gold, lib, g):
    W = ref.golden_graph(gold, g)
    for normalization, k in ref.DECOMPS:
        key = 'dec_%s_%s_' % (g, normalization)
        vals, vecs, steps, restarts, probe = ref.host_decomp(lib, W, normalization, k)
        got = ref.measure(W, normalization, vals, vecs, gold[key + 'vals'], gold[key + 'vecs'])
        print(g, normalization, k, 'steps', steps, 'restarts', restarts, got)
        for q in ref.QUANTITIES:
            assert got[q] <= float(gold['bound_' + q]), (q, got[q])
    ind, labels = gold['pois_%s_ind' % g], gold['pois_%s_labels' % g]
    vals, vecs, _, _, _ = ref.host_decomp(lib, ref.without_diagonal(W), 'randomwalk', 11)
    for p in (1, 2):
        prob = ref.poisson_spectral(vals, vecs, W.shape[0], ind, labels, p=p)
        d = ref.prob_difference(prob, gold['pois_%s_p%d_prob' % (g, p)])
        print(g, 'p', p, 'largest difference over largest |prob|', d, 'bound', float(gold['bound_prob']))
        assert d <= float(gold['bound_prob'])
        assert np.array_equal(np.argmax(prob, axis=1), gold['pois_%s_p%d_pred' % (g, p)])


def test_the_stand_alone_program_of_the_host_plan(tmp_path):
    exe = str(tmp_path / 'eig_plan_main')
    subprocess.run(['g++', '-O2', '-ffp-contract=off', '-std=c++17', '-DEIG_PLAN_MAIN', '-I' + os.path.join(ROOT, 'graphlearning_amd', 'csrc'),
                    '-o', exe, os.path.join(ROOT, 'tests', 'eig_plan_host.cpp')], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith('ok alpha '), (res.returncode, res.stdout)


def test_entry_points_are_declared():
    with open(os.path.join(ROOT, 'include', 'glx_experimental.h')) as f:
        text = f.read()
    with open(os.path.join(ROOT, 'include', 'glx.h')) as f:
        core = f.read()
    names = ('glx_eig_create', 'glx_eig_set_column', 'glx_eig_orthonormalize', 'glx_eig_run', 'glx_eig_rotate', 'glx_eig_get_columns',
             'glx_eig_destroy')
    for name in names:
        assert re.search(r'int %s\(' % name, text) and name not in core and name in _hip.EXPORTED_SYMBOLS
        assert getattr(_hip.load(), name) is not None
    assert re.search(r'int glx_eig_create\(int64_t n, const int64_t\* row_ptr, const int32_t\* col, const double\* val, int m, int device,', text)
    with open(os.path.join(ROOT, 'graphlearning_amd', 'csrc', 'eig_plan.h')) as f:
        plan = f.read()
    assert 'hip' not in re.sub(r'//.*', '', plan).lower()                                          # no HIP header
    assert '#include "fixed_sum.h"' in plan and '#include "ck_plan.h"' not in plan                 # the shared sum, not another learner's plan
    for name in ('set_column', 'orthonormalize', 'run', 'rotate', 'get_columns', 'close', '__enter__', '__exit__'):
        assert callable(getattr(_hip.Eig, name))
    assert callable(gl.graph.graph.eigen_decomp)
