"""The centered-kernel learner without a device: both restatements of tests/ck_ref.py against the reference's golden vectors within
the bound measured when the fixture was made, csrc/ck_plan.h compiled for the host against the device-order restatement bit for bit
at three chunk lengths, the refusals of ck_validate and of the learner (all raised before any device call), the stop rule's corner
cases, and the declaration of the entry point.

Regenerate the fixture with tests/golden/make_golden_ck.py (it needs the reference)."""
import os
import re
import subprocess
import sys
import numpy as np
import pytest
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import ck_ref as ref                # noqa: E402
import graphlearning_amd as gl      # noqa: E402
from graphlearning_amd import _hip  # noqa: E402


def load_golden():
    with np.load(os.path.join(ROOT, 'tests', 'golden', ref.GOLDEN_FILE)) as z:
        return {k: z[k] for k in z.files}


def golden_graph(gold, g):
    ip, ix, d = gold['graph_%s_indptr' % g], gold['graph_%s_indices' % g], gold['graph_%s_data' % g]
    n = len(ip) - 1
    return sparse.csr_matrix((d, ix, ip), shape=(n, n))


def golden_case(gold, name):
    """(W, train_ind, train_labels, classes, seed, the start vector e that seed gives)"""
    g, k = ref.GOLDEN_CASES[name]
    W = golden_graph(gold, g)
    seed = int(gold['case_%s_seed' % name])
    e = np.random.RandomState(seed).rand(W.shape[0], 1)          # what np.random.seed(seed); np.random.rand(n, 1) draws
    return W, gold['case_%s_ind' % name], gold['case_%s_labels' % name], k, seed, e


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope='module')
def gold():
    return load_golden()


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return ref.build_host_lib(tmp_path_factory.mktemp('ck_plan'))


def test_the_fixture_is_what_the_tests_need(gold):
    assert 0 < float(gold['bound']) <= 1e-12 and float(gold['bound']) == 16 * float(gold['delta_ref'])
    assert float(gold['delta_ref']) == max(float(gold['case_%s_delta_ref' % c]) for c in ref.GOLDEN_CASES)
    assert 0 < float(gold['l_bound']) <= 1e-12
    deg = np.diff(ref.without_diagonal(golden_graph(gold, 'loops')).indptr)
    assert deg.max() == 257 and int((deg == 0).sum()) == 2 and np.count_nonzero(golden_graph(gold, 'loops').diagonal()) > 50
    assert (abs(golden_graph(gold, 'directed') - golden_graph(gold, 'directed').T) > 0).nnz > 0
    for name in ref.GOLDEN_CASES:
        W, ind, labels, k, seed, e = golden_case(gold, name)
        errs, T, prob = gold['case_%s_errs' % name], int(gold['case_%s_T' % name]), gold['case_%s_prob' % name]
        assert len(errs) == T and errs[T - 1] <= 1e-10 < errs[T - 2]
        assert min(abs(errs[T - 1] - 1e-10), abs(errs[T - 2] - 1e-10)) >= 1e-13          # the stop is not a coin toss
        assert ref.top_two_gap(prob, ind) > 1e-9                                           # no vertex's label hangs on the last bits
        assert len(gold['case_%s_lines' % name]) == T


@pytest.mark.parametrize('name', sorted(ref.GOLDEN_CASES))
def test_golden_reference_order(gold, name):
    W, ind, labels, k, seed, e = golden_case(gold, name)
    u, l, T, errs = ref.ck_reference_order(W, ind, labels, k, e)
    prob = gold['case_%s_prob' % name]
    print(name, 'T', T, 'largest difference', np.abs(u - prob).max(), 'bound', float(gold['bound']))
    assert T == int(gold['case_%s_T' % name])
    assert np.abs(u - prob).max() <= float(gold['bound'])
    assert abs(l - float(gold['case_%s_l' % name])) <= float(gold['l_bound']) * abs(float(gold['case_%s_l' % name]))
    assert np.array_equal(ref.predict(u), gold['case_%s_pred' % name])
    assert np.allclose(errs, gold['case_%s_errs' % name], rtol=1e-6, atol=0)


@pytest.mark.parametrize('name', sorted(ref.GOLDEN_CASES))
def test_golden_device_order_and_host_loop(gold, lib, name):
    W, ind, labels, k, seed, e = golden_case(gold, name)
    u, l, T, errs, capped = ref.device_order_case(W, ind, labels, k, e)
    prob = gold['case_%s_prob' % name]
    print(name, 'T', T, 'largest difference', np.abs(u - prob).max(), 'bound', float(gold['bound']))
    assert T == int(gold['case_%s_T' % name]) and not capped
    assert np.abs(u - prob).max() <= float(gold['bound'])
    assert abs(l - float(gold['case_%s_l' % name])) <= float(gold['l_bound']) * abs(float(gold['case_%s_l' % name]))
    assert np.array_equal(ref.predict(u), gold['case_%s_pred' % name])
    Wd = ref.without_diagonal(W)
    val = np.ascontiguousarray(ref.start_values(W.shape[0], ind, labels, k)[ind])
    hu, hl, hT, herr, hcap = ref.host_solve(lib, Wd.indptr, Wd.indices, Wd.data, ind, val, e, cap=T + 5)
    assert same_bits(hu, u) and hl == l and hT == T and same_bits(herr, errs) and not hcap


PROBLEMS = [(0, 65, 2, 0, False), (1, 257, 3, 65, True), (2, 1, 1, 0, False), (3, 2, 2, 0, False), (4, 300, 17, 257, True), (5, 64, 10, 0, True),
            (7, 130, 1, 0, False)]


@pytest.mark.parametrize('seed,n,k,hub,directed', PROBLEMS)
def test_host_loop_equals_the_device_order_restatement(lib, seed, n, k, hub, directed):
    """ck_host_reference runs the device's schedule -- chunks, slots, two buffers, the look at the slot before -- with a loop in
    place of the kernels: the same bits at every chunk length, empty rows and negative weights included."""
    W, ind, val, e = ref.random_problem(seed, n, k, hub=hub, directed=directed, empty_rows=2 if n > 100 else 0)
    u, l, T, errs, capped = ref.ck_device_order(W.indptr, W.indices, W.data, ind, val, e, tol=1e-6)
    assert not capped and T >= 1
    for chunk in (1, 7, 64):
        hu, hl, hT, herr, hcap = ref.host_solve(lib, W.indptr, W.indices, W.data, ind, val, e, tol=1e-6, chunk=chunk, cap=T + 3)
        assert same_bits(hu, u) and hT == T and same_bits(herr, errs) and not hcap, chunk
        assert hl == l or (hl != hl and l != l), chunk


def test_stop_rule_corner_cases(gold, lib):
    W, ind, labels, k, seed, e = golden_case(gold, 'tiny')
    n = W.shape[0]
    K = ref.start_values(n, ind, labels, k)
    val = np.ascontiguousarray(K[ind])
    W = ref.without_diagonal(W)
    full = ref.ck_device_order(W.indptr, W.indices, W.data, ind, val, e)
    for tol in (1.0, 2.5, np.nan, np.inf):                       # `1 > tol` is false: no iteration, the start comes back
        for chunk in (1, 64):
            hu, hl, hT, herr, hcap = ref.host_solve(lib, W.indptr, W.indices, W.data, ind, val, e, tol=tol, chunk=chunk, cap=4)
            assert hT == 0 and same_bits(hu, K) and len(herr) == 0 and not hcap and hl == full[1]
    # a stop in the middle of a chunk: the iterate includes the stopping iteration's update and nothing after it
    errs = full[3]
    for T in (1, 6, 7, 8, 64, 65):
        tol = ref.stop_tol(errs, T)
        want = ref.ck_device_order(W.indptr, W.indices, W.data, ind, val, e, tol=tol)
        assert want[2] == T
        for chunk in (1, 7, 64):
            hu, hl, hT, herr, hcap = ref.host_solve(lib, W.indptr, W.indices, W.data, ind, val, e, tol=tol, chunk=chunk, cap=100)
            assert hT == T and same_bits(hu, want[0]) and same_bits(herr, errs[:T]) and not hcap, (T, chunk)
    # max_it reached, on and off a chunk's end; a negative tol never stops on a number
    for max_it in (5, 7, 64, 70):
        for chunk in (1, 7, 64):
            hu, hl, hT, herr, hcap = ref.host_solve(lib, W.indptr, W.indices, W.data, ind, val, e, tol=-1.0, max_it=max_it, chunk=chunk, cap=100)
            assert hcap and hT == max_it and same_bits(herr, errs[:max_it])


def test_a_nan_err_stops(lib):
    """np.max hands a NaN on and `nan > tol` is false: the reference stops there, and so does the maximum of the bit patterns."""
    W, ind, val, e = ref.random_problem(5, 64, 10, directed=True)
    val = val.copy()
    val[0, 0] = np.inf                                    # inf - inf in the first product of a neighbour of that vertex
    want = ref.ck_device_order(W.indptr, W.indices, W.data, ind, val, e, tol=1e-6)
    assert want[2] >= 1 and np.isnan(want[3][-1]) and not want[4]
    for tol in (1e-6, -1.0):
        hu, hl, hT, herr, hcap = ref.host_solve(lib, W.indptr, W.indices, W.data, ind, val, e, tol=tol, chunk=7, cap=50)
        assert hT == want[2] and np.isnan(herr[-1]) and not hcap
        assert same_bits(np.isnan(hu), np.isnan(want[0])) and np.array_equal(hu[~np.isnan(hu)], want[0][~np.isnan(hu)])


def test_refusals_of_ck_plan(lib):
    W, ind, val, e = ref.random_problem(0, 65, 2)
    indptr, indices, data = W.indptr.astype(np.int64), W.indices.astype(np.int32), W.data
    assert ref.host_validate(lib, indptr, indices, data, 2, ind) == 0

    def changed(arr, at, value):
        out = arr.copy()
        out[at] = value
        return out
    assert ref.host_validate(lib, indptr, indices, data, 0, ind) == 1
    assert ref.host_validate(lib, indptr, indices, data, 257, ind) == 9
    assert ref.host_validate(lib, indptr, indices, data, 256, ind) == 0
    assert ref.host_validate(lib, changed(indptr, 0, 1), indices, data, 2, ind) == 2
    assert ref.host_validate(lib, indptr, changed(indices, 3, 65), data, 2, ind) == 3
    assert ref.host_validate(lib, indptr, changed(indices, 3, -1), data, 2, ind) == 3
    row = int(np.searchsorted(indptr, 1, side='right') - 1)         # the row of entry 1 (and of entry 0)
    assert indptr[row + 1] - indptr[row] >= 2
    assert ref.host_validate(lib, indptr, changed(indices, indptr[row] + 1, indices[indptr[row]]), data, 2, ind) == 4     # a duplicate
    assert ref.host_validate(lib, indptr, changed(indices, indptr[row], row), data, 2, ind) in (4, 5)                  # the diagonal
    Wd = sparse.csr_matrix(W + sparse.identity(65))
    Wd.sort_indices()
    assert ref.host_validate(lib, Wd.indptr, Wd.indices, Wd.data, 2, ind) == 5
    for bad in (np.nan, np.inf, -np.inf):
        assert ref.host_validate(lib, indptr, indices, changed(data, 7, bad), 2, ind) == 6
    assert ref.host_validate(lib, indptr, indices, changed(data, 7, -3.0), 2, ind) == 0                               # negative weights are legal
    assert ref.host_validate(lib, indptr, indices, data, 2, np.array([0, 65])) == 7
    assert ref.host_validate(lib, indptr, indices, data, 2, np.array([-1])) == 7
    assert ref.host_validate(lib, indptr, indices, data, 2, ind, power_it=0) == 8
    assert ref.host_validate(lib, indptr, indices, data, 2, ind, max_it=0) == 8
    assert ref.host_validate(lib, indptr, indices, data, 2, ind, max_it=(1 << 24) + 1) == 8
    assert ref.host_validate(lib, indptr, indices, data, 2, ind, alpha_frac=np.nan) == 8


def test_column_tiles_of_the_pass(lib):
    for k in range(1, 257):
        t = ref.host_tiles(lib, k)
        assert len(t) == (k + 15) // 16 and t[0, 0] == 0 and t[:, 1].sum() == k and np.array_equal(t[1:, 0], np.cumsum(t[:-1, 1]))
        assert 1 <= t[:, 1].min() and t[:, 1].max() <= 16 and t[:, 1].max() - t[:, 1].min() <= 1 and t[0, 1] == t[:, 1].max()


def test_the_stand_alone_program_of_the_host_plan(tmp_path):
    exe = str(tmp_path / 'ck_plan_main')
    subprocess.run(['g++', '-O2', '-ffp-contract=off', '-std=c++17', '-DCK_PLAN_MAIN', '-I' + os.path.join(ROOT, 'graphlearning_amd', 'csrc'),
                    '-o', exe, os.path.join(ROOT, 'tests', 'ck_plan_host.cpp')], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith('ok T '), (res.returncode, res.stdout)


def test_learner_attributes():
    assert hasattr(gl.ssl, 'centered_kernel')
    W = ref.random_problem(0, 65, 2)[0]
    m = gl.ssl.centered_kernel(W)
    assert m.name == 'Centered Kernel' and m.accuracy_filename == '_centered_kernel' and m.onevsrest is False and m.similarity is True
    assert (m.tol, m.power_it, m.alpha) == (1e-10, 100, 1.05)
    assert m.get_accuracy_filename() == '_centered_kernel_accuracy.csv'
    assert gl.ssl.centered_kernel(W, class_priors=np.ones(2)).get_accuracy_filename() == '_centered_kernel_classpriors_accuracy.csv'
    m = gl.ssl.centered_kernel(W, None, 1e-6, 20, 1.5)               # the reference's positional order
    assert (m.tol, m.power_it, m.alpha) == (1e-6, 20, 1.5)


def test_value_errors_before_any_device_call(monkeypatch):
    calls = []

    def no_device(*a, **k):
        calls.append(a)
        raise AssertionError('the device call was reached')
    monkeypatch.setattr(_hip, 'ck_solve', no_device)
    W = ref.random_problem(6, 120, 3, directed=False)[0]
    n = W.shape[0]
    ind = np.array([0, 5, 17, 40, 80, 119])
    labels = np.array([0, 1, 2, 0, 1, 2])

    def fit(Wx, i=ind, l=labels, **kw):
        return gl.ssl.centered_kernel(Wx, **kw).fit(i, l)
    state = np.random.RandomState(5)
    np.random.seed(5)
    with pytest.raises(AssertionError):           # the accepted input gets as far as the device call ..
        fit(W)
    row_ptr, col, data, ti, val, e = calls[0][:6]
    assert same_bits(np.asarray(e), state.rand(n, 1)) and np.random.rand() == state.rand()      # .. with exactly n draws of the global stream
    assert same_bits(np.asarray(val), ref.start_values(n, ind, labels, 3)[ind])
    lonely = W.tolil()
    lonely[5, :] = 0
    neg = W.copy()
    neg.data[3] = -0.25
    for legal in (lonely.tocsr(), neg, W + sparse.identity(n)):          # rows without entries, negative weights, a stored diagonal
        with pytest.raises(AssertionError):
            fit(legal)
    assert calls[-1][0][-1] == W.nnz                                      # the diagonal is gone before the call
    with pytest.raises(ValueError, match='power_it'):
        fit(W, power_it=0)
    for bad in (np.nan, np.inf, -np.inf):
        Wb = W.copy()
        Wb.data[3] = bad
        with pytest.raises(ValueError, match='NaN or infinite'):
            fit(Wb)
    with pytest.raises(ValueError, match='out of range'):
        fit(W, i=np.concatenate([ind[:-1], [n]]))
    with pytest.raises(ValueError, match='out of range'):
        fit(W, i=np.concatenate([ind[:-1], [-1]]))
    with pytest.raises(ValueError, match='not exactly 0'):
        fit(W, l=labels + 1)
    with pytest.raises(ValueError, match='not exactly 0'):
        fit(W, l=np.where(labels == 1, 3, labels))
    with pytest.raises(ValueError, match='not exactly 0'):
        fit(W, l=labels + 0.5)
    with pytest.raises(ValueError, match='training indices for'):
        fit(W, l=labels[:-1])
    with pytest.raises(ValueError, match='no training vertex'):
        fit(W, i=np.zeros(0, dtype=np.int64), l=np.zeros(0, dtype=np.int64))
    big = sparse.identity(300, format='csr')
    with pytest.raises(ValueError, match='at most 256'):
        fit(big, i=np.arange(257), l=np.arange(257))
    assert len(calls) == 4


def test_entry_point_is_declared():
    with open(os.path.join(ROOT, 'include', 'glx_experimental.h')) as f:
        text = f.read()
    assert re.search(r'int glx_ck_solve\(int64_t n, int64_t M, const int64_t\* row_ptr, const int32_t\* col, const double\* W, int k,', text)
    with open(os.path.join(ROOT, 'include', 'glx.h')) as f:
        assert 'glx_ck_solve' not in f.read()
    assert 'glx_ck_solve' in _hip.EXPORTED_SYMBOLS and callable(_hip.ck_solve)
    assert len(_hip._SIGNATURES['glx_ck_solve']) == 23
    assert getattr(_hip.load(), 'glx_ck_solve') is not None
    with open(os.path.join(ROOT, 'graphlearning_amd', 'csrc', 'ck_plan.h')) as f:
        plan = f.read()
    assert '#include <hip' not in plan and 'glx_internal.h' not in plan and 'glx_stops.h' not in plan      # host only, its own stop struct
    assert 'struct CkStops' in plan
    with open(os.path.join(ROOT, 'graphlearning_amd', 'csrc', 'ck.hip')) as f:
        kern = f.read()
    assert not re.search(r'atomicAdd|unsafeAtomicAdd|cooperative_groups|hipMemsetAsync', kern)             # no float atomics, no grid wait, no memset node
