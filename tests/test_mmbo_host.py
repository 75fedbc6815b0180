"""The multiclass MBO learner without a device: csrc/mmbo_plan.h compiled for the host against the reference's golden labels from
the recorded start and the stored eigenpairs (equality on every vertex), the plain-numpy form of the reference's loop beside it, every
refusal of mmbo_validate, the recorded state of numpy's global stream, the refusals of the learner (all raised before any library
call), and the declaration of the entry point.

Regenerate the fixture with tests/golden/make_golden_mmbo.py (it needs the reference)."""
import os
import re
import subprocess
import sys
import numpy as np
import pytest
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import eig_ref                      # noqa: E402
import fixed_sum_ref                # noqa: E402
import mmbo_ref as ref              # noqa: E402
import graphlearning_amd as gl      # noqa: E402
from graphlearning_amd import _hip  # noqa: E402


@pytest.fixture(scope='module')
def gold():
    return ref.load_golden()


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return ref.build_host_lib(tmp_path_factory.mktemp('mmbo_plan'))


def golden_case(gold, name):
    """(W, truth, ind, labels, k, params, start labels)"""
    g = ref.GOLDEN_CASES[name][0]
    W, truth = eig_ref.golden_graph(gold, g), gold['graph_%s_truth' % g]
    key = 'case_%s_' % name
    return W, truth, gold[key + 'ind'], gold[key + 'labels'], len(np.unique(truth)), ref.case_params(name), gold[key + 'start']


def test_the_fixture_is_what_the_tests_need(gold):
    assert float(gold['min_gap']) >= ref.MIN_GAP
    assert float(gold['min_gap']) == min(float(gold['case_%s_min_gap' % c]) for c in ref.GOLDEN_CASES)
    assert len(ref.GOLDEN_CASES) == 10
    for name, (g, seed, changed) in ref.GOLDEN_CASES.items():
        W, truth, ind, labels, k, params, start = golden_case(gold, name)
        assert len(ind) == 5 * k and np.array_equal(labels, truth[ind]) and np.array_equal(start[ind], labels)
        assert gold['case_%s_key' % name].shape == (624,) and 0 <= int(gold['case_%s_pos' % name]) <= 624
        assert gold['case_%s_prob_labels' % name].shape == (W.shape[0],)
    assert {ref.case_params(c)['num_eig'] for c in ref.GOLDEN_CASES} == {20, 50}
    assert ref.case_params('blobs_short') == dict(Ns=3, T=4, dt=0.3, mu=10, num_eig=50)
    for name in ref.LINES_CASES:
        assert len(gold['case_%s_lines' % name]) == ref.case_params(name)['T']


@pytest.mark.parametrize('name', sorted(ref.GOLDEN_CASES))
def test_golden_host_reference_and_numpy_loop(gold, lib, name):
    W, truth, ind, labels, k, params, start = golden_case(gold, name)
    vals, X = ref.golden_eigenpairs(gold, name)
    args = dict(Ns=params['Ns'], T=params['T'], dt=params['dt'], mu=params['mu'])
    hist, Z, gap = ref.host_solve(lib, X, vals, start, ind, labels, k, Ns=args['Ns'], T=args['T'], dt=args['dt'], mu=float(args['mu']))
    want = gold['case_%s_prob_labels' % name]
    print(name, 'rows that differ', int((hist[-1] != want).sum()), 'smallest top-two gap', gap)
    assert np.array_equal(hist[-1], want)
    assert np.array_equal(hist[-1], gold['case_%s_pred' % name])          # one-hot scores: predict() is the label itself
    assert gap >= ref.MIN_GAP
    nhist, ngap = ref.numpy_loop(vals, X, start, ind, labels, k, **args)
    assert np.array_equal(nhist, hist) and ngap >= ref.MIN_GAP


@pytest.mark.parametrize('name', sorted(ref.GOLDEN_CASES))
def test_the_recorded_state_reproduces_the_start(gold, name):
    W, truth, ind, labels, k, params, start = golden_case(gold, name)
    saved = np.random.get_state()
    try:
        np.random.set_state(ref.numpy_state(gold, name))
        u = np.random.rand(k, W.shape[0])
    finally:
        np.random.set_state(saved)
    assert np.array_equal(ref.start_labels(u, ind, labels), start)


def test_host_reference_on_seeded_shapes(lib):
    """the chain inside a partial, the chains and the tree across partials, every step mode: against a direct restatement in numpy
    that adds in the documented order"""
    for seed, n, m, k, Ns, T in [(0, 1, 1, 1, 1, 1), (1, 65, 3, 2, 1, 3), (2, 200, 5, 3, 2, 2), (3, 4200, 2, 3, 3, 1)]:
        X, vals, lab0, ind, lab = ref.random_problem(seed, n, m, k)
        hist, Z, gap = ref.host_solve(lib, X, vals, lab0, ind, lab, k, Ns=Ns, T=T, dt=0.15, mu=50.0)
        h = 0.15 / Ns
        c0, d = h * 50.0, 1.0 / (1.0 + h * vals)
        tl = np.full(n, -1)
        tl[ind] = lab
        Y = X * d[None, :]
        labels, Zc, want = lab0.copy(), None, []
        for g in range(T * Ns + 1):
            if g > 0:
                u = np.zeros((n, k))
                for j in range(m):
                    u = u + Zc[None, :, j] * X[:, j, None]
                if g % Ns == 0:
                    labels = np.argmax(u, axis=1).astype(np.int32)
                    want.append(labels)
            if g == T * Ns:
                break
            if g % Ns == 0:
                u = ref.onehot(labels, k)
            b = np.where((tl >= 0)[:, None], u - c0 * (u - ref.onehot(np.maximum(tl, 0), k)), u)
            P = (n + 63) // 64
            part = np.zeros((P, k, m))
            for i in range(n):
                part[i // 64] = part[i // 64] + b[i][:, None] * Y[i][None, :]
            Zc = fixed_sum_ref.finish(part)
        assert np.array_equal(hist, np.array(want)) and eig_ref.same_bits(Z, Zc), (n, m, k)


def test_refusals_of_mmbo_plan(lib):
    X, vals, lab0, ind, lab = ref.random_problem(0, 65, 4, 3)

    def changed(arr, at, value):
        out = arr.copy()
        out[at] = value
        return out
    ok = lambda **kw: ref.host_validate(lib, X, vals, lab0, ind, lab, 3, **kw)          # noqa: E731
    assert ok() == 0
    assert ref.host_validate(lib, X, vals, lab0, ind, lab, 0) == 1
    assert ok(n=0) == 1 and ok(m=0) == 1
    assert ok(Ns=0) == 2 and ok(T=0) == 2 and ok(Ns=1 << 12, T=(1 << 12) + 1) == 2 and ok(Ns=1 << 12, T=1 << 12) in (0, 8)
    assert ok(dt=np.nan) == 3 and ok(mu=np.inf) == 3
    assert ref.host_validate(lib, X, vals, lab0, changed(ind, 0, 65), lab, 3) == 4
    assert ref.host_validate(lib, X, vals, lab0, changed(ind, 0, -1), lab, 3) == 4
    assert ref.host_validate(lib, X, vals, lab0, ind, changed(lab, 0, 3), 3) == 5
    assert ref.host_validate(lib, X, vals, lab0, ind, changed(lab, 0, -1), 3) == 5
    assert ref.host_validate(lib, X, vals, changed(lab0, 64, 3), ind, lab, 3) == 6
    for bad in (np.nan, np.inf):
        assert ref.host_validate(lib, changed(X, (64, 3), bad), vals, lab0, ind, lab, 3) == 7
        assert ref.host_validate(lib, X, changed(vals, 2, bad), lab0, ind, lab, 3) == 7
    assert ref.host_validate(lib, X, changed(vals, 2, -4.0), lab0, ind, lab, 3, Ns=1, dt=0.25) == 7          # 1 + (dt / Ns) * vals = 0
    assert ref.host_validate(lib, X, vals, lab0, ind[:0], lab[:0], 3) == 0                            # no training vertex is legal here
    # the caps: k, m at most 256 and k * m at most 4096
    for n, m, k, want in [(3, 16, 256, 0), (3, 16, 257, 8), (3, 256, 16, 0), (3, 257, 1, 8), (3, 64, 64, 0), (3, 65, 64, 8), (3, 256, 10, 0),
                          (3, 4097, 1, 8), (3, 241, 17, 8), (3, 240, 17, 0)]:
        Xc, vc, l0, ic, lc = ref.random_problem(1, n, m, k, ntrain=1)
        assert ref.host_validate(lib, Xc, vc, l0, ic, lc, k) == want, (m, k)
    assert ref.CAP == 4096 and gl.ssl.MMBO_CAP == 4096


def test_rows_held_in_lds_at_a_time(lib):
    """64 rows while 48 KiB of LDS hold them with Z, halved down to 8; never above the 64 KiB a workgroup may ask for"""
    seen = set()
    for k in range(1, 257):
        for m in range(1, 257):
            if k * m > ref.CAP:
                break
            sub, lds = ref.host_sub_rows(lib, k, m)
            seen.add(sub)
            assert sub in (8, 16, 32, 64) and lds == (k * (m | 1) + sub * (m + k)) * 8 and lds <= 52 * 1024 + 512
            assert lds <= 48 * 1024 or sub == 8
            assert sub == 64 or (k * (m | 1) + 2 * sub * (m + k)) * 8 > 48 * 1024          # the next size up would not fit
    assert seen == {8, 16, 32, 64}
    assert [ref.host_sub_rows(lib, k, m)[0] for k, m in [(10, 50), (4, 128), (8, 200), (64, 64), (10, 256), (256, 16)]] == [64, 32, 16, 8, 8, 8]


def test_the_stand_alone_program_of_the_host_plan(tmp_path):
    exe = str(tmp_path / 'mmbo_plan_main')
    subprocess.run(['g++', '-O2', '-ffp-contract=off', '-std=c++17', '-DMMBO_PLAN_MAIN', '-I' + os.path.join(ROOT, 'graphlearning_amd', 'csrc'),
                    '-o', exe, os.path.join(ROOT, 'tests', 'mmbo_plan_host.cpp')], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith('ok gap '), (res.returncode, res.stdout)


def test_learner_attributes():
    assert hasattr(gl.ssl, 'multiclass_mbo')
    W = sparse.identity(5, format='csr')
    m = gl.ssl.multiclass_mbo(W)
    assert m.name == 'Multiclass MBO' and m.requires_eig is True and m.onevsrest is False
    assert (m.Ns, m.T, m.dt, m.mu, m.num_eig) == (6, 10, 0.15, 50, 50)
    assert m.accuracy_filename == '_multiclass_mbo_Ns_6_T_10_dt_0.150_mu_50.00'
    assert m.get_accuracy_filename() == '_multiclass_mbo_Ns_6_T_10_dt_0.150_mu_50.00_accuracy.csv'
    assert gl.ssl.multiclass_mbo(W, class_priors=np.ones(2)).get_accuracy_filename().endswith('_mu_50.00_classpriors_accuracy.csv')
    m = gl.ssl.multiclass_mbo(W, None, 3, 4, 0.3, 10, 20)               # the reference's positional order
    assert (m.Ns, m.T, m.dt, m.mu, m.num_eig) == (3, 4, 0.3, 10, 20)
    assert m.accuracy_filename == '_multiclass_mbo_Ns_3_T_4_dt_0.300_mu_10.00'


def test_value_errors_before_any_library_call(gold, monkeypatch):
    calls = []

    def no_device(*a, **k):
        calls.append((a, k))
        raise AssertionError('the device call was reached')

    def no_library(*a, **k):
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_hip, 'mmbo_solve', no_device)
    monkeypatch.setattr(_hip, 'load', no_library)
    monkeypatch.setattr(_hip, 'Eig', no_library)
    name = 'moons_s0'
    W, truth, ind, labels, k, params, start = golden_case(gold, name)
    n = W.shape[0]
    vals, X = ref.golden_eigenpairs(gold, name)

    def model(**kw):
        m = gl.ssl.multiclass_mbo(W, **kw)
        m.graph.eigendata['normalized'].update(dict(method='exact', k=50, c=100, gamma=0, tol=0, q=1, eigenvalues=vals, eigenvectors=X))
        return m

    def fit(i=ind, l=labels, **kw):
        return model(**kw).fit(i, l)
    np.random.set_state(ref.numpy_state(gold, name))
    twin = np.random.RandomState()
    twin.set_state(ref.numpy_state(gold, name))
    with pytest.raises(AssertionError, match='device call'):           # the accepted input gets as far as the device call ..
        fit()
    a, kw = calls[0]
    assert a[0] is X and a[1] is vals and np.array_equal(a[2], start) and a[5] == k and kw['Ns'] == 6 and kw['T'] == 10
    twin.rand(k, n)
    assert np.random.rand() == twin.rand()                               # .. with exactly one rand(k, n) of the global stream
    for bad in (dict(Ns=0), dict(T=0), dict(Ns=1 << 12, T=(1 << 12) + 1), dict(Ns=2.5)):
        with pytest.raises(ValueError, match='Ns='):
            fit(**bad)
    for bad in (dict(dt=np.nan), dict(mu=np.inf), dict(dt=-np.inf)):
        with pytest.raises(ValueError, match='not finite'):
            fit(**bad)
    with pytest.raises(ValueError, match='out of range'):
        fit(i=np.concatenate([ind[:-1], [n]]))
    with pytest.raises(ValueError, match='out of range'):
        fit(i=np.concatenate([ind[:-1], [-1]]))
    with pytest.raises(ValueError, match='not exactly 0'):
        fit(l=labels + 1)
    with pytest.raises(ValueError, match='not exactly 0'):
        fit(l=labels + 0.5)
    with pytest.raises(ValueError, match='training indices for'):
        fit(l=labels[:-1])
    with pytest.raises(ValueError, match='no training vertex'):
        fit(i=np.zeros(0, dtype=np.int64), l=np.zeros(0, dtype=np.int64))
    with pytest.raises(ValueError, match='at most 256'):
        gl.ssl.multiclass_mbo(sparse.identity(300, format='csr')).fit(np.arange(257), np.arange(257))
    with pytest.raises(ValueError, match='above the limit of 4096'):
        gl.ssl.multiclass_mbo(sparse.identity(300, format='csr'), num_eig=50).fit(np.arange(82), np.arange(82))
    for what, at in (('eigenvalues', 3), ('eigenvectors', (7, 3))):
        for bad in (np.nan, np.inf):
            m = model()
            arr = m.graph.eigendata['normalized'][what].copy()
            arr[at] = bad
            m.graph.eigendata['normalized'][what] = arr
            with pytest.raises(ValueError, match='NaN or infinite'):
                m.fit(ind, labels)
    assert len(calls) == 1


def test_entry_point_is_declared():
    with open(os.path.join(ROOT, 'include', 'glx_experimental.h')) as f:
        text = f.read()
    assert re.search(r'int glx_mmbo_solve\(int64_t n, int m, const double\* X, const double\* vals, const int32_t\* lab0, int64_t ntrain,', text)
    with open(os.path.join(ROOT, 'include', 'glx.h')) as f:
        assert 'glx_mmbo_solve' not in f.read()
    assert 'glx_mmbo_solve' in _hip.EXPORTED_SYMBOLS and callable(_hip.mmbo_solve)
    assert len(_hip._SIGNATURES['glx_mmbo_solve']) == 17
    assert getattr(_hip.load(), 'glx_mmbo_solve') is not None
    with open(os.path.join(ROOT, 'graphlearning_amd', 'csrc', 'mmbo_plan.h')) as f:
        plan = f.read()
    assert 'hip' not in re.sub(r'//.*', '', plan).lower() and 'glx_internal.h' not in plan                # host only
    assert '#include "fixed_sum.h"' in plan and '#include "ck_plan.h"' not in plan                       # the shared sum, not another learner's plan
    with open(os.path.join(ROOT, 'graphlearning_amd', 'csrc', 'mmbo.hip')) as f:
        kern = f.read()
    assert not re.search(r'atomicAdd|unsafeAtomicAdd|cooperative_groups|hipMemsetAsync|__builtin_amdgcn_mfma|fma\(', kern)
    assert kern.count('#pragma clang fp contract(off)') == 2                              # one per kernel
