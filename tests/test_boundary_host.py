"""utils.boundary_statistic without a GPU: the numpy restatement tests/boundary_ref.py (both forms) equals every golden vector of the
reference (tests/golden/g25_boundary.npz, written by tests/golden/make_golden_boundary.py); the stand-alone host program for
csrc/bstat_plan.h (tests/bstat_plan_host.cpp: the kernels' own arithmetic on plain memory) equals the restatement bit for bit on every
device case, its generalised numpy-order sum equals numpy for every row length from 1 to 300, and it runs clean under the address and
undefined-behaviour sanitizers; the conditions on the case list; and the surface: declaration, export, binding, refusals."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_ref as ref  # noqa: E402
import boundary_cases as cases  # noqa: E402

TAGS = {(False, True): 'o1', (True, True): 'o2c', (True, False): 'o2'}


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'g25_boundary.npz'))


@pytest.fixture(scope='module')
def device_cases():
    return cases.device_cases()


def golden_case(gold, name):
    mode, n, d, r, seed = cases.GOLDEN[name]
    X = cases.golden_points(name)
    assert np.array_equal(gold[name + '_X'], X) and float(gold[name + '_r']) == r
    if mode == 'knn':
        J = gold[name + '_J']
        indptr, indices = ref.knn_pattern(J, r)
    else:
        J = None
        indptr, indices = ref.ball_pattern(X, r)
    return X, indptr, indices, J


@pytest.mark.parametrize('name', sorted(cases.GOLDEN))
def test_restatement_equals_the_reference(gold, name):
    """nu bit for bit and T equal as numbers, for every stored case, the three order settings and both forms of the restatement"""
    assert sorted(gold['case_names']) == sorted(cases.GOLDEN)
    X, indptr, indices, J = golden_case(gold, name)
    for (second, cutoff), tag in TAGS.items():
        for form in (ref.statistic_rows, ref.statistic):
            T, nu = form(X, indptr, indices, J=J, second_order=second, cutoff=cutoff)
            assert nu.tobytes() == gold['%s_nu_%s' % (name, tag)].tobytes(), (name, tag, form.__name__)
            assert np.array_equal(T, gold['%s_T_%s' % (name, tag)]), (name, tag, form.__name__)
            assert not np.signbit(T[T == 0]).any()


def test_golden_cases_meet_their_conditions(gold):
    most_full = 0
    for name, (mode, n, d, r, seed) in cases.GOLDEN.items():
        X, indptr, indices, J = golden_case(gold, name)
        lens = np.diff(indptr)
        assert lens.min() >= 1, name
        if mode == 'knn':
            Js = np.sort(J, axis=1)
            assert not (Js[:, 1:] == Js[:, :-1]).any(), name
            assert (lens == r - 1).all()                 # k - 1 neighbours per vertex: self was in every list
        else:
            assert d <= 5
            most_full = max(most_full, int((lens == lens.max()).sum()))
    assert most_full >= 2
    # r_edge: rows of exactly maxdeg - 1 entries with a negative maximum in every order setting (the reference's list is the row:
    # no 0 joins), beside shorter rows, where a 0 does
    X, indptr, indices, J = golden_case(gold, 'r_edge')
    lens = np.diff(indptr)
    edge = np.flatnonzero(lens == lens.max() - 1)
    assert len(edge) and (lens < lens.max() - 1).any()
    for tag in TAGS.values():
        assert (gold['r_edge_T_' + tag][edge] < 0).any(), tag
        assert (gold['r_edge_T_' + tag][lens < lens.max() - 1] >= 0).all(), tag


@pytest.mark.parametrize('name', sorted(q for q in cases.GOLDEN if cases.GOLDEN[q][0] == 'knn'))
def test_restatement_with_wider_lists_equals_the_reference(gold, name):
    """knn_data wider than k, as the reference uses it: the graph from the first k + 1 columns, the maximum over all columns"""
    mode, n, d, k, seed = cases.GOLDEN[name]
    X = cases.golden_points(name)
    Jw, Dw = ref.knn_lists(X, k + 5)
    T, nu = ref.statistic(X, *ref.knn_pattern(Jw, k + 1), J=Jw)
    assert np.array_equal(T, gold[name + '_Twide'])


# ---- the header on the host ------------------------------------------------------------------------------------------------------------

def _build(tmp, name, extra=()):
    exe = str(tmp / name)
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-Wall', '-Werror', *extra,
                    '-I' + os.path.join(ROOT, 'graphlearning_amd', 'csrc'), '-o', exe, os.path.join(ROOT, 'tests', 'bstat_plan_host.cpp')],
                   check=True)
    return exe


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('bstat')
    return _build(tmp, 'bstat_plan_host'), tmp


def run_stat(exe, tmp, c, second, cutoff, wave_row=0, expect_ok=True):
    """(status, rows[3], T, nu, stdout) of the host program on one case"""
    X = np.ascontiguousarray(c['X'], dtype=np.float64)
    n, d = X.shape
    J = c['J']
    k = 0 if J is None else J.shape[1]
    wave_row = wave_row or cases.plan_constants()[0]
    fin, fout = str(tmp / 'in.bin'), str(tmp / 'out.bin')
    with open(fin, 'wb') as f:
        f.write(np.array([n, d, len(c['indices']), k, (1 if second else 0) | (2 if cutoff else 0), wave_row], dtype=np.int64).tobytes())
        f.write(X.tobytes())
        f.write(np.ascontiguousarray(c['indptr'], dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(c['indices'], dtype=np.int32).tobytes())
        if J is not None:
            f.write(np.ascontiguousarray(J, dtype=np.int32).tobytes())
    res = subprocess.run([exe, 'stat', fin, fout], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    raw = open(fout, 'rb').read()
    head = np.frombuffer(raw[:32], dtype=np.int64)
    T = np.frombuffer(raw[32:32 + 8 * n], dtype=np.float64)
    nu = np.frombuffer(raw[32 + 8 * n:], dtype=np.float64).reshape(n, d)
    return int(head[0]), head[1:].tolist(), T, nu, res.stdout


def test_host_program_equals_the_restatement(host_program, device_cases):
    """csrc/bstat_plan.h on plain memory == tests/boundary_ref.py bit for bit (zeros are +0.0 on both sides), on every device case
    and the three order settings; the class threshold changes the split and nothing else"""
    exe, tmp = host_program
    for name, c in device_cases.items():
        for second, cutoff in ref.ORDERS:
            want_T, want_nu = ref.statistic(c['X'], c['indptr'], c['indices'], J=c['J'], second_order=second, cutoff=cutoff)
            status, rows, T, nu, _ = run_stat(exe, tmp, c, second, cutoff)
            assert status == 0, name
            assert nu.tobytes() == want_nu.tobytes(), (name, second, cutoff)
            assert T.tobytes() == want_T.tobytes(), (name, second, cutoff)
            assert rows[0] + rows[1] == len(c['X'])
    c = device_cases['lengths']
    want_T, _ = ref.statistic(c['X'], c['indptr'], c['indices'])
    splits = set()
    for wave_row in (1, 64, 65, 4096):
        status, rows, T, nu, _ = run_stat(exe, tmp, c, True, True, wave_row=wave_row)
        assert T.tobytes() == want_T.tobytes()
        splits.add(tuple(rows[:2]))
    assert len(splits) == 4


def test_restatement_forms_agree_on_small_device_cases(device_cases):
    for name in ('n2_radius', 'n2_knn', 'n65_radius', 'n65_knn', 'd9_radius', 'full_rows', 'no_self'):
        c = device_cases[name]
        for second, cutoff in ref.ORDERS:
            a = ref.statistic_rows(c['X'], c['indptr'], c['indices'], J=c['J'], second_order=second, cutoff=cutoff)
            b = ref.statistic(c['X'], c['indptr'], c['indices'], J=c['J'], second_order=second, cutoff=cutoff)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), name
    assert np.isneginf(ref.statistic(**{q: device_cases['n2_radius'][q] for q in ('X', 'indptr', 'indices')})[0]).all()


def test_host_program_names_the_first_vertex_without_a_normal(host_program):
    exe, tmp = host_program
    X = cases.lattice()
    indptr, indices = ref.ball_pattern(X, 1.5)
    c = {'X': X, 'indptr': indptr, 'indices': indices, 'J': None}
    # first order: the first interior vertex of the 12 x 12 grid; second order: the first whose neighbours all have 8 neighbours
    for second, first in ((False, 13), (True, 26)):
        with pytest.raises(ref.ZeroNormal) as e:
            ref.statistic(X, indptr, indices, second_order=second)
        with pytest.raises(ref.ZeroNormal) as e2:
            ref.statistic_rows(X, indptr, indices, second_order=second)
        assert e.value.vertex == e2.value.vertex == first
        assert run_stat(exe, tmp, c, second, True)[0] == 1 + first
    Xd, J, D, first = cases.duplicates_knn()
    indptr, indices = ref.knn_pattern(J, J.shape[1])
    assert (np.diff(indptr) == J.shape[1]).any()           # a vertex that is missing from its own list
    c = {'X': Xd, 'indptr': indptr, 'indices': indices, 'J': J.astype(np.int32)}
    assert run_stat(exe, tmp, c, False, True)[0] == 1 + first
    with pytest.raises(ref.ZeroNormal) as e:
        ref.statistic(Xd, indptr, indices, J=J, second_order=False)
    assert e.value.vertex == first


def test_host_program_refuses_malformed_arguments(host_program):
    exe, tmp = host_program
    X = np.random.default_rng(0).random((4, 2))
    good = {'X': X, 'indptr': [0, 1, 2, 3, 4], 'indices': [1, 0, 3, 2], 'J': None}
    assert run_stat(exe, tmp, good, True, True)[0] == 0
    for change, word in (({'indptr': [0, 1, 1, 3, 4]}, 'no neighbour'), ({'indptr': [0, 2, 2, 3, 4], 'indices': [1, 1, 3, 2]}, 'canonical'),
                         ({'indices': [1, 0, 4, 2]}, 'out of range'), ({'indptr': [0, 1, 2, 3, 3]}, 'row pointers'),
                         ({'indptr': [0, 2, 1, 3, 4], 'indices': [0, 1, 3, 2]}, 'row pointers'), ({'J': np.array([[0, 1], [1, 0], [2, 3], [3, 4]])}, 'list index'),
                         ({'J': np.array([[0, 1], [1, 0], [2, -1], [3, 2]])}, 'list index')):
        status, _, _, _, said = run_stat(exe, tmp, dict(good, **change), True, True)
        assert status == -1 and word in said, (change, said)


def test_term_walk_equals_numpy(host_program):
    """csrc/npsum_exact.h over a term functor == np.sum(..., axis=1) bit for bit for every row length 1 .. 300 and beyond the second
    split: the squared difference (what the epsilon-ball weights use), the product of two rows, and the statistic's two terms"""
    exe, tmp = host_program
    rng = np.random.default_rng(0)
    fin, fout = str(tmp / 'np_in.bin'), str(tmp / 'np_out.bin')
    for d in list(range(1, 301)) + [511, 512, 513, 1000, 1025, 3000]:
        U, V, W = rng.normal(size=(3, 16, d))
        if d % 3 == 0:
            U, V = U + 1e6, V + 1e6
        with open(fin, 'wb') as f:
            f.write(np.array([16, d], dtype=np.int64).tobytes() + U.tobytes() + V.tobytes() + W.tobytes())
        subprocess.run([exe, 'npsum', fin, fout], check=True, capture_output=True)
        got = np.fromfile(fout, dtype=np.float64).reshape(4, 16)
        D = U - V
        want = [np.sum(D * D, axis=1), np.sum(U * V, axis=1), np.sum(D * W, axis=1), np.sum(D * ((W + U) / 2), axis=1)]
        for q in range(4):
            assert got[q].tobytes() == want[q].tobytes(), (d, q)


def test_host_program_runs_clean_under_sanitizers(tmp_path, device_cases):
    exe = _build(tmp_path, 'bstat_plan_host_san', extra=('-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'))
    for name in ('n2_radius', 'd129_knn', 'lengths', 'hub', 'd9_radius'):
        c = device_cases[name]
        status, rows, T, nu, said = run_stat(exe, tmp_path, c, True, True)
        assert status == 0 and 'runtime error' not in said
    U = np.random.default_rng(1).normal(size=(3, 4, 300))
    fin, fout = str(tmp_path / 'a.bin'), str(tmp_path / 'b.bin')
    with open(fin, 'wb') as f:
        f.write(np.array([4, 300], dtype=np.int64).tobytes() + U.tobytes())
    res = subprocess.run([exe, 'npsum', fin, fout], capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr, res.stderr


# ---- the case list ---------------------------------------------------------------------------------------------------------------------

def test_case_list_reaches_every_path(device_cases):
    wave_row, short_lanes = cases.plan_constants()
    assert short_lanes == 16 and 64 <= wave_row <= 1024
    lens_radius, lens_knn, dims = set(), set(), set()
    full_rows = {}
    for name, c in device_cases.items():
        lens = np.diff(c['indptr'])
        assert lens.min() >= 1, name
        dims.add(c['X'].shape[1])
        if c['J'] is None:
            lens_radius |= set(lens.tolist())
            full_rows[name] = int((lens == lens.max()).sum())
        else:
            lens_knn.add(c['J'].shape[1])
    assert {1, 63, 64, 65, wave_row - 1, wave_row, wave_row + 1} <= lens_radius          # both classes, the lengths around the threshold
    assert max(lens_radius) >= 2000                                                      # the hub row
    assert {2, 61} <= lens_knn
    assert {1, 7, 8, 9, 128, 129} <= dims                                                # where numpy's row sum changes its walk
    assert min(full_rows.values()) >= 1 and full_rows['full_rows'] == 27 and full_rows['hub'] == 1
    assert {c['X'].shape[0] for c in device_cases.values()} >= {2, 65, 257}
    assert (np.diff(device_cases['no_self']['indptr']) == device_cases['no_self']['J'].shape[1]).all()


# ---- the surface -----------------------------------------------------------------------------------------------------------------------

def test_glx_boundary_stat_is_declared_exported_and_bound():
    from graphlearning_amd import _hip
    hdr = open(os.path.join(ROOT, 'include', 'glx_experimental.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    decl = re.search(r'int glx_boundary_stat\(([^)]*)\);', hdr)
    assert decl and [a.split()[-1].lstrip('*') for a in decl.group(1).split(',')] == \
        ['n', 'd', 'X', 'nnz', 'indptr', 'indices', 'k', 'J', 'flags', 'T', 'nu', 'stats_out', 'device']
    assert 'glx_boundary_stat' not in open(os.path.join(ROOT, 'include', 'glx.h')).read()
    for sym in ('glx_boundary_stat', 'glx_boundary_stat_set_wave_row'):
        assert sym in _hip.EXPORTED_SYMBOLS and sym in _hip._SIGNATURES
        assert getattr(_hip.load(), sym) is not None
    assert list(inspect.signature(_hip.boundary_stat).parameters) == ['X', 'indptr', 'indices', 'second_order', 'cutoff', 'J', 'device']
    assert (_hip.BSTAT_SECOND_ORDER, _hip.BSTAT_CUTOFF) == (1, 2)
    assert re.search(r'#define GLX_BSTAT_SECOND_ORDER 1\b', hdr) and re.search(r'#define GLX_BSTAT_CUTOFF 2\b', hdr)


def test_public_signature_is_the_reference_s_plus_device():
    import graphlearning_amd as gl
    params = inspect.signature(gl.utils.boundary_statistic).parameters
    assert list(params) == ['X', 'r', 'knn', 'return_normals', 'second_order', 'cutoff', 'knn_data', 'device']
    assert [params[p].default for p in list(params)[2:]] == [False, False, True, True, None, None]


@pytest.fixture
def no_library(monkeypatch):
    """any call into the library fails the test"""
    from graphlearning_amd import _hip

    def boom(*a, **k):
        raise AssertionError('the library was called')
    monkeypatch.setattr(_hip, 'load', boom)
    monkeypatch.setattr(_hip, 'boundary_stat', boom)


def test_refusals_come_before_any_library_call(no_library):
    import graphlearning_amd as gl
    bs = gl.utils.boundary_statistic
    X = np.random.default_rng(0).random((30, 2))
    for bad in (np.nan, np.inf, -np.inf):
        Y = X.copy()
        Y[7, 1] = bad
        for knn in (False, True):
            with pytest.raises(ValueError, match='finite'):
                bs(Y, 5 if knn else 0.3, knn=knn)
    for r in (-1.0, float('nan'), -1e-300, None, '0.3', [0.3], True):
        with pytest.raises(ValueError, match='radius'):
            bs(X, r)
    Jw, Dw = ref.knn_lists(np.random.default_rng(1).random((1100, 1)), 1030)
    with pytest.raises(ValueError, match='knn_data'):           # lists wider than min(n, 1024)
        bs(np.random.default_rng(1).random((1100, 1)), 5, knn=True, knn_data=(Jw, Dw))
    for k in (2.5, '5', None, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='integer'):
            bs(X, k, knn=True)
    for k in (1, 0, -3, 31, 2000):
        with pytest.raises(ValueError, match='outside'):
            bs(X, k, knn=True)
    with pytest.raises(ValueError, match='outside'):
        bs(np.random.default_rng(1).random((1100, 1)), 1025, knn=True)
    J, D = ref.knn_lists(X, 6)
    for knn_data in ((J[:, :4], D[:, :4]), (J[:20], D[:20]), (J, D[:, :5]), (J.astype(np.float64), D)):
        with pytest.raises(ValueError, match='knn_data'):
            bs(X, 5, knn=True, knn_data=knn_data)
    for v in (30, -1, 1 << 40):
        Jb = J.copy()
        Jb[3, 2] = v
        with pytest.raises(ValueError, match='index'):
            bs(X, 5, knn=True, knn_data=(Jb, D))
    Jb = J.copy()
    Jb[3, 2] = Jb[3, 1]
    with pytest.raises(ValueError, match='twice'):
        bs(X, 5, knn=True, knn_data=(Jb, D))
    with pytest.raises(ValueError):
        bs(X[:, 0], 0.3)


def test_graph_refusals_come_before_the_statistic_s_call(monkeypatch):
    """A vertex with no neighbour and a weight other than 1 show only in the graph: with the graph constructors replaced by host
    stand-ins, the refusals fire before the statistic's library call."""
    import graphlearning_amd as gl
    from graphlearning_amd import _hip

    def boom(*a, **k):
        raise AssertionError('the library was called')
    monkeypatch.setattr(_hip, 'load', boom)
    monkeypatch.setattr(_hip, 'boundary_stat', boom)
    X = np.random.default_rng(0).random((30, 2))
    X[11] = [5.0, 5.0]

    def ball(data, epsilon, kernel='gaussian', **kw):
        assert kernel == 'uniform'
        indptr, indices = ref.ball_pattern(data, epsilon)
        return sparse.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(len(data),) * 2)
    monkeypatch.setattr(gl.weightmatrix, 'epsilon_ball', ball)
    with pytest.raises(ValueError, match='vertex 11 has no neighbour'):
        gl.utils.boundary_statistic(X, 0.4)

    def twos(data, epsilon, kernel='gaussian', **kw):
        W = ball(data, epsilon, kernel)
        W.data[5] = 2.0
        return W
    monkeypatch.setattr(gl.weightmatrix, 'epsilon_ball', twos)
    with pytest.raises(ValueError, match='other than 1'):
        gl.utils.boundary_statistic(X[:10], 0.6)
