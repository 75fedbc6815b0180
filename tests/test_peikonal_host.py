"""The p-eikonal solver without a device: csrc/peik_plan.h compiled for the host (tests/peik_plan_host.cpp) against the reference's
golden vectors -- bit for bit where the fixture says the fixed point is the marching solver's result (p = 1, f > 0), within the
recorded 16 x delta of the case's (p, num_bisection_it) class elsewhere --, a 7-vertex path against values written out by hand, every
code of peik_validate, the refusals of graph.peikonal and ssl.peikonal (all raised before any library call), the batch against single
problems, an unreached component, graph.peikonal and ssl.peikonal end to end with the host restatement in place of the device call,
the declaration of the entry point, and the stand-alone program under the host's address and undefined-behaviour sanitizers.

Regenerate the fixture with tests/golden/make_golden_peikonal.py (it needs the reference)."""
import os
import re
import subprocess
import sys
import numpy as np
import pytest
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import peik_ref as ref              # noqa: E402
import graphlearning_amd as gl      # noqa: E402
from graphlearning_amd import _hip  # noqa: E402

GRAPHS = ('blobs', 'moons', 'path', 'grid', 'directed', 'twocomp', 'star', 'loops')
FITS = ('p1', 'p2', 'p1_priors', 'p2_priors', 'D', 'eps')


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope='module')
def gold():
    return ref.load_golden()


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return ref.build_host_lib(tmp_path_factory.mktemp('peik_plan'))


def path_graph(n):
    r = np.arange(n - 1)
    return sparse.csr_matrix((np.ones(2 * (n - 1)), (np.concatenate([r, r + 1]), np.concatenate([r + 1, r]))), shape=(n, n))


def test_the_fixture_is_what_the_tests_need(gold):
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', ref.GOLDEN_FILE)) < os.path.getsize(
        os.path.join(ROOT, 'tests', 'golden', 'g3_blobs5000.npz'))
    names = ref.case_names(gold)
    seen = set()
    for name in names:
        c = ref.case(gold, name)
        seen.add((c['graph'], c['p']))
        assert np.all(c['g'] != 0) and c['u'].shape == (ref.graph(gold, c['graph']).shape[0],)
        if c['p'] == 1 and np.min(c['f']) > 0:
            assert bool(gold['case_%s_exact' % name])
    assert seen >= {(g, p) for g in GRAPHS for p in (1.0, 2.0, 1.5, 0.5)}
    assert {int(ref.case(gold, n)['nbis']) for n in names} == {30, 60}
    assert any(ref.case(gold, n)['nl_bdy'] for n in names) and any(ref.case(gold, n)['has_u0'] for n in names)
    assert any(ref.case(gold, n)['f'].ndim == 1 and (ref.case(gold, n)['f'] == 0).any() for n in names)
    assert np.array_equal(gold['class_bound'], 16 * gold['class_delta']) and np.all(gold['class_delta'] > 0)
    for p, nbis, want in ((2.0, 30, 1e-7), (1.5, 30, 1e-7), (2.0, 60, 1e-13), (1.5, 60, 1e-13), (1.0, 30, 1e-13), (1.0, 60, 1e-13)):
        assert ref.bound(gold, p, nbis) < want, (p, nbis)
    assert np.diff(ref.graph(gold, 'star').indptr).max() == 300 and (ref.graph(gold, 'loops').diagonal() != 0).sum() == 4
    Wd = ref.graph(gold, 'directed')
    assert (abs(Wd - Wd.T) > 0).nnz > 0


def test_restatement_against_the_golden(gold, lib):
    """every case: bits where the fixture says so, the class's bound elsewhere; the rounds are the recorded ones"""
    for name in ref.case_names(gold):
        c, W, bdy, g, f, u0 = ref.case_problem(gold, name)
        rc, u, rounds = ref.host_solve(lib, W, f, [bdy], [g], c['p'], c['nbis'], u0=u0)
        assert rc == 0 and rounds == c['rounds'], (name, rc, rounds, c['rounds'])
        if bool(gold['case_%s_exact' % name]):
            assert same_bits(u[:, 0].copy(), c['u']), name
        else:
            err = np.abs(u[:, 0] - c['u']).max() / np.abs(c['u']).max()
            assert err <= ref.bound(gold, c['p'], c['nbis']), (name, err)


def test_path_by_hand(lib):
    """unit path 0 - 1 - .. - 6, both ends at 0, f = 1, p = 1: a vertex next to one smaller neighbour takes its value + 1, the middle
    vertex solves (1 + 2 + 2) / 2 from both neighbours at 2"""
    W = path_graph(7)
    rc, u, rounds = ref.host_solve(lib, W, 1.0, [np.array([0, 6])], [np.zeros(2)], 1, 30)
    assert rc == 0 and rounds == 4 and np.array_equal(u[:, 0], [0, 1, 2, 2.5, 2, 1, 0])
    # one end at 0.25, f = 2, weights 4: steps of f / w = 0.5
    rc, u, rounds = ref.host_solve(lib, 4 * W, 2.0, [np.array([0])], [np.array([0.25])], 1, 30)
    assert rc == 0 and rounds == 7 and np.array_equal(u[:, 0], 0.25 + 0.5 * np.arange(7))
    # p = 2, 60 halvings: (t - u)^2 w = f from the one smaller neighbour, steps of sqrt(f / w) = 0.5
    rc, u, _ = ref.host_solve(lib, 4 * W, 1.0, [np.array([0])], [np.array([0.25])], 2, 60)
    assert rc == 0 and np.abs(u[:, 0] - (0.25 + 0.5 * np.arange(7))).max() < 1e-14


def test_every_refusal_of_the_checker(lib):
    W = path_graph(7)
    n = 7
    row_ptr, nbr, V = ref.entries(W)
    ok = dict(f=1.0, bdy_sets=[np.array([0, 6])], bdy_vals=[np.array([0.5, 1.0])], p=1.0, nbis=30)

    def code(row_ptr=row_ptr, nbr=nbr, V=V, n=n, **kw):
        a = dict(ok, **kw)
        return ref.host_validate(lib, n, row_ptr, nbr, V, a['f'], a['bdy_sets'], a['bdy_vals'], a['p'], a['nbis'], u0=a.get('u0'), B=a.get('B'),
                                 M=a.get('M'))
    assert code() == 0
    assert code(M=-1) == 1 and code(M=len(nbr) - 1) == 1
    bad = row_ptr.copy()
    bad[3] = bad[2] - 1
    assert code(row_ptr=bad) == 1
    for v in (-1, n):
        bad = nbr.copy()
        bad[4] = v
        assert code(nbr=bad) == 1
    assert code(bdy_sets=[np.array([0, 7])]) == 2 and code(bdy_sets=[np.array([-1, 6])]) == 2
    assert code(bdy_sets=[np.array([0, 6]), np.zeros(0, dtype=np.int64)], bdy_vals=[np.array([0.5, 1.0]), np.zeros(0)]) == 3
    for w in (0.0, -1.0, np.nan, np.inf):
        bad = V.copy()
        bad[5] = w
        assert code(V=bad) == 4
    for x in (-1e-300, np.nan, np.inf):
        f = np.ones(n)
        f[2] = x
        assert code(f=f) == 5
    assert code(f=np.zeros(n)) == 0
    for x in (np.nan, np.inf, -np.inf):
        assert code(bdy_vals=[np.array([0.5, x])]) == 6
        u0 = np.zeros(n)
        u0[6] = x
        assert code(u0=u0) == 6
    assert code(bdy_vals=[np.array([-0.5, 1.0])]) == 0
    for p in (0.0, -1.0, np.nan, np.inf):
        assert code(p=p) == 7
    assert code(nbis=0) == 8 and code(nbis=129) == 8 and code(nbis=128) == 0 and code(nbis=1) == 0
    assert code(B=0) == 9 and code(B=257) == 9
    big = 1 << 24                                        # 2^24 vertices x 256 problems > 2^31; nothing is read behind the size checks
    assert ref.host_validate(lib, big, np.zeros(1, dtype=np.int64), nbr, V, 1.0, ok['bdy_sets'], ok['bdy_vals'], 1.0, 30, u0=np.zeros(1), B=256,
                             M=0) == 10
    const = np.zeros(6, dtype=np.int64)
    lib.peik_host_constants(const.ctypes.data)
    assert list(const) == [256, 128, 1 << 31, ref.ECAP, 202, 442]


def test_batch_columns_equal_single_problems(gold, lib):
    W = ref.graph(gold, 'blobs')
    rng = np.random.default_rng(5)
    sets = [np.sort(rng.choice(600, size=m, replace=False)) for m in (1, 4, 9)]
    vals = [rng.uniform(-1, 1, size=len(s)) for s in sets]
    f = rng.uniform(0.5, 1.5, size=600)
    for p, nbis in ((1, 30), (2, 30)):
        rc, u, rounds = ref.host_solve(lib, W, f, sets, vals, p, nbis)
        assert rc == 0
        singles = [ref.host_solve(lib, W, f, [s], [v], p, nbis) for s, v in zip(sets, vals)]
        assert rounds == max(s[2] for s in singles)
        for b in range(3):
            assert singles[b][0] == 0 and same_bits(u[:, b].copy(), singles[b][1][:, 0].copy()), (p, b)
    # a vertex listed twice takes its last value
    rc, u, _ = ref.host_solve(lib, W, 1.0, [np.array([3, 10, 3])], [np.array([5.0, 1.0, 0.5])], 1, 30)
    rc2, u2, _ = ref.host_solve(lib, W, 1.0, [np.array([10, 3])], [np.array([1.0, 0.5])], 1, 30)
    assert rc == 0 and rc2 == 0 and u[3, 0] == 0.5 and same_bits(u, u2)


def test_unreached_component_and_round_cap(gold, lib):
    W = ref.graph(gold, 'twocomp')
    u0 = np.arange(17) * 0.5 - 3
    rc, u, rounds = ref.host_solve(lib, W, 1.0, [np.array([2])], [np.array([0.25])], 1, 30, u0=u0)
    assert rc == 0 and np.array_equal(u[12:, 0], u0[12:]) and np.all(u[:12, 0] >= 0.25) and np.all(np.isfinite(u))
    rc, u, _ = ref.host_solve(lib, W, 1.0, [np.array([2])], [np.array([0.25])], 1, 30)
    assert rc == 0 and np.all(u[12:, 0] == 0)
    # a vertex all of whose neighbours are unreached, and one whose only entry is its own loop
    A = sparse.csr_matrix(np.array([[0, 1, 0, 0, 0], [1, 0, 0, 0, 0], [0, 0, 0, 1, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, 2.0]]))
    rc, u, rounds = ref.host_solve(lib, A, 1.0, [np.array([0])], [np.array([1.0])], 1, 30, u0=np.full(5, 9.0))
    assert rc == 0 and rounds == 2 and np.array_equal(u[:, 0], [1, 2, 9, 9, 9])
    # the cap: the path of 7 needs 4 rounds
    P = path_graph(7)
    rc, u, rounds = ref.host_solve(lib, P, 1.0, [np.array([0, 6])], [np.zeros(2)], 1, 30, max_rounds=3)
    assert rc == ref.ECAP and rounds == 3
    rc, u, rounds = ref.host_solve(lib, P, 1.0, [np.array([0, 6])], [np.zeros(2)], 1, 30, max_rounds=4)
    assert rc == 0 and rounds == 4


def host_device(lib):
    """_hip.peikonal with the host restatement behind it"""
    def peikonal(row_ptr, nbr, W, f, bdy_ptr, bdy_idx, bdy_val, p, num_bisection_it, u0, device=None, max_rounds=0):
        n, B = len(row_ptr) - 1, len(bdy_ptr) - 1
        u = np.empty((n, B))
        import ctypes
        rounds = ctypes.c_int64(0)
        arrs = [np.ascontiguousarray(a, dtype=t) for a, t in ((row_ptr, np.int64), (nbr, np.int32), (W, np.float64), (f, np.float64),
                                                               (bdy_ptr, np.int64), (bdy_idx, np.int32), (bdy_val, np.float64), (u0, np.float64))]
        q = [a.ctypes.data for a in arrs]
        rc = lib.peik_host_solve(n, len(nbr), q[0], q[1], q[2], q[3], B, q[4], q[5], q[6], float(p), int(num_bisection_it), q[7], int(max_rounds),
                                 u.ctypes.data, ctypes.byref(rounds))
        if rc:
            raise _hip.GlxError('glx_peikonal failed (%d)' % rc)
        return u, int(rounds.value)
    return peikonal


def test_graph_peikonal_on_the_host_restatement(gold, lib, monkeypatch):
    """graph.peikonal's preparation (the entry arrays, f, nl_bdy, u0) around the host form of the device call: the golden cases"""
    monkeypatch.setattr(_hip, 'peikonal', host_device(lib))
    for name in ref.case_names(gold):
        c = ref.case(gold, name)
        if c['graph'] in ('blobs', 'moons') and not (c['nl_bdy'] or c['p'] == 1):
            continue                                     # the long bisection cases ran once above
        G = gl.graph(ref.graph(gold, c['graph']))
        f = c['f'] if c['f'].ndim else float(c['f'])
        u = G.peikonal(c['bdy'], bdy_val=c['g'], f=f, p=c['p'], nl_bdy=c['nl_bdy'], u0=c['u0'] if c['has_u0'] else None,
                       num_bisection_it=c['nbis'])
        assert G.peikonal_rounds == c['rounds'], name
        if bool(gold['case_%s_exact' % name]):
            assert same_bits(u, c['u']), name
        else:
            assert np.abs(u - c['u']).max() / np.abs(c['u']).max() <= ref.bound(gold, c['p'], c['nbis']), name
    G = gl.graph(ref.graph(gold, 'grid'))
    mask = np.zeros(36, dtype=bool)
    mask[[0, 35]] = True
    assert same_bits(G.peikonal(mask, bdy_val=[0.5, 1.0]), G.peikonal([0, 35], bdy_val=np.array([0.5, 1.0])))
    ub = G._peikonal_batch([[0, 35], mask, [7]], [np.array([0.5, 1.0]), 0.25, 0], f=2.0)
    assert same_bits(ub[:, 1].copy(), G.peikonal(mask, bdy_val=0.25, f=2.0)) and same_bits(ub[:, 2].copy(), G.peikonal([7], f=2.0))


def test_learner_on_the_host_restatement(gold, lib, monkeypatch):
    monkeypatch.setattr(_hip, 'peikonal', host_device(lib))
    for gname in ('blobs', 'moons'):
        W = ref.graph(gold, gname)
        truth = gold['graph_%s_truth' % gname].astype(np.int64)
        priors = gold['fit_%s_priors' % gname]
        kws = dict(p1=dict(p=1), p2=dict(p=2), p1_priors=dict(p=1, class_priors=priors), p2_priors=dict(p=2, class_priors=priors),
                   D=dict(p=1, D=W, alpha=2), eps=dict(p=2, eps_ball_graph=True, alpha=0.5))
        for tag in FITS:
            if 'priors' in tag:                          # the projection onto the priors runs on the device: tests/test_gpu_peikonal.py
                continue
            key = 'fit_%s_%s' % (gname, tag)
            ind = gold[key + '_train_ind']
            model = gl.ssl.peikonal(W, **kws[tag])
            assert model.name == str(gold[key + '_name']) and model.accuracy_filename == str(gold[key + '_file'])
            assert model.onevsrest is True and model.similarity is False
            prob = model.fit(ind, truth[ind])
            want = gold[key + '_prob']
            if kws[tag]['p'] == 1:
                assert same_bits(prob, want), key
            else:
                assert np.abs(prob - want).max() / np.abs(want).max() <= ref.bound(gold, 2, 30), key
            assert np.array_equal(np.argmin(prob, axis=1), gold[key + '_pred']), key          # (predict() itself runs on the device)
            assert model.num_iter == int(gold[key + '_rounds'].max())
            if tag == 'p1':                              # class by class through graph.peikonal: the same columns
                cols = [model._fit(ind, truth[ind] == l) for l in np.unique(truth[ind])]
                assert same_bits(np.stack(cols, axis=1), want)


def test_value_errors_before_any_library_call(monkeypatch, gold):
    calls = []

    def no_device(*a, **k):
        calls.append((a, k))
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_hip, 'peikonal', no_device)
    monkeypatch.setattr(_hip, 'call', no_device)
    W = ref.graph(gold, 'grid')
    n = 36
    G = gl.graph(W)
    with pytest.raises(AssertionError):                  # the accepted input gets as far as the library ..
        G.peikonal([0, 35], bdy_val=[0.5, 1.0], f=2, p=1.5, num_bisection_it=40, u0=np.ones(n))
    (row_ptr, nbr, V, f, bptr, bidx, bval, p, nbis, u0), kw = calls[0]
    want_ptr, want_nbr, want_V = ref.entries(W)          # .. with the reference's entry arrays
    assert np.array_equal(row_ptr, want_ptr) and np.array_equal(nbr, want_nbr) and same_bits(np.asarray(V), want_V)
    assert np.array_equal(f, np.full(n, 2.0)) and list(bptr) == [0, 2] and list(bidx) == [0, 35] and list(bval) == [0.5, 1.0]
    assert (p, nbis) == (1.5, 40) and np.array_equal(u0, np.ones(n)) and kw['max_rounds'] == 0
    with pytest.raises(NotImplementedError, match='level schedule'):
        G.peikonal([0], solver='gauss-seidel')
    with pytest.raises(ValueError, match='unknown solver'):
        G.peikonal([0], solver='heap')
    with pytest.raises(ValueError, match='boundary values for'):
        G.peikonal([0, 35], bdy_val=np.array([1.0, 2.0, 3.0]))
    with pytest.raises(ValueError, match='boundary values for'):
        G.peikonal(np.arange(n) < 2, bdy_val=[1.0])
    with pytest.raises(ValueError, match='empty boundary'):
        G.peikonal(np.zeros(0, dtype=np.int64))
    with pytest.raises(ValueError, match='empty boundary'):
        G._peikonal_batch([[0], np.zeros(n, dtype=bool)])
    for bad in ([0, n], [-1, 3]):
        with pytest.raises(ValueError, match='out of range'):
            G.peikonal(bad)
        with pytest.raises(ValueError, match='out of range'):
            G.peikonal(bad, nl_bdy=True)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match='bdy_val'):
            G.peikonal([0, 35], bdy_val=[0.5, bad])
        with pytest.raises(ValueError, match='u0'):
            G.peikonal([0], u0=np.where(np.arange(n) == 4, bad, 0.0))
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match='f has an entry'):
            G.peikonal([0], f=bad)
        with pytest.raises(ValueError, match='f has an entry'):
            G.peikonal([0], f=np.where(np.arange(n) == 4, bad, 1.0))
    with pytest.raises(ValueError, match='f has shape'):
        G.peikonal([0], f=np.ones(n + 1))
    with pytest.raises(ValueError, match='u0 has shape'):
        G.peikonal([0], u0=np.ones(n - 1))
    for bad in (0, -2, np.nan, np.inf):
        with pytest.raises(ValueError, match='p='):
            G.peikonal([0], p=bad)
        with pytest.raises(ValueError, match='p='):
            gl.ssl.peikonal(W, p=bad)
    for bad in (0, 129, 2.5, -1):
        with pytest.raises(ValueError, match='num_bisection_it'):
            G.peikonal([0], num_bisection_it=bad)
        with pytest.raises(ValueError, match='num_bisection_it'):
            gl.ssl.peikonal(W, num_bisection_it=bad)
    with pytest.raises(ValueError, match='boundary sets'):
        G._peikonal_batch([])
    with pytest.raises(ValueError, match='boundary sets'):
        G._peikonal_batch([[0]] * 257)
    with pytest.raises(ValueError, match='boundary value entries'):
        G._peikonal_batch([[0], [1]], [0.5])
    for bad in (-1.0, np.nan, np.inf):                   # (an explicit zero is no entry: sparse.find drops it)
        Wb = W.copy()
        Wb.data[7] = bad
        with pytest.raises(ValueError, match='weight matrix'):
            gl.graph(Wb).peikonal([0])
        with pytest.raises(ValueError, match='weight matrix'):
            gl.ssl.peikonal(Wb).fit(np.array([0, 35]), np.array([0, 1]))
    with pytest.raises(AssertionError):                  # the learner's accepted input reaches the library too, all classes in one call
        gl.ssl.peikonal(W, p=2).fit(np.array([0, 5, 35]), np.array([0, 1, 1]))
    (_, _, _, f, bptr, bidx, bval, p, nbis, _), _ = calls[-1]
    assert list(bptr) == [0, 1, 3] and list(bidx) == [0, 5, 35] and np.all(bval == 0) and (p, nbis) == (2.0, 30) and np.all(f == 1)
    assert len(calls) == 2


def test_learner_attributes(gold):
    W = ref.graph(gold, 'grid')
    m = gl.ssl.peikonal(W)
    assert (m.p, m.alpha, m.max_num_it, m.tol, m.num_bisection_it, m.f) == (1, 1, 1e5, 1e-3, 30, 1)
    assert m.name == 'p-eikonal (p=1.00, alpha=1.00)' and m.accuracy_filename == '_peikonal_p1.00_alpha1.00'
    assert m.onevsrest is True and m.similarity is False
    m = gl.ssl.peikonal(W, None, W, 2, 0.5, 10, 1e-2, 40, False)          # the reference's positional order
    assert (m.p, m.alpha, m.max_num_it, m.tol, m.num_bisection_it) == (2, 0.5, 10, 1e-2, 40)
    d = np.asarray(W.max(axis=1).todense()).ravel()
    assert same_bits(np.asarray(m.f), (d / d.max()) ** 0.5)
    m = gl.ssl.peikonal(W, eps_ball_graph=True, alpha=2)
    d = W * np.ones(36)
    assert same_bits(np.asarray(m.f), (d / d.max()) ** (-2))


def test_entry_point_is_declared():
    with open(os.path.join(ROOT, 'include', 'glx_experimental.h')) as f:
        text = f.read()
    decl = re.search(r'int glx_peikonal\(([^;]*)\);', text)
    assert decl and decl.group(1).startswith('int64_t n, int64_t M, const int64_t* row_ptr, const int32_t* nbr, const double* W, const double* f, int B,')
    with open(os.path.join(ROOT, 'include', 'glx.h')) as f:
        assert 'glx_peikonal' not in f.read()
    assert 'glx_peikonal' in _hip.EXPORTED_SYMBOLS and callable(_hip.peikonal)
    assert len(_hip._SIGNATURES['glx_peikonal']) == decl.group(1).count(',') + 1 == 18
    assert getattr(_hip.load(), 'glx_peikonal') is not None
    with open(os.path.join(ROOT, 'graphlearning_amd', 'csrc', 'peik_plan.h')) as f:
        plan = f.read()
    assert '#include <hip' not in plan and 'glx_internal.h' not in plan          # host only
    with open(os.path.join(ROOT, 'graphlearning_amd', 'csrc', 'peik.hip')) as f:
        kern = f.read()
    assert not re.search(r'atomic[A-Z]|__hip_atomic|cooperative_groups|fma\(', kern)          # no atomics, no grid wait, no fma


def test_the_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """A program of its own, built with -fsanitize=address,undefined and run on the host; nothing is loaded into Python."""
    exe = ref.build_host_exe(tmp_path, 'peik_plan_main', extra=('-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'))
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith('ok rounds 4 u 2.5 '), (res.returncode, res.stdout, res.stderr)
