"""graph.peikonal, graph._peikonal_batch, ssl.peikonal and _hip.peikonal on the device.  p = 1: the device against the reference's
golden vectors bit for bit wherever the fixture marks the case `exact` (f > 0 everywhere; the cases whose f holds exact zeros are held
to their recorded 16 x delta, see tests/golden/make_golden_peikonal.py), and against peik_host_reference (csrc/peik_plan.h built on
the host) bit for bit, rounds included, on EVERY p = 1 case.  p != 1: within the recorded bound of the case's (p, num_bisection_it)
class of the golden vectors and of the restatement (the distances are printed).  The batch against single calls, the shapes where the
kernel can go wrong, the cap on the rounds through the test hook, and the learner against the reference's prob and predict().

Every test runs under a time limit of its own: a test that exceeds it ends the whole session on the spot (traceback of every
thread, then exit), so nothing more is started on a device that may have hung; nothing is retried."""
import faulthandler
import os
import sys

import numpy as np
import pytest
from scipy import sparse

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import peik_ref as ref  # noqa: E402
from test_peikonal_host import same_bits, path_graph, FITS  # noqa: E402

pytestmark = pytest.mark.gpu


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
def gold():
    return ref.load_golden()


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return ref.build_host_lib(tmp_path_factory.mktemp('peik_plan'))


def run_case(gl, gold, name):
    c = ref.case(gold, name)
    G = gl.graph(ref.graph(gold, c['graph']))
    f = c['f'] if c['f'].ndim else float(c['f'])
    u = G.peikonal(c['bdy'], bdy_val=c['g'], f=f, p=c['p'], nl_bdy=c['nl_bdy'], u0=c['u0'] if c['has_u0'] else None,
                   num_bisection_it=c['nbis'])
    return c, u, G.peikonal_rounds


def test_p1_bit_for_bit(gl, gold, lib):
    """every p = 1 case: the host restatement's bits and rounds; the reference's bits where the fixed point is its result"""
    names = [n for n in ref.case_names(gold) if ref.case(gold, n)['p'] == 1]
    assert {ref.case(gold, n)['graph'] for n in names if ref.case(gold, n)['exact']} >= {'blobs', 'moons', 'path', 'grid', 'directed',
                                                                                        'twocomp', 'star', 'loops'}
    for name in names:
        c, u, rounds = run_case(gl, gold, name)
        _, W, bdy, g, f, u0 = ref.case_problem(gold, name)
        rc, want, want_rounds = ref.host_solve(lib, W, f, [bdy], [g], 1, c['nbis'], u0=u0)
        print(name, 'rounds', rounds, 'differing from the restatement', int((u != want[:, 0]).sum()), 'from the reference', int((u != c['u']).sum()))
        assert rc == 0 and same_bits(u, want[:, 0].copy()) and rounds == want_rounds == c['rounds'], name
        if c['exact']:
            assert same_bits(u, c['u']), name
        else:
            assert np.abs(u - c['u']).max() / np.abs(c['u']).max() <= ref.bound(gold, 1, c['nbis']), name


def test_bisection_cases_within_the_recorded_bound(gl, gold, lib):
    """p != 1: the device's pow is not the host's, so both distances are held to 16 x the distance between the restatement and the
    reference that the fixture records for the class.  For p < 1 that distance is of the size of u itself (the marching pass's values
    depend on its schedule there, csrc/peik_plan.h) and the class bound says nothing: device and restatement, the same algorithm, are
    held there to the bound of the p = 2 class with the same number of halvings -- the resolution of a bisection relative to its
    bracket is 2^-halvings whatever p."""
    names = [n for n in ref.case_names(gold) if ref.case(gold, n)['p'] != 1]
    assert {(ref.case(gold, n)['p'], ref.case(gold, n)['nbis']) for n in names} == {(p, b) for p in (2.0, 1.5, 0.5) for b in (30, 60)}
    for name in names:
        c, u, rounds = run_case(gl, gold, name)
        _, W, bdy, g, f, u0 = ref.case_problem(gold, name)
        rc, want, want_rounds = ref.host_solve(lib, W, f, [bdy], [g], c['p'], c['nbis'], u0=u0)
        scale = np.abs(c['u']).max()
        d_ref, d_host = np.abs(u - c['u']).max() / scale, np.abs(u - want[:, 0]).max() / scale
        bound = ref.bound(gold, c['p'], c['nbis'])
        print('%-22s rounds %d (restatement %d) from the reference %.3g from the restatement %.3g bound %.3g' % (name, rounds, want_rounds,
                                                                                                                 d_ref, d_host, bound))
        assert rc == 0 and np.all(np.isfinite(u))
        assert d_ref <= bound and d_host <= bound, name
        if c['p'] < 1:
            assert d_host <= ref.bound(gold, 2, c['nbis']), name


def test_batch_equals_single_calls(gl, gold):
    G = gl.graph(ref.graph(gold, 'blobs'))
    rng = np.random.default_rng(5)
    sets = [np.sort(rng.choice(600, size=m, replace=False)) for m in (1, 4, 9)]
    vals = [rng.uniform(-1, 1, size=len(s)) for s in sets]
    f = rng.uniform(0.5, 1.5, size=600)
    for p in (1, 2):
        u = G._peikonal_batch(sets, vals, f=f, p=p)
        rounds = G.peikonal_rounds
        again = G._peikonal_batch(sets, vals, f=f, p=p)
        assert same_bits(u, again) and G.peikonal_rounds == rounds
        single_rounds = []
        for b in range(3):
            one = G.peikonal(sets[b], bdy_val=vals[b], f=f, p=p)
            single_rounds.append(G.peikonal_rounds)
            assert same_bits(np.ascontiguousarray(u[:, b]), one), (p, b)
        assert rounds == max(single_rounds)


def ring_graph(n, seed):
    """a ring with chords and random weights; vertex n - 1 only has its own loop when n == 1"""
    if n == 1:
        return sparse.csr_matrix(np.array([[2.0]]))
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    rows = np.concatenate([i, (i + 1) % n, i, (i + 5) % n])
    cols = np.concatenate([(i + 1) % n, i, (i + 5) % n, i])
    w = rng.uniform(0.5, 1.5, size=2 * n)
    W = sparse.coo_matrix((np.concatenate([w[:n], w[:n], w[n:], w[n:]]), (rows, cols)), shape=(n, n)).tocsr()
    W.sum_duplicates()
    return W


@pytest.mark.parametrize('n,B', [(1, 1), (65, 1), (65, 4), (257, 3), (301, 5)])
def test_sizes_and_rows_bit_for_bit(gl, gold, lib, n, B):
    """one vertex; just past a wavefront; more than one workgroup with values of one vertex in two workgroups (257 x 3); the hub with
    300 neighbours in five problems"""
    W = ref.graph(gold, 'star') if n == 301 else ring_graph(n, n)
    rng = np.random.default_rng(n + B)
    sets = [np.sort(rng.choice(n, size=min(n, 1 + b), replace=False)) for b in range(B)]
    vals = [rng.uniform(0.1, 1, size=len(s)) for s in sets]
    f = rng.uniform(0.5, 1.5, size=n)
    u0 = rng.uniform(-2, 2, size=n)
    G = gl.graph(W)
    u = G._peikonal_batch(sets, vals, f=f, u0=u0)
    rc, want, want_rounds = ref.host_solve(lib, W, f, sets, vals, 1, 30, u0=u0)
    assert rc == 0 and same_bits(u, want) and G.peikonal_rounds == want_rounds
    u2 = G._peikonal_batch(sets, vals, f=f, u0=u0, p=2)
    rc, want2, _ = ref.host_solve(lib, W, f, sets, vals, 2, 30, u0=u0)
    d = np.abs(u2 - want2).max() / np.abs(want2).max()
    print(n, B, 'p = 2 from the restatement', d)
    assert rc == 0 and d <= ref.bound(gold, 2, 30)


def test_unreached_neighbours_and_duplicates(gl, lib):
    """a vertex all of whose neighbours are unreached, a vertex whose only entry is its own loop, a vertex listed twice"""
    A = sparse.csr_matrix(np.array([[0, 1, 0, 0, 0], [1, 0, 0, 0, 0], [0, 0, 0, 1, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, 2.0]]))
    G = gl.graph(A)
    u = G.peikonal([0], bdy_val=1.0, u0=np.full(5, 9.0))
    assert np.array_equal(u, [1, 2, 9, 9, 9]) and G.peikonal_rounds == 2
    assert np.array_equal(G.peikonal([0], bdy_val=1.0), [1, 2, 0, 0, 0])
    P = gl.graph(path_graph(7))
    assert np.array_equal(P.peikonal([0, 6]), [0, 1, 2, 2.5, 2, 1, 0]) and P.peikonal_rounds == 4
    assert np.array_equal(P.peikonal([0, 6, 0], bdy_val=np.array([5.0, 0.0, 0.0])), [0, 1, 2, 2.5, 2, 1, 0])


def test_round_cap_through_the_hook(gl):
    """the cap is reached on the host side of the loop: the call enqueues max_rounds rounds, reads their flags and refuses"""
    from graphlearning_amd import _hip
    P = gl.graph(path_graph(7))
    with pytest.raises(_hip.GlxError, match='still fall after 3 rounds'):
        P._peikonal_batch([[0, 6]], 0, max_rounds=3)
    assert np.array_equal(P._peikonal_batch([[0, 6]], 0, max_rounds=4)[:, 0], [0, 1, 2, 2.5, 2, 1, 0])
    long = gl.graph(path_graph(80))                      # more rounds than one chunk of 32
    with pytest.raises(_hip.GlxError, match='still fall after 40 rounds'):
        long._peikonal_batch([[0]], 0, max_rounds=40)
    assert np.array_equal(long.peikonal([0]), np.arange(80.0)) and long.peikonal_rounds == 80


def test_learner_against_the_golden(gl, gold):
    for gname in ('blobs', 'moons'):
        W = ref.graph(gold, gname)
        truth = gold['graph_%s_truth' % gname].astype(np.int64)
        priors = gold['fit_%s_priors' % gname]
        kws = dict(p1=dict(p=1), p2=dict(p=2), p1_priors=dict(p=1, class_priors=priors), p2_priors=dict(p=2, class_priors=priors),
                   D=dict(p=1, D=W, alpha=2), eps=dict(p=2, eps_ball_graph=True, alpha=0.5))
        for tag in FITS:
            key = 'fit_%s_%s' % (gname, tag)
            ind = gold[key + '_train_ind']
            model = gl.ssl.peikonal(W, **kws[tag])
            pred = model.fit_predict(ind, truth[ind])
            prob, want = model.prob, gold[key + '_prob']
            if kws[tag]['p'] == 1:
                assert same_bits(np.ascontiguousarray(prob), want), key
                assert model.num_iter == int(gold[key + '_rounds'].max())
            else:
                d = np.abs(prob - want).max() / np.abs(want).max()
                print(key, 'from the reference', d)
                assert d <= ref.bound(gold, 2, 30), key
            assert np.array_equal(pred, gold[key + '_pred']), key


def test_ssl_trials(gl, gold, tmp_path, monkeypatch):
    W = ref.graph(gold, 'blobs')
    truth = gold['graph_blobs_truth'].astype(np.int64)
    ind = gold['fit_blobs_p1_train_ind']
    rng = np.random.default_rng(3)
    other = np.concatenate([rng.choice(np.where(truth == c)[0], size=2, replace=False) for c in np.unique(truth)])
    monkeypatch.setattr(gl.ssl, 'results_dir', str(tmp_path / 'results'))
    model = gl.ssl.peikonal(W)
    model.ssl_trials([other, ind], truth, tag='pe_')
    lines = (tmp_path / 'results' / 'pe__peikonal_p1.00_alpha1.00_accuracy.csv').read_text().splitlines()
    assert lines[0] == 'Number of labels,Accuracy' and len(lines) == 3
    acc = gl.ssl.ssl_accuracy(gold['fit_blobs_p1_pred'], truth, ind)
    assert lines[2] == '%d,%.2f' % (len(ind), acc)
    assert model.trials_statistics(tag='pe_')[0].tolist() == sorted([len(other), len(ind)])
