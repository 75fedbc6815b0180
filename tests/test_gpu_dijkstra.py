"""graph.dijkstra, graph.dijkstra_hl, graph.distance, graph.distance_matrix and ssl.graph_nearest_neighbor on the device: the
golden vectors of the compiled reference bit for bit (distances and closest points), a randomised sweep against the restatement
tests/dijkstra_ref.py, the grid where ties are everywhere, the degenerate graphs, the batched form against single calls, the path
walk, the learner against the golden fits and one input at scale against scipy.

Every test runs under a time limit of its own: a test that exceeds it ends the whole session on the spot (traceback of every
thread, then exit), so nothing more is started on a device that may have hung; nothing is retried."""
import faulthandler
import os
import sys

import numpy as np
import pytest
from scipy import sparse
from scipy.sparse import csgraph

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dijkstra_ref as ref  # noqa: E402
from test_dijkstra_host import load_golden, golden_graph, golden_case  # noqa: E402

pytestmark = pytest.mark.gpu

TIME_LIMIT = {'test_one_million_points_against_scipy': 900}


@pytest.fixture(autouse=True)
def _time_limit(request):
    faulthandler.dump_traceback_later(TIME_LIMIT.get(request.node.originalname or request.node.name, 240), exit=True)
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
    return load_golden()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run(G, src, g, f, max_dist, hl, recip):
    if hl:
        return G.dijkstra_hl(src, bdy_val=g, f=f, max_dist=max_dist, return_cp=True)
    return G.dijkstra(src, bdy_val=g, f=f, max_dist=max_dist, return_cp=True, reciprocal_weights=recip)


@pytest.mark.parametrize('name', sorted(ref.GOLDEN_CASES))
def test_golden_bit_for_bit(gl, gold, name):
    """Distances and closest points of the compiled reference; inf / -1 exactly where the reference's value exceeds max_dist."""
    W, src, g, f, max_dist, hl, recip, want, raw_cp = golden_case(gold, name)
    G = gl.graph(W)
    dist, cp = run(G, src, g, f, max_dist, hl, recip)
    assert dist.dtype == np.float64 and cp.dtype == np.int32 and dist.shape == (W.shape[0],) and cp.shape == dist.shape
    print(name, 'rounds', G.dijkstra_rounds, 'differing distances', int((dist != want).sum()))
    assert same_bits(dist, want)
    reached = np.isfinite(want)
    raw = gold[name + '_dist']
    assert np.array_equal(np.isinf(dist), (raw > max_dist) | np.isinf(raw))
    assert np.array_equal(cp == -1, np.isinf(dist))
    assert np.array_equal(cp[reached], raw_cp[reached])
    assert (cp[~reached] == -1).all()
    # without the closest point: the same distances
    d_only = G.dijkstra_hl(src, bdy_val=g, f=f, max_dist=max_dist) if hl else G.dijkstra(src, bdy_val=g, f=f, max_dist=max_dist,
                                                                                           reciprocal_weights=recip)
    assert same_bits(d_only, want)


def random_graph(rng, n, deg, sym):
    A = sparse.random(n, n, density=min(1.0, deg / n), random_state=int(rng.integers(1 << 30)), format='csr')
    if sym:
        A = A.maximum(A.T).tocsr()
    return A


def test_randomised_sweep_against_restatement(gl):
    """n, degree, dimension, directed and symmetric graphs, number of sources, f, max_dist, both relaxations, reciprocal weights."""
    rng = np.random.default_rng(2024)
    for trial in range(40):
        kind = trial % 4
        if kind == 3:         # a kNN graph built on the device
            n = int(rng.integers(50, 3000))
            d = int(rng.choice([2, 3, 20]))
            k = int(rng.integers(3, 15))
            W = gl.weightmatrix.knn(rng.random((n, d)), k, kernel='distance', symmetrize=bool(trial % 8 == 3))
        else:
            n = int(rng.integers(2, 2500))
            W = random_graph(rng, n, float(rng.integers(1, 12)), sym=bool(kind == 1))
        m = int(rng.integers(1, min(n, 9) + 1))
        src = rng.choice(n, size=m, replace=False)
        g = rng.random(m) * float(rng.choice([0.0, 0.1, 1.0]))
        f = [1, 0.6, 0.5 + rng.random(n)][trial % 3]
        hl = bool(trial % 5 == 1)
        recip = bool(trial % 7 == 2) and not hl
        u_inf, _ = ref.dijkstra(W, src, g, f, np.inf, recip, hl)
        fin = u_inf[np.isfinite(u_inf)]
        max_dist = np.inf if trial % 3 == 0 else float(np.quantile(fin, rng.random()))
        want_u, want_cp = ref.dijkstra(W, src, g, f, max_dist, recip, hl)
        dist, cp = run(gl.graph(W), src, g, f, max_dist, hl, recip)
        what = (trial, n, m, hl, recip, max_dist)
        assert same_bits(dist, want_u), what
        assert np.array_equal(cp, want_cp), what


def test_integer_grid_with_ties(gl):
    """Distances bit for bit; the closest point is the restatement's smallest index among the tied sources, and tight-reachable."""
    m = 40
    idx = np.arange(m * m).reshape(m, m)
    rows = np.concatenate([idx[:-1, :].ravel(), idx[:, :-1].ravel()])
    cols = np.concatenate([idx[1:, :].ravel(), idx[:, 1:].ravel()])
    W = sparse.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(m * m, m * m))
    W = (W + W.T).tocsr()
    src = np.array([idx[20, 20], idx[30, 10], idx[10, 10]])
    g = np.zeros(3)
    for hl in (False, True):
        want_u, want_cp = ref.dijkstra(W, src, g, hl=hl)
        dist, cp = run(gl.graph(W), src, g, 1, np.inf, hl, False)
        assert same_bits(dist, want_u)
        assert np.array_equal(cp, want_cp)
    r, c = np.divmod(np.arange(m * m), m)
    man = np.stack([abs(r - sr) + abs(c - sc) for sr, sc in (divmod(int(s), m) for s in src)])
    dist, cp = run(gl.graph(W), src, g, 1, np.inf, False, False)
    assert np.array_equal(dist, man.min(axis=0).astype(np.float64))
    tied = man == man.min(axis=0)[None, :]
    assert (tied.sum(axis=0) > 1).sum() > 100                      # ties are everywhere
    assert np.array_equal(cp, np.array([src[tied[:, v]].min() for v in range(m * m)]))
    # every cp[j] reaches j along tight edges: walking back from j over tight edges with the same cp arrives at the source
    I, J, C = ref.edges(W)
    t = ref._tight(dist, I, J, C, np.inf, False)
    back = {}
    for i, j in zip(I[t], J[t]):
        if cp[i] == cp[j]:
            back.setdefault(int(j), int(i))
    for v in range(m * m):
        p, steps = v, 0
        while p != cp[v]:
            p = back[p]
            steps += 1
            assert steps <= m * m
        assert dist[v] == steps


def test_degenerate_graphs(gl):
    # empty rows and an unreachable component
    W = sparse.lil_matrix((9, 9))
    W[0, 1] = 1.5
    W[1, 2] = 2.5
    W[2, 0] = 0.5
    W[4, 5] = 1.0
    W[5, 4] = 1.0          # 3, 6, 7, 8 have no entry at all; {4, 5} is cut off from {0, 1, 2}
    W[7, 7] = 3.0          # only a diagonal entry
    W = W.tocsr()
    dist, cp = gl.graph(W).dijkstra([0], return_cp=True)
    assert np.array_equal(dist, [0.0, 1.5, 4.0, np.inf, np.inf, np.inf, np.inf, np.inf, np.inf])
    assert np.array_equal(cp, [0, 0, 0, -1, -1, -1, -1, -1, -1])
    want_u, want_cp = ref.dijkstra(W, [0, 5], np.array([0.25, 0.0]))
    dist, cp = gl.graph(W).dijkstra([0, 5], bdy_val=np.array([0.25, 0.0]), return_cp=True)
    assert same_bits(dist, want_u) and np.array_equal(cp, want_cp)
    assert np.array_equal(cp, [0, 0, 0, -1, 5, 5, -1, -1, -1])
    # a matrix without any entry; a single vertex
    dist, cp = gl.graph(sparse.csr_matrix((5, 5))).dijkstra([3], bdy_val=2.0, return_cp=True)
    assert np.array_equal(dist, [np.inf, np.inf, np.inf, 2.0, np.inf]) and np.array_equal(cp, [-1, -1, -1, 3, -1])
    dist, cp = gl.graph(sparse.csr_matrix(np.array([[2.0]]))).dijkstra([0], return_cp=True)
    assert np.array_equal(dist, [0.0]) and np.array_equal(cp, [0])
    dist = gl.graph(sparse.csr_matrix(np.array([[2.0]]))).dijkstra_hl([0], bdy_val=1.0)
    assert np.array_equal(dist, [1.0])
    # all vertices as sources: those whose own value is undercut are dominated, the others keep it
    rng = np.random.default_rng(3)
    A = random_graph(rng, 300, 6, sym=True)
    g = rng.random(300)
    want_u, want_cp = ref.dijkstra(A, np.arange(300), g)
    dist, cp = gl.graph(A).dijkstra(np.arange(300), bdy_val=g, return_cp=True)
    assert same_bits(dist, want_u) and np.array_equal(cp, want_cp)
    assert (dist < g).any() and (dist == g).any()
    # a boolean mask as boundary set, max_dist below every boundary value
    mask = np.zeros(300, dtype=bool)
    mask[[3, 17]] = True
    dist, cp = gl.graph(A).dijkstra(mask, bdy_val=1.0, max_dist=0.5, return_cp=True)
    assert np.isinf(dist).all() and (cp == -1).all()


def test_batched_form_equals_single_calls(gl, monkeypatch):
    """distance_matrix rows == n single calls bit for bit, with one batch and with several; B not a multiple of the wave width;
    problems with different source lists and closest points in one call."""
    graph_mod = sys.modules['graphlearning_amd.graph']          # (the package exposes the class under the module's name)
    rng = np.random.default_rng(8)
    n = 131
    W = gl.weightmatrix.knn(rng.random((n, 2)), 6, kernel='gaussian')
    G = gl.graph(W)
    singles = np.stack([G.dijkstra([i], reciprocal_weights=True) for i in range(n)])
    T = G.distance_matrix()
    assert same_bits(T, singles)
    monkeypatch.setattr(graph_mod, '_DISTANCE_MATRIX_VALUES', n * 37)          # batches of 37, 37, 37, 20
    assert same_bits(G.distance_matrix(), singles)
    Jc = np.eye(n) - (1 / n) * np.ones((n, n))
    assert same_bits(G.distance_matrix(centered=True), -0.5 * Jc @ singles @ Jc)
    want = csgraph.dijkstra(sparse.csr_matrix((1 / W.data, W.indices, W.indptr), shape=W.shape), directed=True)
    assert same_bits(singles, want)
    for B in (3, 65):
        problems = []
        for b in range(B):
            m = int(rng.integers(1, 5))
            problems.append((rng.choice(n, size=m, replace=False), rng.random(m) * 0.3))
        f = 0.5 + rng.random(n)
        for hl in (False, True):
            dist, cp = G._dijkstra_batch(problems, f=f, max_dist=5.0, return_cp=True, hopf_lax=hl)
            assert dist.shape == (n, B) and cp.shape == (n, B)
            for b, (s, g) in enumerate(problems):
                d1, c1 = run(G, s, g, f, 5.0, hl, False)
                assert same_bits(np.ascontiguousarray(dist[:, b]), d1) and np.array_equal(cp[:, b], c1), (B, b, hl)


def test_distance_and_path(gl):
    rng = np.random.default_rng(4)
    n = 400
    W = gl.weightmatrix.knn(rng.random((n, 2)), 7, kernel='gaussian')
    G = gl.graph(W)
    I, J, C = ref.edges(W, reciprocal=True)
    for i, j in ((0, 399), (17, 230), (5, 5)):
        v_want, _ = ref.fixed_point(n, I, J, C, [i], np.zeros(1))
        d, p, v = G.distance(i, j, return_path=True, return_distance_vector=True)
        assert same_bits(v, v_want) and d == v_want[j]
        assert np.array_equal(p, ref.path(W, v_want, i, j)) and p[0] == j and p[-1] == i
        assert G.distance(i, j) == d
        d2, v2 = G.distance(i, j, return_distance_vector=True)
        assert d2 == d and same_bits(v2, v_want)
        d3, p3 = G.distance(i, j, return_path=True)
        assert d3 == d and np.array_equal(p3, p)


def test_graph_nearest_neighbor_against_golden_fits(gl, gold):
    W = golden_graph(gold, 'blobs')
    lab = gold['graph_blobs_labels']
    ti = gold['nn_train_ind']
    for tag, kw in (('plain', {}), ('priors', {'class_priors': gold['nn_priors']}), ('D', {'D': W, 'alpha': 2})):
        model = gl.ssl.graph_nearest_neighbor(W, **kw)
        pred = model.fit_predict(ti, lab[ti])
        assert same_bits(np.asarray(model.prob, dtype=np.float64), gold['nn_%s_prob' % tag]), tag
        assert np.array_equal(pred, gold['nn_%s_pred' % tag]), tag
        prob = gl.ssl.graph_nearest_neighbor(W, **kw).fit(ti, lab[ti])
        assert same_bits(np.asarray(prob, dtype=np.float64), gold['nn_%s_prob' % tag]), tag


def test_one_million_points_against_scipy(gl):
    """n = 10^6 in the plane, k = 10, the graph built on the device; f = 1, one source: scipy's Dijkstra bit for bit."""
    import time
    n = 1000000
    X = np.random.default_rng(77).random((n, 2))
    W = gl.weightmatrix.knn(X, 10, kernel='distance')
    G = gl.graph(W)
    t0 = time.perf_counter()
    dist, cp = G.dijkstra([0], return_cp=True)
    t1 = time.perf_counter()
    want = csgraph.dijkstra(W, directed=True, indices=0)
    t2 = time.perf_counter()
    print('n=%d entries=%d: device call %.3f s (rounds %s), scipy %.3f s' % (n, W.nnz, t1 - t0, G.dijkstra_rounds, t2 - t1))
    assert same_bits(dist, want)
    assert np.array_equal(cp, np.where(np.isfinite(want), 0, -1))


def test_full_sweeps_equal_active_values(gl, gold, monkeypatch):
    """The measurement form (every round looks at every value) and the default (only values whose in-neighbours moved): same bits,
    and the default needs no more rounds than vertices."""
    from graphlearning_amd import _hip
    rng = np.random.default_rng(12)
    cases = [golden_case(gold, name)[:7] for name in ('sym_multi_md', 'dir_hl', 'gdir_recip')]
    W = random_graph(rng, 1500, 5, sym=False)
    cases.append((W, rng.choice(1500, size=4, replace=False), rng.random(4), 0.5 + rng.random(1500), 3.0, False, False))
    for W, src, g, f, max_dist, hl, recip in cases:
        G = gl.graph(W)
        monkeypatch.setattr(_hip, 'SSSP_FULL_SWEEPS', False)
        d_act, cp_act = run(G, src, g, f, max_dist, hl, recip)
        r_act = G.dijkstra_rounds
        monkeypatch.setattr(_hip, 'SSSP_FULL_SWEEPS', True)
        d_full, cp_full = run(G, src, g, f, max_dist, hl, recip)
        assert same_bits(d_act, d_full) and np.array_equal(cp_act, cp_full)
        assert max(r_act) <= W.shape[0] + 1 and max(G.dijkstra_rounds) <= W.shape[0] + 1
        want_u, want_cp = ref.dijkstra(W, src, g, f, max_dist, recip, hl)
        assert same_bits(d_act, want_u) and np.array_equal(cp_act, want_cp)
