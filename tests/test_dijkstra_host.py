"""graph.dijkstra and its family without a GPU: the restatement tests/dijkstra_ref.py against the golden vectors of the compiled
reference (tests/golden/make_golden_dijkstra.py) and against scipy, its two forms against each other, the conditions on the fixtures
that make the GPU comparisons complete, and the surface: the entry point is declared and exported, the Python calls exist and fail
the way every solver of this package fails without a device."""
import os
import re
import sys
import numpy as np
import pytest
from scipy import sparse
from scipy.sparse import csgraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import dijkstra_ref as ref          # noqa: E402
import graphlearning_amd as gl      # noqa: E402
from graphlearning_amd import _hip  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'g14_dijkstra.npz')


def load_golden():
    g = dict(np.load(GOLDEN, allow_pickle=False))
    for fn in sorted(set(g['entry_files'].tolist())):
        if fn != 'g14_dijkstra.npz':
            g.update(dict(np.load(os.path.join(ROOT, 'tests', 'golden', fn), allow_pickle=False)))
    return g


def golden_graph(g, name):
    n = len(g['graph_%s_indptr' % name]) - 1
    return sparse.csr_matrix((g['graph_%s_data' % name], g['graph_%s_indices' % name], g['graph_%s_indptr' % name]), shape=(n, n))


def golden_case(g, name):
    """(W, src, g, f, max_dist, hl, recip, want_dist, raw_cp) of a golden case; want_dist is the reference's output with the values
    above max_dist mapped to inf (what its documentation promises)."""
    gname, _, _, fk, _, hl, recip = ref.GOLDEN_CASES[name]
    W = golden_graph(g, gname)
    f = g[name + '_f']
    f = float(f) if f.ndim == 0 else f
    max_dist = float(g[name + '_max_dist'])
    raw = g[name + '_dist']
    return W, g[name + '_src'].astype(np.int64), g[name + '_g'], f, max_dist, hl, recip, np.where(raw <= max_dist, raw, np.inf), g[name + '_cp']


@pytest.fixture(scope='module')
def gold():
    return load_golden()


def test_golden_covers_the_cases_the_feature_names(gold):
    cases = ref.GOLDEN_CASES
    assert set(c for c in cases) <= set(gold['entry_names'].tolist())
    kinds = {(ref.GOLDEN_GRAPHS[c[0]]['kind'], ref.GOLDEN_GRAPHS[c[0]].get('kernel'), ref.GOLDEN_GRAPHS[c[0]].get('symmetrize')) for c in cases.values()}
    assert {('knn', 'distance', True), ('knn', 'distance', False), ('knn', 'gaussian', True), ('knn', 'gaussian', False),
            ('ball', 'distance', None)} <= kinds
    assert any(c[5] for c in cases.values()) and any(not c[5] for c in cases.values())              # both relaxations
    assert any(c[4] is not None for c in cases.values())                                          # a finite max_dist
    assert any(c[3] == 'vec' for c in cases.values()) and any(isinstance(c[3], float) for c in cases.values())
    assert all(c[6] for c in cases.values() if ref.GOLDEN_GRAPHS[c[0]].get('kernel') == 'gaussian')  # gaussian graphs: reciprocal weights
    for name, c in cases.items():
        W, src, g, f, max_dist, hl, recip, want, _ = golden_case(gold, name)
        assert len(src) == c[1] and len(np.unique(src)) == len(src)
        if c[1] > 1:
            assert len(np.unique(g)) == len(g), 'unequal boundary values'
        if c[2]:
            assert want[src[1]] < g[1], 'the dominated source is not dominated'
        if c[4] is not None:
            assert np.isfinite(max_dist) and 0 < np.isfinite(want).sum() < len(want)
        # the inputs are what the generator derives from the seeds
        s2, g2, f2 = ref.golden_case_inputs(name, W)
        assert np.array_equal(s2, src) and np.array_equal(g2, g) and np.array_equal(np.asarray(f2, dtype=np.float64), np.asarray(f))


def test_conditions_on_the_fixtures(gold):
    """No comparison downstream is silently narrowed: no empty row, one tight-reachable source per reached vertex, no subnormal."""
    for gname in ref.GOLDEN_GRAPHS:
        W = golden_graph(gold, gname)
        assert np.diff(W.indptr).min() >= 1 and W.data.min() > 0, gname
    for name in ref.GOLDEN_CASES:
        W, src, g, f, max_dist, hl, recip, want, _ = golden_case(gold, name)
        I, J, C = ref.edges(W, f, recip)
        reached = np.isfinite(want)
        assert ref.unique_closest(W.shape[0], I, J, C, src, g, want, max_dist, hl)[reached].all(), name
        pos = want[reached & (want > 0)]
        assert pos.min() >= np.finfo(np.float64).tiny, name
        assert (want[reached] <= max_dist).all()


@pytest.mark.parametrize('name', sorted(ref.GOLDEN_CASES))
def test_restatement_equals_golden(gold, name):
    """Fixed-point form, heap form and the tight-chain closest point against the compiled reference, bit for bit; the closest point
    on ALL vertices with u <= max_dist."""
    W, src, g, f, max_dist, hl, recip, want, raw_cp = golden_case(gold, name)
    n = W.shape[0]
    I, J, C = ref.edges(W, f, recip)
    u, rounds = ref.fixed_point(n, I, J, C, src, g, max_dist, hl)
    assert u.tobytes() == want.tobytes()
    assert rounds <= n
    uh, lh = ref.heap(n, I, J, C, src, g, max_dist, hl)
    assert uh.tobytes() == want.tobytes()
    reached = np.isfinite(want)
    cp = ref.closest_point(n, I, J, C, src, g, u, max_dist, hl)
    assert np.array_equal(cp[reached], raw_cp[reached])
    assert (cp[~reached] == -1).all()
    assert np.array_equal(lh[reached], raw_cp[reached])
    assert np.isin(cp[reached], src).all()
    # the one-call restatement the GPU tests use
    u2, cp2 = ref.dijkstra(W, src, g, f, max_dist, recip, hl)
    assert u2.tobytes() == want.tobytes() and np.array_equal(cp2, cp)


def test_restatement_equals_scipy():
    """f = 1, one source: scipy's Dijkstra adds the same costs in the same order along the same optimal paths."""
    rng = np.random.default_rng(5)
    for n, deg, sym in ((400, 6, True), (700, 5, False), (300, 12, True)):
        A = sparse.random(n, n, density=deg / n, random_state=int(rng.integers(1 << 30)), format='csr')
        A.setdiag(0)
        A.eliminate_zeros()
        if sym:
            A = A.maximum(A.T).tocsr()
        s = int(rng.integers(n))
        want = csgraph.dijkstra(A, directed=True, indices=s)
        I, J, C = ref.edges(A)
        u, _ = ref.fixed_point(n, I, J, C, [s], np.zeros(1))
        assert u.tobytes() == want.tobytes()
        uh, _ = ref.heap(n, I, J, C, [s], np.zeros(1))
        assert uh.tobytes() == want.tobytes()


def test_heap_equals_fixed_point_randomised():
    rng = np.random.default_rng(9)
    for trial in range(12):
        n = int(rng.integers(2, 300))
        A = sparse.random(n, n, density=min(1.0, rng.integers(1, 8) / n), random_state=int(rng.integers(1 << 30)), format='csr')
        if trial % 2:
            A = A.maximum(A.T).tocsr()
        m = int(rng.integers(1, min(n, 6) + 1))
        src = rng.choice(n, size=m, replace=False)
        g = rng.random(m)
        f = 0.5 + rng.random(n)
        hl = bool(trial % 3 == 0)
        max_dist = np.inf if trial % 4 else float(rng.random() * 2)
        I, J, C = ref.edges(A, f, reciprocal=bool(trial % 5 == 0))
        u, _ = ref.fixed_point(n, I, J, C, src, g, max_dist, hl)
        uh, lh = ref.heap(n, I, J, C, src, g, max_dist, hl)
        assert u.tobytes() == uh.tobytes(), trial
        cp = ref.closest_point(n, I, J, C, src, g, u, max_dist, hl)
        uniq = ref.unique_closest(n, I, J, C, src, g, u, max_dist, hl)
        assert np.array_equal(cp[uniq], lh[uniq]), trial
        assert ((cp == -1) == ~np.isfinite(u)).all(), trial


def test_grid_ties_smallest_index():
    """On the unit grid ties are everywhere: the rule picks the smallest index among the sources tied for closest, and the heap's
    own answer is always one of them."""
    m = 12
    idx = np.arange(m * m).reshape(m, m)
    rows = np.concatenate([idx[:-1, :].ravel(), idx[:, :-1].ravel()])
    cols = np.concatenate([idx[1:, :].ravel(), idx[:, 1:].ravel()])
    W = sparse.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(m * m, m * m))
    W = (W + W.T).tocsr()
    src = np.array([idx[2, 3], idx[9, 9], idx[3, 10]])
    g = np.zeros(3)
    I, J, C = ref.edges(W)
    u, _ = ref.fixed_point(m * m, I, J, C, src, g)
    r, c = np.divmod(np.arange(m * m), m)
    man = np.stack([abs(r - sr) + abs(c - sc) for sr, sc in (divmod(int(s), m) for s in src)])
    assert np.array_equal(u, man.min(axis=0).astype(np.float64))
    cp = ref.closest_point(m * m, I, J, C, src, g, u)
    want = np.array([src[np.where(man[:, v] == man[:, v].min())[0]].min() for v in range(m * m)])
    assert np.array_equal(cp, want)
    _, lh = ref.heap(m * m, I, J, C, src, g)
    assert all(man[list(src).index(lh[v]), v] == man[:, v].min() for v in range(m * m))


def test_symbol_declared_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'glx_experimental.h')).read()
    assert re.search(r'\bint\s+glx_sssp\s*\(', hdr)
    assert re.search(r'#define\s+GLX_SSSP_PLAIN\s+%d\b' % _hip.GLX_SSSP_PLAIN, hdr)
    assert re.search(r'#define\s+GLX_SSSP_HOPF_LAX\s+%d\b' % _hip.GLX_SSSP_HOPF_LAX, hdr)
    assert 'glx_sssp' in _hip.EXPORTED_SYMBOLS
    assert getattr(_hip.load(), 'glx_sssp') is not None


def _path_graph():
    return sparse.identity(6, format='csr') + sparse.diags([1.0] * 5, 1) + sparse.diags([1.0] * 5, -1)


def test_entry_points_exist_and_refuse_without_a_device():
    """The calls exist (no AttributeError) and, like every solver here, raise GlxError when there is no device: no CPU fallback."""
    G = gl.graph(_path_graph())
    for name in ('dijkstra', 'dijkstra_hl', 'distance', 'distance_matrix', 'neighbors', '_dijkstra_batch'):
        assert callable(getattr(G, name)), name
    model = gl.ssl.graph_nearest_neighbor(_path_graph())
    assert model.name == 'Graph NN (alpha=1.00)' and model.accuracy_filename == '_graph_nearest_neighbor_alpha1.00'
    assert model.get_accuracy_filename() == '_graph_nearest_neighbor_alpha1.00_accuracy.csv'
    pri = gl.ssl.graph_nearest_neighbor(_path_graph(), class_priors=np.array([0.5, 0.5]), alpha=2)
    assert pri.onevsrest and not pri.similarity and pri.get_accuracy_filename() == '_graph_nearest_neighbor_alpha2.00_classpriors_accuracy.csv'
    nb, w = G.neighbors(2, return_weights=True)
    assert np.array_equal(nb, [1, 3]) and np.array_equal(w, [1.0, 1.0]) and np.array_equal(G.neighbors(0), [1])
    try:
        n_dev = _hip.device_count()
    except _hip.GlxError:
        n_dev = 0
    if n_dev > 0:
        assert np.array_equal(G.dijkstra([0]), np.arange(6.0))
        return
    with pytest.raises(_hip.GlxError):
        G.dijkstra([0])
    with pytest.raises(_hip.GlxError):
        G.dijkstra_hl([0], bdy_val=0.5, f=2.0, max_dist=3.0, return_cp=True)
    with pytest.raises(_hip.GlxError):
        G.distance(0, 4)
    with pytest.raises(_hip.GlxError):
        G.distance_matrix()
    with pytest.raises(_hip.GlxError):
        model.fit(np.array([0, 5]), np.array([0, 1]))
    with pytest.raises(_hip.GlxError):
        pri.fit(np.array([0, 5]), np.array([0, 1]))


def test_refusals_are_value_errors():
    """Stated deviations: what the reference's heap does not survive, or what has no meaning as a cost, is refused before any device call."""
    G = gl.graph(_path_graph())
    with pytest.raises(ValueError):
        G.dijkstra([0, 0])
    with pytest.raises(ValueError):
        G.dijkstra([0], bdy_val=-1.0)
    with pytest.raises(ValueError):
        G.dijkstra([0], bdy_val=np.array([np.nan]))
    with pytest.raises(ValueError):
        G.dijkstra([0], f=-1.0)
    with pytest.raises(ValueError):
        G.dijkstra_hl([0], f=np.array([1, 1, np.nan, 1, 1, 1.0]))
    with pytest.raises(ValueError):
        G.dijkstra([7])
    with pytest.raises(ValueError):
        G.dijkstra([0], max_dist=np.nan)
    Wn = _path_graph().tolil()
    Wn[1, 2] = -1.0
    with pytest.raises(ValueError):
        gl.graph(Wn.tocsr()).dijkstra([0])


def test_in_edges_handle_empty_rows_zeros_and_the_diagonal():
    """The edge lists handed to the device: explicit zeros and the diagonal are gone, a vertex without entries has an empty list
    (the reference's `K` is wrong there), and the costs are W[i, j] * f[i] listed by the vertex they enter."""
    W = sparse.csr_matrix(np.array([[5.0, 2.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [3.0, 0.0, 1.0, 4.0], [0.0, 7.0, 0.0, 0.0]]))
    W.data[1] = 0.0                                     # an explicit zero at (0, 1)
    G = gl.graph(W)
    in_ptr, in_idx, V, Vinv, out_ptr, out_idx = G._in_edges()
    assert out_ptr.tolist() == [0, 0, 0, 2, 3] and out_idx.tolist() == [0, 3, 1]
    assert in_ptr.tolist() == [0, 1, 2, 2, 3]
    assert in_idx.tolist() == [2, 3, 2] and V.tolist() == [3.0, 7.0, 4.0]
    assert Vinv.tobytes() == (1 / V).tobytes()
    I, J, C = ref.edges(W)
    assert sorted(zip(J.tolist(), I.tolist(), C.tolist())) == sorted(zip(np.repeat(np.arange(4), np.diff(in_ptr)).tolist(), in_idx.tolist(), V.tolist()))
