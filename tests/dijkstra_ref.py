"""graph.dijkstra / graph.dijkstra_hl restated from their rules, numpy and scipy only (tests/test_dijkstra_host.py checks the
restatement against golden vectors of the compiled reference, tests/test_gpu_dijkstra.py checks the device against it):

  edges        the stored entries (i, j, w) of W with w != 0 and j != i (`sparse.find` in the reference's __ccode_init__; its loop
               skips j == i); cost c_ij = w_ij * f_i (1/w_ij * f_i with reciprocal weights) -- f at the vertex the edge LEAVES;
  relaxation   plain  a + c;   Hopf-Lax  (c + sqrt(c*c + 4*a*a)) / 2.0;   every operation rounded on its own (no fused multiply-add);
  distances    u = the minimum over paths from the sources of the cost folded left to right along the path, starting from the
               source's boundary value.  Two forms that must agree bit for bit: `heap` (Dijkstra with a binary heap, strict `<`)
               and `fixed_point` (u_j <- min(u_j, min_i relax(u_i, c_ij)) until nothing moves);
  max_dist     a vertex is relaxed from i only if u_i <= max_dist; afterwards values above max_dist are +inf (as documented);
  closest pt   a source s attains its value if u_s == g_s (and g_s <= max_dist); an edge i -> j is tight if u_i <= max_dist,
               u_j < inf and relax(u_i, c_ij) == u_j; cp[j] = the smallest source index reaching j along tight edges, -1: none."""
import heapq
import numpy as np
from scipy import sparse

NO_CP = np.iinfo(np.int32).max


def edges(W, f=1, reciprocal=False):
    """(I, J, cost) of the edges i -> j, sorted by i (the order inside a vertex's block does not matter to any result here)."""
    W = sparse.csr_matrix(W)
    n = W.shape[0]
    I, J, V = sparse.find(W)
    keep = I != J
    I, J, V = I[keep], J[keep], V[keep].astype(np.float64)
    ind = np.argsort(I, kind='stable')
    I, J, V = I[ind], J[ind], V[ind]
    if type(f) != np.ndarray:
        f = np.ones((n,)) * f
    with np.errstate(divide='ignore'):
        if reciprocal:
            V = 1 / V
    return I.astype(np.int64), J.astype(np.int64), V * f[I]


def relax(a, c, hl):
    with np.errstate(over='ignore'):
        if hl:
            return (c + np.sqrt(c * c + 4 * a * a)) / 2.0
        return a + c


def heap(n, I, J, C, src, g, max_dist=np.inf, hl=False):
    """Dijkstra with a priority queue and the reference's arithmetic.  Returns (u, cp) with the tentative values above max_dist
    already replaced by +inf / -1; cp is the label handed down the shortest-path tree (history-dependent where sources tie)."""
    K = np.concatenate(([0], np.cumsum(np.bincount(I, minlength=n))))
    d = np.full(n, np.inf)
    l = np.full(n, -1, dtype=np.int64)
    final = np.zeros(n, dtype=bool)
    pq = []
    for s, v in zip(src, g):
        d[s] = v
        l[s] = s
        heapq.heappush(pq, (float(v), int(s)))
    while pq:
        di, i = heapq.heappop(pq)
        if final[i] or di != d[i]:
            continue
        final[i] = True
        if di > max_dist:
            break
        for jj in range(K[i], K[i + 1]):
            j = J[jj]
            if final[j]:
                continue
            t = relax(np.float64(di), C[jj], hl)
            if t < d[j]:
                d[j] = t
                l[j] = l[i]
                heapq.heappush(pq, (float(t), int(j)))
    far = ~(d <= max_dist)
    d[far] = np.inf
    l[far] = -1
    return d, l.astype(np.int32)


def fixed_point(n, I, J, C, src, g, max_dist=np.inf, hl=False):
    """Synchronous label-correcting rounds.  Returns (u, rounds)."""
    u = np.full(n, np.inf)
    u[np.asarray(src, dtype=np.int64)] = g
    rounds = 0
    while True:
        rounds += 1
        assert rounds <= n + 1
        a = u[I]
        ok = a <= max_dist
        new = u.copy()
        np.minimum.at(new, J[ok], relax(a[ok], C[ok], hl))
        if np.array_equal(new, u):
            break
        u = new
    u[~(u <= max_dist)] = np.inf
    return u, rounds


def _tight(u, I, J, C, max_dist, hl):
    a = u[I]
    with np.errstate(invalid='ignore'):
        return (a <= max_dist) & (u[J] < np.inf) & (relax(a, C, hl) == u[J])


def closest_point(n, I, J, C, src, g, u, max_dist=np.inf, hl=False, largest=False):
    """The smallest (largest=True: largest) source index reaching each vertex along tight edges; -1 where none does."""
    src = np.asarray(src, dtype=np.int64)
    g = np.asarray(g, dtype=np.float64)
    t = _tight(u, I, J, C, max_dist, hl)
    Ti, Tj = I[t], J[t]
    sign = -1 if largest else 1
    cp = np.full(n, NO_CP, dtype=np.int64)
    att = (g <= max_dist) & (u[src] == g)
    cp[src[att]] = sign * src[att]
    while True:
        new = cp.copy()
        np.minimum.at(new, Tj, cp[Ti])
        if np.array_equal(new, cp):
            break
        cp = new
    out = np.where(cp == NO_CP, -1, sign * cp)
    return out.astype(np.int32)


def unique_closest(n, I, J, C, src, g, u, max_dist=np.inf, hl=False):
    """True where exactly one source reaches the vertex along tight edges (smallest == largest) or the vertex is unreached."""
    lo = closest_point(n, I, J, C, src, g, u, max_dist, hl)
    hi = closest_point(n, I, J, C, src, g, u, max_dist, hl, largest=True)
    return lo == hi


def dijkstra(W, bdy_set, bdy_val=0, f=1, max_dist=np.inf, reciprocal_weights=False, hl=False):
    """(dist, cp) of graph.dijkstra / graph.dijkstra_hl as this package defines them: the fixed point and the tight-chain rule."""
    n = W.shape[0]
    src = np.asarray(bdy_set, dtype=np.int64)
    g = np.ones(len(src)) * bdy_val if type(bdy_val) != np.ndarray else bdy_val.astype(np.float64)
    I, J, C = edges(W, f, reciprocal_weights)
    u, _ = fixed_point(n, I, J, C, src, g, max_dist, hl)
    return u, closest_point(n, I, J, C, src, g, u, max_dist, hl)


def path(W, v, i, j):
    """graph.distance's walk from j back to i over the distance vector v to i (reference graph.py:1029-1037)."""
    W = sparse.csr_matrix(W)
    p = j
    out = [p]
    while p != i:
        nn = W[p, :].nonzero()[1]
        nn = nn[nn != p]
        w = W[p, nn].toarray().flatten()
        p = nn[np.argmin(v[nn] + w ** -1)]
        out.append(p)
    return np.array(out)


# ---- the golden cases of tests/golden/g14_dijkstra*.npz ---------------------------------------------------------------------------
# graphs (built by the generator with the reference's weightmatrix; stored as CSR): name -> how
GOLDEN_GRAPHS = {
    'knn_sym': dict(kind='knn', seed=0, n=1000, d=2, k=8, kernel='distance', symmetrize=True),
    'knn_dir': dict(kind='knn', seed=0, n=1000, d=2, k=8, kernel='distance', symmetrize=False),
    'gauss_sym': dict(kind='knn', seed=1, n=900, d=3, k=8, kernel='gaussian', symmetrize=True),
    'gauss_dir': dict(kind='knn', seed=1, n=900, d=3, k=8, kernel='gaussian', symmetrize=False),
    'ball': dict(kind='ball', seed=2, n=700, d=2, eps=0.09, kernel='distance'),
    'blobs': dict(kind='blobs', seed=3, n=900, d=4, k=8, C=3, kernel='distance', symmetrize=True),
}


def golden_sources(n, seed, m, W=None, dominated=False):
    """m distinct sources with unequal boundary values; dominated=True: the second source is an out-neighbour of the first
    whose own value lies far above what the first one offers it (so u_s < g_s there)."""
    rng = np.random.default_rng(seed)
    src = rng.choice(n, size=m, replace=False).astype(np.int64)
    g = rng.random(m) * 0.05
    if dominated:
        W = sparse.csr_matrix(W)
        nb = W[src[0], :].nonzero()[1]
        nb = nb[(nb != src[0]) & ~np.isin(nb, src)]
        src[1] = nb[0]
        g[1] = g[0] + 1000.0
    return src, g


def golden_f(n, seed):
    return 0.5 + np.random.default_rng(seed).random(n)


# case -> (graph, sources m, dominated, f: None | scalar | 'vec', max_dist: None | quantile of the finite distances, hl, reciprocal)
GOLDEN_CASES = {
    'sym_single': ('knn_sym', 1, False, None, None, False, False),
    'sym_multi': ('knn_sym', 7, True, 'vec', None, False, False),
    'sym_multi_md': ('knn_sym', 7, True, 'vec', 0.4, False, False),
    'sym_hl': ('knn_sym', 7, True, 'vec', None, True, False),
    'sym_hl_md': ('knn_sym', 5, False, 0.7, 0.5, True, False),
    'dir_multi': ('knn_dir', 6, True, 0.7, None, False, False),
    'dir_md': ('knn_dir', 6, False, 'vec', 0.3, False, False),
    'dir_hl': ('knn_dir', 4, False, 'vec', None, True, False),
    'gsym_recip_single': ('gauss_sym', 1, False, None, None, False, True),
    'gsym_recip_multi': ('gauss_sym', 5, True, 'vec', 0.6, False, True),
    'gdir_recip': ('gauss_dir', 5, False, 1.3, None, False, True),
    'ball_multi': ('ball', 6, True, 'vec', None, False, False),
    'ball_hl_md': ('ball', 6, False, None, 0.5, True, False),
}


def golden_case_inputs(name, W, seed_base=100):
    """(src, g, f) of a golden case on its graph W; max_dist is stored in the file (it is derived from the reference's output)."""
    gname, m, dom, fk, _, _, _ = GOLDEN_CASES[name]
    n = W.shape[0]
    seed = seed_base + sorted(GOLDEN_CASES).index(name)
    src, g = golden_sources(n, seed, m, W, dom)
    if m == 1:
        g = np.zeros(1)
    f = 1 if fk is None else (golden_f(n, seed + 1000) if fk == 'vec' else fk)
    return src, g, f
