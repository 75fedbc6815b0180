"""The head of a run of the single stop-column sweep (glx_sweep_run, csrc/solver.hip): the start kernel that writes the start iterate
and clears the stop row (sweep_start_kernel through glx_sweep_head_rows, csrc/sweep_core.hip), the eager first run, the capture and
the replay of its launch graph, and the single host wait of a run that stops at its head (glx_sweep_tail) -- bit for bit (u_T, T, the first tested sweep and every
stop value) against the host restatement tests/sweep_ref.py.

The graph is the smallest at which the head can go wrong: 333 rows (no multiple of 16: the last slice is partial) of a symmetric
pattern, 6 .. 14 entries per row plus one row of 30 and one of 110 (the split-row classes S = 4 and S = 16 of the 4-lane plans), the
vertices renumbered, so that the start values travel through the permutation.  Every row of the operator sums to 0.5: the stop value
halves per sweep, and the scale of w0 -- or max_iter -- places the stop AT the head (T = min_iter), one sweep behind it, and inside
the first tail chunk (six sweeps behind it).  (min_iter = 0 has no stop at the head by max_iter: a sweep with max_iter = 0 has no
stop column, and glx_sweep_run refuses it.)"""
import functools
import numpy as np
import pytest
from scipy import sparse
import sweep_ref as R

pytestmark = pytest.mark.gpu

N = 333
DT = {'f64': np.float64, 'f32': np.float32}
WIDTHS = (10, 3)
MIN_ITERS = (0, 1, 2, 3, 17)
BEHIND = (0, 1, 6)             # the stop: at the head, one sweep behind it, inside the first tail chunk
FAR = 40.0                     # w0 = 2^FAR w_unit: the stop test does not fire within min_iter + 6 sweeps
ROWS = [(dtype, C, min_iter, graph) for dtype in DT for C in WIDTHS for min_iter in MIN_ITERS for graph in (False, True)]
IDS = ['%s-C%d-min%d-%s' % (d, C, m, 'graph' if g else 'eager') for d, C, m, g in ROWS]


@functools.lru_cache(maxsize=None)
def operator():
    """(A, deg, vinf, w_unit), read-only.  Pattern: the ring i +- 1, 2, 3 (6 entries per row), vertex 7 joined to 104 and vertex 200
    to 24 further vertices, then random pairs among the others while both ends stay at 14 entries or fewer."""
    rng = np.random.default_rng(333)
    adj = [set() for _ in range(N)]

    def join(i, j):
        adj[i].add(j)
        adj[j].add(i)

    for i in range(N):
        for d in (1, 2, 3):
            join(i, (i + d) % N)
    hubs = {7: 110, 200: 30}
    for h, want in hubs.items():
        free = [j for j in rng.permutation(N) if j not in adj[h] and j != h and j not in hubs]
        for j in free[:want - len(adj[h])]:
            join(h, int(j))
    for _ in range(900):
        i, j = (int(x) for x in rng.integers(0, N, size=2))
        if i != j and i not in hubs and j not in hubs and j not in adj[i] and len(adj[i]) < 14 and len(adj[j]) < 14:
            join(i, j)
    lens = np.array([len(a) for a in adj])
    assert lens[7] == 110 and lens[200] == 30
    rest = np.delete(lens, [7, 200])
    assert rest.min() >= 6 and rest.max() <= 14 and len(set(rest.tolist())) >= 6, sorted(set(rest.tolist()))
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = np.concatenate([rng.permutation(sorted(a)) for a in adj]).astype(np.int32)        # stored order: unsorted
    data = np.empty(indptr[-1])
    for i in range(N):
        v = rng.random(lens[i]) + 0.25
        data[indptr[i]:indptr[i + 1]] = 0.5 * v / v.sum()
    A = sparse.csr_matrix((data, indices, indptr), shape=(N, N))
    A.has_sorted_indices = False
    pattern = sparse.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(N, N))
    assert (pattern != pattern.T).nnz == 0
    assert R.prove_products(A)
    deg, vinf, w_unit = R.stop_vectors(N, seed=334)
    for a in (A.data, A.indices, A.indptr, deg, vinf, w_unit):
        a.setflags(write=False)
    return A, deg, vinf, w_unit


@functools.lru_cache(maxsize=None)
def stop_table(dtype):
    """{T: k}: from w0 = 2^k w_unit the stop test, tried from sweep 0 on, first holds in front of sweep T.  Found on the host from the
    stop column's own recurrence (the weights rounded to the state's dtype); k from the middle of those that give this T."""
    A, deg, vinf, w_unit = operator()
    A_w = R.as_dtype(R.as_dtype(A, DT[dtype]), np.float64)
    hits = {}
    for k in np.arange(-16.0, 24.0, 0.125):
        w, t = 2.0 ** k * w_unit, 0
        while t < 64 and np.max(np.abs(deg * w - vinf)) > 1 / N:
            w, t = A_w @ w, t + 1
        hits.setdefault(t, []).append(float(k))
    return {t: ks[len(ks) // 2] for t, ks in hits.items()}


def scale_for(T, dtype):
    return stop_table(dtype)[T]


@functools.lru_cache(maxsize=None)
def reference(C, db_seed, k, min_iter, max_iter, dtype):
    A, deg, vinf, w_unit = operator()
    u, T, first, vals = R.poisson_sweeps(A, R.bias(C, n=N, seed=db_seed), 2.0 ** k * w_unit, deg, vinf, min_iter, max_iter, DT[dtype])
    u.setflags(write=False)
    vals.setflags(write=False)
    return u, T, first, vals


def by_stop_test(C, db_seed, min_iter, behind, dtype):
    """(k, max_iter, the reference's run): the stop test ends the run at T = min_iter + behind."""
    k, max_iter = scale_for(min_iter + behind, dtype), min_iter + 24
    want = reference(C, db_seed, k, min_iter, max_iter, dtype)
    assert want[1] == min_iter + behind and len(want[3]) == behind + 1 and not want[3][-1] > 1 / N
    return k, max_iter, want


def by_max_iter(C, db_seed, min_iter, behind, dtype):
    """(k, max_iter, the reference's run): max_iter = min_iter + behind ends the run; every tested value is above 1 / n."""
    max_iter = min_iter + behind
    want = reference(C, db_seed, FAR, min_iter, max_iter, dtype)
    assert want[1] == max_iter and len(want[3]) == behind and np.all(want[3] > 1 / N)
    return FAR, max_iter, want


def positions(C, db_seed, min_iter, dtype):
    out = [by_stop_test(C, db_seed, min_iter, b, dtype) for b in BEHIND]
    return out + [by_max_iter(C, db_seed, min_iter, b, dtype) for b in BEHIND if min_iter + b > 0]


@pytest.fixture(scope='module')
def hip():
    from graphlearning_amd import _hip
    _hip.require_device()
    return _hip


@pytest.fixture(scope='module')
def graphs(hip):
    A, deg, vinf, w_unit = operator()
    order = hip.host_locality_order(A.indptr, A.indices)
    out = {name: hip.DeviceGraph(A, dtype=dt, order=order) for name, dt in DT.items()}
    for G in out.values():
        perm = G.order()
        assert not np.array_equal(perm, np.arange(N)) and np.array_equal(np.sort(perm), np.arange(N))
    yield out
    for G in out.values():
        G.close()


def _same(got, want, what):
    u, T, first, vals = got
    ur, Tr, firstr, valsr = want
    assert T == Tr and first == firstr, (what, T, Tr, first, firstr)
    assert vals.dtype == np.float64 and vals.shape == valsr.shape, (what, vals.shape, valsr.shape)
    assert np.array_equal(vals, valsr), (what, vals, valsr)
    assert u.dtype == ur.dtype and u.shape == ur.shape and np.array_equal(u, ur), (what, 'iterate')


def _run(sw):
    T, _ = sw.run()
    first, vals = sw.stop_values()
    return np.array(sw.fetch()), T, first, vals


def _set(sw, C, db_seed, k, dtype):
    A, deg, vinf, w_unit = operator()
    sw.set_problem(R.bias(C, n=N, seed=db_seed).astype(DT[dtype]), 2.0 ** k * w_unit, deg, vinf)


@pytest.mark.parametrize('dtype,C,min_iter,graph', ROWS, ids=IDS)
def test_eager_run_capture_and_replay(hip, graphs, dtype, C, min_iter, graph):
    """Three runs of one object -- the eager one, the one that captures, the replay (use_hipgraph off: three eager ones) -- give the
    same bits, the reference's, at every stop position."""
    assert hip.record_layout(C, DT[dtype], True)['G'] == 4
    for k, max_iter, want in positions(C, 61, min_iter, dtype):
        sw = hip.Sweep(graphs[dtype], C, min_iter=min_iter, max_iter=max_iter, use_hipgraph=graph)
        _set(sw, C, 61, k, dtype)
        l0 = sw.launches()
        for run in range(3):
            _same(_run(sw), want, (k, max_iter, 'run', run))
        assert sw.launches() - l0 == 3 * want[1]
        sw.close()


@pytest.mark.parametrize('dtype,C,min_iter,graph', ROWS, ids=IDS)
def test_second_problem_on_stale_buffers(hip, graphs, dtype, C, min_iter, graph):
    """A first problem whose stop values are large and which runs six sweeps past the head, twice (the launch graph exists); then a
    second training set and a second w0 on the same object, twice.  Both iterates then hold the first problem's data and the stop
    rows hold maxima above 1 / n, larger than any the second problem produces: a stop row that was not cleared keeps the run going,
    a record that was not rewritten changes u."""
    k1, max_iter, want1 = by_stop_test(C, 61, min_iter, 6, dtype)
    sw = hip.Sweep(graphs[dtype], C, min_iter=min_iter, max_iter=max_iter, use_hipgraph=graph)
    _set(sw, C, 61, k1, dtype)
    for run in range(2):
        _same(_run(sw), want1, ('first', run))
    for behind in (0, 1):
        k2 = scale_for(min_iter + behind, dtype)
        want2 = reference(C, 62, k2, min_iter, max_iter, dtype)
        assert want2[1] == min_iter + behind and np.all(want2[3] < want1[3][:len(want2[3])])
        assert not np.array_equal(want2[0], want1[0])
        _set(sw, C, 62, k2, dtype)
        for run in range(2):
            _same(_run(sw), want2, ('second', behind, run))
        _set(sw, C, 61, k1, dtype)
        _same(_run(sw), want1, ('first again', behind))
    sw.close()


@pytest.mark.parametrize('dtype,C,min_iter,graph', ROWS, ids=IDS)
def test_odd_then_even_sweep_count(hip, graphs, dtype, C, min_iter, graph):
    """A run that ends on an odd T, then one that ends on an even T, then the odd one again, on one object: u_T is read from the
    ping-pong buffer of T's parity."""
    odd, even = (1, 2) if min_iter % 2 == 0 else (2, 1)
    max_iter = min_iter + 24
    sw = hip.Sweep(graphs[dtype], C, min_iter=min_iter, max_iter=max_iter, use_hipgraph=graph)
    for behind in (odd, even, odd, even):
        k = scale_for(min_iter + behind, dtype)
        want = reference(C, 63, k, min_iter, max_iter, dtype)
        assert want[1] == min_iter + behind and want[1] % 2 == (behind == odd)
        _set(sw, C, 63, k, dtype)
        _same(_run(sw), want, ('parity', behind))
    sw.close()
