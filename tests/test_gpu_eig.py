"""graph.eigen_decomp, ssl.poisson(solver='spectral') and _hip.Eig on the device: every operation of the solver object against the host
restatement of csrc/eig_plan.h BIT FOR BIT at the shapes where the kernels can go wrong, whole solves against the same driver on the
host backend bit for bit, the reference's golden vectors within the bounds measured when the fixture was made, the two run-time
errors with a solve behind them, and repeatability with the pool on, off and poisoned.

Every test runs under a time limit of its own: a test that exceeds it ends the whole session on the spot (traceback of every
thread, then exit), so nothing more is started on a device that may have hung; nothing is retried."""
import faulthandler
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eig_ref as ref  # noqa: E402

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
    return ref.build_host_lib(tmp_path_factory.mktemp('eig_plan'))


def operation_matrix(n):
    """a canonical CSR matrix for the per-operation tests: the order is the contract, not the mathematics, so it need not be symmetric;
    rows without entries from n = 65 on"""
    from scipy import sparse
    rng = np.random.default_rng(50 + n)
    if n < 16:
        return sparse.csr_matrix(rng.uniform(0.5, 1.5, size=(n, n)))
    W = ref.seeded_graph(n).tolil()
    if n >= 65:
        for i in (3, 40, n - 1):
            W[i, :] = 0
    W = W.tocsr()
    W.eliminate_zeros()
    W.sort_indices()
    return W


def both(gl, lib, A, m):
    from graphlearning_amd import _hip
    indptr, indices, data = ref.csr_arrays(A)
    return _hip.Eig(indptr, indices, data, m), ref.HostBackend(lib, A, m)


def same_basis(dev, host, m):
    for j0 in range(0, m + 1, 256):
        j1 = min(j0 + 256, m + 1)
        a, b = dev.get_columns(j0, j1), host.get_columns(j0, j1)
        if not ref.same_bits(a, b):
            return False
    return True


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 257, 1000])
def test_operations_bit_for_bit(gl, lib, n):
    """run, orthonormalize, rotate and get_columns on a seeded random basis that is NOT orthonormal: n covers one partial exactly (64),
    one row past it (65) and several chains of the finishing kernel's 64 (1000: 16 partials; 257: 5); j covers one and several rounds
    of its 16 columns (15, 16, 17, 64) and the widest basis (511)."""
    A = operation_matrix(n)
    m = min(n, 513)
    if n >= 65:
        assert (np.diff(A.indptr) == 0).sum() >= 3
    dev, host = both(gl, lib, A, m)
    try:
        rng = np.random.default_rng(n)
        for j in range(m + 1):
            x = rng.uniform(-1, 1, size=n)
            dev.set_column(j, x)
            host.set_column(j, x)
        assert same_basis(dev, host, m)
        for j in [j for j in (0, 1, 15, 16, 17, 64, 511) if j < m]:
            j1 = min(j + 2, m)
            (a, b), (ha, hb) = dev.run(j, j1), host.run(j, j1)
            print(n, 'run', (j, j1), 'alpha', a, 'beta', b)
            assert ref.same_bits(a, ha) and ref.same_bits(b, hb) and np.all(np.isfinite(a)) and np.all(np.isfinite(b)), j
            assert ref.same_bits(dev.get_columns(j + 1, j1 + 1), host.get_columns(j + 1, j1 + 1)), j
        for j in [j for j in (0, 1, 15, 16, 17, 64, 511) if j <= m]:
            norm, hnorm = dev.orthonormalize(j), host.orthonormalize(j)
            assert norm == hnorm and np.isfinite(norm), j
            assert ref.same_bits(dev.get_columns(j, j + 1), host.get_columns(j, j + 1)), j
        for rows, keep in [(20, 12), (23, 17), (513, 384)]:
            if rows > m:
                continue
            Y = np.random.default_rng(rows).uniform(-1, 1, size=(rows, keep))
            dev.rotate(Y, rows, keep)
            host.rotate(Y, rows, keep)
            assert same_basis(dev, host, m), (rows, keep)
        if m >= 2:
            Y = np.random.default_rng(7).uniform(-1, 1, size=(m, m))          # keep = rows: no column moves behind the rotation
            dev.rotate(Y, m, m)
            host.rotate(Y, m, m)
        assert same_basis(dev, host, m)
    finally:
        dev.close()
        host.close()


def test_sums_of_65_partials_bit_for_bit(gl, lib):
    """n = 4097: 65 partials, so chain 0 of the finishing kernel adds two of them (the stride of 64 between the partials of a chain).
    j covers 1, 2, 16, 17 and 18 columns: one and two workgroups of the finishing kernel."""
    n, m = 4097, 20
    A = operation_matrix(n)
    dev, host = both(gl, lib, A, m)
    try:
        rng = np.random.default_rng(n)
        for j in range(m + 1):
            x = rng.uniform(-1, 1, size=n)
            dev.set_column(j, x)
            host.set_column(j, x)
        for j in (0, 1, 15, 16, 17):
            (a, b), (ha, hb) = dev.run(j, j + 1), host.run(j, j + 1)
            print(n, 'run', j, 'alpha', a, 'beta', b)
            assert ref.same_bits(a, ha) and ref.same_bits(b, hb) and np.all(np.isfinite(a)) and np.all(np.isfinite(b)), j
            assert ref.same_bits(dev.get_columns(j + 1, j + 2), host.get_columns(j + 1, j + 2)), j
        for j in (0, 1, 15, 16, 17):
            norm, hnorm = dev.orthonormalize(j), host.orthonormalize(j)
            assert norm == hnorm and np.isfinite(norm), j
            assert ref.same_bits(dev.get_columns(j, j + 1), host.get_columns(j, j + 1)), j
        assert same_basis(dev, host, m)
    finally:
        dev.close()
        host.close()


def test_refusals_of_the_object(gl, lib):
    from graphlearning_amd import _hip
    A = operation_matrix(65)
    dev, host = both(gl, lib, A, 20)
    host.close()
    with dev:
        x = np.ones(65)
        for call in (lambda: dev.set_column(-1, x), lambda: dev.set_column(21, x), lambda: dev.orthonormalize(21), lambda: dev.run(0, 21),
                     lambda: dev.run(3, 3), lambda: dev.rotate(np.zeros((21, 2)), 21, 2), lambda: dev.rotate(np.zeros((5, 6)), 5, 6),
                     lambda: dev.get_columns(0, 22), lambda: dev.get_columns(4, 4)):
            with pytest.raises(_hip.GlxError):
                call()
        with pytest.raises(_hip.GlxError, match='shape'):
            dev.set_column(0, np.ones(64))
        dev.set_column(20, x)
        assert ref.same_bits(dev.get_columns(20, 21), x[:, None])
    with pytest.raises(_hip.GlxError, match='closed'):
        dev.run(0, 1)
    big = operation_matrix(1000)
    with _hip.Eig(*ref.csr_arrays(big), 513) as wide:
        with pytest.raises(_hip.GlxError, match='at most 256'):
            wide.get_columns(0, 257)


@pytest.mark.parametrize('normalization', ref.NORMALIZATIONS)
@pytest.mark.parametrize('n,k', ref.SHAPES)
def test_whole_solves_bit_for_bit(gl, lib, n, k, normalization):
    W = ref.seeded_graph(n)
    want = ref.host_decomp(lib, W, normalization, k)
    G = gl.graph(W)
    vals, vecs = G.eigen_decomp(normalization=normalization, k=k)
    print((n, k), normalization, 'steps', G.eig_steps, 'restarts', G.eig_restarts, 'probe', G.eig_probe, 'differing values',
          int((vecs != want[1]).sum()))
    assert ref.same_bits(vals, want[0]) and ref.same_bits(vecs, want[1])
    assert (G.eig_steps, G.eig_restarts, G.eig_probe) == want[2:]
    again = G.eigen_decomp(normalization=normalization, k=k)                   # cached under the reference's six parameters
    assert again[0] is vals and again[1] is vecs


@pytest.mark.parametrize('g', ref.GRAPHS)
def test_golden_eigen_decomp(gl, gold, g):
    W = ref.golden_graph(gold, g)
    G = gl.graph(W)
    for normalization, k in ref.DECOMPS:
        key = 'dec_%s_%s_' % (g, normalization)
        vals, vecs = G.eigen_decomp(normalization=normalization, k=k)
        got = ref.measure(W, normalization, vals, vecs, gold[key + 'vals'], gold[key + 'vecs'])
        print(g, normalization, k, 'steps', G.eig_steps, 'restarts', G.eig_restarts, got, {q: float(gold['bound_' + q]) for q in ref.QUANTITIES})
        assert vals.shape == (k,) and vecs.shape == (W.shape[0], k) and np.all(np.diff(vals) > 0)
        for q in ref.QUANTITIES:
            assert got[q] <= float(gold['bound_' + q]), (q, got[q])
        assert G.eigendata[normalization]['k'] == k and G.eigendata[normalization]['eigenvalues'] is vals


@pytest.mark.parametrize('g', ref.GRAPHS)
def test_golden_poisson_spectral(gl, gold, g, monkeypatch):
    from graphlearning_amd import _eig
    W = ref.golden_graph(gold, g)
    ind, labels, priors = gold['pois_%s_ind' % g], gold['pois_%s_labels' % g], gold['pois_%s_priors' % g]
    solves = []
    solver = _eig.thick_restart
    monkeypatch.setattr(_eig, 'thick_restart', lambda *a, **kw: (solves.append(1), solver(*a, **kw))[1])
    for p in (1, 2):
        key = 'pois_%s_p%d_' % (g, p)
        model = gl.ssl.poisson(W, solver='spectral', p=p)
        assert model.solver == 'spectral'
        prob = model.fit(ind, labels)
        d = ref.prob_difference(prob, gold[key + 'prob'])
        print(g, 'p', p, 'largest difference over largest |prob|', d, 'bound', float(gold['bound_prob']))
        assert d <= float(gold['bound_prob'])
        assert np.array_equal(model.predict(), gold[key + 'pred'])
        before = len(solves)
        again = model.fit(ind, labels)                                           # the decomposition is cached with the graph's key
        assert len(solves) == before and ref.same_bits(again, prob)
        steps = model._cache[2]['graph'].eig_steps
        assert steps is not None and steps > 0
        with_priors = gl.ssl.poisson(W, class_priors=priors, solver='spectral', p=p)
        assert np.array_equal(with_priors.fit_predict(ind, labels), gold[key + 'pred_priors'])
        assert ref.same_bits(np.ascontiguousarray(with_priors.prob), np.ascontiguousarray(prob))
    assert len(solves) == 4                                                      # one per model, none per repeated fit


def test_ssl_trials_writes_its_file(gl, gold, tmp_path, monkeypatch):
    from graphlearning_amd import _eig
    W = ref.golden_graph(gold, 'blobs')
    truth, ind = gold['graph_blobs_truth'], gold['pois_blobs_ind']
    rng = np.random.default_rng(3)
    other = np.concatenate([rng.choice(np.where(truth == c)[0], size=2, replace=False) for c in np.unique(truth)])
    monkeypatch.setattr(gl.ssl, 'results_dir', str(tmp_path / 'results'))
    solves = []
    solver = _eig.thick_restart
    monkeypatch.setattr(_eig, 'thick_restart', lambda *a, **kw: (solves.append(1), solver(*a, **kw))[1])
    model = gl.ssl.poisson(W, solver='spectral')
    model.ssl_trials([other, ind], truth, tag='eig_')
    assert len(solves) == 1                                                      # two trials, one decomposition
    path = tmp_path / 'results' / 'eig__poisson_N10_accuracy.csv'
    lines = path.read_text().splitlines()
    assert lines[0] == 'Number of labels,Accuracy' and len(lines) == 3
    assert [int(s.split(',')[0]) for s in lines[1:]] == [len(other), len(ind)]
    acc = gl.ssl.ssl_accuracy(gold['pois_blobs_p1_pred'], truth, ind)
    assert lines[2] == '%d,%.2f' % (len(ind), acc)


def test_poisson_mbo_runs_on_the_spectral_solver(gl, gold):
    W = ref.golden_graph(gold, 'blobs')
    ind, labels, priors = gold['pois_blobs_ind'], gold['pois_blobs_labels'], gold['pois_blobs_priors']
    pred = gl.ssl.poisson_mbo(W, priors, solver='spectral').fit_predict(ind, labels)
    assert pred.shape == (600,) and pred.min() >= 0 and pred.max() <= 2 and gl.ssl.ssl_accuracy(pred, gold['graph_blobs_truth'], ind) > 50


def test_errors_leave_the_device_usable(gl, lib):
    from graphlearning_amd import _hip
    with pytest.raises(_hip.GlxError, match='a multiple eigenvalue was missed'):
        gl.graph(ref.components_graph(10, 60)).eigen_decomp(normalization='normalized', k=11)
    with pytest.raises(_hip.GlxError, match='a multiple eigenvalue was missed'):
        gl.graph(ref.path_graph(101)).eigen_decomp(normalization='normalized', k=3)
    with pytest.raises(_hip.GlxError, match='breakdown'):
        gl.graph(ref.complete_graph(30)).eigen_decomp(normalization='normalized', k=3)
    W = ref.seeded_graph(600)
    want = ref.host_decomp(lib, W, 'normalized', 11)
    vals, vecs = gl.graph(W).eigen_decomp(normalization='normalized', k=11)
    assert ref.same_bits(vals, want[0]) and ref.same_bits(vecs, want[1])


def test_the_same_bits_with_the_pool_on_off_and_poisoned(gl, lib):
    from graphlearning_amd import _hip
    W = ref.seeded_graph(600)
    want = ref.host_decomp(lib, W, 'randomwalk', 11)

    def solve():
        G = gl.graph(W)
        return G.eigen_decomp(normalization='randomwalk', k=11) + (G.eig_steps, G.eig_restarts, G.eig_probe)

    def same(a, b):
        return ref.same_bits(a[0], b[0]) and ref.same_bits(a[1], b[1]) and a[2:] == b[2:]
    a, b = solve(), solve()
    assert same(a, b) and same(a, want)
    _hip.pool_set_enabled(False)
    try:
        c = solve()
    finally:
        _hip.pool_set_enabled(True)
    assert same(a, c)
    for byte in (0xFF, 0x7F):                       # every pooled block filled with NaN patterns / huge numbers when it is handed out
        _hip.pool_set_poison(byte)
        try:
            d = solve()
        finally:
            session = [s for s in os.environ.get('GLX_TEST_ABLATE', '').split(',') if s.startswith('poison')]      # (an ablation run's own fill)
            _hip.pool_set_poison(int(session[0][6:] or '255') if session else -1)
        assert same(a, d), byte


def test_the_global_stream_is_left_alone(gl):
    np.random.seed(123)
    before = np.random.get_state()
    gl.graph(ref.seeded_graph(200)).eigen_decomp(normalization='normalized', k=7)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
