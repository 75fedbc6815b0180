"""CPU: the host-side glue of ssl.laplace(order=2 | 3), vector tau and their operator cache, on the 600-vertex fixture of
tests/golden/g24_laplace_order.npz.  scipy's SpGEMM leaves the rows of L*L unsorted, so everything that is written for canonical rows
has to step aside: the Laplacian handed to the device must be the oracle's entry for entry IN STORED ORDER, and the right-hand side
must be the literal `-L[:, train_ind] * F` (a row's terms added in stored order).  The device object is a stub here."""
import numpy as np
import pytest
from scipy import sparse

import graphlearning_amd as gl
from graphlearning_amd import _hip, ssl as glssl
from oracle import gl_oracle as orc
import laplace_order_ref as lo

N = 600


@pytest.fixture(scope='module')
def fix():
    g = lo.load_golden()
    J, D = lo.knn_lists(g, N)
    W = orc.knn_weights(J, D, lo.K)
    ti, lab = lo.training_set(g, N)
    return g, W, ti, lab


class _StubGraph:
    """Stands where _hip.DeviceGraph would: keeps what it was given, touches no device."""
    built = []

    def __init__(self, A, dtype=np.float64, device=None, keep_order=False, order=None):
        self.A, self.keep_order, self.order, self.closed = sparse.csr_matrix(A), keep_order, order, False
        _StubGraph.built.append(self)

    def close(self):
        self.closed = True


@pytest.fixture
def stub(monkeypatch):
    _StubGraph.built = []
    monkeypatch.setattr(_hip, 'DeviceGraph', _StubGraph)
    return _StubGraph


def _same_csr(A, B):
    return np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and np.array_equal(A.data, B.data)


@pytest.mark.parametrize('order', lo.ORDERS)
@pytest.mark.parametrize('norm', lo.NORMS)
@pytest.mark.parametrize('tau', lo.TAUS)
def test_laplacian_and_rhs_equal_the_oracle_in_stored_order(fix, order, norm, tau):
    g, W, ti, lab = fix
    tv = lo.tau_value(g, N, tau)
    model = gl.ssl.laplace(W, normalization=norm, tau=tv, order=order)
    L = sparse.csr_matrix(model._laplacian(model.graph))
    Lo = sparse.csr_matrix(orc.laplace_operator(W, norm, tv, order))
    assert _same_csr(L, Lo)
    assert not L.has_sorted_indices                       # SpGEMM order: the canonical-row routes must not be taken
    # the census that makes the case one: long rows, and a right-hand side whose rows are sums of three and more terms
    assert lo.longest_row(L) > (64 if order == 2 else 256)
    assert lo.rows_with_three(L, ti) >= 40
    F = orc.labels_to_onehot(lab, lo.CLASSES)
    b = glssl._neg_columns_times(L, L.tocsc(), ti, F)
    assert np.array_equal(b, -Lo[:, ti] * F)
    assert glssl._neg_columns_times_rows(L, L.tocsc(), ti, F) is None
    # ... and stored order is not ascending-column order: summed the canonical way, some row of b comes out with other bits (tau = 0,
    # order 2, combinatorial is the case the issue's census was taken on; the others are not asserted to differ)
    if (order, norm, tau) == (2, 'combinatorial', '0'):
        Ls = L.copy()
        Ls.sort_indices()
        assert not np.array_equal(-Ls[:, ti] * F, b)


def test_order_three_is_not_symmetric_bit_for_bit(fix):
    g, W, ti, lab = fix
    L3 = sparse.csr_matrix(gl.ssl.laplace(W, order=3)._laplacian(gl.graph.graph(W)))
    asym = abs(L3 - L3.T).max()
    assert 0 < asym < 1e-12
    assert abs(orc.laplace_operator(W, order=3) - L3).max() == 0


def test_names_equal_the_reference(fix):
    g, W, ti, lab = fix
    seen = set()
    for case in lo.CASES:
        n, order, norm, tau, ms = case
        if n != N:
            continue
        model = gl.ssl.laplace(W, normalization=norm, tau=lo.tau_value(g, N, tau), order=order, mean_shift=ms)
        key = lo.case_key(*case)
        assert model.accuracy_filename == str(g['fname_' + key]), key
        assert model.name == str(g['name_' + key]), key
        seen.add(model.accuracy_filename)
    assert {'_laplace_order2', '_laplace_order3', '_laplace_tau_0.020', '_laplace_normalized_meanshift_order3_tau_0.020'} <= seen
    assert '_tau_%.3f' % np.max(g['tau%d' % N]) == '_tau_0.020'


def test_full_system_cache_key(fix, stub):
    """One operator per (graph, normalization, tau bytes, order): every change of one of them rebuilds it and closes the old one; an
    unchanged model keeps the object.  The operator is M L M of the oracle's L, entries in stored order, uploaded with keep_order."""
    g, W, ti, lab = fix
    tau = np.array(g['tau%d' % N])
    model = gl.ssl.laplace(W)
    seen = []

    def system(**attrs):
        for k, v in attrs.items():
            setattr(model, k, v)
        L, Mv, dev = model._full_system()
        again = model._full_system()
        assert again[2] is dev and again[0] is L                 # asked twice: the cached objects
        assert all(dev is not d for d in seen) and not dev.closed
        assert all(d.closed for d in seen)                       # what it replaces is closed
        seen.append(dev)
        return L, Mv, dev

    flat = np.ones(N) * tau.max()                                # a scalar tau as the constructor stores it
    other = tau.copy()
    other[N // 2] = np.nextafter(other[N // 2], 1)               # one entry, one ulp
    assert other.max() == tau.max() == flat.max()
    steps = [dict(order=1), dict(order=2), dict(order=3), dict(order=2, tau=flat), dict(tau=tau), dict(tau=other),
             dict(normalization='normalized'), dict(order=1, tau=np.zeros(N), normalization='combinatorial')]
    for step in steps:
        L, Mv, dev = system(**step)
        Lo = sparse.csr_matrix(orc.laplace_operator(W, model.normalization, model.tau, model.order))
        assert _same_csr(sparse.csr_matrix(L), Lo)
        M = sparse.spdiags(1 / np.sqrt(Lo.diagonal() + 1e-10), 0, N, N).tocsr()
        assert _same_csr(dev.A, sparse.csr_matrix(M * Lo * M)) and dev.keep_order and dev.order is None
        assert np.array_equal(Mv, 1 / np.sqrt(Lo.diagonal() + 1e-10))
    assert len(stub.built) == len(steps)
    # a graph that carries a vertex order hands it on, whatever the order of the Laplacian
    W2 = W.copy()
    W2._glx_order = np.arange(N, dtype=np.int32)[::-1].copy()
    dev = gl.ssl.laplace(W2, order=2)._full_system()[2]
    assert not dev.keep_order and np.array_equal(dev.order, W2._glx_order)
