"""The two gather stages of the sweep kernel (csrc/sweep.hip: gather_quad at 4 lanes per row, gather_wide at 8, 16, 32 and 64) at
every width and every segment class, on the smallest graph that reaches them: 640 rows whose lengths cycle through both sides of
the row classes 24 / 96 (and of the relaxed plans' 64 / 256), every remainder mod 4 and an empty row; distinct columns in unsorted
stored order, weights of both signs.

Reference: a host loop over the entries of a row in stored order, `acc = acc + (x * v)` as two separately rounded numpy operations
in the state's dtype, then `Db + acc` -- the order and the roundings of scipy's csr_matvecs, which the fixture proves on the CPU by
comparing the loop with `A @ u` in float64.  The device is held to equal bits."""
import numpy as np
import pytest
from scipy import sparse
from sweep_ref import host_sweep      # the entry-order loop (tests/test_sweep_ref_host.py holds it against scipy too)

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 3, 4, 5, 23, 24, 25, 63, 64, 65, 95, 96, 97, 255, 256, 257, 300]
N = 640
WIDTHS = [1, 16, 17, 33, 65, 129]         # 4, 4, 8, 16, 32, 64 lanes per row


@pytest.fixture(scope='module')
def gl():
    import graphlearning_amd as gl
    from graphlearning_amd import _hip
    _hip.require_device()
    return gl


def _graph(seed):
    rng = np.random.default_rng(seed)
    lengths = np.array([LENGTHS[i % len(LENGTHS)] for i in range(N)])
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    indices = np.empty(indptr[-1], dtype=np.int32)
    for i in range(N):
        indices[indptr[i]:indptr[i + 1]] = rng.choice(N, size=lengths[i], replace=False)
    A = sparse.csr_matrix((rng.normal(size=indptr[-1]), indices, indptr), shape=(N, N))
    A.has_sorted_indices = False
    return A, lengths


@pytest.fixture(scope='module')
def forms(gl):
    """The graph, its operands at the widest width, and one operator per dtype (every width's plan lives in it)."""
    from graphlearning_amd import _hip
    A, lengths = _graph(11)
    assert set(lengths.tolist()) == set(LENGTHS) and 57000 < A.nnz < 59000
    last = A.indices[A.indptr[-2]:A.indptr[-1]]
    assert len(last) > 1 and not np.all(np.diff(last) > 0)                          # stored order: unsorted
    assert all(len(set(A.indices[A.indptr[i]:A.indptr[i + 1]].tolist())) == lengths[i] for i in range(N))
    assert A.data.min() < 0 < A.data.max()
    rng = np.random.default_rng(12)
    u = rng.normal(size=(N, max(WIDTHS)))
    Db = rng.normal(size=(N, max(WIDTHS)))
    assert np.array_equal(host_sweep(A, u, None, np.float64), A @ u)                # the reference itself, against scipy
    assert np.array_equal(host_sweep(A, u, Db, np.float64), Db + A @ u)
    graphs = {dt: _hip.DeviceGraph(A, dtype=dt, keep_order=True) for dt in (np.float64, np.float32)}
    for G in graphs.values():
        assert np.array_equal(G.order(), np.arange(N)) and G.info()['max_row'] == max(LENGTHS)
    yield A, u, Db, graphs
    for G in graphs.values():
        G.close()


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('C', WIDTHS)
def test_spmm_bias_equals_the_entry_order_loop(forms, C, dtype):
    """With and without Db, one and two applications."""
    A, u, Db, graphs = forms
    G = graphs[dtype]
    uc = np.ascontiguousarray(u[:, :C]).astype(dtype)
    for bias in (np.ascontiguousarray(Db[:, :C]).astype(dtype), None):
        ref = uc
        for iters in (1, 2):
            ref = host_sweep(A, ref, bias, dtype)
            got = G.spmm_bias(uc, bias, iters=iters)
            assert got.dtype == dtype and got.shape == (N, C)
            assert np.array_equal(got, ref), (C, np.dtype(dtype).name, bias is not None, iters)
