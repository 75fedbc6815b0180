"""The bit-for-bit cover of the DEFAULT mode of weightmatrix.knn and weightmatrix.epsilon_ball: the Gaussian weights computed on
the device (knn_weights_kernel's gaussian and symgaussian branches in csrc/assemble.hip, ball_weight in csrc/ball.hip, both
through csrc/exp_cr.h).  The rest of the suite runs in the compatibility mode (conftest.py sets GLX_HOST_EXP=1: numpy's exp on
the host, handed to the assembly as given weights) and the few older default-mode tests allow 1 to 8 ulps against one host's
numpy -- wide enough for another order of the operations before the exponential, a contraction, or an exponential that is an ulp
off.  None is needed: every operation before and after the exponential is one IEEE operation that numpy performs identically,
and the exponential has an exact answer.  So every comparison here is equality of indptr, indices and the bytes of data with
tests/weights_cr_ref.py (numpy, scipy and decimal only), the one exception being the payload of a NaN (test_kth_neighbour_at_distance_zero).

Recorded on the MI355X (the tests print them): the underflow lists give 744 subnormal and 330 zero weights among 9600, 1488 subnormal
stored weights symmetrised and 744 not, 660 and 330 entries fewer than the uniform kernel stores; on the 30 020 arguments of the
underflow band the device's exp_cr equals the two-step contract everywhere and differs from a single rounding in 274 results.

Every test runs under a time limit of its own: a test that exceeds it ends the whole session on the spot, so nothing more is
started on a device that may have hung."""
import faulthandler
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epsball_ref  # noqa: E402
import weights_cr_ref as ref  # noqa: E402
from conftest import blobs  # noqa: E402
from test_epsball_host import GOLDEN_ENTRIES  # noqa: E402
from test_gpu_wide_graph import _boundary_lists, _circulant, _given_ref  # noqa: E402
from test_weights_cr_ref_host import band_arguments  # noqa: E402

pytestmark = pytest.mark.gpu
TINY = np.ldexp(1.0, -1022)
GAUSSIANS = [(kernel, symmetrize) for kernel in ('gaussian', 'symgaussian') for symmetrize in (True, False)]


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
def orc():
    from oracle import gl_oracle
    return gl_oracle


def assert_bits(W, want, tag):
    if not ref.same_matrix(W, want):
        raise AssertionError('%s: (same structure, weights with other bits) = %s; %d stored entries, the reference %d'
                             % (tag, ref.differing(W, want), W.nnz, want.nnz))


def _lists_match(gl, ind, dist, k, tag):
    for kernel, symmetrize in GAUSSIANS:
        W = gl.weightmatrix.knn(None, k, kernel=kernel, symmetrize=symmetrize, knn_data=(ind, dist.copy()))
        assert_bits(W, ref.knn_weights_cr(ind, dist, k, kernel, symmetrize), (tag, kernel, symmetrize))


@pytest.mark.parametrize('mutual', [False, True])
@pytest.mark.parametrize('K,n', [(11, 700), (32, 1500), (65, 1300)])
def test_lists_every_rule(gl, device_exp, K, n, mutual):
    """Constructed lists through both host branches of the assembly (k <= 64 and above), edges listed from one end and from
    both, a duplicate neighbour, gaussian and symgaussian, symmetrised (the mean; W + W^T*(W^T>W) - W*(W^T>W)) and not.
    n K = 7700 at K = 11 is no multiple of the weights kernel's 256 threads: its last block is part empty."""
    ind, dist, _ = _boundary_lists(K, n, 90 + K, mutual)
    if K == 11:
        assert (n * K) % 256 != 0
    _lists_match(gl, ind, dist, K - 1, (K, n, mutual))


@pytest.mark.parametrize('mutual', [False, True])
def test_lists_wider_than_k(gl, device_exp, mutual):
    """40 columns, k = 10: the k-th distance is column 10 of a row of 40 (not the last one), and the neighbour's is read at the
    same stride.  Expected: the reference on the first 11 columns."""
    ind, dist = _circulant(900, 40, 17, mutual)
    for kernel, symmetrize in GAUSSIANS:
        W = gl.weightmatrix.knn(None, 10, kernel=kernel, symmetrize=symmetrize, knn_data=(ind, dist.copy()))
        want = ref.knn_weights_cr(ind[:, :11].copy(), dist[:, :11].copy(), 10, kernel, symmetrize)
        assert_bits(W, want, ('kk=40', kernel, symmetrize))
        assert_bits(want, ref.knn_weights_cr(ind, dist, 10, kernel, symmetrize), 'the reference clamps alike')


@pytest.mark.parametrize('similarity', ['euclidean', 'angular'])
@pytest.mark.parametrize('k', [10, 70])
def test_from_data(gl, device_exp, k, similarity):
    """weightmatrix.knn(X, k): searched, weighted and assembled on the device, the distances never visit the host (k = 70: the
    wide search plan).  Expected: the reference on the lists of weightmatrix.knnsearch(X, k + 1) (the search has tests of its own)."""
    X, _ = blobs(2000, 5, 4, 31, 2.0)
    ind, dist = gl.weightmatrix.knnsearch(X, k + 1, similarity=similarity)
    ind, dist = np.array(ind), np.array(dist)
    for kernel, symmetrize in GAUSSIANS:
        W = gl.weightmatrix.knn(X, k, kernel=kernel, symmetrize=symmetrize, similarity=similarity)
        assert_bits(W, ref.knn_weights_cr(ind, dist, k, kernel, symmetrize), (k, similarity, kernel, symmetrize))


def test_underflow(gl, device_exp):
    """Symgaussian weights across the subnormal range and past the point where they become zero (weights_cr_ref.underflow_lists):
    zeros are dropped, so the structure hangs on the exact underflow behaviour of exp_cr and of the device's ldexp, and the rule
    W + W^T*(W^T>W) - W*(W^T>W) adds and subtracts subnormal weights.  Then exp_cr alone on the arguments of the host test of the
    band.  Counts printed: subnormal stored weights, dropped entries, two-step against single-rounding differences."""
    from graphlearning_amd import _hip
    ind, d = ref.underflow_lists()
    n, K = ind.shape
    x = ref.knn_arguments(ind, d, K - 1, 'symgaussian')
    c = ref.census(x, ref.exp_contract(x))
    assert c['subnormal'] >= 200 and c['zeros_inside'] >= 20 and c['two_step_differs'] >= 3
    for symmetrize in (True, False):
        W = gl.weightmatrix.knn(None, K - 1, kernel='symgaussian', symmetrize=symmetrize, knn_data=(ind, d.copy()))
        want = ref.knn_weights_cr(ind, d, K - 1, 'symgaussian', symmetrize)
        full = gl.weightmatrix.knn(None, K - 1, kernel='uniform', symmetrize=symmetrize, knn_data=(ind, d.copy()))
        sub = int(((W.data > 0) & (W.data < TINY)).sum())
        print('underflow lists, symmetrize=%s: %d stored weights, %d of them subnormal, %d entries fewer than the uniform kernel stores'
              % (symmetrize, W.nnz, sub, full.nnz - W.nnz))
        assert np.array_equal(W.indptr, want.indptr) and np.array_equal(W.indices, want.indices), symmetrize
        assert_bits(W, want, ('underflow', symmetrize))
        assert sub >= 200 and full.nnz - W.nnz >= c['zeros_inside']
    xb = band_arguments()
    got = _hip.exp_cr(xb)
    want = ref.exp_contract(xb)
    once = ref.exp_rounded_once(xb)
    print('underflow band on the device: %d arguments, %d subnormal results, %d zeros, %d results differ from the two-step contract, %d from a single rounding'
          % (len(xb), int(((got > 0) & (got < TINY)).sum()), int((got == 0).sum()), int((got.view(np.int64) != want.view(np.int64)).sum()),
             int((got.view(np.int64) != once.view(np.int64)).sum())))
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize('mutual', [False, True])
def test_subnormal_given_weights(gl, orc, device_exp, mutual):
    """The merge kernels on subnormal operands: given weights 2^-1060 (1 + t) under the mean of two subnormals (an inexact
    halving), the maximum, the symgaussian rule and unsymmetrised, against the scipy expressions."""
    def eta(t):
        return 2.0 ** -1060 * (1 + t)
    K = 11
    ind, dist, _ = _boundary_lists(K, 700, 90 + K, mutual)
    sq = dist * dist
    w = eta(sq / sq[:, K - 1][:, None])
    assert (w > 0).all() and (w < TINY).all() and len(np.unique(w)) > 1000
    for kernel, symmetrize, rule in [('gaussian', True, 'mean'), ('uniform', True, 'max'), ('symgaussian', True, 'symgauss'),
                                     ('gaussian', False, 'none')]:
        W = gl.weightmatrix.knn(None, K - 1, kernel=kernel, eta=eta, symmetrize=symmetrize, knn_data=(ind, dist.copy()))
        want = _given_ref(orc, ind, w, rule)
        assert want.nnz > 0 and (want.data < TINY).all()
        assert_bits(W, want, ('subnormal given weights', rule, mutual))
        assert_bits(want, ref.assemble(ind, w, rule), 'the two restatements of the assembly')


@pytest.mark.parametrize('symmetrize', [True, False])
def test_kth_neighbour_at_distance_zero(gl, device_exp, symmetrize):
    """30 of 700 rows whose whole list is at distance 0 (K identical points): the reference evaluates exp((-4*0)/0) = exp(NaN) =
    NaN for every entry of such a row, stores them (NaN != 0) off the diagonal, and the mean with the other direction is NaN
    too.  Established from the reference on the host: 300 NaN stored unsymmetrised (30 rows x 10 neighbours), 600 symmetrised
    (their transposes as well; rows 5 and 6 are adjacent, so (5, 6) adds two NaN), all of them 0xfff8000000000000 there.  The device has to hold NaN at exactly those positions -- the payload of
    a NaN is nobody's to define -- and identical bits everywhere else."""
    K, n = 11, 700
    ind, dist = _circulant(n, K, 23)
    rows = np.concatenate([[5, 6], 29 + 24 * np.arange(28)])
    assert len(set(rows.tolist())) == 30 and rows.max() < n
    dist[rows] = 0
    with np.errstate(all='ignore'):
        want = ref.knn_weights_cr(ind, dist, K - 1, 'gaussian', symmetrize)
        W = gl.weightmatrix.knn(None, K - 1, kernel='gaussian', symmetrize=symmetrize, knn_data=(ind, dist.copy()))
    nan = np.isnan(want.data)
    assert int(nan.sum()) == (600 if symmetrize else 300)
    assert np.array_equal(W.indptr, want.indptr) and np.array_equal(W.indices, want.indices)
    assert np.array_equal(np.isnan(W.data), nan)
    assert W.data[~nan].tobytes() == want.data[~nan].tobytes()


@pytest.mark.parametrize('name', sorted(GOLDEN_ENTRIES))
def test_epsilon_ball(gl, device_exp, name):
    """Every golden case of the epsilon-ball graphs with the Gaussian kernel, with the case's features and without: W equals the
    reference's product of exponentials, zeros dropped.  (`dups0`, epsilon = 0: every weight is exp(-0/0), a NaN -- positions
    compared, as above.)"""
    X, eps, F, eps_f = epsball_ref.golden_inputs()[name]
    n = X.shape[0]
    for feats in ([F, None] if F is not None else [None]):
        prep = epsball_ref.prepare(X, eps, feats)
        assert len(prep['I']) == GOLDEN_ENTRIES[name]
        with np.errstate(all='ignore'):
            W = gl.weightmatrix.epsilon_ball(X, eps, features=feats, epsilon_f=eps_f)
            want = ref.ball_matrix_cr(n, prep, eps, eps_f)
        if name == 'dups0':
            assert want.nnz == GOLDEN_ENTRIES[name] and np.isnan(want.data).all()
            assert np.array_equal(W.indptr, want.indptr) and np.array_equal(W.indices, want.indices) and np.isnan(W.data).all()
        else:
            assert_bits(W, want, (name, feats is not None))


def test_epsilon_ball_product_in_the_subnormal_range(gl, device_exp):
    """A feature factor near exp(-737) times a distance factor in [exp(-4), 1]: the product of two normal numbers is rounded onto
    the subnormal grid, or to zero and dropped -- one IEEE multiplication, numpy's bits."""
    rng = np.random.default_rng(24)
    X = rng.random((1500, 2))
    F = rng.choice([0.0, 13.3, 13.57, 13.65], size=(1500, 1))
    prep = epsball_ref.prepare(X, 0.05, F)
    W = gl.weightmatrix.epsilon_ball(X, 0.05, features=F, epsilon_f=1.0)
    want = ref.ball_matrix_cr(1500, prep, 0.05, 1.0)
    sub = int(((want.data > 0) & (want.data < TINY)).sum())
    print('%d pairs, %d stored, %d of them subnormal' % (len(prep['I']), want.nnz, sub))
    assert sub >= 1000 and 0 < len(prep['I']) - want.nnz
    assert_bits(W, want, 'subnormal products')
