"""The Gaussian weights of weightmatrix.knn and weightmatrix.epsilon_ball in their DEFAULT mode, restated without the library and
without csrc/exp_cr.h (numpy, scipy and `decimal` only): the reference's own expressions (graphlearning/weightmatrix.py:140-187,
oracle/gl_oracle.py::knn_weights) with np.exp replaced by the exponential that exp_cr.h promises.  Every operation before and
after the exponential is one IEEE operation that numpy performs as the device does, and the exponential has an exact answer, so
the device's W has to equal what this module computes bit for bit (tests/test_gpu_weights_exact.py); tests/test_weights_cr_ref_host.py
checks the module itself.

The promise of exp_cr.h: the exact exp(x) rounded once to 53 bits (round to nearest even); where that lies below 2^-1022 it is
then rounded a second time, onto the subnormal grid."""
from decimal import Decimal, localcontext

import numpy as np
from scipy import sparse

EXP_OVERFLOW = 709.782712893384         # above: inf (the thresholds of exp_cr.h, restated)
EXP_ZERO = -745.2                       # below: 0
TWO_STEP_BELOW = -700.0                 # below this argument the second rounding is applied (it changes nothing above 2^-1022)
_TWO200 = Decimal(2) ** 200
_LD = np.longdouble


def _exp_decimal(x):
    with localcontext() as c:
        c.prec = 60
        return Decimal(float(x)).exp()


def exp_rounded_once_scalar(x):
    x = float(x)
    if x != x:
        return x
    if x > EXP_OVERFLOW:
        return np.inf
    if x < -800.0:
        return 0.0
    return float(_exp_decimal(x))


def exp_contract_scalar(x):
    x = float(x)
    if x != x:
        return x
    if x > EXP_OVERFLOW:
        return np.inf
    if x < EXP_ZERO:
        return 0.0
    e = _exp_decimal(x)
    if x >= TWO_STEP_BELOW:
        return float(e)
    with localcontext() as c:
        c.prec = 140                    # 60 digits times the 61 digits of 2^200: the product is exact
        m = float(e * _TWO200)          # first rounding: 53 bits, as if the exponent range had no end
    return float(np.ldexp(m, -200))     # second rounding: onto the subnormal grid (exact where the result is normal)


def exp_rounded_once(x):
    """float(Decimal(x).exp()) everywhere: ONE rounding, also onto the subnormal grid -- what exp_contract is counted against."""
    x = np.asarray(x, dtype=np.float64)
    return np.array([exp_rounded_once_scalar(v) for v in x.ravel()]).reshape(x.shape)


def exp_contract_decimal(x):
    """exp_contract by Decimal alone, value by value (about 30 us each)."""
    x = np.asarray(x, dtype=np.float64)
    return np.array([exp_contract_scalar(v) for v in x.ravel()], dtype=np.float64).reshape(x.shape)


def hard_values(x):
    """Which arguments the fast path of exp_contract hands to Decimal: the long-double exponential lies within 2^-8 of a float64
    spacing from a rounding boundary (a long-double exp is good to about 2^-11 of that spacing), the result is a power of two
    (the spacing below it is half the one above), anything non-finite, and every result below 2.3e-308."""
    x = np.asarray(x, dtype=np.float64).ravel()
    with np.errstate(all='ignore'):
        ld = np.exp(x.astype(_LD))
        y = ld.astype(np.float64)
        frac = np.abs((ld - y.astype(_LD)) / np.spacing(y).astype(_LD))
        hard = ~np.isfinite(x) | ~np.isfinite(y) | (y < 2.3e-308) | ~(frac < _LD(0.5) - _LD(2.0) ** -8)
        hard |= (y.view(np.int64) & ((1 << 52) - 1)) == 0
    return y, hard


def exp_contract(x, stats=None):
    """The exponential csrc/exp_cr.h promises, elementwise over an array.  stats (a dict): receives how many values went to
    Decimal."""
    x = np.asarray(x, dtype=np.float64)
    if np.finfo(_LD).nmant < 63:
        return exp_contract_decimal(x)
    y, hard = hard_values(x)
    at = np.flatnonzero(hard)
    flat = x.ravel()
    for i in at:
        y[i] = exp_contract_scalar(flat[i])
    if stats is not None:
        stats['decimal'] = stats.get('decimal', 0) + len(at)
    return y.reshape(x.shape)


# ---- weightmatrix.knn --------------------------------------------------------------------------------------------------------

def sparse_max(A, B):
    """utils.sparse_max of the reference (graphlearning/utils.py:263-286)."""
    nz = (A + B) > 0
    b_wins = B > A
    a_wins = nz - b_wins
    return A.multiply(a_wins) + B.multiply(b_wins)


def assemble(ind, w, rule):
    """COO -> CSR with duplicates summed, the symmetrisation rule ('mean', 'max', 'symgauss' or 'none'), setdiag(0),
    eliminate_zeros: the reference's scipy expressions (weightmatrix.py:171-186)."""
    n, K = ind.shape
    rows = (np.ones((n, K)) * np.arange(n)[:, None]).flatten()
    W = sparse.coo_matrix((np.asarray(w).flatten(), (rows, np.asarray(ind).flatten())), shape=(n, n)).tocsr()
    if rule == 'max':
        W = sparse_max(W, W.transpose())
    elif rule == 'symgauss':
        W = W + W.T.multiply(W.T > W) - W.multiply(W.T > W)
    elif rule == 'mean':
        W = (W + W.transpose()) / 2
    else:
        assert rule == 'none'
    W.setdiag(0)
    W.eliminate_zeros()
    return W


def knn_arguments(ind, dist, k, kernel):
    """What the Gaussian kernels hand to the exponential, (n, k+1) -- k excludes self and is clamped to the columns at hand."""
    k = int(min(np.shape(ind)[1], k + 1))
    J = np.asarray(ind)[:, :k]
    D = np.asarray(dist, dtype=np.float64)[:, :k]
    with np.errstate(all='ignore'):
        if kernel == 'gaussian':
            sq = D * D
            eps = sq[:, k - 1]
            return (-4 * sq) / eps[:, None]
        if kernel == 'symgaussian':
            eps = D[:, k - 1]
            return -4 * D * D / eps[:, None] / eps[J]
    raise ValueError(kernel)


def knn_kernel_weights_cr(ind, dist, k, kernel):
    """The (n, k+1) weights before the assembly."""
    return exp_contract(knn_arguments(ind, dist, k, kernel))


def knn_weights_cr(ind, dist, k, kernel='gaussian', symmetrize=True):
    """weightmatrix.knn(None, k, kernel, symmetrize=..., knn_data=(ind, dist)) in the default mode."""
    w = knn_kernel_weights_cr(ind, dist, k, kernel)
    J = np.asarray(ind)[:, :w.shape[1]]
    rule = 'none' if not symmetrize else ('symgauss' if kernel == 'symgaussian' else 'mean')
    with np.errstate(all='ignore'):
        return assemble(J, w, rule)


def same_matrix(A, B):
    """indptr, indices and the bytes of data."""
    A, B = sparse.csr_matrix(A), sparse.csr_matrix(B)
    return (A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
            and A.data.dtype == B.data.dtype == np.float64 and A.data.tobytes() == B.data.tobytes())


def differing(A, B):
    """For a failing comparison's message: (same structure, number of stored weights whose bits differ or None)."""
    A, B = sparse.csr_matrix(A), sparse.csr_matrix(B)
    same = A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
    return same, (int(np.sum(A.data.view(np.int64) != B.data.view(np.int64))) if same else None)


# ---- weightmatrix.epsilon_ball -----------------------------------------------------------------------------------------------

def ball_weights_cr(prep, eps, eps_f=1):
    """The Gaussian weight of every pair of epsball_ref.prepare's output, zeros not yet dropped."""
    with np.errstate(all='ignore'):
        w = exp_contract(-4 * prep['dists'] / (eps * eps))
        if prep['fdists'] is not None:
            w = w * exp_contract(-4 * prep['fdists'] / (eps_f * eps_f))
    return w


def ball_matrix_cr(n, prep, eps, eps_f=1):
    """weightmatrix.epsilon_ball(X, eps, features=..., epsilon_f=eps_f) in the default mode: the pairs of `prep` with the weights
    above, zeros dropped."""
    I, J = prep['I'], prep['J']
    if len(I) == 0:
        return sparse.csr_matrix((n, n))
    w = ball_weights_cr(prep, eps, eps_f)
    keep = w != 0
    I, J, w = I[keep], J[keep], w[keep]
    indptr = np.concatenate(([0], np.cumsum(np.bincount(I, minlength=n))))
    W = sparse.csr_matrix((w, J.astype(np.int32), indptr.astype(np.int32)), shape=(n, n))
    W.has_sorted_indices = True
    return W


# ---- lists whose symgaussian arguments sweep the underflow band ------------------------------------------------------------------

def underflow_lists(n=600, K=16, seed=1):
    """Circulant lists (ind[i, t] = (i + t) % n) in which odd rows are tight (k-th distance 4/750) and even rows wide (k-th
    distance 1): a wide row that names a tight vertex evaluates exp(-750 d^2), d^2 uniform in (0, 1) -- and in (0.93, 1) in every
    fourth row, arguments from -697.5 to -750, across the subnormal range and the point where the result becomes zero."""
    rng = np.random.default_rng(seed)
    ind = ((np.arange(n)[:, None] + np.arange(K)[None, :]) % n).astype(np.int64)
    d = np.zeros((n, K))
    d[:, 1:] = np.sqrt(np.sort(rng.uniform(0, 1, size=(n, K - 1)), axis=1))
    band = np.sqrt(np.sort(rng.uniform(0.93, 1, size=(n, K - 1)), axis=1))
    d[::4, 1:] = band[::4]
    d[:, K - 1] = 1
    d[1::2] *= 4 / 750
    return ind, d


def census(x, w):
    """Counts over the arguments x and weights w = exp_contract(x) of a list: subnormal weights, weights in the lowest four
    normal binades, exact zeros, exact zeros outside the last column, and subnormal or zero weights where the two-step contract
    differs from a single rounding."""
    tiny = np.ldexp(1.0, -1022)
    sub = (w > 0) & (w < tiny)
    low = (w >= tiny) & (w < np.ldexp(1.0, -1018))
    zero = w == 0
    at = (w < tiny) & (x >= -760)
    once = exp_rounded_once(x[at])
    return dict(subnormal=int(sub.sum()), low_normal=int(low.sum()), zeros=int(zero.sum()), zeros_inside=int(zero[:, :-1].sum()),
                two_step_differs=int(np.sum(once.view(np.int64) != w[at].view(np.int64))), lowest_argument=float(x.min()))
