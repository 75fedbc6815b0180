"""The host half of the eigensolver behind graph.eigen_decomp: thick-restart Lanczos with full reorthogonalisation on B = A A, so
that the k largest SINGULAR values of a symmetric A are found, negative eigenvalues of large modulus included -- what
scipy.sparse.linalg.svds (ARPACK on A^H A) returns.  DESIGN.md 4.12 is the contract.

The driver is written against a small backend interface -- set_column(j, x), orthonormalize(j) -> norm, run(j0, j1) -> (alpha, beta),
rotate(Y, rows, keep), get_columns(j0, j1) -> (n, j1 - j0) -- and owns every decision: the projected matrix, the stop, the restart,
the breakdown test, the probe.  _hip.Eig (the device) and the host restatement of csrc/eig_plan.h run this same code, so a whole
solve is equal bit for bit on both as soon as every operation is.

numpy's global random stream is never touched: the two start vectors come from generators of their own."""
import numpy as np
from scipy import sparse

from ._hip import GlxError

START_SEED = 20240229           # of the start vector
PROBE_SEED = 20240301           # of the probe's vector
MAX_K = 256
MAX_M = 513
PROBE_STEPS = 20
STOP_FLOOR = 2.0 ** -46         # tol = 0 means machine precision, as in ARPACK
TINY = 2.0 ** -40               # a beta below TINY * max|alpha| ends the Krylov space; the probe's margin over theta_{k-1}


def basis_size(n, k):
    """ARPACK's ncv as scipy's svds chooses it"""
    return int(min(max(2 * k + 1, 20), n))


def _breakdown(alpha, beta, amax, last_counts):
    """index of the first step of a run whose coefficients end the Krylov space, or -1"""
    for i in range(len(alpha)):
        if not np.isfinite(alpha[i]):
            return i
        amax = max(amax, abs(alpha[i]))
        if (i < len(alpha) - 1 or last_counts) and not (np.isfinite(beta[i]) and beta[i] > TINY * amax):
            return i
    return -1


def thick_restart(backend, n, k, tol=0.0, m=None, max_restarts=None):
    """The k largest eigenvalues theta of B = A A, descending, with their vectors left in the columns 0 .. k - 1 of the backend's
    basis.  Returns (theta (k), Lanczos steps of the solve, restarts, the probe's largest Ritz value or None when n == m).
    GlxError: a breakdown (fewer reachable distinct eigenvalues than m), a missed multiple eigenvalue found by the probe, or no
    convergence within max_restarts (default 10 n, ARPACK's maxiter)."""
    n, k = int(n), int(k)
    m = basis_size(n, k) if m is None else int(m)
    if not (1 <= k < n and k <= MAX_K and k <= m <= min(n, MAX_M)) or (m == k and n != m):
        raise ValueError('thick_restart: need 1 <= k < n, k <= %d and k < m <= min(n, %d) (n=%d k=%d m=%d)' % (MAX_K, MAX_M, n, k, m))
    if max_restarts is None:
        max_restarts = 10 * n
    tol = float(tol)
    backend.set_column(0, np.random.default_rng(START_SEED).random(n))
    backend.orthonormalize(0)
    T = np.zeros((m, m))
    j0, steps, restarts = 0, 0, 0
    while True:
        alpha, beta = backend.run(j0, m)
        steps += m - j0
        amax = float(np.abs(np.diag(T)[:j0]).max()) if j0 else 0.0
        bad = _breakdown(alpha, beta, amax, last_counts=False)
        if bad >= 0:
            raise GlxError('eigensolver breakdown at Lanczos step %d of a basis of %d: the start vector reaches fewer distinct eigenvalues '
                           'than the basis has columns (beta=%r); no partial result is returned' % (j0 + bad, m, float(beta[bad])))
        for i, j in enumerate(range(j0, m)):
            T[j, j] = alpha[i]
            if j < m - 1:
                T[j, j + 1] = T[j + 1, j] = beta[i]
        beta_m = float(beta[-1])
        w, Y = np.linalg.eigh(T)
        theta, Y = w[::-1].copy(), np.ascontiguousarray(Y[:, ::-1])
        if n == m:                   # the run spans the whole space: its Ritz pairs are the eigenpairs whatever beta_{m-1} is
            break
        if not np.isfinite(beta_m):
            raise GlxError('eigensolver breakdown at Lanczos step %d of a basis of %d (beta=%r); no partial result is returned'
                           % (m - 1, m, beta_m))
        if np.abs(beta_m * Y[m - 1, :k]).max() <= max(tol, STOP_FLOOR) * theta[0]:
            break
        if restarts >= max_restarts:
            raise GlxError('eigensolver: no convergence within %d restarts (n=%d k=%d m=%d)' % (max_restarts, n, k, m))
        keep = k + (m - k) // 2
        backend.rotate(np.ascontiguousarray(Y[:, :keep]), m, keep)
        s = beta_m * Y[m - 1, :keep]
        T[:] = 0.0
        T[np.arange(keep), np.arange(keep)] = theta[:keep]
        T[keep, :keep] = s
        T[:keep, keep] = s
        j0 = keep
        restarts += 1
    backend.rotate(np.ascontiguousarray(Y[:, :k]), m, k)
    probe = None
    if n != m:
        # A single-vector Krylov method finds one vector per distinct eigenvalue.  A second random vector, made orthogonal to the k
        # converged ones, is run for a few steps: a Ritz value of its tridiagonal block is a LOWER bound of an eigenvalue of B on the
        # complement, so one above theta_{k-1} proves that a copy was missed.  Detection only: silence proves nothing, nothing is repaired.
        p = min(PROBE_STEPS, m - k)
        backend.set_column(k, np.random.default_rng(PROBE_SEED).random(n))
        backend.orthonormalize(k)
        a, b = backend.run(k, k + p)
        bad = _breakdown(a, b, float(theta[0]), last_counts=False)
        q = p if bad < 0 else (bad + 1 if np.isfinite(a[bad]) else bad)          # the complement is exhausted: its Ritz values are exact
        if q >= 1:
            Tp = np.diag(a[:q]) + np.diag(b[:q - 1], 1) + np.diag(b[:q - 1], -1)
            probe = float(np.linalg.eigvalsh(Tp).max())
            if probe > theta[k - 1] + TINY * theta[0]:
                raise GlxError('eigensolver: a multiple eigenvalue was missed: the probe finds %.17g above theta[k-1]=%.17g in the complement '
                               'of the %d converged vectors (a disconnected or bipartite graph does this); no result is returned'
                               % (probe, float(theta[k - 1]), k))
    return theta[:k].copy(), steps, restarts, probe


def operator(W, normalization):
    """(A, D, M): the symmetric matrix whose largest singular values are wanted, built on the host entry by entry as the reference
    builds it (graph.py:728-753) -- D W D with D = degree_matrix(p=-0.5) (and D itself) for 'normalized' and 'randomwalk', M I - L with
    M = 2 max(deg) for 'combinatorial' -- as a canonical CSR matrix."""
    n = W.shape[0]
    deg = W * np.ones(n)
    if normalization in ('normalized', 'randomwalk'):
        D = sparse.spdiags(deg ** (-0.5), 0, n, n).tocsr()
        A, M = D * W * D, None
    elif normalization == 'combinatorial':
        D = None
        L = (sparse.spdiags(deg, 0, n, n).tocsr() - W).tocsr()
        M = 2 * np.max(deg)
        A = M * sparse.identity(n) - L
    else:
        raise ValueError('Invalid choice of normalization')
    A = sparse.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A, D, M


def check_weights(W, normalization, k):
    """The stated deviations of graph.eigen_decomp, each a ValueError before any device call."""
    n = W.shape[0]
    if not (1 <= int(k) < n):
        raise ValueError('eigen_decomp: k=%d outside [1, n) (n=%d); scipy.sparse.linalg.svds refuses it too' % (k, n))
    if k > MAX_K:
        raise ValueError('eigen_decomp: k=%d above %d' % (k, MAX_K))
    if W.shape[0] != W.shape[1]:
        raise ValueError('eigen_decomp: the weight matrix is not square')
    if not np.all(np.isfinite(W.data)) or np.any(W.data < 0):
        raise ValueError('eigen_decomp: NaN, infinite or negative weights')
    C = sparse.csr_matrix(W)
    if not C.has_canonical_format:
        C = C.copy()
        C.sum_duplicates()
    Ct = sparse.csr_matrix(C.T)
    Ct.sort_indices()
    # (stored zeros count as entries on both sides: a matrix with a stored zero on one side only is refused although it is symmetric)
    if not (np.array_equal(C.indptr, Ct.indptr) and np.array_equal(C.indices, Ct.indices) and C.data.tobytes() == Ct.data.tobytes()):
        raise ValueError('eigen_decomp: the weight matrix is not symmetric bit for bit (svds would work on A^H A; the weight matrices '
                         'this package builds are symmetric)')
    if normalization in ('normalized', 'randomwalk') and np.any(W * np.ones(n) == 0):
        raise ValueError("eigen_decomp: a vertex of degree 0 (the reference divides by zero for normalization='%s')" % normalization)
