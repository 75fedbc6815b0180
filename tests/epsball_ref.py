"""weightmatrix.epsilon_ball restated from its rules, numpy and scipy only (tests/test_epsball_host.py checks it against the
golden vectors of the reference, tests/test_gpu_epsball.py checks the device against it):

  membership   the unordered pair {i, j}, i != j, is an edge iff d2_tree(x_i, x_j) <= epsilon*epsilon in fp64, d2_tree being
               the accumulation order of scipy's cKDTree: four accumulators over blocks of four coordinates, added left to right,
               the remaining coordinates one by one, no fused multiply-add;
  distances    the weights see np.sum(V*V, axis=1) with V = x_i - x_j (numpy's pairwise sum over the row), NOT d2_tree;
  weights      uniform 1 | gaussian exp(-4*dists/(eps*eps)) | distance sqrt(dists) | singular 1/sqrt(dists), 1 where dists == 0;
               eta(dists/(eps*eps)) when a callable is given; times the same kernel of the feature distance with epsilon_f;
  zeros        entries whose weight is exactly 0 are dropped; no pair at all gives the empty (n, n) matrix.
Brute force over all pairs, in row blocks."""
import numpy as np
from scipy import sparse

KERNELS = ('uniform', 'gaussian', 'distance', 'singular')


def d2_tree(x, Y):
    """cKDTree's squared distance between row x (d,) and every row of Y (m, d), in its accumulation order."""
    d = Y.shape[1]
    D = x[None, :] - Y
    S = D * D
    acc = [np.zeros(Y.shape[0]) for _ in range(4)]
    i = 0
    while i + 4 <= d:
        for j in range(4):
            acc[j] = acc[j] + S[:, i + j]
        i += 4
    s = ((acc[0] + acc[1]) + acc[2]) + acc[3]
    while i < d:
        s = s + S[:, i]
        i += 1
    return s


def d2_tree_matrix(X, rows=None):
    """d2_tree between the rows `rows` of X (all by default) and all rows: (len(rows), n), coordinate by coordinate."""
    X = np.asarray(X, dtype=np.float64)
    Q = X if rows is None else X[rows]
    d = X.shape[1]
    acc = [np.zeros((Q.shape[0], X.shape[0])) for _ in range(4)]
    i = 0

    def term(f):
        D = Q[:, f][:, None] - X[:, f][None, :]
        return D * D
    while i + 4 <= d:
        for j in range(4):
            acc[j] = acc[j] + term(i + j)
        i += 4
    s = ((acc[0] + acc[1]) + acc[2]) + acc[3]
    while i < d:
        s = s + term(i)
        i += 1
    return s


def full_d2(X, block=512):
    """d2_tree between all rows, (n, n), filled block by block (for callers that ask several questions of one point set)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    n = X.shape[0]
    out = np.empty((n, n))
    for lo in range(0, n, block):
        out[lo:lo + block] = d2_tree_matrix(X, np.arange(lo, min(n, lo + block)))
    return out


def pairs(X, epsilon, block=1024, D2=None):
    """(I, J) of every ordered pair i != j with d2_tree <= epsilon*epsilon, sorted by (i, j).  D2: full_d2(X) if at hand."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    n = X.shape[0]
    e2 = np.float64(epsilon) * np.float64(epsilon)
    I, J = [], []
    for lo in range(0, n, block):
        rows = np.arange(lo, min(n, lo + block))
        M = (d2_tree_matrix(X, rows) if D2 is None else D2[rows]) <= e2
        M[np.arange(len(rows)), rows] = False
        r, c = np.nonzero(M)
        I.append(rows[r])
        J.append(c)
    return np.concatenate(I), np.concatenate(J)


def kernel_weights(dists, epsilon, kernel, eta):
    with np.errstate(all='ignore'):
        if eta is not None:
            return np.asarray(eta(dists / (epsilon * epsilon)), dtype=np.float64)
        if kernel == 'uniform':
            return np.ones_like(dists)
        if kernel == 'gaussian':
            return np.exp(-4 * dists / (epsilon * epsilon))
        if kernel == 'distance':
            return np.sqrt(dists)
        if kernel == 'singular':
            w = np.sqrt(dists)
            w[dists == 0] = 1
            return 1 / w
    raise ValueError(kernel)


def rowsum_sqdiff(X, I, J, chunk=200000):
    """np.sum(V*V, axis=1) with V = X[I] - X[J], in chunks of pairs (every row is summed on its own: the same bits)."""
    out = np.empty(len(I))
    for lo in range(0, len(I), chunk):
        V = X[I[lo:lo + chunk]] - X[J[lo:lo + chunk]]
        out[lo:lo + chunk] = np.sum(V * V, axis=1)
    return out


def prepare(X, epsilon, features=None, D2=None):
    """The kernel-independent part: the pairs and the distances the weights see."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    I, J = pairs(X, epsilon, D2=D2)
    prep = {'I': I, 'J': J, 'dists': rowsum_sqdiff(X, I, J), 'fdists': None}
    if features is not None:
        prep['fdists'] = rowsum_sqdiff(np.ascontiguousarray(features, dtype=np.float64), I, J)
    return prep


def epsilon_ball(X, epsilon, kernel='gaussian', features=None, epsilon_f=1, eta=None, prep=None):
    """The restated weight matrix (canonical CSR, float64, int32 indices).  prep: prepare(X, epsilon, features) if the caller
    builds several kernels on one point set."""
    n = np.shape(X)[0]
    if prep is None:
        prep = prepare(X, epsilon, features)
    I, J = prep['I'], prep['J']
    if len(I) == 0:
        return sparse.csr_matrix((n, n))
    w = kernel_weights(prep['dists'], epsilon, kernel, eta)
    if features is not None:
        w = w * kernel_weights(prep['fdists'], epsilon_f, kernel, eta)
    keep = w != 0
    I, J, w = I[keep], J[keep], w[keep]
    indptr = np.concatenate(([0], np.cumsum(np.bincount(I, minlength=n))))
    W = sparse.csr_matrix((w, J.astype(np.int32), indptr.astype(np.int32)), shape=(n, n))
    W.has_sorted_indices = True
    return W


def near_boundary(X, epsilon, rel=1e-12, block=1024, D2=None):
    """Is there a pair with 0 < |d2_tree - eps^2| <= rel * eps^2?  (The tree of the reference accepts whole sub-trees by their
    bounding boxes; only for such a pair can that differ from the membership rule.)"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    e2 = np.float64(epsilon) * np.float64(epsilon)
    for lo in range(0, X.shape[0], block):
        rows = np.arange(lo, min(X.shape[0], lo + block))
        G = np.abs((d2_tree_matrix(X, rows) if D2 is None else D2[rows]) - e2)
        if ((G > 0) & (G <= rel * e2)).any():
            return True
    return False


# the golden cases of tests/golden/g13_epsball.npz: name -> (X, epsilon, features, epsilon_f)
def golden_inputs():
    g = np.meshgrid(np.arange(40.0), np.arange(40.0), indexing='ij')
    grid40 = np.stack([g[0].ravel(), g[1].ravel()], axis=1)
    g = np.meshgrid(np.arange(32.0), np.arange(32.0), indexing='ij')
    grid32 = np.stack([g[0].ravel(), g[1].ravel()], axis=1)
    dups = np.repeat(np.random.default_rng(3).random((300, 2)), 3, axis=0)
    rand2 = np.random.default_rng(0).random((1500, 2))
    return {
        'rand2': (rand2, 0.05, None, 1),
        'rand3': (np.random.default_rng(1).random((1500, 3)), 0.12, None, 1),
        'blobs9': (np.random.default_rng(7).normal(size=(1200, 9)), 2.2, None, 1),
        'blobs20': (np.random.default_rng(2).normal(size=(1200, 20)), 4.5, None, 1),
        'grid_int': (grid40, 2.0, None, 1),
        'dups': (dups, 0.06, None, 1),
        'dups0': (dups, 0.0, None, 1),
        'feat': (grid32, 3.0, np.random.default_rng(5).random((1024, 3)), 0.5),
        'rand2_tiny': (rand2, 1e-6, None, 1),
    }


# kernels whose `data` the golden file stores per case (gaussian everywhere; uniform needs the structure alone)
GOLDEN_DATA_KERNELS = {'rand2': KERNELS, 'grid_int': KERNELS, 'dups': KERNELS, 'dups0': KERNELS, 'feat': KERNELS}


def eta_hat(t):
    return np.maximum(1 - t, 0)
