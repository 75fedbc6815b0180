"""Helpers on the hot path (reference graphlearning/utils.py), restated; `conjgrad` runs on the GPU."""
import sys
import numpy as np
from scipy import sparse
from . import _hip


def labels_to_onehot(labels, k, standardize=False):
    """One-hot encoding, reference utils.py:536-572.  Width = max(max(labels)+1, k)."""
    labels = np.asarray(labels)
    n = labels.shape[0]
    k = max(int(np.max(labels)) + 1, k)
    if standardize:
        uniq = np.unique(labels)
        k = len(uniq)
        labels = np.searchsorted(uniq, labels)
    labels = labels.astype(int)
    onehot = np.zeros((n, k))
    onehot[np.arange(n), labels] = 1
    return onehot


def boundary_statistic(X, r, knn=False, return_normals=False, second_order=True, cutoff=True, knn_data=None, device=None):
    """Boundary test statistic of a point cloud (reference utils.py:18-114, plus `device`; J. Calder, S. Park, D. Slepcev, Boundary
    Estimation from Point Clouds, arXiv:2111.03217): T (n,) float64, small at the boundary; with return_normals=True (T, nu), nu (n, d)
    the estimated unit normals.

    Radius mode: the ball graph of weightmatrix.epsilon_ball(X, r, kernel='uniform'); kNN mode (knn=True, r = k neighbours with self
    counted): the lists of weightmatrix.knnsearch(X, k), or `knn_data`, and the graph weightmatrix.knn(X, k, kernel='uniform',
    symmetrize=False, knn_data=...).  Everything behind the graph is one device call (csrc/bstat.hip): the normals equal the
    reference's bit for bit, T as numbers (a zero is +0.0; the reference leaves its sign to np.max over a masked product).
    Where the reference's second search and this walk over the ball graph part ways, the call refuses with ValueError before any
    device call: a vertex with no neighbour (the reference divides 0 by 0 and spreads the NaN), non-finite X, a negative or NaN
    radius, a k that is no integer in 2 .. min(n, 1024), knn_data with fewer than k or more than min(n, 1024) columns, other row
    counts or an index out of range, a duplicate in a neighbour list (a weight other than 1).  knn_data wider than k is used as the
    reference uses it: the graph from its first k + 1 columns, the maximum over all of them.  A normal of norm zero (a lattice; the reference returns NaN there
    and around it) raises GlxError naming the vertex.  Radius-mode membership is the ball graph's sq <= r*r; the reference masks its
    lists with sqrt(sq) <= r, which can differ for a pair within rounding of the radius."""
    from . import weightmatrix           # (weightmatrix imports utils)
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError('boundary_statistic: X must be (n, d) with n, d >= 1 (got shape %s)' % (X.shape,))
    if not np.isfinite(X).all():
        raise ValueError('boundary_statistic: X must be finite')
    n = X.shape[0]
    J = None
    if knn:
        if isinstance(r, (bool, np.bool_)) or not isinstance(r, (int, np.integer)):
            if not (isinstance(r, (float, np.floating)) and float(r).is_integer()):
                raise ValueError('boundary_statistic: with knn=True r is the number of neighbours, an integer (got %r)' % (r,))
        k = int(r)
        if k < 2 or k > min(n, 1024):
            raise ValueError('boundary_statistic: k = %d outside 2 .. min(n, 1024) = %d' % (k, min(n, 1024)))
        if knn_data is not None:
            J, D = np.asarray(knn_data[0]), np.asarray(knn_data[1])
            if J.ndim != 2 or D.ndim != 2 or J.shape != D.shape or J.shape[0] != n or not k <= J.shape[1] <= min(n, 1024):
                raise ValueError('boundary_statistic: knn_data must be two (n, k .. min(n, 1024)) arrays (got %s and %s for n = %d, k = %d)'
                                 % (J.shape, D.shape, n, k))
            if J.dtype.kind not in 'iu':
                raise ValueError('boundary_statistic: knn_data indices must be integers, not %s' % J.dtype)
            if J.size and (int(J.min()) < 0 or int(J.max()) >= n):
                raise ValueError('boundary_statistic: knn_data holds an index outside 0 .. n - 1')
            # as in the reference, wider lists are used in full: weightmatrix.knn counts self on top of k and builds the graph
            # from the first k + 1 columns, the maximum runs over every column handed in
            Js = np.sort(J[:, :k + 1], axis=1)
            if (Js[:, 1:] == Js[:, :-1]).any():
                raise ValueError('boundary_statistic: a neighbour list of knn_data names a vertex twice (a weight other than 1)')
        else:
            J, D = weightmatrix.knnsearch(X, k, device=device)
        W = weightmatrix.knn(X, k, kernel='uniform', symmetrize=False, knn_data=(J, D), device=device)
        J = np.ascontiguousarray(J, dtype=np.int32)
    else:
        if isinstance(r, (bool, np.bool_)) or not isinstance(r, (int, float, np.integer, np.floating)) or not r >= 0:
            raise ValueError('boundary_statistic: the radius must be a number, not negative or NaN (got %r)' % (r,))
        W = weightmatrix.epsilon_ball(X, r, kernel='uniform', device=device)
    W = sparse.csr_matrix(W)
    if not W.has_canonical_format:
        W.sum_duplicates()
    if (W.data != 1).any():
        raise ValueError('boundary_statistic: a weight other than 1 (a neighbour list names a vertex twice)')
    if (np.diff(W.indptr) == 0).any():
        raise ValueError('boundary_statistic: vertex %d has no neighbour (the reference divides 0 by 0 there)'
                         % int(np.flatnonzero(np.diff(W.indptr) == 0)[0]))
    T, nu = _hip.boundary_stat(X, W.indptr, W.indices, second_order=bool(second_order), cutoff=bool(cutoff), J=J, device=device)
    if return_normals:
        return T, nu
    return T


def class_priors(labels):
    """Fraction of data in each class, negative labels ignored (reference utils.py:117-142)."""
    labels = np.asarray(labels)
    classes = np.unique(labels)
    classes = classes[classes >= 0]
    total = np.sum(labels >= 0)
    priors = np.zeros((len(classes),))
    for i, c in enumerate(classes):
        priors[i] = np.sum(labels == c) / total
    return priors


def sparse_max(A, B):
    """Element-wise max of two non-negative square sparse matrices (reference utils.py:263-286)."""
    nz = (A + B) > 0
    b_wins = B > A
    a_wins = nz - b_wins
    return A.multiply(a_wins) + B.multiply(b_wins)


def conjgrad(A, b, x0=None, max_iter=1e5, tol=1e-10, dtype=np.float64, return_info=False, device=None, reduce='exact'):
    """Multi right-hand-side conjugate gradient, reference utils.py:483-532, on the GPU
    (glx_cg_solve).  Per-column alpha/beta, global stop sqrt(sum_cols ||r||^2) <= tol.
    With x0 the iteration starts like the reference's: `x = x0.copy(); r = b - A@x` (utils.py:510-514,
    the residual formed on the host with the reference's own expression) and x accumulates from x0.
    reduce='tree' selects the tolerance mode of the reductions (include/glx.h GLX_CG_TREE)."""
    G = _hip.DeviceGraph(sparse.csr_matrix(A), dtype=dtype, device=device, keep_order=True)
    try:
        if x0 is None:
            x, it, err = G.cg(np.asarray(b), tol=tol, max_iter=int(max_iter), reduce=reduce)
        else:
            x0 = np.asarray(x0)
            r0 = b - A @ x0
            x, it, err = G.cg(r0, tol=tol, max_iter=int(max_iter), x0=x0, reduce=reduce)
    finally:
        G.close()
    return (x, it, err) if return_info else x


def _boundary_handling(bdy_set, bdy_val):
    """Boundary data in standard form: index array + value array (reference utils.py:144-174)."""
    if type(bdy_set) == list:
        bdy_set = np.array(bdy_set)
    if bdy_set.dtype == bool:
        bdy_set = np.where(bdy_set)[0]
    m = len(bdy_set)
    if type(bdy_val) != np.ndarray:
        bdy_val = np.ones((m,)) * bdy_val
    return bdy_set, bdy_val


def matrix_fingerprint(W):
    """Content fingerprint of a scipy sparse matrix: shape, nnz and a 128-bit hash of its three arrays (the library's threaded
    host hash: ~0.2 ms for the 25 MB of the config-3 graph; hashlib's blake2b when the library is not built).  The
    device-resident operators of the learners are keyed by it, so a matrix whose values were edited IN PLACE between two fits
    is seen as a new graph -- the reference rebuilds its operator on every fit (ssl.py:615-644), an `id(W)` key would silently
    reuse the stale one."""
    arrays = [np.ascontiguousarray(getattr(W, name)) for name in ('data', 'indices', 'indptr') if hasattr(W, name)]
    if not arrays:                                          # a dense matrix or another sparse format
        arrays = [np.ascontiguousarray(sparse.csr_matrix(W).data)]
    digest = _hip.host_fingerprint(arrays)
    if digest is None:                                      # slower, same role
        import hashlib
        h = hashlib.blake2b(digest_size=16)
        for a in arrays:
            h.update(memoryview(a).cast('B'))
        digest = int.from_bytes(h.digest(), 'little')
    return (tuple(W.shape), int(getattr(W, 'nnz', arrays[0].size)), str(arrays[0].dtype), digest)


def symmetric_fingerprint(W):
    """What weightmatrix.knn stamps on a matrix it has just symmetrised (attribute `_glx_sym`), so that later consumers may
    skip forming W^T: the content fingerprint.  Any edit -- of the structure or of a single value in place -- gives another
    fingerprint, and the matrix is then treated as unknown (the general, transposing operator build)."""
    return matrix_fingerprint(W)


def known_symmetric(W, fingerprint=None):
    """Is W a matrix weightmatrix.knn symmetrised, unchanged since?  `fingerprint`: matrix_fingerprint(W) if the caller has it."""
    tag = getattr(W, '_glx_sym', None)
    if tag is None:
        return False
    return tag == (matrix_fingerprint(W) if fingerprint is None else fingerprint)
