"""Lattice data and an exact reference for the kNN search under power-of-two rescaling (tests/test_knn_scale_host.py,
tests/test_gpu_knn_scale.py).

Every point is a vector of integers times a per-column power of two.  After the columns are shifted to their common (smallest)
exponent `pmin`, all pairwise squared distances are integers below 2^53, computed here in int64: every fp64 difference, square and
partial sum of such data is exact in ANY order and with or without fma, so `sqrt(float64(D2)) * 2^pmin` is THE correctly rounded
distance and an exact search must return it bit for bit, ordered by (D2, index).  Multiplying the data by 2^e (|e| small enough for
fp64 to stay normal) is exact and scales everything exactly: the same index lists, distances `ldexp(D, e)`."""
import functools

import numpy as np

# exponents of the scale ladder: every one keeps the fp64 squares of these data finite and normal
LADDER = (0, 8, -8, 24, -24, -50, -56, -60, -62, -64, -66, -68, -70, -72, -75, -80, -100, -400,
          40, 50, 55, 58, 60, 62, 63, 64, 66, 100, 400)
EXACT_COUNT_RANGE = (8, -8, 24, -24)       # scales at which the search takes these data as they come and the filter's arithmetic scales exactly

# name: (style, n, d, k incl. self)
CASES = {
    'gauss20': ('gauss', 2048, 20, 11),
    'gauss3': ('gauss', 2048, 3, 11),
    'gauss200': ('gauss', 700, 200, 15),
    'shell': ('shell', 2000, 64, 27),
    'mixed': ('mixed', 1500, 21, 11),
    'wide': ('gauss', 3000, 20, 101),
    'blobs': ('blobs', 4096, 8, 11),
}


def lattice(style, n, d, seed=1):
    """(M int64 (n, d), p int64 (d,)): the points are M * 2^p (column by column)."""
    rng = np.random.default_rng(seed)
    p = np.zeros(d, dtype=np.int64)
    if style == 'gauss':
        M = np.rint(256 * rng.standard_normal((n, d)))
    elif style == 'shell':
        g = rng.standard_normal((n, d))
        M = np.rint(1024 * g / np.linalg.norm(g, axis=1)[:, None])
    elif style == 'mixed':
        M = np.rint(64 * rng.standard_normal((n, d)))
        p = rng.integers(-6, 7, size=d).astype(np.int64)
    elif style == 'blobs':
        M = np.rint(256 * rng.standard_normal((n, d)))
        cen = np.rint(4096 * rng.standard_normal((16, d)))
        M = M + cen[rng.integers(0, 16, size=n)]
    else:
        raise ValueError(style)
    return M.astype(np.int64), p


def points(M, p, e=0):
    """The fp64 points M * 2^(p + e): exact."""
    return np.ascontiguousarray(np.ldexp(M.astype(np.float64), (p + e)[None, :].astype(np.int64)))


def exact_knn(M, p, k, rows=None):
    """(ind int64 (nq, k), D float64 (nq, k), D2max): the k nearest (self included) of the rows `rows` (all by default), ordered
    by (squared distance, index), from int64 arithmetic on the columns shifted to their common exponent."""
    pmin = int(p.min())
    Z = M << (p - pmin)[None, :]                       # integers: the points in units of 2^pmin
    assert np.abs(Z).max() < 2 ** 30
    Q = Z if rows is None else Z[rows]
    sq = np.einsum('ij,ij->i', Z, Z)
    D2 = np.einsum('ij,ij->i', Q, Q)[:, None] + sq[None, :] - 2 * (Q @ Z.T)
    assert D2.min() >= 0 and D2.max() < 2 ** 53
    order = np.argsort(D2, axis=1, kind='stable')[:, :k]          # stable: ties go to the lower index
    D = np.ldexp(np.sqrt(np.take_along_axis(D2, order, axis=1).astype(np.float64)), pmin)
    return order.astype(np.int64), D, int(D2.max())


def exact_sqdist(M, p, cols):
    """(D2 int64 (n, len(cols)), pmin): the squared distances from every point to the points `cols`, in units of 4^pmin."""
    pmin = int(p.min())
    Z = M << (p - pmin)[None, :]
    D2 = np.einsum('ij,ij->i', Z, Z)[:, None] + np.einsum('ij,ij->i', Z[cols], Z[cols])[None, :] - 2 * (Z @ Z[cols].T)
    assert D2.min() >= 0 and D2.max() < 2 ** 53
    return D2, pmin


@functools.lru_cache(maxsize=None)
def case(name):
    """(M, p, k, ind, D) of a named case: computed once per process; callers must not write into the arrays."""
    style, n, d, k = CASES[name]
    M, p = lattice(style, n, d)
    ind, D, _ = exact_knn(M, p, k)
    for a in (M, p, ind, D):
        a.setflags(write=False)
    return M, p, k, ind, D


def longdouble_knn(X, k, rows):
    """The same lists from all-pairs direct differences in numpy's longdouble (feature by feature), for the rows `rows`."""
    Xl = X.astype(np.longdouble)
    acc = np.zeros((len(rows), X.shape[0]), dtype=np.longdouble)
    for f in range(X.shape[1]):
        diff = Xl[rows, f][:, None] - Xl[None, :, f]
        acc += diff * diff
    order = np.argsort(acc, axis=1, kind='stable')[:, :k]
    # (the squared distances are exact in either format: the square root is taken in fp64, where it is rounded once)
    return order.astype(np.int64), np.sqrt(np.take_along_axis(acc, order, axis=1).astype(np.float64))


def float64_knn(X, k, rows):
    """The lists from plain fp64 numpy (direct differences, feature by feature) for the rows `rows`."""
    acc = np.zeros((len(rows), X.shape[0]))
    for f in range(X.shape[1]):
        diff = X[rows, f][:, None] - X[None, :, f]
        acc += diff * diff
    order = np.argsort(acc, axis=1, kind='stable')[:, :k]
    return order.astype(np.int64), np.sqrt(np.take_along_axis(acc, order, axis=1))


# ---- the split-bf16 filter's arithmetic on the host (knn_prep_bf16_kernel + the tile kernel's contraction), numpy float32 ------------
def bf16_rn(x):
    """float32 -> the nearest bf16 (ties to even), returned as float32: the prep kernel's f32_to_bf16_rn."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


def bf16_filter_error(X, rows, cerr):
    """The two-piece split of the centred fp32 images, the three split products accumulated in fp32 feature by feature, fp32 norms:
    returns (err, bound) for the queries `rows` against all refs -- err[q] = the largest |filter value - exact dist^2| over the
    refs, bound[q] = cerr * (|q| + rmax)^2 as the re-rank computes it.  numpy keeps fp32 subnormals, as the device does."""
    n, d = X.shape
    mean = X.sum(axis=0) / n
    C = X - mean[None, :]
    x32 = C.astype(np.float32)
    hi = bf16_rn(x32)
    lo = bf16_rn(x32 - hi)
    nrm = np.zeros(n, dtype=np.float32)
    for f in range(d):
        nrm = (x32[:, f] * x32[:, f] + nrm).astype(np.float32)
    dot = np.zeros((len(rows), n), dtype=np.float32)
    for part_q, part_r in ((hi, hi), (hi, lo), (lo, hi)):
        for f in range(d):
            dot = (dot + part_q[rows, f][:, None] * part_r[None, :, f]).astype(np.float32)
    val = (nrm[rows][:, None] + (nrm[None, :] - np.float32(2) * dot)).astype(np.float32)
    exact = np.zeros((len(rows), n))
    for f in range(d):
        diff = X[rows, f][:, None] - X[None, :, f]
        exact += diff * diff
    err = np.abs(val.astype(np.float64) - exact).max(axis=1)
    rmax = np.float32(np.sqrt((C * C).sum(axis=1).max()) * (1.0 + 1e-6))
    rq = np.sqrt(nrm[rows]).astype(np.float64) + float(rmax)
    return err, cerr * rq * rq


def bf16_cerr(d):
    """knn_plan.h: the error constant of the split-bf16 filter for d features in blocks of 16."""
    dpa = next(16 * c for c in (1, 2, 4, 6, 8) if 16 * c >= d)
    return 2.0 * (2.0 ** -17 + (1.5 * (3.0 * dpa + 4.0) + d + 16.0) * 2.0 ** -24)
