"""numpy restatement of what csrc/cc.hip computes: union by minimum, then the roots ranked.  Every stored entry (i, j), i != j, of the
CSR pattern joins i and j whatever its direction or value; the root of a tree is always its smallest vertex, so the final roots are
the components' smallest vertices, and ranking the roots in ascending order is scipy's numbering.

The unions run in vectorised rounds here (every entry hooks the larger of its two roots under the smaller with np.minimum.at, then
all pointers jump to their roots) -- one more interleaving of the same hooks; the result does not depend on it."""
import numpy as np


def components(indptr, indices, n):
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    if len(indptr) != n + 1 or indptr[0] != 0 or indptr[-1] != len(indices) or (np.diff(indptr) < 0).any():
        raise ValueError('row pointers do not describe %d entries in %d rows' % (len(indices), n))
    if len(indices) and (indices.min() < 0 or indices.max() >= n):
        raise ValueError('column index out of range')
    a = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    b = indices
    parent = np.arange(n, dtype=np.int64)
    while True:
        ra, rb = parent[a], parent[b]                       # roots: the pointers were flattened at the end of the round before
        hi, lo = np.maximum(ra, rb), np.minimum(ra, rb)
        move = hi != lo
        if not move.any():
            break
        np.minimum.at(parent, hi[move], lo[move])           # hooks only go downward: parent[x] <= x throughout
        while True:                                          # flatten
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
    assert (parent <= np.arange(n)).all() and np.array_equal(parent[parent], parent)
    is_root = parent == np.arange(n)
    rank = np.cumsum(is_root) - is_root                      # exclusive prefix sum of the flags
    return int(is_root.sum()), rank[parent].astype(np.int32)
