#!/usr/bin/env python3
"""Generate tests/golden/g24_laplace_order.npz from THE REFERENCE: ssl.laplace(order=2 | 3), ssl.laplace(tau=<vector>) and
ssl.randomwalk(alpha=...) on the CPU.

Run where the reference is importable (it never travels to the GPU box):

    PYTHONPATH=<the reference's checkout> PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg \
        python3 tests/golden/make_golden_laplace_order.py        (from the repository root)

The cases are laplace_order_ref.CASES.  Per size n in (600, 2000): 3 Gaussian blobs in 5 dimensions (`X<n>`, float32 values),
their classes (`labels<n>`), the reference's kNN lists for 10 neighbours and self (`J<n>` int32, `D<n>`), laplace_order_ref.TRIALS
training sets of 5 labels per class (`train<n>`; set 0 is the one every single fit uses) and a random tau vector in [0, 0.02]
(`tau<n>`).  Per case: the reference's u (`u_<case>`) and the iteration count of its conjugate gradients (`iters_<case>`: the
reference does not report it; it is the oracle's, recorded only after the oracle returned the reference's u bit for bit), and the model's `accuracy_filename` and `name` (`fname_<case>`, `name_<case>`).  n = 600
also: ssl.randomwalk(alpha=a) for a in laplace_order_ref.ALPHAS (`rw_alpha<a>_u`, `_iters`).  `census_<n>_order<o>`: longest row of
L, rows of -L[:, train] with three or more entries, whether L's rows are sorted, max |L - L^T| (combinatorial, tau = 0).

The file holds inputs and recorded results (data only).  Asserted before anything is written: the conditions that make the cases
meaningful (rows of L unsorted for order >= 2; a row longer than 64 at order 2 and longer than 256 at order 3; at least 40 rows of
the right-hand side with three or more entries at n = 600, 10 at n = 2000; every order >= 2 solve longer than 100 iterations), and that the oracle
(oracle/gl_oracle.py with `order`) reproduces every u bit for bit.  A seed that fails a condition is replaced, not waived."""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # the repository: oracle/

import graphlearning as gl                      # the REFERENCE (first on PYTHONPATH)
import laplace_order_ref as ref
from oracle import gl_oracle as orc

assert 'graphlearning_amd' not in gl.__file__ and hasattr(gl.ssl, 'laplace'), gl.__file__
SEEDS = {600: 24, 2000: 25}
LIMIT = 800 * 1024


def blobs(n, seed):
    rng = np.random.default_rng(seed)
    centers = rng.normal(size=(ref.CLASSES, ref.DIM)) * 1.5
    labels = rng.integers(0, ref.CLASSES, size=n)
    X = (centers[labels] + rng.normal(size=(n, ref.DIM))).astype(np.float32)
    train = []
    for _ in range(ref.TRIALS):
        train.append(np.concatenate([rng.choice(np.flatnonzero(labels == c), ref.PER_CLASS, replace=False) for c in range(ref.CLASSES)]))
    tau = rng.uniform(0, 0.02, size=n)
    return X, labels.astype(np.int64), np.stack(train).astype(np.int64), tau


def main():
    out = {}
    graphs = {}
    for n in ref.SIZES:
        X32, labels, train, tau = blobs(n, SEEDS[n])
        X = X32.astype(np.float64)
        J, D = gl.weightmatrix.knnsearch(X, ref.K + 1, method='kdtree')
        assert J.max() < 2 ** 31 and np.array_equal(J[:, 0], np.arange(n))
        W = gl.weightmatrix.knn(X, ref.K, knn_data=(J, D))
        Wo = orc.knn_weights(J, D, ref.K)
        assert np.array_equal(W.indptr, Wo.indptr) and np.array_equal(W.indices, Wo.indices) and np.array_equal(W.data, Wo.data)
        out['X%d' % n], out['labels%d' % n], out['J%d' % n], out['D%d' % n] = X32, labels, J.astype(np.int32), D
        out['train%d' % n], out['tau%d' % n] = train, tau
        graphs[n] = (W, labels, train, tau)
        for order in (2, 3):
            L = orc.laplace_operator(W, 'combinatorial', 0, order)
            census = [ref.longest_row(L), ref.rows_with_three(L, train[0]), int(L.has_sorted_indices), abs(L - L.T).max()]
            print('n %d order %d: longest row %d (mean %.1f), rows of the rhs with >= 3 entries %d, sorted %d, |L - L^T| %.1e'
                  % (n, order, census[0], L.nnz / n, census[1], census[2], census[3]))
            assert not L.has_sorted_indices and census[0] > (64 if order == 2 else 256), (n, order, census)
            assert census[1] >= (40 if n == 600 else 10), (n, order, census)     # (15 labels among 2000 vertices share fewer neighbours)
            out['census_%d_order%d' % (n, order)] = np.array(census, dtype=np.float64)

    for case in ref.CASES:
        n, order, norm, tau_tag, ms = case
        W, labels, train, tau = graphs[n]
        ind = train[0]
        tau_arg = tau if tau_tag == 'vec' else float(tau_tag)
        model = gl.ssl.laplace(W, normalization=norm, tau=tau_arg, order=order, mean_shift=ms, tol=ref.TOL)
        u = np.ascontiguousarray(model.fit(ind, labels[ind]), dtype=np.float64)
        assert u.shape == (n, ref.CLASSES) and np.isfinite(u).all(), case
        uo, it = orc.laplace_fit(W, ind, labels[ind], normalization=norm, tau=tau_arg, mean_shift=ms, tol=ref.TOL, order=order,
                                 return_iters=True)
        assert np.array_equal(u, uo), case
        assert order == 1 or it > 100, (case, it)
        key = ref.case_key(*case)
        print('%-44s iterations %4d accuracy %.2f  %s' % (key, it, gl.ssl.ssl_accuracy(model.predict(), labels, ind), model.accuracy_filename))
        out['u_' + key], out['iters_' + key] = u, np.int64(it)
        out['fname_' + key], out['name_' + key] = np.array(model.accuracy_filename), np.array(model.name)

    W, labels, train, _ = graphs[600]
    ind = train[0]
    for a in ref.ALPHAS:
        u = np.ascontiguousarray(gl.ssl.randomwalk(W, alpha=a).fit(ind, labels[ind]), dtype=np.float64)
        uo, it = orc.randomwalk_fit(W, ind, labels[ind], alpha=a, return_iters=True)
        assert np.array_equal(u, uo), a
        print('randomwalk alpha %.2f iterations %d' % (a, it))
        out['rw_alpha%s_u' % a], out['rw_alpha%s_iters' % a] = u, np.int64(it)

    path = os.path.join(HERE, ref.GOLDEN_FILE)
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < LIMIT, os.path.getsize(path)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
