#!/usr/bin/env python3
"""Generate the centered-kernel fixture tests/golden/g18_ck.npz from THE REFERENCE.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONPATH=<the reference's checkout> PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg \
        python3 tests/golden/make_golden_ck.py        (from the repository root)

kNN graphs go through the reference's knnsearch(..., method='kdtree') (annoy is not installed there).  Captured with Python 3.10.12,
numpy 2.2.6, scipy 1.15.3, reference graphlearning 1.7.5.

The file holds inputs and recorded results (data only): the graphs as canonical CSR (diagonal included where a case stores one) and,
per case of ck_ref.GOLDEN_CASES, the seed passed to np.random.seed before the fit, the training vertices and labels, the reference's
prob, its predict() with and without class priors, the lines one fit with all_labels prints, l, T and the err history of the
reference-order restatement of tests/ck_ref.py, the largest difference between the reference's prob and either restatement
(`delta_ref`), the relative difference of l between the restatements, and the reference's own time for one fit on the machine that
ran this generator.  `bound` = 16 * max delta_ref and `l_bound` = 16 * max relative difference of l are what the tests allow.

Asserted before anything is written: both restatements stop at the reference-order T; err_{T-1} and err_T are at least 1e-3 * tol
away from tol; the smallest top-two gap of prob over the unlabelled vertices exceeds 1e-9; the bound is at most 1e-12."""
import contextlib
import io
import os
import sys
import time
import numpy as np
from scipy import sparse

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import graphlearning as gl                      # the REFERENCE (first on PYTHONPATH)
import ck_ref as ref                            # the restatements, cross-checked below

assert 'graphlearning_amd' not in gl.__file__ and hasattr(gl.ssl, 'centered_kernel'), gl.__file__
LIMIT = 1000000      # bytes
TOL = 1e-10


def blob_points(rng, n, d, k, spread):
    centres = rng.normal(size=(k, d)) * spread
    lab = np.arange(n) % k
    return centres[lab] + rng.normal(size=(n, d)), lab


def knn_graph(X, k, symmetrize=True):
    knn_data = gl.weightmatrix.knnsearch(X, k, method='kdtree')
    return gl.weightmatrix.knn(X, k, symmetrize=symmetrize, knn_data=knn_data)


def pick(rng, lab, per_class):
    return np.concatenate([rng.choice(np.where(lab == c)[0], size=per_class, replace=False) for c in np.unique(lab)])


def make_graphs():
    rng = np.random.default_rng(18)
    G, truth = {}, {}
    X, lab = blob_points(rng, 600, 5, 3, 1.6)
    G['blobs'], truth['blobs'] = knn_graph(X, 10), lab
    G['directed'], truth['directed'] = knn_graph(X, 10, symmetrize=False), lab
    X, lab = blob_points(rng, 2000, 5, 10, 3.0)
    G['ten'], truth['ten'] = knn_graph(X, 10), lab
    # stored diagonal entries, two vertices without any entry, one hub row of 257 entries
    X, lab = blob_points(rng, 300, 2, 3, 2.0)
    W = sparse.lil_matrix(knn_graph(X, 10))
    hub = rng.choice(np.setdiff1d(np.arange(300), [7, 11, 150]), size=257, replace=False)
    W[150, :] = 0
    W[150, hub] = 0.3
    for lone in (11, 150 + 37):
        W[lone, :] = 0
        W[:, lone] = 0
    W = sparse.csr_matrix(W)
    d = np.zeros(300)
    d[::3] = 0.7
    d[[11, 187]] = 0
    W = W - sparse.diags(W.diagonal()) + sparse.diags(d)
    W.eliminate_zeros()
    G['loops'], truth['loops'] = W, lab
    X, lab = blob_points(rng, 65, 3, 2, 1.5)
    G['tiny'], truth['tiny'] = knn_graph(X, 10), lab
    return {g: ref.canonical(W) for g, W in G.items()}, truth


def main():
    graphs, truth = make_graphs()
    out = {}
    for g, W in graphs.items():
        deg = np.diff(ref.without_diagonal(W).indptr)
        print('%-9s n %4d entries %6d row lengths %d .. %d stored diagonal %d symmetric %s' % (
            g, W.shape[0], W.nnz, deg.min(), deg.max(), int(np.count_nonzero(W.diagonal())), (abs(W - W.T) > 0).nnz == 0))
        out['graph_%s_indptr' % g] = W.indptr.astype(np.int64)
        out['graph_%s_indices' % g] = W.indices.astype(np.int32)
        out['graph_%s_data' % g] = W.data
        out['graph_%s_truth' % g] = truth[g].astype(np.int64)
    deg = np.diff(ref.without_diagonal(graphs['loops']).indptr)
    assert deg.max() == 257 and int((deg == 0).sum()) == 2 and np.count_nonzero(graphs['loops'].diagonal()) > 50
    assert (abs(graphs['directed'] - graphs['directed'].T) > 0).nnz > 0

    rng = np.random.default_rng(181)
    deltas, lrels = [], []
    for number, (name, (g, k)) in enumerate(ref.GOLDEN_CASES.items()):
        W = graphs[g]
        n = W.shape[0]
        lab = truth[g]
        ind = pick(rng, lab, 5)
        labels = lab[ind]
        seed = 1800 + number
        assert len(np.unique(labels)) == k
        priors = np.bincount(lab) / len(lab)

        np.random.seed(seed)
        t0 = time.perf_counter()
        model = gl.ssl.centered_kernel(W)
        prob = np.ascontiguousarray(model.fit(ind, labels), dtype=np.float64)
        sec = time.perf_counter() - t0
        assert prob.shape == (n, k) and np.all(np.isfinite(prob)), name
        pred = model.predict().astype(np.int64)
        np.random.seed(seed)
        model_p = gl.ssl.centered_kernel(W, class_priors=priors)
        pred_p = model_p.fit_predict(ind, labels).astype(np.int64)
        buf = io.StringIO()
        np.random.seed(seed)
        with contextlib.redirect_stdout(buf):
            gl.ssl.centered_kernel(W).fit(ind, labels, all_labels=lab)
        lines = buf.getvalue().splitlines()

        np.random.seed(seed)
        e = np.random.rand(n, 1)
        u_ref, l_ref, T, errs = ref.ck_reference_order(W, ind, labels, k, e)
        u_dev, l_dev, T_dev, errs_dev, capped = ref.device_order_case(W, ind, labels, k, e)
        assert T_dev == T and not capped, (name, T, T_dev)
        assert len(lines) == T and all(s.startswith('Accuracy = ') for s in lines), (name, len(lines), T)
        d_ref = float(np.abs(prob - u_ref).max())
        d_dev = float(np.abs(prob - u_dev).max())
        delta = max(d_ref, d_dev)
        lrel = abs(l_ref - l_dev) / abs(l_ref)
        for q in (T - 1, T):                                   # the stop is not a coin toss
            assert q < 1 or abs(errs[q - 1] - TOL) >= 1e-3 * TOL, (name, q, errs[q - 1])
            assert q < 1 or abs(errs_dev[q - 1] - TOL) >= 1e-3 * TOL, (name, q, errs_dev[q - 1])
        gap = min(ref.top_two_gap(prob, ind), ref.top_two_gap(u_dev, ind))
        assert gap > 1e-9, (name, gap)
        assert np.array_equal(ref.predict(prob), pred) and np.array_equal(ref.predict(u_dev), pred), name
        print('%-9s k %2d T %3d l %.15g reference %.2f s |prob - reference order| %.2e |prob - device order| %.2e l rel %.1e gap %.1e '
              'err_T-1, err_T %.4e %.4e' % (name, k, T, l_ref, sec, d_ref, d_dev, lrel, gap, errs[T - 2], errs[T - 1]))
        deltas.append(delta)
        lrels.append(lrel)
        out['case_%s_seed' % name] = np.int64(seed)
        out['case_%s_ind' % name] = ind.astype(np.int64)
        out['case_%s_labels' % name] = labels.astype(np.int64)
        out['case_%s_priors' % name] = priors
        out['case_%s_prob' % name] = prob
        out['case_%s_pred' % name] = pred
        out['case_%s_pred_priors' % name] = pred_p
        out['case_%s_lines' % name] = np.array(lines)
        out['case_%s_l' % name] = np.float64(l_ref)
        out['case_%s_T' % name] = np.int64(T)
        out['case_%s_errs' % name] = errs
        out['case_%s_delta_ref' % name] = np.float64(delta)
        out['case_%s_delta_reference_order' % name] = np.float64(d_ref)
        out['case_%s_l_rel' % name] = np.float64(lrel)
        out['case_%s_reference_seconds' % name] = np.float64(sec)
    bound = 16 * max(deltas)
    l_bound = 16 * max(max(lrels), np.finfo(np.float64).eps)
    print('delta_ref %.3e bound %.3e l_bound %.3e' % (max(deltas), bound, l_bound))
    assert 0 < bound <= 1e-12, bound
    out['delta_ref'] = np.float64(max(deltas))
    out['bound'] = np.float64(bound)
    out['l_bound'] = np.float64(l_bound)
    path = os.path.join(HERE, ref.GOLDEN_FILE)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(ref.GOLDEN_FILE, size, 'bytes')
    assert size <= LIMIT, size


if __name__ == '__main__':
    main()
