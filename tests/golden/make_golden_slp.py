#!/usr/bin/env python3
"""Generate the sparse-label-propagation fixtures tests/golden/g16_slp*.npz from THE REFERENCE.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONPATH=<the reference's checkout> PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg \
        python3 tests/golden/make_golden_slp.py        (from the repository root)

kNN graphs go through the reference's knnsearch(..., method='kdtree') (annoy is not installed there).  Captured with Python 3.10.12,
numpy 2.2.6, scipy 1.15.3, reference graphlearning 1.7.5.

The files hold inputs and the reference's outputs (data only).  g16_slp.npz: the graphs as canonical CSR and, per case of
slp_ref.GOLDEN_CASES, the training vertices, their labels and the reference's prob (n, k).  g16_slp_2.npz: the learner's fit_predict on
`blobs` with and without class priors, the accuracy lines one fit with all_labels prints, gradient / divergence of a seeded random
field on `blobs_dir`, and the reference's own time for 3 000 vertices and 3 classes on the machine that ran this generator.

Before anything is written: both restatement forms of tests/slp_ref.py equal the reference bit for bit on every case (the
interpreted form on at most three class columns of a case); in every case with T >= 10 the share of entries clamped in the last
iteration is above 0 and below 1; no graph has an empty row."""
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
import slp_ref as ref                           # the restatement, cross-checked below

assert 'graphlearning_amd' not in gl.__file__ and hasattr(gl.ssl, 'sparse_label_propagation'), gl.__file__
LIMIT = 1000000      # bytes per file


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


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
    rng = np.random.default_rng(16)
    G, truth = {}, {}
    X, lab = blob_points(rng, 600, 5, 3, 1.6)
    G['blobs'], truth['blobs'] = knn_graph(X, 7), lab
    G['blobs_dir'], truth['blobs_dir'] = knn_graph(X, 7, symmetrize=False), lab
    X, lab = blob_points(rng, 900, 5, 17, 3.0)
    G['wide17'], truth['wide17'] = knn_graph(X, 6), lab
    X, lab = blob_points(rng, 300, 2, 3, 2.0)
    W = knn_graph(X, 5).tolil()
    W[0, :] = 0.3
    W[:, 0] = 0.3
    W = W.tocsr()
    d = np.zeros(300)
    d[::3] = 0.7
    W = W - sparse.diags(W.diagonal()) + sparse.diags(d)
    G['hub_diag'], truth['hub_diag'] = W, lab
    for seed in range(100):                      # the first seed whose radius graph has no isolated point
        X = np.random.default_rng(500 + seed).random((500, 2))
        W = gl.weightmatrix.epsilon_ball(X, 0.09)
        if np.diff(ref.canonical(W).indptr).min() >= 1:
            break
    G['ball'], truth['ball'] = W, (X[:, 0] > 0.5).astype(np.int64)
    return {g: ref.canonical(W) for g, W in G.items()}, truth


def main():
    graphs, truth = make_graphs()
    out, out2 = {}, {}
    for g in ref.GOLDEN_GRAPHS:
        W = graphs[g]
        deg = np.diff(W.indptr)
        assert deg.min() >= 1, g
        assert np.all(np.isfinite(W.data)) and W.data.min() > 0, g
        print('%-10s n %4d entries %6d row lengths %d .. %d symmetric %s' % (g, W.shape[0], W.nnz, deg.min(), deg.max(), (abs(W - W.T) > 0).nnz == 0))
        out['graph_%s_indptr' % g] = W.indptr.astype(np.int64)
        out['graph_%s_indices' % g] = W.indices.astype(np.int32)
        out['graph_%s_data' % g] = W.data
        out['graph_%s_truth' % g] = truth[g].astype(np.int64)
    rng = np.random.default_rng(161)
    for name, (g, k, T) in ref.GOLDEN_CASES.items():
        W = graphs[g]
        if name == 'oneclass':
            ind = rng.choice(W.shape[0], size=6, replace=False)
            labels = np.zeros(6, dtype=np.int64)
        else:
            ind = pick(rng, truth[g], 2 if name == 'wide17' else 5)
            labels = truth[g][ind]
        assert len(np.unique(labels)) == k
        t0 = time.perf_counter()
        model = gl.ssl.sparse_label_propagation(W, T=T)
        prob = np.ascontiguousarray(model.fit(ind, labels), dtype=np.float64)
        sec = time.perf_counter() - t0
        assert prob.shape == (W.shape[0], k) and np.all(np.isfinite(prob)), name
        u, share = ref.slp_numpy(W, ind, labels, T, clamped=True)
        assert same_bits(u, prob), (name, 'numpy form', int((u != prob).sum()))
        cols = sorted(set([0, k - 2, k - 1]) & set(range(k)))
        up = ref.slp_python(W, ind, labels, T, cols=cols)
        assert same_bits(up, np.ascontiguousarray(prob[:, cols])), (name, 'interpreted form')
        if T >= 10:
            assert 0 < share < 1, (name, share)
        print('%-10s k %2d T %3d reference %.2f s clamped share %.2f' % (name, k, T, sec, share))
        out['case_%s_ind' % name] = ind.astype(np.int64)
        out['case_%s_labels' % name] = labels.astype(np.int64)
        out['case_%s_prob' % name] = prob
        out['case_%s_clamped' % name] = np.float64(share)

    # the learner: predictions with and without priors, the lines of an all_labels fit
    W, lab = graphs['blobs'], truth['blobs']
    ind, labels = out['case_blobs_ind'], out['case_blobs_labels']
    out2['learner_pred'] = gl.ssl.sparse_label_propagation(W, T=100).fit_predict(ind, labels).astype(np.int64)
    priors = np.bincount(lab) / len(lab)
    out2['learner_priors'] = priors
    out2['learner_pred_priors'] = gl.ssl.sparse_label_propagation(W, class_priors=priors, T=100).fit_predict(ind, labels).astype(np.int64)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        gl.ssl.sparse_label_propagation(W, T=12).fit(ind, labels, all_labels=lab)
    lines = buf.getvalue().splitlines()
    assert len(lines) == 12 and lines[0].startswith('0,Accuracy = '), lines[:2]
    out2['learner_lines'] = np.array(lines)

    # the calculus on the directed graph
    Gd = gl.graph(graphs['blobs_dir'])
    field = np.random.default_rng(162).normal(size=Gd.num_nodes)
    out2['calc_field'] = field
    for key, M in (('adjacency', Gd.adjacency()), ('grad', Gd.gradient(field)), ('grad_w', Gd.gradient(field, weighted=True)),
                   ('grad_p', Gd.gradient(field, p=0.5))):
        M = sparse.csr_matrix(M)
        out2['calc_%s_indptr' % key], out2['calc_%s_indices' % key], out2['calc_%s_data' % key] = M.indptr, M.indices, M.data
    V = Gd.gradient(field, weighted=True)
    out2['calc_div_w'] = np.asarray(Gd.divergence(V), dtype=np.float64)
    out2['calc_div'] = np.asarray(Gd.divergence(V, weighted=False), dtype=np.float64)

    # the reference's own time (3 000 vertices, 3 classes, T = 100), on the machine that runs this generator
    X, lab = blob_points(np.random.default_rng(163), 3000, 5, 3, 1.6)
    W = knn_graph(X, 7)
    ind = pick(np.random.default_rng(164), lab, 5)
    t0 = time.perf_counter()
    gl.ssl.sparse_label_propagation(W, T=100).fit(ind, lab[ind])
    out2['reference_seconds_n3000_k3_T100'] = np.float64(time.perf_counter() - t0)
    out2['reference_entries_n3000'] = np.int64(ref.canonical(W).nnz)
    print('reference, 3000 vertices, 3 classes, T = 100: %.2f s (%d entries)' % (out2['reference_seconds_n3000_k3_T100'], out2['reference_entries_n3000']))

    for fname, data in (('g16_slp.npz', out), ('g16_slp_2.npz', out2)):
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **data)
        size = os.path.getsize(path)
        print(fname, size, 'bytes')
        assert size <= LIMIT, (fname, size)


if __name__ == '__main__':
    main()
