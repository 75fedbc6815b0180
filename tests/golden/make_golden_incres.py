#!/usr/bin/env python3
"""Generate the INCRES fixture tests/golden/g21_incres.npz from THE REFERENCE.

Run where the reference is importable (it never travels to the GPU box):

    PYTHONPATH=<the reference's checkout> PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg \
        python3 tests/golden/make_golden_incres.py        (from the repository root)

Graphs are read from the fixtures that hold them and not stored again: `blobs` from g18_ck.npz, `moons` from g19_eig.npz.  The cases
are incres_ref.GOLDEN_CASES: the blobs graph with 3 clusters at the defaults, with speed=50, T=20, and with 5 clusters; the moons graph
with 2 clusters.

The file holds recorded results (data only).  Per case c: the seed (`case_<c>_seed`); the reference's labels after every outer
iteration (`_labels`, (T, n) uint8), recorded by wrapping np.argmax during the fit; the sweeps of every grow loop (`_sweeps`), recorded
by counting the np.min calls (one more than the sweeps of a loop); fit_predict()'s result is the last row (asserted).  For
incres_ref.LINES_CASE: the printed lines of an all_labels fit (`_lines`).  Metrics on recorded inputs: `metric_pred`, `metric_true`
-> `metric_accuracy`, `metric_purity`, `metric_purity_each`; `metric_x` -> `metric_withinss` (w, m); `metric_X`, `metric_rp1d_seed`,
`metric_rp1d_T` -> `metric_rp1d`.

Asserted before anything is written: every graph is connected and not bipartite (scipy.sparse.csgraph; the reference's loop would not
end otherwise); incres_ref.fit (the numpy restatement) reproduces every recorded label and count from the same seed; the all_labels fit
gives the labels of the plain fit; the file stays below the size of g3_blobs5000.npz.  A case that fails is replaced by another seed in
incres_ref.GOLDEN_CASES, not waived."""
import contextlib
import io
import os
import sys
import numpy as np
from scipy.sparse import csgraph

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.append(os.path.dirname(os.path.dirname(HERE)))      # graphlearning_amd, behind the reference

import graphlearning as gl                      # the REFERENCE (first on PYTHONPATH)
import incres_ref as ref

assert 'graphlearning_amd' not in gl.__file__ and hasattr(gl.clustering, 'incres'), gl.__file__
LIMIT = os.path.getsize(os.path.join(HERE, 'g3_blobs5000.npz'))


def connected_and_not_bipartite(W):
    count, _ = csgraph.connected_components(W, directed=False)
    if count != 1:
        return False
    if W.diagonal().any():
        return True
    # two-colour by breadth-first depth: an edge inside a colour class is an odd cycle
    order, pred = csgraph.breadth_first_order(W, 0, directed=False)
    depth = np.zeros(W.shape[0], dtype=np.int64)
    for v in order[1:]:
        depth[v] = depth[pred[v]] + 1
    coo = W.tocoo()
    return bool(np.any((depth[coo.row] & 1) == (depth[coo.col] & 1)))


def reference_fit(W, k, seed, params, all_labels=None):
    """(fit_predict's result, labels after every outer iteration, sweeps of every grow loop, what the fit printed)"""
    hist, mins = [], [0]
    orig_argmax, orig_min = np.argmax, np.min

    def argmax(*a, **kw):
        out = orig_argmax(*a, **kw)
        if kw.get('axis') == 1 and getattr(a[0], 'shape', None) == (W.shape[0], k):
            hist.append(np.array(out))
            mins.append(0)
        return out

    def amin(*a, **kw):
        if getattr(a[0], 'shape', None) == (W.shape[0], k):
            mins[-1] += 1
        return orig_min(*a, **kw)
    model = gl.clustering.incres(W, k, **params)
    np.random.seed(seed)
    np.argmax, np.min = argmax, amin
    out = io.StringIO()
    try:
        with contextlib.redirect_stdout(out):
            pred = model.fit_predict(all_labels=all_labels)
    finally:
        np.argmax, np.min = orig_argmax, orig_min
    return pred, np.array(hist), np.array(mins[:len(hist)], dtype=np.int64) - 1, out.getvalue().splitlines()


def main():
    import eig_ref
    gold = eig_ref.load_golden()
    out = {}
    for name, (g, k, seed, params) in ref.GOLDEN_CASES.items():
        W, truth = eig_ref.golden_graph(gold, g), gold['graph_%s_truth' % g]
        assert connected_and_not_bipartite(W), (name, 'the reference would not end')
        T = params.get('T', 200)
        pred, hist, sweeps, _ = reference_fit(W, k, seed, params)
        assert hist.shape == (T, W.shape[0]) and sweeps.shape == (T,) and np.array_equal(pred, hist[-1]) and hist.max() < 256
        np.random.seed(seed)
        mine, counts, _ = ref.fit(W, k, **params)
        assert np.array_equal(mine, hist) and np.array_equal(counts, sweeps), name
        key = 'case_%s_' % name
        out[key + 'seed'], out[key + 'labels'], out[key + 'sweeps'] = np.int64(seed), hist.astype(np.uint8), sweeps
        if name == ref.LINES_CASE:
            pred_l, hist_l, _, lines = reference_fit(W, k, seed, params, all_labels=truth)
            assert np.array_equal(hist_l, hist) and len(lines) == T and all(s.startswith('Iteration ') for s in lines)
            out[key + 'lines'] = np.array(lines)
        print(name, 'accuracy %.2f' % gl.clustering.clustering_accuracy(pred, truth), 'sweeps', sweeps.min(), '..', sweeps.max())
    # metrics on recorded inputs
    rng = np.random.default_rng(21)
    true = rng.integers(0, 4, 300) * 3 + 1                       # classes 1, 4, 7, 10
    pred = np.where(rng.random(300) < 0.7, (true - 1) // 3, rng.integers(0, 4, 300))[rng.permutation(300)]
    x = np.concatenate([rng.normal(0, 1, 40), rng.normal(5, 1, 37)])
    X = np.concatenate([rng.normal(0, 1, (30, 3)), rng.normal(4, 1, (25, 3))])
    out['metric_pred'], out['metric_true'], out['metric_x'], out['metric_X'] = pred, true, x, X
    out['metric_accuracy'] = np.float64(gl.clustering.clustering_accuracy(pred, true))
    p, each = gl.clustering.purity(pred, true)
    out['metric_purity'], out['metric_purity_each'] = np.float64(p), each
    out['metric_withinss'] = np.array(gl.clustering.withinss(x), dtype=np.float64)
    out['metric_rp1d_seed'], out['metric_rp1d_T'] = np.int64(5), np.int64(12)
    np.random.seed(5)
    out['metric_rp1d'] = gl.clustering.RP1D(X, 12)
    path = os.path.join(HERE, ref.GOLDEN_FILE)
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < LIMIT, os.path.getsize(path)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
