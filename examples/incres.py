"""Mirrors the reference's INCRES clustering (Bresson et al., 2016: incremental reseeding) on three Gaussian blobs and on two moons,
without any label: T outer iterations, each planting m random seeds per cluster, growing them with the random walk F <- P F until no
entry of F is zero, and harvesting the row-wise argmax; m grows from iteration to iteration.  The grow loop runs on the device, one
call per outer iteration; every random number comes from numpy's global stream in the reference's order, so
the same np.random.seed gives the reference's labels.  A graph on which the reference's loop would never end -- disconnected,
bipartite, or so long that values underflow -- raises GlxError after max_grow sweeps instead."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import sklearn.datasets as datasets
import graphlearning_amd as gl

for name, (X, labels), k in [('blobs', datasets.make_blobs(n_samples=3000, centers=[[0, 0], [6, 0], [3, 5]], cluster_std=1.5, random_state=0), 3),
                             ('moons', datasets.make_moons(n_samples=2000, noise=0.1, random_state=0), 2)]:
    W = gl.weightmatrix.knn(X, 10)
    np.random.seed(0)
    model = gl.clustering.incres(W, num_clusters=k)
    t0 = time.perf_counter()
    pred = model.fit_predict()
    ms = 1e3 * (time.perf_counter() - t0)
    plan = model.incres_plan
    print('%s: accuracy %.2f%%, purity %.2f%% in %.1f ms (%d .. %d sweeps per outer iteration, %d enqueued for %d counted, %d chunks read)'
          % (name, gl.clustering.clustering_accuracy(pred, labels), gl.clustering.purity(pred, labels)[0], ms, min(model.grow_sweeps),
             max(model.grow_sweeps), plan['enqueued'], plan['counted'], plan['chunks']))

# the accuracy after the first outer iterations, as the reference prints it
np.random.seed(0)
gl.clustering.incres(W, num_clusters=2, T=5).fit(all_labels=labels)

# a graph with two components: the reference would loop for ever
X, _ = datasets.make_blobs(n_samples=400, centers=[[0, 0], [50, 50]], random_state=0)
try:
    gl.clustering.incres(gl.weightmatrix.knn(X, 5), num_clusters=2, max_grow=100).fit()
except gl.GlxError as e:
    print('refused:', e)
