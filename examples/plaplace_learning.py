"""Mirrors the reference's p-Laplace learner on two moons: semi-supervised learning by the game-theoretic p-Laplace equation, with the
reference's default in-order sweeps (fast=True) and with the Jacobi iteration of upper and lower barriers (fast=False), beside AMLE
(p = infinity), Laplace and Poisson learning.  Both classes are the columns of one device call."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import sklearn.datasets as datasets
import graphlearning_amd as gl

X, labels = datasets.make_moons(n_samples=2000, noise=0.1, random_state=0)
W = gl.weightmatrix.knn(X, 10)
train_ind = gl.trainsets.generate(labels, rate=5, seed=0)
train_labels = labels[train_ind]
for model in [gl.ssl.plaplace(W), gl.ssl.plaplace(W, p=3), gl.ssl.plaplace(W, fast=False),
              gl.ssl.plaplace(W, class_priors=gl.utils.class_priors(labels)), gl.ssl.amle(W), gl.ssl.laplace(W), gl.ssl.poisson(W)]:
    t0 = time.perf_counter()
    pred_labels = model.fit_predict(train_ind, train_labels)
    ms = 1e3 * (time.perf_counter() - t0)
    extra = ''
    if isinstance(model, gl.ssl.plaplace):
        extra = '   (fast=%s, iterations per class %s)' % (model.fast, model.num_iter)
    print('%s: %.2f%% in %.1f ms%s' % (model.name, gl.ssl.ssl_accuracy(pred_labels, labels, train_ind), ms, extra))

# the batched solve itself: three boundary-value columns on the same boundary vertices, each stopping on its own
G = gl.graph(W)
vals = np.array([[0.0, 0.0, 1.0], [1.0, 0.01, 1.0]])
u = G._plaplace_batch([0, 1], vals, 10, tol=1e-2, fast=False)
print('graph._plaplace_batch between vertices 0 and 1: stopping iterations %s, column ranges %s' % (
    G.plaplace_iters.tolist(), [(round(float(u[:, b].min()), 3), round(float(u[:, b].max()), 3)) for b in range(3)]))
