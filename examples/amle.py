"""Mirrors the reference's AMLE learner on two moons: semi-supervised learning by the absolutely minimal Lipschitz extension
(p-Laplace learning with p = infinity), unweighted and weighted, beside Laplace and Poisson learning.  The reference's in-order
Gauss-Seidel sweeps run on the GPU level by level and give its iterates bit for bit; both classes are the
columns of one device call."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import sklearn.datasets as datasets
import graphlearning_amd as gl

X, labels = datasets.make_moons(n_samples=2000, noise=0.1, random_state=0)
W = gl.weightmatrix.knn(X, 10)
train_ind = gl.trainsets.generate(labels, rate=5, seed=0)
train_labels = labels[train_ind]
for model in [gl.ssl.amle(W), gl.ssl.amle(W, weighted=True), gl.ssl.amle(W, class_priors=gl.utils.class_priors(labels)),
              gl.ssl.laplace(W), gl.ssl.poisson(W)]:
    t0 = time.perf_counter()
    pred_labels = model.fit_predict(train_ind, train_labels)
    ms = 1e3 * (time.perf_counter() - t0)
    extra = ''
    if isinstance(model, gl.ssl.amle):
        extra = '   (weighted=%s, %d levels, sweeps per class %s)' % (model.weighted, model.graph.amle_levels, model.num_iter)
    print('%s: %.2f%% in %.1f ms%s' % (model.name, gl.ssl.ssl_accuracy(pred_labels, labels, train_ind), ms, extra))

# the extension itself: boundary values 0 and 1 on two vertices, the progress lines of the reference
G = gl.graph(W)
u = G.amle([0, 1], np.array([0.0, 1.0]), tol=1e-4, max_num_it=25, weighted=False, prog=False)
print('graph.amle between vertices 0 and 1: %d sweeps, values in [%.3f, %.3f]' % (G.amle_iters, u.min(), u.max()))
