"""Mirrors the reference's sparse label propagation learner on two moons: T primal-dual sweeps for the total-variation problem, a field
on the edges beside the labels on the vertices, beside Laplace and Poisson learning.  All classes are the columns of one device call and
the result is the reference's bit for bit.  With all_labels the accuracy after every iteration is printed."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import sklearn.datasets as datasets
import graphlearning_amd as gl

X, labels = datasets.make_moons(n_samples=2000, noise=0.1, random_state=0)
W = gl.weightmatrix.knn(X, 10)
train_ind = gl.trainsets.generate(labels, rate=5, seed=0)
train_labels = labels[train_ind]
for model in [gl.ssl.sparse_label_propagation(W), gl.ssl.sparse_label_propagation(W, T=400),
              gl.ssl.sparse_label_propagation(W, class_priors=gl.utils.class_priors(labels)), gl.ssl.laplace(W), gl.ssl.poisson(W)]:
    t0 = time.perf_counter()
    pred_labels = model.fit_predict(train_ind, train_labels)
    ms = 1e3 * (time.perf_counter() - t0)
    extra = '   (T=%d, launches per iteration / in all / column tile %s)' % (model.T, model.slp_plan,) if hasattr(model, 'slp_plan') else ''
    print('%s: %.2f%% in %.1f ms%s' % (model.name, gl.ssl.ssl_accuracy(pred_labels, labels, train_ind), ms, extra))

# the accuracy after each of the first iterations, as the reference prints it
gl.ssl.sparse_label_propagation(W, T=5).fit(train_ind, train_labels, all_labels=labels)

# the graph calculus the method is written in (host scipy)
G = gl.graph(W)
u = np.random.default_rng(0).normal(size=G.num_nodes)
print('div grad u == -L u:', np.allclose(G.divergence(G.gradient(u, weighted=True), weighted=False), -G.laplacian() @ u))
