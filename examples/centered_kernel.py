"""Mirrors the reference's centered kernel learner (Mai and Couillet, ICML 2018) on two moons, beside Laplace and Poisson learning: a
power iteration for the largest eigenvalue of the centred weight matrix, then a fixed-point loop until the update falls below tol.  Both
loops run in one device call, all classes as columns; the result is a pure function of the inputs and equals the reference's to about
1e-15 with the same iteration count.  The start vector comes from numpy's global stream, so seed it as you
would for the reference.  With all_labels the accuracy after every iteration is printed while the solve runs (slow: one download each)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import sklearn.datasets as datasets
import graphlearning_amd as gl

X, labels = datasets.make_moons(n_samples=2000, noise=0.1, random_state=0)
W = gl.weightmatrix.knn(X, 10)
train_ind = gl.trainsets.generate(labels, rate=5, seed=0)
train_labels = labels[train_ind]
for model in [gl.ssl.centered_kernel(W), gl.ssl.centered_kernel(W, tol=1e-6), gl.ssl.centered_kernel(W, alpha=1.5),
              gl.ssl.centered_kernel(W, class_priors=gl.utils.class_priors(labels)), gl.ssl.laplace(W), gl.ssl.poisson(W)]:
    np.random.seed(0)
    t0 = time.perf_counter()
    pred_labels = model.fit_predict(train_ind, train_labels)
    ms = 1e3 * (time.perf_counter() - t0)
    extra = ''
    if hasattr(model, 'ck_plan'):
        extra = '   (%d iterations, eigenvalue %.6f, kernels per iteration / launches / chunk / partial sums %s)' % (
            model.num_iter, model.eigenvalue, model.ck_plan)
    print('%s: %.2f%% in %.1f ms%s' % (model.name, gl.ssl.ssl_accuracy(pred_labels, labels, train_ind), ms, extra))

# the accuracy after each iteration, as the reference prints it (a loose tol keeps the list short)
np.random.seed(0)
gl.ssl.centered_kernel(W, tol=1e-2).fit(train_ind, train_labels, all_labels=labels)
