"""Mirrors the reference's dynamic label propagation learner (Wang, Tu and Tsotsos, ICCV 2013) on two moons, beside Laplace and Poisson
learning.  The reference holds the evolving transition matrix as a dense n x n array and refuses more than 5000 vertices; here it is
applied through its unrolled recursion -- sparse products and k x k Gram matrices, all T steps in one device call, all classes as
columns -- so the 20 000-vertex graph below is solved like the small one.  The result is a pure function of the inputs and equals the
reference's to about 1e-15 of its largest entry.  A step carries a label only a few edges further, so with
five labels per class on a kNN graph the default T = 2 leaves most vertices undecided and more steps help.  With all_labels the accuracy after every step is printed
after the solve."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import sklearn.datasets as datasets
import graphlearning_amd as gl

for n in (2000, 20000):
    X, labels = datasets.make_moons(n_samples=n, noise=0.1, random_state=0)
    W = gl.weightmatrix.knn(X, 10)
    train_ind = gl.trainsets.generate(labels, rate=5, seed=0)
    train_labels = labels[train_ind]
    print('%d vertices' % n)
    for model in [gl.ssl.dynamic_label_propagation(W), gl.ssl.dynamic_label_propagation(W, T=6),
                  gl.ssl.dynamic_label_propagation(W, alpha=0.5, lam=0.01, T=4),
                  gl.ssl.dynamic_label_propagation(W, class_priors=gl.utils.class_priors(labels)), gl.ssl.laplace(W), gl.ssl.poisson(W)]:
        t0 = time.perf_counter()
        pred_labels = model.fit_predict(train_ind, train_labels)
        ms = 1e3 * (time.perf_counter() - t0)
        extra = ''
        if hasattr(model, 'dlp_plan'):
            extra = '   (T = %d: launches / sparse passes / Gram matrices / partial sums %s)' % (model.num_iter, model.dlp_plan)
        print('  %s: %.2f%% in %.1f ms%s' % (model.name, gl.ssl.ssl_accuracy(pred_labels, labels, train_ind), ms, extra))

# the accuracy after each step, as the reference prints it
gl.ssl.dynamic_label_propagation(W, T=4).fit(train_ind, train_labels, all_labels=labels)
