"""Poisson learning with the spectral solver on two moons, beside the default conjugate-gradient solver: the spectral_cutoff + 1 lowest
random-walk eigenpairs of the graph come from graph.eigen_decomp -- thick-restart Lanczos with full reorthogonalisation on the GPU
 -- once per graph; a fit is then V (L^-p (V^T source)) in host numpy, so repeated fits cost nothing.  p != 1
switches to the spectral solver, as in the reference.  The eigenvalues equal scipy's svds to about 1e-15; a disconnected or bipartite
graph ends in a GlxError that says a multiple eigenvalue was missed."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import sklearn.datasets as datasets
import graphlearning_amd as gl

X, labels = datasets.make_moons(n_samples=2000, noise=0.1, random_state=0)
W = gl.weightmatrix.knn(X, 10)
train_ind = gl.trainsets.generate(labels, rate=5, seed=0)
train_labels = labels[train_ind]
for model in [gl.ssl.poisson(W, solver='spectral'), gl.ssl.poisson(W, solver='spectral', spectral_cutoff=30), gl.ssl.poisson(W, p=2),
              gl.ssl.poisson(W)]:
    for attempt in ('first fit', 'second fit'):
        t0 = time.perf_counter()
        pred_labels = model.fit_predict(train_ind, train_labels)
        ms = 1e3 * (time.perf_counter() - t0)
        print('%s (solver %s, p = %g), %s: %.2f%% in %.1f ms' % (model.name, model.solver, model.p, attempt,
                                                                gl.ssl.ssl_accuracy(pred_labels, labels, train_ind), ms))

G = gl.graph(W)
for normalization, k in (('normalized', 50), ('randomwalk', 11), ('combinatorial', 10)):
    t0 = time.perf_counter()
    vals, vecs = G.eigen_decomp(normalization=normalization, k=k)
    print('eigen_decomp(%s, k=%d): %.1f ms, %d Lanczos steps, %d restarts, lowest eigenvalues %s'
          % (normalization, k, 1e3 * (time.perf_counter() - t0), G.eig_steps, G.eig_restarts, np.array2string(vals[:4], precision=6)))
