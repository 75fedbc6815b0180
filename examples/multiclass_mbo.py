"""Mirrors the reference's multiclass MBO learner (Garcia-Cardona et al., IEEE PAMI 2014) on two moons, beside Laplace and Poisson
learning: T outer iterations of Ns diffusion steps in the basis of the num_eig lowest eigenvectors of the normalised Laplacian, each
followed by a projection of every vertex onto its largest class.  The decomposition is graph.eigen_decomp('normalized', k=num_eig),
cached in the graph (pass a gl.graph to share it between models); all steps and projections run in one device call (DESIGN.md
section 4.13).  The random start is one np.random.rand(k, n) from numpy's global stream.  The reference draws it after an eigen_decomp
that takes its ARPACK start vector from the same stream, and this package's eigen_decomp does not touch the stream: the same seed
gives another start here than in the reference.  With all_labels the accuracy after every outer iteration is printed after the solve."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import sklearn.datasets as datasets
import graphlearning_amd as gl

X, labels = datasets.make_moons(n_samples=2000, noise=0.1, random_state=0)
G = gl.graph(gl.weightmatrix.knn(X, 10))
train_ind = gl.trainsets.generate(labels, rate=5, seed=0)
train_labels = labels[train_ind]
for model in [gl.ssl.multiclass_mbo(G), gl.ssl.multiclass_mbo(G, Ns=3, T=4, dt=0.3, mu=10), gl.ssl.multiclass_mbo(G, num_eig=20),
              gl.ssl.multiclass_mbo(G, class_priors=gl.utils.class_priors(labels)), gl.ssl.laplace(G), gl.ssl.poisson(G)]:
    np.random.seed(0)
    t0 = time.perf_counter()
    pred_labels = model.fit_predict(train_ind, train_labels)
    ms = 1e3 * (time.perf_counter() - t0)
    extra = ''
    if hasattr(model, 'mmbo_plan'):
        extra = '   (%d steps; launches per step / rows per partial / partials / caps on k*m, k, m / launches %s)' % (model.num_iter, model.mmbo_plan)
    print('%s: %.2f%% in %.1f ms%s' % (model.name, gl.ssl.ssl_accuracy(pred_labels, labels, train_ind), ms, extra))

# the accuracy after each outer iteration, as the reference prints it
np.random.seed(0)
gl.ssl.multiclass_mbo(G).fit(train_ind, train_labels, all_labels=labels)
