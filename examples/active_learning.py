"""Mirrors the reference's active-learning examples (graphlearning/active_learning.py) on two moons, without the plots: a Laplace
learner, one labelled vertex per class, ten rounds of select_queries / update under each acquisition function.  The four covariance
criteria work in the basis of the 50 lowest eigenvectors of the normalised Laplacian; V and the 50 x 50 covariance C stay on the
device, a round is one pass over V and one rank-one launch.  var_opt and sigma_opt do not look at labels, so
select_greedy plans all ten queries in one device call -- the same vertices, before a single label is asked for."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import sklearn.datasets as datasets
import graphlearning_amd as gl

al = gl.active_learning
X, labels = datasets.make_moons(n_samples=500, noise=0.1, random_state=0)
G = gl.graph(gl.weightmatrix.knn(X, 10))
train_ind = np.array([np.where(labels == c)[0][0] for c in np.unique(labels)])
evals, evecs = G.eigen_decomp(normalization='normalized', k=50)
C = np.diag(1. / (evals + 1e-11))

for acq, kwargs in [(al.unc_sampling, {}), (al.unc_sampling, dict(unc_method='entropy')), (al.var_opt, dict(C=C.copy(), V=evecs.copy())),
                    (al.sigma_opt, dict(C=C.copy(), V=evecs.copy())), (al.model_change, dict(C=C.copy(), V=evecs.copy())),
                    (al.model_change_var_opt, dict(C=C.copy(), V=evecs.copy()))]:
    model = gl.ssl.laplace(G)
    AL = al.active_learner(model, acq, train_ind, labels[train_ind], **kwargs)
    planned = AL.select_greedy(10) if acq in (al.var_opt, al.sigma_opt) else None
    t0 = time.perf_counter()
    for it in range(10):
        query_points = AL.select_queries()          # this round's newly chosen points
        query_labels = labels[query_points]         # the human in the loop
        AL.update(query_points, query_labels)
    ms = 1e3 * (time.perf_counter() - t0)
    acc = gl.ssl.ssl_accuracy(model.predict(), labels, AL.labeled_ind)
    extra = '' if planned is None else '   (select_greedy planned the same ten: %s)' % np.array_equal(planned, AL.labeled_ind[len(train_ind):])
    print('%s%s: queries %s, accuracy %.2f%% with %d labels, ten rounds in %.1f ms%s'
          % (acq.__name__, ' (%s)' % kwargs['unc_method'] if 'unc_method' in kwargs else '', AL.labeled_ind[len(train_ind):].tolist(), acc,
             len(AL.labeled_ind), ms, extra))
