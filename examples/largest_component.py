"""A disconnected graph and what to do about it: the kNN graph of three well-separated blobs has three components, on which
eigen_decomp finds a multiple eigenvalue 0 (and may refuse), INCRES never ends and the Poisson system is inconsistent.
graph.connected_components counts and labels the components on the device (scipy's labels on every vertex),
graph.largest_connected_component hands back the largest one as a graph of its own and the mask of its vertices; the spectral
decomposition and a Poisson fit then run on that component."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import graphlearning_amd as gl

rng = np.random.default_rng(0)
sizes = (3000, 2000, 1000)
X = np.concatenate([rng.normal(size=(m, 2)) + [50.0 * c, 0.0] for c, m in enumerate(sizes)])
W = gl.weightmatrix.knn(X, 10)
G = gl.graph(W)

t0 = time.perf_counter()
ncomp, labels = G.connected_components()
ms = 1e3 * (time.perf_counter() - t0)
print('%d vertices, %d entries: %d components of %s vertices in %.2f ms; isconnected() says %s'
      % (G.num_nodes, W.nnz, ncomp, np.bincount(labels).tolist(), ms, G.isconnected()))

try:
    vals, _ = G.eigen_decomp('normalized', k=5)
    print('whole graph: eigenvalues', np.round(vals, 6), '-- one zero per component')
except gl.GlxError as e:
    print('whole graph, eigen_decomp refused:', e)

H, ind = G.largest_connected_component()
print('largest component: %d vertices, %d entries, connected: %s' % (H.num_nodes, H.weight_matrix.nnz, H.connected_components()[0] == 1))
vals, vecs = H.eigen_decomp('normalized', k=5)
print('its eigenvalues:', np.round(vals, 6), '-- a single zero')

# two classes inside the component (left and right of its centre), five labels each
y = (X[ind, 0] > np.median(X[ind, 0])).astype(np.int64)
train_ind = np.concatenate([rng.choice(np.flatnonzero(y == c), 5, replace=False) for c in (0, 1)])
pred = gl.ssl.poisson(H.weight_matrix).fit_predict(train_ind, y[train_ind])
print('Poisson learning on the component: accuracy %.2f%% from %d labels' % (gl.ssl.ssl_accuracy(pred, y, train_ind), len(train_ind)))
