"""Mirrors reference examples/dijkstra.py: the graph distance to one point on kNN `distance` graphs (k = 50) of growing size, compared
with the Euclidean cone it approximates.  Graph and distances are built on the GPU (weightmatrix.knn, graph.dijkstra); the second
part shows the closest-point output, the Hopf-Lax form and a geodesic nearest-neighbour classifier on the same graph."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import graphlearning_amd as gl

rng = np.random.default_rng(0)
centre = np.array([0.5, 0.5])
for n in (10 ** 3, 10 ** 4, 10 ** 5):
    X = rng.random((n, 2))
    X[0] = centre
    G = gl.graph(gl.weightmatrix.knn(X, 50, kernel='distance'))
    t0 = time.perf_counter()
    u = G.dijkstra([0])
    ms = 1e3 * (time.perf_counter() - t0)
    cone = np.linalg.norm(X - centre, axis=1)
    print('n = %d, Error = %f   (%d rounds, %.1f ms)' % (n, np.linalg.norm(u - cone, ord=np.inf), G.dijkstra_rounds[0], ms))

# distance to a set with boundary values, closest points, a radius
seeds = rng.choice(n, size=5, replace=False)
u, cp = G.dijkstra(seeds, bdy_val=np.linspace(0, 0.1, 5), max_dist=0.4, return_cp=True)
print('5 seeds, max_dist 0.4: %d vertices reached, cell sizes %s' % (np.isfinite(u).sum(), [int((cp == s).sum()) for s in seeds]))
print('Hopf-Lax distance to the centre: max %.4f' % G.dijkstra_hl([0]).max())
d, path = G.distance(0, int(np.argmax(np.linalg.norm(X - centre, axis=1))), return_path=True)
print('reciprocal-weight distance to the farthest point: %.1f over %d hops' % (d, len(path) - 1))
labels = (X[:, 0] > X[:, 1]).astype(int)
train = rng.choice(n, size=20, replace=False)
model = gl.ssl.graph_nearest_neighbor(G)
print('%s: accuracy %.2f%%' % (model.name, gl.ssl.ssl_accuracy(model.fit_predict(train, labels[train]), labels, train)))
