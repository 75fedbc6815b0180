"""Mirrors reference examples/peikonal.py: a data depth from the p-eikonal equation.  10 000 uniform points of the unit square, an
epsilon-ball graph, the points within epsilon of the square's edge as the boundary at 0: u grows towards the middle of the cloud.
Graph and solve run on the GPU (weightmatrix.epsilon_ball, graph.peikonal); the second part solves the same boundary for p = 2 and
classifies two halves of the square with ssl.peikonal.  The figure is drawn only where matplotlib is installed."""
import os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import graphlearning_amd as gl

rng = np.random.default_rng(0)
X = rng.random((int(1e4), 2))
x, y = X[:, 0], X[:, 1]

eps = 0.02
W = gl.weightmatrix.epsilon_ball(X, eps)
G = gl.graph(W)

bdy_set = (x < eps) | (x > 1 - eps) | (y < eps) | (y > 1 - eps)
t0 = time.perf_counter()
u = G.peikonal(bdy_set)
ms = 1e3 * (time.perf_counter() - t0)
deepest = int(np.argmax(u))
print('p = 1: %d boundary points, %d rounds, %.1f ms; the deepest point is (%.3f, %.3f) with u = %.4g'
      % (bdy_set.sum(), G.peikonal_rounds, ms, x[deepest], y[deepest], u[deepest]))
centre_dist = np.max(np.abs(X - 0.5), axis=1)
print('rank correlation of the depth with the distance to the edge: %.3f'
      % np.corrcoef(np.argsort(np.argsort(u)), np.argsort(np.argsort(-centre_dist)))[0, 1])

u2 = G.peikonal(bdy_set, p=2)
print('p = 2: %d rounds, max u = %.4g' % (G.peikonal_rounds, u2.max()))

labels = (x > y).astype(int)
train = rng.choice(len(X), size=20, replace=False)
model = gl.ssl.peikonal(G)          # (eps_ball_graph=True would weigh by the degree, which an isolated point of the cloud makes 0)
print('%s: accuracy %.2f%%' % (model.name, gl.ssl.ssl_accuracy(model.fit_predict(train, labels[train]), labels, train)))

try:
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
except ImportError:
    plt = None
if plt is not None:
    plt.scatter(x, y, c=u, s=0.25)
    plt.scatter(x[bdy_set], y[bdy_set], c='r', s=0.5)
    out = os.path.join(tempfile.gettempdir(), 'peikonal.png')
    plt.savefig(out, dpi=150)
    print('figure written to', out)
