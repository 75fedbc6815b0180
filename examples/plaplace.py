"""Mirrors reference examples/plaplace.py: p-Laplace interpolation of boundary values on a random
geometric graph, the epsilon-ball graph of the reference example (weightmatrix.epsilon_ball, built on
the GPU).  fast=False selects the Jacobi iteration of the reference's C extension, which runs on the
GPU.  The reference's default fast=True is an in-order Gauss-Seidel sweep; its exact parallel form (levels, as for graph.amle:
examples/amle.py) exists in the library but plaplace(fast=True) is not switched on yet."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import graphlearning_amd as gl

X = np.random.default_rng(2).random((int(1e4), 2))      # (a seed whose graph has no isolated vertex: minimum degree 2)
x, y = X[:, 0], X[:, 1]
eps = 0.02
t0 = time.perf_counter()
W = gl.weightmatrix.epsilon_ball(X, eps)
print('epsilon-ball graph (eps=%g) of %d points: %d entries, degrees %d..%d, in %.1f ms'
      % (eps, len(x), W.nnz, np.diff(W.indptr).min(), np.diff(W.indptr).max(), 1e3 * (time.perf_counter() - t0)))
G = gl.graph(W)
bdy_set = (x < eps) | (x > 1 - eps) | (y < eps) | (y > 1 - eps)
bdy_val = (x - 0.5) ** 2 + (y - 0.5) ** 2
t0 = time.perf_counter()
u = G.plaplace(bdy_set, bdy_val[bdy_set], p=10, fast=False)
print('p-Laplace (p=10) on %d vertices: %d Jacobi iterations in %.2f s; interior mean %.4f, range [%.4f, %.4f]'
      % (len(x), G.plaplace_iters, time.perf_counter() - t0, u[~bdy_set].mean(), u.min(), u.max()))
print('PageRank: largest entries at', np.argsort(-G.page_rank())[:5], 'after', G.page_rank_iters, 'sweeps')
