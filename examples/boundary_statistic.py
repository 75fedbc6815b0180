"""The boundary of a point cloud, found from the points alone: 20 000 points uniform in the unit disc, the boundary test of Calder,
Park and Slepcev (utils.boundary_statistic) in its radius and its kNN form.  T estimates the distance to the
boundary along the estimated inward normal, so the points whose T lies below a low quantile are the boundary points: here they are
compared with the points that really lie within a thin ring at the disc's edge, and the normals with the true ones.  The graphs are
built, and the statistic is computed, on the device; the normals equal the reference's bit for bit."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import graphlearning_amd as gl

rng = np.random.default_rng(0)
n = 20000
radius = np.sqrt(rng.random(n))
angle = 2 * np.pi * rng.random(n)
X = np.stack([radius * np.cos(angle), radius * np.sin(angle)], axis=1)
dist_to_boundary = 1.0 - radius

for what, r, knn in (('radius 0.05', 0.05, False), ('k = 50 neighbours', 50, True)):
    gl.utils.boundary_statistic(X, r, knn=knn)                      # warm
    t0 = time.perf_counter()
    T, nu = gl.utils.boundary_statistic(X, r, knn=knn, return_normals=True)
    ms = 1e3 * (time.perf_counter() - t0)
    found = T < np.quantile(T, 0.05)                                # the 5 % of the points with the smallest statistic
    ring = dist_to_boundary < np.quantile(dist_to_boundary, 0.05)   # the 5 % that really are closest to the edge
    inward = -X[found] / radius[found, None]
    print('%s: %.2f ms; of the %d points marked as boundary %d lie in the outer ring (%.1f %%), the farthest %.3f from the edge; '
          'their normals point inward within %.1f degrees (median)'
          % (what, ms, found.sum(), (found & ring).sum(), 100.0 * (found & ring).sum() / found.sum(), dist_to_boundary[found].max(),
             np.degrees(np.median(np.arccos(np.clip(np.sum(nu[found] * inward, axis=1), -1, 1))))))
