"""graph.dijkstra and graph.distance_matrix against scipy.sparse.csgraph.dijkstra (C, one core) on the same machine, graph and job.

Inputs: kNN `distance` graphs (k = 10, symmetrised, built on the device) of n = 70 000 and 10^6 uniform points in the plane and in
d = 20, one source, f = 1; a Gaussian kNN graph of n = 5 000 for distance_matrix (reciprocal weights) beside n scipy calls.
Per input and per form -- `active` (the default: a round looks at the values whose in-neighbours moved) and `full` (every round
looks at every value, _hip.SSSP_FULL_SWEEPS) --: end-to-end milliseconds of the call (median of the repeats after a warm-up that
also builds the edge lists; uploads and downloads included), the rounds, the library's host milliseconds per phase
(_hip.sssp_last_ms), and whether the bits equal scipy's.

    python scripts/dijkstra_profile.py [--out profiles/dijkstra.txt] [--only N]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python scripts/dijkstra_profile.py --trace-run
    python scripts/dijkstra_profile.py --kernel-stats DIR --out profiles/dijkstra.txt        (appends the per-kernel table)

profiles/dijkstra.txt is those three steps in one job."""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'dijkstra.txt'))
ap.add_argument('--only', type=int, default=None)
ap.add_argument('--trace-run', action='store_true')
ap.add_argument('--kernel-stats', default=None)
a = ap.parse_args()

INPUTS = [('planar', 70000, 2), ('planar', 1000000, 2), ('d = 20', 70000, 20), ('d = 20', 1000000, 20)]


def timed(fn, min_s=1.0, min_n=3):
    out, ts = None, []
    t_begin = time.perf_counter()
    while time.perf_counter() - t_begin < min_s or len(ts) < min_n:
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


def main():
    import graphlearning_amd as gl
    from graphlearning_amd import _hip
    from scipy import sparse
    from scipy.sparse import csgraph
    _hip.require_device()
    lines = ['# graph.dijkstra on one MI355X against scipy.sparse.csgraph.dijkstra (one core) on the same machine and graph; ms = median '
             'of the repeats, phases = host ms inside the library (uploads | distance rounds | closest-point rounds | downloads)']
    for idx, (name, n, d) in enumerate(INPUTS):
        if a.only is not None and idx != a.only:
            continue
        X = np.random.default_rng(100 + idx).random((n, d))
        W = gl.weightmatrix.knn(X, 10, kernel='distance')
        G = gl.graph(W)
        G.dijkstra([0])                                   # warm-up: edge lists, code objects, pools
        if a.trace_run:
            G.dijkstra([0], return_cp=True)
            continue
        t0 = time.perf_counter()
        want = csgraph.dijkstra(W, directed=True, indices=0)
        t_scipy = (time.perf_counter() - t0) * 1e3
        lines.append('%s n=%d k=10: entries=%d | scipy %.1f ms' % (name, n, W.nnz, t_scipy))
        for form in ('active', 'full'):
            _hip.SSSP_FULL_SWEEPS = form == 'full'
            for cp in (False, True):
                res, ts = timed(lambda: G.dijkstra([0], return_cp=cp))
                dist = res[0] if cp else res
                med = float(np.median(ts))
                lines.append('   %-6s %-14s end to end %8.1f ms (median of %d, min %.1f max %.1f) = scipy / %.2f | rounds %s | phases %s | bits %s'
                             % (form, 'with cp' if cp else 'distances only', med, len(ts), min(ts), max(ts), t_scipy / med, G.dijkstra_rounds,
                                ' | '.join('%.1f' % v for v in _hip.sssp_last_ms), 'equal' if dist.tobytes() == want.tobytes() else 'DIFFER'))
        _hip.SSSP_FULL_SWEEPS = False
        print('\n'.join(lines[-5:]), flush=True)
        del W, G, X
    if a.only is None or a.only == len(INPUTS):
        n = 5000
        W = gl.weightmatrix.knn(np.random.default_rng(7).random((n, 2)), 10, kernel='gaussian')
        G = gl.graph(W)
        G.distance_matrix()
        if not a.trace_run:
            Wr = sparse.csr_matrix((1 / W.data, W.indices, W.indptr), shape=W.shape)
            t0 = time.perf_counter()
            want = np.stack([csgraph.dijkstra(Wr, directed=True, indices=i) for i in range(n)])
            t_calls = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            csgraph.dijkstra(Wr, directed=True)
            t_one = (time.perf_counter() - t0) * 1e3
            lines.append('distance_matrix n=%d k=10 gaussian: entries=%d | %d scipy calls %.0f ms, one all-pairs scipy call %.0f ms' % (n, W.nnz, n, t_calls, t_one))
            for form in ('active', 'full'):
                _hip.SSSP_FULL_SWEEPS = form == 'full'
                T, ts = timed(G.distance_matrix)
                med = float(np.median(ts))
                lines.append('   %-6s end to end %8.1f ms (median of %d, min %.1f max %.1f) = the %d calls / %.1f = the one call / %.1f | rounds %s | '
                             'phases %s | bits %s' % (form, med, len(ts), min(ts), max(ts), n, t_calls / med, t_one / med, G.dijkstra_rounds,
                                                      ' | '.join('%.1f' % v for v in _hip.sssp_last_ms), 'equal' if T.tobytes() == want.tobytes() else 'DIFFER'))
            _hip.SSSP_FULL_SWEEPS = False
            print('\n'.join(lines[-3:]), flush=True)
    if not a.trace_run:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


def kernel_stats():
    fs = glob.glob(os.path.join(a.kernel_stats, '**', '*kernel_stats.csv'), recursive=True)
    if not fs:
        sys.exit('no kernel_stats.csv under ' + a.kernel_stats)
    rows = list(csv.DictReader(open(fs[0])))
    out = ['# rocprofv3 --kernel-trace --stats over the graph builds, one warm-up and one call with closest points per input and one '
           'distance_matrix (a run of its own, default form): per kernel, all inputs together; the copies are the __amd_rocclr rows']
    out.append('%-64s %7s %12s %12s %7s' % ('kernel', 'calls', 'total ms', 'average us', '%'))
    for r in rows:
        name = r.get('Name') or r.get('KernelName') or ''
        out.append('%-64s %7s %12.3f %12.2f %7.2f' % (name[:64], r['Calls'], float(r['TotalDurationNs']) / 1e6, float(r['AverageNs']) / 1e3,
                                                     float(r['Percentage'])))
    with open(a.out, 'a') as f:
        f.write('\n'.join(out) + '\n')
    print('\n'.join(out))


if __name__ == '__main__':
    if a.kernel_stats:
        kernel_stats()
    else:
        main()
