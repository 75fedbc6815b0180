"""weightmatrix.epsilon_ball against the reference-equivalent host path, on the same machine in the same job.

Inputs: 10^6 uniform points in 3-D at epsilon = 0.0174 (21.6 M entries); a 512 x 512 pixel grid, epsilon = 5, three features per
pixel; the reference example's 10^4 x 2 at epsilon = 0.02.  Per input: end-to-end milliseconds of epsilon_ball (median over
repeats filling more than a second, after a warm-up; uploads, checked transfers and the scipy wrapper included) beside the host
path's seconds (cKDTree.query_pairs + numpy row sums + COO -> CSR: once with the reference's own set of tuples, once with
query_pairs' array output, which is the fastest the host offers); device ms per stage, pairs tested and accepted
(_hip.ball_stats); pair tests per second of the count pass against the fp64 vector ceiling without fused multiply-adds, and the bytes the fill writes against
HBM bandwidth, naming which of the two bounds the fill.

    python scripts/epsball_profile.py [--out profiles/epsball.txt] [--no-host] [--only N]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python scripts/epsball_profile.py --trace-run
    python scripts/epsball_profile.py --kernel-stats DIR --out profiles/epsball.txt        (appends the per-kernel table)

profiles/epsball.txt is those three steps in one job."""
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
ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'epsball.txt'))
ap.add_argument('--no-host', action='store_true')
ap.add_argument('--only', type=int, default=None)
ap.add_argument('--trace-run', action='store_true')
ap.add_argument('--kernel-stats', default=None)
a = ap.parse_args()

# fp64 vector ceiling of THESE kernels: 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 39.3 T instructions/s.  The usual 78.6 TFLOP/s
# (half the fp32 vector rate of the hardware guide's table) counts a fused multiply-add as two, and contraction is off here by
# design (the sums must round as the reference's do), so a subtraction, a multiplication and an addition are one flop each.
# HBM3E 8 TB/s (spec)
FP64_PEAK, HBM_PEAK = 39.3e12, 8.0e12


def inputs():
    m = 512
    g = np.meshgrid(np.arange(float(m)), np.arange(float(m)), indexing='ij')
    yield ('uniform 10^6 x 3, eps 0.0174', np.random.default_rng(8).random((10 ** 6, 3)), 0.0174, None)
    yield ('pixels 512 x 512, eps 5, 3 features', np.stack([g[0].ravel(), g[1].ravel()], axis=1), 5.0,
           np.random.default_rng(12).random((m * m, 3)))
    yield ('uniform 10^4 x 2, eps 0.02', np.random.default_rng(0).random((10 ** 4, 2)), 0.02, None)


def host_path(X, eps, F, output_type):
    """The reference's steps (weightmatrix.py:234-266) with numpy and scipy."""
    from scipy import sparse, spatial
    n = X.shape[0]
    t0 = time.perf_counter()
    M = spatial.cKDTree(X).query_pairs(eps, output_type=output_type)
    if output_type == 'set':
        M = np.array(list(M))
    t1 = time.perf_counter()
    V = X[M[:, 0]] - X[M[:, 1]]
    w = np.exp(-4 * np.sum(V * V, axis=1) / (eps * eps))
    if F is not None:
        VF = F[M[:, 0]] - F[M[:, 1]]
        w = w * np.exp(-4 * np.sum(VF * VF, axis=1) / 1.0)
    W = sparse.coo_matrix((np.concatenate((w, w)), (np.concatenate((M[:, 0], M[:, 1])), np.concatenate((M[:, 1], M[:, 0])))), shape=(n, n))
    W = W.tocsr()
    t2 = time.perf_counter()
    return W, t1 - t0, t2 - t1


def main():
    import graphlearning_amd as gl
    from graphlearning_amd import _hip
    _hip.require_device()
    os.environ.pop('GLX_HOST_EXP', None)          # the default mode: the exponential on the device
    lines = ['# weightmatrix.epsilon_ball (gaussian kernel, default mode) on one MI355X against the host path on the same machine; '
             'ms = median of the repeats, device ms from _hip.ball_stats (minimum over the repeats); the fp64 ceiling is 39.3 TFLOP/s: '
             'one flop per instruction, since nothing here may be fused (78.6 TFLOP/s would count an fma as two)']
    for idx, (name, X, eps, F) in enumerate(inputs()):
        if a.only is not None and idx != a.only:
            continue
        W = gl.weightmatrix.epsilon_ball(X, eps, features=F)          # warm-up: code objects, pools, page-locked result arrays
        if a.trace_run:
            gl.weightmatrix.epsilon_ball(X, eps, features=F)
            continue
        wall, stats = [], []
        t_begin = time.perf_counter()
        while time.perf_counter() - t_begin < 1.2 or len(wall) < 5:
            t0 = time.perf_counter()
            W = gl.weightmatrix.epsilon_ball(X, eps, features=F)
            wall.append((time.perf_counter() - t0) * 1e3)
            stats.append(_hip.ball_stats())
        st = {k: min(s[k] for s in stats) for k in stats[0]}
        n, d = X.shape
        nnz = W.nnz
        dev = st['grid_ms'] + st['count_ms'] + st['fill_ms'] + st['sort_ms'] + st['weights_ms']
        lines.append('%s: n=%d entries=%d | end to end %.1f ms (median of %d, min %.1f max %.1f) | device kernels %.2f ms: grid %.2f, '
                     'count+scan %.2f, fill %.2f, sort %.2f, weights+scan %.2f | cells %d'
                     % (name, n, nnz, float(np.median(wall)), len(wall), min(wall), max(wall), dev, st['grid_ms'], st['count_ms'],
                        st['fill_ms'], st['sort_ms'], st['weights_ms'], st['cells']))
        flop = 3 * d            # per pair test: d subtractions, d multiplications, d additions (no fma)
        tests = st['pairs_tested']
        t_ops = tests * flop / FP64_PEAK
        t_bytes = nnz * 4 / HBM_PEAK
        lines.append('   pairs tested %.3e (%.2e n^2, %.1f per accepted pair), accepted %d | count pass %.3e pair tests/s = %.2f TFLOP/s fp64 '
                     '(%d flop per test, none fused) = %.3f of the %.1f TFLOP/s the vector unit gives without fma'
                     % (tests, tests / (float(n) * n), tests / max(nnz, 1), nnz, tests / (st['count_ms'] * 1e-3),
                        tests * flop / (st['count_ms'] * 1e-3) / 1e12, flop, tests * flop / (st['count_ms'] * 1e-3) / FP64_PEAK, FP64_PEAK / 1e12))
        lines.append('   fill: the same %.3e tests need %.3f ms at that ceiling, its %.1f MB of column ids %.3f ms at %.0f TB/s: bound by %s; '
                     'measured %.2f ms = %.3f of that bound'
                     % (tests, t_ops * 1e3, nnz * 4 / 1e6, t_bytes * 1e3, HBM_PEAK / 1e12, 'arithmetic' if t_ops > t_bytes else 'bandwidth',
                        st['fill_ms'], max(t_ops, t_bytes) * 1e3 / st['fill_ms']))
        lines.append('   result %.1f MB (indptr, indices, data) comes down over the host link inside the end-to-end figure'
                     % ((nnz * 12 + 4 * (n + 1)) / 1e6))
        if not a.no_host:
            for ot in ('set', 'ndarray'):
                Wh, t_pairs, t_asm = host_path(X, eps, F, ot)
                same = Wh.nnz == nnz
                lines.append('   host path (query_pairs -> %s): pairs %.2f s + assembly %.2f s = %.2f s = %.0f x the end-to-end time above; entries %s'
                             % (ot, t_pairs, t_asm, t_pairs + t_asm, (t_pairs + t_asm) * 1e3 / float(np.median(wall)),
                                'equal' if same else 'DIFFER (%d)' % Wh.nnz))
                del Wh
        print('\n'.join(lines[-7:]), flush=True)
    if not a.trace_run:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


def kernel_stats():
    fs = glob.glob(os.path.join(a.kernel_stats, '**', '*kernel_stats.csv'), recursive=True)
    if not fs:
        sys.exit('no kernel_stats.csv under ' + a.kernel_stats)
    rows = list(csv.DictReader(open(fs[0])))
    out = ['# rocprofv3 --kernel-trace --stats over one warm-up and one timed call per input (a run of its own): per kernel, all inputs together']
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
