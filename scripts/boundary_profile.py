"""utils.boundary_statistic on one MI355X against the vectorised numpy restatement (tests/boundary_ref.py: statistic) on one core of the
same machine.  Per case: the public call end to end (graph construction on the device included, warm), the library call alone
(_hip.boundary_stat on the finished pattern) with its parts (_hip.boundary_stat_last: checks, upload, kernels, download), results
compared bit for bit; then the kernels under other thresholds between the row classes (csrc/bstat_plan.h: BSTAT_WAVE_ROW).  The
baseline gets the finished pattern and lists: neither the graph construction nor the reference's second search (a kNN search with
k = the largest degree, which the walk over the ball graph replaces) is in its time.  Cases: 70 000 uniform points in the unit
square with a radius that gives degrees around 50, the same points in the kNN mode with k = 30, a radius with degrees around 200
and the first pattern plus one vertex joined to all others (both thresholds only), and 600 points.  Last: what the compiler reports for the new kernels (registers, scratch, occupancy).

    python scripts/boundary_profile.py [--out profiles/boundary.txt] [--no-resources]"""
import argparse
import os
import re
import subprocess
import sys
import time

for var in ('OMP_NUM_THREADS', 'OPENBLAS_NUM_THREADS', 'MKL_NUM_THREADS'):       # the baseline runs on one core
    os.environ[var] = '1'
import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'tests'))
ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'boundary.txt'))
ap.add_argument('--no-resources', action='store_true')
a = ap.parse_args()

THRESHOLDS = (1, 64, 128, 256, 512, 1024, 4096, 1 << 30)


def spread(ts):
    return '%.3f ms (median of %d, %.3f .. %.3f)' % (float(np.median(ts)), len(ts), min(ts), max(ts))


def thresholds(say, X, W, J):
    from graphlearning_amd import _hip
    try:
        for t in THRESHOLDS:
            _hip.boundary_stat_set_wave_row(t)
            ks = []
            for _ in range(7):
                _hip.boundary_stat(X, W.indptr, W.indices, J=J)
                ks.append(_hip.boundary_stat_last[6])
            say('    rows of >= %s members take a wavefront (%d rows do, %d take 16 lanes): kernels %s'
                % ('never' if t == 1 << 30 else t, _hip.boundary_stat_last[2], _hip.boundary_stat_last[1], spread(ks[1:])))
    finally:
        _hip.boundary_stat_set_wave_row(0)


def graph_of(gl, X, r, knn):
    if knn:
        J, D = gl.weightmatrix.knnsearch(X, r)
        return gl.weightmatrix.knn(X, r, kernel='uniform', symmetrize=False, knn_data=(J, D)), np.ascontiguousarray(J, dtype=np.int32)
    return gl.weightmatrix.epsilon_ball(X, r, kernel='uniform'), None


def case(say, gl, X, r, knn, what, repeats=7, baseline=True):
    import boundary_ref as ref
    from graphlearning_amd import _hip
    W, J = graph_of(gl, X, r, knn)
    lens = np.diff(W.indptr)
    say('%s: n=%d d=%d %s, entries=%d, row lengths %d .. %d' % (what, X.shape[0], X.shape[1], ('k=%d' % r) if knn else ('r=%.5f' % r), W.nnz,
                                                                 lens.min(), lens.max()))
    if not baseline:
        thresholds(say, X, W, J)
        return
    cpu = []
    for _ in range(2):
        t0 = time.perf_counter()
        want_T, want_nu = ref.statistic(X, W.indptr, W.indices, J=J)
        cpu.append((time.perf_counter() - t0) * 1e3)
    gl.utils.boundary_statistic(X, r, knn=knn)                         # warm: the pools, the staging area
    ts, lib, parts = [], [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        T, nu = gl.utils.boundary_statistic(X, r, knn=knn, return_normals=True)
        ts.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        T2, nu2 = _hip.boundary_stat(X, W.indptr, W.indices, J=J)
        lib.append((time.perf_counter() - t0) * 1e3)
        parts.append(_hip.boundary_stat_last)
    parts = np.median(np.array(parts), axis=0)
    say('  bits: nu %s, T %s (public call); library call alone: nu %s, T %s'
        % tuple('equal' if x.tobytes() == y.tobytes() else 'DIFFERENT' for x, y in ((nu, want_nu), (T, want_T), (nu2, want_nu), (T2, want_T))))
    say('  restatement (vectorised numpy) on one core, pattern and lists given: %s' % spread(cpu))
    pub, one = float(np.median(ts)), float(np.median(lib))
    say('  public call end to end (graph built on the device): %s -> x %.1f%s'
        % (spread(ts), np.median(cpu) / pub, '' if np.median(cpu) > pub else ' (SLOWER than one core)'))
    say('  library call alone: %s -> x %.1f%s' % (spread(lib), np.median(cpu) / one, '' if np.median(cpu) > one else ' (SLOWER than one core)'))
    say('    %d launches; %d rows on 16 lanes, %d on a wavefront, %d full rows; checks %.3f ms, upload %.3f ms, kernels %.3f ms, '
        'download %.3f ms; kernels alone x %.0f' % (parts[0], parts[1], parts[2], parts[3], parts[4], parts[5], parts[6], parts[7],
                                                    np.median(cpu) / parts[6]))
    say('  other thresholds between the row classes:')
    thresholds(say, X, W, J)


def resources(say):
    """registers, scratch and occupancy of the kernels of csrc/bstat.hip as the compiler reports them"""
    from graphlearning_amd import _build
    src = os.path.join(HERE, 'graphlearning_amd', 'csrc', 'bstat.hip')
    res = subprocess.run([_build._hipcc()] + _build._flags() + ['-Rpass-analysis=kernel-resource-usage', '-c', src, '-o', os.devnull],
                         capture_output=True, text=True)
    say('kernels of csrc/bstat.hip, as the compiler reports them (gfx950):')
    name = None
    row = {}
    for line in res.stderr.splitlines():
        m = re.search(r'remark:\s+(.*?)\s+\[-Rpass', line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith('Function Name:'):
            name, row = text.split(':', 1)[1].strip(), {}
        for key in ('VGPRs', 'AGPRs', 'TotalSGPRs', 'ScratchSize [bytes/lane]', 'Occupancy [waves/SIMD]', 'LDS Size [bytes/block]'):
            if text.startswith(key + ':'):
                row[key] = text.split(':', 1)[1].strip()
        if name and text.startswith('LDS Size'):
            say('  %s: VGPRs %s, AGPRs %s, SGPRs %s, scratch %s bytes/lane, occupancy %s waves/SIMD, LDS %s bytes'
                % (name, row.get('VGPRs'), row.get('AGPRs'), row.get('TotalSGPRs'), row.get('ScratchSize [bytes/lane]'),
                   row.get('Occupancy [waves/SIMD]'), row.get('LDS Size [bytes/block]')))
            name = None


def main():
    import graphlearning_amd as gl
    from graphlearning_amd import _hip
    _hip.require_device()
    lines = ['# utils.boundary_statistic on one MI355X against the vectorised numpy restatement on one core of the same machine; times warm']

    def say(line):
        lines.append(line)
        print(line, flush=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    rng = np.random.default_rng(1)
    X = rng.random((70000, 2))
    r50 = float(np.sqrt(50 / (70000 * np.pi)))
    case(say, gl, X, r50, False, 'radius mode, degrees around 50')
    case(say, gl, X, 30, True, 'kNN mode, k = 30')
    case(say, gl, X, 2 * r50, False, 'radius mode, degrees around 200 (thresholds only)', baseline=False)
    from scipy import sparse
    W = gl.weightmatrix.epsilon_ball(X, r50, kernel='uniform')
    hub = sparse.bmat([[W, np.ones((70000, 1))], [np.ones((1, 70000)), None]], format='csr')
    hub.sort_indices()
    say('the degrees-around-50 pattern plus one vertex joined to all others: n=%d entries=%d, longest row %d; thresholds only:'
        % (hub.shape[0], hub.nnz, np.diff(hub.indptr).max()))
    thresholds(say, np.vstack([X, [[0.5, 0.5]]]), hub, None)
    Y = rng.random((600, 2))
    case(say, gl, Y, float(np.sqrt(20 / (600 * np.pi))), False, '600 points, radius mode, degrees around 20')
    case(say, gl, Y, 15, True, '600 points, kNN mode, k = 15')
    if not a.no_resources:
        resources(say)


if __name__ == '__main__':
    main()
