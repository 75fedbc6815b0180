"""graph.eigen_decomp and ssl.poisson(solver='spectral') on the headline graph and on the 600-vertex `blobs` fixture, against
scipy.sparse.linalg.svds (ARPACK, what the reference calls) on one core of the same machine: steps, restarts, time per step.

The graph is the 70 000-vertex k = 10, 10-class graph of bench.py's generator at scale = 0.8, its `connected` workload: the classes
overlap and the kNN graph is ONE component.  (At the generator's default scale the graph has nine components; the eigenvalue 1 is
nine-fold and eigen_decomp ends in the missed-copy error, which is timed too.)  Every time is end to end (the host's scipy
set-up of A, uploads, the host's eigh of the projected matrix, downloads included), over repeated solves on fresh graph objects:
median (min .. max); the first solve of the process is shown apart.  The split of a step into SpMV, projection and update needs a
kernel trace: run this script with --solves N --case NAME under a profiler in a run of its own; it then only repeats that solve.

    python scripts/eig_profile.py [--out profiles/eig.txt] [--no-svds] [--solves N --case normalized|randomwalk|combinatorial]"""
import argparse
import os
import sys
import time

for var in ('OMP_NUM_THREADS', 'OPENBLAS_NUM_THREADS', 'MKL_NUM_THREADS'):       # svds runs on one core
    os.environ[var] = '1'
import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'tests'))
CASES = {'normalized': 50, 'randomwalk': 11, 'combinatorial': 10}
ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'eig.txt'))
ap.add_argument('--no-svds', action='store_true')
ap.add_argument('--solves', type=int, default=0)
ap.add_argument('--case', default='normalized')
a = ap.parse_args()


def timed(fn, min_s=1.0, min_n=3, max_n=9):
    out, ts = None, []
    t_begin = time.perf_counter()
    while (time.perf_counter() - t_begin < min_s or len(ts) < min_n) and len(ts) < max_n:
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


def spread(ts):
    return '%.2f ms (median of %d, %.2f .. %.2f)' % (float(np.median(ts)), len(ts), min(ts), max(ts))


def mean_columns(n, k, steps, restarts):
    """the mean number of basis columns a step's projection and update stream, from the driver's schedule"""
    from graphlearning_amd import _eig
    m = _eig.basis_size(n, k)
    keep = k + (m - k) // 2
    total = sum(range(1, m + 1)) + restarts * sum(range(keep + 1, m + 1))
    return total / float(m + restarts * (m - keep)), m, keep


def decomp_case(say, gl, ref, W, normalization, k, svds=True):
    from graphlearning_amd import _eig
    n = W.shape[0]

    def solve():
        G = gl.graph(W)
        return G.eigen_decomp(normalization=normalization, k=k) + (G.eig_steps, G.eig_restarts, G.eig_probe)
    t0 = time.perf_counter()
    vals, vecs, steps, restarts, probe = solve()
    first = (time.perf_counter() - t0) * 1e3
    _, ts = timed(solve, min_s=max(1.0, 2e-3 * first))
    t0 = time.perf_counter()
    A, D, M = _eig.operator(W, normalization)
    _eig.check_weights(W, normalization, k)
    setup = (time.perf_counter() - t0) * 1e3
    cols, m, keep = mean_columns(n, k, steps, restarts)
    med = float(np.median(ts))
    say("  eigen_decomp('%s', k=%d): m=%d keep=%d steps=%d restarts=%d probe=%.6g | %s, first solve of the process %.0f ms; host set-up of A "
        'and the checks %.1f ms of it -> %.1f us per step all told, %.1f columns per step on average'
        % (normalization, k, m, keep, steps, restarts, probe, spread(ts), first, setup, (med - setup) * 1e3 / steps, cols))
    if svds:
        t0 = time.perf_counter()
        s_ref, u_ref = ref.svds_reference(A, k)
        sec = time.perf_counter() - t0
        s = (1 - vals) if M is None else (M - vals)
        say('    scipy svds(tol=0) on one core of this machine: %.2f s, largest |s - s_ref| / s_max %.1e, subspace defect %.1e -> x %.1f %s'
            % (sec, float(np.abs(s - s_ref).max() / s_ref[0]), ref.subspace_defect(ref.a_vectors(W, normalization, vecs), u_ref),
               sec * 1e3 / med, '' if sec * 1e3 > med else '(SLOWER than the CPU)'))
    return med


def main():
    import graphlearning_amd as gl
    from graphlearning_amd import _hip
    import eig_ref as ref
    from bench import load_labels, make_features
    _hip.require_device()
    labels = load_labels(70000)
    W = gl.weightmatrix.knn(make_features(labels, scale=0.8), 10)
    if a.solves:
        for _ in range(a.solves):
            G = gl.graph(W)
            G.eigen_decomp(normalization=a.case, k=CASES[a.case])
        print('solves', a.solves, a.case, 'steps', G.eig_steps, 'restarts', G.eig_restarts, 'ms of the last', flush=True)
        return
    lines = ['# graph.eigen_decomp and ssl.poisson(solver=\'spectral\') on one MI355X; times end to end']

    def say(line):
        lines.append(line)
        print(line, flush=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    gold = ref.load_golden()
    Wb = ref.golden_graph(gold, 'blobs')
    say('blobs fixture: n=%d entries=%d' % (Wb.shape[0], Wb.nnz))
    for normalization, k in CASES.items():
        decomp_case(say, gl, ref, Wb, normalization, k, svds=not a.no_svds)
    from scipy import sparse
    say('70 000-vertex graph (scale 0.8): n=%d entries=%d components=%d' % (W.shape[0], W.nnz, sparse.csgraph.connected_components(W)[0]))
    train_ind = gl.trainsets.generate(labels, rate=10, seed=0)
    tl = labels[train_ind]
    model = gl.ssl.poisson(W, solver='spectral')
    t0 = time.perf_counter()
    model.fit(train_ind, tl)
    cold = (time.perf_counter() - t0) * 1e3
    _, ts = timed(lambda: model.fit(train_ind, tl))
    acc = gl.ssl.ssl_accuracy(model.predict(), labels, train_ind)
    say("  poisson(solver='spectral') fit, 10 classes, 100 labels: cold (the decomposition of the graph without its diagonal, k=11) %.1f ms; "
        'cached %s; accuracy %.2f %%' % (cold, spread(ts), acc))
    for normalization, k in CASES.items():
        decomp_case(say, gl, ref, W, normalization, k, svds=not a.no_svds)
    Wd = gl.weightmatrix.knn(make_features(labels), 10)
    t0 = time.perf_counter()
    try:
        gl.graph(Wd).eigen_decomp(normalization='normalized', k=50)
        say('  default scale (%d components): no error' % sparse.csgraph.connected_components(Wd)[0])
    except _hip.GlxError as e:
        say('  default scale (%d components): %.1f ms until %s' % (sparse.csgraph.connected_components(Wd)[0], (time.perf_counter() - t0) * 1e3,
                                                                  str(e)[:120]))


if __name__ == '__main__':
    main()
