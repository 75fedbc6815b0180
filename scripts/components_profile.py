"""graph.connected_components on one MI355X against scipy.sparse.csgraph.connected_components(W, directed=False) on one core of the
same machine: the call end to end (warm), its four parts (_hip.components_last_ms: upload, checks, kernels, download), labels
compared on every vertex; then the kernels alone under other row-class thresholds (csrc/cc_plan.h: CC_WAVE_ROW).  Graphs: bench.py's
70 000-vertex k = 10 graph at the default scale (nine components) and at scale 0.8 (`connected`), a 10^6-vertex k = 10 graph from the
same generator, the 600-vertex `blobs` fixture, and -- for the thresholds only -- the 70 000-vertex graph plus one vertex joined to all
others and two epsilon-ball graphs with rows of hundreds of entries.

    python scripts/components_profile.py [--out profiles/components.txt] [--skip-million]"""
import argparse
import os
import sys
import time

for var in ('OMP_NUM_THREADS', 'OPENBLAS_NUM_THREADS', 'MKL_NUM_THREADS'):       # scipy's traversal runs on one core anyway
    os.environ[var] = '1'
import numpy as np  # noqa: E402
from scipy import sparse  # noqa: E402

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'tests'))
ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'components.txt'))
ap.add_argument('--skip-million', action='store_true')
a = ap.parse_args()

THRESHOLDS = (8, 32, 128, 512, 1024, 4096, 1 << 30)


def spread(ts):
    return '%.3f ms (median of %d, %.3f .. %.3f)' % (float(np.median(ts)), len(ts), min(ts), max(ts))


def thresholds(say, gl, W):
    from graphlearning_amd import _hip
    G = gl.graph(W)
    try:
        for t in THRESHOLDS:
            _hip.components_set_wave_row(t)
            ks = []
            for _ in range(7):
                G.connected_components()
                ks.append(_hip.components_last_ms[2])
            say('    rows of >= %s entries take a wavefront (%d rows do): kernels %s'
                % ('never' if t == 1 << 30 else t, _hip.components_plan()[3], spread(ks[1:])))
    finally:
        _hip.components_set_wave_row(0)


def case(say, gl, W, what, repeats=7):
    from graphlearning_amd import _hip
    from scipy.sparse import csgraph
    n = W.shape[0]
    lengths = np.diff(W.indptr)
    cpu = []
    for _ in range(3):
        t0 = time.perf_counter()
        want_n, want = csgraph.connected_components(W, directed=False)
        cpu.append((time.perf_counter() - t0) * 1e3)
    G = gl.graph(W)
    G.connected_components()                                  # warm: the pools, the staging area
    ts, parts = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        ncomp, labels = G.connected_components()
        ts.append((time.perf_counter() - t0) * 1e3)
        parts.append(_hip.components_last_ms)
    parts = np.median(np.array(parts), axis=0)
    sizes = np.bincount(labels, minlength=ncomp)
    say('%s: n=%d entries=%d, row lengths %d .. %d, %d components (largest %d, smallest %d), labels that differ from scipy\'s: %d'
        % (what, n, W.nnz, lengths.min(), lengths.max(), ncomp, sizes.max(), sizes.min(), int((labels != want).sum()) + abs(ncomp - want_n)))
    say('  scipy on one core: %s' % spread(cpu))
    gpu, kern = float(np.median(ts)), float(parts[2])
    say('  device, end to end: %s -> x %.1f%s' % (spread(ts), np.median(cpu) / gpu, '' if np.median(cpu) > gpu else ' (SLOWER than one core)'))
    say('    upload %.3f ms, checks %.3f ms, kernels %.3f ms, download %.3f ms; kernels alone x %.0f against scipy'
        % (parts[0], parts[1], kern, parts[3], np.median(cpu) / kern))
    t0 = time.perf_counter()
    Gl, ind = G.largest_connected_component()
    say('  largest_connected_component end to end: %.3f ms (%d of %d vertices kept; the host\'s W[ind, :][:, ind] is the rest)'
        % ((time.perf_counter() - t0) * 1e3, int(ind.sum()), n))
    say('  other thresholds between the row classes (the library\'s: %d):' % _hip.components_plan()[1])
    thresholds(say, gl, W)


def main():
    import graphlearning_amd as gl
    from graphlearning_amd import _hip
    import eig_ref
    from bench import load_labels, make_features
    _hip.require_device()
    lines = ['# graph.connected_components on one MI355X against scipy on one core of the same machine; times warm']

    def say(line):
        lines.append(line)
        print(line, flush=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    case(say, gl, eig_ref.golden_graph(eig_ref.load_golden(), 'blobs'), 'blobs fixture')
    labels = load_labels(70000)
    case(say, gl, gl.weightmatrix.knn(make_features(labels), 10), '70 000-vertex k = 10 graph, default scale')
    case(say, gl, gl.weightmatrix.knn(make_features(labels, scale=0.8), 10), '70 000-vertex k = 10 graph, scale 0.8 (`connected`)')
    W70 = gl.weightmatrix.knn(make_features(labels), 10)
    hub = sparse.bmat([[W70, np.ones((70000, 1))], [np.ones((1, 70000)), None]], format='csr')
    say('the 70 000-vertex graph plus one vertex joined to all others: n=%d entries=%d, longest row %d; thresholds only:'
        % (hub.shape[0], hub.nnz, np.diff(hub.indptr).max()))
    thresholds(say, gl, hub)
    Y = np.random.default_rng(5).random((20000, 2))
    for radius in (0.05, 0.1):
        W = gl.weightmatrix.epsilon_ball(Y, radius)
        say('epsilon-ball graph (20 000 uniform points in the unit square, radius %s): n=%d entries=%d, row lengths %d .. %d; thresholds only:'
            % (radius, W.shape[0], W.nnz, np.diff(W.indptr).min(), np.diff(W.indptr).max()))
        thresholds(say, gl, W)
    if not a.skip_million:
        labels = load_labels(1000000)
        case(say, gl, gl.weightmatrix.knn(make_features(labels), 10), '10^6-vertex k = 10 graph, default scale', repeats=5)


if __name__ == '__main__':
    main()
