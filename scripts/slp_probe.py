"""ssl.sparse_label_propagation on the headline graph: milliseconds per fit and per iteration, the rate on the algorithmic bytes, and
the numpy restatement of tests/slp_ref.py on one core of the same machine.

The 70 000-vertex k = 10, 10-class graph of the headline configuration (bench.py's generator), 10 labels per class, T = 100: the
learner's fit end to end (host set-up, reverse index, uploads, 200 launches, download), warm, median of the repeats; the marginal
time of an iteration from two calls of _hip.slp_iterate that differ by six replayed chunks (T = 100 and T = 196: set-up, transfers and
the eager tail are the same in both, so the difference is 96 iterations of the two kernels); the bytes one iteration has to move at
least (every array read or written once per phase) over that time, beside what the micro-architecture guide measured for random
whole-line gathers out of the Infinity Cache.  The numpy form runs --ref-classes class columns for --ref-iters iterations and is
scaled to 10 classes and T = 100; equal bits with the device are ASSERTED on those columns.  A second, small configuration (3 000
vertices, 3 classes) stands beside the time the golden generator measured for the reference itself (tests/golden/g16_slp_2.npz).

    python scripts/slp_probe.py [--out profiles/slp.txt] [--ref-classes 2] [--ref-iters 10]"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'tests'))
ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'slp.txt'))
ap.add_argument('--ref-classes', type=int, default=2)
ap.add_argument('--ref-iters', type=int, default=10)
a = ap.parse_args()


def timed(fn, min_s=1.0, min_n=5, max_n=25):
    out, ts = None, []
    t_begin = time.perf_counter()
    while (time.perf_counter() - t_begin < min_s or len(ts) < min_n) and len(ts) < max_n:
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


def iteration_bytes(n, M, tiles):
    """What one iteration reads and writes at least, every array once per phase, summed over the column tiles."""
    total = 0
    for cols in tiles:
        vertex = M * (2 * 8 * cols + 8 + 4) + n * (8 + 8 + 4 + 3 * 8 * cols)          # Y[e], Y[rev[e]], w, rev | row_ptr, gamma, lab, u in/out, ut
        edge = M * (3 * 8 * cols + 8 + 8 + 4) + n * (8 + 8 * cols)                    # Y in/out, ut[j], w, lam, col | row_ptr, ut[i]
        total += vertex + edge
    return total


def measure(gl, _hip, ref, W, train_ind, train_labels, k, name, lines, numpy_too):
    n, M = W.shape[0], W.nnz
    model = gl.ssl.sparse_label_propagation(W, T=100)
    model.fit(train_ind, train_labels)                               # warm-up: code objects, pools
    prob, ts = timed(lambda: np.array(model.fit(train_ind, train_labels), copy=True))
    fit_ms = float(np.median(ts))
    indptr, indices, w, lam, gamma, _ = ref.setup(W)
    val = (train_labels[:, None] == np.arange(k)[None, :]).astype(np.float64)
    ind32 = train_ind.astype(np.int32)
    call = lambda T: _hip.slp_iterate(indptr, indices, w, lam, gamma, ind32, val, T)
    u100, t100 = timed(lambda: call(100))
    assert u100[0].tobytes() == prob.tobytes()
    _, t196 = timed(lambda: call(196))
    it_ms = (float(np.median(t196)) - float(np.median(t100))) / 96
    tiles = [k] if k <= 16 else None
    nbytes = iteration_bytes(n, M, tiles)
    lines.append('%s: n=%d entries=%d classes=%d labelled=%d T=100 plan=%s' % (name, n, M, k, len(train_ind), model.slp_plan))
    lines.append('    fit, end to end          %8.2f ms (median of %d, %.2f .. %.2f) = %.3f ms per iteration of wall time' % (
        fit_ms, len(ts), min(ts), max(ts), fit_ms / 100))
    lines.append('    device call alone        %8.2f ms for T=100, %8.2f ms for T=196 -> %.4f ms per iteration on the device (two kernels), '
                 '%.2f ms for 100' % (float(np.median(t100)), float(np.median(t196)), it_ms, it_ms * 100))
    lines.append('    algorithmic bytes        %.1f MB per iteration -> %.2f TB/s (the guide: random whole lines out of the Infinity Cache '
                 '7.4-8.6 TB/s, in-order HBM sweep 6.0-6.1 TB/s)' % (nbytes / 1e6, nbytes / (it_ms * 1e-3) / 1e12))
    if numpy_too:
        K, Tn = max(1, min(a.ref_classes, k)), a.ref_iters
        cols = list(range(K))
        t0 = time.perf_counter()
        un = ref.slp_numpy(W, train_ind, train_labels, Tn, k=k, cols=cols)
        np_ms = (time.perf_counter() - t0) * 1e3
        ud = call(Tn)[0]
        assert np.ascontiguousarray(ud[:, cols]).tobytes() == un.tobytes(), 'the device differs from the numpy form'
        scaled = np_ms * (k / K) * (100 / Tn)
        lines.append('    numpy form, one core     %8.0f ms for %d class columns x %d iterations -> %.0f ms scaled to %d classes x 100 = fit x %.0f '
                     '| bits equal' % (np_ms, K, Tn, scaled, k, scaled / fit_ms))
    for ln in lines[-5:]:
        print(ln, flush=True)
    return fit_ms


def main():
    import graphlearning_amd as gl
    from graphlearning_amd import _hip
    from bench import load_labels, make_features
    import slp_ref as ref
    _hip.require_device()
    lines = ['# ssl.sparse_label_propagation on one MI355X; ms = median of the warm repeats (min .. max)']
    labels = load_labels(70000)
    W = ref.canonical(gl.weightmatrix.knn(make_features(labels), 10))
    train_ind = gl.trainsets.generate(labels, rate=10, seed=0)
    measure(gl, _hip, ref, W, train_ind, labels[train_ind].astype(np.int64), len(np.unique(labels)), 'headline graph', lines, True)

    rng = np.random.default_rng(163)
    lab = np.arange(3000) % 3
    X = (rng.normal(size=(3, 5)) * 1.6)[lab] + rng.normal(size=(3000, 5))
    W = ref.canonical(gl.weightmatrix.knn(X, 7))
    ind = np.concatenate([rng.choice(np.where(lab == c)[0], size=5, replace=False) for c in range(3)])
    fit_ms = measure(gl, _hip, ref, W, ind, lab[ind].astype(np.int64), 3, 'small graph', lines, True)
    gold = np.load(os.path.join(HERE, 'tests', 'golden', 'g16_slp_2.npz'))
    ref_s = float(gold['reference_seconds_n3000_k3_T100'])
    lines.append('    the reference itself     %8.0f ms for 3 000 vertices (%d entries), 3 classes, T=100 -- measured by tests/golden/make_golden_slp.py '
                 'on ANOTHER machine (the build container, one core), not on this one = fit x %.0f' % (
                     ref_s * 1e3, int(gold['reference_entries_n3000']), ref_s * 1e3 / fit_ms))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
