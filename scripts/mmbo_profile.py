"""ssl.multiclass_mbo on the 70 000-vertex `connected` graph of profiles/eig.txt (bench.py's generator at scale = 0.8: 10 classes, one
component) with 10 labels per class at the defaults, and on the 600-vertex `blobs` fixture, against the plain-numpy form of the
reference's loop (ssl.py:972-996, tests/mmbo_ref.py: numpy_loop) on one core of the same machine with the same eigenpairs and the same
start: the fit with a cold and with a cached decomposition, the device call alone, a call of one step (the uploads), time per step.
Every time is end to end, warm, median (min .. max).  The split of a step into pass and finishing kernel needs a kernel trace: run
this script with --calls N under a profiler in a run of its own; it then only repeats the device call on the large graph.

    python scripts/mmbo_profile.py [--out profiles/mmbo.txt] [--calls N]"""
import argparse
import os
import sys
import time

for var in ('OMP_NUM_THREADS', 'OPENBLAS_NUM_THREADS', 'MKL_NUM_THREADS'):       # the numpy loop runs on one core
    os.environ[var] = '1'
import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'tests'))
ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'mmbo.txt'))
ap.add_argument('--calls', type=int, default=0)
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


def case(say, gl, ref, W, truth, per_class, what):
    from graphlearning_amd import _hip
    n = W.shape[0]
    k = len(np.unique(truth))
    rng = np.random.default_rng(0)
    ind = np.concatenate([rng.choice(np.where(truth == c)[0], size=per_class, replace=False) for c in range(k)])
    labels = truth[ind].astype(np.int32)

    def cold():
        np.random.seed(0)
        model = gl.ssl.multiclass_mbo(gl.graph(W))
        model.fit(ind, labels)
        return model
    cold()
    model, ts_cold = timed(cold)
    _, ts_warm = timed(lambda: model.fit(ind, labels))
    vals, X = model.graph.eigen_decomp(normalization='normalized', k=50)
    np.random.seed(0)
    lab0 = ref.start_labels(np.random.rand(k, n), ind, labels)
    (hist, Z, plan), ts_call = timed(lambda: _hip.mmbo_solve(X, vals, lab0, ind, labels, k))
    _, ts_one = timed(lambda: _hip.mmbo_solve(X, vals, lab0, ind, labels, k, Ns=1, T=1))
    steps = 60
    per_step = (float(np.median(ts_call)) - float(np.median(ts_one))) * 1e3 / (steps - 1)
    acc = gl.ssl.ssl_accuracy(hist[-1], truth, ind)
    say('%s: n=%d entries=%d classes=%d labels=%d, Ns=6 T=10 num_eig=50, plan %s, accuracy %.2f %%' % (what, n, W.nnz, k, len(ind), plan, acc))
    say('  fit, cold decomposition: %s; cached decomposition: %s' % (spread(ts_cold), spread(ts_warm)))
    say('  device call alone (uploads, 121 launches, downloads): %s; the same call with ONE step (the checked upload of X, %.1f MB, and the '
        'other arrays): %s -> %.1f us per step beyond the first, %.2f TB/s on the n m 8 = %.1f MB of X a pass reads'
        % (spread(ts_call), n * 50 * 8 / 1e6, spread(ts_one), per_step, n * 50 * 8 / per_step / 1e6, n * 50 * 8 / 1e6))
    t0 = time.perf_counter()
    nhist, gap = ref.numpy_loop(vals, X, lab0, ind, labels, k)
    sec = time.perf_counter() - t0
    med = float(np.median(ts_call))
    say('  plain-numpy loop on one core of this machine, same eigenpairs and start: %.1f ms, labels that differ %d of %d (smallest top-two gap '
        '%.2g) -> x %.1f against the device call%s, x %.1f against the cached fit'
        % (sec * 1e3, int((nhist[-1] != hist[-1]).sum()), n, gap, sec * 1e3 / med, '' if sec * 1e3 > med else ' (SLOWER than the CPU)',
           sec * 1e3 / float(np.median(ts_warm))))
    return X, vals, lab0, ind, labels, k


def main():
    import graphlearning_amd as gl
    from graphlearning_amd import _hip
    import eig_ref
    import mmbo_ref as ref
    from bench import load_labels, make_features
    _hip.require_device()
    labels = load_labels(70000)
    W = gl.weightmatrix.knn(make_features(labels, scale=0.8), 10)
    if a.calls:
        G = gl.graph(W)
        vals, X = G.eigen_decomp(normalization='normalized', k=50)
        ind = gl.trainsets.generate(labels, rate=10, seed=0)
        lab0 = ref.start_labels(np.random.RandomState(0).rand(10, 70000), ind, labels[ind])
        for _ in range(a.calls):
            _hip.mmbo_solve(X, vals, lab0, ind, labels[ind], 10)
        print('calls', a.calls, flush=True)
        return
    lines = ['# ssl.multiclass_mbo on one MI355X; times end to end, warm']

    def say(line):
        lines.append(line)
        print(line, flush=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    gold = eig_ref.load_golden()
    case(say, gl, ref, eig_ref.golden_graph(gold, 'blobs'), gold['graph_blobs_truth'], 5, 'blobs fixture')
    case(say, gl, ref, W, labels, 10, '70 000-vertex graph (scale 0.8)')


if __name__ == '__main__':
    main()
