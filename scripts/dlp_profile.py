"""ssl.dynamic_label_propagation: the whole fit and the device call alone, warm, on the 70 000-vertex k = 10 graph of bench.py's
generator (10 classes, 10 labels per class) at T = 2 and T = 8, on a 5 000-vertex graph of the same generator (the reference's cap)
and on the 600-vertex `blobs` fixture beside the reference's formula with the dense n x n array (tests/dlp_ref.py: dense_loop; numpy
on one core of the same machine -- the reference itself is not on the GPU machine), and the time per sparse pass and per Gram.

Every time is end to end (uploads, the transpose on the host, downloads included), warm, over repeated runs: median (min .. max).
The time per sparse pass and per Gram (its partial pass and its finishing kernel) needs a kernel trace: run this script with --fits N
under a profiler in a run of its own (scripts/prof_run.py); it then only repeats the T = 8 fit on the headline graph N times, and the
per-kernel table goes into the output file by hand.  What one row of 3 000 entries costs
(one thread walks it alone: the chain is the contract): a 4 097-vertex graph of 10 entries per row with and without such a row, the
difference over the 7 passes over P of a T = 3 call.

    python scripts/dlp_profile.py [--out profiles/dlp.txt] [--no-dense] [--fits N]"""
import argparse
import os
import sys
import time

for var in ('OMP_NUM_THREADS', 'OPENBLAS_NUM_THREADS', 'MKL_NUM_THREADS'):       # the dense loop runs on one core
    os.environ[var] = '1'
import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'tests'))
ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'dlp.txt'))
ap.add_argument('--no-dense', action='store_true')
ap.add_argument('--fits', type=int, default=0)
a = ap.parse_args()


def timed(fn, min_s=1.0, min_n=3, max_n=15):
    out, ts = None, []
    t_begin = time.perf_counter()
    while (time.perf_counter() - t_begin < min_s or len(ts) < min_n) and len(ts) < max_n:
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


def spread(ts):
    return '%.2f ms (median of %d, %.2f .. %.2f)' % (float(np.median(ts)), len(ts), min(ts), max(ts))


def measure(say, gl, _hip, ref, name, W, train_ind, tl, Ts, dense_T=None):
    n, k = W.shape[0], len(np.unique(tl))
    P = ref.transition(W)
    val = ref.onehot(tl, k)
    say('%s: n=%d entries=%d classes=%d labelled=%d' % (name, n, P.nnz, k, len(train_ind)))
    for T in Ts:
        model = gl.ssl.dynamic_label_propagation(W, T=T)
        t0 = time.perf_counter()
        model.fit(train_ind, tl)
        first = time.perf_counter() - t0
        prob, ts_fit = timed(lambda: np.array(model.fit(train_ind, tl), copy=True))
        out, ts_call = timed(lambda: _hip.dlp_solve(P.indptr, P.indices, P.data, train_ind, val, T=T))
        assert out[0].tobytes() == prob.tobytes()
        say('  T=%d: fit %s | device call alone %s | plan (launches, sparse passes, Grams, partials) %s (first fit %.0f ms)' % (
            T, spread(ts_fit), spread(ts_call), model.dlp_plan, first * 1e3))
        if T == dense_T and not a.no_dense:
            t0 = time.perf_counter()
            u, _ = ref.dense_loop(P, train_ind, val, T=T)
            sec = time.perf_counter() - t0
            say('    the reference\'s formula with the dense array, numpy on one core of this machine: %.2f s, largest difference to the device '
                '/ largest entry %.2e -> fit x %.2f' % (sec, float(np.abs(u - prob).max() / np.abs(u).max()), sec * 1e3 / float(np.median(ts_fit))))


def main():
    import graphlearning_amd as gl
    from graphlearning_amd import _hip
    import dlp_ref as ref
    from bench import load_labels, make_features
    from test_dlp_host import load_golden, golden_case
    _hip.require_device()
    lines = ['# ssl.dynamic_label_propagation (alpha 0.05, lam 0.1) on one MI355X; times end to end, warm']

    def say(line):
        lines.append(line)
        print(line, flush=True)
    labels = load_labels(70000)
    W = gl.weightmatrix.knn(make_features(labels), 10)
    train_ind = gl.trainsets.generate(labels, rate=10, seed=0)
    if a.fits:
        model = gl.ssl.dynamic_label_propagation(W, T=8)
        for _ in range(a.fits):
            model.fit(train_ind, labels[train_ind])
        print('fits', a.fits, 'plan', model.dlp_plan)
        return
    measure(say, gl, _hip, ref, 'headline graph', W, train_ind, labels[train_ind], (2, 8))
    labels = load_labels(5000)
    W = gl.weightmatrix.knn(make_features(labels), 10)
    train_ind = gl.trainsets.generate(labels, rate=10, seed=0)
    measure(say, gl, _hip, ref, 'the reference\'s cap', W, train_ind, labels[train_ind], (2,), dense_T=2)
    gold = load_golden()
    Wb, truth, ind, lab, k, params = golden_case(gold, 'blobs')
    measure(say, gl, _hip, ref, 'blobs fixture', Wb, ind, lab, (2, 6), dense_T=2)
    plain = ref.random_problem(4097, 4097, 10, deg=10, exact=True)
    hub = ref.random_problem(4097, 4097, 10, deg=10, exact=True, hub=3000)
    t = [float(np.median(timed(lambda: _hip.dlp_solve(p.indptr, p.indices, p.data, i, v, T=3), min_s=0.5)[1])) for p, i, v in (plain, hub)]
    say('one row of 3 000 entries among 4 097 rows of 10, T = 3: call %.2f ms without it, %.2f ms with it -> %.0f us per pass over P' % (
        t[0], t[1], (t[1] - t[0]) / 7 * 1e3))
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
