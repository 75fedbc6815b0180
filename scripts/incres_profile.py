"""clustering.incres on the 70 000-vertex `connected` graph of profiles/eig.txt (bench.py's generator at scale = 0.8: one component) with
10 clusters at the defaults, and on the 600-vertex `blobs` fixture with 3, against the numpy restatement of the reference's loop
(tests/incres_ref.py) on one core of the same machine from the same seed: the fit end to end, the time inside the device calls and
the host's share (the draws), sweeps counted and sweeps wasted behind the stop, chunks read.  Every time is warm, median (min .. max).
The split of the device time into plant, sweeps and census needs a kernel trace: run this script with --trace under a profiler in a
run of its own; it then only fits once on the large graph.

    python scripts/incres_profile.py [--out profiles/incres.txt] [--trace] [--baseline-T T]"""
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
ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'incres.txt'))
ap.add_argument('--trace', action='store_true')
ap.add_argument('--baseline-T', type=int, default=200, help='outer iterations of the numpy baseline on the large graph (the device runs the same)')
a = ap.parse_args()


def spread(ts):
    return '%.2f ms (median of %d, %.2f .. %.2f)' % (float(np.median(ts)), len(ts), min(ts), max(ts))


def usable_seed(gl, W, k, T):
    """the first seed whose fit keeps every cluster alive (an empty cluster is numpy's ValueError, in the reference too)"""
    for seed in range(20):
        np.random.seed(seed)
        try:
            gl.clustering.incres(W, k, T=T).fit()
            return seed
        except ValueError:
            continue
    raise SystemExit('no usable seed')


def schedules(say, gl, W, k, T, seed):
    """the same fit under other schedules (first chunk = the count before + margin, then `next` sweeps, doubling): same labels, other cost"""
    from graphlearning_amd import _hip
    base = None
    for margin, nxt in ((None, None), (1, 2), (1, 8), (2, 4), (4, 4), (6, 8)):
        ts = []
        with _hip.incres_options(margin=margin, next=nxt):
            for _ in range(3):
                np.random.seed(seed)
                model = gl.clustering.incres(W, k, T=T)
                t0 = time.perf_counter()
                got = model.fit()
                ts.append((time.perf_counter() - t0) * 1e3)
        base = got if base is None else base
        plan = model.incres_plan
        say('    margin %s next %s: fit %s, %d chunks read, %d sweeps enqueued for %d counted, labels that differ %d'
            % (margin or 'default', nxt or 'default', spread(ts), plan['chunks'], plan['enqueued'], plan['counted'], int((got != base).sum())))


def case(say, gl, ref, W, k, what, T, repeats):
    from graphlearning_amd import _hip
    n = W.shape[0]
    seed = usable_seed(gl, W, k, T)
    inside = []
    real_step = _hip.Incres.step

    def timed_step(self, *args, **kw):
        t0 = time.perf_counter()
        try:
            return real_step(self, *args, **kw)
        finally:
            inside[-1] += time.perf_counter() - t0
    _hip.Incres.step = timed_step
    ts, model = [], None
    try:
        for _ in range(repeats):
            np.random.seed(seed)
            model = gl.clustering.incres(W, k, T=T)
            inside.append(0.0)
            t0 = time.perf_counter()
            model.fit()
            ts.append((time.perf_counter() - t0) * 1e3)
    finally:
        _hip.Incres.step = real_step
    plan = model.incres_plan
    sweeps = np.array(model.grow_sweeps)
    dev_ms = [v * 1e3 for v in inside]
    say('%s: n=%d entries=%d clusters=%d T=%d seed=%d, sweeps per outer iteration %d .. %d (%d in all), %d lanes per record of %d doubles, '
        'renumbered %d' % (what, n, W.nnz, k, T, seed, sweeps.min(), sweeps.max(), sweeps.sum(), plan['lanes'], plan['record'], plan['renumbered']))
    say('  fit end to end: %s; inside the %d device calls: %s -> %.1f us per outer iteration, %.1f us per counted sweep; the rest (P, the '
        'draws, the handle): %.2f ms' % (spread(ts), T, spread(dev_ms), float(np.median(dev_ms)) * 1e3 / T,
                                         float(np.median(dev_ms)) * 1e3 / max(int(sweeps.sum()), 1), float(np.median(ts)) - float(np.median(dev_ms))))
    say('  schedule: %d chunks read, %d sweeps enqueued, %d counted -> %d wasted behind the stop (%.0f %%)'
        % (plan['chunks'], plan['enqueued'], plan['counted'], plan['enqueued'] - plan['counted'],
           100.0 * (plan['enqueued'] - plan['counted']) / max(plan['enqueued'], 1)))
    say('  other schedules (the library\'s: first guess %d, margin %d, second chunk %d, doubling):' % (plan['first_chunk'], plan['margin'], plan['next_chunk']))
    schedules(say, gl, W, k, T, seed)
    Tb = min(T, a.baseline_T)
    np.random.seed(seed)
    t0 = time.perf_counter()
    hist, counts, _ = ref.fit(W, k, T=Tb)
    sec = time.perf_counter() - t0
    np.random.seed(seed)
    t0 = time.perf_counter()
    short = gl.clustering.incres(W, k, T=Tb)
    got = short.fit()
    dev_sec = time.perf_counter() - t0
    say('  numpy restatement on one core of this machine, same seed, T=%d: %.1f ms against %.1f ms on the device, labels that differ %d of %d, '
        'sweep counts equal: %s -> x %.1f%s' % (Tb, sec * 1e3, dev_sec * 1e3, int((hist[-1] != got).sum()), n,
                                                bool(np.array_equal(counts, short.grow_sweeps)), sec / dev_sec,
                                                '' if sec > dev_sec else ' (SLOWER than the CPU)'))


def main():
    import graphlearning_amd as gl
    from graphlearning_amd import _hip
    import incres_ref as ref
    from bench import load_labels, make_features
    _hip.require_device()
    labels = load_labels(70000)
    W = gl.weightmatrix.knn(make_features(labels, scale=0.8), 10)
    if a.trace:
        np.random.seed(usable_seed(gl, W, 10, 200))
        model = gl.clustering.incres(W, 10)
        model.fit()
        print('traced one fit', sum(model.grow_sweeps), 'sweeps counted', model.incres_plan, flush=True)
        return
    lines = ['# clustering.incres on one MI355X; times end to end, warm']

    def say(line):
        lines.append(line)
        print(line, flush=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    gold = ref.load_golden()
    case(say, gl, ref, ref.golden_graph(gold, 'blobs'), 3, 'blobs fixture', 200, 7)
    case(say, gl, ref, W, 10, '70 000-vertex graph (scale 0.8)', 200, 3)


if __name__ == '__main__':
    main()
