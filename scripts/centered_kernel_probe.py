"""ssl.centered_kernel on the headline graph and on the 600-vertex `blobs` fixture: the whole fit, the device call alone, the time per
iteration, and the numpy restatement in the reference's formula order (tests/ck_ref.py: ck_reference_order, shown bit-equal to the
reference when the fixture was made) on one core of the same machine with the same start vector.

The headline graph is the 70 000-vertex k = 10, 10-class graph of bench.py's generator, 10 labels per class, defaults (tol 1e-10,
power_it 100, alpha 1.05).  Every time is end to end (uploads, host bookkeeping, downloads included), warm, over repeated runs:
median (min .. max).  Per iteration of the fixed-point loop: (call at the default tol - call with tol = 1, which runs the power
iteration and no iteration of the loop) / T.  Per step of the power iteration: (call with tol = 1 - the same with power_it = 1) / 99.
The split between the sparse pass and the finishing kernel needs a kernel trace: run this script with --fits N under a profiler in a
run of its own; it then only repeats the fit N times.

    python scripts/centered_kernel_probe.py [--out profiles/centered_kernel.txt] [--no-ref] [--fits N]"""
import argparse
import os
import sys
import time

for var in ('OMP_NUM_THREADS', 'OPENBLAS_NUM_THREADS', 'MKL_NUM_THREADS'):       # the restatement runs on one core
    os.environ[var] = '1'
import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'tests'))
ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'centered_kernel.txt'))
ap.add_argument('--no-ref', action='store_true')
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


def measure(say, gl, _hip, ref, name, W, train_ind, tl, reference_seconds=None):
    n, k = W.shape[0], len(np.unique(tl))
    model = gl.ssl.centered_kernel(W)
    np.random.seed(0)
    t0 = time.perf_counter()
    model.fit(train_ind, tl)
    first = time.perf_counter() - t0
    T, l = model.num_iter, model.eigenvalue

    def fit():
        np.random.seed(0)
        return np.array(model.fit(train_ind, tl), copy=True)
    prob, ts_fit = timed(fit, min_s=max(1.0, 3 * first))
    Wd = ref.without_diagonal(W)
    val = np.ascontiguousarray(ref.start_values(n, train_ind, tl, k)[train_ind])
    e = np.random.RandomState(0).rand(n, 1)
    args = (Wd.indptr, Wd.indices, Wd.data, train_ind, val, e)
    out, ts_call = timed(lambda: _hip.ck_solve(*args), min_s=max(1.0, 3 * first))
    assert out[0].tobytes() == prob.tobytes() and out[2] == T
    _, ts_zero = timed(lambda: _hip.ck_solve(*args, tol=1.0))
    _, ts_one = timed(lambda: _hip.ck_solve(*args, tol=1.0, power_it=1))
    per_it = (np.median(ts_call) - np.median(ts_zero)) / T * 1e3
    per_pw = (np.median(ts_zero) - np.median(ts_one)) / 99 * 1e3
    say('%s: n=%d entries=%d classes=%d labelled=%d | T=%d l=%.15g plan=%s (first fit %.0f ms)' % (name, n, Wd.nnz, k, len(train_ind), T, l,
                                                                                               model.ck_plan, first * 1e3))
    say('  fit %s | device call alone %s' % (spread(ts_fit), spread(ts_call)))
    say('  with tol = 1 (power iteration only) %s, and power_it = 1 %s -> %.2f us per iteration of the loop (two launches), %.2f us per '
        'power step' % (spread(ts_zero), spread(ts_one), per_it, per_pw))
    if not a.no_ref:
        t0 = time.perf_counter()
        u, l_ref, T_ref, errs = ref.ck_reference_order(W, train_ind, tl, k, e)
        sec = time.perf_counter() - t0
        say('  restatement in the reference\'s formula order, numpy on one core of this machine: %.2f s, T=%d (%s), largest difference to the '
            'device %.2e, l relative %.1e -> fit x %.1f' % (sec, T_ref, 'equal' if T_ref == T else 'NOT EQUAL', float(np.abs(u - prob).max()),
                                                            abs(l_ref - l) / abs(l_ref), sec * 1e3 / float(np.median(ts_fit))))
    if reference_seconds is not None:
        say('  the reference itself, recorded with the fixture ON ANOTHER MACHINE: %.3f s for one fit' % reference_seconds)
    return model


def main():
    import graphlearning_amd as gl
    from graphlearning_amd import _hip
    import ck_ref as ref
    from bench import load_labels, make_features
    from test_ck_host import load_golden, golden_case
    _hip.require_device()
    labels = load_labels(70000)
    W = gl.weightmatrix.knn(make_features(labels), 10)
    train_ind = gl.trainsets.generate(labels, rate=10, seed=0)
    tl = labels[train_ind]
    if a.fits:
        model = gl.ssl.centered_kernel(W)
        for _ in range(a.fits):
            np.random.seed(0)
            model.fit(train_ind, tl)
        print('fits', a.fits, 'T', model.num_iter)
        return
    lines = ['# ssl.centered_kernel (tol 1e-10, power_it 100, alpha 1.05) on one MI355X; times end to end, warm']

    def say(line):
        lines.append(line)
        print(line, flush=True)
    measure(say, gl, _hip, ref, 'headline graph', W, train_ind, tl)
    gold = load_golden()
    Wb, ind, lab, k, seed, e = golden_case(gold, 'blobs')
    measure(say, gl, _hip, ref, 'blobs fixture', Wb, ind, lab, reference_seconds=float(gold['case_blobs_reference_seconds']))
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
