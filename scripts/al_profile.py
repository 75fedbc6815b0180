"""graphlearning_amd.active_learning on the 70 000-vertex `connected` graph of profiles/eig.txt (bench.py's generator at scale = 0.8: 10
classes, one component) with M = 50 eigenpairs, and on the 600-vertex `blobs` fixture: one compute per criterion over all unlabelled
vertices, one update, select_greedy(100), and a ten-round var_opt loop end to end with the share that is ssl.laplace's fit -- against
the reference's formulas (active_learning.py:296-317) in numpy on one core of the same machine, its Python loop of one np.inner per
candidate included, with the same eigenpairs.  Every time is end to end, warm, median (min .. max).

    python scripts/al_profile.py [--out profiles/active_learning.txt]"""
import argparse
import os
import sys
import time

for var in ('OMP_NUM_THREADS', 'OPENBLAS_NUM_THREADS', 'MKL_NUM_THREADS'):       # the numpy formulas run on one core
    os.environ[var] = '1'
import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'tests'))
ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'active_learning.txt'))
a = ap.parse_args()
GAMMA2 = 0.1 ** 2.
NAMES = ('var_opt', 'sigma_opt', 'model_change', 'model_change_var_opt')


def timed(fn, min_s=0.5, min_n=3, max_n=9):
    out, ts = None, []
    t_begin = time.perf_counter()
    while (time.perf_counter() - t_begin < min_s or len(ts) < min_n) and len(ts) < max_n:
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


def spread(ts):
    return '%.2f ms (median of %d, %.2f .. %.2f)' % (float(np.median(ts)), len(ts), min(ts), max(ts))


def ratio(cpu_ms, dev_ms):
    return 'x %.1f' % (cpu_ms / dev_ms) if cpu_ms >= dev_ms else '**x %.2f: SLOWER than the CPU**' % (cpu_ms / dev_ms)


def numpy_compute(kind, C, V, cand, unc):
    """the reference's truncated formulas, its loop of np.inner included"""
    Cavk = C @ V[cand, :].T
    diag = GAMMA2 + np.array([np.inner(V[k, :], Cavk[:, i]) for i, k in enumerate(cand)])
    if kind == 1:
        return np.sum(Cavk, axis=0) ** 2. / diag
    norms = np.linalg.norm(Cavk, axis=0)
    if kind == 0:
        return norms ** 2. / diag
    return unc * (norms if kind == 2 else norms ** 2.) / diag


def numpy_update(C, V, query):
    for k in query:
        vk = V[k]
        Cavk = C @ vk
        C -= np.outer(Cavk, Cavk) / (GAMMA2 + np.inner(vk, Cavk))


def case(say, gl, W, truth, what, greedy_cpu_rounds):
    from graphlearning_amd import _hip
    al = gl.active_learning
    n, k = W.shape[0], len(np.unique(truth))
    model = gl.ssl.laplace(W)
    vals, V = model.graph.eigen_decomp(normalization='normalized', k=50)
    V = np.ascontiguousarray(V)
    C0 = np.diag(1. / (vals + 1e-11))
    rng = np.random.default_rng(0)
    ind = np.array([rng.choice(np.where(truth == c)[0]) for c in range(k)])
    cand = np.setdiff1d(np.arange(n), ind)
    unc = rng.random(len(cand))
    h = _hip.Acq(V, C0, GAMMA2)
    h.update(ind)
    C = h.get_c()
    say('%s: n=%d entries=%d classes=%d, M=50, C = diag(1 / (evals + 1e-11)) after the first %d labels, %d candidates, plan %s'
        % (what, n, W.nnz, k, len(ind), len(cand), h.stats()))
    for kind, name in enumerate(NAMES):
        dev, ts = timed(lambda: h.compute(kind, cand, unc))
        t0 = time.perf_counter()
        cpu = numpy_compute(kind, C, V, cand, unc)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        say('  compute %-21s device call (uploads of candidates%s, one launch, download): %s; numpy on one core %.1f ms -> %s; values differ by '
            '%.2g of the largest' % (name, ' and unc' if kind >= 2 else '', spread(ts), cpu_ms, ratio(cpu_ms, float(np.median(ts))),
                                      float(np.abs(dev - cpu).max() / np.abs(cpu).max())))
    _, ts = timed(lambda: h.update(cand[:1]))
    Cc = C.copy()
    _, ts_cpu = timed(lambda: numpy_update(Cc, V, cand[:1]))
    say('  update of one query (one launch): %s; numpy %s -> %s' % (spread(ts), spread(ts_cpu), ratio(float(np.median(ts_cpu)), float(np.median(ts)))))
    _, ts = timed(lambda: h.update(cand[:100]))
    say('  update of a batch of 100 (one launch): %s' % spread(ts))
    h.close()
    h = _hip.Acq(V, C, GAMMA2)
    (q, qv), ts = timed(lambda: h.greedy(0, cand, 100), max_n=5)
    Cc, left, picks = C.copy(), cand.copy(), []
    t0 = time.perf_counter()
    for _ in range(greedy_cpu_rounds):
        v = numpy_compute(0, Cc, V, left, None)
        p = int(np.argmax(v))
        picks.append(int(left[p]))
        numpy_update(Cc, V, left[p:p + 1])
        left = np.delete(left, p)
    cpu_ms = (time.perf_counter() - t0) * 1e3 * 100 / greedy_cpu_rounds
    say('  greedy design of 100 var_opt queries (200 launches, nothing read back in between): %s; numpy rounds of compute / argmax / update: '
        '%.0f ms (%d rounds timed, scaled to 100) -> %s; the first %d queries equal: %s'
        % (spread(ts), cpu_ms, greedy_cpu_rounds, ratio(cpu_ms, float(np.median(ts))), greedy_cpu_rounds, cand[q[:greedy_cpu_rounds]].tolist() == picks))
    h.close()
    # the loop end to end
    fit_s = [0.0]
    fit = model.fit

    def timed_fit(*args, **kw):
        t0 = time.perf_counter()
        out = fit(*args, **kw)
        fit_s[0] += time.perf_counter() - t0
        return out
    model.fit = timed_fit

    def loop():
        AL = al.active_learner(model, al.var_opt, ind, truth[ind], C=C0, V=V)
        fit_s[0] = 0.0
        t0 = time.perf_counter()
        for _ in range(10):
            query = AL.select_queries()
            AL.update(query, truth[query])
        total = time.perf_counter() - t0
        AL.acq_function.close()
        return total * 1e3, fit_s[0] * 1e3
    loop()
    runs = [loop() for _ in range(3)]
    total, fits = float(np.median([r[0] for r in runs])), float(np.median([r[1] for r in runs]))
    say('  ten rounds of select_queries / update with var_opt and ssl.laplace, end to end: %.1f ms, of which ssl.laplace\'s ten fits %.1f ms '
        '(%.0f %%); the rest -- candidates by setdiff1d, compute, argsort, update -- %.1f ms' % (total, fits, 100 * fits / total, total - fits))


def main():
    import graphlearning_amd as gl
    from graphlearning_amd import _hip
    import eig_ref
    from bench import load_labels, make_features
    _hip.require_device()
    lines = ['# graphlearning_amd.active_learning on one MI355X; times end to end, warm']

    def say(line):
        lines.append(line)
        print(line, flush=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    gold = eig_ref.load_golden()
    case(say, gl, eig_ref.golden_graph(gold, 'blobs'), gold['graph_blobs_truth'], 'blobs fixture', 100)
    labels = load_labels(70000)
    W = gl.weightmatrix.knn(make_features(labels, scale=0.8), 10)
    case(say, gl, W, labels, '70 000-vertex graph (scale 0.8)', 5)


if __name__ == '__main__':
    main()
