"""ssl.plaplace on the headline graph: the batched Jacobi iteration (fast=False) beside ten single _hip.lp_iterate calls on the same
columns in the same process (the cost of the same answer before the batched kernel existed) and beside the compiled reference on one
core of the same machine; and the fast=True fit beside the compiled reference.

The graph is the 70 000-vertex k = 10, 10-class graph of the headline configuration (bench.py's generator), 10 labels per class,
p = 10.  Every time is end to end (uploads, host bookkeeping, downloads included), warm, over repeated runs: median (min .. max).
The per-iteration device time is (call with the full cap - call with T = 0) / iterations of the longest column.  Equal bits are
ASSERTED between the batched call and the single calls, and against every column the reference ran in full.

The reference is oracle/_ref/liblp_ref.so (the reference's own lp_iterate.cpp, g++ -O2 -ffp-contract=off) through ctypes on the same
__ccode_init__ arrays, class after class as the reference's one-vs-rest loop does.  --ref-classes K runs it on the first K classes and
scales by 10 / K.  When a trial run of 20 iterations predicts more than --ref-budget seconds for those K classes, the reference's
Jacobi iteration is timed over --ref-iters iterations per class instead and scaled to the class's stopping iteration (every iteration
does the same work); the output says which was done.

    python scripts/plaplace_probe.py [--out profiles/plaplace.txt] [--max-it T] [--ref-classes K] [--ref-budget S] [--no-ref]"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'plaplace.txt'))
ap.add_argument('--max-it', type=float, default=1e6)
ap.add_argument('--ref-classes', type=int, default=2)
ap.add_argument('--ref-budget', type=float, default=60.0)
ap.add_argument('--ref-iters', type=int, default=200)
ap.add_argument('--no-ref', action='store_true')
a = ap.parse_args()
P, TOL = 10, 1e-1


def timed(fn, min_s=1.0, min_n=3, max_n=15):
    out, ts = None, []
    t_begin = time.perf_counter()
    while (time.perf_counter() - t_begin < min_s or len(ts) < min_n) and len(ts) < max_n:
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


def spread(ts):
    return '%.1f ms (median of %d, %.1f .. %.1f)' % (float(np.median(ts)), len(ts), min(ts), max(ts))


def bind_reference():
    so = os.path.join(HERE, 'oracle', '_ref', 'liblp_ref.so')
    if a.no_ref or not os.path.exists(so):
        return None, None
    lib = ctypes.CDLL(so)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    lip = getattr(lib, '_Z16lip_iterate_mainPdPiS0_S_S0_S_idbiiidd')
    lip.argtypes = [dp, ip, ip, dp, ip, dp, ctypes.c_int, ctypes.c_double, ctypes.c_bool, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                    ctypes.c_double, ctypes.c_double]
    lip.restype = None
    lp = getattr(lib, '_Z15lp_iterate_mainPdS_PiS0_S_S0_S_didbiii')
    lp.argtypes = [dp, dp, ip, ip, dp, ip, dp, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_bool, ctypes.c_int, ctypes.c_int,
                   ctypes.c_int]
    lp.restype = None

    def fast(G, ind, val, T):
        u = np.zeros(G.num_nodes)
        ind = np.ascontiguousarray(ind, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        lip(u.ctypes.data_as(dp), G.J.ctypes.data_as(ip), G.I.ctypes.data_as(ip), G.V.ctypes.data_as(dp), ind.ctypes.data_as(ip),
            val.ctypes.data_as(dp), int(T), 1e-6, False, len(u), len(G.V), len(ind), 1 / (P - 1), 1 - 1 / (P - 1))
        return u

    def jacobi(G, ind, val, T):
        ind = np.ascontiguousarray(ind, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        uu = np.max(val) * np.ones(G.num_nodes)
        ul = np.min(val) * np.ones(G.num_nodes)
        uu[ind] = val
        ul[ind] = val
        lp(uu.ctypes.data_as(dp), ul.ctypes.data_as(dp), G.J.ctypes.data_as(ip), G.I.ctypes.data_as(ip), G.V.ctypes.data_as(dp),
           ind.ctypes.data_as(ip), val.ctypes.data_as(dp), float(P), int(T), TOL, False, len(uu), len(G.V), len(ind))
        return (uu + ul) / 2
    return fast, jacobi


def main():
    import graphlearning_amd as gl
    from graphlearning_amd import _hip
    from bench import load_labels, make_features
    _hip.require_device()
    ref_fast, ref_jacobi = bind_reference()
    T = int(a.max_it)
    lines = ['# ssl.plaplace (p = 10) on one MI355X; times end to end, warm; reference = the compiled lp_iterate.cpp on one core of the same '
             'machine, class after class']
    labels = load_labels(70000)
    W = gl.weightmatrix.knn(make_features(labels), 10)
    train_ind = gl.trainsets.generate(labels, rate=10, seed=0)
    tl = labels[train_ind]
    G = gl.graph(W)
    G.__ccode_init__()
    classes = np.unique(tl)
    C = len(classes)
    vals = (tl[:, None] == classes[None, :]).astype(np.float64)
    ind32 = np.ascontiguousarray(train_ind, dtype=np.int32)
    lines.append('headline graph: n=%d entries=%d classes=%d labelled=%d max_num_it=%d' % (W.shape[0], W.nnz, C, len(train_ind), T))

    def say(line):
        lines.append(line)
        print(line, flush=True)

    # ---- fast=False: the Jacobi iteration, tol 1e-1 ----
    model = gl.ssl.plaplace(G, p=P, max_num_it=T, tol=TOL, fast=False)
    t0 = time.perf_counter()
    model.fit(train_ind, tl)                              # warm-up: entry arrays, code objects, pools
    first = time.perf_counter() - t0
    stops = list(model.num_iter)
    say('fast=False tol=1e-1: stopping iteration per class %s%s (first fit %.0f ms)' % (stops, ' (the cap: not converged)' if max(stops) >= T else '',
                                                                                     first * 1e3))
    prob, ts_fit = timed(lambda: np.array(model.fit(train_ind, tl), copy=True), min_s=max(1.0, 3 * first))
    _, ts_call = timed(lambda: _hip.lp_iterate_batch(G.num_nodes, G.J, G.I, G.V, ind32, vals, P, T, TOL), min_s=max(1.0, 3 * first))
    _, ts_zero = timed(lambda: _hip.lp_iterate_batch(G.num_nodes, G.J, G.I, G.V, ind32, vals, P, 0, TOL))
    per_it = (np.median(ts_call) - np.median(ts_zero)) / max(1, min(T, max(stops) + 1)) * 1e3
    say('  batched fit (one call, %d columns): %s | device call alone %s, with T=0 %s -> %.1f us per iteration' % (
        C, spread(ts_fit), spread(ts_call), spread(ts_zero), per_it))

    def singles():
        cols, its = [], []
        for c in range(C):
            val = np.ascontiguousarray(vals[:, c])
            uu = np.max(val) * np.ones(G.num_nodes)
            ul = np.min(val) * np.ones(G.num_nodes)
            uu[train_ind] = val
            ul[train_ind] = val
            its.append(_hip.lp_iterate(uu, ul, G.J, G.I, G.V, ind32, val, P, T, TOL))
            cols.append((uu + ul) / 2)
        return np.stack(cols, axis=1), its
    singles()
    (sp, sits), ts_single = timed(singles, min_s=max(1.0, 3 * first))
    assert sp.tobytes() == prob.tobytes() and sits == stops, 'the batched call differs from the single calls'
    ratio = float(np.median(ts_single) / np.median(ts_fit))
    say('  ten single _hip.lp_iterate calls, summed: %s | bits and stops equal | batched fit is x %.2f faster (slowest batched %.1f ms against '
        'fastest singles %.1f ms)' % (spread(ts_single), ratio, max(ts_fit), min(ts_single)))
    if ref_jacobi is not None:
        K = max(1, min(a.ref_classes, C))
        t0 = time.perf_counter()
        for c in range(K):
            ref_jacobi(G, train_ind, vals[:, c], 20)
        per = (time.perf_counter() - t0) / (20 * K)
        predicted = per * sum(min(s + 1, T) for s in stops[:K])
        if predicted <= a.ref_budget:
            t0 = time.perf_counter()
            cols = [ref_jacobi(G, train_ind, vals[:, c], T) for c in range(K)]
            t_ref = (time.perf_counter() - t0) * 1e3
            assert all(cols[c].tobytes() == np.ascontiguousarray(prob[:, c]).tobytes() for c in range(K)), 'device != compiled reference'
            how = '%d class%s run in full (bits equal), %.0f ms' % (K, '' if K == 1 else 'es', t_ref)
            total = t_ref * C / K
        else:
            n_it = a.ref_iters
            t0 = time.perf_counter()
            for c in range(K):
                ref_jacobi(G, train_ind, vals[:, c], n_it)
            per = (time.perf_counter() - t0) / (n_it * K)
            total = per * sum(min(s + 1, T) for s in stops) * 1e3
            how = '%d class%s timed over %d iterations each (%.2f ms per iteration; a full run was predicted at %.0f s), scaled to the stopping iterations' % (
                K, '' if K == 1 else 'es', n_it, per * 1e3, predicted)
        say('  compiled reference, one core: %s -> %.0f ms for %d classes = batched fit x %.1f' % (how, total, C, total / float(np.median(ts_fit))))

    # ---- fast=True: the in-order sweeps by levels, tol 1e-6 ----
    model = gl.ssl.plaplace(G, p=P, max_num_it=T, fast=True)
    model.fit(train_ind, tl)
    prob, ts = timed(lambda: np.array(model.fit(train_ind, tl), copy=True))
    plan = G.plaplace_plan
    line = 'fast=True (tol 1e-6): fit %s | levels %d, launches per sweep %d, launches in all %d | sweeps per class %s' % (
        spread(ts), plan[0], plan[1], plan[2], model.num_iter)
    if ref_fast is not None:
        t0 = time.perf_counter()
        cols = [ref_fast(G, train_ind, vals[:, c], T) for c in range(C)]
        t_ref = (time.perf_counter() - t0) * 1e3
        assert all(cols[c].tobytes() == np.ascontiguousarray(prob[:, c]).tobytes() for c in range(C)), 'device != compiled reference'
        line += ' | reference %d classes %.0f ms = device x %.2f | bits equal' % (C, t_ref, t_ref / float(np.median(ts)))
    say(line)

    # ---- a small graph: the golden blobs3 cases ----
    sys.path.insert(0, os.path.join(HERE, 'tests'))
    import plaplace_ref as pref
    gold = pref.load_golden()
    Wg = pref.golden_graph(gold, 'blobs3')
    Gg = gl.graph(Wg)
    Gg.__ccode_init__()
    ti = gold['graph_blobs3_train_ind']
    tlg = gold['graph_blobs3_labels'][ti]
    vg = pref.class_columns(tlg)
    for fast in (False, True):
        m = gl.ssl.plaplace(Gg, p=P, tol=TOL, fast=fast)
        m.fit(ti, tlg)
        _, ts = timed(lambda: m.fit(ti, tlg))
        line = 'blobs3 n=%d fast=%s: fit %s | iterations %s' % (Wg.shape[0], fast, spread(ts), m.num_iter)
        fn = ref_fast if fast else ref_jacobi
        if fn is not None:
            t0 = time.perf_counter()
            for c in range(vg.shape[1]):
                fn(Gg, ti, vg[:, c], 10 ** 6)
            line += ' | reference %.1f ms' % ((time.perf_counter() - t0) * 1e3)
        say(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
