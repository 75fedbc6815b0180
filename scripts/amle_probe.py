"""ssl.amle on the headline graph beside the compiled reference on one core of the same machine, and the measurement behind the
"small level" constant of the level plan (csrc/lip_plan.h LIP_SMALL).

Part 1: the 70 000-vertex k = 10, 10-class graph of the headline configuration (bench.py's generator), 10 labels per class,
ssl.amle with weighted=False and weighted=True at the learner's default tol 1e-3: all classes as the columns of one device call,
warm, median of the repeats, end to end (uploads, plan, downloads included).  The reference is oracle/_ref/liblp_ref.so (the
reference's own lp_iterate.cpp, g++ -O2 -ffp-contract=off) through ctypes on the same __ccode_init__ arrays, one class after
another as the reference's one-vs-rest loop does; equal bits are ASSERTED for every class the reference ran.  --ref-classes K runs
the reference's WEIGHTED solver on the first K classes only (it takes minutes for ten) and scales its time by 10 / K in the ratio.

Part 2: the sorted-plane and path goldens (hundreds of levels of a few vertices) and the blobs golden with several values of the
constant through the plan override for measurements, `small_level` of graph._amle_batch (0: every level a launch of its own).

    python scripts/amle_probe.py [--out profiles/amle.txt] [--ref-classes K] [--no-ref]"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'tests'))
ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'amle.txt'))
ap.add_argument('--ref-classes', type=int, default=10)
ap.add_argument('--no-ref', action='store_true')
a = ap.parse_args()


def timed(fn, min_s=1.0, min_n=3, max_n=25):
    out, ts = None, []
    t_begin = time.perf_counter()
    while (time.perf_counter() - t_begin < min_s or len(ts) < min_n) and len(ts) < max_n:
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


def bind_reference():
    so = os.path.join(HERE, 'oracle', '_ref', 'liblp_ref.so')
    if a.no_ref or not os.path.exists(so):
        return None
    lib = ctypes.CDLL(so)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    plain = getattr(lib, '_Z16lip_iterate_mainPdPiS0_S_S0_S_idbiiidd')
    plain.argtypes = [dp, ip, ip, dp, ip, dp, ctypes.c_int, ctypes.c_double, ctypes.c_bool, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                      ctypes.c_double, ctypes.c_double]
    plain.restype = None
    wfn = getattr(lib, '_Z25lip_iterate_weighted_mainPdPiS0_S_S0_S_idbiii')
    wfn.argtypes = plain.argtypes[:12]
    wfn.restype = None

    def run(G, ind, val, weighted, T, tol):
        u = np.zeros(G.num_nodes)
        ind = np.ascontiguousarray(ind, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        args = [u.ctypes.data_as(dp), G.J.ctypes.data_as(ip), G.I.ctypes.data_as(ip), G.V.ctypes.data_as(dp), ind.ctypes.data_as(ip),
                val.ctypes.data_as(dp), int(T), float(tol), False, len(u), len(G.V), len(ind)]
        if weighted:
            wfn(*args)
        else:
            plain(*(args + [0.0, 1.0]))
        return u
    return run


def main():
    import graphlearning_amd as gl
    from graphlearning_amd import _hip
    from bench import load_labels, make_features
    from test_amle_host import load_golden, golden_graph, golden_case
    _hip.require_device()
    ref_run = bind_reference()
    lines = ['# ssl.amle / graph.amle on one MI355X; ms = end to end, median of the warm repeats (min .. max); reference = the compiled '
             'lp_iterate.cpp on one core of the same machine, class after class']
    labels = load_labels(70000)
    W = gl.weightmatrix.knn(make_features(labels), 10)
    train_ind = gl.trainsets.generate(labels, rate=10, seed=0)
    G = gl.graph(W)
    G.__ccode_init__()
    classes = np.unique(labels[train_ind])
    lines.append('headline graph: n=%d entries=%d classes=%d labelled=%d' % (W.shape[0], W.nnz, len(classes), len(train_ind)))
    for weighted in (False, True):
        model = gl.ssl.amle(G, weighted=weighted)
        model.fit(train_ind, labels[train_ind])                     # warm-up: entry arrays, code objects, pools
        prob, ts = timed(lambda: np.array(model.fit(train_ind, labels[train_ind]), copy=True))
        med = float(np.median(ts))
        plan = G.amle_plan
        line = 'weighted=%d tol=1e-3: device %9.1f ms (median of %d, %.1f .. %.1f) | levels %d, launches per sweep %d, launches in all %d | sweeps per class %s' % (
            weighted, med, len(ts), min(ts), max(ts), plan[0], plan[1], plan[2], model.num_iter)
        if ref_run is not None:
            K = max(1, min(a.ref_classes, len(classes))) if weighted else len(classes)
            t0 = time.perf_counter()
            cols = [ref_run(G, train_ind, labels[train_ind] == c, weighted, 100000, 1e-3) for c in classes[:K]]
            t_ref = (time.perf_counter() - t0) * 1e3
            same = all(cols[i].tobytes() == np.ascontiguousarray(prob[:, i]).tobytes() for i in range(K))
            assert same, 'the device result differs from the compiled reference'
            line += ' | reference %d class%s %.0f ms -> %.0f ms for %d = device x %.1f | bits equal' % (
                K, '' if K == 1 else 'es', t_ref, t_ref * len(classes) / K, len(classes), t_ref * len(classes) / K / med)
        lines.append(line)
        print(line, flush=True)
        vals = (labels[train_ind][:, None] == classes[None, :]).astype(np.float64)
        for small in (0, 8, 32, 128, 512):
            run = lambda: G._amle_batch(train_ind, vals, tol=1e-3, max_num_it=1e5, weighted=weighted, small_level=small)
            assert run().tobytes() == prob.tobytes()
            _, ts = timed(run, min_s=0.5)
            lines.append('    small=%-5d %9.1f ms (median of %d) | launches per sweep %d' % (small, float(np.median(ts)), len(ts), G.amle_plan[1]))
            print(lines[-1], flush=True)

    gold = load_golden()
    for name in ('sorted_u', 'sorted_w', 'path_u', 'path_w', 'blobs_u_3', 'blobs_w_3'):
        gname, ind, vals, weighted, tol, T, alpha, beta, U, sweeps, errs = golden_case(gold, name)
        Gg = gl.graph(golden_graph(gold, gname))
        out = []
        for small in (0, 8, 32, 128, 512):
            Gg._amle_batch(ind, vals, tol=tol, max_num_it=T, weighted=weighted, small_level=small)
            u, ts = timed(lambda: Gg._amle_batch(ind, vals, tol=tol, max_num_it=T, weighted=weighted, small_level=small), min_s=0.4)
            assert u.tobytes() == U.tobytes(), (name, small)
            out.append('small=%d: %.1f ms (%d launches per sweep)' % (small, float(np.median(ts)), Gg.amle_plan[1]))
        t_ref = ''
        if ref_run is not None:
            t0 = time.perf_counter()
            for b in range(vals.shape[1]):
                ref_run(Gg, ind, vals[:, b], weighted, T, tol)
            t_ref = ' | reference %.1f ms' % ((time.perf_counter() - t0) * 1e3)
        lines.append('%-10s n=%d levels=%d columns=%d sweeps=%s | %s%s' % (name, Gg.num_nodes, Gg.amle_levels, vals.shape[1], sweeps.tolist(),
                                                                        ', '.join(out), t_ref))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
