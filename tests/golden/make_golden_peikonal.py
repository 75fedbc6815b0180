#!/usr/bin/env python3
"""Generate the p-eikonal fixture tests/golden/g26_peikonal.npz from THE COMPILED REFERENCE.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONPATH=<the reference's checkout> PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg \
        python3 tests/golden/make_golden_peikonal.py        (from the repository root)

Like make_golden_dijkstra.py the generator compiles the two source files behind the reference's solvers (c_code/hjsolvers.cpp,
c_code/memory_allocation.cpp) where they lie into a temporary directory OUTSIDE the repository (g++ -O2 -ffp-contract=off -fPIC
-shared) and binds peikonal_fmm_main through ctypes as the module `graphlearning.cextensions`, so that the reference's
own graph.peikonal and ssl.peikonal run unchanged on the arrays its __ccode_init__ builds.  Nothing compiled is kept.

The file holds data only.  Graphs: `blobs` and `moons` are read from g18_ck.npz / g19_eig.npz and not stored again; stored here are a
7-vertex unit path, a 6 x 6 integer grid (ties), `directed` (a symmetric pattern with unsymmetric weights), `twocomp` (a second
component no boundary reaches), `star` (a hub with 300 neighbours) and `loops` (stored self loops).  Every stored graph has an entry in
every row (the reference's row pointers are wrong otherwise) and a symmetric PATTERN: the reference's marching pass solves a vertex
again only when a vertex that LISTS it leaves the heap, so on an unsymmetric pattern its result depends on that schedule and is not the
fixed point (printed below for one such graph, not stored).
Cases: p in {1, 2, 1.5, 0.5}, num_bisection_it in {30, 60}, f a scalar or a random positive vector with exact zeros, non-zero boundary
values, nl_bdy=True, an explicit u0; per case the inputs, the reference's u and the rounds of the restatement.  Learner: ssl.peikonal on
`blobs` (3 classes, 5 labels each) and `moons` (2 classes) with p = 1 and p = 2, with and without class priors, with D, with
eps_ball_graph=True: prob and predict().

Asserted before anything is written, with the restatement = csrc/peik_plan.h compiled for the host (tests/peik_plan_host.cpp):
  p == 1, f > 0 everywhere: restatement == reference bit for bit on every vertex of every case and every learner fit (`exact`);
  p == 1, f with exact zeros: NOT equal, and it cannot be.  Where f_j = 0 the solve returns fl(fl(u_k w_k) / w_k), which rounding can
    put one unit in the last place BELOW the neighbour u_k it was solved from; the marching pass never solves a finalised vertex again
    and stops there, the rounds go on to the fixed point, a few units lower on the vertices behind (with the zeros replaced by a
    positive number the same cases are equal bit for bit).  These cases are kept and held to a recorded delta like p != 1;
  p != 1: delta = the largest |restatement - reference| / max |reference| per (p, num_bisection_it) class is recorded, bound = 16 delta;
  p != 1 learner fits: every vertex's gap between its two smallest class scores exceeds 1000 bound max |u| (else another label seed)."""
import ctypes
import os
import subprocess
import sys
import tempfile
import types
import numpy as np
from scipy import sparse

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import graphlearning as gl                      # the REFERENCE
import peik_ref as ref

assert 'graphlearning_amd' not in gl.__file__, gl.__file__
REF_ROOT = os.path.dirname(os.path.dirname(gl.__file__))
LIMIT = 1000000      # bytes


def compile_reference(tmp):
    assert not os.path.abspath(tmp).startswith(os.path.dirname(os.path.dirname(HERE))), tmp
    so = os.path.join(tmp, 'hjsolvers.so')
    src = [os.path.join(REF_ROOT, 'c_code', f) for f in ('hjsolvers.cpp', 'memory_allocation.cpp')]
    subprocess.run(['g++', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-o', so] + src, check=True)
    syms = subprocess.run(['nm', '-D', so], check=True, capture_output=True, text=True).stdout.split()
    fmm = [s for s in syms if 'peikonal_fmm_main' in s]
    assert len(fmm) == 1, fmm
    lib = ctypes.CDLL(so)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    fn = getattr(lib, fmm[0])
    # (u, WI, K, WV, I, f, g, p_val, num_bisection_it, n, M, k): hjsolvers.cpp:342
    fn.argtypes = [dp, ip, ip, dp, ip, dp, dp, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    fn.restype = None

    def peikonal_fmm(u, WI, K, WV, I, f, g, p, num_bisection_it):
        for a, dt in ((u, np.float64), (WI, np.int32), (K, np.int32), (WV, np.float64), (I, np.int32), (f, np.float64), (g, np.float64)):
            assert isinstance(a, np.ndarray) and a.dtype == dt and a.flags['C_CONTIGUOUS'], (a.dtype, dt)
        assert len(K) == len(u) + 1, 'a vertex without an entry: the reference\'s row pointers are wrong'
        fn(u.ctypes.data_as(dp), WI.ctypes.data_as(ip), K.ctypes.data_as(ip), WV.ctypes.data_as(dp), I.ctypes.data_as(ip),
           f.ctypes.data_as(dp), g.ctypes.data_as(dp), float(p), int(num_bisection_it), len(u), len(WI), len(I))
    mod = types.ModuleType('graphlearning.cextensions')
    mod.peikonal_fmm = peikonal_fmm
    sys.modules['graphlearning.cextensions'] = mod
    gl.cextensions = mod


def sym_pattern(n, pairs, rng, unsym=False, unit=False):
    rows, cols, vals = [], [], []
    for i, j in pairs:
        a = 1.0 if unit else float(rng.uniform(0.5, 1.5))
        b = float(rng.uniform(0.5, 1.5)) if unsym else a
        rows += [i, j]
        cols += [j, i]
        vals += [a, b]
    W = sparse.csr_matrix((vals, (rows, cols)), shape=(n, n))
    W.sort_indices()
    return W


def small_graphs():
    rng = np.random.default_rng(26)
    out = {}
    out['path'] = sym_pattern(7, [(i, i + 1) for i in range(6)], rng, unit=True)
    grid = [(6 * r + c, 6 * r + c + 1) for r in range(6) for c in range(5)] + [(6 * r + c, 6 * r + c + 6) for r in range(5) for c in range(6)]
    out['grid'] = sym_pattern(36, grid, rng, unit=True)
    out['directed'] = sym_pattern(40, [(i, (i + 1) % 40) for i in range(40)] + [(i, (i + 7) % 40) for i in range(40)], rng, unsym=True)
    two = [(i, (i + 1) % 12) for i in range(12)] + [(i, (i + 3) % 12) for i in range(12)] + [(12 + i, 12 + (i + 1) % 5) for i in range(5)]
    out['twocomp'] = sym_pattern(17, two, rng)
    star = [(0, i) for i in range(1, 301)] + [(i, i + 1) for i in range(1, 300)]
    out['star'] = sym_pattern(301, star, rng)
    loops = [(4 * r + c, 4 * r + c + 1) for r in range(4) for c in range(3)] + [(4 * r + c, 4 * r + c + 4) for r in range(3) for c in range(4)]
    L = sym_pattern(16, loops, rng).tolil()
    for i in (0, 5, 6, 15):
        L[i, i] = float(rng.uniform(0.5, 1.5))
    out['loops'] = sparse.csr_matrix(L)
    out['loops'].sort_indices()
    return out


def case_inputs(W, gname, seed, fkind):
    n = W.shape[0]
    rng = np.random.default_rng(seed)
    if gname == 'path':
        bdy = np.array([0, 6])
    elif gname == 'twocomp':
        bdy = np.sort(rng.choice(12, size=2, replace=False))
    else:
        bdy = np.sort(rng.choice(n, size=min(5, max(2, n // 8)), replace=False))
    g = np.round(rng.uniform(0.1, 1.0, size=len(bdy)), 3)
    if fkind == 'scalar':
        f = np.float64(1.0 if seed % 2 == 0 else 0.5)
    else:
        f = rng.uniform(0.2, 2.0, size=n)
        if fkind == 'vector':                    # 'positive': the same draw without the zeros
            f[rng.choice(n, size=max(1, n // 10), replace=False)] = 0.0
    return bdy.astype(np.int32), g, f


def main():
    tmp = tempfile.mkdtemp(prefix='glx_peikonal_ref_')
    compile_reference(tmp)
    lib = ref.build_host_lib(tmp)
    gold = ref.load_golden()
    for k in [k for k in gold if not k.startswith('graph_')]:
        del gold[k]
    out = {}
    for gname, W in small_graphs().items():
        assert np.diff(W.indptr).min() >= 1 and W.data.min() > 0 and (abs((W != 0) - (W != 0).T)).nnz == 0, gname
        out['graph_%s_indptr' % gname] = W.indptr.astype(np.int32)
        out['graph_%s_indices' % gname] = W.indices.astype(np.int32)
        out['graph_%s_data' % gname] = W.data.astype(np.float64)
        gold.update({k: v for k, v in out.items() if k.startswith('graph_%s_' % gname)})
    graphs = {g: ref.graph(gold, g) for g in ('blobs', 'moons', 'path', 'grid', 'directed', 'twocomp', 'star', 'loops')}
    for gname, W in graphs.items():
        print('graph %-9s n=%d entries=%d degrees %d..%d symmetric=%s diagonal=%d' % (gname, W.shape[0], W.nnz, np.diff(W.indptr).min(),
              np.diff(W.indptr).max(), (abs(W - W.T) > 0).nnz == 0, int((W.diagonal() != 0).sum())))

    # name -> (graph, p, nbis, f kind, seed, nl_bdy, explicit u0)
    cases = {}
    seed = 100
    for gname in graphs:
        for p in (1, 2, 1.5, 0.5):
            seed += 1
            cases['%s_p%g' % (gname, p)] = (gname, p, 30, 'scalar', seed, False, False)
    for gname in ('blobs', 'moons', 'grid'):
        for p in (1, 2, 1.5, 0.5):
            seed += 1
            cases['%s_p%g_fvec60' % (gname, p)] = (gname, p, 60, 'vector', seed, False, False)
    for gname in ('blobs', 'moons', 'grid', 'star'):
        seed += 1
        cases['%s_p1_fpos' % gname] = (gname, 1, 30, 'positive', seed, False, False)
    for p in (1, 2):
        seed += 1
        cases['blobs_p%g_nonlocal' % p] = ('blobs', p, 30, 'positive' if p == 1 else 'vector', seed, True, False)
        seed += 1
        cases['twocomp_p%g_start' % p] = ('twocomp', p, 30, 'scalar', seed, False, True)
        seed += 1
        cases['star_p%g_fvec' % p] = ('star', p, 30, 'vector', seed, False, False)

    deltas = {}

    def check(tag, W, bdy, g, f, p, nbis, u0, u_ref):
        """restatement against the reference: bits for p == 1, the class's delta otherwise; returns the rounds"""
        rc, u, rounds = ref.host_solve(lib, W, f, [bdy], [g], p, nbis, u0=u0)
        assert rc == 0, (tag, rc)
        if p == 1 and np.min(f) > 0:
            assert u[:, 0].tobytes() == u_ref.tobytes(), (tag, 'restatement != reference', np.abs(u[:, 0] - u_ref).max())
        else:
            d = float(np.abs(u[:, 0] - u_ref).max() / np.abs(u_ref).max())
            deltas[(float(p), int(nbis))] = max(deltas.get((float(p), int(nbis)), 0.0), d)
        return rounds

    for name, (gname, p, nbis, fkind, sd, nl, has_u0) in cases.items():
        W = graphs[gname]
        n = W.shape[0]
        bdy, g, f = case_inputs(W, gname, sd, fkind)
        u0 = np.round(np.random.default_rng(sd).uniform(-3, 3, size=n), 2) if has_u0 else None
        G = gl.graph(W)
        u_ref = G.peikonal(bdy, bdy_val=g, f=f if fkind != 'scalar' else float(f), p=p, nl_bdy=nl, u0=u0, solver='fmm', num_bisection_it=nbis)
        sb, sg = ref.dilate(W, bdy, g) if nl else (bdy, g)
        rounds = check(name, W, sb, sg, f, p, nbis, u0, u_ref)
        if gname == 'twocomp':
            assert np.array_equal(u_ref[12:], u0[12:] if has_u0 else np.zeros(5)), name
        print('case %-20s n=%-4d p=%-4g nbis=%d bdy=%d rounds=%d max|u|=%.4g' % (name, n, p, nbis, len(sb), rounds, np.abs(u_ref).max()))
        out.update({'case_%s_graph' % name: np.array(gname), 'case_%s_p' % name: np.float64(p), 'case_%s_nbis' % name: np.int64(nbis),
                    'case_%s_bdy' % name: bdy, 'case_%s_g' % name: g, 'case_%s_f' % name: np.asarray(f, dtype=np.float64),
                    'case_%s_nl_bdy' % name: np.bool_(nl), 'case_%s_exact' % name: np.bool_(p == 1 and np.min(f) > 0), 'case_%s_has_u0' % name: np.bool_(has_u0),
                    'case_%s_u0' % name: u0 if has_u0 else np.zeros(0), 'case_%s_u' % name: u_ref, 'case_%s_rounds' % name: np.int64(rounds)})
    out['case_names'] = np.array(list(cases))

    # what the marching pass does on an unsymmetric PATTERN (not stored): vertex 3 lists 0, nobody lists 3
    Wd = sparse.csr_matrix(np.array([[0, 1, 0, 0], [1, 0, 1, 0], [0, 1, 0, 0], [1, 0, 0, 0.0]]))
    Wd[3, 0] = 1.0
    u_ref = gl.graph(Wd).peikonal(np.array([0]), bdy_val=0.25)
    _, u_fix, _ = ref.host_solve(lib, Wd, 1.0, [np.array([0])], [np.array([0.25])], 1, 30)
    print('unsymmetric pattern: reference', u_ref, 'fixed point', u_fix[:, 0])

    # the learner
    fits = {}
    for gname, per_class in (('blobs', 5), ('moons', 5)):
        W = graphs[gname]
        truth = gold['graph_%s_truth' % gname].astype(np.int64)
        classes = np.unique(truth)
        priors = gl.utils.class_priors(truth)
        for tag, kw in (('p1', dict(p=1)), ('p2', dict(p=2)), ('p1_priors', dict(p=1, class_priors=priors)),
                        ('p2_priors', dict(p=2, class_priors=priors)), ('D', dict(p=1, D=W, alpha=2)),
                        ('eps', dict(p=2, eps_ball_graph=True, alpha=0.5))):
            label_seed = 7
            while True:
                rng = np.random.default_rng(label_seed)
                train_ind = np.sort(np.concatenate([rng.choice(np.where(truth == c)[0], size=per_class, replace=False) for c in classes]))
                model = gl.ssl.peikonal(W, **kw)
                pred = model.fit_predict(train_ind, truth[train_ind])
                prob = np.asarray(model.prob, dtype=np.float64)
                p = kw['p']
                rounds = [check('fit_%s_%s' % (gname, tag), W, train_ind[truth[train_ind] == c], np.zeros(int((truth[train_ind] == c).sum())),
                                model.f, p, 30, None, prob[:, q].copy()) for q, c in enumerate(classes)]
                if p == 1:
                    break
                part = np.partition(prob, 1, axis=1)
                gap = float((part[:, 1] - part[:, 0]).min())
                need = 1000 * 16 * deltas[(float(p), 30)] * float(np.abs(prob).max())
                if gap > need:
                    break
                print('fit %s %s: label seed %d leaves a gap of %.3g (needs %.3g), next seed' % (gname, tag, label_seed, gap, need))
                label_seed += 1
            key = 'fit_%s_%s' % (gname, tag)
            fits.update({key + '_train_ind': train_ind.astype(np.int64), key + '_prob': prob, key + '_pred': np.asarray(pred).astype(np.int64),
                         key + '_rounds': np.array(rounds, dtype=np.int64), key + '_name': np.array(model.name),
                         key + '_file': np.array(model.accuracy_filename)})
            print('fit %-6s %-10s accuracy %.2f%% rounds=%s name=%r' % (gname, tag, gl.ssl.ssl_accuracy(pred, truth, train_ind), rounds, model.name))
        fits['fit_%s_priors' % gname] = priors
    out.update(fits)

    classes = sorted(deltas)
    out['class_p'] = np.array([c[0] for c in classes])
    out['class_nbis'] = np.array([c[1] for c in classes], dtype=np.int64)
    out['class_delta'] = np.array([deltas[c] for c in classes])
    out['class_bound'] = 16 * out['class_delta']
    for c in classes:
        print('class p=%g nbis=%d delta=%.3g bound=%.3g' % (c[0], c[1], deltas[c], 16 * deltas[c]))
    assert all(deltas[c] > 0 for c in classes)
    # the learner fits were checked with the deltas known when they ran: once more against the final ones
    for key in [k[:-5] for k in fits if k.endswith('_prob')]:
        tagp = 2.0 if ('_p2' in key or key.endswith('_eps')) else 1.0
        if tagp != 1:
            prob = fits[key + '_prob']
            part = np.partition(prob, 1, axis=1)
            assert (part[:, 1] - part[:, 0]).min() > 1000 * 16 * deltas[(tagp, 30)] * np.abs(prob).max(), key

    path = os.path.join(HERE, ref.GOLDEN_FILE)
    np.savez_compressed(path, **out)
    print(ref.GOLDEN_FILE, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) <= LIMIT, path


if __name__ == '__main__':
    main()
