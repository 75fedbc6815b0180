#!/usr/bin/env python3
"""Generate the shortest-path golden fixtures tests/golden/g14_dijkstra*.npz from THE COMPILED REFERENCE.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONPATH=<the reference's checkout> PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg \
        python3 tests/golden/make_golden_dijkstra.py        (from the repository root)

The reference's C extension is not installed there, so the generator compiles the two source files behind its Dijkstra
(c_code/hjsolvers.cpp, c_code/memory_allocation.cpp) where they lie into a temporary directory OUTSIDE the repository
(g++ -O2 -ffp-contract=off -fPIC -shared) and binds dijkstra_main / dijkstra_hl_main through ctypes as the module
`graphlearning.cextensions`, so that the reference's own graph.dijkstra, graph.dijkstra_hl and ssl.graph_nearest_neighbor run
unchanged on the arrays its __ccode_init__ builds.  Captured with Python 3.10.12, numpy 2.2.6, scipy 1.15.3, g++ 11.4,
reference graphlearning 1.7.5.

The files hold inputs and the reference's outputs (data only): the graphs as CSR, and per case the sources, boundary values, f,
max_dist and the reference's RAW `dist` / `cp` (above max_dist the reference leaves heap-tentative values; the tests map them to
inf / -1, as its documentation says).  Before anything is written the restatement tests/dijkstra_ref.py (heap form, fixed-point
form, tight-chain closest point) is checked against the compiled reference on every case, and the conditions the host tests rely on
are asserted: no empty row, exactly one tight-reachable source per reached vertex, no subnormal distance."""
import ctypes
import io
import os
import subprocess
import sys
import tempfile
import types
import numpy as np
from scipy import sparse

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import graphlearning as gl                      # the REFERENCE (PYTHONPATH=/root/reference)
import dijkstra_ref as ref                      # the restatement, cross-checked below

assert gl.__file__.startswith('/root/reference'), gl.__file__
REF_ROOT = os.path.dirname(os.path.dirname(gl.__file__))
LIMIT = 1000000      # bytes per file


def compile_reference():
    tmp = tempfile.mkdtemp(prefix='glx_dijkstra_ref_')
    assert not os.path.abspath(tmp).startswith(os.path.dirname(os.path.dirname(HERE))), tmp
    so = os.path.join(tmp, 'hjsolvers.so')
    src = [os.path.join(REF_ROOT, 'c_code', f) for f in ('hjsolvers.cpp', 'memory_allocation.cpp')]
    subprocess.run(['g++', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-o', so] + src, check=True)
    lib = ctypes.CDLL(so)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    fns = {}
    for name, sym in (('dijkstra', '_Z13dijkstra_mainPdPiS0_S0_S_S0_S_S_biiid'), ('dijkstra_hl', '_Z16dijkstra_hl_mainPdPiS0_S0_S_S0_S_S_biiid')):
        fn = getattr(lib, sym)
        fn.argtypes = [dp, ip, ip, ip, dp, ip, dp, dp, ctypes.c_bool, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double]
        fn.restype = None
        fns[name] = fn

    def bind(fn):
        # the argument list of c_code/cextensions.cpp:152-231: (d, l, WI, K, WV, I, g, f, prog, max_radius)
        def call(d, l, WI, K, WV, I, g, f, prog, max_dist):
            for a, dt in ((d, np.float64), (l, np.int32), (WI, np.int32), (K, np.int32), (WV, np.float64), (I, np.int32), (g, np.float64),
                          (f, np.float64)):
                assert isinstance(a, np.ndarray) and a.dtype == dt and a.flags['C_CONTIGUOUS'], (a.dtype, dt)
            fn(d.ctypes.data_as(dp), l.ctypes.data_as(ip), WI.ctypes.data_as(ip), K.ctypes.data_as(ip), WV.ctypes.data_as(dp),
               I.ctypes.data_as(ip), g.ctypes.data_as(dp), f.ctypes.data_as(dp), bool(prog), len(d), len(WI), len(I), float(max_dist))
        return call
    mod = types.ModuleType('graphlearning.cextensions')
    mod.dijkstra = bind(fns['dijkstra'])
    mod.dijkstra_hl = bind(fns['dijkstra_hl'])
    sys.modules['graphlearning.cextensions'] = mod
    gl.cextensions = mod


def blobs(n, d, C, seed, scale=1.5):
    rng = np.random.default_rng(seed)
    centers = rng.normal(size=(C, d)) * scale
    labels = rng.integers(0, C, size=n)
    return centers[labels] + rng.normal(size=(n, d)), labels.astype(np.int64)


def build_graph(spec):
    labels = None
    if spec['kind'] == 'blobs':
        X, labels = blobs(spec['n'], spec['d'], spec['C'], spec['seed'])
    else:
        X = np.random.default_rng(spec['seed']).random((spec['n'], spec['d']))
    if spec['kind'] == 'ball':
        W = gl.weightmatrix.epsilon_ball(X, spec['eps'], kernel=spec['kernel'])
    else:
        knn_data = gl.weightmatrix.knnsearch(X, spec['k'], method='kdtree')
        W = gl.weightmatrix.knn(None, spec['k'], kernel=spec['kernel'], symmetrize=spec['symmetrize'], knn_data=knn_data)
    W = sparse.csr_matrix(W)
    W.sort_indices()
    assert W.data.min() > 0 and np.diff(W.indptr).min() >= 1, 'a golden graph has an empty row or a non-positive weight'
    return W, labels


def check_case(name, W, src, g, f, max_dist, hl, recip, raw_d, raw_cp):
    """restatement == compiled reference, and the conditions the host tests rely on."""
    n = W.shape[0]
    I, J, C = ref.edges(W, f, recip)
    want = np.where(raw_d <= max_dist, raw_d, np.inf)
    u, rounds = ref.fixed_point(n, I, J, C, src, g, max_dist, hl)
    assert u.tobytes() == want.tobytes(), (name, 'fixed point != reference')
    uh, lh = ref.heap(n, I, J, C, src, g, max_dist, hl)
    assert uh.tobytes() == want.tobytes(), (name, 'heap != reference')
    reached = np.isfinite(want)
    assert ref.unique_closest(n, I, J, C, src, g, u, max_dist, hl)[reached].all(), (name, 'a vertex has two tight-reachable sources')
    cp = ref.closest_point(n, I, J, C, src, g, u, max_dist, hl)
    assert np.array_equal(cp[reached], raw_cp[reached]) and (cp[~reached] == -1).all(), (name, 'closest point != reference')
    assert np.array_equal(lh[reached], raw_cp[reached]), (name, 'heap closest point != reference')
    pos = want[reached & (want > 0)]
    assert pos.size == 0 or pos.min() >= np.finfo(np.float64).tiny, (name, 'subnormal distance')
    return rounds, int(reached.sum())


def run_reference(G, src, g, f, max_dist, hl, recip):
    if hl:
        d, cp = G.dijkstra_hl(src, bdy_val=g, f=f, max_dist=max_dist, return_cp=True)
    else:
        d, cp = G.dijkstra(src, bdy_val=g, f=f, max_dist=max_dist, return_cp=True, reciprocal_weights=recip)
    return d, cp


def main():
    compile_reference()
    cases = []
    graphs, labels = {}, {}
    for gname, spec in ref.GOLDEN_GRAPHS.items():
        W, lab = build_graph(spec)
        graphs[gname], labels[gname] = W, lab
        arrs = {'graph_%s_indptr' % gname: W.indptr.astype(np.int32), 'graph_%s_indices' % gname: W.indices.astype(np.int32),
                'graph_%s_data' % gname: W.data.astype(np.float64)}
        if lab is not None:
            arrs['graph_%s_labels' % gname] = lab
        cases.append(('graph_' + gname, arrs))
        print('graph %-10s n=%d entries=%d degrees %d..%d symmetric=%s' % (gname, W.shape[0], W.nnz, np.diff(W.indptr).min(),
                                                                          np.diff(W.indptr).max(), (abs(W - W.T) > 0).nnz == 0))
    for name, (gname, m, dom, fk, md_q, hl, recip) in ref.GOLDEN_CASES.items():
        W = graphs[gname]
        G = gl.graph(W)
        src, g, f = ref.golden_case_inputs(name, W)
        max_dist = np.inf
        if md_q is not None:
            d0, _ = run_reference(G, src, g, f, np.inf, hl, recip)
            max_dist = float(np.quantile(d0[np.isfinite(d0)], md_q))
        raw_d, raw_cp = run_reference(G, src, g, f, max_dist, hl, recip)
        rounds, reached = check_case(name, W, src, g, f, max_dist, hl, recip, raw_d, raw_cp)
        if dom:
            assert raw_d[src[1]] < g[1], (name, 'the dominated source is not dominated')
        print('case %-18s %-9s sources=%d max_dist=%-8.4g hl=%d recip=%d reached=%d rounds=%d' % (name, gname, m, max_dist, hl, recip,
                                                                                                   reached, rounds))
        cases.append((name, {name + '_src': src.astype(np.int32), name + '_g': g, name + '_f': np.asarray(f, dtype=np.float64),
                             name + '_max_dist': np.float64(max_dist), name + '_dist': raw_d, name + '_cp': raw_cp.astype(np.int32)}))

    # ssl.graph_nearest_neighbor on the blobs graph: closest-point labels, one-vs-rest distances under class priors, and the
    # density reweighting f = (distance to the farthest neighbour / its maximum)**alpha
    W, lab = graphs['blobs'], labels['blobs']
    from scipy.sparse import csgraph
    assert csgraph.connected_components(W)[0] == 1, 'the fit graph must be connected (one-vs-rest distances are finite)'
    rng = np.random.default_rng(11)
    train_ind = np.sort(np.concatenate([rng.choice(np.where(lab == c)[0], size=4, replace=False) for c in range(3)]))
    fits = {'nn_train_ind': train_ind.astype(np.int64)}
    priors = gl.utils.class_priors(lab)
    for tag, kw in (('plain', {}), ('priors', {'class_priors': priors}), ('D', {'D': W, 'alpha': 2})):
        model = gl.ssl.graph_nearest_neighbor(W, **kw)
        pred = model.fit_predict(train_ind, lab[train_ind])
        fits['nn_%s_pred' % tag] = np.asarray(pred).astype(np.int64)
        fits['nn_%s_prob' % tag] = np.asarray(model.prob, dtype=np.float64)
        print('fit %-7s accuracy %.2f%%  name=%r file=%r' % (tag, gl.ssl.ssl_accuracy(pred, lab, train_ind), model.name, model.accuracy_filename))
        # every fit is a Dijkstra call of the kind checked above: the same conditions on the inputs it actually uses
        f = model.f
        groups = [train_ind[lab[train_ind] == c] for c in range(3)] if 'class_priors' in kw else [train_ind]
        for src in groups:
            g = np.zeros(len(src))
            raw_d, raw_cp = G_run(W, src, g, f)
            check_case('nn_' + tag, W, src, g, f, np.inf, False, False, raw_d, raw_cp)
    fits['nn_priors'] = priors
    cases.append(('nn', fits))

    files, where = [dict()], {}
    for name, arrs in cases:
        trial = dict(files[-1])
        trial.update(arrs)
        buf = io.BytesIO()
        np.savez_compressed(buf, **trial)
        if buf.tell() > LIMIT - 20000 and files[-1]:
            files.append(dict(arrs))
        else:
            files[-1] = trial
        where[name] = len(files) - 1
    names = ['g14_dijkstra.npz'] + ['g14_dijkstra_%d.npz' % i for i in range(2, len(files) + 1)]
    files[0]['entry_names'] = np.array(sorted(where))
    files[0]['entry_files'] = np.array([names[where[c]] for c in sorted(where)])
    for fn, arrs in zip(names, files):
        path = os.path.join(HERE, fn)
        np.savez_compressed(path, **arrs)
        print(fn, os.path.getsize(path), 'bytes')
        assert os.path.getsize(path) <= 1024 * 1024, fn


def G_run(W, src, g, f):
    return run_reference(gl.graph(W), src, g, f, np.inf, False, False)


if __name__ == '__main__':
    main()
