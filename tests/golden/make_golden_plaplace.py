#!/usr/bin/env python3
"""Generate the p-Laplace learner's golden fixtures tests/golden/g17_plaplace*.npz from THE COMPILED REFERENCE.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONPATH=<the reference's checkout> PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg \
        python3 tests/golden/make_golden_plaplace.py        (from the repository root)

The reference's C extension is not installed there.  The generator loads oracle/_ref/liblp_ref.so (the reference's own
c_code/lp_iterate.cpp + memory_allocation.cpp, g++ -O2 -ffp-contract=off, the recipe of oracle/Makefile) or, when that is missing,
compiles the two files where they lie into a temporary directory OUTSIDE the repository, and binds lip_iterate_main and lp_iterate_main
through ctypes as `graphlearning.cextensions.lip_iterate` / `.lp_iterate` with the argument lists of c_code/cextensions.cpp, so that the
reference's own ssl.plaplace(...).fit(...) runs unchanged on the arrays its __ccode_init__ builds.

The files hold inputs and the reference's outputs (data only): the graphs as CSR plus the entry lists I, J, V of the capturing host's
__ccode_init__, the labels and the training set, and per case the reference's prob, predict() and the iterations every class ran.  For
fast=True the iterations are counted from the reference's own progress lines (a second call per class with prog on, its u asserted equal
to the fit's column); for fast=False they come from oracle.gl_oracle.plaplace_jacobi(..., return_iters=True) after its uu / ul were
asserted equal to the compiled reference's bit for bit.  Asserted before anything is written: no empty row; the per-class stopping
iterations of the (p = 10, tol 1e-1) Jacobi case on blobs3 are not all equal and hold both an even and an odd one."""
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
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import graphlearning as gl                      # the REFERENCE (PYTHONPATH points at its checkout)
import plaplace_ref as ref
from oracle import gl_oracle as orc

REF_ROOT = os.path.dirname(os.path.dirname(gl.__file__))
assert not os.path.abspath(gl.__file__).startswith(ROOT), gl.__file__
LIMIT = 1000000      # bytes per file


class captured_stdout:
    """The C library's standard output (its progress lines) into a file for the duration of the block."""
    def __enter__(self):
        sys.stdout.flush()
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(1)
        os.dup2(self.tmp.fileno(), 1)
        return self

    def __exit__(self, *exc):
        ctypes.CDLL(None).fflush(None)
        os.dup2(self.saved, 1)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode()
        self.tmp.close()


def blobs(n, d, C, seed, scale=1.5):
    rng = np.random.default_rng(seed)
    centers = rng.normal(size=(C, d)) * scale
    labels = rng.integers(0, C, size=n)
    return centers[labels] + rng.normal(size=(n, d)), labels.astype(np.int64)


def bind_reference():
    so = os.path.join(ROOT, 'oracle', '_ref', 'liblp_ref.so')
    if not os.path.exists(so):
        tmp = tempfile.mkdtemp(prefix='glx_plaplace_ref_')
        assert not os.path.abspath(tmp).startswith(ROOT), tmp
        so = os.path.join(tmp, 'liblp_ref.so')
        src = [os.path.join(REF_ROOT, 'c_code', f) for f in ('lp_iterate.cpp', 'memory_allocation.cpp')]
        subprocess.run(['g++', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-I' + os.path.join(REF_ROOT, 'c_code'), '-o', so] + src,
                       check=True)
    lib = ctypes.CDLL(so)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    lip = getattr(lib, '_Z16lip_iterate_mainPdPiS0_S_S0_S_idbiiidd')
    lip.argtypes = [dp, ip, ip, dp, ip, dp, ctypes.c_int, ctypes.c_double, ctypes.c_bool, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                    ctypes.c_double, ctypes.c_double]
    lip.restype = None
    lp = getattr(lib, '_Z15lp_iterate_mainPdS_PiS0_S_S0_S_didbiii')      # as tests/golden/make_golden.py:g9_plaplace calls it
    lp.argtypes = [dp, dp, ip, ip, dp, ip, dp, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_bool, ctypes.c_int, ctypes.c_int,
                   ctypes.c_int]
    lp.restype = None

    def check(arrs):
        for a, dt in arrs:
            assert isinstance(a, np.ndarray) and a.dtype == dt and a.flags['C_CONTIGUOUS'], (a.dtype, dt)

    def lip_iterate(u, II, J, W, ind, val, Td, tol, progd, weightedd, alpha, beta):
        check(((u, np.float64), (II, np.int32), (J, np.int32), (W, np.float64), (ind, np.int32), (val, np.float64)))
        assert not bool(weightedd)
        lip(u.ctypes.data_as(dp), II.ctypes.data_as(ip), J.ctypes.data_as(ip), W.ctypes.data_as(dp), ind.ctypes.data_as(ip),
            val.ctypes.data_as(dp), int(Td), float(tol), bool(progd), u.shape[0], II.shape[0], ind.shape[0], float(alpha), float(beta))

    def lp_iterate(uu, ul, II, J, W, ind, val, p, Td, tol, progd):
        check(((uu, np.float64), (ul, np.float64), (II, np.int32), (J, np.int32), (W, np.float64), (ind, np.int32), (val, np.float64)))
        lp(uu.ctypes.data_as(dp), ul.ctypes.data_as(dp), II.ctypes.data_as(ip), J.ctypes.data_as(ip), W.ctypes.data_as(dp),
           ind.ctypes.data_as(ip), val.ctypes.data_as(dp), float(p), int(Td), float(tol), bool(progd), uu.shape[0], II.shape[0], ind.shape[0])
    mod = types.ModuleType('graphlearning.cextensions')
    mod.lip_iterate = lip_iterate
    mod.lp_iterate = lp_iterate
    sys.modules['graphlearning.cextensions'] = mod
    gl.cextensions = mod
    return mod


def build_graph(spec):
    X, labels = blobs(spec['n'], spec['d'], spec['C'], spec['seed'])
    knn_data = gl.weightmatrix.knnsearch(X, spec['k'], method='kdtree')
    W = gl.weightmatrix.knn(None, spec['k'], kernel='gaussian', symmetrize=spec['symmetrize'], knn_data=knn_data)
    W = sparse.csr_matrix(W)
    W.sort_indices()
    W.eliminate_zeros()
    assert W.data.min() > 0 and np.diff(W.indptr).min() >= 1, 'a golden graph has an empty row or a non-positive weight'
    rng = np.random.default_rng(spec['seed'] + 100)
    ti = np.sort(np.concatenate([rng.choice(np.where(labels == c)[0], size=spec['per_class'], replace=False) for c in range(spec['C'])]))
    return W, labels, ti.astype(np.int64)


def fast_iterations(G, ti, col, p, T, want_u):
    """Sweeps of one class, counted from the reference's progress lines; its u is the fit's column."""
    u = np.ascontiguousarray(np.zeros((G.num_nodes,)), dtype=np.float64)
    with captured_stdout() as out:
        gl.cextensions.lip_iterate(u, G.J, G.I, G.V, np.ascontiguousarray(ti, dtype=np.int32), np.ascontiguousarray(col, dtype=np.float64),
                                   T, 1e-6, float(True), float(False), float(1 / (p - 1)), float(1 - 1 / (p - 1)))
    lines = [l for l in out.text.splitlines() if l.startswith('Iter=')]
    assert [int(l.split(',')[0][5:]) for l in lines] == list(range(len(lines)))
    assert u.tobytes() == np.ascontiguousarray(want_u).tobytes(), 'the counted run is not the fit'
    return len(lines)


def main():
    bind_reference()
    cases = []
    graphs = {}
    for gname, spec in ref.GOLDEN_GRAPHS.items():
        W, lab, ti = build_graph(spec)
        G = gl.graph(W)
        I, J, V = orc.ccode_arrays(W)
        assert np.array_equal(I, G.I) and np.array_equal(J, G.J) and V.tobytes() == G.V.tobytes(), 'ccode_arrays != __ccode_init__'
        graphs[gname] = (W, lab, ti)
        cases.append(('graph_' + gname, {
            'graph_%s_indptr' % gname: W.indptr.astype(np.int32), 'graph_%s_indices' % gname: W.indices.astype(np.int32),
            'graph_%s_data' % gname: W.data.astype(np.float64), 'graph_%s_I' % gname: G.I, 'graph_%s_J' % gname: G.J, 'graph_%s_V' % gname: G.V,
            'graph_%s_labels' % gname: lab, 'graph_%s_train_ind' % gname: ti, 'graph_%s_priors' % gname: gl.utils.class_priors(lab)}))
        print('graph %-12s n=%d entries=%d degrees %d..%d symmetric=%s' % (gname, W.shape[0], W.nnz, np.diff(W.indptr).min(),
                                                                          np.diff(W.indptr).max(), (abs(W - W.T) > 0).nnz == 0))

    for name, (gname, fast, p, tol, T) in ref.GOLDEN_CASES.items():
        W, lab, ti = graphs[gname]
        G = gl.graph(W)
        tl = lab[ti]
        model = gl.ssl.plaplace(W, p=p, max_num_it=T, tol=tol, fast=fast)
        prob = np.asarray(model.fit(ti, tl), dtype=np.float64)
        pred = np.asarray(model.predict()).astype(np.int64)
        classes = np.unique(tl)
        iters = np.zeros(len(classes), dtype=np.int64)
        for c, l in enumerate(classes):
            if fast:
                iters[c] = fast_iterations(G, ti, tl == l, p, T, prob[:, c])
            else:
                u, it, ouu, oul = orc.plaplace_jacobi(W, ti, (tl == l).astype(np.float64), p, tol=tol, max_num_it=T, return_iters=True,
                                                      return_bounds=True)
                # the compiled reference on the same column: uu, ul bit for bit
                bdy_val = np.ascontiguousarray(tl == l, dtype=np.float64)
                uu, ul = ref.start_values(W.shape[0], ti, bdy_val)
                gl.cextensions.lp_iterate(uu, ul, G.J, G.I, G.V, np.ascontiguousarray(ti, dtype=np.int32), bdy_val, p, float(T), float(tol), 0.0)
                assert uu.tobytes() == ouu.tobytes() and ul.tobytes() == oul.tobytes(), (name, c, 'oracle != compiled reference')
                assert ((uu + ul) / 2).tobytes() == np.ascontiguousarray(prob[:, c]).tobytes(), (name, c, 'column != fit')
                iters[c] = it
        arrs = {name + '_prob': prob, name + '_pred': pred, name + '_iters': iters}
        if name == ref.PRIORS_CASE:
            pm = gl.ssl.plaplace(W, class_priors=gl.utils.class_priors(lab), p=p, max_num_it=T, tol=tol, fast=fast)
            ppred = pm.fit_predict(ti, tl)
            assert np.asarray(pm.prob, dtype=np.float64).tobytes() == prob.tobytes()
            arrs[name + '_priors_pred'] = np.asarray(ppred).astype(np.int64)
            assert len(set(iters.tolist())) > 1 and len(set((iters % 2).tolist())) == 2, (name, iters, 'change the seed: the stops must differ '
                                                                                         'and hold both parities')
        print('case %-16s %-12s fast=%d p=%g tol=%g T=%g iterations=%s accuracy %.2f%% file=%r' % (
            name, gname, fast, p, tol, T, iters.tolist(), gl.ssl.ssl_accuracy(pred, lab, ti), model.get_accuracy_filename()))
        cases.append((name, arrs))

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
    names = ['g17_plaplace.npz'] + ['g17_plaplace_%d.npz' % i for i in range(2, len(files) + 1)]
    files[0]['entry_names'] = np.array(sorted(where))
    files[0]['entry_files'] = np.array([names[where[c]] for c in sorted(where)])
    for fn, arrs in zip(names, files):
        path = os.path.join(HERE, fn)
        np.savez_compressed(path, **arrs)
        print(fn, os.path.getsize(path), 'bytes')
        assert os.path.getsize(path) <= LIMIT, fn


if __name__ == '__main__':
    main()
