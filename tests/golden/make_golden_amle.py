#!/usr/bin/env python3
"""Generate the AMLE golden fixtures tests/golden/g15_amle*.npz from THE COMPILED REFERENCE.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONPATH=<the reference's checkout> PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg \
        python3 tests/golden/make_golden_amle.py        (from the repository root)

The reference's C extension is not installed there.  The generator loads oracle/_ref/liblp_ref.so (the reference's own
c_code/lp_iterate.cpp + memory_allocation.cpp, g++ -O2 -ffp-contract=off, the recipe of oracle/Makefile) or, when that is missing,
compiles the two files where they lie into a temporary directory OUTSIDE the repository, and binds lip_iterate_main /
lip_iterate_weighted_main through ctypes as `graphlearning.cextensions.lip_iterate` with the argument list of
c_code/cextensions.cpp:62-107, so that the reference's own graph.amle and ssl.amle run unchanged on the arrays its __ccode_init__
builds.  Captured with Python 3.10.12, numpy 2.2.6, scipy 1.15.3, g++ 11.4, reference graphlearning 1.7.5.

The files hold inputs and the reference's outputs (data only): the graphs as CSR with the neighbour order of their entry lists, and per
case the boundary vertices, the boundary values (m, B), the reference's u (n, B), the sweeps every column ran and its error history.
The sweeps and errors come from the reference's own progress lines (`Iter=%d, err=%.15f`, read from its standard output) for the
count and from the restatement for the bits.  Before anything is written, on every case: the host restatement of
tests/lip_plan_host.cpp, in index order and level by level, equals the compiled reference bit for bit; so do the Python forms of
tests/amle_ref.py on the cases short enough for them (amle_ref.python_forms_fit).  Asserted and stored: no empty row, the level
counts, and that the per-class stop sweeps of the learner cases are not all equal."""
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

import graphlearning as gl                      # the REFERENCE (PYTHONPATH=/root/reference)
import amle_ref as ref                          # the restatement, cross-checked below

assert gl.__file__.startswith('/root/reference'), gl.__file__
REF_ROOT = os.path.dirname(os.path.dirname(gl.__file__))
LIMIT = 1000000      # bytes per file


def bind_reference():
    so = os.path.join(ROOT, 'oracle', '_ref', 'liblp_ref.so')
    if not os.path.exists(so):
        tmp = tempfile.mkdtemp(prefix='glx_amle_ref_')
        assert not os.path.abspath(tmp).startswith(ROOT), tmp
        so = os.path.join(tmp, 'liblp_ref.so')
        src = [os.path.join(REF_ROOT, 'c_code', f) for f in ('lp_iterate.cpp', 'memory_allocation.cpp')]
        subprocess.run(['g++', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-I' + os.path.join(REF_ROOT, 'c_code'), '-o', so] + src,
                       check=True)
    lib = ctypes.CDLL(so)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    plain = getattr(lib, '_Z16lip_iterate_mainPdPiS0_S_S0_S_idbiiidd')
    plain.argtypes = [dp, ip, ip, dp, ip, dp, ctypes.c_int, ctypes.c_double, ctypes.c_bool, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                      ctypes.c_double, ctypes.c_double]
    plain.restype = None
    weighted_fn = getattr(lib, '_Z25lip_iterate_weighted_mainPdPiS0_S_S0_S_idbiii')
    weighted_fn.argtypes = [dp, ip, ip, dp, ip, dp, ctypes.c_int, ctypes.c_double, ctypes.c_bool, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    weighted_fn.restype = None

    def lip_iterate(u, II, J, W, ind, val, Td, tol, progd, weightedd, alpha, beta):
        # the argument list and casts of c_code/cextensions.cpp:62-107
        for a, dt in ((u, np.float64), (II, np.int32), (J, np.int32), (W, np.float64), (ind, np.int32), (val, np.float64)):
            assert isinstance(a, np.ndarray) and a.dtype == dt and a.flags['C_CONTIGUOUS'], (a.dtype, dt)
        n, M, m = u.shape[0], II.shape[0], ind.shape[0]
        args = [u.ctypes.data_as(dp), II.ctypes.data_as(ip), J.ctypes.data_as(ip), W.ctypes.data_as(dp), ind.ctypes.data_as(ip),
                val.ctypes.data_as(dp), int(Td), float(tol), bool(progd), n, M, m]
        if bool(weightedd):
            weighted_fn(*args)
        else:
            plain(*(args + [float(alpha), float(beta)]))
    mod = types.ModuleType('graphlearning.cextensions')
    mod.lip_iterate = lip_iterate
    sys.modules['graphlearning.cextensions'] = mod
    gl.cextensions = mod
    return mod


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


def build_graph(spec):
    labels = None
    kind = spec['kind']
    if kind == 'path':
        n = spec['n']
        W = sparse.diags([np.ones(n - 1), np.ones(n - 1)], [1, -1], format='csr')
    else:
        if kind == 'blobs':
            X, labels = blobs(spec['n'], spec['d'], spec['C'], spec['seed'])
        else:
            X = np.random.default_rng(spec['seed']).random((spec['n'], spec['d']))
        if kind == 'sorted':
            X = X[np.argsort(X[:, 0])]
        if kind == 'ball':
            W = gl.weightmatrix.epsilon_ball(X, spec['eps'], kernel=spec['kernel'])
        else:
            knn_data = gl.weightmatrix.knnsearch(X, spec['k'], method='kdtree')
            W = gl.weightmatrix.knn(None, spec['k'], kernel=spec['kernel'], symmetrize=spec['symmetrize'], knn_data=knn_data)
        if kind == 'diag':
            n = spec['n']
            d = np.zeros(n)
            d[::3] = 0.5 + np.random.default_rng(spec['seed'] + 1).random(len(d[::3]))
            W = sparse.csr_matrix(W) + sparse.diags(d, 0, format='csr')
    W = sparse.csr_matrix(W)
    W.sort_indices()
    W.eliminate_zeros()
    assert W.data.min() > 0 and np.diff(W.indptr).min() >= 1, 'a golden graph has an empty row or a non-positive weight'
    return W, labels


def reference_column(G, ind, val, weighted, tol, T, alpha, beta):
    """u, sweeps and printed errors of the compiled reference for one column, through the reference's own graph.amle where the case is
    graph.amle's (alpha 0, beta 1), else through its cextensions call with plaplace(fast=True)'s arguments (graph.py:1252-1261)."""
    with captured_stdout() as out:
        if alpha == 0.0 and beta == 1.0:
            u = G.amle(ind, val, tol=tol, max_num_it=T, weighted=weighted, prog=True)
        else:
            u = np.ascontiguousarray(np.zeros((G.num_nodes,)), dtype=np.float64)
            gl.cextensions.lip_iterate(u, G.J, G.I, G.V, np.ascontiguousarray(ind, dtype=np.int32), np.ascontiguousarray(val, dtype=np.float64),
                                       float(T), tol, float(True), float(weighted), float(alpha), float(beta))
    lines = [l for l in out.text.splitlines() if l.startswith('Iter=')]
    printed = [float(l.split('err=')[1]) for l in lines]
    assert [int(l.split(',')[0][5:]) for l in lines] == list(range(len(lines)))
    return u, len(lines), printed


def main():
    bind_reference()
    lib = ref.build_host_lib(tempfile.mkdtemp(prefix='glx_amle_host_'))
    cases = []
    graphs, labels, ents = {}, {}, {}
    for gname, spec in ref.GOLDEN_GRAPHS.items():
        W, lab = build_graph(spec)
        graphs[gname], labels[gname] = W, lab
        G = gl.graph(W)
        rows, nbr, V = ref.entries(W)
        assert np.array_equal(rows, G.I) and np.array_equal(nbr, G.J) and V.tobytes() == G.V.tobytes(), 'entries() != __ccode_init__'
        ents[gname] = (rows, nbr, V)
        arrs = {'graph_%s_indptr' % gname: W.indptr.astype(np.int32), 'graph_%s_indices' % gname: W.indices.astype(np.int32),
                'graph_%s_data' % gname: W.data.astype(np.float64), 'graph_%s_J' % gname: nbr}
        if lab is not None:
            arrs['graph_%s_labels' % gname] = lab
        cases.append(('graph_' + gname, arrs))
        print('graph %-10s n=%d entries=%d degrees %d..%d diagonal=%d symmetric=%s' % (
            gname, W.shape[0], W.nnz, np.diff(W.indptr).min(), np.diff(W.indptr).max(), int((W.diagonal() != 0).sum()),
            (abs(W - W.T) > 0).nnz == 0))

    rng = np.random.default_rng(11)
    lab = labels['blobs']
    train_ind = np.sort(np.concatenate([rng.choice(np.where(lab == c)[0], size=4, replace=False) for c in range(3)]))
    fits = {'fit_train_ind': train_ind.astype(np.int64), 'fit_priors': gl.utils.class_priors(lab)}

    for name, (gname, bd, weighted, tol, T, alpha, beta) in ref.GOLDEN_CASES.items():
        W = graphs[gname]
        n = W.shape[0]
        G = gl.graph(W)
        rows, nbr, V = ents[gname]
        ind, vals = ref.case_boundary(name, W, labels['blobs'], train_ind)
        B = vals.shape[1]
        mask, _ = ref.boundary(n, ind, vals[:, 0])
        plan = ref.host_plan(lib, n, rows, nbr, mask)
        assert np.array_equal(plan['level'], ref.levels(n, rows, nbr, mask)), (name, 'plan levels != definition')
        U = np.zeros((n, B))
        sweeps = np.zeros(B, dtype=np.int64)
        hist = []
        for b in range(B):
            val = np.ascontiguousarray(vals[:, b])
            u, done, printed = reference_column(G, ind, val, weighted, tol, T, alpha, beta)
            for levelled in (False, True):
                u2, done2, errs2 = ref.host_sweeps(lib, n, rows, nbr, V, ind, val, weighted, alpha, beta, T, tol, levelled)
                assert u2.tobytes() == u.tobytes() and done2 == done, (name, b, 'host restatement != reference', levelled)
                assert ['%.15f' % e for e in errs2] == ['%.15f' % e for e in printed], (name, b, 'error history != printed')
            forms = ref.python_forms_fit(done, len(nbr), plan['nlevels'], weighted)
            for form, fn in (('sequential', ref.sequential), ('levelled', ref.levelled)):
                if form in forms:
                    u3, done3, errs3 = fn(n, rows, nbr, V, ind, val, weighted, alpha, beta, T, tol)
                    assert u3.tobytes() == u.tobytes() and done3 == done and errs3 == errs2, (name, b, form + ' != reference')
            U[:, b], sweeps[b] = u, done
            hist.append(np.array(errs2))
        H = np.full((int(sweeps.max()), B), np.nan)
        for b in range(B):
            H[:sweeps[b], b] = hist[b]
        if bd[0] == 'labels':
            assert len(set(sweeps.tolist())) > 1, (name, 'the per-class stop sweeps are all equal')
        small_only = bool(np.all(plan['launches'][:, 2] == 1))
        print('case %-13s %-9s B=%d weighted=%d tol=%g T=%d alpha=%.3g levels=%d launches=%d all-small=%d sweeps=%s' % (
            name, gname, B, weighted, tol, T, alpha, plan['nlevels'], len(plan['launches']), small_only, sweeps.tolist()))
        cases.append((name, {name + '_ind': ind.astype(np.int32), name + '_vals': vals, name + '_u': U, name + '_sweeps': sweeps,
                             name + '_errs': H, name + '_levels': np.int64(plan['nlevels'])}))

    # ssl.amle on the blobs graph, unweighted and weighted, with and without class priors: the reference's own fit_predict
    W = graphs['blobs']
    for tag, weighted in (('u', False), ('w', True)):
        for ptag, kw in (('plain', {}), ('priors', {'class_priors': fits['fit_priors']})):
            model = gl.ssl.amle(W, weighted=weighted, **kw)
            pred = model.fit_predict(train_ind, lab[train_ind])
            key = 'fit_%s_%s' % (tag, ptag)
            fits[key + '_pred'] = np.asarray(pred).astype(np.int64)
            case = 'blobs_%s_3' % tag              # the learner's defaults (tol 1e-3, max_num_it 1e5): `prob` is that case's u, stored once
            got = dict(cases)[case][case + '_u']
            assert np.asarray(model.prob, dtype=np.float64).tobytes() == got.tobytes(), (key, 'the fit is not the case of the same arguments')
            print('fit %-9s accuracy %.2f%%  name=%r file=%r' % (key, gl.ssl.ssl_accuracy(pred, lab, train_ind), model.name,
                                                                 model.get_accuracy_filename()))
    cases.append(('fit', fits))

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
    names = ['g15_amle.npz'] + ['g15_amle_%d.npz' % i for i in range(2, len(files) + 1)]
    files[0]['entry_names'] = np.array(sorted(where))
    files[0]['entry_files'] = np.array([names[where[c]] for c in sorted(where)])
    for fn, arrs in zip(names, files):
        path = os.path.join(HERE, fn)
        np.savez_compressed(path, **arrs)
        print(fn, os.path.getsize(path), 'bytes')
        assert os.path.getsize(path) <= 1024 * 1024, fn


if __name__ == '__main__':
    main()
