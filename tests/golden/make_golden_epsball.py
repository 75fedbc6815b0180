#!/usr/bin/env python3
"""Generate the epsilon-ball golden fixtures tests/golden/g13_epsball*.npz by IMPORTING THE REFERENCE.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONPATH=<the reference's checkout> PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg \
        python3 tests/golden/make_golden_epsball.py        (from the repository root)

Captured with Python 3.10.12, numpy 2.2.6, scipy 1.15.3, reference graphlearning 1.7.5.  The files hold inputs and the
reference's outputs (data only): per case X (and F), epsilon, `indptr` / `indices` once and `data` per stored kernel; where a
kernel drops zeros (`distance` between duplicate points) that structure is stored too.  The cases are spread over several files
so that each stays below the repository's limit for a committed file; g13_epsball.npz lists which file holds which case.
"""
import os
import sys
import numpy as np
from scipy import sparse

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import graphlearning as gl                      # the REFERENCE (PYTHONPATH=/root/reference)
import epsball_ref as ref                       # the restatement, cross-checked below

assert gl.__file__.startswith('/root/reference'), gl.__file__

LIMIT = 1000000      # bytes per file


def same(A, B):
    A, B = sparse.csr_matrix(A), sparse.csr_matrix(B)
    A.sort_indices()
    B.sort_indices()
    return (A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
            and A.data.tobytes() == B.data.tobytes())


def case_arrays(name, X, eps, F, eps_f):
    out = {name + '_X': X, name + '_eps': np.float64(eps)}
    if F is not None:
        out[name + '_F'] = F
        out[name + '_eps_f'] = np.float64(eps_f)
    base = None
    for kernel in ref.KERNELS:
        with np.errstate(all='ignore'):
            W = sparse.csr_matrix(gl.weightmatrix.epsilon_ball(X, eps, kernel=kernel, features=F, epsilon_f=eps_f))
        W.sort_indices()
        with np.errstate(all='ignore'):
            assert same(W, ref.epsilon_ball(X, eps, kernel=kernel, features=F, epsilon_f=eps_f)), (name, kernel)
        if kernel == 'uniform':
            base = W
            out[name + '_indptr'] = W.indptr.astype(np.int32)
            out[name + '_indices'] = W.indices.astype(np.int32)
            print('%-10s n=%d d=%d eps=%g entries=%d degrees %d..%d' % (name, X.shape[0], X.shape[1], eps, W.nnz,
                                                                        np.diff(W.indptr).min() if W.nnz else 0,
                                                                        np.diff(W.indptr).max() if W.nnz else 0))
            continue
        stored = kernel == 'gaussian' or kernel in ref.GOLDEN_DATA_KERNELS.get(name, ())
        if not (np.array_equal(W.indptr, base.indptr) and np.array_equal(W.indices, base.indices)):
            print('   %s drops zeros: %d entries' % (kernel, W.nnz))
            assert stored, (name, kernel)
            out['%s_%s_indptr' % (name, kernel)] = W.indptr.astype(np.int32)
            out['%s_%s_indices' % (name, kernel)] = W.indices.astype(np.int32)
        if stored and W.nnz:
            out['%s_%s_data' % (name, kernel)] = W.data.astype(np.float64)
    return out


def main():
    cases = []
    for name, (X, eps, F, eps_f) in ref.golden_inputs().items():
        cases.append((name, case_arrays(name, X, eps, F, eps_f)))
    # the user-kernel case: a hat function on the integer grid -- the pairs at distance exactly epsilon get weight 0 and go
    X, eps, _, _ = ref.golden_inputs()['grid_int']
    W = sparse.csr_matrix(gl.weightmatrix.epsilon_ball(X, eps, eta=ref.eta_hat))
    W.sort_indices()
    assert same(W, ref.epsilon_ball(X, eps, eta=ref.eta_hat))
    print('eta        entries=%d smallest weight %g' % (W.nnz, W.data.min()))
    cases.append(('eta', {'eta_indptr': W.indptr.astype(np.int32), 'eta_indices': W.indices.astype(np.int32), 'eta_data': W.data}))

    # pack the cases into files below LIMIT (compressed size, measured)
    import io
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
    names = ['g13_epsball.npz'] + ['g13_epsball_%d.npz' % i for i in range(2, len(files) + 1)]
    files[0]['case_names'] = np.array(sorted(where))
    files[0]['case_files'] = np.array([names[where[c]] for c in sorted(where)])
    for fn, arrs in zip(names, files):
        path = os.path.join(HERE, fn)
        np.savez_compressed(path, **arrs)
        print(fn, os.path.getsize(path), 'bytes')
        assert os.path.getsize(path) <= 1024 * 1024, fn


if __name__ == '__main__':
    main()
