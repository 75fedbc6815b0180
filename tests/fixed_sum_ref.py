"""The fixed-order column sum of csrc/fixed_sum.h restated in numpy, one addition at a time, for
tests/test_fixed_sum_host.py and tests/test_mmbo_host.py, and the header compiled for the host behind tests/fixed_sum_host.cpp."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 64           # FS_ROWS and FS_CHAINS of fixed_sum.h


def tree(a):
    """a (64, ...) -> (...): a[r] += a[r + h] for r < h, h = 32 .. 1"""
    a = np.array(a, dtype=np.float64, copy=True)
    assert a.shape[0] == ROWS
    h = ROWS // 2
    while h >= 1:
        a[:h] = a[:h] + a[h:2 * h]
        h //= 2
    return a[0]


def finish(part):
    """part (P, ...) -> (...): chain q adds the partials q, q + 64, .. in ascending order from +0.0, then the tree over the chains"""
    chains = np.zeros((ROWS,) + part.shape[1:])
    for p in range(part.shape[0]):
        chains[p % ROWS] = chains[p % ROWS] + part[p]
    return tree(chains)


def build_host_lib(tmp):
    """csrc/fixed_sum.h compiled for the host: `g++ -O2 -ffp-contract=off` behind tests/fixed_sum_host.cpp."""
    so = os.path.join(str(tmp), 'libfixed_sum_host.so')
    subprocess.run(['g++', '-O2', '-ffp-contract=off', '-std=c++17', '-fPIC', '-shared', '-I' + os.path.join(ROOT, 'graphlearning_amd', 'csrc'),
                    '-o', so, os.path.join(ROOT, 'tests', 'fixed_sum_host.cpp')], check=True)
    lib = ctypes.CDLL(so)
    vp, i64, f64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
    lib.fs_host_constants.argtypes = [vp]
    lib.fs_host_constants.restype = None
    lib.fs_host_partials.argtypes = [i64]
    lib.fs_host_partials.restype = i64
    lib.fs_host_tree64.argtypes = [vp, ctypes.c_int]
    lib.fs_host_tree64.restype = f64
    lib.fs_host_tree_dot.argtypes = [vp, vp, i64, i64]
    lib.fs_host_tree_dot.restype = f64
    lib.fs_host_finish.argtypes = [vp, i64, ctypes.c_int, vp]
    lib.fs_host_finish.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_tree64(lib, v):
    v = np.ascontiguousarray(v, dtype=np.float64)
    return lib.fs_host_tree64(_p(v), len(v))


def host_tree_dot(lib, x, y, p):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return lib.fs_host_tree_dot(_p(x), _p(y), len(x), p)


def host_finish(lib, part):
    part = np.ascontiguousarray(part, dtype=np.float64)
    S = np.empty(part.shape[1])
    lib.fs_host_finish(_p(part), part.shape[0], part.shape[1], _p(S))
    return S
