"""The decisions of the weight-matrix assembly without a device: csrc/assemble_plan.h compiled for the host
(tests/assemble_plan_host.cpp) -- which merge kernel a row belongs to, the hub scratch, the rows' slots in the scratch image, the
sort key, and the per-column rule BIT FOR BIT against the reference's scipy expressions (_given_ref of tests/test_gpu_wide_graph.py)
on lists with duplicates, a self entry away from column 0, weights over 40 binades and exact zeros."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

REGISTER, WAVEFRONT, HUB = 0, 1, 2
SYM = {'none': 0, 'mean': 1, 'max': 2, 'symgauss': 3}


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp('assemble_plan')), 'libassemble_plan_host.so')
    subprocess.run(['g++', '-O2', '-ffp-contract=off', '-std=c++17', '-fPIC', '-shared', '-I' + os.path.join(ROOT, 'graphlearning_amd', 'csrc'),
                    '-o', so, os.path.join(ROOT, 'tests', 'assemble_plan_host.cpp')], check=True)
    lib = ctypes.CDLL(so)
    vp, i64, u32, u64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64
    lib.asm_host_constants.argtypes = [vp]
    lib.asm_host_constants.restype = None
    lib.asm_host_row_class.argtypes = [ctypes.c_int, i64]
    lib.asm_host_row_class.restype = ctypes.c_int
    lib.asm_host_hub_scratch.argtypes = [i64]
    lib.asm_host_hub_scratch.restype = i64
    lib.asm_host_row_slot.argtypes = [i64, ctypes.c_int, ctypes.c_int, i64]
    lib.asm_host_row_slot.restype = i64
    lib.asm_host_key.argtypes = [u32, u32, u32, u32]
    lib.asm_host_key.restype = u64
    lib.asm_host_unpack.argtypes = [u64, vp]
    lib.asm_host_unpack.restype = None
    lib.asm_host_assemble.argtypes = [vp, vp, i64, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
    lib.asm_host_assemble.restype = i64
    return lib


def test_row_classes_and_hub_scratch(lib):
    import test_gpu_wide_graph as wide
    out = np.zeros(3, dtype=np.int32)
    lib.asm_host_constants(out.ctypes.data)
    assert out.tolist() == [64, 1024, 2048]
    assert out[1] == wide.ROW_CAP and out[2] == wide.HUB_FLOOR           # what the GPU tests' censuses are counted against
    assert [lib.asm_host_row_class(32, M) for M in (63, 64, 65)] == [REGISTER, REGISTER, WAVEFRONT]
    assert [lib.asm_host_row_class(64, M) for M in (64, 65)] == [REGISTER, WAVEFRONT]
    assert [lib.asm_host_row_class(65, M) for M in (63, 64, 65)] == [WAVEFRONT] * 3      # lists too long for one entry per lane
    for k in (1, 32, 64, 65, 512, 1024):
        assert [lib.asm_host_row_class(k, M) for M in (1023, 1024, 1025)] == [WAVEFRONT, WAVEFRONT, HUB], k
    assert lib.asm_host_row_class(2000, 2000) == HUB and lib.asm_host_row_class(10, 1 << 40) == HUB
    assert [lib.asm_host_hub_scratch(M) for M in (1025, 2047, 2048, 2049, 4096, 4097)] == [2048, 2048, 2048, 4096, 4096, 8192]
    assert lib.asm_host_hub_scratch((1 << 31) + 1) == 1 << 32


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_rows_slots_tile_the_scratch_image(lib, seed):
    """Row i keeps its candidates at [slot, slot + M) of the scratch image: disjoint, and inside what each entry point allocates --
    2 n k for the whole matrix (n k reverse entries), m k + n_rev for a block that received n_rev tuples."""
    rng = np.random.default_rng(700 + seed)
    n, k = 300, int(rng.integers(1, 70))
    whole = np.bincount(rng.integers(0, n, size=n * k), minlength=n)          # every list entry names some row
    whole[5] += whole[9]                                                      # (one popular row, one nobody names)
    whole[9] = 0
    block = rng.integers(0, 3 * k, size=n) * (rng.random(n) < 0.7)
    for rcnt, image in ((whole, 2 * n * k), (block, n * k + int(block.sum()))):
        roff = np.concatenate([[0], np.cumsum(rcnt)])
        for sym in (0, 1, 2, 3):
            slot = np.array([lib.asm_host_row_slot(i, k, sym, int(roff[i])) for i in range(n)])
            M = k + (rcnt if sym else np.zeros_like(rcnt))
            assert slot[0] == 0 and np.all(slot[1:] >= slot[:-1] + M[:-1]), sym
            assert slot[-1] + M[-1] <= image, sym
    assert lib.asm_host_row_slot((1 << 31) - 2, 1, 1, 1 << 31) == (1 << 32) - 2           # 64-bit


def _tuples(rng, count):
    col = rng.integers(0, 1 << 31, size=count)
    col[:8] = [0, 0, (1 << 31) - 1, (1 << 31) - 1, 1, 1, 1 << 30, 1 << 30]
    kind = rng.integers(0, 2, size=count)
    pos = rng.integers(0, 1 << 16, size=count)
    pos[::3] = rng.choice([0, 65535], size=len(pos[::3]))
    col[200:400] = col[200]                                                 # many entries of one column: kind and position decide
    pos[300:400] = pos[300]
    kind[300:350], kind[350:400] = 0, 1
    return col, kind, pos, rng.integers(0, 64, size=count)


def test_keys_order_as_their_tuples(lib):
    rng = np.random.default_rng(11)
    col, kind, pos, lane = _tuples(rng, 1000)
    key = np.array([lib.asm_host_key(int(c), int(t), int(p), int(l)) for c, t, p, l in zip(col, kind, pos, lane)], dtype=np.uint64)
    out = np.zeros(4, dtype=np.uint32)
    for j in range(len(key)):
        lib.asm_host_unpack(int(key[j]), out.ctypes.data)
        assert out.tolist() == [col[j], kind[j], pos[j], lane[j]], j
    assert np.all(key < np.uint64(0xffffffffffffffff))                     # the padding key sorts last
    for lanes in (lane, np.zeros_like(lane), rng.integers(0, 64, size=len(lane))):
        k2 = np.array([lib.asm_host_key(int(c), int(t), int(p), int(l)) for c, t, p, l in zip(col, kind, pos, lanes)], dtype=np.uint64)
        a, b = rng.integers(0, len(key), size=(2, 20000))
        a = np.concatenate([a, np.arange(200, 399)])                        # neighbours inside the one-column run too
        b = np.concatenate([b, np.arange(201, 400)])
        ta, tb = np.stack([col[a], kind[a], pos[a]]), np.stack([col[b], kind[b], pos[b]])
        differ = np.any(ta != tb, axis=0)
        first = np.argmax(ta != tb, axis=0)
        less = np.take_along_axis(ta, first[None], 0)[0] < np.take_along_axis(tb, first[None], 0)[0]
        assert np.array_equal((k2[a] < k2[b])[differ], less[differ])
        assert np.array_equal((k2[a] > k2[b])[differ], ~less[differ])
        order = np.lexsort((lanes, pos, kind, col))
        assert np.array_equal(np.sort(k2), k2[order])


def _lists(n, K, seed):
    """Distinct neighbours inside a row, except that every fourth row lists one neighbour twice (never three times: with three
    different weights on one edge scipy's own order of the sum is an accident of its sort); one self entry away from column 0.
    Weights uniform(0, 1) scaled by 2^[-20, 20], a tenth of them exactly 0."""
    rng = np.random.default_rng(9000 + seed)
    ind = np.stack([rng.choice(n, size=K, replace=False) for _ in range(n)]).astype(np.int64)
    ind[::4, K - 1] = ind[::4, 1]
    row = ind[7]
    if 7 in row:
        at = int(np.flatnonzero(row == 7)[0])
        row[at], row[2] = row[2], row[at]
    else:
        row[2] = 7
    assert ind[7, 2] == 7 and ind[7, 0] != 7
    assert max(np.bincount(r).max() for r in ind) == 2 and sum(len(set(r.tolist())) < K for r in ind) == n // 4
    w = rng.random((n, K)) * 2.0 ** rng.integers(-20, 21, size=(n, K))
    w[rng.random((n, K)) < 0.1] = 0.0
    return ind, w


@pytest.mark.parametrize('K', [5, 40])
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_the_rule_bit_for_bit_against_scipy(lib, K, seed):
    from oracle import gl_oracle as orc
    from test_gpu_wide_graph import _given_ref
    n = 200
    ind, w = _lists(n, K, seed)
    assert np.sum(w == 0) > n * K // 20 and np.log2(w[w > 0].max() / w[w > 0].min()) > 35
    lanes = np.random.default_rng(seed).integers(0, 256, size=2 * n * K).astype(np.uint8)
    for rule, sym in SYM.items():
        indptr = np.zeros(n + 1, dtype=np.int32)
        indices = np.zeros(2 * n * K, dtype=np.int32)
        data = np.zeros(2 * n * K)
        nnz = lib.asm_host_assemble(ind.ctypes.data, w.ctypes.data, n, K, sym, lanes.ctypes.data, indptr.ctypes.data, indices.ctypes.data,
                                    data.ctypes.data)
        Wo = _given_ref(orc, ind, w, rule)
        assert nnz == Wo.nnz and np.array_equal(indptr, Wo.indptr), (rule, K, seed)
        assert np.array_equal(indices[:nnz], Wo.indices), (rule, K, seed)
        assert data[:nnz].tobytes() == np.ascontiguousarray(Wo.data, dtype=np.float64).tobytes(), (rule, K, seed)
        assert not np.any(indices[:nnz] == np.repeat(np.arange(n), np.diff(indptr))) and np.all(data[:nnz] != 0)
