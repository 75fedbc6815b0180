"""The fixed-order column sum by itself, without a device: csrc/fixed_sum.h compiled for the host against the numpy restatement of
tests/fixed_sum_ref.py BIT FOR BIT, on data whose sum depends on the order -- uniform(-1, 1) values scaled by random powers of two
over about 40 binades -- with a check that the order is visible at all: the restatement differs from a plain ascending sum."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import fixed_sum_ref as ref  # noqa: E402

PARTIALS = (1, 2, 63, 64, 65, 127, 128, 129, 200)
COLUMNS = (1, 15, 16, 17, 33)


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return ref.build_host_lib(tmp_path_factory.mktemp('fixed_sum'))


def wide_data(seed, shape):
    rng = np.random.default_rng(2100 + seed)
    return rng.uniform(-1, 1, size=shape) * 2.0 ** rng.integers(-20, 21, size=shape)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def ascending_sum(part):
    s = np.zeros(part.shape[1:])
    for p in range(part.shape[0]):
        s = s + part[p]
    return s


def test_constants_and_partials(lib):
    out = np.zeros(3, dtype=np.int32)
    lib.fs_host_constants(out.ctypes.data)
    assert out.tolist() == [64, 64, 16] and ref.ROWS == 64
    for n in (1, 2, 63, 64, 65, 128, 129, 4096, 4097, 70000, (1 << 31) - 1):
        assert lib.fs_host_partials(n) == -(-n // 64), n


@pytest.mark.parametrize('P', PARTIALS)
def test_finish_bit_for_bit(lib, P):
    for nq in COLUMNS:
        part = wide_data(1000 * P + nq, (P, nq))
        got, want = ref.host_finish(lib, part), ref.finish(part)
        print((P, nq), 'differing values', int((got != want).sum()), 'that differ from the ascending sum', int((want != ascending_sum(part)).sum()))
        assert same_bits(got, want), (P, nq)


def test_the_order_is_visible():
    """were the restatement equal to a plain ascending sum on every input, a header that added in the wrong order would pass"""
    differing = {(P, nq): int((ref.finish(part) != ascending_sum(part)).sum())
                 for P in PARTIALS for nq in COLUMNS for part in [wide_data(1000 * P + nq, (P, nq))]}
    print(differing)
    assert differing[(1, 1)] == 0 and differing[(2, 33)] == 0          # (one or two partials: one addition at the most, no order)
    assert any(differing.values())
    # and the chains matter, not only the tree: with more than 64 partials the result differs from the tree over an ascending sum of
    # the first 64 and of the rest, somewhere
    part = wide_data(7, (129, 33))
    halves = np.zeros((64, 33))
    halves[0], halves[1] = ascending_sum(part[:64]), ascending_sum(part[64:])
    assert (ref.finish(part) != ref.tree(halves)).any()


@pytest.mark.parametrize('live', [1, 63, 64])
def test_tree_bit_for_bit(lib, live):
    for seed in range(8):
        v = wide_data(50 * live + seed, (live,))
        pad = np.zeros(64)
        pad[:live] = v
        got, want = ref.host_tree64(lib, v), ref.tree(pad)
        assert same_bits(got, want), (live, seed)
        if live == 1:
            assert same_bits(got, v[0])
    differing = sum(bool(ref.tree(wide_data(50 * 64 + seed, (64,))) != ascending_sum(wide_data(50 * 64 + seed, (64,)))) for seed in range(8))
    assert differing > 0


@pytest.mark.parametrize('n', [1, 63, 64, 65, 130])
def test_tree_dot_bit_for_bit(lib, n):
    """partial p of x . y: every product rounded on its own, rows past n count as +0.0"""
    x, y = wide_data(n, (n,)), wide_data(n + 500, (n,))
    for p in range(-(-n // 64)):
        pad = np.zeros(64)
        rows = slice(64 * p, min(n, 64 * p + 64))
        pad[:rows.stop - rows.start] = x[rows] * y[rows]
        assert same_bits(ref.host_tree_dot(lib, x, y, p), ref.tree(pad)), (n, p)


def test_the_header_is_host_only_and_the_only_definition():
    csrc = os.path.join(ROOT, 'graphlearning_amd', 'csrc')
    with open(os.path.join(csrc, 'fixed_sum.h')) as f:
        text = f.read()
    assert 'hip' not in re.sub(r'//.*', '', text).lower()                              # no HIP header
    for name in ('ck_plan.h', 'eig_plan.h', 'mmbo_plan.h'):
        with open(os.path.join(csrc, name)) as f:
            plan = f.read()
        assert '#include "fixed_sum.h"' in plan and not re.search(r'ck_tree64|ck_finish\b|CK_CHAINS|CK_ROWS', plan), name
    with open(os.path.join(csrc, 'fixed_sum_device.h')) as f:
        dev = f.read()
    assert dev.count('#pragma clang fp contract(off)') == 2 and '#include "fixed_sum.h"' in dev      # one per function with arithmetic
    for name in ('ck.hip', 'eig.hip', 'mmbo.hip'):
        with open(os.path.join(csrc, name)) as f:
            kern = f.read()
        assert '#include "fixed_sum_device.h"' in kern and 'fs_finish_cols(' in kern, name
        assert not re.search(r'p \+= \w*CHAINS', kern), name                           # the chain loop lives in the two headers alone
