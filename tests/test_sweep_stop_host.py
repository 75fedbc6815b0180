"""The stop test of the Poisson sweeps without a device: csrc/sweep_stop_plan.h compiled for the host (tests/sweep_stop_host.cpp).

The test plays the device.  Group b is given its stop values e_b[t]; sweep t of group b runs iff t < min_iter or the row err[t] it
reads says e_b[t] > thresh, and a sweep that runs adds e_b[t + 1] to row t + 1 by a maximum over bit patterns (so the row must have
been cleared: rows start out poisoned); a sweep that does not run leaves the row as the driver put it.  The walk is driven through
exactly the reads of glx_sweep_tail (csrc/sweep_core.hip) -- row t in front of a chunk, rows t + 1 .. end behind it -- and its T_b,
stopped_b, first tested sweep, tested count, compared values and final buffer parity are held against a plain
`while (t < min_iter or e[t] > thresh) and t < max_iter` per group."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESH = 1.0 / 1024
MIN_ITER, MAX_ITER = 3, 60
POISON = int(np.array([1e300]).view(np.uint64)[0])      # an uncleared row reads as a value far above the threshold


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp('sweep_stop')), 'libsweep_stop_host.so')
    subprocess.run(['g++', '-O2', '-ffp-contract=off', '-std=c++17', '-fPIC', '-shared', '-I' + os.path.join(ROOT, 'graphlearning_amd', 'csrc'),
                    '-o', so, os.path.join(ROOT, 'tests', 'sweep_stop_host.cpp')], check=True)
    lib = ctypes.CDLL(so)
    vp, ci, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.ssw_constants.argtypes, lib.ssw_constants.restype = [vp], None
    lib.ssw_stop_value.argtypes, lib.ssw_stop_value.restype = [vp, ci], dbl
    lib.ssw_stop_bits.argtypes, lib.ssw_stop_bits.restype = [dbl], ctypes.c_uint64
    lib.ssw_new.argtypes, lib.ssw_new.restype = [], vp
    lib.ssw_free.argtypes, lib.ssw_free.restype = [vp], None
    lib.ssw_start.argtypes, lib.ssw_start.restype = [vp, ci, ci, ci, ci, dbl], None
    lib.ssw_test.argtypes, lib.ssw_test.restype = [vp, ci, vp, ci], None
    for name, args in (('head', [vp]), ('running', [vp]), ('chunk_end', [vp, ci]), ('finish', [vp]), ('T', [vp, ci]), ('stopped', [vp, ci]),
                       ('tested_count', [vp, ci]), ('parity', [ci])):
        fn = getattr(lib, 'ssw_' + name)
        fn.argtypes, fn.restype = args, ci
    out = np.zeros(2, dtype=np.int32)
    lib.ssw_constants(out.ctypes.data)
    assert out.tolist() == [16, 32]
    return lib


def _value(shards):
    """The maximum of the bit patterns as a double, in numpy."""
    return float(np.array([shards.max()], dtype=np.uint64).view(np.float64)[0])


def _plain(e, min_iter, max_iter):
    """(T, stopped, first, the values compared) of one group."""
    t = 0
    while (t < min_iter or e[t] > THRESH) and t < max_iter:
        t += 1
    first = min(min_iter, max_iter)
    stopped = t < max_iter      # the value at t = max_iter is never compared
    return t, stopped, first, [e[q] for q in range(first, t + (1 if stopped else 0))]


class Device:
    def __init__(self, lib, E, B, used, min_iter, max_iter, nshards):
        self.E, self.B, self.used, self.min_iter, self.max_iter, self.nshards = E, B, used, min_iter, max_iter, nshards
        self.err = np.full((max_iter + 2, B, nshards), POISON, dtype=np.uint64)
        self.buffer = 0           # the ping-pong buffer written last
        self.launched = 0
        # the head (glx_sweep_head_rows and the callers' unconditional sweeps): row `head` cleared, row 0 = err0 when min_iter = 0
        head = min(min_iter, max_iter)
        self.err[head] = 0
        if min_iter == 0:
            for b in range(B):
                self.err[0, b, 0] = lib.ssw_stop_bits(float(E[b][0]))
        for t in range(head):
            self.sweep(t)

    def sweep(self, t):
        assert t == self.launched and t < self.max_iter      # every sweep once, in order
        self.launched += 1
        ran = False
        for b in range(self.used):
            if t >= self.min_iter and not (_value(self.err[t, b]) > THRESH):
                continue
            ran = True
            if t + 1 >= self.min_iter:
                e = np.array([self.E[b][t + 1], 0.5 * self.E[b][t + 1]]).view(np.uint64)
                k = (7 * t + 3 * b) % self.nshards        # the maximum sits in the first, a middle or the last shard in turn
                k = (0, k, self.nshards - 1)[t % 3]
                for shard, v in ((k, e[0]), ((k + 1) % self.nshards, e[1])):
                    self.err[t + 1, b, shard] = max(self.err[t + 1, b, shard], v)
        if ran:
            self.buffer = (t + 1) & 1


def _drive(lib, E, B, used, min_iter, max_iter, nshards):
    dev = Device(lib, E, B, used, min_iter, max_iter, nshards)
    mirror = np.full_like(dev.err, POISON)
    if min_iter == 0:
        mirror[0] = dev.err[0]
    w = lib.ssw_new()
    lib.ssw_start(w, B, used, min_iter, max_iter, THRESH)
    head = lib.ssw_head(w)
    assert head == min(min_iter, max_iter)
    t = head
    while t < max_iter and lib.ssw_running(w):
        mirror[t] = dev.err[t]
        lib.ssw_test(w, t, mirror[t].ctypes.data, nshards)
        if not lib.ssw_running(w):
            break
        end, t0 = lib.ssw_chunk_end(w, t), t
        assert t0 < end <= min(max_iter, t0 + 16)
        dev.err[t0 + 1:end + 1] = 0
        for t in range(t0, end):
            dev.sweep(t)
        t = end
        mirror[t0 + 1:end + 1] = dev.err[t0 + 1:end + 1]
        for q in range(t0 + 1, end):
            lib.ssw_test(w, q, np.ascontiguousarray(mirror[q]).ctypes.data, nshards)
    T_max = lib.ssw_finish(w)
    assert not lib.ssw_running(w)
    got = []
    for b in range(B):
        count = lib.ssw_tested_count(w, b)
        vals = [lib.ssw_stop_value(np.ascontiguousarray(mirror[head + i, b]).ctypes.data, nshards) for i in range(count)]
        got.append((lib.ssw_T(w, b), bool(lib.ssw_stopped(w, b)), head, vals))
    parity = lib.ssw_parity(T_max)
    lib.ssw_free(w)
    return got, T_max, parity, dev


def _check(lib, E, B, used, min_iter=MIN_ITER, max_iter=MAX_ITER, nshards=16):
    got, T_max, parity, dev = _drive(lib, E, B, used, min_iter, max_iter, nshards)
    want = [_plain(E[b], min_iter, max_iter) for b in range(used)]
    for b in range(used):
        T, stopped, first, vals = got[b]
        assert (T, stopped, first) == want[b][:3], (b, got[b], want[b])
        assert len(vals) == len(want[b][3]) == max(0, T - first + stopped), (b, vals, want[b][3])
        assert np.array_equal(np.array(vals), np.array(want[b][3]), equal_nan=True), (b, vals, want[b][3])
    for b in range(used, B):      # idle: no sweep, nothing tested
        assert got[b] == (0, False, min(min_iter, max_iter), []), (b, got[b])
    assert T_max == max([min(min_iter, max_iter)] + [w[0] for w in want])
    assert parity == T_max & 1 == dev.buffer, (parity, T_max, dev.buffer)      # the device's last write went to the buffer that holds u_T
    return [w[0] for w in want]


def _seq(stop, at=0.0, max_iter=MAX_ITER):
    """1 everywhere but at `stop`: a sweep that ran on behind its stop would find a value above the threshold again."""
    e = np.ones(max_iter + 2)
    if stop is not None:
        e[stop] = at
    return e


HEAD = MIN_ITER
STOPS = [HEAD, HEAD + 1, HEAD + 15, HEAD + 16, HEAD + 17, HEAD + 32, MAX_ITER - 1, MAX_ITER, None]


@pytest.mark.parametrize('stop', STOPS)
def test_single_form_stops_where_the_plain_loop_stops(lib, stop):
    T = _check(lib, [_seq(stop)], 1, 1, nshards=64)
    assert T == [MAX_ITER if stop is None else stop]


@pytest.mark.parametrize('B', [2, 5, 32])
def test_groups_stop_each_at_their_own_sweep(lib, B):
    """used < B; every stop position in every group's place in turn; neighbours stop in different chunks."""
    used = B - 1
    seen = set()
    for shift in range(len(STOPS)):
        stops = [STOPS[(shift + 2 * b) % len(STOPS)] for b in range(B)]
        E = [_seq(s) for s in stops]
        T = _check(lib, E, B, used)
        assert T == [MAX_ITER if s is None else s for s in stops[:used]]
        seen.update(stops[:used])
    assert seen == set(STOPS)
    chunks = {(s - HEAD) // 16 for s in STOPS if s is not None}
    assert chunks >= {0, 1, 2, 3}


def test_iteration_bounds(lib):
    for nshards, B, used in ((64, 1, 1), (16, 5, 3)):
        # min_iter = 0 and the start at or below the threshold: no sweep, one value tested
        for at in (THRESH, 0.25 * THRESH, 0.0):
            got, T_max, parity, dev = _drive(lib, [_seq(0, at)] * B, B, used, 0, MAX_ITER, nshards)
            assert all(g == (0, True, 0, [at]) for g in got[:used]) and T_max == 0 and parity == 0 and dev.launched == 0
            _check(lib, [_seq(0, at)] * B, B, used, min_iter=0, nshards=nshards)
        assert _check(lib, [_seq(9)] * B, B, used, min_iter=0, nshards=nshards) == [9] * used      # no unconditional head
        # min_iter = max_iter and min_iter > max_iter: nothing is compared
        for min_iter, max_iter in ((7, 7), (9, 7)):
            E = [_seq(3, max_iter=max_iter)] * B
            got, T_max, parity, dev = _drive(lib, E, B, used, min_iter, max_iter, nshards)
            assert all(g == (max_iter, False, max_iter, []) for g in got[:used]) and T_max == max_iter and dev.launched == max_iter
            _check(lib, E, B, used, min_iter=min_iter, max_iter=max_iter, nshards=nshards)
        # max_iter reached: the value at t = max_iter is never compared
        got, T_max, _, _ = _drive(lib, [_seq(10, max_iter=10)] * B, B, used, 3, 10, nshards)
        assert all(g == (10, False, 3, [1.0] * 7) for g in got[:used])


def test_equality_stops_and_infinity_runs_on(lib):
    assert _check(lib, [_seq(HEAD + 5, THRESH)], 1, 1, nshards=64) == [HEAD + 5]
    assert _check(lib, [_seq(HEAD + 5, np.nextafter(THRESH, 1.0))], 1, 1, nshards=64) == [MAX_ITER]
    e = _seq(None)
    e[HEAD + 2:] = np.inf
    got, _, _, _ = _drive(lib, [e], 1, 1, MIN_ITER, MAX_ITER, 64)
    assert got[0][0] == MAX_ITER and not got[0][1] and np.all(np.isposinf(got[0][3][2:])) and len(got[0][3]) == MAX_ITER - HEAD
    _check(lib, [e], 1, 1, nshards=64)
    # groups: equality in one, infinity in the next
    assert _check(lib, [_seq(HEAD + 20, THRESH), e, _seq(HEAD + 1)], 3, 3) == [HEAD + 20, MAX_ITER, HEAD + 1]


@pytest.mark.parametrize('where', [HEAD, HEAD + 7, HEAD + 16])
def test_nan_in_one_group_stops_that_group_alone(lib, where):
    stops = [HEAD + 33, None, HEAD + 2, HEAD + 18, None]
    E = [_seq(s) for s in stops]
    E[1] = _seq(where, np.nan)
    T = _check(lib, E, 5, 5)
    assert T == [HEAD + 33, where, HEAD + 2, HEAD + 18, MAX_ITER]
    got, _, _, _ = _drive(lib, E, 5, 5, MIN_ITER, MAX_ITER, 16)
    assert np.isnan(got[1][3][-1]) and got[1][1]
    # the start value itself (min_iter = 0), beside running groups
    E[1] = _seq(0, np.nan)
    assert _check(lib, E, 5, 5, min_iter=0) == [HEAD + 33, 0, HEAD + 2, HEAD + 18, MAX_ITER]


def test_stop_value_and_stop_bits(lib):
    def bits(x):
        return int(np.array([x], dtype=np.float64).view(np.uint64)[0])

    rng = np.random.default_rng(3)
    for nshards in (16, 64):
        for at in (0, nshards // 2 - 1, nshards - 1):
            for top in (3.5, THRESH, np.inf, 5e-324, 0.0):
                row = (rng.random(nshards) * min(top, 1.0)).view(np.uint64).copy()
                row[at] = bits(top)
                got = lib.ssw_stop_value(row.ctypes.data, nshards)
                assert got == top == _value(row), (nshards, at, top, got)
            # a NaN sorts above every number, +inf included, wherever it sits; a NaN with the sign bit set above that
            row = np.full(nshards, bits(np.inf), dtype=np.uint64)
            row[at] = bits(np.nan)
            assert np.isnan(lib.ssw_stop_value(row.ctypes.data, nshards))
            row[(at + 1) % nshards] = 0xfff8000000000000
            assert np.isnan(lib.ssw_stop_value(row.ctypes.data, nshards))
    assert lib.ssw_stop_value(np.zeros(16, dtype=np.uint64).ctypes.data, 16) == 0.0
    for x in (0.0, 5e-324, THRESH, 1.0, 1e300, np.inf):
        assert lib.ssw_stop_bits(x) == bits(x)
    for nan in (0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001, 0xffffffffffffffff):
        x = float(np.array([nan], dtype=np.uint64).view(np.float64)[0])
        assert np.isnan(x) and lib.ssw_stop_bits(x) == 0x7ff8000000000000
    # the canonical NaN still ends the loop and beats every number in a row of maxima
    row = np.array([bits(np.inf), lib.ssw_stop_bits(float('nan'))], dtype=np.uint64)
    assert np.isnan(lib.ssw_stop_value(row.ctypes.data, 2)) and not (lib.ssw_stop_value(row.ctypes.data, 2) > THRESH)
