"""graphlearning_amd/csrc/cg_plan.h, the host arithmetic of the two conjugate-gradient solves (cg.hip, cg_fused.hip), built on the host
with no HIP header (tests/cg_plan_host.cpp): numpy's pairwise-summation tree against numpy itself, the per-system stop state against a
restatement here, the chunk lengths of the tolerance mode / the reduction forms of the reference-order mode / its first decision / the
limits against the table recorded from both solves as they stood before the plan was a header of its own (tests/golden/cg_plans.txt),
the layout of the staged upload, and the replay key."""
import hashlib
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'cg_plans.txt')
CG_LEN = (32, 16, 4)


@pytest.fixture(scope='module')
def driver():
    exe = os.path.join(tempfile.mkdtemp(), 'cg_plan_host')
    subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'graphlearning_amd', 'csrc'), '-o', exe,
                    os.path.join(ROOT, 'tests', 'cg_plan_host.cpp')], check=True)

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (args, r.returncode, r.stderr[-4000:])
        return r.stdout
    return run


# ---- 1. the pairwise plan against numpy itself ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 7, 8, 9, 15, 16, 127, 128, 129, 255, 256, 257, 1000, 4097, 8191, 8192, 8193, 8200, 16384, 16385, 24577,
                               70000, 100003])
def test_pairwise_plan_adds_as_numpy_does(driver, n):
    rows = [[int(v) for v in line.split()] for line in driver('pw', n).split('\n') if line]
    nl, ni, nlevels = rows[0]
    leaves, nodes = rows[1:1 + nl], rows[1 + nl:]
    assert len(nodes) == ni
    assert all(1 <= ln <= 128 for _, ln in leaves)
    assert leaves[0][0] == 0 and leaves[-1][0] + leaves[-1][1] == n
    assert all(a[0] + a[1] == b[0] for a, b in zip(leaves, leaves[1:]))                # the leaves tile [0, n) in order
    level = [0] * nl + [h for h, _, _ in nodes]
    assert level[nl:] == sorted(level[nl:]) and (ni == 0 or level[-1] == nlevels)
    for q, (h, l, r) in enumerate(nodes):
        assert 0 <= l < nl + q and 0 <= r < nl + q and level[l] < h and level[r] < h, (q, h, l, r)
    for seed in range(3):
        rng = np.random.default_rng(1000 * seed + n)
        a = rng.standard_normal(n) * np.exp(5 * rng.standard_normal(n))
        vals = [np.sum(a[off:off + ln]) for off, ln in leaves]                          # a run of at most 128 elements: numpy's own leaf
        for h in range(1, nlevels + 1):                                                 # level by level, as the device adds them
            done = len(vals)
            for hh, l, r in nodes[done - nl:]:
                if hh != h:
                    break
                assert l < done and r < done
                vals.append(vals[l] + vals[r])
        assert len(vals) == nl + ni
        assert vals[-1].tobytes() == np.sum(a).tobytes(), (n, seed)


# ---- 2. the stop state against a restatement ------------------------------------------------------------------------------------------
def stop_state(h, tol, chunk):
    """iters, err, done per system, running, the two latest maxima and the margin, from the rows of the history `h` (systems + 1
    columns) read `chunk` rows at a time: utils.conjgrad's `while err > tol` per system"""
    rows, stride = h.shape
    ng = stride - 1
    iters, err, done = [0] * ng, [1.0] * ng, [not (1.0 > tol)] * ng
    e_prev = e_last = 1.0
    margin = math.inf
    for it0 in range(0, rows, chunk):
        for q in range(it0, min(rows, it0 + chunk)):
            if all(done):
                break
            for g in range(ng):
                if done[g]:
                    continue
                iters[g], err[g] = q + 1, h[q, g]
                if tol > 0 and not math.isnan(err[g]):
                    margin = min(margin, abs(err[g] - tol) / tol)
                if not err[g] > tol:
                    done[g] = True
            e_prev, e_last = e_last, h[q, ng]
    return iters, err, done, done.count(False), e_prev, e_last, margin


@pytest.mark.parametrize('tol', [0.0, 1e-9, 0.5, 1.0, 2.0])
def test_stop_state(driver, tol):
    rng = np.random.default_rng(int(tol * 1e9) + 3)
    tmp = tempfile.mkdtemp()
    for case, ng in enumerate([1, 2, 3, 8, 32, 33] + list(rng.integers(1, 34, 6))):
        ng = int(ng)
        rows = int(rng.integers(1, 70))
        # residuals that fall at a rate of their own per system, not monotonically, and cross 1e-9 and 0.5 at different rows
        rate = rng.uniform(0.3, 0.95, ng)
        h = np.empty((rows, ng + 1))
        h[:, :ng] = rate ** np.arange(1, rows + 1)[:, None] * np.exp(0.5 * rng.standard_normal((rows, ng)))
        if case % 3 == 1:
            h[rng.integers(0, rows), rng.integers(0, ng)] = np.nan                      # stops its own system, the others run on
        if case % 3 == 2 and tol > 0:
            h[rng.integers(0, rows), rng.integers(0, ng)] = tol                          # err == tol stops
        h[:, ng] = np.max(np.where(np.isnan(h[:, :ng]), 0.0, h[:, :ng]), axis=1)     # (the maximum over the systems still running skips a NaN)
        path = os.path.join(tmp, 'h%d.bin' % case)
        h.tofile(path)
        for chunk, cut in [(8, rows), (1, rows), (rows, rows), (5, max(1, rows // 2))]:   # (cut: the history ends before the systems do)
            out = [line.split() for line in driver('stop', path, ng, float(tol).hex(), chunk, cut).split('\n') if line]
            iters, err, done, running, e_prev, e_last, margin = stop_state(h[:cut], tol, chunk)
            got = (int(out[0][0]),) + tuple(float.fromhex(v) for v in out[0][1:])
            want = (running, e_prev, e_last, margin)
            assert np.array_equal(np.array(got), np.array(want), equal_nan=True), (case, chunk, cut, got, want)
            for g in range(ng):
                it_g, err_g, done_g = int(out[1 + g][0]), float.fromhex(out[1 + g][1]), int(out[1 + g][2])
                assert (it_g, done_g) == (iters[g], int(done[g])), (case, chunk, cut, g)
                assert err_g == err[g] or (math.isnan(err_g) and math.isnan(err[g])), (case, chunk, cut, g)
            if not (1.0 > tol):                                                         # no iteration runs
                assert iters == [0] * ng and margin == math.inf and running == 0
            if case % 3 == 1 and tol == 0.0 and cut == rows:
                nan_sys = [g for g in range(ng) if np.isnan(h[:, g]).any()]
                assert all(done[g] for g in nan_sys) and running == ng - 1


def test_the_margin_takes_every_residual_of_a_running_system(driver):
    """not only the deciding ones: system 0 comes within 1e-3 of tol at row 2 and stops at row 5 with a margin of 0.5"""
    tol = 1e-3
    h = np.array([[0.5, 0.5], [tol * (1 + 1e-3), 0.1], [0.4, 0.1], [0.3, 0.1], [tol * 0.5, 0.1], [0.0, 0.0]])
    h[:, 1] = h[:, 0]
    path = os.path.join(tempfile.mkdtemp(), 'h.bin')
    h.tofile(path)
    out = driver('stop', path, 1, float(tol).hex(), 8, 6).split('\n')
    assert int(out[1].split()[0]) == 5
    assert float.fromhex(out[0].split()[3]) == abs(tol * (1 + 1e-3) - tol) / tol < 1.1e-3


# ---- 3. chunk length, reduction forms, first decision, limits: the recorded table ------------------------------------------------------
@pytest.fixture(scope='module')
def plans(driver):
    out = driver('plans')
    return out, [r for r in out.split('\n') if r]


def test_every_decision_of_the_grid_is_the_recorded_one(plans):
    out, rows = plans
    recorded = [r for r in open(GOLDEN).read().split('\n') if r and not r.startswith('#')]
    digest = recorded[0].split()
    assert digest[:2] == ['sha256', 'plans']
    got = set(rows)
    missing = [r for r in recorded[1:] if r not in got]          # (the readable rows first: they say WHICH decision moved)
    assert not missing, 'decisions that differ from the recorded ones (recorded rows shown):\n' + '\n'.join(missing[:20])
    assert len(rows) == len(recorded) - 1 == 2199
    assert hashlib.sha256(out.encode()).hexdigest() == digest[2]


def next_kind(looked, launched, e_prev, e_last, tol):
    """the longest chunk that does not overshoot the iterations the last ratio of residuals predicts by more than two"""
    if looked < 4:
        return 2
    if not e_last > tol or not e_last < e_prev:
        return 1
    still_open = math.log(tol / e_last) / math.log(e_last / e_prev) - (launched - looked)
    return next((v for v in (0, 1) if CG_LEN[v] <= still_open + 2.0), 2)


def test_chunk_lengths_follow_the_predicted_iterations(plans):
    rows = [r for r in plans[1] if r.startswith('K ')]
    assert len(rows) == 4 * 5 * (6 * 5 + 2)
    kinds = set()
    for r in rows:
        case, kind = r.split(' | ')
        f = case.split()[1:]
        e_prev, e_last, tol = (float('nan') if v == 'nan' else float.fromhex(v) for v in f[2:])
        assert int(kind) == next_kind(int(f[0]), int(f[1]), e_prev, e_last, tol), r
        kinds.add(int(kind))
    assert kinds == {0, 1, 2}


def forms_look(now, seen, hs, cnt, ncols, n, nchunks, outcome):
    """a kind of reduction leaves the block form when it costs more than the chain, and chunks are launched ahead only while every
    kind in block form costs under half of it (microseconds per chain)"""
    cheap = True
    for m in range(2):
        if not now[m]:
            continue
        by_rec, by_rows = hs[m][1] - seen[m][1], hs[m][2] - seen[m][2]
        seen[m] = list(hs[m])
        blocks_us = (by_rec * 0.7 + by_rows * 1.5) / (float(cnt) * ncols) + nchunks * 0.6 + 14.5
        chain_us = n * 0.0024
        outcome[m] = 'switch' if blocks_us > chain_us else 'stay' if blocks_us > 0.5 * chain_us else 'cheap'
        if blocks_us > chain_us:
            now[m] = False
        elif blocks_us > 0.5 * chain_us:
            cheap = False
    return cheap


def test_reduction_forms_follow_the_cost_comparison(plans):
    rows = [r for r in plans[1] if r.startswith('F ')]
    outcomes = {0: set(), 1: set()}
    for r in rows:
        parts = r.split(' | ')
        if parts[0].endswith('chain'):
            assert parts[1].split() == ['0', '0', '1'] + ['0'] * 6          # never looked at: launched ahead, nothing counted
            continue
        n, ncols, cnt, forced, r0, r1 = (int(v) for v in parts[0].split()[1:])
        chains = cnt * ncols
        hs = [[100 * chains, 5 * chains, r0 * chains], [100 * chains, 5 * chains, r1 * chains]]
        now, seen, ahead = [True, True], [[0, 0, 0], [0, 0, 0]], bool(forced)
        for look in (1, 2):
            was, outcome = list(now), [None, None]
            if not forced:
                ahead = forms_look(now, seen, hs, cnt, ncols, n, (n + 16383) // 16384, outcome)
            got = [int(v) for v in parts[look].split()]
            assert got == [int(now[0]), int(now[1]), int(ahead)] + seen[0] + seen[1], (r, look)
            for m in range(2):
                if look == 1 and not forced:
                    outcomes[m].add(outcome[m])
                if look == 2 and not was[m] and not forced:
                    assert seen[m][0] == 100 * chains                          # a kind that switched is skipped: its counters stay
                if look == 2 and was[m] and not forced:
                    assert seen[m][0] == 107 * chains
            hs = [[v[0] + 7 * chains, v[1], v[2]] for v in hs]
    assert outcomes[0] >= {'switch', 'cheap', 'stay'} and outcomes[1] >= {'switch', 'cheap', 'stay'}


def test_first_decision_for_the_block_form(plans):
    rows = [r for r in plans[1] if r.startswith('D ')]
    assert len(rows) == 4 * 5 * 2 * 3 * 3
    for r in rows:
        n, flags, np1d, nchunks, max_chunks, rec = (int(v) for v in r.split(' | ')[0].split()[1:])
        want = (not np1d and not flags & 16 and nchunks <= max_chunks and n >= 1 and rec <= 1 << 30 and (bool(flags & 8) or n >= 8192))
        assert int(r.split(' | ')[1]) == int(want), r


def test_limits(plans):
    rows = {tuple(int(v) for v in r.split(' | ')[0].split()[1:]): r.split(' | ')[1:] for r in plans[1] if r.startswith('L ')}

    def limit(mode, n=1000, C=4, Cg=4, ncols=4, ld=4, max_iter=100, ngroups=1, nmask=0):
        code, msg = rows[(mode, n, C, Cg, ncols, ld, max_iter, ngroups, nmask)]
        return int(code), msg.strip()
    for mode in (0, 1):
        assert limit(mode) == (0, '')
        assert limit(mode, C=256, Cg=128, ncols=256, ld=256, ngroups=2) == (0, '')
        assert limit(mode, C=257, Cg=1, ncols=260, ld=260, ngroups=257) == (-4, 'glx_cg_multi: C=257 too wide for the column reducer')
        assert limit(mode, max_iter=2 ** 24 - 1) == (0, '')
        assert limit(mode, max_iter=2 ** 24) == (-4, 'glx_cg_multi: max_iter 16777216 exceeds the supported 2^24-1')
        assert limit(mode, n=2 ** 27 - 1) == (0, '')
        assert limit(mode, C=128, Cg=128, ncols=128, ld=128) == (0, '')
        assert limit(mode, C=32, Cg=1, ncols=32, ld=32, ngroups=32, nmask=5) == (0, '')
        assert limit(mode, C=33, Cg=1, ncols=36, ld=36, ngroups=33, nmask=0) == (0, '')
    wide = dict(C=129, Cg=129, ncols=132, ld=132)
    assert limit(0, **wide) == (-4, 'glx_cg_multi: 129 columns per system too wide for the reference-order reducer')
    assert limit(1, **wide) == (0, '')
    assert limit(0, n=2 ** 27) == (-4, "glx_cg_multi: 134217728 rows exceed the reference-order reducer's 32-bit offsets")
    assert limit(1, n=2 ** 27) == (0, '')
    many = dict(C=33, Cg=1, ncols=36, ld=36, ngroups=33, nmask=5)
    assert limit(0, **many) == (0, '')
    assert limit(1, **many) == (-4, 'glx_cg_groups_masked: at most 32 systems with Dirichlet rows per tolerance-mode solve (got 33)')


# ---- 4. the staged upload, 5. the replay key --------------------------------------------------------------------------------------------
def test_stage_layout(driver):
    rows = [r for r in driver('stage').split('\n') if r]
    assert len(rows) == 3 * 3 * 3 * 2 * 2
    for r in rows:
        nb, nmask, C, esize, nscale = (int(v) for v in r.split(' | ')[0].split())
        o_rows, o_mrows, o_mgrp, o_vals, o_scale, total = (int(v) for v in r.split(' | ')[1].split())
        sizes = [(o_rows, nb * 4), (o_mrows, nmask * 4), (o_mgrp, nmask * 4), (o_vals, nb * C * esize), (o_scale, nscale * 8)]
        assert o_rows == 0 and o_vals % 16 == 0 and o_scale % 16 == 0, r
        for (a, size), (b, _) in zip(sizes, sizes[1:] + [(total, 0)]):                   # rows | mask rows | mask systems | values | scale
            assert a + size <= b, r
        assert o_scale + nscale * 8 == total, r
        assert (total == 0) == (nb == 0 and nmask == 0 and nscale == 0), r


def test_replay_key_words(driver):
    assert driver('key').split() == ['1234', 'f' * 16, '10000000000', '1', '8000000000000000', '3ff8000000000000']
