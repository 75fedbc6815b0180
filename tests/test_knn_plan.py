"""graphlearning_amd/csrc/knn_plan.h, the plan of one pass of the exact kNN search (list length, tile width, ref ranges, candidate
count, query chunks, the filter's error constant, the seeding / escalation / wide-fallback decisions), the power of two the filter's
operands are scaled by and the chain of the cells:
built on the host with no HIP header (tests/knn_plan_host.cpp) and compared with the table recorded from the search pass as it
stood before the plan was a header of its own (tests/golden/knn_plans.txt)."""
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'knn_plans.txt')
BQ = 128
KNN_CAND_BUDGET = 1 << 30
FIELDS = ('KP', 'DH', 'nkb', 'NKB', 'dpa', 'BR', 'ntiles', 'nsplit', 'lists', 'ncand', 'M', 'chunk', 'nchunks', 'short_lists', 'wide',
          'use_bf16', 'cat')


@pytest.fixture(scope='module')
def driver():
    exe = os.path.join(tempfile.mkdtemp(), 'knn_plan_host')
    subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'graphlearning_amd', 'csrc'), '-o', exe,
                    os.path.join(ROOT, 'tests', 'knn_plan_host.cpp')], check=True)

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (args, r.returncode, r.stderr[-4000:])
        return r.stdout
    return run


@pytest.fixture(scope='module')
def golden():
    digests, rows, extras = {}, [], []
    for line in open(GOLDEN).read().split('\n'):
        if not line or line.startswith('#'):
            continue
        if line.startswith('sha256 '):
            digests[line.split()[1]] = line.split()[2]
        elif line[0] in 'SEF':
            extras.append(line)
        else:
            rows.append(line)
    return digests, rows, extras


def parse(row):
    """(n, d, k, nq, long_lists, overrides, concat), {field: value}"""
    case, plan = row.split(' | ')
    vals = plan.split()
    p = {f: int(v) for f, v in zip(FIELDS, vals)}
    p['cerr'] = vals[len(FIELDS)]
    return tuple(int(v) for v in case.split()), p


@pytest.fixture(scope='module')
def plans(driver):
    out = driver('plans')
    return out, dict(parse(r) for r in out.split('\n') if r)


def test_every_plan_of_the_grid_is_the_recorded_one(plans, golden):
    out, _ = plans
    digests, rows, _ = golden
    got = set(out.split('\n'))
    missing = [r for r in rows if r not in got]      # (the readable rows first: they say WHICH plan moved)
    assert not missing, 'plans that differ from the recorded ones (recorded rows shown):\n' + '\n'.join(missing[:20])
    assert out.count('\n') == 11662
    assert hashlib.sha256(out.encode()).hexdigest() == digests['plans']


def test_seeding_escalation_and_wide_fallback_decisions_are_the_recorded_ones(driver, golden):
    digests, _, extras = golden
    out = driver('extras')
    got = [r for r in out.split('\n') if r]
    assert len(got) == len(extras)
    diff = [(g, w) for g, w in zip(got, extras) if g != w]
    assert not diff, 'decisions that differ (got, recorded):\n' + '\n'.join('%s\n%s' % gw for gw in diff[:20])
    assert hashlib.sha256(out.encode()).hexdigest() == digests['extras']
    # the thresholds the grid is there to cross
    rows = {r.split(' | ')[0]: r.split(' | ')[1] for r in got}
    assert rows['F 61 1'].split()[0] == '128' and rows['F 64 1'].split()[0] == '128'
    assert rows['F 65 1'].split()[0] == '256' and rows['F 1024 1'].split()[0] == '2048'
    assert any(r.startswith('E ') and ' 64:0 65:1 ' in r for r in got)                      # more than 64 flagged rows
    assert rows['S 70000 20 60 70000 0 16'] == '8 1' and rows['S 70000 20 61 70000 0 16'] == '8 0'    # never the wide plan
    assert rows['S 70000 20 12 70000 0 1'] == '0 0' and rows['S 70000 20 12 70000 0 -1'] == '0 0'   # one cell, no cells


def test_anchor_plans(plans):
    _, p = plans
    default = (0, -1)

    def plan(n, d, k, nq, long_lists):
        return p[(n, d, k, nq, int(long_lists)) + default]

    def has(q, **want):
        got = {f: q[f] for f in want}
        assert got == want, (got, want)
    # config 2 of the benchmark: the split-bf16 filter with 8 lists of 8; its long-list repeat on the fp32-input filter
    has(plan(70000, 20, 12, 70000, False), use_bf16=1, KP=8, nsplit=4, ncand=64, cat=2, nchunks=1, cerr='0x1.3ap-15')
    has(plan(70000, 20, 12, 70000, True), use_bf16=0, KP=16, BR=128, nsplit=2, cerr='0x1p-17')
    # the wide plan
    has(plan(70000, 20, 128, 70000, False), lists=16, KP=32, ncand=512)
    has(plan(70000, 20, 1024, 70000, False), lists=64, KP=32, ncand=2048, chunk=65536, nchunks=2)
    has(plan(70000, 20, 1024, 70000, True), lists=64, KP=64, ncand=4096, chunk=32768, nchunks=3)
    for long_lists in (False, True):
        has(plan(70000, 784, 1024, 70000, long_lists), use_bf16=0, DH=16, nkb=25, dpa=800)


def test_invariants_of_every_plan(plans):
    _, p = plans
    assert len(p) == 11662
    for (n, d, k, nq, long_lists, overrides, concat), q in p.items():
        case = (n, d, k, nq, long_lists, overrides, concat, q)
        assert q['lists'] == 2 * q['nsplit'], case
        assert q['ncand'] == q['lists'] * q['KP'], case
        M = 64
        while M < q['ncand']:
            M *= 2
        assert q['M'] == M, case
        if q['wide'] and q['chunk'] > BQ:
            assert q['chunk'] * q['ncand'] * 8 <= KNN_CAND_BUDGET, case
        if q['use_bf16']:
            assert q['short_lists'] and d <= 128 and q['KP'] <= 32, case
        if q['wide']:
            assert q['ncand'] >= k, case


def chain_places(cen):
    """The greedy chain of nearest centres from the centre farthest from the centres' mean, on every cfs-th feature; sums in the
    header's order (feature by feature, left to right)."""
    m, d = cen.shape
    mean = np.zeros(d)
    for c in range(m):
        mean += cen[c] / m
    sub = np.arange(0, d, (d + 31) // 32)

    def dist2(a, b):
        t = np.zeros(len(a))
        for f in sub:
            t += (a[:, f] - b[f]) ** 2
        return t
    cur = int(np.argmax(dist2(cen, mean)))
    place = np.full(m, -1)
    for pos in range(m):
        place[cur] = pos
        t = np.where(place < 0, dist2(cen, cen[cur]), np.inf)
        cur = int(np.argmin(t))
    return place


@pytest.mark.parametrize('m,d', [(1, 3), (2, 20), (37, 3), (128, 20), (512, 64), (300, 100)])
def test_chain_of_the_cells(driver, m, d):
    rng = np.random.default_rng(1000 * m + d)
    cen = rng.standard_normal((m, d)) * rng.uniform(0.1, 10.0, size=d)
    path = os.path.join(tempfile.mkdtemp(), 'cen.bin')
    cen.tofile(path)
    got = np.array(driver('chain', path, m, d).split(), dtype=np.int64)
    assert np.array_equal(np.sort(got), np.arange(m))
    assert np.array_equal(got, chain_places(cen))


def test_scale_of_the_filters_operands(driver):
    """knn_filter_scale: 1 inside the window [2^-40, 2^40] in which the filter's relative error bound is valid (data there is taken
    as it comes), elsewhere the exact power of two that brings the largest centred norm into [1, 2); 1 where nothing can be done."""
    def scales(values):
        return [float.fromhex(t) for t in driver('scale', *[v.hex() for v in values]).split()]
    inside = [2.0 ** -40, 2.0 ** -40 * (1 + 2.0 ** -52), 1e-6, 1.0, 1.5, 1e6, 2.0 ** 40 * (1 - 2.0 ** -53), 2.0 ** 40]
    assert scales(inside) == [1.0] * len(inside)
    rng = np.random.default_rng(5)
    outside = [2.0 ** -40 * (1 - 2.0 ** -53), 2.0 ** 40 * (1 + 2.0 ** -52), 1e-20, 1e20, 2.0 ** -1022, 2.0 ** 1023 * (1 - 2.0 ** -53), 2.0 ** -66 * 1024,
               2.0 ** 400 * 1447.3] + list(np.ldexp(rng.uniform(1, 2, 64), rng.integers(-1022, -41, 64))) + list(np.ldexp(rng.uniform(1, 2, 64), rng.integers(41, 1023, 64)))
    for r, s in zip(outside, scales(outside)):
        m, e = np.frexp(s)
        assert m == 0.5 and 1.0 <= r * s < 2.0, (r, s)                 # an exact power of two, a normal number; r * s is exact
        assert np.isfinite(s) and s >= 2.0 ** -1022
    nothing = [0.0, 5e-324, 2.0 ** -1023, 2.0 ** 1023, float('inf'), float('nan')]
    assert scales(nothing) == [1.0] * len(nothing)


# ---- the coverage census of the narrow search (k <= 60): tests/knn_narrow_cases.py against the header ---------------------------------
def _plan_rows(out):
    import knn_narrow_cases as nc
    for row in out.split('\n'):
        if row:
            (n, d, k, nq, long_lists, _, _), q = parse(row)
            yield (n, d, k, nq, long_lists), nc.Plan(q['KP'], q['DH'], q['nkb'], q['NKB'], q['dpa'], q['BR'], q['ntiles'], q['nsplit'], bool(q['use_bf16']),
                                                     q['cat'], bool(q['short_lists']))


@pytest.fixture(scope='module')
def census(driver):
    """Every plan of d = 1 .. 400 x k = 1 .. 60 x filter {default, f32} x lists {default, long} at the n of the GPU cases:
    {kernel key: a (d, k, filter, lists) that takes it}; the Python restatement must give the header's plan at every point, for the
    escalated pass (long_lists = 1) as well."""
    import knn_narrow_cases as nc
    keys = {}
    for filt in (None, 'f32'):
        for lists in (None, 'long'):
            for long_lists in (0, 1):
                out = driver('plan', nc.N_MAIN, '1:400', '1:60', nc.N_MAIN, long_lists, nc.FILTER[filt], nc.LISTS[lists], 0, -1)
                rows = list(_plan_rows(out))
                assert len(rows) == 400 * 60
                for (n, d, k, nq, ll), p in rows:
                    assert p == nc.plan(n, d, k, nq, bool(ll), filter=filt, lists=lists), (d, k, filt, lists, ll)
                    if not long_lists:
                        keys.setdefault(nc.kernel_key(p), (d, k, filt, lists))
    return keys


def test_narrow_cases_reach_every_tile_kernel(census):
    """Every instantiation of the two tile kernels that some (d, k, filter, lists) with k <= 60 launches is launched by a case of
    tests/test_gpu_knn_narrow.py's main matrix (n = 2999).  A tile class added to the plan without a case fails here."""
    import knn_narrow_cases as nc
    # bf16: NKB 1, 2 (three operand forms), 4, 6, 8 x lists of 8, 16, 32; fp32: DH 8, 12, 18, 34, 66 x lists of 8, 16, 32, lists of 64
    # at DH 8, 12, 18, and the blocked variant with DH = 32 (lists of 16, 32) and 16 (lists of 64)
    assert len(census) == 7 * 3 + 5 * 3 + 3 + 3, sorted(census)
    hit = {}
    for c in nc.CASES:
        if c.n == nc.N_MAIN and c.group in ('main', 'f32', 'long'):
            hit.setdefault(nc.kernel_key(nc.case_plan(c)), nc.case_id(c))
    missing = {key: where for key, where in census.items() if key not in hit}
    assert not missing, 'tile kernels no case runs (key: a d, k, filter, lists that takes it): %s' % missing
    assert set(hit) == set(census)           # (and no case claims a key the plan never produces)


def test_narrow_case_table_is_the_issued_one():
    import knn_narrow_cases as nc
    by = {}
    for c in nc.CASES:
        by.setdefault(c.group, []).append(c)
    main = by['main']
    assert {(c.d, c.k) for c in main if c.style == 'iso'} == {(d, k) for d in nc.MAIN_D for k in nc.MAIN_K}
    for d in nc.MAIN_D:
        adv = {c.k: c.style for c in main if c.d == d and c.style != 'iso'}
        assert sorted(adv) == [12, 29] and all(s in nc.ADVERSARIAL or (s == 'grid' and d <= 3) for s in adv.values()), (d, adv)
    for lo, hi in ((1, 16), (17, 32), (33, 64), (65, 96), (97, 128)):           # every NKB class meets near-duplicates and an offset
        styles = {c.style for c in main if lo <= c.d <= hi}
        assert {'neardup', 'offset'} <= styles, (lo, hi, styles)
    assert {(c.d, c.k) for c in by['f32']} == {(d, k) for d in (14, 15, 22, 23, 34, 35, 66, 67, 128) for k in nc.MAIN_K}
    assert {(c.d, c.k) for c in by['long']} >= {(d, k) for d in (20, 33, 64, 96, 130, 190, 191) for k in (12, 28, 29, 60)}
    assert all(dict(c.opts) == {'filter': 'f32'} for c in by['f32']) and all(dict(c.opts) == {'lists': 'long'} for c in by['long'])
    assert {(c.d, c.k, c.opts) for c in by['repair']} >= {(d, 12, (('nsplit', 1),)) for d in (96, 128)}
    assert {(c.d, c.k, c.style) for c in by['split']} == {(d, k, 'lohalf') for d in (32, 64, 96, 128) for k in (12, 29)}
    assert {(c.d, c.n, c.k) for c in by['small']} == {(d, n, k) for d in (21, 96, 128, 130) for n, k in ((60, 60), (33, 12), (129, 29))}
    assert len({nc.case_id(c) for c in nc.CASES}) == len(nc.CASES)


def test_every_narrow_case_plans_as_the_header_does(driver):
    """Case by case, with the case's own n and overrides: the restatement the GPU test takes its expected statistics from is the
    header's plan, for the first pass and for the long-list repeat."""
    import knn_narrow_cases as nc
    for c in nc.CASES:
        o = dict(c.opts)
        for long_lists in (0, 1):
            out = driver('plan', c.n, c.d, c.k, c.n, long_lists, nc.FILTER[o.get('filter')], nc.LISTS[o.get('lists')], o.get('nsplit', 0), -1)
            (_, p), = _plan_rows(out)
            assert p == nc.case_plan(c, bool(long_lists)), (nc.case_id(c), long_lists)
    # the classes the issue names, spelled out once
    want = {(96, 12): ('bf16', 6, 0, 8, 32), (128, 28): ('bf16', 8, 0, 16, 32), (21, 12): ('bf16', 2, 1, 8, 64), (20, 60): ('bf16', 2, 2, 32, 32),
            (22, 13): ('bf16', 2, 0, 16, 64), (130, 12): ('f32', 66, 8, False, 32), (131, 60): ('f32', 16, 64, True, 32)}
    for (d, k), key in want.items():
        assert nc.kernel_key(nc.plan(nc.N_MAIN, d, k)) == key, (d, k)


def test_margin_of_the_acceptance_test(driver):
    """knn_accept_eps = cerr (|q| + R)^2 + 2^-12 cerr (|q| + rmax)^2 with R = min(rmax, (|q| + dk) (1 + 2^-10)): never above the
    uniform margin cerr (|q| + rmax)^2 by more than its 2^-12 floor, equal to it (plus the floor) once |q| + dk reaches rmax, never
    below the pair bound cerr (|q| + |r|)^2 of any ref the triangle inequality does not exclude (|r| <= |q| + dk), growing with dk."""
    def eps(cerr, q, rmax, dk2):
        return float.fromhex(driver('accept_eps', float(cerr).hex(), float(q).hex(), float(rmax).hex(), float(dk2).hex()).strip())
    rng = np.random.default_rng(8)
    cerr = float.fromhex('0x1.3ap-15')
    for _ in range(200):
        rmax = float(np.ldexp(rng.uniform(1, 2), int(rng.integers(-40, 41))))
        q = rmax * float(rng.uniform(0, 1))
        dk = rmax * float(10.0 ** rng.uniform(-6, 0.5))
        old = cerr * (q + rmax) ** 2
        e = eps(cerr, q, rmax, dk * dk)
        R = min(rmax, (q + dk) * (1 + 2.0 ** -10))
        want = cerr * (q + R) * (q + R) + 2.0 ** -12 * cerr * (q + rmax) * (q + rmax)
        assert abs(e - want) <= 1e-15 * want          # (a host compiler may contract the products and sums)
        assert e <= old * (1 + 2.0 ** -12) * (1 + 1e-15)
        if q + dk >= rmax:
            assert e >= old * (1 - 1e-15)
        r = min(rmax, q + dk)                       # the farthest ref the triangle inequality leaves in play
        assert e >= cerr * (q + r) ** 2 * (1 - 1e-15)
        assert eps(cerr, q, rmax, 4 * dk * dk) >= e
    assert abs(eps(cerr, 1.0, 3.0, float('inf')) / (cerr * 16.0 * (1 + 2.0 ** -12)) - 1) <= 1e-15
    assert abs(eps(cerr, 0.0, 3.0, 0.0) / (2.0 ** -12 * cerr * 9.0) - 1) <= 1e-15          # the floor: absolute errors of underflowing products
