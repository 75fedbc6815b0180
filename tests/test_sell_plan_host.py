"""tests/sell_plan_ref.py -- the numpy restatement of the shape of glx_graph_plan's sliced-ELL image -- held to its own invariants on
the fixtures of tests/big_state_cases.py, and the fixtures held to what tests/test_gpu_big_state.py claims of them: the plan for
states beyond 32 MB with more than one window AND rows split over 4 and 16 slots in every range, one-slot slices of 16 chunks, the
flip of the row classes exactly at 262 144 (fp64) / 524 288 (fp32) columns.  Last, the test of the tests: the image put together
again from the restatement's slot map gives A @ u, and the same map with the split rows' offset left out of the windows' placement
does not.  No GPU."""
import numpy as np
import pytest
import sell_plan_ref as S
import big_state_cases as K

# (fixture, columns, lanes per row, element size) -> big state, nslices, stored: the table of the issue this file came with
SHAPES = [('B', K.N_B, K.N_B, 4, 8, True, 19584, 1854016),
          ('B', K.N_B, K.N_B, 4, 4, False, 20320, 1851456),
          ('B', K.N_B, K.N_B, 8, 8, True, 37600, 2822272),
          ('B', K.N_B, K.N_B, 8, 4, True, 37600, 2822272),
          ('B', K.N_B32, K.N_B32, 4, 4, True, 39104, 3695360),
          ('A', K.N_A, K.FLIP['f64'] - 1, 4, 8, False, 288, 67136),
          ('A', K.N_A, K.FLIP['f64'], 4, 8, True, 160, 69056),
          ('A', K.N_A, K.FLIP['f32'] - 1, 4, 4, False, 288, 67136),
          ('A', K.N_A, K.FLIP['f32'], 4, 4, True, 160, 69056)]
PLANS = [(f, n, nc, G, es) for f, n, nc, G, es, _, _, _ in SHAPES] + [('B', K.N_B, K.N_B, 16, 8), ('B', K.N_B, K.N_B, 16, 4)]
IDS = ['%s-n%d-cols%d-G%d-es%d' % p for p in PLANS]


def _lens(fixture, n):
    return K.lengths_a() if fixture == 'A' else K.lengths_b(n)


def _plan(fixture, n, n_cols, G, esize, **kw):
    return S.plan(_lens(fixture, n), n_cols, G, esize, **kw)


@pytest.mark.parametrize('fixture,n,n_cols,G,esize,big,nslices,stored', SHAPES, ids=IDS[:len(SHAPES)])
def test_shape_numbers(fixture, n, n_cols, G, esize, big, nslices, stored):
    p = _plan(fixture, n, n_cols, G, esize)
    assert (p['big'], p['nslices'], p['stored']) == (big, nslices, stored)
    assert p['nslices'] % (S.NX * S.WPB) == 0 and p['stored'] % 64 == 0
    assert sum(r['rows'] for r in p['ranges']) == n


@pytest.mark.parametrize('fixture,n,n_cols,G,esize', PLANS, ids=IDS)
def test_invariants_of_the_slot_map(fixture, n, n_cols, G, esize):
    lens = _lens(fixture, n)
    p = S.plan(lens, n_cols, G, esize)
    R = p['R']
    row, slen = p['slot_row'], p['slot_len']
    used = np.flatnonzero(row >= 0)
    S_of = p['S'][used // R]
    # every row exactly once: S slots each, consecutive, starting at a multiple of S inside the slice
    firsts = used[(used % R) % S_of == 0]
    assert np.array_equal(np.sort(row[firsts]), np.arange(n))
    assert len(used) == int(S_of[(used % R) % S_of == 0].sum())
    assert np.array_equal(row[used], row[used - (used % R) % S_of]) and np.array_equal(slen[used], lens[row[used]])
    assert np.array_equal(S_of, S.klass(lens[row[used]], p['L1'], p['L4']))
    # a slice is wide enough for its longest row, and `full` chunks are full in every slot
    per_slot = p['nchunks'] * (4 * p['S'] if G == 4 else G)
    assert np.all(np.repeat(per_slot, R) >= slen)
    if G == 4:
        shortest = slen.reshape(-1, R).min(axis=1)
        assert np.array_equal(p['full'], shortest // (4 * p['S'])) and np.all(p['full'] <= p['nchunks'])
    # a slice belongs to the range of its rows
    xr = np.searchsorted(p['xb'], row[used], side='right') - 1
    assert np.array_equal(xr, used // R // (p['nslices'] // S.NX))
    for r in p['ranges']:
        order, nlong = r['order'], r['nlong']
        assert np.array_equal(np.sort(order), np.arange(r['first'], r['first'] + r['rows']))
        lo = lens[order]
        assert np.all(np.diff(lo[:nlong]) <= 0)                                    # the split rows longest first
        if p['windowed'] and r['windows'] > 1:
            assert np.all(S.klass(lo[:nlong], p['L1'], p['L4']) > 1) and np.all(S.klass(lo[nlong:], p['L1'], p['L4']) == 1)
        rest = order[nlong:]
        for w0 in range(0, len(rest), S.SIGMA if r['windows'] > 1 else max(1, len(rest))):
            w = rest[w0:w0 + S.SIGMA] if r['windows'] > 1 else rest
            assert np.all(np.diff(lens[w]) <= 0)                                   # inside a window the lengths do not increase
            if r['windows'] > 1:                                                   # and a window is a stretch of the vertex order
                assert w.max() - w.min() < S.SIGMA + nlong and (w0 == 0 or w.min() > rest[:w0].max())
        assert r['windows'] == (-(-(r['rows'] - nlong) // S.SIGMA) if p['big'] and r['rows'] > S.SIGMA else 1)


def test_ranges_carry_equal_work():
    lens = K.lengths_b()
    xb = S.ranges(lens)
    work = np.add.reduceat(lens + S.ROW_COST, xb[:-1])
    assert xb[0] == 0 and xb[-1] == K.N_B and np.all(np.diff(xb) > 0)
    assert work.max() - work.min() <= 2 * (max(K.LENGTHS) + S.ROW_COST)
    # the loop of csrc/graph.hip:736-742, said as a loop
    total, acc, i, want_xb = int((lens + 3).sum()), 0, 0, [0]
    for x in range(1, 8):
        while i < len(lens) and acc < total * x // 8:
            acc += int(lens[i]) + 3
            i += 1
        want_xb.append(i)
    assert xb[:-1].tolist() == want_xb
    assert S.ranges(np.array([5, 0, 9])).tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 3]


@pytest.mark.parametrize('dt', ['f64', 'f32'])
def test_classes_flip_exactly_at_the_32_MiB_state(dt):
    es, flip = K.ESIZE[dt], K.FLIP[dt]
    assert flip * 4 * 4 * es == 32 * 1024 * 1024
    assert S.classes(flip - 1, 4, es) == (False, False, 24, 96)
    assert S.classes(flip, 4, es) == (True, False, 64, 256)
    assert S.classes(flip // 2 - 1, 8, es)[0] is False and S.classes(flip // 2, 8, es)[0] is True
    assert S.classes(flip // 2, 8, es)[2:] == (1 << 30, 1 << 30) and S.classes(100, 8, es, relaxed=True)[1] is False
    assert S.classes(100, 4, es, relaxed=True) == (False, True, 64, 256)
    below, at = _plan('A', K.N_A, flip - 1, 4, es), _plan('A', K.N_A, flip, 4, es)
    lens = K.lengths_a()
    for p, (L1, L4) in ((below, (24, 96)), (at, (64, 256))):
        R = p['R']
        first = np.flatnonzero((p['slot_row'] >= 0) & (np.arange(len(p['slot_row'])) % R % np.repeat(p['S'], R) == 0))
        got = dict(zip(p['slot_row'][first].tolist(), np.repeat(p['S'], R)[first].tolist()))
        assert all(got[i] == (16 if lens[i] > L4 else 4 if lens[i] > L1 else 1) for i in range(K.N_A))
    # the two sides give different classes to the rows between the limits, and only to those
    moved = {int(l) for l in set(lens.tolist()) if S.klass(l, 24, 96) != S.klass(l, 64, 256)}
    assert moved == {25, 63, 64, 97, 255, 256}
    assert not np.array_equal(below['S'][:below['nslices'] // 8], at['S'][:below['nslices'] // 8])
    assert max(r['max_nchunks_one_slot'] for r in below['ranges']) == 6 and max(r['max_nchunks_one_slot'] for r in at['ranges']) == 16
    assert not below['windowed'] and not at['windowed']


@pytest.mark.parametrize('n,dt', [(K.N_B, 'f64'), (K.N_B32, 'f32')])
def test_fixture_b_reaches_windows_and_split_rows_together(n, dt):
    p = _plan('B', n, n, 4, K.ESIZE[dt])
    assert p['big'] and p['windowed'] and (p['L1'], p['L4']) == (64, 256)
    for r in p['ranges']:
        assert r['windows'] >= 2 and r['nlong'] > 0, r
        assert r['classes'] == {1, 4, 16}
        assert r['max_nchunks_one_slot'] == 16                # a row of 61 .. 64 entries in one slot
    if n == K.N_B:
        assert all(r['windows'] == 2 and 250 <= r['nlong'] <= 270 and 37000 <= r['rows'] <= 38000 for r in p['ranges'])
    else:
        assert all(r['windows'] == 3 for r in p['ranges'])
    # full chunks under the larger classes: some slice of every class has some, and some one-slot slice has fewer than it has chunks
    for cls in (1, 4, 16):
        assert np.any(p['full'][p['S'] == cls] > 0)
    assert np.any((p['S'] == 1) & (p['full'] > 0) & (p['full'] < p['nchunks']))


def test_the_control_is_the_small_state_plan():
    p = _plan('B', K.N_B, K.N_B, 4, 4)
    assert not p['big'] and not p['windowed'] and (p['L1'], p['L4']) == (24, 96)
    assert all(r['nlong'] == 0 and r['windows'] == 1 for r in p['ranges'])
    for G in (8, 16):
        for es in (4, 8):
            q = _plan('B', K.N_B, K.N_B, G, es)
            assert q['big'] and q['windowed'] and all(r['windows'] == 2 and r['nlong'] == 0 and r['classes'] == {1} for r in q['ranges'])


def test_stop_runs_on_fixture_b_stop_where_the_device_test_says():
    A, deg, vinf, w_unit = K.stop_fixture()
    for k, T in K.STOP_K_T:
        u, t, first, vals = K.stop_run(2, 0, k)
        assert t == T and first == K.STOP_MIN and len(vals) == T - K.STOP_MIN + (1 if T < K.STOP_MAX else 0)
        # decided by a margin: no compared value within 10 % of 1 / n
        assert np.all(np.abs(vals * K.N_B - 1) > 0.1), vals * K.N_B
        assert np.isfinite(u).all() and u.any()


@pytest.mark.parametrize('fixture,n,n_cols,G,esize', [('A', K.N_A, K.FLIP['f64'], 4, 8), ('A', K.N_A, K.FLIP['f64'] - 1, 4, 8),
                                                       ('B', K.N_B, K.N_B, 4, 8), ('B', K.N_B, K.N_B, 8, 8), ('B', K.N_B, K.N_B, 4, 4)])
def test_replay_of_the_slot_map_gives_the_product(fixture, n, n_cols, G, esize):
    A = K.rect(n_cols) if fixture == 'A' else K.square()
    u = np.random.default_rng(5).normal(size=(n_cols, 2))
    p = _plan(fixture, n, n_cols, G, esize)
    slot, jj = S.slot_entries(p)
    assert len(slot) == A.nnz                                   # every entry is held by exactly one slot
    assert np.array_equal(S.replay(p, A, u), A @ u)


def test_a_wrong_plan_gives_a_wrong_product():
    """The check of the checks, on the CPU only: with the split rows' offset dropped from the windows' placement (`order[w0 + ...]` for
    `order[nlong + w0 + ...]`, csrc/graph.hip:783) the first window overwrites the split rows and the tail of the order is never
    written.  The counts info() reports may even stay plausible; the replayed product does not equal A @ u."""
    A = K.square()
    u = np.random.default_rng(5).normal(size=(K.N_B, 2))
    want = A @ u
    good = _plan('B', K.N_B, K.N_B, 4, 8)
    assert np.array_equal(S.replay(good, A, u), want)          # first: the replay itself is right
    bad = _plan('B', K.N_B, K.N_B, 4, 8, perturb='drop_nlong')
    got = S.replay(bad, A, u)
    assert not np.array_equal(got, want, equal_nan=True)
    lost = np.flatnonzero(np.isnan(got).any(axis=1))
    nlong = sum(r['nlong'] for r in good['ranges'])
    assert len(lost) == nlong > 0 and np.all(K.lengths_b()[lost] > 64)      # the rows that went missing are split rows
    # and where there is nothing to drop the perturbation changes nothing: the control plan has no split-row offset
    same = _plan('B', K.N_B, K.N_B, 4, 4, perturb='drop_nlong')
    assert np.array_equal(S.replay(same, A, u), want)


def test_the_hubs_cg_case_reaches_a_windowed_relaxed_plan_with_split_rows():
    """'large-hubs-C3-f64' of tests/cg_cases.py: what tests/test_gpu_cg_wide.py solves on is the relaxed plan of a state beyond 32 MB
    with rows of class 4 (75 entries) and 16 (305) in front of two windows in every range."""
    import cg_cases
    import cg_ref
    case = cg_cases.BY_ID['large-hubs-C3-f64']
    assert case['keep_order'] and case['C'] == 3 and case['dt'] == 'f64'      # 3 columns: 4 lanes per row, where relaxed plans exist
    A = cg_ref.banded_hubs(case['n'])
    lens = np.diff(A.indptr).astype(np.int64)
    assert {75, 305} <= set(lens.tolist()) and lens.max() == 305
    p = S.plan(lens, case['n'], 4, 8, relaxed=True)
    assert p['big'] and p['relaxed'] and p['windowed'] and (p['L1'], p['L4']) == (64, 256)
    assert all(r['windows'] == 2 and 8 <= r['nlong'] <= 10 and r['classes'] == {1, 4, 16} for r in p['ranges'])
    assert (p['nslices'], p['stored']) == (18880, 2412864)
    u = np.random.default_rng(6).normal(size=(case['n'], 2))
    assert np.array_equal(S.replay(p, A, u), A @ u)
