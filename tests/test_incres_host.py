"""INCRES clustering without a GPU: the numpy restatement (tests/incres_ref.py) against the reference's recorded labels and sweep counts
(tests/golden/g21_incres.npz), the chunked schedule of csrc/incres_plan.h (tests/incres_plan_host.cpp: plain loops stand in for the
kernels) against the restatement at forced chunk lengths, and the summation order the contract rests on."""
import os
import sys
import numpy as np
import pytest
from scipy import sparse

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import incres_ref as ref  # noqa: E402

CHUNKS = (1, 2, 7, 0)      # 0: the plan decides


@pytest.fixture(scope='module')
def gold():
    return ref.load_golden()


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return ref.build_host_lib(tmp_path_factory.mktemp('incres_host'))


@pytest.fixture(scope='module')
def restated(gold):
    """name -> (labels (T, n), sweeps (T), seeds per iteration) of the restatement under the recorded seed: computed once, shared"""
    out = {}
    for name, (g, k, seed, params) in ref.GOLDEN_CASES.items():
        np.random.seed(seed)
        out[name] = ref.fit(ref.golden_graph(gold, g), k, **params)
    return out


@pytest.mark.parametrize('name', list(ref.GOLDEN_CASES))
def test_restatement_equals_the_reference_after_every_outer_iteration(gold, restated, name):
    g, k, seed, params = ref.GOLDEN_CASES[name]
    hist, sweeps, _ = restated[name]
    assert int(gold['case_%s_seed' % name]) == seed
    assert hist.shape == gold['case_%s_labels' % name].shape == (params.get('T', 200), ref.golden_graph(gold, g).shape[0])
    assert np.array_equal(hist, gold['case_%s_labels' % name])
    assert np.array_equal(sweeps, gold['case_%s_sweeps' % name])


def drive(lib, P, k, planted, chunk):
    """the plan driver over recorded seeds: (labels, sweeps, (slot, chunks, enqueued)) per iteration"""
    labels, sweeps, where = [], [], []
    with ref.HostIncres(lib, P, k, chunk) as host:
        for seeds in planted:
            lab, s = host.step(seeds)
            labels.append(lab)
            sweeps.append(s)
            where.append(host.last)
    return np.array(labels), np.array(sweeps), where


@pytest.mark.parametrize('name', ['blobs3_fast', 'blobs5', 'moons2'])
def test_plan_driver_equals_the_restatement_at_every_chunk_length(gold, restated, lib, name):
    g, k, seed, params = ref.GOLDEN_CASES[name]
    hist, counts, planted = restated[name]
    P = ref.transition(ref.golden_graph(gold, g))
    take = slice(0, 40)                                         # the first 40 outer iterations: every chunk length walks them
    last_slot = first_slot = False
    for chunk in CHUNKS:
        labels, sweeps, where = drive(lib, P, k, planted[take], chunk)
        assert np.array_equal(labels, hist[take]) and np.array_equal(sweeps, counts[take]), chunk
        for s, (slot, chunks, enqueued) in zip(sweeps, where):
            assert enqueued >= s and (chunk == 0 or chunks == max(1, -(-s // chunk)))
            if chunk:
                last_slot |= slot == chunk
                first_slot |= slot == 1 and chunks > 1
    if name == 'moons2':                                        # counts of 14 .. 38: both corner cases occur at chunk lengths 2 and 7
        assert last_slot and first_slot


def test_a_stop_on_the_last_and_on_the_first_slot_of_a_chunk(gold, restated, lib):
    """chunk length 7: an iteration whose count is a multiple of 7 stops on a chunk's last slot, one with count = 1 mod 7 above 7 on
    the first slot of a later chunk; both occur among the recorded counts, and both give the restatement's labels"""
    hist, counts, planted = restated['moons2']
    P = ref.transition(ref.golden_graph(gold, 'moons'))
    on_last = [i for i, s in enumerate(counts) if s % 7 == 0]
    on_first = [i for i, s in enumerate(counts) if s % 7 == 1 and s > 7]
    assert on_last and on_first
    with ref.HostIncres(lib, P, 2, 7) as host:
        for i, want in ((on_last[0], 7), (on_first[0], 1)):
            lab, s = host.step(planted[i])
            assert s == counts[i] and np.array_equal(lab, hist[i]) and host.last[0] == want
            assert host.last[1] == -(-s // 7) and host.last[2] == 7 * host.last[1]


def test_zero_sweeps_when_the_planted_state_has_no_zero(lib):
    """n = 2, one cluster, T = 30: as soon as both vertices are seeded the grow loop does not run at all"""
    W = sparse.csr_matrix(np.ones((2, 2)))
    np.random.seed(3)
    hist, counts, planted = ref.fit(W, 1, T=30)
    assert (counts == 0).any() and (counts > 0).any()           # the restatement really shows both
    P = ref.transition(W)
    for chunk in CHUNKS:
        labels, sweeps, where = drive(lib, P, 1, planted, chunk)
        assert np.array_equal(labels, hist) and np.array_equal(sweeps, counts)
        assert all(w[0] == 0 for w, s in zip(where, sweeps) if s == 0)


def test_the_stored_order_of_p_is_reversed_and_decides_bits(gold, restated):
    W = ref.golden_graph(gold, 'blobs')
    assert W.has_sorted_indices
    P = ref.transition(W)
    assert not P.has_sorted_indices
    row = slice(P.indptr[0], P.indptr[1])
    assert np.array_equal(P.indices[row], W.indices[row][::-1])
    Q = P.copy()
    Q.sort_indices()
    assert (P != Q).nnz == 0                                     # the same matrix, another order
    seeds = restated['blobs3'][2][0]
    F, s = ref.grow(P, ref.plant(600, 3, seeds))
    Fs, ss = ref.grow(Q, ref.plant(600, 3, seeds))
    assert s == ss == restated['blobs3'][1][0]
    assert not np.array_equal(F.view(np.uint64), Fs.view(np.uint64))      # at least one bit differs: the order test is not vacuous


def test_denormals_stay_nonzero_on_the_long_path(lib):
    """665 vertices in a row with self loops, one cluster, one seed at vertex 0: 664 sweeps, and the smallest value of the final state
    is a denormal -- which the zero test must see as nonzero"""
    P = ref.transition(ref.path_graph(665))
    labels, sweeps, F = ref.step(P, 1, [[0]])
    assert sweeps == 664 and 0 < F.min() < ref.DENORMAL_MIN_NORMAL and not labels.any()
    with ref.HostIncres(lib, P, 1) as host:
        lab, s = host.step([[0]])
        assert s == 664 and not lab.any()


def test_the_cap_ends_a_loop_that_would_not_end(lib):
    two = sparse.block_diag([ref.ring_graph(20), ref.ring_graph(23)]).tocsr()
    for W in (two, ref.path_graph(40, loops=False)):
        P = ref.transition(W)
        labels, sweeps, _ = ref.step(P, 1, [[0]], max_grow=50)
        assert labels is None and sweeps == 50
        for chunk in CHUNKS:
            with ref.HostIncres(lib, P, 1, chunk) as host:
                with pytest.raises(RuntimeError, match='capped after 50 sweeps'):
                    host.step([[0]], max_grow=50)
                assert host.last[2] == 50                            # not one sweep more was enqueued
                lab, s = host.step([list(range(W.shape[0]))])        # usable afterwards
                assert s == 0 and not lab.any()
    # a loop that needs exactly max_grow sweeps succeeds
    P = ref.transition(ref.path_graph(30))
    want = ref.step(P, 1, [[0]])
    assert want[1] == 29
    with ref.HostIncres(lib, P, 1, 7) as host:
        lab, s = host.step([[0]], max_grow=29)
        assert s == 29 and np.array_equal(lab, want[0])
        with pytest.raises(RuntimeError, match='capped after 28 sweeps'):
            host.step([[0]], max_grow=28)


def test_chunk_lengths_of_the_plan(lib):
    c = np.zeros(5, dtype=np.int64)
    lib.incres_host_constants(c.ctypes.data)
    max_cols, max_chunk, first, margin, nxt = (int(v) for v in c)
    assert (max_cols, max_chunk) == (256, 64) and 1 <= margin < first <= max_chunk and 1 <= nxt <= max_chunk
    big = 1 << 40
    length = lib.incres_host_chunk_len                                # (forced, count before, sweeps done, cap, chunks done in this loop)
    assert length(0, -1, 0, big, 0) == first                          # nothing known yet
    assert length(0, 12, 0, big, 0) == 12 + margin                    # the count before plus the margin
    assert length(0, 0, 0, big, 0) == margin
    assert length(0, 500, 0, big, 0) == max_chunk                     # the buffers have a fixed size
    assert [length(0, 12, 13, big, nth) for nth in range(1, 9)] == [min(nxt << (nth - 1), max_chunk) for nth in range(1, 9)]      # doubling
    assert length(0, 12, 13, big, 1) == nxt and length(0, 12, 13, big, 40) == max_chunk
    assert length(7, 12, 0, big, 0) == 7 == length(7, -1, 21, big, 3)
    assert length(0, 12, 0, 5, 0) == 5 and length(7, 12, 49, 50, 7) == 1      # never past the cap
    assert length(100, -1, 0, big, 0) == max_chunk
    assert lib.incres_host_chunk_len2(2, 3, 12, 0, big, 0) == 14 and lib.incres_host_chunk_len2(2, 3, 12, 14, big, 2) == 6      # overrides
