"""graphlearning_amd.active_learning and _hip.Acq on the device: the device against csrc/acq_plan.h on the host BIT FOR BIT (values, C
after updates, the greedy design's queries and values) at the shapes where the kernels can go wrong; the acquisition values, C and the
query against the reference's recorded rounds; the whole active_learner loop with this package's ssl.laplace against the reference's
query sequences; select_greedy against rounds of select_queries / update on a twin learner; refusals that leave the device usable;
device handling.

Every test runs under a time limit of its own: a test that exceeds it ends the whole session on the spot (traceback of every
thread, then exit), so nothing more is started on a device that may have hung; nothing is retried."""
import faulthandler
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import al_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
# the host tests' grid and the two shapes of the issue: several thousand rows (65 workgroups, a short last tile), the widest M off a tile
SHAPES = [(n, M) for M in ref.SHAPE_M for n in ref.SHAPE_N] + [(4097, 50), (300, 256)]


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope='module')
def gl():
    import graphlearning_amd as gl
    from graphlearning_amd import _hip
    _hip.require_device()
    return gl


@pytest.fixture(scope='module')
def gold():
    return ref.load_golden()


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return ref.build_host_lib(tmp_path_factory.mktemp('acq_plan'))


def acq(V, C, gamma2=ref.GAMMA2, device=None):
    from graphlearning_amd import _hip
    return _hip.Acq(V, C, gamma2, device=device)


@pytest.mark.parametrize('M', ref.SHAPE_M + (50,))
def test_device_equals_host_restatement_bit_for_bit(gl, lib, M):
    for n, _ in [s for s in SHAPES if s[1] == M]:
        V, C, cand, unc = ref.random_problem(1, n, M, ties=(n == 129))
        with acq(V, C) as h:
            for kind in (ref.VAR, ref.SIGMA, ref.MC, ref.MCVAR):
                got = h.compute(kind, cand, unc)
                assert ref.same_bits(got, ref.host_compute(lib, V, C, kind, cand, unc)), (n, M, kind)
                assert ref.same_bits(h.compute(kind, cand, unc), got), (n, M, kind)           # a second call: identical bits
            assert h.compute(ref.VAR, cand[:0]).shape == (0,) and h.stats()['pass_launches'] == 8      # no candidate: nothing launched
            assert ref.same_bits(h.get_c(), C)
            b = min(5, len(np.unique(cand)))
            for kind in (ref.VAR, ref.SIGMA):
                rc, q, qv = ref.host_greedy(lib, V, C, kind, cand, b)
                dq, dqv = h.greedy(kind, cand, b)
                assert rc == 0 and np.array_equal(dq, q) and ref.same_bits(dqv, qv), (n, M, kind)
            assert ref.same_bits(h.get_c(), C) and h.stats()['greedy_launches'] == 4 * b           # the greedy design leaves C alone
            query = cand[:4]                                                                      # a batch with whatever repeats it holds
            h.update(query)
            C1 = ref.host_update(lib, V, C, query)
            assert ref.same_bits(h.get_c(), C1), (n, M)
            h.update(query[:1])
            h.update(query[:0])
            C2 = ref.host_update(lib, V, C1, query[:1])
            assert ref.same_bits(h.get_c(), C2) and h.stats()['update_launches'] == 2, (n, M)
            assert ref.same_bits(h.compute(ref.VAR, cand), ref.host_compute(lib, V, C2, ref.VAR, cand)), (n, M)
            st = h.stats()
            assert (st['tile_rows'], st['pass_lds'], st['update_lds']) == ref.host_tiling(lib, M) and (st['n'], st['M']) == (n, M)


@pytest.mark.parametrize('name', sorted(ref.GOLDEN_CASES))
def test_values_C_and_argmax_against_the_reference_rounds(gl, gold, name):
    """from the recorded u and the recorded candidates: values within bound_vals and C within bound_C in every round, the reference's
    query chosen by the module's own selection expressions"""
    al = gl.active_learning
    case = ref.GOLDEN_CASES[name]
    W, truth, V, C0, ind, labels, subset = ref.case_state(gold, name)
    kind, key = ref.KINDS[case['acq']], 'case_%s_' % name
    bound_vals, bound_C = float(gold['bound_vals_' + case['cond']]), float(gold['bound_C_' + case['cond']])
    Cref = ref.reference_C_sequence(gold, name)
    f = getattr(al, case['acq'])(C=C0, V=V)
    f.update(ind, labels)
    labeled = ind.copy()
    worst_v = worst_c = 0.0
    for r in range(ref.ROUNDS):
        cand = subset if subset is not None else np.setdiff1d(np.arange(len(truth)), labeled)
        query, top, big = gold[key + 'r%d_query' % r], gold[key + 'r%d_top_pos' % r], abs(gold[key + 'r%d_top_val' % r][0])
        worst_c = max(worst_c, ref.rel_diff(f.C, Cref[r]))
        assert ref.rel_diff(f.C, Cref[r]) <= bound_C, r
        if kind >= ref.MC and r not in ref.FULL_ROUNDS:          # the rows of u that are stored: those of the best six
            u = np.zeros((len(truth), gold[key + 'r%d_top_u' % r].shape[1]))
            u[cand[top]] = gold[key + 'r%d_top_u' % r]
            vals, want = f.compute(u, cand[top]), gold[key + 'r%d_top_val' % r]
            assert cand[top][np.argmax(vals)] == query[0], r
        else:
            vals = f.compute(gold[key + 'r%d_u' % r] if kind >= ref.MC else None, cand)
            if case['policy'] == 'max':
                assert np.array_equal(cand[(-vals).argsort()[:case['batch']]], query), r
                assert cand[np.argmax(vals)] == query[0], r
            if r in ref.FULL_ROUNDS:
                want = gold[key + 'r%d_vals' % r]
            else:
                vals, want = vals[top], gold[key + 'r%d_top_val' % r]
        worst_v = max(worst_v, float(np.abs(vals - want).max() / big))
        assert np.abs(vals - want).max() <= bound_vals * big, r
        f.update(query, truth[query])
        labeled = np.append(labeled, query)
    assert ref.rel_diff(f.C, Cref[ref.ROUNDS]) <= bound_C
    print(name, 'values differ by up to', worst_v, 'of', bound_vals, 'C by up to', worst_c, 'of', bound_C)
    f.close()


def learner(gl, gold, name, policy=None):
    case = ref.GOLDEN_CASES[name]
    W, truth, V, C0, ind, labels, subset = ref.case_state(gold, name)
    model = gl.ssl.laplace(W)
    AL = gl.active_learning.active_learner(model, getattr(gl.active_learning, case['acq']), ind, labels, policy or case['policy'], C=C0.copy(), V=V.copy())
    return AL, truth, subset


@pytest.mark.parametrize('name', sorted(ref.GOLDEN_CASES))
def test_whole_loop_reproduces_the_reference_queries(gl, gold, name):
    """the active_learner loop with this package's ssl.laplace and the stored eigenpairs: the reference's query in every round"""
    case = ref.GOLDEN_CASES[name]
    AL, truth, subset = learner(gl, gold, name)
    key = 'case_%s_' % name
    saved = np.random.get_state()
    try:
        for r in range(ref.ROUNDS):
            if case['policy'] == 'prop':
                np.random.set_state(ref.numpy_state(gold, name, r))
            q = AL.select_queries(case['batch'], candidate_ind=('full' if subset is None else subset))
            assert np.array_equal(q, gold[key + 'r%d_query' % r]), (r, q, gold[key + 'r%d_query' % r])
            AL.update(q, truth[q])
    finally:
        np.random.set_state(saved)
    assert len(AL.labeled_ind) == len(np.unique(truth)) + ref.ROUNDS * case['batch']
    AL.acq_function.close()


@pytest.mark.parametrize('name', ['%s_%s_%s' % (g, a, c) for g in ('blobs', 'moons') for a in ('var_opt', 'sigma_opt') for c in ref.CONDITIONINGS])
def test_select_greedy_equals_rounds_on_a_twin(gl, gold, name):
    AL, truth, _ = learner(gl, gold, name)
    twin, _, _ = learner(gl, gold, name)
    before = AL.acq_function.C
    picks = AL.select_greedy(ref.ROUNDS)
    assert ref.same_bits(AL.acq_function.C, before) and len(AL.labeled_ind) == len(np.unique(truth))      # neither C nor the learner changed
    loop = []
    for r in range(ref.ROUNDS):
        q = twin.select_queries(1)
        loop.append(int(q[0]))
        twin.update(q, truth[q])
    recorded = [int(gold['case_%s_r%d_query' % (name, r)][0]) for r in range(ref.ROUNDS)]
    assert picks.tolist() == loop == recorded
    AL.update(picks, truth[picks])
    assert ref.same_bits(AL.acq_function.C, twin.acq_function.C)
    assert np.array_equal(AL.labeled_ind, twin.labeled_ind) and np.array_equal(AL.unlabeled_ind, twin.unlabeled_ind)
    AL.acq_function.close()
    twin.acq_function.close()


def test_refusals_leave_the_device_usable(gl, gold, lib):
    from graphlearning_amd import _hip
    V, C, cand, unc = ref.random_problem(3, 65, 5)
    want = ref.host_compute(lib, V, C, ref.VAR, cand)
    h = acq(V, C)

    def still_works():
        assert ref.same_bits(h.compute(ref.VAR, cand), want)
    with pytest.raises(gl.GlxError, match='at most 256'):
        acq(np.zeros((3, 257)), np.eye(257))
    still_works()
    with pytest.raises(gl.GlxError, match='not finite'):
        acq(V, C, gamma2=np.nan)
    still_works()
    with pytest.raises(gl.GlxError, match='vertices'):
        h.greedy(ref.VAR, np.array([3, 3, 5]), 3)
    still_works()
    with pytest.raises(gl.GlxError, match='rounds'):
        h.greedy(ref.VAR, np.array([3, 5]), 3)
    still_works()
    for bad in (65, -1):
        with pytest.raises(gl.GlxError, match='outside'):
            h.compute(ref.VAR, np.array([0, bad]))
        with pytest.raises(gl.GlxError, match='outside'):
            h.update(np.array([bad]))
        with pytest.raises(gl.GlxError, match='outside'):
            h.greedy(ref.SIGMA, np.array([0, bad]), 1)
        still_works()
    with pytest.raises(gl.GlxError, match='kind'):
        h.greedy(ref.MC, cand, 1)
    with pytest.raises(gl.GlxError, match='kind'):
        h.compute(7, cand)
    with pytest.raises(gl.GlxError, match='multiplier'):
        h.compute(ref.MCVAR, cand)
    still_works()
    assert ref.same_bits(h.get_c(), C)
    closed = acq(V, C)
    closed.close()
    closed.close()
    for call in (lambda: closed.compute(ref.VAR, cand), lambda: closed.update(cand[:1]), lambda: closed.greedy(ref.VAR, cand, 1), closed.get_c,
                 closed.stats):
        with pytest.raises(gl.GlxError, match='closed'):
            call()
    still_works()
    AL, truth, _ = learner(gl, gold, 'moons_model_change_e2')
    with pytest.raises(TypeError, match='var_opt or sigma_opt'):
        AL.select_greedy(3)
    assert len(AL.select_queries(2)) == 2
    AL2, truth, _ = learner(gl, gold, 'moons_var_opt_e2')
    with pytest.raises(ValueError, match='distinct'):
        AL2.select_greedy(len(AL2.unlabeled_ind) + 1)
    with pytest.raises(ValueError, match='candidate_ind'):
        AL2.select_greedy(1, candidate_ind=np.array([0, len(truth)]))
    assert len(AL2.select_greedy(2)) == 2
    still_works()
    h.close()


def test_device_argument_default_device_and_release(gl, lib):
    from graphlearning_amd import _hip
    V, C, cand, unc = ref.random_problem(4, 65, 5)
    want = ref.host_compute(lib, V, C, ref.SIGMA, cand)
    last = _hip.device_count() - 1
    with acq(V, C, device=last) as h:
        assert ref.same_bits(h.compute(ref.SIGMA, cand), want)
    f = gl.active_learning.sigma_opt(C=C, V=V, device=last)
    assert ref.same_bits(f.compute(None, cand), want) and f._acq is not None
    f.update(cand[:2], None)
    C1 = f.C
    f.close()                                              # the covariance comes back to the host; the next call uploads it again
    assert f._acq is None and ref.same_bits(f.C, C1) and ref.same_bits(C1, ref.host_update(lib, V, C, cand[:2]))
    assert ref.same_bits(f.compute(None, cand), ref.host_compute(lib, V, C1, ref.SIGMA, cand))
    # the default device (GLX_DEVICE at import, set_default_device later) is what a call without `device` uses
    saved = _hip.default_device()
    assert saved == _hip._dev(None) and _hip._dev(last) == last
    try:
        _hip.set_default_device(last)
        assert _hip._dev(None) == last
        with acq(V, C) as h:
            assert ref.same_bits(h.compute(ref.SIGMA, cand), want)
    finally:
        _hip.set_default_device(saved)
    # garbage collection releases the handle: creating and dropping many does not exhaust anything
    for _ in range(20):
        acq(V, C)
    gc.collect()
    with acq(V, C) as h:
        assert ref.same_bits(h.compute(ref.SIGMA, cand), want)
