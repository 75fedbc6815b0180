"""Active learning without a device: csrc/acq_plan.h compiled for the host against a plain-numpy loop in the same documented order
(bit for bit) and against the reference's recorded rounds (within the fixture's bounds, every query reproduced), its validation codes
and tie rule, unc_sampling and the full-storage forms against the reference's recorded values, the reference's three defects handled
as the module states, the refusals raised before any device call, and the declaration of the entry points.

Regenerate the fixture with tests/golden/make_golden_al.py (it needs the reference)."""
import os
import re
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import al_ref as ref                # noqa: E402
import graphlearning_amd as gl      # noqa: E402
from graphlearning_amd import _hip  # noqa: E402

al = gl.active_learning


@pytest.fixture(scope='module')
def gold():
    return ref.load_golden()


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return ref.build_host_lib(tmp_path_factory.mktemp('acq_plan'))


class StubModel:
    """a learner that needs no device: fit returns one-hot rows of the labels it was given, 0.5 elsewhere"""

    def __init__(self, n, k):
        self.graph = type('g', (), {'num_nodes': n})()
        self.k = k
        self.fits = 0

    def fit(self, ind, labels):
        self.fits += 1
        u = np.full((self.graph.num_nodes, self.k), 0.5) + 0.001 * np.arange(self.graph.num_nodes)[:, None] * np.arange(1, self.k + 1)[None, :]
        u[ind] = np.eye(self.k)[labels]
        return u


def test_the_fixture_is_what_the_tests_need(gold):
    assert len(ref.GOLDEN_CASES) == 19 and os.path.getsize(os.path.join(ROOT, 'tests', 'golden', ref.GOLDEN_FILE)) < 1 << 20
    for c in ref.CONDITIONINGS:
        assert 0 < float(gold['bound_vals_' + c]) and 0 < float(gold['bound_C_' + c])
        assert float(gold['min_gap_' + c]) >= 8 * float(gold['bound_vals_' + c])
    for name, case in ref.GOLDEN_CASES.items():
        for r in range(ref.ROUNDS):
            key = 'case_%s_r%d_' % (name, r)
            assert gold[key + 'query'].shape == (case['batch'],) and gold[key + 'w'].shape == (case['batch'], 50)
            assert gold[key + 'top_val'].shape == (ref.TOP,)
            assert (key + 'vals' in gold) == (r in ref.FULL_ROUNDS)
            if case['policy'] == 'max':          # the recorded values decide the recorded query with the margin over the bound
                assert float(ref.top_gaps(gold[key + 'top_val'], 5 if case['batch'] > 1 else 1).min()) >= 8 * float(gold['bound_vals_' + case['cond']])


@pytest.mark.parametrize('M', ref.SHAPE_M)
def test_plan_arithmetic_equals_the_numpy_loop_bit_for_bit(lib, M):
    for n in ref.SHAPE_N:
        V, C, cand, unc = ref.random_problem(1, n, M)
        assert len(np.unique(cand)) < len(cand) or n == 1            # repeated, unsorted candidates
        for kind in (ref.VAR, ref.SIGMA, ref.MC, ref.MCVAR):
            got = ref.host_compute(lib, V, C, kind, cand, unc)
            want = ref.numpy_compute(V, C, kind, cand, unc)
            assert ref.same_bits(got, want), (n, M, kind)
        query = cand[:4]
        assert ref.same_bits(ref.host_update(lib, V, C, query), ref.numpy_update(V, C, query)), (n, M)
        if M <= 65:
            b = min(3, len(np.unique(cand)))
            for kind in (ref.VAR, ref.SIGMA):
                rc, q, qv = ref.host_greedy(lib, V, C, kind, cand, b)
                nq, nqv = ref.numpy_greedy(V, C, kind, cand, b)
                assert rc == 0 and np.array_equal(q, nq) and ref.same_bits(qv, nqv), (n, M, kind)


def test_validation_codes(lib):
    V, C, cand, unc = ref.random_problem(0, 65, 4)

    def changed(arr, at, value):
        out = arr.copy()
        out[at] = value
        return out
    assert ref.host_validate_state(lib, V, C) == 0
    assert ref.host_validate_state(lib, V, C, n=0) == 1 and ref.host_validate_state(lib, V, C, M=0) == 1
    for bad in (np.nan, np.inf, -np.inf):
        assert ref.host_validate_state(lib, changed(V, (64, 3), bad), C) == 2
        assert ref.host_validate_state(lib, V, changed(C, (3, 3), bad)) == 2
        assert ref.host_validate_state(lib, V, C, gamma2=bad) == 2
    V256, C256, _, _ = ref.random_problem(0, 3, 256)
    assert ref.host_validate_state(lib, V256, C256) == 0
    V257 = np.zeros((3, 257))
    assert ref.host_validate_state(lib, V257, np.eye(257)) == 8                      # unsupported, before the arrays are looked at
    assert ref.host_validate_state(lib, changed(V257, (0, 0), np.nan), np.eye(257)) == 8
    for kind in range(4):
        assert ref.host_validate_cand(lib, 65, kind, cand) == 0
    assert ref.host_validate_cand(lib, 65, 4, cand) == 3 and ref.host_validate_cand(lib, 65, -1, cand) == 3
    assert ref.host_validate_cand(lib, 65, ref.MC, cand, greedy=True) == 3 and ref.host_validate_cand(lib, 65, ref.SIGMA, cand, greedy=True) == 0
    assert ref.host_validate_cand(lib, 65, ref.VAR, changed(cand, 5, 65)) == 4 and ref.host_validate_cand(lib, 65, ref.VAR, changed(cand, 5, -1)) == 4
    assert ref.host_validate_cand(lib, 65, ref.VAR, cand[:0]) == 0                     # no candidate is legal
    with pytest.raises(ValueError, match='refused'):
        ref.host_compute(lib, V, C, ref.MC, cand, None)                                # the multiplier is required there
    # more rounds than distinct vertices
    assert ref.host_greedy(lib, V, C, ref.VAR, [3, 3, 5], 3)[0] == -100 and ref.host_greedy(lib, V, C, ref.VAR, [3, 3, 5], 2)[0] == 0
    # a round without a finite maximum is named: gamma2 = 0 and a zero row give 0 / 0 in the only round
    Vz = V.copy()
    Vz[7] = 0.0
    rc, q, qv = ref.host_greedy(lib, Vz, C, ref.VAR, [7, 7], 1, gamma2=0.0)
    assert rc == 1


def test_tiling_rule(lib):
    """64 candidates per workgroup while 56 KiB of LDS hold their rows of V and of w, halved down to 8 at M = 256; the update holds C
    in LDS up to M = 80, within the 64 KiB a workgroup may ask for"""
    seen = set()
    for M in range(1, 257):
        rows, lds, upd = ref.host_tiling(lib, M)
        seen.add(rows)
        assert rows in (8, 16, 32, 64) and 256 % rows == 0 and lds == 2 * rows * (M | 1) * 8 <= 56 * 1024
        assert rows == 64 or 2 * lds > 56 * 1024                                       # the next size up would not fit
        assert upd == (M * (M | 1) * 8 if M <= 80 else 0) and upd + 2 * 256 * 8 + 64 <= 64 * 1024
    assert seen == {8, 16, 32, 64}
    assert [ref.host_tiling(lib, M)[0] for M in (50, 54, 56, 110, 112, 222, 224, 256)] == [64, 64, 32, 32, 16, 16, 8, 8]


def test_greedy_tie_rule_first_position_wins(lib):
    V, C, _, _ = ref.random_problem(2, 64, 5, ties=True)
    assert np.array_equal(V[0], V[1])
    for kind in (ref.VAR, ref.SIGMA):
        cand = np.arange(64)
        rc, q, qv = ref.host_greedy(lib, V, C, kind, cand, 4)
        vals = ref.host_compute(lib, V, C, kind, cand)
        assert rc == 0 and vals[q[0]] == qv[0] and q[0] % 2 == 0 and vals[q[0] + 1] == vals[q[0]]      # the twin has the same value and loses
        back = cand[::-1].copy()                                                      # the same vertices the other way round: now the odd twin comes first
        rc, q2, qv2 = ref.host_greedy(lib, V, C, kind, back, 4)
        assert rc == 0 and back[q2[0]] == q[0] + 1 and qv2[0] == qv[0]
    # the rule itself: larger wins, equal goes to the smaller position, NaN beats numbers, no candidate never wins
    better = lambda *a: bool(lib.acq_host_better(*a))                               # noqa: E731
    assert better(2.0, 5, 1.0, 1) and not better(1.0, 1, 2.0, 5) and better(1.0, 1, 1.0, 5) and not better(1.0, 5, 1.0, 1)
    assert better(np.nan, 9, np.inf, 0) and not better(np.inf, 0, np.nan, 9) and better(np.nan, 1, np.nan, 2) and not better(np.nan, 2, np.nan, 1)
    assert not better(5.0, -1, 1.0, 3) and better(-np.inf, 3, 0.0, -1)


@pytest.mark.parametrize('name', sorted(ref.GOLDEN_CASES))
def test_host_plan_against_the_reference_rounds(gold, lib, name):
    """the plan with its own C from the same start: values and C within the fixture's bounds in every round, the reference's query
    reproduced by the module's own selection expressions"""
    case = ref.GOLDEN_CASES[name]
    W, truth, V, C0, ind, labels, subset = ref.case_state(gold, name)
    kind, key = ref.KINDS[case['acq']], 'case_%s_' % name
    bound_vals, bound_C = float(gold['bound_vals_' + case['cond']]), float(gold['bound_C_' + case['cond']])
    Cref = ref.reference_C_sequence(gold, name)
    C = ref.host_update(lib, V, C0, ind)
    labeled = ind.copy()
    unc_fn = al.unc_sampling()
    worst_v = worst_c = 0.0
    for r in range(ref.ROUNDS):
        cand = subset if subset is not None else np.setdiff1d(np.arange(len(truth)), labeled)
        query, top = gold[key + 'r%d_query' % r], gold[key + 'r%d_top_pos' % r]
        assert ref.rel_diff(C, Cref[r]) <= bound_C
        if kind >= ref.MC and r not in ref.FULL_ROUNDS:          # the rows of u that are stored: the best six
            unc = unc_fn.compute(gold[key + 'r%d_top_u' % r], np.arange(ref.TOP))
            vals = ref.host_compute(lib, V, C, kind, cand[top], unc)
            want = gold[key + 'r%d_top_val' % r]
            assert cand[top][np.argmax(vals)] == query[0], r
        else:
            unc = unc_fn.compute(gold[key + 'r%d_u' % r], cand) if kind >= ref.MC else None
            vals = ref.host_compute(lib, V, C, kind, cand, unc)
            want = gold[key + 'r%d_vals' % r] if r in ref.FULL_ROUNDS else gold[key + 'r%d_top_val' % r]
            if case['policy'] == 'max':
                assert np.array_equal(cand[(-vals).argsort()[:case['batch']]], query), r
            else:
                saved = np.random.get_state()
                try:
                    np.random.set_state(ref.numpy_state(gold, name, r))
                    probs = np.exp(1.0 * (vals - vals.max()))
                    probs /= probs.sum()
                    assert np.array_equal(np.random.choice(cand, case['batch'], p=probs), query), r
                finally:
                    np.random.set_state(saved)
            if r not in ref.FULL_ROUNDS:
                vals = vals[top]
        worst_v = max(worst_v, float(np.abs(vals - want).max() / np.abs(gold[key + 'r%d_top_val' % r][0])))
        assert np.abs(vals - want).max() <= bound_vals * abs(gold[key + 'r%d_top_val' % r][0]), r
        C = ref.host_update(lib, V, C, query)
        labeled = np.append(labeled, query)
        worst_c = max(worst_c, ref.rel_diff(C, Cref[r + 1]))
    assert ref.rel_diff(C, Cref[ref.ROUNDS]) <= bound_C
    print(name, 'values differ by up to', worst_v, 'of', bound_vals, 'C by up to', worst_c, 'of', bound_C)


def test_unc_sampling_all_six_methods(gold):
    u = gold['case_%s_r0_u' % ref.UNC_CASE]
    cand = ref.unc_candidates(len(u))
    assert al.unc_sampling().unc_method == 'smallest_margin' and al.unc_sampling.METHODS == ref.UNC_METHODS
    for method in ref.UNC_METHODS:
        got = al.unc_sampling(unc_method=method).compute(u, cand)
        assert got.shape == (len(cand),) and np.allclose(got, gold['unc_' + method], rtol=1e-13, atol=1e-15), method
    with pytest.raises(ValueError, match='unc_method'):
        al.unc_sampling(unc_method='margin').compute(u, cand)


def test_full_storage_forms_against_the_reference(gold, monkeypatch):
    monkeypatch.setattr(_hip, 'Acq', lambda *a, **k: (_ for _ in ()).throw(AssertionError('a device handle was created')))
    n, u = ref.FULL_N, gold['full_u']
    every, some = np.arange(n), np.array([31, 2, 2, 17, 39])
    for acq in ref.KINDS:
        f = getattr(al, acq)(C=ref.full_C(n))
        assert f.storage == 'full' and f.V is None and f.gamma2 == ref.GAMMA2
        assert np.allclose(f.compute(u, every), gold['full_%s_vals0' % acq], rtol=1e-13, atol=0)
        # a candidate subset: the reference raises for the two model-change criteria (it broadcasts n against the candidate count)
        assert np.allclose(f.compute(u, some), gold['full_%s_vals0' % acq][some], rtol=1e-13, atol=0)
        f.update(ref.FULL_QUERIES, None)
        assert np.allclose(f.C, gold['full_C'], rtol=1e-13, atol=0)
        assert np.allclose(f.compute(u, every), gold['full_%s_vals1' % acq], rtol=1e-13, atol=0)
    # the greedy design with full storage: what rounds of compute / argmax / update choose, C untouched
    f = al.var_opt(C=ref.full_C(n))
    before = f.C.copy()
    q, vals = f.greedy(every, 4)
    assert ref.same_bits(f.C, before)
    twin = al.var_opt(C=ref.full_C(n))
    left = every.copy()
    for r in range(4):
        v = twin.compute(None, left)
        k = left[np.argmax(v)]
        assert k == q[r] and v.max() == vals[r]
        twin.update([k], None)
        left = left[left != k]


def test_learner_loop_and_the_reference_defects_handled_as_stated(gold):
    n = ref.FULL_N
    model = StubModel(n, 3)
    ind, labels = np.array([0, 1, 2]), np.array([0, 1, 2])
    AL = al.active_learner(model, al.unc_sampling, ind, labels)
    assert isinstance(AL.acq_function, al.unc_sampling) and AL.policy == 'max' and model.fits == 1
    assert np.array_equal(AL.labeled_ind, ind) and np.array_equal(AL.labels, labels) and AL.u.shape == (n, 3)
    assert np.array_equal(AL.unlabeled_ind, np.arange(3, n))
    q, vals = AL.select_queries(2, return_acq_vals=True)
    assert vals.shape == (n - 3,) and np.array_equal(q, AL.unlabeled_ind[(-vals).argsort()[:2]])
    # defect 1: 'full' with allow_repeat=True uses all vertices (the reference calls np.arange on an array and raises)
    q, vals = AL.select_queries(1, allow_repeat=True, return_acq_vals=True)
    assert vals.shape == (n,)
    # defect 2: a candidate index == n is refused (the reference tests > n and then indexes out of range)
    with pytest.raises(ValueError, match='candidate_ind'):
        AL.select_queries(1, candidate_ind=np.array([1, n]))
    with pytest.raises(ValueError, match='candidate_ind'):
        AL.select_queries(1, candidate_ind=np.array([-1, 2]))
    assert AL.select_queries(1, candidate_ind=np.array([n - 1])) == n - 1
    with pytest.raises(ValueError, match='Invalid input'):
        AL.select_queries(1, candidate_ind='half')
    # defect 3: model_change with full storage on the unlabelled vertices (the reference broadcasts n against n - 3 and raises)
    AL3 = al.active_learner(StubModel(n, 3), al.model_change, ind, labels, C=ref.full_C(n))
    q, vals = AL3.select_queries(1, return_acq_vals=True)
    assert vals.shape == (n - 3,) and q[0] == AL3.unlabeled_ind[np.argmax(vals)]
    # update: the labels grow, the model is fitted again, the acquisition function is told
    before = AL3.acq_function.C.copy()
    AL3.update(q, np.array([1]))
    assert len(AL3.labeled_ind) == 4 and AL3.labels[-1] == 1 and AL3.model.fits == 2 and q[0] not in AL3.unlabeled_ind
    assert not np.array_equal(AL3.acq_function.C, before)
    # policies: 'prop' and 'rand' draw from numpy's global stream with the reference's calls
    np.random.seed(5)
    got = AL.select_queries(2, policy='prop', prop_gamma=2.0)
    np.random.seed(5)
    vals = AL.acq_function.compute(AL.u, AL.unlabeled_ind)
    probs = np.exp(2.0 * (vals - vals.max()))
    probs /= probs.sum()
    assert np.array_equal(got, np.random.choice(AL.unlabeled_ind, 2, p=probs))
    np.random.seed(6)
    got, vals = AL.select_queries(1, candidate_ind='rand', rand_frac=0.5, return_acq_vals=True)
    np.random.seed(6)
    cand = np.random.choice(AL.unlabeled_ind, size=int(0.5 * len(AL.unlabeled_ind)), replace=False)
    assert len(vals) == len(cand) and got[0] == cand[np.argmax(vals)]
    assert AL.select_queries(3, policy=lambda cand, vals, b: cand[:b]).tolist() == [3, 4, 5]          # a callable is passed through
    # select_greedy: only for the criteria that do not look at labels
    with pytest.raises(TypeError, match='var_opt or sigma_opt'):
        AL3.select_greedy(2)
    with pytest.raises(TypeError, match='var_opt or sigma_opt'):
        AL.select_greedy(2)
    AL4 = al.active_learner(StubModel(n, 3), al.sigma_opt, ind, labels, C=ref.full_C(n))
    before, fits = AL4.acq_function.C.copy(), AL4.model.fits
    picks = AL4.select_greedy(3)
    assert ref.same_bits(AL4.acq_function.C, before) and AL4.model.fits == fits and len(AL4.labeled_ind) == 3
    for k in picks:
        assert AL4.select_queries(1)[0] == k
        AL4.update(np.array([k]), np.array([0]))


def test_value_errors_before_any_device_call(monkeypatch):
    monkeypatch.setattr(_hip, 'Acq', lambda *a, **k: (_ for _ in ()).throw(AssertionError('a device handle was created')))
    monkeypatch.setattr(_hip, 'load', lambda *a, **k: (_ for _ in ()).throw(AssertionError('the library was loaded')))
    V, C, cand, unc = ref.random_problem(0, 30, 4)
    for bad in (np.nan, np.inf):
        for acq in ref.KINDS:
            Cb, Vb = C.copy(), V.copy()
            Cb[1, 2] = bad
            Vb[29, 3] = bad
            with pytest.raises(ValueError, match='NaN or infinite'):
                getattr(al, acq)(C=Cb, V=V)
            with pytest.raises(ValueError, match='NaN or infinite'):
                getattr(al, acq)(C=C, V=Vb)
            with pytest.raises(ValueError, match='not finite'):
                getattr(al, acq)(C=C, V=V, gamma2=bad)
    with pytest.raises(ValueError, match='at most 256'):
        al.var_opt(C=np.eye(257), V=np.zeros((3, 257)))
    with pytest.raises(ValueError, match='not square'):
        al.var_opt(C=np.ones((4, 5)), V=V)
    with pytest.raises(ValueError, match='does not go with'):
        al.var_opt(C=np.eye(5), V=V)
    with pytest.raises(ValueError, match='does not go with'):
        al.sigma_opt(C=np.eye(4), V=V[:, 0])
    f = al.model_change(C=C, V=V)
    assert f.storage == 'trunc' and f.unc_sampling.unc_method == 'smallest_margin' and ref.same_bits(f.C, C)
    u = np.full((30, 2), 0.5)
    u[4, 1] = np.nan
    with pytest.raises(ValueError, match='NaN or infinite'):
        f.compute(u, np.arange(30))
    with pytest.raises(ValueError, match=r'\[0, 30\)'):
        al.var_opt(C=C, V=V).compute(None, np.array([0, 30]))
    with pytest.raises(ValueError, match=r'\[0, 30\)'):
        al.var_opt(C=C, V=V).update(np.array([-1]), None)
    with pytest.raises(ValueError, match='distinct'):
        al.var_opt(C=C, V=V).greedy(np.array([1, 1, 2]), 3)
    with pytest.raises(TypeError, match='looks at labels'):
        f.greedy(np.arange(30), 2)
    # the positional order of the reference
    g = al.model_change_var_opt(C, V, 0.5, 'entropy')
    assert g.gamma2 == 0.5 and g.unc_sampling.unc_method == 'entropy'
    assert al.var_opt(C, V, 0.25).gamma2 == 0.25


def test_truncated_forms_have_no_cpu_fallback(monkeypatch):
    def no_library(*a, **k):
        raise gl.GlxError('libglx.so not found')
    monkeypatch.setattr(_hip, 'load', no_library)
    V, C, cand, unc = ref.random_problem(0, 30, 4)
    f = al.var_opt(C=C, V=V)
    with pytest.raises(gl.GlxError):
        f.compute(None, np.arange(30))
    with pytest.raises(gl.GlxError):
        f.update(np.array([3]), None)
    assert al.unc_sampling().compute(np.random.default_rng(0).random((30, 3)), np.arange(30)).shape == (30,)
    assert al.var_opt(C=ref.full_C(30)).compute(None, np.arange(30)).shape == (30,)


def test_the_stand_alone_program_of_the_host_plan(tmp_path):
    exe = str(tmp_path / 'acq_plan_main')
    subprocess.run(['g++', '-O2', '-ffp-contract=off', '-std=c++17', '-DACQ_PLAN_MAIN', '-I' + os.path.join(ROOT, 'graphlearning_amd', 'csrc'),
                    '-o', exe, os.path.join(ROOT, 'tests', 'acq_plan_host.cpp')], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith('ok first '), (res.returncode, res.stdout)


def test_entry_points_are_declared():
    names = ['glx_acq_create', 'glx_acq_compute', 'glx_acq_update', 'glx_acq_greedy', 'glx_acq_get_c', 'glx_acq_stats', 'glx_acq_destroy']
    with open(os.path.join(ROOT, 'include', 'glx_experimental.h')) as f:
        text = f.read()
    with open(os.path.join(ROOT, 'include', 'glx.h')) as f:
        stable = f.read()
    with open(os.path.join(ROOT, 'graphlearning_amd', 'csrc', 'acq.hip')) as f:
        kern = f.read()
    for name in names:
        decl = re.search(r'int %s\(([^;]*)\);' % name, text)
        assert decl and name not in stable, name
        assert name in _hip.EXPORTED_SYMBOLS and len(_hip._SIGNATURES[name]) == decl.group(1).count(',') + 1, name
        assert re.search(r'extern "C" int %s\(' % name, kern), name
    assert sorted(n for n in _hip.EXPORTED_SYMBOLS if n.startswith('glx_acq_')) == sorted(names)
    assert (_hip.ACQ_VAR, _hip.ACQ_SIGMA, _hip.ACQ_MC, _hip.ACQ_MCVAR) == (ref.VAR, ref.SIGMA, ref.MC, ref.MCVAR)
    for k, name in enumerate(('VAR', 'SIGMA', 'MC', 'MCVAR')):
        assert re.search(r'#define GLX_ACQ_%s %d\b' % (name, k), text)
    assert _hip.ACQ_MAX_M == 256 and al.MAX_M == 256 and hasattr(gl, 'active_learning')
    if _hip.load(required=False) is not None:
        for name in names:
            assert getattr(_hip.load(), name) is not None
    with open(os.path.join(ROOT, 'graphlearning_amd', 'csrc', 'acq_plan.h')) as f:
        plan = f.read()
    assert 'glx_internal.h' not in plan and 'hip_runtime' not in plan                                   # builds on the host alone
    assert not re.search(r'atomicAdd|unsafeAtomicAdd|cooperative_groups|hipMemsetAsync|__builtin_amdgcn_mfma|fma\(', kern)
    assert kern.count('#pragma clang fp contract(off)') == 2                                            # the pass and the rank-one step
    assert 'matplotlib' not in open(os.path.join(ROOT, 'graphlearning_amd', 'active_learning.py')).read().replace('matplotlib is not', '')
