"""The label decision without a GPU: the restatement tests/decision_ref.py equals oracle/gl_oracle.py bit for bit and reproduces
the golden vectors of the reference (tests/golden/g5_projection.npz), and every input of tests/test_gpu_decision.py ends the way
it is there for -- on the step cap, by convergence, after exactly one or two steps --, so that a case cannot quietly degenerate."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decision_ref as ref  # noqa: E402
import decision_cases as dc  # noqa: E402
from oracle import gl_oracle as orc  # noqa: E402


def same(a, b):
    """Two (labels, weights, err, steps) results, bit for bit (NaN weights in the same places)."""
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True) and a[1].dtype == b[1].dtype == np.float64
            and (a[2] == b[2] or (a[2] != a[2] and b[2] != b[2])) and a[3] == b[3])


# the oracle has no step cap: only inputs that stop by themselves, or whose 10^4 steps are cheap
@pytest.mark.parametrize('dtype', sorted(dc.DTYPES))
@pytest.mark.parametrize('name', ['C1', 'C2', 'C3', 'C4', 'C5', 'n255', 'one_step', 'two_steps', 'argmin_C5', 'n257'])
def test_restatement_equals_the_oracle(name, dtype):
    c = dc.build(name, dtype)
    for w in (1, 1 + 0.1 * np.arange(c['prob'].shape[1])):
        assert np.array_equal(ref.predict(c['prob'], w, c['similarity']), orc.predict(c['prob'], w, c['similarity']))
    want = orc.volume_label_projection(c['prob'], c['priors'], c['weights'], c['similarity'])
    got = ref.volume_label_projection(c['prob'], c['priors'], c['weights'], c['similarity'])
    assert same(got, want)
    again = ref.volume_label_projection(c['prob'], c['priors'], got[1], c['similarity'])         # from the first call's weights
    assert same(again, orc.volume_label_projection(c['prob'], c['priors'], want[1], c['similarity']))
    if want[3] > 3:     # a cap below the stopping step ends there, with the weights the uncapped run had at that step
        capped = ref.volume_label_projection(c['prob'], c['priors'], c['weights'], c['similarity'], max_steps=3)
        assert capped[3] == 3 and capped[2] > 1e-3
    none = ref.volume_label_projection(c['prob'], c['priors'], c['weights'], c['similarity'], max_steps=0)
    assert none[3] == 0 and none[2] == 1 and np.array_equal(none[0], ref.predict(c['prob'], c['weights'], c['similarity']))


def test_restatement_equals_the_oracle_on_degenerate_input():
    for kind in dc.DEGENERATE:
        if kind in ('constant', 'nan', 'inf', 'w0_zero'):     # these stop at once or never: 10^4 steps of the oracle on 500 x 4 are cheap
            c = dc.build('deg_' + kind, 'f64')
            with np.errstate(all='ignore'):
                want = orc.volume_label_projection(c['prob'], c['priors'], c['weights'], True)
                got = ref.volume_label_projection(c['prob'], c['priors'], c['weights'], True)
            assert same(got, want), kind


def test_restatement_equals_the_golden_vectors(golden):
    """Both calls of tests/golden/make_golden.py g5_projection: what the file holds of them (labels and weights of both, err
    and step count of the first)."""
    g = golden('g5_projection.npz')
    assert np.array_equal(ref.predict(g['prob']), g['pred_plain'])
    lab, w, err, it = ref.volume_label_projection(g['prob'], g['priors'], 1)
    assert it == int(g['iters_1']) and it > 1 and err == float(g['err_1'])
    assert np.array_equal(w, g['weights_1']) and np.array_equal(lab, g['labels_1'])
    lab2, w2, err2, it2 = ref.volume_label_projection(g['prob'], g['priors'], w)
    assert np.array_equal(w2, g['weights_2']) and np.array_equal(lab2, g['labels_2'])
    assert same((lab2, w2, err2, it2), orc.volume_label_projection(g['prob'], g['priors'], w))


def test_float32_input_is_normalised_in_float32():
    prob = dc.draw(2000, 6, 90).astype(np.float32)
    s = ref.scores_of(prob)
    assert s.dtype == np.float32 and (s * np.ones(6)).dtype == np.float64
    assert not np.array_equal(s, ref.scores_of(prob.astype(np.float64)))


@pytest.mark.parametrize('dtype', sorted(dc.DTYPES))
@pytest.mark.parametrize('name', sorted(dc.CASES))
def test_case_ends_as_stated(name, dtype):
    c, res = dc.case_and_ref(name, dtype)
    assert dc.ends_as_stated(name, res, c), (name, dtype, res[3], res[2])
    assert c['prob'].dtype == dc.DTYPES[dtype]


def test_cases_cover_what_they_are_there_for():
    # a 'conv' case that stops exactly on a host look (2 + 4 + 8 + 16 = 30 steps) and ones between looks
    assert dc.case_and_ref('C4', 'f64')[1][3] in dc.LOOKS
    assert dc.case_and_ref('C5', 'f64')[1][3] not in dc.LOOKS
    # C > 256 beyond the first four looks, with float32 rounding that shows in the weights
    a, b = dc.case_and_ref('C257', 'f64')[1], dc.case_and_ref('C257', 'f32')[1]
    assert a[3] > 94 and b[3] > 94 and not np.array_equal(a[1], b[1])
    # most bins of the widest histogram are empty
    c, res = dc.case_and_ref('C4096', 'f64')
    assert 300 < len(np.unique(res[0])) < 600
    # ties: some row's best score is shared by two classes under unit weights, in both directions
    for name, pick in (('ties_argmax', np.max), ('ties_argmin', np.min)):
        c, _ = dc.case_and_ref(name, 'f64')
        s = ref.scores_of(c['prob'])
        assert (np.sum(s == pick(s, axis=1)[:, None], axis=1) > 1).sum() > 500
    # degenerate inputs do what the test says of them
    c, res = dc.case_and_ref('deg_constant', 'f64')
    with np.errstate(all='ignore'):
        assert np.isnan(ref.scores_of(c['prob'])).all() and (res[0] == 0).all()
    for kind in ('nan', 'inf'):
        c, res = dc.case_and_ref('deg_' + kind, 'f64')
        with np.errstate(all='ignore'):
            assert np.isnan(ref.scores_of(c['prob'])).any()
    c, _ = dc.case_and_ref('deg_priors_sum', 'f64')
    assert abs(np.sum(c['priors']) - 1.3) < 1e-12
    # the row count above which the argmax pass strides its grid
    assert dc.case_and_ref('n530000', 'f64')[0]['prob'].shape[0] > 2048 * 256


@pytest.mark.parametrize('dtype', sorted(dc.DTYPES))
def test_step_caps_stop_the_two_inputs_as_stated(dtype):
    natural = dc.cap_case_and_ref('conv', 10000, dtype)[1][3]
    assert 30 < natural < 62                                    # it stops by itself between the fourth and the fifth look
    for cap in dc.CAPS:
        _, res = dc.cap_case_and_ref('never', cap, dtype)
        assert res[3] == cap and res[2] > 1e-3, cap             # the cap is what stops it
        _, res = dc.cap_case_and_ref('conv', cap, dtype)
        assert res[3] == min(cap, natural) and (res[2] <= 1e-3) == (cap >= natural), cap


@pytest.mark.parametrize('dtype', sorted(dc.DTYPES))
def test_reuse_sequence_ends_as_stated(dtype):
    steps = [dc.reuse_case_and_ref(pos, dtype)[1][3] for pos in range(len(dc.REUSE))]
    assert steps[0] == steps[5] and 30 < steps[0] < 10000 and steps[1:5] == [60, 30, 30, 1]
