"""The exact reference of the scale tests (tests/knn_scale_ref.py) checked on the host: the int64 lists against an all-pairs search in
longdouble, their invariance under the scale ladder in plain fp64 numpy, and -- the reason the scale tests exist -- the split-bf16
filter's arithmetic in numpy float32 against the error bound the acceptance test of the re-rank trusts."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_scale_ref as ref  # noqa: E402


def sample_rows(n, step):
    return np.arange(0, n, step)


@pytest.mark.parametrize('name', sorted(ref.CASES))
def test_the_int64_lists_are_those_of_a_longdouble_search(name):
    M, p, k, ind, D = ref.case(name)
    rows = sample_rows(M.shape[0], 4)
    got_i, got_d = ref.longdouble_knn(ref.points(M, p), k, rows)
    assert np.array_equal(got_i, ind[rows])
    assert got_d.tobytes() == D[rows].tobytes()
    assert np.array_equal(ind[:, 0], np.arange(M.shape[0]))          # no duplicate points: every row finds itself first
    ties = int((D[rows, k - 1] == ref.exact_knn(M, p, k + 1, rows=rows)[1][:, k]).sum())
    print(name, 'sampled rows with a tie at rank k:', ties)


@pytest.mark.parametrize('name', sorted(ref.CASES))
def test_the_lists_are_invariant_under_the_scale_ladder_in_fp64(name):
    M, p, k, ind, D = ref.case(name)
    rows = sample_rows(M.shape[0], 64)
    for e in ref.LADDER:
        X = ref.points(M, p, e)
        assert np.isfinite(X).all() and (np.ldexp(X, -e) == ref.points(M, p)).all(), e         # the scaling itself is exact
        got_i, got_d = ref.float64_knn(X, k, rows)
        assert np.array_equal(got_i, ind[rows]), e
        assert got_d.tobytes() == np.ldexp(D[rows], e).tobytes(), e


def test_where_the_split_bf16_filter_leaves_its_error_bound():
    """|filter value - exact dist^2| <= cerr (|q| + rmax)^2 is a RELATIVE bound: it holds while the fp32 products and sums are
    normal numbers, and fails once they are multiples of 2^-149.  On the `shell` data (|x| = 2^10 2^e), with fp32 subnormals kept
    as the device keeps them: the largest error is 0.047 of the bound at every e down to -70 (the arithmetic scales exactly), 0.36
    at -75, 231 times the bound at -80; below that every filter value is 0.  (At e = -66 the products are still normal: the bound
    holds there.)"""
    M, p, k, ind, D = ref.case('shell')
    rows = sample_rows(M.shape[0], 31)
    cerr = ref.bf16_cerr(M.shape[1])
    ratio = {}
    for e in (0, -24, -66, -75, -80):
        err, bound = ref.bf16_filter_error(ref.points(M, p, e), rows, cerr)
        ratio[e] = float((err / bound).max())
        print('e = %d: largest error / bound = %.4g' % (e, ratio[e]))
    assert ratio[0] < 0.5 and ratio[-24] == ratio[0] and ratio[-66] == ratio[0]
    assert ratio[-75] < 1.0
    assert ratio[-80] > 2.0          # (the acceptance test allows for twice the bound)
