"""tests/weights_cr_ref.py, the bit-for-bit reference of the default mode's Gaussian weights, checked on the host: its fast
path against pure Decimal, csrc/exp_cr.h (compiled with gcc) against it where the result is subnormal or zero, the census of
the underflow lists from the reference alone, and the reference against the golden weight matrices within the bounds the older
tests allow (the golden files hold one host's numpy exp: within an ulp of the correctly rounded one)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weights_cr_ref as ref  # noqa: E402
from test_exp_cr import _arguments  # noqa: E402

THRESHOLDS = (-745.2, -745.1332191019412, -708.3964185322641, 709.782712893384)
TINY = np.ldexp(1.0, -1022)


def threshold_neighbours():
    """Every threshold of the exponential with the two doubles on either side of it."""
    out = []
    for t in THRESHOLDS:
        lo = hi = t
        out.append(t)
        for _ in range(2):
            lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
            out += [lo, hi]
    return np.array(out)


def band_arguments():
    """Arguments across the underflow band (normal results at the top, zero at the bottom) and the threshold neighbours."""
    return np.concatenate([np.random.default_rng(5).uniform(-746, -707, 30000), threshold_neighbours()])


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('which', ['exp_cr_arguments', 'uniform', 'thresholds'])
def test_fast_path_equals_pure_decimal(which):
    x = {'exp_cr_arguments': _arguments, 'uniform': lambda: np.random.default_rng(6).uniform(-760, 0, 20000),
         'thresholds': threshold_neighbours}[which]()
    stats = {}
    fast = ref.exp_contract(x, stats)
    if np.finfo(np.longdouble).nmant >= 63:         # (without an 80-bit long double exp_contract is pure Decimal itself)
        print('%s: %d of %d values went to Decimal' % (which, stats['decimal'], len(x)))
        assert 0 < stats['decimal'] < len(x) // 4 or which == 'thresholds'
    assert same_bits(fast, ref.exp_contract_decimal(x))


def test_pass_throughs_and_the_second_rounding_by_hand():
    out = ref.exp_contract(np.array([np.nan, np.inf, -np.inf, 800.0, -800.0, 0.0, -745.3]))
    assert np.isnan(out[0]) and out[1] == np.inf and out[2] == 0.0 and out[3] == np.inf and out[4] == 0.0 and out[5] == 1.0 and out[6] == 0.0
    # np.ldexp(m, -200) rounds to nearest even onto the subnormal grid: the same as one exact and one rounded multiplication
    x = np.random.default_rng(7).uniform(-745.2, -708, 2000)
    for v in x[:200]:
        e = ref._exp_decimal(v)
        from decimal import localcontext
        with localcontext() as c:
            c.prec = 140
            m = float(e * ref._TWO200)
        assert float(np.ldexp(m, -200)) == (m * 2.0 ** -100) * 2.0 ** -100 == ref.exp_contract_scalar(v)
    # above the band the second rounding changes nothing
    y = np.random.default_rng(8).uniform(-708, -700, 500)
    assert same_bits(ref.exp_contract_decimal(y), ref.exp_rounded_once(y))


def test_header_on_the_host_in_the_underflow_band(tmp_path):
    """csrc/exp_cr.h below 2^-1022 -- results that are subnormal, or zero -- against exp_contract, bit for bit: the header's
    documented two roundings.  Of the 30 020 arguments 28 236 have a subnormal result, 709 are zero, and 274 results differ from
    the exact exponential rounded ONCE (each by one unit of the subnormal grid)."""
    src = tmp_path / 'exp_host.c'
    src.write_text('#include "%s"\nvoid exp_cr_array(const double* x, double* out, long n) { for (long i = 0; i < n; ++i) out[i] = exp_cr(x[i]); }\n'
                   % os.path.join(ROOT, 'graphlearning_amd', 'csrc', 'exp_cr.h'))
    so = tmp_path / 'libexpcr.so'
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-shared', '-fPIC', '-o', str(so), str(src), '-lm'], check=True)
    lib = ctypes.CDLL(str(so))
    x = band_arguments()
    out = np.empty_like(x)
    lib.exp_cr_array(x.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_long(len(x)))
    want = ref.exp_contract(x)
    once = ref.exp_rounded_once(x)
    differ = once.view(np.int64) != want.view(np.int64)
    print('underflow band: %d arguments, %d subnormal results, %d zeros, %d normal; the two-step contract differs from a single rounding in %d'
          % (len(x), int(((want > 0) & (want < TINY)).sum()), int((want == 0).sum()), int((want >= TINY).sum()), int(differ.sum())))
    assert ((want > 0) & (want < TINY)).sum() > 20000 and (want == 0).sum() > 100 and (want >= TINY).sum() > 100
    assert same_bits(out, want)
    # the second rounding moves a result by one unit of the subnormal grid at most, and only below 2^-1022
    assert np.abs(once.view(np.int64) - want.view(np.int64)).max() <= 1 and not differ[want >= TINY].any()
    assert (differ.sum(), int(((want > 0) & (want < TINY)).sum()), int((want == 0).sum())) == (274, 28236, 709)


def test_census_of_the_underflow_lists():
    """What tests/test_gpu_weights_exact.py::test_underflow rests on, from the reference alone (measured: 744 subnormal weights,
    65 in the lowest four normal binades, 330 zeros of which 30 outside the last column, 10 two-step differences, arguments down
    to -750; 17 340 stored entries against the uniform kernel's 18 000)."""
    ind, d = ref.underflow_lists()
    n, K = ind.shape
    x = ref.knn_arguments(ind, d, K - 1, 'symgaussian')
    w = ref.exp_contract(x)
    c = ref.census(x, w)
    print(c)
    assert c['subnormal'] >= 200 and c['zeros_inside'] >= 20 and c['low_normal'] >= 30 and c['two_step_differs'] >= 3
    assert c['lowest_argument'] <= -749
    for symmetrize in (True, False):
        Wg = ref.knn_weights_cr(ind, d, K - 1, 'symgaussian', symmetrize)
        Wu = ref.assemble(ind, np.ones_like(d), 'max' if symmetrize else 'none')
        print('symmetrize=%s: %d stored entries, uniform kernel %d' % (symmetrize, Wg.nnz, Wu.nnz))
        assert Wg.nnz < Wu.nnz
        assert ((Wg.data > 0) & (Wg.data < TINY)).sum() >= 200


@pytest.mark.parametrize('kernel,most', [('gaussian', 2), ('symgaussian', 8)])
def test_reference_within_the_old_bounds_of_the_golden_matrices(golden, kernel, most):
    """The same function as the reference's: on the golden two-moons lists, the structure of the stored matrices and their
    weights within the ulp bounds of tests/test_gpu_knn.py (the stored weights carry their host's numpy exp)."""
    from conftest import csr_from
    g = golden('g1_twomoons.npz')
    W = ref.knn_weights_cr(g['knn_ind'], g['knn_dist'], 10, kernel)
    Wg = csr_from(g, 'W_' + kernel)
    assert np.array_equal(W.indptr, Wg.indptr) and np.array_equal(W.indices, Wg.indices)
    ulps = np.abs(W.data.view(np.int64) - Wg.data.view(np.int64))
    print(kernel, 'ulps from the golden matrix:', np.bincount(np.minimum(ulps, 9)))
    assert ulps.max() <= most
    if kernel == 'gaussian':
        Wn = ref.knn_weights_cr(g['knn_ind'], g['knn_dist'], 10, kernel, symmetrize=False)
        Wgn = csr_from(g, 'W_gaussian_nosym')
        assert np.array_equal(Wn.indices, Wgn.indices)
        assert np.abs(Wn.data.view(np.int64) - Wgn.data.view(np.int64)).max() <= 1
