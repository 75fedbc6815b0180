"""The exact kNN search under power-of-two rescaling of the data.

The search promises exact lists, but its candidate filter works on fp32 / split-bf16 images of the centred data, and the acceptance
test of the re-rank trusts a RELATIVE error bound for it.  Multiplying the data by s = 2^e is exact in fp64 and changes no fp64
comparison: the index lists must not change and the distances must be exactly ldexp(D, e), ties included -- at 1e-20 and 1e+20 as
much as at 1.  The unscaled answer comes from the int64 reference of tests/knn_scale_ref.py (lattice data whose distances are
exact in any summation order), so this is not the code agreeing with itself.  Per scale the statistics of the search are printed:
the log shows whether the filter still does the work or the exact fallback has taken over.  (Before the filter's operands were
scaled -- knn_plan.h: knn_filter_scale -- these tests found wrong lists at e = -72, -75, -80 and +55, all of them accepted rows.)

Every test runs under a time limit of its own: a test that exceeds it ends the whole session on the spot (traceback of every
thread, then exit), so nothing more is started on a device that may have hung; nothing is retried."""
import faulthandler
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_scale_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope='module')
def hip():
    from graphlearning_amd import _hip
    _hip.require_device()
    return _hip


def run_ladder(hip, label, M, p, k, want_i, want_d, search, n_queries=None):
    """search(X, k) -> (ind, dist) at every scale of the ladder against the exact lists (want_i, want_d at e = 0).  Every scale is
    run and printed before anything is asserted, so that one log names every scale that fails."""
    nq = M.shape[0] if n_queries is None else n_queries
    wrong, counts, stats = [], {}, {}
    for e in ref.LADDER:
        got_i, got_d = search(ref.points(M, p, e), k)
        st = stats[e] = hip.knn_stats()
        bad_i = int((np.asarray(got_i) != want_i).any(axis=1).sum())
        bad_d = int((np.asarray(got_d).view(np.uint64) != np.ldexp(want_d, e).view(np.uint64)).any(axis=1).sum())
        counts[e] = (int(st['fallback_rows']), int(st['escalated_rows']))
        print('%s e=%+4d: fallback rows %5d of %d, escalated %5d, filter %s KP %d concat %d, visited share %.3f, rows with wrong '
              'indices %d, with wrong distances %d' % (label, e, counts[e][0], nq, counts[e][1], st['filter'], st['KP'], st['concatenated'],
                                                      st['visited_share'], bad_i, bad_d))
        if bad_i or bad_d:
            wrong.append((e, bad_i, bad_d))
    assert not wrong, '%s: (e, rows with wrong indices, rows with wrong distances) %s' % (label, wrong)
    # what keeps the test from passing for the wrong reason: at e = 0 the filter does the work ...
    assert sum(counts[0]) < 0.05 * nq, (label, counts[0])
    # ... and does the same work at every scale.  For e in EXACT_COUNT_RANGE the data is inside the window in which it is taken as it
    # comes (knn_plan.h: knn_filter_scale), the filter's arithmetic scales exactly and the centred norms stay far below the 1e30 of
    # the spare rows: a difference there means that some constant in the code does not scale.  At the other scales the operands are
    # multiplied by an exact power of two before they are rounded, so the filter sees these data times a power of two again, with
    # every product and sum a normal fp32 number as at e = 0: the same roundings, the same comparisons, the same counts.
    for e in ref.LADDER:
        assert counts[e] == counts[0], (label, e, counts[e], counts[0], 'inside the window' if e in ref.EXACT_COUNT_RANGE else 'scaled operands')
    return stats


def bruteforce(hip, **kw):
    return lambda X, k: hip.knn_bruteforce(X, k, **kw)


@pytest.mark.parametrize('name', sorted(ref.CASES))
def test_knnsearch_default_plan(hip, name):
    """weightmatrix.knnsearch as a caller gets it: `gauss200` takes the feature-blocked fp32 filter, `wide` (k = 101) the wide plan
    of a result object, the others the split-bf16 filter with short lists."""
    from graphlearning_amd import weightmatrix
    M, p, k, ind, D = ref.case(name)
    st = run_ladder(hip, name, M, p, k, ind, D, lambda X, k: weightmatrix.knnsearch(X, k))[0]
    if name == 'gauss200':
        assert st['filter'] == 'f32' and st['dpa'] > 132
    if name == 'wide':
        assert st['wide']


@pytest.mark.parametrize('name,opts', [('gauss20', dict(filter='f32')), ('gauss20', dict(filter='bf16', concat=0)),
                                       ('gauss20', dict(filter='bf16', concat=1)), ('gauss20', dict(filter='bf16', concat=2)),
                                       ('mixed', dict(concat=0)), ('mixed', dict(concat=1)),
                                       ('shell', dict(lists='short')), ('shell', dict(lists='long'))],
                         ids=lambda v: v if isinstance(v, str) else '-'.join('%s=%s' % kv for kv in sorted(v.items())))
def test_every_plan_override(hip, name, opts):
    M, p, k, ind, D = ref.case(name)
    with hip.knn_options(**opts):
        st = run_ladder(hip, '%s %s' % (name, opts), M, p, k, ind, D, bruteforce(hip, clustered=0))[0]
    if 'concat' in opts:
        assert st['filter'] == 'bf16x3' and st['concatenated'] == opts['concat']
    if opts.get('filter') == 'f32' or opts.get('lists') == 'long':
        assert st['filter'] == 'f32'


def test_result_object_lists_at_k_101(hip):
    M, p, k, ind, D = ref.case('wide')

    def search(X, k):
        res = hip.KnnResult(X, k)
        try:
            return res.lists()
        finally:
            res.close()
    run_ladder(hip, 'KnnResult k=101', M, p, k, ind, D, search)


def test_query_range(hip):
    M, p, k, ind, D = ref.case('gauss20')
    run_ladder(hip, 'query_range', M, p, k, ind[300:811], D[300:811], bruteforce(hip, query_range=(300, 811)), n_queries=511)


def test_cells_formed_by_the_library(hip):
    """clustered=16: the rows reordered by cell, the seeded thresholds and the bound ub2 that decides which cells a block visits."""
    M, p, k, ind, D = ref.case('blobs')
    st = run_ladder(hip, 'clustered=16', M, p, k, ind, D, bruteforce(hip, clustered=16))[0]
    print('clustered=16 at e = 0:', st)
    assert st['cells'] == 16 and 0 < st['visited_share'] < 1         # the pruning is at work where the filter is


def test_cells_given_by_the_caller(hip):
    """cell_starts= from dist_build.coarse_locality_order (worked out once, on the unscaled data): the same pruned search on rows
    that come in cells."""
    from graphlearning_amd import dist_build
    M, p, k, _, _ = ref.case('blobs')
    perm, starts = dist_build.coarse_locality_order(ref.points(M, p), ncells=16, return_cells=True)
    Mp = np.ascontiguousarray(M[perm])
    ind, D, _ = ref.exact_knn(Mp, p, k)
    st = run_ladder(hip, 'cell_starts', Mp, p, k, ind, D, bruteforce(hip, cell_starts=starts))[0]
    print('cell_starts at e = 0:', st)
    assert st['cells'] == 16 and 0 < st['visited_share'] < 1         # the pruning is at work where the filter is


WEIGHT_SCALES = (0, -24, -66, -100, 60, 100)
KERNELS = ('gaussian', 'symgaussian', 'uniform', 'distance', 'singular')


def check_weights(hip):
    from graphlearning_amd import weightmatrix
    M, p, k, ind, D = ref.case('gauss20')              # k = 11 with self: weightmatrix.knn's k = 10
    n = M.shape[0]
    edges = np.zeros((n, n), dtype=bool)
    edges[np.repeat(np.arange(n), k - 1), ind[:, 1:].ravel()] = True
    edges |= edges.T
    for kernel in KERNELS:
        base = None
        for e in WEIGHT_SCALES:
            W = weightmatrix.knn(ref.points(M, p, e), k - 1, kernel=kernel)
            if base is None:
                base = W
                assert np.array_equal(W.toarray() != 0, edges), kernel        # the graph of the exact lists
            assert np.array_equal(W.indptr, base.indptr) and np.array_equal(W.indices, base.indices), (kernel, e)
            shift = {'distance': e, 'singular': -e}.get(kernel, 0)
            same = W.data.tobytes() == np.ldexp(base.data, shift).tobytes()
            print('weights %s e=%+4d: %s' % (kernel, e, 'same bits' if same else 'DIFFERENT'))
            assert same, (kernel, e)


def test_weight_matrices_with_the_host_exponential(hip):
    assert os.environ.get('GLX_HOST_EXP') == '1'
    check_weights(hip)


def test_weight_matrices_with_the_device_exponential(hip, device_exp):
    assert os.environ.get('GLX_HOST_EXP') is None
    check_weights(hip)


NEIGHBOUR_SCALES = (0, -66, -100, -400, 100, 400)


def test_nearest_dist(hip):
    M, p, k, _, _ = ref.case('gauss3')
    idx = np.arange(7, M.shape[0], 41)
    D2, pmin = ref.exact_sqdist(M, p, idx)
    want = np.ldexp(np.sqrt(D2.min(axis=1).astype(np.float64)), pmin)
    for e in NEIGHBOUR_SCALES:
        got = hip.nearest_dist(ref.points(M, p, e), idx)
        assert np.asarray(got).tobytes() == np.ldexp(want, e).tobytes(), e


def test_epsilon_ball(hip):
    from graphlearning_amd import weightmatrix
    M, p, k, _, _ = ref.case('gauss3')
    n, eps = M.shape[0], 64
    D2, pmin = ref.exact_sqdist(M, p, np.arange(n))
    assert pmin == 0
    pairs = D2 <= eps * eps                              # (a pair AT distance epsilon belongs)
    np.fill_diagonal(pairs, False)
    print('epsilon_ball: %d pairs, %d at distance epsilon exactly' % (pairs.sum() // 2, (D2 == eps * eps).sum() // 2))
    base = None
    for e in NEIGHBOUR_SCALES:
        W = weightmatrix.epsilon_ball(ref.points(M, p, e), float(np.ldexp(float(eps), e)))
        if base is None:
            base = W
            assert np.array_equal(W.toarray() != 0, pairs)
        assert np.array_equal(W.indptr, base.indptr) and np.array_equal(W.indices, base.indices), e
        assert W.data.tobytes() == base.data.tobytes(), e
