"""ssl.dynamic_label_propagation and _hip.dlp_solve on the device: the device against dlp_host_reference (csrc/dlp_plan.h built on the
host) BIT FOR BIT, final iterate and every iterate of the history, on seeded graphs at the shapes where the kernels can go wrong and
beyond the reference's cap of 5000 vertices; the learner against the reference's golden vectors within the bound measured when the
fixture was made, predict() equal on every vertex, the lines of an all_labels fit, ssl_trials' file, and the refusals.

Every test runs under a time limit of its own: a test that exceeds it ends the whole session on the spot (traceback of every
thread, then exit), so nothing more is started on a device that may have hung; nothing is retried."""
import faulthandler
import os
import sys

import numpy as np
import pytest
from scipy import sparse

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dlp_ref as ref  # noqa: E402
from test_dlp_host import load_golden, golden_case, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu


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
    return load_golden()


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return ref.build_host_lib(tmp_path_factory.mktemp('dlp_plan'))


def solve(P, ind, val, **kw):
    from graphlearning_amd import _hip
    return _hip.dlp_solve(P.indptr, P.indices, P.data, ind, val, want_history=kw.pop('want_history', True), **kw)


def plan_for(n, T):
    """launches (the start, the sparse passes, two kernels per Gram), sparse passes, Gram passes, partials per Gram entry"""
    sparse_passes, grams = T * T + max(T - 2, 0), T * (T - 1) // 2
    return (1 + sparse_passes + 2 * grams, sparse_passes, grams, (n + 63) // 64)


def check_against_host(lib, P, ind, val, **kw):
    want, want_hist = ref.host_solve(lib, P.indptr, P.indices, P.data, ind, val, **kw)
    assert np.all(np.isfinite(want))
    u, hist, plan = solve(P, ind, val, **kw)
    T = kw.get('T', 2)
    print(P.shape[0], val.shape[1], T, 'differing values', int((u != want).sum()), 'in the history', int((hist != want_hist).sum()), 'plan', plan)
    assert same_bits(u, want) and same_bits(hist, want_hist)
    assert plan == plan_for(P.shape[0], T)
    return u, hist


# n, k, T, options: one vertex; one partial short of, exactly and just past 64 rows; three partials with the widest Gram (k = 64: four
# column tiles of 16, 4096 entries, 32 KB of LDS) and tiles of unequal width (k = 17: 9 + 8); ten partials at T = 6 (15 Grams, Y_5, both R
# buffers); 65 partials (n = 4097: chain 0 of the finishing kernel holds two) with one row of 3 000 entries among rows of 10
SHAPES = [(1, 1, 1, {}), (63, 2, 2, {}), (64, 3, 3, {}), (65, 17, 2, {}), (129, 64, 3, {}), (600, 3, 6, {}), (2000, 10, 2, {}),
          (4097, 10, 3, {'hub': 3000, 'deg': 10, 'exact': True})]


@pytest.mark.parametrize('n,k,T,options', SHAPES)
def test_seeded_shapes_bit_for_bit(gl, lib, n, k, T, options):
    P, ind, val = ref.random_problem(n, n, k, **options)
    if options.get('hub'):
        assert sorted(np.unique(np.diff(P.indptr)).tolist()) == [10, 3000]
    u, hist = check_against_host(lib, P, ind, val, T=T)
    assert same_bits(u[ind], val) and same_bits(hist[-1], u)


# n, k: uneven column tiles together with a ragged last row block, the smallest shapes at which a wrong first column or width of a tile
# shows in the sparse pass or the Gram pass: k = 1 and 16 are one tile, 17 is 9 + 8, 33 is three tiles of 11; n = 65 and 130 leave the 64
# rows of a partial with a remainder of one row and of two ((65, 17) is among SHAPES).  T = 3: three Grams, an epilogue with and without
# the reset of the training rows
TILE_SHAPES = [(65, 1), (65, 16), (65, 33), (130, 1), (130, 16), (130, 17), (130, 33)]


@pytest.mark.parametrize('n,k', TILE_SHAPES)
def test_uneven_tiles_on_a_ragged_row_block_bit_for_bit(gl, lib, n, k):
    P, ind, val = ref.random_problem(n + k, n, k)
    u, hist = check_against_host(lib, P, ind, val, T=3)
    assert same_bits(u[ind], val) and same_bits(hist[-1], u)


def test_the_directed_golden_graph_bit_for_bit(gl, gold, lib):
    W, truth, ind, labels, k, params = golden_case(gold, 'directed_T3')
    P = ref.transition(W)
    assert (abs(P - P.T) > 0).nnz > 0
    check_against_host(lib, P, ind, ref.onehot(labels, k), **params)


def test_special_inputs_bit_for_bit(gl, lib):
    """Negative values and rows without entries; a vertex listed twice takes its last row; every vertex a training vertex; alpha = 0
    and lam = 0 are evaluated as written; without a history the same final iterate; a second call returns identical bits."""
    P, ind, val = ref.random_problem(7, 300, 5, empty_rows=3)
    assert (P.data < 0).any() and (np.diff(P.indptr) == 0).sum() == 3
    first, first_hist = check_against_host(lib, P, ind, val, T=3)
    again, again_hist, _ = solve(P, ind, val, T=3)
    assert same_bits(again, first) and same_bits(again_hist, first_hist)
    plain, none, plan = solve(P, ind, val, T=3, want_history=False)
    assert none is None and same_bits(plain, first) and plan == plan_for(300, 3)
    twice_ind, twice_val = np.concatenate([ind, ind[:2]]), np.concatenate([val, val[2:4]])
    u, _ = check_against_host(lib, P, twice_ind, twice_val, T=3)
    assert same_bits(u[ind[:2]], val[2:4]) and not same_bits(val[:2], val[2:4])
    for alpha, lam in ((0.0, 0.1), (0.05, 0.0), (0.0, 0.0)):
        check_against_host(lib, P, ind, val, alpha=alpha, lam=lam, T=3)
    P, ind, val = ref.random_problem(8, 130, 3, all_train=True)
    u, hist = check_against_host(lib, P, ind, val, T=3)
    want = np.zeros((130, 3))
    want[ind] = val
    assert all(same_bits(h, want) for h in hist)


def test_twenty_thousand_vertices_bit_for_bit(gl, lib):
    """Four times the reference's cap: 10 entries in every row, 10 classes, T = 3."""
    P, ind, val = ref.random_problem(20, 20000, 10, deg=10, exact=True)
    assert np.all(np.diff(P.indptr) == 10)
    check_against_host(lib, P, ind, val, T=3)


def test_the_learner_solves_5001_vertices(gl, lib):
    """The reference prints "Cannot use Dynamic Label Propagation on large datasets." there and returns the one-hot start."""
    W = abs(ref.random_problem(21, 5001, 4, deg=8, symmetric=True)[0])
    ind = np.arange(0, 5001, 250)
    labels = np.arange(len(ind)) % 4
    model = gl.ssl.dynamic_label_propagation(W)
    u = model.fit(ind, labels)
    start = np.zeros((5001, 4))
    start[ind] = ref.onehot(labels, 4)
    assert not np.array_equal(u, start) and np.count_nonzero(np.any(u != 0, axis=1)) > len(ind)
    P = ref.transition(W)
    want, _ = ref.host_solve(lib, P.indptr, P.indices, P.data, ind, ref.onehot(labels, 4), want_history=False)
    assert same_bits(np.ascontiguousarray(u), want) and model.num_iter == 2 and model.dlp_plan == plan_for(5001, 2)


@pytest.mark.parametrize('name', sorted(ref.GOLDEN_CASES))
def test_golden_within_the_measured_bound(gl, gold, lib, name, capsys):
    W, truth, ind, labels, k, params = golden_case(gold, name)
    prob, bound = gold['case_%s_prob' % name], float(gold['bound_prob'])
    model = gl.ssl.dynamic_label_propagation(W, **params)
    u = model.fit(ind, labels)
    diff = np.abs(u - prob).max() / np.abs(prob).max()
    print(name, 'largest difference / largest entry', diff, 'bound', bound, 'plan', model.dlp_plan)
    assert diff <= bound
    assert np.array_equal(model.predict(), gold['case_%s_pred' % name])
    assert model.num_iter == params['T'] and model.dlp_plan == plan_for(W.shape[0], params['T'])
    with_priors = gl.ssl.dynamic_label_propagation(W, class_priors=gold['case_%s_priors' % name], **params)
    assert np.array_equal(with_priors.fit_predict(ind, labels), gold['case_%s_pred_priors' % name])
    assert same_bits(np.ascontiguousarray(with_priors.prob), np.ascontiguousarray(u))
    # and the device is the host reference, bit for bit
    P = ref.transition(W)
    want, _ = ref.host_solve(lib, P.indptr, P.indices, P.data, ind, ref.onehot(labels, k), want_history=False, **params)
    assert same_bits(np.ascontiguousarray(u), want)
    if name in ref.LINES_CASES:
        capsys.readouterr()
        lined = gl.ssl.dynamic_label_propagation(W, **params)
        u_lines = lined.fit(ind, labels, all_labels=truth)
        out = capsys.readouterr().out.splitlines()
        assert out == [str(s) for s in gold['case_%s_lines' % name]]
        assert same_bits(np.ascontiguousarray(u_lines), np.ascontiguousarray(u))


def test_a_stored_diagonal_changes_nothing(gl, gold):
    W, truth, ind, labels, k, params = golden_case(gold, 'blobs')
    plain = gl.ssl.dynamic_label_propagation(W).fit(ind, labels)
    d = np.zeros(W.shape[0])
    d[::3] = 0.7
    loops = gl.ssl.dynamic_label_propagation(sparse.csr_matrix(W + sparse.diags(d))).fit(ind, labels)
    assert same_bits(np.ascontiguousarray(loops), np.ascontiguousarray(plain))


def test_ssl_trials_writes_the_reference_format(gl, gold, tmp_path, monkeypatch):
    W, truth, ind, labels, k, params = golden_case(gold, 'blobs')
    rng = np.random.default_rng(3)
    other = np.concatenate([rng.choice(np.where(truth == c)[0], size=2, replace=False) for c in range(k)])
    monkeypatch.setattr(gl.ssl, 'results_dir', str(tmp_path / 'results'))
    model = gl.ssl.dynamic_label_propagation(W)
    model.ssl_trials([other, ind], truth, tag='dlp_')
    path = tmp_path / 'results' / 'dlp__dynamic_label_propagation_accuracy.csv'
    lines = path.read_text().splitlines()
    assert lines[0] == 'Number of labels,Accuracy' and len(lines) == 3
    counts = [int(s.split(',')[0]) for s in lines[1:]]
    assert counts == [len(other), len(ind)]
    acc = gl.ssl.ssl_accuracy(gl.ssl.dynamic_label_propagation(W).fit_predict(ind, labels), truth, ind)
    assert lines[2] == '%d,%.2f' % (len(ind), acc)
    assert model.trials_statistics(tag='dlp_')[0].tolist() == sorted(counts)


def test_refusals(gl, monkeypatch):
    from graphlearning_amd import _hip
    P, ind, val = ref.random_problem(9, 130, 3)
    wide = np.zeros((len(ind), 65))
    wide[:, 0] = 1.0
    with pytest.raises(_hip.GlxError, match=r'glx_dlp_solve failed \(-4\)'):          # GLX_EUNSUPPORTED
        solve(P, ind, wide)
    with pytest.raises(_hip.GlxError, match=r'glx_dlp_solve failed \(-4\)'):
        solve(P, ind, val, T=65)
    with pytest.raises(_hip.GlxError, match=r'glx_dlp_solve failed \(-1\)'):          # GLX_EINVAL
        solve(P, ind, val, T=0)
    with pytest.raises(_hip.GlxError, match=r'glx_dlp_solve failed \(-1\)'):
        solve(P, ind, val, alpha=np.nan)
    bad = P.copy()
    bad.indices[3] = 130
    with pytest.raises(_hip.GlxError, match=r'glx_dlp_solve failed \(-1\)'):
        solve(bad, ind, val)
    assert same_bits(solve(P, ind, val)[0], solve(P, ind, val)[0])                    # and the library goes on working
    calls = []
    real = _hip.dlp_solve
    monkeypatch.setattr(_hip, 'dlp_solve', lambda *a, **k: calls.append(a) or real(*a, **k))
    W = abs(ref.random_problem(6, 120, 3, symmetric=True)[0])
    ind, labels = np.array([0, 5, 17, 40, 80, 119]), np.array([0, 1, 2, 0, 1, 2])
    lonely = W.tolil()
    lonely[5, :] = 0
    nan = W.copy()
    nan.data[3] = np.nan
    for Wx, i, l, kw in ((lonely.tocsr(), ind, labels, {}), (nan, ind, labels, {}), (W, ind, labels, {'T': 0}), (W, ind, labels, {'T': 65}),
                         (W, ind, labels, {'alpha': np.inf}), (W, ind, labels, {'lam': np.nan}), (W, ind + 1, labels, {}), (W, ind, labels + 1, {}),
                         (W, ind, labels[:-1], {}), (W, ind[:0], labels[:0], {})):
        with pytest.raises(ValueError):
            gl.ssl.dynamic_label_propagation(Wx, **kw).fit(i, l)
    assert not calls
    gl.ssl.dynamic_label_propagation(W).fit(ind, labels)
    assert len(calls) == 1
