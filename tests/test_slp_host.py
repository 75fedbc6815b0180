"""Sparse label propagation without a device: the golden vectors of the reference against both restatement forms of tests/slp_ref.py,
csrc/slp_plan.h compiled for the host (the reverse-entry index, the refusals, the column tiling, a host loop of the contract against
the goldens), graph.adjacency / gradient / divergence against their fixtures, every ValueError of the learner (all raised before
any device call), and the declaration of the entry point.

Regenerate the fixtures with tests/golden/make_golden_slp.py (it needs the reference)."""
import os
import re
import sys
import numpy as np
import pytest
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import slp_ref as ref               # noqa: E402
import graphlearning_amd as gl      # noqa: E402
from graphlearning_amd import _hip  # noqa: E402


def load_golden():
    gold = {}
    for f in ref.GOLDEN_FILES:
        with np.load(os.path.join(ROOT, 'tests', 'golden', f)) as z:
            gold.update({k: z[k] for k in z.files})
    return gold


def golden_graph(gold, g):
    ip, ix, d = gold['graph_%s_indptr' % g], gold['graph_%s_indices' % g], gold['graph_%s_data' % g]
    n = len(ip) - 1
    return sparse.csr_matrix((d, ix, ip), shape=(n, n))


def golden_case(gold, name):
    """(W, train_ind, train_labels, classes, T, the reference's prob)"""
    g, k, T = ref.GOLDEN_CASES[name]
    return golden_graph(gold, g), gold['case_%s_ind' % name], gold['case_%s_labels' % name], k, T, gold['case_%s_prob' % name]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope='module')
def gold():
    return load_golden()


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return ref.build_host_lib(tmp_path_factory.mktemp('slp_plan'))


def test_fixture_graphs_are_what_the_cases_need(gold):
    for g in ref.GOLDEN_GRAPHS:
        W = golden_graph(gold, g)
        assert W.has_canonical_format or ref.canonical(W).nnz == W.nnz
        assert np.diff(W.indptr).min() >= 1 and W.data.min() > 0 and np.all(np.isfinite(W.data))
    assert (abs(golden_graph(gold, 'blobs_dir') - golden_graph(gold, 'blobs_dir').T) > 0).nnz > 0          # reverse entries missing
    deg = np.diff(golden_graph(gold, 'hub_diag').indptr)
    assert deg.max() == 300 and deg.min() == 5 and golden_graph(gold, 'hub_diag').diagonal()[::3].min() == 0.7
    for name, (g, k, T) in ref.GOLDEN_CASES.items():
        share = float(gold['case_%s_clamped' % name])
        assert T < 10 or 0 < share < 1, (name, share)           # both branches of the clamp run


@pytest.mark.parametrize('name', sorted(ref.GOLDEN_CASES))
def test_golden_numpy_form(gold, name):
    W, ind, labels, k, T, prob = golden_case(gold, name)
    u = ref.slp_numpy(W, ind, labels, T)
    assert prob.shape == (W.shape[0], k)
    assert same_bits(u, prob), int((u != prob).sum())
    if T == 0:
        assert not prob.any()


@pytest.mark.parametrize('name', sorted(ref.GOLDEN_CASES))
def test_golden_interpreted_form(gold, name):
    """Entry by entry in Python floats; at most three class columns of a case (the columns are independent)."""
    W, ind, labels, k, T, prob = golden_case(gold, name)
    cols = sorted(set([0, k - 2, k - 1]) & set(range(k)))
    u = ref.slp_python(W, ind, labels, T, cols=cols)
    assert same_bits(u, np.ascontiguousarray(prob[:, cols]))


@pytest.mark.parametrize('name', sorted(ref.GOLDEN_CASES))
def test_golden_host_loop_of_slp_plan(gold, lib, name):
    W, ind, labels, k, T, prob = golden_case(gold, name)
    assert same_bits(ref.host_iterate(lib, W, ind, labels, T, k), prob)


def test_reverse_index_against_numpy(gold, lib):
    graphs = [golden_graph(gold, g) for g in ref.GOLDEN_GRAPHS] + [ref.random_problem(s)[0] for s in range(6)] + [ref.hub_problem(65)[0]]
    graphs.append(sparse.csr_matrix(np.array([[0.7, 0.5, 0.0], [0.5, 0.0, 0.25], [1.0, 0.0, 0.0]])))
    missing = diagonal = 0
    for W in graphs:
        indptr, indices, _, _, _, rev = ref.setup(W)
        got = ref.host_reverse(lib, indptr, indices)
        assert np.array_equal(got.astype(np.int64), rev)
        rows = np.repeat(np.arange(W.shape[0]), np.diff(indptr))
        has = got >= 0
        assert np.array_equal(indices[got[has]], rows[has]) and np.array_equal(rows[got[has]], indices[has])      # (j, i) indeed
        assert np.array_equal(got[indices == rows], np.where(indices == rows)[0])                                  # a diagonal entry is its own
        missing += int((~has).sum())
        diagonal += int((indices == rows).sum())
    assert missing > 0 and diagonal > 0
    assert ref.host_reverse(lib, *ref.setup(graphs[-1])[:2]).tolist() == [0, 2, 1, -1, -1]


def test_column_tiling(lib):
    for C in list(range(1, 70)) + [1000]:
        t = ref.host_tiles(lib, C)
        assert t[0, 0] == 0 and t[:, 1].sum() == C and np.array_equal(t[1:, 0], np.cumsum(t[:-1, 1]))
        assert t[:, 1].max() <= 16 and t[:, 1].min() >= 1 and t[:, 1].max() - t[:, 1].min() <= 1 and t[0, 1] == t[:, 1].max()
        assert len(t) == (C + 15) // 16
        for c0, cols, cpad in t:
            assert cpad in (1, 2, 4, 8, 16) and cols <= cpad < 2 * cols
    assert ref.host_tiles(lib, 17)[:, 1].tolist() == [9, 8]


def test_refusals_of_slp_plan(lib):
    W = ref.random_problem(2)[0]
    indptr, indices, w, lam, gamma, _ = ref.setup(W)
    ind = np.array([0, 5], dtype=np.int32)
    assert ref.host_validate(lib, indptr, indices, w, lam, gamma, 3, ind) == 0

    def changed(arr, at, value):
        out = arr.copy()
        out[at] = value
        return out
    assert ref.host_validate(lib, indptr, indices, w, lam, gamma, 0, ind) == 1                                # C < 1
    assert ref.host_validate(lib, changed(indptr, 0, 1), indices, w, lam, gamma, 3, ind) == 2
    assert ref.host_validate(lib, changed(indptr, 5, indptr[4]), indices, w, lam, gamma, 3, ind) == 3         # row 4 empty
    assert ref.host_validate(lib, indptr, changed(indices, 3, len(indptr) - 1), w, lam, gamma, 3, ind) != 0   # column n
    assert ref.host_validate(lib, indptr, changed(indices, 3, -1), w, lam, gamma, 3, ind) == 4
    swapped = indices.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    assert ref.host_validate(lib, indptr, swapped, w, lam, gamma, 3, ind) == 5                                # not ascending
    assert ref.host_validate(lib, indptr, changed(indices, 1, indices[0]), w, lam, gamma, 3, ind) == 5       # a duplicate
    for bad in (0.0, -0.5, np.nan, np.inf):
        assert ref.host_validate(lib, indptr, indices, changed(w, 7, bad), lam, gamma, 3, ind) == 6
    for bad in (np.nan, np.inf):
        assert ref.host_validate(lib, indptr, indices, w, changed(lam, 7, bad), gamma, 3, ind) == 7
        assert ref.host_validate(lib, indptr, indices, w, lam, changed(gamma, 2, bad), 3, ind) == 7
    assert ref.host_validate(lib, indptr, indices, w, lam, gamma, 3, np.array([0, len(indptr) - 1], dtype=np.int32)) == 8
    assert ref.host_validate(lib, indptr, indices, w, lam, gamma, 3, np.array([-1], dtype=np.int32)) == 8


def _fixture_matrix(gold, key, n):
    return sparse.csr_matrix((gold['calc_%s_data' % key], gold['calc_%s_indices' % key], gold['calc_%s_indptr' % key]), shape=(n, n))


def test_graph_calculus_against_the_reference(gold):
    W = golden_graph(gold, 'blobs_dir')
    n = W.shape[0]
    G = gl.graph(W)
    field = gold['calc_field']
    for key, M in (('adjacency', G.adjacency()), ('grad', G.gradient(field)), ('grad_w', G.gradient(field, weighted=True)),
                   ('grad_p', G.gradient(field, p=0.5))):
        assert sparse.issparse(M) and M.format == 'csr' and M.shape == (n, n) and M.dtype == np.float64, key
        assert np.array_equal(M.toarray(), _fixture_matrix(gold, key, n).toarray()), key
    assert np.array_equal(G.adjacency().toarray(), (W.toarray() != 0).astype(np.float64))
    V = G.gradient(field, weighted=True)
    assert same_bits(np.asarray(G.divergence(V)), gold['calc_div_w'])
    assert same_bits(np.asarray(G.divergence(V, weighted=False)), gold['calc_div'])


def test_learner_attributes():
    W = ref.random_problem(2)[0]
    m = gl.ssl.sparse_label_propagation(W, T=7)
    assert m.name == 'Sparse LP' and m.accuracy_filename == '_sparse_label_propagation' and m.onevsrest is False and m.T == 7
    assert m.get_accuracy_filename() == '_sparse_label_propagation_accuracy.csv'
    assert gl.ssl.sparse_label_propagation(W).T == 100
    assert gl.ssl.sparse_label_propagation(W, class_priors=np.ones(3)).get_accuracy_filename() == '_sparse_label_propagation_classpriors_accuracy.csv'


def test_value_errors_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError('the device call was reached')
    monkeypatch.setattr(_hip, 'slp_iterate', no_device)
    W, ind, labels, k, T = ref.random_problem(2)
    n = W.shape[0]

    def fit(Wx, i=ind, l=labels, **kw):
        return gl.ssl.sparse_label_propagation(Wx, T=3).fit(i, l, **kw)
    with pytest.raises(AssertionError):           # the accepted input gets as far as the device call
        fit(W)
    empty = W.tolil()
    empty[5, :] = 0
    with pytest.raises(ValueError, match='no stored entry'):
        fit(empty.tocsr())
    for bad in (-0.25, np.nan, np.inf, -np.inf):
        Wb = W.copy()
        Wb.data[3] = bad
        with pytest.raises(ValueError, match='negative, NaN or infinite'):
            fit(Wb)
    # a row whose only entries cancel to zero when duplicates are summed: zero after eliminate_zeros means no entry
    rows = np.concatenate([np.repeat(np.arange(n), np.diff(W.indptr)), [5]])
    keep = rows[:-1] != 5
    Wz = sparse.csr_matrix(sparse.coo_matrix((np.concatenate([W.data[keep], [0.0]]), (np.concatenate([rows[:-1][keep], [5]]),
                                                                                         np.concatenate([W.indices[keep], [6]]))), shape=(n, n)))
    with pytest.raises(ValueError, match='no stored entry'):
        fit(Wz)
    with pytest.raises(ValueError, match='out of range'):
        fit(W, i=np.concatenate([ind[:-1], [n]]))
    with pytest.raises(ValueError, match='out of range'):
        fit(W, i=np.concatenate([ind[:-1], [-1]]))
    with pytest.raises(ValueError, match='not exactly 0'):
        fit(W, l=labels + 1)
    with pytest.raises(ValueError, match='not exactly 0'):
        fit(W, l=np.where(labels == 1, 3, labels))
    with pytest.raises(ValueError, match='not exactly 0'):
        fit(W, l=labels + 0.5)
    with pytest.raises(ValueError, match='training indices for'):
        fit(W, l=labels[:-1])
    big = gl.ssl.sparse_label_propagation(W, T=(1 << 30) // (8 * n * k) + 1)
    with pytest.raises(ValueError, match=r'take \d+ bytes'):
        big.fit(ind, labels, all_labels=np.zeros(n, dtype=np.int64))


def test_entry_point_is_declared():
    with open(os.path.join(ROOT, 'include', 'glx_experimental.h')) as f:
        text = f.read()
    assert re.search(r'int glx_slp_iterate\(int64_t n, int64_t M, const int64_t\* row_ptr, const int32_t\* col, const double\* W,', text)
    assert 'glx_slp_iterate' in _hip.EXPORTED_SYMBOLS and callable(_hip.slp_iterate)
    assert len(_hip._SIGNATURES['glx_slp_iterate']) == 16
    with open(os.path.join(ROOT, 'graphlearning_amd', 'csrc', 'slp_plan.h')) as f:
        plan = f.read()
    assert '#include <hip' not in plan and 'glx_internal.h' not in plan      # host only
