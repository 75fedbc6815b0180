"""weightmatrix.epsilon_ball without a GPU: the restatement tests/epsball_ref.py equals every golden vector of the reference
(tests/golden/g13_epsball*.npz, written by tests/golden/make_golden_epsball.py); the HIP-free headers the kernels are built from
-- numpy's row sum (csrc/npsum_exact.h), the tree-order squared distance (csrc/sqdist_tree.h), the search plan
(csrc/ball_plan.h) -- compiled for the host; and the refusals of the public function, which come before the library is loaded."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epsball_ref as ref  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
_vp = ctypes.c_void_p


def load_golden():
    head = np.load(os.path.join(GOLDEN, 'g13_epsball.npz'))
    files = {}
    out = {}
    for name, fn in zip(head['case_names'], head['case_files']):
        if fn not in files:
            files[fn] = np.load(os.path.join(GOLDEN, str(fn)))
        out[str(name)] = files[fn]
    return out


def golden_matrix(g, name, kernel, n):
    """The reference's matrix of a stored (case, kernel), or None when the file holds no `data` for it."""
    pre = '%s_%s_' % (name, kernel)
    sp = pre if pre + 'indptr' in g.files else name + '_'
    indptr, indices = g[sp + 'indptr'], g[sp + 'indices']
    if kernel == 'uniform':
        data = np.ones(len(indices))
    elif len(indices) == 0:
        data = np.zeros(0)
    elif pre + 'data' in g.files:
        data = g[pre + 'data']
    else:
        return None
    return sparse.csr_matrix((data, indices, indptr), shape=(n, n))


def same_matrix(A, B):
    A, B = sparse.csr_matrix(A), sparse.csr_matrix(B)
    return (A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
            and A.data.tobytes() == B.data.tobytes())


GOLDEN_ENTRIES = {'rand2': 16812, 'rand3': 14028, 'blobs9': 25372, 'blobs20': 50890, 'grid_int': 18404, 'dups': 9918, 'dups0': 1800,
                  'feat': 26404, 'rand2_tiny': 0}


@pytest.mark.parametrize('name', sorted(GOLDEN_ENTRIES))
def test_restatement_equals_the_reference(name):
    """The rules (d2_tree membership, np.sum distances, the four kernels, zeros dropped) reproduce the reference bit for bit."""
    gold = load_golden()
    g = gold[name]
    X, eps, F, eps_f = ref.golden_inputs()[name]
    assert np.array_equal(g[name + '_X'], X) and float(g[name + '_eps']) == eps
    if F is not None:
        assert np.array_equal(g[name + '_F'], F) and float(g[name + '_eps_f']) == eps_f
    assert len(g[name + '_indices']) == GOLDEN_ENTRIES[name]
    assert not ref.near_boundary(X, eps)          # no pair within rounding of the radius: the tree's shortcut cannot matter
    prep = ref.prepare(X, eps, F)
    checked = 0
    for kernel in ref.KERNELS:
        want = golden_matrix(g, name, kernel, X.shape[0])
        if want is None:
            continue
        got = ref.epsilon_ball(X, eps, kernel=kernel, features=F, epsilon_f=eps_f, prep=prep)
        assert same_matrix(got, want), (name, kernel)
        checked += 1
    assert checked >= 2
    if name == 'dups':
        assert golden_matrix(g, name, 'distance', X.shape[0]).nnz == 8118


def test_restatement_user_kernel():
    g = load_golden()['eta']
    X, eps, _, _ = ref.golden_inputs()['grid_int']
    want = sparse.csr_matrix((g['eta_data'], g['eta_indices'], g['eta_indptr']), shape=(1600, 1600))
    assert want.nnz == 12324 and want.data.min() == 0.5
    assert same_matrix(ref.epsilon_ball(X, eps, eta=ref.eta_hat), want)


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('epsball') / 'libeb.so')
    subprocess.run(['g++', '-O2', '-ffp-contract=off', '-shared', '-fPIC', '-o', out, os.path.join(ROOT, 'tests', 'epsball_host.cpp')],
                   check=True)
    return ctypes.CDLL(out)


def _rows(fn, U, V):
    U, V = np.ascontiguousarray(U), np.ascontiguousarray(V)
    out = np.empty(U.shape[0])
    fn(U.ctypes.data_as(_vp), V.ctypes.data_as(_vp), ctypes.c_int64(U.shape[0]), ctypes.c_int(U.shape[1]), out.ctypes.data_as(_vp))
    return out


def test_numpy_order_sum_header_equals_numpy(lib):
    """csrc/npsum_exact.h == np.sum(V*V, axis=1) bit for bit for every row length 1 .. 300 (and a few beyond the second split)."""
    rng = np.random.default_rng(0)
    for d in list(range(1, 301)) + [511, 512, 513, 1000, 1025, 3000]:
        U, V = rng.normal(size=(64, d)), rng.normal(size=(64, d))
        if d % 3 == 0:
            U, V = U + 1e6, V + 1e6
        D = U - V
        assert _rows(lib.eb_npsum_rows, U, V).tobytes() == np.sum(D * D, axis=1).tobytes(), d


def test_tree_order_distance_header(lib):
    """csrc/sqdist_tree.h == the numpy emulation of cKDTree's accumulation order; equal to the numpy-order sum below 8
    coordinates, different from it somewhere from 8 on."""
    rng = np.random.default_rng(1)
    differs = 0
    for d in list(range(1, 70)) + [100, 128, 129, 130, 137, 200, 300]:
        U, V = rng.normal(size=(200, d)), rng.normal(size=(200, d))
        got = _rows(lib.eb_sqdist_rows, U, V)
        want = np.array([ref.d2_tree(U[i], V[i:i + 1])[0] for i in range(200)])
        assert got.tobytes() == want.tobytes(), d
        nps = _rows(lib.eb_npsum_rows, U, V)
        if d < 8:
            assert got.tobytes() == nps.tobytes(), d
        else:
            differs += int((got != nps).any())
    assert differs > 50
    # scipy's tree itself, on a pair list: the emulation is the tree's arithmetic
    from scipy.spatial import cKDTree
    X = rng.normal(size=(400, 20))
    dist, ind = cKDTree(X).query(X, k=5)
    want = np.array([[ref.d2_tree(X[i], X[j:j + 1])[0] for j in ind[i]] for i in range(400)])
    assert np.array_equal(dist, np.sqrt(want))


ONES = lambda d, v: [v] * d   # noqa: E731
# name, n, d, epsilon, lo, hi -> g, axis[3], nc[3], stride[3], ncells, coarsened, nqb
PLANS = [
    ('one cell', 100, 3, 2.0, [0, 0, 0], [1, 1, 1], [3, 2, 1, 0, 1, 1, 1, 1, 1, 1, 1, 0, 2]),
    ('two cells on one axis', 100, 1, 0.6, [0], [1], [1, 0, 0, 0, 2, 1, 1, 1, 0, 0, 2, 0, 2]),
    ('rand2 golden', 1500, 2, 0.05, [0, 0], [1, 1], [2, 1, 0, 0, 20, 20, 1, 20, 1, 0, 400, 0, 24]),
    ('1e6 cells', 1000000, 3, 0.01, [0, 0, 0], [1, 1, 1], [3, 2, 1, 0, 100, 100, 100, 10000, 100, 1, 1000000, 0, 15625]),
    ('the cap', 1000000, 3, 0.0001, [0, 0, 0], [1, 1, 1], [3, 2, 1, 0, 126, 126, 126, 15876, 126, 1, 2000376, 1, 15625]),
    ('cap by n', 900, 2, 1e-05, [0, 0], [1, 1], [2, 1, 0, 0, 59, 59, 1, 59, 1, 0, 3481, 1, 15]),
    ('zero-extent axis', 1000, 3, 0.1, [0, 5, 0], [1, 5, 2], [3, 1, 0, 2, 1, 10, 20, 200, 20, 1, 200, 0, 16]),
    ('epsilon 0', 900, 2, 0.0, [0, 0], [1, 1], [2, 1, 0, 0, 59, 59, 1, 59, 1, 0, 3481, 1, 15]),
    ('epsilon 0, one point repeated', 3000, 2, 0.0, [0.5, 0.5], [0.5, 0.5], [2, 1, 0, 0, 1, 1, 1, 1, 1, 0, 1, 0, 47]),
    ('high d', 5000, 130, 3.0, ONES(130, -1), ONES(129, 1) + [4], [3, 1, 0, 129, 1, 1, 2, 2, 2, 1, 2, 0, 79]),
    ('scale input', 1000000, 3, 0.0174, [0, 0, 0], [1, 1, 1], [3, 2, 1, 0, 58, 58, 58, 3364, 58, 1, 195112, 0, 15625]),
    ('pixels', 262144, 2, 5.0, [0, 0], [511, 511], [2, 1, 0, 0, 103, 103, 1, 103, 1, 0, 10609, 0, 4096]),
    ('long axis', 50000, 2, 1e-09, [0, 0], [1, 3], [2, 0, 1, 0, 439, 439, 1, 439, 1, 0, 192721, 1, 782]),
    ('infinite epsilon', 10, 2, float('inf'), [0, 0], [1, 1], [2, 1, 0, 0, 1, 1, 1, 1, 1, 0, 1, 0, 1]),
]


@pytest.mark.parametrize('case', PLANS, ids=[p[0] for p in PLANS])
def test_plan_table(lib, case):
    """csrc/ball_plan.h on a recorded table of shapes, and the properties the search's correctness rests on: a cell is never
    narrower than epsilon (1 + 1e-6) nor than 1e-150, an axis never has more than 2^20 cells, the grid never more than 2^21, every
    coordinate of the box lands in a cell of its axis, and the cell coordinate is monotone."""
    name, n, d, eps, lo, hi, want = case
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    io, do = np.zeros(13, np.int64), np.zeros(6)
    lib.eb_plan(ctypes.c_int64(n), ctypes.c_int(d), ctypes.c_double(eps), lo.ctypes.data_as(_vp), hi.ctypes.data_as(_vp),
                io.ctypes.data_as(_vp), do.ctypes.data_as(_vp))
    assert io.tolist() == want
    g, axis, nc, stride, ncells = int(io[0]), io[1:4], io[4:7], io[7:10], int(io[10])
    assert g == min(d, 3) and ncells == int(np.prod(nc[:g])) <= (1 << 21) and ncells <= max(1024, 4 * n)
    assert len(set(axis[:g].tolist())) == g
    for a in range(g):
        h = do[3 + a]
        assert h >= eps * (1 + 1e-6) and h >= 1e-150 and 1 <= nc[a] <= (1 << 20)
        assert do[a] == lo[axis[a]]
        assert stride[a] == int(np.prod(nc[a + 1:g]))
        x = np.sort(np.concatenate([np.linspace(lo[axis[a]], hi[axis[a]], 1001), [lo[axis[a]], hi[axis[a]]]]))
        c = np.zeros(len(x), np.int64)
        lib.eb_cell_coords(ctypes.c_int64(n), ctypes.c_int(d), ctypes.c_double(eps), lo.ctypes.data_as(_vp), hi.ctypes.data_as(_vp),
                           ctypes.c_int(a), x.ctypes.data_as(_vp), ctypes.c_int64(len(x)), c.ctypes.data_as(_vp))
        assert c.min() == 0 and c.max() <= nc[a] - 1 and (np.diff(c) >= 0).all()
        # points two or more cells apart are farther apart than epsilon
        far = np.abs(c[:, None] - c[None, :]) >= 2
        if far.any() and np.isfinite(eps):
            assert (np.abs(x[:, None] - x[None, :])[far] > eps).all()


def test_refusals_come_before_the_library(monkeypatch):
    """Bad kernel -> SystemExit with the reference's message; negative / NaN epsilon and non-finite data -> ValueError; none of
    them loads the library."""
    import graphlearning_amd as gl
    from graphlearning_amd import _hip

    def boom(*a, **k):
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_hip, 'load', boom)
    X = np.random.default_rng(0).random((20, 2))
    with pytest.raises(SystemExit) as e:
        gl.weightmatrix.epsilon_ball(X, 0.3, kernel='symgaussian')
    assert str(e.value) == 'Invalid choice of kernel: symgaussian'
    for eps in (-1.0, float('nan'), -0.001):
        with pytest.raises(ValueError):
            gl.weightmatrix.epsilon_ball(X, eps)
    for bad in (np.nan, np.inf, -np.inf):
        Y = X.copy()
        Y[7, 1] = bad
        with pytest.raises(ValueError):
            gl.weightmatrix.epsilon_ball(Y, 0.3)
        with pytest.raises(ValueError):
            gl.weightmatrix.epsilon_ball(X, 0.3, features=Y)
    with pytest.raises(ValueError):
        gl.weightmatrix.epsilon_ball(X, 0.3, features=X[:10])
