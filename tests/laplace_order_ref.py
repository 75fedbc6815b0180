"""Cases and fixture access for Laplace learning of order 2 and 3, vector tau and randomwalk's alpha (tests/golden/g24_laplace_order.npz,
written by tests/golden/make_golden_laplace_order.py from the reference).  Shared by the maker, tests/test_oracle_golden.py,
tests/test_laplace_order_host.py and tests/test_gpu_laplace_order.py, so that all of them speak of the same cases.

Graphs: kNN with K = 10 neighbours on 3 Gaussian blobs in 5 dimensions, n = 600 and n = 2000, 5 labels per class.  The point sets are
float32 values (stored as such, used as float64)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_FILE = 'g24_laplace_order.npz'
K = 10
CLASSES = 3
DIM = 5
PER_CLASS = 5
TOL = 1e-5
SIZES = (600, 2000)
ORDERS = (2, 3)
NORMS = ('combinatorial', 'normalized')
TAUS = ('0', '0.01', 'vec')                  # 'vec': the recorded random vector in [0, 0.02]
ALPHAS = (0.5, 0.99)
TRIALS = 5

# every recorded Laplace fit: (n, order, normalization, tau tag, mean_shift).  n = 600: the full grid; n = 2000: order 2 only, and
# order 1 with a vector tau at n = 600 (the fast right-hand-side route)
CASES = [(600, o, nm, t, ms) for o in ORDERS for nm in NORMS for t in TAUS for ms in (False, True)]
CASES += [(2000, 2, 'combinatorial', '0', False)]
CASES += [(600, 1, 'combinatorial', 'vec', False), (600, 1, 'normalized', 'vec', True)]


def case_key(n, order, norm, tau, mean_shift):
    return 'n%d_order%d_%s_tau%s_ms%d' % (n, order, norm, tau, int(mean_shift))


def load_golden():
    return dict(np.load(os.path.join(HERE, 'golden', GOLDEN_FILE), allow_pickle=False))


def points(g, n):
    return np.ascontiguousarray(g['X%d' % n], dtype=np.float64)


def knn_lists(g, n):
    return np.ascontiguousarray(g['J%d' % n], dtype=np.int64), np.ascontiguousarray(g['D%d' % n], dtype=np.float64)


def training_set(g, n, trial=0):
    ind = np.ascontiguousarray(g['train%d' % n][trial], dtype=np.int64)
    return ind, g['labels%d' % n][ind]


def tau_value(g, n, tau):
    return {'0': 0, '0.01': 0.01}[tau] if tau != 'vec' else g['tau%d' % n]


def longest_row(A):
    return int(np.diff(A.indptr).max())


def rows_with_three(L, train_ind):
    """How many rows of -L[:, train_ind] hold three or more entries: the rows of the right-hand side whose sum has an order."""
    return int((np.diff((-L[:, train_ind]).tocsr().indptr) >= 3).sum())
