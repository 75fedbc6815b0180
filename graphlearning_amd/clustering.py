"""Graph-based clustering with the interface of the reference's graphlearning.clustering: the base class `clustering`, the INCRES
learner `incres` whose grow loop runs on the device, and the host metrics clustering_accuracy, purity, withinss and RP1D.

    model = gl.clustering.incres(W, num_clusters=3)
    labels = model.fit_predict()

`spectral` and `fokker_planck` are not provided: see the README.
"""
import sys
import numpy as np
from scipy import sparse
from scipy.optimize import linear_sum_assignment

from . import _hip
from .graph import graph as _graph

MAX_CLUSTERS = 256      # the column cap of the device's state records


class clustering:
    """Base class: fit() runs the learner's _fit(), predict() returns what it found (reference clustering.py:19-110)."""

    def __init__(self, W, num_clusters):
        self.graph = W if type(W) == _graph else _graph(W)
        self.cluster_labels = None
        self.num_clusters = num_clusters
        self.fitted = False

    def predict(self):
        if not self.fitted:
            sys.exit('Model has not been fitted yet.')
        return self.cluster_labels

    def fit(self, all_labels=None):
        labels = self._fit(all_labels=all_labels)
        self.fitted = True
        self.cluster_labels = labels
        return labels

    def fit_predict(self, all_labels=None):
        self.fit(all_labels=all_labels)
        return self.predict()

    def _fit(self, all_labels=None):
        raise NotImplementedError('Must override _fit')


class incres(clustering):
    """INCRES clustering (X. Bresson, H. Hu, T. Laurent, A. Szlam, J. von Brecht: An incremental reseeding strategy for clustering,
    2016; reference clustering.py:282-371).  T outer iterations, each: plant m random seeds per cluster, grow them with the random
    walk F <- P F, P = W D^-1, until no entry of F is zero, harvest the row-wise argmax; m grows by max(int(speed * 1e-4 * n / k), 1).

    Every random number is drawn from numpy's global stream by the reference's calls in the reference's order, the products are the
    reference's sums term by term, so after np.random.seed(s) the labels equal the reference's on every vertex after every outer
    iteration.  One device call per outer iteration: the (k, m) seed indices go up, the labels and the sweep count
    come down.

    Unlike the reference, whose grow loop never ends on such graphs, a grow loop of more than max_grow sweeps (default 2 n + 2)
    raises GlxError: the graph is disconnected, or bipartite, or so long that values underflow to zero before they arrive.

    After fit(): grow_sweeps (the sweeps of every outer iteration) and incres_plan (what the chunked schedule cost).
    ValueError, before anything is drawn or sent to the device: a vertex of degree 0, a weight that is negative or not finite,
    num_clusters outside 1 .. 256, T < 1, max_grow < 1."""

    def __init__(self, W, num_clusters, speed=5, T=200, max_grow=None, device=None):
        super().__init__(W, num_clusters)
        self.speed = speed
        self.T = T
        self.max_grow = max_grow
        self.device = device
        self.grow_sweeps = None
        self.incres_plan = None
        self._checked()

    def _checked(self):
        """(n, k, T, max_grow) as ints, or ValueError"""
        W = self.graph.weight_matrix
        n = self.graph.num_nodes
        k, T = self.num_clusters, self.T
        if not (isinstance(k, (int, np.integer)) and 1 <= k <= MAX_CLUSTERS):
            raise ValueError('incres: num_clusters=%r, supported are 1 .. %d clusters' % (k, MAX_CLUSTERS))
        if not (isinstance(T, (int, np.integer)) and T >= 1):
            raise ValueError('incres: T=%r, at least one outer iteration is needed' % (T,))
        max_grow = 2 * n + 2 if self.max_grow is None else self.max_grow
        if not (isinstance(max_grow, (int, np.integer)) and max_grow >= 1):
            raise ValueError('incres: max_grow=%r, at least one sweep is needed' % (self.max_grow,))
        if W.shape[0] != W.shape[1] or n < 1:
            raise ValueError('incres: the weight matrix must be square and not empty')
        data = np.asarray(W.data, dtype=np.float64)
        if not np.all(np.isfinite(data)) or np.any(data < 0):
            raise ValueError('incres: a weight is negative or not finite')
        degree = self.graph.degree_vector()
        if not np.all(degree > 0):
            raise ValueError('incres: vertex %d has degree 0 (its column of P = W D^-1 does not exist)' % int(np.flatnonzero(~(degree > 0))[0]))
        return n, int(k), int(T), int(max_grow)

    def _transition(self):
        """P = W D^-1 by the reference's own expression: scipy's sparse product leaves every row in REVERSE order of discovery, and
        that stored order is the order of every sum of the grow loop.  Nothing here may sort the indices."""
        D = self.graph.degree_matrix(p=-1)
        return self.graph.weight_matrix * D

    def _fit(self, all_labels=None):
        n, k, T, max_grow = self._checked()
        step = max(int(self.speed * 1e-4 * n / k), 1)
        u = np.random.randint(0, k, size=n)
        P = sparse.csr_matrix(self._transition())
        self.grow_sweeps = []
        m = 1
        with _hip.Incres(P.indptr, P.indices, P.data, k, device=self.device) as dev:
            labels = _hip.pinned_empty((n,), np.int32)      # page-locked from a size on: the labels come down at full speed
            labels[:] = u
            for it in range(T):
                # the members of every cluster in ascending vertex order (J[u == r]) from one counting sort; the draws cluster by cluster
                counts, order = _hip.host_group_by_label(labels, k)
                ends = np.cumsum(counts)
                seeds = np.empty((k, m), dtype=np.int32)
                for r in range(k):
                    members = order[ends[r] - counts[r]:ends[r]]
                    seeds[r] = members[np.random.choice(len(members), m)]      # (an empty cluster: numpy's own ValueError)
                try:
                    labels, sweeps = dev.step(seeds, max_grow, out=labels)
                finally:
                    self.incres_plan = dict(dev.stats(), max_grow=max_grow, seed_step=step)
                self.grow_sweeps.append(sweeps)
                m += step
                if all_labels is not None:
                    print('Iteration %d: Accuracy = %.2f%%, #seeds= %d' % (it, clustering_accuracy(labels, all_labels), m))
            u = labels.astype(np.int64)
        return u


def clustering_accuracy(pred_labels, true_labels):
    """Accuracy in [0, 100] under the best matching of cluster labels to classes (a linear sum assignment on the numbers of
    mismatches).  The classes are the distinct values of true_labels in ascending order; predicted labels are 0 .. k-1."""
    pred_labels = np.asarray(pred_labels)
    classes, truth = np.unique(np.asarray(true_labels), return_inverse=True)
    c = len(classes)
    cost = np.zeros((c, c), dtype=float)
    for i in range(c):
        mine = truth.ravel()[pred_labels == i]
        cost[i] = len(mine) - np.bincount(mine, minlength=c)       # predicted i, true class not j
    rows, cols = linear_sum_assignment(cost)
    return 100 * (1 - cost[rows, cols].sum() / len(pred_labels))


def purity(cluster_labels, true_labels):
    """(purity in [0, 100], per-cluster purities): the share of vertices that belong to the largest class of their cluster."""
    cluster_labels, true_labels = np.asarray(cluster_labels), np.asarray(true_labels)
    largest, size = [], []
    for c in np.unique(cluster_labels):
        inside = true_labels[cluster_labels == c]
        largest.append(np.max(np.bincount(inside)))
        size.append(len(inside))
    largest, size = np.array(largest), np.array(size)
    return 100 * np.sum(largest) / np.sum(size), largest / size


def withinss(x):
    """(w, m): the exact optimum of 2-means on the 1D data x -- the WithinSS value w and the threshold m that splits x."""
    x = np.sort(x)
    n = x.shape[0]
    sigma = np.std(x)
    score = np.zeros(n - 1)
    left, right = np.mean(x[:1]), np.mean(x[1:])        # means of the i + 1 smallest and of the others, updated as i grows
    for i in range(n - 1):
        score[i] = (i + 1) * left ** 2 + (n - i - 1) * right ** 2
        if i < n - 2:
            left = ((i + 1) * left + x[i + 1]) / (i + 2)
            right = ((n - i - 1) * right - x[i + 1]) / (n - i - 2)
    best = np.argmax(score)
    return (np.sum(x ** 2) - score[best]) / (n * sigma ** 2), x[best]


def RP1D(X, T=100):
    """Binary clustering by random projections to one dimension (S. Han, M. Boutin: The hidden structure of image datasets, 2015):
    of T random directions (np.random.rand(T, d)) the one with the smallest WithinSS splits the data at its threshold.  Returns a
    0 / 1 float array."""
    n, d = X.shape[0], X.shape[1]
    directions = np.random.rand(T, d)
    lowest, chosen = np.inf, 0
    for i in range(T):
        w, _ = withinss(np.sum(directions[i, :] * X, axis=1))
        if w < lowest:
            lowest, chosen = w, i
    x = np.sum(directions[chosen, :] * X, axis=1)
    _, threshold = withinss(x)
    out = np.zeros(n)
    out[x > threshold] = 1
    return out
