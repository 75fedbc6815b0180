"""Active learning: the `active_learner` loop and the acquisition functions of the reference's graphlearning.active_learning
(unc_sampling, var_opt, sigma_opt, model_change, model_change_var_opt), with the covariance of the truncated forms on the GPU.

    model = gl.ssl.laplace(W)
    evals, evecs = model.graph.eigen_decomp(normalization='normalized', k=50)
    AL = gl.active_learning.active_learner(model, gl.active_learning.var_opt, train_ind, y[train_ind],
                                           C=np.diag(1. / (evals + 1e-11)), V=evecs)
    for it in range(10):
        q = AL.select_queries()
        AL.update(q, y[q])

With V given (storage 'trunc') the state is the (n, M) matrix of eigenvectors and the M x M covariance C; both stay on the device
(_hip.Acq, csrc/acq.hip), a round is one pass over V and one rank-one launch, and `select_greedy` runs a whole design of the two
criteria that do not look at labels in one device call.  The contract of the arithmetic is DESIGN.md 4.19.  With V=None (storage
'full', a dense n x n C: small graphs) everything is host numpy, as is unc_sampling (O(n classes)).  The choice among the downloaded
values happens on the host by the reference's expressions, so equal values give equal choices, and 'prop' / 'rand' draw from numpy's
global stream with the same calls in the same order.

Deviations from the reference, all where it raises or reads what it does not mean: candidate_ind='full' with allow_repeat=True uses
all vertices (the reference hands an array to np.arange); a candidate index >= n is refused (the reference tests > n); model_change
and model_change_var_opt with full storage index the candidate columns (the reference broadcasts n against the candidate count);
non-finite C, V, gamma2 or u, M > 256 and arrays of the wrong shape are a ValueError before any device call; matplotlib is not
imported.  There is no CPU fallback of the truncated forms: without the library or a GPU they raise GlxError."""
import numpy as np
from scipy.special import softmax

from . import _hip

MAX_M = _hip.ACQ_MAX_M


class acquisition_function:
    """Base class: `compute(u, candidate_ind)` returns one value per candidate, larger = more worth a label; `update(query_ind,
    query_labels)` takes note of the vertices that were labelled."""

    def compute(self, u, candidate_ind):
        raise NotImplementedError("Must override compute")

    def update(self, query_ind, query_labels):
        return


class unc_sampling(acquisition_function):
    """Uncertainty sampling (Settles 2012) from the score matrix u (n, classes), on the host.  unc_method: 'norm', 'entropy',
    'least_confidence', 'smallest_margin', 'largest_margin', 'unc_2norm'."""
    METHODS = ('norm', 'entropy', 'least_confidence', 'smallest_margin', 'largest_margin', 'unc_2norm')

    def __init__(self, unc_method='smallest_margin'):
        self.unc_method = unc_method

    def compute(self, u, candidate_ind):
        uc = u[candidate_ind]
        method = self.unc_method
        if method == 'norm':
            probs = softmax(uc, axis=1)
            predicted = np.eye(u.shape[1])[np.argmax(uc, axis=1)]
            return np.linalg.norm((probs - predicted), axis=1)
        if method == 'entropy':
            probs = softmax(uc, axis=1)
            return np.max(probs, axis=1) - np.sum(probs * np.log(probs + .00001), axis=1)
        if method == 'least_confidence':
            return np.ones((uc.shape[0],)) - np.max(uc, axis=1)
        if method == 'smallest_margin':
            srt = np.sort(uc)
            return 1. - (srt[:, -1] - srt[:, -2])
        if method == 'largest_margin':
            srt = np.sort(uc)
            return 1. - (srt[:, -1] - srt[:, 0])
        if method == 'unc_2norm':
            return 1. - np.linalg.norm(uc, axis=1)
        raise ValueError("unc_method %r is none of %s" % (method, ', '.join(self.METHODS)))


def _int32_positions(ind, n, what):
    ind = np.asarray(ind)
    if ind.size and (ind.min() < 0 or ind.max() >= n):
        raise ValueError("%s must have integer values in [0, %d)" % (what, n))
    return np.ascontiguousarray(ind, dtype=np.int32).ravel()


class _covariance_acquisition(acquisition_function):
    """What var_opt, sigma_opt, model_change and model_change_var_opt share: the covariance C, with V its truncated form on the device.
    `.C` is the current matrix (downloaded from the device in the truncated form)."""
    kind = None
    uses_unc = False

    def __init__(self, C, V=None, gamma2=0.1 ** 2., unc_method='smallest_margin', device=None):
        C = np.array(C, dtype=np.float64)
        gamma2 = float(gamma2)
        if C.ndim != 2 or C.shape[0] != C.shape[1]:
            raise ValueError("C of shape %s is not square" % (C.shape,))
        if V is not None:
            V = np.ascontiguousarray(V, dtype=np.float64)
            if V.ndim != 2 or V.shape[0] < 1 or V.shape[1] != C.shape[0]:
                raise ValueError("V of shape %s does not go with C of shape %s: expected (n, M) and (M, M)" % (V.shape, C.shape))
            if V.shape[1] > MAX_M:
                raise ValueError("M = %d columns of V, at most %d (the cap of eigen_decomp's k)" % (V.shape[1], MAX_M))
            if not np.isfinite(V).all():
                raise ValueError("V holds NaN or infinite entries")
        if C.shape[0] < 1 or not np.isfinite(C).all() or not np.isfinite(gamma2):
            raise ValueError("C holds NaN or infinite entries (or is empty), or gamma2 = %r is not finite" % gamma2)
        self._C = C
        self.V = V
        self.gamma2 = gamma2
        self.device = device
        self.storage = 'full' if V is None else 'trunc'
        self.unc_sampling = unc_sampling(unc_method=unc_method) if self.uses_unc else None
        self._acq = None

    # ---- the device handle of the truncated form: created on first use -----------------------------------------------------------
    def _handle(self):
        if self._acq is None:
            self._acq = _hip.Acq(self.V, self._C, self.gamma2, device=self.device)
        return self._acq

    @property
    def C(self):
        if self._acq is not None:
            return self._acq.get_c()
        return self._C

    @C.setter
    def C(self, value):
        value = np.array(value, dtype=np.float64)
        if value.shape != self._C.shape or not np.isfinite(value).all():
            raise ValueError("C must keep its shape %s and be finite" % (self._C.shape,))
        self.close()
        self._C = value

    def close(self):
        """release the device memory; the covariance comes back to the host and a later call uploads it again"""
        if self._acq is not None:
            self._C = self._acq.get_c()
            self._acq.close()
            self._acq = None

    def _rows(self):
        return self._C.shape[0] if self.storage == 'full' else self.V.shape[0]

    def _numerator(self, cols):
        """full storage: the numerator from the candidate columns of C"""
        if self.kind == _hip.ACQ_SIGMA:
            return np.sum(cols, axis=0) ** 2.
        if self.kind == _hip.ACQ_MC:
            return np.linalg.norm(cols, axis=0)
        return np.linalg.norm(cols, axis=0) ** 2.

    def compute(self, u, candidate_ind):
        cand = _int32_positions(candidate_ind, self._rows(), 'candidate_ind')
        unc = None
        if self.uses_unc:
            unc = np.asarray(self.unc_sampling.compute(u, candidate_ind), dtype=np.float64)
            if not np.isfinite(unc).all():
                raise ValueError("u gives uncertainty terms that are NaN or infinite")
        if self.storage == 'full':
            num, den = self._numerator(self._C[:, cand]), self.gamma2 + self._C.diagonal()[cand]
            return unc * num / den if self.uses_unc else num / den          # (left to right, like the reference)
        return self._handle().compute(self.kind, cand, unc)

    def update(self, query_ind, query_labels):
        query = _int32_positions(np.atleast_1d(query_ind), self._rows(), 'query_ind')
        if self.storage == 'full':
            for k in query:
                self._C -= np.outer(self._C[:, k], self._C[:, k]) / (self.gamma2 + self._C[k, k])
            return
        self._handle().update(query)

    def greedy(self, candidate_ind, batch_size):
        """the indices and values `batch_size` rounds of evaluate / first maximum / update choose among candidate_ind, on a copy of C"""
        if self.uses_unc:
            raise TypeError("%s looks at labels: no greedy design" % type(self).__name__)
        cand = _int32_positions(candidate_ind, self._rows(), 'candidate_ind')
        batch_size = int(batch_size)
        if batch_size < 0 or batch_size > len(np.unique(cand)):
            raise ValueError("batch_size = %d for %d distinct candidates" % (batch_size, len(np.unique(cand))))
        if self.storage == 'trunc':
            pos, vals = self._handle().greedy(self.kind, cand, batch_size)
            return np.asarray(candidate_ind)[pos], vals
        C, left, out, got = self._C.copy(), np.ones(len(cand), dtype=bool), [], []
        for _ in range(batch_size):
            vals = self._numerator(C[:, cand]) / (self.gamma2 + C.diagonal()[cand])
            vals = np.where(left, vals, -np.inf)
            p = int(np.argmax(vals))
            if not np.isfinite(vals[p]):
                raise ValueError("a round of the greedy design has no finite maximum")
            k = cand[p]
            out.append(p)
            got.append(vals[p])
            left &= cand != k
            C -= np.outer(C[:, k], C[:, k]) / (self.gamma2 + C[k, k])
        return np.asarray(candidate_ind)[np.array(out, dtype=np.int64)], np.array(got)

    def __del__(self):
        try:
            if self._acq is not None:
                self._acq.close()
        except Exception:
            pass


class var_opt(_covariance_acquisition):
    """Variance optimisation (Ji and Han 2012): ||C v_i||^2 / (gamma2 + v_i^T C v_i)."""
    kind = _hip.ACQ_VAR

    def __init__(self, C, V=None, gamma2=0.1 ** 2., device=None):
        super().__init__(C, V, gamma2, device=device)


class sigma_opt(_covariance_acquisition):
    """Sigma optimality (Ma, Garnett and Schneider 2013): (1^T C v_i)^2 / (gamma2 + v_i^T C v_i)."""
    kind = _hip.ACQ_SIGMA

    def __init__(self, C, V=None, gamma2=0.1 ** 2., device=None):
        super().__init__(C, V, gamma2, device=device)


class model_change(_covariance_acquisition):
    """Model change (Miller and Bertozzi 2021): unc ||C v_i|| / (gamma2 + v_i^T C v_i), unc from unc_sampling(unc_method)."""
    kind = _hip.ACQ_MC
    uses_unc = True


class model_change_var_opt(_covariance_acquisition):
    """Model change times variance optimisation: unc ||C v_i||^2 / (gamma2 + v_i^T C v_i)."""
    kind = _hip.ACQ_MCVAR
    uses_unc = True


class active_learner:
    """The loop around a graph-based learner `model` (anything with fit(ind, labels) and graph.num_nodes) and an acquisition function
    class `acq_function` built from **kwargs: select_queries picks vertices to label, update takes their labels, refits and lets the
    acquisition function know.  Attributes as in the reference: labeled_ind, labels, u, unlabeled_ind, acq_function, policy."""

    def __init__(self, model, acq_function, labeled_ind, labels, policy='max', **kwargs):
        self.model = model
        self.labeled_ind = labeled_ind.copy()
        self.labels = labels.copy()
        self.acq_function = acq_function(**kwargs)
        self.acq_function.update(labeled_ind, labels)
        self.policy = policy
        self.u = self.model.fit(self.labeled_ind, self.labels)
        self.n = self.model.graph.num_nodes
        self.all_inds = np.arange(self.n)
        self.unlabeled_ind = np.setdiff1d(self.all_inds, self.labeled_ind)
        self.printed_warning = False

    def _candidates(self, candidate_ind, rand_frac=0.1, allow_repeat=False):
        if isinstance(candidate_ind, np.ndarray):
            if (candidate_ind.min() < 0) or (candidate_ind.max() >= self.n):
                raise ValueError(f"candidate_ind must have integer values between 0 and {self.n - 1}")
            return candidate_ind
        if candidate_ind == 'full':
            if allow_repeat:
                return self.all_inds
            return np.setdiff1d(self.all_inds, self.labeled_ind)
        if (candidate_ind == 'rand') and (rand_frac > 0 and rand_frac < 1):
            if allow_repeat:
                return np.random.choice(self.all_inds, size=int(rand_frac * self.n), replace=False)
            return np.random.choice(self.unlabeled_ind, size=int(rand_frac * len(self.unlabeled_ind)), replace=False)
        raise ValueError("Invalid input for candidate_ind")

    def select_queries(self, batch_size=1, policy=None, candidate_ind='full', rand_frac=0.1, return_acq_vals=False, prop_gamma=1.0,
                       allow_repeat=False):
        if policy is None:
            policy = self.policy
        candidate_ind = self._candidates(candidate_ind, rand_frac, allow_repeat)
        acq_vals = self.acq_function.compute(self.u, candidate_ind)
        if callable(policy):
            query_ind = policy(candidate_ind, acq_vals, batch_size)
        elif policy == 'max':
            query_ind = candidate_ind[(-acq_vals).argsort()[:batch_size]]
        elif policy == 'prop':
            probs = np.exp(prop_gamma * (acq_vals - acq_vals.max()))
            probs /= probs.sum()
            query_ind = np.random.choice(candidate_ind, batch_size, p=probs)
        else:
            raise ValueError("policy %r is neither 'max', 'prop' nor a callable" % (policy,))
        if return_acq_vals:
            return query_ind, acq_vals
        return query_ind

    def select_greedy(self, batch_size, candidate_ind='full'):
        """The indices that `batch_size` rounds of select_queries(1) + update would choose under var_opt or sigma_opt, which do not look
        at labels -- in one device call (truncated storage), with every chosen vertex struck from the candidates.  Changes neither the
        learner nor C: hand the result to update(query_ind, labels) once the labels are known.  TypeError for any other acquisition
        function."""
        if not isinstance(self.acq_function, (var_opt, sigma_opt)):
            raise TypeError("select_greedy needs var_opt or sigma_opt, not %s: the other criteria depend on the labels between the rounds"
                            % type(self.acq_function).__name__)
        candidate_ind = self._candidates(candidate_ind)
        return self.acq_function.greedy(candidate_ind, batch_size)[0]

    def update(self, query_ind, query_labels):
        if np.intersect1d(query_ind, self.labeled_ind).size > 0 and not self.printed_warning:
            print("WARNING: Having multiple observations at a single node detected")
            self.printed_warning = True
        self.labeled_ind = np.append(self.labeled_ind, query_ind)
        self.labels = np.append(self.labels, query_labels)
        self.u = self.model.fit(self.labeled_ind, self.labels)
        self.unlabeled_ind = np.setdiff1d(self.all_inds, self.labeled_ind)
        self.acq_function.update(query_ind, query_labels)
        return
