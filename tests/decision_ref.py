"""ssl.predict / ssl.volume_label_projection restated from their rules, numpy only (tests/test_decision_host.py checks the
restatement bit for bit against oracle/gl_oracle.py and the golden vectors of the reference, tests/test_gpu_decision.py checks
the device against it):

  scores       (prob - min(prob)) / max(prob - min(prob)), minimum and maximum over the WHOLE array; a float32 prob stays float32
               through both operations (numpy's type rules), only the product with the fp64 class weights is wider.  A NaN anywhere
               or a constant array makes every score NaN; a +inf entry makes its own score NaN and every other one 0;
  labels       argmax (similarity) or argmin (distances) over the classes of scores * weights; the first index wins a tie, the
               first NaN wins over everything (np.argmax / np.argmin);
  projection   from weights w (ones when the integer 1 is given), at most max_steps times and while err > 1e-3 (err = 1 before the
               first step):  sizes = mean of onehot(labels) per class;  grad = sizes - priors;  err = max|grad| (NaN propagates);
               w = w + dt * grad with dt = -0.1 (similarity) or +0.1 (distances);  w = w / w[0].
               Then the labels with the final weights.  Returns (labels, weights, err, steps).

The normalisation does not depend on the weights, so it is done once and not once per step as the reference's loop does: the same
operations on the same numbers."""
import numpy as np


def scores_of(prob):
    prob = np.asarray(prob)
    scores = prob - np.min(prob)
    return scores / np.max(scores)


def _weights(weights, k):
    if type(weights) == int:
        return np.ones((k,))
    return np.array(weights, dtype=float)


def _decide(scores, weights, similarity):
    if similarity:
        return np.argmax(scores * weights, axis=1)
    return np.argmin(scores * weights, axis=1)


def onehot(labels, k):
    out = np.zeros((labels.shape[0], k))
    out[np.arange(labels.shape[0]), labels] = 1
    return out


def predict(prob, weights=1, similarity=True):
    return _decide(scores_of(prob), weights, similarity)


def volume_label_projection(prob, priors, weights=1, similarity=True, max_steps=10000):
    prob = np.asarray(prob)
    k = prob.shape[1]
    weights = _weights(weights, k)
    scores = scores_of(prob)
    dt = 0.1
    if similarity:
        dt *= -1
    it = 0
    err = 1
    while it < max_steps and err > 1e-3:
        it += 1
        sizes = np.mean(onehot(_decide(scores, weights, similarity), k), axis=0)
        grad = sizes - priors
        err = np.max(np.absolute(grad))
        weights += dt * grad
        weights = weights / weights[0]
    return _decide(scores, weights, similarity), weights, err, it
