"""The inputs of tests/test_gpu_decision.py, built on the host so that tests/test_decision_host.py can pin what each of them is
there for -- how its run of the restatement (tests/decision_ref.py) ends -- without a GPU.

A case is (prob, priors, weights, similarity, max_steps) and how the projection must end on it:
  'cap'    the step cap stops it: steps == max_steps with err still above 1e-3;
  'conv'   it stops by itself, after at least `min_steps` and fewer than max_steps steps;
  an int   it stops by itself after exactly that many steps.
Every reference run is capped so that it costs a couple of seconds of numpy at the most, and is computed once per process."""
import functools

import numpy as np

import decision_ref as ref

DTYPES = {'f64': np.float64, 'f32': np.float32}
LOOKS = (2, 6, 14, 30, 62, 94)              # the step counts after which the host looks at the device's `done` flag (2, 4, 8, 16, 32, 32 ...)
CAPS = (1, 2, 3, 6, 7, 14, 15, 30, 31, 62, 63, 94, 95, 10000)


def draw(n, C, seed, shift=0.5):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, C)) + shift * rng.normal(size=C)


def priors_for(C, seed):
    p = 1 + 0.3 * np.random.default_rng(1000 + seed).random(C)
    return p / np.sum(p)


def _plain(n, C, seed, max_steps=10000, similarity=True, weights=1):
    return dict(prob=draw(n, C, seed), priors=priors_for(C, seed), weights=weights, similarity=similarity, max_steps=max_steps)


def _one_step(dtype):
    """Priors equal to the class sizes of the plain argmax: the first step finds err = 0."""
    c = _plain(3000, 5, 31)
    lab = ref.predict(c['prob'].astype(dtype))
    c['priors'] = np.bincount(lab, minlength=5) / 3000
    return c


def _two_steps(dtype):
    """Two classes, column 0 constant: 600 rows are class 1 under any weights near 1, 400 rows become class 1 once
    w[1] / w[0] > 1 / 0.97, which the first step (w = (0.98, 1.02), then divided by 0.98) achieves; the second step finds the
    class sizes equal to the priors."""
    n = 2000
    prob = np.zeros((n, 2))
    prob[:, 0] = 1.0
    prob[:600, 1] = 1.5
    prob[600:1000, 1] = 0.97
    prob = prob[np.random.default_rng(32).permutation(n)]
    return dict(prob=prob, priors=np.array([0.5, 0.5]), weights=1, similarity=True, max_steps=10000)


def _ties(similarity):
    prob = np.random.default_rng(50).integers(0, 3, size=(2000, 4)).astype(np.float64)
    return dict(prob=prob, priors=np.array([0.3, 0.2, 0.25, 0.25]), weights=1, similarity=similarity, max_steps=200)


def _degenerate(kind):
    c = _plain(500, 4, 60, max_steps=50)
    if kind == 'constant':
        c['prob'] = np.full((500, 4), 0.7)
    elif kind == 'nan':
        c['prob'][123, 2] = np.nan
    elif kind == 'inf':
        c['prob'][321, 1] = np.inf
    elif kind == 'priors_sum':
        c['priors'] = c['priors'] * 1.3
    elif kind == 'prior_zero':
        c['priors'] = np.array([0.5, 0.0, 0.3, 0.2])
    elif kind == 'w_negative':
        c['weights'] = np.array([1.0, -0.5, 2.0, 1.0])
    elif kind == 'w0_zero':
        c['weights'] = np.array([0.0, 1.0, 1.0, 1.0])
    else:
        raise ValueError(kind)
    return c


# name -> (builder(dtype) -> case, how it ends, least number of steps of a 'conv' case)
CASES = {
    # a. class counts
    'C1': (lambda dt: dict(prob=draw(300, 1, 1), priors=np.array([1.0]), weights=1, similarity=True, max_steps=10000), 1, 0),
    'C2': (lambda dt: _plain(4000, 2, 2), 'conv', 3),
    'C3': (lambda dt: _plain(3001, 3, 3), 'conv', 3),
    'C4': (lambda dt: _plain(2999, 4, 4), 'conv', 3),
    'C5': (lambda dt: _plain(3000, 5, 5), 'conv', 15),
    'C61': (lambda dt: _plain(3000, 61, 6, max_steps=150), 'cap', 0),
    'C255': (lambda dt: _plain(2000, 255, 7, max_steps=40), 'cap', 0),
    'C256': (lambda dt: _plain(2001, 256, 8, max_steps=40), 'cap', 0),
    'C257': (lambda dt: _plain(2500, 257, 9), 'conv', 95),
    'C1000': (lambda dt: _plain(3000, 1000, 10, max_steps=40), 'cap', 0),
    'C4096': (lambda dt: _plain(600, 4096, 11, max_steps=7), 'cap', 0),
    'C257_n1': (lambda dt: _plain(1, 257, 12, max_steps=5), 'cap', 0),
    'C4096_n1': (lambda dt: _plain(1, 4096, 13, max_steps=3), 'cap', 0),
    # b. row counts (below, at and just above one workgroup of 256 rows; the strided argmax pass above 2048 * 256 rows)
    'n1': (lambda dt: _plain(1, 3, 21, max_steps=40), 'cap', 0),
    'n5': (lambda dt: _plain(5, 3, 22, max_steps=40), 'cap', 0),
    'n255': (lambda dt: _plain(255, 3, 23, max_steps=40), 'conv', 15),
    'n256': (lambda dt: _plain(256, 3, 24, max_steps=40), 'cap', 0),
    'n257': (lambda dt: _plain(257, 3, 25, max_steps=40), 'cap', 0),
    'n530000': (lambda dt: _plain(530000, 3, 26), 'conv', 7),
    # c. first-look decisions
    'one_step': (_one_step, 1, 0),
    'two_steps': (_two_steps, 2, 0),
    # d. dissimilarities (argmin, dt = +0.1) with priors
    'argmin_C5': (lambda dt: _plain(3000, 5, 41, similarity=False), 'conv', 15),
    'argmin_C257': (lambda dt: _plain(2500, 257, 42, max_steps=100, similarity=False), 'cap', 0),
    # e. exact ties between classes
    'ties_argmax': (lambda dt: _ties(True), 'cap', 0),
    'ties_argmin': (lambda dt: _ties(False), 'cap', 0),
}
DEGENERATE = ('constant', 'nan', 'inf', 'priors_sum', 'prior_zero', 'w_negative', 'w0_zero')
for _k in DEGENERATE:
    CASES['deg_' + _k] = ((lambda kind: lambda dt: _degenerate(kind))(_k), None, 0)     # how these end is the reference's business

# c. the step cap on and beside every look: an input that never converges (class sizes move in steps of 1/257 > 1e-3) and one
# that converges by itself after a few dozen steps
NEVER = lambda cap: _plain(257, 3, 33, max_steps=cap)         # noqa: E731
CONVERGES = lambda cap: _plain(3000, 5, 34, max_steps=cap)    # noqa: E731

# g. the one-shot entry point's cached buffers: shrinking and growing n, changing C
REUSE = [(5000, 5, 10000), (300, 5, 60), (300, 257, 30), (7000, 257, 30), (10, 1, 10000), (5000, 5, 10000)]


def build(name, dtype_name):
    c = dict(CASES[name][0](DTYPES[dtype_name]))
    c['prob'] = np.ascontiguousarray(c['prob'].astype(DTYPES[dtype_name]))
    return c


def run_ref(c, max_steps=None):
    """The restatement on a case: (labels, weights, err, steps)."""
    with np.errstate(all='ignore'):
        return ref.volume_label_projection(c['prob'], c['priors'], c['weights'], c['similarity'],
                                           c['max_steps'] if max_steps is None else max_steps)


@functools.lru_cache(maxsize=None)
def case_and_ref(name, dtype_name):
    c = build(name, dtype_name)
    return c, run_ref(c)


@functools.lru_cache(maxsize=None)
def cap_case_and_ref(which, cap, dtype_name):
    c = dict((NEVER if which == 'never' else CONVERGES)(cap))
    c['prob'] = np.ascontiguousarray(c['prob'].astype(DTYPES[dtype_name]))
    return c, run_ref(c)


@functools.lru_cache(maxsize=None)
def reuse_case_and_ref(pos, dtype_name):
    n, C, cap = REUSE[pos]
    c = _plain(n, C, 70 + C + n % 7, max_steps=cap)
    c['prob'] = np.ascontiguousarray(c['prob'].astype(DTYPES[dtype_name]))
    return c, run_ref(c)


def ends_as_stated(name, res, c):
    """Does the reference run `res` of case `name` end the way the case is there for?"""
    how, least = CASES[name][1], CASES[name][2]
    _, _, err, steps = res
    if how == 'cap':
        return steps == c['max_steps'] and err > 1e-3
    if how == 'conv':
        return least <= steps < c['max_steps'] and err <= 1e-3
    if how is None:
        return steps <= c['max_steps']
    return steps == how and err <= 1e-3
