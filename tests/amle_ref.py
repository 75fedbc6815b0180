"""graph.amle restated in plain Python / numpy: the three loops of the reference's lip_iterate (c_code/lp_iterate.cpp:129-259 -- the
vertex blocks of the sorted entry list, the unweighted update, the weighted bisection update) in two forms that must agree bit for
bit,

    sequential   vertex after vertex in index order on the in-place array, as the reference runs them (Python floats: IEEE doubles,
                 every operation rounded on its own);
    levelled     level after level of `levels` (the schedule the device uses), the vertices of a level at once with numpy;

and the level function itself.  Every form returns (u, sweeps done, error history).  MIN(a,b) is `a if a < b else b`, MAX(a,b) is
`a if a > b else b`, ABS(a) is `-a if a < 0 else a`, as in the reference's vector_operations.h: the entry order decides the sign of a
zero and the rounding of the sums.

GOLDEN_GRAPHS / GOLDEN_CASES describe the fixtures tests/golden/g15_amle*.npz (tests/golden/make_golden_amle.py)."""
import numpy as np
from scipy import sparse

# name -> how the generator builds the graph (the fixtures hold the result as CSR)
GOLDEN_GRAPHS = {
    'blobs': dict(kind='blobs', n=3000, d=5, C=3, seed=3, k=8, kernel='gaussian', symmetrize=True),
    'blobs_dir': dict(kind='blobs', n=3000, d=5, C=3, seed=3, k=8, kernel='gaussian', symmetrize=False),
    'sorted': dict(kind='sorted', n=2500, d=2, seed=5, k=6, kernel='gaussian', symmetrize=True),
    'path': dict(kind='path', n=1500),
    'ball': dict(kind='ball', n=1200, d=2, seed=7, eps=0.06, kernel='gaussian'),
    'diag': dict(kind='diag', n=900, d=3, seed=9, k=5, kernel='gaussian', symmetrize=True),
}

# name -> (graph, boundary: ('labels', per class) | ('ends',) | ('random', m), weighted, tol, T, alpha, beta)
# a 'labels' case is the learner's: one column per class, the 0/1 indicator of the class on the labelled vertices
GOLDEN_CASES = {
    'blobs_u_3': ('blobs', ('labels', 4), False, 1e-3, 100000, 0.0, 1.0),
    'blobs_u_5': ('blobs', ('labels', 4), False, 1e-5, 100000, 0.0, 1.0),
    'blobs_w_3': ('blobs', ('labels', 4), True, 1e-3, 100000, 0.0, 1.0),
    'blobs_w_5': ('blobs', ('labels', 4), True, 1e-5, 100000, 0.0, 1.0),
    'blobsdir_u': ('blobs_dir', ('labels', 4), False, 1e-3, 100000, 0.0, 1.0),
    'blobsdir_w': ('blobs_dir', ('labels', 4), True, 1e-3, 100000, 0.0, 1.0),
    'sorted_u': ('sorted', ('random', 12), False, 1e-3, 100000, 0.0, 1.0),
    'sorted_w': ('sorted', ('random', 12), True, 1e-3, 100000, 0.0, 1.0),
    'path_u': ('path', ('ends',), False, 1e-3, 100000, 0.0, 1.0),
    'path_w': ('path', ('ends',), True, 1e-3, 1000, 0.0, 1.0),
    'ball_u': ('ball', ('random', 9), False, 1e-4, 100000, 0.0, 1.0),
    'ball_w': ('ball', ('random', 9), True, 1e-4, 100000, 0.0, 1.0),
    'diag_u': ('diag', ('random', 7), False, 1e-4, 100000, 0.0, 1.0),
    'diag_w': ('diag', ('random', 7), True, 1e-4, 100000, 0.0, 1.0),
    # stops: no sweep, fewer sweeps than 22, a tolerance everything is below (exactly 22 sweeps)
    'stop_T0': ('diag', ('random', 7), True, 1e-5, 0, 0.0, 1.0),
    'stop_T5_u': ('blobs_dir', ('random', 7), False, 1e-5, 5, 0.0, 1.0),
    'stop_T5_w': ('sorted', ('random', 7), True, 1e-5, 5, 0.0, 1.0),
    'stop_tol10_u': ('ball', ('random', 7), False, 10.0, 1000, 0.0, 1.0),
    'stop_tol10_w': ('ball', ('random', 7), True, 10.0, 1000, 0.0, 1.0),
    # graph.plaplace(fast=True)'s arguments: lip_iterate_main with alpha = 1/(p-1), beta = 1-alpha, tol 1e-6
    'alpha_p3': ('blobs', ('random', 10), False, 1e-6, 100000, 1 / (3 - 1), 1 - 1 / (3 - 1)),
    'alpha_p10': ('blobs_dir', ('random', 10), False, 1e-6, 100000, 1 / (10 - 1), 1 - 1 / (10 - 1)),
}


def entries(W):
    """(rows, nbr, V): the stored entries sorted by vertex, the expressions of the reference's __ccode_init__ (graph.py:69-84)."""
    I, J, V = sparse.find(sparse.csr_matrix(W))
    ind = np.argsort(I)
    return (np.ascontiguousarray(I[ind], dtype=np.int32), np.ascontiguousarray(J[ind], dtype=np.int32),
            np.ascontiguousarray(V[ind], dtype=np.float64))


def blocks(n, rows):
    """start (n + 1,): vertex i's entries are start[i] .. start[i + 1] of the sorted list (lp_iterate.cpp:138-145)."""
    return np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=n)))).astype(np.int64)


def boundary(n, ind, val):
    """mask (n,), u0 (n,): `u[ind[j]] = val[j]` in order -- a vertex listed twice takes its last value."""
    mask = np.zeros(n, dtype=bool)
    u0 = np.zeros(n)
    for q, i in enumerate(ind):
        u0[i] = val[q]
        mask[i] = True
    return mask, u0


def levels(n, rows, nbr, mask):
    """level (n,) int: -1 on the boundary; 0 where no lower-numbered non-boundary vertex is adjacent in the pattern of W or of its
    transpose; else 1 + the largest level among those.  Written from the definition: W's pattern and the transposed one apart."""
    lower = [[] for _ in range(n)]
    for i, j in zip(rows.tolist(), nbr.tolist()):
        if i == j or mask[i] or mask[j]:
            continue
        lo, hi = (i, j) if i < j else (j, i)
        lower[hi].append(lo)          # entry (hi, lo) or its transpose (lo, hi): hi waits for lo either way
    level = np.full(n, -1, dtype=np.int64)
    for i in range(n):
        if not mask[i]:
            level[i] = 1 + max((level[j] for j in lower[i]), default=-1)
    return level


def _update(u, nb, w, weighted, alpha, beta):
    """The new value of a vertex whose entries are nb (indices) and w (weights), Python floats."""
    first = u[nb[0]]
    minu = maxu = first
    if not weighted:
        sumu = 0.0
        deg = 0.0
        for j, wj in zip(nb, w):
            x = u[j]
            sumu = sumu + wj * x
            deg = deg + wj
            minu = x if x < minu else minu
            maxu = x if x > maxu else maxu
        return alpha * sumu / deg + beta * (minu + maxu) / 2
    for j in nb:
        x = u[j]
        minu = x if x < minu else minu
        maxu = x if x > maxu else maxu
    a, b = minu, maxu
    xs = [u[j] for j in nb]
    for _ in range(30):
        minw = 0.0
        maxw = 0.0
        t = (a + b) / 2.0
        for x, wj in zip(xs, w):
            v = wj * (t - x)
            minw = v if v < minw else minw
            maxw = v if v > maxw else maxw
        if minw + maxw > 0:
            b = t
        else:
            a = t
    return (a + b) / 2.0


def sequential(n, rows, nbr, V, ind, val, weighted, alpha=0.0, beta=1.0, T=1000, tol=1e-5):
    """The reference's loop as it stands.  Returns (u (n,), sweeps done, [err of every sweep])."""
    start = blocks(n, rows).tolist()
    mask, u0 = boundary(n, ind, val)
    u = u0.tolist()
    nbl, wl = nbr.tolist(), V.tolist()
    todo = [(i, nbl[start[i]:start[i + 1]], wl[start[i]:start[i + 1]]) for i in range(n) if not mask[i]]
    errs = []
    with np.errstate(all='ignore'):
        for it in range(T):
            err = 0.0
            for i, nb, w in todo:
                ne = _update(u, nb, w, weighted, alpha, beta)
                d = u[i] - ne
                d = -d if d < 0 else d
                err = d if d > err else err
                u[i] = ne
            errs.append(err)
            if err < tol and it > 20:
                break
    return np.array(u, dtype=np.float64), len(errs), errs


def levelled(n, rows, nbr, V, ind, val, weighted, alpha=0.0, beta=1.0, T=1000, tol=1e-5):
    """Level after level; the vertices of a level at once (they read nothing a vertex of their own level writes).  A vertex's
    entries are folded left to right, position after position, so that every sum and every zero is the sequential loop's."""
    start = blocks(n, rows)
    mask, u = boundary(n, ind, val)
    level = levels(n, rows, nbr, mask)
    plan = []
    for l in range(int(level.max()) + 1 if (~mask).any() else 0):
        vs = np.where(level == l)[0]
        cnt = (start[vs + 1] - start[vs]).astype(np.int64)
        D = int(cnt.max())
        pos = np.arange(D)[None, :]
        valid = pos < cnt[:, None]
        at = np.where(valid, start[vs][:, None] + pos, start[vs][:, None])
        plan.append((vs, nbr[at], np.where(valid, V[at], 0.0), valid, D))
    errs = []
    with np.errstate(all='ignore'):
        for it in range(T):
            err = 0.0
            for vs, nb, w, valid, D in plan:
                X = u[nb]
                minu = X[:, 0].copy()
                maxu = X[:, 0].copy()
                sumu = np.zeros(len(vs))
                deg = np.zeros(len(vs))
                for d in range(D):
                    ok = valid[:, d]
                    x = X[:, d]
                    if not weighted:
                        sumu = np.where(ok, sumu + w[:, d] * x, sumu)
                        deg = np.where(ok, deg + w[:, d], deg)
                    minu = np.where(ok & (x < minu), x, minu)
                    maxu = np.where(ok & (x > maxu), x, maxu)
                if not weighted:
                    ne = alpha * sumu / deg + beta * (minu + maxu) / 2
                else:
                    a, b = minu, maxu
                    for _ in range(30):
                        t = (a + b) / 2.0
                        v = w * (t[:, None] - X)
                        # only whether minw + maxw > 0 is used: neither the order of the fold nor the sign of a zero reaches it;
                        # a NaN product leaves minw and maxw alone (MIN / MAX with the NaN on the left), like a product of 0
                        v = np.where(valid & ~np.isnan(v), v, 0.0)
                        up = np.minimum(v.min(axis=1), 0.0) + np.maximum(v.max(axis=1), 0.0) > 0
                        b = np.where(up, t, b)
                        a = np.where(up, a, t)
                    ne = (a + b) / 2.0
                d = np.abs(u[vs] - ne)
                d = d[d > 0]
                if len(d) and d.max() > err:
                    err = float(d.max())
                u[vs] = ne
            errs.append(err)
            if err < tol and it > 20:
                break
    return u, len(errs), errs


def python_forms_fit(sweeps, n_entries, nlevels, weighted):
    """Which of the two Python forms finish a column of this length within a few seconds: `sequential` costs about
    sweeps * entries (* 30 bisection passes) interpreted operations, `levelled` sweeps * levels batches of numpy calls (about 0.1 ms a
    batch unweighted, 1.5 ms weighted).  The numpy form then covers every unweighted golden but the sorted plane and the path (48 000
    and 380 000 batches) and the shortest column of the weighted blobs cases; the other cases are checked with the compiled host
    restatement (tests/lip_plan_host.cpp), both forms."""
    forms = set()
    if sweeps * n_entries * (30 if weighted else 1) <= 2500000:
        forms.add('sequential')
    if sweeps * nlevels <= (3600 if weighted else 12000):
        forms.add('levelled')
    return forms


def case_boundary(name, W, labels=None, train_ind=None):
    """(ind (m,), vals (m, B)) of a golden case, derived from its name alone (the generator stores them too)."""
    import zlib
    gname, bd = GOLDEN_CASES[name][:2]
    n = W.shape[0]
    if bd[0] == 'labels':
        classes = np.unique(labels[train_ind])
        return train_ind.astype(np.int64), (labels[train_ind][:, None] == classes[None, :]).astype(np.float64)
    if bd[0] == 'ends':
        return np.array([0, n - 1], dtype=np.int64), np.array([[0.0], [1.0]])
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    ind = np.sort(rng.choice(n, size=bd[1], replace=False)).astype(np.int64)
    return ind, rng.random((bd[1], 1))


# ---- the host build of csrc/lip_plan.h and the long-case restatement (tests/lip_plan_host.cpp) ------------------------------------
def build_host_lib(outdir):
    import ctypes
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    out = os.path.join(str(outdir), 'liblph.so')
    subprocess.run(['g++', '-O2', '-ffp-contract=off', '-shared', '-fPIC', '-o', out, os.path.join(here, 'lip_plan_host.cpp')], check=True)
    lib = ctypes.CDLL(out)
    vp = ctypes.c_void_p
    lib.lph_constants.argtypes = [vp]
    lib.lph_plan.argtypes = [ctypes.c_int64, vp, vp, vp, ctypes.c_int, vp, vp, vp, vp, vp]
    lib.lph_sweeps.argtypes = [ctypes.c_int64, vp, vp, vp, vp, vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int64,
                               ctypes.c_double, ctypes.c_int, vp]
    lib.lph_sweeps.restype = ctypes.c_int64
    lib.lph_plan.restype = None
    lib.lph_constants.restype = None
    return lib


def _p(a):
    return a.ctypes.data


def host_constants(lib):
    out = np.zeros(3, dtype=np.int64)
    lib.lph_constants(_p(out))
    return dict(small=int(out[0]), block=int(out[1]), chunk=int(out[2]))


def host_plan(lib, n, rows, nbr, mask, small=-1):
    """The plan of csrc/lip_plan.h: dict(level, order, lvl_ptr, launches (k, 3): lvl0, lvl1, merged)."""
    start = blocks(n, rows)
    nbr = np.ascontiguousarray(nbr, dtype=np.int32)
    bdy = np.ascontiguousarray(mask, dtype=np.uint8)
    level = np.zeros(n, dtype=np.int32)
    order = np.zeros(n, dtype=np.int32)
    lvl_ptr = np.zeros(n + 1, dtype=np.int64)
    launches = np.zeros(3 * max(n, 1), dtype=np.int32)
    counts = np.zeros(3, dtype=np.int64)
    lib.lph_plan(n, _p(start), _p(nbr), _p(bdy), int(small), _p(level), _p(order), _p(lvl_ptr), _p(launches), _p(counts))
    nl, no, nk = (int(c) for c in counts)
    return dict(level=level, order=order[:no], lvl_ptr=lvl_ptr[:nl + 1], launches=launches[:3 * nk].reshape(nk, 3), nlevels=nl)


def host_sweeps(lib, n, rows, nbr, V, ind, val, weighted, alpha=0.0, beta=1.0, T=1000, tol=1e-5, levelled=False):
    """The long-case restatement: (u, sweeps done, errs) like `sequential` / `levelled`."""
    start = blocks(n, rows)
    nbr = np.ascontiguousarray(nbr, dtype=np.int32)
    V = np.ascontiguousarray(V, dtype=np.float64)
    mask, u = boundary(n, ind, val)
    bdy = np.ascontiguousarray(mask, dtype=np.uint8)
    errs = np.zeros(max(int(T), 1))
    done = lib.lph_sweeps(n, _p(start), _p(nbr), _p(V), _p(bdy), _p(u), 1 if weighted else 0, float(alpha), float(beta), int(T), float(tol),
                          1 if levelled else 0, _p(errs))
    return u, int(done), errs[:done].tolist()
