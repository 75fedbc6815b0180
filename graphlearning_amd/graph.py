"""Graph object: the part of reference graphlearning/graph.py on the hot path
(`graph.__init__` :25-67, `degree_vector` :108-122, `degree_matrix` :210-233,
`laplacian` :469-513) and its shortest-path family (`dijkstra` :1077-1175, `dijkstra_hl`
:916-997, `distance` :999-1046, `distance_matrix` :1048-1075).  The reference's `__ccode_init__` (graph.py:69-84, 0.4-0.6 s per
construction at 70k nodes, never used by this path) is not executed."""
import sys
import numpy as np
from scipy import sparse


# distance_matrix: values (vertices x sources) of one batched device call -- 2^26 doubles are 512 MiB on the device and in the result
_DISTANCE_MATRIX_VALUES = 1 << 26


class graph:
    def __init__(self, W, labels=None, features=None, label_names=None, node_names=None):
        self.weight_matrix = sparse.csr_matrix(W)
        if getattr(W, '_glx_sym', None) is not None:
            self.weight_matrix._glx_sym = W._glx_sym      # a CONTENT fingerprint: utils.known_symmetric re-hashes the arrays, so an edited copy is simply unknown
        if getattr(W, '_glx_order', None) is not None:
            self.weight_matrix._glx_order = W._glx_order    # (a vertex order stays valid whatever happens to the values)
        self.labels = labels
        self.features = features
        self.num_nodes = W.shape[0]
        self.label_names = label_names
        self.node_names = node_names
        # what eigen_decomp computed last, per normalization (reference graph.py:55-67)
        self.eigendata = {norm: dict.fromkeys(('eigenvectors', 'eigenvalues', 'method', 'k', 'c', 'gamma', 'tol', 'q'))
                          for norm in ('combinatorial', 'randomwalk', 'normalized')}
        self.eig_steps = self.eig_restarts = self.eig_probe = None

    def degree_vector(self):
        """d_i = sum_j w_ij (row sums; reference graph.py:108-122)."""
        return self.weight_matrix * np.ones(self.num_nodes)

    def degree_matrix(self, p=1):
        """Sparse diagonal matrix of d^p (reference graph.py:210-233)."""
        d = self.degree_vector()
        return sparse.spdiags(d ** p, 0, self.num_nodes, self.num_nodes).tocsr()

    def laplacian(self, normalization='combinatorial'):
        """D-W, I-D^-1 W or I-D^-1/2 W D^-1/2 (reference graph.py:469-513)."""
        I = sparse.identity(self.num_nodes)
        D = self.degree_matrix()
        if normalization == 'combinatorial':
            L = D - self.weight_matrix
        elif normalization == 'randomwalk':
            L = I - self.degree_matrix(p=-1) * self.weight_matrix
        elif normalization == 'normalized':
            Dh = self.degree_matrix(p=-0.5)
            L = I - Dh * self.weight_matrix * Dh
        else:
            sys.exit('Invalid option for graph Laplacian normalization.')
        return L.tocsr()

    def eigen_decomp(self, normalization='combinatorial', method='exact', k=10, c=None, gamma=0, tol=0, q=1, device=None):
        """The k lowest eigenvalues (ascending) and eigenvectors (n, k) of the combinatorial, random-walk or normalised graph
        Laplacian (reference graph.py:623-850, method='exact', gamma=0), cached in self.eigendata[normalization] under the reference's
        six parameters.  The reference takes `svds` (ARPACK) of A = D^-1/2 W D^-1/2, or of M I - L with M = 2 max(deg), and returns
        1 - s or M - s; here the k largest singular values of the same A, built on the host by the same scipy expressions, come from
        thick-restart Lanczos with full reorthogonalisation on A A on the GPU (csrc/eig.hip, _eig.py).  `tol` is the
        relative residual at which a Ritz pair counts as converged, 0 = machine precision as in ARPACK.  The vectors are the
        eigenvectors v of A A (scipy's u = A v / s is +-v for a symmetric A), times D^-1/2 for 'randomwalk' as in the reference;
        their signs are arbitrary, as the reference's are.  Sets eig_steps (Lanczos steps), eig_restarts and eig_probe.

        The result is held to a TOLERANCE contract against the reference (eigenvalues, invariant subspace, residual: the bounds
        measured in tests/golden/g19_eig.npz), and to a bit-for-bit contract against the host restatement of csrc/eig_plan.h.

        Stated deviations, each a ValueError before any device call: a W that is not symmetric bit for bit, a vertex of degree 0 for
        the two normalised forms, NaN / infinite / negative weights, k < 1, k >= n, k > 256.  NotImplementedError: method='lowrank'
        (randomised SVD) and gamma != 0 (modularity).  GlxError at run time: a breakdown (fewer reachable distinct eigenvalues than
        basis columns, e.g. a complete graph), and a missed multiple eigenvalue -- a single-vector Krylov method finds one vector per
        distinct eigenvalue, so after convergence a second random vector probes the complement for a few steps; disconnected and
        bipartite graphs usually end there.  The probe detects, it does not prove absence, and nothing is repaired."""
        from . import _hip, _eig
        if c is None:
            c = 2 * k
        if normalization not in self.eigendata:
            sys.exit('Invalid choice of normalization')
        data = self.eigendata[normalization]
        params = {'method': method, 'k': k, 'c': c, 'gamma': gamma, 'tol': tol, 'q': q}
        if data['eigenvalues'] is not None and all(data[name] == value for name, value in params.items()):
            return data['eigenvalues'], data['eigenvectors']
        if method == 'lowrank':
            raise NotImplementedError("eigen_decomp(method='lowrank') is randomised SVD, which this package does not provide")
        if method != 'exact':
            sys.exit('Invalid eigensolver method ' + method)
        if gamma != 0:
            raise NotImplementedError('eigen_decomp(gamma != 0) needs an eigensolver on an operator with a rank-one term '
                                      '(modularity), which this package does not provide')
        k = int(k)
        _eig.check_weights(self.weight_matrix, normalization, k)
        A, D, M = _eig.operator(self.weight_matrix, normalization)
        n = self.num_nodes
        with _hip.Eig(A.indptr, A.indices, A.data, _eig.basis_size(n, k), device=device) as backend:
            theta, self.eig_steps, self.eig_restarts, self.eig_probe = _eig.thick_restart(backend, n, k, tol=tol)
            vecs = backend.get_columns(0, k)
        s = np.sqrt(np.maximum(theta, 0.0))
        vals = (1 - s) if M is None else (M - s)
        ind = np.argsort(vals, kind='stable')
        vals, vecs = vals[ind], vecs[:, ind]
        if normalization == 'randomwalk':
            vecs = D @ vecs
        data.update(params)
        data['eigenvalues'], data['eigenvectors'] = vals, vecs
        return vals, vecs

    def reweight(self, idx, method='poisson', normalization='combinatorial', tau=0, X=None, alpha=2, zeta=1e7, r=0.1):
        """Reweight the graph more heavily near the labelled nodes `idx` (reference
        graph.py:368-466).  'poisson' solves one Poisson problem with the GPU conjugate-gradient
        solver (1-D right-hand side: numpy's pairwise-summed reductions are reproduced);
        'wnll' is a diagonal scaling; 'properly' scales by the distance to the nearest labelled point (all pairs on
        the GPU, glx_nearest_dist: cKDTree's distances bit for bit).  (The 'poisson' system is the singular graph Laplacian: its
        conjugate-gradient iterates amplify rounding, so the solve always uses the reference-order
        reductions -- the tolerance mode of ssl.laplace / ssl.randomwalk does not apply here.)"""
        from . import utils
        n = self.num_nodes
        if method == 'poisson':
            f = np.zeros(n)
            f[idx] = 1
            if normalization == 'combinatorial':
                f -= np.mean(f)
                L = self.laplacian()
            elif normalization == 'normalized':
                d = self.degree_vector() ** (0.5)
                c = np.sum(d * f) / np.sum(d)
                f -= c
                L = self.laplacian(normalization=normalization)
            else:
                sys.exit('Unsupported normalization ' + normalization + ' for graph.reweight.')
            w = utils.conjgrad(L, f, tol=1e-5)
            w -= np.min(w)
            w += 1e-5
            D = sparse.spdiags(w, 0, n, n).tocsr()
            return D * self.weight_matrix * D
        elif method == 'wnll':
            m = len(idx)
            a = np.ones((n,))
            a[idx] = n / m
            D = sparse.spdiags(a, 0, n, n).tocsr()
            return D * self.weight_matrix + self.weight_matrix * D
        elif method == 'properly':     # reference graph.py:448-462
            if X is None:
                sys.exit('Must provide data features X for properly weighted graph Laplacian.')
            from . import _hip
            rzeta = r / (zeta - 1) ** (1 / alpha)
            # `D, J = cKDTree(X[idx, :]).query(X)`: the distance to the nearest labelled point, all pairs on the GPU (the reference's bits)
            D = _hip.nearest_dist(X, idx)
            D[D < rzeta] = rzeta
            gamma = 1 + (r / D) ** alpha
            D = sparse.spdiags(gamma, 0, n, n).tocsr()
            return D * self.weight_matrix + self.weight_matrix * D
        else:
            sys.exit('Invalid reweighting method ' + method + '.')

    def page_rank(self, alpha=0.85, v=None, tol=1e-10, device=None):
        """PageRank vector by the power iteration u <- alpha P u + (1-alpha) v, P = W^T D^-1, from
        u = 1/n until max|u_new - u_old| <= tol (reference graph.py:1371-1412).  The host builds
        alpha*P with the reference's own scipy expressions; every sweep and the stop test run on the
        GPU (glx_affine_iterate).  Bit-identical to the reference: a row's products are added in
        the order scipy's matvec of that matrix adds them."""
        from . import _hip
        n = self.num_nodes
        u = np.ones((n,)) / n
        if v is None:
            v = np.ones((n,)) / n
        D = self.degree_matrix(p=-1)
        P = self.weight_matrix.T @ D
        aP = alpha * P              # `alpha*P@u` in the reference is (alpha*P)@u
        # csc_matvec adds a row's products column after column (ascending), which is the row order
        # csc -> csr conversion produces; a csr operand is used by csr_matvec in stored order
        A = aP.tocsr()
        self.page_rank_iters = 0
        if not (tol + 1 > tol):     # `err = tol+1; while err > tol` never enters the loop
            return u
        dev = _hip.DeviceGraph(A, dtype=np.float64, device=device)
        try:
            u, it, _ = dev.affine_iterate(u, b=(1 - alpha) * v, tol=tol)
        finally:
            dev.close()
        self.page_rank_iters = it
        return u

    def __ccode_init__(self):
        """Stored entries as (vertex, neighbour, weight) arrays sorted by vertex, the form the
        reference hands to its C extension (reference graph.py:69-84, same expressions: the order
        inside a vertex's block is whatever np.argsort's default sort leaves)."""
        I, J, V = sparse.find(self.weight_matrix)
        ind = np.argsort(I)
        self.I, self.J, self.V = I[ind], J[ind], V[ind]
        self.I = np.ascontiguousarray(self.I, dtype=np.int32)
        self.J = np.ascontiguousarray(self.J, dtype=np.int32)
        self.V = np.ascontiguousarray(self.V, dtype=np.float64)

    def _entries(self):
        if getattr(self, 'I', None) is None:
            self.__ccode_init__()
        return self.I, self.J, self.V

    def adjacency(self):
        """The 0/1 pattern of the weight matrix as a float CSR matrix: A_ij = 1 where w_ij is stored and nonzero (reference
        graph.py:274-290).  Host scipy, on the arrays of __ccode_init__."""
        I, J, V = self._entries()
        n = self.num_nodes
        return sparse.coo_matrix((np.ones(len(V)), (I, J)), shape=(n, n)).tocsr()

    def gradient(self, u, weighted=False, p=0.0):
        """Graph gradient of the vertex function u: the sparse matrix with (u_j - u_i) on every entry (i, j) of the weight matrix,
        times w_ij^p when weighted (reference graph.py:292-332: p != 0 implies weighted, weighted with p == 0 means p = 1).  Host scipy."""
        I, J, V = self._entries()
        n = self.num_nodes
        if p != 0.0:
            weighted = True
        if weighted == True and p == 0.0:
            p = 1.0
        diff = u[J] - u[I]
        vals = (V ** p) * diff if weighted else diff
        return sparse.coo_matrix((vals, (I, J)), shape=(n, n)).tocsr()

    def divergence(self, V, weighted=True):
        """Graph divergence of the edge field V (a sparse matrix): half the row sums of V - V^T, entry by entry times the weight
        matrix when weighted (reference graph.py:334-365).  Host scipy."""
        V = V - V.transpose()
        if weighted:
            V = V.multiply(self.weight_matrix)
        return V * np.ones(self.num_nodes) / 2

    def plaplace(self, bdy_set, bdy_val, p, tol=1e-1, max_num_it=1e6, prog=False, fast=True, device=None):
        """Game-theoretic p-Laplace equation with Dirichlet data (reference graph.py:1177-1278).
        `fast=False` -- the Jacobi iteration of upper / lower barriers, lp_iterate_main of the
        reference's C extension -- runs on the GPU (glx_lp_iterate) and returns (uu+ul)/2 like the
        reference.  The reference's default `fast=True` is an in-order Gauss-Seidel sweep (lip_iterate_main,
        c_code/lp_iterate.cpp:129-187) with alpha = 1/(p-1), beta = 1-alpha.  Such a sweep does have an exact parallel form, the
        level schedule of a sparse triangular solve, and the device routine behind `graph.amle` (glx_lip_iterate) runs it with
        these arguments bit for bit; `fast=True` itself is not switched on yet and is refused rather than answered by another
        iteration."""
        from . import _hip, utils
        if fast:
            raise NotImplementedError('graph.plaplace(fast=True) is not switched on yet (its in-order Gauss-Seidel sweep runs on the GPU as '
                                      '_hip.lip_iterate with alpha=1/(p-1), beta=1-alpha); pass fast=False for the Jacobi iteration')
        if getattr(self, 'I', None) is None:
            self.__ccode_init__()
        n = self.num_nodes
        bdy_set, bdy_val = utils._boundary_handling(bdy_set, bdy_val)
        uu = np.max(bdy_val) * np.ones((n,))
        ul = np.min(bdy_val) * np.ones((n,))
        uu[bdy_set] = bdy_val
        ul[bdy_set] = bdy_val
        uu = np.ascontiguousarray(uu, dtype=np.float64)
        ul = np.ascontiguousarray(ul, dtype=np.float64)
        bdy_set = np.ascontiguousarray(bdy_set, dtype=np.int32)
        bdy_val = np.ascontiguousarray(bdy_val, dtype=np.float64)
        self.plaplace_iters = _hip.lp_iterate(uu, ul, self.J, self.I, self.V, bdy_set, bdy_val, p, int(max_num_it), float(tol),
                                              device=device)
        return (uu + ul) / 2

    def _amle_entries(self):
        """The arrays of __ccode_init__ checked for graph.amle: every weight >= 0 (NaN refused), and which vertices have an entry."""
        if getattr(self, 'I', None) is None:
            self.__ccode_init__()
        if not np.all(self.V >= 0):
            raise ValueError('graph.amle: the weight matrix has a negative or NaN entry')
        return np.bincount(self.I, minlength=self.num_nodes) > 0

    def _lip_checked(self, what, bdy_set, vals, max_num_it):
        """The arguments of a batched in-order sweep (_hip.lip_iterate), checked: (bdy_set int64, vals (m, B) float64, T).  ValueError,
        before any device call: values whose shape does not match the boundary set, an index out of range, a non-finite value, more
        than 2^24 sweeps, a negative or NaN weight, a vertex off the boundary without a stored entry."""
        from . import utils
        n = self.num_nodes
        bdy_set, _ = utils._boundary_handling(bdy_set, 0)
        bdy_set = np.ascontiguousarray(bdy_set, dtype=np.int64).ravel()
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        if vals.ndim != 2 or vals.shape[0] != len(bdy_set) or vals.shape[1] < 1:
            raise ValueError('%s: boundary values of shape %s for %d boundary vertices' % (what, vals.shape, len(bdy_set)))
        if len(bdy_set) and (bdy_set.min() < 0 or bdy_set.max() >= n):
            raise ValueError('%s: boundary index out of range' % what)
        if not np.all(np.isfinite(vals)):
            raise ValueError('%s: bdy_val has a non-finite entry' % what)
        T = int(float(max_num_it))
        if T > (1 << 24):
            raise ValueError('%s: max_num_it=%r above the supported 2^24 sweeps' % (what, max_num_it))
        T = max(T, 0)                    # `for(it=0;it<T;it++)`: a negative T sweeps nothing
        has_entry = self._amle_entries()
        free = ~has_entry
        free[bdy_set] = False
        if free.any():
            raise ValueError('%s: vertex %d is not on the boundary and has no stored entry (the reference reads another '
                             'vertex\'s entry there)' % (what, int(np.where(free)[0][0])))
        return bdy_set, vals, T

    def _amle_batch(self, bdy_set, vals, tol=1e-5, max_num_it=1000, weighted=True, prog=False, device=None, small_level=-1):
        """B AMLE problems that share the boundary vertices `bdy_set`, one per column of `vals` (m, B), in one device call
        (glx_lip_iterate): returns u (n, B) float64; every column equals its single `amle` call bit for bit, and stops on its own.
        Sets amle_iters (sweeps done per column), amle_levels and amle_plan (levels, launches per sweep, launches enqueued in all).
        With `prog` the reference's progress lines are printed AFTER the solve, from the errors the host read while it ran, one
        column after another (the order of the reference's class-by-class calls).  small_level: plan override for measurements
        (_hip.lip_iterate); the result does not depend on it."""
        from . import _hip
        n = self.num_nodes
        tol = float(tol)
        bdy_set, vals, T = self._lip_checked('graph.amle', bdy_set, vals, max_num_it)
        if not np.isfinite(tol):
            raise ValueError('graph.amle: tol is not finite')
        u, iters, plan, errs = _hip.lip_iterate(n, self.J, self.I, self.V, bdy_set.astype(np.int32), vals, weighted, 0.0, 1.0, T, tol,
                                                device=device, want_errors=bool(prog), small_level=small_level)
        self.amle_iters = iters
        self.amle_levels = plan[0]
        self.amle_plan = plan
        if prog:                         # the reference's lines (lp_iterate.cpp:156, :180), one column after another
            for b in range(vals.shape[1]):
                for it in range(int(iters[b])):
                    sys.stdout.write('Iter=%d, err=%.15f\n' % (it, errs[it, b]))
            sys.stdout.flush()
        return u

    def _plaplace_batch(self, bdy_set, vals, p, tol=1e-1, max_num_it=1e6, fast=True, device=None):
        """B p-Laplace problems (reference graph.py:1177-1278) that share the boundary vertices `bdy_set`, one per column of `vals`
        (m, B), in one device call: returns u (n, B) float64 and sets plaplace_iters (B,).  Every column stops on its own.
        fast=True: the reference's in-order Gauss-Seidel sweeps lip_iterate_main with alpha = 1/(p-1), beta = 1-alpha on the 0/1
        pattern, from zero, tol overridden to 1e-6 (graph.py:1259-1261), level by level through _hip.lip_iterate like graph.amle, with
        graph.amle's refusals; also sets plaplace_levels and plaplace_plan.  fast=False: the Jacobi iteration of upper and lower
        barriers through _hip.lp_iterate_batch, every column bit for bit its `plaplace(fast=False)` call; returns (uu + ul) / 2.
        Refused there with ValueError: values whose shape does not match the boundary set, an index out of range, more than 2^24
        iterations; a vertex without entries gives NaN as in the single call."""
        from . import _hip, utils
        n = self.num_nodes
        if fast:
            alpha = 1 / (p - 1)
            beta = 1 - alpha
            tol = 1e-6
            bdy_set, vals, T = self._lip_checked('graph.plaplace', bdy_set, vals, max_num_it)
            u, iters, plan, _ = _hip.lip_iterate(n, self.J, self.I, self.V, bdy_set.astype(np.int32), vals, False, alpha, beta, T, tol,
                                                 device=device)
            self.plaplace_iters = iters
            self.plaplace_levels = plan[0]
            self.plaplace_plan = plan
            return u
        bdy_set, _ = utils._boundary_handling(bdy_set, 0)
        bdy_set = np.ascontiguousarray(bdy_set, dtype=np.int64).ravel()
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        if vals.ndim != 2 or vals.shape[0] != len(bdy_set) or vals.shape[1] < 1:
            raise ValueError('graph.plaplace: boundary values of shape %s for %d boundary vertices' % (vals.shape, len(bdy_set)))
        if len(bdy_set) == 0:
            raise ValueError('graph.plaplace: no boundary vertex (the barriers start from the largest and smallest boundary value)')
        if bdy_set.min() < 0 or bdy_set.max() >= n:
            raise ValueError('graph.plaplace: boundary index out of range')
        T = int(float(max_num_it))
        if T > (1 << 24):
            raise ValueError('graph.plaplace: max_num_it=%r above the supported 2^24 iterations' % (max_num_it,))
        T = max(T, 0)
        I, J, V = self._entries()
        uu, ul, iters = _hip.lp_iterate_batch(n, J, I, V, bdy_set.astype(np.int32), vals, p, T, float(tol), device=device)
        self.plaplace_iters = iters
        return (uu + ul) / 2

    def amle(self, bdy_set, bdy_val, tol=1e-5, max_num_it=1000, weighted=True, prog=False, device=None):
        """Absolutely minimal Lipschitz extension of the boundary values: the solution of the graph infinity-Laplace equation
        min_j w_ij (u_i - u_j) + max_j w_ij (u_i - u_j) = 0 off the boundary (reference graph.py:1281-1332).  The reference's
        in-order Gauss-Seidel sweeps (lip_iterate_weighted_main: 30 bisection passes per vertex; `weighted=False`,
        lip_iterate_main: the midpoint of the smallest and largest neighbouring value) run on the GPU level by level
        (glx_lip_iterate; the argument heads csrc/lip_plan.h) and give the reference's iterates bit for bit.  Returns u float64
        (n,); sets amle_iters (sweeps done) and amle_levels.  With `prog` the reference's progress lines are printed after the solve
        has finished, not while it runs.  A vertex listed twice in `bdy_set` takes its last value.  Refused
        with ValueError: a vertex off the boundary without a stored entry (the reference reads another vertex's entry, or past
        its arrays), a negative or NaN weight, a non-finite `bdy_val` or `tol`."""
        from . import utils
        bdy_set, bdy_val = utils._boundary_handling(bdy_set, bdy_val)
        bdy_val = np.asarray(bdy_val, dtype=np.float64).ravel()
        u = self._amle_batch(bdy_set, bdy_val[:, None], tol=tol, max_num_it=max_num_it, weighted=weighted, prog=prog, device=device)
        self.amle_iters = int(self.amle_iters[0])
        return np.ascontiguousarray(u[:, 0])

    def _peikonal_batch(self, bdy_sets, bdy_vals=0, f=1, p=1, u0=None, num_bisection_it=30, device=None, max_rounds=0):
        """B p-eikonal problems on this graph in one device call (glx_peikonal): `bdy_sets` is a list of boundary sets (indices or
        masks), `bdy_vals` one value (a float or an array per set) for all of them or a list with one per set.  Returns u (n, B)
        float64; every column equals the single `peikonal` call bit for bit.  Sets peikonal_rounds.  Refused with ValueError before
        any device call: the refusals of `peikonal`.  max_rounds: a cap on the rounds below the library's own (a test hook)."""
        from . import _hip, utils
        n = self.num_nodes
        I, J, V = self._entries()
        if not np.all(np.isfinite(V) & (V > 0)):
            raise ValueError('graph.peikonal: the weight matrix has an entry that is not finite or not positive')
        if type(f) != np.ndarray:           # the reference's `f = np.ones((n,))*f`
            f = np.ones((n,)) * f
        f = np.ascontiguousarray(f, dtype=np.float64)
        if f.shape != (n,):
            raise ValueError('graph.peikonal: f has shape %s, expected (%d,)' % (f.shape, n))
        if not np.all(np.isfinite(f) & (f >= 0)):
            raise ValueError('graph.peikonal: f has an entry that is negative or not finite')
        u0 = np.zeros((n,)) if u0 is None else np.ascontiguousarray(u0, dtype=np.float64)
        if u0.shape != (n,):
            raise ValueError('graph.peikonal: u0 has shape %s, expected (%d,)' % (u0.shape, n))
        if not np.all(np.isfinite(u0)):
            raise ValueError('graph.peikonal: u0 has a non-finite entry')
        p = float(p)
        if not (np.isfinite(p) and p > 0):
            raise ValueError('graph.peikonal: p=%r is not finite or not positive' % (p,))
        nb = int(num_bisection_it)
        if nb != num_bisection_it or not 1 <= nb <= 128:
            raise ValueError('graph.peikonal: num_bisection_it=%r outside 1 .. 128' % (num_bisection_it,))
        bdy_sets = list(bdy_sets)
        B = len(bdy_sets)
        if not 1 <= B <= 256:
            raise ValueError('graph.peikonal: %d boundary sets in one call (1 .. 256 are supported)' % B)
        if n * B > (1 << 31):
            raise ValueError('graph.peikonal: n * B = %d values above the supported 2^31' % (n * B))
        if not isinstance(bdy_vals, (list, tuple)):
            bdy_vals = [bdy_vals] * B
        if len(bdy_vals) != B:
            raise ValueError('graph.peikonal: %d boundary value entries for %d boundary sets' % (len(bdy_vals), B))
        ptr, idx, val = [0], [], []
        for bdy_set, bdy_val in zip(bdy_sets, bdy_vals):
            bdy_set = np.asarray(bdy_set)
            m = int(np.sum(bdy_set)) if bdy_set.dtype == bool else bdy_set.size
            if np.ndim(bdy_val) > 0 and np.size(bdy_val) != m:
                raise ValueError('graph.peikonal: %d boundary values for %d boundary vertices' % (np.size(bdy_val), m))
            bdy_set, bdy_val = utils._boundary_handling(bdy_set, bdy_val)
            bdy_set = np.ascontiguousarray(bdy_set, dtype=np.int64).ravel()
            bdy_val = np.ascontiguousarray(bdy_val, dtype=np.float64).ravel()
            if len(bdy_set) == 0:
                raise ValueError('graph.peikonal: an empty boundary set')
            if bdy_set.min() < 0 or bdy_set.max() >= n:
                raise ValueError('graph.peikonal: boundary index out of range')
            if not np.all(np.isfinite(bdy_val)):
                raise ValueError('graph.peikonal: bdy_val has a non-finite entry')
            idx.append(bdy_set.astype(np.int32))
            val.append(bdy_val)
            ptr.append(ptr[-1] + len(bdy_set))
        row_ptr = np.concatenate(([0], np.cumsum(np.bincount(I, minlength=n)))).astype(np.int64)
        u, rounds = _hip.peikonal(row_ptr, J, V, f, np.array(ptr, dtype=np.int64), np.concatenate(idx), np.concatenate(val), p, nb, u0,
                                  device=device, max_rounds=max_rounds)
        self.peikonal_rounds = rounds
        return u

    def peikonal(self, bdy_set, bdy_val=0, f=1, p=1, nl_bdy=False, u0=None, solver='fmm', max_num_it=1e5, tol=1e-3, num_bisection_it=30,
                 prog=False, device=None):
        """The graph p-eikonal equation sum_j w_ij (u_i - u_j)_+^p = f_i off the boundary, u = bdy_val on it (reference
        graph.py:793-914).  `solver='fmm'`, the reference's fast-marching pass peikonal_fmm_main, runs on the GPU as synchronous
        fixed-point rounds with the same local solves (glx_peikonal; the argument heads csrc/peik_plan.h): for p = 1 the marching
        solver's values bit for bit, for p != 1 to the resolution of the `num_bisection_it` halvings.  A vertex no boundary vertex
        reaches keeps `u0` (0 by default), as in the reference.  `nl_bdy=True` extends the boundary to its graph neighbours by the
        reference's host expressions.  Returns u float64 (n,); sets peikonal_rounds.  max_num_it, tol and prog belong to the
        'gauss-seidel' solver, an in-order sweep that has an exact parallel form -- the level schedule of csrc/lip_plan.h -- but is not
        switched on: NotImplementedError (for p = 1 it converges to the values 'fmm' returns).  Refused with ValueError before any
        device call: `bdy_val` of another length than the boundary set, an empty boundary set, an index out of range, a weight that is
        not finite and positive, an `f` that is negative or not finite, a non-finite `bdy_val` or `u0`, p not finite or <= 0,
        num_bisection_it outside 1 .. 128."""
        from . import utils
        if solver != 'fmm':
            if solver == 'gauss-seidel':
                raise NotImplementedError("graph.peikonal(solver='gauss-seidel') is not switched on: the reference's in-order sweep is a "
                                          "level schedule (csrc/lip_plan.h) that is not wired to this equation; use solver='fmm'")
            raise ValueError("graph.peikonal: unknown solver %r ('fmm' or 'gauss-seidel')" % (solver,))
        n = self.num_nodes
        bdy_set = np.asarray(bdy_set)
        m = int(np.sum(bdy_set)) if bdy_set.dtype == bool else bdy_set.size
        if np.ndim(bdy_val) > 0 and np.size(bdy_val) != m:
            raise ValueError('graph.peikonal: %d boundary values for %d boundary vertices' % (np.size(bdy_val), m))
        bdy_set, bdy_val = utils._boundary_handling(bdy_set, bdy_val)
        if nl_bdy:                           # reference graph.py:891-901, the same scipy expressions
            if len(bdy_set) and (np.min(bdy_set) < 0 or np.max(bdy_set) >= n):
                raise ValueError('graph.peikonal: boundary index out of range')
            D = self.degree_matrix(p=-1)
            bdy_mask = np.zeros(n)
            bdy_mask[bdy_set] = 1
            bdy_dilate = (D * self.weight_matrix * bdy_mask) > 0
            bdy_set = np.where(bdy_dilate)[0]
            bdy_val_all = np.zeros(n)
            bdy_val_all[bdy_mask == 1] = bdy_val
            bdy_val = D * self.weight_matrix * bdy_val_all
            bdy_val = bdy_val[bdy_set]
        u = self._peikonal_batch([bdy_set], [bdy_val], f=f, p=p, u0=u0, num_bisection_it=num_bisection_it, device=device)
        return np.ascontiguousarray(u[:, 0])

    def neighbors(self, i, return_weights=False):
        """Neighbours of vertex i (and the weights of the edges to them), reference graph.py:124-151."""
        N = self.weight_matrix[i, :].nonzero()[1]
        N = N[N != i]
        if return_weights:
            return N, self.weight_matrix[i, N].toarray().flatten()
        return N

    def _in_edges(self):
        """The edges the reference's Dijkstra walks (`sparse.find` in its __ccode_init__, graph.py:72: explicit zeros dropped; the
        loop itself skips j == i), listed by the vertex they ENTER: (in_ptr (n+1,), in_idx = the vertex i each edge leaves, V, 1/V),
        and the same edges by the vertex they LEAVE (out_ptr, out_idx: the device marks along them which values a lowered value
        can still lower).  Built once per graph object, like the arrays of __ccode_init__.  Unlike the reference's `K`
        (graph.py:75-76) the pointers are right when a vertex has no entry."""
        if getattr(self, '_sssp_edges', None) is None:
            n = self.num_nodes
            Wc = self.weight_matrix.tocsc(copy=True)
            Wc.sum_duplicates()
            col = np.repeat(np.arange(n, dtype=np.int32), np.diff(Wc.indptr))
            keep = (Wc.data != 0) & (Wc.indices != col)
            V = np.ascontiguousarray(Wc.data[keep], dtype=np.float64)
            if not np.all(V >= 0):
                raise ValueError('graph.dijkstra: the weight matrix has a negative or NaN entry')
            in_ptr = np.concatenate(([0], np.cumsum(np.bincount(col[keep], minlength=n)))).astype(np.int64)
            with np.errstate(divide='ignore'):
                Vinv = 1 / V
            Wr = self.weight_matrix.copy()
            Wr.sum_duplicates()
            row = np.repeat(np.arange(n, dtype=np.int32), np.diff(Wr.indptr))
            keep_r = (Wr.data != 0) & (Wr.indices != row)
            out_ptr = np.concatenate(([0], np.cumsum(np.bincount(row[keep_r], minlength=n)))).astype(np.int64)
            self._sssp_edges = (in_ptr, np.ascontiguousarray(Wc.indices[keep], dtype=np.int32), V, Vinv, out_ptr,
                                np.ascontiguousarray(Wr.indices[keep_r], dtype=np.int32))
        return self._sssp_edges

    def _dijkstra_batch(self, problems, f=1, max_dist=np.inf, return_cp=False, reciprocal_weights=False, hopf_lax=False, device=None):
        """B shortest-path problems on this graph in one device call (glx_sssp): `problems` is a list of (bdy_set, bdy_val) in the
        standard form.  Returns dist (n, B) float64, cp (n, B) int32 or None; every column equals the single call bit for bit."""
        from . import _hip
        n = self.num_nodes
        f_scalar = None
        if type(f) != np.ndarray:           # the reference's `f = np.ones((n,))*f`: every vertex holds fl(1.0 * f) = float64(f)
            f_scalar = np.float64(f)
            f = np.reshape(f_scalar, (1,))
        else:
            f = np.ascontiguousarray(f, dtype=np.float64)
            if f.shape != (n,):
                raise ValueError('graph.dijkstra: f has shape %s, expected (%d,)' % (f.shape, n))
        if not np.all(f >= 0):
            raise ValueError('graph.dijkstra: f has a negative or NaN entry')
        max_dist = float(max_dist)
        if max_dist != max_dist:
            raise ValueError('graph.dijkstra: max_dist is NaN')
        src_ptr, src_idx, src_val = [0], [], []
        for bdy_set, bdy_val in problems:
            bdy_set = np.ascontiguousarray(bdy_set, dtype=np.int64).ravel()
            bdy_val = np.ascontiguousarray(bdy_val, dtype=np.float64).ravel()
            if len(bdy_set) != len(bdy_val):
                raise ValueError('graph.dijkstra: %d boundary values for %d boundary vertices' % (len(bdy_val), len(bdy_set)))
            if len(bdy_set) and (bdy_set.min() < 0 or bdy_set.max() >= n):
                raise ValueError('graph.dijkstra: boundary index out of range')
            if len(np.unique(bdy_set)) != len(bdy_set):
                raise ValueError('graph.dijkstra: bdy_set lists a vertex twice (the reference\'s heap does not survive that)')
            if not np.all(bdy_val >= 0):
                raise ValueError('graph.dijkstra: bdy_val has a negative or NaN entry')
            src_idx.append(bdy_set.astype(np.int32))
            src_val.append(bdy_val)
            src_ptr.append(src_ptr[-1] + len(bdy_set))
        in_ptr, in_idx, V, Vinv, out_ptr, out_idx = self._in_edges()
        # c_ij = W[i,j] * f[i]: f at the vertex the edge leaves (hjsolvers.cpp:210); a constant f needs no gather, and w * 1.0 is w
        Vx = Vinv if reciprocal_weights else V
        cost = Vx * f[in_idx] if f_scalar is None else (Vx if f_scalar == 1 else Vx * f_scalar)
        dist, cp, rounds = _hip.sssp(in_ptr, in_idx, cost, np.array(src_ptr, dtype=np.int64),
                                     np.concatenate(src_idx) if src_idx else np.zeros(0, dtype=np.int32),
                                     np.concatenate(src_val) if src_val else np.zeros(0), max_dist=max_dist, hopf_lax=hopf_lax,
                                     return_cp=return_cp, device=device, out_ptr=out_ptr, out_idx=out_idx)
        self.dijkstra_rounds = rounds
        return dist, cp

    def _dijkstra_one(self, bdy_set, bdy_val, f, max_dist, return_cp, reciprocal_weights, hopf_lax, device):
        from . import utils
        bdy_set, bdy_val = utils._boundary_handling(bdy_set, bdy_val)
        dist, cp = self._dijkstra_batch([(bdy_set, bdy_val)], f=f, max_dist=max_dist, return_cp=return_cp,
                                        reciprocal_weights=reciprocal_weights, hopf_lax=hopf_lax, device=device)
        if return_cp:
            return np.ascontiguousarray(dist[:, 0]), np.ascontiguousarray(cp[:, 0])
        return np.ascontiguousarray(dist[:, 0])

    def dijkstra(self, bdy_set, bdy_val=0, f=1, max_dist=np.inf, return_cp=False, reciprocal_weights=False, device=None):
        """Distance function u(x) = min over boundary vertices i of g_i + d(x_i, x), d the cheapest path with edge costs
        w_ij f_i (1/w_ij with `reciprocal_weights`), and optionally the closest boundary vertex (reference graph.py:1077-1175,
        dijkstra_main of its C extension).  Runs on the GPU as label-correcting rounds whose fixed point is the heap's result
        bit for bit (glx_sssp; the argument heads csrc/sssp.hip).  Returns dist_func float64 (n,), and cp int32 (n,) with
        `return_cp`.  Where the reference's documentation and code differ this follows the documentation: vertices farther
        than `max_dist` hold inf and cp -1.  Where several boundary vertices tie for closest, cp is the smallest index among
        them (the reference's choice depends on its heap's history).  Refused with ValueError: a vertex listed twice in
        `bdy_set`; a negative or NaN `f`, `bdy_val` or weight."""
        return self._dijkstra_one(bdy_set, bdy_val, f, max_dist, return_cp, reciprocal_weights, False, device)

    def dijkstra_hl(self, bdy_set, bdy_val=0, f=1, max_dist=np.inf, return_cp=False, device=None):
        """Dijkstra's algorithm with the Hopf-Lax relaxation u_j = (c + sqrt(c^2 + 4 u_i^2)) / 2, c = w_ij f_i (reference
        graph.py:916-997, dijkstra_hl_main), on the GPU; conventions as in `dijkstra`."""
        return self._dijkstra_one(bdy_set, bdy_val, f, max_dist, return_cp, False, True, device)

    def distance(self, i, j, return_path=False, return_distance_vector=False):
        """Shortest-path distance between vertices i and j with edge costs 1/w, optionally a shortest path (from j back to i) and the
        distance vector to i (reference graph.py:999-1046; the path walk is the reference's host loop)."""
        v = self.dijkstra([i], reciprocal_weights=True)
        d = v[j]
        if return_path:
            if not np.isfinite(d):
                raise ValueError('graph.distance: no path from %d to %d' % (i, j))
            p = j
            path = [p]
            while p != i:
                nn, w = self.neighbors(p, return_weights=True)
                k = np.argmin(v[nn] + w ** -1)
                p = nn[k]
                path += [p]
            path = np.array(path)
            if return_distance_vector:
                return d, path, v
            return d, path
        if return_distance_vector:
            return d, v
        return d

    def distance_matrix(self, centered=False):
        """All-pairs shortest-path distances with edge costs 1/w (reference graph.py:1048-1075: n calls of `distance`); here the
        sources ride as the columns of a few batched device calls, every row equal to the single call bit for bit."""
        n = self.num_nodes
        T = np.zeros((n, n))
        batch = max(1, min(n, _DISTANCE_MATRIX_VALUES // n))
        zero = np.zeros(1)
        for lo in range(0, n, batch):
            hi = min(n, lo + batch)
            dist, _ = self._dijkstra_batch([(np.array([s]), zero) for s in range(lo, hi)], reciprocal_weights=True)
            T[lo:hi, :] = dist.T
        if centered:
            J = np.eye(n) - (1 / n) * np.ones((n, n))
            T = -0.5 * J @ T @ J
        return T

    def subgraph(self, ind):
        W = self.weight_matrix
        return graph(W[ind, :][:, ind])

    def isconnected(self):
        """On the host (scipy), so it works without a GPU; `connected_components()[0] == 1` is the same answer from the device."""
        from scipy.sparse import csgraph
        return csgraph.connected_components(self.weight_matrix)[0] == 1

    def connected_components(self, device=None):
        """(ncomp, labels int32 (n,)): the connected components of the weight matrix's pattern, found on the GPU (csrc/cc.hip; DESIGN.md
        4.16).  Every stored entry joins its two vertices whatever its direction and value, so the result equals
        `scipy.sparse.csgraph.connected_components(W, directed=False)` -- and the default weak form `isconnected` uses -- on every
        vertex: components are numbered by their smallest vertex.  There is no strong connectivity.  The matrix is taken as
        `W.tocsr()` yields it (unsorted rows, duplicates and stored zeros included)."""
        from . import _hip
        W = self.weight_matrix.tocsr()
        if W.ndim != 2 or W.shape[0] != W.shape[1] or W.shape[0] < 1:
            raise ValueError('connected_components needs a square weight matrix, got shape %s' % (W.shape,))
        indptr = _hip.int32_index_array(W.indptr, 'the weight matrix: indptr')
        indices = _hip.int32_index_array(W.indices, 'the weight matrix: indices')
        return _hip.components(indptr, indices, W.shape[0], device=device)

    def largest_connected_component(self, device=None):
        """(G, ind) as the reference returns them (graph.py:553-582): the graph restricted to its largest connected component and the
        bool mask of that component's vertices; among components of equal size the first one (the one with the smallest vertex) wins.
        The components come from the GPU; the restriction `W[ind, :][:, ind]` is the reference's own scipy expression on the host."""
        ncomp, labels = self.connected_components(device=device)
        ind = labels == np.argmax(np.bincount(labels, minlength=ncomp))
        A = self.weight_matrix[ind, :]
        A = A[:, ind]
        return graph(A), ind


# the reference exposes the class as `graphlearning.graph` (its __init__ rebinds the name of this
# module to the class); `gl.graph.graph(W)` -- the module-style spelling -- keeps working too
graph.graph = graph
