#!/usr/bin/env python3
"""Generate the boundary-statistic golden fixture tests/golden/g25_boundary.npz by IMPORTING THE REFERENCE.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONPATH=<the reference's checkout> PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg \
        python3 tests/golden/make_golden_boundary.py        (from the repository root)

Captured with Python 3.10.12, numpy 2.2.6, scipy 1.15.3, reference graphlearning 1.7.5.  The file holds inputs and the reference's
outputs (data only): per case of tests/boundary_cases.py GOLDEN the points X, the radius or k, in the kNN mode the lists J and D of
the reference's knnsearch(method='kdtree') handed to it as knn_data, and T and nu of utils.boundary_statistic for the three order
settings (first order, second order with and without cutoff).

Conditions asserted on every stored case (on the cases, not on any code under test): no isolated vertex, every norm above 0 (the
reference returns no NaN), no pair within 1e-12 relative of the radius; radius cases: a full row in each, two or more in at least one,
no tie for the farthest entry of a full row; kNN cases: no index twice in a list.  The restatement tests/boundary_ref.py is
cross-checked on the way: nu bit for bit, T equal as numbers, in both of its forms."""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import graphlearning as gl                      # the REFERENCE (PYTHONPATH=/root/reference)
import boundary_ref as ref                      # the restatement, cross-checked below
import boundary_cases as cases
import epsball_ref

assert gl.__file__.startswith('/root/reference'), gl.__file__

TAGS = {(False, True): 'o1', (True, True): 'o2c', (True, False): 'o2'}


def main():
    out = {}
    most_full = 0
    for name, (mode, n, d, r, seed) in cases.GOLDEN.items():
        X = cases.golden_points(name)
        assert X.shape == (n, d)
        out[name + '_X'] = X
        out[name + '_r'] = np.float64(r)
        if mode == 'knn':
            J, D = gl.weightmatrix.knnsearch(X, r, method='kdtree')
            assert np.array_equal(J, ref.knn_lists(X, r)[0])
            Js = np.sort(J, axis=1)
            assert not (Js[:, 1:] == Js[:, :-1]).any(), name
            indptr, indices = ref.knn_pattern(J, r)
            out[name + '_J'], out[name + '_D'] = J.astype(np.int32), D
            knn_data = (J, D)
        else:
            assert not epsball_ref.near_boundary(X, r), name
            indptr, indices = ref.ball_pattern(X, r)
            W = gl.weightmatrix.epsilon_ball(X, r, kernel='uniform').tocsr()
            W.sort_indices()
            assert np.array_equal(W.indptr, indptr) and np.array_equal(W.indices, indices) and (W.data == 1).all(), name
            J, knn_data = None, None
            lens = np.diff(indptr)
            full = np.flatnonzero(lens == lens.max())
            assert len(full) >= 1
            most_full = max(most_full, len(full))
            for i in full:
                sq = epsball_ref.d2_tree(X[i], X[indices[indptr[i]:indptr[i + 1]]])
                assert (sq == sq.max()).sum() == 1, (name, i)
        assert np.diff(indptr).min() >= 1, name
        for (second, cutoff), tag in TAGS.items():
            T, nu = gl.utils.boundary_statistic(X, r, knn=mode == 'knn', return_normals=True, second_order=second, cutoff=cutoff,
                                                knn_data=knn_data)
            assert np.isfinite(T).all() and np.isfinite(nu).all(), (name, tag)
            for form in (ref.statistic_rows, ref.statistic):
                T2, nu2 = form(X, indptr, indices, J=None if J is None else J.astype(np.int32), second_order=second, cutoff=cutoff)
                assert nu2.tobytes() == nu.tobytes(), (name, tag, form.__name__)
                assert np.array_equal(T2, T), (name, tag, form.__name__)
                assert not np.signbit(T2[T2 == 0]).any()
                if mode == 'knn':
                    assert T2.tobytes() == T.tobytes(), (name, tag, form.__name__)
            out['%s_T_%s' % (name, tag)] = T
            out['%s_nu_%s' % (name, tag)] = nu
            if name == 'r_edge':        # a row of maxdeg - 1 entries with a negative maximum, in every order setting: no 0 was added
                edge = np.flatnonzero(np.diff(indptr) == np.diff(indptr).max() - 1)
                assert (T[edge] < 0).any(), (name, tag)
                assert (np.diff(indptr) < np.diff(indptr).max() - 1).any()
            if mode == 'knn' and tag == 'o2c':
                # lists wider than k: weightmatrix.knn counts self on top and takes the first k + 1 columns, the maximum runs over all
                Jw, Dw = gl.weightmatrix.knnsearch(X, r + 5, method='kdtree')
                Tw, nuw = gl.utils.boundary_statistic(X, r, knn=True, return_normals=True, knn_data=(Jw, Dw))
                Tw2, nuw2 = ref.statistic(X, *ref.knn_pattern(Jw, r + 1), J=Jw.astype(np.int32))
                assert nuw2.tobytes() == nuw.tobytes() and np.array_equal(Tw2, Tw), name
                out[name + '_Twide'] = Tw
        print('%-6s n=%d d=%d r=%g degrees %d..%d' % (name, n, d, r, np.diff(indptr).min(), np.diff(indptr).max()))
    assert most_full >= 2, most_full
    out['case_names'] = np.array(sorted(cases.GOLDEN))
    path = os.path.join(HERE, 'g25_boundary.npz')
    np.savez_compressed(path, **out)
    print('g25_boundary.npz', os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) <= 1000000


if __name__ == '__main__':
    main()
