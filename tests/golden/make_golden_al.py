#!/usr/bin/env python3
"""Generate the active-learning fixture tests/golden/g23_al.npz from THE REFERENCE.

Run where the reference is importable (it never travels to the GPU box):

    PYTHONPATH=<the reference's checkout> PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg \
        python3 tests/golden/make_golden_al.py        (from the repository root)

Graphs and eigenpairs are read from the fixtures that hold them and not stored again: `blobs` (600) from g18_ck.npz, `moons` (500) and
the reference's eigen_decomp('normalized', k=50) of both from g19_eig.npz.  The cases are al_ref.GOLDEN_CASES: per graph the four
criteria at two conditionings of C -- the documented diag(1 / (evals + 1e-11)) and diag(1 / (evals + 1e-2)) --, one case with
batch_size=5, one with a candidate subset, one with policy='prop'.  Each runs the reference's active_learner with ssl.laplace for ten
rounds of select_queries(return_acq_vals=True) / update from one labelled vertex per class.

The file holds recorded results (data only).  Per case c: what the reference's first update computed, C v (`case_<c>_init_w`, one row
per labelled vertex) and v.C v (`_init_ip`); per round r the query (`_r<r>_query`), C v and v.C v of every query in order (`_r<r>_w`,
`_r<r>_ip`) -- from these al_ref.reference_C rebuilds the reference's C after every update bit for bit, by elementwise numpy alone,
which is asserted here against the reference's own matrix: 51 numbers per query stand for 2 500 --; the best six values with their
positions among the candidates and the rows of u at those vertices (`_r<r>_top_pos`, `_top_val`, `_top_u`); in the rounds
al_ref.FULL_ROUNDS the whole value vector and, for the criteria that read it, the whole u (`_r<r>_vals`, `_r<r>_u`): every round of
every case would be 6 MB, and no committed file may exceed 1 MiB.  The candidates are the unlabelled vertices in ascending order, or
the stored subset (`_subset`).  The 'prop' case stores numpy's global state before every draw (`_r<r>_key`, `_pos`, `_has_gauss`,
`_cached_gaussian`).  `unc_<method>`: the reference's unc_sampling in its six methods on the u of al_ref.UNC_CASE, round 0, at
al_ref.unc_candidates.  `full_u`, `full_<criterion>_vals0`, `_vals1`, `full_C`: the four criteria with full storage on al_ref.full_C
(40 vertices) at all vertices, before and after update(al_ref.FULL_QUERIES), and the covariance after it.

`bound_vals_<conditioning>` and `bound_C_<conditioning>`: 16 times the largest difference, over all rounds and cases of that
conditioning, between the reference and csrc/acq_plan.h run on the host with its own C from the same start (values relative to the
round's largest value, C relative to its largest entry).  The factor covers a host whose BLAS orders its sums differently.

Asserted before anything is written: in every round of the 'max' cases the relative gap between the best two values -- all gaps among
the best six at batch_size=5 -- is at least 8 times bound_vals; acq_plan.h and the package's own selection expressions reproduce the
reference's query in every round, the 'prop' draws included; the file stays below 1 MiB.  A case that fails is replaced by another
seed in al_ref.GOLDEN_CASES, not waived."""
import os
import sys
import tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.append(os.path.dirname(os.path.dirname(HERE)))      # graphlearning_amd, behind the reference

import graphlearning as gl                      # the REFERENCE (first on PYTHONPATH)
import al_ref as ref
from graphlearning_amd import active_learning as amd_al

assert 'graphlearning_amd' not in gl.__file__ and hasattr(gl, 'active_learning'), gl.__file__
LIMIT = 1 << 20


def steps_of(C, V, queries, gamma2):
    """C v and v.C v of every query in order, by the reference's expressions (active_learning.py:312-315)"""
    C = C.copy()
    ws, ips = [], []
    for k in queries:
        vk = V[k]
        Cavk = C @ vk
        ip = np.inner(vk, Cavk)
        C -= np.outer(Cavk, Cavk) / (gamma2 + ip)
        ws.append(Cavk)
        ips.append(ip)
    return np.array(ws), np.array(ips), C


def main():
    gold = ref.eig_ref.load_golden()
    lib = ref.build_host_lib(tempfile.mkdtemp())
    out = {}
    worst = {c: dict(vals=0.0, C=0.0, gap=np.inf) for c in ref.CONDITIONINGS}
    for name, case in ref.GOLDEN_CASES.items():
        W, truth, V, C0, ind, labels, subset = ref.case_state(gold, name)
        kind, key = ref.KINDS[case['acq']], 'case_%s_' % name
        uses_unc = kind >= ref.MC
        model = gl.ssl.laplace(W)
        AL = gl.active_learning.active_learner(model, getattr(gl.active_learning, case['acq']), ind, labels, case['policy'], C=C0.copy(), V=V.copy())
        assert AL.acq_function.gamma2 == ref.GAMMA2
        ws, ips, Cr = steps_of(C0, V, ind, ref.GAMMA2)
        assert ref.same_bits(Cr, AL.acq_function.C) and ref.same_bits(ref.reference_C(C0, ws, ips), Cr)
        out[key + 'init_w'], out[key + 'init_ip'] = ws, ips
        Cp = ref.host_update(lib, V, C0, ind)                                  # the plan's own C
        unc_fn = amd_al.unc_sampling()
        if subset is not None:
            out[key + 'subset'] = subset
        w = worst[case['cond']]
        for r in range(ref.ROUNDS):
            u = AL.u.copy()
            cand = subset if subset is not None else AL.unlabeled_ind.copy()
            state = np.random.get_state()
            query, vals = AL.select_queries(case['batch'], candidate_ind=('full' if subset is None else subset), return_acq_vals=True)
            query = np.atleast_1d(query)
            unc = unc_fn.compute(u, cand) if uses_unc else None
            pvals = ref.host_compute(lib, V, Cp, kind, cand, unc)
            w['vals'] = max(w['vals'], ref.rel_diff(pvals, vals))
            if case['policy'] == 'max':
                assert np.array_equal(cand[(-pvals).argsort()[:case['batch']]], query), (name, r)
                w['gap'] = min(w['gap'], float(ref.top_gaps(vals, 5 if case['batch'] > 1 else 1).min()))
            else:
                np.random.set_state(state)
                probs = np.exp(1.0 * (pvals - pvals.max()))
                probs /= probs.sum()
                assert np.array_equal(np.random.choice(cand, case['batch'], p=probs), query), (name, r)
                out[key + 'r%d_key' % r], out[key + 'r%d_pos' % r] = np.asarray(state[1], dtype=np.uint32), np.int64(state[2])
                out[key + 'r%d_has_gauss' % r], out[key + 'r%d_cached_gaussian' % r] = np.int64(state[3]), np.float64(state[4])
            before = AL.acq_function.C.copy()
            ws, ips, Cr = steps_of(before, V, query, ref.GAMMA2)
            AL.update(query, truth[query])
            assert ref.same_bits(Cr, AL.acq_function.C) and ref.same_bits(ref.reference_C(before, ws, ips), Cr), (name, r)
            Cp = ref.host_update(lib, V, Cp, query)
            w['C'] = max(w['C'], ref.rel_diff(Cp, Cr))
            top = np.argsort(-vals, kind='stable')[:ref.TOP]
            out[key + 'r%d_query' % r], out[key + 'r%d_w' % r], out[key + 'r%d_ip' % r] = query.astype(np.int64), ws, ips
            out[key + 'r%d_top_pos' % r], out[key + 'r%d_top_val' % r] = top.astype(np.int64), vals[top]
            if uses_unc:
                out[key + 'r%d_top_u' % r] = u[cand[top]]
            if r in ref.FULL_ROUNDS:
                out[key + 'r%d_vals' % r] = vals
                if uses_unc:
                    out[key + 'r%d_u' % r] = u
        print(name, 'labelled', len(AL.labeled_ind), 'worst so far', w)
    # unc_sampling, all six methods, on a recorded u; the full-storage forms on a dense C that elementwise arithmetic defines
    u = out['case_%s_r0_u' % ref.UNC_CASE]
    for method in ref.UNC_METHODS:
        out['unc_' + method] = gl.active_learning.unc_sampling(unc_method=method).compute(u, ref.unc_candidates(len(u)))
    n = ref.FULL_N
    full_u = np.random.default_rng(11).random((n, 3))
    out['full_u'] = full_u
    every = np.arange(n)
    for acq in ref.KINDS:
        f = getattr(gl.active_learning, acq)(C=ref.full_C(n))
        assert f.storage == 'full' and f.gamma2 == ref.GAMMA2
        out['full_%s_vals0' % acq] = f.compute(full_u, every)          # (all vertices: the reference's model_change takes nothing else)
        f.update(ref.FULL_QUERIES, None)
        out['full_%s_vals1' % acq] = f.compute(full_u, every)
        if 'full_C' in out:
            assert ref.same_bits(out['full_C'], f.C)
        out['full_C'] = f.C.copy()
    for c, w in worst.items():
        out['bound_vals_' + c], out['bound_C_' + c] = np.float64(16 * w['vals']), np.float64(16 * w['C'])
        out['min_gap_' + c] = np.float64(w['gap'])
        print(c, 'values differ by up to', w['vals'], 'C by up to', w['C'], 'smallest deciding gap', w['gap'], 'margin over 8 x bound',
              w['gap'] / (8 * 16 * w['vals']))
        assert w['gap'] >= 8 * 16 * w['vals'], (c, w)
    path = os.path.join(HERE, ref.GOLDEN_FILE)
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < LIMIT, os.path.getsize(path)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
