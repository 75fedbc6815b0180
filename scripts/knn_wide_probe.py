"""Stage times of the wide kNN search (k > 60, self included) next to the k <= 60 plans: device time per stage (knn_stats: filter
incl. set-up, re-rank, fallback) and wall time of KnnResult at config 2 (70 000 x 20 blobs) for k in {11, 60, 61, 101, 256, 1024},
the same at 10^6 x 64 blobs with k = 101, and the host cKDTree at 70 000 x 20, k = 101 (all rows queried), for comparison.
Usage: python scripts/knn_wide_probe.py [--out profiles/knn_wide_k.txt] [--reps 5] [--ks 11,60,...] [--no-big] [--no-host]
                                        [--lists long] [--root DIR] [--label TEXT] [--append]
--lists long: the plan override knn_options(lists='long') (the fp32 filter's lists of 64); --root: search with the package of
another checkout (e.g. the parent commit's, built there), whose knn_stats may lack the wide plan's fields; --label: line prefix;
--append: add to --out instead of replacing it.  profiles/knn_wide_k.txt is three runs into one file:
  python scripts/knn_wide_probe.py --reps 7
  python scripts/knn_wide_probe.py --reps 7 --ks 11,60 --no-big --no-host --root PARENT --label 'parent ' --append
  python scripts/knn_wide_probe.py --reps 7 --ks 512,1024 --no-big --no-host --lists long --label 'long lists ' --append"""
import argparse
import hashlib
import os
import sys
import time
import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join('profiles', 'knn_wide_k.txt'))
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--ks', default='11,60,61,101,256,1024')
ap.add_argument('--no-big', action='store_true')
ap.add_argument('--no-host', action='store_true')
ap.add_argument('--lists', default=None, choices=[None, 'short', 'long'])
ap.add_argument('--root', default=HERE)
ap.add_argument('--label', default='')
ap.add_argument('--append', action='store_true')
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
import bench  # noqa: E402
from graphlearning_amd import _hip  # noqa: E402


def run(X, k, reps):
    rows = []
    for r in range(reps):
        t0 = time.perf_counter()
        res = _hip.KnnResult(X, k, want_order=True)
        wall = (time.perf_counter() - t0) * 1e3
        st = _hip.knn_stats()
        if r == 0:
            J, _ = res.lists()
            sha = hashlib.sha256(np.ascontiguousarray(J).tobytes()).hexdigest()[:12]
        res.close()
        rows.append((st['tile_ms'], st['rerank_ms'], st['fallback_ms'], st['total_ms'], wall))
    best = np.min(np.array(rows), axis=0)
    med = np.median(np.array(rows), axis=0)
    return best, med, st, sha


def line(name, k, best, med, st, sha):
    return ('%-22s k=%-5d filter %7.3f  re-rank %7.3f  fallback %7.3f  kernels %7.3f ms (min)  | kernels %7.3f  wall %8.2f ms (median) | '
            '%s KP=%d nsplit=%d cand=%s chunks=%s wide=%s fallback_rows=%d escalated=%d lists %s'
            % (name, k, best[0], best[1], best[2], best[3], med[3], med[4], st['filter'], st['KP'], st['nsplit'], st.get('candidates', '-'),
               st.get('chunks', '-'), st.get('wide', '-'), st['fallback_rows'], st['escalated_rows'], sha))


def main():
    _hip.require_device()
    if a.lists:
        opts = _hip.knn_options(lists=a.lists)
        opts.__enter__()                 # (for the whole run: the options are the calling thread's)
    out = []

    def emit(s):
        print(s, flush=True)
        out.append(s)
    emit('# kNN search by k (self included): device ms per stage from knn_stats, min over %d searches; wall = KnnResult(X, k, want_order=True)'
         '; package of %s%s' % (a.reps, 'this checkout' if os.path.samefile(a.root, HERE) else 'the checkout given by --root',
                                  '; knn_options(lists=%r)' % a.lists if a.lists else ''))
    labels = bench.load_labels(70000)
    X = bench.make_features(labels)
    for k in [int(v) for v in a.ks.split(',') if v]:
        _hip.KnnResult(X, k, want_order=True).close()          # (first use of the plan: code objects, pools)
        emit(line(a.label + 'config2 70000x20', k, *run(X, k, a.reps)))
    if not a.no_big:
        rng = np.random.default_rng(2)
        lab = rng.integers(0, 10, size=1000000)
        Xb = rng.normal(size=(10, 64))[lab] * 4.0 + rng.normal(size=(1000000, 64))
        _hip.KnnResult(Xb[:200000], 101).close()
        emit(line(a.label + 'blobs 1000000x64', 101, *run(Xb, 101, max(2, a.reps // 2))))
        del Xb
    if not a.no_host:
        from scipy import spatial
        t0 = time.perf_counter()
        tree = spatial.cKDTree(X)
        t_tree = time.perf_counter() - t0
        t0 = time.perf_counter()
        tree.query(X, k=101, workers=16)
        t_q = time.perf_counter() - t0
        emit('host cKDTree 70000x20 k=101: tree %.3f s, query of all 70000 rows %.3f s (16 workers), %.3f s in all' % (t_tree, t_q, t_tree + t_q))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a' if a.append else 'w') as f:
        f.write('\n'.join(out) + '\n')


if __name__ == '__main__':
    main()
