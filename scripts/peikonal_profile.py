"""graph.peikonal / ssl.peikonal on the headline graph: device time and rounds for one problem and for all classes in one call.

The 70 000-vertex k = 10, 10-class graph of the headline configuration (bench.py's generator), 10 labels per class; p = 1 and
p = 2 (30 halvings); warm, median of the repeats, end to end (entry arrays, uploads and the download included), with the library's
own host milliseconds per phase.  --save PATH writes the graph and the training set as .npz, so that the compiled reference can be
timed on the same problem where it is available (the reference is not on the GPU machine; profiles/peikonal.txt says where its
figures come from).

    python scripts/peikonal_profile.py [--out profiles/peikonal.txt] [--save graph.npz]"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'peikonal.txt'))
ap.add_argument('--save', default=None)
a = ap.parse_args()


def timed(fn, min_s=1.0, min_n=3, max_n=25):
    out, ts = None, []
    t_begin = time.perf_counter()
    while (time.perf_counter() - t_begin < min_s or len(ts) < min_n) and len(ts) < max_n:
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


def main():
    import graphlearning_amd as gl
    from graphlearning_amd import _hip
    from bench import load_labels, make_features
    _hip.require_device()
    labels = load_labels(70000)
    W = gl.weightmatrix.knn(make_features(labels), 10)
    train_ind = gl.trainsets.generate(labels, rate=10, seed=0)
    G = gl.graph(W)
    classes = np.unique(labels[train_ind])
    lines = ['# graph.peikonal / ssl.peikonal on one MI355X; ms = end to end, median of the warm repeats (min .. max); phases = host ms '
             'inside the library (uploads | rounds | download)',
             'headline graph: n=%d entries=%d classes=%d labelled=%d' % (W.shape[0], W.nnz, len(classes), len(train_ind))]
    if a.save:
        np.savez_compressed(a.save, indptr=W.indptr, indices=W.indices, data=W.data, train_ind=train_ind, labels=labels)
    for p in (1, 2):
        one = train_ind[labels[train_ind] == classes[0]]
        G.peikonal(one, p=p)                                       # warm-up: entry arrays, code objects, pools
        u, ts = timed(lambda: G.peikonal(one, p=p))
        lines.append('p=%d one problem (%d boundary vertices): %8.1f ms (median of %d, %.1f .. %.1f) | rounds %d | phases %s | max u %.6g' % (
            p, len(one), float(np.median(ts)), len(ts), min(ts), max(ts), G.peikonal_rounds,
            ' | '.join('%.1f' % v for v in _hip.peikonal_last_ms), u.max()))
        print(lines[-1], flush=True)
        model = gl.ssl.peikonal(G, p=p)
        model.fit(train_ind, labels[train_ind])
        prob, ts = timed(lambda: np.array(model.fit(train_ind, labels[train_ind]), copy=True))
        reached = float(np.mean(prob != 0))                          # a vertex no labelled vertex of the class reaches keeps u0 = 0
        lines.append('p=%d %d classes in one call:            %8.1f ms (median of %d, %.1f .. %.1f) | rounds %d | phases %s | share of nonzero values %.3f' % (
            p, len(classes), float(np.median(ts)), len(ts), min(ts), max(ts), model.num_iter,
            ' | '.join('%.1f' % v for v in _hip.peikonal_last_ms), reached))
        print(lines[-1], flush=True)
        if a.save:
            np.save(a.save[:-4] + '_prob_p%d.npy' % p, prob)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
