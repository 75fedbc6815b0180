"""The Gaussian weights of weightmatrix.knn in its DEFAULT mode (exp correctly rounded, on the device) against the host-exp mode
(numpy's exp: this host's reference) at configs 2 and 3: how many weights differ and by how much, and what that does downstream
-- sweep count T, CG iteration counts, predicted labels, iterates.  The histogram is printed (and kept in
profiles/r04_weights_ulp_histogram.txt from the run on the MI355X box)."""
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu


def _ulps(a, b):
    return np.abs(a.view(np.int64) - b.view(np.int64))


def _both(gl, X, k, **kw):
    old = os.environ.pop('GLX_HOST_EXP', None)
    try:
        Wd = gl.weightmatrix.knn(X, k, **kw)
        os.environ['GLX_HOST_EXP'] = '1'
        Wh = gl.weightmatrix.knn(X, k, **kw)
    finally:
        if old is None:
            os.environ.pop('GLX_HOST_EXP', None)
        else:
            os.environ['GLX_HOST_EXP'] = old
    assert np.array_equal(Wd.indptr, Wh.indptr) and np.array_equal(Wd.indices, Wh.indices)
    return Wd, Wh


def _report(tag, Wd, Wh):
    u = _ulps(Wd.data, Wh.data)
    hist = np.bincount(np.minimum(u, 3), minlength=4)
    print('%s: %d stored weights; ulp distance device (correctly rounded) vs host numpy exp: 0: %d  1: %d  2: %d  >2: %d  (%.2f %% differ)'
          % (tag, len(u), hist[0], hist[1], hist[2], hist[3], 100.0 * (len(u) - hist[0]) / len(u)))
    return hist


def test_config2_device_weights_histogram_and_downstream():
    import bench
    import graphlearning_amd as gl
    labels = bench.load_labels(70000)
    X = bench.make_features(labels)
    Wd, Wh = _both(gl, X, 10)
    hist = _report('config 2 (n=70000, k=10, gaussian, symmetrised)', Wd, Wh)
    # a stored weight is (w_ij + w_ji)/2 of two exponentials: one ulp each at most (numpy's exp is within an ulp; ours is exact)
    assert hist[3] == 0 and hist[2] <= 0.01 * len(Wd.data)
    ti = gl.trainsets.generate(labels, rate=1, seed=0)
    out = {}
    for name, W in (('device', Wd), ('host', Wh)):
        gd = gl.ssl.poisson(W, solver='gradient_descent')
        u = gd.fit(ti, labels[ti])
        cg = gl.ssl.poisson(W)
        cg.fit(ti, labels[ti])
        out[name] = dict(T=gd.num_iter, u=np.array(u), pred=gd.predict(), cg_it=cg.num_iter, cg_pred=cg.predict())
    d, h = out['device'], out['host']
    du = float(np.max(np.abs(d['u'] - h['u'])))
    print('config 2 downstream: T %d / %d, max |u_device - u_host| = %.3e (max |u| %.3e), labels equal %s; Poisson CG iterations %d / %d, CG labels equal %s'
          % (d['T'], h['T'], du, float(np.max(np.abs(h['u']))), bool(np.array_equal(d['pred'], h['pred'])), d['cg_it'], h['cg_it'],
             bool(np.array_equal(d['cg_pred'], h['cg_pred']))))
    assert d['T'] == h['T'] and np.array_equal(d['pred'], h['pred'])
    assert du <= 1e-5 * max(1.0, float(np.max(np.abs(h['u']))))            # the north star's tolerance; measured ~1e-16 relative
    # The default Poisson solver is CG on a SINGULAR system stopped at 1e-3: its iteration count is decided by rounding noise, and a
    # one-ulp change in 5 % of the weights moves it from 140 to several hundred (measured: 462).  Both runs are the reference's
    # algorithm to the letter (each equals the oracle on its own W: bench.py, tests/test_gpu_fullsize.py); which one a host's reference
    # produces depends on that host's libm.  Nothing to assert but that both end.
    assert d['cg_it'] >= 1 and h['cg_it'] >= 1


def test_config3_device_weights_histogram_and_downstream():
    import bench
    import graphlearning_amd as gl
    lab, X = bench.config3_data()
    Wd, Wh = _both(gl, X, 20)
    hist = _report('config 3 (n=60000, k=20, gaussian, symmetrised)', Wd, Wh)
    assert hist[3] == 0 and hist[2] <= 0.01 * len(Wd.data)
    ti = gl.trainsets.generate(lab, rate=10, seed=0)
    res = {}
    for name, W in (('device', Wd), ('host', Wh)):
        m = gl.ssl.laplace(W)
        u = m.fit(ti, lab[ti])
        res[name] = (m.num_iter, np.array(u), m.predict())
    du = float(np.max(np.abs(res['device'][1] - res['host'][1])))
    print('config 3 downstream: Laplace CG iterations %d / %d, max |u_device - u_host| = %.3e, labels equal %s'
          % (res['device'][0], res['host'][0], du, bool(np.array_equal(res['device'][2], res['host'][2]))))
    assert res['device'][0] == res['host'][0] and du <= 1e-5 and np.array_equal(res['device'][2], res['host'][2])


def test_symgaussian_and_unsymmetrised_kernels_within_an_ulp():
    import graphlearning_amd as gl
    rng = np.random.default_rng(4)
    X = rng.normal(size=(5000, 12))
    for kw, most in ((dict(kernel='symgaussian'), 8), (dict(symmetrize=False), 1)):
        # (symgaussian's rule W + W^T*(W^T>W) - W*(W^T>W) subtracts: fl(fl(a+b)-a) carries the one-ulp differences of a and b into
        #  a few ulps of the smaller entry)
        Wd, Wh = _both(gl, X, 12, **kw)
        u = _ulps(Wd.data, Wh.data)
        assert u.max() <= most, kw
        # and the default mode bit for bit: the reference's expressions with a correctly rounded exponential, on the same lists
        from weights_cr_ref import knn_weights_cr, same_matrix
        J, D = gl.weightmatrix.knnsearch(X, 13)
        assert same_matrix(Wd, knn_weights_cr(np.array(J), np.array(D), 12, kw.get('kernel', 'gaussian'), kw.get('symmetrize', True))), kw
