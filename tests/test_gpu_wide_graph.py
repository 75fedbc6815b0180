"""Everything BEHIND the wide search on graphs of 61 .. 1023 neighbours: the assembly's three row-merge paths at their boundaries
(csrc/assemble.hip: registers up to 64 entries, one wavefront in LDS up to ROW_CAP = 1024, one workgroup in a global scratch of a
power-of-two size >= 2048 above), weight matrices of real wide graphs through both entry routes, the operator's row classes on a
ladder of exact row lengths, and the learners end to end on graphs whose every row is hundreds to thousands of entries long.
References: oracle.gl_oracle and scipy's CSR product; bit for bit in the GLX_HOST_EXP=1 mode of conftest.py unless a test says
otherwise.  M below is what the assembly merges for a row: its k list entries plus the entries of all lists that name it (its own
self entry included) -- every census is asserted from the lists themselves, so a change of the construction, of ROW_CAP or of the
2048 floor shows here."""
import numpy as np
import pytest
from scipy import sparse
from scipy.sparse import csgraph
from conftest import blobs
from test_gpu_fuzz import _virtual_ranks_sweep, _ulps
from weights_cr_ref import knn_weights_cr, same_matrix

pytestmark = pytest.mark.gpu

KERNELS = ['uniform', 'gaussian', 'symgaussian', 'distance', 'singular']
ROW_CAP = 1024           # csrc/assemble_plan.h: the most one wavefront merges in LDS (repeated here on purpose: the censuses below
                         # are counted independently of the header; tests/test_assemble_host.py ties the two together)
HUB_FLOOR = 2048         # the smallest global scratch of a hub row


@pytest.fixture(scope='module')
def gl():
    import graphlearning_amd as gl
    from graphlearning_amd import _hip
    _hip.require_device()
    return gl


@pytest.fixture(scope='module')
def orc():
    from oracle import gl_oracle
    return gl_oracle


def _same(W, Wo, tag, exact=True):
    assert W.shape == Wo.shape, tag
    assert np.array_equal(W.indptr, Wo.indptr) and np.array_equal(W.indices, Wo.indices), tag
    if exact:
        assert np.array_equal(W.data, Wo.data), tag


def _as_float32(A):
    """The float32 matrix with the entries in A's order (astype would sort the columns of an unsorted row, and the entry order
    inside a row is the order of the sum)."""
    A = sparse.csr_matrix(A)
    A32 = sparse.csr_matrix((A.data.astype(np.float32), A.indices, A.indptr), shape=A.shape)
    A32.has_sorted_indices = A.has_sorted_indices
    return A32


def _census(ind, K):
    """M of every row when the lists are symmetrised: K list entries + every occurrence of the row's index in the lists."""
    return K + np.bincount(np.asarray(ind)[:, :K].ravel(), minlength=len(ind))


# ---- 1. assembly at the path boundaries, from constructed lists ------------------------------------------------------------------------

def _circulant(n, K, seed, mutual=False):
    """ind[i, t] = (i + t) % n: every vertex is named by exactly K lists (its own included), M = 2 K in every row, and no edge
    is listed from both ends.  mutual: the offsets 0, +1, -1, +2, -2, ... instead -- the same census, but nearly every edge is
    listed from both ends with two different weights, so every merged column combines a forward and a reverse entry.
    Distances: sorted random rows, first column 0."""
    assert n > 2 * K
    rng = np.random.default_rng(seed)
    t = np.arange(K)
    offsets = np.where(t % 2 == 1, (t + 1) // 2, -(t // 2)) if mutual else t
    ind = (np.arange(n)[:, None] + offsets[None, :]) % n
    dist = np.sort(rng.random((n, K)), axis=1)
    dist[:, 0] = 0
    return ind.astype(np.int64), dist


def _redirect(ind, row, col, to_col):
    """The entry (row, col) names the vertex of (row, to_col) instead: the old target loses one reverse entry, the new one gains
    one, the row lists a neighbour twice."""
    ind[row, col] = ind[row, to_col]


def _eta(t):
    return 1.0 / (1.0 + 3.0 * t)


_RULE_OF = {'gaussian': 'mean', 'uniform': 'max', 'symgaussian': 'symgauss'}


def _given_ref(orc, ind, w, rule):
    """The oracle's assembly (knn_weights: COO -> CSR, its symmetrisation rules, setdiag(0), eliminate_zeros) for weights that
    are handed in: what weightmatrix.knn(eta=...) has to give."""
    n, K = ind.shape
    rows = (np.ones((n, K)) * np.arange(n)[:, None]).flatten()
    W = sparse.coo_matrix((w.flatten(), (rows, ind.flatten())), shape=(n, n)).tocsr()
    if rule == 'max':
        W = orc.sparse_max(W, W.transpose())
    elif rule == 'symgauss':
        W = W + W.T.multiply(W.T > W) - W.multiply(W.T > W)
    elif rule == 'mean':
        W = (W + W.transpose()) / 2
    else:
        assert rule == 'none'
    W.setdiag(0)
    W.eliminate_zeros()
    return W


def _all_kernels_match(gl, orc, ind, dist, tag):
    """Every kernel, symmetrised and not, and given weights under all four symmetrisation rules: identical to the oracle."""
    K = ind.shape[1]
    k = K - 1
    for kernel in KERNELS:
        for symmetrize in (True, False):
            W = gl.weightmatrix.knn(None, k, kernel=kernel, symmetrize=symmetrize, knn_data=(ind, dist.copy()))
            Wo = orc.knn_weights(ind, dist.copy(), k, kernel=kernel, symmetrize=symmetrize)
            _same(W, Wo, (tag, kernel, symmetrize))
    sq = dist * dist
    w = _eta(sq / sq[:, K - 1][:, None])
    for kernel, symmetrize in [('gaussian', True), ('uniform', True), ('symgaussian', True), ('gaussian', False)]:
        W = gl.weightmatrix.knn(None, k, kernel=kernel, eta=_eta, symmetrize=symmetrize, knn_data=(ind, dist.copy()))
        Wo = _given_ref(orc, ind, w, _RULE_OF[kernel] if symmetrize else 'none')
        _same(W, Wo, (tag, 'eta', kernel, symmetrize))


def _boundary_lists(K, n, seed, mutual=False):
    """All rows at M = 2 K, one at 2 K - 1, one at 2 K + 1, one duplicate neighbour."""
    ind, dist = _circulant(n, K, seed, mutual)
    listed = sparse.csr_matrix((np.ones(ind.size), (np.repeat(np.arange(n), K), ind.ravel())), shape=(n, n))
    both = listed.multiply(listed.T).nnz - n                           # edges listed from both ends (self entries aside)
    assert both >= n * (K - 2) if mutual else both == 0
    row, col, to_col = n // 3, K // 2, 3
    lost, gained = int(ind[row, col]), int(ind[row, to_col])
    _redirect(ind, row, col, to_col)
    M = _census(ind, K)
    assert M[lost] == 2 * K - 1 and M[gained] == 2 * K + 1
    assert np.sum(M == 2 * K) == n - 2
    return ind, dist, M


@pytest.mark.parametrize('mutual', [False, True])
def test_rows_at_the_wavefront_cap(gl, orc, mutual):
    """K = 512: every row at M = 1024 = ROW_CAP (the last wavefront row: LDS image full, no padding key), one at 1023, one at 1025 --
    a single hub among wavefront rows under the k > 64 host branch.  (Unsymmetrised, a row merges its K list entries alone.)"""
    ind, dist, M = _boundary_lists(512, 1500, 1, mutual)
    assert sorted(set(M.tolist())) == [ROW_CAP - 1, ROW_CAP, ROW_CAP + 1] and np.sum(M > ROW_CAP) == 1
    _all_kernels_match(gl, orc, ind, dist, 'K=512')


@pytest.mark.parametrize('mutual', [False, True])
def test_rows_at_the_hub_scratch_size(gl, orc, mutual):
    """K = 1024: every row a hub, M = 2048 = its scratch exactly (no padding key), one at 2047, one at 2049 (scratch 4096).
    Unsymmetrised, every row has M = K = 1024 = ROW_CAP: the wavefront kernel's last row again, in all rows."""
    ind, dist, M = _boundary_lists(1024, 2600, 2, mutual)
    assert sorted(set(M.tolist())) == [HUB_FLOOR - 1, HUB_FLOOR, HUB_FLOOR + 1] and np.all(M > ROW_CAP)
    _all_kernels_match(gl, orc, ind, dist, 'K=1024')


@pytest.mark.parametrize('K', [32, 64, 65])
def test_small_and_general_host_branches_with_a_hub(gl, orc, K):
    """The switch between the k <= 64 host branch (register kernel + the list of longer rows) and the general kernel, each with a
    redirect and with one vertex that is everyone's neighbour (a hub).  K = 32 puts every other row at M = 64, the register kernel's
    last row (63 and 65 beside it), before the hub is added."""
    n = 1500
    ind, dist, M = _boundary_lists(K, n, 3 + K)
    if K == 32:
        assert sorted(set(M.tolist())) == [63, 64, 65]
        _all_kernels_match(gl, orc, ind, dist, 'K=32')
    hub = 700
    ind[:, K - 2] = hub                        # everyone's neighbour (rows that listed it already now list it twice)
    M = _census(ind, K)
    assert M[hub] > ROW_CAP and np.sum(M > ROW_CAP) == 1
    if K == 32:
        assert np.sum(M <= 64) == n - 1                # all but the hub: the register kernel's
    else:
        assert np.sum((M > 64) & (M <= ROW_CAP)) == n - 1
    _all_kernels_match(gl, orc, ind, dist, 'K=%d hub' % K)


@pytest.mark.parametrize('K,n', [(512, 1500), (1024, 2600)])
def test_several_redirects_in_one_matrix(gl, orc, K, n):
    """Duplicates far down the lists (positions above 255, and above 1000 at K = 1024: wide reverse positions), a neighbour listed
    three times, a self entry that is not in column 0, a hub that lists another hub twice (K = 1024: every row is one), a second
    self entry (must vanish with the diagonal).
    The three entries of the triple carry the SAME distance.  With three different weights the reference's own sum is not defined:
    scipy's COO -> CSR sorts the columns of a row longer than 16 entries with an unstable sort before it adds duplicates, so the
    order of the three terms is an accident of that sort (measured with three different weights at K = 512, kernel 'singular':
    the oracle holds (w2 + w3) + w1 = 601.8669260628621, the assembly adds in list order, (w1 + w2) + w3 = 601.8669260628623;
    DESIGN.md 4.3).  Two duplicates commute, and so do three equal ones."""
    ind, dist = _circulant(n, K, 40 + K)
    dist[30, 400] = dist[30, K - 30] = dist[30, 2]
    _redirect(ind, 10, 300, 5)
    _redirect(ind, 20, K - 14, K - 19)                              # both beyond 1000 at K = 1024
    _redirect(ind, 30, 400, 2)
    _redirect(ind, 30, K - 30, 2)                                   # three times
    ind[40, 0], ind[40, 7] = ind[40, 7], ind[40, 0]                 # self in column 7, at a distance > 0
    _redirect(ind, 50, K - 3, 0)                                    # a second self entry
    _redirect(ind, 60, 290, 280)
    assert ind[40, 7] == 40 and ind[50, K - 3] == 50 and np.sum(ind[30] == ind[30, 2]) == 3
    if K == 1024:
        assert K - 19 > 1000
    M = _census(ind, K)
    if K == 1024:
        assert np.all(M > ROW_CAP) and np.sum(M > HUB_FLOOR) >= 3 and np.sum(M < HUB_FLOOR) >= 3
    else:
        assert np.sum(M > ROW_CAP) >= 3 and np.sum(M < ROW_CAP) >= 3 and np.sum(M == ROW_CAP) > n - 20
    _all_kernels_match(gl, orc, ind, dist, 'redirects K=%d' % K)


@pytest.mark.parametrize('K,n', [(512, 1500), (1024, 2600)])
def test_boundary_rows_with_the_device_exp(gl, orc, K, n, device_exp):
    """The default mode (correctly rounded exp on the device) on the boundary lists: structure identical; gaussian within 1 ulp
    unsymmetrised and 2 symmetrised, symgaussian within rtol = 1e-15 (tests/test_gpu_knn.py::test_knn_to_csr_hub_vertex)."""
    ind, dist, _ = _boundary_lists(K, n, 1 if K == 512 else 2)
    for kernel in ('gaussian', 'symgaussian'):
        for symmetrize in (True, False):
            W = gl.weightmatrix.knn(None, K - 1, kernel=kernel, symmetrize=symmetrize, knn_data=(ind, dist.copy()))
            Wo = orc.knn_weights(ind, dist.copy(), K - 1, kernel=kernel, symmetrize=symmetrize)
            _same(W, Wo, (K, kernel, symmetrize), exact=False)
            worst = int(_ulps(W.data, Wo.data).max())
            print('K=%d %s symmetrize=%s: %d ulps at most' % (K, kernel, symmetrize, worst))
            if kernel == 'symgaussian' and symmetrize:
                assert np.allclose(W.data, Wo.data, rtol=1e-15, atol=0), (K, kernel, worst)
            else:
                assert worst <= (2 if symmetrize else 1), (K, kernel, symmetrize, worst)
            assert same_matrix(W, knn_weights_cr(ind, dist, K - 1, kernel, symmetrize)), (K, kernel, symmetrize, 'bit for bit')


BLOCK_CENSUS = {        # K: (smallest M, largest M, rows with M <= 64, with 64 < M <= ROW_CAP, with M > ROW_CAP)
    32: (63, 65, 699, 1, 0),
    65: (128, 1429, 0, 1299, 1),
    512: (1023, 1025, 0, 1499, 1),
    1024: (2047, 2049, 0, 0, 2600),
}


def _block_lists(K, n, mutual):
    """Circulant lists with one redirect (K = 65: and a vertex that everyone lists), given weights, and the census of the rows."""
    ind, _ = _circulant(n, K, 60 + K, mutual)
    _redirect(ind, n // 3, K // 2, 3)
    if K == 65:
        ind[:, K - 2] = 700
    w = np.random.default_rng(K + mutual).random((n, K)) + 0.25
    M = _census(ind, K)
    census = (int(M.min()), int(M.max()), int(np.sum(M <= 64)), int(np.sum((M > 64) & (M <= ROW_CAP))), int(np.sum(M > ROW_CAP)))
    return ind, w, census


@pytest.mark.parametrize('mutual', [False, True])
@pytest.mark.parametrize('K,n', [(32, 700), (65, 1300), (512, 1500), (1024, 2600)])
def test_block_assembly_at_every_row_class(K, n, mutual):
    """A rank's block of rows (glx_knn_rows_to_csr, row_base != 0: dist_build.assemble_rows_device) where the rows are register
    rows with one longer one (K = 32), wavefront rows under the k > 64 host branch with a hub (65), rows at the wavefront cap with
    a hub (512) and hubs at the scratch boundary (1024): identical to the scipy expressions on the block
    (dist_build.assemble_rows) and to the rows of the whole matrix, for unequal blocks, both rules and unsymmetrised."""
    from graphlearning_amd import dist_build, _hip
    _hip.require_device()
    ind, w, census = _block_lists(K, n, mutual)
    assert census == BLOCK_CENSUS[K], census
    bounds = np.array([0, n // 5, n // 2, n], dtype=np.int64)
    msgs = [dist_build.reverse_messages(ind[bounds[r]:bounds[r + 1]], w[bounds[r]:bounds[r + 1]], int(bounds[r]), bounds) for r in range(3)]
    for rule, sym in (('mean', 1), ('max', 2), (None, 0)):
        whole = _hip.knn_to_csr(ind, None, K, kernel='given', sym=sym, weights=w)
        for me in range(3):
            lo, hi = int(bounds[me]), int(bounds[me + 1])
            received = [msgs[r][me] for r in range(3)] if rule else None
            args = (lo, hi, n, ind[lo:hi], w[lo:hi], received, rule is not None, rule or 'mean')
            ref = dist_build.assemble_rows(*args)
            got = dist_build.assemble_rows_device(*args, device=0)
            tag = (K, mutual, rule, me)
            assert got.shape == ref.shape == (hi - lo, n), tag
            assert np.array_equal(got.indptr, ref.indptr) and np.array_equal(got.indices, ref.indices), tag
            assert np.array_equal(got.data, ref.data), tag
            rows = whole[lo:hi]
            assert np.array_equal(got.indptr, rows.indptr) and np.array_equal(got.indices, rows.indices), tag
            assert np.array_equal(got.data, rows.data), tag


# ---- 2. weight matrices of real wide graphs, both entry routes -------------------------------------------------------------------------

N_BLOBS = 2500


def _blob_set():
    return blobs(N_BLOBS, 8, 5, 21, 3.0)


@pytest.fixture(scope='module')
def blob_lists(orc):
    """cKDTree's lists of the blob set, by k (self excluded)."""
    X, _ = _blob_set()
    cache = {}

    def get(k):
        if k not in cache:
            cache[k] = orc.knnsearch(X, k + 1)
        return cache[k]
    return get


def _assert_blob_census(k, M):
    if k == 511:        # rows on both sides of the wavefront cap, and ON it
        assert np.sum(M <= ROW_CAP) > 1000 and np.sum(M > ROW_CAP) > 300, (k, M.min(), M.max())
        assert np.sum(M == ROW_CAP) > 0 and np.sum(M == ROW_CAP + 1) > 0 and np.sum(M == ROW_CAP - 1) > 0
    if k == 1023:       # every row a hub, scratches of 2048 and of 4096 entries
        assert np.all(M > ROW_CAP) and np.sum(M > HUB_FLOOR) > 500 and np.sum(M <= HUB_FLOOR) > 500, (k, M.min(), M.max())


@pytest.mark.parametrize('k', [64, 255, 511, 1023])
def test_wide_weight_matrices_both_routes(gl, orc, blob_lists, k):
    """weightmatrix.knn(X, k) (device-resident lists: glx_knn_result_to_csr) and the knn_data route (glx_knn_to_csr_into) against
    the oracle: all five kernels, symmetrised and not."""
    X, _ = _blob_set()
    Jo, Do = blob_lists(k)
    M = _census(Jo, k + 1)
    _assert_blob_census(k, M)
    for kernel in KERNELS:
        for symmetrize in (True, False):
            Wo = orc.knn_weights(Jo, Do.copy(), k, kernel=kernel, symmetrize=symmetrize)
            W = gl.weightmatrix.knn(X, k, kernel=kernel, symmetrize=symmetrize)
            _same(W, Wo, (k, kernel, symmetrize, 'searched'))
            W = gl.weightmatrix.knn(None, k, kernel=kernel, symmetrize=symmetrize, knn_data=(Jo, Do.copy()))
            _same(W, Wo, (k, kernel, symmetrize, 'knn_data'))


@pytest.mark.parametrize('style,k', [('grid', 511), ('grid', 1023), ('repeat3', 511)])
def test_wide_weight_matrices_with_masses_of_ties(gl, orc, style, k):
    """Integer grids and tripled points: equal distances everywhere, duplicates at distance 0 (cKDTree then does not put the self
    entry into column 0).  The lists are the oracle's (ties may be listed in another order by the search): the knn_data route."""
    from test_gpu_knn_wide import _data
    X = _data(style, 2400, 3, 77 + k)
    Jo, Do = orc.knnsearch(X, k + 1)
    assert np.sum(Do[:, 1:] == Do[:, :-1]) > Do.size // 4
    M = _census(Jo, k + 1)
    assert np.sum(M > ROW_CAP) > 100, (M.min(), M.max())
    for kernel in KERNELS:
        for symmetrize in (True, False):
            with np.errstate(all='ignore'):
                Wo = orc.knn_weights(Jo, Do.copy(), k, kernel=kernel, symmetrize=symmetrize)
                W = gl.weightmatrix.knn(None, k, kernel=kernel, symmetrize=symmetrize, knn_data=(Jo, Do.copy()))
            assert np.array_equal(W.indptr, Wo.indptr) and np.array_equal(W.indices, Wo.indices), (style, k, kernel, symmetrize)
            assert np.array_equal(W.data, Wo.data, equal_nan=True), (style, k, kernel, symmetrize)


@pytest.mark.parametrize('k', [255, 1023])
def test_wide_weight_matrices_with_the_device_exp(gl, orc, blob_lists, k, device_exp):
    """The default mode on the real wide graphs: 1 ulp unsymmetrised, 2 for gaussian, 8 for symgaussian."""
    X, _ = _blob_set()
    Jo, Do = blob_lists(k)
    for kernel in ('gaussian', 'symgaussian'):
        for symmetrize in (True, False):
            Wo = orc.knn_weights(Jo, Do.copy(), k, kernel=kernel, symmetrize=symmetrize)
            Wc = knn_weights_cr(Jo, Do, k, kernel, symmetrize)
            for W in (gl.weightmatrix.knn(X, k, kernel=kernel, symmetrize=symmetrize),
                      gl.weightmatrix.knn(None, k, kernel=kernel, symmetrize=symmetrize, knn_data=(Jo, Do.copy()))):
                _same(W, Wo, (k, kernel, symmetrize), exact=False)
                worst = int(_ulps(W.data, Wo.data).max())
                assert worst <= (1 if not symmetrize else (2 if kernel == 'gaussian' else 8)), (k, kernel, symmetrize, worst)
                assert same_matrix(W, Wc), (k, kernel, symmetrize, 'bit for bit')


def test_hub_heavy_result_through_ordinary_memory(gl, orc, blob_lists, monkeypatch):
    """_PINNED_CSR_MAX small: the result of an assembly in which every row is a hub comes back through glx_download instead of
    the compaction kernels writing into page-locked arrays -- identical to the pinned result and to the oracle, both routes."""
    from graphlearning_amd import _hip
    X, _ = _blob_set()
    k = 1023
    Jo, Do = blob_lists(k)
    assert np.all(_census(Jo, k + 1) > ROW_CAP)
    pinned = gl.weightmatrix.knn(X, k)
    monkeypatch.setattr(_hip, '_PINNED_CSR_MAX', 1 << 12)
    Wo = orc.knn_weights(Jo, Do.copy(), k)
    for W in (gl.weightmatrix.knn(X, k), gl.weightmatrix.knn(None, k, knn_data=(Jo, Do.copy()))):
        _same(W, Wo, 'ordinary memory')
        _same(W, pinned, 'ordinary memory against pinned')


def test_twenty_thousand_hub_rows(gl, orc):
    """n = 20 000, k = 1023: twenty thousand hub workgroups and a scratch of 0.94 GB (58.8 million 16-byte entries), once."""
    n, k = 20000, 1023
    X, _ = blobs(n, 8, 5, 33, 3.0)
    Jo, Do = orc.knnsearch(X, k + 1)
    M = _census(Jo, k + 1)
    assert np.all(M > ROW_CAP) and np.sum(M > HUB_FLOOR) > 1000
    scratch = int(np.sum(np.maximum(HUB_FLOOR, 2 ** np.ceil(np.log2(M)).astype(np.int64))))        # entries, 16 bytes each
    assert scratch * 16 > 900e6
    Wo = orc.knn_weights(Jo, Do, k, kernel='distance')
    W = gl.weightmatrix.knn(X, k, kernel='distance')
    _same(W, Wo, 'n=20000 k=1023')


# ---- 3. a row-length ladder for the operator ---------------------------------------------------------------------------------------------

LADDER = [0, 1, 3, 4, 5, 23, 24, 25, 63, 64, 65, 95, 96, 97, 255, 256, 257, 1023, 1024, 1025, 2500]


def _ladder_matrix(seed):
    """2688 rows whose lengths walk the ladder with period 21 (every sixteenth of the rows holds every length eight times),
    distinct random columns in random order inside a row, weights of both signs."""
    rng = np.random.default_rng(seed)
    n = 21 * 128
    lengths = np.array([LADDER[i % len(LADDER)] for i in range(n)])
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    indices = np.empty(indptr[-1], dtype=np.int32)
    for i in range(n):
        indices[indptr[i]:indptr[i + 1]] = rng.choice(n, size=lengths[i], replace=False)
    data = rng.normal(size=indptr[-1])
    A = sparse.csr_matrix((data, indices, indptr), shape=(n, n))
    A.has_sorted_indices = False
    return A, lengths


def _assert_ladder_spread(lengths, order):
    """Every length occurs in every sixteenth of the rows in the order the operator keeps them: the eight XCD ranges carry equal
    work and the ladder is periodic, so each range is about an eighth of the rows and holds a whole sixteenth."""
    kept = lengths[order]
    n = len(kept)
    for b in range(16):
        block = kept[b * n // 16:(b + 1) * n // 16]
        assert set(block.tolist()) == set(LADDER), b


@pytest.mark.parametrize('C', [1, 4, 10, 13, 30])
def test_operator_on_the_row_length_ladder(gl, C):
    """Db + A u against scipy's csr_matvecs bit for bit on rows of exactly 0 .. 2500 entries: both sides of every row class
    (24 / 25 and 96 / 97; 64 / 65 and 256 / 257 of relaxed plans), fp64 and fp32, one and three applications."""
    from graphlearning_amd import _hip
    A, lengths = _ladder_matrix(5)
    assert np.array_equal(np.diff(A.indptr), lengths) and set(lengths.tolist()) == set(LADDER)
    assert not np.all(np.diff(A.indices[A.indptr[-2]:A.indptr[-1]]) > 0)              # entry order inside rows: unsorted
    n = A.shape[0]
    rng = np.random.default_rng(C)
    u = rng.normal(size=(n, C))
    Db = rng.normal(size=(n, C))
    for keep_order in (True, False):
        G = _hip.DeviceGraph(A, keep_order=keep_order)
        try:
            if keep_order:
                assert np.array_equal(G.order(), np.arange(n))
                _assert_ladder_spread(lengths, np.arange(n))
            assert G.info()['max_row'] == 2500
            assert np.array_equal(G.spmm_bias(u, Db), Db + A * u), (C, keep_order)
            assert np.array_equal(G.spmm_bias(u, Db, iters=3), Db + A * (Db + A * (Db + A * u))), (C, keep_order)
            assert np.array_equal(G.spmm_bias(u, None), A * u), (C, keep_order)
        finally:
            G.close()
    A32 = _as_float32(A)
    assert np.array_equal(A32.indices, A.indices)
    u32, Db32 = u.astype(np.float32), Db.astype(np.float32)
    G = _hip.DeviceGraph(A, dtype=np.float32, keep_order=True)
    try:
        got = G.spmm_bias(u32, Db32)
        assert got.dtype == np.float32
        assert np.array_equal(got, Db32 + A32 * u32), C
        assert np.array_equal(G.spmm_bias(u32, Db32, iters=3), Db32 + A32 * (Db32 + A32 * (Db32 + A32 * u32))), C
    finally:
        G.close()


def _ladder_graph(seed):
    """A symmetric non-negative graph with prescribed degrees: one group of vertices per target degree t, a circulant of degree
    t - 1 inside the group (t of the three widest groups), and one edge from every vertex of the other groups to a vertex of its own
    in the widest groups, which ties the graph together without a long chain.  Vertices shuffled."""
    rng = np.random.default_rng(seed)
    targets = [3, 4, 5, 23, 24, 25, 26, 63, 64, 65, 66, 95, 96, 97, 98, 255, 256, 257, 258, 1023, 1024, 1025]
    rows, cols = [], []
    start, groups = 0, []
    for t in targets:
        core = t >= 1023
        deg = t if core else t - 1
        size = deg + 3 + ((deg + 3) % 2)                 # even, above the degree
        v = np.arange(size)
        for off in range(1, deg // 2 + 1):
            rows.append(start + v)
            cols.append(start + (v + off) % size)
        if deg % 2:
            rows.append(start + v[:size // 2])
            cols.append(start + v[:size // 2] + size // 2)
        groups.append((t, start, size, core))
        start += size
    n = start
    core_vertices = np.concatenate([np.arange(s, s + m) for _, s, m, c in groups if c])
    others = np.concatenate([np.arange(s, s + m) for _, s, m, c in groups if not c])
    assert len(others) <= len(core_vertices)
    rows.append(others)
    cols.append(rng.permutation(core_vertices)[:len(others)])
    r, c = np.concatenate(rows), np.concatenate(cols)
    half = sparse.coo_matrix((rng.random(len(r)) + 0.1, (r, c)), shape=(n, n)).tocsr()
    perm = rng.permutation(n)
    W = sparse.csr_matrix((half + half.T)[perm][:, perm])
    W.sort_indices()
    lab = (perm % 3).astype(np.int64)
    return W, lab


def test_learners_on_a_graph_of_ladder_degrees(gl, orc):
    """Poisson gradient descent, laplace(reduce='exact') and laplace(reduce='tree') on a symmetric graph whose degrees sit on both
    sides of 24, 64, 96 and 256 (and at 1023 .. 1026)."""
    W, lab = _ladder_graph(9)
    deg = np.diff(W.indptr)
    have = set(deg.tolist())
    for edge in (24, 64, 96, 256):
        assert edge in have and edge + 1 in have, (edge, sorted(have))
    assert {1023, 1024, 1025} <= have and deg.min() == 3
    assert (W != W.T).nnz == 0 and W.diagonal().sum() == 0 and W.data.min() > 0
    assert csgraph.connected_components(W, directed=False)[0] == 1
    ti = orc.trainsets_generate(lab, rate=4, seed=1)
    u_ref, T_ref = orc.poisson_gd(W, ti, lab[ti], min_iter=20, max_iter=70, return_T=True)
    m = gl.ssl.poisson(W, solver='gradient_descent', min_iter=20, max_iter=70)
    u = m.fit(ti, lab[ti])
    assert m.num_iter == T_ref and np.array_equal(u, u_ref)
    assert np.array_equal(m.predict(), orc.predict(u_ref))
    u_ref, it_ref = orc.laplace_fit(W, ti, lab[ti], return_iters=True)
    m = gl.ssl.laplace(W, reduce='exact')
    u = m.fit(ti, lab[ti])
    assert m.num_iter == it_ref and np.array_equal(u, u_ref)
    m = gl.ssl.laplace(W, reduce='tree')
    u = m.fit(ti, lab[ti])
    _tolerance_contract('ladder degrees, tree', u, m.num_iter, m.predict(), u_ref, it_ref, orc)


def _tolerance_contract(tag, u, it, pred, u_ref, it_ref, orc):
    """tests/test_gpu_auto.py's contract of the tolerance mode: iteration count equal, iterates within 1e-5 * max(1, max |u_ref|),
    labels equal."""
    scale = max(1.0, float(np.max(np.abs(u_ref))))
    du = float(np.max(np.abs(u - u_ref)))
    print('%s: %d iterations, |du| / scale = %.2e' % (tag, it, du / scale))
    assert it == it_ref, (tag, it, it_ref, du)
    assert du <= 1e-5 * scale, (tag, du)
    assert np.array_equal(pred, orc.predict(u_ref)), tag


# ---- 4. the whole path on wide graphs ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def wide_graph(gl, orc, blob_lists):
    """W = weightmatrix.knn(X, k) of the blob set, proven equal to the oracle's, by k."""
    X, lab = _blob_set()
    cache = {}

    def get(k):
        if k not in cache:
            Jo, Do = blob_lists(k)
            Wo = orc.knn_weights(Jo, Do.copy(), k)
            W = gl.weightmatrix.knn(X, k)
            _same(W, Wo, k)
            rowlen = np.diff(W.indptr)
            assert rowlen.min() >= k > 96                   # every row in the operator's widest class
            if k == 1023:
                assert rowlen.min() > 256                   # ... of the relaxed plans too
            cache[k] = (W, Wo, lab)
        return cache[k]
    return get


def _trainsets(orc, lab, count, seed):
    return [orc.trainsets_generate(lab, rate=2, seed=seed + j) for j in range(count)]


@pytest.mark.parametrize('k', [255, 1023])
def test_poisson_on_wide_graphs(gl, orc, wide_graph, k):
    """ssl.poisson, gradient descent and CG (in the --cg-form of the session): iterates, iteration counts, labels."""
    W, Wo, lab = wide_graph(k)
    ti = _trainsets(orc, lab, 1, 3)[0]
    u_ref, T_ref = orc.poisson_gd(Wo, ti, lab[ti], return_T=True)
    m = gl.ssl.poisson(W, solver='gradient_descent')
    u = m.fit(ti, lab[ti])
    assert m.num_iter == T_ref and np.array_equal(u, u_ref)
    assert np.array_equal(m.predict(), orc.predict(u_ref))
    u_ref, it_ref = orc.poisson_cg(Wo, ti, lab[ti], return_iters=True)
    m = gl.ssl.poisson(W)
    u = m.fit(ti, lab[ti])
    assert m.num_iter == it_ref and np.array_equal(u, u_ref)
    assert np.array_equal(m.predict(), orc.predict(u_ref))


@pytest.mark.parametrize('k', [255, 1023])
def test_laplace_in_three_modes_on_wide_graphs(gl, orc, wide_graph, k):
    """reduce='exact' bit for bit; 'tree' and the default 'auto' under the contract of tests/test_gpu_auto.py -- the relaxed plan on
    a graph whose every row is in the 16-slot class."""
    from test_gpu_auto import _check
    W, Wo, lab = wide_graph(k)
    ti = _trainsets(orc, lab, 1, 3)[0]
    u_ref, it_ref = orc.laplace_fit(Wo, ti, lab[ti], return_iters=True)
    m = gl.ssl.laplace(W, reduce='exact')
    u = m.fit(ti, lab[ti])
    assert m.num_iter == it_ref and np.array_equal(u, u_ref)
    assert np.array_equal(m.predict(), orc.predict(u_ref))
    m = gl.ssl.laplace(W, reduce='tree')
    u = m.fit(ti, lab[ti])
    _tolerance_contract('k=%d tree' % k, u, m.num_iter, m.predict(), u_ref, it_ref, orc)
    m = gl.ssl.laplace(W)
    assert m.reduce == 'auto'
    u = m.fit(ti, lab[ti])
    counts = dict(handed_back=0, tolerance_mode=0, worst=0.0)
    _check(gl, orc, 'k=%d auto' % k, u, m.num_iter, m.predict(), u_ref, it_ref, counts)
    print('k=%d auto: %s' % (k, counts))


@pytest.mark.parametrize('k', [255, 1023])
def test_stacked_trials_on_wide_graphs(gl, orc, wide_graph, k):
    """model._fit_batch: gradient descent with four and with five training sets (a full and a partial batch of ssl.GD_TRIAL_BATCH)
    and CG -- each trial equal to its own fit and to the oracle."""
    from graphlearning_amd import ssl as glssl
    W, Wo, lab = wide_graph(k)
    sets = _trainsets(orc, lab, 5, 10)
    assert glssl.GD_TRIAL_BATCH == 4
    refs = [orc.poisson_gd(Wo, t, lab[t], return_T=True) for t in sets]
    m = gl.ssl.poisson(W, solver='gradient_descent')
    for count in (4, 5):
        probs = m._fit_batch([(t, lab[t]) for t in sets[:count]])
        assert probs is not None and len(probs) == count
        its = list(m.num_iter)
        for j in range(count):
            assert its[j] == refs[j][1] and np.array_equal(probs[j], refs[j][0]), (k, count, j)
    own = gl.ssl.poisson(W, solver='gradient_descent')
    for j in (0, 4):
        assert np.array_equal(own.fit(sets[j], lab[sets[j]]), probs[j]) and own.num_iter == its[j], (k, j)
    m = gl.ssl.poisson(W)
    probs = m._fit_batch([(t, lab[t]) for t in sets[:3]])
    its = list(m.num_iter)
    own = gl.ssl.poisson(W)
    for j in range(3):
        u_ref, it_ref = orc.poisson_cg(Wo, sets[j], lab[sets[j]], return_iters=True)
        assert its[j] == it_ref and np.array_equal(probs[j], u_ref), (k, j)
        assert np.array_equal(own.fit(sets[j], lab[sets[j]]), probs[j]) and own.num_iter == it_ref, (k, j)


@pytest.mark.parametrize('k', [255, 1023])
def test_comparison_methods_on_wide_graphs(gl, orc, wide_graph, k):
    """PoissonMBO (short schedule, volume constraint), random walk, reweighted Laplace, page rank, the p-Laplace Jacobi iteration."""
    W, Wo, lab = wide_graph(k)
    ti = _trainsets(orc, lab, 1, 3)[0]
    priors = orc.class_priors(lab)
    u_ref, lab_ref, w_ref = orc.poisson_mbo_fit(Wo, ti, lab[ti], priors, solver='gradient_descent', Ns=12, T=4)
    m = gl.ssl.poisson_mbo(W, priors, solver='gradient_descent', Ns=12, T=4)
    pred = m.fit_predict(ti, lab[ti])
    assert np.array_equal(m.prob, u_ref) and np.array_equal(pred, lab_ref), k
    assert np.array_equal(np.asarray(m.weights), np.asarray(w_ref)), k
    u_ref, it_ref = orc.randomwalk_fit(Wo, ti, lab[ti], return_iters=True)
    m = gl.ssl.randomwalk(W, reduce='exact')
    u = m.fit(ti, lab[ti])
    assert m.num_iter == it_ref and np.array_equal(u, u_ref), k
    for rw in ('poisson', 'wnll'):
        u_ref = orc.laplace_reweighted_fit(Wo, ti, lab[ti], rw)
        u = gl.ssl.laplace(W, reweighting=rw, reduce='exact').fit(ti, lab[ti])
        assert np.array_equal(u, u_ref), (k, rw)
    G = gl.graph(W)
    pr_ref, it_ref = orc.page_rank(Wo, return_iters=True)
    pr = G.page_rank()
    assert G.page_rank_iters == it_ref and np.array_equal(pr, pr_ref), k
    rng = np.random.default_rng(k)
    bdy = rng.choice(W.shape[0], size=40, replace=False)
    val = rng.normal(size=40)
    u = G.plaplace(bdy, val, 3.0, tol=1e-2, max_num_it=150, fast=False)
    uo, it = orc.plaplace_jacobi(Wo, bdy, val, 3.0, tol=1e-2, max_num_it=150, return_iters=True)
    assert G.plaplace_iters == it and np.array_equal(u, uo, equal_nan=True), k


@pytest.mark.parametrize('k', [255, 1023])
def test_fp32_on_wide_graphs(gl, orc, wide_graph, k):
    """use_cuda=True: same T and labels, iterates within the project's stated 1e-5 * max(1, max |u_ref|).  The iterates of a wide
    graph are small, so that bound only catches gross errors here (a float32 restatement of the oracle's sweep on the host stays
    within 7e-9 of the fp64 oracle at k = 255 and 7e-10 at k = 1023).  The sharp check is the operator's own float32 contract
    (tests/test_gpu_parity.py::test_spmm_fp32: the order and roundings of scipy's float32 csr_matvecs) on the wide graph's
    P = D^-1 W^T, bit for bit for 1, 3 and 50 sweeps."""
    from graphlearning_amd import _hip
    W, Wo, lab = wide_graph(k)
    ti = _trainsets(orc, lab, 1, 3)[0]
    u_ref, T_ref = orc.poisson_gd(Wo, ti, lab[ti], return_T=True)
    m = gl.ssl.poisson(W, solver='gradient_descent', use_cuda=True)
    u = m.fit(ti, lab[ti])
    assert u.dtype == np.float32 and m.num_iter == T_ref
    du = float(np.max(np.abs(u - u_ref)))
    print('k=%d fp32 gradient descent: T=%d, max |du| = %.2e, max |u_ref| = %.2e' % (k, T_ref, du, np.max(np.abs(u_ref))))
    assert du <= 1e-5 * max(1.0, np.max(np.abs(u_ref)))
    assert np.array_equal(m.predict(), orc.predict(u_ref))
    s = orc.poisson_gd_setup(Wo, ti, lab[ti])
    P = sparse.csr_matrix(s['P'])
    P32 = _as_float32(P)
    Db32 = s['Db'].astype(np.float32)
    G = _hip.DeviceGraph(P, dtype=np.float32)
    try:
        done, v = 0, np.zeros_like(Db32)
        for T in (1, 3, 50):
            while done < T:
                v = Db32 + P32 * v
                done += 1
            got = G.spmm_bias(np.zeros_like(Db32), Db32, iters=T)
            assert got.dtype == np.float32 and np.array_equal(got, v), (k, T)
    finally:
        G.close()


def test_solvers_on_a_device_exp_wide_graph(gl, orc, blob_lists, device_exp):
    """The default mode at k = 255: W within two ulps of the oracle's, then the solvers against the oracle on the SAME matrix."""
    X, lab = _blob_set()
    k = 255
    Jo, Do = blob_lists(k)
    Wo = orc.knn_weights(Jo, Do.copy(), k)
    W = gl.weightmatrix.knn(X, k)
    _same(W, Wo, 'device exp', exact=False)
    assert int(_ulps(W.data, Wo.data).max()) <= 2
    Ws = sparse.csr_matrix(W)
    ti = _trainsets(orc, lab, 1, 3)[0]
    u_ref, T_ref = orc.poisson_gd(Ws, ti, lab[ti], return_T=True)
    m = gl.ssl.poisson(W, solver='gradient_descent')
    assert np.array_equal(m.fit(ti, lab[ti]), u_ref) and m.num_iter == T_ref
    u_ref, it_ref = orc.poisson_cg(Ws, ti, lab[ti], return_iters=True)
    m = gl.ssl.poisson(W)
    assert np.array_equal(m.fit(ti, lab[ti]), u_ref) and m.num_iter == it_ref
    u_ref, it_ref = orc.laplace_fit(Ws, ti, lab[ti], return_iters=True)
    m = gl.ssl.laplace(W, reduce='exact')
    assert np.array_equal(m.fit(ti, lab[ti]), u_ref) and m.num_iter == it_ref


def test_vertex_partition_of_a_wide_graph(gl, orc, wide_graph):
    """Three ranks, equal blocks of the locality order, on the k = 255 graph: T and the gathered iterate equal to the oracle in
    both exchange forms.  The ranks import 3350 rows between them, dist.halo_share = 0.503 of the rows they do not own (five blobs
    over three blocks: a rank needs about half of everybody else's rows), which is below dist.GATHER_SHARE = 0.9, so
    dist.make_plan(exchange='auto') picks the halo lists (RankPlan), not the all-gather of whole blocks."""
    from graphlearning_amd import dist as gdist, _hip
    W, Wo, lab = wide_graph(255)
    ti = _trainsets(orc, lab, 1, 3)[0]
    u_ref, T_ref = orc.poisson_gd(Wo, ti, lab[ti], return_T=True)
    prob = gdist.poisson_problem(Wo, ti, lab[ti])
    n = Wo.shape[0]
    order = gdist.locality_order(prob['P'])
    bounds = gdist.block_bounds(n, 3)
    share = gdist.halo_share(prob['P'], order, bounds)
    auto = gdist.make_plan(prob['P'], order, bounds, 0, exchange='auto')
    print('halo share %.3f, exchange=auto picks %s' % (share, type(auto).__name__))
    assert 0.4 <= share < gdist.GATHER_SHARE and type(auto) is gdist.RankPlan
    for gather in (False, True):
        u, T, halo = _virtual_ranks_sweep(gdist, _hip, prob, order, bounds, 50, 1000, gather=gather)
        assert T == T_ref and np.array_equal(u, u_ref), gather
        if not gather:
            assert halo == round(share * 2 * n)
