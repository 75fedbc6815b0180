"""csrc/csr_plan.h without a device: the column-tile rule in both of its forms, the training-row map, the walk over a canonical CSR
matrix with each of its codes and hook positions, the range check of a vertex list with both nouns, and -- through the four
validators that are built on it -- which of two faults in one input is answered.

The codes in the *_FIRST_FAULT tables are literals: each was taken by running the validator of the commit before csr_plan.h existed,
where every validator held its own copy of the walk, on that very input, so the order of the refusals is pinned to what it was."""
import ctypes
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import ck_ref       # noqa: E402
import dlp_ref      # noqa: E402
import eig_ref      # noqa: E402
import slp_ref      # noqa: E402

WALK_PTR, WALK_COL, WALK_CANON, HOOK_BEFORE, HOOK_ENTRY, HOOK_AFTER = 12, 13, 14, 21, 22, 23
NAN, INF = float('nan'), float('inf')


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    """csrc/csr_plan.h compiled for the host: `g++ -O2 -ffp-contract=off` behind tests/csr_plan_host.cpp."""
    so = os.path.join(str(tmp_path_factory.mktemp('csr_plan')), 'libcsr_plan_host.so')
    subprocess.run(['g++', '-O2', '-ffp-contract=off', '-std=c++17', '-fPIC', '-shared', '-I' + os.path.join(ROOT, 'graphlearning_amd', 'csrc'),
                    '-o', so, os.path.join(ROOT, 'tests', 'csr_plan_host.cpp')], check=True)
    lib = ctypes.CDLL(so)
    vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.csr_host_walk.argtypes = [i64, i64, vp, vp, i64, i64, i64, vp, ctypes.c_char_p, ci]
    lib.csr_host_walk_entries.argtypes = [i64, i64, vp, vp, i64, ctypes.c_char_p, ci]
    lib.csr_host_check_vertices.argtypes = [vp, i64, i64, ci, ctypes.c_char_p, ctypes.c_char_p, ci]
    lib.csr_host_label_rows.argtypes = [i64, i64, vp, vp]
    lib.csr_host_label_rows.restype = None
    lib.csr_host_tiles.argtypes = [ci, ci, vp, vp, ci, vp]
    return lib


def walk(lib, row_ptr, col, before_at=-1, entry_at=-1, after_at=-1, M=None):
    """(code, message, (before, entry, after) calls, the entries the before hooks were promised)"""
    row_ptr, col = np.asarray(row_ptr, dtype=np.int64), np.asarray(col, dtype=np.int32)
    counts, msg = np.zeros(4, dtype=np.int64), ctypes.create_string_buffer(256)
    rc = lib.csr_host_walk(len(row_ptr) - 1, len(col) if M is None else M, _p(row_ptr), _p(col), before_at, entry_at, after_at, _p(counts), msg, 256)
    return rc, msg.value.decode(), tuple(int(c) for c in counts[:3]), int(counts[3])


# ---- the column-tile rule ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('width', [1, 16, 64])
def test_tile_rule(lib, width):
    for k in range(1, 257):
        out, out_at, ct = np.zeros(2 * 256, dtype=np.int32), np.zeros(2 * 256, dtype=np.int32), np.zeros(1, dtype=np.int32)
        nt = lib.csr_host_tiles(k, width, _p(out), _p(out_at), 256, _p(ct))
        assert nt == -(-k // width), (k, width)
        tiles = out[:2 * nt].reshape(nt, 2)
        c0, cols = tiles[:, 0], tiles[:, 1]
        assert c0[0] == 0 and np.array_equal(c0[1:], np.cumsum(cols)[:-1]) and cols.sum() == k, (k, width)       # [0, k) exactly, in order
        assert cols.min() >= 1 and cols.max() <= width and cols.max() - cols.min() <= 1, (k, width)
        assert np.all(np.diff(cols) <= 0) and int(ct[0]) == cols[0] == cols.max(), (k, width)                      # the wider ones first
        assert np.array_equal(out_at[:2 * nt].reshape(nt, 2), tiles), (k, width)                                  # (tile, tbase, textra) agrees


def test_tile_examples(lib):
    """the shapes the device tests lean on: 17 columns are 9 + 8, 33 are three tiles of 11"""
    def tiles(k, width=16):
        out, out_at, ct = np.zeros(64, dtype=np.int32), np.zeros(64, dtype=np.int32), np.zeros(1, dtype=np.int32)
        nt = lib.csr_host_tiles(k, width, _p(out), _p(out_at), 32, _p(ct))
        return out[:2 * nt].reshape(nt, 2).tolist()
    assert tiles(17) == [[0, 9], [9, 8]]
    assert tiles(33) == [[0, 11], [11, 11], [22, 11]]
    assert tiles(16) == [[0, 16]] and tiles(1) == [[0, 1]]
    assert tiles(256, 64) == [[0, 64], [64, 64], [128, 64], [192, 64]]


# ---- the training-row map and the vertex list -------------------------------------------------------------------------------------------

def test_label_rows(lib):
    def rows(n, ind):
        ind, lab = np.asarray(ind, dtype=np.int32), np.full(n, 77, dtype=np.int32)
        lib.csr_host_label_rows(n, len(ind), _p(ind) if len(ind) else None, _p(lab))
        return lab.tolist()
    assert rows(5, [3, 0]) == [1, -1, -1, 0, -1]                       # an unlisted vertex is -1
    assert rows(5, [3, 0, 3, 3]) == [1, -1, -1, 3, -1]                 # a vertex listed twice takes its last row
    assert rows(4, []) == [-1, -1, -1, -1]                             # m = 0 is accepted
    assert rows(1, [0]) == [0]


def test_vertex_list(lib):
    def check(ind, n, code, noun):
        ind, msg = np.asarray(ind, dtype=np.int32), ctypes.create_string_buffer(128)
        rc = lib.csr_host_check_vertices(_p(ind) if len(ind) else None, len(ind), n, code, noun.encode(), msg, 128)
        return rc, msg.value.decode()
    assert check([0, 4, 2], 5, 7, 'training') == (0, '')
    assert check([], 5, 7, 'training') == (0, '')
    assert check([0, 5, -1], 5, 7, 'training') == (7, 'training vertex 5 out of range')          # the first one in the list
    assert check([0, -1, 5], 5, 8, 'labelled') == (8, 'labelled vertex -1 out of range')


# ---- the walk ------------------------------------------------------------------------------------------------------------------------------

PTR = [0, 2, 3, 3, 5, 5]                # rows 0: (1, 2), 1: (0), 2: (), 3: (0, 4), 4: (): an empty row inside and a last row that is empty
COL = [1, 2, 0, 0, 4]


def test_walk_accepts_and_is_one_pass(lib):
    assert walk(lib, PTR, COL) == (0, '', (5, 5, 5), 5)                 # every row asked once before and once after, every entry once
    assert walk(lib, [0, 0], []) == (0, '', (1, 0, 1), 0)               # n = 1 with M = 0
    assert walk(lib, [0, 0, 0], []) == (0, '', (2, 0, 2), 0)
    msg = ctypes.create_string_buffer(64)
    ptr, col = np.asarray(PTR, dtype=np.int64), np.asarray(COL, dtype=np.int32)
    assert lib.csr_host_walk_entries(5, 5, _p(ptr), _p(col), -1, msg, 64) == 0
    assert lib.csr_host_walk_entries(5, 5, _p(ptr), _p(col), 3, msg, 64) == HOOK_ENTRY and msg.value == b'entry 3'


def test_walk_row_pointers(lib):
    assert walk(lib, [1, 2, 3, 3, 5, 5], COL)[:2] == (WALK_PTR, 'row pointers run from 1 to 5, expected 0 to M=5')
    assert walk(lib, PTR, COL, M=4)[:2] == (WALK_PTR, 'row pointers run from 0 to 5, expected 0 to M=4')
    assert walk(lib, [0, 2, 1, 3, 5, 5], COL)[:2] == (WALK_PTR, 'row pointers of vertex 1 are not ascending within [0, M]')
    assert walk(lib, [0, 7, 3, 3, 5, 5], COL)[:2] == (WALK_PTR, 'row pointers of vertex 0 are not ascending within [0, M]')
    assert walk(lib, [0, 2, 1, 3, 5, 5], COL)[2] == (1, 2, 1)           # row 0 was walked, row 1 was not begun


def test_walk_columns(lib):
    assert walk(lib, PTR, [1, 2, 0, -1, 4])[:2] == (WALK_COL, 'column index -1 of entry 3 out of range')
    assert walk(lib, PTR, [1, 5, 0, 0, 4])[:2] == (WALK_COL, 'column index 5 of entry 1 out of range')
    text = 'row %d is not canonical: its columns are not strictly ascending (entry %d)'
    assert walk(lib, PTR, [1, 1, 0, 0, 4])[:2] == (WALK_CANON, text % (0, 1))          # a duplicate
    assert walk(lib, PTR, [1, 2, 0, 4, 0])[:2] == (WALK_CANON, text % (3, 4))          # descending
    assert walk(lib, PTR, [2, 1, 0, 0, 4])[0] == WALK_CANON
    assert walk(lib, PTR, [1, 2, 0, 0, 0])[0] == WALK_CANON
    assert walk(lib, PTR, [1, 2, 2, 1, 4])[0] == 0                                     # the order is a row's own: 2 | 1 across rows is fine
    assert walk(lib, PTR, [1, 2, 0, 4, 9])[0] == WALK_COL                              # the range comes before the order


def test_walk_hook_positions(lib):
    assert walk(lib, PTR, COL, before_at=2)[:2] == (HOOK_BEFORE, 'before row 2 with 0 entries')
    assert walk(lib, PTR, COL, before_at=3)[:2] == (HOOK_BEFORE, 'before row 3 with 2 entries')
    assert walk(lib, PTR, COL, entry_at=4)[:2] == (HOOK_ENTRY, 'entry 4 of row 3')
    assert walk(lib, PTR, COL, after_at=4)[:2] == (HOOK_AFTER, 'after row 4')
    assert walk(lib, PTR, COL, after_at=4)[2] == (5, 5, 5)
    # before: behind the row's pointers, ahead of its entries
    assert walk(lib, [0, 2, 3, 3, 2, 5], COL, before_at=3)[0] == WALK_PTR
    assert walk(lib, PTR, [1, 2, 0, 9, 4], before_at=3)[0] == HOOK_BEFORE
    assert walk(lib, PTR, [1, 2, 9, 0, 4], before_at=3)[0] == WALK_COL
    # entry: behind both checks of its own entry, ahead of the next entry's
    assert walk(lib, PTR, [1, 9, 0, 0, 4], entry_at=1)[0] == WALK_COL
    assert walk(lib, PTR, [1, 1, 0, 0, 4], entry_at=1)[0] == WALK_CANON
    assert walk(lib, PTR, [1, 9, 0, 0, 4], entry_at=0)[0] == HOOK_ENTRY
    # after: behind the row's entries, ahead of the next row's pointers
    assert walk(lib, PTR, [1, 9, 0, 0, 4], after_at=0)[0] == WALK_COL
    assert walk(lib, PTR, COL, entry_at=1, after_at=0)[0] == HOOK_ENTRY
    assert walk(lib, [0, 2, 1, 3, 5, 5], COL, after_at=0)[0] == HOOK_AFTER
    assert walk(lib, PTR, COL, before_at=1, after_at=0)[0] == HOOK_AFTER
    assert walk(lib, PTR, COL, before_at=1, after_at=1)[0] == HOOK_BEFORE


# ---- first fault wins: the four validators ----------------------------------------------------------------------------------------------

RING_PTR = [0, 2, 4, 6, 8, 10]          # five vertices on a ring, no diagonal: entries 2 i and 2 i + 1 belong to row i
RING_COL = [1, 4, 0, 2, 1, 3, 2, 4, 0, 3]


def ring(ptr=None, col=None, **values):
    """(row_ptr, col, ten values of 1.0 with `values` = {entry: value} put in)"""
    data = np.ones(10)
    for e, v in values.items():
        data[int(e[1:])] = v
    col = list(RING_COL) if col is None else col
    return (np.asarray(RING_PTR if ptr is None else ptr, dtype=np.int64), np.asarray(col, dtype=np.int32), data[:len(col)].copy())


def put(col, **at):
    out = list(RING_COL) if col is None else list(col)
    for e, v in at.items():
        out[int(e[1:])] = v
    return out


def slp_case(ptr=None, col=None, w=None, lam=None, gamma=None, C=2, ind=(0, 3)):
    rp, cl, W = ring(ptr, col, **(w or {}))
    L = ring(ptr, col, **(lam or {}))[2]
    g = np.ones(5)
    for i, v in (gamma or {}).items():
        g[i] = v
    return rp, cl, W, L, g, C, np.asarray(ind, dtype=np.int32)


SLP_FIRST_FAULT = [
    ('an empty row 3 and a bad gamma[1]', dict(ptr=[0, 2, 4, 6, 6, 8], col=RING_COL[:6] + RING_COL[8:], gamma={1: NAN}), 7),
    ('an empty row 1 and a bad gamma[3]', dict(ptr=[0, 2, 2, 4, 6, 8], col=RING_COL[:2] + RING_COL[4:], gamma={3: INF}), 3),
    ('a bad column in row 2 and a bad weight in row 1', dict(col=put(None, e4=5), w={'e3': NAN}), 6),
    ('a bad weight in row 2 and a bad column in row 1', dict(col=put(None, e3=-1), w={'e4': NAN}), 4),
    ('a duplicate at entry 3 and a bad lam at entry 2', dict(col=put(None, e3=0), lam={'e2': NAN}), 7),
    ('one entry with a bad column and a bad weight', dict(col=put(None, e5=7), w={'e5': 0.0}), 4),
    ('one entry out of order with a bad weight', dict(col=put(None, e5=1), w={'e5': -1.0}), 5),
    ('a bad weight and a bad lam on one entry', dict(w={'e6': INF}, lam={'e6': INF}), 6),
    ('a bad lam at entry 1 and a bad gamma[0]', dict(lam={'e1': NAN}, gamma={0: NAN}), 7),
    ('a labelled vertex out of range and a bad gamma[4]', dict(ind=(0, 5), gamma={4: NAN}), 7),
    ('descending row pointers at row 3 and an empty row 1', dict(ptr=[0, 2, 2, 6, 4, 10]), 3),
    ('row pointers that end short and a bad weight', dict(ptr=[0, 2, 4, 6, 8, 9], w={'e0': NAN}), 2),
    ('C = 0 and row pointers that start at 1', dict(ptr=[1, 2, 4, 6, 8, 10], C=0), 1),
]

CK_FIRST_FAULT = [
    ('a duplicate that is also the diagonal', dict(col=put(None, e4=2, e5=2)), {}, 5),
    ('a descending entry that is also the diagonal', dict(col=put(None, e4=3, e5=2)), {}, 4),
    ('a stored diagonal with a weight that is not finite', dict(col=put(None, e2=1), e2=NAN), {}, 5),
    ('a bad column in row 2 and a weight that is not finite in row 1', dict(col=put(None, e4=5), e3=INF), {}, 6),
    ('a weight that is not finite in row 2 and a bad column in row 1', dict(col=put(None, e3=9), e4=INF), {}, 3),
    ('a training vertex out of range and a NaN in the last entry', dict(e9=NAN), dict(ind=(7,)), 6),
    ('a training vertex out of range and a diagonal in row 4', dict(col=put(None, e9=4)), dict(ind=(0, -2)), 5),
    ('257 columns and power_it = 0', {}, dict(k=257, power_it=0), 9),
    ('power_it = 0 and row pointers that start at 1', dict(ptr=[1, 2, 4, 6, 8, 10]), dict(power_it=0), 8),
    ('k = 0 and 257 columns is not the question', {}, dict(k=0, power_it=0), 1),
    ('descending row pointers at row 2 and a diagonal in row 0', dict(ptr=[0, 2, 4, 3, 8, 10], col=put(None, e0=0)), {}, 5),
]

DLP_FIRST_FAULT = [
    ('a bad column in row 2 and a value that is not finite in row 1', dict(col=put(None, e4=5), e3=NAN), {}, 5),
    ('a value that is not finite in row 2 and a bad column in row 1', dict(col=put(None, e2=-3), e4=NAN), {}, 3),
    ('a duplicate whose value is not finite', dict(col=put(None, e7=2), e7=INF), {}, 4),
    ('a duplicate in row 3 and a training vertex out of range', dict(col=put(None, e7=2)), dict(ind=(5,)), 4),
    ('a training vertex out of range and a value that is not finite', dict(e9=NAN), dict(ind=(5,)), 5),
    ('T = 0 and 65 columns', {}, dict(T=0, k=65), 7),
    ('65 columns and row pointers that end short', dict(ptr=[0, 2, 4, 6, 8, 9]), dict(k=65), 9),
    ('alpha not finite and k = 0', {}, dict(alpha=NAN, k=0), 1),
    ('row pointers that end short and a bad column', dict(ptr=[0, 2, 4, 6, 8, 9], col=put(None, e0=9)), {}, 2),
]

EIG_FIRST_FAULT = [
    ('a bad column in row 2 and a value that is not finite in row 1', dict(col=put(None, e4=5), e3=NAN), 3, 6),
    ('a value that is not finite in row 2 and a bad column in row 1', dict(col=put(None, e2=-3), e4=NAN), 3, 3),
    ('a duplicate whose value is not finite', dict(col=put(None, e7=2), e7=INF), 3, 4),
    ('descending row pointers at row 3 and a duplicate in row 1', dict(ptr=[0, 2, 4, 8, 6, 10], col=put(None, e3=0)), 3, 4),
    ('descending row pointers at row 1 and a duplicate in row 3', dict(ptr=[0, 2, 1, 6, 8, 10], col=put(None, e7=2)), 3, 2),
    ('m = 0 and row pointers that start at 1', dict(ptr=[1, 2, 4, 6, 8, 10]), 0, 8),
    ('m = 6 above n and a value that is not finite', dict(e0=NAN), 6, 8),
    ('a negative last row pointer and a value that is not finite', dict(ptr=[0, 2, 4, 6, 8, -1], e0=NAN), 3, 2),
    ('a stored diagonal is legal here, the NaN behind it is not', dict(col=put(None, e2=1), e3=NAN), 3, 6),
]


@pytest.fixture(scope='module')
def validators(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('csr_validators')
    return {name: mod.build_host_lib(tmp) for name, mod in (('slp', slp_ref), ('ck', ck_ref), ('dlp', dlp_ref), ('eig', eig_ref))}


def slp_code(lib, kw):
    return slp_ref.host_validate(lib, *slp_case(**kw))


def ck_code(lib, graph, call):
    rp, cl, W = ring(**graph)
    call = dict(dict(k=2, ind=(0, 3)), **call)
    return ck_ref.host_validate(lib, rp, cl, W, call.pop('k'), np.asarray(call.pop('ind'), dtype=np.int32), **call)


def dlp_code(lib, graph, call):
    rp, cl, P = ring(**graph)
    call = dict(dict(k=2, ind=(0, 3)), **call)
    return dlp_ref.host_validate(lib, rp, cl, P, call.pop('k'), np.asarray(call.pop('ind'), dtype=np.int32), **call)


def eig_code(lib, graph, m):
    return eig_ref.host_validate(lib, *ring(**graph), m)


@pytest.mark.parametrize('what,kw,code', SLP_FIRST_FAULT, ids=[c[0] for c in SLP_FIRST_FAULT])
def test_first_fault_slp(validators, what, kw, code):
    """slp_validate on inputs that hold two faults; `code` is what the validator answered before it was built on csr_walk."""
    assert slp_code(validators['slp'], kw) == code


@pytest.mark.parametrize('what,graph,call,code', CK_FIRST_FAULT, ids=[c[0] for c in CK_FIRST_FAULT])
def test_first_fault_ck(validators, what, graph, call, code):
    """ck_validate on inputs that hold two faults; `code` is what the validator answered before it was built on csr_walk."""
    assert ck_code(validators['ck'], graph, call) == code


@pytest.mark.parametrize('what,graph,call,code', DLP_FIRST_FAULT, ids=[c[0] for c in DLP_FIRST_FAULT])
def test_first_fault_dlp(validators, what, graph, call, code):
    """dlp_validate on inputs that hold two faults; `code` is what the validator answered before it was built on csr_walk."""
    assert dlp_code(validators['dlp'], graph, call) == code


@pytest.mark.parametrize('what,graph,m,code', EIG_FIRST_FAULT, ids=[c[0] for c in EIG_FIRST_FAULT])
def test_first_fault_eig(validators, what, graph, m, code):
    """eig_validate on inputs that hold two faults; `code` is what the validator answered before it was built on csr_walk."""
    assert eig_code(validators['eig'], graph, m) == code


def test_the_clean_ring_passes(validators):
    assert slp_code(validators['slp'], {}) == 0 and ck_code(validators['ck'], {}, {}) == 0
    assert dlp_code(validators['dlp'], {}, {}) == 0 and eig_code(validators['eig'], {}, 3) == 0


def test_one_definition_per_rule():
    """the rules this header took over are written nowhere else in the plan headers and kernels"""
    csrc = os.path.join(ROOT, 'graphlearning_amd', 'csrc')
    with open(os.path.join(csrc, 'csr_plan.h')) as f:
        text = f.read()
    assert '#include <hip' not in text and 'glx_internal.h' not in text          # host only
    for rule in ('is not canonical', 'lab[ind[q]]', 'tile < textra', 'vertex %d out of range'):
        holders = [name for name in sorted(os.listdir(csrc)) if name.endswith(('.h', '.hip')) and rule in open(os.path.join(csrc, name)).read()]
        assert holders == ['csr_plan.h'], (rule, holders)
