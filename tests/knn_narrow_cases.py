"""The cases of tests/test_gpu_knn_narrow.py (the exact kNN search with k <= 60 at every feature-width class and list length) and
a restatement in Python of what graphlearning_amd/csrc/knn_plan.h decides for them: which tile-kernel instantiation a case runs
(its KERNEL KEY) and the statistics the search must report.  tests/test_knn_plan.py checks the restatement against the header on
the host for every d <= 400, k <= 60, and that the cases reach every kernel key there is -- no GPU needed for the coverage claim;
tests/test_gpu_knn_narrow.py runs the cases and asserts, from glx_knn_stats, that the instantiation the key names is the one that ran."""
from collections import namedtuple

N_MAIN = 2999                 # no multiple of 32, 64 or 128: 94 / 47 / 24 ref tiles, the last one ragged
BQ = 128
FILTER = {None: 0, 'bf16': 1, 'f32': 2}
LISTS = {None: 0, 'short': 1, 'long': 2}

Plan = namedtuple('Plan', 'KP DH nkb NKB dpa BR ntiles nsplit use_bf16 cat short_lists')


def _tile_nsub(DH, KP):
    stride = 2 * DH + 2
    for ns in (4, 2):
        if 2 * 32 * ns * stride * 4 + (KP + 8) * 256 * 8 <= (53 if KP == 8 else 78) * 1024:
            return ns
    return 1


def plan(n, d, k, nq=None, long_lists=False, filter=None, lists=None, nsplit=None, concat=None):
    """knn_make_plan for k <= 60 (the narrow search), field by field."""
    assert 1 <= k <= 60
    nq = n if nq is None else nq
    short = not long_lists and d + 2 <= 132 and LISTS[lists] != 2
    if short:
        KP = 8 if k <= 12 else 16 if k <= 28 else 32
    else:
        KP = 16 if k <= 12 else 32 if k <= 28 else 64
    DH, nkb = (16 if KP == 64 else 32), 1
    if d + 2 <= 132 and not (KP == 64 and d + 2 > 36):
        DH = next(c for c in (8, 12, 18, 34, 66) if 2 * c >= d + 2)
    else:
        nkb = (d + 2 + 2 * DH - 1) // (2 * DH)
    use_bf16 = short and d <= 128 and FILTER[filter] != 2
    NKB = next(c for c in (1, 2, 4, 6, 8) if 16 * c >= d) if use_bf16 else 0
    dpa = 16 * NKB if use_bf16 else 2 * DH * nkb
    nqb = (nq + BQ - 1) // BQ
    BR = 32 * (1 if (NKB >= 4 or KP >= 32) else 2) if use_bf16 else 32 * _tile_nsub(DH, KP)
    ntiles = (n + BR - 1) // BR
    ns = max(1, min(8, ntiles, (1024 + nqb - 1) // nqb))
    if short:
        ns = max(ns, min(8 if (KP == 8 and n * d * 8.0 > 64.0 * 1024 * 1024) else 4, ntiles))
    if nsplit:
        ns = max(1, min(8, ntiles, nsplit))
    cat = 0
    if use_bf16 and NKB == 2 and d <= 21:
        cat = 2 if d < 21 else 1
        if concat is not None:
            cat = min(cat, concat)
    return Plan(KP, DH, nkb, NKB, dpa, BR, ntiles, ns, use_bf16, cat, short)


def kernel_key(p):
    """The template instantiation a plan launches: ('bf16', NKB, cat, KP, BR) of knn_tile_bf16_kernel, ('f32', DH, KP, blocked, BR)
    of knn_tile_kernel."""
    return ('bf16', p.NKB, p.cat, p.KP, p.BR) if p.use_bf16 else ('f32', p.DH, p.KP, p.nkb > 1, p.BR)


def list_of_ref(j, p):
    """Which of a query's 2 nsplit candidate lists ref j can enter, for both filters alike.  Read from the tile kernels
    (knn_tile_bf16.h, knn_tile_f32.h): workgroup (query block, sp) walks the ref tiles t = sp, sp + nsplit, ... of BR refs each, so
    range = (j // BR) % nsplit; within a tile the value of query column `lane & 31` against ref `t * BR + sub * 32 + (e & 3) +
    8 * (e >> 2) + 4 * h` sits in accumulator element e of sub-tile `sub` of the lane with h = lane >> 5 (the 32 x 32 MFMA result
    layout), and every lane keeps its own list: half = h = ((j % 32) // 4) % 2.  The lists are written out as list sp * 2 + h."""
    return ((j // p.BR) % p.nsplit) * 2 + ((j % 32) // 4) % 2


Case = namedtuple('Case', 'group d k style n opts')       # opts: the knn_options of the case, as a tuple of (name, value) pairs


def _case(group, d, k, style, n=N_MAIN, **opts):
    return Case(group, d, k, style, n, tuple(sorted(opts.items())))


MAIN_D = (1, 16, 17, 20, 21, 22, 32, 33, 48, 49, 64, 65, 80, 96, 97, 112, 128, 129, 130, 131)
MAIN_K = (12, 13, 28, 29, 60)               # both sides of each list-length class
F32_D = (14, 15, 22, 23, 34, 35, 66, 67, 128)             # both sides of every DH class of the fp32-input filter
LONG_D = (14, 20, 33, 64, 96, 130, 190, 191)              # (14: the only width class whose lists of 64 stay unblocked with DH = 8)
LONG_K = (12, 28, 29, 60)
ADVERSARIAL = ('offset', 'neardup', 'repeat3', 'badscale')
# one adversarial style per d at k = 12, the next one at k = 29.  The rotation starts so that every NKB class (d <= 16, 32, 64, 96,
# 128) meets 'neardup' and 'offset': test_knn_plan.py checks that it does.
ADVERSARIAL_K = (12, 29)


def _cases():
    out = []
    for d in MAIN_D:
        for k in MAIN_K:
            out.append(_case('main', d, k, 'iso'))
    for i, d in enumerate(MAIN_D):
        for j, k in enumerate(ADVERSARIAL_K):
            out.append(_case('main', d, k, 'grid' if d <= 3 and j == 1 else ADVERSARIAL[(i + 2 * j) % 4]))
    for d in F32_D:
        for k in MAIN_K:
            out.append(_case('f32', d, k, 'iso', filter='f32'))
    for d in LONG_D:
        for k in LONG_K:
            out.append(_case('long', d, k, 'iso', lists='long'))
    for d in (32, 64, 96, 128):                       # the full-width edge of NKB = 2, 4, 6, 8: the last feature block's lo halves matter
        for k in ADVERSARIAL_K:
            out.append(_case('split', d, k, 'lohalf'))
    for d in (96, 128):                               # forced repair: 2 lists of 8 for 12 neighbours (so many rows fail that the search
        out.append(_case('repair', d, 12, 'iso', nsplit=1))       # is repeated with the long lists), 4 lists of 8 (a few rows fail: the
        out.append(_case('repair', d, 12, 'iso', nsplit=2))       # exact fallback, row by row)
    for d in (21, 96, 128, 130):                      # one tile, one ragged tile, fewer tiles than nsplit
        out.append(_case('small', d, 60, 'iso', n=60))
        out.append(_case('small', d, 12, 'iso', n=33))
        out.append(_case('small', d, 29, 'iso', n=129))
    return out


CASES = _cases()


def case_plan(c, long_lists=False):
    return plan(c.n, c.d, c.k, long_lists=long_lists, **dict(c.opts))


def case_id(c):
    return '-'.join([c.group, 'd%d' % c.d, 'k%d' % c.k, c.style] + (['n%d' % c.n] if c.n != N_MAIN else []) +
                    ['nsplit%d' % v for o, v in c.opts if o == 'nsplit'])
