"""Host restatement of the SHAPE of the sliced-ELL plan glx_graph_plan builds (csrc/graph.hip:679-916), in plain numpy: which rows
go to which slots of which slice, and the counts glx_graph_info reports.  No GPU, no library call.  tests/test_sell_plan_host.py
holds it on the fixtures of tests/test_gpu_big_state.py, which compares `nslices` and `stored` with DeviceGraph.info().

What it states, with the lines of csrc/graph.hip it restates:

    big state (711-712)   n_cols * G * 4 * esize >= 32 MiB: the row classes are 64 / 256 entries instead of 24 / 96 (697); relaxed
                          plans use 64 / 256 always (707); plans of G != 4 have one class (716; relaxed exists at G = 4 only, 680)
    class of a row (722)  16 slots above L4 entries, 4 above L1, else 1
    ranges (730-744)      eight contiguous ranges of equal work, work of a row = entries + 3; fewer than 8 rows: equal counts
    order (762-784)       big state and more than 32 768 rows in the range: the rows of class 4 / 16 first, longest first (stable), then
                          the others sorted by decreasing length (stable: a counting sort) inside windows of 32 768 consecutive ones;
                          otherwise the whole range is one window and nothing is pulled out
    slices (785-809)      walking the order: a slice takes up to R / S rows of the class S of its first row, S slots each;
                          nchunks = ceil(longest / (4 S)) at G = 4, ceil(longest / G) otherwise; full = shortest // (4 S), an empty
                          slot counting as length 0 (G = 4 only)
    reorder (814-835)     unless a range so far was windowed: slices by decreasing nchunks * cost(S), stable; cost 4 / 8 / 12 for
                          S = 1 / 4 / 16, 4 for every class of a relaxed plan
    padding (838-861)     every range padded with empty slices to the same number of 4-slice blocks;
                          stored = 64 * (nslices + sum over slices of max(nchunks - 1, 0))

`replay` puts the image together again from the slot map the way sell_fill_kernel deals entries to slots (csrc/graph.hip:629-669)
and multiplies: a plan that drops or repeats a row, or a slot that holds the wrong entries, gives another product than A @ u."""
import numpy as np
from scipy import sparse

SIGMA = 32768
NX = 8
WPB = 4
ROW_COST = 3
WINDOW_MIN_BYTES = 32 * 1024 * 1024


def classes(n_cols, G, esize, relaxed=False):
    """(big_state, relaxed, L1, L4)"""
    if G != 4:
        relaxed = False
    big = float(n_cols) * G * 4.0 * esize >= WINDOW_MIN_BYTES
    L1, L4 = (64, 256) if (relaxed or big) else (24, 96)
    if G != 4:
        L1 = L4 = 1 << 30
    return big, relaxed, L1, L4


def klass(lens, L1, L4):
    lens = np.asarray(lens)
    return np.where(lens > L4, 16, np.where(lens > L1, 4, 1))


def ranges(lens):
    """xb[0..8]: range x holds the rows xb[x] .. xb[x + 1] - 1"""
    n = len(lens)
    xb = np.zeros(NX + 1, dtype=np.int64)
    xb[NX] = n
    if n < NX:
        for x in range(1, NX):
            xb[x] = n * x // NX
        return xb
    cum = np.cumsum(np.asarray(lens, dtype=np.int64) + ROW_COST)
    total = int(cum[-1])
    for x in range(1, NX):
        want = total * x // NX
        # the first i with cum[i - 1] >= want (the loop adds rows while the sum is below `want`)
        xb[x] = 0 if want <= 0 else min(n, int(np.searchsorted(cum, want, side='left')) + 1)
    return xb


def _by_length(rows, lens):
    return rows[np.argsort(-lens[rows], kind='stable')]


def range_order(lens, b0, b1, big, L1, L4, perturb=None):
    """(order, nlong, windows, windowed) of the rows b0 .. b1 - 1.  perturb='drop_nlong' restates a WRONG plan, for the test of
    the tests: the windows are placed from position 0 instead of behind the split rows."""
    m = b1 - b0
    rows = np.arange(b0, b1, dtype=np.int64)
    sigma = SIGMA if big else m
    if not sigma < m:
        return _by_length(rows, lens), 0, (1 if m else 0), False
    k = klass(lens[rows], L1, L4)
    lng = _by_length(rows[k > 1], lens)
    rest = rows[k == 1]
    nlong = len(lng)
    order = np.zeros(m, dtype=np.int64)      # (the library's vector starts from zeros too)
    order[:nlong] = lng
    at = 0 if perturb == 'drop_nlong' else nlong
    windows = 0
    for w0 in range(0, m - nlong, sigma):
        w1 = min(m - nlong, w0 + sigma)
        order[at + w0:at + w1] = _by_length(rest[w0:w1], lens)
        windows += 1
    return order, nlong, windows, True


def range_slices(order, lens, G, L1, L4):
    """The slices of one range in the order they are cut: (S, nchunks, full, count, start): slice q holds the rows
    order[start[q] : start[q] + count[q]]."""
    R = 64 // G
    m = len(order)
    if m == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z, z, z
    ol = lens[order].astype(np.int64)
    k = klass(ol, L1, L4).astype(np.int64)
    run_start = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
    run_len = np.diff(np.concatenate([run_start, [m]]))
    per = R // k[run_start]                                   # rows per slice in the run
    nsl = (run_len + per - 1) // per
    run_of = np.repeat(np.arange(len(run_start)), nsl)
    j = np.arange(len(run_of)) - np.repeat(np.cumsum(nsl) - nsl, nsl)
    start = run_start[run_of] + j * per[run_of]
    count = np.minimum(per[run_of], run_start[run_of] + run_len[run_of] - start)
    S = k[start]
    width = np.maximum.reduceat(ol, start)
    narrow = np.where(count < per[run_of], 0, np.minimum.reduceat(ol, start))      # an empty slot has length 0
    if G == 4:
        nchunks = (width + 4 * S - 1) // (4 * S)
        full = narrow // (4 * S)
    else:
        nchunks = (width + G - 1) // G
        full = np.zeros_like(nchunks)
    return S, nchunks, full, count, start


def plan(lens, n_cols, G, esize, relaxed=False, perturb=None):
    """lens: row lengths in plan order (the caller's with keep_order, lens[G.order()] otherwise)."""
    lens = np.asarray(lens, dtype=np.int64)
    R = 64 // G
    big, relaxed, L1, L4 = classes(n_cols, G, esize, relaxed)
    xb = ranges(lens)
    windowed = False
    per_range, info = [], []
    for x in range(NX):
        b0, b1 = int(xb[x]), int(xb[x + 1])
        order, nlong, windows, w = range_order(lens, b0, b1, big, L1, L4, perturb)
        windowed = windowed or w
        S, nchunks, full, count, start = range_slices(order, lens, G, L1, L4)
        if not windowed:
            cost = nchunks * (4 if relaxed else np.where(S == 1, 4, np.where(S == 4, 8, 12)))
            idx = np.argsort(-cost, kind='stable')
            S, nchunks, full, count, start = S[idx], nchunks[idx], full[idx], count[idx], start[idx]
        per_range.append((order, S, nchunks, full, count, start))
        one = nchunks[S == 1]
        info.append(dict(rows=b1 - b0, first=b0, nlong=nlong, windows=windows, order=order, classes=set(S.tolist()),
                         max_nchunks=int(nchunks.max()) if len(nchunks) else 0, max_nchunks_one_slot=int(one.max()) if len(one) else 0,
                         slices=len(S)))
    bpx = max((len(p[1]) + WPB - 1) // WPB for p in per_range)
    spx = bpx * WPB
    nslices = spx * NX
    slot_row = np.full(nslices * R, -1, dtype=np.int64)
    slot_len = np.zeros(nslices * R, dtype=np.int64)
    hS = np.ones(nslices, dtype=np.int64)
    hn = np.zeros(nslices, dtype=np.int64)
    hf = np.zeros(nslices, dtype=np.int64)
    for x, (order, S, nchunks, full, count, start) in enumerate(per_range):
        ns = len(S)
        hS[x * spx:x * spx + ns], hn[x * spx:x * spx + ns], hf[x * spx:x * spx + ns] = S, nchunks, full
        if ns == 0:
            continue
        # row j of slice q sits in the slots j S .. j S + S - 1 of the slice
        q = np.repeat(np.arange(ns), count * S)
        within = np.arange(len(q)) - np.repeat(np.cumsum(count * S) - count * S, count * S)
        row = order[np.repeat(start, count * S) + within // np.repeat(S, count * S)]
        at = (x * spx + q) * R + within
        slot_row[at] = row
        slot_len[at] = lens[row]
    stored = 64 * (nslices + int(np.maximum(hn - 1, 0).sum()))
    return dict(G=G, R=R, big=big, relaxed=relaxed, L1=L1, L4=L4, windowed=windowed, xb=xb, nslices=int(nslices), stored=stored,
                ranges=info, slot_row=slot_row, slot_len=slot_len, S=hS, nchunks=hn, full=hf)


def slot_entries(p):
    """(slot, jj) for every entry the image holds: slot w / G of a slice holds, in chunk k at lane t, entry
    jj = (k S + seg) 4 + t of its row at G = 4 (seg = slot & (S - 1)) and jj = k G + t otherwise, where jj < len."""
    G, R = p['G'], p['R']
    slots = np.flatnonzero(p['slot_row'] >= 0)
    sl = slots // R
    S, nch = p['S'][sl], p['nchunks'][sl]
    seg = (slots % R) & (S - 1)
    per = nch * G                                           # (k, t) pairs of a slot
    which = np.repeat(np.arange(len(slots)), per)
    kt = np.arange(len(which)) - np.repeat(np.cumsum(per) - per, per)
    k, t = kt // G, kt % G
    jj = (k * S[which] + seg[which]) * 4 + t if G == 4 else k * G + t
    keep = jj < p['slot_len'][slots][which]
    return slots[which][keep], jj[keep]


def replay(p, A, u):
    """The product as the image of plan `p` gives it: every group of S slots yields one row sum, over the entries its slots hold in
    increasing jj, and WRITES it to its row; a row no group holds stays NaN.  A in plan order, stored order kept."""
    R = p['R']
    slot, jj = slot_entries(p)
    sl = slot // R
    group = sl * R + (slot % R) // p['S'][sl] * p['S'][sl]      # the first slot of the row's S slots
    row = p['slot_row'][slot]
    o = np.lexsort((jj, group))
    group, jj, row = group[o], jj[o], row[o]
    gid, first, counts = np.unique(group, return_index=True, return_counts=True)
    indptr = np.concatenate([[0], np.cumsum(counts)])
    src = A.indptr[row].astype(np.int64) + jj
    M = sparse.csr_matrix((A.data[src], A.indices[src], indptr), shape=(len(gid), A.shape[1]))
    M.has_sorted_indices = False
    out = np.full((A.shape[0],) + u.shape[1:], np.nan, dtype=u.dtype)
    out[row[first]] = M @ u
    # rows without entries: their slots write the empty sum
    empty = p['slot_row'][(p['slot_row'] >= 0) & (p['slot_len'] == 0)]
    out[empty] = 0
    return out
