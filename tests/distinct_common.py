"""What test_distinct_cpu.py and test_distinct_gpu.py share: the numpy model of vc_search_knn_distinct* in two independent formulations
-- the minimum packed value per label, and the round protocol over a brute-force sorted list -- and the crafted cases."""
import functools

import numpy as np

MAX_K = 8192
TRUNCATED = 0x80000000
INF = np.uint64(0xFFFFFFFFFFFFFFFF)
STALE = np.uint64(0xA5A5A5A5DEADBEEF)
STALE32 = np.uint32(0xDEADBEEF)
GIVE_UP = 0xFFFFFFFF
WAVE_MAX, BLOCK_MAX = 64, 1024            # the collapse kernel's size classes: k' <= 64, <= 1024, <= 8192
K_FIRSTS = lambda k: (k, 2 * k, 0, 8192)  # what the model formulations are compared under
_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint32)


def zero_stats():
    return {"n_rounds": 0, "k_last": 0, "n_searched": 0, "n_truncated": 0, "n_short": 0}


def first_k(k, k_first):
    return k_first if k_first else min(MAX_K, 2 * k)


def size_class(kp):
    return 0 if kp <= WAVE_MAX else 1 if kp <= BLOCK_MAX else 2


def sorted_lists(codes, queries, id_base=0):
    """per query the brute-force k-NN list of ALL records: packed dist << 32 | id, ascending"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    ids = np.arange(len(codes), dtype=np.uint64) + np.uint64(id_base)
    out = []
    for q in np.ascontiguousarray(queries, dtype=np.uint8).reshape(-1, codes.shape[1]):
        d = _POP8[codes ^ q[None, :]].sum(axis=1, dtype=np.uint64)
        out.append(np.sort(d << np.uint64(32) | ids))
    return out


def labels_of(packed, labels, id_base):
    return np.asarray(labels, dtype=np.uint32)[((packed & np.uint64(0xFFFFFFFF)) - np.uint64(id_base)).astype(np.int64)]


def _finish(rows, rls, counts, i, kept, kept_labels, k, count):
    w = min(len(kept), k)
    rows[i, :w], rls[i, :w], counts[i] = kept[:w], kept_labels[:w], count


def _blank(nq, k):
    return np.full((nq, k), INF, dtype=np.uint64), np.zeros((nq, k), dtype=np.uint32), np.zeros(nq, dtype=np.uint32)


# ---- formulation 1: the minimum packed value per label, sorted, cut to k ---------------------------------------------------------------
def _heads(packed, labs):
    uniq, inv = np.unique(labs, return_inverse=True)
    heads = np.full(len(uniq), INF, dtype=np.uint64)
    np.minimum.at(heads, inv.reshape(-1), packed)
    order = np.argsort(heads, kind="stable")
    return heads[order], uniq[order].astype(np.uint32)


def heads_model(lists, labels, k, id_base=0):
    """(rows, row_labels, counts, n_truncated, n_short): the k smallest heads; a query whose k-th head does not lie among its 8192
    nearest records gets the heads of those 8192 and the flag, unless the database has fewer than 8192 records (then: every group)"""
    rows, rls, counts = _blank(len(lists), k)
    n_trunc = n_short = 0
    for i, L in enumerate(lists):
        heads, hl = _heads(L, labels_of(L, labels, id_base))
        if len(heads) >= k and np.searchsorted(L, heads[k - 1]) < MAX_K:
            _finish(rows, rls, counts, i, heads, hl, k, k)
        elif len(L) < MAX_K:
            _finish(rows, rls, counts, i, heads, hl, k, len(heads))
            n_short += 1
        else:
            heads, hl = _heads(L[:MAX_K], labels_of(L[:MAX_K], labels, id_base))
            _finish(rows, rls, counts, i, heads, hl, k, len(heads) | TRUNCATED)
            n_trunc += 1
    return rows, rls, counts, n_trunc, n_short


# ---- formulation 2: the round protocol over the sorted list ----------------------------------------------------------------------------
def sure_entries(L, kp, tie_cut):
    """how many of the first k' entries of a list count.  All that are there -- unless the search underneath is exact MIH (tie_cut),
    the row is full and a wider one can be asked for: its rows hold every record nearer than their last distance D but only some of
    the ties at D, so only the entries nearer than D are sure."""
    cnt = min(kp, len(L))
    if tie_cut and cnt == kp and kp < MAX_K:
        return int(np.searchsorted(L >> np.uint64(32), L[kp - 1] >> np.uint64(32), side="left"))
    return cnt


def protocol_model(lists, labels, k, k_first=0, id_base=0, tie_cut=False):
    """(rows, row_labels, counts, stats, trace): the rounds as the header states them; trace = per round (k', queries searched,
    {query: d} of the queries that went on).  tie_cut: VC_MODE_MIH_EXACT underneath (see sure_entries)"""
    nq = len(lists)
    rows, rls, counts = _blank(nq, k)
    st = zero_stats()
    if nq and len(lists[0]) == 0:
        return rows, rls, counts, st, []
    firsts = []
    for L in lists:                                   # the positions of the first occurrences in the whole list, ascending
        labs = labels_of(L, labels, id_base)
        firsts.append(np.sort(np.unique(labs, return_index=True)[1]))
    todo, kp, trace = list(range(nq)), first_k(k, k_first), []
    while todo:
        st["n_rounds"] += 1
        st["k_last"] = kp
        st["n_searched"] += len(todo)
        again = {}
        for i in todo:
            L, cnt = lists[i], min(kp, len(lists[i]))
            pos = firsts[i][:np.searchsorted(firsts[i], sure_entries(L, kp, tie_cut))]
            d = len(pos)
            kept, kl = L[pos], labels_of(L[pos], labels, id_base)
            if d >= k:
                _finish(rows, rls, counts, i, kept, kl, k, k)
            elif cnt < kp:
                _finish(rows, rls, counts, i, kept, kl, k, d)
                st["n_short"] += 1
            elif kp >= MAX_K:
                _finish(rows, rls, counts, i, kept, kl, k, d | TRUNCATED)
                st["n_truncated"] += 1
            else:
                again[i] = d
        trace.append((kp, len(todo), again))
        todo, kp = sorted(again), min(MAX_K, 2 * kp)
    return rows, rls, counts, st, trace


def walk(L, labs, kp, k, tie_cut=False):
    """plain loop, for small inputs: the kept entries of the first kp of the list, their labels, how many entries the search returned"""
    seen, kept, kl = set(), [], []
    cnt = min(kp, len(L))
    for j in range(cnt):
        if tie_cut and cnt == kp and kp < MAX_K and int(L[j]) >> 32 >= int(L[kp - 1]) >> 32:
            break
        if int(labs[j]) not in seen:
            seen.add(int(labs[j]))
            kept.append(int(L[j]))
            kl.append(int(labs[j]))
    return kept, kl, cnt


def same_run(got, want, what=None):
    """(rows, row_labels, counts[, stats]) against the model's, every word"""
    for name, g, w in zip(("rows", "row_labels", "counts"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[0]
            assert False, (what, name, "first difference at", tuple(bad), g[tuple(bad)], w[tuple(bad)])
    if len(got) > 3 and got[3] is not None:
        assert got[3] == want[3], (what, "stats", got[3], want[3])


def reverse_valid(rows, rls, counts):
    """VC_ORDER_FARTHEST_FIRST: the valid part of every row, and of its labels, turned round"""
    rows, rls = rows.copy(), rls.copy()
    for i, c in enumerate(counts):
        v = int(c) & ~TRUNCATED
        rows[i, :v], rls[i, :v] = rows[i, :v][::-1].copy(), rls[i, :v][::-1].copy()
    return rows, rls


# ---- the crafted cases -----------------------------------------------------------------------------------------------------------------
def _flip(rng, code, n_flips):
    out = code.copy()
    for b in rng.choice(len(code) * 8, size=n_flips, replace=False):
        out[b // 8] ^= np.uint8(1 << (b % 8))
    return out


# (centres, copies per centre) of the families of a duplicate-heavy store.  A query at a centre of a family first sees centres x copies
# records of `centres` groups; with k = 10 and k' = 20, 40, 80, 160, 320 the families end in rounds 0, 1, 2, 3 and 4.
FAMILIES = ((12, 1), (6, 5), (5, 14), (4, 35), (7, 40))
DUP_K = 10


@functools.lru_cache(maxsize=None)
def dup_case(bits, n_queries=257, seed=5):
    """(codes, labels, queries): two instances of every family and 1500 singletons, shuffled.  Family members lie within 6 bits of
    their family's code, copies within 1 bit of their centre; the labels are the centre's number + 100."""
    rng = np.random.default_rng(seed + bits)
    nbytes = bits // 8
    codes, labels, centres, group = [], [], [], 100
    for inst in range(2):
        for n_centres, copies in FAMILIES:
            fam = rng.integers(0, 256, size=nbytes, dtype=np.uint8)
            for _ in range(n_centres):
                centre = _flip(rng, fam, 3)
                centres.append(centre)
                for c in range(copies):
                    codes.append(centre if c == 0 else _flip(rng, centre, 1))
                    labels.append(group)
                group += 1
    for _ in range(1500):
        codes.append(rng.integers(0, 256, size=nbytes, dtype=np.uint8))
        labels.append(group)
        group += 1
    order = rng.permutation(len(codes))
    codes, labels = np.array(codes, dtype=np.uint8)[order], np.array(labels, dtype=np.uint32)[order]
    picks = [centres[i % len(centres)] for i in range(n_queries - 40)] + [codes[i] for i in rng.integers(0, len(codes), size=40)]
    queries = np.array([_flip(rng, c, 1) for c in picks], dtype=np.uint8)
    return codes, labels, queries


def hostile_values(n):
    """n distinct label values: the extremes, values that differ only above bit 16, only in the low 4 bits, only in one high bit"""
    vals = [0, 0xFFFFFFFF, 0xFFFFFFFE, 1, 0x80000000, 0x7FFFFFFF]
    vals += [0x12345670 + j for j in range(16)]
    vals += [(j << 16) | 0xBEEF for j in range(1, 1 + n)]
    vals += [(j << 28) | (j << 4) for j in range(1, 16)]
    seen, out = set(), []
    for v in vals:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return np.array(out[:n], dtype=np.uint32)


def hostile_labels(labels):
    """the same partition under hostile values: the groups in order of their size, the largest first, get hostile_values in turn"""
    uniq, inv, size = np.unique(labels, return_inverse=True, return_counts=True)
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[np.argsort(-size, kind="stable")] = np.arange(len(uniq))
    return hostile_values(len(uniq))[rank][inv.reshape(-1)]


@functools.lru_cache(maxsize=None)
def truncation_case(bits=64):
    """(codes, labels, queries): N = 9000 -- 8600 records of label 5 within distance 2 of a base code, 400 records at distance >= 20
    with labels of their own; three queries within distance 1 of the base"""
    rng = np.random.default_rng(77 + bits)
    nbytes = bits // 8
    base = rng.integers(0, 256, size=nbytes, dtype=np.uint8)
    codes = [_flip(rng, base, int(rng.integers(0, 3))) for _ in range(8600)] + [_flip(rng, base, int(rng.integers(20, 40))) for _ in range(400)]
    labels = [5] * 8600 + [1000 + i for i in range(400)]
    order = rng.permutation(9000)
    queries = np.array([base, _flip(rng, base, 1), _flip(rng, base, 1)], dtype=np.uint8)
    return np.array(codes, dtype=np.uint8)[order], np.array(labels, dtype=np.uint32)[order], queries


@functools.lru_cache(maxsize=None)
def ties_case(bits=64):
    """(codes, labels, queries): the query is 0; 64 records at distance 1 (labels i % 5, in an order that is not the ids'), 200 at
    distance 2 (labels 5 + j % 7 and, every third, one of the first five), 16 at distance 0 with two labels"""
    rng = np.random.default_rng(9)
    nbytes = bits // 8
    zero = np.zeros(nbytes, dtype=np.uint8)
    codes, labels = [], []
    for i in rng.permutation(64):
        c = zero.copy()
        c[i // 8] |= np.uint8(1 << (i % 8))
        codes.append(c)
        labels.append(int(i) % 5)
    for j in range(200):
        codes.append(_flip(rng, zero, 2))
        labels.append(j % 5 if j % 3 == 0 else 5 + j % 7)
    for j in range(16):
        codes.append(zero.copy())
        labels.append(50 + (j & 1))
    order = rng.permutation(len(codes))
    queries = np.array([zero, _flip(rng, zero, 1)], dtype=np.uint8)
    return np.array(codes, dtype=np.uint8)[order], np.array(labels, dtype=np.uint32)[order], queries


@functools.lru_cache(maxsize=None)
def dup_lists(bits, id_base=0):
    codes, _, queries = dup_case(bits)
    return sorted_lists(codes, queries, id_base)


@functools.lru_cache(maxsize=None)
def dup_expect(bits, k=DUP_K, k_first=0, id_base=0, hostile=False, tie_cut=False):
    labels = dup_case(bits)[1]
    return protocol_model(dup_lists(bits, id_base), hostile_labels(labels) if hostile else labels, k, k_first, id_base, tie_cut)


@functools.lru_cache(maxsize=None)
def truncation_lists(bits=64):
    codes, _, queries = truncation_case(bits)
    return sorted_lists(codes, queries)


def rounds_of(trace, nq):
    """per query the number of rounds it took part in"""
    r = np.zeros(nq, dtype=np.int64)
    alive = set(range(nq))
    for _, _, again in trace:
        for i in alive:
            r[i] += 1
        alive = set(again)
    return r
