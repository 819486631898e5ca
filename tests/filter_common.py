"""What test_filter_cpu.py and test_filter_gpu.py share: the numpy model of vc_search_knn_filtered* -- per query the brute-force sorted
list of packed values over the ALLOWED records, and the post-filter round protocol (with and without the tie cut of exact MIH) with
the plan's route, schedule, windows and sub-batches for the statistics -- and the crafted cases."""
import functools

import numpy as np

import distinct_common as DC

MAX_K = 8192
POST_MAX_K = 199                  # VC_FILTER_POST_MAX_K
SCRATCH = 64 << 20                # VC_FILTER_SCRATCH's default
WINDOW = 1 << 20                  # VC_FILTER_WINDOW's default
MASK, ROOTS, EQUAL, NOT_EQUAL, BITS = 0, 1, 2, 3, 4
RAN_POST, RAN_PRE = 1, 2
INF, STALE, STALE32 = DC.INF, DC.STALE, DC.STALE32
STAT_NAMES = ("n_allowed", "routes", "n_rounds", "k_last", "n_windows", "n_searched", "n_fallback", "n_short")


def zero_stats():
    return {name: 0 for name in STAT_NAMES}


# ---- the filter -------------------------------------------------------------------------------------------------------------------------
def allowed_of(sel, kind, value, n, id_base=0):
    """the boolean mask over the n records that `sel` means under `kind`"""
    sel = np.asarray(sel, dtype=np.uint32)
    i = np.arange(n, dtype=np.uint64)
    if kind == MASK:
        return sel[:n] != 0
    if kind == ROOTS:
        return sel[:n] == ((i + np.uint64(id_base)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    if kind == EQUAL:
        return sel[:n] == np.uint32(value)
    if kind == NOT_EQUAL:
        return sel[:n] != np.uint32(value)
    assert kind == BITS
    return ((sel[(i >> np.uint64(5)).astype(np.int64)] >> (i & np.uint64(31)).astype(np.uint32)) & np.uint32(1)) != 0


def sel_for(allowed, kind, id_base=0, value=0, other=None, junk=0):
    """a `sel` array that means `allowed` under `kind`.  other: the values of the records on the far side of EQUAL / NOT_EQUAL (all
    != value) and of the ROOTS non-representatives; junk: ORed into the bits of the last BITS word past N"""
    allowed = np.asarray(allowed, dtype=bool)
    n = len(allowed)
    if kind == MASK:
        return np.where(allowed, np.uint32(1) if other is None else other, np.uint32(0)).astype(np.uint32)
    if kind == ROOTS:
        own = (np.arange(n, dtype=np.uint64) + np.uint64(id_base)).astype(np.uint32)
        return np.where(allowed, own, own + np.uint32(1) if other is None else other).astype(np.uint32)
    if kind in (EQUAL, NOT_EQUAL):
        far = np.full(n, (value + 1) & 0xFFFFFFFF, dtype=np.uint32) if other is None else np.asarray(other, dtype=np.uint32)
        assert np.all(far != np.uint32(value))
        return np.where(allowed == (kind == EQUAL), np.uint32(value), far).astype(np.uint32)
    words = np.zeros((n + 31) // 32, dtype=np.uint32)
    idx = np.nonzero(allowed)[0]
    np.bitwise_or.at(words, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    if n % 32 and len(words):
        words[-1] |= np.uint32(junk) & ~np.uint32((1 << (n % 32)) - 1)
    return words


# ---- the rule -----------------------------------------------------------------------------------------------------------------------------
def allowed_lists(lists, allowed, id_base=0):
    """per query the sorted list cut down to the allowed records"""
    allowed = np.asarray(allowed, dtype=bool)
    return [L[allowed[((L & np.uint64(0xFFFFFFFF)) - np.uint64(id_base)).astype(np.int64)]] for L in lists]


def model_rows(lists, allowed, k, id_base=0):
    """(rows [nq, k] uint64, counts [nq] uint32): the k smallest packed values over the allowed records, padded"""
    nq = len(lists)
    rows, counts = np.full((nq, k), INF, dtype=np.uint64), np.zeros(nq, dtype=np.uint32)
    for i, L in enumerate(allowed_lists(lists, allowed, id_base)):
        w = min(k, len(L))
        rows[i, :w], counts[i] = L[:w], w
    return rows, counts


# ---- the plan (vc_filter_plan.hpp) ----------------------------------------------------------------------------------------------------------
def expected_k(k, N, A):
    return (k * N + A - 1) // A


def route_of(k, N, A, knob=0):
    if knob in (1, 2):
        return knob
    return RAN_POST if 2 * expected_k(k, N, A) <= POST_MAX_K else RAN_PRE


def first_k(k, k_first, N, A):
    return k_first if k_first else max(k, min(MAX_K, 2 * expected_k(k, N, A)))


def steps(W):
    return {1: 8, 2: 4, 4: 2, 8: 1}[W]


def slice_len(W):
    return 64 * steps(W)


def n_slices(n, W):
    return (n + slice_len(W) - 1) // slice_len(W)


def pre_scans(A, nq, W, window=WINDOW, scratch=SCRATCH):
    """window scans of the pre-filter route for nq queries: windows x sub-batches"""
    per = max(1, min(nq, scratch // (8 * max(1, n_slices(min(A, window), W)))))
    return ((A + window - 1) // window) * ((nq + per - 1) // per)


def sure_entries(L, kp, tie_cut):
    """how many of the first k' entries count: under exact MIH (tie_cut) a full row counts only below its last distance, at EVERY k'"""
    cnt = min(kp, len(L))
    if tie_cut and cnt == kp:
        return int(np.searchsorted(L >> np.uint64(32), L[kp - 1] >> np.uint64(32), side="left"))
    return cnt


def stats_model(lists, allowed, k, k_first=0, id_base=0, tie_cut=False, route=0, W=1, window=WINDOW, scratch=SCRATCH):
    """(stats, trace): what the call reports; trace = per post-filter round (k', queries searched, queries that went on)"""
    allowed = np.asarray(allowed, dtype=bool)
    nq, N, A = len(lists), len(allowed), int(np.count_nonzero(allowed))
    st = zero_stats()
    if N == 0:
        return st, []
    st["n_allowed"], st["n_short"] = A, nq if A < k else 0
    if A == 0:
        return st, []
    if route_of(k, N, A, route) == RAN_PRE:
        st["routes"], st["n_windows"] = RAN_PRE, pre_scans(A, nq, W, window, scratch)
        return st, []
    st["routes"] = RAN_POST
    todo, kp, trace = list(range(nq)), first_k(k, k_first, N, A), []
    while todo:
        st["n_rounds"] += 1
        st["k_last"] = kp
        st["n_searched"] += len(todo)
        again = []
        for i in todo:
            L = lists[i]
            cnt = min(kp, len(L))
            head = L[:sure_entries(L, kp, tie_cut)]
            kept = int(np.count_nonzero(allowed[((head & np.uint64(0xFFFFFFFF)) - np.uint64(id_base)).astype(np.int64)]))
            if kept < k and cnt >= kp:
                again.append(i)
        trace.append((kp, len(todo), list(again)))
        todo = again
        if todo and kp >= MAX_K:
            st["n_fallback"] = len(todo)
            st["routes"] |= RAN_PRE
            st["n_windows"] = pre_scans(A, len(todo), W, window, scratch)
            break
        kp = min(MAX_K, 2 * kp)
    return st, trace


def model(lists, allowed, k, **kw):
    """(rows, counts, stats)"""
    rows, counts = model_rows(lists, allowed, k, kw.get("id_base", 0))
    return rows, counts, stats_model(lists, allowed, k, **kw)[0]


def same_run(got, want, what=None):
    """(rows, counts[, stats]) against the model's, every word"""
    for name, g, w in zip(("rows", "counts"), got, want):
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[0]
            assert False, (what, name, "first difference at", tuple(bad), g[tuple(bad)], w[tuple(bad)])
    if len(got) > 2 and got[2] is not None and len(want) > 2:
        assert got[2] == want[2], (what, "stats", got[2], want[2])


def reverse_valid(rows, counts):
    rows = rows.copy()
    for i, c in enumerate(counts):
        rows[i, :int(c)] = rows[i, :int(c)][::-1].copy()
    return rows


# ---- plain loops, for small inputs ------------------------------------------------------------------------------------------------------------
def loop_rows(codes, queries, allowed, k, id_base=0):
    out, counts = [], []
    for q in queries:
        best = []
        for i, c in enumerate(codes):
            if allowed[i]:
                d = sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(c, q))
                best.append((d << 32) | (id_base + i))
        best.sort()
        out.append(best[:k] + [int(INF)] * (k - min(k, len(best))))
        counts.append(min(k, len(best)))
    return np.array(out, dtype=np.uint64).reshape(len(queries), k), np.array(counts, dtype=np.uint32)


# ---- the crafted cases ----------------------------------------------------------------------------------------------------------------------
def random_mask(n, one_in, seed):
    """about n / one_in records allowed, at least one"""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, one_in, size=n) == 0
    m[int(rng.integers(0, n))] = True
    return m


@functools.lru_cache(maxsize=None)
def uniform_case(bits, n=4000, nq=37, seed=1):
    rng = np.random.default_rng(seed + bits)
    return rng.integers(0, 256, size=(n, bits // 8), dtype=np.uint8), rng.integers(0, 256, size=(nq, bits // 8), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def tie_case(bits, A, seed=3):
    """(codes, allowed, queries, k): 2 A records, the odd ids allowed, record 2 p a DISALLOWED copy of record 2 p + 1.  List position
    p is at distance 1 (one in eight), 3 (one in eight) or 2 (the tie group, everywhere in the list) of the zero code, from few
    distinct codes; k takes the distance-1 records and about half of the ties.  The second query is one bit off the first."""
    rng = np.random.default_rng(seed + bits + A)
    nbytes = bits // 8
    pool = {d: [] for d in (1, 2, 3)}
    for d in pool:
        for _ in range(3):
            c = np.zeros(nbytes, dtype=np.uint8)
            for b in rng.choice(16, size=d, replace=False):
                c[b // 8] |= np.uint8(1 << (b % 8))
            pool[d].append(c)
    dist = np.where(np.arange(A) % 8 == 3, 1, np.where(np.arange(A) % 8 == 6, 3, 2))
    dist = dist[rng.permutation(A)] if A > 8 else dist
    codes = np.zeros((2 * A, nbytes), dtype=np.uint8)
    for p in range(A):
        codes[2 * p] = codes[2 * p + 1] = pool[int(dist[p])][int(rng.integers(0, 3))]
    allowed = np.arange(2 * A) % 2 == 1
    n1, n2 = int(np.count_nonzero(dist == 1)), int(np.count_nonzero(dist == 2))
    queries = np.zeros((2, nbytes), dtype=np.uint8)
    queries[1, nbytes - 1] = 0x80
    return codes, allowed, queries, n1 + max(1, n2 // 2)


def tie_reach(bits, A):
    """on the model alone: (ties at the k-th distance of query 0, how many of them the row takes, the wave-slices the taken ones lie in)"""
    codes, allowed, queries, k = tie_case(bits, A)
    L = allowed_lists(DC.sorted_lists(codes, queries[:1]), allowed)[0]
    dk = int(L[k - 1] >> np.uint64(32))
    d = (L >> np.uint64(32)).astype(np.int64)
    ties, below = int(np.count_nonzero(d == dk)), int(np.count_nonzero(d < dk))
    taken_ids = (L[below:k] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    positions = (taken_ids - 1) // 2                 # list position of allowed id 2 p + 1
    return ties, k - below, sorted(set((positions // slice_len(bits // 64)).tolist()))


@functools.lru_cache(maxsize=None)
def fallback_case():
    """distinct_common.truncation_case() under NOT_EQUAL 5: (codes, sel, queries, allowed) -- the 8600 nearest records are disallowed"""
    codes, labels, queries = DC.truncation_case()
    return codes, labels, queries, labels != 5
