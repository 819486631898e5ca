"""What test_scope_cpu.py and test_scope_gpu.py share: the numpy model of vc_search_knn_scoped* -- per query the brute-force sorted list
of distinct_common.sorted_lists restricted to scope == qscope[q] and cut at k, the statistics from their definitions with the plan of
vc_scope_plan.hpp (segments, counters, sub-batches, windows) -- and the crafted cases."""
import functools

import numpy as np

import distinct_common as DC
import filter_common as FC

MAX_K = 8192
SCRATCH = 64 << 20                # VC_SCOPE_SCRATCH's default
WINDOW = 1 << 20                  # VC_SCOPE_WINDOW's default
WINDOW_MAX = 1 << 24
COUNTER_BYTES = 8                 # VC_SCOPE_COUNTER_BYTES
MAX_COUNTERS = 1 << 28            # VC_SCOPE_MAX_COUNTERS
INF, STALE, STALE32 = DC.INF, DC.STALE, DC.STALE32
STAT_NAMES = ("n_matched", "n_pairs", "n_scopes", "n_windows", "n_short", "n_empty")
slice_len = FC.slice_len


def zero_stats():
    return {name: 0 for name in STAT_NAMES}


# ---- the rule -----------------------------------------------------------------------------------------------------------------------------
def model_rows(lists, scope, qscope, k, id_base=0):
    """(rows [nq, k] uint64, counts [nq] uint32): per query the k smallest packed values over the records of its own scope, padded"""
    scope, qscope = np.asarray(scope, dtype=np.uint32), np.asarray(qscope, dtype=np.uint32)
    nq = len(lists)
    rows, counts = np.full((nq, k), INF, dtype=np.uint64), np.zeros(nq, dtype=np.uint32)
    for i, L in enumerate(lists):
        own = L[scope[((L & np.uint64(0xFFFFFFFF)) - np.uint64(id_base)).astype(np.int64)] == qscope[i]] if len(scope) else L[:0]
        w = min(k, len(own))
        rows[i, :w], counts[i] = own[:w], w
    return rows, counts


# ---- the plan (vc_scope_plan.hpp) -----------------------------------------------------------------------------------------------------------
def window_of(knob):
    return WINDOW if knob == 0 or knob > WINDOW_MAX else knob


def key_bits(U):
    return max(0, int(U - 1).bit_length())


def segments(scope, qscope):
    """(uniq [U] ascending, seg [U + 1], order [nq] the queries sorted stably by scope, slot [nq] of the SORTED queries)"""
    scope, qscope = np.asarray(scope, dtype=np.uint32), np.asarray(qscope, dtype=np.uint32)
    uniq = np.unique(qscope)
    sizes = np.array([int(np.count_nonzero(scope == u)) for u in uniq], dtype=np.int64)
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    order = np.argsort(qscope, kind="stable")
    return uniq, seg, order, np.searchsorted(uniq, qscope[order])


def slices_of(a, b, ln):
    return (b - 1) // ln - a // ln + 1


def cost(lo, hi, window, ln):
    """(query, slice) counters of a segment: the slices it touches, window after window"""
    if hi <= lo:
        return 0
    wa, wb = lo // window, (hi - 1) // window
    if wa == wb:
        return slices_of(lo - wa * window, hi - wa * window, ln)
    return slices_of(lo - wa * window, window, ln) + (wb - wa - 1) * ((window + ln - 1) // ln) + slices_of(0, hi - wb * window, ln)


def batches(costs, scratch):
    """[(b0, b1)] of the sorted queries: counters under the budget, always one query"""
    cap, out, b0, n = min(scratch // COUNTER_BYTES, MAX_COUNTERS), [], 0, len(costs)
    while b0 < n:
        total, b1 = costs[b0], b0 + 1
        while b1 < n and total + costs[b1] <= cap:
            total, b1 = total + costs[b1], b1 + 1
        out.append((b0, b1))
        b0 = b1
    return out


def n_windows_of(plo, phi, window):
    return (phi - 1) // window - plo // window + 1 if phi > plo else 0


def plan(scope, qscope, W=1, window=WINDOW, scratch=SCRATCH):
    """the plan of a call: dict(uniq, seg, order, slot, lo, hi [sorted queries], cost, batches, n_windows)"""
    window, ln = window_of(window), slice_len(W)
    uniq, seg, order, slot = segments(scope, qscope)
    lo, hi = seg[slot], seg[slot + 1]
    costs = [cost(int(a), int(b), window, ln) for a, b in zip(lo, hi)]
    bt = batches(costs, scratch)
    nw = sum(n_windows_of(int(lo[b0]), int(hi[b1 - 1]), window) for b0, b1 in bt)
    return dict(uniq=uniq, seg=seg, order=order, slot=slot, lo=lo, hi=hi, cost=costs, batches=bt, n_windows=nw, window=window, len=ln)


PLAN_CASES = ((1 << 20, 1, 64 << 20), (256, 1, 4096), (1000, 8, 64))      # (window, W, scratch) of tests/cpp/scope_plan_test.cc's CASE lines


def plan_scene():
    """the scene of those lines: 40 slots, slot u of 37 u^2 mod 1500 records and 1 + u mod 3 queries"""
    scope = np.concatenate([np.full(37 * u * u % 1500, u, dtype=np.uint32) for u in range(40)])
    qscope = np.concatenate([np.full(1 + u % 3, u, dtype=np.uint32) for u in range(40)])
    return scope, qscope


def stats_model(scope, qscope, k, W=1, window=WINDOW, scratch=SCRATCH):
    st = zero_stats()
    if len(scope) == 0:
        return st
    p = plan(scope, qscope, W, window, scratch)
    S = p["hi"] - p["lo"]
    st["n_scopes"], st["n_matched"] = len(p["uniq"]), int(p["seg"][-1])
    st["n_pairs"], st["n_short"], st["n_empty"] = int(S.sum()), int(np.count_nonzero(S < k)), int(np.count_nonzero(S == 0))
    st["n_windows"] = p["n_windows"] if st["n_matched"] else 0
    return st


def model(lists, scope, qscope, k, id_base=0, **kw):
    """(rows, counts, stats)"""
    rows, counts = model_rows(lists, scope, qscope, k, id_base)
    return rows, counts, stats_model(scope, qscope, k, **kw)


same_run = FC.same_run
reverse_valid = FC.reverse_valid


# ---- plain loops, for small inputs ------------------------------------------------------------------------------------------------------------
def loop_rows(codes, queries, scope, qscope, k, id_base=0):
    out, counts = [], []
    for q, qs in zip(queries, qscope):
        best = []
        for i, c in enumerate(codes):
            if int(scope[i]) == int(qs):
                d = sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(c, q))
                best.append((d << 32) | (id_base + i))
        best.sort()
        out.append(best[:k] + [int(INF)] * (k - min(k, len(best))))
        counts.append(min(k, len(best)))
    return np.array(out, dtype=np.uint64).reshape(len(queries), k), np.array(counts, dtype=np.uint32)


# ---- the crafted cases ----------------------------------------------------------------------------------------------------------------------
def _codes(rng, n, nbytes):
    return rng.integers(0, 256, size=(n, nbytes), dtype=np.uint8)


def lay_out(sizes, values, rng, strangers=0, stranger_values=()):
    """scope [N]: value values[i] on sizes[i] records, `strangers` records on stranger_values, all in a random record order"""
    parts = [np.full(s, v, dtype=np.uint32) for s, v in zip(sizes, values)]
    if strangers:
        parts.append(np.asarray(stranger_values, dtype=np.uint32)[rng.integers(0, len(stranger_values), size=strangers)])
    scope = np.concatenate(parts)
    return scope[rng.permutation(len(scope))]


@functools.lru_cache(maxsize=None)
def seven_case(bits, n=4000, nq=41, seed=5):
    """a random assignment into 7 scopes of very different sizes; every query names one of them"""
    rng = np.random.default_rng(seed + bits)
    values = np.array([3, 900, 17, 0x80000000, 5, 0xFFFFFFFF, 0], dtype=np.uint32)
    p = np.array([0.5, 0.25, 0.12, 0.08, 0.03, 0.015, 0.005])
    scope = values[rng.choice(7, size=n, p=p)]
    qscope = values[rng.integers(0, 7, size=nq)]
    return _codes(rng, n, bits // 8), _codes(rng, nq, bits // 8), scope, qscope


def edge_sizes(bits, k):
    ln = slice_len(bits // 64)
    sizes = [8] * 64 + [1, k - 1, k, k + 1, 63, 64, 65, ln - 1, ln, ln + 1, 4 * ln + 1]
    if ln == 64:
        sizes += [65] * 64          # segments that begin and end at every offset of a slice
    return sizes


@functools.lru_cache(maxsize=None)
def edge_case(bits, k=10, seed=11):
    """(codes, queries, scope, qscope): the segment edges.  Scope values ascend in the order of edge_sizes, so that is the order of the
    segments in the sorted list: first 64 scopes of 8 records -- at 64 bits exactly the first slice --, then the sizes around k, 64
    and the slice, each beginning where the one before ends.  Value 5 j + 7 carries size j; the values 5 j + 8 lie between them in the
    store and are named by no query; one query names a value no record carries.  The first scopes are named by 1, 2 and 17 queries, one
    query is there twice, and the query order is shuffled."""
    rng = np.random.default_rng(seed + bits)
    sizes = edge_sizes(bits, k)
    values = [5 * j + 7 for j in range(len(sizes))]
    scope = lay_out(sizes, values, rng, strangers=300, stranger_values=[5 * j + 8 for j in range(len(sizes))])
    named = list(values) + [values[1]] + [values[2]] * 16 + [values[-1]] * 2 + [5 * len(sizes) + 7, 5 * 66 + 9]      # the last two: size 0
    qscope = np.array(named, dtype=np.uint32)
    queries = _codes(rng, len(qscope), bits // 8)
    qscope, queries = np.append(qscope, qscope[70]), np.vstack([queries, queries[70:71]])                # one query twice
    order = rng.permutation(len(qscope))
    return _codes(rng, len(scope), bits // 8), np.ascontiguousarray(queries[order]), scope, qscope[order]


HOSTILE = np.array([0, 1, 0x80000000, 0xFFFFFFFF, 0x01345678, 0x02345678, 0x12345600, 0x12345601, 0x00010000, 0x00FF0000, 0x7FFFFFFF, 0xFFFFFFFE],
                   dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def hostile_case(bits=64, n=3000, seed=21):
    """scope values 0, 1, 2^31, 2^32 - 1 and pairs that differ only in their top or bottom byte; 0xFFFFFFFE is in the store and named by
    no query, 0x7FFFFFFF is named and not in the store"""
    rng = np.random.default_rng(seed)
    in_store = HOSTILE[HOSTILE != 0x7FFFFFFF]
    scope = in_store[rng.integers(0, len(in_store), size=n)]
    qscope = np.concatenate([HOSTILE[HOSTILE != 0xFFFFFFFE]] * 3)
    return _codes(rng, n, bits // 8), _codes(rng, len(qscope), bits // 8), scope, qscope[rng.permutation(len(qscope))]


@functools.lru_cache(maxsize=None)
def tie_case(bits, ties, seed=31):
    """(codes, queries, scope, qscope, k): record 2 p is a copy of query 0's code in its OWN scope (value 4), record 2 p + 1 a copy in a
    foreign scope (value 9, named by query 1), p < ties; then 40 own-scope records two bits away.  k = ties - 5 cuts through the copies:
    the row is the k smallest even ids.  Scope 4 sorts first, so the copies are positions 0 .. ties - 1 of the sorted list."""
    rng = np.random.default_rng(seed + bits + ties)
    nbytes = bits // 8
    q = _codes(rng, 1, nbytes)[0]
    far = q.copy()
    far[0] ^= 3
    codes = np.vstack([np.tile(q, (2 * ties, 1)), np.tile(far, (40, 1))])
    scope = np.concatenate([np.tile(np.array([4, 9], dtype=np.uint32), ties), np.full(40, 4, dtype=np.uint32)])
    queries = np.vstack([q, q, far])
    return codes, queries, scope, np.array([4, 9, 4], dtype=np.uint32), ties - 5


@functools.lru_cache(maxsize=None)
def large_case(seed=41):
    """N = 9000: one scope of 8800 records (more than VC_MAX_K) next to small ones of 120, 50 and 30"""
    rng = np.random.default_rng(seed)
    scope = lay_out([8800, 120, 50, 30], [77, 1, 2, 0xFFFFFFFF], rng)
    qscope = np.array([77, 1, 77, 2, 0xFFFFFFFF, 77, 1], dtype=np.uint32)
    return _codes(rng, 9000, 8), _codes(rng, len(qscope), 8), scope, qscope
