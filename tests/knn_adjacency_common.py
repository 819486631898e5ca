"""The numpy model of vc_knn_adjacency*, shared by test_knn_adjacency_cpu.py (which pins it against plain set loops) and
test_knn_adjacency_gpu.py.  It is a function of (rows, counts, kk, flags, max_dist, id_base) only: knn_graph_common.edge_sets gives
the positions every row lists -- as Python sets, which know nothing of the one-compare trick --, the (target, dist, neighbour)
triples of the asked set are gathered and np.lexsort puts them into the contract's order.  Also a mirror of
vc_knn_adjacency_plan.hpp and the crafted input with a pair at distance exactly `bits`."""
import functools

import numpy as np

import knn_graph_common as KG

MUTUAL, EITHER, REVERSE = 0, 1, 2
FLAGS = (REVERSE, MUTUAL, EITHER)
NO_CAP = 0xFFFFFFFF
STALE64 = np.uint64(0xA5A5A5A5DEADBEEF)
MAX_ITEMS = 2 ** 31 - 1
TEAM_DEGREE = 1024
RS_TILE, RS_BLOCK_ITEMS = 4096, 16384           # vc_sort.hip: a sub-tile, a block's items
ADJ_STATS = ("n_edges", "n_entries", "n_empty", "max_degree")
ADJ_NAMES = ["vc_knn_adjacency", "vc_knn_adjacency_dev", "vc_sharded_knn_adjacency", "vc_sharded_knn_adjacency_dev"]


def zero_stats():
    return dict.fromkeys(ADJ_STATS, 0)


# ---- the plan (vc_knn_adjacency_plan.hpp) ------------------------------------------------------------------------------------------------
def kk_ok(k, kk):
    return 1 <= kk <= k


def flags_ok(flags):
    return flags <= REVERSE


def items_ok(n, kk):
    return n * kk <= MAX_ITEMS


def bound(n, kk, flags):
    return (2 if flags == EITHER else 1) * n * kk


def dist_passes(max_dist, bits):
    return (int(min(max_dist, bits)).bit_length() + 7) // 8


def key_passes(n):
    return (int(n).bit_length() + 7) // 8


def item_bytes(n, kk, flags, adj_cap):
    return 24 * n * kk if flags != MUTUAL and adj_cap else 0


def counter_words(n, flags):
    return (2 if flags == EITHER else 1) * (n + 1)


def row_lanes(kk):
    p = 1
    while p < kk and p < 64:
        p *= 2
    return p


def stage_total(n, k, kk, flags, adj_cap, with_counts):
    return n * k * 8 + (n + 1) * 8 + min(adj_cap, bound(n, kk, flags)) * 8 + (((n * 4 + 7) & ~7) if with_counts else 0)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------
def listed(rows, counts, kk, max_dist=NO_CAP, id_base=0):
    """(E, D): E[i] the positions row i lists (knn_graph_common.edge_sets), D[i, j] the distance of a listed entry"""
    n = len(rows)
    if counts is None:
        counts = np.full(n, KG.row_count(n, rows.shape[1]), dtype=np.uint32)
    E = KG.edge_sets(rows, counts, kk, max_dist, id_base)
    D = {}
    for i in range(n):
        for v in rows[i, :min(kk, int(counts[i]))].tolist():
            if (v >> 32) <= max_dist:
                D[i, (v & 0xFFFFFFFF) - id_base] = v >> 32
    return E, D


def adjacency_from(n, E, D, flags, id_base=0):
    """(offsets uint64 [n + 1], adj uint64 [T], stats) of one flag from the listed sets"""
    who = [set() for _ in range(n)]                                        # who[j] = the records that list j
    for i in range(n):
        for j in E[i]:
            who[j].add(i)
    tgt, dist, src = [], [], []
    for j in range(n):
        members = who[j] if flags == REVERSE else (who[j] & E[j]) if flags == MUTUAL else (who[j] | E[j])
        for i in members:
            tgt.append(j)
            dist.append(D[i, j] if (i, j) in D else D[j, i])
            src.append(i + id_base)
    tgt, dist, src = np.array(tgt, dtype=np.int64), np.array(dist, dtype=np.uint64), np.array(src, dtype=np.uint64)
    order = np.lexsort((src, dist, tgt))                                   # by target, then distance, then the neighbour's id
    adj = ((dist << np.uint64(32)) | src)[order]
    deg = np.bincount(tgt, minlength=n) if n else np.zeros(0, dtype=np.int64)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(deg)
    st = dict(n_edges=sum(len(e) for e in E), n_entries=len(adj), n_empty=int((deg == 0).sum()), max_degree=int(deg.max()) if n else 0)
    return offsets, adj, st


def adjacency_model(rows, counts, kk, flags, max_dist=NO_CAP, id_base=0):
    E, D = listed(rows, counts, kk, max_dist, id_base)
    return adjacency_from(len(rows), E, D, flags, id_base)


def adjacency_models(rows, counts, kk, max_dist=NO_CAP, id_base=0):
    """{flags: (offsets, adj, stats)} for the three flags from one pass over the rows"""
    E, D = listed(rows, counts, kk, max_dist, id_base)
    return {flags: adjacency_from(len(rows), E, D, flags, id_base) for flags in FLAGS}


def segments(offsets, adj):
    return [adj[int(offsets[j]):int(offsets[j + 1])] for j in range(len(offsets) - 1)]


def components(offsets, adj, id_base=0):
    """labels (the smallest id of each component) of the graph whose adjacency this is, by a host union-find"""
    n = len(offsets) - 1
    parent = list(range(n))
    tgt = np.repeat(np.arange(n), np.diff(offsets.astype(np.int64)))
    for j, w in zip(tgt.tolist(), adj.tolist()):
        a, b = KG._find(parent, j), KG._find(parent, (w & 0xFFFFFFFF) - id_base)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([KG._find(parent, i) + id_base for i in range(n)], dtype=np.uint32)


def same_adjacency(got, want, what=None):
    assert got[2] == want[2], (what, "stats", got[2], want[2])
    bad = np.nonzero(got[0] != want[0])[0]
    assert len(bad) == 0, (what, "offsets", bad[:8], got[0][bad[:8]], want[0][bad[:8]])
    assert len(got[1]) == len(want[1]), (what, "T", len(got[1]), len(want[1]))
    bad = np.nonzero(got[1] != want[1])[0]
    assert len(bad) == 0, (what, "adj", len(bad), bad[:8], got[1][bad[:8]], want[1][bad[:8]])


# ---- the crafted input ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def complement_case(bits):
    """40 records: a code, 19 records 1 .. 3 flips from it, its EXACT bitwise complement and 19 records 1 .. 3 flips from that.  A row of
    k >= N - 1 lists the whole store, so the code and its complement list each other at distance exactly `bits`, and every segment
    holds distances of a few bits beside distances of nearly all."""
    rng = np.random.default_rng(900 + bits)
    base = rng.integers(0, 256, size=bits // 8, dtype=np.uint8)
    far = base ^ np.uint8(0xFF)
    codes = [base] + [KG._flip(base, rng.choice(bits, size=int(rng.integers(1, 4)), replace=False)) for _ in range(19)]
    codes += [far] + [KG._flip(far, rng.choice(bits, size=int(rng.integers(1, 4)), replace=False)) for _ in range(19)]
    codes = np.array(codes, dtype=np.uint8)[rng.permutation(40)]
    codes.setflags(write=False)
    return codes
