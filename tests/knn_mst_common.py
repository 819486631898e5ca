"""The model of vc_knn_mst* and vc_mst_cut*, shared by test_knn_mst_cpu.py (which pins it against a brute force over all spanning
forests) and test_knn_mst_gpu.py.  The edge set comes from knn_graph_common.edge_sets, which knows nothing of the one-compare trick; the
home rule and the weights are applied to it by plain loops; Kruskal runs under the contract's order as TUPLES (weight, a, dist, b) --
the 64-bit key is only checked to give the same order --; a synchronous Boruvka counts the rounds; the cut is cluster_model's
union-find.  Also a mirror of vc_knn_mst_plan.hpp."""
import functools
import itertools

import numpy as np

import knn_graph_common as KG

MUTUAL, EITHER, REVERSE = 0, 1, 2
DISTANCE, REACHABILITY = 0, 1
NO_CAP = 0xFFFFFFFF
MAX_ITEMS = 0x7FFFFFFF
STALE64 = np.uint64(0xA5A5A5A5DEADBEEF)
EDGE = np.dtype([("a", np.uint32), ("b", np.uint32), ("weight", np.uint32), ("dist", np.uint32)])   # vc_mst_edge
MST_STATS = ("n_edges", "n_graph_edges", "n_tree", "n_clusters", "total_weight", "max_weight", "n_rounds")
MST_NAMES = ["vc_knn_mst", "vc_knn_mst_dev", "vc_sharded_knn_mst", "vc_sharded_knn_mst_dev",
             "vc_mst_cut", "vc_mst_cut_dev", "vc_sharded_mst_cut", "vc_sharded_mst_cut_dev"]


def zero_stats():
    return dict.fromkeys(MST_STATS, 0)


# ---- the plan (vc_knn_mst_plan.hpp) ----------------------------------------------------------------------------------------------------
def items_ok(n, kk):
    return n == 0 or n <= MAX_ITEMS // kk


def min_pts_ok(kind, k, min_pts):
    return 1 <= min_pts <= k + 1 if kind == REACHABILITY else min_pts == 1


def key(weight, pos_a, kk, jj):
    return (weight << 32) | (pos_a * kk + jj)


def ceil_log2(n):
    return 0 if n <= 1 else (n - 1).bit_length()


def round_bound(n):
    return ceil_log2(n) + 1


def words4(words):
    return (words * 4 + 7) & ~7


def live_bound(n, kk, flags):
    return n * kk // 2 if flags == MUTUAL else n * kk


def live_bytes(n, kk, flags):
    L = max(live_bound(n, kk, flags), 1)
    return 2 * (L * 8 + words4(L))


def forest_bytes(n):
    return n * 8 + 2 * words4(n)


def pick_bytes(n):
    m = max(n - 1, 1)
    return 2 * (m * 8 + words4(m))


def stage_total(n, k, bits, with_counts):
    return n * k * 8 + max(n - 1, 0) * 16 + (bits + 1) * 8 + words4(n) + (words4(n) if with_counts else 0)


# ---- the graph --------------------------------------------------------------------------------------------------------------------------
def core_distances(rows, counts, min_pts, bits):
    """c_i: 0 at min_pts 1; else the distance of entry min_pts - 2 of row i, `bits` when the row is shorter"""
    n = len(rows)
    if min_pts == 1:
        return [0] * n
    return [int(rows[i, min_pts - 2]) >> 32 if int(counts[i]) >= min_pts - 1 else bits for i in range(n)]


def graph_edges(rows, counts, kk, flags, max_dist=NO_CAP, id_base=0, weight_kind=DISTANCE, min_pts=1, bits=64):
    """(the undirected edges of the chosen graph as tuples (weight, a, dist, b, jj) of positions, a the HOME end and jj the position of b
    in row a -- unsorted --, the number of listed entries)"""
    n = len(rows)
    counts = np.full(n, KG.row_count(n, rows.shape[1]), dtype=np.uint32) if counts is None else counts
    E = KG.edge_sets(rows, counts, kk, max_dist, id_base)
    core = core_distances(rows, counts, min_pts if weight_kind == REACHABILITY else 1, bits)
    where = [{(int(v) & 0xFFFFFFFF) - id_base: (jj, int(v) >> 32) for jj, v in enumerate(rows[i, :min(kk, int(counts[i]))])} for i in range(n)]
    out = set()
    for i in range(n):
        for j in E[i]:
            lo, hi = min(i, j), max(i, j)
            if flags == MUTUAL and not (lo in E[hi] and hi in E[lo]):
                continue
            a = lo if hi in E[lo] else hi                    # THE HOME RULE: the smaller id if it lists the other, otherwise the larger
            b = lo + hi - a
            jj, d = where[a][b]
            out.add((max(d, core[a], core[b]), a, d, b, jj))
    return sorted(out, key=lambda e: e[1:]), sum(len(e) for e in E)


def _find(parent, x):
    return KG._find(parent, x)


def kruskal(n, edges):
    """the edges kept, taking them ascending in (weight, a, dist, b); the parents at the end"""
    parent, kept = list(range(n)), []
    for e in sorted(edges, key=lambda e: e[:4]):
        ra, rb = _find(parent, e[1]), _find(parent, e[3])
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
            kept.append(e)
    return kept, parent


def boruvka(n, edges):
    """synchronous Boruvka under the same order: (the picked edges as a set, the rounds that hooked something, the live edges at the
    start of every round)"""
    parent, picked, rounds, live_counts = list(range(n)), set(), 0, []
    live = list(edges)
    while True:
        comp = [_find(parent, i) for i in range(n)]
        live = [e for e in live if comp[e[1]] != comp[e[3]]]
        live_counts.append(len(live))
        best = {}
        for e in live:
            for c in (comp[e[1]], comp[e[3]]):
                if c not in best or e[:4] < best[c][:4]:
                    best[c] = e
        if not best:
            return picked, rounds, live_counts
        rounds += 1
        for e in best.values():
            picked.add(e)
            ra, rb = _find(parent, e[1]), _find(parent, e[3])
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)


def to_edges(kept, id_base=0):
    out = np.zeros(len(kept), dtype=EDGE)
    for t, (w, a, d, b, _) in enumerate(kept):
        out[t] = (a + id_base, b + id_base, w, d)
    return out


def mst_model(rows, counts, kk, flags, max_dist=NO_CAP, id_base=0, weight_kind=DISTANCE, min_pts=1, bits=64, with_rounds=True):
    """(edges EDGE [M], labels uint32 [N], hist uint64 [bits + 1], stats dict) of the contract; n_rounds is the synchronous Boruvka's"""
    n = len(rows)
    edges, n_listed = graph_edges(rows, counts, kk, flags, max_dist, id_base, weight_kind, min_pts, bits) if n else ([], 0)
    kept, parent = kruskal(n, edges)
    labels = np.array([_find(parent, i) + id_base for i in range(n)], dtype=np.uint32)
    hist = np.bincount([e[0] for e in kept], minlength=bits + 1).astype(np.uint64)
    st = dict(n_edges=n_listed, n_graph_edges=len(edges), n_tree=len(kept), n_clusters=n - len(kept), total_weight=sum(e[0] for e in kept),
              max_weight=max([e[0] for e in kept], default=0), n_rounds=0)
    if with_rounds:
        picked, st["n_rounds"], _ = boruvka(n, edges)
        assert picked == set(kept)
    return to_edges(kept, id_base), labels, hist, st


def cut_model(n, edges, max_weight, id_base=0):
    """(labels, n_clusters) under the EDGE records of weight <= max_weight: cluster_model's union-find"""
    parent = list(range(n))
    for e in edges:
        if int(e["weight"]) <= max_weight:
            ra, rb = _find(parent, int(e["a"]) - id_base), _find(parent, int(e["b"]) - id_base)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    labels = np.array([_find(parent, i) + id_base for i in range(n)], dtype=np.uint32)
    return labels, len(set(labels.tolist()))


def brute_force(n, edges):
    """the spanning forest that is smallest in the order, by enumeration: of all acyclic edge subsets of the largest size, the one whose
    ascending sequence of ranks is lexicographically smallest (the ranks are strict, so it is unique)"""
    ranked = sorted(edges, key=lambda e: e[:4])
    _, parent = kruskal(n, edges)
    size = n - len({_find(parent, i) for i in range(n)})
    for subset in itertools.combinations(range(len(ranked)), size):   # ascending tuples of ranks, themselves in lexicographic order
        p, ok = list(range(n)), True
        for t in subset:
            ra, rb = _find(p, ranked[t][1]), _find(p, ranked[t][3])
            if ra == rb:
                ok = False
                break
            p[max(ra, rb)] = min(ra, rb)
        if ok:
            return [ranked[t] for t in subset]                         # the first acyclic one is the smallest
    return []


def same_mst(got, want, what=None, rounds=False):
    """edges, labels, hist and the stats (n_rounds only on request: it is implementation-defined)"""
    assert got[0].dtype == EDGE and np.array_equal(got[0], want[0]), (what, "edges", len(got[0]), len(want[0]))
    if got[1] is not None:
        assert np.array_equal(got[1], want[1]), (what, "labels")
    if got[2] is not None:
        assert np.array_equal(got[2], want[2]), (what, "hist")
    if got[3] is not None:
        for name in MST_STATS:
            if name != "n_rounds" or rounds:
                assert got[3][name] == want[3][name], (what, name, got[3][name], want[3][name])


# ---- the inputs -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def uniform_case():
    codes = np.random.default_rng(3).integers(0, 256, (4096, 8), dtype=np.uint8)
    codes.setflags(write=False)
    return codes


@functools.lru_cache(maxsize=None)
def thermometer_case(bits=512):
    """record i = i leading ones, i = 0 .. bits: dist(i, j) = |i - j|"""
    codes = np.zeros((bits + 1, bits // 8), dtype=np.uint8)
    for i in range(bits + 1):
        b = np.zeros(bits, dtype=np.uint8)
        b[:i] = 1
        codes[i] = np.packbits(b, bitorder="little")
    codes.setflags(write=False)
    return codes


@functools.lru_cache(maxsize=None)
def complement_pair(bits=512):
    code = np.random.default_rng(9).integers(0, 256, bits // 8).astype(np.uint8)
    codes = np.stack([code, code ^ np.uint8(0xFF)])
    codes.setflags(write=False)
    return codes


@functools.lru_cache(maxsize=None)
def graph(name, k, id_base=0):
    codes = {"clustered": lambda: KG.clustered_case(64, n=2000), "small": lambda: KG.clustered_case(64, n=700), "uniform": uniform_case,
             "thermo": thermometer_case, "hub": lambda: KG.hub_case()[0], "dup": KG.dup_case, "pair": complement_pair}[name]()
    rows, counts = KG.model_rows(codes, k, id_base)
    rows.setflags(write=False)
    return codes, rows, counts


@functools.lru_cache(maxsize=None)
def model(name, k, kk, flags, max_dist=NO_CAP, id_base=0, weight_kind=DISTANCE, min_pts=1):
    codes, rows, counts = graph(name, k, id_base)
    return mst_model(rows, counts, kk, flags, max_dist, id_base, weight_kind, min_pts, codes.shape[1] * 8)
