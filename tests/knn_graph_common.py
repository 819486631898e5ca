"""The numpy model of vc_knn_graph* and vc_cluster_knn*, shared by test_knn_graph_cpu.py (which pins it against plain loops) and
test_knn_graph_gpu.py: brute-force rows by (dist, id); the edge sets as Python sets, which know nothing of the one-compare trick;
in-degrees and a host union-find for both flags; and a mirror of vc_knn_graph_plan.hpp, which predicts the statistics exactly -- the
number of exact-MIH rounds a record takes depends on the multiset of its distances only."""
import functools

import numpy as np

MAX_K = 8192
INF = np.uint64(0xFFFFFFFFFFFFFFFF)
STALE = np.uint64(0xA5A5A5A5DEADBEEF)
STALE32 = np.uint32(0xDEADBEEF)
GIVE_UP = 0xFFFFFFFF
LINEAR, MIH_EXACT, MIH_APPROX = 0, 1, 2
MUTUAL, EITHER = 0, 1
BATCH_DEFAULT = 4096
SCRATCH_DEFAULT = 64 << 20
TABLES = {64: 2, 128: 4, 256: 8, 512: 16}     # n_tables of the exact-MIH handles
GRAPH_STATS = ("n_rounds_max", "k_last", "n_searched", "n_linear", "n_gave_up")
CLUSTER_STATS = ("n_edges", "n_mutual", "n_clusters", "max_in_degree")
GRAPH_NAMES = ["vc_knn_graph", "vc_knn_graph_dev", "vc_sharded_knn_graph", "vc_sharded_knn_graph_dev"]
CLUSTER_NAMES = ["vc_cluster_knn", "vc_cluster_knn_dev", "vc_sharded_cluster_knn", "vc_sharded_cluster_knn_dev"]


def zero_graph_stats():
    return dict.fromkeys(GRAPH_STATS, 0)


def zero_cluster_stats():
    return dict.fromkeys(CLUSTER_STATS, 0)


# ---- the plan (vc_knn_graph_plan.hpp) ------------------------------------------------------------------------------------------------------
def k_ok(k):
    return 1 <= k <= MAX_K - 1


def k_first_ok(k, k_first):
    return k_first == 0 or k + 1 <= k_first <= MAX_K


def next_k(kp):
    return MAX_K if kp >= MAX_K // 2 else 2 * kp


def first_k(k, k_first, linear):
    return k + 1 if linear else (k_first or next_k(k + 1))


def schedule(k, k_first):
    """the k' of the exact-MIH rounds, to VC_MAX_K"""
    kp, out = first_k(k, k_first, False), []
    while True:
        out.append(kp)
        if kp >= MAX_K:
            return out
        kp = next_k(kp)


def sub_batch(budget, kp):
    return min(max(budget // (8 * kp), 1), 0xFFFFFFFF)


def rows_bytes(n, budget, kp):
    return 8 * kp * min(n, sub_batch(budget, kp))


def row_count(n, k):
    return 0 if n == 0 else min(n - 1, k)


def key_range(n, first, count):
    """(ok, rows) of vc_kgraph_range"""
    if first > n or count > n - first:
        return False, 0
    return True, count or n - first


def work_total(nq, W, scan_words):
    """VcKgraphWork(nq, W, scan_words).total"""
    row4 = (nq * 4 + 7) & ~7
    return 16 + 2 * row4 + ((scan_words * 4 + 7) & ~7) + 5 * row4 + 2 * nq * W * 8


# ---- distances ---------------------------------------------------------------------------------------------------------------------------------
def _bits(codes):
    return np.unpackbits(np.ascontiguousarray(codes, dtype=np.uint8), axis=1).astype(np.float32)


def dist_block(bits_all, lo, hi):
    """Hamming distances of the records lo .. hi - 1 to all records, int64 [hi - lo, N] (exact: the sums stay far below 2^24)"""
    a = bits_all[lo:hi]
    return np.rint(a @ (1.0 - bits_all).T + (1.0 - a) @ bits_all.T).astype(np.int64)


def model_rows(codes, k, id_base=0, first=0, count=0):
    """THE RULE: row p - first = the k smallest packed (dist << 32 | id) over the records other than record p, ascending, INF padded;
    counts = min(k, N - 1).  (rows uint64 [n, k], counts uint32 [n])"""
    n = len(codes)
    ok, rows_n = key_range(n, first, count)
    assert ok
    rows = np.full((rows_n, k), INF, dtype=np.uint64)
    counts = np.full(rows_n, row_count(n, k), dtype=np.uint32)
    if n < 2 or rows_n == 0:
        return rows, counts
    bits_all, ids = _bits(codes), np.arange(n, dtype=np.uint64) + np.uint64(id_base)
    take = min(k, n - 1)
    for lo in range(first, first + rows_n, 512):
        hi = min(lo + 512, first + rows_n)
        packed = (dist_block(bits_all, lo, hi).astype(np.uint64) << np.uint64(32)) | ids[None, :]
        packed[np.arange(hi - lo), np.arange(lo, hi)] = INF          # the record itself, wherever its duplicates are
        part = np.partition(packed, take - 1, axis=1)[:, :take] if take < n else packed
        rows[lo - first:hi - first, :take] = np.sort(part, axis=1)[:, :take]
    return rows, counts


def loop_rows(codes, k, id_base=0):
    """the same by a plain double loop (small inputs)"""
    n = len(codes)
    rows = np.full((n, k), INF, dtype=np.uint64)
    for i in range(n):
        lst = sorted((bin(int.from_bytes(bytes(codes[i] ^ codes[j]), "little")).count("1") << 32) | (id_base + j) for j in range(n) if j != i)
        for j, v in enumerate(lst[:k]):
            rows[i, j] = v
    return rows, np.full(n, min(k, max(n - 1, 0)), dtype=np.uint32)


def dist_hist(codes, first=0, count=0):
    """H[p - first, d] = the records (the own one included) at distance d of record p"""
    n, nb = len(codes), codes.shape[1] * 8 + 1
    ok, rows_n = key_range(n, first, count)
    assert ok
    bits_all = _bits(codes)
    H = np.zeros((rows_n, nb), dtype=np.int64)
    for lo in range(first, first + rows_n, 512):
        hi = min(lo + 512, first + rows_n)
        d = dist_block(bits_all, lo, hi) + np.arange(hi - lo)[:, None] * nb
        H[lo - first:hi - first] = np.bincount(d.ravel(), minlength=(hi - lo) * nb).reshape(hi - lo, nb)
    return H


def plan_stats(H, k, k_first=0, linear=False):
    """THE PLAN MIRROR: the statistics of a call over the records whose distance histograms are H (dist_hist).  A full k' row is
    unsettled iff, among the k' nearest including the record itself, fewer than k other records lie below the k'-th distance."""
    n = len(H)
    st = zero_graph_stats()
    if n == 0:
        return st
    if linear:
        st.update(n_rounds_max=1, k_last=k + 1, n_searched=n)
        return st
    total = int(H[0].sum())                                         # N
    cum = np.cumsum(H, axis=1)
    open_ = np.ones(n, dtype=bool)
    rounds = np.zeros(n, dtype=np.int64)
    for kp in schedule(k, k_first):
        rounds[open_] += 1
        st["n_searched"] += int(open_.sum())
        st["k_last"] = kp
        if total < kp:                                              # no row is full: the whole store
            open_[:] = False
            break
        D = np.argmax(cum >= kp, axis=1)                            # the k'-th distance
        below = np.where(D > 0, cum[np.arange(n), np.maximum(D, 1) - 1], 0)
        others = below - (below > 0)
        open_ &= others < k
        if not open_.any():
            break
    st["n_linear"] = int(open_.sum())
    rounds[open_] += 1
    st["n_rounds_max"] = int(rounds.max())
    return st


# ---- edges, in-degrees, components -------------------------------------------------------------------------------------------------------------
def edge_sets(rows, counts, kk, max_dist, id_base=0):
    """E[i] = the positions row i lists: among its first min(kk, count_i) entries, at a distance <= max_dist"""
    out = []
    for i in range(len(rows)):
        m = min(kk, int(counts[i]))
        out.append({int(v & np.uint64(0xFFFFFFFF)) - id_base for v in rows[i, :m] if int(v >> np.uint64(32)) <= max_dist})
    return out


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def cluster_model(rows, counts, kk, flags=MUTUAL, max_dist=0xFFFFFFFF, id_base=0):
    """(labels uint32 [N] -- the smallest id of each component --, in_degree uint32 [N], stats dict)"""
    n = len(rows)
    E = edge_sets(rows, counts, kk, max_dist, id_base)
    deg = np.zeros(n, dtype=np.uint32)
    parent = list(range(n))
    n_mutual = 0
    for i in range(n):
        for j in E[i]:
            deg[j] += 1
            mutual = i in E[j]
            n_mutual += 1 if mutual and i < j else 0
            if mutual or flags == EITHER:
                a, b = _find(parent, i), _find(parent, j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    labels = np.array([_find(parent, i) + id_base for i in range(n)], dtype=np.uint32) if n else np.zeros(0, dtype=np.uint32)
    st = dict(n_edges=sum(len(e) for e in E), n_mutual=n_mutual, n_clusters=len(set(labels.tolist())), max_in_degree=int(deg.max()) if n else 0)
    return labels, deg, st


# ---- the crafted inputs ----------------------------------------------------------------------------------------------------------------------
def _flip(code, positions):
    code = code.copy()
    for b in positions:
        code[b // 8] ^= np.uint8(1 << (b % 8))
    return code


@functools.lru_cache(maxsize=None)
def clustered_case(bits, n=2000, centres=5, flips=3, seed=11):
    """few centres, at most `flips` flipped bits: every distance has many ties"""
    rng = np.random.default_rng(seed * 1000 + bits)
    cs = rng.integers(0, 256, size=(centres, bits // 8), dtype=np.uint8)
    codes = np.empty((n, bits // 8), dtype=np.uint8)
    for i in range(n):
        codes[i] = _flip(cs[rng.integers(0, centres)], rng.choice(bits, size=int(rng.integers(0, flips + 1)), replace=False))
    codes.setflags(write=False)
    return codes


DUP_N, DUP_COPIES, DUP_K, DUP_K_FIRST = 9000, 8300, 5, 2048


@functools.lru_cache(maxsize=None)
def dup_case(bits=64):
    """9000 records of which 8300 are one code, scattered over the ids; the others lie 1 .. 3 flips from it or around a far centre"""
    rng = np.random.default_rng(77)
    base = rng.integers(0, 256, size=bits // 8, dtype=np.uint8)
    far = base ^ np.uint8(0xFF)
    codes = np.tile(base, (DUP_N, 1))
    others = np.sort(np.concatenate([[0, 1], 2 + rng.choice(DUP_N - 2, size=DUP_N - DUP_COPIES - 2, replace=False)]))   # (the smallest ids are no copies)
    for t, i in enumerate(others):
        centre = base if t % 2 == 0 else far
        codes[i] = _flip(centre, rng.choice(bits, size=int(rng.integers(1, 4)), replace=False))
    codes.setflags(write=False)
    return codes


def dup_copies(codes):
    """the positions of the most frequent code, ascending"""
    uniq, inverse, sizes = np.unique(codes, axis=0, return_inverse=True, return_counts=True)
    return np.nonzero(inverse.ravel() == np.argmax(sizes))[0]


HUB_K, HUB_SATELLITES = 10, 40


@functools.lru_cache(maxsize=None)
def hub_case(bits=64):
    """one hub code with 40 satellites at distance 1 (one flipped bit each, so two satellites are 2 apart), and a far clump of 30.
    Every satellite lists the hub first; the hub lists only the k satellites of smallest id.  Returns (codes, the hub's position)."""
    rng = np.random.default_rng(5)
    hub = rng.integers(0, 256, size=bits // 8, dtype=np.uint8)
    far = hub ^ np.uint8(0xFF)
    sats = [_flip(hub, [b]) for b in range(HUB_SATELLITES)]
    clump = [_flip(far, rng.choice(bits, size=2, replace=False)) for _ in range(30)]
    codes = np.array(sats[:25] + [hub] + sats[25:] + clump, dtype=np.uint8)
    codes.setflags(write=False)
    return codes, 25


def same_graph(got, want, what=None):
    rows, counts = got[0], got[1]
    assert np.array_equal(counts, want[1]), (what, "counts", np.nonzero(counts != want[1])[0][:8])
    bad = np.nonzero((rows != want[0]).any(axis=1))[0]
    assert len(bad) == 0, (what, "rows", bad[:8], rows[bad[0]] if len(bad) else None, want[0][bad[0]] if len(bad) else None)
