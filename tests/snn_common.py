"""The numpy model of vc_cluster_snn*, shared by test_snn_cpu.py (which pins it against plain set loops) and test_snn_gpu.py: the
edge sets of knn_graph_common, the overlaps as the boolean membership matrix times its transpose, a host union-find, the histogram
and the statistics; a mirror of vc_snn_plan.hpp; and the noisy input on which the thresholds bite."""
import functools

import numpy as np

import knn_graph_common as KG

MAX_KK = 1024
NONE = np.uint32(0xFFFFFFFF)
WAVE_KK = 128                                  # VC_SNN_WAVE_KK, pinned against the header's by test_snn_cpu.py
STALE64 = np.uint64(0xA5A5A5A5DEADBEEF)
SNN_STATS = ("n_edges", "n_mutual", "n_joined", "n_clusters", "max_shared")
SNN_NAMES = ["vc_cluster_snn", "vc_cluster_snn_dev", "vc_sharded_cluster_snn", "vc_sharded_cluster_snn_dev"]


def zero_stats():
    return dict.fromkeys(SNN_STATS, 0)


# ---- the plan (vc_snn_plan.hpp) ------------------------------------------------------------------------------------------------------------
def kk_ok(k, kk):
    return 1 <= kk <= min(k, MAX_KK)


def pow2_at_least(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def table_slots(kk):
    return pow2_at_least(2 * kk)


def team_waves(kk):
    return 1 if kk <= WAVE_KK else 4


def entry_lanes(kk):
    return min(64, pow2_at_least(kk))


def stage_total(n, k, kk, with_counts, with_shared, with_hist):
    """VcSnnStage(...).total"""
    up8 = lambda b: (b + 7) & ~7
    return n * k * 8 + (up8(n * 4) if with_counts else 0) + (up8(n * kk * 4) if with_shared else 0) + (kk * 8 if with_hist else 0)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------
def shared_matrix(E, n):
    """shared[i, j] = |S_i & S_j| for all pairs: the membership matrix times its transpose (float32, exact: every sum stays below 2^24)"""
    M = np.zeros((n, n), dtype=np.float32)
    for i, e in enumerate(E):
        if e:
            M[i, list(e)] = 1.0
    return np.rint(M @ M.T).astype(np.int64)


def snn_weights(rows, counts, kk, max_dist=0xFFFFFFFF, id_base=0):
    """what does not depend on the threshold or the flag: (shared uint32 [N, kk], hist uint64 [kk], edges -- the listed entries as
    (i, j, shared, j lists i) in row order)"""
    n = len(rows)
    E = KG.edge_sets(rows, counts, kk, max_dist, id_base)
    S = shared_matrix(E, n)
    shared = np.full((n, kk), NONE, dtype=np.uint32)
    hist = np.zeros(kk, dtype=np.uint64)
    edges = []
    for i in range(n):
        for jj in range(min(kk, int(counts[i]))):
            v = int(rows[i, jj])
            if (v >> 32) > max_dist:
                continue
            j = (v & 0xFFFFFFFF) - id_base
            s = int(S[i, j])
            shared[i, jj] = s
            hist[s] += np.uint64(1)
            edges.append((i, j, s, i in E[j]))
    return shared, hist, edges


def snn_labels(n, edges, min_shared, flags=KG.MUTUAL, id_base=0):
    """(labels uint32 [N] -- the smallest id of each component --, stats dict) of the edges of snn_weights"""
    parent = list(range(n))
    st = zero_stats()
    for i, j, s, mutual in edges:
        st["n_edges"] += 1
        st["n_mutual"] += 1 if mutual and i < j else 0
        st["max_shared"] = max(st["max_shared"], s)
        if s >= min_shared and (mutual or flags == KG.EITHER):
            st["n_joined"] += 1 if (i < j or not mutual) else 0      # a mutual pair from its smaller member, a one-sided pair from its lister
            a, b = KG._find(parent, i), KG._find(parent, j)
            if a != b:
                parent[max(a, b)] = min(a, b)
    labels = np.array([KG._find(parent, i) + id_base for i in range(n)], dtype=np.uint32) if n else np.zeros(0, dtype=np.uint32)
    st["n_clusters"] = len(set(labels.tolist()))
    return labels, st


def snn_model(rows, counts, kk, min_shared, flags=KG.MUTUAL, max_dist=0xFFFFFFFF, id_base=0):
    """(labels uint32 [N], shared uint32 [N, kk], hist uint64 [kk], stats dict)"""
    shared, hist, edges = snn_weights(rows, counts, kk, max_dist, id_base)
    labels, st = snn_labels(len(rows), edges, min_shared, flags, id_base)
    return labels, shared, hist, st


def same_snn(got, want, what=None):
    """every word: labels, weights (None: not asked for), histogram (likewise), stats"""
    assert np.array_equal(got[0], want[0]), (what, "labels", np.nonzero(got[0] != want[0])[0][:8])
    if got[1] is not None:
        bad = np.argwhere(got[1] != want[1])
        assert len(bad) == 0, (what, "shared", bad[:8], got[1][tuple(bad[0])] if len(bad) else None, want[1][tuple(bad[0])] if len(bad) else None)
    if got[2] is not None:
        assert np.array_equal(got[2], want[2]), (what, "hist", got[2], want[2])
    assert got[3] == want[3], (what, got[3], want[3])


# ---- the input -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_case(bits, n=700, centres=12, flips=None, noise=0.3, seed=3):
    """groups with noise between them: with probability `noise` a record is a uniform random code, otherwise a random centre with
    0 .. flips (default bits // 5) bits flipped.  The overlaps of neighbouring lists then span the whole range and every threshold bites."""
    flips = bits // 5 if flips is None else flips
    rng = np.random.default_rng(seed * 1000 + bits)
    cs = rng.integers(0, 256, size=(centres, bits // 8), dtype=np.uint8)
    codes = np.empty((n, bits // 8), dtype=np.uint8)
    for i in range(n):
        if rng.random() < noise:
            codes[i] = rng.integers(0, 256, size=bits // 8, dtype=np.uint8)
        else:
            codes[i] = KG._flip(cs[rng.integers(0, centres)], rng.choice(bits, size=int(rng.integers(0, flips + 1)), replace=False))
    codes.setflags(write=False)
    return codes


@functools.lru_cache(maxsize=None)
def mixed_graph(bits, k, n=700):
    """(codes, rows, counts) of mixed_case at id_base 0: the reference, computed once and left unchanged"""
    codes = mixed_case(bits, n=n)
    rows, counts = KG.model_rows(codes, k)
    rows.setflags(write=False)
    counts.setflags(write=False)
    return codes, rows, counts


def thresholds(kk):
    return [0, 1, kk // 4, kk // 2, 3 * kk // 4, kk - 1, kk, 0xFFFFFFFF]
