"""The numpy model of vc_knn_graph_retain*, shared by test_knn_graph_retain_cpu.py (which pins it against knn_graph_common.model_rows
over the survivors) and test_knn_graph_retain_gpu.py.  It knows nothing of ballots: every old row of a surviving record is translated
through the map, its dead entries are dropped by a stable partition, a row is marked short by the rule m < min(k, K - 1), and the
short rows are answered from model_rows over the survivors.  It predicts n_rows_kept, n_rows_short and n_entries_dropped exactly, and
through knn_graph_common.plan_stats the statistics of the repair."""
import functools

import numpy as np

import knn_graph_common as KG
import knn_graph_update_common as KU

INF = KG.INF
DEAD = 0xFFFFFFFF
WAVE, BLOCK = 64, 256
RETAIN_STATS = ("n_rows_kept", "n_rows_short", "n_entries_dropped")
RETAIN_NAMES = ["vc_knn_graph_retain", "vc_knn_graph_retain_dev", "vc_sharded_knn_graph_retain", "vc_sharded_knn_graph_retain_dev"]
RETAIN_KERNELS = ("vc_kgraph_live_kernel", "vc_kgraph_map_kernel", "vc_kgraph_retain_kernel", "vc_kgraph_back_kernel", "vc_kgraph_short_kernel")


def zero_retain_stats(kept=0):
    return dict(repair=KG.zero_graph_stats(), n_rows_kept=kept, n_rows_short=0, n_entries_dropped=0)


# ---- the plan (vc_knn_graph_retain_plan.hpp) -------------------------------------------------------------------------------------------------
def lanes(k):
    p = 1
    while p < k and p < WAVE:
        p *= 2
    return p


def rows_per_wave(k):
    return WAVE // lanes(k)


def steps(k):
    return -(-k // lanes(k))


def chunk_rows(budget, k, n_old):
    return min(max(budget // (8 * k), 1), max(n_old, 1))


def full(K, k):
    return 0 if K == 0 else min(K - 1, k)


def is_short(m, K, k):
    return m < full(K, k)


def work_total(n_old, K, scan_words):
    """VcKgretWork(n_old, K, scan_words).total"""
    row4 = ((n_old + 1) * 4 + 7) & ~7
    return 32 + 4 * row4 + ((max(K, 1) * 4 + 7) & ~7) + ((scan_words * 4 + 7) & ~7)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------
def retain_map(keep, id_base=0):
    """vc_retain*'s map of a keep mask: new_ids[i] = id_base + the survivors before i, or 0xFFFFFFFF"""
    keep = np.asarray(keep, dtype=bool)
    new_ids = np.full(len(keep), DEAD, dtype=np.uint32)
    new_ids[keep] = (np.arange(int(keep.sum()), dtype=np.uint64) + np.uint64(id_base)).astype(np.uint32)
    return new_ids


def translate(old_rows, old_counts, new_ids, k, id_base=0):
    """the rows of the surviving records with their dead entries dropped and their ids translated, before any repair:
    (rows [K, k], m [K], n_entries_dropped)"""
    new_ids = np.asarray(new_ids, dtype=np.uint32)
    live_row = new_ids != DEAD
    K = int(live_row.sum())
    rows = np.full((K, k), INF, dtype=np.uint64)
    m = np.zeros(K, dtype=np.int64)
    dropped = 0
    for at, i in enumerate(np.nonzero(live_row)[0]):
        c = int(old_counts[i])
        entries = old_rows[i, :c]
        ids = ((entries & np.uint64(0xFFFFFFFF)) - np.uint64(id_base)).astype(np.int64)
        mapped = new_ids[ids]
        alive = mapped != DEAD
        dropped += int((~alive).sum())
        kept = (entries[alive] & np.uint64(0xFFFFFFFF00000000)) | mapped[alive].astype(np.uint64)
        rows[at, :len(kept)] = kept
        m[at] = len(kept)
    return rows, m, dropped


def retain_model(codes, keep, k, id_base=0, old=None):
    """(rows [K, k], counts [K], stats, short): the old graph (`old`, or the model's over all of `codes`) carried across the removal of
    the records with keep == 0; `short` lists the new positions of the rows that were answered again"""
    keep = np.asarray(keep, dtype=bool)
    old_rows, old_counts = old if old is not None else KG.model_rows(codes, k, id_base)
    new_ids = retain_map(keep, id_base)
    K = int(keep.sum())
    rows, m, dropped = translate(old_rows, old_counts, new_ids, k, id_base)
    short = np.nonzero(m < full(K, k))[0]
    counts = m.astype(np.uint32)
    if len(short):
        fresh = KG.model_rows(codes[keep], k, id_base)
        rows[short] = fresh[0][short]
        counts[short] = fresh[1][short]
    st = dict(n_rows_kept=K, n_rows_short=len(short), n_entries_dropped=dropped)
    return rows, counts, st, short


def repair_stats(codes, keep, short, k, k_first=0, linear=False):
    """vc_knn_graph_stats of the searches over the short rows: the plan mirror over their distance histograms among the survivors"""
    if len(short) == 0:
        return KG.zero_graph_stats()
    return KG.plan_stats(KG.dist_hist(codes[np.asarray(keep, dtype=bool)])[short], k, k_first, linear)


# ---- the crafted inputs ----------------------------------------------------------------------------------------------------------------------
def random_keep(n, fraction, seed=5):
    """a keep mask with round(fraction * n) records removed at random"""
    rng = np.random.default_rng(seed)
    keep = np.ones(n, dtype=bool)
    keep[rng.choice(n, size=int(round(fraction * n)), replace=False)] = False
    return keep


CRAFT_K, CRAFT_LONE, CRAFT_CLUSTER = KU.CRAFT_K, KU.CRAFT_LONE, KU.CRAFT_CLUSTER
CRAFT_N = CRAFT_LONE + CRAFT_CLUSTER


@functools.lru_cache(maxsize=None)
def crafted_codes():
    """40 lone codes and a cluster of 30 codes one flip from a centre, two apart from each other, so that at k = 5 the row of a member
    lists the five members of smallest id, all tied at distance 2.  The lone codes are random in their low 48 bits with the high 16
    clear, the centre has the high 16 set: a lone code lies at least 15 further from any member than 16 bits alone, and no lone row
    lists a member (test_knn_graph_retain_cpu.py shows it)"""
    rng = np.random.default_rng(2025)
    lone = rng.integers(0, 256, size=(CRAFT_LONE, 8), dtype=np.uint8)
    lone[:, 6:] = 0
    centre = rng.integers(0, 256, size=8, dtype=np.uint8)
    centre[6:] = 0xFF
    cluster = [KG._flip(centre, [b]) for b in range(CRAFT_CLUSTER)]
    codes = np.concatenate([lone, np.array(cluster, dtype=np.uint8)])
    codes.setflags(write=False)
    return codes


TIE_ROW, TIE_WINNER, TIE_LOSER = CRAFT_LONE + 10, CRAFT_LONE + 4, CRAFT_LONE + 5


def crafted_patterns():
    """{name: keep mask} over crafted_codes()"""
    def without(dead):
        keep = np.ones(CRAFT_N, dtype=bool)
        keep[list(dead)] = False
        return keep
    return {
        "cluster": without(range(CRAFT_LONE, CRAFT_N)),     # a whole cluster: the lone rows list no member and stay untouched
        "tie": without([TIE_WINNER]),                       # the smaller id of two records tied at a row's last distance
        "first": without([0]),
        "last": without([CRAFT_N - 1]),
        "alternate": without(range(1, CRAFT_N, 2)),         # every second record
    }


def dense_cluster_keep():
    """knn_graph_update_common.dense_case with the whole cluster of its most frequent code removed: (codes, keep)"""
    codes = KU.dense_case()[0]
    centre = codes[KG.dup_copies(codes)[0]]
    dist = np.unpackbits(codes ^ centre[None, :], axis=1).sum(axis=1)
    return codes, dist > 6                                   # a member lies at most 3 flips from its centre, two members at most 6 apart
