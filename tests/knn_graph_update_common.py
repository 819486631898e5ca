"""The numpy model of vc_knn_graph_update*, shared by test_knn_graph_update_cpu.py (which pins it against knn_graph_common.model_rows
over the whole store) and test_knn_graph_update_gpu.py: the old rows carried along, the loop over old batches and windows with the
thresholds read from the rows as they are, the window rule of vc_knn_graph_update_plan.hpp and a merge by sorting -- which knows
nothing of rank counting.  It predicts every statistic of the join exactly."""
import functools

import numpy as np

import knn_graph_common as KG

INF = KG.INF
OLD_BATCH_DEFAULT, OLD_BATCH_MAX = 1 << 18, 1 << 24
WINDOW_DEFAULT, WINDOW_MAX = 1024, 1 << 20
GATHER_CHUNK = 1 << 18
LDS_WORDS, BLOCK = 2048, 256
UPDATE_STATS = ("n_rows_changed", "n_inserted", "n_hits", "n_windows", "n_halvings")
UPDATE_NAMES = ["vc_knn_graph_update", "vc_knn_graph_update_dev", "vc_sharded_knn_graph_update", "vc_sharded_knn_graph_update_dev"]


def zero_update_stats():
    return dict(build=KG.zero_graph_stats(), **dict.fromkeys(UPDATE_STATS, 0))


# ---- the plan (vc_knn_graph_update_plan.hpp) -------------------------------------------------------------------------------------------------
def old_batch(knob):
    return OLD_BATCH_DEFAULT if knob == 0 or knob > OLD_BATCH_MAX else knob


def window(knob):
    return WINDOW_DEFAULT if knob == 0 or knob > WINDOW_MAX else knob


def records(W):
    return 8 if W <= 1 else 4 if W == 2 else 2


def blocks(nb, W):
    return (nb + BLOCK * records(W) - 1) // (BLOCK * records(W))


def accept(H, budget, nw):
    return nw <= 1 or (H <= 0xFFFFFFFF and 8 * H <= budget)


def halve(nw):
    return max(nw // 2, 1)


def merge_sub(budget, k):
    return min(max(budget // (8 * k), 1), 0xFFFFFFFF)


def merge_bytes(affected, budget, k):
    return 8 * k * min(affected, merge_sub(budget, k))


def work_total(nb, ng, W, scan_words):
    """VcKgupdWork(nb, ng, W, scan_words).total"""
    row4, big4 = (nb * 4 + 7) & ~7, (max(nb, ng) * 4 + 7) & ~7
    return 64 + 6 * row4 + ((blocks(nb, W) * 4 + 7) & ~7) + ((nb + 7) & ~7) + ((scan_words * 4 + 7) & ~7) + 2 * big4 + nb * W * 8


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------
def join_model(codes, n_old, k, old_rows, old_counts, id_base=0, window_knob=0, old_batch_knob=0, budget=KG.SCRATCH_DEFAULT):
    """the old rows after the join against the records [n_old, N): (rows [n_old, k], counts [n_old], stats of the join)"""
    n, n_new = len(codes), len(codes) - n_old
    rows, counts = old_rows.copy(), old_counts.astype(np.int64)
    st = dict.fromkeys(UPDATE_STATS, 0)
    if n_old == 0 or n_new == 0:
        return rows, counts.astype(np.uint32), st
    bits = KG._bits(codes)
    new_bits, new_ids = bits[n_old:], np.arange(n_old, n, dtype=np.uint64) + np.uint64(id_base)
    ob, changed = old_batch(old_batch_knob), np.zeros(n_old, dtype=bool)
    for pos in range(0, n_old, ob):
        hi = min(pos + ob, n_old)
        a = bits[pos:hi]
        size, j0 = window(window_knob), 0
        while j0 < n_new:
            nw = min(size, n_new - j0)
            while True:
                b = new_bits[j0:j0 + nw]
                d = np.rint(a @ (1.0 - b).T + (1.0 - a) @ b.T).astype(np.uint64)
                p = (d << np.uint64(32)) | new_ids[None, j0:j0 + nw]
                T = np.where(counts[pos:hi] == k, rows[pos:hi, k - 1], INF)          # read from the rows as they are now
                hit = p < T[:, None]
                H = int(hit.sum())
                st["n_windows"] += 1
                if accept(H, budget, nw):
                    break
                size = nw = halve(nw)
                st["n_halvings"] += 1
            st["n_hits"] += H
            if H:
                merged = np.sort(np.concatenate([rows[pos:hi], np.where(hit, p, INF)], axis=1), axis=1)[:, :k]
                rows[pos:hi] = merged
                counts[pos:hi] = np.minimum(k, counts[pos:hi] + hit.sum(axis=1))
                changed[pos:hi] |= hit.any(axis=1)
            j0 += nw
    st["n_rows_changed"] = int(changed.sum())
    live = rows != INF
    st["n_inserted"] = int((live & (((rows & np.uint64(0xFFFFFFFF)) - np.uint64(id_base)) >= np.uint64(n_old))).sum())
    return rows, counts.astype(np.uint32), st


def update_model(codes, n_old, k, id_base=0, window_knob=0, old_batch_knob=0, budget=KG.SCRATCH_DEFAULT, old=None):
    """(rows [N, k], counts [N], the join's stats): the old records' rows of the store of n_old records (`old`, or the model's) joined
    against the appended records, above the new records' rows of the whole store"""
    n = len(codes)
    old_rows, old_counts = old if old is not None else KG.model_rows(codes[:n_old], k, id_base)
    j_rows, j_counts, st = join_model(codes, n_old, k, old_rows, old_counts, id_base, window_knob, old_batch_knob, budget)
    if n == n_old:
        return j_rows, j_counts, st
    new_rows, new_counts = KG.model_rows(codes, k, id_base, first=n_old, count=n - n_old)
    return np.concatenate([j_rows, new_rows]), np.concatenate([j_counts, new_counts]), st


def changed_rows(before, after):
    """the old rows of which at least one word differs"""
    return int((before != after[:len(before)]).any(axis=1).sum())


# ---- the crafted inputs ----------------------------------------------------------------------------------------------------------------------
PLANTED = 200


@functools.lru_cache(maxsize=None)
def planted_case(bits, n=2000, planted=PLANTED, seed=3):
    """knn_graph_common.clustered_case(bits) followed by `planted` records planted next to old ones: copies of old records with 0 .. 2
    flipped bits.  Random clustered records alone would not do: at 128 bits three of them change no old row.  (codes, n_old)"""
    base = KG.clustered_case(bits, n=n)
    rng = np.random.default_rng(seed * 100 + bits)
    extra = np.empty((planted, bits // 8), dtype=np.uint8)
    for j in range(planted):
        extra[j] = KG._flip(base[rng.integers(0, n)], rng.choice(bits, size=int(rng.integers(0, 3)), replace=False))
    codes = np.concatenate([base, extra])
    codes.setflags(write=False)
    return codes, n


CRAFT_K, CRAFT_LONE, CRAFT_CLUSTER, CRAFT_DUPS = 5, 40, 30, 8


@functools.lru_cache(maxsize=None)
def crafted_case(bits=64):
    """Old: 40 lone random codes (about bits / 2 apart) and a dense cluster of 30 codes one flip from a centre (two apart from each
    other).  New: 8 exact duplicates of lone record 3, whose row at k = 5 they replace entirely (more than k hits in one window); one
    more code one flip from the centre, which ties the last distance of every member's row and loses on its id; two exact duplicates
    of cluster members; the complement of a lone code.  Most lone rows take no hit.  (codes, n_old, the position of the replaced row,
    the position of the tie)"""
    rng = np.random.default_rng(2024)
    lone = rng.integers(0, 256, size=(CRAFT_LONE, bits // 8), dtype=np.uint8)
    centre = rng.integers(0, 256, size=bits // 8, dtype=np.uint8)
    cluster = [KG._flip(centre, [b]) for b in range(CRAFT_CLUSTER)]
    old = np.concatenate([lone, np.array(cluster, dtype=np.uint8)])
    new = [lone[3]] * CRAFT_DUPS + [KG._flip(centre, [CRAFT_CLUSTER + 1])] + [cluster[4], cluster[17]] + [lone[3] ^ np.uint8(0xFF)]
    codes = np.concatenate([old, np.array(new, dtype=np.uint8)])
    codes.setflags(write=False)
    return codes, len(old), 3, len(old) + CRAFT_DUPS


DENSE_K, DENSE_NEW, DENSE_BUDGET, DENSE_WINDOW = 500, 16, 4096, 16


@functools.lru_cache(maxsize=None)
def dense_case(bits=64):
    """clustered_case(bits) followed by 16 duplicates of its most frequent code.  k = 500 is more than a cluster holds (at a smaller k
    the rows of a cluster are full of nearer records and take none of them), so every row of the cluster, some 400, takes every one of
    them: a budget of 4096 bytes (512 hits) cuts a window of 16 in half down to single records.  (codes, n_old)"""
    base = KG.clustered_case(bits)
    code = base[KG.dup_copies(base)[0]]
    codes = np.concatenate([base, np.tile(code, (DENSE_NEW, 1))])
    codes.setflags(write=False)
    return codes, len(base)
