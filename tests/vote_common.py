"""What test_vote_cpu.py and test_vote_gpu.py share: THE MODEL of vc_knn_vote* and vc_label_propagate* -- a plain dict loop per segment
(tally, first position, the three-rule winner) and the round loop --, a mirror of csrc/vc_vote_plan.hpp (team shape per length, table
slots, scratch bytes) and the labelled inputs: snn_common.mixed_graph(bits, 10) with seeded labels, a few classes, about 60 % of the
records unlabelled."""
import functools

import numpy as np

import knn_adjacency_common as KA
import snn_common as SN

NONE = 0xFFFFFFFF                  # VC_VOTE_NONE
COUNT, CLOSENESS = 0, 1            # VC_VOTE_*
CLAMP = 1                          # VC_LP_CLAMP_SEEDS
MAX_ITERS = 64                     # VC_LP_MAX_ITERS
MAX_K = 8192                       # VC_MAX_K
NO_CAP = 0xFFFFFFFF
STALE32 = np.uint32(0xDEADBEEF)
VOTE_STATS = ("n_voted", "n_unlabelled", "n_ties", "n_entries")
LP_STATS = ("n_iters", "converged", "n_changed_last", "n_labelled", "n_ties_last")
VOTE_NAMES = ["vc_knn_vote", "vc_knn_vote_dev", "vc_sharded_knn_vote", "vc_sharded_knn_vote_dev",
              "vc_label_propagate", "vc_label_propagate_dev", "vc_sharded_label_propagate", "vc_sharded_label_propagate_dev"]

# ---- the mirror of csrc/vc_vote_plan.hpp, pinned against the header by test_vote_cpu.py ----------------------------------------------------------
TEAM_MIN, TEAM_MAX, WAVE_MAX, SMALL_MAX, BIG_MAX = 8, 64, 256, 1024, 8192
MIN_SLOTS, SLOT_BYTES, LONG_AUX_BYTES, STAT_BYTES, PLAN_STAT_BYTES, BLOCK, BINS = 64, 8, 16, 64, 128, 256, 8
BIN_NAMES = ("P8", "P16", "P32", "P64", "WAVE", "SMALL", "BIG", "LONG")


def zero_vote_stats():
    return {name: 0 for name in VOTE_STATS}


def zero_lp_stats():
    return {name: 0 for name in LP_STATS}


def pow2_at_least(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def team_lanes(length):
    return max(TEAM_MIN, pow2_at_least(length))


def bin_of(length):
    for b, top in enumerate((8, 16, 32, TEAM_MAX, WAVE_MAX, SMALL_MAX, BIG_MAX)):
        if length <= top:
            return b
    return 7


def slots(length):
    s = MIN_SLOTS
    while s < 2 * length:
        s <<= 1
    return s


def lds_bytes(bound):
    return slots(bound) * SLOT_BYTES


def table_threads(bound):
    return 64 if bound <= WAVE_MAX else BLOCK


def length_ok(length, bits):
    return length <= 0xFFFFFFFF // (bits + 1)


def key(tally, is_current, pos):
    return (tally << 32) | (0x80000000 if is_current else 0) | (0x7FFFFFFF - pos)


def _w4(words):
    return (words * 4 + 7) & ~7


def lp_bytes(n):
    return 3 * _w4(n) + _w4(BINS * ((n + BLOCK - 1) // BLOCK))


def long_bytes(n_long, n_slots):
    return n_long * LONG_AUX_BYTES + n_slots * SLOT_BYTES


def long_cap(n_entries):
    return n_entries // (BIG_MAX + 1) + 1


def lp_stat_bytes():
    return PLAN_STAT_BYTES + MAX_ITERS * STAT_BYTES


def vote_stage_total(n_rows, k, n, with_counts):
    return max(n_rows * k * 8 + _w4(n) + 3 * _w4(n_rows) + (_w4(n_rows) if with_counts else 0), 8)


def lp_stage_total(n, n_entries):
    return (n + 1) * 8 + n_entries * 8 + 4 * _w4(n)


# ---- THE MODEL -------------------------------------------------------------------------------------------------------------------------------------
def weight(kind, bits, d):
    return bits + 1 - d if kind == CLOSENESS else 1


def vote_segment(words, labels, kind, bits, current=NONE, id_base=0):
    """One segment (packed words in order) under `labels` -> (winner, votes, total, rule, voting entries): a dict of tallies and first
    positions, then the strict order -- the larger tally, then the current label, then the earliest first occurrence.  rule is 0 when
    nothing votes, 1 when the tally alone decides, 2 when the current label breaks the tie, 3 when the first occurrence does."""
    tally, first, total, voting = {}, {}, 0, 0
    for pos, w in enumerate(words):
        w = int(w)
        lab = int(labels[(w & 0xFFFFFFFF) - id_base])
        if lab == NONE:
            continue
        wt = weight(kind, bits, w >> 32)
        assert wt >= 1
        tally[lab] = tally.get(lab, 0) + wt
        first.setdefault(lab, pos)
        total += wt
        voting += 1
    if not tally:
        return NONE, 0, 0, 0, 0
    top = max(tally.values())
    tied = [lab for lab, t in tally.items() if t == top]
    if len(tied) == 1:
        return tied[0], top, total, 1, voting
    if current != NONE and current in tied:
        return current, top, total, 2, voting
    return min(tied, key=lambda lab: first[lab]), top, total, 3, voting


def row_segment(row, count, kk, max_dist):
    return [w for w in row[:min(kk, int(count))].tolist() if (w >> 32) <= max_dist]


def vote_model(rows, counts, kk, labels, kind=COUNT, max_dist=NO_CAP, bits=64, n=None, id_base=0):
    """vc_knn_vote*: (label, votes, total uint32 [n_rows], stats)"""
    n_rows, k = rows.shape
    n = len(labels) if n is None else n
    out = np.full(n_rows, NONE, dtype=np.uint32)
    votes, total = np.zeros(n_rows, dtype=np.uint32), np.zeros(n_rows, dtype=np.uint32)
    st = zero_vote_stats()
    for r in range(n_rows):
        c = int(counts[r]) if counts is not None else min(k, n)
        win, v, t, rule, voting = vote_segment(row_segment(rows[r], c, kk, max_dist), labels, kind, bits, NONE, id_base)
        out[r], votes[r], total[r] = win, v, t
        st["n_voted"] += rule != 0
        st["n_unlabelled"] += rule == 0
        st["n_ties"] += rule == 3
        st["n_entries"] += voting
    return out, votes, total, st


def propagate_round(offsets, adj, labels, seeds, kind, bits, id_base=0):
    """one synchronous round: (new labels, votes, total, changed, ties, records decided by rule 2)"""
    n = len(offsets) - 1
    new = labels.copy()
    votes, total = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    ties = rule2 = 0
    for i in range(n):
        cur = int(labels[i])
        win, v, t, rule, _ = vote_segment(adj[int(offsets[i]):int(offsets[i + 1])], labels, kind, bits, cur, id_base)
        votes[i], total[i] = v, t
        ties += rule == 3
        rule2 += rule == 2
        if rule:
            new[i] = win
        if seeds is not None and int(seeds[i]) != NONE:
            new[i] = seeds[i]
    return new, votes, total, int((new != labels).sum()), ties, rule2


def propagate_model(offsets, adj, labels_in, kind=COUNT, flags=0, max_iters=MAX_ITERS, bits=64, id_base=0, trace=None):
    """vc_label_propagate*: (labels, votes, total uint32 [N], stats); trace (a list) gets (changed, ties, rule 2) per round"""
    labels = np.array(labels_in, dtype=np.uint32)
    n = len(labels)
    st = zero_lp_stats()
    votes, total = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    if n == 0:
        return labels, votes, total, st
    seeds = labels.copy() if flags & CLAMP else None
    for _ in range(max_iters):
        labels, votes, total, changed, ties, rule2 = propagate_round(offsets, adj, labels, seeds, kind, bits, id_base)
        st["n_iters"] += 1
        st["n_changed_last"], st["n_ties_last"] = changed, ties
        if trace is not None:
            trace.append((changed, ties, rule2))
        if changed == 0:
            st["converged"] = 1
            break
    st["n_labelled"] = int((labels != NONE).sum())
    return labels, votes, total, st


def same_vote(got, want, what=None):
    assert got[3] == want[3], (what, "stats", got[3], want[3])
    for name, g, w in zip(("label", "votes", "total"), got[:3], want[:3]):
        bad = np.nonzero(np.asarray(g) != np.asarray(w))[0]
        assert len(bad) == 0, (what, name, len(bad), bad[:8], np.asarray(g)[bad[:8]], np.asarray(w)[bad[:8]])


# ---- the labelled inputs ---------------------------------------------------------------------------------------------------------------------------
K = 10
N_CLASSES = 5


@functools.lru_cache(maxsize=None)
def seeded_labels(bits, n=700, classes=N_CLASSES, unlabelled=0.6, seed=5):
    """a few classes at random, about 60 % VC_VOTE_NONE; the generator is seeded explicitly"""
    rng = np.random.default_rng(seed + bits)
    labels = rng.integers(0, classes, n).astype(np.uint32)
    labels[rng.random(n) < unlabelled] = NONE
    labels.setflags(write=False)
    return labels


@functools.lru_cache(maxsize=None)
def sparse_seeds(bits, n_seeds=40, n=700, classes=N_CLASSES, seed=9):
    """n_seeds labelled records, the rest unlabelled: the semi-supervised input"""
    rng = np.random.default_rng(seed + bits)
    labels = np.full(n, NONE, dtype=np.uint32)
    at = rng.choice(n, size=n_seeds, replace=False)
    labels[at] = rng.integers(0, classes, n_seeds).astype(np.uint32)
    labels.setflags(write=False)
    return labels


def community_labels(n, id_base=0):
    return (np.arange(n, dtype=np.uint64) + id_base).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def graph(bits):
    """(codes, rows, counts) of the 700 mixed records at k = 10"""
    return SN.mixed_graph(bits, K)


@functools.lru_cache(maxsize=None)
def adjacency(bits, flags, kk=K):
    _, rows, counts = graph(bits)
    offsets, adj, _ = KA.adjacency_model(rows, counts, kk, flags)
    offsets.setflags(write=False)
    adj.setflags(write=False)
    return offsets, adj


@functools.lru_cache(maxsize=None)
def vote_expected(bits, kk, kind, max_dist=NO_CAP):
    _, rows, counts = graph(bits)
    return vote_model(rows, counts, kk, seeded_labels(bits), kind, max_dist, bits)


@functools.lru_cache(maxsize=None)
def propagate_expected(bits, flags, form, max_iters, kind=COUNT):
    """form: "seeded" (the 60 %-unlabelled classes, clamped), "sparse" (40 seeds, clamped), "community" (labels = ids, no clamp)"""
    offsets, adj = adjacency(bits, flags)
    labels, lp_flags = form_input(bits, form)
    trace = []
    return propagate_model(offsets, adj, labels, kind, lp_flags, max_iters, bits, trace=trace), tuple(trace)


def form_input(bits, form):
    if form == "community":
        return community_labels(700), 0
    return (seeded_labels(bits) if form == "seeded" else sparse_seeds(bits)), CLAMP


def padded_rows(offsets, adj):
    """a CSR as rows of stride max degree with counts, for vc_knn_vote* over the same segments"""
    n = len(offsets) - 1
    deg = np.diff(offsets.astype(np.int64))
    k = max(int(deg.max()) if n else 1, 1)
    rows = np.full((n, k), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    for i in range(n):
        rows[i, :deg[i]] = adj[int(offsets[i]):int(offsets[i + 1])]
    return rows, deg.astype(np.uint32)
