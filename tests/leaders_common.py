"""Shared by test_leaders_cpu.py and test_leaders_gpu.py (vc_leaders_radius*, vc_sharded_leaders_radius*): the engine-free
expectation.  Shapes and data are ids_common.py's, the pairs cluster_common.pairs_of's (radius_ids_common.brute_pairs).

Record i is a LEADER iff no leader with a smaller id lies within the radius of it; its label is its own id then, otherwise the
smallest-id leader within the radius -- a function of the data and the radius only -- so it is computed here twice, by two methods
that share nothing but the pair list:
  greedy   the sequential one-pass rule: walk the records in id order, keep a record iff no kept record so far is adjacent;
  rounds   synchronous rounds of the EAGER rule over all records at once (an undecided record is dropped as soon as one smaller
           neighbour is a decided leader, a leader when all its smaller neighbours are decided and dropped), then the assign
           pass: a dropped record takes the minimum over ALL its leader neighbours.  Also returns the rounds that had work.
Pairs are a << 32 | b with a < b, positions relative to id_base; labels come back relative too, `expect` adds id_base.

T512 is the thermometer data set: 513 records of 512 bits, record i has its first i bits set, so records i and j are |i - j| bits
apart and the rule has the closed form label[i] = i - i % (R + 1).  One batch of it needs 513 rounds at R = 1: a dependency chain
through every record, deeper than any group of rounds the driver enqueues between two read-backs."""
import numpy as np

import cluster_common as CC
import ids_common as I

RADII = CC.RADII
T512 = dict(bits=512, m=16, n=513, capacity=513, id_base=5)
T512_RADII = (1, 2, 5)

_labels = {}


def _smaller_neighbours(n, pairs):
    """(a sorted by b, start[n + 1]): the neighbours a < b of record b are a2[start[b] : start[b + 1]]"""
    a, b = CC.split(pairs)
    order = np.argsort(b, kind="stable")
    start = np.zeros(n + 1, dtype=np.int64)
    start[1:] = np.cumsum(np.bincount(b, minlength=n))
    return a[order], start


def greedy(n, pairs):
    """labels [n] (int64): one record after the other, in id order"""
    a2, start = _smaller_neighbours(n, pairs)
    lab = np.arange(n, dtype=np.int64)
    leader = np.zeros(n, dtype=bool)
    for i in range(n):
        nb = a2[start[i]:start[i + 1]]
        lead = nb[leader[nb]]
        if len(lead):
            lab[i] = lead.min()
        else:
            leader[i] = True
    return lab


UNDECIDED, LEADER, DROPPED = 0, 1, 2


def rounds(n, pairs):
    """(labels [n] int64, rounds): every round reads the state the previous round left"""
    a, b = CC.split(pairs)
    state = np.full(n, UNDECIDED, dtype=np.int8)
    la, lb = a, b                                   # the pairs whose larger member is still undecided
    n_rounds = 0
    while np.any(state == UNDECIDED):
        n_rounds += 1
        sa = state[la]
        has_leader = np.bincount(lb[sa == LEADER], minlength=n) > 0
        blocked = np.bincount(lb[sa == UNDECIDED], minlength=n) > 0
        und = state == UNDECIDED
        new = state.copy()
        new[und & has_leader] = DROPPED             # eager: one decided leader is enough
        new[und & ~has_leader & ~blocked] = LEADER
        assert not np.array_equal(new, state)       # the smallest undecided id is decided in every round
        state = new
        live = state[lb] == UNDECIDED
        la, lb = la[live], lb[live]
    lab = np.arange(n, dtype=np.int64)
    m = (state[a] == LEADER) & (state[b] == DROPPED)
    np.minimum.at(lab, b[m], a[m])                  # the assign pass: the minimum over ALL leader neighbours
    return lab, n_rounds


def labels_of(name, radius):
    """labels relative to id_base (int64) of a shape's data at a radius, computed once by greedy; never written to"""
    key = CC._key(name) + (radius,)
    if key not in _labels:
        lab = greedy(I.SHAPES[name]["n"], CC.pairs_of(name, radius))
        lab.setflags(write=False)
        _labels[key] = lab
    return _labels[key]


def expect(name, radius):
    """what vc_leaders_radius returns: uint32 GLOBAL ids"""
    return (labels_of(name, radius) + I.SHAPES[name]["id_base"]).astype(np.uint32)


def n_leaders(labels):
    """the leaders of a labels array in either id space: every label names a leader and a leader is labelled with itself, so the
    leaders are the distinct labels"""
    return len(np.unique(labels))


def old_labels(name, radius):
    """the labels (relative) of the first cluster_common.n_old records ALONE"""
    k = CC.n_old(name)
    p = CC.pairs_of(name, radius)
    return greedy(k, p[CC.split(p)[1] < k])


def far_members(lab, pairs):
    """members (label != own id) that are NOT within the radius of their label"""
    member = np.flatnonzero(lab != np.arange(len(lab)))
    link = (lab[member].astype(np.uint64) << I.SH) | member.astype(np.uint64)
    return int(np.count_nonzero(~np.isin(link, pairs)))


def close_leaders(lab, pairs):
    """pairs of leaders within the radius of each other"""
    a, b = CC.split(pairs)
    own = np.arange(len(lab))
    return int(np.count_nonzero((lab[a] == own[a]) & (lab[b] == own[b])))


# ---- the thermometer data set ------------------------------------------------------------------------------------------------------
def t512_codes():
    n, nbytes = T512["n"], T512["bits"] // 8
    bits = (np.arange(T512["bits"])[None, :] < np.arange(n)[:, None]).astype(np.uint8)        # record i: bits 0 .. i - 1
    codes = np.zeros((n, nbytes), dtype=np.uint8)
    for j in range(8):
        codes |= bits[:, j::8] << np.uint8(j)
    return codes


def t512_pairs(radius):
    n = T512["n"]
    a = np.repeat(np.arange(n, dtype=np.uint64), radius)
    b = a + np.tile(np.arange(1, radius + 1, dtype=np.uint64), n)
    keep = b < n
    return np.sort((a[keep] << I.SH) | b[keep])


def t512_labels(radius):
    """the closed form, relative: the leaders are the multiples of R + 1"""
    i = np.arange(T512["n"], dtype=np.int64)
    return i - i % (radius + 1)


def t512_expect(radius):
    return (t512_labels(radius) + T512["id_base"]).astype(np.uint32)
