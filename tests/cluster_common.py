"""Shared by test_cluster_cpu.py and test_cluster_gpu.py (vc_cluster_radius*, vc_sharded_cluster_radius*): the engine-free
expectation.  Shapes and data are ids_common.py's, the pairs radius_ids_common.brute_pairs'.

The label of a record is the smallest id of its connected component in the radius graph -- a function of the data and the radius
only -- so it is computed here twice, by two methods that share nothing but the pair list:
  union_find   a union-find that hooks the larger root under the smaller (the device's rule, run one pair after the other);
  propagate    min-label propagation over the pair list, iterated to a fixed point.
Pairs are a << 32 | b with a < b, positions relative to id_base; labels come back relative too, `expect` adds id_base."""
import numpy as np

import ids_common as I
import radius_ids_common as R

RADII = R.RADII
OLD_SHARE = 0.6           # the incremental cases: the first 60 % of the records are the old part

_pairs, _labels = {}, {}


def _key(name):
    s = I.SHAPES[name]
    return (s["bits"], s["n"], s["centres"], s["flips"])


def pairs_of(name, radius):
    """radius_ids_common.brute_pairs, computed once per data set and radius; never written to"""
    key = _key(name) + (radius,)
    if key not in _pairs:
        bits, n = I.SHAPES[name]["bits"], I.SHAPES[name]["n"]
        p = np.zeros(0, dtype=np.uint64) if n < 2 else (R.brute_pairs(name, radius) if radius < bits else _all_pairs(n))
        p.setflags(write=False)
        _pairs[key] = p
    return _pairs[key]


def _all_pairs(n):
    a, b = np.triu_indices(n, 1)
    return (a.astype(np.uint64) << I.SH) | b.astype(np.uint64)


def split(pairs):
    pairs = np.asarray(pairs, dtype=np.uint64)
    return (pairs >> I.SH).astype(np.int64), (pairs & R.LOW).astype(np.int64)


def _roots(parent):
    """every record's root, by pointer jumping on a copy"""
    r = parent.copy()
    while True:
        nxt = r[r]
        if np.array_equal(nxt, r):
            return r
        r = nxt


def union_find(n, pairs, init=None):
    """labels [n] (int64) = the smallest id of each component.  One pair after the other: find both roots with path halving,
    hook the LARGER root under the smaller.  `init`: a forest to go on from (labels of an earlier call; records behind it start
    as their own roots).  Only to keep millions of pairs affordable the pairs are taken in growing chunks, and a chunk first
    drops the pairs that the forest as it stands connects already: they would find equal roots and do nothing."""
    parent = np.arange(n, dtype=np.int64)
    if init is not None:
        parent[:len(init)] = init
    a, b = split(pairs)
    lo, step = 0, 256
    while lo < len(a):
        ca, cb = a[lo:lo + step], b[lo:lo + step]
        lo, step = lo + step, step * 2
        r = _roots(parent)
        live = np.flatnonzero(r[ca] != r[cb])
        par = parent.tolist()
        for x, y in zip(ca[live].tolist(), cb[live].tolist()):
            while par[x] != x:
                par[x] = par[par[x]]
                x = par[x]
            while par[y] != y:
                par[y] = par[par[y]]
                y = par[y]
            if x != y:
                par[max(x, y)] = min(x, y)
        parent = np.array(par, dtype=np.int64)
    return _roots(parent)


def propagate(n, pairs):
    """labels [n] by iterated min-label propagation: every record takes the smallest label among itself and its neighbours, until
    nothing changes.  No forest, no roots: independent of union_find."""
    a, b = split(pairs)
    lab = np.arange(n, dtype=np.int64)
    if len(a) == 0:
        return lab
    by_b = np.argsort(b, kind="stable")
    a2, b2 = a[by_b], b[by_b]
    start_a = np.flatnonzero(np.r_[True, a[1:] != a[:-1]])      # (the pairs are sorted: grouped by a already)
    start_b = np.flatnonzero(np.r_[True, b2[1:] != b2[:-1]])
    while True:
        new = lab.copy()
        new[a[start_a]] = np.minimum(new[a[start_a]], np.minimum.reduceat(lab[b], start_a))
        new[b2[start_b]] = np.minimum(new[b2[start_b]], np.minimum.reduceat(lab[a2], start_b))
        if np.array_equal(new, lab):
            return lab
        lab = new


def labels_of(name, radius):
    """labels relative to id_base (int64) of a shape's data at a radius, computed once by union_find; never written to"""
    key = _key(name) + (radius,)
    if key not in _labels:
        lab = union_find(I.SHAPES[name]["n"], pairs_of(name, radius))
        lab.setflags(write=False)
        _labels[key] = lab
    return _labels[key]


def expect(name, radius):
    """what vc_cluster_radius returns: uint32 GLOBAL ids"""
    return (labels_of(name, radius) + I.SHAPES[name]["id_base"]).astype(np.uint32)


def n_pairs(name, radius, n_labelled=0):
    """the pairs a call examines: those whose larger member is not labelled yet"""
    return int(np.count_nonzero(split(pairs_of(name, radius))[1] >= n_labelled))


def n_clusters(labels):
    return len(np.unique(labels))


def n_old(name):
    return int(I.SHAPES[name]["n"] * OLD_SHARE)


def old_labels(name, radius):
    """the labels (relative) of the first n_old records ALONE: what a store that held only them would have returned"""
    k = n_old(name)
    p = pairs_of(name, radius)
    return union_find(k, p[split(p)[1] < k])


def kept_entries(n, pairs, n_labelled):
    """THE KEEP RULE, entry by entry: the records n_labelled .. n - 1 are queried, a query q finds itself and every neighbour v, and
    keeps v when v > q or v < n_labelled.  Returns the kept (q, v) as min << 32 | max, in the order they are met."""
    a, b = split(pairs)
    out = []
    for q in range(n_labelled, n):
        found = np.concatenate([[q], b[a == q], a[b == q]])
        for v in found.tolist():
            if v > q or v < n_labelled:
                out.append((min(q, v) << 32) | max(q, v))
    return np.array(out, dtype=np.uint64)


def figures(name, radius):
    """(clusters, singletons, largest cluster, members not adjacent to their own label)"""
    lab = labels_of(name, radius)
    _, counts = np.unique(lab, return_counts=True)
    member = np.flatnonzero(lab != np.arange(len(lab)))
    link = (lab[member].astype(np.uint64) << I.SH) | member.astype(np.uint64)
    far = int(np.count_nonzero(~np.isin(link, pairs_of(name, radius))))
    return len(counts), int(np.count_nonzero(counts == 1)), int(counts.max()), far
