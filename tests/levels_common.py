"""Shared by test_levels_cpu.py and test_levels_gpu.py (vc_cluster_levels*, vc_sharded_cluster_levels*): the engine-free
expectation.  Shapes and data are ids_common.py's, the union-find cluster_common.py's.

Level r of the call is vc_cluster_radius at radius r, so the expectation of level r is cluster_common.union_find over the pairs of
distance <= r -- one union-find per level, nothing carried from level to level.  What IS shared is the O(n^2) loop: the pairs of a
data set are computed once, WITH their distances, at the largest radius (twice the flips of the data); level r's pairs are those
with d <= r, and the histogram is a bincount.  `scheme` is the device's way (a pair in the forest of its distance only, then the
cascade), on the host, for test_levels_cpu.py to pin against the per-level union-find.
Pairs are a << 32 | b with a < b, positions relative to id_base; labels come back relative too, `expect` adds id_base."""
import numpy as np

import cluster_common as CC
import ids_common as I

LEVELS_MAX = 64

# A 64-bit store of even-popcount codes: every distance between two of them is even, so the odd levels have no pairs of their own
# and only the cascade writes them.  Three centres of even weight, 0 / 2 / 4 flips each.
EVEN = dict(bits=64, m=2, n=300, capacity=512, id_base=2 ** 31 - 150, centres=3, flips=4, shards=0)

_codes, _pairs, _labels = {}, {}, {}


def shape(name):
    return EVEN if name == "EVEN" else I.SHAPES[name]


def max_radius(name):
    """the levels of a shape in the tests: 0 .. twice the flips of its data (the last level takes in whole clusters)"""
    return 2 * shape(name)["flips"]


def codes_of(name):
    if name != "EVEN":
        return I.codes_of(name)
    if name not in _codes:
        s = EVEN
        rng = np.random.default_rng(6400300)
        centres = rng.integers(0, 256, size=(s["centres"], 8), dtype=np.uint8)
        for c in centres:                                           # even weight: flip bit 0 where it is odd
            if int(np.unpackbits(c).sum()) % 2:
                c[0] ^= np.uint8(1)
        codes = centres[rng.integers(0, s["centres"], size=s["n"])].copy()
        for i in range(s["n"]):
            for b in rng.choice(64, size=2 * int(rng.integers(0, s["flips"] // 2 + 1)), replace=False):
                codes[i, b // 8] ^= np.uint8(1 << (b % 8))
        codes.setflags(write=False)
        _codes[name] = codes
    return _codes[name]


def _key(name):
    s = shape(name)
    return (name == "EVEN", s["bits"], s["n"], s["centres"], s["flips"])


def brute_pairs_dist(codes, radius):
    """every unordered pair {a < b} within `radius`, ascending a << 32 | b, and its distance: (pairs uint64, dist int64)"""
    ps, ds = [np.zeros(0, dtype=np.uint64)], [np.zeros(0, dtype=np.int64)]
    for a in range(len(codes) - 1):
        d = I.distances(codes[a + 1:], codes[a])
        b = np.flatnonzero(d <= radius)
        ps.append((np.uint64(a) << I.SH) | (b.astype(np.uint64) + np.uint64(a + 1)))
        ds.append(d[b].astype(np.int64))
    return np.concatenate(ps), np.concatenate(ds)


def pairs_dist(name, radius=None):
    """(pairs, dist) of a shape within `radius` (default: max_radius): ONE brute-force loop per data set, at max_radius, cut by
    distance for every smaller radius (a larger radius has a loop of its own); never written to"""
    top = max_radius(name)
    radius = top if radius is None else radius
    key = _key(name) + (max(radius, top),)
    if key not in _pairs:
        p, d = brute_pairs_dist(codes_of(name), max(radius, top))
        p.setflags(write=False)
        d.setflags(write=False)
        _pairs[key] = (p, d)
    p, d = _pairs[key]
    return (p, d) if radius >= top else (p[d <= radius], d[d <= radius])


def levels_from(n, pairs, dist, R, n_first=None):
    """labels [R + 1, n] (int64, relative): one cluster_common.union_find per level over the pairs with d <= r.  n_first: over the
    first n_first records ALONE ([R + 1, n_first])"""
    if n_first is not None:
        keep = CC.split(pairs)[1] < n_first
        pairs, dist, n = pairs[keep], dist[keep], n_first
    return np.stack([CC.union_find(n, pairs[dist <= r]) for r in range(R + 1)])


def labels_of(name, radius=None):
    """labels [R + 1, n] relative to id_base of a shape, computed once at max_radius (its first rows serve every smaller radius);
    never written to"""
    top = max_radius(name)
    radius = top if radius is None else radius
    key = _key(name) + (max(radius, top),)
    if key not in _labels:
        p, d = pairs_dist(name, max(radius, top))
        lab = levels_from(shape(name)["n"], p, d, max(radius, top))
        lab.setflags(write=False)
        _labels[key] = lab
    return _labels[key][:radius + 1]


def expect(name, radius=None, base=None):
    """what vc_cluster_levels returns: uint32 GLOBAL ids, [R + 1, n]"""
    base = shape(name)["id_base"] if base is None else base
    return (labels_of(name, radius) + base).astype(np.uint32)


def histogram(name, radius=None, n_labelled=0):
    """n_pairs [R + 1]: the pairs at distance exactly d whose larger member is not labelled yet"""
    radius = max_radius(name) if radius is None else radius
    p, d = pairs_dist(name, radius)
    return np.bincount(d[CC.split(p)[1] >= n_labelled], minlength=radius + 1).astype(np.uint64)


def cluster_counts(labels):
    """n_clusters [R + 1] of a [R + 1, n] label array"""
    return np.array([len(np.unique(row)) for row in labels], dtype=np.uint64)


def old_labels(name, n_first, radius=None):
    """[R + 1, n_first]: the levels of the first n_first records ALONE -- what a store that held only them would have returned"""
    radius = max_radius(name) if radius is None else radius
    p, d = pairs_dist(name, radius)
    return levels_from(shape(name)["n"], p, d, radius, n_first=n_first)


def scheme(n, pairs, dist, R, old=None):
    """THE DEVICE'S WAY on the host.  One forest per level; a pair of distance d is united in forest d ONLY; then, for r = 1 .. R,
    every record that is no root at level r - 1 is united at level r with its root of level r - 1.  `old` [R + 1, k]: the
    incoming labels of the incremental form -- `pairs` then are the keep rule's (larger member >= k).  Returns [R + 1, n]."""
    forests = [CC.union_find(n, pairs[dist == r], init=None if old is None else old[r]) for r in range(R + 1)]
    for r in range(1, R + 1):
        below = forests[r - 1]                                       # final and flat: below[i] is the root of i
        member = np.flatnonzero(below != np.arange(n))
        links = (below[member].astype(np.uint64) << I.SH) | member.astype(np.uint64)
        forests[r] = CC.union_find(n, links, init=forests[r])
    return np.stack(forests)

