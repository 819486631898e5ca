"""Shared by test_dbscan_levels_cpu.py and test_dbscan_levels_gpu.py (vc_dbscan_levels*, vc_sharded_dbscan_levels*): the engine-free
expectation.  Shapes and data are ids_common.py's, levels_common's even-parity store and dbscan_common's planted shape.

Level r of the call is vc_dbscan_radius at radius r, so the expectation of level r is dbscan_common.dbscan over the pairs of distance
<= r -- one DBSCAN per level, nothing carried from level to level.  What IS shared is levels_common's O(n^2) loop: the pairs of a
data set with their distances, once, at the largest radius.  core_dist comes from the sorted per-record distances, by a method that
shares nothing with dbscan's degrees.  `scheme` is the device's way on the host -- a pair in the forest of w = max(d, both core
distances) only, the cascade over the cores of the level below, anchor candidates of exactly one level plus their prefix minimum --
with a switch for each part, for test_dbscan_levels_cpu.py to pin against the per-level DBSCAN and to show that the data needs
every part.
Pairs are a << 32 | b with a < b, positions relative to id_base; labels come back relative too, `expect` adds id_base."""
import numpy as np

import cluster_common as CC
import dbscan_common as DC
import ids_common as I
import levels_common as LC

CORE_NEVER = 0xFFFFFFFF
FIELDS = ("n_pairs", "n_clusters", "n_core", "n_border", "n_noise")

_pairs, _expect = {}, {}


def shape(name):
    return DC.PLANTED[name] if name in DC.PLANTED else LC.shape(name)


def max_radius(name):
    """the levels of a shape in the tests: levels_common's, 0 .. 4 for the planted shape (PLANT_R = 2 in the middle)"""
    return 4 if name in DC.PLANTED else LC.max_radius(name)


def pairs_dist(name, radius=None):
    """(pairs, dist) within `radius` (default: max_radius): levels_common's, for the planted shape one brute-force loop of its own"""
    radius = max_radius(name) if radius is None else radius
    if name not in DC.PLANTED:
        return LC.pairs_dist(name, radius)
    if radius not in _pairs:
        p, d = LC.brute_pairs_dist(DC.planted_codes(), radius)
        p.setflags(write=False)
        d.setflags(write=False)
        _pairs[radius] = (p, d)
    return _pairs[radius]


def core_dist(n, pairs, dist, min_pts):
    """[n] int64: the min_pts-th smallest entry of a record's sorted distances -- to itself (0) and to every pair partner -- or
    CORE_NEVER where the list is shorter"""
    a, b = CC.split(pairs)
    rec = np.concatenate([np.arange(n, dtype=np.int64), a, b])
    d = np.concatenate([np.zeros(n, dtype=np.int64), dist, dist])
    assert d.max() < LC.LEVELS_MAX
    d = np.sort(rec * LC.LEVELS_MAX + d) % LC.LEVELS_MAX             # by record, then by distance
    count = np.bincount(rec, minlength=n)
    start = np.cumsum(count) - count
    cd = np.full(n, CORE_NEVER, dtype=np.int64)
    has = count >= min_pts
    cd[has] = d[start[has] + min_pts - 1]
    return cd


def per_level(n, pairs, dist, R, min_pts):
    """(labels [R + 1, n] int64, degrees [R + 1, n] int64, stats {field: uint64 [R + 1]}): dbscan_common.dbscan level by level"""
    labels, degrees = np.empty((R + 1, n), dtype=np.int64), np.empty((R + 1, n), dtype=np.int64)
    stats = {f: np.zeros(R + 1, dtype=np.uint64) for f in FIELDS}
    for r in range(R + 1):
        within = pairs[dist <= r]
        labels[r], degrees[r] = DC.dbscan(n, within, min_pts)
        st = DC.stats_of(labels[r], degrees[r], min_pts, within)
        for f in FIELDS[1:]:
            stats[f][r] = st[f]
    stats["n_pairs"] = np.bincount(dist, minlength=R + 1).astype(np.uint64)
    return labels, degrees, stats


def relative(name, min_pts, radius=None):
    """(labels [R + 1, n], core_dist [n], stats) relative to id_base of a shape's data, computed once; never written to"""
    radius = max_radius(name) if radius is None else radius
    s = shape(name)
    key = (name in DC.PLANTED, name == "EVEN", s["bits"], s["n"], radius, min_pts)
    if key not in _expect:
        p, d = pairs_dist(name, radius)
        lab, deg, stats = per_level(s["n"], p, d, radius, min_pts)
        cd = core_dist(s["n"], p, d, min_pts)
        assert all(np.array_equal(cd <= r, deg[r] >= min_pts) for r in range(radius + 1))
        for arr in (lab, cd) + tuple(stats.values()):
            arr.setflags(write=False)
        _expect[key] = (lab, cd, stats)
    return _expect[key]


def expect(name, min_pts, radius=None, base=None):
    """what vc_dbscan_levels returns: (labels uint32 GLOBAL ids [R + 1, n], core_dist uint32 [n], stats)"""
    lab, cd, stats = relative(name, min_pts, radius)
    base = shape(name)["id_base"] if base is None else base
    return (lab + base).astype(np.uint32), cd.astype(np.uint32), stats


def _lower(anchor, level, sparse, cand):
    """anchor[level, sparse] = min(itself, cand), entry by entry"""
    flat = anchor.reshape(-1)
    np.minimum.at(flat, level * anchor.shape[1] + sparse, cand)


def scheme(n, pairs, dist, R, min_pts, cascade=True, unite_at_w=True, prefix_min=True):
    """THE DEVICE'S WAY on the host, returns labels [R + 1, n].  cd = core_dist.  One forest per level: a pair {a, b} of distance d
    is united in forest w = max(d, cd[a], cd[b]) ONLY; then, for r = 1 .. R, every record with cd <= r - 1 that is no root at level
    r - 1 is united at level r with its root of level r - 1.  Anchors: slot (t, i) with t < cd[i] holds the smallest v with
    max(d(i, v), cd[v]) == t (n: none); the anchor of a non-core i at level r is the minimum of its slots (t <= r, i).  A core takes its
    root, a non-core the root of its anchor or its own id.  The three switches take one part out each (broken on purpose)."""
    a, b = CC.split(pairs)
    cd = core_dist(n, pairs, dist, min_pts)
    w = np.maximum(dist, np.maximum(cd[a], cd[b])) if unite_at_w else dist
    forests = [CC.union_find(n, pairs[w == r]) for r in range(R + 1)]
    if cascade:
        for r in range(1, R + 1):
            below = forests[r - 1]                                   # final and flat: below[i] is the root of i
            member = np.flatnonzero((cd <= r - 1) & (below != np.arange(n)))
            links = (below[member].astype(np.uint64) << I.SH) | member.astype(np.uint64)
            forests[r] = CC.union_find(n, links, init=forests[r])
    anchor = np.full((R + 1, n), n, dtype=np.int64)
    for x, v in ((a, b), (b, a)):                                    # v a core neighbour of x from level t on
        t = np.maximum(dist, cd[v])
        act = (t < cd[x]) & (t <= R)
        _lower(anchor, t[act], x[act], v[act])
    if prefix_min:
        anchor = np.minimum.accumulate(anchor, axis=0)
    out = np.empty((R + 1, n), dtype=np.int64)
    own = np.arange(n)
    for r in range(R + 1):
        core = cd <= r
        border = ~core & (anchor[r] < n)
        out[r] = np.where(core, forests[r], own)
        out[r, border] = forests[r][anchor[r, border]]
    return out
