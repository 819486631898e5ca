"""Shared by test_dbscan_cpu.py and test_dbscan_gpu.py (vc_dbscan_radius*, vc_sharded_dbscan_radius*): the engine-free expectation.
Shapes and data are ids_common.py's plus one planted shape, the pairs cluster_common.pairs_of's (radius_ids_common.brute_pairs).

degrees[i] = 1 + the pairs record i is a member of (the record itself is counted); record i is a CORE iff degrees[i] >= min_pts;
a core's label is the smallest id among the cores of its component in the graph of the core-core pairs; a BORDER (a non-core record
with a core neighbour) takes the label of its SMALLEST-ID core neighbour; NOISE keeps its own id.  A function of the data, the
radius and min_pts only, so it is computed here twice, by two methods that share nothing but the pair list:
  dbscan     cluster_common.union_find over the core-core pairs, the anchors by np.minimum.at;
  dbscan_b   cluster_common.propagate over the core-core pairs, the anchors by a loop over the records.
Pairs are a << 32 | b with a < b, positions relative to id_base; labels come back relative too, `expect` adds id_base.

P64 / PH3 is the planted shape: 450 uniform random 64-bit records (none has a neighbour within PLANT_R) with five BRIDGES planted at
PLANT_R = 2, PLANT_MIN_PTS = 4.  A bridge is, XOR a random 64-bit base of its own (which keeps the distances inside it and puts the
bridges about 32 bits apart):
  a0 = 0, a1..a3 = a0 with bit 10, 11 or 12 set       group A: pairwise within 2, so four cores
  b0 = bits 0..3, b1..b3 = b0 with bit 20, 21 or 22   group B: the same; A and B are at least 4 apart
  X  = bits 0 and 1                                   2 from a0 and from b0 only: degree 3, a border CONTESTED between A and B
The bridges differ in where their members sit in id order, see BRIDGES.  PH3 holds the same records over 3 shards of 200 ids."""
import numpy as np

import cluster_common as CC
import ids_common as I

RADII = (0, 3, 6)
MIN_PTS = (1, 3, 8, 64)
PLANT_R, PLANT_MIN_PTS = 2, 4
PLANT_BATCHES = (1, 7, 257)

PLANTED = {
    "P64": dict(bits=64, m=2, n=450, capacity=512, id_base=9, shards=0),
    "PH3": dict(bits=64, m=2, n=450, capacity=600, id_base=2 ** 31 + 5, shards=3),      # shards of 200, 200 and 50 records
}
# positions (ids relative to id_base) of a0..a3, b0..b3 and the X records of every bridge
BRIDGES = {
    # X below both anchors; X, a0 and b0 in one batch of 7
    "x_below": dict(a=(15, 17, 18, 19), b=(16, 21, 22, 23), x=(14,)),
    # X between the groups; a batch boundary of 257 between X and b0
    "x_between": dict(a=(100, 101, 102, 103), b=(300, 301, 302, 303), x=(230,)),
    # X above both; X is the first record of PH3's shard 1, its anchors lie in shard 0; all in the first batch of 257
    "x_above": dict(a=(40, 41, 42, 43), b=(44, 45, 46, 47), x=(200,)),
    # group A owns the smallest id (a1 = 60) while b0 = 61 < a0 = 62: "smallest core neighbour" says B (61), "smallest label" says A (60)
    "rules_disagree": dict(a=(62, 60, 63, 64), b=(61, 65, 66, 67), x=(420,)),
    # X twice: both X have degree 4, are cores and weld A and B into one cluster of ten
    "x_twice": dict(a=(120, 121, 122, 123), b=(350, 351, 352, 353), x=(10, 440)),
}
CONTESTED = ("x_below", "x_between", "x_above", "rules_disagree")

_codes, _pairs, _expect = {}, {}, {}


def shape(name):
    return PLANTED[name] if name in PLANTED else I.SHAPES[name]


def _bit(*positions):
    return sum(1 << p for p in positions)


def planted_codes():
    if "planted" not in _codes:
        n = PLANTED["P64"]["n"]
        rng = np.random.default_rng(64450)
        words = rng.integers(0, 2 ** 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
        a0, b0, x = 0, _bit(0, 1, 2, 3), _bit(0, 1)
        for br in BRIDGES.values():
            base = int(rng.integers(0, 2 ** 63, dtype=np.uint64)) * 2 + int(rng.integers(0, 2))
            members = [a0, a0 | _bit(10), a0 | _bit(11), a0 | _bit(12), b0, b0 | _bit(20), b0 | _bit(21), b0 | _bit(22)] + [x] * len(br["x"])
            for pos, code in zip(br["a"] + br["b"] + br["x"], members):
                words[pos] = np.uint64(code ^ base)
        codes = np.ascontiguousarray(words.astype("<u8")).view(np.uint8).reshape(n, 8).copy()
        codes.setflags(write=False)
        _codes["planted"] = codes
    return _codes["planted"]


def codes_of(name):
    return planted_codes() if name in PLANTED else I.codes_of(name)


def brute_pairs(codes, radius):
    """radius_ids_common.brute_pairs for any array of codes"""
    out = [np.zeros(0, dtype=np.uint64)]
    for a in range(len(codes) - 1):
        b = np.flatnonzero(I.distances(codes[a + 1:], codes[a]) <= radius).astype(np.uint64) + np.uint64(a + 1)
        out.append((np.uint64(a) << I.SH) | b)
    return np.sort(np.concatenate(out))


def pairs_of(name, radius):
    if name not in PLANTED:
        return CC.pairs_of(name, radius)
    if radius not in _pairs:
        p = brute_pairs(planted_codes(), radius)
        p.setflags(write=False)
        _pairs[radius] = p
    return _pairs[radius]


def degrees_of(n, pairs):
    a, b = CC.split(pairs)
    return 1 + np.bincount(a, minlength=n) + np.bincount(b, minlength=n)


def dbscan(n, pairs, min_pts, by_label=False):
    """(labels [n] int64, degrees [n] int64).  by_label: the OTHER tie-break of a contested border, the smallest LABEL among its core
    neighbours -- not the contract, only there to show that the data tells the two rules apart"""
    a, b = CC.split(pairs)
    deg = degrees_of(n, pairs)
    core = deg >= min_pts
    lab = CC.union_find(n, pairs[core[a] & core[b]])
    key = lab if by_label else np.arange(n, dtype=np.int64)
    anchor = np.full(n, n, dtype=np.int64)
    up, down = core[a] & ~core[b], ~core[a] & core[b]
    np.minimum.at(anchor, b[up], key[a[up]])
    np.minimum.at(anchor, a[down], key[b[down]])
    border = ~core & (anchor < n)
    lab[border] = lab[anchor[border]]
    return lab, deg


def dbscan_b(n, pairs, min_pts):
    """the second method: min-label propagation over the core-core pairs, then one record after the other"""
    a, b = CC.split(pairs)
    nb = [[] for _ in range(n)]
    for x, y in zip(a.tolist(), b.tolist()):
        nb[x].append(y)
        nb[y].append(x)
    deg = np.array([1 + len(v) for v in nb], dtype=np.int64)
    core = deg >= min_pts
    lab = CC.propagate(n, pairs[core[a] & core[b]])
    out = lab.copy()
    for i in range(n):
        if not core[i]:
            cores = [v for v in nb[i] if core[v]]
            out[i] = lab[min(cores)] if cores else i
    return out, deg


def kinds(lab, deg, min_pts):
    """(core, border, noise) masks"""
    own = np.arange(len(lab))
    core = deg >= min_pts
    return core, ~core & (lab != own), ~core & (lab == own)


def stats_of(lab, deg, min_pts, pairs):
    core, border, noise = kinds(lab, deg, min_pts)
    return dict(n_pairs=len(pairs), n_clusters=len(np.unique(lab[core])), n_core=int(core.sum()), n_border=int(border.sum()), n_noise=int(noise.sum()))


def expect_codes(codes, radius, min_pts, id_base):
    """what vc_dbscan_radius returns for any array of codes: (labels uint32 GLOBAL ids, degrees uint32, stats)"""
    pairs = brute_pairs(codes, radius)
    lab, deg = dbscan(len(codes), pairs, min_pts)
    return (lab + id_base).astype(np.uint32), deg.astype(np.uint32), stats_of(lab, deg, min_pts, pairs)


def relative(name, radius, min_pts):
    """(labels, degrees) relative to id_base (int64) and the stats of a shape's data, computed once by dbscan; never written to"""
    s = shape(name)
    key = (s["bits"], s["n"], name in PLANTED, radius, min_pts)
    if key not in _expect:
        pairs = pairs_of(name, radius)
        lab, deg = dbscan(s["n"], pairs, min_pts)
        lab.setflags(write=False)
        deg.setflags(write=False)
        _expect[key] = (lab, deg, stats_of(lab, deg, min_pts, pairs))
    return _expect[key]


def expect(name, radius, min_pts):
    """what vc_dbscan_radius returns: (labels uint32 GLOBAL ids, degrees uint32, stats)"""
    lab, deg, stats = relative(name, radius, min_pts)
    return (lab + shape(name)["id_base"]).astype(np.uint32), deg.astype(np.uint32), stats


def batch_of(pos, batch):
    return pos // batch
