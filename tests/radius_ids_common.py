"""Shared by test_radius_ids_cpu.py and test_radius_ids_gpu.py (vc_search_radius_ids*, vc_sharded_search_radius_ids*): the
engine-free expectation.  Shapes, data and id lists are ids_common.py's.

The expectation of one id: brute-force distances of its record to every record, the entries within the radius, sorted packed --
what the radius search returns for the code of that record -- then the two flag rules: VC_IDS_EXCLUDE_SELF drops the entry
(0, own id) by value, VC_IDS_ONLY_GREATER every entry whose id is <= the own id.  An id that is not resident owns nothing."""
import numpy as np

import ids_common as I

EXCLUDE_SELF = 0x1
ONLY_GREATER = 0x2
FLAG_SETS = (0, EXCLUDE_SELF, ONLY_GREATER, EXCLUDE_SELF | ONLY_GREATER)
LOW = np.uint64(0xFFFFFFFF)
# the radii of the single-engine cases per shape: 0, 3, 6 and twice the flips of the data (two members of a cluster differ in at
# most that many bits, so the last radius takes in the query's whole cluster)
RADII = {name: (0, 3, 6, 2 * s["flips"]) for name, s in I.SHAPES.items()}

_sorted = {}


def sorted_row(name, pos):
    """all records in ascending packed (dist, id) order of their distance to record `pos` (ids relative to id_base), shared by
    every radius and flag set; never written to"""
    s = I.SHAPES[name]
    key = (s["bits"], s["n"], pos)
    if key not in _sorted:
        codes = I.codes_of(name)
        row = np.sort(I.pack(I.distances(codes, codes[pos]), np.arange(len(codes), dtype=np.uint64)))
        row.setflags(write=False)
        _sorted[key] = row
    return _sorted[key]


def apply_flags(seg, qid, id_flags):
    """the two flag rules on one ascending segment (global ids)"""
    seg = np.asarray(seg, dtype=np.uint64)
    if id_flags & EXCLUDE_SELF:
        seg = seg[seg != np.uint64(qid)]
    if id_flags & ONLY_GREATER:
        seg = seg[(seg & LOW) > np.uint64(qid)]
    return seg


def expect(name, qid, radius, id_flags=0):
    """the segment of the id qid (global): empty when it is not resident"""
    s = I.SHAPES[name]
    pos = int(qid) - s["id_base"]
    if not 0 <= pos < s["n"]:
        return np.zeros(0, dtype=np.uint64)
    row = sorted_row(name, pos)
    seg = row[:np.searchsorted(row, np.uint64(radius + 1) << I.SH)] + np.uint64(s["id_base"])
    return apply_flags(seg, qid, id_flags)


def expect_batch(name, ids, radius, id_flags=0):
    """(offsets [nq + 1], flat results) of a batch"""
    segs = [expect(name, q, radius, id_flags) for q in ids]
    offs = np.zeros(len(ids) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in segs])
    return offs, (np.concatenate(segs) if segs else np.zeros(0, dtype=np.uint64)), segs


def self_position(seg, qid):
    """where the own entry sits in the distance-0 run of an unflagged segment: 'only', 'first', 'mid' or 'last'"""
    run = seg[(seg >> I.SH) == 0]
    at = int(np.flatnonzero(run == np.uint64(qid))[0])
    if len(run) == 1:
        return "only"
    return "first" if at == 0 else ("last" if at == len(run) - 1 else "mid")


def brute_pairs(name, radius):
    """every unordered pair {a < b} of records (ids relative to id_base) within `radius`, as a sorted array of a << 32 | b"""
    codes = I.codes_of(name)
    out = []
    for a in range(len(codes) - 1):
        d = I.distances(codes[a + 1:], codes[a])
        b = np.flatnonzero(d <= radius).astype(np.uint64) + np.uint64(a + 1)
        out.append((np.uint64(a) << I.SH) | b)
    return np.sort(np.concatenate(out))


def edge_list(name):
    """ids with a missing id first, in the middle and last (ids_common.id_list starts every list with a resident id): the
    segments behind an empty one shift, and the batch begins and ends with an empty segment"""
    s = I.SHAPES[name]
    base, n = s["id_base"], s["n"]
    missing = base + n if base + n < 2 ** 32 else base - 1
    return np.array([0xFFFFFFFF, base, base + n - 1, missing, base + n // 2, base + 1, missing], dtype=np.uint32)
