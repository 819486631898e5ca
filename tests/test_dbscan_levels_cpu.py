"""Density clustering at every radius in one walk, without a GPU: the ABI surface, the code object of the four kernels, and the
expectation of test_dbscan_levels_gpu.py -- that the device's scheme (a pair in the forest of its mutual-reachability distance only,
the cascade over the cores of the level below, anchor candidates of exactly one level and their prefix minimum) gives the per-radius
DBSCAN at every level, that the core distance is the degree test of every level, and that the data cannot pass without any one part."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

import cluster_common as CC
import dbscan_common as DC
import dbscan_levels_common as DL
import levels_common as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vc_dbscan_levels", "vc_dbscan_levels_dev", "vc_sharded_dbscan_levels", "vc_sharded_dbscan_levels_dev"]
KERNELS = ("vc_dbscan_levels_core_kernel", "vc_dbscan_levels_edge_kernel", "vc_dbscan_levels_cascade_kernel", "vc_dbscan_levels_finish_kernel")
# LDS of the object: the edge kernel's histogram (64 counters of 32 bits) and the finish kernel's 4 x 64 counters; nothing else
LDS_BYTES = {"vc_dbscan_levels_core_kernel": 0, "vc_dbscan_levels_edge_kernel": 256, "vc_dbscan_levels_cascade_kernel": 0,
             "vc_dbscan_levels_finish_kernel": 1024}
FIELDS = ["n_pairs", "n_clusters", "n_core", "n_border", "n_noise"]


def test_header_declares_and_library_exports_the_new_names(vc):
    txt = open(os.path.join(ROOT, "include", "verticut_gpu.h")).read()
    assert re.search(r"#define\s+VC_ABI_VERSION\s+2\b", txt)             # entry points are only added
    assert "NO n_labelled form" in txt                                     # the header says why there is none
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"#define\s+VC_CORE_NEVER\s+0xFFFFFFFFu", code)
    assert re.search(r"typedef struct vc_dbscan_levels_stats\s*\{\s*uint64_t n_pairs\[VC_LEVELS_MAX\];\s*uint64_t n_clusters\[VC_LEVELS_MAX\];\s*"
                     r"uint64_t n_core\[VC_LEVELS_MAX\], n_border\[VC_LEVELS_MAX\], n_noise\[VC_LEVELS_MAX\];\s*\}\s*vc_dbscan_levels_stats;", code)
    L = ctypes.CDLL(vc.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(L, name), name
        assert name in vc.EXPORTS
    assert vc.CORE_NEVER == DL.CORE_NEVER == 2 ** 32 - 1
    assert ctypes.sizeof(vc.VcDbscanLevelsStats) == 2560 == 5 * 8 * vc.LEVELS_MAX
    assert [f[0] for f in vc.VcDbscanLevelsStats._fields_] == FIELDS == list(DL.FIELDS)
    assert [getattr(vc.VcDbscanLevelsStats, f).offset for f in FIELDS] == [0, 512, 1024, 1536, 2048]
    for cls in (vc.Engine, vc.ShardedEngine):
        for meth in ("dbscan_levels", "dbscan_levels_dev"):
            assert callable(getattr(cls, meth))
    host = open(os.path.join(ROOT, "verticut_amd", "host", "verticut_host.hpp")).read()
    assert re.search(r"virtual int dbscan_levels\([^)]*\)\s*=\s*0;", host)
    assert len(re.findall(r"int dbscan_levels\([^)]*\)\s*override", host)) == 2
    assert "return vc_dbscan_levels(h_," in host and "return vc_sharded_dbscan_levels(h_," in host


def test_kernels_use_no_scratch_and_only_the_counters_in_lds(vc):
    """vc_dbscan_levels.o holds exactly the core, edge, cascade and finish kernels: no scratch, no spills; LDS is the edge kernel's 64
    pair counters and the finish kernel's 4 x 64 kind counters.  The forest primitives are vc_forest.hpp's, included and not copied."""
    from verticut_amd import build as vb
    assert "vc_dbscan_levels.hip" in vb.SOURCES and "vc_forest.hpp" in vb.HEADERS
    res = vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_dbscan_levels.o"))
    assert len(res) == 4, sorted(res)
    for kernel in KERNELS:                                                          # (mangled names)
        assert sum(kernel in name for name in res) == 1, (kernel, sorted(res))
    for name, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == [b for k, b in LDS_BYTES.items() if k in name][0], (name, r)
    csrc = os.path.join(ROOT, "verticut_amd", "csrc")
    text = open(os.path.join(csrc, "vc_dbscan_levels.hip")).read()
    assert '#include "vc_forest.hpp"' in text and "cl_unite(labels + (uint64_t)w * n," in text and "asm" not in text
    defined = [os.path.basename(f) for f in sorted(glob.glob(os.path.join(csrc, "*"))) if "void cl_unite(" in open(f).read()]
    assert defined == ["vc_forest.hpp"]


# shape, max_radius, the min_pts values
CASES = [("S64", None, DC.MIN_PTS), ("S512", None, DC.MIN_PTS), ("EVEN", 7, DC.MIN_PTS), ("P64", 4, (4, 5))]


@pytest.mark.parametrize("name,R,all_min_pts", CASES)
def test_the_scheme_is_the_per_radius_dbscan(name, R, all_min_pts):
    """labels at every level; cd <= r iff the degree at radius r reaches min_pts; the kinds sum to N; min_pts 1 is single linkage"""
    n = DL.shape(name)["n"]
    R = DL.max_radius(name) if R is None else R
    pairs, dist = DL.pairs_dist(name, R)
    for min_pts in all_min_pts:
        want, degrees, stats = DL.per_level(n, pairs, dist, R, min_pts)
        assert np.array_equal(DL.scheme(n, pairs, dist, R, min_pts), want), min_pts
        cd = DL.core_dist(n, pairs, dist, min_pts)
        for r in range(R + 1):
            assert np.array_equal(cd <= r, degrees[r] >= min_pts), (min_pts, r)
        assert np.all((cd <= R) | (cd == DL.CORE_NEVER))
        assert np.all(stats["n_core"] + stats["n_border"] + stats["n_noise"] == n)
        assert np.array_equal(stats["n_pairs"], LC.histogram(name, R) if name != "P64" else np.bincount(dist, minlength=R + 1))
        if min_pts == 1:
            assert not cd.any() and np.array_equal(want, LC.labels_of(name, R))
        got = DL.relative(name, min_pts, R)                                           # what the GPU tests compare with
        assert np.array_equal(got[0], want) and np.array_equal(got[1], cd)


def _wrong_levels(name, R, min_pts):
    """the number of levels at which the scheme without (the cascade, w, the prefix minimum) differs from the expectation"""
    n = DL.shape(name)["n"]
    pairs, dist = DL.pairs_dist(name, R)
    want = DL.relative(name, min_pts, R)[0]
    return tuple(sum(not np.array_equal(row, want[r]) for r, row in enumerate(DL.scheme(n, pairs, dist, R, min_pts, **{part: False})))
                 for part in ("cascade", "unite_at_w", "prefix_min"))


# (shape, max_radius, min_pts): levels wrong without the cascade, with pairs united at d instead of w, without the prefix minimum
WRONG = {
    ("EVEN", 7, 64): (3, 4, 3),
    ("EVEN", 7, 3): (5, 0, 1),
    ("S64", 8, 64): (4, 2, 0),
    ("P64", 4, 4): (2, 4, 0),
    ("P64", 4, 5): (1, 3, 0),
}


@pytest.mark.parametrize("case", sorted(WRONG))
def test_the_data_needs_every_part(case):
    """every part of the scheme is caught by some shape of the GPU tests: each column below has a non-zero entry"""
    assert _wrong_levels(*case) == WRONG[case]
    assert all(any(w[part] for w in WRONG.values()) for part in range(3))


S64_MOVING_BORDERS = 197


def _anchors(n, pairs, dist, R, min_pts):
    """[R + 1, n]: the smallest core neighbour of every non-core record at every level, n for none; one level at a time"""
    out = np.full((R + 1, n), n, dtype=np.int64)
    for r in range(R + 1):
        within = pairs[dist <= r]
        a, b = CC.split(within)
        core = DC.degrees_of(n, within) >= min_pts
        up, down = core[a] & ~core[b], ~core[a] & core[b]
        np.minimum.at(out[r], b[up], a[up])
        np.minimum.at(out[r], a[down], b[down])
    return out


def test_what_the_shapes_hold():
    """S64 at min_pts 64: borders whose anchor moves from one level to the next.  EVEN at min_pts 64: records that never become a
    core, and levels that only the cascade and the prefix minimum write.  P64 at min_pts 4, level 2: the contested borders, where
    "smallest label" would differ from "smallest core neighbour"."""
    n, R = DL.shape("S64")["n"], DL.max_radius("S64")
    pairs, dist = DL.pairs_dist("S64")
    anchor = _anchors(n, pairs, dist, R, 64)
    both = (anchor[1:] < n) & (anchor[:-1] < n)
    assert int(np.count_nonzero(np.any(both & (anchor[1:] != anchor[:-1]), axis=0))) == S64_MOVING_BORDERS
    lab, cd, stats = DL.relative("EVEN", 64, 7)
    assert int(np.count_nonzero(cd == DL.CORE_NEVER)) == 27 and set(cd.tolist()) == {2, 4, 6, DL.CORE_NEVER}
    assert stats["n_core"].tolist() == [0, 0, 35, 35, 153, 153, 273, 273] and stats["n_border"].tolist() == [0, 0, 41, 41, 147, 147, 27, 27]
    assert stats["n_clusters"].tolist() == [0, 0, 1, 1, 3, 3, 3, 3]
    for r in (1, 3, 5, 7):                                                            # no pair, no core distance of an odd level
        assert stats["n_pairs"][r] == 0 and np.array_equal(lab[r], lab[r - 1])
    p, d = DL.pairs_dist("P64", 4)
    within = p[d <= DC.PLANT_R]
    rule, other = DC.dbscan(450, within, DC.PLANT_MIN_PTS)[0], DC.dbscan(450, within, DC.PLANT_MIN_PTS, by_label=True)[0]
    assert np.array_equal(DL.relative("P64", DC.PLANT_MIN_PTS, 4)[0][DC.PLANT_R], rule)
    assert np.flatnonzero(rule != other).tolist() == [DC.BRIDGES["rules_disagree"]["x"][0]]
    stats = DL.relative("P64", 4, 4)[2]
    assert stats["n_border"].tolist() == [0, 30, 4, 0, 0] and stats["n_clusters"].tolist() == [0, 10, 9, 5, 5]



def _pairs(*edges):
    p = np.array([(min(a, b) << 32) | max(a, b) for a, b, _ in edges], dtype=np.uint64)
    order = np.argsort(p)
    return p[order], np.array([d for _, _, d in edges], dtype=np.int64)[order]


def test_hand_made_graph():
    """min_pts 4, nine records.  4, 5, 6, 7 lie pairwise at distance 1: cores from level 1 on.  3 has 4 at distance 1 and 5, 6 at
    distance 2: a border of 4 at level 1, a core only at level 2 -- and its edge to 4, of distance 1, joins two cores only then
    (w = 2), which renames the cluster from 4 to 3.  8 has 5 at distance 1 and 1 at distance 3, and never becomes a core: its
    anchor is 5 at levels 1 and 2 (at level 2 only through the prefix minimum: it has no candidate of exactly that level) and 1 at
    level 3, when 1 becomes a core through 0, 2 and 8, a cluster of its own.  0 and 2 are noise until then."""
    n, R, min_pts = 9, 3, 4
    never = DL.CORE_NEVER
    pairs, dist = _pairs((4, 5, 1), (4, 6, 1), (4, 7, 1), (5, 6, 1), (5, 7, 1), (6, 7, 1), (5, 8, 1), (3, 4, 1), (3, 5, 2), (3, 6, 2),
                         (0, 1, 3), (1, 2, 3), (1, 8, 3))
    want = np.array([[0, 1, 2, 3, 4, 5, 6, 7, 8],
                     [0, 1, 2, 4, 4, 4, 4, 4, 4],
                     [0, 1, 2, 3, 3, 3, 3, 3, 3],
                     [1, 1, 1, 3, 3, 3, 3, 3, 1]])
    labels, _, stats = DL.per_level(n, pairs, dist, R, min_pts)
    assert np.array_equal(labels, want)
    assert np.array_equal(DL.scheme(n, pairs, dist, R, min_pts), want)
    assert DL.core_dist(n, pairs, dist, min_pts).tolist() == [never, 3, never, 2, 1, 1, 1, 1, never]
    assert stats["n_pairs"].tolist() == [0, 8, 2, 3] and stats["n_clusters"].tolist() == [0, 1, 1, 2]
    assert stats["n_core"].tolist() == [0, 4, 5, 6] and stats["n_border"].tolist() == [0, 2, 1, 3] and stats["n_noise"].tolist() == [9, 3, 3, 0]
    for r in range(R + 1):                                                            # the second host method agrees
        assert np.array_equal(DC.dbscan_b(n, pairs[dist <= r], min_pts)[0], want[r]), r
    at_d = DL.scheme(n, pairs, dist, R, min_pts, unite_at_w=False)                  # 3-4 united at level 1: 3 names the cluster too early
    assert at_d[1].tolist() == [0, 1, 2, 3, 3, 3, 3, 3, 3]
    no_prefix = DL.scheme(n, pairs, dist, R, min_pts, prefix_min=False)             # 8 loses its anchor at level 2
    assert no_prefix[2].tolist() == [0, 1, 2, 3, 3, 3, 3, 3, 8] and np.array_equal(no_prefix[[0, 1, 3]], want[[0, 1, 3]])
    no_cascade = DL.scheme(n, pairs, dist, R, min_pts, cascade=False)               # level 3 forgets the cluster of level 2
    assert no_cascade[3].tolist() == [1, 1, 1, 3, 4, 5, 6, 7, 1]
