"""Clusters at every radius in one walk, without a GPU: the ABI surface, the code objects of the three kernels, and the expectation
of test_levels_gpu.py -- that its pairs are cluster_common's, that the device's scheme (a pair in the forest of its distance only,
then the cascade) gives the per-radius union-find at every level, from scratch and from old labels, and that the data cannot pass
without the cascade."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

import cluster_common as CC
import ids_common as I
import levels_common as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vc_cluster_levels", "vc_cluster_levels_dev", "vc_sharded_cluster_levels", "vc_sharded_cluster_levels_dev"]
KERNELS = ("vc_levels_union_kernel", "vc_levels_cascade_kernel", "vc_levels_flatten_kernel")
HIST_LDS_BYTES = 256      # the union kernel's histogram: 64 counters of 32 bits; no other LDS in the object


def test_header_declares_and_library_exports_the_new_names(vc):
    txt = open(os.path.join(ROOT, "include", "verticut_gpu.h")).read()
    assert re.search(r"#define\s+VC_ABI_VERSION\s+2\b", txt)             # entry points are only added
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"#define\s+VC_LEVELS_MAX\s+64\b", code)
    assert re.search(r"typedef struct vc_levels_stats\s*\{\s*uint64_t n_pairs\[VC_LEVELS_MAX\];\s*uint64_t n_clusters\[VC_LEVELS_MAX\];\s*\}\s*vc_levels_stats;", code)
    L = ctypes.CDLL(vc.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(L, name), name
        assert name in vc.EXPORTS
    assert vc.LEVELS_MAX == LC.LEVELS_MAX == 64
    assert ctypes.sizeof(vc.VcLevelsStats) == 1024 and vc.VcLevelsStats.n_clusters.offset == 512
    assert [f[0] for f in vc.VcLevelsStats._fields_] == ["n_pairs", "n_clusters"]
    for cls in (vc.Engine, vc.ShardedEngine):
        for meth in ("cluster_levels", "cluster_levels_dev"):
            assert callable(getattr(cls, meth))
    host = open(os.path.join(ROOT, "verticut_amd", "host", "verticut_host.hpp")).read()
    assert re.search(r"virtual int cluster_levels\([^)]*\)\s*=\s*0;", host)
    assert len(re.findall(r"int cluster_levels\([^)]*\)\s*override", host)) == 2
    assert "return vc_cluster_levels(h_," in host and "return vc_sharded_cluster_levels(h_," in host


def test_levels_kernels_use_no_scratch_and_only_the_histogram_in_lds(vc):
    """vc_levels.o holds exactly the union, cascade and flatten kernels: no scratch, no spills; LDS is the union kernel's 64 pair
    counters and nothing else.  The forest primitives are vc_forest.hpp's, included and not copied."""
    from verticut_amd import build as vb
    assert "vc_levels.hip" in vb.SOURCES and "vc_forest.hpp" in vb.HEADERS
    res = vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_levels.o"))
    assert len(res) == 3, sorted(res)
    for kernel in KERNELS:                                                          # (mangled names)
        assert sum(kernel in name for name in res) == 1, (kernel, sorted(res))
    for name, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == (HIST_LDS_BYTES if "vc_levels_union_kernel" in name else 0), (name, r)
    csrc = os.path.join(ROOT, "verticut_amd", "csrc")
    text = open(os.path.join(csrc, "vc_levels.hip")).read()
    assert '#include "vc_forest.hpp"' in text and "cl_unite(labels + (uint64_t)d * n," in text
    defined = [os.path.basename(f) for f in sorted(glob.glob(os.path.join(csrc, "*"))) if "void cl_unite(" in open(f).read()]
    assert defined == ["vc_forest.hpp"]


@pytest.mark.parametrize("name", I.SINGLE)
def test_the_filtered_pairs_are_the_cluster_tests_pairs(name):
    """one O(n^2) loop at the largest radius, cut by distance, gives what radius_ids_common.brute_pairs gives radius by radius"""
    pairs, dist = LC.pairs_dist(name)
    assert LC.max_radius(name) == CC.RADII[name][-1] and dist.max() == LC.max_radius(name)
    assert np.all(pairs[1:] > pairs[:-1])
    for radius in CC.RADII[name]:
        assert np.array_equal(pairs[dist <= radius], CC.pairs_of(name, radius)), radius
        assert np.array_equal(LC.labels_of(name)[radius], CC.labels_of(name, radius)), radius
        assert int(LC.histogram(name)[:radius + 1].sum()) == CC.n_pairs(name, radius)
        k = CC.n_old(name)
        assert int(LC.histogram(name, n_labelled=k)[:radius + 1].sum()) == CC.n_pairs(name, radius, k)


@pytest.mark.parametrize("name", I.SINGLE + ("EVEN",))
def test_forest_d_only_plus_the_cascade_is_the_per_radius_union_find(name):
    """at every level, from scratch and -- with the keep rule's pairs on top of the old part's own levels -- incrementally"""
    n, R = LC.shape(name)["n"], LC.max_radius(name)
    pairs, dist = LC.pairs_dist(name)
    want = LC.labels_of(name)
    assert want.shape == (R + 1, n)
    assert np.array_equal(LC.scheme(n, pairs, dist, R), want)
    assert np.all(want[1:] <= want[:-1]) and np.all(want <= np.arange(n))            # nested; the smallest id of the component
    k = int(n * CC.OLD_SHARE)
    old = LC.old_labels(name, k)
    new = CC.split(pairs)[1] >= k
    assert 0 < np.count_nonzero(new) < len(pairs)
    assert np.array_equal(LC.scheme(n, pairs[new], dist[new], R, old=old), want)
    assert any(not np.array_equal(old[r], want[r, :k]) for r in range(R + 1))        # new records bridge old components


# pairs within R; clusters per level; levels at which the distance-d pairs ALONE do not give the level's partition
FIGURES = {
    "S64": (1123875, [1991, 1033, 361, 4, 4, 4, 4, 4, 4], 6),
    "S256": (374487, [1321, 1104, 918, 722, 543, 357, 175, 18] + [3] * 9, 14),
    "S512": (374649, [1329, 1141, 957, 769, 587, 440, 246, 74] + [3] * 9, 13),
}
S64_HISTOGRAM = [45867, 97921, 147266, 192350, 234527, 180542, 123238, 68656, 33508]


@pytest.mark.parametrize("name", sorted(FIGURES))
def test_the_data_needs_the_cascade(name):
    """a kernel that unites a pair in the forest of its distance and stops there is caught at most levels; no level is empty"""
    n, R = LC.shape(name)["n"], LC.max_radius(name)
    pairs, dist = LC.pairs_dist(name)
    want = LC.labels_of(name)
    alone = sum(not np.array_equal(CC.union_find(n, pairs[dist == r]), want[r]) for r in range(R + 1))
    assert (len(pairs), LC.cluster_counts(want).tolist(), alone) == FIGURES[name]
    assert np.all(LC.histogram(name) > 0)
    if name == "S64":
        assert LC.histogram(name).tolist() == S64_HISTOGRAM


def test_the_even_parity_store_has_empty_odd_levels():
    codes = LC.codes_of("EVEN")
    assert codes.shape == (300, 8) and not np.any(np.unpackbits(codes, axis=1).sum(axis=1) % 2)
    hist = LC.histogram("EVEN", 7)
    assert hist.tolist() == [1407, 0, 3092, 0, 5325, 0, 3482, 0]
    want = LC.labels_of("EVEN", 7)
    assert LC.cluster_counts(want).tolist() == [210, 210, 107, 107, 3, 3, 3, 3]
    for r in (1, 3, 5, 7):
        assert np.array_equal(want[r], want[r - 1])
    # up to the cap: every pair of the store lies within 63 bits, and the odd distances stay empty
    pairs, dist = LC.pairs_dist("EVEN", 63)
    assert len(pairs) == 300 * 299 // 2 and not np.any(dist % 2)
    assert LC.cluster_counts(LC.labels_of("EVEN", 63))[-1] == 1


def _pairs(*edges):
    p = np.array([(min(a, b) << 32) | max(a, b) for a, b, _ in edges], dtype=np.uint64)
    order = np.argsort(p)
    return p[order], np.array([d for _, _, d in edges], dtype=np.int64)[order]


def test_hand_made_graph():
    """a = 4, b = 1, c = 6: a-b at distance 1, b-c at distance 3, nothing between a and c within 3.  Level 3 joins {a, b, c} only
    through the cascade: forest 3 holds the pair b-c alone.  2-5 at distance 0; 0 and 3 isolated."""
    n, R = 7, 3
    pairs, dist = _pairs((4, 1, 1), (1, 6, 3), (2, 5, 0))
    want = np.array([[0, 1, 2, 3, 4, 2, 6],
                     [0, 1, 2, 3, 1, 2, 6],
                     [0, 1, 2, 3, 1, 2, 6],
                     [0, 1, 2, 3, 1, 2, 1]])
    assert np.array_equal(LC.levels_from(n, pairs, dist, R), want)
    assert np.array_equal(LC.scheme(n, pairs, dist, R), want)
    assert np.array_equal(CC.union_find(n, pairs[dist == 3]), [0, 1, 2, 3, 4, 5, 1])     # without the cascade: a is missing, 2-5 too
    assert LC.cluster_counts(want).tolist() == [6, 5, 5, 4]
    for k in range(n + 1):                                                             # n_labelled anywhere
        old = LC.levels_from(n, pairs, dist, R, n_first=k)
        new = CC.split(pairs)[1] >= k
        assert np.array_equal(LC.scheme(n, pairs[new], dist[new], R, old=old), want), k
