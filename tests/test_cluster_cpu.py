"""Near-duplicate clustering, without a GPU: the ABI surface, the code objects of the three kernels, and the expectation of
test_cluster_gpu.py -- that its two methods agree, that the data makes transitivity, the incremental merge and the keep rule
matter, and the rules themselves on a hand-made graph."""
import ctypes
import os
import re

import numpy as np
import pytest

import cluster_common as CC
import ids_common as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vc_cluster_radius", "vc_cluster_radius_dev", "vc_sharded_cluster_radius", "vc_sharded_cluster_radius_dev"]


def test_header_declares_and_library_exports_the_new_names(vc):
    txt = open(os.path.join(ROOT, "include", "verticut_gpu.h")).read()
    assert re.search(r"#define\s+VC_ABI_VERSION\s+2\b", txt)             # entry points are only added
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"typedef struct vc_cluster_stats\s*\{\s*uint64_t n_pairs;\s*uint64_t n_clusters;\s*\}\s*vc_cluster_stats;", code)
    L = ctypes.CDLL(vc.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(L, name), name
        assert name in vc.EXPORTS
    assert ctypes.sizeof(vc.VcClusterStats) == 16 and vc.VcClusterStats.n_clusters.offset == 8
    for cls in (vc.Engine, vc.ShardedEngine):
        for meth in ("cluster_radius", "cluster_radius_dev"):
            assert callable(getattr(cls, meth))
    host = open(os.path.join(ROOT, "verticut_amd", "host", "verticut_host.hpp")).read()
    assert re.search(r"virtual int cluster_radius\([^)]*\)\s*=\s*0;", host)
    assert len(re.findall(r"int cluster_radius\([^)]*\)\s*override", host)) == 2
    assert "return vc_cluster_radius(h_," in host and "return vc_sharded_cluster_radius(h_," in host


def test_cluster_kernels_use_no_lds_and_no_scratch(vc):
    """vc_cluster.o holds exactly the three vc_cluster_* kernels: no scratch, no spills, no LDS (there is no plan and no chunk
    table: a thread finds its query by binary search)"""
    from verticut_amd import build as vb
    assert "vc_cluster.hip" in vb.SOURCES and "vc_walk.hip" in vb.SOURCES
    res = vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_cluster.o"))
    assert len(res) == 3, sorted(res)
    for kernel in ("vc_cluster_init_kernel", "vc_cluster_union_kernel", "vc_cluster_flatten_kernel"):      # (mangled names)
        assert sum(kernel in name for name in res) == 1, (kernel, sorted(res))
    for name, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == 0, (name, r)


@pytest.mark.parametrize("name", I.SINGLE)
def test_the_two_expectation_methods_agree(name):
    n = I.SHAPES[name]["n"]
    for radius in CC.RADII[name]:
        pairs = CC.pairs_of(name, radius)
        lab = CC.labels_of(name, radius)
        assert np.array_equal(lab, CC.propagate(n, pairs)), radius
        assert np.all(lab <= np.arange(n)) and np.array_equal(lab[lab], lab)        # the smallest id, itself labelled with itself
        a, b = CC.split(pairs)
        assert np.array_equal(lab[a], lab[b])                                       # adjacent records share a label
        assert CC.n_pairs(name, radius) == len(pairs) and CC.n_pairs(name, radius, n) == 0


# (clusters, singletons, largest cluster, members not adjacent to their own label)
FIGURES = {
    ("S128", 3): (2027, 2022, 1482, 1825), ("S128", 6): (180, 177, 2459, 3608),
    ("S256", 3): (722, 719, 281, 268), ("S256", 6): (175, 172, 469, 325),
    ("S512", 3): (769, 766, 261, 295), ("S512", 6): (246, 243, 446, 598),
}
# components of the old part alone, minus the labels the old records carry in the full clustering
MERGED_BY_NEW = {("S128", 3): 42, ("S128", 6): 71, ("S256", 3): 24, ("S256", 6): 27, ("S512", 3): 15, ("S512", 6): 17}


@pytest.mark.parametrize("name", ["S128", "S256", "S512"])
def test_the_data_needs_transitivity(name):
    """members that are NOT within the radius of their own label: a neighbour list of the label would miss them"""
    for radius in (3, 6):
        assert CC.figures(name, radius) == FIGURES[name, radius], radius


def test_extreme_radii():
    assert len(CC.pairs_of("S128", 16)) == 6249100                                 # what a caller copies home today
    assert CC.figures("S128", 16)[:2] == (2, 0)
    for radius in CC.RADII["S64"][1:]:
        assert CC.figures("S64", radius)[:2] == (4, 0)
    # R = 0: the components are exactly the groups of identical codes
    for name in I.SINGLE:
        codes = I.codes_of(name)
        _, first, inverse = np.unique(codes, axis=0, return_index=True, return_inverse=True)
        assert np.array_equal(CC.labels_of(name, 0), first[inverse.reshape(-1)]), name
    lab = CC.labels_of("S128", 0)
    assert CC.n_clusters(lab) == 4039
    assert set(lab[list(I.GROUP7)]) == {37} and set(lab[list(I.GROUP40)]) == {100}
    # sharded: GROUP7 spans H3's shard boundary 1999 | 2000
    assert I.shard_bounds("H3")[0] == (0, 2000) and 1999 in I.GROUP7 and 2000 in I.GROUP7
    base = I.SHAPES["H3"]["id_base"]
    assert np.array_equal(CC.expect("H3", 6), (CC.labels_of("S128", 6) + base).astype(np.uint32)) and CC.expect("H3", 6).max() >= 2 ** 31
    assert CC.expect("S512", 3).min() >= 2 ** 31                                    # labels with the top bit


@pytest.mark.parametrize("name", ["S128", "S256", "S512"])
def test_new_records_merge_old_components(name):
    """an incremental call that only appended labels for the new records would be caught: new records bridge old components"""
    n, k = I.SHAPES[name]["n"], CC.n_old(name)
    assert 0 < k < n
    for radius in (3, 6):
        pairs, full = CC.pairs_of(name, radius), CC.labels_of(name, radius)
        old = CC.old_labels(name, radius)
        assert CC.n_clusters(old) - CC.n_clusters(full[:k]) == MERGED_BY_NEW[name, radius]
        assert not np.array_equal(old, full[:k])
        # the keep rule's pairs on top of the old forest give the full clustering
        a, b = CC.split(pairs)
        assert np.array_equal(CC.union_find(n, pairs[b >= k], init=old), full)
        assert CC.n_pairs(name, radius, k) == int((b >= k).sum()) and 0 < CC.n_pairs(name, radius, k) < len(pairs)


def _pairs(*edges):
    return np.sort(np.array([(min(a, b) << 32) | max(a, b) for a, b in edges], dtype=np.uint64))


def test_hand_made_graph():
    """a path 5-3-9-1; {0, 2} and {4, 6} bridged by the later record 10; 7 isolated; 8, 11, 12 identical codes (a triangle)"""
    n = 13
    pairs = _pairs((5, 3), (3, 9), (9, 1), (0, 2), (4, 6), (2, 10), (10, 4), (8, 11), (8, 12), (11, 12))
    want = np.array([0, 1, 0, 1, 0, 1, 0, 7, 8, 1, 0, 8, 8])
    assert np.array_equal(CC.union_find(n, pairs), want) and np.array_equal(CC.propagate(n, pairs), want)
    assert CC.n_clusters(want) == 4
    rng = np.random.default_rng(5)
    for _ in range(8):                                                             # any order of the pairs
        assert np.array_equal(CC.union_find(n, rng.permutation(pairs)), want)
    a, b = CC.split(pairs)
    for k in range(n + 1):                                                         # n_labelled anywhere, the middle included
        kept = CC.kept_entries(n, pairs, k)
        assert len(np.unique(kept)) == len(kept)                                    # every pair once
        assert np.array_equal(np.sort(kept), pairs[b >= k])                         # all those with a new member, none among old
        old = CC.union_find(k, pairs[b < k])
        assert np.array_equal(CC.union_find(n, kept, init=old), want), k
    # n_labelled = 10: the old part knows {0, 2} and {4, 6} as two components, record 10 merges them
    old = CC.union_find(10, pairs[b < 10])
    assert old[2] == 0 and old[6] == 4 and old[9] == 1
    assert len(CC.kept_entries(n, pairs, 10)) == 5 and len(CC.kept_entries(n, pairs, n)) == 0
