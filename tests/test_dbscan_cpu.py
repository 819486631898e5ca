"""Density clustering, without a GPU: the ABI surface, the code objects of the kernels, and the expectation of test_dbscan_gpu.py --
that its two methods agree, that the shapes show all three kinds, that min_pts 1 and 2 are single linkage, and that the planted
shape tells the anchor rule from every other."""
import ctypes
import os
import re

import numpy as np
import pytest

import cluster_common as CC
import dbscan_common as DC
import ids_common as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vc_dbscan_radius", "vc_dbscan_radius_dev", "vc_sharded_dbscan_radius", "vc_sharded_dbscan_radius_dev"]


def test_header_declares_and_library_exports_the_new_names(vc):
    txt = open(os.path.join(ROOT, "include", "verticut_gpu.h")).read()
    assert re.search(r"#define\s+VC_ABI_VERSION\s+2\b", txt)             # entry points are only added
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"typedef struct vc_dbscan_stats\s*\{\s*uint64_t n_pairs;\s*uint64_t n_clusters;\s*uint64_t n_core, n_border, n_noise;\s*\}\s*vc_dbscan_stats;", code)
    L = ctypes.CDLL(vc.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(L, name), name
        assert name in vc.EXPORTS
    assert ctypes.sizeof(vc.VcDbscanStats) == 40
    assert [f[0] for f in vc.VcDbscanStats._fields_] == ["n_pairs", "n_clusters", "n_core", "n_border", "n_noise"]
    for cls in (vc.Engine, vc.ShardedEngine):
        for meth in ("dbscan_radius", "dbscan_radius_dev"):
            assert callable(getattr(cls, meth))
    host = open(os.path.join(ROOT, "verticut_amd", "host", "verticut_host.hpp")).read()
    assert re.search(r"virtual int dbscan_radius\([^)]*\)\s*=\s*0;", host)
    assert len(re.findall(r"int dbscan_radius\([^)]*\)\s*override", host)) == 2
    assert "return vc_dbscan_radius(h_," in host and "return vc_sharded_dbscan_radius(h_," in host


def test_dbscan_kernels_use_no_scratch_and_no_lds(vc):
    """vc_dbscan.o holds exactly the degree, edge and finish kernels: no scratch, no spills, no LDS; the forest primitives are
    vc_forest.hpp's, one copy shared with vc_cluster.hip"""
    from verticut_amd import build as vb
    assert "vc_dbscan.hip" in vb.SOURCES and "vc_forest.hpp" in vb.HEADERS
    res = vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_dbscan.o"))
    assert len(res) == 3, sorted(res)
    for kernel in ("vc_dbscan_degree_kernel", "vc_dbscan_edge_kernel", "vc_dbscan_finish_kernel"):      # (mangled names)
        assert sum(kernel in name for name in res) == 1, (kernel, sorted(res))
    for name, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == 0, (name, r)
    csrc = os.path.join(ROOT, "verticut_amd", "csrc")
    for src in ("vc_cluster.hip", "vc_dbscan.hip"):
        text = open(os.path.join(csrc, src)).read()
        assert '#include "vc_forest.hpp"' in text and "uint32_t cl_find_halving(" not in text, src
    assert open(os.path.join(csrc, "vc_forest.hpp")).read().count("uint32_t cl_find_halving(") == 1


# ---- the expectation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", I.SINGLE + ("P64",))
def test_the_two_expectation_methods_agree(name):
    n = DC.shape(name)["n"]
    own = np.arange(n)
    for radius in DC.RADII + ((DC.PLANT_R,) if name == "P64" else ()):
        pairs = DC.pairs_of(name, radius)
        for min_pts in DC.MIN_PTS + ((DC.PLANT_MIN_PTS,) if name == "P64" else ()):
            lab, deg, stats = DC.relative(name, radius, min_pts)
            lab_b, deg_b = DC.dbscan_b(n, pairs, min_pts)
            assert np.array_equal(lab, lab_b) and np.array_equal(deg, deg_b), (radius, min_pts)
            core, border, noise = DC.kinds(lab, deg, min_pts)
            assert stats["n_core"] + stats["n_border"] + stats["n_noise"] == n and stats["n_pairs"] == len(pairs)
            assert np.all(core[lab[~noise]]) and np.array_equal(lab[lab], lab)         # a label of a cluster names a core labelled with itself
            assert np.all(lab[core] <= own[core])                                      # ... the smallest core of the component
            assert stats["n_clusters"] == int(np.count_nonzero(core & (lab == own)))
            assert deg.sum() == n + 2 * len(pairs) and (min_pts > 1 or not border.any())


def test_the_existing_shapes_show_all_three_kinds():
    """the figures the GPU suite's parameter sets give; three kinds at once on every shape at R = 3 and 6"""
    def figures(name, radius, min_pts):
        s = DC.relative(name, radius, min_pts)[2]
        return s["n_core"], s["n_border"], s["n_noise"]
    assert figures("S128", 3, 8) == (2703, 264, 2033)
    assert figures("S512", 6, 64) == (1003, 254, 243)
    assert figures("S64", 0, 8) == (617, 0, 2383) and DC.relative("S64", 0, 8)[2]["n_clusters"] == 6
    assert figures("S256", 0, 64) == (0, 0, 1500) and figures("S512", 0, 64) == (0, 0, 1500)      # all noise
    for name in ("S128", "S256", "S512"):
        for radius in (3, 6):
            for min_pts in (3, 8, 64):
                assert min(figures(name, radius, min_pts)) > 0, (name, radius, min_pts)
    for name in I.SINGLE:
        for min_pts in DC.MIN_PTS:
            assert figures(name, 0, min_pts)[1] == 0                                    # exact duplicates: no borders
            twice = 2 * I.SHAPES[name]["flips"]
            if min_pts < 64:
                lab, deg = DC.dbscan(I.SHAPES[name]["n"], CC.pairs_of(name, twice), min_pts)
                assert np.all(deg >= min_pts)                                           # R = 2 x flips: everything is a core


@pytest.mark.parametrize("name", I.SINGLE)
def test_no_border_of_the_existing_shapes_is_contested(name):
    """every border's core neighbours lie in one cluster: these shapes cannot tell the anchor rule from any other, the planted one must"""
    n = I.SHAPES[name]["n"]
    for radius in DC.RADII:
        pairs = DC.pairs_of(name, radius)
        for min_pts in DC.MIN_PTS:
            assert np.array_equal(DC.dbscan(n, pairs, min_pts, by_label=True)[0], DC.relative(name, radius, min_pts)[0])


@pytest.mark.parametrize("name", I.SINGLE + ("P64",))
def test_min_pts_1_and_2_are_single_linkage(name):
    n = DC.shape(name)["n"]
    own = np.arange(n)
    for radius in DC.RADII:
        pairs = DC.pairs_of(name, radius)
        single = CC.labels_of(name, radius) if name in I.SHAPES else CC.union_find(n, pairs)
        lab1, deg1 = DC.dbscan(n, pairs, 1)
        assert np.array_equal(lab1, single) and not DC.kinds(lab1, deg1, 1)[2].any()
        lab2, deg2 = DC.dbscan(n, pairs, 2)
        core, border, noise = DC.kinds(lab2, deg2, 2)
        assert np.array_equal(lab2, single) and not border.any()
        assert np.array_equal(noise, deg2 == 1) and np.all(single[noise] == own[noise])           # the isolated records are the noise
    lab, deg = DC.dbscan(n, DC.pairs_of(name, 3), n + 1)
    assert np.array_equal(lab, own) and DC.stats_of(lab, deg, n + 1, DC.pairs_of(name, 3))["n_clusters"] == 0


# ---- the planted shape ----------------------------------------------------------------------------------------------------------------
def test_planted_shape():
    s = DC.PLANTED["P64"]
    n, R, M = s["n"], DC.PLANT_R, DC.PLANT_MIN_PTS
    codes = DC.planted_codes()
    assert codes.shape == (n, 8) and np.array_equal(DC.codes_of("PH3"), codes)
    pairs = DC.pairs_of("P64", R)
    a, b = CC.split(pairs)
    planted = sorted(p for br in DC.BRIDGES.values() for p in br["a"] + br["b"] + br["x"])
    assert len(planted) == len(set(planted)) == 8 * 5 + 6
    filler = np.setdiff1d(np.arange(n), planted)
    assert not np.isin(a, filler).any() and not np.isin(b, filler).any()               # no filler record has a neighbour at the planted radius
    owner = {p: k for k, br in DC.BRIDGES.items() for p in br["a"] + br["b"] + br["x"]}
    assert all(owner[x] == owner[y] for x, y in zip(a.tolist(), b.tolist()))           # the bridges do not touch each other
    lab, deg = DC.dbscan(n, pairs, M)
    by_label = DC.dbscan(n, pairs, M, by_label=True)[0]
    assert np.array_equal(DC.dbscan_b(n, pairs, M)[0], lab)
    core, border, noise = DC.kinds(lab, deg, M)
    adjacent = set(pairs.tolist())

    def near(x, y):
        return ((min(x, y) << 32) | max(x, y)) in adjacent

    differ = 0
    for k in DC.CONTESTED:
        br = DC.BRIDGES[k]
        (x,), a0, b0 = br["x"], br["a"][0], br["b"][0]
        assert core[list(br["a"] + br["b"])].all() and deg[x] == 3 and border[x], k
        assert [v for v in planted if v != x and near(x, v)] == sorted((a0, b0)), k    # X touches a0 and b0 only
        assert not any(near(p, q) for p in br["a"] for q in br["b"]), k                # A and B are apart
        la, lb = lab[a0], lab[b0]
        assert la == min(br["a"]) and lb == min(br["b"]) and la != lb, k               # two clusters: the border is CONTESTED
        assert lab[x] == lab[min(a0, b0)] and by_label[x] == min(la, lb), k
        differ += lab[x] != by_label[x]
    assert differ >= 1 and lab[DC.BRIDGES["rules_disagree"]["x"][0]] == 61 and by_label[DC.BRIDGES["rules_disagree"]["x"][0]] == 60
    # X relative to its anchors in id order: below both, between, above both -- both directions of "seen from the larger member"
    pos = {k: (DC.BRIDGES[k]["x"][0], DC.BRIDGES[k]["a"][0], DC.BRIDGES[k]["b"][0]) for k in DC.CONTESTED}
    assert pos["x_below"][0] < min(pos["x_below"][1:]) and pos["x_above"][0] > max(pos["x_above"][1:])
    assert pos["x_between"][1] < pos["x_between"][0] < pos["x_between"][2]
    # the duplicate of X: degree 4 each, both cores, A and B welded into one cluster of ten
    br = DC.BRIDGES["x_twice"]
    members = list(br["a"] + br["b"] + br["x"])
    assert np.all(deg[list(br["x"])] == 4) and core[members].all() and np.all(lab[members] == min(members))
    assert DC.stats_of(lab, deg, M, pairs) == dict(n_pairs=73, n_clusters=9, n_core=42, n_border=4, n_noise=404)
    # batches of 1, 7 and 257 ids: X and its two anchors fall into one batch and into different ones
    together = {bs: [k for k, p in pos.items() if len({DC.batch_of(v, bs) for v in p}) == 1] for bs in DC.PLANT_BATCHES}
    assert together[1] == [] and together[7] == ["x_below"] and sorted(together[257]) == ["x_above", "x_below"]
    # PH3: shards of 200 ids; x_above's border is the first record of shard 1 and its anchors lie in shard 0
    cap, g = DC.PLANTED["PH3"]["capacity"], DC.PLANTED["PH3"]["shards"]
    assert cap // g == 200 and pos["x_above"][0] // 200 == 1 and pos["x_above"][1] // 200 == pos["x_above"][2] // 200 == 0
