"""vc_knn_mst* and vc_mst_cut* without a GPU: the ABI surface, the code objects of the kernels, the plan arithmetic under the
sanitizers, and the expectation of test_knn_mst_gpu.py -- that the model's Kruskal, its synchronous Boruvka and a brute force over all
spanning forests agree on small stores, that a cut of the forest gives cluster_model's labels at every height, and the figures of the
inputs the GPU tests run on."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import knn_graph_common as KG
import knn_mst_common as KM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_new_names(vc):
    txt = open(os.path.join(ROOT, "include", "verticut_gpu.h")).read()
    assert re.search(r"#define\s+VC_ABI_VERSION\s+2\b", txt)             # entry points are only added
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"typedef struct vc_mst_edge\s*\{\s*uint32_t a;\s*uint32_t b;\s*uint32_t weight;\s*uint32_t dist;\s*\}\s*vc_mst_edge;", code)
    assert re.search(r"typedef struct vc_knn_mst_stats\s*\{\s*uint64_t n_edges;\s*uint64_t n_graph_edges;\s*uint64_t n_tree;\s*uint64_t n_clusters;"
                     r"\s*uint64_t total_weight;\s*uint32_t max_weight;\s*uint32_t n_rounds;\s*\}\s*vc_knn_mst_stats;", code)
    assert re.search(r"#define\s+VC_MST_DISTANCE\s+0u", code) and re.search(r"#define\s+VC_MST_REACHABILITY\s+1u", code)
    assert code.index("vc_knn_adjacency_stats;") < code.index("VC_MST_DISTANCE") < code.index("vc_device_status")   # after the vc_knn_adjacency* block
    L = ctypes.CDLL(vc.LIB_PATH)
    for name in KM.MST_NAMES:
        assert hasattr(L, name), name
        assert name in vc.EXPORTS
    for name in ("vc_knn_mst_dev", "vc_sharded_knn_mst_dev"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*const uint64_t\* d_rows,\s*const uint32_t\* d_counts,\s*uint32_t k,\s*uint32_t kk,"
                         r"\s*uint32_t flags,\s*uint32_t max_dist,\s*uint32_t weight_kind,\s*uint32_t min_pts,\s*vc_mst_edge\* d_edges,\s*uint32_t\* d_labels,"
                         r"\s*uint64_t\* d_hist,\s*vc_knn_mst_stats\* stats,\s*void\* stream\)" % name, code), name
    for name in ("vc_knn_mst", "vc_sharded_knn_mst"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*const uint64_t\* rows,\s*const uint32_t\* counts,\s*uint32_t k,\s*uint32_t kk,"
                         r"\s*uint32_t flags,\s*uint32_t max_dist,\s*uint32_t weight_kind,\s*uint32_t min_pts,\s*vc_mst_edge\* edges,\s*uint32_t\* labels,"
                         r"\s*uint64_t\* hist,\s*vc_knn_mst_stats\* stats\)" % name, code), name
    for name in ("vc_mst_cut_dev", "vc_sharded_mst_cut_dev"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*const vc_mst_edge\* d_edges,\s*uint64_t n_edges,\s*uint32_t max_weight,\s*uint32_t\* d_labels,"
                         r"\s*uint64_t\* n_clusters,\s*void\* stream\)" % name, code), name
    for name in ("vc_mst_cut", "vc_sharded_mst_cut"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*const vc_mst_edge\* edges,\s*uint64_t n_edges,\s*uint32_t max_weight,\s*uint32_t\* labels,"
                         r"\s*uint64_t\* n_clusters\)" % name, code), name
    flat = " ".join(txt.split()).replace(" * ", " ")
    for phrase in ("PRECONDITION AND \"LISTS\": exactly vc_cluster_knn*'s", "VC_KNN_REVERSE is refused", "a is the HOME end", "(weight, a, dist, b)",
                   "which is the order of the 64-bit key weight << 32 |", "The order is strict, so the MSF is unique", "words beyond M are untouched",
                   "min_pts = 1 under VC_MST_REACHABILITY gives VC_MST_DISTANCE's output bit for bit", "c_i = bits", "at most ceil(log2 N) + 1",
                   "it takes ANY edge list, sorted or not", "ERRORS, checked before any work", "THE OUTPUTS ARE THEN UNDEFINED", "N kk > 2^31 - 1",
                   "WAITS: one small read-back per round, plus one at the end", "no shard is touched", "NOT OFFERED: an incremental form",
                   "the condensed tree and stability selection"):
        assert " ".join(phrase.split()) in flat, phrase
    assert vc.VC_ABI_VERSION == 2 and (vc.MST_DISTANCE, vc.MST_REACHABILITY) == (KM.DISTANCE, KM.REACHABILITY)
    st = vc.VcKnnMstStats
    assert ctypes.sizeof(st) == 48 and [getattr(st, n).offset for n in KM.MST_STATS] == [0, 8, 16, 24, 32, 40, 44]
    assert st().as_dict() == KM.zero_stats()
    assert vc.MST_EDGE == KM.EDGE and vc.MST_EDGE.itemsize == 16
    for cls in (vc.Engine, vc.ShardedEngine):
        for meth in ("knn_mst", "knn_mst_dev", "mst_cut", "mst_cut_dev"):
            assert callable(getattr(cls, meth)), (cls, meth)
    host = open(os.path.join(ROOT, "verticut_amd", "host", "verticut_host.hpp")).read()
    assert re.search(r"virtual int knn_mst\([^)]*\)\s*=\s*0;", host) and re.search(r"virtual int mst_cut\([^)]*\)\s*=\s*0;", host)
    assert len(re.findall(r"int knn_mst\([^)]*\)\s*override", host)) == 2 and len(re.findall(r"int mst_cut\([^)]*\)\s*override", host)) == 2
    for call in ("return vc_knn_mst(h_,", "return vc_sharded_knn_mst(h_,", "return vc_mst_cut(h_,", "return vc_sharded_mst_cut(h_,"):
        assert call in host, call
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "5.21" in design and "vc_knn_mst" in design
    for doc in ("README.md", "INTEGRATION.md"):
        assert "vc_knn_mst" in open(os.path.join(ROOT, doc)).read(), doc
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_knn_mst.py"))


def test_mst_kernels_use_no_scratch_and_only_the_write_launch_has_lds(vc):
    from verticut_amd import build as vb
    assert "vc_knn_mst.hip" in vb.SOURCES and "vc_knn_mst_plan.hpp" in vb.HEADERS
    res = vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_knn_mst.o"))
    kernels = ("vc_mst_init_kernel", "vc_mst_enumerate_kernel", "vc_mst_min_kernel", "vc_mst_hook_kernel", "vc_mst_flatten_kernel", "vc_mst_write_kernel",
               "vc_mst_cut_kernel")
    for kernel in kernels:
        assert sum(kernel in name for name in res) == 1, (kernel, sorted(res))
    assert len(res) == len(kernels), sorted(res)
    for name, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == (513 * 4 if "vc_mst_write_kernel" in name else 0), (name, r)
    text = open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_knn_mst.hip")).read()
    for word in ("hipLaunchCooperativeKernel", "grid_group", "extern __shared__", "getenv", "asm"):
        assert word not in text, word
    assert '#include "vc_forest.hpp"' in text and text.count("cl_unite(") >= 2 and "void cl_unite" not in text   # vc_forest.hpp's union, not a copy


def test_plan_arithmetic_under_the_sanitizers(tmp_path):
    """tests/cpp/knn_mst_plan_test.cc over csrc/vc_knn_mst_plan.hpp, host code only, with AddressSanitizer and UBSan; the figures it
    prints are those of the model's mirror"""
    src = os.path.join(ROOT, "tests", "cpp", "knn_mst_plan_test.cc")
    exe = tmp_path / "knn_mst_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           src, "-I", os.path.join(ROOT, "verticut_amd", "csrc")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert out.stdout.startswith("knn mst plan ok: MAX_ITEMS %d STAT 48 EDGE 16\n" % KM.MAX_ITEMS)
    for n in (1, 2, 71, 513, 2000, 4096, 9000, 1000000):
        assert re.search(r"^ROUNDS %d %d$" % (n, KM.round_bound(n)), out.stdout, flags=re.M), n
    for flags in (KM.MUTUAL, KM.EITHER):
        line = "SCRATCH %d %d %d %d %d" % (flags, KM.live_bytes(9000, 5, flags), KM.forest_bytes(9000), KM.pick_bytes(9000), KM.stage_total(9000, 5, 64, True))
        assert re.search("^%s$" % line, out.stdout, flags=re.M), line
    assert re.search(r"^KEY %d$" % KM.key(512, 2 ** 31 - 2, 1, 0), out.stdout, flags=re.M)
    assert KM.items_ok(214748364, 10) and not KM.items_ok(214748365, 10)
    assert KM.min_pts_ok(KM.REACHABILITY, 10, 11) and not KM.min_pts_ok(KM.REACHABILITY, 10, 12) and not KM.min_pts_ok(KM.DISTANCE, 10, 2)


# ---- the model is the contract ----------------------------------------------------------------------------------------------------------------
def _tiny_stores():
    rng = np.random.default_rng(21)
    for n in (2, 3, 5, 6, 7):
        for bits, flips in ((64, 2), (64, 6)):
            base = rng.integers(0, 256, bits // 8, dtype=np.uint8)
            codes = np.array([KG._flip(base, rng.choice(bits, size=int(rng.integers(0, flips + 1)), replace=False)) for _ in range(n)], dtype=np.uint8)
            yield codes


def test_kruskal_boruvka_and_the_brute_force_agree_on_tiny_stores():
    seen = 0
    for codes in _tiny_stores():
        n = len(codes)
        for k, kk in ((3, 3), (3, 1), (6, 2)):
            k = min(k, 6)
            rows, counts = KG.loop_rows(codes, k, 100)
            for flags in (KM.MUTUAL, KM.EITHER):
                for kind, min_pts in ((KM.DISTANCE, 1), (KM.REACHABILITY, 2), (KM.REACHABILITY, 3)):
                    for max_dist in (KM.NO_CAP, 3):
                        edges, _ = KM.graph_edges(rows, counts, kk, flags, max_dist, 100, kind, min_pts)
                        assert len({(e[1], e[3]) for e in edges}) == len(edges) == len({frozenset((e[1], e[3])) for e in edges})   # every pair once
                        assert len({KM.key(e[0], e[1], kk, e[4]) for e in edges}) == len(edges)                                       # the order is strict
                        assert sorted(edges, key=lambda e: KM.key(e[0], e[1], kk, e[4])) == sorted(edges, key=lambda e: e[:4])      # the key IS the order
                        kept, _ = KM.kruskal(n, edges)
                        picked, rounds, live = KM.boruvka(n, edges)
                        assert picked == set(kept) and set(KM.brute_force(n, edges)) == set(kept), (n, k, kk, flags, kind, min_pts, max_dist)
                        assert rounds <= KM.round_bound(n) and (rounds >= 1) == bool(kept) and live[0] == len(edges)
                        seen += bool(kept)
    assert seen > 100


def test_a_cut_of_the_forest_is_cluster_knn_at_every_height():
    for codes, k, id_base in ((KG.clustered_case(64, n=300), 12, 50), (KG.hub_case()[0], KG.HUB_K, 0), (KM.uniform_case()[:200], 4, 7)):
        n, bits = len(codes), codes.shape[1] * 8
        rows, counts = KG.model_rows(codes, k, id_base)
        for kk in (1, 4, k):
            for flags in (KM.MUTUAL, KM.EITHER):
                for cap in (KM.NO_CAP, 2):
                    edges, labels, hist, st = KM.mst_model(rows, counts, kk, flags, cap, id_base, bits=bits)
                    whole, _, cl = KG.cluster_model(rows, counts, kk, flags, cap, id_base)
                    assert np.array_equal(labels, whole) and st["n_clusters"] == cl["n_clusters"] and st["n_edges"] == cl["n_edges"]
                    assert int(hist.sum()) == st["n_tree"] and st["total_weight"] == int((hist * np.arange(bits + 1, dtype=np.uint64)).sum())
                    for h in range(0, st["max_weight"] + 2):
                        want, _, cl = KG.cluster_model(rows, counts, kk, flags, min(cap, h), id_base)
                        got, count = KM.cut_model(n, edges, h, id_base)
                        assert np.array_equal(got, want) and count == cl["n_clusters"] == n - int(hist[:h + 1].sum()), (kk, flags, cap, h)
                    assert np.all(np.diff(edges["weight"].astype(np.int64)) >= 0)


def test_reachability_at_min_pts_1_is_the_distance_and_above_it_is_not():
    codes, rows, counts = KM.graph("small", 12)
    for flags in (KM.MUTUAL, KM.EITHER):
        plain = KM.mst_model(rows, counts, 10, flags)
        KM.same_mst(KM.mst_model(rows, counts, 10, flags, weight_kind=KM.REACHABILITY, min_pts=1), plain, flags, rounds=True)
        reach = KM.mst_model(rows, counts, 10, flags, weight_kind=KM.REACHABILITY, min_pts=6)
        assert reach[3]["total_weight"] > plain[3]["total_weight"] and np.array_equal(reach[1], plain[1])   # heavier, the same components
        assert np.all(reach[0]["weight"] >= reach[0]["dist"]) and np.any(reach[0]["weight"] > reach[0]["dist"])
    # a row shorter than min_pts - 1: the core distance is the code width
    hub = KG.hub_case()[0][:4]
    rows, counts = KG.model_rows(hub, 5)
    assert KM.core_distances(rows, counts, 5, 64) == [64] * 4 and KM.core_distances(rows, counts, 4, 64) == [int(r[2]) >> 32 for r in rows]
    edges = KM.mst_model(rows, counts, 3, KM.EITHER, weight_kind=KM.REACHABILITY, min_pts=5)[0]
    assert len(edges) == 3 and np.all(edges["weight"] == 64) and np.all(edges["dist"] < 64)


# ---- the pins: the figures of the inputs test_knn_mst_gpu.py runs on ----------------------------------------------------------------------------
def _st(name, k, kk, flags, **kw):
    return KM.model(name, k, kk, flags, **kw)[3]


def test_the_clustered_set():
    st = _st("clustered", 12, 10, KM.MUTUAL)
    assert (st["n_graph_edges"], st["n_tree"], st["n_rounds"]) == (990, 526, 3)
    edges = KM.model("clustered", 12, 10, KM.MUTUAL)[0]
    assert all(int((edges["weight"] == w).sum()) > 1 for w in np.unique(edges["weight"]))       # ties at every weight
    st = _st("clustered", 12, 10, KM.EITHER)
    assert (st["n_graph_edges"], st["n_tree"], st["n_clusters"], st["n_rounds"]) == (19010, 1995, 5, 4)
    assert _st("clustered", 12, 1, KM.MUTUAL)["n_tree"] == 169 and _st("clustered", 12, 1, KM.EITHER)["n_tree"] == 1831
    reach = KM.model("clustered", 12, 10, KM.EITHER, weight_kind=KM.REACHABILITY, min_pts=5)
    assert reach[3]["n_tree"] == 1995 and np.any(reach[0]["weight"] != reach[0]["dist"])
    capped = _st("clustered", 12, 10, KM.EITHER, max_dist=16)
    assert capped["n_tree"] == 1995


def test_the_uniform_set():
    st = _st("uniform", 4, 2, KM.EITHER)
    assert (st["n_tree"], st["n_clusters"], st["n_rounds"]) == (4095, 1, 6) and st["max_weight"] <= 21
    st = _st("uniform", 4, 4, KM.MUTUAL)
    assert (st["n_tree"], st["n_clusters"], st["n_rounds"]) == (3962, 134, 6)
    reach = KM.model("uniform", 4, 4, KM.MUTUAL, weight_kind=KM.REACHABILITY, min_pts=3)
    assert reach[3]["n_tree"] == 3962 and reach[3]["total_weight"] > st["total_weight"]


def test_the_thermometer_chain_hooks_in_one_round():
    codes, rows, counts = KM.graph("thermo", 2)
    assert codes.shape == (513, 64) and all(int(rows[i, 0]) >> 32 == 1 for i in range(513))
    for flags in (KM.MUTUAL, KM.EITHER):
        edges, labels, hist, st = KM.model("thermo", 2, 2, flags)
        assert (st["n_tree"], st["n_rounds"], st["max_weight"], st["total_weight"]) == (512, 1, 1, 512) and np.all(labels == 0)
        assert edges["a"].tolist() == list(range(512)) and edges["b"].tolist() == list(range(1, 513))   # the tie-break alone decides


def test_the_hub_set_the_pair_and_the_duplicates():
    st = _st("hub", 100, 100, KM.EITHER)
    assert (st["n_graph_edges"], st["n_tree"]) == (71 * 70 // 2, 70)                              # the complete graph
    assert _st("hub", 10, 10, KM.MUTUAL)["n_tree"] == 34
    for flags in (KM.MUTUAL, KM.EITHER):
        edges, _, hist, st = KM.model("pair", 3, 3, flags)
        assert len(edges) == 1 and tuple(edges[0]) == (0, 1, 512, 512) and int(hist[512]) == 1 and st["max_weight"] == 512   # the key's tenth weight bit
    st = _st("dup", KG.DUP_K, KG.DUP_K, KM.MUTUAL)
    assert (st["n_edges"], st["n_graph_edges"], st["n_tree"], st["n_clusters"], st["total_weight"], st["max_weight"], st["n_rounds"]) == (45000, 577, 338, 8662, 246, 2, 4)
    st = _st("dup", KG.DUP_K, KG.DUP_K, KM.EITHER)
    assert (st["n_edges"], st["n_graph_edges"], st["n_tree"], st["n_clusters"], st["total_weight"], st["max_weight"], st["n_rounds"]) == (45000, 44423, 8998, 2, 782, 2, 4)
    rows, counts = KM.graph("dup", KG.DUP_K)[1:]
    listers = np.bincount((rows[:, :KG.DUP_K].ravel() & np.uint64(0xFFFFFFFF)).astype(np.int64), minlength=KG.DUP_N)
    assert int(listers.max()) == 8525                                                            # one record with 8 525 listers: the contention case
