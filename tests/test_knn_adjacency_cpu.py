"""vc_knn_adjacency* without a GPU: the ABI surface, the code objects of the kernels and of the sort's new instantiation, the plan
arithmetic under the sanitizers, and the expectation of test_knn_adjacency_gpu.py -- that the numpy model agrees with plain set
loops, that its inputs reach the long segments, the empty ones and both distance passes, and that its totals and components are
those of knn_graph_common.cluster_model."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import knn_adjacency_common as KA
import knn_graph_common as KG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_new_names(vc):
    txt = open(os.path.join(ROOT, "include", "verticut_gpu.h")).read()
    assert re.search(r"#define\s+VC_ABI_VERSION\s+2\b", txt)             # entry points are only added
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"typedef struct vc_knn_adjacency_stats\s*\{\s*uint64_t n_edges;\s*uint64_t n_entries;\s*uint64_t n_empty;\s*uint32_t max_degree;"
                     r"\s*uint32_t pad;\s*\}\s*vc_knn_adjacency_stats;", code)
    assert re.search(r"#define\s+VC_KNN_REVERSE\s+2u", code) and re.search(r"#define\s+VC_KNN_MUTUAL\s+0u", code) and re.search(r"#define\s+VC_KNN_EITHER\s+1u", code)
    assert code.index("vc_cluster_snn_stats;") < code.index("VC_KNN_REVERSE") < code.index("vc_device_status")   # after the vc_cluster_snn* block
    L = ctypes.CDLL(vc.LIB_PATH)
    for name in KA.ADJ_NAMES:
        assert hasattr(L, name), name
        assert name in vc.EXPORTS
    for name in ("vc_knn_adjacency_dev", "vc_sharded_knn_adjacency_dev"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*const uint64_t\* d_rows,\s*const uint32_t\* d_counts,\s*uint32_t k,\s*uint32_t kk,"
                         r"\s*uint32_t flags,\s*uint32_t max_dist,\s*uint64_t\* d_adj,\s*uint64_t adj_cap,\s*uint64_t\* d_offsets,"
                         r"\s*vc_knn_adjacency_stats\* stats,\s*void\* stream\)" % name, code), name
    for name in ("vc_knn_adjacency", "vc_sharded_knn_adjacency"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*const uint64_t\* rows,\s*const uint32_t\* counts,\s*uint32_t k,\s*uint32_t kk,"
                         r"\s*uint32_t flags,\s*uint32_t max_dist,\s*uint64_t\* adj,\s*uint64_t adj_cap,\s*uint64_t\* offsets,"
                         r"\s*vc_knn_adjacency_stats\* stats\)" % name, code), name
    flat = " ".join(txt.split()).replace(" * ", " ")
    for phrase in ("PRECONDITION AND \"LISTS\": exactly vc_cluster_knn*'s", "OUTPUTS.", "CAPACITY, the protocol of the radius calls", "HOW.", "ERRORS, checked before any work",
                   "WAITS: one in the device form", "NOT OFFERED: segments ordered by neighbour id", "ASCENDING in the packed word",
                   "T = n_edges", "T = 2 n_mutual", "T = 2 (n_edges - n_mutual)", "d_offsets[N] = T", "is the sizing call",
                   "NO OUTPUT WORD IS WRITTEN BEFORE THAT WAIT", "N kk > 2^31 - 1", "24 N kk bytes", "NOT bounded by VC_KGRAPH_SCRATCH",
                   "a sort cannot be chunked", "N == 0 gives VC_OK, zero stats and d_offsets[0] = 0", "no shard is touched", "a per-segment degree cap",
                   "an incremental form after vc_add_codes / vc_retain*", "the call terminates and stays in bounds"):
        assert " ".join(phrase.split()) in flat, phrase
    assert vc.VC_ABI_VERSION == 2 and (vc.KNN_MUTUAL, vc.KNN_EITHER, vc.KNN_REVERSE) == (KA.MUTUAL, KA.EITHER, KA.REVERSE)
    st = vc.VcKnnAdjacencyStats
    assert ctypes.sizeof(st) == 32 and [getattr(st, n).offset for n in KA.ADJ_STATS] == [0, 8, 16, 24]
    assert st().as_dict() == KA.zero_stats()
    for cls in (vc.Engine, vc.ShardedEngine):
        for meth in ("knn_adjacency", "knn_adjacency_dev"):
            assert callable(getattr(cls, meth)), (cls, meth)
    host = open(os.path.join(ROOT, "verticut_amd", "host", "verticut_host.hpp")).read()
    assert re.search(r"virtual int knn_adjacency\([^)]*\)\s*=\s*0;", host)
    assert len(re.findall(r"int knn_adjacency\([^)]*\)\s*override", host)) == 2
    assert "return vc_knn_adjacency(h_," in host and "return vc_sharded_knn_adjacency(h_," in host
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "5.20" in design and "vc_knn_adjacency" in design and "VC_ADJ_TEAM_DEGREE" in design
    for doc in ("README.md", "INTEGRATION.md"):
        assert "vc_knn_adjacency" in open(os.path.join(ROOT, doc)).read(), doc
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_knn_adjacency.py"))


def _clean(name, r):
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)


def test_adjacency_kernels_use_no_scratch_and_the_sort_stays_in_static_lds(vc):
    """every kernel of vc_knn_adjacency.o has no scratch memory, no spills and no LDS; the sort's 64-bit-payload instantiation stages
    48 KiB instead of 32, still static, and the 32-bit one is what it was"""
    from verticut_amd import build as vb
    assert "vc_knn_adjacency.hip" in vb.SOURCES and "vc_knn_adjacency_plan.hpp" in vb.HEADERS
    res = vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_knn_adjacency.o"))
    kernels = ("vc_adj_enumerate_kernelILb0E", "vc_adj_enumerate_kernelILb1E", "vc_adj_mutual_kernelILb0E", "vc_adj_mutual_kernelILb1E",
               "vc_adj_degree_kernel", "vc_adj_offsets_kernel", "vc_adj_merge_kernel")
    for kernel in kernels:
        assert sum(kernel in name for name in res) == 1, (kernel, sorted(res))
    assert len(res) == len(kernels), sorted(res)
    for name, r in res.items():
        _clean(name, r)
        assert r["group_segment_fixed_size"] == 0, (name, r)
    plan = open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_knn_adjacency_plan.hpp")).read()
    assert re.search(r"#define\s+VC_ADJ_TEAM_DEGREE\s+%du" % KA.TEAM_DEGREE, plan) and re.search(r"#define\s+VC_ADJ_SORT_TILE\s+%du" % KA.RS_TILE, plan)
    fixed = (4 * 256 + 257 + 256 + 4) * 4
    lds64, lds32 = fixed + KA.RS_TILE * 12, fixed + KA.RS_TILE * 8                 # VC_ADJ_SORT_LDS_BYTES; the pairs' sort
    assert "// 48 KiB of staging: %d" % lds64 in plan
    sort = vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_sort.o"))
    scatter = {name: r for name, r in sort.items() if "rs_scatter_kernel" in name}
    hist = {name: r for name, r in sort.items() if "rs_hist_kernel" in name}
    assert len(scatter) == 3 and len(hist) == 3, sorted(sort)                      # <u32, key>, <u64, key>, <u64, value>
    for name, r in list(scatter.items()) + list(hist.items()):
        _clean(name, r)
    for name, r in scatter.items():
        want = lds32 if "IjLi0E" in name else lds64
        assert want <= r["group_segment_fixed_size"] <= want + 16 < 65536, (name, r, want)     # (alignment of the 8-byte array)
    assert sum(r["group_segment_fixed_size"] >= lds64 for r in scatter.values()) == 2
    for name, r in hist.items():
        assert r["group_segment_fixed_size"] == 1024, (name, r)
    text = open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_knn_adjacency.hip")).read()
    for word in ("hipLaunchCooperativeKernel", "grid_group", "extern __shared__", "__shared__", "getenv"):
        assert word not in text, word
    # one copy of the sort's kernels
    sort_text = open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_sort.hip")).read()
    assert sort_text.count("rs_scatter_kernel(") == 1 and sort_text.count("rs_hist_kernel(") == 1 and "template <class V, int SRC>" in sort_text


def test_plan_arithmetic_under_the_sanitizers(tmp_path):
    """tests/cpp/knn_adjacency_plan_test.cc over csrc/vc_knn_adjacency_plan.hpp, host code only, with AddressSanitizer and UBSan; the
    figures it prints are those of the model's mirror"""
    src = os.path.join(ROOT, "tests", "cpp", "knn_adjacency_plan_test.cc")
    exe = tmp_path / "knn_adjacency_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           src, "-I", os.path.join(ROOT, "verticut_amd", "csrc")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert out.stdout.startswith("knn adjacency plan ok: MAX_ITEMS %d TEAM_DEGREE %d STAT 32 LDS 55316\n" % (KA.MAX_ITEMS, KA.TEAM_DEGREE))
    for n in (1, 2, 71, 2000, 9000, 66000, 1000000):
        for bits in (64, 128, 256, 512):
            line = "PASSES %d %d %d %d %d" % (n, bits, KA.dist_passes(KA.NO_CAP, bits), KA.dist_passes(bits // 4, bits), KA.key_passes(n))
            assert re.search("^%s$" % line, out.stdout, flags=re.M), line
    assert (KA.dist_passes(KA.NO_CAP, 128), KA.dist_passes(KA.NO_CAP, 256), KA.key_passes(66000), KA.key_passes(65535)) == (1, 2, 3, 2)
    for flags in KA.FLAGS:
        line = "SCRATCH %d %d %d %d %d" % (flags, KA.bound(9000, 5, flags), KA.item_bytes(9000, 5, flags, 1), KA.counter_words(9000, flags),
                                          KA.stage_total(9000, 5, 5, flags, 50000, True))
        assert re.search("^%s$" % line, out.stdout, flags=re.M), line
    for kk in (1, 5, 10, 33, 100):
        assert re.search(r"^LANES %d %d$" % (kk, KA.row_lanes(kk)), out.stdout, flags=re.M), kk
    assert KA.items_ok(214748364, 10) and not KA.items_ok(214748365, 10)


# ---- the expectation ------------------------------------------------------------------------------------------------------------------
def _loops(rows, counts, kk, flags, max_dist, id_base):
    """the contract by plain Python loops: who lists whom, then every segment sorted as a list of (dist, id) tuples"""
    n = len(rows)
    lists = [[(int(v) >> 32, (int(v) & 0xFFFFFFFF) - id_base) for v in rows[i, :min(kk, int(counts[i]))]] for i in range(n)]
    S = [{j: d for d, j in lst if d <= max_dist} for lst in lists]
    offsets, adj = [0], []
    for j in range(n):
        seg = []
        for i in range(n):
            i_lists_j, j_lists_i = j in S[i], i in S[j]
            take = i_lists_j if flags == KA.REVERSE else (i_lists_j and j_lists_i) if flags == KA.MUTUAL else (i_lists_j or j_lists_i)
            if take:
                seg.append((S[i][j] if i_lists_j else S[j][i], i + id_base))
        adj += [(d << 32) | i for d, i in sorted(seg)]
        offsets.append(len(adj))
    deg = np.diff(offsets) if n else np.zeros(0, dtype=np.int64)
    st = dict(n_edges=sum(len(s) for s in S), n_entries=len(adj), n_empty=int((deg == 0).sum()), max_degree=int(deg.max()) if n else 0)
    return np.array(offsets, dtype=np.uint64), np.array(adj, dtype=np.uint64), st


def _pin(codes, k, kks, id_base, cap):
    rows, counts = KG.model_rows(codes, k, id_base)
    for kk in kks:
        for max_dist in (KA.NO_CAP, cap):
            models = KA.adjacency_models(rows, counts, kk, max_dist, id_base)
            _, _, cl = KG.cluster_model(rows, counts, kk, KG.MUTUAL, max_dist, id_base)
            for flags in KA.FLAGS:
                got = models[flags]
                KA.same_adjacency(got, _loops(rows, counts, kk, flags, max_dist, id_base), (kk, flags, max_dist))
                KA.same_adjacency(KA.adjacency_model(rows, None, kk, flags, max_dist, id_base), got, "counts NULL")
                for seg in KA.segments(got[0], got[1]):
                    assert np.all(seg[1:] > seg[:-1])                          # ascending, every neighbour once
                want_T = {KA.REVERSE: cl["n_edges"], KA.MUTUAL: 2 * cl["n_mutual"], KA.EITHER: 2 * (cl["n_edges"] - cl["n_mutual"])}[flags]
                assert got[2]["n_entries"] == want_T == int(got[0][-1]) and got[2]["n_edges"] == cl["n_edges"], (kk, flags, max_dist)


def test_the_model_is_the_contract_on_the_hub_set():
    codes, _ = KG.hub_case()
    _pin(codes, KG.HUB_K, (1, 3, KG.HUB_K), 1000, 1)
    _pin(codes, 100, (100,), 0, 2)                                             # rows shorter than kk: every row holds the whole store


def test_the_model_is_the_contract_on_a_small_clustered_set_and_on_the_complement_set():
    _pin(KG.clustered_case(64, n=150), 12, (1, 5, 12), 7, 64 // 4)
    _pin(KA.complement_case(256), 100, (100, 30), 2 ** 32 - 100, 255)


def test_the_totals_and_the_components_are_cluster_knns():
    """REVERSE degrees are the in-degrees; T = n_edges, 2 n_mutual, 2 (n_edges - n_mutual); a union-find over the MUTUAL / EITHER
    adjacency gives cluster_model's labels"""
    for codes, k, id_base in ((KG.clustered_case(64, n=400), 12, 50), (KG.hub_case()[0], KG.HUB_K, 0)):
        rows, counts = KG.model_rows(codes, k, id_base)
        for kk in (1, 4, k):
            for max_dist in (KA.NO_CAP, 2):
                models = KA.adjacency_models(rows, counts, kk, max_dist, id_base)
                for flags in (KG.MUTUAL, KG.EITHER):
                    labels, deg, cl = KG.cluster_model(rows, counts, kk, flags, max_dist, id_base)
                    assert np.array_equal(np.diff(models[KA.REVERSE][0].astype(np.int64)), deg)
                    assert models[KA.REVERSE][2]["n_entries"] == cl["n_edges"] and models[KA.REVERSE][2]["max_degree"] == cl["max_in_degree"]
                    assert models[KA.MUTUAL][2]["n_entries"] == 2 * cl["n_mutual"]
                    assert models[KA.EITHER][2]["n_entries"] == 2 * (cl["n_edges"] - cl["n_mutual"])
                    assert np.array_equal(KA.components(*models[flags][:2], id_base), labels), (kk, flags, max_dist)


# ---- reach: so that test_knn_adjacency_gpu.py cannot pass vacuously -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def dup_models():
    rows, counts = KG.model_rows(KG.dup_case(), KG.DUP_K)
    return KA.adjacency_models(rows, counts, KG.DUP_K)


def test_the_duplicates_make_hubs_and_empty_segments(dup_models):
    """dup_case() at kk = 5: segments longer than a sub-tile of the sort and than the merge's wave team, and thousands of empty ones"""
    deg = np.diff(dup_models[KA.REVERSE][0].astype(np.int64))
    assert int(deg.max()) == 8525 and int((deg > KA.RS_TILE).sum()) == 5 and int((deg == 0).sum()) == 8550
    assert 2 * KA.RS_TILE < 8525 and 8525 > KA.TEAM_DEGREE                   # a run over three sub-tiles; the block team
    assert [dup_models[f][2]["n_entries"] for f in KA.FLAGS] == [45000, 1154, 88846]
    assert dup_models[KA.REVERSE][2] == dict(n_edges=45000, n_entries=45000, n_empty=8550, max_degree=8525)
    either = np.diff(dup_models[KA.EITHER][0].astype(np.int64))
    assert int(either.max()) > KA.TEAM_DEGREE and 0 < int(either.min()) <= KA.TEAM_DEGREE and KG.DUP_N * KG.DUP_K > 2 * KA.RS_BLOCK_ITEMS
    assert int((np.diff(dup_models[KA.MUTUAL][0].astype(np.int64)) == 0).sum()) > 0


def test_the_three_flags_differ_on_the_hub_set():
    codes, hub = KG.hub_case()
    rows, counts = KG.model_rows(codes, KG.HUB_K)
    m = KA.adjacency_models(rows, counts, KG.HUB_K)
    assert len({m[f][2]["n_entries"] for f in KA.FLAGS}) == 3
    seg = {f: KA.segments(m[f][0], m[f][1])[hub] for f in KA.FLAGS}
    assert len(seg[KA.REVERSE]) == KG.HUB_SATELLITES and len(seg[KA.MUTUAL]) == KG.HUB_K and len(seg[KA.EITHER]) == KG.HUB_SATELLITES
    for a, b in ((KA.REVERSE, KA.MUTUAL), (KA.REVERSE, KA.EITHER), (KA.MUTUAL, KA.EITHER)):
        assert not (np.array_equal(m[a][0], m[b][0]) and np.array_equal(m[a][1], m[b][1]))
    assert max(int(v) >> 32 for v in KG.model_rows(KG.hub_case(256)[0], 100)[0].ravel().tolist() if v != int(KG.INF)) == 255   # no distance of `bits` there


@pytest.mark.parametrize("bits", [256, 512])
def test_the_complement_set_has_both_distance_digits_inside_one_segment(bits):
    codes = KA.complement_case(bits)
    assert len(codes) == 40
    rows, counts = KG.model_rows(codes, 100)
    assert int(rows[:, :39].max() >> np.uint64(32)) == bits                  # the code and its exact complement list each other
    for flags in KA.FLAGS:
        offsets, adj, st = KA.adjacency_model(rows, counts, 100, flags)
        assert st["n_entries"] == 40 * 39 and st["n_empty"] == 0
        both = [int((seg >> np.uint64(32)).min()) < 256 <= int((seg >> np.uint64(32)).max()) for seg in KA.segments(offsets, adj)]
        assert sum(both) >= (2 if bits == 256 else 40), (bits, flags)        # digits of the first AND of the second distance pass in one segment
    assert KA.dist_passes(KA.NO_CAP, bits) == 2


def test_the_sweep_crosses_a_block_of_the_sort_and_the_big_store_takes_three_key_passes():
    assert 2000 * 10 > KA.RS_BLOCK_ITEMS > 2000 * 1 and KA.key_passes(2000) == 2 and KA.key_passes(66000) == 3
    codes = KG.clustered_case(64, n=2000)
    rows, counts = KG.model_rows(codes, 12)
    for max_dist in (KA.NO_CAP, 64 // 4):
        m = KA.adjacency_models(rows, counts, 10, max_dist)
        assert len({m[f][2]["n_entries"] for f in KA.FLAGS}) == 3 and all(m[f][2]["n_entries"] > 0 for f in KA.FLAGS), max_dist
