"""vc_cluster_snn* without a GPU: the ABI surface, the code objects of the kernels, the plan arithmetic under the sanitizers, and the
expectation of test_snn_gpu.py -- that the numpy model agrees with plain set loops, and that the noisy input makes every threshold
and both flags matter."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import knn_graph_common as KG
import snn_common as SN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_new_names(vc):
    txt = open(os.path.join(ROOT, "include", "verticut_gpu.h")).read()
    assert re.search(r"#define\s+VC_ABI_VERSION\s+2\b", txt)             # entry points are only added
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"typedef struct vc_cluster_snn_stats\s*\{\s*uint64_t n_edges;\s*uint64_t n_mutual;\s*uint64_t n_joined;\s*uint64_t n_clusters;"
                     r"\s*uint32_t max_shared;\s*uint32_t pad;\s*\}\s*vc_cluster_snn_stats;", code)
    assert re.search(r"#define\s+VC_SNN_MAX_KK\s+1024u", code) and re.search(r"#define\s+VC_SNN_NONE\s+0xFFFFFFFFu", code)
    assert code.index("vc_cluster_knn_stats;") < code.index("VC_SNN_MAX_KK") < code.index("vc_device_status")   # after the vc_cluster_knn* block
    L = ctypes.CDLL(vc.LIB_PATH)
    for name in SN.SNN_NAMES:
        assert hasattr(L, name), name
        assert name in vc.EXPORTS
    for name in ("vc_cluster_snn_dev", "vc_sharded_cluster_snn_dev"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*const uint64_t\* d_rows,\s*const uint32_t\* d_counts,\s*uint32_t k,\s*uint32_t kk,"
                         r"\s*uint32_t flags,\s*uint32_t max_dist,\s*uint32_t min_shared,\s*uint32_t\* d_labels,\s*uint32_t\* d_shared,\s*uint64_t\* d_hist,"
                         r"\s*vc_cluster_snn_stats\* stats,\s*void\* stream\)" % name, code), name
    for name in ("vc_cluster_snn", "vc_sharded_cluster_snn"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*const uint64_t\* rows,\s*const uint32_t\* counts,\s*uint32_t k,\s*uint32_t kk,"
                         r"\s*uint32_t flags,\s*uint32_t max_dist,\s*uint32_t min_shared,\s*uint32_t\* labels,\s*uint32_t\* shared,\s*uint64_t\* hist,"
                         r"\s*vc_cluster_snn_stats\* stats\)" % name, code), name
    flat = " ".join(txt.split()).replace(" * ", " ")
    for phrase in ("Jarvis and Patrick, 1973", "the record itself is never in its own set", "kk lies in 1 .. min(k, VC_SNN_MAX_KK)",
                   "shared(i, j) = |S_i n S_j|, symmetric, in 0 .. kk - 1", "Every word is written", "it sums to n_edges",
                   "joined iff they are a candidate pair AND shared(i, j) >= min_shared",
                   "min_shared == 0 gives vc_cluster_knn*'s labels, n_edges, n_mutual and n_clusters bit for bit", "min_shared >= kk joins nothing",
                   "a mutual pair from its smaller member, a one-sided pair (VC_KNN_EITHER) from the row that lists it",
                   "not of lane order, block order or the hash function used", "an entry whose id equals the row's own",
                   "nothing is read or written out of bounds", "the call terminates and stays in bounds",
                   "N == 1 gives the record its own label and all of d_shared VC_SNN_NONE", "WAITS: one, at the end", "no shard is touched",
                   "NOT OFFERED: closed neighbour sets", "a Jaccard threshold, which the caller derives from d_shared and the counts", "kk above 1024"):
        assert " ".join(phrase.split()) in flat, phrase
    assert vc.VC_ABI_VERSION == 2
    st = vc.VcClusterSnnStats
    assert ctypes.sizeof(st) == 40 and [getattr(st, n).offset for n in SN.SNN_STATS] == [0, 8, 16, 24, 32]
    assert st().as_dict() == SN.zero_stats()
    assert (vc.SNN_NONE, vc.SNN_MAX_KK) == (int(SN.NONE), SN.MAX_KK)
    for cls in (vc.Engine, vc.ShardedEngine):
        for meth in ("cluster_snn", "cluster_snn_dev"):
            assert callable(getattr(cls, meth)), (cls, meth)
    host = open(os.path.join(ROOT, "verticut_amd", "host", "verticut_host.hpp")).read()
    assert re.search(r"virtual int cluster_snn\([^)]*\)\s*=\s*0;", host)
    assert len(re.findall(r"int cluster_snn\([^)]*\)\s*override", host)) == 2
    assert "return vc_cluster_snn(h_," in host and "return vc_sharded_cluster_snn(h_," in host
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "5.19" in design and "vc_cluster_snn" in design and "VC_SNN_WAVE_KK" in design
    for doc in ("README.md", "INTEGRATION.md"):
        assert "vc_cluster_snn" in open(os.path.join(ROOT, doc)).read(), doc
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_snn.py"))


def test_snn_kernels_use_static_lds_only(vc):
    """every kernel of vc_snn.o has no scratch memory and no spills, and no more static LDS than the plan header states"""
    from verticut_amd import build as vb
    assert "vc_snn.hip" in vb.SOURCES and "vc_snn_plan.hpp" in vb.HEADERS
    res = vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_snn.o"))
    plan = open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_snn_plan.hpp")).read()
    assert re.search(r"#define\s+VC_SNN_WAVE_KK\s+%du" % SN.WAVE_KK, plan)
    lds_wave = 4 * 4 * 2 * SN.WAVE_KK + 4 * SN.WAVE_KK                      # VC_SNN_LDS_BYTES_WAVE: four sets of 2 B words, B counters
    lds_block = 4 * 2 * SN.MAX_KK + 4 * SN.MAX_KK                           # VC_SNN_LDS_BYTES_BLOCK
    assert "// %d" % lds_wave in plan and "// %d" % lds_block in plan
    limits = {"vc_snn_init_kernel": 0, "vc_snn_kernelILi1E": lds_wave, "vc_snn_kernelILi4E": lds_block}
    for kernel in limits:
        assert sum(kernel in name for name in res) == 1, (kernel, sorted(res))
    assert len(res) == len(limits), sorted(res)
    for name, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        limit = [v for k, v in limits.items() if k in name][0]
        assert r["group_segment_fixed_size"] <= limit, (name, r)
    text = open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_snn.hip")).read()
    for word in ("hipLaunchCooperativeKernel", "grid_group", "extern __shared__", "getenv"):
        assert word not in text, word
    # the other graph object keeps its kernels to itself
    assert "vc_snn" not in open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_knn_graph.hip")).read()


def test_plan_arithmetic_under_the_sanitizers(tmp_path):
    """tests/cpp/snn_plan_test.cc over csrc/vc_snn_plan.hpp, host code only, with AddressSanitizer and UBSan; the constants and the
    shapes it prints are those of the model's mirror"""
    src = os.path.join(ROOT, "tests", "cpp", "snn_plan_test.cc")
    exe = tmp_path / "snn_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           src, "-I", os.path.join(ROOT, "verticut_amd", "csrc")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert out.stdout.startswith("snn plan ok: WAVE_KK %d MAX_KK %d STAT 40\n" % (SN.WAVE_KK, SN.MAX_KK))
    B = SN.WAVE_KK
    for kk in (1, 64, 65, B, B + 1, SN.MAX_KK):
        assert re.search(r"^TEAM %d %d %d %d$" % (kk, SN.table_slots(kk), SN.team_waves(kk), SN.entry_lanes(kk)), out.stdout, flags=re.M), (kk, out.stdout)
    assert re.search(r"^STAGE %d$" % SN.stage_total(700, 70, 64, True, True, True), out.stdout, flags=re.M)
    assert SN.team_waves(B) == 1 and SN.team_waves(B + 1) == 4 and SN.table_slots(SN.MAX_KK) == 2048
    assert SN.kk_ok(10, 10) and not SN.kk_ok(10, 11) and not SN.kk_ok(10, 0) and SN.kk_ok(8191, 1024) and not SN.kk_ok(8191, 1025)


# ---- the expectation ------------------------------------------------------------------------------------------------------------------
def _loops(rows, counts, kk, min_shared, flags, max_dist, id_base):
    """the contract by plain Python sets and relabelling until nothing changes"""
    n = len(rows)
    lists = [[(int(v) >> 32, (int(v) & 0xFFFFFFFF) - id_base) for v in rows[i, :min(kk, int(counts[i]))]] for i in range(n)]
    S = [{j for d, j in lst if d <= max_dist} for lst in lists]
    shared = np.full((n, kk), SN.NONE, dtype=np.uint32)
    hist = np.zeros(kk, dtype=np.uint64)
    joined = set()
    for i in range(n):
        assert i not in S[i]
        for jj, (d, j) in enumerate(lists[i]):
            if d > max_dist:
                continue
            s = len(S[i] & S[j])
            shared[i, jj] = s
            hist[s] += np.uint64(1)
            candidate = (i in S[j]) if flags == KG.MUTUAL else True
            if candidate and s >= min_shared:
                joined.add((min(i, j), max(i, j)))
    comp = list(range(n))
    changed = True
    while changed:
        changed = False
        for a, b in joined:
            if comp[a] != comp[b]:
                comp[a] = comp[b] = min(comp[a], comp[b])
                changed = True
    listed = [int(x) for x in shared[shared != SN.NONE]]
    st = dict(n_edges=sum(len(s) for s in S), n_mutual=sum(1 for i in range(n) for j in S[i] if i < j and i in S[j]), n_joined=len(joined),
              n_clusters=len(set(comp)), max_shared=max(listed) if listed else 0)
    return np.array(comp, dtype=np.uint32) + np.uint32(id_base), shared, hist, st


def _pin(codes, k, kks, id_base, cap):
    rows, counts = KG.model_rows(codes, k, id_base)
    for kk in kks:
        for flags in (KG.MUTUAL, KG.EITHER):
            for max_dist in (0xFFFFFFFF, cap):
                for min_shared in (0, 1, kk):
                    got = SN.snn_model(rows, counts, kk, min_shared, flags, max_dist, id_base)
                    SN.same_snn(got, _loops(rows, counts, kk, min_shared, flags, max_dist, id_base), (kk, flags, max_dist, min_shared))
                    assert int(got[2].sum()) == got[3]["n_edges"] and (min_shared < kk or got[3]["n_joined"] == 0)
                    # symmetric, below kk, and NONE exactly where nothing is listed
                    listed = got[1] != SN.NONE
                    assert np.all(got[1][listed] < kk) and int(listed.sum()) == got[3]["n_edges"]


def test_the_model_is_the_contract_on_the_hub_set():
    codes, _ = KG.hub_case()
    _pin(codes, KG.HUB_K, (1, 3, KG.HUB_K), 1000, 1)
    _pin(codes, 100, (100,), 0, 2)                                             # rows shorter than kk: every row holds the whole store


def test_the_model_is_the_contract_on_a_small_mixed_set():
    codes = SN.mixed_case(64, n=120)
    _pin(codes, 12, (1, 5, 10, 12), 7, 64 // 4)


def test_no_threshold_is_cluster_knn():
    for codes, k in ((SN.mixed_case(64, n=120), 12), (KG.hub_case()[0], KG.HUB_K)):
        rows, counts = KG.model_rows(codes, k, 50)
        for kk in (1, 4, k):
            for flags in (KG.MUTUAL, KG.EITHER):
                for max_dist in (0xFFFFFFFF, 16):
                    labels, _, _, st = SN.snn_model(rows, counts, kk, 0, flags, max_dist, 50)
                    want_labels, _, want = KG.cluster_model(rows, counts, kk, flags, max_dist, 50)
                    assert np.array_equal(labels, want_labels)
                    assert [st[n] for n in ("n_edges", "n_mutual", "n_clusters")] == [want[n] for n in ("n_edges", "n_mutual", "n_clusters")]


# ---- reach: the noisy input makes the thresholds and the flags matter, so that test_snn_gpu.py cannot pass vacuously --------------------
@pytest.mark.parametrize("bits", [64, 128, 256])
def test_the_mixed_set_spreads_the_overlaps_and_every_threshold_bites(bits):
    for k, kk in ((12, 10), (70, 64), (70, 65)):
        codes, rows, counts = SN.mixed_graph(bits, k)
        assert len(codes) == 700
        shared, hist, edges = SN.snn_weights(rows, counts, kk)
        if kk >= 64:
            assert np.all(hist > 0), (bits, kk, hist)                          # shared spans 0 .. kk - 1
        seen = {}
        for flags in (KG.MUTUAL, KG.EITHER):
            counts_by_t = []
            for t in (0, 1, kk // 4, kk // 2, 3 * kk // 4, kk - 1):
                seen[flags, t] = SN.snn_labels(len(rows), edges, t, flags)
                counts_by_t.append(seen[flags, t][1]["n_clusters"])
            assert all(a < b for a, b in zip(counts_by_t[1:], counts_by_t[2:])), (bits, kk, flags, counts_by_t)   # 1 < kk/4 < kk/2 < 3kk/4 < kk - 1
            if kk == 10:
                assert counts_by_t[0] < counts_by_t[1], (bits, flags, counts_by_t)                                 # and 0 apart from 1
            else:
                assert counts_by_t[0] == counts_by_t[1] == 1
        # the flags differ: one-sided pairs pass the threshold, so EITHER joins more pairs than MUTUAL does.  At kk = 10 that holds
        # at every threshold, in the labels too.  At kk = 64 and 65 it holds up to kk / 2 (in the labels from kk / 4 on: at 1 both
        # flags give one cluster); two lists that share three quarters or more of their entries belong to records that list each
        # other on this input, at 128 and 256 bits without exception, so there the flags coincide and only the threshold is tested.
        low = (1, kk // 4, kk // 2)
        for t in low + ((3 * kk // 4, kk - 1) if kk == 10 else ()):
            assert seen[KG.MUTUAL, t][1]["n_joined"] < seen[KG.EITHER, t][1]["n_joined"], (bits, kk, t)
            if kk == 10 or t != 1:
                assert not np.array_equal(seen[KG.MUTUAL, t][0], seen[KG.EITHER, t][0]), (bits, kk, t)
                assert seen[KG.MUTUAL, t][1]["n_clusters"] > seen[KG.EITHER, t][1]["n_clusters"], (bits, kk, t)
        if (bits, kk) == (64, 10):
            assert [seen[f, t][1]["n_clusters"] for f in (KG.MUTUAL, KG.EITHER) for t in (0, 1)] == [299, 372, 1, 7]
        capped = SN.snn_weights(rows, counts, kk, bits // 4)                   # the cap of the sweep removes some entries, not all
        assert 0 < len(capped[2]) < len(edges) and np.any(capped[0][:, 0] == SN.NONE) and np.any(capped[0][:, 0] != SN.NONE), (bits, kk)
