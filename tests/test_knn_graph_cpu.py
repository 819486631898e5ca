"""The k-NN graph calls without a GPU: the ABI surface, the code object of the kernels, the plan arithmetic under the sanitizers, and
the expectation of test_knn_graph_gpu.py -- that the numpy model agrees with plain loops, and that the crafted inputs reach what they
are there for."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import knn_graph_common as KG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_new_names(vc):
    txt = open(os.path.join(ROOT, "include", "verticut_gpu.h")).read()
    assert re.search(r"#define\s+VC_ABI_VERSION\s+2\b", txt)             # entry points are only added
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"typedef struct vc_knn_graph_stats\s*\{\s*uint32_t n_rounds_max;\s*uint32_t k_last;\s*uint64_t n_searched;\s*uint64_t n_linear;"
                     r"\s*uint64_t n_gave_up;\s*\}\s*vc_knn_graph_stats;", code)
    assert re.search(r"typedef struct vc_cluster_knn_stats\s*\{\s*uint64_t n_edges;\s*uint64_t n_mutual;\s*uint64_t n_clusters;\s*uint32_t max_in_degree;"
                     r"\s*uint32_t pad;\s*\}\s*vc_cluster_knn_stats;", code)
    assert re.search(r"#define\s+VC_KNN_MUTUAL\s+0u", code) and re.search(r"#define\s+VC_KNN_EITHER\s+1u", code)
    L = ctypes.CDLL(vc.LIB_PATH)
    for name in KG.GRAPH_NAMES + KG.CLUSTER_NAMES:
        assert hasattr(L, name), name
        assert name in vc.EXPORTS
    for name in ("vc_knn_graph_dev", "vc_sharded_knn_graph_dev"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*uint32_t k,\s*uint32_t mode,\s*uint32_t batch,\s*uint64_t first,\s*uint64_t count,"
                         r"\s*uint32_t k_first,\s*uint64_t\* d_rows,\s*uint32_t\* d_counts,\s*vc_knn_graph_stats\* stats,\s*void\* stream\)" % name, code), name
    for name in ("vc_knn_graph", "vc_sharded_knn_graph"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*uint32_t k,\s*uint32_t mode,\s*uint32_t batch,\s*uint64_t first,\s*uint64_t count,"
                         r"\s*uint32_t k_first,\s*uint64_t\* rows,\s*uint32_t\* counts,\s*vc_knn_graph_stats\* stats\)" % name, code), name
    for name in ("vc_cluster_knn_dev", "vc_sharded_cluster_knn_dev"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*const uint64_t\* d_rows,\s*const uint32_t\* d_counts,\s*uint32_t k,\s*uint32_t kk,"
                         r"\s*uint32_t flags,\s*uint32_t max_dist,\s*uint32_t\* d_labels,\s*uint32_t\* d_in_degree,\s*vc_cluster_knn_stats\* stats,"
                         r"\s*void\* stream\)" % name, code), name
    for name in ("vc_cluster_knn", "vc_sharded_cluster_knn"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*const uint64_t\* rows,\s*const uint32_t\* counts,\s*uint32_t k,\s*uint32_t kk,"
                         r"\s*uint32_t flags,\s*uint32_t max_dist,\s*uint32_t\* labels,\s*uint32_t\* in_degree,\s*vc_cluster_knn_stats\* stats\)" % name, code), name
    flat = " ".join(txt.split()).replace(" * ", " ")
    for phrase in ("count == 0 means \"to the end\"", "over all resident records OTHER than record id_base + p itself", "d_counts[p - first] = min(k, N - 1)",
                   "Ties go to the smaller id", "Duplicates of the record are ordinary neighbours at distance 0",
                   "a function of the database, k and the range only", "VC_MODE_MIH_APPROX is refused",
                   "without VC_FLAG_REF_SIGNEXT_KEYS and without VC_FLAG_REF_STOP_LITERAL4 at n_tables < 4", "There is no truncation flag",
                   "k lies in 1 .. VC_MAX_K - 1", "With count_j < kk (N - 1 < kk) every other record is in row j", "max_dist >= bits means no cap",
                   "(d << 32 | i) <= row_j[m - 1]", "There is no `order` argument"):
        assert " ".join(phrase.split()) in flat, phrase
    assert vc.VC_ABI_VERSION == 2
    st = vc.VcKnnGraphStats
    assert ctypes.sizeof(st) == 32 and [getattr(st, n).offset for n in KG.GRAPH_STATS] == [0, 4, 8, 16, 24]
    assert st().as_dict() == KG.zero_graph_stats()
    st = vc.VcClusterKnnStats
    assert ctypes.sizeof(st) == 32 and [getattr(st, n).offset for n in KG.CLUSTER_STATS] == [0, 8, 16, 24]
    assert st().as_dict() == KG.zero_cluster_stats()
    assert (vc.KNN_MUTUAL, vc.KNN_EITHER) == (KG.MUTUAL, KG.EITHER)
    for cls in (vc.Engine, vc.ShardedEngine):
        for meth in ("knn_graph", "knn_graph_dev", "cluster_knn", "cluster_knn_dev"):
            assert callable(getattr(cls, meth)), (cls, meth)
    host = open(os.path.join(ROOT, "verticut_amd", "host", "verticut_host.hpp")).read()
    for meth in ("knn_graph", "cluster_knn"):
        assert re.search(r"virtual int %s\([^)]*\)\s*=\s*0;" % meth, host)
        assert len(re.findall(r"int %s\([^)]*\)\s*override" % meth, host)) == 2
        assert "return vc_%s(h_," % meth in host and "return vc_sharded_%s(h_," % meth in host
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "5.16" in design and "vc_knn_graph" in design and "vc_cluster_knn" in design
    for doc in ("README.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "vc_knn_graph" in text and "vc_cluster_knn" in text, doc
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_knn_graph.py"))


def test_graph_kernels_use_no_scratch_and_no_lds(vc):
    """every kernel of vc_knn_graph.o has no scratch memory, no spills and no LDS"""
    from verticut_amd import build as vb
    assert "vc_knn_graph.hip" in vb.SOURCES and "vc_knn_graph_plan.hpp" in vb.HEADERS
    res = vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_knn_graph.o"))
    kernels = ("vc_kgraph_settle_kernel", "vc_kgraph_gather_kernel", "vc_kgraph_init_kernel", "vc_kgraph_edge_kernel", "vc_kgraph_degree_kernel")
    for kernel in kernels:
        assert sum(kernel in name for name in res) == 1, (kernel, sorted(res))
    assert len(res) == len(kernels), sorted(res)
    for name, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == 0, (name, r)
    text = open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_knn_graph.hip")).read()
    assert "getenv" not in text                                              # the knob is read in read_knobs, nowhere else
    engine = open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_engine.hip")).read()
    assert engine.count('getenv("VC_KGRAPH_SCRATCH")') == 1
    for word in ("hipLaunchCooperativeKernel", "__threadfence", "grid_group", "__shared__"):
        assert word not in text, word


def test_plan_arithmetic_under_the_sanitizers(tmp_path):
    """tests/cpp/knn_graph_plan_test.cc over csrc/vc_knn_graph_plan.hpp, host code only, with AddressSanitizer and UBSan; the constants
    and the planned cases it prints are those of the model's mirror"""
    src = os.path.join(ROOT, "tests", "cpp", "knn_graph_plan_test.cc")
    exe = tmp_path / "knn_graph_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           src, "-I", os.path.join(ROOT, "verticut_amd", "csrc")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert out.stdout.startswith("knn graph plan ok: MAXK %d SCRATCH %d BATCH %d\n" % (KG.MAX_K, KG.SCRATCH_DEFAULT, KG.BATCH_DEFAULT))
    for k in (1, 10, 100, 5, 4095, 8191):
        assert re.search(r"^FIRST %d %d$" % (k, KG.first_k(k, 0, False)), out.stdout, flags=re.M), (k, out.stdout)
    for nq in (1, 4096):
        assert re.search(r"^WORK %d %d$" % (nq, KG.work_total(nq, 2, 33)), out.stdout, flags=re.M), (nq, out.stdout)
    assert KG.schedule(10, 0) == [22, 44, 88, 176, 352, 704, 1408, 2816, 5632, 8192] and KG.schedule(10, 8192) == [8192]
    assert KG.sub_batch(KG.SCRATCH_DEFAULT, 8192) == 1024 and KG.sub_batch(0, 8192) == 1 and KG.rows_bytes(5, 1 << 20, 100) == 4000
    assert KG.key_range(10, 3, 0) == (True, 7) and KG.key_range(10, 3, 8) == (False, 0) and KG.key_range(0, 0, 0) == (True, 0)
    assert KG.k_ok(1) and KG.k_ok(8191) and not KG.k_ok(8192) and KG.k_first_ok(10, 11) and not KG.k_first_ok(10, 10)


# ---- the expectation ------------------------------------------------------------------------------------------------------------------
def _dist(a, b):
    return bin(int.from_bytes(bytes(a ^ b), "little")).count("1")


@pytest.mark.parametrize("seed", range(6))
def test_the_model_is_the_rule(seed):
    """against plain double loops, on small random inputs with few distinct codes, so that ties and duplicates are common"""
    rng = np.random.default_rng(seed)
    nbytes, n, id_base = 8, int(rng.integers(1, 60)), int(rng.integers(0, 50))
    pool = rng.integers(0, 256, size=(5, nbytes), dtype=np.uint8)
    codes = pool[rng.integers(0, 5, size=n)] ^ rng.integers(0, 2, size=(n, nbytes), dtype=np.uint8)
    for k in (1, 3, max(n - 1, 1), n + 2):
        rows, counts = KG.model_rows(codes, k, id_base)
        want_rows, want_counts = KG.loop_rows(codes, k, id_base)
        assert np.array_equal(rows, want_rows) and np.array_equal(counts, want_counts), k
        if n > 4:
            part = KG.model_rows(codes, k, id_base, first=2, count=n - 4)
            assert np.array_equal(part[0], rows[2:n - 2]) and np.array_equal(part[1], counts[2:n - 2])
        for kk in {1, min(2, k), k}:
            for flags in (KG.MUTUAL, KG.EITHER):
                for max_dist in (0xFFFFFFFF, 3):
                    labels, deg, st = KG.cluster_model(rows, counts, kk, flags, max_dist, id_base)
                    # the edges by the definition: j is one of the min(kk, N - 1) nearest others of i by (dist, id), within the cap
                    lists = [sorted((_dist(codes[i], codes[j]), j) for j in range(n) if j != i)[:kk] for i in range(n)]
                    E = [{j for d, j in lst if d <= max_dist} for lst in lists]
                    assert st["n_edges"] == sum(len(e) for e in E)
                    assert np.array_equal(deg, np.bincount([j for e in E for j in e], minlength=n).astype(np.uint32))
                    assert st["n_mutual"] == sum(1 for i in range(n) for j in E[i] if i < j and i in E[j])
                    comp = list(range(n))                                  # components by relabelling until nothing changes
                    changed = True
                    while changed:
                        changed = False
                        for i in range(n):
                            for j in E[i]:
                                if (flags == KG.EITHER or i in E[j]) and comp[i] != comp[j]:
                                    comp[i] = comp[j] = min(comp[i], comp[j])
                                    changed = True
                    assert np.array_equal(labels, np.array(comp, dtype=np.uint32) + np.uint32(id_base))
                    assert st["n_clusters"] == len(set(comp)) and st["max_in_degree"] == (int(deg.max()) if n else 0)
                    # and the one compare agrees with the sets
                    for i in range(n):
                        for j in range(n):
                            mj = min(kk, int(counts[j]))
                            if i != j and mj:
                                d = _dist(codes[i], codes[j])
                                listed = ((d << 32) | (id_base + i)) <= int(rows[j, mj - 1])
                                assert listed == (i in {x for _, x in lists[j]}), (i, j)


@pytest.mark.parametrize("seed", range(4))
def test_the_plan_mirror_is_the_rounds(seed):
    """plan_stats against a literal replay of the rounds on sorted distance lists"""
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(2, 80))
    pool = rng.integers(0, 256, size=(3, 8), dtype=np.uint8)
    codes = pool[rng.integers(0, 3, size=n)] ^ (rng.integers(0, 8, size=(n, 8)) == 0).astype(np.uint8)
    H = KG.dist_hist(codes)
    assert np.all(H.sum(axis=1) == n) and np.all(H[:, 0] >= 1)
    for k in (1, 2, 7):
        for k_first in (0, k + 1, 16):
            if not KG.k_first_ok(k, k_first):
                continue
            searched, linear, k_last, rounds_max = 0, 0, 0, 0
            for i in range(n):
                ds = sorted(_dist(codes[i], codes[j]) for j in range(n))     # the own record's 0 among them
                rounds = 0
                for kp in KG.schedule(k, k_first):
                    rounds, searched, k_last = rounds + 1, searched + 1, max(k_last, kp)
                    if n < kp:
                        break
                    D = ds[kp - 1]
                    if sum(1 for d in ds[:kp] if d < D) - (1 if D > 0 else 0) >= k:
                        break
                else:
                    linear, rounds = linear + 1, rounds + 1
                rounds_max = max(rounds_max, rounds)
            assert KG.plan_stats(H, k, k_first) == dict(n_rounds_max=rounds_max, k_last=k_last, n_searched=searched, n_linear=linear, n_gave_up=0), (k, k_first)
        assert KG.plan_stats(H, k, linear=True) == dict(n_rounds_max=1, k_last=k + 1, n_searched=n, n_linear=0, n_gave_up=0)


# ---- reach: the crafted inputs do what they are for ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [64, 128, 256, 512])
def test_the_tie_heavy_sets_take_more_than_one_round(bits):
    codes = KG.clustered_case(bits)
    assert 1500 <= len(codes) <= 9000
    H = KG.dist_hist(codes)
    for k in (1, 10, 100):
        st = KG.plan_stats(H, k)
        assert st["n_linear"] == 0 and st["n_searched"] >= len(codes), (bits, k, st)
        if k <= 10:                                                          # (at k = 100 the first k' = 202 may already reach past the ties)
            assert st["n_rounds_max"] > 2 and st["n_searched"] > 2 * len(codes), (bits, k, st)
        assert KG.plan_stats(H, k, KG.MAX_K) == dict(n_rounds_max=1, k_last=KG.MAX_K, n_searched=len(codes), n_linear=0, n_gave_up=0)
    rows, _ = KG.model_rows(codes, 10)
    last = rows[:, 9] >> np.uint64(32)
    tied = sum(int(H[i, int(last[i])]) > 10 for i in range(len(codes)))
    assert tied > len(codes) // 2                                            # more records tie at the tenth distance than the row takes


def test_the_duplicate_set_reaches_the_linear_scan():
    codes = KG.dup_case()
    assert len(codes) == KG.DUP_N <= 9000
    copies = KG.dup_copies(codes)
    assert len(copies) == KG.DUP_COPIES > KG.MAX_K and copies[0] > 0 and np.any(np.diff(copies) > 1)      # scattered over the ids
    H = KG.dist_hist(codes)
    st = KG.plan_stats(H, KG.DUP_K, KG.DUP_K_FIRST)
    assert KG.DUP_COPIES <= st["n_linear"] < KG.DUP_N and st["k_last"] == KG.MAX_K and st["n_rounds_max"] == len(KG.schedule(KG.DUP_K, KG.DUP_K_FIRST)) + 1
    assert KG.plan_stats(H, KG.DUP_K)["n_linear"] == st["n_linear"]          # k_first moves the rounds, not the verdicts
    rows, counts = KG.model_rows(codes, KG.DUP_K, first=int(copies[-1]), count=1)
    assert np.array_equal(rows[0], copies[:KG.DUP_K].astype(np.uint64)) and counts[0] == KG.DUP_K


def test_the_clustered_graph_has_asymmetric_pairs_and_merging_components():
    codes = KG.clustered_case(64)
    rows, counts = KG.model_rows(codes, 10)
    for kk in (1, 4, 10):
        E = KG.edge_sets(rows, counts, kk, 0xFFFFFFFF)
        assert any(i not in E[j] for i in range(len(E)) for j in E[i]), kk    # j is listed by i but does not list i
        mutual, either = KG.cluster_model(rows, counts, kk, KG.MUTUAL), KG.cluster_model(rows, counts, kk, KG.EITHER)
        assert mutual[2]["n_clusters"] > either[2]["n_clusters"] > 0
        merged = [(i, j) for i in range(len(E)) for j in E[i] if mutual[0][i] != mutual[0][j] and either[0][i] == either[0][j]]
        assert merged, kk                                                     # two mutual components that one-way edges make one
        assert mutual[2]["n_edges"] == either[2]["n_edges"] and mutual[2]["n_mutual"] == either[2]["n_mutual"] and np.array_equal(mutual[1], either[1])
    capped = KG.cluster_model(rows, counts, 10, KG.EITHER, 2)
    assert 0 < capped[2]["n_edges"] < KG.cluster_model(rows, counts, 10, KG.EITHER)[2]["n_edges"]


def test_the_hub_set_and_the_short_rows():
    codes, hub = KG.hub_case()
    k = KG.HUB_K
    rows, counts = KG.model_rows(codes, k)
    sats = [i for i in range(KG.HUB_SATELLITES + 1) if i != hub]
    assert all(int(rows[i, 0]) == (1 << 32) | hub for i in sats)             # every satellite lists the hub first
    assert [int(v) & 0xFFFFFFFF for v in rows[hub]] == sats[:k]              # the hub lists the k satellites of smallest id
    for kk in (1, 3, k):
        mutual, either = KG.cluster_model(rows, counts, kk, KG.MUTUAL), KG.cluster_model(rows, counts, kk, KG.EITHER)
        assert mutual[1][hub] == KG.HUB_SATELLITES > k and mutual[2]["max_in_degree"] == KG.HUB_SATELLITES
        assert mutual[2]["n_clusters"] > either[2]["n_clusters"]
        assert len({int(either[0][i]) for i in sats + [hub]}) == 1
    assert KG.cluster_model(rows, counts, 3, KG.MUTUAL)[0][KG.HUB_SATELLITES] == KG.HUB_SATELLITES
    # rows shorter than kk: N - 1 < kk, every other record is listed, the graph is complete both ways
    short = KG.clustered_case(64)[:7]
    rows, counts = KG.model_rows(short, 10)
    assert np.all(counts == 6)
    for kk in (7, 10):
        labels, deg, st = KG.cluster_model(rows, counts, kk, KG.MUTUAL)
        assert st == dict(n_edges=42, n_mutual=21, n_clusters=1, max_in_degree=6) and np.all(deg == 6) and np.all(labels == 0)
