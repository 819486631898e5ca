"""vc_knn_graph_retain* without a GPU: the ABI surface, the code object of the kernels, the plan arithmetic under the sanitizers, and
the expectation of test_knn_graph_retain_gpu.py -- that the numpy model over the whole old graph equals knn_graph_common.model_rows
over the survivors for every crafted input, and that the inputs reach what they are there for."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import knn_graph_common as KG
import knn_graph_retain_common as KR
import knn_graph_update_common as KU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_new_names(vc):
    txt = open(os.path.join(ROOT, "include", "verticut_gpu.h")).read()
    assert re.search(r"#define\s+VC_ABI_VERSION\s+2\b", txt)             # entry points are only added
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"typedef struct vc_knn_graph_retain_stats\s*\{\s*vc_knn_graph_stats repair;\s*uint64_t n_rows_kept;\s*uint64_t n_rows_short;"
                     r"\s*uint64_t n_entries_dropped;\s*uint64_t pad;\s*\}\s*vc_knn_graph_retain_stats;", code)
    L = ctypes.CDLL(vc.LIB_PATH)
    for name in KR.RETAIN_NAMES:
        assert hasattr(L, name), name
        assert name in vc.EXPORTS
    for name in ("vc_knn_graph_retain_dev", "vc_sharded_knn_graph_retain_dev"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*uint32_t k,\s*uint32_t mode,\s*uint32_t batch,\s*uint64_t n_old,\s*uint32_t k_first,"
                         r"\s*const uint32_t\* d_new_ids,\s*uint64_t\* d_rows,\s*uint32_t\* d_counts,\s*vc_knn_graph_retain_stats\* stats,\s*void\* stream\)"
                         % name, code), name
    for name in ("vc_knn_graph_retain", "vc_sharded_knn_graph_retain"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*uint32_t k,\s*uint32_t mode,\s*uint32_t batch,\s*uint64_t n_old,\s*uint32_t k_first,"
                         r"\s*const uint32_t\* new_ids,\s*uint64_t\* rows,\s*uint32_t\* counts,\s*vc_knn_graph_retain_stats\* stats\)" % name, code), name
    flat = " ".join(txt.split()).replace(" * ", " ")
    for phrase in ("n_old is the record count before it and d_new_ids (n_old words) the map it wrote",
                   "every old row then holds min(k, n_old - 1) entries, and no counts are written", "vc_retain* leaves a current index current",
                   "THE SAME WORDS as vc_knn_graph*(first = 0, count = K)", "Rows and counts [K, n_old) are unspecified afterwards",
                   "Nothing outside the two buffers is written", "the translation has no mode", "m < min(k, K - 1)",
                   "K == n_old: VC_OK, nothing written, the stats zero apart from n_rows_kept", "K == 1: count 0 and a UINT64_MAX row",
                   "n_old < vc_size", "THE OUTPUTS ARE THEN UNDEFINED", "the j-th live word must equal id_base + j", "ONE WAIT for the length S",
                   "that form is vc_knn_graph_retain* below"):
        assert " ".join(phrase.split()) in flat, phrase
    assert vc.VC_ABI_VERSION == 2
    st = vc.VcKnnGraphRetainStats
    assert ctypes.sizeof(st) == 64 and st.repair.offset == 0 and [getattr(st, n).offset for n in KR.RETAIN_STATS] == [32, 40, 48]
    assert st().as_dict() == KR.zero_retain_stats()
    for cls in (vc.Engine, vc.ShardedEngine):
        for meth in ("knn_graph_retain", "knn_graph_retain_dev"):
            assert callable(getattr(cls, meth)), (cls, meth)
    host = open(os.path.join(ROOT, "verticut_amd", "host", "verticut_host.hpp")).read()
    assert re.search(r"virtual int knn_graph_retain\([^)]*\)\s*=\s*0;", host)
    assert len(re.findall(r"int knn_graph_retain\([^)]*\)\s*override", host)) == 2
    assert "return vc_knn_graph_retain(h_," in host and "return vc_sharded_knn_graph_retain(h_," in host
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "5.18" in design and "vc_knn_graph_retain" in design
    for doc in ("README.md", "INTEGRATION.md", os.path.join("profiles", "README.md")):
        assert "knn_graph_retain" in open(os.path.join(ROOT, doc)).read(), doc
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_knn_graph_retain.py"))


def test_retain_kernels_use_no_scratch_and_no_lds(vc):
    """every kernel of vc_knn_graph_retain.o, read from the code object's metadata: no scratch memory, no spills, no LDS; the files
    read no environment and wait for no other block"""
    from verticut_amd import build as vb
    assert "vc_knn_graph_retain.hip" in vb.SOURCES and "vc_knn_graph_retain_plan.hpp" in vb.HEADERS
    res = vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_knn_graph_retain.o"))
    for kernel in KR.RETAIN_KERNELS:
        assert sum(kernel in name for name in res) == 1, (kernel, sorted(res))
    assert len(res) == len(KR.RETAIN_KERNELS), sorted(res)
    for name, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == 0, (name, r)
    # the settle kernel took the id list: still no scratch and no LDS
    graph = vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_knn_graph.o"))
    settle = [r for name, r in graph.items() if "vc_kgraph_settle_kernel" in name]
    assert len(settle) == 1 and settle[0]["private_segment_fixed_size"] == 0 and settle[0]["group_segment_fixed_size"] == 0
    csrc = os.path.join(ROOT, "verticut_amd", "csrc")
    for name in ("vc_knn_graph_retain.hip", "vc_knn_graph_retain_plan.hpp"):
        text = open(os.path.join(csrc, name)).read()
        for word in ("getenv", "hipLaunchCooperativeKernel", "__threadfence", "grid_group", "__shared__", "asm"):
            assert word not in text, (name, word)


def test_plan_arithmetic_under_the_sanitizers(tmp_path):
    """tests/cpp/knn_graph_retain_plan_test.cc over csrc/vc_knn_graph_retain_plan.hpp, host code only, with AddressSanitizer and UBSan;
    the lane map, the chunks and the layout it prints are those of the model's mirror"""
    src = os.path.join(ROOT, "tests", "cpp", "knn_graph_retain_plan_test.cc")
    exe = tmp_path / "knn_graph_retain_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           src, "-I", os.path.join(ROOT, "verticut_amd", "csrc")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert out.stdout.endswith("knn graph retain plan ok: WAVE %d BLOCK %d\n" % (KR.WAVE, KR.BLOCK))
    for k in range(1, 66):
        assert re.search(r"^LANES %d %d %d %d$" % (k, KR.lanes(k), KR.rows_per_wave(k), KR.steps(k)), out.stdout, flags=re.M), (k, out.stdout[:2000])
    assert [KR.rows_per_wave(k) for k in (1, 2, 3, 4, 5, 16, 17, 32, 33, 64, 65)] == [64, 32, 16, 16, 8, 4, 2, 2, 1, 1, 1]
    assert [KR.steps(k) for k in (32, 33, 64, 65, 129, 500)] == [1, 1, 1, 2, 3, 8]
    assert re.search(r"^CHUNK %d %d %d$" % (KR.chunk_rows(4096, 100, 2000), KR.chunk_rows(1, 5, 70), KR.chunk_rows(64 << 20, 10, 2000)), out.stdout, flags=re.M)
    assert (KR.chunk_rows(4096, 100, 2000), KR.chunk_rows(1, 5, 70), KR.chunk_rows(64 << 20, 10, 2000)) == (5, 1, 2000)
    for n in (1, 2, 70, 2000, 1000000):
        assert re.search(r"^WORK %d %d$" % (n, KR.work_total(n, n - n // 10, 33)), out.stdout, flags=re.M), (n, out.stdout[-600:])
    assert not KR.is_short(4, 5, 10) and KR.is_short(3, 5, 10) and KR.is_short(9, 1000, 10) and not KR.is_short(0, 1, 10)


# ---- the expectation ------------------------------------------------------------------------------------------------------------------
def _check(codes, keep, k, id_base=0, what=None):
    """the model over the whole old graph is model_rows over the survivors; returns (old graph, the model's result)"""
    old = KG.model_rows(codes, k, id_base)
    rows, counts, st, short = KR.retain_model(codes, keep, k, id_base, old=old)
    want = KG.model_rows(codes[np.asarray(keep, dtype=bool)], k, id_base)
    KG.same_graph((rows, counts), want, what)
    assert st["n_rows_kept"] == int(np.sum(keep)) and st["n_rows_short"] == len(short)
    # and the rows that were NOT answered again are the rebuild's by translation alone
    plain, m, dropped = KR.translate(old[0], old[1], KR.retain_map(keep, id_base), k, id_base)
    untouched = np.setdiff1d(np.arange(len(plain)), short)
    assert np.array_equal(plain[untouched], want[0][untouched]) and np.array_equal(m[untouched], want[1][untouched]) and dropped == st["n_entries_dropped"]
    return old, (rows, counts, st, short)


@pytest.mark.parametrize("bits,k", [(64, 1), (64, 10), (64, 100), (128, 10), (256, 1), (512, 10)])
def test_the_model_is_the_rule_under_a_random_removal(bits, k):
    codes = KG.clustered_case(bits, n=600)
    for fraction in (0.01, 0.1, 0.5):
        _, (_, _, st, _) = _check(codes, KR.random_keep(len(codes), fraction), k, what=(bits, k, fraction))
        assert st["n_entries_dropped"] > 0


def test_a_random_one_percent_at_k_10_leaves_short_and_untouched_rows():
    """the case of the GPU test's knob runs: 2000 clustered records, 1 % removed, k = 10; and the 10 % removal of its rows test"""
    codes = KG.clustered_case(64)
    for fraction in (0.01, 0.1):
        keep = KR.random_keep(len(codes), fraction)
        old, (rows, counts, st, short) = _check(codes, keep, 10, what=fraction)
        K = st["n_rows_kept"]
        assert K == len(codes) - round(fraction * len(codes))
        plain, m, _ = KR.translate(old[0], old[1], KR.retain_map(keep), 10)
        assert 0 < st["n_rows_short"] < K                                   # both short rows ...
        assert int((m == 10).sum()) == K - st["n_rows_short"] > 0           # ... and rows that needed nothing
        whole = (old[0][keep] != KG.INF).sum(axis=1) == m                   # rows none of whose entries died
        assert 0 < int(whole.sum()) < K and st["n_entries_dropped"] >= st["n_rows_short"]


def test_the_model_with_an_id_base():
    codes = KG.clustered_case(64, n=600)
    _check(codes, KR.random_keep(len(codes), 0.1), 7, id_base=2 ** 32 - 5000, what="id_base")


def test_the_crafted_patterns_reach_their_cases():
    codes, k = KR.crafted_codes(), KR.CRAFT_K
    pats = KR.crafted_patterns()
    got = {name: _check(codes, keep, k, what=name) for name, keep in pats.items()}
    dist = lambda a, b: bin(int.from_bytes(bytes(codes[a] ^ codes[b]), "little")).count("1")
    # a whole cluster removed: no lone row lists a member, so nothing is dropped and nothing is short
    st = got["cluster"][1][2]
    assert (st["n_rows_kept"], st["n_rows_short"], st["n_entries_dropped"]) == (KR.CRAFT_LONE, 0, 0)
    # the tie: the row's last entry is the removed record, the record behind it ties at that distance with a larger id and moves in
    old, (rows, counts, st, short) = got["tie"]
    r, win, lose = KR.TIE_ROW, KR.TIE_WINNER, KR.TIE_LOSER
    assert int(old[0][r, k - 1]) == (dist(r, win) << 32) | win and dist(r, lose) == dist(r, win) and lose > win and not pats["tie"][win]
    assert lose not in (old[0][r] & np.uint64(0xFFFFFFFF)).tolist()
    new_r, new_lose = r - 1, lose - 1                                      # one record below them was removed
    assert new_r in short.tolist() and int(rows[new_r, k - 1]) == (dist(r, lose) << 32) | new_lose
    assert st["n_rows_short"] == st["n_entries_dropped"] >= KR.CRAFT_CLUSTER - 1   # every other member listed the winner, and every row was full
    # the ends of the map
    for name, dead in (("first", 0), ("last", KR.CRAFT_N - 1)):
        st = got[name][1][2]
        listed = int(((got[name][0][0] & np.uint64(0xFFFFFFFF)) == np.uint64(dead)).any(axis=1).sum())   # the rows that list the removed record
        assert st["n_rows_kept"] == KR.CRAFT_N - 1 and st["n_entries_dropped"] == st["n_rows_short"] == listed
    assert got["first"][1][2]["n_rows_short"] > 0
    st = got["alternate"][1][2]
    assert st["n_rows_kept"] == KR.CRAFT_N // 2 and st["n_rows_short"] > KR.CRAFT_CLUSTER // 2


@pytest.mark.parametrize("K", [1, 2, KR.CRAFT_K, KR.CRAFT_K + 1, KR.CRAFT_K + 2])
def test_small_stores(K):
    """K in {1, 2, k, k + 1, k + 2} out of 20 records: at K - 1 <= k every surviving row ends up holding the whole new store"""
    codes, k = KR.crafted_codes()[30:50], KR.CRAFT_K
    keep = np.zeros(len(codes), dtype=bool)
    keep[np.random.default_rng(K).choice(len(codes), size=K, replace=False)] = True
    _, (rows, counts, st, _) = _check(codes, keep, k, what=K)
    assert np.all(counts == min(k, K - 1)) and st["n_rows_kept"] == K
    if K == 1:
        assert np.all(rows == KG.INF) and st["n_rows_short"] == 0


def test_rows_that_held_the_whole_store_lose_entries_without_becoming_short():
    """n_old - 1 < k: every old row lists every other record; after a removal it lists every other survivor, so it lost entries, is
    not short and is not searched"""
    codes, k = KR.crafted_codes()[30:35], KR.CRAFT_K
    assert len(codes) - 1 < k
    keep = np.array([1, 0, 1, 1, 0], dtype=bool)
    old, (rows, counts, st, short) = _check(codes, keep, k, what="whole store")
    assert np.all(old[1] == 4) and len(short) == 0 and st == dict(n_rows_kept=3, n_rows_short=0, n_entries_dropped=6)
    assert np.all(counts == 2) and KR.repair_stats(codes, keep, short, k) == KG.zero_graph_stats()
    # nothing removed: nothing dropped, nothing short
    _, (_, _, st, _) = _check(codes, np.ones(5, dtype=bool), k)
    assert st == dict(n_rows_kept=5, n_rows_short=0, n_entries_dropped=0)


def test_the_dense_set_with_its_cluster_removed():
    codes, keep = KR.dense_cluster_keep()
    k = KU.DENSE_K
    removed = int((~keep).sum())
    assert 300 < removed < 600 and int(keep.sum()) > k + 1
    _, (_, _, st, _) = _check(codes, keep, k, what="dense")
    assert st["n_rows_short"] > 100 and st["n_entries_dropped"] > 1000
