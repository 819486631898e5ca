"""vc_knn_graph_update* without a GPU: the ABI surface, the code object of the kernels, the plan arithmetic under the sanitizers, and
the expectation of test_knn_graph_update_gpu.py -- that the windowed numpy model equals knn_graph_common.model_rows over the whole
store for every window, and that the crafted inputs reach what they are there for."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import knn_graph_common as KG
import knn_graph_update_common as KU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_new_names(vc):
    txt = open(os.path.join(ROOT, "include", "verticut_gpu.h")).read()
    assert re.search(r"#define\s+VC_ABI_VERSION\s+2\b", txt)             # entry points are only added
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"typedef struct vc_knn_graph_update_stats\s*\{\s*vc_knn_graph_stats build;\s*uint64_t n_rows_changed;\s*uint64_t n_inserted;"
                     r"\s*uint64_t n_hits;\s*uint32_t n_windows;\s*uint32_t n_halvings;\s*\}\s*vc_knn_graph_update_stats;", code)
    L = ctypes.CDLL(vc.LIB_PATH)
    for name in KU.UPDATE_NAMES:
        assert hasattr(L, name), name
        assert name in vc.EXPORTS
    for name in ("vc_knn_graph_update_dev", "vc_sharded_knn_graph_update_dev"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*uint32_t k,\s*uint32_t mode,\s*uint32_t batch,\s*uint64_t n_old,\s*uint32_t k_first,"
                         r"\s*uint64_t\* d_rows,\s*uint32_t\* d_counts,\s*vc_knn_graph_update_stats\* stats,\s*void\* stream\)" % name, code), name
    for name in ("vc_knn_graph_update", "vc_sharded_knn_graph_update"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*uint32_t k,\s*uint32_t mode,\s*uint32_t batch,\s*uint64_t n_old,\s*uint32_t k_first,"
                         r"\s*uint64_t\* rows,\s*uint32_t\* counts,\s*vc_knn_graph_update_stats\* stats\)" % name, code), name
    flat = " ".join(txt.split()).replace(" * ", " ")
    for phrase in ("The first n_old rows and counts are what vc_knn_graph* wrote when the store held exactly its first n_old records",
                   "every old row then holds min(k, n_old - 1) entries, and no counts are written", "the caller has run vc_update_index",
                   "THE SAME WORDS as vc_knn_graph*(first = 0, count = N)", "the join below has no mode", "n_old == N: VC_OK, nothing written, zero stats",
                   "n_old == 0: a plain build", "a stale index after vc_add_codes counts as none", "THE OUTPUTS ARE THEN UNDEFINED",
                   "VC_KGRAPH_OLD_BATCH", "VC_KGRAPH_WINDOW", "Not offered: a form for vc_retain*"):
        assert " ".join(phrase.split()) in flat, phrase
    assert vc.VC_ABI_VERSION == 2
    st = vc.VcKnnGraphUpdateStats
    assert ctypes.sizeof(st) == 64 and st.build.offset == 0 and [getattr(st, n).offset for n in KU.UPDATE_STATS] == [32, 40, 48, 56, 60]
    assert st().as_dict() == KU.zero_update_stats()
    for cls in (vc.Engine, vc.ShardedEngine):
        for meth in ("knn_graph_update", "knn_graph_update_dev"):
            assert callable(getattr(cls, meth)), (cls, meth)
    host = open(os.path.join(ROOT, "verticut_amd", "host", "verticut_host.hpp")).read()
    assert re.search(r"virtual int knn_graph_update\([^)]*\)\s*=\s*0;", host)
    assert len(re.findall(r"int knn_graph_update\([^)]*\)\s*override", host)) == 2
    assert "return vc_knn_graph_update(h_," in host and "return vc_sharded_knn_graph_update(h_," in host
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "5.17" in design and "vc_knn_graph_update" in design and "vc_retain" in design
    for doc in ("README.md", "INTEGRATION.md"):
        assert "vc_knn_graph_update" in open(os.path.join(ROOT, doc)).read(), doc
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_knn_graph_update.py"))


def test_update_kernels_use_no_scratch_and_the_join_16_kib_of_lds(vc):
    """every kernel of vc_knn_graph_update.o has no scratch memory and no spills; the join kernel holds its tile in 16 KiB of LDS and
    nothing else does; the knobs are read in read_knobs only"""
    from verticut_amd import build as vb
    assert "vc_knn_graph_update.hip" in vb.SOURCES and "vc_knn_graph_update_plan.hpp" in vb.HEADERS
    res = vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_knn_graph_update.o"))
    joins = [name for name in res if "vc_kgraph_join_kernel" in name]
    assert len(joins) == 8, sorted(res)                                      # four widths, count and fill
    for kernel in ("vc_kgraph_list_kernel", "vc_kgraph_merge_kernel", "vc_kgraph_copy_kernel", "vc_kgraph_marks_kernel", "vc_kgraph_inserted_kernel"):
        assert sum(kernel in name for name in res) == 1, (kernel, sorted(res))
    assert len(res) == 13, sorted(res)
    for name, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == (8 * KU.LDS_WORDS if name in joins else 0) <= 16384, (name, r)
    csrc = os.path.join(ROOT, "verticut_amd", "csrc")
    for name in ("vc_knn_graph_update.hip", "vc_knn_graph_update_plan.hpp"):
        text = open(os.path.join(csrc, name)).read()
        assert "getenv" not in text, name
        for word in ("hipLaunchCooperativeKernel", "__threadfence", "grid_group"):
            assert word not in text, (name, word)
    engine = open(os.path.join(csrc, "vc_engine.hip")).read()
    knobs = engine[engine.index("void read_knobs("):]
    knobs = knobs[:knobs.index("\n}\n")]
    for knob in ("VC_KGRAPH_SCRATCH", "VC_KGRAPH_OLD_BATCH", "VC_KGRAPH_WINDOW"):
        assert engine.count('getenv("%s")' % knob) == 1 and knobs.count('getenv("%s")' % knob) == 1, knob
    for name in os.listdir(csrc):
        if name != "vc_engine.hip":
            assert "VC_KGRAPH_WINDOW\")" not in open(os.path.join(csrc, name)).read(), name


def test_plan_arithmetic_under_the_sanitizers(tmp_path):
    """tests/cpp/knn_graph_update_plan_test.cc over csrc/vc_knn_graph_update_plan.hpp, host code only, with AddressSanitizer and UBSan;
    the constants and the planned cases it prints are those of the model's mirror"""
    src = os.path.join(ROOT, "tests", "cpp", "knn_graph_update_plan_test.cc")
    exe = tmp_path / "knn_graph_update_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           src, "-I", os.path.join(ROOT, "verticut_amd", "csrc")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert out.stdout.startswith("knn graph update plan ok: OLD_BATCH %d WINDOW %d LDS %d BLOCK %d\n"
                                 % (KU.OLD_BATCH_DEFAULT, KU.WINDOW_DEFAULT, KU.LDS_WORDS, KU.BLOCK))
    for W in (1, 2, 4, 8):
        assert re.search(r"^MAP %d %d %d %d$" % (W, KU.records(W), KU.blocks(9000, W), KU.LDS_WORDS // W), out.stdout, flags=re.M), (W, out.stdout)
    for nb in (1, 2000, 1 << 18):
        assert re.search(r"^WORK %d %d$" % (nb, KU.work_total(nb, 200, 2, 33)), out.stdout, flags=re.M), (nb, out.stdout)
    assert re.search(r"^SUB %d %d$" % (KU.merge_sub(4096, 100), KU.merge_bytes(1000, 4096, 100)), out.stdout, flags=re.M)
    assert KU.old_batch(0) == 1 << 18 and KU.old_batch(100) == 100 and KU.old_batch((1 << 24) + 1) == 1 << 18
    assert KU.window(0) == 1024 and KU.window(1) == 1 and KU.window((1 << 20) + 1) == 1024
    assert KU.accept(512, 4096, 7) and not KU.accept(513, 4096, 7) and KU.accept(513, 4096, 1) and not KU.accept(1 << 32, 1 << 60, 2)
    assert [KU.halve(x) for x in (1, 2, 3, 64, 1024)] == [1, 1, 1, 32, 512]


# ---- the expectation ------------------------------------------------------------------------------------------------------------------
SHAPES = [(64, 10), (64, 100), (128, 1), (256, 10)]


@pytest.mark.parametrize("window", [1, 3, 64, 4096])
@pytest.mark.parametrize("bits,k", SHAPES)
def test_the_windowed_model_is_the_rule(bits, k, window):
    """old rows carried through the window loop equal model_rows over the whole store; n_rows_changed and n_inserted are what a
    comparison of the two graphs says"""
    codes, n_old = KU.planted_case(bits, n=600, planted=70)
    want = KG.model_rows(codes, k)
    old = KG.model_rows(codes[:n_old], k)
    for ob in (0, 250):
        rows, counts, st = KU.update_model(codes, n_old, k, window_knob=window, old_batch_knob=ob, old=old)
        KG.same_graph((rows, counts), want, (bits, k, window, ob))
        assert st["n_rows_changed"] == KU.changed_rows(old[0], want[0]) > 0
        new_id = (want[0][:n_old] & np.uint64(0xFFFFFFFF)) >= np.uint64(n_old)
        assert st["n_inserted"] == int((new_id & (want[0][:n_old] != KG.INF)).sum()) > 0
        n_batches = 1 if ob == 0 else -(-n_old // ob)
        assert st["n_halvings"] == 0 and st["n_windows"] == n_batches * -(-(len(codes) - n_old) // window)
        assert st["n_hits"] >= st["n_inserted"]                             # a hit may be pushed out again by a later window


def test_the_model_with_an_id_base_and_a_chain_of_appends():
    codes, _ = KU.planted_case(64, n=600, planted=70)
    k, id_base, n = 7, 2 ** 32 - 5000, 500
    got = KG.model_rows(codes[:n], k, id_base)
    for step in (1, 7, 100, 62):
        rows, counts, _ = KU.update_model(codes[:n + step], n, k, id_base, window_knob=16, old=got)
        n += step
        KG.same_graph((rows, counts), KG.model_rows(codes[:n], k, id_base), ("chain", n))
        got = (rows, counts)


def test_random_clustered_records_alone_change_nothing_at_128_bits():
    """why the appended records are planted: three more records of the clustered case change no old row"""
    base = KG.clustered_case(128)
    rng = np.random.default_rng(99)
    far = rng.integers(0, 256, size=(3, 16), dtype=np.uint8)
    codes = np.concatenate([base, far])
    _, _, st = KU.update_model(codes, len(base), 10)
    assert st["n_rows_changed"] == 0 and st["n_inserted"] == 0 and st["n_hits"] == 0 and st["n_windows"] == 1
    for bits in (64, 128, 256, 512):
        codes, n_old = KU.planted_case(bits)
        assert len(codes) == n_old + KU.PLANTED
        assert KU.update_model(codes, n_old, 10, window_knob=64)[2]["n_rows_changed"] > KU.PLANTED // 2, bits


# ---- reach: the crafted inputs do what they are for ----------------------------------------------------------------------------------------
def test_the_crafted_set_reaches_every_case():
    codes, n_old, replaced, tie = KU.crafted_case()
    k = KU.CRAFT_K
    old = KG.model_rows(codes[:n_old], k)
    want = KG.model_rows(codes, k)
    for window in (1, 3, 64):
        rows, counts, st = KU.update_model(codes, n_old, k, window_knob=window, old=old)
        KG.same_graph((rows, counts), want, ("crafted", window))
    dist = lambda a, b: bin(int.from_bytes(bytes(codes[a] ^ codes[b]), "little")).count("1")
    # more than k hits in one window, and a row replaced entirely: the 8 duplicates of the lone record
    new_ids = np.arange(n_old, len(codes))
    hits = [j for j in new_ids if ((dist(replaced, j) << 32) | j) < int(old[0][replaced, k - 1])]
    assert len(hits) == KU.CRAFT_DUPS > k and max(hits) - min(hits) < 64
    assert not set(old[0][replaced].tolist()) & set(want[0][replaced].tolist())
    assert np.array_equal(want[0][replaced], np.arange(n_old, n_old + k).astype(np.uint64))           # at distance 0, the smallest new ids
    # a new record that ties a row's last distance and loses on its id
    members = range(KU.CRAFT_LONE, n_old)
    tied = [i for i in members if dist(i, tie) == int(old[0][i, k - 1] >> np.uint64(32)) and old[1][i] == k]
    assert len(tied) == KU.CRAFT_CLUSTER and all(tie not in (want[0][i] & np.uint64(0xFFFFFFFF)).tolist() for i in tied)
    # exact duplicates of old records, and rows with no hit
    assert sum(1 for j in new_ids for i in range(n_old) if dist(i, j) == 0) >= KU.CRAFT_DUPS + 2
    unchanged = [i for i in range(n_old) if np.array_equal(old[0][i], want[0][i])]
    assert unchanged and len(unchanged) < n_old and st["n_rows_changed"] == n_old - len(unchanged)


@pytest.mark.parametrize("n_old", [0, 1, 2, KU.CRAFT_K, KU.CRAFT_K + 1])
def test_rows_that_are_not_full(n_old):
    """n_old <= k: no old row is full, every new record is a hit of every old row until the row fills"""
    codes, _, _, _ = KU.crafted_case()
    codes, k = codes[30:50], KU.CRAFT_K
    old = KG.model_rows(codes[:n_old], k)
    assert n_old > k or np.all(old[1] < k)
    for window in (1, 3, 64):
        rows, counts, st = KU.update_model(codes, n_old, k, window_knob=window, old=old)
        KG.same_graph((rows, counts), KG.model_rows(codes, k), (n_old, window))
        if 0 < n_old <= k:
            assert st["n_rows_changed"] == n_old and st["n_hits"] >= n_old * (k - (n_old - 1))


def test_the_dense_set_forces_halvings():
    codes, n_old = KU.dense_case()
    k = KU.DENSE_K
    old = KG.model_rows(codes[:n_old], k)
    want = KG.model_rows(codes, k)
    rows, counts, tight = KU.update_model(codes, n_old, k, window_knob=KU.DENSE_WINDOW, budget=KU.DENSE_BUDGET, old=old)
    KG.same_graph((rows, counts), want, "dense, tight budget")
    rows, counts, loose = KU.update_model(codes, n_old, k, window_knob=KU.DENSE_WINDOW, old=old)
    KG.same_graph((rows, counts), want, "dense")
    assert tight["n_halvings"] >= 2 and loose["n_halvings"] == 0 and loose["n_windows"] == 1 < tight["n_windows"]
    assert tight["n_rows_changed"] == loose["n_rows_changed"] > 100 and tight["n_inserted"] == loose["n_inserted"]
    assert tight["n_hits"] <= loose["n_hits"]                               # thresholds tighten from window to window
    assert 8 * loose["n_hits"] > KU.DENSE_BUDGET
