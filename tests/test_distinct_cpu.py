"""One result per label group in k-NN search, without a GPU: the ABI surface, the code object of the kernels, the plan arithmetic under
the sanitizers, and the expectation of test_distinct_gpu.py -- that the two formulations of the numpy model agree with each other and
with plain loops, and that the crafted cases reach what they are there for."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import distinct_common as DC
import groups_common as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vc_search_knn_distinct", "vc_search_knn_distinct_dev", "vc_sharded_search_knn_distinct", "vc_sharded_search_knn_distinct_dev"]


def test_header_declares_and_library_exports_the_new_names(vc):
    txt = open(os.path.join(ROOT, "include", "verticut_gpu.h")).read()
    assert re.search(r"#define\s+VC_ABI_VERSION\s+2\b", txt)             # entry points are only added
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"#define\s+VC_DISTINCT_TRUNCATED\s+0x80000000u\b", code)
    assert re.search(r"typedef struct vc_distinct_stats\s*\{\s*uint32_t n_rounds;\s*uint32_t k_last;\s*uint64_t n_searched;\s*uint64_t n_truncated;"
                     r"\s*uint64_t n_short;\s*\}\s*vc_distinct_stats;", code)
    L = ctypes.CDLL(vc.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(L, name), name
        assert name in vc.EXPORTS
    for name in ("vc_search_knn_distinct_dev", "vc_sharded_search_knn_distinct_dev"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*const void\* d_queries,\s*uint32_t nq,\s*uint32_t k,\s*uint32_t mode,\s*const uint32_t\* d_labels,"
                         r"\s*uint32_t k_first,\s*uint64_t\* d_out,\s*uint32_t\* d_row_labels,\s*uint32_t\* d_counts,\s*vc_distinct_stats\* stats,"
                         r"\s*void\* stream\)" % name, code), name
    for name in ("vc_search_knn_distinct", "vc_sharded_search_knn_distinct"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*const void\* queries,\s*uint32_t nq,\s*uint32_t k,\s*uint32_t mode,\s*uint32_t order,"
                         r"\s*const uint32_t\* labels,\s*uint32_t k_first,\s*uint64_t\* out,\s*uint32_t\* row_labels,\s*uint32_t\* counts,"
                         r"\s*vc_distinct_stats\* stats\)" % name, code), name
    # what the header has to say
    flat = " ".join(txt.split())
    for phrase in ("the collapse of the row the underlying call returns at the final k'", "ONCE PER ROUND", "in VC_MODE_LINEAR too",
                   "should keep the labels in HBM and use the device form", "VC_MODE_MIH_APPROX is refused"):
        assert " ".join(phrase.split()) in flat.replace(" * ", " "), phrase
    assert vc.VC_ABI_VERSION == 2 and vc.DISTINCT_TRUNCATED == 0x80000000 == DC.TRUNCATED
    st = vc.VcDistinctStats
    assert ctypes.sizeof(st) == 32
    assert (st.n_rounds.offset, st.k_last.offset, st.n_searched.offset, st.n_truncated.offset, st.n_short.offset) == (0, 4, 8, 16, 24)
    assert set(st().as_dict()) == set(DC.zero_stats()) and st().as_dict() == DC.zero_stats()
    for cls in (vc.Engine, vc.ShardedEngine):
        for meth in ("search_knn_distinct", "search_knn_distinct_dev"):
            assert callable(getattr(cls, meth)), (cls, meth)
    host = open(os.path.join(ROOT, "verticut_amd", "host", "verticut_host.hpp")).read()
    assert re.search(r"virtual int search_knn_distinct\([^)]*\)\s*=\s*0;", host)
    assert len(re.findall(r"int search_knn_distinct\([^)]*\)\s*override", host)) == 2
    assert "return vc_search_knn_distinct(h_," in host and "return vc_sharded_search_knn_distinct(h_," in host
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "5.13" in design and "vc_search_knn_distinct" in design


def test_distinct_kernels_use_no_scratch(vc):
    """vc_distinct.o holds the wave form, the block form at both block sizes, the gather and the empty-store fill -- with no scratch
    and no spills; static LDS is the wave sums only (the labels and the table are dynamic)"""
    from verticut_amd import build as vb
    assert "vc_distinct.hip" in vb.SOURCES and "vc_distinct_plan.hpp" in vb.HEADERS
    res = vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_distinct.o"))
    once = ("vc_distinct_wave_kernel", "vc_distinct_gather_kernel", "vc_distinct_empty_kernel")
    for kernel in once:
        assert sum(kernel in name for name in res) == 1, (kernel, sorted(res))
    table = sorted(name for name in res if "vc_distinct_table_kernel" in name)
    assert len(table) == 2 and len(res) == len(once) + 2, sorted(res)
    for T in (256, 1024):
        assert sum("vc_distinct_table_kernelILi%dEE" % T in name for name in table) == 1, (T, table)
    for name, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["group_segment_fixed_size"] <= 64, (name, r)
    assert all(res[name]["group_segment_fixed_size"] == 0 for name in res if "table" not in name)
    text = open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_distinct.hip")).read()
    assert "getenv" not in text                                            # the knob is read in read_knobs, nowhere else
    engine = open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_engine.hip")).read()
    assert engine.count('getenv("VC_DISTINCT_SCRATCH")') == 1
    for word in ("hipLaunchCooperativeKernel", "__threadfence", "grid_group"):    # blocks meet in a later launch only
        assert word not in text, word


def test_plan_arithmetic_under_the_sanitizers(tmp_path):
    """tests/cpp/distinct_plan_test.cc over csrc/vc_distinct_plan.hpp, host code only, with AddressSanitizer and UBSan; the size classes
    the crafted cases are laid out against are the plan's"""
    src = os.path.join(ROOT, "tests", "cpp", "distinct_plan_test.cc")
    exe = tmp_path / "distinct_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           src, "-I", os.path.join(ROOT, "verticut_amd", "csrc")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert out.stdout.startswith("distinct plan ok:")
    for key, val in (("WAVE", DC.WAVE_MAX), ("BLOCK", DC.BLOCK_MAX), ("MAXK", DC.MAX_K)):
        assert re.search(r"^%s %d$" % (key, val), out.stdout, flags=re.M), out.stdout


# ---- the expectation ------------------------------------------------------------------------------------------------------------------
def _agree(lists, labels, k, id_base=0, what=None):
    """both formulations under every k_first; returns the protocol runs by k_first"""
    heads = DC.heads_model(lists, labels, k, id_base)
    runs = {}
    for k_first in DC.K_FIRSTS(k):
        for tie_cut in (True, False):                                     # exact MIH underneath, then the linear scan: the same rows
            run = DC.protocol_model(lists, labels, k, k_first, id_base, tie_cut)
            DC.same_run(run[:3], heads[:3], (what, k, k_first, tie_cut))
            assert (run[3]["n_truncated"], run[3]["n_short"]) == heads[3:], (what, k, k_first, tie_cut)
            assert run[3]["n_searched"] == sum(n for _, n, _ in run[4]) and run[3]["n_rounds"] == len(run[4])
            if tie_cut:
                cut = run
        runs[k_first] = run
        assert cut[3]["n_rounds"] >= run[3]["n_rounds"] and cut[3]["n_searched"] >= run[3]["n_searched"]      # the sure prefix is never longer
    return runs


@pytest.mark.parametrize("seed", range(8))
def test_the_model_is_the_rule(seed):
    """against plain loops, on small random inputs with few distinct codes and labels (so that ties and short rows are common)"""
    rng = np.random.default_rng(seed)
    bits = 64 if seed % 2 else 128
    n, nq = int(rng.integers(1, 80)), 6
    k = int(rng.integers(1, 12))
    id_base = int(rng.integers(1, 1000)) if seed % 3 else 0
    codes = np.zeros((n, bits // 8), np.uint8)
    codes[:, :2] = rng.integers(0, 4, size=(n, 2), dtype=np.uint8)
    queries = codes[rng.integers(0, n, size=nq)]
    labels = rng.integers(0, max(2, n // 3), size=n).astype(np.uint32) * np.uint32(0x01010101)
    lists = DC.sorted_lists(codes, queries, id_base)
    for L in lists:
        assert len(L) == n and np.all(np.diff(L.astype(np.int64)) > 0)
    runs = _agree(lists, labels, k, id_base, seed)
    for k_first, (rows, rls, counts, st, trace) in runs.items():
        for tie_cut in (False, True):
            n_rounds = 0
            for i, L in enumerate(lists):
                labs = DC.labels_of(L, labels, id_base)
                kp, mine = DC.first_k(k, k_first), 1
                while True:
                    kept, kl, cnt = DC.walk(L, labs, kp, k, tie_cut)
                    if len(kept) >= k or cnt < kp or kp >= DC.MAX_K:
                        break
                    kp, mine = min(DC.MAX_K, 2 * kp), mine + 1
                w = min(len(kept), k)
                assert counts[i] == w and list(rows[i, :w]) == kept[:w] and list(rls[i, :w]) == kl[:w], (seed, k_first, i, tie_cut)
                assert np.all(rows[i, w:] == DC.INF) and np.all(rls[i, w:] == 0)
                n_rounds = max(n_rounds, mine)
            assert n_rounds == DC.protocol_model(lists, labels, k, k_first, id_base, tie_cut)[3]["n_rounds"], (seed, k_first, tie_cut)


def test_the_model_on_nothing():
    got = DC.protocol_model([np.zeros(0, np.uint64)] * 3, np.zeros(0, np.uint32), 4)
    assert np.all(got[0] == DC.INF) and got[0].shape == (3, 4) and np.all(got[1] == 0) and np.all(got[2] == 0) and got[3] == DC.zero_stats()


# ---- reach: each crafted case does what it is for, on the model alone ------------------------------------------------------------------
@pytest.mark.parametrize("bits", [64, 128, 256, 512])
def test_duplicate_heavy_case(bits):
    """257 queries; with k = 10 some finish in round 0 and some need exactly 1, 2, 3 and 4 more; hostile values change no row position"""
    codes, labels, queries = DC.dup_case(bits)
    assert len(queries) == 257 and len(codes) <= 9000 and codes.shape[1] == bits // 8
    sizes = np.unique(labels, return_counts=True)[1]
    assert sizes.min() == 1 and sizes.max() == 40
    if bits > 128:                                                        # (one GPU case each: the protocol run is all that is needed)
        run = DC.dup_expect(bits)
    else:
        run = _agree(DC.dup_lists(bits), labels, DC.DUP_K, 0, bits)[0]
        assert all(np.array_equal(a, b) for a, b in zip(run[:3], DC.dup_expect(bits)[:3]))
    rounds = DC.rounds_of(run[4], 257)
    assert set(rounds.tolist()) == {1, 2, 3, 4, 5} and run[3]["n_rounds"] == 5 and run[3]["k_last"] == 320
    assert run[3]["n_short"] == 0 and run[3]["n_truncated"] == 0 and np.all(run[2] == DC.DUP_K)
    again = run[4][0][2]                                                  # the retry list of round 0 is no prefix and no suffix of the batch
    assert 0 < len(again) < 257 and sorted(again) != list(range(len(again))) and sorted(again) != list(range(257 - len(again), 257))
    if bits == 64:
        hostile = DC.hostile_labels(labels)
        assert len(np.unique(hostile)) == len(np.unique(labels)) and {0, 0xFFFFFFFF, 0xFFFFFFFE} <= set(hostile.tolist())
        assert np.array_equal(np.unique(labels, return_inverse=True)[1].reshape(-1) == 0, hostile == hostile[labels == labels.min()][0])
        h = DC.dup_expect(bits, DC.DUP_K, 0, 0, True)
        assert np.array_equal(h[0], run[0]) and np.array_equal(h[2], run[2]) and h[3] == run[3]
        values = np.unique(hostile)
        assert np.count_nonzero((values & np.uint32(0xFFFF)) == 0xBEEF) > 1000 and np.count_nonzero((values >> np.uint32(4)) == 0x1234567) == 16


def test_size_class_edges_are_hit():
    """k = 32 over the duplicate-heavy store: k_first 64 | 65 puts the first round on either side of the wave form's edge, 1024 | 1025
    on either side of the block form's; the rounds behind 64 and 65 run in the block form; 8192 is the widest table"""
    bits, k = 64, 32
    labels = DC.dup_case(bits)[1]
    classes = {}
    for k_first in (64, 65, 1024, 1025, 8192):
        run = DC.dup_expect(bits, k, k_first)
        classes[k_first] = [DC.size_class(kp) for kp, _, _ in run[4]]
        assert np.all(run[2] == k)
        assert all(np.array_equal(a, b) for a, b in zip(run[:3], DC.heads_model(DC.dup_lists(bits), labels, k)[:3]))
    assert classes[64][0] == 0 and classes[65][0] == 1 and len(classes[64]) > 1 and set(classes[64][1:]) == {1}
    assert classes[1024] == [1] and classes[1025] == [2] and classes[8192] == [2]
    assert len(DC.dup_case(bits)[0]) > 1025                              # the rows of k' = 1025 are full
    assert [DC.size_class(kp) for kp in (1, 64, 65, 1024, 1025, 8192)] == [0, 0, 1, 1, 2, 2]


def test_truncation_case():
    codes, labels, queries = DC.truncation_case()
    assert len(codes) == 9000 and np.count_nonzero(labels == 5) == 8600 and len(np.unique(labels)) == 401
    lists = DC.truncation_lists()
    for L in lists:                                                       # the 8192 nearest records all carry the one label
        assert np.all(DC.labels_of(L[:DC.MAX_K], labels, 0) == 5) and int(L[8599] >> np.uint64(32)) <= 3 < int(L[8600] >> np.uint64(32))
    runs = _agree(lists, labels, 2, 0, "truncation")
    for run in runs.values():
        assert np.all(run[2] == (1 | DC.TRUNCATED)) and run[3]["n_truncated"] == 3 and run[3]["n_short"] == 0 and run[3]["k_last"] == DC.MAX_K
    assert runs[0][3]["n_rounds"] == 12 and runs[8192][3]["n_rounds"] == 1
    for run in _agree(lists, labels, 1, 0, "k = 1").values():
        assert np.all(run[2] == 1) and run[3]["n_truncated"] == 0 and run[3]["n_rounds"] == 1


def test_one_group_case():
    codes = GC.uniform_codes(300, 64, 21)
    lists = DC.sorted_lists(codes, codes[:5] ^ np.uint8(1))
    runs = _agree(lists, np.full(300, 7, dtype=np.uint32), 4, 0, "one group")
    assert runs[0][3] == {"n_rounds": 7, "k_last": 512, "n_searched": 35, "n_truncated": 0, "n_short": 5}
    assert np.all(runs[0][2] == 1) and np.all(runs[0][1][:, 0] == 7) and np.all(runs[0][0][:, 1:] == DC.INF)


@pytest.mark.parametrize("bits", [64, 128])
def test_ties_case(bits):
    codes, labels, queries = DC.ties_case(bits)
    lists = DC.sorted_lists(codes, queries, 50)
    dist = lists[0] >> np.uint64(32)
    assert np.count_nonzero(dist == 0) == 16 and np.count_nonzero(dist == 1) == 64 and np.count_nonzero(dist == 2) == 200
    labs = DC.labels_of(lists[0], labels, 50)
    assert len(set(labs[dist == 1].tolist())) == 5 and len(set(labs[dist == 0].tolist())) == 2
    for k in (3, 8, 14):
        runs = _agree(lists, labels, k, 50, ("ties", k))
        rows, rls = runs[0][0], runs[0][1]
        assert len(np.unique(labels)) == 14 and np.all(runs[0][2] == min(k, 14))
        d0 = rows[0, :min(k, 14)] >> np.uint64(32)
        assert np.all(np.diff(rows[0, :min(k, 14)].astype(np.int64)) > 0)                # heads at equal distance: in id order
        assert list(d0[:2]) == [0, 0] and (k < 8 or list(d0[2:7]) == [1] * 5)
        for j in range(min(k, 14)):                                       # a head is its group's smallest (dist, id)
            assert rows[0, j] == lists[0][labs == rls[0, j]].min()
