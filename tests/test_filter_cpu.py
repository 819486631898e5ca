"""Filtered k-NN without a GPU: the ABI surface, the code object of the kernels, the plan arithmetic under the sanitizers, and the
expectation of test_filter_gpu.py -- that the numpy model agrees with plain loops, that a finished post-filter row is the brute
force, and that the crafted cases reach what they are there for."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import distinct_common as DC
import filter_common as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vc_search_knn_filtered", "vc_search_knn_filtered_dev", "vc_sharded_search_knn_filtered", "vc_sharded_search_knn_filtered_dev"]


def test_header_declares_and_library_exports_the_new_names(vc):
    txt = open(os.path.join(ROOT, "include", "verticut_gpu.h")).read()
    assert re.search(r"#define\s+VC_ABI_VERSION\s+2\b", txt)             # entry points are only added
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, val in (("MASK", 0), ("ROOTS", 1), ("EQUAL", 2), ("NOT_EQUAL", 3), ("BITS", 4), ("RAN_POST", 1), ("RAN_PRE", 2)):
        assert re.search(r"#define\s+VC_FILTER_%s\s+%du\b" % (name, val), code), name
        assert getattr(vc, "FILTER_" + name) == val == getattr(FC, name)
    assert re.search(r"typedef struct vc_filter_stats\s*\{\s*uint64_t n_allowed;\s*uint32_t routes;\s*uint32_t n_rounds;\s*uint32_t k_last;\s*uint32_t n_windows;"
                     r"\s*uint64_t n_searched;\s*uint64_t n_fallback;\s*uint64_t n_short;\s*\}\s*vc_filter_stats;", code)
    L = ctypes.CDLL(vc.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in vc.EXPORTS
    for name in ("vc_search_knn_filtered_dev", "vc_sharded_search_knn_filtered_dev"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*const void\* d_queries,\s*uint32_t nq,\s*uint32_t k,\s*uint32_t mode,\s*const uint32_t\* d_sel,"
                         r"\s*uint32_t kind,\s*uint32_t value,\s*uint32_t k_first,\s*uint64_t\* d_out,\s*uint32_t\* d_counts,\s*vc_filter_stats\* stats,"
                         r"\s*void\* stream\)" % name, code), name
    for name in ("vc_search_knn_filtered", "vc_sharded_search_knn_filtered"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*const void\* queries,\s*uint32_t nq,\s*uint32_t k,\s*uint32_t mode,\s*uint32_t order,"
                         r"\s*const uint32_t\* sel,\s*uint32_t kind,\s*uint32_t value,\s*uint32_t k_first,\s*uint64_t\* out,\s*uint32_t\* counts,"
                         r"\s*vc_filter_stats\* stats\)" % name, code), name
    flat = " ".join(txt.split()).replace(" * ", " ")
    for phrase in ("a filter per query is out of scope", "should keep sel in HBM, preferably as VC_FILTER_BITS", "There is no truncation flag",
                   "VC_MODE_MIH_APPROX is refused", "the bits of the last word past N are ignored"):
        assert " ".join(phrase.split()) in flat, phrase
    assert vc.VC_ABI_VERSION == 2
    st = vc.VcFilterStats
    assert ctypes.sizeof(st) == 48
    assert [getattr(st, n).offset for n in FC.STAT_NAMES] == [0, 8, 12, 16, 20, 24, 32, 40]
    assert st().as_dict() == FC.zero_stats()
    for cls in (vc.Engine, vc.ShardedEngine):
        for meth in ("search_knn_filtered", "search_knn_filtered_dev"):
            assert callable(getattr(cls, meth)), (cls, meth)
    host = open(os.path.join(ROOT, "verticut_amd", "host", "verticut_host.hpp")).read()
    assert re.search(r"virtual int search_knn_filtered\([^)]*\)\s*=\s*0;", host)
    assert len(re.findall(r"int search_knn_filtered\([^)]*\)\s*override", host)) == 2
    assert "return vc_search_knn_filtered(h_," in host and "return vc_sharded_search_knn_filtered(h_," in host
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "5.14" in design and "vc_search_knn_filtered" in design
    assert "vc_search_knn_filtered" in open(os.path.join(ROOT, "README.md")).read()


def test_filter_kernels_use_no_scratch(vc):
    """every kernel of vc_filter.o, the three walks at each of the four code widths among them, has no scratch and no spills"""
    from verticut_amd import build as vb
    assert "vc_filter.hip" in vb.SOURCES and "vc_filter_plan.hpp" in vb.HEADERS
    res = vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_filter.o"))
    for kernel in ("vc_filter_bits_kernel", "vc_filter_strip_kernel", "vc_filter_gather_kernel", "vc_filter_emit_kernel", "vc_filter_list_kernel",
                   "vc_filter_cut_kernel", "vc_filter_base_kernel"):
        assert sum(kernel in name for name in res) == 1, (kernel, sorted(res))
    for walk in ("vc_filter_hist_kernel", "vc_filter_count_kernel", "vc_filter_place_kernel"):
        for W in (1, 2, 4, 8):
            assert sum("%sILi%dEE" % (walk, W) in name for name in res) == 1, (walk, W, sorted(res))
    assert len(res) == 7 + 12, sorted(res)
    for name, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["group_segment_fixed_size"] <= 2048, (name, r)              # the query tile and its thresholds; the histograms are dynamic
    text = open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_filter.hip")).read()
    assert "getenv" not in text                                              # the knobs are read in read_knobs, nowhere else
    engine = open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_engine.hip")).read()
    for knob in ("VC_FILTER_ROUTE", "VC_FILTER_SCRATCH", "VC_FILTER_WINDOW"):
        assert engine.count('getenv("%s")' % knob) == 1, knob
    code = re.sub(r"//[^\n]*", "", text)
    for word in ("hipLaunchCooperativeKernel", "__threadfence", "grid_group"):      # blocks meet in a later launch only
        assert word not in code, word


def test_plan_arithmetic_under_the_sanitizers(tmp_path):
    """tests/cpp/filter_plan_test.cc over csrc/vc_filter_plan.hpp, host code only, with AddressSanitizer and UBSan; the constants the
    model and the crafted cases are laid out against are the plan's"""
    src = os.path.join(ROOT, "tests", "cpp", "filter_plan_test.cc")
    exe = tmp_path / "filter_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           src, "-I", os.path.join(ROOT, "verticut_amd", "csrc")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert out.stdout.startswith("filter plan ok:")
    for key, val in (("MAXK", FC.MAX_K), ("POSTMAXK", FC.POST_MAX_K), ("WINDOW", FC.WINDOW), ("SCRATCH", FC.SCRATCH)):
        assert re.search(r"^%s %d$" % (key, val), out.stdout, flags=re.M), (key, out.stdout)
    for W in (1, 2, 4, 8):
        assert re.search(r"^SLICE %d %d$" % (W, FC.slice_len(W)), out.stdout, flags=re.M), out.stdout


# ---- the expectation ------------------------------------------------------------------------------------------------------------------
def _finished_rows(lists, allowed, k, k_first, tie_cut, id_base=0):
    """the rows the post-filter rounds finish, from the round protocol itself: {query: row}; the others fall back"""
    done = {}
    N, A = len(allowed), int(np.count_nonzero(allowed))
    todo, kp = list(range(len(lists))), FC.first_k(k, k_first, N, A)
    while todo:
        again = []
        for i in todo:
            L = lists[i]
            cnt = min(kp, len(L))
            head = L[:FC.sure_entries(L, kp, tie_cut)]
            kept = head[allowed[((head & np.uint64(0xFFFFFFFF)) - np.uint64(id_base)).astype(np.int64)]]
            if len(kept) >= k or cnt < kp:
                done[i] = kept[:k]
            else:
                again.append(i)
        if kp >= FC.MAX_K:
            break
        todo, kp = again, min(FC.MAX_K, 2 * kp)
    return done


@pytest.mark.parametrize("seed", range(8))
def test_the_model_is_the_rule(seed):
    """against plain loops, on small random inputs with few distinct codes, so that ties are common; every kind means the same set;
    a row the post-filter rounds finish is the brute force, with and without the tie cut, for every k_first"""
    rng = np.random.default_rng(seed)
    nbytes, n, id_base = 8, int(rng.integers(1, 90)), int(rng.integers(0, 50))
    pool = rng.integers(0, 256, size=(4, nbytes), dtype=np.uint8)
    codes = pool[rng.integers(0, 4, size=n)]
    queries = pool[rng.integers(0, 4, size=5)] ^ np.uint8(1)
    allowed = rng.integers(0, 3, size=n) != 0 if seed % 4 else np.zeros(n, dtype=bool)
    lists = DC.sorted_lists(codes, queries, id_base)
    for kind in range(5):
        sel = FC.sel_for(allowed, kind, id_base, value=0xFFFFFFFF, junk=0xFFFFFFFF)
        assert np.array_equal(FC.allowed_of(sel, kind, 0xFFFFFFFF, n, id_base), allowed), kind
    for k in (1, 3, n, n + 2):
        rows, counts = FC.model_rows(lists, allowed, k, id_base)
        want_rows, want_counts = FC.loop_rows(codes, queries, allowed, k, id_base)
        assert np.array_equal(rows, want_rows) and np.array_equal(counts, want_counts), k
        if not allowed.any():
            continue
        for k_first in (0, k, 2 * k):
            for tie_cut in (False, True):
                done = _finished_rows(lists, allowed, k, k_first, tie_cut, id_base)
                st, trace = FC.stats_model(lists, allowed, k, k_first, id_base, tie_cut, route=1)
                assert len(done) == len(lists) - st["n_fallback"] and st["n_searched"] == sum(t[1] for t in trace)
                for i, row in done.items():
                    assert np.array_equal(row, rows[i][:len(row)]) and len(row) == counts[i], (k, k_first, tie_cut, i)


def test_route_and_stats_of_the_model():
    codes, queries = FC.uniform_case(64)
    lists = DC.sorted_lists(codes, queries)
    n, nq = len(codes), len(queries)
    dense, sparse = FC.random_mask(n, 2, 5), FC.random_mask(n, 256, 6)
    st, _ = FC.stats_model(lists, dense, 10)
    assert st["routes"] == FC.RAN_POST and st["n_windows"] == 0 and st["n_rounds"] >= 1 and st["n_allowed"] == np.count_nonzero(dense)
    st, _ = FC.stats_model(lists, sparse, 10)
    assert st["routes"] == FC.RAN_PRE and st["n_rounds"] == 0 and st["n_windows"] == 1 and st["k_last"] == 0
    st, _ = FC.stats_model(lists, sparse, 10, route=1)
    assert st["routes"] & FC.RAN_POST and st["n_rounds"] >= 1
    a = int(np.count_nonzero(dense))
    st, _ = FC.stats_model(lists, dense, 10, route=2, window=256)
    assert st["n_windows"] == (a + 255) // 256 and a > 1500
    st, _ = FC.stats_model(lists, dense, 10, route=2, window=256, scratch=64)         # 8 queries per sub-batch at one slice
    assert st["n_windows"] == ((a + 255) // 256) * ((nq + 7) // 8)


# ---- reach: the crafted cases do what they are for ------------------------------------------------------------------------------------------
def test_the_fallback_case_reaches_the_fallback():
    codes, sel, queries, allowed = FC.fallback_case()
    assert np.array_equal(FC.allowed_of(sel, FC.NOT_EQUAL, 5, len(codes)), allowed) and np.count_nonzero(allowed) == 400
    lists = DC.truncation_lists()
    for L in lists:                                                          # more than 8192 disallowed records lie nearest to every query
        first = int(np.argmax(allowed[(L & np.uint64(0xFFFFFFFF)).astype(np.int64)]))
        assert first == 8600 > FC.MAX_K
    for tie_cut in (False, True):
        st, trace = FC.stats_model(lists, allowed, 5, route=1, tie_cut=tie_cut)
        assert st["k_last"] == FC.MAX_K and st["n_fallback"] == len(queries) and st["routes"] == FC.RAN_POST | FC.RAN_PRE and st["n_windows"] == 1
        assert trace[-1][0] == FC.MAX_K
    rows, counts = FC.model_rows(lists, allowed, 5)
    assert np.all(counts == 5) and np.all(rows != FC.INF) and np.all((rows >> np.uint64(32)) >= 15)


@pytest.mark.parametrize("bits,A", [(64, 63), (64, 64), (64, 65), (64, 1300), (512, 200), (128, 700)])
def test_the_tie_case_has_its_ties_where_it_wants_them(bits, A):
    codes, allowed, queries, k = FC.tie_case(bits, A)
    assert len(codes) == 2 * A and np.count_nonzero(allowed) == A and np.array_equal(codes[0::2], codes[1::2])
    ties, take, slices = FC.tie_reach(bits, A)
    assert 0 < take < ties, (ties, take)                                     # the k-th distance holds more allowed records than the row takes
    if A > FC.slice_len(bits // 64):
        assert len(slices) >= 2, slices                                      # the taken ties straddle a wave-slice edge
    assert len(np.unique(codes, axis=0)) <= 9
    lists = DC.sorted_lists(codes, queries)
    rows, _ = FC.model_rows(lists, allowed, k)
    assert np.all((rows & np.uint64(1)) == 1)                                # only odd ids: the disallowed copies are skipped
    # ties go to the smaller id: the taken ties are the first of their distance in id order
    L = FC.allowed_lists(lists, allowed)[0]
    dk = L[k - 1] >> np.uint64(32)
    group = np.sort(L[(L >> np.uint64(32)) == dk])
    assert np.array_equal(rows[0][k - take:], group[:take])
