"""Scoped k-NN without a GPU: the ABI surface, the code object of the kernels, the plan arithmetic under the sanitizers, and the
expectation of test_scope_gpu.py -- that the numpy model agrees with plain loops and with the plan header, and that the crafted cases
reach what they are there for."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import distinct_common as DC
import scope_common as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vc_search_knn_scoped", "vc_search_knn_scoped_dev", "vc_sharded_search_knn_scoped", "vc_sharded_search_knn_scoped_dev"]


def test_header_declares_and_library_exports_the_new_names(vc):
    txt = open(os.path.join(ROOT, "include", "verticut_gpu.h")).read()
    assert re.search(r"#define\s+VC_ABI_VERSION\s+2\b", txt)             # entry points are only added
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"typedef struct vc_scope_stats\s*\{\s*uint64_t n_matched;\s*uint64_t n_pairs;\s*uint32_t n_scopes;\s*uint32_t n_windows;"
                     r"\s*uint64_t n_short;\s*uint64_t n_empty;\s*\}\s*vc_scope_stats;", code)
    L = ctypes.CDLL(vc.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in vc.EXPORTS
    for name in ("vc_search_knn_scoped_dev", "vc_sharded_search_knn_scoped_dev"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*const void\* d_queries,\s*uint32_t nq,\s*uint32_t k,\s*const uint32_t\* d_scope,"
                         r"\s*const uint32_t\* d_qscope,\s*uint32_t flags,\s*uint64_t\* d_out,\s*uint32_t\* d_counts,\s*vc_scope_stats\* stats,"
                         r"\s*void\* stream\)" % name, code), name
    for name in ("vc_search_knn_scoped", "vc_sharded_search_knn_scoped"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*const void\* queries,\s*uint32_t nq,\s*uint32_t k,\s*uint32_t order,\s*const uint32_t\* scope,"
                         r"\s*const uint32_t\* qscope,\s*uint32_t flags,\s*uint64_t\* out,\s*uint32_t\* counts,\s*vc_scope_stats\* stats\)" % name, code), name
    flat = " ".join(txt.split()).replace(" * ", " ")
    for phrase in ("a filter per query is out of scope) (see vc_search_knn_scoped*)", "There is no truncation flag and no mode argument",
                   "flags is reserved and must be 0", "VC_FILTER_NOT_EQUAL per query", "a form for queries named by id", "0, 0x80000000 and 0xFFFFFFFF included",
                   "row 0 of vc_search_knn_filtered* called with VC_FILTER_EQUAL, value = qscope[q], VC_MODE_LINEAR and that one query",
                   "not of the order of the queries"):
        assert " ".join(phrase.split()) in flat, phrase
    assert vc.VC_ABI_VERSION == 2
    st = vc.VcScopeStats
    assert ctypes.sizeof(st) == 40
    assert [getattr(st, n).offset for n in SC.STAT_NAMES] == [0, 8, 16, 20, 24, 32]
    assert st().as_dict() == SC.zero_stats()
    for cls in (vc.Engine, vc.ShardedEngine):
        for meth in ("search_knn_scoped", "search_knn_scoped_dev"):
            assert callable(getattr(cls, meth)), (cls, meth)
    host = open(os.path.join(ROOT, "verticut_amd", "host", "verticut_host.hpp")).read()
    assert re.search(r"virtual int search_knn_scoped\([^)]*\)\s*=\s*0;", host)
    assert len(re.findall(r"int search_knn_scoped\([^)]*\)\s*override", host)) == 2
    assert "return vc_search_knn_scoped(h_," in host and "return vc_sharded_search_knn_scoped(h_," in host
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "5.15" in design and "vc_search_knn_scoped" in design
    assert "vc_search_knn_scoped" in open(os.path.join(ROOT, "README.md")).read()
    assert "vc_search_knn_scoped" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_scope_kernels_use_no_scratch(vc):
    """every kernel of vc_scope.o, the three walks at each of the four code widths among them, has no scratch and no spills"""
    from verticut_amd import build as vb
    assert "vc_scope.hip" in vb.SOURCES and "vc_scope_plan.hpp" in vb.HEADERS
    res = vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_scope.o"))
    plain = ("vc_scope_pairs_kernel", "vc_scope_heads_kernel", "vc_scope_slots_kernel", "vc_scope_match_kernel", "vc_scope_list_kernel",
             "vc_scope_segs_kernel", "vc_scope_cost_kernel", "vc_scope_cut_kernel", "vc_scope_base_kernel", "vc_scope_emit_kernel")
    for kernel in plain:
        assert sum(kernel in name for name in res) == 1, (kernel, sorted(res))
    for W in (1, 2, 4, 8):
        for walk in (0, 1, 2):
            assert sum("vc_scope_walk_kernelILi%dELi%dEE" % (W, walk) in name for name in res) == 1, (W, walk, sorted(res))
    assert len(res) == len(plain) + 12, sorted(res)
    for name, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["group_segment_fixed_size"] <= 16, (name, r)                 # the match kernel's four popcounts; the histograms are dynamic
    text = open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_scope.hip")).read()
    assert "getenv" not in text                                              # the knobs are read in read_knobs, nowhere else
    engine = open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_engine.hip")).read()
    for knob in ("VC_SCOPE_SCRATCH", "VC_SCOPE_WINDOW"):
        assert engine.count('getenv("%s")' % knob) == 1, knob
    for word in ("hipLaunchCooperativeKernel", "__threadfence", "grid_group"):      # blocks meet in a later launch only
        assert word not in text, word
    filt = vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_filter.o"))       # and nothing of it went into the filtered call's unit
    assert not any("vc_scope" in name for name in filt)


def test_plan_arithmetic_under_the_sanitizers(tmp_path):
    """tests/cpp/scope_plan_test.cc over csrc/vc_scope_plan.hpp, host code only, with AddressSanitizer and UBSan; the constants and the
    planned cases it prints are those of the model"""
    src = os.path.join(ROOT, "tests", "cpp", "scope_plan_test.cc")
    exe = tmp_path / "scope_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           src, "-I", os.path.join(ROOT, "verticut_amd", "csrc")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert out.stdout.startswith("scope plan ok:")
    for key, val in (("WINDOW", SC.WINDOW), ("WINDOWMAX", SC.WINDOW_MAX), ("SCRATCH", SC.SCRATCH), ("COUNTERBYTES", SC.COUNTER_BYTES),
                     ("MAXCOUNTERS", SC.MAX_COUNTERS)):
        assert re.search(r"^%s %d$" % (key, val), out.stdout, flags=re.M), (key, out.stdout)
    for W in (1, 2, 4, 8):
        assert re.search(r"^SLICE %d %d$" % (W, SC.slice_len(W)), out.stdout, flags=re.M), out.stdout
    scope, qscope = SC.plan_scene()
    for window, W, scratch in SC.PLAN_CASES:
        p = SC.plan(scope, qscope, W, window, scratch)
        assert re.search(r"^CASE %d %d %d %d %d$" % (window, W, scratch, p["n_windows"], len(p["batches"])), out.stdout, flags=re.M), (window, W, scratch, out.stdout)
    assert [SC.key_bits(U) for U in (1, 2, 3, 4, 5, 256, 257, 65536)] == [0, 1, 2, 2, 3, 8, 9, 16]


# ---- the expectation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
def test_the_model_is_the_rule(seed):
    """against a plain double loop, on small random inputs with few distinct codes, so that ties are common"""
    rng = np.random.default_rng(seed)
    nbytes, n, id_base, nq = 8, int(rng.integers(1, 90)), int(rng.integers(0, 50)), 7
    pool = rng.integers(0, 256, size=(4, nbytes), dtype=np.uint8)
    codes = pool[rng.integers(0, 4, size=n)]
    queries = pool[rng.integers(0, 4, size=nq)] ^ np.uint8(1)
    values = np.array([0, 0xFFFFFFFF, 0x80000000, 7], dtype=np.uint32)
    scope = values[rng.integers(0, 3, size=n)]                             # 7 is carried by no record
    qscope = values[rng.integers(0, 4, size=nq)]
    lists = DC.sorted_lists(codes, queries, id_base)
    for k in (1, 3, n, n + 2):
        rows, counts = SC.model_rows(lists, scope, qscope, k, id_base)
        want_rows, want_counts = SC.loop_rows(codes, queries, scope, qscope, k, id_base)
        assert np.array_equal(rows, want_rows) and np.array_equal(counts, want_counts), k
        st = SC.stats_model(scope, qscope, k)
        sizes = np.array([np.count_nonzero(scope == v) for v in qscope])
        assert st["n_pairs"] == sizes.sum() and st["n_empty"] == np.count_nonzero(sizes == 0) and st["n_short"] == np.count_nonzero(sizes < k)
        assert st["n_scopes"] == len(set(qscope.tolist())) and st["n_matched"] == np.count_nonzero(np.isin(scope, qscope))
        assert np.array_equal(counts, np.minimum(sizes, k))
        assert st["n_windows"] == (1 if st["n_matched"] else 0)


# ---- reach: the crafted cases do what they are for ------------------------------------------------------------------------------------------
def _slices_scopes(p, W):
    """per slice of the one default window: the set of slots with a position in it"""
    ln, seg = SC.slice_len(W), p["seg"]
    slot_of = np.repeat(np.arange(len(seg) - 1), np.diff(seg))
    return [set(slot_of[s:s + ln].tolist()) for s in range(0, len(slot_of), ln)]


@pytest.mark.parametrize("bits", [64, 512])
def test_the_edge_case_has_its_edges(bits):
    k, W = 10, bits // 64
    codes, queries, scope, qscope = SC.edge_case(bits, k)
    assert len(codes) <= 9000
    ln = SC.slice_len(W)
    p = SC.plan(scope, qscope, W)
    sizes = np.diff(p["seg"])
    for want in (0, 1, k - 1, k, k + 1, 63, 64, 65, ln - 1, ln, ln + 1, 4 * ln + 1):
        assert want in sizes, want
    assert max(len(s) for s in _slices_scopes(p, W)) >= (64 if bits == 64 else 8)              # one slice packed with 64 scopes of 8 records
    if bits == 64:
        assert np.all(sizes[:64] == 8) and p["seg"][64] == ln
    starts, ends = p["seg"][:-1][sizes > 0] % ln, p["seg"][1:][sizes > 0] % ln
    if ln == 64:                                                             # a segment begins and ends at every offset of a slice
        assert set(starts.tolist()) == set(range(64)) and set(ends.tolist()) == set(range(64))
    else:                                                                    # (512 offsets do not fit under N <= 9000: the 512-bit case has them all)
        assert len(set(starts.tolist())) >= 70 and 0 in starts and 0 in ends and 1 in ends
    big = int(np.argmax(sizes))                                              # a segment that spans a block's four slices
    assert sizes[big] == 4 * ln + 1 and (p["seg"][big + 1] - 1) // ln - p["seg"][big] // ln >= 4
    per_scope = np.bincount(p["slot"], minlength=len(sizes))
    assert {1, 2, 17} <= set(per_scope.tolist())
    assert np.count_nonzero(~np.isin(scope, qscope)) >= 250                  # scopes named by no query
    assert np.count_nonzero(~np.isin(qscope, scope)) == 2                    # queries whose scope no record carries
    same = [(i, j) for i in range(len(queries)) for j in range(i) if qscope[i] == qscope[j] and np.array_equal(queries[i], queries[j])]
    assert len(same) == 1


def test_the_hostile_values_reach_every_radix_digit():
    _, _, scope, qscope = SC.hostile_case()
    u = np.unique(qscope)
    for shift in (0, 8, 16, 24):                                             # every digit of the query sort tells two of the values apart
        assert len(set(((u >> np.uint32(shift)) & np.uint32(0xFF)).tolist())) >= 2, shift
    for v in (0, 1, 0x80000000, 0xFFFFFFFF):
        assert v in u and v in scope
    assert 0x7FFFFFFF in u and 0x7FFFFFFF not in scope and 0xFFFFFFFE in scope and 0xFFFFFFFE not in u
    assert (0x01345678 in u and 0x02345678 in u) and (0x12345600 in u and 0x12345601 in u)


@pytest.mark.parametrize("bits,ties", [(64, 63), (64, 64), (64, 65), (64, 600), (512, 100)])
def test_the_tie_case_has_its_ties_where_it_wants_them(bits, ties):
    codes, queries, scope, qscope, k = SC.tie_case(bits, ties)
    assert 0 < k < ties
    lists = DC.sorted_lists(codes, queries)
    rows, counts = SC.model_rows(lists, scope, qscope, k)
    own = lists[0][scope[(lists[0] & np.uint64(0xFFFFFFFF)).astype(np.int64)] == 4]
    assert np.count_nonzero((own >> np.uint64(32)) == 0) == ties              # the k-th distance holds more own-scope records than the row takes
    assert np.count_nonzero((lists[0] >> np.uint64(32)) == 0) == 2 * ties     # and as many foreign ones, interleaved by id
    assert np.all(rows[0] % np.uint64(2) == 0) and np.all(rows[1] % np.uint64(2) == 1)
    p = SC.plan(scope, qscope, bits // 64)
    assert p["seg"][0] == 0 and p["uniq"][0] == 4                             # the copies are positions 0 .. ties - 1 of the list
    if ties == 600:
        assert (k - 1) // SC.slice_len(1) == 1                               # the taken ties cross a slice edge
    if (bits, ties) == (512, 100):
        assert (k - 1) // SC.slice_len(8) == 1


def test_the_window_case_straddles_windows_and_has_sub_batches():
    for bits in (64, 256):
        _, _, scope, qscope = SC.seven_case(bits, nq=300)
        W = bits // 64
        p = SC.plan(scope, qscope, W, window=256)
        assert any(lo // 256 != (hi - 1) // 256 for lo, hi in zip(p["lo"], p["hi"]) if hi > lo)                  # a segment straddling a window
        assert any(lo % 256 and lo // 256 != (hi - 1) // 256 for lo, hi in zip(p["lo"], p["hi"]) if hi > lo)     # that begins inside one
        assert p["n_windows"] == (int(p["seg"][-1]) + 255) // 256 > 6 and len(p["batches"]) == 1
        p = SC.plan(scope, qscope, W, window=256, scratch=4096)
        assert len(p["batches"]) >= 2 and p["n_windows"] > (int(p["seg"][-1]) + 255) // 256
        for b0, b1 in p["batches"]:
            assert b1 == b0 + 1 or sum(p["cost"][b0:b1]) * SC.COUNTER_BYTES <= 4096
        p = SC.plan(scope, qscope, W, window=1 << 25, scratch=1)
        assert len(p["batches"]) == 300 and p["window"] == SC.WINDOW and p["n_windows"] == np.count_nonzero(p["hi"] > p["lo"])


def test_the_large_case():
    codes, _, scope, qscope = SC.large_case()
    assert len(codes) == 9000 and np.count_nonzero(scope == 77) == 8800 > SC.MAX_K
    assert max(np.count_nonzero(scope == v) for v in (1, 2, 0xFFFFFFFF)) < 200 and 77 in qscope
