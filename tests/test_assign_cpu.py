"""Nearest of K codes and k-majority, without a GPU: the ABI surface, the code object of the kernels, the plan arithmetic under the
sanitizers, and the expectation of test_assign_gpu.py / test_kmajority_gpu.py -- that the numpy models are the contracts (against plain
loops) and that the crafted cases reach what they are there for."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import assign_common as AC
import groups_common as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vc_assign_nearest", "vc_assign_nearest_dev", "vc_sharded_assign_nearest", "vc_sharded_assign_nearest_dev",
       "vc_kmajority", "vc_kmajority_dev", "vc_sharded_kmajority", "vc_sharded_kmajority_dev"]


def test_header_declares_and_library_exports_the_new_names(vc):
    txt = open(os.path.join(ROOT, "include", "verticut_gpu.h")).read()
    assert re.search(r"#define\s+VC_ABI_VERSION\s+2\b", txt)             # entry points are only added
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"#define\s+VC_KMAJ_MAX_ITERS\s+64\b", code)
    assert re.search(r"typedef struct vc_kmajority_stats\s*\{\s*uint32_t n_iters, converged;\s*uint64_t n_empty;\s*uint64_t cost_final;"
                     r"\s*uint64_t cost\[VC_KMAJ_MAX_ITERS\];\s*uint64_t n_changed\[VC_KMAJ_MAX_ITERS\];\s*\}\s*vc_kmajority_stats;", code)
    L = ctypes.CDLL(vc.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(L, name), name
        assert name in vc.EXPORTS
    assert vc.VC_ABI_VERSION == 2 and vc.KMAJ_MAX_ITERS == 64 == AC.MAX_ITERS
    st = vc.VcKmajorityStats
    assert ctypes.sizeof(st) == 1048
    assert (st.n_iters.offset, st.converged.offset, st.n_empty.offset, st.cost_final.offset, st.cost.offset, st.n_changed.offset) == (0, 4, 8, 16, 24, 536)
    assert set(st().as_dict()) == set(AC.zero_stats())
    for cls in (vc.Engine, vc.ShardedEngine):
        for meth in ("assign_nearest", "assign_nearest_dev", "kmajority", "kmajority_dev", "get_codes"):
            assert callable(getattr(cls, meth)), (cls, meth)
    host = open(os.path.join(ROOT, "verticut_amd", "host", "verticut_host.hpp")).read()
    for meth in ("assign_nearest", "kmajority"):
        assert re.search(r"virtual int %s\([^)]*\)\s*=\s*0;" % meth, host), meth
        assert len(re.findall(r"int %s\([^)]*\)\s*override" % meth, host)) == 2, meth
        assert "return vc_%s(h_," % meth in host and "return vc_sharded_%s(h_," % meth in host


def test_assign_kernels_use_no_scratch(vc):
    """vc_assign.o holds every new kernel -- vc_assign_kernel once per code width -- with no scratch and no spills; the tile of
    centres is the only LDS of any size"""
    from verticut_amd import build as vb
    assert "vc_assign.hip" in vb.SOURCES and "vc_assign_plan.hpp" in vb.HEADERS
    res = vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_assign.o"))
    once = ("vc_assign_init_kernel", "vc_kmaj_round_kernel", "vc_kmaj_scatter_kernel", "vc_kmaj_empty_kernel")
    for kernel in once:
        assert sum(kernel in name for name in res) == 1, (kernel, sorted(res))
    main = sorted(name for name in res if "vc_assign_kernel" in name)
    assert len(main) == 4 and len(res) == len(once) + 4, sorted(res)
    for W, R in ((1, 8), (2, 4), (4, 2), (8, 2)):                         # the template arguments <W, R> of the plan
        assert sum("vc_assign_kernelILi%dELi%dEE" % (W, R) in name for name in main) == 1, (W, main)
    for name, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == (16384 if "vc_assign_kernel" in name else 32 if "round" in name or "empty" in name else 0), (name, r)
        for banned in ("retain_", "mih_update_", "mih_query_kernel", "vc_scan_kernel"):
            assert banned not in name
    text = open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_assign.hip")).read()
    assert "getenv" not in text                                            # the knobs are read in read_knobs, nowhere else
    engine = open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_engine.hip")).read()
    assert engine.count('getenv("VC_ASSIGN_TILE")') == 1 and engine.count('getenv("VC_ASSIGN_SLICES")') == 1
    for src in os.listdir(os.path.join(ROOT, "verticut_amd", "csrc")):
        if src != "vc_engine.hip":
            assert "VC_ASSIGN_TILE\")" not in open(os.path.join(ROOT, "verticut_amd", "csrc", src)).read(), src


def test_plan_arithmetic_under_the_sanitizers(tmp_path):
    """tests/cpp/assign_plan_test.cc over csrc/vc_assign_plan.hpp, host code only, with AddressSanitizer and UBSan"""
    src = os.path.join(ROOT, "tests", "cpp", "assign_plan_test.cc")
    exe = tmp_path / "assign_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           src, "-I", os.path.join(ROOT, "verticut_amd", "csrc")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert out.stdout.startswith("assign plan ok:")


# ---- the expectation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("seed", range(6))
def test_the_models_are_the_contracts(bits, seed):
    """against plain loops, on small random inputs with few distinct bits (so that ties of distance between centres are common)"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 60))
    k = int(rng.integers(1, min(n, 9) + 1))
    id_base = int(rng.integers(0, 1000)) if seed % 2 else 0
    codes = np.zeros((n, bits // 8), np.uint8)
    codes[:, :2] = rng.integers(0, 4, size=(n, 2), dtype=np.uint8)
    centres = codes[rng.integers(0, n, size=k)]
    a = AC.assign_model(codes, centres)
    assert a.dtype == np.uint64 and np.array_equal(a, AC.assign_naive(codes, centres))
    assert len(AC.tie_witnesses(codes, centres)) > 0 or k == 1
    assert np.array_equal(AC.assign_model(codes, centres, 1, n - 1), a[1:])
    AC.same_run(AC.kmajority_model(codes, centres, 8, id_base), AC.kmajority_naive(codes, centres, 8, id_base), (bits, seed))
    codes = GC.uniform_codes(n, bits, seed)
    AC.same_run(AC.kmajority_model(codes, codes[:k], 8, id_base), AC.kmajority_naive(codes, codes[:k], 8, id_base), (bits, seed, "uniform"))


def test_the_models_on_nothing():
    assert len(AC.assign_model(np.zeros((5, 8), np.uint8), np.zeros((2, 8), np.uint8), 5, 0)) == 0
    got = AC.kmajority_model(np.zeros((0, 8), np.uint8), np.zeros((3, 8), np.uint8))
    assert got[0].shape == (3, 8) and len(got[1]) == 0 and len(got[2]) == 0
    AC.same_stats(got[3], AC.zero_stats())


# what each crafted case is for: (n, bits, k, rounds, converged, duplicate seeds, n_empty)
REACH = {1: (4096, 64, 40, 6, 1, 1, 1), 2: (4096, 128, 40, 6, 1, 2, 5), 3: (4096, 256, 64, 64, 0, 0, 0), 4: (1000, 64, 1000, 2, 1, 0, 0)}


@pytest.mark.parametrize("number", AC.CASES)
def test_the_crafted_cases_reach_what_they_are_for(number):
    codes, seeds = AC.case(number)
    centres, assign, labels, st = AC.case_expect(number)
    n, bits, k, rounds, converged, dup, n_empty = REACH[number]
    assert codes.shape == (n, bits // 8) and seeds.shape == (k, bits // 8)
    assert (st["n_iters"], st["converged"], st["n_empty"]) == (rounds, converged, n_empty)
    assert k - len(np.unique(seeds, axis=0)) == dup
    cost = st["cost"][:rounds].astype(np.int64)
    assert np.all(np.diff(cost) <= 0) and st["cost_final"] <= cost[-1]      # the cost never rises
    assert np.all(st["cost"][rounds:] == 0) and np.all(st["n_changed"][rounds:] == 0) and st["n_changed"][0] == n
    assert (st["n_changed"][rounds - 1] == 0) == bool(converged)
    assert np.array_equal(assign, AC.assign_model(codes, centres)) and np.array_equal(labels, AC.index_of(assign).astype(np.uint32))
    assert st["cost_final"] == AC.dist_of(assign).sum() and st["n_empty"] == k - len(np.unique(labels))
    if number == 4:
        # every record is its own centre at distance 0 and the codes are distinct, so the NEAREST centre is unique: a tie at the
        # minimum cannot occur here.  What the case does hold is ties between two centres farther away, which must not disturb it.
        assert st["cost"][0] == 0 and np.array_equal(AC.index_of(assign), np.arange(n))
        d = AC.distances(codes[:50], centres)
        assert any(len(np.unique(row)) < len(row) for row in d)
        return
    assert st["cost_final"] > 0
    # the tie rule's witness: a record whose smallest distance is reached by two centres of different index, at the seeds and at the end
    for cen in (seeds, centres):
        w = AC.tie_witnesses(codes, cen)
        assert len(w) > 0
        d = AC.distances(codes[w[:1]], cen)[0]
        assert AC.index_of(AC.assign_model(codes[w[:1]], cen))[0] == np.flatnonzero(d == d.min())[0]
    if dup:                                                                  # the later of two equal seeds wins no record in round 0
        first = {}
        later = [c for c in range(k) if first.setdefault(seeds[c].tobytes(), c) != c]
        assert len(later) == dup and not np.isin(later, AC.index_of(AC.assign_model(codes, seeds))).any()


def test_max_iters_cuts_the_same_run_short():
    full = AC.case_expect(1)[3]
    for m in (0, 1, 2):
        st = AC.case_expect(1, m)[3]
        assert st["n_iters"] == m and st["converged"] == 0 and np.array_equal(st["cost"][:m], full["cost"][:m])
    assert AC.case_expect(1, 0)[3]["cost_final"] == full["cost"][0]          # no round: just the assign to the seeds


@pytest.mark.parametrize("bits", AC.WIDTHS)
def test_the_crafted_assign_inputs(bits):
    codes, centres = AC.tie_case(bits)
    want = AC.assign_model(codes, centres)
    assert np.array_equal(centres[AC.TIE_P], centres[AC.TIE_Q]) and AC.TIE_P // 64 != AC.TIE_Q // 64
    per_slice = -(-len(centres) // 3)
    assert AC.TIE_P // per_slice != AC.TIE_Q // per_slice                   # VC_ASSIGN_SLICES=3 separates them as well
    for i in AC.TIE_RECORDS:
        assert want[i] == np.uint64(AC.TIE_P | 1 << 32), i                   # distance 1 to both, the smaller index wins
    assert want[AC.HIT_RECORD] == np.uint64(AC.HIT_CENTRE) and AC.HIT_CENTRE == len(centres) - 1 == 4 * 64
