"""Device-side seeding, without a GPU: the ABI surface, the code object of the kernels, the plan arithmetic under the sanitizers, and
the expectation of test_seed_gpu.py -- that the numpy model is the header's rule (against plain loops, the generator against an
independent transcription) and that the crafted cases reach what they are there for."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import seed_common as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vc_seed_centres", "vc_seed_centres_dev", "vc_sharded_seed_centres", "vc_sharded_seed_centres_dev"]


def test_header_declares_and_library_exports_the_new_names(vc):
    txt = open(os.path.join(ROOT, "include", "verticut_gpu.h")).read()
    assert re.search(r"#define\s+VC_ABI_VERSION\s+2\b", txt)             # entry points are only added
    assert "there is no device-side seeding" not in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"#define\s+VC_SEED_FARTHEST\s+0u\b", code) and re.search(r"#define\s+VC_SEED_WEIGHTED\s+1u\b", code)
    assert re.search(r"typedef struct vc_seed_stats\s*\{\s*uint64_t cost;\s*uint32_t radius, n_zero_picks;\s*\}\s*vc_seed_stats;", code)
    L = ctypes.CDLL(vc.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(L, name), name
        assert name in vc.EXPORTS
    for name in ("vc_seed_centres_dev", "vc_sharded_seed_centres_dev"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*uint32_t n_centres,\s*uint32_t method,\s*uint64_t seed,\s*void\* d_centres,\s*uint64_t\* d_picks,"
                         r"\s*uint64_t\* d_assign,\s*vc_seed_stats\* stats,\s*void\* stream\)" % name, code), name
    assert vc.VC_ABI_VERSION == 2 and (vc.SEED_FARTHEST, vc.SEED_WEIGHTED) == (0, 1) == (SC.FARTHEST, SC.WEIGHTED)
    st = vc.VcSeedStats
    assert ctypes.sizeof(st) == 16
    assert (st.cost.offset, st.radius.offset, st.n_zero_picks.offset) == (0, 8, 12)
    assert set(st().as_dict()) == set(SC.zero_stats())
    for cls in (vc.Engine, vc.ShardedEngine):
        for meth in ("seed_centres", "seed_centres_dev", "kmajority"):
            assert callable(getattr(cls, meth)), (cls, meth)
        assert "there is no device-side seeding" not in cls.kmajority.__doc__ and "seed_centres" in cls.kmajority.__doc__
    host = open(os.path.join(ROOT, "verticut_amd", "host", "verticut_host.hpp")).read()
    assert re.search(r"virtual int seed_centres\([^)]*\)\s*=\s*0;", host)
    assert len(re.findall(r"int seed_centres\([^)]*\)\s*override", host)) == 2
    assert "return vc_seed_centres(h_," in host and "return vc_sharded_seed_centres(h_," in host
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "there is no device-side seeding" not in design and "5.12" in design


def test_seed_kernels_use_no_scratch(vc):
    """vc_seed.o holds every new kernel -- the round kernel once per code width -- with no scratch and no spills, and a few words of
    LDS (the four wave results of a block)"""
    from verticut_amd import build as vb
    assert "vc_seed.hip" in vb.SOURCES and "vc_seed_plan.hpp" in vb.HEADERS
    res = vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_seed.o"))
    once = ("vc_seed_init_kernel", "vc_seed_pick_kernel", "vc_seed_finish_kernel")
    for kernel in once:
        assert sum(kernel in name for name in res) == 1, (kernel, sorted(res))
    main = sorted(name for name in res if "vc_seed_round_kernel" in name)
    assert len(main) == 4 and len(res) == len(once) + 4, sorted(res)
    for W in (1, 2, 4, 8):
        assert sum("vc_seed_round_kernelILi%dEE" % W in name for name in main) == 1, (W, main)
    for name, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["group_segment_fixed_size"] <= 64, (name, r)
        for banned in ("vc_assign_kernel", "vc_kmaj", "retain_", "mih_", "vc_scan_kernel"):
            assert banned not in name
    text = open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_seed.hip")).read()
    assert "getenv" not in text                                            # no knob changes a bit of the result: there is none
    for word in ("hipLaunchCooperativeKernel", "__threadfence", "grid_group"):    # blocks meet in atomics or in a later launch only
        assert word not in text, word


def _plan_test(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "seed_plan_test.cc")
    exe = tmp_path / "seed_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           src, "-I", os.path.join(ROOT, "verticut_amd", "csrc")])
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)


def test_plan_arithmetic_under_the_sanitizers(tmp_path):
    """tests/cpp/seed_plan_test.cc over csrc/vc_seed_plan.hpp, host code only, with AddressSanitizer and UBSan; the block size the
    crafted cases are laid out against is the plan's"""
    out = _plan_test(tmp_path)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert out.stdout.startswith("seed plan ok:")
    assert re.search(r"^B %d$" % SC.B, out.stdout, flags=re.M) and re.search(r"^TRIP %d$" % SC.PICK_TRIP, out.stdout, flags=re.M), out.stdout


# ---- the expectation ------------------------------------------------------------------------------------------------------------------
def test_the_generator_against_an_independent_transcription():
    """SplitMix64 as one reads it off the issue, state and all; its first outputs for seed 0 are the published ones"""
    class SplitMix:
        def __init__(self, seed):
            self.x = seed

        def next(self):
            m = 0xFFFFFFFFFFFFFFFF
            self.x = (self.x + 0x9E3779B97F4A7C15) & m
            z = self.x
            z = ((z ^ z >> 30) * 0xBF58476D1CE4E5B9) & m
            z = ((z ^ z >> 27) * 0x94D049BB133111EB) & m
            return z ^ z >> 31

    for seed in (0, 1, 0xFFFFFFFFFFFFFFFF, 0x0123456789ABCDEF):
        g = SplitMix(seed)
        assert [g.next() for _ in range(6)] == [SC.draw(seed, t) for t in range(6)], seed
    assert [SC.draw(0, t) for t in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


@pytest.mark.parametrize("method", SC.METHODS)
@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("seed", [0, 1, 2, 0xDEADBEEFCAFEF00D, 5, 6])
def test_the_model_is_the_rule(bits, seed, method):
    """against plain loops, on small random inputs with few distinct bits (so that ties of distance and exhausted stores are common)"""
    rng = np.random.default_rng(seed & 0xFFFF)
    n = int(rng.integers(2, 60))
    k = int(rng.integers(1, min(n, 12) + 1))
    id_base = int(rng.integers(1, 1000)) if seed % 2 else 0
    codes = np.zeros((n, bits // 8), np.uint8)
    codes[:, :2] = rng.integers(0, 4, size=(n, 2), dtype=np.uint8)
    SC.same_run(SC.seed_model(codes, k, method, seed, id_base), SC.seed_naive(codes, k, method, seed, id_base), (bits, seed, method))
    codes = SC.GC.uniform_codes(n, bits, seed & 0xFFFF)
    got = SC.seed_model(codes, k, method, seed, id_base)
    SC.same_run(got, SC.seed_naive(codes, k, method, seed, id_base), (bits, seed, method, "uniform"))
    assert got[0].dtype == np.uint8 and got[1].dtype == np.uint64 and got[2].dtype == np.uint64
    assert np.array_equal(SC.index_of(got[1]) - id_base, [np.flatnonzero((codes == c).all(axis=1))[0] for c in got[0]])   # picks name the centres' records


def test_the_model_on_nothing():
    got = SC.seed_model(np.zeros((0, 8), np.uint8), 3, SC.FARTHEST, 0)
    assert got[0].shape == (3, 8) and len(got[1]) == 3 and len(got[2]) == 0 and got[3] == SC.zero_stats()


def _assign_nearest(codes, centres):
    d = np.stack([SC.dist_to(codes, c) for c in centres], axis=1)
    idx = np.argmin(d, axis=1)
    return d[np.arange(len(codes)), idx].astype(np.uint64) << np.uint64(32) | idx.astype(np.uint64)


# ---- reach: each crafted case does what it is for, on the model -----------------------------------------------------------------------
@pytest.mark.parametrize("method", SC.METHODS)
@pytest.mark.parametrize("bits", SC.WIDTHS)
@pytest.mark.parametrize("number", SC.CASES)
def test_consequences_of_the_rule(number, bits, method):
    codes, k = SC.case_codes(number, bits), SC.case_k(number)
    centres, picks, assign, st, _ = SC.case_expect(number, bits, method)
    assert centres.shape == (k, bits // 8) and picks.shape == (k,) and assign.shape == (len(codes),)
    if number != 5 or bits == 64:                                        # (K full distance passes over 262 149 records: once is enough)
        assert np.array_equal(assign, _assign_nearest(codes, centres))   # the same strict < in ascending index
    assert st["cost"] == SC.dist_of(assign).sum() and st["radius"] == SC.dist_of(assign).max()
    pd = SC.dist_of(picks)
    assert pd[0] == 0 and st["n_zero_picks"] == np.count_nonzero(pd[1:] == 0)
    assert np.array_equal(codes[SC.index_of(picks)], centres)
    if method == SC.FARTHEST:
        assert np.all(np.diff(pd[1:]) <= 0) and st["radius"] <= pd[-1]                # the covering radii never rise
    zero = np.flatnonzero(pd[1:] == 0) + 1                               # a zero pick: every record coincides with a seed, record 0 it is
    assert np.all(SC.index_of(picks)[zero] == 0)
    if len(zero):
        assert st["cost"] == 0 and np.all(pd[zero[0]:] == 0)


@pytest.mark.parametrize("bits", SC.WIDTHS)
def test_case_1_ties(bits):
    codes = SC.case_codes(1, bits)
    assert codes.shape == (4099, bits // 8) and len(np.unique(codes, axis=0)) <= 16 and np.all(codes[:, 2:] == codes[0, 2:])
    trace = SC.case_expect(1, bits, SC.FARTHEST)[4]
    assert len(trace) == SC.case_k(1) - 1 and all(r["n_at_max"] >= 2 for r in trace)      # every maximum is shared ...
    centres, picks = SC.case_expect(1, bits, SC.FARTHEST)[:2]
    for t, r in enumerate(trace):                                                         # ... and the smallest index is taken
        d = np.min(np.stack([SC.dist_to(codes, c) for c in centres[:t + 1]]), axis=0)
        assert r["record"] == np.flatnonzero(d == d.max())[0] == SC.index_of(picks)[t + 1]
    trace = SC.case_expect(1, bits, SC.WEIGHTED)[4]
    assert len({r["block"] for r in trace}) > 1                                           # the weighted picks fall into several blocks


@pytest.mark.parametrize("method", SC.METHODS)
@pytest.mark.parametrize("bits", SC.WIDTHS)
def test_case_2_exhaustion(bits, method):
    codes = SC.case_codes(2, bits)
    assert len(codes) == 300 and len(np.unique(codes, axis=0)) == 5 and SC.case_k(2) == 9
    centres, picks, assign, st, _ = SC.case_expect(2, bits, method)
    pd, pi = SC.dist_of(picks), SC.index_of(picks)
    assert np.all(pd[1:5] > 0) and np.all(pd[5:] == 0) and st["n_zero_picks"] == 4       # exactly 5 picks that are the first or at a distance
    assert np.all(pi[5:] == 0) and len(np.unique(centres[:5], axis=0)) == 5 and st["cost"] == 0 and st["radius"] == 0


@pytest.mark.parametrize("bits", SC.WIDTHS)
def test_case_3_edges(bits):
    codes = SC.case_codes(3, bits)
    assert len(codes) == 3 * SC.B + 1 and SC.EDGE_RECORDS == (0, SC.B - 1, SC.B, 2 * SC.B - 1, 3 * SC.B - 1, 3 * SC.B)
    common = codes[1]
    d = SC.dist_to(codes, common)
    assert tuple(d[list(SC.EDGE_RECORDS)]) == SC.EDGE_FLIPS and np.count_nonzero(d) == 6 and len(set(SC.EDGE_FLIPS)) == 6
    picks = SC.case_expect(3, bits, SC.FARTHEST)[1]
    order = [i for _, i in sorted(zip(SC.EDGE_FLIPS, SC.EDGE_RECORDS), reverse=True)]
    assert SC.index_of(picks)[0] not in SC.EDGE_RECORDS
    assert list(SC.index_of(picks)[1:]) == order and list(SC.dist_of(picks)[1:]) == sorted(SC.EDGE_FLIPS, reverse=True)   # descending distance, whatever the block
    seen = set()
    for seed in SC.EDGE_SEEDS:                                                           # a condition on the inputs, met by the model alone
        seen |= set(SC.index_of(SC.case_expect(3, bits, SC.WEIGHTED, 0, seed)[1]).tolist())
    assert set(SC.EDGE_RECORDS) <= seen


@pytest.mark.parametrize("method", SC.METHODS)
@pytest.mark.parametrize("bits", SC.WIDTHS)
def test_case_4_every_record_is_picked(bits, method):
    picks, st = SC.case_expect(4, bits, method)[1], SC.case_expect(4, bits, method)[3]
    assert sorted(SC.index_of(picks)) == list(range(50)) and st == SC.zero_stats()


@pytest.mark.parametrize("bits", SC.WIDTHS)
def test_case_5_long_scan(bits):
    codes = SC.case_codes(5, bits)
    assert len(codes) == 256 * SC.B + 5 and -(-len(codes) // SC.B) > SC.PICK_TRIP         # more partials than one trip of the pick kernel holds
    trace = SC.case_expect(5, bits, SC.WEIGHTED)[4]
    assert len(trace) == 7 and max(r["block"] for r in trace) >= 256 and min(r["block"] for r in trace) < 256
    assert trace[0]["block"] == 256                                                       # what long_scan_seed looks for
