"""Label groups summarised, without a GPU: the ABI surface, the code objects of the kernels, the plan arithmetic under the sanitizers,
and the expectation of test_groups_gpu.py -- that the numpy model is the contract (against plain loops) and that the crafted inputs
reach every case they are there for."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import groups_common as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vc_group_summary", "vc_group_summary_dev", "vc_sharded_group_summary", "vc_sharded_group_summary_dev"]


def test_header_declares_and_library_exports_the_new_names(vc):
    txt = open(os.path.join(ROOT, "include", "verticut_gpu.h")).read()
    assert re.search(r"#define\s+VC_ABI_VERSION\s+2\b", txt)             # entry points are only added
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"typedef struct vc_group\s*\{\s*uint32_t label;\s*uint32_t size;\s*uint32_t rep;\s*uint32_t rep_dist;\s*uint32_t max_dist;"
                     r"\s*uint32_t reserved;\s*\}\s*vc_group;", code)
    L = ctypes.CDLL(vc.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(L, name), name
        assert name in vc.EXPORTS
    assert vc.GROUP_DTYPE.itemsize == 24 and vc.GROUP_DTYPE.names == GC.GROUP_FIELDS and vc.GROUP_DTYPE == GC.GROUP_DTYPE
    for cls in (vc.Engine, vc.ShardedEngine):
        for meth in ("group_summary", "group_summary_dev"):
            assert callable(getattr(cls, meth))
    host = open(os.path.join(ROOT, "verticut_amd", "host", "verticut_host.hpp")).read()
    assert re.search(r"virtual int group_summary\([^)]*\)\s*=\s*0;", host)
    assert len(re.findall(r"int group_summary\([^)]*\)\s*override", host)) == 2
    assert "return vc_group_summary(h_," in host and "return vc_sharded_group_summary(h_," in host


def test_group_kernels_use_no_scratch_and_no_lds(vc):
    """vc_groups.o holds the new kernels -- the two window kernels once per code width -- with no scratch, no spills and no LDS"""
    from verticut_amd import build as vb
    assert "vc_groups.hip" in vb.SOURCES and "vc_groups_plan.hpp" in vb.HEADERS
    res = vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_groups.o"))
    once = ("prep", "heads", "starts", "sizes", "meta", "windows", "big_init", "big_centroid", "big_finish", "scatter")
    for kernel in once:
        assert sum("vc_groups_%s_kernel" % kernel in name for name in res) == 1, (kernel, sorted(res))
    for kernel in ("small", "items"):
        assert sum("vc_groups_%s_kernel" % kernel in name for name in res) == 4, (kernel, sorted(res))       # W = 1, 2, 4, 8
    assert len(res) == len(once) + 8, sorted(res)
    for name, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == 0, (name, r)
    text = open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_groups.hip")).read()
    assert "getenv" not in text                                            # the knob is read in read_knobs, nowhere else
    engine = open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_engine.hip")).read()
    assert engine.count('getenv("VC_GROUP_WINDOW")') == 1


def test_plan_arithmetic_under_the_sanitizers(tmp_path):
    """tests/cpp/groups_plan_test.cc over csrc/vc_groups_plan.hpp, host code only, with AddressSanitizer and UBSan"""
    src = os.path.join(ROOT, "tests", "cpp", "groups_plan_test.cc")
    exe = tmp_path / "groups_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           src, "-I", os.path.join(ROOT, "verticut_amd", "csrc")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert out.stdout.startswith("groups plan ok:")


# ---- the expectation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("seed", range(6))
def test_the_model_is_the_contract(bits, seed):
    """against plain loops, on small random inputs with few bits set apart (so that ties of both kinds are common)"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 60))
    id_base = int(rng.integers(0, 1000)) if seed % 2 else 0
    codes = np.zeros((n, bits // 8), np.uint8)
    codes[:, :2] = rng.integers(0, 4, size=(n, 2), dtype=np.uint8)
    labels = (rng.integers(0, max(1, n // 4 + seed), size=n) % n + id_base).astype(np.uint32)
    GC.same(GC.model(codes, labels, id_base), GC.naive(codes, labels, id_base), (bits, seed))
    codes = GC.uniform_codes(n, bits, seed)
    GC.same(GC.model(codes, labels, id_base), GC.naive(codes, labels, id_base), (bits, seed, "uniform"))


def test_the_model_on_nothing():
    got = GC.model(np.zeros((0, 8), np.uint8), np.zeros(0, np.uint32))
    assert [len(x) for x in got] == [0, 0, 0, 0] and got[1].shape == (0, 8)


def _bit_counts(codes, members):
    return np.unpackbits(codes[members], axis=1, bitorder="little").sum(axis=0)


@pytest.mark.parametrize("bits", GC.WIDTHS)
def test_the_crafted_inputs_reach_every_case(bits):
    codes, labels = GC.tier_case(bits)
    groups, cents, rep_labels, group_index = GC.tier_expect(bits)
    n, sizes = len(labels), GC.tier_sizes()
    assert 6000 <= n <= 8192 and tuple(groups["size"]) == sizes and set(GC.TIER_SIZES) <= set(sizes)
    starts = np.r_[0, np.cumsum(sizes)]
    members = lambda g: np.flatnonzero(group_index == g)
    # an even group with a bit set in exactly half of the members: the centroid bit is 0
    even = [g for g, s in enumerate(sizes) if s % 2 == 0 and 4 <= s <= 1024]
    assert {64, 1024} <= {sizes[g] for g in even}
    for g in even:
        assert _bit_counts(codes, members(g))[0] * 2 == sizes[g] and cents[g, 0] & 1 == 0
    pair = sizes.index(2)
    a, b = codes[members(pair)]
    assert np.array_equal(cents[pair], a & b) and (a != b).any()
    # a representative tie that the id breaks, in each tier
    unpack = lambda x: np.unpackbits(x, axis=-1, bitorder="little").astype(np.int64)
    tied = set()
    for g, s in enumerate(sizes):
        m = members(g)
        d = np.abs(unpack(codes[m]) - unpack(cents[g])).sum(axis=1)
        assert d.min() == groups["rep_dist"][g] and d.max() == groups["max_dist"][g]
        first = m[np.flatnonzero(d == d.min())]
        assert groups["rep"][g] == first[0] and np.all(rep_labels[m] == first[0])
        if len(first) > 1:
            tied.add(min(s, 1025) if s > 2 else 2)
    assert {2, 3, 1025} <= tied
    pairs = [g for g, s in enumerate(sizes) if s == 2]
    assert any(groups["rep"][g] == members(g)[1] for g in pairs) and any(groups["rep_dist"][g] < groups["max_dist"][g] for g in pairs)
    big = sizes.index(2049)
    assert groups["rep_dist"][big] == 0 and groups["rep"][big] != members(big)[0]
    # a label value that is no member of its own group; and labels that are no fixed points
    foreign = [g for g in range(len(sizes)) if group_index[groups["label"][g]] != g]
    assert len(foreign) > len(sizes) // 2 and np.count_nonzero(labels[labels] != labels) > n // 2
    assert np.all(rep_labels[rep_labels] == rep_labels)                   # what VC_RETAIN_ROOTS needs
    # the layout against windows of 2048 sorted positions
    W = GC.SMALL_WINDOW
    assert -(-n // W) == 4
    g = int(np.searchsorted(starts, 2047))
    assert starts[g] == 2047 and sizes[g] == 2                             # a pair astride the first boundary: the small tier reads the overlap
    g = int(np.searchsorted(starts, 4094))
    assert starts[g] == 4094 and sizes[g] == 65                            # a wave-tier group astride the second
    assert starts[big] == 4159
    chunk_windows = [(starts[big] + 1024 * c) // W for c in range(3)]
    big_starts = [starts[g] + 1024 * c for g, s in enumerate(sizes) if s > 1024 for c in range(-(-s // 1024))]
    assert sorted({p // W for p in big_starts}) == [0, 2, 3]              # window 1 holds no chunk of a big group: the second walk skips it
    assert chunk_windows == [2, 2, 3] and starts[big] + 1024 < 3 * W < starts[big] + 2048   # chunks in two windows, one astride 6144
    one_window = sizes.index(1025)
    assert starts[one_window] == 0 and sizes.index(1024) > one_window


def test_the_clustered_codes_group():
    codes = GC.clustered_codes(600, 64, 5)
    assert len(np.unique(codes, axis=0)) > 100 and codes.shape == (600, 8)
