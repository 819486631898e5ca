"""Radius search for queries named by id, without a GPU: the ABI surface, the code objects of the compaction kernels, and the
test data of test_radius_ids_gpu.py -- that the engine-free expectation of radius_ids_common.py is the radius search's result
for the record's code, and that the id lists really produce every case the compaction has to get right."""
import ctypes
import os
import re

import numpy as np
import pytest

import ids_common as I
import radius_ids_common as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vc_search_radius_ids", "vc_search_radius_ids_dev", "vc_sharded_search_radius_ids", "vc_sharded_search_radius_ids_dev"]


def test_header_declares_and_library_exports_the_new_names(vc):
    txt = open(os.path.join(ROOT, "include", "verticut_gpu.h")).read()
    assert re.search(r"#define\s+VC_IDS_ONLY_GREATER\s+0x2u", txt)
    assert re.search(r"#define\s+VC_ABI_VERSION\s+2\b", txt)             # entry points are only added
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = ctypes.CDLL(vc.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(L, name), name
        assert name in vc.EXPORTS
    assert (vc.IDS_EXCLUDE_SELF, vc.IDS_ONLY_GREATER) == (R.EXCLUDE_SELF, R.ONLY_GREATER) == (1, 2)
    for cls in (vc.Engine, vc.ShardedEngine):
        for meth in ("search_radius_ids", "search_radius_ids_dev"):
            assert callable(getattr(cls, meth))
    host = open(os.path.join(ROOT, "verticut_amd", "host", "verticut_host.hpp")).read()
    assert re.search(r"virtual int search_radius_ids\([^)]*\)\s*=\s*0;", host)
    assert host.count("search_radius_ids(") >= 4 and "search_image_by_id_within(uint32_t id, uint32_t radius" in host


def test_compaction_kernels_keep_lds_to_the_block_prefix(vc):
    """five kernels, none with scratch or spills; LDS only for the waves' sums of a block-level prefix (at most 16 words of 8
    bytes), and the chunk of entries the work is cut into is at most 2 048"""
    from verticut_amd import build as vb
    res = vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_ids_radius.o"))
    kernels = {k: v for k, v in res.items() if "vc_ids_radius_" in k}
    assert len(kernels) == 5, sorted(res)
    for name, r in kernels.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["group_segment_fixed_size"] <= 128, (name, r)
    hdr = open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_internal.hpp")).read()
    chunk = int(re.search(r"#define\s+VC_IDS_RCHUNK\s+(\d+)u", hdr).group(1))
    assert chunk <= 2048 and 2540 > chunk          # S128 at R = 16 puts a segment across at least two chunks


@pytest.mark.parametrize("name", ["S128", "S64"])
def test_expectation_without_flags_is_the_radius_search(oracle, name):
    """MihOracle.radius on the record's code == brute force, filter, sort -- for every resident id of the longest list"""
    s = I.SHAPES[name]
    codes = I.codes_of(name)
    mo = oracle.MihOracle(codes, s["m"], key_mode=1, id_base=s["id_base"])
    try:
        ids = I.id_list(name, 257)
        for radius in (0, 3, 6):
            for qid in ids[I.resident(name, ids)][::4]:
                got, _ = mo.radius(codes[int(qid) - s["id_base"]], radius)
                assert np.array_equal(got, R.expect(name, qid, radius)), (radius, qid)
    finally:
        mo.close()
    for qid in ids[~I.resident(name, ids)]:
        assert len(R.expect(name, qid, 6)) == 0


def test_flag_rules_on_a_hand_made_segment():
    d1 = 1 << 32
    seg = np.array([3, 9, 12, d1 | 1, d1 | 9, d1 | 10, 2 * d1 | 4, 2 * d1 | 11], dtype=np.uint64)
    assert np.array_equal(R.apply_flags(seg, 9, R.EXCLUDE_SELF), seg[[0, 2, 3, 4, 5, 6, 7]])     # (1, 9) is not the own entry
    assert np.array_equal(R.apply_flags(seg, 9, R.ONLY_GREATER), seg[[2, 5, 7]])
    assert np.array_equal(R.apply_flags(seg, 9, R.ONLY_GREATER | R.EXCLUDE_SELF), seg[[2, 5, 7]])
    assert len(R.apply_flags(seg, 12, R.ONLY_GREATER)) == 0


def test_s128_figures():
    """the figures the GPU cases rely on, at L = 257"""
    name = "S128"
    ids = I.id_list(name, 257)
    res = I.resident(name, ids)
    assert 32 <= (~res).sum() <= 34 and res.sum() == 225
    lens0 = np.array([len(R.expect(name, q, 0)) for q in ids])
    assert ((lens0 == 1) & res).sum() == 157                             # the own entry alone: empty after EXCLUDE_SELF
    assert sum(len(R.expect(name, q, 0, R.EXCLUDE_SELF)) == 0 for q in ids[res]) == 157
    assert sum(len(R.expect(name, q, 0, R.ONLY_GREATER)) == 0 for q in ids[res]) == 170
    lens16 = np.array([len(R.expect(name, q, 16)) for q in ids])
    assert lens16.sum() == 562620 and lens16.max() == 2540               # the longest segment spans three chunks of 1 024
    assert sum(len(R.expect(name, q, 16, R.ONLY_GREATER)) == 0 for q in ids[res]) == 2
    assert max(len(R.expect("S64", q, 0)) for q in I.id_list("S64", 257)) == 173


@pytest.mark.parametrize("name", I.SINGLE)
def test_inputs_produce_every_case(name):
    s = I.SHAPES[name]
    # a missing id first, in the middle and last in a list; lists whose later segments shift behind an empty one
    edge = R.edge_list(name)
    res = I.resident(name, edge)
    assert not res[0] and not res[-1] and not res[3] and res[1] and res[2] and res[4]
    ids = I.id_list(name, 257)
    res = I.resident(name, ids)
    gaps = np.flatnonzero(~res)
    assert 32 <= len(gaps) <= 34 and gaps.min() < 16 and gaps.max() > 240 and np.all(np.diff(gaps) < 32)     # scattered
    assert not I.resident(name, I.id_list(name, 64))[-1]                 # the list of 64 ends with a missing id
    longest = []
    for radius in R.RADII[name]:
        offs, flat, segs = R.expect_batch(name, ids, radius)
        lens = np.diff(offs.astype(np.int64))
        assert np.all(lens[~res] == 0) and np.all(lens[res] >= 1)
        assert np.any((lens[:-1] == 0) & (lens[1:] > 1)) and np.any((lens[:-1] > 1) & (lens[1:] == 0))   # empty next to full
        longest.append(int(lens.max()))
        # the own entry first, in the middle and last in its distance-0 run: the match is by value
        where = {R.self_position(seg, q) for seg, q in zip(segs, ids) if len(seg)}
        assert {"first", "mid", "last"} <= where, (radius, where)
        # ONLY_GREATER drops entries that are NOT one contiguous run of the segment
        scattered = 0
        for seg, q in zip(segs, ids):
            if len(seg) < 3:
                continue
            dropped = np.flatnonzero((seg & R.LOW) <= np.uint64(q))
            kept = R.apply_flags(seg, q, R.ONLY_GREATER)
            assert len(kept) + len(dropped) == len(seg) and np.all(np.diff(kept.astype(np.int64) >> 32) >= 0)
            if len(dropped) > 1 and dropped[-1] - dropped[0] + 1 > len(dropped):
                scattered += 1
        assert scattered > 0 or radius == 0, radius
        for seg, q in zip(segs, ids):                                    # EXCLUDE_SELF removes exactly one entry of a resident id
            assert len(R.apply_flags(seg, q, R.EXCLUDE_SELF)) == max(len(seg) - 1, 0)
    if name != "S128":
        assert 54 <= min(longest) and max(longest) <= 763
    assert s["id_base"] + s["capacity"] <= 2 ** 32


def test_only_greater_lists_every_pair_exactly_once():
    """S128, R = 2, all ids: the union of the ONLY_GREATER segments is exactly the brute force's set of unordered pairs"""
    name, radius = "S128", 2
    n = I.SHAPES[name]["n"]
    pairs = []
    for q in range(n):
        seg = R.expect(name, q, radius, R.ONLY_GREATER)
        pairs.append((np.uint64(q) << I.SH) | (seg & R.LOW))
    pairs = np.concatenate(pairs)
    assert len(np.unique(pairs)) == len(pairs)                           # once
    assert np.array_equal(np.sort(pairs), R.brute_pairs(name, radius))   # and all of them
    assert len(pairs) > n
