"""Queries named by id, without a GPU: the ABI surface (header, exports, binding), the code objects of the three new kernels,
and the test data of test_ids_gpu.py -- that the planted groups really put a query's own record everywhere the strip kernel has
to find it, that every id list really holds what it claims, and that the host-side strip used for the GPU expectations is
"brute force over all items except self"."""
import ctypes
import os
import re

import numpy as np
import pytest

import ids_common as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vc_get_codes_dev", "vc_search_knn_ids", "vc_search_knn_ids_dev", "vc_sharded_get_codes_dev", "vc_sharded_search_knn_ids",
       "vc_sharded_search_knn_ids_dev"]


def test_header_declares_and_library_exports_the_new_names(vc):
    txt = open(os.path.join(ROOT, "include", "verticut_gpu.h")).read()
    assert re.search(r"#define\s+VC_IDS_EXCLUDE_SELF\s+0x1u", txt)
    assert re.search(r"#define\s+VC_ABI_VERSION\s+2\b", txt)             # no struct changed
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = ctypes.CDLL(vc.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(L, name), name
        assert name in vc.EXPORTS
    assert vc.IDS_EXCLUDE_SELF == 1
    for cls in (vc.Engine, vc.ShardedEngine):
        for meth in ("get_codes_dev", "search_knn_ids", "search_knn_ids_dev"):
            assert callable(getattr(cls, meth))


def test_header_states_the_contract():
    txt = open(os.path.join(ROOT, "include", "verticut_gpu.h")).read()
    flat = " ".join(txt.split())
    for phrase in ("image_search_client.h:12-27", "linear_search.cc:45-46", "VC_MAX_K - 1", "Repeated ids are independent queries",
                   "Radius search by id is not offered", "no VC_NOT_FOUND"):
        assert phrase in flat, phrase


def test_new_kernels_use_no_lds_and_no_scratch(vc):
    from verticut_amd import build as vb
    res = vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_ids.o"))
    kernels = {k: v for k, v in res.items() if "vc_ids_" in k}
    assert len(kernels) == 3, sorted(res)
    for name, r in kernels.items():
        assert r["group_segment_fixed_size"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)


def test_planted_groups_are_exactly_the_planted_records():
    codes = I.codes_of("S128")
    for group in (I.GROUP7, I.GROUP40):
        same = np.flatnonzero((codes == codes[group[0]]).all(axis=1))
        assert tuple(same) == group
    assert not np.array_equal(codes[I.GROUP7[0]], codes[I.GROUP40[0]])
    assert I.codes_of("H3") is codes and I.codes_of("H8") is codes


@pytest.mark.parametrize("name", ["S128", "H3"])
def test_planted_data_produces_all_four_self_positions(name):
    base = I.SHAPES[name]["id_base"]
    seen = {(p, k): I.self_position(name, base + p, k) for p in I.PLANTED_QUERIES for k in I.KS_GROUPS}
    assert set(seen.values()) == {"first", "mid", "last", "absent"}
    # the lowest id of a group is always first; rank 3 of 7 is cut off by k = 1 and mid-row at k = 6; the highest of 7 ends the
    # 7-entry row of k = 6; the highest of 40 ends the 40-entry row of k = 39 and is cut off by k = 6
    assert all(seen[(I.GROUP7[0], k)] == "first" and seen[(I.GROUP40[0], k)] == "first" for k in I.KS_GROUPS)
    assert seen[(I.GROUP7[3], 1)] == "absent" and seen[(I.GROUP7[3], 6)] == "mid"
    assert seen[(I.GROUP7[6], 6)] == "last" and seen[(I.GROUP7[6], 39)] == "mid"
    assert seen[(I.GROUP40[39], 39)] == "last" and seen[(I.GROUP40[39], 6)] == "absent" and seen[(I.GROUP40[39], 100)] == "mid"


@pytest.mark.parametrize("name", list(I.SHAPES))
def test_id_lists_hold_what_they_claim(name):
    s = I.SHAPES[name]
    base, n, cap = s["id_base"], s["n"], s["capacity"]
    assert base + cap <= 2 ** 32
    one = I.id_list(name, 1)
    assert len(one) == 1 and I.resident(name, one)[0]
    for length in (64, 257):
        ids = I.id_list(name, length)
        assert ids.dtype == np.uint32 and len(ids) == length
        li = ids.astype(np.int64)
        for lo, hi in I.shard_bounds(name):                              # first and last id of every non-empty shard
            if hi > lo:
                assert base + lo in li and base + hi - 1 in li
        if base > 0:
            assert np.any(li < base)                                     # missing below the range
        assert np.any(li >= base + n)                                    # missing above it
        if cap > n:
            assert np.any((li >= base + n) & (li < base + cap))          # inside the capacity, not resident
        assert 0xFFFFFFFF in li and not I.resident(name, [0xFFFFFFFF])[0]
        assert np.max(np.unique(li, return_counts=True)[1]) >= 3         # an id three times
        if s["bits"] == 128:
            assert all(base + p in li for p in I.PLANTED_QUERIES)
        assert I.resident(name, ids).sum() > length // 2
    for h in I.SHARDED:
        b = I.shard_bounds(h)
        assert any(0 < hi - lo < I.SHAPES[h]["capacity"] // I.SHAPES[h]["shards"] for lo, hi in b)      # a partly filled shard
    assert I.shard_bounds("H8")[-1] == (5000, 5000)                      # an empty one
    assert I.SHAPES["H3"]["id_base"] >= 2 ** 31                          # ids use the top bit
    assert I.GROUP7[2] + 1 == I.GROUP7[3] == I.shard_bounds("H3")[1][0]  # the group of 7 straddles a shard boundary


def test_host_strip_is_brute_force_without_self():
    """every record of S128 as the query, every k: the k + 1 row with the own entry removed by value == the k smallest over
    all items except the query's own -- the expectation test_ids_gpu.py uses is pinned here without the engine"""
    codes = I.codes_of("S128")
    kmax = max(I.KS_GROUPS)
    ids = np.arange(len(codes), dtype=np.uint64)
    for qid in range(len(codes)):
        d = I.distances(codes, codes[qid])
        full = np.sort(I.pack(d, ids))
        keep = ids != np.uint64(qid)
        without = np.sort(I.pack(d[keep], ids[keep]))
        assert full[0] >> I.SH == 0
        for k in I.KS_GROUPS:
            assert np.array_equal(I.strip_row(full[:k + 1], qid, k), without[:k]), (qid, k)
    assert kmax + 1 < len(codes)


def test_host_strip_on_short_and_foreign_rows():
    row = np.array([5, 9, (1 << 32) | 3], dtype=np.uint64)
    assert np.array_equal(I.strip_row(row, 9, 2), [5, (1 << 32) | 3])     # removed from the middle
    assert np.array_equal(I.strip_row(row, 7, 2), [5, 9])                 # not there: cut to k
    assert np.array_equal(I.strip_row(row[:1], 5, 3), [])                 # a database of one record
    assert np.array_equal(I.strip_row(row, 3, 3), row)                    # id 3 at distance 1 is not the own entry


def test_unflagged_approximate_cases_can_stop():
    """without VC_FLAG_GLOBAL_APPROX a shard needs 20 (k + 1) candidates of its own: the k the GPU file runs in that case leave
    every non-empty shard enough records of either cluster, and the group positions 'first', 'mid', 'last' and 'absent' still occur"""
    for name in I.SHARDED:
        s, ks = I.SHAPES[name], I.unflagged_approx_ks(name)
        assert ks == (1, 6)
        codes = I.codes_of(name)
        centre_of = (codes[:, None, :] ^ codes[[I.GROUP7[0], I.GROUP40[0]]][None, :, :])
        near = (I._POP[centre_of].sum(axis=2) <= 2 * s["flips"])                 # [n, 2]: member of the cluster of group 7 / group 40
        for lo, hi in I.shard_bounds(name):
            if hi > lo:
                assert near[lo:hi].sum(axis=0).min() >= 20 * (max(ks) + 1), (name, lo, hi)
        seen = {I.self_position(name, s["id_base"] + p, k) for p in I.PLANTED_QUERIES for k in ks}
        assert seen == {"first", "mid", "last", "absent"}
    assert I.unflagged_approx_ks("S128") == I.KS_GROUPS
