"""vc_update_index without a GPU: the update RULE as a numpy model against a stable sort from scratch, the planted inputs of the
GPU tests, the reference-shaped oracle's buckets over old + new records, and the ABI surface."""
import ctypes
import os
import re

import numpy as np
import pytest

import index_update_common as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR_SET = sorted({(b, m, n0, d) for b, m, n0, d in U.cases()})


@pytest.mark.parametrize("bits,m", U.SHAPES, ids=["%d-%d" % c for c in U.SHAPES])
def test_the_update_rule_gives_the_index_of_a_build(bits, m):
    """For every (n0, delta) the GPU test runs at this shape and for every table: the old table merged with the sorted new pairs by
    insert points -- no old entry sorted again -- IS the table of a stable sort of all keys: ids, offsets (direct and ranked, with
    the new buckets' ranks), distinct keys (the bitmap), bucket count."""
    s = bits // m
    pairs = [(n0, d) for b, mm, n0, d in PAIR_SET if (b, mm) == (bits, m)]
    assert len(pairs) == len(U.PAIRS) + (len(U.SWEEP_N0) if (bits, m) in U.SWEEP_SHAPES else 0)
    for n0, d in pairs:
        old_k, new_k = U.keys(bits, m, n0, d)
        for t in range(m if n0 + d <= 6000 else min(m, 3)):       # (the large pairs: three tables, their data are built alike)
            old = U.table_from_scratch(old_k[:, t], s)
            got = U.update_model(old, new_k[:, t], n0, s)
            exp = U.table_from_scratch(np.concatenate([old_k[:, t], new_k[:, t]]), s)
            where = (bits, m, n0, d, t)
            assert np.array_equal(got.ids, exp.ids), where
            assert np.array_equal(got.offsets, exp.offsets), where
            assert np.array_equal(got.bitmap_keys, exp.bitmap_keys) and got.n_unique == exp.n_unique, where


def test_the_rule_applied_three_times_is_one_build():
    """repeated updates (the GPU test's rounds): the model chained over three appended parts of different sizes"""
    for bits, m in ((64, 4), (64, 2)):
        s = bits // m
        old_k, new_k = U.keys(bits, m, 300, 20000)
        k = np.concatenate([old_k[:, 0], new_k[:, 0]])
        cuts = (300, 301, 4500, 20300)
        tab = U.table_from_scratch(k[: cuts[0]], s)
        for a, b in zip(cuts, cuts[1:]):
            tab = U.update_model(tab, k[a:b], a, s)
        exp = U.table_from_scratch(k, s)
        assert np.array_equal(tab.ids, exp.ids) and np.array_equal(tab.offsets, exp.offsets) and tab.n_unique == exp.n_unique


@pytest.mark.parametrize("bits,m", U.SHAPES, ids=["%d-%d" % c for c in U.SHAPES])
def test_the_planted_inputs_contain_every_case(bits, m):
    """cases (a) .. (f) of index_update_common, table by table, on every pair that has room for them"""
    s = bits // m
    pairs = [(n0, d) for b, mm, n0, d in PAIR_SET if (b, mm) == (bits, m) and n0 >= U.PLANT_MIN_OLD and d >= U.PLANT_MIN_NEW]
    assert (300, 20000) in pairs and ((bits, m) not in U.SWEEP_SHAPES or len(pairs) == 1 + len(U.SWEEP_N0))
    for n0, d in pairs:
        old_k, new_k = U.keys(bits, m, n0, d)
        for t in range(m):
            old, new = set(old_k[:, t].tolist()), new_k[:, t].tolist()
            new_only = set(new) - old
            lo, hi = min(old), max(old)
            where = (bits, m, n0, d, t)
            assert len(old) >= U.POOL and len(old_k) // len(old) >= 5, where                 # duplicate-heavy old buckets
            assert len(set(new) & old) >= 10, where                                            # (a)
            assert 0 in new_only and sum(k < lo for k in new_only) >= 2, where                 # (b)
            assert sum(lo < k < hi for k in new_only) >= 4, where                              # (c)
            assert (1 << s) - 1 in new_only and sum(k > hi for k in new_only) >= 2, where      # (d)
            p = U.plan(bits, m, t)
            assert p.many_old in old and new.count(p.many_old) >= U.MANY, where                # (e) a key with an old bucket
            assert p.many_new in new_only and new.count(p.many_new) >= U.MANY, where           # (e) a new key
            if s == 32:                                                                        # (f)
                e = U.EDGE_BASE
                assert e % 256 == 0 and {e + 127, e + 128, e + 255, e + 256} <= new_only, where
                assert any(k >> 8 == e >> 8 for k in old) and any(k >> 8 == (e >> 8) + 1 for k in old), where
                assert U.EMPTY_BLOCK_KEY in new_only and all(k >> 8 != U.EMPTY_BLOCK_KEY >> 8 for k in old), where


@pytest.mark.parametrize("bits,m", [(64, 8), (64, 4), (64, 2), (128, 4)])
def test_oracle_buckets_of_old_and_new_are_old_then_new(oracle, bits, m):
    """build_hash_tables.cc:40-70 over old + new records (MihOracle's rule a12 buckets): every bucket is the old bucket followed by
    its new ids -- what makes the update a merge.  Also pins the key convention of the data builder against the oracle's."""
    n0, d = 300, 20000
    old_c, new_c = U.codes(bits, m, n0, d)
    old_k, new_k = U.keys(bits, m, n0, d)
    both = np.concatenate([old_c, new_c])
    mo_old = oracle.MihOracle(old_c, m, key_mode=1)
    mo_all = oracle.MihOracle(both, m, key_mode=1)
    for t in range(m):
        assert [mo_all.key(both[i], t) for i in (0, 1, n0, n0 + 1)] == [int(old_k[0, t]), int(old_k[1, t]), int(new_k[0, t]), int(new_k[1, t])]
        for key in sorted(set(old_k[:, t].tolist()) | set(new_k[:, t].tolist())):
            was, now = mo_old.bucket(t, key), mo_all.bucket(t, key)
            fresh = n0 + np.nonzero(new_k[:, t] == key)[0]
            assert np.array_equal(now[: len(was)], was) and np.array_equal(now[len(was):], fresh), (bits, m, t, key)
    mo_old.close()
    mo_all.close()


def test_abi_surface(vc):
    """the header declares both entry points, the built library exports them, the bindings expose them"""
    header = open(os.path.join(ROOT, "include", "verticut_gpu.h")).read()
    assert re.search(r"^int vc_update_index\(vc_engine\* e\);", header, re.M)
    assert re.search(r"^int vc_sharded_update_index\(vc_sharded\* h\);", header, re.M)
    assert "#define VC_ABI_VERSION 2" in header
    lib = ctypes.CDLL(vc.LIB_PATH)
    assert lib.vc_update_index and lib.vc_sharded_update_index
    assert {"vc_update_index", "vc_sharded_update_index"} <= set(vc.EXPORTS)
    assert callable(vc.Engine.update_index) and callable(vc.ShardedEngine.update_index)
    host = open(os.path.join(ROOT, "verticut_amd", "host", "verticut_host.hpp")).read()
    assert host.count("int update_index() override") == 2 and "virtual int update_index() = 0;" in host


def test_new_kernels_use_no_scratch(vc):
    """the update's kernels stream: none may spill or use scratch (the conditions test_build_cpu puts on the search kernels)"""
    from verticut_amd import build as vb
    res = {k: v for k, v in vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_mih.o")).items() if "mih_update_" in k}
    assert len(res) >= 8 and sum("merge_kernel" in k for k in res) == 4, sorted(res)
    for k, v in res.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
