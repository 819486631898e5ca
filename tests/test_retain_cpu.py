"""vc_retain* without a GPU: the filter RULE as a numpy model against a stable sort of the survivors, the databases and masks of
the GPU tests (every bucket situation must occur: a mask or database that reaches none of them is a test bug, and this is where it
shows), and the ABI surface."""
import ctypes
import os
import re

import numpy as np
import pytest

import index_update_common as U
import retain_common as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.cases()


def _groups():
    """(bits, m, kind, size) -> its masks"""
    out = {}
    for b, m, kind, size, mk in CASES:
        out.setdefault((b, m, kind, size), []).append(mk)
    return out


GROUPS = _groups()


def test_the_case_list_is_the_one_of_the_issue():
    assert len(R.MASKS) == 13 and len(set(R.MASKS)) == 13
    for b, m in U.SHAPES:
        for db in R.DATABASES:
            assert GROUPS[(b, m, "db", db)] == list(R.MASKS)
    for b, m in U.SWEEP_SHAPES:
        for n in R.SWEEP_N:
            assert GROUPS[(b, m, "sweep", n)] == list(R.SWEEP_MASKS)
    assert {63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 16383, 16384, 16385} <= set(R.SWEEP_N)
    assert sorted({bits // m for bits, m in U.SWEEP_SHAPES}) == [8, 16, 32]


@pytest.mark.parametrize("bits,m,kind,size", sorted(GROUPS, key=str), ids=["%d-%d-%s-%s" % (b, m, k, s) for b, m, k, s in sorted(GROUPS, key=str)])
def test_the_filter_rule_gives_the_index_of_a_build(bits, m, kind, size):
    """For every (shape, database, mask) the GPU test runs and for every table: the table of all records filtered by the rule --
    no entry sorted -- IS the table of a stable sort of the survivors' keys: ids, offsets (direct and ranked, with the vanished
    buckets' ranks closed up), distinct keys (the bitmap), bucket count; and new_ids is the survivors' rank."""
    s = bits // m
    keys = R.case_keys(bits, m, kind, size)
    tables = [U.table_from_scratch(keys[:, t], s) for t in range(m if len(keys) <= 6000 else min(m, 3))]   # (large: three tables, built alike)
    for mk in GROUPS[(bits, m, kind, size)]:
        keep = R.mask(mk, keys, bits, m)
        assert keep.dtype == bool and keep.shape == (len(keys),)
        ids = R.new_ids_model(keep, 1000)
        assert np.array_equal(ids[keep], 1000 + np.arange(keep.sum())) and np.all(ids[~keep] == R.GONE)
        for t, tab in enumerate(tables):
            got = R.retain_model(tab, keep, s)
            exp = U.table_from_scratch(keys[keep][:, t], s)
            assert R.same_table(got, exp), (bits, m, kind, size, mk, t)


def _situations(keys, keep, s):
    """what a mask does to one table's buckets"""
    out = set()
    col = keys.astype(np.int64)
    order = np.argsort(col, kind="stable")
    sk, kp = col[order], keep[order]
    starts = np.nonzero(np.append(True, sk[1:] != sk[:-1]))[0]
    ends = np.append(starts[1:], len(sk))
    alive_keys = set(col[keep].tolist())
    vanished = []
    for a, b in zip(starts, ends):
        key, k = int(sk[a]), kp[a:b]
        if not k.any():
            vanished.append(key)
            continue
        if not k[0]:
            out.add("head")
        if not k[-1]:
            out.add("tail")
        if b - a >= 3 and not k[1:-1].all():
            out.add("middle")
    if not vanished:
        out.add("no_bucket_vanishes")
    lo, hi = (min(alive_keys), max(alive_keys)) if alive_keys else (None, None)
    for key in vanished:
        if key == 0:
            out.add("vanish_0")
        if key == (1 << s) - 1:
            out.add("vanish_top")
        if alive_keys and lo < key < hi:
            out.add("vanish_between")
        if s == 32:
            e = U.EDGE_BASE
            for name, edge_key in (("line_lo", e + 127), ("line_hi", e + 128), ("block_lo", e + 255), ("block_hi", e + 256)):
                if key == edge_key:
                    out.add(name)
            if not any(k >> 8 == key >> 8 for k in alive_keys):
                out.add("block_left_empty")
    if s == 32 and {"line_lo", "line_hi"} <= out and any(k >> 7 == U.EDGE_BASE >> 7 for k in alive_keys) and any(k >> 7 == (U.EDGE_BASE >> 7) + 1 for k in alive_keys):
        out.add("line_edge_with_neighbours")      # both lines at the edge keep a bit while losing one
    return out


@pytest.mark.parametrize("s", [8, 16, 32])
def test_the_data_makes_every_case_occur(s):
    """per substring width, over the databases and masks at the first shape of that width: a bucket loses its head, its tail, a
    middle entry; a bucket vanishes at key 0, at 2^s - 1 and between survivors; for s = 32 on both sides of a line edge and of a
    block edge, with a block left empty; a table where no bucket vanishes; K = 0, K = N, K = 1"""
    bits, m = next((b, mm) for b, mm in U.SHAPES if b // mm == s)
    seen, ks = set(), set()
    for db in R.DATABASES:
        keys = R.db_keys(bits, m, *db)
        for mk in R.MASKS:
            keep = R.mask(mk, keys, bits, m)
            K = int(keep.sum())
            ks.add("K=0" if K == 0 else "K=N" if K == len(keys) else "K=1" if K == 1 else "other")
            if 0 < K < len(keys):
                for t in range(m):
                    seen |= _situations(keys[:, t], keep, s)
            elif K == len(keys):
                seen.add("no_bucket_vanishes")
    want = {"head", "tail", "middle", "vanish_0", "vanish_top", "vanish_between", "no_bucket_vanishes"}
    if s == 32:
        want |= {"line_lo", "line_hi", "block_lo", "block_hi", "block_left_empty", "line_edge_with_neighbours"}
    assert want <= seen, sorted(want - seen)
    assert {"K=0", "K=N", "K=1", "other"} <= ks


def test_whole_buckets_removes_exactly_the_vanish_sets():
    for bits, m in ((64, 8), (64, 4), (64, 2), (128, 4)):
        keys = R.db_keys(bits, m, 300, 20000)
        keep = R.mask("whole_buckets", keys, bits, m)
        assert 0 < keep.sum() < len(keys)
        for t in range(m):
            gone = set(R.vanish_set(bits, m, t))
            assert gone <= set(keys[:, t].tolist()), (bits, m, t)                 # every such bucket existed
            assert not gone & set(keys[keep][:, t].tolist()), (bits, m, t)        # ... and is gone whole


def test_two_removals_compose():
    """two retains in a row are one with the composed mask (the GPU test's 'life goes on')"""
    bits, m, s = 64, 4, 16
    keys = R.db_keys(bits, m, 300, 20000)
    k1 = R.mask("sparse", keys, bits, m)
    k2 = R.mask("every_other", keys[k1], bits, m)
    both = k1.copy()
    both[np.nonzero(k1)[0][~k2]] = False
    tab = R.retain_model(R.retain_model(U.table_from_scratch(keys[:, 0], s), k1, s), k2, s)
    assert R.same_table(tab, U.table_from_scratch(keys[both][:, 0], s))


def test_abi_surface(vc):
    """the header declares the four entry points and the two kinds, the built library exports them, the bindings expose them"""
    header = open(os.path.join(ROOT, "include", "verticut_gpu.h")).read()
    for decl in (r"^int vc_retain_dev\(vc_engine\* e, const uint32_t\* d_sel, uint32_t kind, uint32_t\* d_new_ids, uint64_t\* n_kept, void\* stream\);",
                 r"^int vc_retain\(vc_engine\* e, const uint32_t\* sel, uint32_t kind, uint32_t\* new_ids, uint64_t\* n_kept\);",
                 r"^int vc_sharded_retain_dev\(vc_sharded\* h, const uint32_t\* d_sel, uint32_t kind, uint32_t\* d_new_ids, uint64_t\* n_kept, void\* stream\);",
                 r"^int vc_sharded_retain\(vc_sharded\* h, const uint32_t\* sel, uint32_t kind, uint32_t\* new_ids, uint64_t\* n_kept\);",
                 r"^#define VC_RETAIN_MASK  0u", r"^#define VC_RETAIN_ROOTS 1u"):
        assert re.search(decl, header, re.M), decl
    assert "#define VC_ABI_VERSION 2" in header
    lib = ctypes.CDLL(vc.LIB_PATH)
    names = ("vc_retain", "vc_retain_dev", "vc_sharded_retain", "vc_sharded_retain_dev")
    for name in names:
        assert getattr(lib, name)
    assert set(names) <= set(vc.EXPORTS)
    assert (vc.RETAIN_MASK, vc.RETAIN_ROOTS) == (0, 1)
    for cls in (vc.Engine, vc.ShardedEngine):
        assert callable(cls.retain) and callable(cls.retain_dev)
    host = open(os.path.join(ROOT, "verticut_amd", "host", "verticut_host.hpp")).read()
    assert host.count("int retain(const uint32_t* sel, uint32_t kind, uint32_t* new_ids, uint64_t* n_kept) override") == 2
    assert "virtual int retain(const uint32_t* sel, uint32_t kind, uint32_t* new_ids, uint64_t* n_kept) = 0;" in host


def test_new_kernels_use_no_scratch(vc):
    """the removal's kernels stream: none may spill or use scratch (the conditions test_build_cpu puts on the search kernels)"""
    from verticut_amd import build as vb
    res = {k: v for k, v in vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_retain.o")).items() if "retain_" in k}
    assert len(res) == 5, sorted(res)
    mih = {k: v for k, v in vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_mih.o")).items() if "mih_retain_" in k}
    assert len(mih) == 9 and sum("bent_kernel" in k for k in mih) == 2, sorted(mih)
    sh = {k: v for k, v in vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_sharded.o")).items() if "retain_" in k}
    assert len(sh) == 1, sorted(sh)
    for k, v in list(res.items()) + list(mih.items()) + list(sh.items()):
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
