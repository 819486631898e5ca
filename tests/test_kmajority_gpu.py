"""k-majority on the device: vc_kmajority, vc_kmajority_dev and their vc_sharded_* forms.

The expectation is assign_common.py's numpy model of the header's loop, whose update step is groups_common.model's centroid (both
pinned against plain loops, and the four crafted cases against what they are there for, by test_assign_cpu.py).  Centres, assignment,
labels and every field of the statistics are integers: every comparison is exact equality.  One device; N <= 4096."""
import ctypes as C

import numpy as np
import pytest

import assign_common as AC
import groups_common as GC

pytestmark = pytest.mark.gpu

STALE32 = 0xDEADBEEF


def _make(vc, monkeypatch, codes, id_base=0, shards=0, capacity=None, window=None, tile=None, slices=None):
    """the knobs are read when the handle is created"""
    for name, value in (("VC_GROUP_WINDOW", window), ("VC_ASSIGN_TILE", tile), ("VC_ASSIGN_SLICES", slices)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))
    bits, capacity = codes.shape[1] * 8, capacity or max(len(codes), 1)
    if shards:
        e = vc.ShardedEngine(bits, capacity=capacity, n_shards=shards, devices=[0], id_base=id_base)
    else:
        e = vc.Engine(bits, capacity=capacity, id_base=id_base)
    if len(codes):
        e.add_codes(codes)
    return e


def _upload(a, word):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).view(word).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _dev(store, seeds, max_iters, with_labels=True, stream=None):
    """the device form on stale-filled outputs: (centres, assign, labels | None, stats)"""
    import torch
    n, k = len(store), len(seeds)
    d_c = _upload(seeds, np.int64)
    d_a = _upload(np.full(n, AC.STALE, dtype=np.uint64), np.int64)
    d_l = _upload(np.full(n, STALE32, dtype=np.uint32), np.int32) if with_labels else None
    st = store.kmajority_dev(k, d_c.data_ptr(), d_a.data_ptr(), d_l.data_ptr() if with_labels else None, max_iters=max_iters, stream=stream)
    torch.cuda.synchronize()
    return (d_c.cpu().numpy().view(np.uint8).reshape(k, -1), d_a.cpu().numpy().view(np.uint64),
            d_l.cpu().numpy().view(np.uint32) if with_labels else None, st)


def _check_both_forms(store, seeds, want, max_iters=AC.MAX_ITERS, what=None):
    AC.same_run(store.kmajority(len(seeds), seeds=seeds, max_iters=max_iters), want, (what, "host form"))
    AC.same_run(_dev(store, seeds, max_iters), want, (what, "device form"))


# ---- 1. the four crafted cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("number", AC.CASES)
def test_the_crafted_cases(vc, monkeypatch, number):
    """converged runs with duplicate seeds and centres that stay empty (1, 2), the cap of 64 rounds (3), K = N (4)"""
    codes, seeds = AC.case(number)
    with _make(vc, monkeypatch, codes) as store:
        _check_both_forms(store, seeds, AC.case_expect(number), what=number)


@pytest.mark.parametrize("max_iters", [0, 1, 2, 64])
def test_max_iters(vc, monkeypatch, max_iters):
    codes, seeds = AC.case(1)
    want = AC.case_expect(1, max_iters)
    assert want[3]["n_iters"] == min(max_iters, 6) and want[3]["converged"] == (1 if max_iters == 64 else 0)
    with _make(vc, monkeypatch, codes) as store:
        _check_both_forms(store, seeds, want, max_iters, what=max_iters)
        got = _dev(store, seeds, max_iters, with_labels=False)              # labels are optional
        AC.same_run((got[0], got[1], want[2], got[3]), want, (max_iters, "no labels"))


def test_default_seeds_are_spread_evenly(vc, monkeypatch):
    codes = AC.case(1)[0]
    n, k = len(codes), 40
    ids = np.arange(k, dtype=np.int64) * n // k
    with _make(vc, monkeypatch, codes, id_base=7) as store:
        want = AC.kmajority_model(codes, codes[ids], id_base=7)
        AC.same_run(store.kmajority(k), want, "default seeds")
        AC.same_run(store.kmajority(k, seed_ids=ids + 7), want, "seed ids")
        assert np.array_equal(store.get_codes(ids + 7), codes[ids])


# ---- 2. the fixed point ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [0, 3])
def test_a_converged_run_is_a_fixed_point_of_the_pipeline(vc, monkeypatch, shards):
    codes, seeds = AC.case(1)
    id_base = 500
    with _make(vc, monkeypatch, codes, id_base=id_base, shards=shards, capacity=4099 if shards else None) as store:
        centres, assign, labels, st = store.kmajority(len(seeds), seeds=seeds)
        assert st["converged"] == 1 and st["n_empty"] == 1
        groups, cents, rep_labels, _ = store.group_summary(labels)
        assert len(groups) == len(seeds) - st["n_empty"]
        assert np.array_equal(cents, centres[groups["label"].astype(np.int64) - id_base])     # every non-empty centre IS its group's centroid
        assert np.array_equal(store.assign_nearest(centres), assign)
        assert st["cost_final"] == AC.dist_of(assign).sum() == st["cost"][st["n_iters"] - 1]
        kept, _ = store.retain(rep_labels, vc.RETAIN_ROOTS)
        assert kept == len(seeds) - st["n_empty"] == len(store)


# ---- 3. no layout changes a bit ------------------------------------------------------------------------------------------------------------
LAYOUTS = [dict(id_base=1000), dict(window=GC.SMALL_WINDOW), dict(tile=8, slices=3), dict(shards=2, capacity=4099), dict(shards=3, capacity=4099, id_base=1000),
           dict(shards=3, capacity=9000, window=GC.SMALL_WINDOW, tile=8, slices=3)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda d: "-".join("%s%s" % kv for kv in d.items()))
def test_layout_independence(vc, monkeypatch, layout):
    """id_base, windows of 2048 sorted positions in the update step, tiles of 8 centres in three slices in the assign step, two and
    three shards (boundaries off any multiple of 64; an empty trailing shard): all bit for bit the plain single-engine run, which
    test_the_crafted_cases holds to the same model"""
    codes, seeds = AC.case(2)
    id_base = layout.get("id_base", 0)
    plain = AC.case_expect(2)
    want = (plain[0], plain[1], (plain[2] + id_base).astype(np.uint32), plain[3])
    with _make(vc, monkeypatch, codes, **layout) as store:
        _check_both_forms(store, seeds, want, what=layout)


# ---- 4. errors and the empty store -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [0, 2])
def test_errors_leave_the_outputs_untouched(vc, monkeypatch, shards):
    bits, n, k = 64, 100, 5
    codes = GC.uniform_codes(n, bits, 11)
    L = vc.load_library()
    fn, fn_dev = (L.vc_sharded_kmajority, L.vc_sharded_kmajority_dev) if shards else (L.vc_kmajority, L.vc_kmajority_dev)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    with _make(vc, monkeypatch, codes, shards=shards) as store:
        big = GC.uniform_codes(n + 1, bits, 12)
        seeds, seeds0 = big.copy(), big.copy()
        assign, labels = np.full(n, AC.STALE, dtype=np.uint64), np.full(n, STALE32, dtype=np.uint32)
        st = vc.VcKmajorityStats()
        bad = [(None, k, 3, p(seeds), p(assign), p(labels)), (store._h, k, 3, None, p(assign), p(labels)), (store._h, k, 3, p(seeds), None, p(labels)),
               (store._h, 0, 3, p(seeds), p(assign), p(labels)), (store._h, n + 1, 3, p(seeds), p(assign), p(labels)),
               (store._h, k, 65, p(seeds), p(assign), p(labels))]
        for args in bad:
            assert fn(*args, C.byref(st)) == vc.VC_ERR_INVALID, args
            assert fn(*args, None) == vc.VC_ERR_INVALID, args
        d_c, d_a = _upload(seeds, np.int64), _upload(assign, np.int64)
        bad_dev = [(None, k, 3, d_c.data_ptr(), d_a.data_ptr(), None), (store._h, k, 3, None, d_a.data_ptr(), None), (store._h, k, 3, d_c.data_ptr(), None, None),
                   (store._h, 0, 3, d_c.data_ptr(), d_a.data_ptr(), None), (store._h, n + 1, 3, d_c.data_ptr(), d_a.data_ptr(), None),
                   (store._h, k, 65, d_c.data_ptr(), d_a.data_ptr(), None)]
        for args in bad_dev:
            assert fn_dev(*args, None, None) == vc.VC_ERR_INVALID, args
        import torch
        torch.cuda.synchronize()
        assert np.array_equal(seeds, seeds0) and np.all(assign == AC.STALE) and np.all(labels == STALE32)
        assert np.array_equal(d_c.cpu().numpy().view(np.uint8).reshape(n + 1, -1), seeds0) and np.all(d_a.cpu().numpy().view(np.uint64) == AC.STALE)
        with pytest.raises(vc.VcError):
            store.kmajority(k, seeds=seeds[:k], max_iters=65)
        AC.same_run(store.kmajority(n, seeds=codes), AC.kmajority_model(codes, codes), "K = N is legal")       # the handle still works


@pytest.mark.parametrize("shards", [0, 2])
def test_the_empty_store(vc, monkeypatch, shards):
    bits, k = 64, 3
    seeds = GC.uniform_codes(k, bits, 5)
    with _make(vc, monkeypatch, np.zeros((0, bits // 8), np.uint8), shards=shards, capacity=16) as store:
        centres, assign, labels, st = store.kmajority(k, seeds=seeds)
        assert np.array_equal(centres, seeds) and len(assign) == 0 and len(labels) == 0
        AC.same_stats(st, AC.zero_stats(), "N == 0")
        L = vc.load_library()
        raw = vc.VcKmajorityStats(n_iters=9, converged=9, n_empty=9)
        fn_dev = L.vc_sharded_kmajority_dev if shards else L.vc_kmajority_dev
        d_c = _upload(seeds, np.int64)
        assert fn_dev(store._h, k, 64, d_c.data_ptr(), d_c.data_ptr(), None, C.byref(raw), None) == vc.VC_OK     # (assign: any non-null address, never touched)
        AC.same_stats(raw.as_dict(), AC.zero_stats(), "N == 0, device form")
        assert np.array_equal(d_c.cpu().numpy().view(np.uint8).reshape(k, -1), seeds)
