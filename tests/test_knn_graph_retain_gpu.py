"""A built k-NN graph brought up to date after a removal: vc_knn_graph_retain* and its vc_sharded_* forms.

Every case checks all K rows and counts against knn_graph_retain_common's model (which test_knn_graph_retain_cpu.py pins against
knn_graph_common.model_rows over the survivors) AND against vc_knn_graph* on a fresh handle that holds the survivors; the statistics
are the model's and, for the repair, the plan mirror's over the short rows.  Every comparison is exact equality on every word; the
device buffers carry stale words on both sides, which must be intact afterwards.  One device; N <= 2016.

Not tested: the sharded forms across real devices, the host form's second answer for repaired rows the linear scan passed on, and the
clause for the reference-fidelity flags."""
import ctypes as C

import numpy as np
import pytest

import knn_graph_common as KG
import knn_graph_retain_common as KR
import knn_graph_update_common as KU

pytestmark = pytest.mark.gpu

PAD = 3          # stale words kept on both sides of every device buffer
MODES = (KG.LINEAR, KG.MIH_EXACT)


def _make(vc, codes, bits, id_base=0, shards=0, capacity=None):
    capacity = capacity or max(len(codes), 1)
    if shards:
        e = vc.ShardedEngine(bits, capacity=capacity, n_shards=shards, devices=[0], id_base=id_base, n_tables=KG.TABLES[bits])
    else:
        e = vc.Engine(bits, capacity=capacity, id_base=id_base, n_tables=KG.TABLES[bits])
    if len(codes):
        e.add_codes(codes)
        e.build_index()
    return e


def _to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    signed = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(a.view(signed).copy()).cuda()


def _staged(words, dtype):
    """a device buffer of PAD + len(words) + PAD words with stale words in the pads"""
    stale = KG.STALE if dtype == np.uint64 else KG.STALE32
    buf = np.full(words.size + 2 * PAD, stale, dtype=dtype)
    buf[PAD:PAD + words.size] = words.reshape(-1)
    return _to_dev(buf)


def _inner(buf, n_words, dtype, what):
    raw = buf.cpu().numpy().view(dtype)
    stale = KG.STALE if dtype == np.uint64 else KG.STALE32
    assert np.all(raw[:PAD] == stale) and np.all(raw[PAD + n_words:] == stale), (what, "words around the buffer")
    return raw[PAD:PAD + n_words]


def _call(store, k, old, new_ids, mode, batch=0, k_first=0, with_counts=True, with_stats=True, stream=None):
    """the device form on the old graph `old` = (rows [n_old, k], counts [n_old]) and the map: (rows [K, k], counts [K] | None, stats | None)"""
    import torch
    K, n_old = len(store), len(new_ids)
    d_r, d_m = _staged(old[0], np.uint64), _staged(new_ids, np.uint32)
    d_c = _staged(old[1], np.uint32) if with_counts else None
    torch.cuda.synchronize()
    st = store.knn_graph_retain_dev(k, n_old, d_m.data_ptr() + 4 * PAD, d_r.data_ptr() + 8 * PAD, d_c.data_ptr() + 4 * PAD if with_counts else None, mode=mode,
                                    batch=batch, k_first=k_first, with_stats=with_stats, stream=stream)
    torch.cuda.synchronize()
    assert np.array_equal(_inner(d_m, n_old, np.uint32, "map"), new_ids)                                # the map is only read
    rows = _inner(d_r, n_old * k, np.uint64, "rows").reshape(n_old, k)[:K]
    return rows, _inner(d_c, n_old, np.uint32, "counts")[:K] if with_counts else None, st


def _scratch(store, k, mode, k_first=0):
    """the handle's own vc_knn_graph_dev from scratch: (rows, counts)"""
    import torch
    n = len(store)
    d_r, d_c = _staged(np.zeros(max(n, 1) * k, dtype=np.uint64), np.uint64), _staged(np.zeros(max(n, 1), dtype=np.uint32), np.uint32)
    store.knn_graph_dev(k, d_r.data_ptr() + 8 * PAD, d_c.data_ptr() + 4 * PAD, mode=mode, k_first=k_first)
    torch.cuda.synchronize()
    return _inner(d_r, max(n, 1) * k, np.uint64, "rows").reshape(max(n, 1), k)[:n], _inner(d_c, max(n, 1), np.uint32, "counts")[:n]


class _Case:
    """a store of `codes` with the records keep == 0 removed by vc_retain, the old graph and the model's expectation"""

    def __init__(self, vc, codes, keep, bits, k, id_base=0, shards=0, capacity=None):
        self.vc, self.codes, self.keep, self.bits, self.k, self.id_base = vc, codes, np.asarray(keep, dtype=bool), bits, k, id_base
        self.old = KG.model_rows(codes, k, id_base)
        self.rows, self.counts, self.stats, self.short = KR.retain_model(codes, self.keep, k, id_base, old=self.old)
        self.store = _make(vc, codes, bits, id_base=id_base, shards=shards, capacity=capacity)
        kept, self.new_ids = self.store.retain(self.keep.astype(np.uint32))
        assert kept == int(self.keep.sum()) == len(self.store) and np.array_equal(self.new_ids, KR.retain_map(self.keep, id_base))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.store.close()

    def want_stats(self, mode, k_first=0):
        return dict(repair=KR.repair_stats(self.codes, self.keep, self.short, self.k, k_first, mode == KG.LINEAR), **self.stats)

    def check(self, mode, what=None, **kw):
        got = _call(self.store, self.k, self.old, self.new_ids, mode, **kw)
        KG.same_graph(got, (self.rows, self.counts), (what, mode, "the model"))
        want = self.want_stats(mode, kw.get("k_first", 0))
        assert got[2] == want, (what, mode, got[2], want)
        return got

    def check_fresh(self, what=None):
        """vc_knn_graph* on a fresh handle that holds the survivors writes the same words"""
        with _make(self.vc, self.codes[self.keep], self.bits, id_base=self.id_base) as fresh:
            for mode in MODES:
                KG.same_graph((self.rows, self.counts), _scratch(fresh, self.k, mode), (what, mode, "a fresh handle"))


def _verify(vc, codes, keep, bits, k, what=None, **kw):
    with _Case(vc, codes, keep, bits, k, **kw) as case:
        for mode in MODES:
            case.check(mode, what)
        case.check_fresh(what)
        return case.stats


# ---- 1. widths and k ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10, 100])
@pytest.mark.parametrize("bits", [64, 128, 256, 512])
def test_rows_against_the_model_and_a_fresh_handle(vc, bits, k):
    """2000 clustered records, 10 % removed at random: both modes give the words of the model and of vc_knn_graph_dev on a fresh handle"""
    codes = KG.clustered_case(bits)
    st = _verify(vc, codes, KR.random_keep(len(codes), 0.1), bits, k, (bits, k))
    assert st["n_rows_kept"] == 1800 and 0 < st["n_rows_short"] and st["n_entries_dropped"] > 0


@pytest.mark.parametrize("k", [2, 3, 16, 17, 32, 33, 63, 64, 65, 129])
def test_every_rows_per_wave_boundary_and_the_chunk_loop(vc, k):
    codes = KG.clustered_case(64)
    st = _verify(vc, codes, KR.random_keep(len(codes), 0.1, seed=k), 64, k, k)
    assert 0 < st["n_rows_short"] <= st["n_rows_kept"] == 1800


def test_one_large_k_on_the_dense_set_with_a_cluster_removed(vc):
    codes, keep = KR.dense_cluster_keep()
    st = _verify(vc, codes, keep, 64, KU.DENSE_K, "dense")
    assert st["n_rows_short"] > 100


# ---- 2. the knobs -------------------------------------------------------------------------------------------------------------------------------
def test_every_batch_and_k_first_gives_the_same_words(vc):
    """1 % removed at k = 10: short and untouched rows side by side (test_knn_graph_retain_cpu.py shows it)"""
    codes = KG.clustered_case(64)
    with _Case(vc, codes, KR.random_keep(len(codes), 0.01), 64, 10) as case:
        assert 0 < case.stats["n_rows_short"] < case.stats["n_rows_kept"]
        for batch in (1, 7, 0):
            for k_first in (12, 0):
                case.check(KG.MIH_EXACT, (batch, k_first), batch=batch, k_first=k_first)
            case.check(KG.LINEAR, batch, batch=batch)
        case.check_fresh("knobs")


@pytest.mark.parametrize("budget", [1, 100, 4096])
def test_a_tight_scratch_budget_gives_the_same_words(vc, monkeypatch, budget):
    """VC_KGRAPH_SCRATCH below one row: the old rows go chunk by chunk of one row (51 at 4096 bytes), and the repair's rounds run in
    sub-batches of one row (23)"""
    monkeypatch.setenv("VC_KGRAPH_SCRATCH", str(budget))
    codes = KG.clustered_case(64, n=600)
    k = 10
    assert KR.chunk_rows(budget, k, 600) == (1 if budget < 160 else 51) and KG.sub_batch(budget, KG.first_k(k, 0, False)) == (1 if budget < 352 else 23)
    st = _verify(vc, codes, KR.random_keep(len(codes), 0.1), 64, k, budget)
    assert st["n_rows_short"] > 10


# ---- 3. removal patterns on the crafted set -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cluster", "tie", "first", "last", "alternate"])
def test_the_crafted_patterns(vc, name):
    codes, keep = KR.crafted_codes(), KR.crafted_patterns()[name]
    st = _verify(vc, codes, keep, 64, KR.CRAFT_K, name)
    if name == "cluster":                      # the lone rows stay untouched: nothing is short, nothing is searched
        assert st == dict(n_rows_kept=KR.CRAFT_LONE, n_rows_short=0, n_entries_dropped=0)
    elif name == "last":                       # no row lists the member of largest id: the rows only move
        assert st == dict(n_rows_kept=KR.CRAFT_N - 1, n_rows_short=0, n_entries_dropped=0)
    else:
        assert st["n_rows_short"] > 0


# ---- 4. small stores ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, KR.CRAFT_K, KR.CRAFT_K + 1, KR.CRAFT_K + 2])
def test_small_stores(vc, K):
    codes, k = KR.crafted_codes()[30:50], KR.CRAFT_K
    keep = np.zeros(len(codes), dtype=bool)
    keep[np.random.default_rng(K).choice(len(codes), size=K, replace=False)] = True
    with _Case(vc, codes, keep, 64, k) as case:
        for mode in MODES:
            rows, counts, st = case.check(mode, K)
            assert np.all(counts == min(k, K - 1))
            if K == 1:
                assert np.all(rows == KG.INF) and counts.tolist() == [0] and st["n_rows_short"] == 0
            rows, counts, st = _call(case.store, k, case.old, case.new_ids, mode, with_counts=False, with_stats=False)   # NULL counts, NULL stats
            assert counts is None and st is None and np.array_equal(rows, case.rows)
        case.check_fresh(K)


def test_rows_that_held_the_whole_store_are_not_searched_and_nothing_removed_writes_nothing(vc):
    codes, k = KR.crafted_codes()[30:35], KR.CRAFT_K
    with _Case(vc, codes, np.array([1, 0, 1, 1, 0], dtype=bool), 64, k) as case:                         # n_old - 1 < k
        for mode in MODES:
            rows, counts, st = case.check(mode, "whole store")
            assert st["n_rows_short"] == 0 and st["repair"]["n_searched"] == 0 and st["n_entries_dropped"] == 6
        case.check_fresh("whole store")
    with _Case(vc, codes, np.ones(5, dtype=bool), 64, k) as case:                                        # K == n_old: VC_OK, nothing written
        stale = (np.full((5, k), KG.STALE, dtype=np.uint64), np.full(5, KG.STALE32, dtype=np.uint32))
        for mode in MODES:
            rows, counts, st = _call(case.store, k, stale, case.new_ids, mode)
            assert np.all(rows == KG.STALE) and np.all(counts == KG.STALE32) and st == KR.zero_retain_stats(kept=5)
    with _Case(vc, codes, np.zeros(5, dtype=bool), 64, k) as case:                                       # K == 0: VC_OK, nothing written
        import torch
        d_r, d_m = _staged(stale[0], np.uint64), _staged(case.new_ids, np.uint32)
        st = case.store.knn_graph_retain_dev(k, 5, d_m.data_ptr() + 4 * PAD, d_r.data_ptr() + 8 * PAD, None, mode=KG.LINEAR)
        torch.cuda.synchronize()
        assert np.all(d_r.cpu().numpy().view(np.uint64) == KG.STALE) and st == KR.zero_retain_stats()


# ---- 5. a chain on one buffer -------------------------------------------------------------------------------------------------------------------
def test_a_chain_of_appends_and_removals_on_one_buffer(vc):
    """build, append + update, retain + this call, append + update again, in one device buffer: every stage is a build from scratch"""
    import torch
    codes, _ = KU.planted_case(64)
    k, n, total = 10, 1800, 2200
    with _make(vc, codes[:n], 64, capacity=total) as store:
        d_r, d_c = _staged(np.zeros(total * k, dtype=np.uint64), np.uint64), _staged(np.zeros(total, dtype=np.uint32), np.uint32)
        d_m = _staged(np.zeros(total, dtype=np.uint32), np.uint32)
        p_r, p_c, p_m = d_r.data_ptr() + 8 * PAD, d_c.data_ptr() + 4 * PAD, d_m.data_ptr() + 4 * PAD

        def stage(what):
            torch.cuda.synchronize()
            n_now = len(store)
            got = (_inner(d_r, total * k, np.uint64, "rows").reshape(total, k)[:n_now], _inner(d_c, total, np.uint32, "counts")[:n_now])
            KG.same_graph(got, _scratch(store, k, KG.MIH_EXACT), ("chain", what))
            return got

        store.knn_graph_dev(k, p_r, p_c, mode=KG.MIH_EXACT)
        stage("build")
        store.add_codes(codes[n:n + 200])
        store.update_index()
        store.knn_graph_update_dev(k, n, p_r, p_c, mode=KG.MIH_EXACT)
        stage("append")
        keep = KR.random_keep(2000, 0.05, seed=9)
        d_sel = _to_dev(keep.astype(np.uint32))
        kept = store.retain_dev(d_sel.data_ptr(), d_new_ids=p_m)
        st = store.knn_graph_retain_dev(k, 2000, p_m, p_r, p_c, mode=KG.MIH_EXACT)
        assert kept == 1900 == st["n_rows_kept"] and 0 < st["n_rows_short"] < 1900
        got = stage("retain")
        survivors = codes[:2000][keep]
        KG.same_graph(got, KG.model_rows(survivors, k), "chain, the model")
        store.add_codes(codes[2000:2200])
        store.update_index()
        store.knn_graph_update_dev(k, 1900, p_r, p_c, mode=KG.MIH_EXACT)
        got = stage("append again")
        KG.same_graph(got, KG.model_rows(np.concatenate([survivors, codes[2000:2200]]), k), "chain, the model at the end")
        _inner(d_m, total, np.uint32, "map")


# ---- 6. handle and pointer variants -------------------------------------------------------------------------------------------------------------
def test_id_base_a_stream_a_warm_handle_and_the_host_form(vc):
    import torch
    codes = KG.clustered_case(64)
    id_base, k = 2 ** 32 - 5000, 10
    with _Case(vc, codes, KR.random_keep(len(codes), 0.1), 64, k, id_base=id_base) as case:
        store, want = case.store, (case.rows, case.counts)
        for mode in MODES:
            case.check(mode, "id_base")
            rows, counts, st = _call(store, k, case.old, case.new_ids, mode, with_counts=False, with_stats=False)      # NULL counts, NULL stats
            assert counts is None and st is None and np.array_equal(rows, want[0])
        case.check_fresh("id_base")
        side = torch.cuda.Stream()
        case.check(KG.MIH_EXACT, "stream", stream=side.cuda_stream)
        # a warm handle: other calls in between, larger and smaller shapes, leave every word the same
        store.search_knn(codes[:33], 50, mode=KG.MIH_EXACT)
        _call(store, 100, KG.model_rows(codes, 100, id_base), case.new_ids, KG.LINEAR)
        store.cluster_radius(1, mode=KG.MIH_EXACT)
        _call(store, 1, KG.model_rows(codes, 1, id_base), case.new_ids, KG.MIH_EXACT, batch=5)
        for mode in MODES:
            case.check(mode, "warm")
            case.check(mode, "warm, twice")
        for mode in MODES:                                                                                          # the host form
            rows, counts, st = store.knn_graph_retain(case.old[0], case.new_ids, case.old[1], mode=mode, with_stats=True)
            KG.same_graph((rows, counts), want, ("host", mode))
            assert st == case.want_stats(mode)
            rows, counts = store.knn_graph_retain(case.old[0], case.new_ids, None, mode=mode)
            assert counts is None and np.array_equal(rows, want[0])


def test_three_shards_and_a_removal_across_a_shard_boundary(vc):
    codes, k, capacity = KG.clustered_case(64), 10, 2010
    keep = KR.random_keep(len(codes), 0.1)
    keep[100:400] = False                                                     # 300 records leave the first shard: the others move forward across both boundaries
    assert int(keep[:capacity // 3].sum()) < capacity // 3 - 250
    with _Case(vc, codes, keep, 64, k, shards=3, capacity=capacity) as case, _Case(vc, codes, keep, 64, k) as single:
        for mode in MODES:
            got = case.check(mode, "sharded", batch=500)
            one = single.check(mode, "single", batch=500)
            assert np.array_equal(got[0], one[0]) and np.array_equal(got[1], one[1]) and got[2] == one[2]
            rows, counts, st = case.store.knn_graph_retain(case.old[0], case.new_ids, case.old[1], mode=mode, with_stats=True)
            KG.same_graph((rows, counts), one, ("sharded host", mode))
            assert st == case.want_stats(mode)
        case.check_fresh("sharded")


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------------------------
def test_every_error_leaves_the_outputs_untouched(vc):
    codes = KG.clustered_case(64)
    with vc.Engine(64, capacity=400, n_tables=2) as store:
        store.add_codes(codes[:300])
        kept, new_ids = store.retain(KR.random_keep(300, 0.1).astype(np.uint32))
        assert kept == 270
        out, cnt = np.full((300, 10), KG.STALE, dtype=np.uint64), np.full(300, KG.STALE32, dtype=np.uint32)
        st = vc.VcKnnGraphRetainStats()
        st.n_rows_short, st.repair.k_last = 7, 7
        L, h, p = store._L, store._h, lambda a: a.ctypes.data
        bad = [
            (vc.VC_ERR_INVALID, (None, 10, KG.LINEAR, 0, 300, 0, p(new_ids), p(out), p(cnt))),                # a null handle
            (vc.VC_ERR_INVALID, (h, 10, KG.LINEAR, 0, 300, 0, p(new_ids), None, p(cnt))),                     # null rows
            (vc.VC_ERR_INVALID, (h, 10, KG.LINEAR, 0, 300, 0, None, p(out), p(cnt))),                         # a null map
            (vc.VC_ERR_INVALID, (h, 0, KG.LINEAR, 0, 300, 0, p(new_ids), p(out), p(cnt))),                    # k out of range
            (vc.VC_ERR_INVALID, (h, KG.MAX_K, KG.LINEAR, 0, 300, 0, p(new_ids), p(out), p(cnt))),
            (vc.VC_ERR_INVALID, (h, 10, KG.LINEAR, 0, 300, 10, p(new_ids), p(out), p(cnt))),                  # a bad k_first
            (vc.VC_ERR_INVALID, (h, 10, KG.LINEAR, 0, 300, KG.MAX_K + 1, p(new_ids), p(out), p(cnt))),
            (vc.VC_ERR_INVALID, (h, 10, KG.MIH_APPROX, 0, 300, 0, p(new_ids), p(out), p(cnt))),               # a refused mode
            (vc.VC_ERR_INVALID, (h, 10, 3, 0, 300, 0, p(new_ids), p(out), p(cnt))),
            (vc.VC_ERR_INVALID, (h, 10, KG.LINEAR, 0, 269, 0, p(new_ids), p(out), p(cnt))),                   # n_old < vc_size
            (vc.VC_ERR_STATE, (h, 10, KG.MIH_EXACT, 0, 300, 0, p(new_ids), p(out), p(cnt))),                   # MIH without an index
        ]
        for want, args in bad:
            assert L.vc_knn_graph_retain(*args, C.byref(st)) == want, args
            assert np.all(out == KG.STALE) and np.all(cnt == KG.STALE32) and st.n_rows_short == 7 and st.repair.k_last == 7
    with vc.ShardedEngine(64, capacity=60, n_shards=3, devices=[0], n_tables=2) as store:
        store.add_codes(codes[:50])
        kept, new_ids = store.retain(KR.random_keep(50, 0.2).astype(np.uint32))
        out = np.full((50, 4), KG.STALE, dtype=np.uint64)
        for mode, k, n_old, want in ((KG.MIH_EXACT, 4, 50, vc.VC_ERR_STATE), (KG.MIH_APPROX, 4, 50, vc.VC_ERR_INVALID), (KG.LINEAR, 0, 50, vc.VC_ERR_INVALID),
                                     (KG.LINEAR, 4, 39, vc.VC_ERR_INVALID)):
            assert store._L.vc_sharded_knn_graph_retain(store._h, k, mode, 0, n_old, 0, new_ids.ctypes.data, out.ctypes.data, None, None) == want
            assert np.all(out == KG.STALE)
        assert store._L.vc_sharded_knn_graph_retain(store._h, 4, KG.LINEAR, 0, 50, 0, None, out.ctypes.data, None, None) == vc.VC_ERR_INVALID


def test_a_corrupted_graph_or_map_is_refused_on_the_device(vc):
    codes, k = KG.clustered_case(64, n=600), 10
    with _Case(vc, codes, KR.random_keep(600, 0.1), 64, k) as case:
        store, old, new_ids = case.store, case.old, case.new_ids
        live = np.nonzero(case.keep)[0]

        def refused(rows, counts, ids):
            with pytest.raises(vc.VcError) as err:
                _call(store, k, (rows, counts), ids, KG.LINEAR)
            assert err.value.code == vc.VC_ERR_INVALID

        for at, value in ((int(live[100]), 11), (int(live[0]), 0xFFFFFFFF), (int(live[-1]), 0x80000000)):    # an old count above k
            broken = old[1].copy()
            broken[at] = value
            refused(old[0], broken, new_ids)
        for value in (600, 0xFFFFFFFE, 0x7FFFFFFF00000000 | 600):                                            # an entry outside the old store
            broken = old[0].copy()
            broken[int(live[50]), 3] = np.uint64(value)
            refused(broken, old[1], new_ids)
        broken = new_ids.copy()                                                                             # a live word altered
        broken[int(live[7])] += 1
        refused(old[0], old[1], broken)
        broken = new_ids.copy()
        broken[int(live[7])], broken[int(live[8])] = broken[int(live[8])], broken[int(live[7])]
        refused(old[0], old[1], broken)
        broken = new_ids.copy()                                                                             # the wrong live count: one too few ...
        broken[int(live[-1])] = KR.DEAD
        refused(old[0], old[1], broken)
        broken = new_ids.copy()                                                                             # ... and one too many
        broken[int(np.nonzero(~case.keep)[0][0])] = 0
        refused(old[0], old[1], broken)
        for mode in MODES:
            case.check(mode, "after the refusals")
