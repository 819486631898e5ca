"""A built k-NN graph brought up to date after an append: vc_knn_graph_update* and its vc_sharded_* forms.

The expectations are knn_graph_common.model_rows over the whole store and the handle's own vc_knn_graph* from scratch; the statistics
of the join are those of knn_graph_update_common's windowed model, which test_knn_graph_update_cpu.py pins against model_rows.  Every
comparison is exact equality on every word; device outputs are pre-filled with a stale pattern behind the old rows, so every new word
is proven written and the words around an output proven untouched.  One device; N <= 9100.

Not tested: the sharded forms across real devices, the host form's second answer for new rows the linear scan passed on, and the
clause for the reference-fidelity flags."""
import ctypes as C

import numpy as np
import pytest

import knn_graph_common as KG
import knn_graph_update_common as KU

pytestmark = pytest.mark.gpu

PAD = 3          # stale words kept on both sides of every device output
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


def _append(store, codes):
    """add_codes and the index brought up to date (a store that was empty has no index to update)"""
    was = len(store)
    if len(codes):
        store.add_codes(codes)
    if len(store):
        store.build_index() if was == 0 else store.update_index()


def _to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    signed = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(a.view(signed).copy()).cuda()


def _staged(old, n, width, dtype):
    """a device buffer of PAD + n * width + PAD words: the old words first, stale words behind them and in the pads"""
    stale = KG.STALE if dtype == np.uint64 else KG.STALE32
    buf = np.full(n * width + 2 * PAD, stale, dtype=dtype)
    buf[PAD:PAD + old.size] = old.reshape(-1)
    return _to_dev(buf)


def _inner(buf, n_words, dtype, what):
    raw = buf.cpu().numpy().view(dtype)
    stale = KG.STALE if dtype == np.uint64 else KG.STALE32
    assert np.all(raw[:PAD] == stale) and np.all(raw[PAD + n_words:] == stale), (what, "words around the output")
    return raw[PAD:PAD + n_words]


def _update(store, k, old, mode, batch=0, k_first=0, with_counts=True, with_stats=True, stream=None):
    """the device form on the old graph `old` = (rows [n_old, k], counts [n_old]): (rows [N, k], counts [N] | None, stats | None)"""
    import torch
    n, n_old = len(store), len(old[0])
    d_r = _staged(old[0], max(n, 1), k, np.uint64)
    d_c = _staged(old[1], max(n, 1), 1, np.uint32) if with_counts else None
    torch.cuda.synchronize()
    st = store.knn_graph_update_dev(k, n_old, d_r.data_ptr() + 8 * PAD, d_c.data_ptr() + 4 * PAD if with_counts else None, mode=mode, batch=batch,
                                    k_first=k_first, with_stats=with_stats, stream=stream)
    torch.cuda.synchronize()
    rows = _inner(d_r, max(n, 1) * k, np.uint64, "rows").reshape(max(n, 1), k)[:n]
    return rows, _inner(d_c, max(n, 1), np.uint32, "counts")[:n] if with_counts else None, st


def _scratch(store, k, mode, first=0, k_first=0):
    """the handle's own vc_knn_graph_dev from scratch: (rows, counts, stats)"""
    import torch
    n = len(store) - first
    d_r, d_c = _staged(np.zeros(0, dtype=np.uint64), max(n, 1), k, np.uint64), _staged(np.zeros(0, dtype=np.uint32), max(n, 1), 1, np.uint32)
    st = store.knn_graph_dev(k, d_r.data_ptr() + 8 * PAD, d_c.data_ptr() + 4 * PAD, mode=mode, first=first, k_first=k_first)
    torch.cuda.synchronize()
    return d_r.cpu().numpy().view(np.uint64)[PAD:PAD + n * k].reshape(n, k), d_c.cpu().numpy().view(np.uint32)[PAD:PAD + n], st


def _join_stats(st):
    return {name: st[name] for name in KU.UPDATE_STATS}


@pytest.fixture(scope="module")
def planted64():
    """the shared references of the 64-bit planted case at id_base 0 and k = 10: the old graph, the graph of the whole store and the
    windowed model's statistics at the default knobs"""
    codes, n_old = KU.planted_case(64)
    old = KG.model_rows(codes[:n_old], 10)
    rows, counts, st = KU.update_model(codes, n_old, 10, old=old)
    want = KG.model_rows(codes, 10)
    KG.same_graph((rows, counts), want, "the model")
    for a in old + want:
        a.setflags(write=False)
    return codes, n_old, old, want, st


# ---- 1. widths and k ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10, 100])
@pytest.mark.parametrize("bits", [64, 128, 256, 512])
def test_rows_against_the_model_and_a_build_from_scratch(vc, monkeypatch, bits, k):
    """2000 clustered records and 200 planted ones, windows of 64: both modes give the words of the model and of vc_knn_graph_dev from
    scratch, the join's statistics are the windowed model's and the build's are those of vc_knn_graph_dev over the new range"""
    monkeypatch.setenv("VC_KGRAPH_WINDOW", "64")
    codes, n_old = KU.planted_case(bits)
    old = KG.model_rows(codes[:n_old], k)
    want = KG.model_rows(codes, k)
    _, _, model = KU.update_model(codes, n_old, k, window_knob=64, old=old)
    assert model["n_rows_changed"] > 0 and model["n_windows"] == 4
    with _make(vc, codes[:n_old], bits, capacity=len(codes)) as store:
        _append(store, codes[n_old:])
        for mode in MODES:
            got = _update(store, k, old, mode)
            KG.same_graph(got, want, (bits, k, mode))
            assert _join_stats(got[2]) == model, (bits, k, mode, got[2], model)
            scratch = _scratch(store, k, mode)
            KG.same_graph(got, scratch, (bits, k, mode, "scratch"))
            assert got[2]["build"] == _scratch(store, k, mode, first=n_old)[2], (bits, k, mode)


# ---- 2. the knobs at 64 bits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,old_batch", [(1, 0), (3, 0), (0, 0), (0, 100), (3, 100)])
def test_every_window_and_old_batch_gives_the_same_words(vc, monkeypatch, planted64, window, old_batch):
    codes, n_old, old, want, default = planted64
    if window:
        monkeypatch.setenv("VC_KGRAPH_WINDOW", str(window))
    if old_batch:
        monkeypatch.setenv("VC_KGRAPH_OLD_BATCH", str(old_batch))
    _, _, model = KU.update_model(codes, n_old, 10, window_knob=window, old_batch_knob=old_batch, old=old)
    assert (model["n_rows_changed"], model["n_inserted"]) == (default["n_rows_changed"], default["n_inserted"])
    with _make(vc, codes[:n_old], 64, capacity=len(codes)) as store:
        _append(store, codes[n_old:])
        for mode in MODES:
            got = _update(store, 10, old, mode)
            KG.same_graph(got, want, (window, old_batch, mode))
            assert _join_stats(got[2]) == model, (window, old_batch, mode, got[2], model)


def test_a_tight_scratch_budget_halves_the_windows(vc, monkeypatch):
    """VC_KGRAPH_SCRATCH=4096 with an append of duplicates of a dense cluster: the same words, n_rows_changed and n_inserted as with the
    default budget, and the halvings the mirror predicts; the merge runs in sub-batches of one row"""
    codes, n_old = KU.dense_case()
    k = KU.DENSE_K
    old = KG.model_rows(codes[:n_old], k)
    want = KG.model_rows(codes, k)
    _, _, tight = KU.update_model(codes, n_old, k, window_knob=KU.DENSE_WINDOW, budget=KU.DENSE_BUDGET, old=old)
    _, _, loose = KU.update_model(codes, n_old, k, window_knob=KU.DENSE_WINDOW, old=old)
    assert tight["n_halvings"] >= 2 and KU.merge_sub(KU.DENSE_BUDGET, k) == 1
    monkeypatch.setenv("VC_KGRAPH_WINDOW", str(KU.DENSE_WINDOW))
    for budget, model in ((None, loose), (KU.DENSE_BUDGET, tight)):
        if budget:
            monkeypatch.setenv("VC_KGRAPH_SCRATCH", str(budget))
        with _make(vc, codes[:n_old], 64, capacity=len(codes)) as store:
            _append(store, codes[n_old:])
            got = _update(store, k, old, KG.LINEAR)
            KG.same_graph(got, want, ("dense", budget))
            assert _join_stats(got[2]) == model, (budget, got[2], model)
    assert (tight["n_rows_changed"], tight["n_inserted"]) == (loose["n_rows_changed"], loose["n_inserted"])


# ---- 3. boundary sizes --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_old", [0, 1, 2, KU.CRAFT_K, KU.CRAFT_K + 1])
def test_small_old_stores(vc, n_old):
    """n_old in {0, 1, 2, k, k + 1}: rows that are not full fill up window by window; n_old == 0 is a plain build"""
    codes, k = KU.crafted_case()[0][30:50], KU.CRAFT_K
    old = KG.model_rows(codes[:n_old], k)
    want = KG.model_rows(codes, k)
    _, _, model = KU.update_model(codes, n_old, k, old=old)
    with _make(vc, codes[:n_old], 64, capacity=len(codes)) as store:
        _append(store, codes[n_old:])
        for mode in MODES:
            got = _update(store, k, old, mode)
            KG.same_graph(got, want, (n_old, mode))
            assert _join_stats(got[2]) == model, (n_old, mode, got[2], model)
            assert got[2]["build"]["n_searched"] >= len(codes) - n_old
            rows, counts, st = _update(store, k, old, mode, with_counts=False, with_stats=False)      # counts and stats may be NULL
            assert counts is None and st is None and np.array_equal(rows, want[0])


def test_nothing_appended_and_a_store_of_one(vc):
    codes, k = KU.crafted_case()[0][30:50], KU.CRAFT_K
    whole = KG.model_rows(codes, k)
    with _make(vc, codes, 64) as store:                                # n_old == N: VC_OK, zero stats, nothing written
        for mode in MODES:
            got = _update(store, k, whole, mode)
            KG.same_graph(got, whole, ("nothing appended", mode))
            assert got[2] == KU.zero_update_stats()
    with _make(vc, codes[:0], 64, capacity=4) as store:                # N = 1 out of nothing: a padded row, count 0
        _append(store, codes[:1])
        for mode in MODES:
            rows, counts, st = _update(store, 3, KG.model_rows(codes[:0], 3), mode)
            assert rows.shape == (1, 3) and np.all(rows == KG.INF) and counts.tolist() == [0] and _join_stats(st) == dict.fromkeys(KU.UPDATE_STATS, 0)
        one = KG.model_rows(codes[:1], 3)                                 # N = 1, n_old = 1: untouched
        rows, counts, st = _update(store, 3, one, KG.LINEAR)
        assert np.all(rows == KG.INF) and counts.tolist() == [0] and st == KU.zero_update_stats()


# ---- 4. duplicates and ties ---------------------------------------------------------------------------------------------------------------------
def test_the_duplicate_set_with_appended_copies(vc):
    """dup_case: 8300 copies of one code among 9000 records; 40 more copies, 20 codes one flip from it and 3 far ones are appended.  A
    copy's row is full at distance 0 with smaller ids, so the new copies tie it and lose; the near records' rows take them."""
    base, k = KG.dup_case(), KG.DUP_K
    copy = base[KG.dup_copies(base)[0]]
    extra = [copy] * 40 + [KG._flip(copy, [b]) for b in range(20)] + [copy ^ np.uint8(0xFF), KG._flip(copy ^ np.uint8(0xFF), [1]), KG._flip(copy, [1, 2, 3, 4, 5, 6])]
    codes = np.concatenate([base, np.array(extra, dtype=np.uint8)])
    want = KG.model_rows(codes, k)
    with _make(vc, base, 64, capacity=len(codes)) as store:
        old = _scratch(store, k, KG.LINEAR)[:2]
        _append(store, codes[len(base):])
        _, _, model = KU.update_model(codes, len(base), k, old=old)
        assert 0 < model["n_rows_changed"] < KG.DUP_N - KG.DUP_COPIES + 100 and model["n_hits"] > model["n_inserted"] > 0
        for mode, k_first in ((KG.LINEAR, 0), (KG.MIH_EXACT, KG.DUP_K_FIRST)):
            got = _update(store, k, old, mode, k_first=k_first)
            KG.same_graph(got, want, ("duplicates", mode))
            assert _join_stats(got[2]) == model, (mode, got[2], model)
        assert got[2]["build"]["n_linear"] >= 40                           # the new copies go to the linear scan under exact MIH


@pytest.mark.parametrize("window", [0, 3])
def test_the_crafted_set(vc, monkeypatch, window):
    """a row replaced entirely by more hits than it has places, a tie at a row's last distance that loses on its id, exact duplicates
    and rows without a hit (test_knn_graph_update_cpu.py shows that the set reaches them)"""
    if window:
        monkeypatch.setenv("VC_KGRAPH_WINDOW", str(window))
    codes, n_old, replaced, _ = KU.crafted_case()
    k = KU.CRAFT_K
    old = KG.model_rows(codes[:n_old], k)
    want = KG.model_rows(codes, k)
    _, _, model = KU.update_model(codes, n_old, k, window_knob=window, old=old)
    with _make(vc, codes[:n_old], 64, capacity=len(codes)) as store:
        _append(store, codes[n_old:])
        for mode in MODES:
            got = _update(store, k, old, mode)
            KG.same_graph(got, want, ("crafted", window, mode))
            assert _join_stats(got[2]) == model
            assert np.array_equal(got[0][replaced], np.arange(n_old, n_old + k).astype(np.uint64))


# ---- 5. a chain of appends ----------------------------------------------------------------------------------------------------------------------
def test_a_chain_of_appends_on_one_buffer(vc):
    """four appends of 1, 7, 300 and 64 records with update_index and the graph update after each, in one device buffer: every stage
    is a build from scratch, and vc_cluster_knn_dev labels on the updated graph are those on the scratch graph"""
    import torch
    codes, _ = KU.planted_case(64)
    k, n, total = 10, 1828, 2200
    assert n + 1 + 7 + 300 + 64 == total == len(codes)
    with _make(vc, codes[:n], 64, capacity=total) as store:
        d_r, d_c = _staged(np.zeros(0, dtype=np.uint64), total, k, np.uint64), _staged(np.zeros(0, dtype=np.uint32), total, 1, np.uint32)
        p_r, p_c = d_r.data_ptr() + 8 * PAD, d_c.data_ptr() + 4 * PAD
        store.knn_graph_dev(k, p_r, p_c, mode=KG.MIH_EXACT)
        for step in (1, 7, 300, 64):
            _append(store, codes[n:n + step])
            st = store.knn_graph_update_dev(k, n, p_r, p_c, mode=KG.MIH_EXACT)
            n += step
            torch.cuda.synchronize()
            got = (d_r.cpu().numpy().view(np.uint64)[PAD:PAD + n * k].reshape(n, k), d_c.cpu().numpy().view(np.uint32)[PAD:PAD + n])
            scratch = _scratch(store, k, KG.MIH_EXACT)
            KG.same_graph(got, scratch, ("chain", n))
            assert st["build"]["n_searched"] >= step and st["n_windows"] == 1
        KG.same_graph(got, KG.model_rows(codes, k), "chain, the model")
        _inner(d_r, total * k, np.uint64, "rows")
        _inner(d_c, total, np.uint32, "counts")
        labels = []
        for rows, counts in (got, scratch[:2]):
            d_l, d_rows, d_counts = _to_dev(np.zeros(total, dtype=np.uint32)), _to_dev(rows), _to_dev(counts)
            store.cluster_knn_dev(d_rows.data_ptr(), d_counts.data_ptr(), k, 4, d_l.data_ptr(), None)
            torch.cuda.synchronize()
            labels.append(d_l.cpu().numpy().view(np.uint32))
        assert np.array_equal(labels[0], labels[1]) and len(set(labels[0].tolist())) > 1


# ---- 6. one large k -----------------------------------------------------------------------------------------------------------------------------
def test_one_large_k(vc):
    codes, n_old = KU.planted_case(64, n=2500, planted=100)
    k = 1000
    old = KG.model_rows(codes[:n_old], k)
    want = KG.model_rows(codes, k)
    _, _, model = KU.update_model(codes, n_old, k, old=old)
    with _make(vc, codes[:n_old], 64, capacity=len(codes)) as store:
        _append(store, codes[n_old:])
        got = _update(store, k, old, KG.MIH_EXACT)
        KG.same_graph(got, want, "k = 1000")
        assert _join_stats(got[2]) == model and model["n_rows_changed"] > 1000


# ---- 7. handle and pointer variants -------------------------------------------------------------------------------------------------------------
def test_id_base_a_stream_a_warm_handle_and_the_host_form(vc, planted64):
    import torch
    codes, n_old, _, _, model = planted64
    id_base, k = 2 ** 32 - 5000, 10
    old = KG.model_rows(codes[:n_old], k, id_base=id_base)
    want = KG.model_rows(codes, k, id_base=id_base)
    with _make(vc, codes[:n_old], 64, id_base=id_base, capacity=len(codes)) as store:
        _append(store, codes[n_old:])
        for mode in MODES:
            got = _update(store, k, old, mode)
            KG.same_graph(got, want, ("id_base", mode))
            assert _join_stats(got[2]) == model
            rows, counts, st = _update(store, k, old, mode, with_counts=False, with_stats=False)      # NULL counts, NULL stats
            assert counts is None and st is None and np.array_equal(rows, want[0])
        side = torch.cuda.Stream()
        KG.same_graph(_update(store, k, old, KG.MIH_EXACT, stream=side.cuda_stream), want, "stream")
        # a warm handle: other calls in between, larger and smaller shapes, leave every word the same
        store.search_knn(codes[:33], 50, mode=KG.MIH_EXACT)
        _update(store, 100, KG.model_rows(codes[:n_old], 100, id_base=id_base), KG.LINEAR)
        store.cluster_radius(1, mode=KG.MIH_EXACT)
        _update(store, 1, KG.model_rows(codes[:n_old], 1, id_base=id_base), KG.MIH_EXACT, batch=5)
        for mode in MODES:
            got = _update(store, k, old, mode)
            KG.same_graph(got, want, ("warm", mode))
            assert _join_stats(got[2]) == model
        for mode in MODES:                                                                          # the host form
            rows, counts, st = store.knn_graph_update(old[0], old[1], mode=mode, with_stats=True)
            KG.same_graph((rows, counts), want, ("host", mode))
            assert _join_stats(st) == model
            rows, counts = store.knn_graph_update(old[0], None, mode=mode)
            assert counts is None and np.array_equal(rows, want[0])


def test_three_shards_and_an_append_across_a_shard_boundary(vc, planted64):
    codes, _, _, want, _ = planted64
    n_old, k, capacity = 1400, 10, len(codes) + 10
    assert n_old < 2 * (capacity // 3) < len(codes)                       # the append starts in the second shard and ends in the third
    old = KG.model_rows(codes[:n_old], k)
    _, _, model = KU.update_model(codes, n_old, k, old=old)
    with _make(vc, codes[:n_old], 64, shards=3, capacity=capacity) as store:
        _append(store, codes[n_old:])
        for mode in MODES:
            got = _update(store, k, old, mode, batch=500)
            KG.same_graph(got, want, ("sharded", mode))
            assert _join_stats(got[2]) == model
            rows, counts, st = store.knn_graph_update(old[0], old[1], mode=mode, with_stats=True)
            KG.same_graph((rows, counts), want, ("sharded host", mode))
            assert _join_stats(st) == model


# ---- 8. errors ----------------------------------------------------------------------------------------------------------------------------------
def test_every_error_leaves_the_outputs_untouched(vc, planted64):
    codes, _, _, _, _ = planted64
    with vc.Engine(64, capacity=400, n_tables=2) as store:
        store.add_codes(codes[:300])
        out, cnt = np.full((300, 10), KG.STALE, dtype=np.uint64), np.full(300, KG.STALE32, dtype=np.uint32)
        st = vc.VcKnnGraphUpdateStats()
        st.n_hits, st.build.k_last = 7, 7
        L, h, p = store._L, store._h, lambda a: a.ctypes.data
        bad = [
            (vc.VC_ERR_INVALID, (None, 10, KG.LINEAR, 0, 200, 0, p(out), p(cnt))),                   # a null handle
            (vc.VC_ERR_INVALID, (h, 10, KG.LINEAR, 0, 200, 0, None, p(cnt))),                        # null rows
            (vc.VC_ERR_INVALID, (h, 0, KG.LINEAR, 0, 200, 0, p(out), p(cnt))),                       # k out of range
            (vc.VC_ERR_INVALID, (h, KG.MAX_K, KG.LINEAR, 0, 200, 0, p(out), p(cnt))),
            (vc.VC_ERR_INVALID, (h, 10, KG.LINEAR, 0, 200, 10, p(out), p(cnt))),                     # a bad k_first
            (vc.VC_ERR_INVALID, (h, 10, KG.LINEAR, 0, 200, KG.MAX_K + 1, p(out), p(cnt))),
            (vc.VC_ERR_INVALID, (h, 10, KG.MIH_APPROX, 0, 200, 0, p(out), p(cnt))),                  # a refused mode
            (vc.VC_ERR_INVALID, (h, 10, 3, 0, 200, 0, p(out), p(cnt))),
            (vc.VC_ERR_INVALID, (h, 10, KG.LINEAR, 0, 301, 0, p(out), p(cnt))),                      # n_old > N
            (vc.VC_ERR_STATE, (h, 10, KG.MIH_EXACT, 0, 200, 0, p(out), p(cnt))),                      # MIH without an index
        ]
        for want, args in bad:
            assert L.vc_knn_graph_update(*args, C.byref(st)) == want, args
            assert np.all(out == KG.STALE) and np.all(cnt == KG.STALE32) and st.n_hits == 7 and st.build.k_last == 7
        store.build_index()
        store.add_codes(codes[300:310])                                                              # a stale index counts as none
        out, cnt = np.full((310, 10), KG.STALE, dtype=np.uint64), np.full(310, KG.STALE32, dtype=np.uint32)
        assert L.vc_knn_graph_update(h, 10, KG.MIH_EXACT, 0, 300, 0, p(out), p(cnt), C.byref(st)) == vc.VC_ERR_STATE
        assert np.all(out == KG.STALE) and st.n_hits == 7
    with vc.ShardedEngine(64, capacity=60, n_shards=3, devices=[0], n_tables=2) as store:
        store.add_codes(codes[:50])
        out = np.full((50, 4), KG.STALE, dtype=np.uint64)
        for mode, k, n_old, want in ((KG.MIH_EXACT, 4, 40, vc.VC_ERR_STATE), (KG.MIH_APPROX, 4, 40, vc.VC_ERR_INVALID), (KG.LINEAR, 0, 40, vc.VC_ERR_INVALID),
                                     (KG.LINEAR, 4, 51, vc.VC_ERR_INVALID)):
            assert store._L.vc_sharded_knn_graph_update(store._h, k, mode, 0, n_old, 0, out.ctypes.data, None, None) == want
            assert np.all(out == KG.STALE)


def test_a_corrupted_old_count_is_refused(vc, planted64):
    codes, n_old, old, want, _ = planted64
    with _make(vc, codes[:n_old], 64, capacity=len(codes)) as store:
        _append(store, codes[n_old:])
        for at, value in ((700, 11), (0, 0xFFFFFFFF), (n_old - 1, 0x80000000)):
            broken = old[1].copy()
            broken[at] = value
            with pytest.raises(vc.VcError) as err:
                _update(store, 10, (old[0], broken), KG.LINEAR)
            assert err.value.code == vc.VC_ERR_INVALID
        KG.same_graph(_update(store, 10, old, KG.LINEAR), want, "after the refusals")
