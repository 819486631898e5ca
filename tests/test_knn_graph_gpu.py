"""The exact k-NN graph of the store and its analysis: vc_knn_graph*, vc_cluster_knn* and their vc_sharded_* forms.

The expectation is knn_graph_common.py's numpy model -- brute-force rows by (dist, id), edge sets as Python sets, a host union-find and
the plan mirror for the statistics -- pinned against plain loops by test_knn_graph_cpu.py, which also shows that the crafted inputs
reach what they are there for.  Rows, counts, labels, in-degrees and statistics are integer functions of the database and the call, so
every comparison is exact equality on every word; device outputs are pre-filled with a stale pattern, so every word is proven
written and the words around an output proven untouched.  One device; N <= 9000.

Not tested: the sharded forms across real devices, the host form's second answer for rows the linear scan passed on (its
ring-overflow recovery has to give up first), and the clause for the reference-fidelity flags."""
import numpy as np
import pytest

import knn_graph_common as KG

pytestmark = pytest.mark.gpu

PAD = 3          # stale words kept on both sides of every device output


def _make(vc, codes, id_base=0, shards=0, capacity=None, index=True, bits=None):
    bits = bits or codes.shape[1] * 8
    capacity = capacity or max(len(codes), 1)
    if shards:
        e = vc.ShardedEngine(bits, capacity=capacity, n_shards=shards, devices=[0], id_base=id_base, n_tables=KG.TABLES[bits])
    else:
        e = vc.Engine(bits, capacity=capacity, id_base=id_base, n_tables=KG.TABLES[bits])
    if len(codes):
        e.add_codes(codes)
        if index:
            e.build_index()
    return e


def _to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    signed = {1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(a.view(signed).copy()).cuda()


def _stale(n_words, dtype):
    return _to_dev(np.full(n_words + 2 * PAD, KG.STALE if dtype == np.uint64 else KG.STALE32, dtype=dtype))


def _inner(buf, n_words, dtype, what):
    """the n_words words between the pads of a synchronised buffer; the pads must still be stale"""
    raw = buf.cpu().numpy().view(dtype)
    stale = KG.STALE if dtype == np.uint64 else KG.STALE32
    assert np.all(raw[:PAD] == stale) and np.all(raw[PAD + n_words:] == stale), (what, "words around the output")
    return raw[PAD:PAD + n_words]


def _graph(store, k, mode, batch=0, first=0, count=0, k_first=0, with_counts=True, with_stats=True, stream=None):
    """the device form on stale-filled outputs: (rows, counts | None, stats | None)"""
    import torch
    n = (count or len(store) - first)
    d_r, d_c = _stale(n * k, np.uint64), _stale(n, np.uint32) if with_counts else None
    torch.cuda.synchronize()
    st = store.knn_graph_dev(k, d_r.data_ptr() + 8 * PAD, d_c.data_ptr() + 4 * PAD if with_counts else None, mode=mode, batch=batch, first=first,
                             count=count, k_first=k_first, with_stats=with_stats, stream=stream)
    torch.cuda.synchronize()
    return _inner(d_r, n * k, np.uint64, "rows").reshape(n, k), _inner(d_c, n, np.uint32, "counts") if with_counts else None, st


def _cluster(store, rows, counts, kk, flags=KG.MUTUAL, max_dist=0xFFFFFFFF, with_degree=True):
    """vc_cluster_knn_dev on stale-filled outputs: (labels, in_degree | None, stats)"""
    import torch
    n, k = rows.shape
    d_r, d_c = _to_dev(rows), _to_dev(counts) if counts is not None else None
    d_l, d_d = _stale(n, np.uint32), _stale(n, np.uint32) if with_degree else None
    torch.cuda.synchronize()
    st = store.cluster_knn_dev(d_r.data_ptr(), d_c.data_ptr() if counts is not None else None, k, kk, d_l.data_ptr() + 4 * PAD,
                               d_d.data_ptr() + 4 * PAD if with_degree else None, flags=flags, max_dist=max_dist)
    torch.cuda.synchronize()
    return _inner(d_l, n, np.uint32, "labels"), _inner(d_d, n, np.uint32, "in-degrees") if with_degree else None, st


def _same_cluster(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "labels", np.nonzero(got[0] != want[0])[0][:8])
    if got[1] is not None:
        assert np.array_equal(got[1], want[1]), (what, "in-degrees", np.nonzero(got[1] != want[1])[0][:8])
    assert got[2] == want[2], (what, got[2], want[2])


@pytest.fixture(scope="module")
def clustered64():
    """the shared reference of the 64-bit clustered case at id_base 0 and k = 10"""
    codes = KG.clustered_case(64)
    rows, counts = KG.model_rows(codes, 10)
    rows.setflags(write=False)
    return codes, rows, counts


# ---- 1. rows against the model -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10, 100])
@pytest.mark.parametrize("bits", [64, 128, 256, 512])
def test_rows_against_the_model(vc, bits, k):
    """both modes, every k_first and every batch give the model's words, and the statistics are the plan mirror's"""
    codes = KG.clustered_case(bits)
    n = len(codes)
    H = KG.dist_hist(codes)
    want = KG.model_rows(codes, k)
    lin = KG.plan_stats(H, k, linear=True)
    with _make(vc, codes) as store:
        for batch in (1, 64, 4096, n + 77):
            got = _graph(store, k, KG.LINEAR, batch=batch)
            KG.same_graph(got, want, (bits, k, "linear", batch))
            assert got[2] == lin, (bits, k, batch, got[2], lin)
        for k_first in (0, k + 1, KG.MAX_K):
            mih = KG.plan_stats(H, k, k_first)
            for batch in (1, 64, 4096, n + 77):
                got = _graph(store, k, KG.MIH_EXACT, batch=batch, k_first=k_first)
                KG.same_graph(got, want, (bits, k, "mih", k_first, batch))
                assert got[2] == mih, (bits, k, k_first, batch, got[2], mih)


def test_the_tie_heavy_set_takes_more_than_one_round(vc):
    codes = KG.clustered_case(64)
    with _make(vc, codes) as store:
        got = _graph(store, 10, KG.MIH_EXACT)
        assert got[2]["n_rounds_max"] > 2 and got[2]["n_searched"] > len(codes) and got[2]["n_linear"] == 0 and got[2]["n_gave_up"] == 0


# ---- 2. the duplicate set -----------------------------------------------------------------------------------------------------------------------
def test_the_duplicate_set_goes_to_the_linear_scan(vc):
    codes, k = KG.dup_case(), KG.DUP_K
    want = KG.model_rows(codes, k)
    plan = KG.plan_stats(KG.dist_hist(codes), k, KG.DUP_K_FIRST)
    assert plan["n_linear"] >= KG.DUP_COPIES
    with _make(vc, codes) as store:
        got = _graph(store, k, KG.MIH_EXACT, k_first=KG.DUP_K_FIRST)
        KG.same_graph(got, want, "duplicates")
        assert got[2] == plan, (got[2], plan)
        copies = KG.dup_copies(codes)
        for i in (int(copies[0]), int(copies[len(copies) // 2]), int(copies[-1])):   # a copy's row: the five smallest ids among the other copies, at distance 0
            assert np.array_equal(got[0][i], copies[copies != i][:k].astype(np.uint64))


# ---- 3. edges of the argument space --------------------------------------------------------------------------------------------------------------
def test_tiny_and_empty_stores(vc):
    codes = KG.clustered_case(64)
    with _make(vc, codes[:1], index=False) as store:                   # N = 1: count 0, a padded row
        for mode in (KG.LINEAR,):
            rows, counts, st = _graph(store, 3, mode)
            assert np.all(rows == KG.INF) and counts.tolist() == [0] and st["n_searched"] == 1
    with _make(vc, codes[:1]) as store:
        rows, counts, st = _graph(store, 3, KG.MIH_EXACT)
        assert np.all(rows == KG.INF) and counts.tolist() == [0]
    with _make(vc, codes[:7], id_base=500) as store:                   # N - 1 < k: counts N - 1, padded rows
        want = KG.model_rows(codes[:7], 10, id_base=500)
        assert np.all(want[1] == 6) and np.all(want[0][:, 6:] == KG.INF)
        for mode in (KG.LINEAR, KG.MIH_EXACT):
            KG.same_graph(_graph(store, 10, mode), want, ("short", mode))
        for kk in (1, 6, 7, 10):                                         # a store with N - 1 < kk: every entry is listed
            for flags in (KG.MUTUAL, KG.EITHER):
                _same_cluster(_cluster(store, want[0], want[1], kk, flags), KG.cluster_model(want[0], want[1], kk, flags, id_base=500), ("short", kk, flags))
    with _make(vc, codes[:0], bits=64) as store:                         # an empty store: VC_OK, zero stats, nothing written
        for mode in (KG.LINEAR, KG.MIH_EXACT):
            rows, counts, st = store.knn_graph(4, mode=mode, with_stats=True)
            assert rows.shape == (0, 4) and counts.shape == (0,) and st == KG.zero_graph_stats()
        labels, deg, st = store.cluster_knn(np.zeros((0, 4), dtype=np.uint64), None, 2)
        assert len(labels) == 0 and st == KG.zero_cluster_stats()


def test_id_base_ranges_and_null_outputs(vc, clustered64):
    codes, _, _ = clustered64
    id_base, k, n = 2 ** 32 - 5000, 10, len(codes)
    want = KG.model_rows(codes, k, id_base=id_base)
    with _make(vc, codes, id_base=id_base) as store:
        for mode in (KG.LINEAR, KG.MIH_EXACT):
            KG.same_graph(_graph(store, k, mode), want, ("id_base", mode))
            a = _graph(store, k, mode, first=0, count=n // 2 + 3, batch=300)
            b = _graph(store, k, mode, first=n // 2 + 3, count=0, batch=300)
            KG.same_graph((np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])), want, ("halves", mode))
            c = _graph(store, k, mode, first=17, count=5)
            KG.same_graph(c, (want[0][17:22], want[1][17:22]), ("inside", mode))
            rows, counts, st = _graph(store, k, mode, with_counts=False, with_stats=False)          # counts and stats may be NULL
            assert counts is None and st is None and np.array_equal(rows, want[0])
        assert store.knn_graph(k, first=n, with_stats=True)[2] == KG.zero_graph_stats()           # an empty range


def test_three_shards_the_host_form_a_stream_and_a_warm_handle(vc, clustered64):
    import torch
    codes, want_rows, want_counts = clustered64
    want, k = (want_rows, want_counts), 10
    H = KG.dist_hist(codes)
    with _make(vc, codes, shards=3, capacity=len(codes) + 10) as store:
        for mode in (KG.LINEAR, KG.MIH_EXACT):
            got = _graph(store, k, mode, batch=500)
            KG.same_graph(got, want, ("sharded", mode))
            assert got[2] == KG.plan_stats(H, k, linear=mode == KG.LINEAR)
            KG.same_graph(store.knn_graph(k, mode=mode), want, ("sharded host", mode))
        for flags in (KG.MUTUAL, KG.EITHER):
            model = KG.cluster_model(want_rows, want_counts, 4, flags)
            _same_cluster(_cluster(store, want_rows, want_counts, 4, flags), model, ("sharded clusters", flags))
            _same_cluster(store.cluster_knn(want_rows, want_counts, 4, flags), model, ("sharded host clusters", flags))
    with _make(vc, codes) as store:
        for mode in (KG.LINEAR, KG.MIH_EXACT):
            rows, counts, st = store.knn_graph(k, mode=mode, with_stats=True)                      # the host form
            KG.same_graph((rows, counts), want, ("host", mode))
            assert st == KG.plan_stats(H, k, linear=mode == KG.LINEAR)
            KG.same_graph(store.knn_graph(k, mode=mode, first=100, count=50, batch=7), (want_rows[100:150], want_counts[100:150]), ("host range", mode))
        side = torch.cuda.Stream()
        got = _graph(store, k, KG.MIH_EXACT, stream=side.cuda_stream)                               # a caller stream
        KG.same_graph(got, want, "stream")
        # a warm handle: other calls in between, larger and smaller shapes, leave every word the same
        store.search_knn(codes[:33], 50, mode=KG.MIH_EXACT)
        _graph(store, 100, KG.MIH_EXACT, k_first=KG.MAX_K, batch=100, count=300)
        store.cluster_radius(1, mode=KG.MIH_EXACT)
        _graph(store, 1, KG.LINEAR, batch=5, count=40)
        for mode in (KG.LINEAR, KG.MIH_EXACT):
            KG.same_graph(_graph(store, k, mode), want, ("warm", mode))


def test_every_error_leaves_the_outputs_untouched(vc, clustered64):
    codes, rows, counts = clustered64
    n = len(codes)
    with _make(vc, codes[:300], index=False, capacity=400) as store:
        out, cnt = np.full((300, 10), KG.STALE, dtype=np.uint64), np.full(300, KG.STALE32, dtype=np.uint32)
        st = vc.VcKnnGraphStats(7, 7, 7, 7, 7)
        L, h, p = store._L, store._h, lambda a: a.ctypes.data
        import ctypes as C
        bad = [
            (vc.VC_ERR_INVALID, (None, 10, KG.LINEAR, 0, 0, 0, 0, p(out), p(cnt))),                # a null handle
            (vc.VC_ERR_INVALID, (h, 10, KG.LINEAR, 0, 0, 0, 0, None, p(cnt))),                     # null rows
            (vc.VC_ERR_INVALID, (h, 0, KG.LINEAR, 0, 0, 0, 0, p(out), p(cnt))),                    # k out of range
            (vc.VC_ERR_INVALID, (h, KG.MAX_K, KG.LINEAR, 0, 0, 0, 0, p(out), p(cnt))),
            (vc.VC_ERR_INVALID, (h, 10, KG.LINEAR, 0, 0, 0, 10, p(out), p(cnt))),                  # a bad k_first
            (vc.VC_ERR_INVALID, (h, 10, KG.LINEAR, 0, 0, 0, KG.MAX_K + 1, p(out), p(cnt))),
            (vc.VC_ERR_INVALID, (h, 10, KG.MIH_APPROX, 0, 0, 0, 0, p(out), p(cnt))),               # a refused mode
            (vc.VC_ERR_INVALID, (h, 10, 3, 0, 0, 0, 0, p(out), p(cnt))),
            (vc.VC_ERR_INVALID, (h, 10, KG.LINEAR, 0, 100, 201, 0, p(out), p(cnt))),               # first + count > N
            (vc.VC_ERR_INVALID, (h, 10, KG.LINEAR, 0, 301, 0, 0, p(out), p(cnt))),
            (vc.VC_ERR_STATE, (h, 10, KG.MIH_EXACT, 0, 0, 0, 0, p(out), p(cnt))),                   # MIH without an index
        ]
        for want, args in bad:
            assert L.vc_knn_graph(*args, C.byref(st)) == want, args
            assert np.all(out == KG.STALE) and np.all(cnt == KG.STALE32) and st.n_searched == 7 and st.k_last == 7
        store.build_index()
        store.add_codes(codes[300:310])                                                              # a stale index counts as none
        assert L.vc_knn_graph(h, 10, KG.MIH_EXACT, 0, 0, 0, 0, p(out), p(cnt), C.byref(st)) == vc.VC_ERR_STATE
        assert np.all(out == KG.STALE) and st.n_searched == 7
        # vc_cluster_knn
        lab, deg = np.full(310, KG.STALE32, dtype=np.uint32), np.full(310, KG.STALE32, dtype=np.uint32)
        g = np.ascontiguousarray(KG.model_rows(codes[:310], 10)[0])
        cst = vc.VcClusterKnnStats(7, 7, 7, 7, 7)
        for args in ((None, p(g), None, 10, 3, 0, 64, p(lab), p(deg)), (h, None, None, 10, 3, 0, 64, p(lab), p(deg)), (h, p(g), None, 10, 3, 0, 64, None, p(deg)),
                     (h, p(g), None, 0, 0, 0, 64, p(lab), p(deg)), (h, p(g), None, KG.MAX_K, 3, 0, 64, p(lab), p(deg)), (h, p(g), None, 10, 0, 0, 64, p(lab), p(deg)),
                     (h, p(g), None, 10, 11, 0, 64, p(lab), p(deg)), (h, p(g), None, 10, 3, 2, 64, p(lab), p(deg))):
            assert L.vc_cluster_knn(*args, C.byref(cst)) == vc.VC_ERR_INVALID, args
            assert np.all(lab == KG.STALE32) and np.all(deg == KG.STALE32) and cst.n_edges == 7
    with _make(vc, codes[:50], shards=3, capacity=60, index=False) as store:
        out = np.full((50, 4), KG.STALE, dtype=np.uint64)
        for mode, k, want in ((KG.MIH_EXACT, 4, vc.VC_ERR_STATE), (KG.MIH_APPROX, 4, vc.VC_ERR_INVALID), (KG.LINEAR, 0, vc.VC_ERR_INVALID)):
            assert store._L.vc_sharded_knn_graph(store._h, k, mode, 0, 0, 0, 0, out.ctypes.data, None, None) == want
            assert np.all(out == KG.STALE)


# ---- 4. vc_cluster_knn* on those graphs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [KG.MUTUAL, KG.EITHER])
def test_clusters_against_the_model(vc, clustered64, flags):
    codes, rows, counts = clustered64
    with _make(vc, codes, index=False) as store:
        for kk in range(1, 11):
            for max_dist in (0xFFFFFFFF, 64, 2):
                got = _cluster(store, rows, counts, kk, flags, max_dist, with_degree=kk % 2 == 1)
                _same_cluster(got, KG.cluster_model(rows, counts, kk, flags, max_dist), (kk, flags, max_dist))
        got = _cluster(store, rows, None, 5, flags)                                                   # counts may be NULL
        _same_cluster(got, KG.cluster_model(rows, counts, 5, flags), ("no counts", flags))


def test_the_hub_set(vc):
    codes, hub = KG.hub_case()
    k, id_base = KG.HUB_K, 1000
    with _make(vc, codes, id_base=id_base) as store:
        rows, counts, _ = _graph(store, k, KG.MIH_EXACT)
        KG.same_graph((rows, counts), KG.model_rows(codes, k, id_base=id_base), "hub graph")
        seen = {}
        for flags in (KG.MUTUAL, KG.EITHER):
            for kk in (1, 3, k):
                got = _cluster(store, rows, counts, kk, flags)
                _same_cluster(got, KG.cluster_model(rows, counts, kk, flags, id_base=id_base), ("hub", kk, flags))
                seen[flags, kk] = got
        for kk in (1, 3, k):
            assert seen[KG.MUTUAL, kk][1][hub] == KG.HUB_SATELLITES > k                              # every satellite lists the hub
            assert seen[KG.MUTUAL, kk][2]["max_in_degree"] == KG.HUB_SATELLITES
            assert seen[KG.MUTUAL, kk][2]["n_clusters"] > seen[KG.EITHER, kk][2]["n_clusters"]
        labels, _, _, = seen[KG.EITHER, 1]
        assert len(set(labels[:KG.HUB_SATELLITES + 1].tolist())) == 1                                # one way is enough: the star is one component
        labels = seen[KG.MUTUAL, 3][0]
        assert labels[KG.HUB_SATELLITES] == id_base + KG.HUB_SATELLITES                              # the last satellite is nobody's mutual neighbour


def test_a_corrupted_graph_is_refused(vc, clustered64):
    codes, rows, counts = clustered64
    with _make(vc, codes, index=False) as store:
        for at, value in ((700, 11), (0, 0xFFFFFFFF)):
            broken = counts.copy()
            broken[at] = value
            with pytest.raises(vc.VcError) as err:
                _cluster(store, rows, broken, 3)
            assert err.value.code == vc.VC_ERR_INVALID
        foreign = rows.copy()
        foreign[5, 0] = np.uint64(len(codes) + 3)                                                    # an id outside the store
        with pytest.raises(vc.VcError) as err:
            _cluster(store, foreign, counts, 3)
        assert err.value.code == vc.VC_ERR_INVALID
        _same_cluster(_cluster(store, rows, counts, 3), KG.cluster_model(rows, counts, 3), "after the refusals")


def test_labels_feed_the_group_summary(vc, clustered64):
    codes, rows, counts = clustered64
    with _make(vc, codes, index=False) as store:
        labels, deg, st = store.cluster_knn(rows, counts, 6, KG.MUTUAL)                              # the host form
        _same_cluster((labels, deg, st), KG.cluster_model(rows, counts, 6), "host clusters")
        groups, _, _, group_index = store.group_summary(labels)
        assert len(groups) == st["n_clusters"] and int(groups["size"].sum()) == len(codes)
        assert np.array_equal(groups["label"][group_index], labels)
