"""Shared-nearest-neighbour clustering of a built k-NN graph: vc_cluster_snn* and its vc_sharded_* forms.

The expectation is snn_common.py's numpy model -- knn_graph_common's edge sets, the overlaps as a matrix product, a host union-find --
pinned against plain set loops by test_snn_cpu.py, which also shows that on the noisy input every threshold and both flags matter.
Labels, weights, histogram and statistics are integer functions of the graph and the call, so every comparison is exact equality on
every word; device outputs are pre-filled with a stale pattern, so every word is proven written and the words around an output proven
untouched.  One device; N <= 1100.

Not tested: the sharded forms across real devices, and a row that lists one id twice (the result is unspecified; that the set's loops
end and stay in bounds for such a row is shown on the CPU by tests/cpp/snn_plan_test.cc)."""
import ctypes as C

import numpy as np
import pytest

import knn_graph_common as KG
import snn_common as SN

pytestmark = pytest.mark.gpu

PAD = 3          # stale words kept on both sides of every device output
B = SN.WAVE_KK
NO_CAP = 0xFFFFFFFF


def _make(vc, codes, id_base=0, shards=0, index=False):
    bits = codes.shape[1] * 8
    if shards:
        e = vc.ShardedEngine(bits, capacity=len(codes) + 10, n_shards=shards, devices=[0], id_base=id_base, n_tables=KG.TABLES[bits])
    else:
        e = vc.Engine(bits, capacity=len(codes), id_base=id_base, n_tables=KG.TABLES[bits])
    e.add_codes(codes)
    if index:
        e.build_index()
    return e


def _to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    signed = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(a.view(signed).copy()).cuda()


def _stale(n_words, dtype):
    return _to_dev(np.full(n_words + 2 * PAD, SN.STALE64 if dtype == np.uint64 else KG.STALE32, dtype=dtype))


def _inner(buf, n_words, dtype, what):
    """the n_words words between the pads of a synchronised buffer; the pads must still be stale"""
    raw = buf.cpu().numpy().view(dtype)
    stale = SN.STALE64 if dtype == np.uint64 else KG.STALE32
    assert np.all(raw[:PAD] == stale) and np.all(raw[PAD + n_words:] == stale), (what, "words around the output")
    return raw[PAD:PAD + n_words]


def _snn(store, rows, counts, kk, min_shared, flags=KG.MUTUAL, max_dist=NO_CAP, with_shared=True, with_hist=True):
    """vc_cluster_snn_dev on stale-filled outputs: (labels, shared | None, hist | None, stats)"""
    import torch
    n, k = rows.shape
    d_r, d_c = _to_dev(rows), _to_dev(counts) if counts is not None else None
    d_l = _stale(n, np.uint32)
    d_s = _stale(n * kk, np.uint32) if with_shared else None
    d_h = _stale(kk, np.uint64) if with_hist else None
    torch.cuda.synchronize()
    st = store.cluster_snn_dev(d_r.data_ptr(), d_c.data_ptr() if counts is not None else None, k, kk, min_shared, d_l.data_ptr() + 4 * PAD,
                               d_s.data_ptr() + 4 * PAD if with_shared else None, d_h.data_ptr() + 8 * PAD if with_hist else None, flags=flags,
                               max_dist=max_dist)
    torch.cuda.synchronize()
    return (_inner(d_l, n, np.uint32, "labels"), _inner(d_s, n * kk, np.uint32, "shared").reshape(n, kk) if with_shared else None,
            _inner(d_h, kk, np.uint64, "hist") if with_hist else None, st)


def _want(weights, n, min_shared, flags, id_base=0):
    shared, hist, edges = weights
    labels, st = SN.snn_labels(n, edges, min_shared, flags, id_base)
    return labels, shared, hist, st


# ---- 1. the sweep ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,kk", [(12, 10), (70, 64), (70, 65), (B + 6, B), (B + 6, B + 1)])
def test_sweep_against_the_model(vc, k, kk):
    """both team shapes and both sides of every boundary of the plan: 16 lanes per entry, the whole wave, two passes over row j,
    the widest wave team, the narrowest block team; both flags, with and without the cap, every threshold"""
    assert B + 6 < 700
    codes, rows, counts = SN.mixed_graph(64, k)
    n = len(codes)
    with _make(vc, codes) as store:
        for max_dist in (NO_CAP, 64 // 4):
            weights = SN.snn_weights(rows, counts, kk, max_dist)
            for flags in (KG.MUTUAL, KG.EITHER):
                for min_shared in SN.thresholds(kk):
                    got = _snn(store, rows, counts, kk, min_shared, flags, max_dist)
                    SN.same_snn(got, _want(weights, n, min_shared, flags), (k, kk, max_dist, flags, min_shared))


# ---- 2. the widest rows and a long-lived handle -----------------------------------------------------------------------------------------
WIDE_N, WIDE_K = 1100, 1030


@pytest.fixture(scope="module")
def wide(vc):
    """mixed_case(64, n = 1100) at k = 1030 from the engine's own LINEAR build, equal to the model's rows; the weights at kk = 1024"""
    codes = SN.mixed_case(64, n=WIDE_N)
    with _make(vc, codes) as store:
        rows, counts = store.knn_graph(WIDE_K, mode=KG.LINEAR)
    KG.same_graph((rows, counts), KG.model_rows(codes, WIDE_K), "wide graph")
    rows.setflags(write=False)
    return codes, rows, counts, SN.snn_weights(rows, counts, SN.MAX_KK)


def test_the_widest_rows(vc, wide):
    codes, rows, counts, weights = wide
    listed = weights[0][weights[0] != SN.NONE]
    middle = int(np.median(listed))                                            # a threshold that splits the listed entries (from the model)
    assert 0 < int((listed >= middle).sum()) and int((listed < middle).sum()) > 0
    with _make(vc, codes) as store:
        for flags, min_shared in ((KG.MUTUAL, middle), (KG.EITHER, int(listed.max())), (KG.MUTUAL, 0), (KG.EITHER, SN.MAX_KK)):
            got = _snn(store, rows, counts, SN.MAX_KK, min_shared, flags)
            SN.same_snn(got, _want(weights, WIDE_N, min_shared, flags), ("wide", flags, min_shared))


def test_call_history_leaves_every_word_the_same(vc, wide):
    codes, rows, counts, weights = wide
    want = {SN.MAX_KK: weights, 10: SN.snn_weights(rows, counts, 10), 64: SN.snn_weights(rows, counts, 64)}
    with _make(vc, codes) as store:
        first = {}
        for step, kk in enumerate((SN.MAX_KK, 10, 64, SN.MAX_KK, 64, 10)):
            min_shared = kk // 2
            got = _snn(store, rows, counts, kk, min_shared, KG.EITHER)
            SN.same_snn(got, _want(want[kk], WIDE_N, min_shared, KG.EITHER), ("history", step, kk))
            if kk in first:
                for a, b in zip(got[:3], first[kk][:3]):
                    assert np.array_equal(a, b)
                assert got[3] == first[kk][3]
            first.setdefault(kk, got)
            labels, _, st = store.cluster_knn(rows, counts, 5)                  # another reader of the graph in between
            assert st == KG.cluster_model(rows, counts, 5)[2] if step == 0 else st["n_edges"] == 5 * WIDE_N


# ---- 3. other graphs ---------------------------------------------------------------------------------------------------------------------------
def test_the_exact_mih_graph(vc):
    codes = SN.mixed_case(128)
    k, kk = 12, 10
    with _make(vc, codes, index=True) as store:
        rows, counts = store.knn_graph(k, mode=KG.MIH_EXACT)
        KG.same_graph((rows, counts), KG.model_rows(codes, k), "mih graph")
        weights = SN.snn_weights(rows, counts, kk)
        for flags in (KG.MUTUAL, KG.EITHER):
            for min_shared in (1, kk // 2):
                SN.same_snn(_snn(store, rows, counts, kk, min_shared, flags), _want(weights, len(codes), min_shared, flags), ("mih", flags, min_shared))


def test_no_threshold_is_cluster_knn(vc):
    codes, rows, counts = SN.mixed_graph(64, 70)
    with _make(vc, codes) as store:
        for kk in (10, 64, 70):
            for flags in (KG.MUTUAL, KG.EITHER):
                for max_dist in (NO_CAP, 16):
                    labels, _, _, st = _snn(store, rows, counts, kk, 0, flags, max_dist)
                    knn_labels, _, knn = store.cluster_knn(rows, counts, kk, flags, max_dist)
                    assert np.array_equal(labels, knn_labels), (kk, flags, max_dist)
                    assert [st[x] for x in ("n_edges", "n_mutual", "n_clusters")] == [knn[x] for x in ("n_edges", "n_mutual", "n_clusters")]


def test_short_rows_and_tiny_stores(vc):
    codes, _ = KG.hub_case()
    n, k = len(codes), 100
    assert n == 71 < k
    rows, counts = KG.model_rows(codes, k)
    assert np.all(counts == n - 1)                                             # every row holds the whole store
    weights = SN.snn_weights(rows, counts, k)
    assert np.all(weights[0][:, :n - 1] == n - 2) and np.all(weights[0][:, n - 1:] == SN.NONE)   # S_i and S_j share everybody but i and j
    with _make(vc, codes) as store:
        for flags in (KG.MUTUAL, KG.EITHER):
            for min_shared in (0, n - 2, n - 1, k):
                SN.same_snn(_snn(store, rows, counts, k, min_shared, flags), _want(weights, n, min_shared, flags), ("short", flags, min_shared))
        SN.same_snn(_snn(store, rows, None, k, n - 2), _want(weights, n, n - 2, KG.MUTUAL), "short, no counts")
    for m in (2, 1):
        rows, counts = KG.model_rows(codes[:m], 3, 40)
        with _make(vc, codes[:m], id_base=40) as store:
            for given in (counts, None):
                for min_shared in (0, 1):
                    got = _snn(store, rows, given, 3, min_shared)
                    SN.same_snn(got, SN.snn_model(rows, counts, 3, min_shared, id_base=40), ("tiny", m, min_shared))
                    if m == 1:
                        assert got[0].tolist() == [40] and np.all(got[1] == SN.NONE) and np.all(got[2] == 0) and got[3] == dict(SN.zero_stats(), n_clusters=1)
                    else:
                        assert got[1].tolist() == [[0, int(SN.NONE), int(SN.NONE)]] * 2 and got[0].tolist() == ([40, 40] if min_shared == 0 else [40, 41])


def test_optional_pointers_and_an_id_base(vc):
    id_base, k, kk, min_shared = 2 ** 32 - 5000, 12, 10, 3
    codes = SN.mixed_case(64)
    rows, counts = KG.model_rows(codes, k, id_base)
    weights = SN.snn_weights(rows, counts, kk, NO_CAP, id_base)
    with _make(vc, codes, id_base=id_base) as store:
        for flags in (KG.MUTUAL, KG.EITHER):
            want = _want(weights, len(codes), min_shared, flags, id_base)
            for given in (counts, None):                                       # counts NULL against counts given
                for with_shared, with_hist in ((True, True), (False, True), (True, False), (False, False)):
                    got = _snn(store, rows, given, kk, min_shared, flags, with_shared=with_shared, with_hist=with_hist)
                    assert (got[1] is None) == (not with_shared) and (got[2] is None) == (not with_hist)
                    SN.same_snn(got, want, (flags, given is None, with_shared, with_hist))
        d_rows, d_labels = _to_dev(rows), _stale(len(codes), np.uint32)
        assert store.cluster_snn_dev(d_rows.data_ptr(), None, k, kk, min_shared, d_labels.data_ptr() + 4 * PAD, with_stats=False) is None   # stats may be NULL
        assert np.array_equal(_inner(d_labels, len(codes), np.uint32, "labels"), _want(weights, len(codes), min_shared, KG.MUTUAL, id_base)[0])


def test_the_host_form_and_three_shards(vc):
    codes, rows, counts = SN.mixed_graph(64, 70)
    n = len(codes)
    with _make(vc, codes) as store, _make(vc, codes, shards=3) as sharded:
        for kk, min_shared, flags, max_dist in ((10, 3, KG.MUTUAL, NO_CAP), (64, 30, KG.EITHER, NO_CAP), (65, 20, KG.MUTUAL, 16)):
            want = _want(SN.snn_weights(rows, counts, kk, max_dist), n, min_shared, flags)
            single = _snn(store, rows, counts, kk, min_shared, flags, max_dist)
            SN.same_snn(single, want, ("device", kk))
            SN.same_snn(store.cluster_snn(rows, counts, kk, min_shared, flags, max_dist), want, ("host", kk))
            SN.same_snn(store.cluster_snn(rows, None, kk, min_shared, flags, max_dist, with_shared=False), want, ("host, no counts, no weights", kk))
            SN.same_snn(store.cluster_snn(rows, counts, kk, min_shared, flags, max_dist, with_hist=False), want, ("host, no histogram", kk))
            SN.same_snn(_snn(sharded, rows, counts, kk, min_shared, flags, max_dist), single, ("sharded", kk))
            SN.same_snn(sharded.cluster_snn(rows, counts, kk, min_shared, flags, max_dist), single, ("sharded host", kk))
        labels, _, _, st = store.cluster_snn(rows, counts, 10, 3)                # the labels feed the group summary unchanged
        groups, _, _, group_index = store.group_summary(labels)
        assert len(groups) == st["n_clusters"] and np.array_equal(groups["label"][group_index], labels)


# ---- 4. errors ---------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_untouched(vc):
    codes, rows, counts = SN.mixed_graph(64, 12)
    n, p = len(codes), lambda a: a.ctypes.data
    g = np.ascontiguousarray(rows)
    wide = np.zeros((n, 1100), dtype=np.uint64)
    lab, sh, hist = np.full(n, KG.STALE32, dtype=np.uint32), np.full(n * 1100, KG.STALE32, dtype=np.uint32), np.full(1100, SN.STALE64, dtype=np.uint64)
    with _make(vc, codes) as store, _make(vc, codes, shards=3) as sharded:
        for L_fn, h in ((store._L.vc_cluster_snn, store._h), (sharded._L.vc_sharded_cluster_snn, sharded._h)):
            st = vc.VcClusterSnnStats(7, 7, 7, 7, 7, 7)
            for args in ((None, p(g), None, 12, 10, 0, 64, 2, p(lab), p(sh), p(hist)),            # a null handle
                         (h, None, None, 12, 10, 0, 64, 2, p(lab), p(sh), p(hist)),                # null rows
                         (h, p(g), None, 12, 10, 0, 64, 2, None, p(sh), p(hist)),                  # null labels
                         (h, p(g), None, 0, 0, 0, 64, 2, p(lab), p(sh), p(hist)),                  # k out of range
                         (h, p(g), None, KG.MAX_K, 10, 0, 64, 2, p(lab), p(sh), p(hist)),
                         (h, p(g), None, 12, 0, 0, 64, 2, p(lab), p(sh), p(hist)),                 # kk out of range
                         (h, p(g), None, 12, 13, 0, 64, 2, p(lab), p(sh), p(hist)),
                         (h, p(wide), None, 1100, SN.MAX_KK + 1, 0, 64, 2, p(lab), p(sh), p(hist)),   # kk <= k but above VC_SNN_MAX_KK
                         (h, p(g), None, 12, 10, 2, 64, 2, p(lab), p(sh), p(hist)),                # unknown flags
                         (h, p(g), None, 12, 10, 0x80000001, 64, 2, p(lab), p(sh), p(hist))):
                assert L_fn(*args, C.byref(st)) == vc.VC_ERR_INVALID, args
                assert np.all(lab == KG.STALE32) and np.all(sh == KG.STALE32) and np.all(hist == SN.STALE64)
                assert (st.n_edges, st.n_joined, st.max_shared) == (7, 7, 7)
        with pytest.raises(vc.VcError) as err:                                                      # the device form checks the same
            _snn(store, rows, counts, 13, 2)
        assert err.value.code == vc.VC_ERR_INVALID


def test_a_corrupted_graph_is_refused_on_the_device(vc):
    id_base = 300
    codes = SN.mixed_case(64)
    n = len(codes)
    with _make(vc, codes, id_base=id_base) as store:
        for k, kk in ((70, 10), (70, 64), (B + 6, B + 1)):                     # 16 lanes per entry, one wave per entry, one block per row
            rows, counts = KG.model_rows(codes, k, id_base)
            want = SN.snn_model(rows, counts, kk, kk // 3, KG.EITHER, id_base=id_base)
            broken = counts.copy()
            broken[n - 1] = k + 1                                              # a count of k + 1
            foreign = rows.copy()
            foreign[5, 1] = (foreign[5, 1] & np.uint64(0xFFFFFFFF00000000)) | np.uint64(n + id_base)    # an id equal to N + id_base
            own = rows.copy()
            own[n // 2, kk - 1] = (own[n // 2, kk - 1] & np.uint64(0xFFFFFFFF00000000)) | np.uint64(n // 2 + id_base)   # the row's own id
            for r, c in ((rows, broken), (foreign, counts), (own, counts), (own, None)):
                with pytest.raises(vc.VcError) as err:
                    _snn(store, r, c, kk, kk // 3, KG.EITHER)
                assert err.value.code == vc.VC_ERR_INVALID
                SN.same_snn(_snn(store, rows, counts, kk, kk // 3, KG.EITHER), want, ("after the refusal", kk))
