"""The minimum spanning forest of a built k-NN graph and the cut of an edge list: vc_knn_mst*, vc_mst_cut* and their vc_sharded_* forms.

The expectation is knn_mst_common.py's model -- knn_graph_common's edge sets, the home rule, Kruskal under the order as tuples --
pinned by test_knn_mst_cpu.py against a brute force over all spanning forests and against cluster_model at every height; the same
file pins the figures of the inputs used here.  Edges, labels, histogram and statistics are integer functions of the graph and the
call, so every comparison is exact equality on every word; device outputs are pre-filled with a stale pattern and padded, so
edges[0 .. M), labels and hist are proven written and edges[M ..) and the words around every output proven untouched.  n_rounds is
implementation-defined and only bounded.  One device.

Not tested: the sharded forms across real devices, N kk near 2^31 - 1 on the device (the limit itself is refused below and checked in
tests/cpp/knn_mst_plan_test.cc), and rows that are no vc_knn_graph* rows beyond the three the device refuses."""
import ctypes as C

import numpy as np
import pytest

import knn_graph_common as KG
import knn_mst_common as KM

pytestmark = pytest.mark.gpu

PAD = 4          # stale 64-bit words kept on both sides of every device output
STALE = KM.STALE64


def _make(vc, codes, id_base=0, shards=0):
    bits = codes.shape[1] * 8
    if shards:
        e = vc.ShardedEngine(bits, capacity=len(codes) + 10, n_shards=shards, devices=[0], id_base=id_base, n_tables=KG.TABLES[bits])
    else:
        e = vc.Engine(bits, capacity=max(len(codes), 1), id_base=id_base, n_tables=KG.TABLES[bits])
    if len(codes):
        e.add_codes(codes)
    return e


def _to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    signed = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(a.view(signed).copy()).cuda()


def _stale(n_words):
    return _to_dev(np.full(n_words + 2 * PAD, STALE, dtype=np.uint64))


def _inner(buf, n_words, what):
    """the n_words 64-bit words between the pads of a synchronised buffer; the pads must still be stale"""
    raw = buf.cpu().numpy().view(np.uint64)
    assert np.all(raw[:PAD] == STALE) and np.all(raw[PAD + n_words:] == STALE), (what, "words around the output")
    return raw[PAD:PAD + n_words]


def _mst(store, rows, counts, kk, flags, max_dist=KM.NO_CAP, kind=KM.DISTANCE, min_pts=1, with_labels=True, with_hist=True, with_stats=True):
    """vc_knn_mst_dev on stale-filled outputs: (the whole edge buffer as 64-bit words [2 (max(N, 1) - 1)], labels [N] | None,
    hist [bits + 1] | None, stats | None)"""
    import torch
    n, k = rows.shape
    cap, lab_words = max(n, 1) - 1, (n + 1) // 2
    d_r, d_c = _to_dev(rows if n else np.zeros((1, 1), dtype=np.uint64)), _to_dev(counts) if counts is not None else None
    d_e, d_l, d_h = _stale(2 * cap), _stale(lab_words), _stale(store.bits + 1)
    torch.cuda.synchronize()
    st = store.knn_mst_dev(d_r.data_ptr(), d_c.data_ptr() if counts is not None else None, k, kk, d_e.data_ptr() + 8 * PAD,
                           d_l.data_ptr() + 8 * PAD if with_labels else None, d_h.data_ptr() + 8 * PAD if with_hist else None, flags=flags, max_dist=max_dist,
                           weight_kind=kind, min_pts=min_pts, with_stats=with_stats)
    torch.cuda.synchronize()
    words, labels, hist = _inner(d_e, 2 * cap, "edges"), _inner(d_l, lab_words, "labels").view(np.uint32), _inner(d_h, store.bits + 1, "hist")
    if n % 2 and with_labels:
        assert labels[n] == np.array([STALE]).view(np.uint32)[1], "the word behind the labels"
    if not with_labels:
        assert np.all(labels.view(np.uint64) == STALE)
    if not with_hist:
        assert np.all(hist == STALE)
    return words, labels[:n] if with_labels else None, hist if with_hist else None, st


def _ok(store, rows, counts, kk, flags, want, what, **kw):
    """a call that must succeed: edges[0 .. M), labels, hist and the stats are the model's, edges[M ..) is still stale"""
    words, labels, hist, st = _mst(store, rows, counts, kk, flags, **kw)
    M, n = len(want[0]), len(rows)
    got = (words[:2 * M].view(KM.EDGE), labels, hist, st)
    KM.same_mst(got, want, what)
    assert np.all(words[2 * M:] == STALE), (what, "beyond M")
    if st is not None:
        assert st["n_rounds"] == 0 if M == 0 else 1 <= st["n_rounds"] <= KM.round_bound(n), (what, st["n_rounds"])
    return got


def _cluster_labels(store, d_r, d_c, n, k, kk, flags, max_dist):
    import torch
    d_l = _to_dev(np.zeros(n, dtype=np.uint32))
    cl = store.cluster_knn_dev(d_r.data_ptr(), d_c.data_ptr(), k, kk, d_l.data_ptr(), None, flags=flags, max_dist=max_dist)
    torch.cuda.synchronize()
    return d_l.cpu().numpy().view(np.uint32), cl


def _cuts_agree_with_cluster_knn(store, rows, counts, kk, flags, edges, max_weight, cap=KM.NO_CAP, heights=None):
    """vc_mst_cut_dev on the forest at every h in 0 .. max_weight + 1 == vc_cluster_knn_dev(max_dist = min(cap, h)), labels and count"""
    import torch
    n, k = rows.shape
    d_r, d_c, d_e = _to_dev(rows), _to_dev(counts), _to_dev(edges.view(np.uint64) if len(edges) else np.zeros(2, dtype=np.uint64))
    for h in (range(0, max_weight + 2) if heights is None else heights):
        d_l = _stale((n + 1) // 2)
        torch.cuda.synchronize()
        count = store.mst_cut_dev(d_e.data_ptr(), len(edges), h, d_l.data_ptr() + 8 * PAD)
        torch.cuda.synchronize()
        got = _inner(d_l, (n + 1) // 2, "cut labels").view(np.uint32)[:n]
        want, cl = _cluster_labels(store, d_r, d_c, n, k, kk, flags, min(cap, h))
        assert np.array_equal(got, want) and count == cl["n_clusters"], (kk, flags, h)


# ---- 1. the clustered set -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kk", [10, 1])
def test_the_clustered_set_against_the_model_and_cluster_knn(vc, kk):
    """ties at every weight; both flags, counts given and NULL, the cap, and every cut of the forest against vc_cluster_knn_dev"""
    codes, rows, counts = KM.graph("clustered", 12)
    n = len(codes)
    with _make(vc, codes) as store:
        d_r, d_c = _to_dev(rows), _to_dev(counts)
        for flags in (KM.MUTUAL, KM.EITHER):
            for max_dist in (KM.NO_CAP, 16):
                want = KM.model("clustered", 12, kk, flags, max_dist)
                for given in (counts, None):
                    got = _ok(store, rows, given, kk, flags, want, (kk, flags, max_dist, given is None), max_dist=max_dist)
                labels, cl = _cluster_labels(store, d_r, d_c, n, 12, kk, flags, max_dist)
                assert np.array_equal(got[1], labels) and got[3]["n_clusters"] == cl["n_clusters"] and got[3]["n_edges"] == cl["n_edges"]
            _cuts_agree_with_cluster_knn(store, rows, counts, kk, flags, got[0], got[3]["max_weight"], cap=16)
        if kk == 10:
            assert KM.model("clustered", 12, 10, KM.MUTUAL)[3]["n_tree"] == 526 and KM.model("clustered", 12, 10, KM.EITHER)[3]["n_tree"] == 1995


def test_reachability_weights(vc):
    codes, rows, counts = KM.graph("clustered", 12)
    with _make(vc, codes) as store:
        for flags in (KM.MUTUAL, KM.EITHER):
            want = KM.model("clustered", 12, 10, flags, weight_kind=KM.REACHABILITY, min_pts=5)
            got = _ok(store, rows, counts, 10, flags, want, ("reach", flags), kind=KM.REACHABILITY, min_pts=5)
            assert np.any(got[0]["weight"] != got[0]["dist"])
            plain = _ok(store, rows, counts, 10, flags, KM.model("clustered", 12, 10, flags), ("plain", flags))
            one = _ok(store, rows, counts, 10, flags, KM.model("clustered", 12, 10, flags), ("min_pts 1", flags), kind=KM.REACHABILITY, min_pts=1)
            assert np.array_equal(one[0], plain[0]) and np.array_equal(one[2], plain[2]) and {**one[3], "n_rounds": 0} == {**plain[3], "n_rounds": 0}
        # min_pts = k + 1 reads the last column; a short row's core distance is the code width
        rows13, counts13 = KG.model_rows(codes, 12)
        want = KM.mst_model(rows13, counts13, 10, KM.EITHER, weight_kind=KM.REACHABILITY, min_pts=13)
        _ok(store, rows13, counts13, 10, KM.EITHER, want, "min_pts = k + 1", kind=KM.REACHABILITY, min_pts=13)
    hub = KG.hub_case()[0][:4]
    rows, counts = KG.model_rows(hub, 5)
    with _make(vc, hub) as store:
        want = KM.mst_model(rows, counts, 3, KM.EITHER, weight_kind=KM.REACHABILITY, min_pts=5)
        got = _ok(store, rows, counts, 3, KM.EITHER, want, "short rows", kind=KM.REACHABILITY, min_pts=5)
        assert np.all(got[0]["weight"] == 64)


# ---- 2. the uniform set: six rounds ---------------------------------------------------------------------------------------------------------------
def test_the_uniform_set(vc):
    codes, rows, counts = KM.graph("uniform", 4)
    with _make(vc, codes) as store:
        got = _ok(store, rows, counts, 2, KM.EITHER, KM.model("uniform", 4, 2, KM.EITHER), "kk 2 either")
        assert got[3]["n_tree"] == 4095 and got[3]["max_weight"] <= 21
        _cuts_agree_with_cluster_knn(store, rows, counts, 2, KM.EITHER, got[0], got[3]["max_weight"])
        got = _ok(store, rows, counts, 4, KM.MUTUAL, KM.model("uniform", 4, 4, KM.MUTUAL), "kk 4 mutual")
        assert got[3]["n_clusters"] == 134
        _cuts_agree_with_cluster_knn(store, rows, counts, 4, KM.MUTUAL, got[0], got[3]["max_weight"])
        for flags in (KM.MUTUAL, KM.EITHER):
            _ok(store, rows, counts, 4, flags, KM.model("uniform", 4, 4, flags, weight_kind=KM.REACHABILITY, min_pts=3), ("reach", flags), kind=KM.REACHABILITY,
                min_pts=3)


# ---- 3. the tie-break alone: a chain of 512 hooks in one round ---------------------------------------------------------------------------------------
def test_the_thermometer_chain(vc):
    codes, rows, counts = KM.graph("thermo", 2)
    with _make(vc, codes) as store:
        for flags in (KM.MUTUAL, KM.EITHER):
            got = _ok(store, rows, counts, 2, flags, KM.model("thermo", 2, 2, flags), ("thermo", flags))
            assert got[0]["a"].tolist() == list(range(512)) and np.all(got[0]["weight"] == 1) and np.all(got[1] == 0)
            _cuts_agree_with_cluster_knn(store, rows, counts, 2, flags, got[0], 1)


# ---- 4. hubs, the complete graph, the duplicates, the tenth weight bit -------------------------------------------------------------------------------
def test_the_hub_set_and_the_complete_graph(vc):
    codes = KG.hub_case()[0]
    with _make(vc, codes) as store:
        _, wide, wide_counts = KM.graph("hub", 100)
        assert np.all(wide_counts == 70)
        for flags in (KM.MUTUAL, KM.EITHER):
            for given in (wide_counts, None):
                got = _ok(store, wide, given, 100, flags, KM.model("hub", 100, 100, flags), ("complete", flags))
            assert got[3]["n_graph_edges"] == 2485 and got[3]["n_tree"] == 70
        _, rows, counts = KM.graph("hub", KG.HUB_K)
        for flags in (KM.MUTUAL, KM.EITHER):
            for kk in (KG.HUB_K, 3):
                got = _ok(store, rows, counts, kk, flags, KM.model("hub", KG.HUB_K, kk, flags), ("hub", kk, flags))
                _cuts_agree_with_cluster_knn(store, rows, counts, kk, flags, got[0], got[3]["max_weight"])


def test_the_duplicates_one_word_with_8525_listers(vc):
    codes, rows, counts = KM.graph("dup", KG.DUP_K)
    with _make(vc, codes) as store:
        for flags in (KM.MUTUAL, KM.EITHER):
            got = _ok(store, rows, counts, KG.DUP_K, flags, KM.model("dup", KG.DUP_K, KG.DUP_K, flags), ("dup", flags))
            _cuts_agree_with_cluster_knn(store, rows, counts, KG.DUP_K, flags, got[0], got[3]["max_weight"])
        assert got[3]["n_tree"] == 8998


def test_a_code_and_its_complement(vc):
    codes, rows, counts = KM.graph("pair", 3)
    with _make(vc, codes) as store:
        for flags in (KM.MUTUAL, KM.EITHER):
            got = _ok(store, rows, counts, 3, flags, KM.model("pair", 3, 3, flags), ("pair", flags))
            assert tuple(got[0][0]) == (0, 1, 512, 512) and int(got[2][512]) == 1
            _cuts_agree_with_cluster_knn(store, rows, counts, 3, flags, got[0], 512, heights=list(range(0, 514)) + [KM.NO_CAP])


# ---- 5. id_base, NULL outputs, tiny stores --------------------------------------------------------------------------------------------------------------
def test_a_high_id_base_and_null_outputs(vc):
    id_base = 1000
    codes, rows, counts = KM.graph("small", 12, id_base)
    with _make(vc, codes, id_base=id_base) as store:
        for flags in (KM.MUTUAL, KM.EITHER):
            want = KM.model("small", 12, 10, flags, id_base=id_base)
            got = _ok(store, rows, counts, 10, flags, want, ("id_base", flags))
            assert int(got[0]["a"].min()) >= id_base and int(got[1].min()) >= id_base
            _cuts_agree_with_cluster_knn(store, rows, counts, 10, flags, got[0], got[3]["max_weight"])
            _ok(store, rows, counts, 10, flags, want, ("no labels", flags), with_labels=False)
            _ok(store, rows, counts, 10, flags, want, ("no hist", flags), with_hist=False)
            _ok(store, rows, counts, 10, flags, want, ("nothing but the edges", flags), with_labels=False, with_hist=False, with_stats=False)
    high = 2 ** 32 - 5000
    codes, rows, counts = KM.graph("small", 12, high)
    with _make(vc, codes, id_base=high) as store:
        _ok(store, rows, counts, 10, KM.EITHER, KM.model("small", 12, 10, KM.EITHER, id_base=high), "ids near 2^32")


def test_tiny_stores(vc):
    codes = KG.hub_case()[0]
    for m in (2, 1):
        rows, counts = KG.model_rows(codes[:m], 3, 40)
        with _make(vc, codes[:m], id_base=40) as store:
            for flags in (KM.MUTUAL, KM.EITHER):
                want = KM.mst_model(rows, counts, 3, flags, id_base=40)
                for given in (counts, None):
                    got = _ok(store, rows, given, 3, flags, want, ("tiny", m, flags))
                if m == 1:
                    assert len(got[0]) == 0 and got[1].tolist() == [40] and got[3] == dict(KM.zero_stats(), n_clusters=1) and not got[2].any()
                else:
                    assert len(got[0]) == 1 and (int(got[0][0]["a"]), int(got[0][0]["b"])) == (40, 41) and got[1].tolist() == [40, 40]
                KM.same_mst(store.knn_mst(rows, counts, 3, flags), want, ("tiny host", m, flags))
                assert store.mst_cut(want[0], KM.NO_CAP)[1] == 1
                alone, count = store.mst_cut(np.zeros(0, dtype=KM.EDGE), 0)                  # no edge at all: every record its own label
                assert alone.tolist() == list(range(40, 40 + m)) and count == m
    with vc.Engine(64, capacity=4, n_tables=2) as store:                       # N == 0: VC_OK, zero stats
        for flags in (KM.MUTUAL, KM.EITHER):
            edges, labels, hist, st = store.knn_mst(np.zeros((0, 3), dtype=np.uint64), None, 3, flags)
            assert len(edges) == 0 and len(labels) == 0 and not hist.any() and st == KM.zero_stats()
            words, labels, hist, st = _mst(store, np.zeros((0, 3), dtype=np.uint64), None, 3, flags)
            assert len(words) == 0 and not hist.any() and st == KM.zero_stats()
        labels, count = store.mst_cut(np.zeros(0, dtype=KM.EDGE), 5)
        assert len(labels) == 0 and count == 0


# ---- 6. vc_mst_cut on any edge list ------------------------------------------------------------------------------------------------------------------------
def test_the_cut_takes_any_edge_list_and_refuses_a_foreign_end(vc):
    import torch
    id_base = 300
    codes, rows, counts = KM.graph("small", 12, id_base)
    n = len(codes)
    rng = np.random.default_rng(4)
    with _make(vc, codes, id_base=id_base) as store:
        loose = np.zeros(3000, dtype=KM.EDGE)                                  # no forest: cycles, duplicates, loops, unsorted
        loose["a"], loose["b"] = rng.integers(id_base, id_base + n, 3000), rng.integers(id_base, id_base + n, 3000)
        loose["weight"], loose["dist"] = rng.integers(0, 9, 3000), 0xDEAD
        loose[7]["b"] = loose[7]["a"]
        for h in (0, 3, 8, KM.NO_CAP):
            want = KM.cut_model(n, loose, h, id_base)
            labels, count = store.mst_cut(loose, h)
            assert np.array_equal(labels, want[0]) and count == want[1], h
        forest = KM.model("small", 12, 10, KM.EITHER, id_base=id_base)[0]
        shuffled = forest[rng.permutation(len(forest))]
        assert np.array_equal(store.mst_cut(shuffled, 1)[0], store.mst_cut(forest, 1)[0])
        # the labels feed vc_group_summary unchanged
        labels, count = store.mst_cut(forest, 1)
        groups = store.group_summary(labels)[0]
        assert len(groups) == count and np.array_equal(groups["label"], np.unique(labels))
        for bad_id in (id_base - 1, id_base + n, 0, 0xFFFFFFFF):
            for end in ("a", "b"):
                broken = forest.copy()
                broken[len(broken) // 2][end] = bad_id
                with pytest.raises(vc.VcError) as err:
                    store.mst_cut(broken, KM.NO_CAP)
                assert err.value.code == vc.VC_ERR_INVALID
                d_e, d_l = _to_dev(broken.view(np.uint64)), _stale((n + 1) // 2)
                with pytest.raises(vc.VcError) as err:
                    store.mst_cut_dev(d_e.data_ptr(), len(broken), KM.NO_CAP, d_l.data_ptr() + 8 * PAD)
                torch.cuda.synchronize()
                assert err.value.code == vc.VC_ERR_INVALID
        assert np.array_equal(store.mst_cut(forest, 1)[0], labels)             # and the handle goes on


# ---- 7. the host forms, three shards, call history ----------------------------------------------------------------------------------------------------------
def test_the_host_forms_and_three_shards(vc):
    codes, rows, counts = KM.graph("small", 12)
    with _make(vc, codes) as store, _make(vc, codes, shards=3) as sharded:
        for kk, flags, max_dist, kind, min_pts in ((10, KM.MUTUAL, KM.NO_CAP, KM.DISTANCE, 1), (10, KM.EITHER, KM.NO_CAP, KM.DISTANCE, 1),
                                                   (5, KM.EITHER, 2, KM.DISTANCE, 1), (10, KM.EITHER, KM.NO_CAP, KM.REACHABILITY, 4), (1, KM.MUTUAL, 16, KM.DISTANCE, 1)):
            want = KM.model("small", 12, kk, flags, max_dist, 0, kind, min_pts)
            kw = dict(max_dist=max_dist, kind=kind, min_pts=min_pts)
            single = _ok(store, rows, counts, kk, flags, want, ("device", kk, flags), **kw)
            KM.same_mst(store.knn_mst(rows, counts, kk, flags, max_dist, kind, min_pts), single, ("host", kk, flags))
            KM.same_mst(store.knn_mst(rows, None, kk, flags, max_dist, kind, min_pts), single, ("host, no counts", kk, flags))
            got = store.knn_mst(rows, counts, kk, flags, max_dist, kind, min_pts, with_labels=False, with_hist=False)
            assert got[1] is None and got[2] is None and np.array_equal(got[0], single[0])
            KM.same_mst(_ok(sharded, rows, counts, kk, flags, want, ("sharded", kk, flags), **kw), single, ("sharded", kk, flags), rounds=True)
            KM.same_mst(sharded.knn_mst(rows, counts, kk, flags, max_dist, kind, min_pts), single, ("sharded host", kk, flags), rounds=True)
            for h in (0, 1, 2, KM.NO_CAP):
                a, b = store.mst_cut(single[0], h), sharded.mst_cut(single[0], h)
                assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[0], KM.cut_model(len(codes), single[0], h)[0])
        # the host form writes M edges and no more
        want = KM.model("small", 12, 10, KM.MUTUAL)
        n, M = len(codes), len(want[0])
        assert 0 < M < n - 1
        for L_fn, h in ((store._L.vc_knn_mst, store._h), (sharded._L.vc_sharded_knn_mst, sharded._h)):
            edges, st = np.full(2 * (n - 1), STALE, dtype=np.uint64), vc.VcKnnMstStats()
            g, c = np.ascontiguousarray(rows), np.ascontiguousarray(counts)
            assert L_fn(h, g.ctypes.data, c.ctypes.data, 12, 10, KM.MUTUAL, KM.NO_CAP, KM.DISTANCE, 1, edges.ctypes.data, None, None, C.byref(st)) == vc.VC_OK
            assert np.array_equal(edges[:2 * M].view(KM.EDGE), want[0]) and np.all(edges[2 * M:] == STALE) and st.n_tree == M


def test_two_shapes_in_a_row_on_one_handle(vc):
    """the grow-only scratch leaves nothing behind: a large call, a small one, the large one again, other graph readers in between"""
    codes, rows, counts = KM.graph("clustered", 12)
    with _make(vc, codes) as store:
        first = {}
        for step, (kk, flags) in enumerate(((10, KM.EITHER), (1, KM.MUTUAL), (10, KM.EITHER), (3, KM.EITHER), (10, KM.MUTUAL), (1, KM.MUTUAL), (10, KM.EITHER))):
            got = _ok(store, rows, counts, kk, flags, KM.model("clustered", 12, kk, flags), ("history", step, kk, flags))
            if (kk, flags) in first:
                assert np.array_equal(got[0], first[kk, flags][0]) and got[3] == first[kk, flags][3]
            first.setdefault((kk, flags), got)
            if step % 2:
                assert store.cluster_knn(rows, counts, 5)[2]["n_edges"] == 5 * len(codes)
            else:
                assert store.knn_adjacency(rows, counts, 3, KM.EITHER)[2]["n_edges"] == 3 * len(codes)
            assert store.mst_cut(got[0], 1)[1] == len(codes) - int((got[0]["weight"] <= 1).sum())


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_untouched(vc):
    """all eight entry points; nothing is dereferenced before the checks, so host addresses serve the device forms too"""
    codes, rows, counts = KM.graph("small", 12)
    n, p = len(codes), lambda a: a.ctypes.data
    g = np.ascontiguousarray(rows)
    edges, labels, hist = np.full(2 * n, STALE, dtype=np.uint64), np.full(n, STALE, dtype=np.uint64), np.full(65, STALE, dtype=np.uint64)
    with _make(vc, codes) as store, _make(vc, codes, shards=3) as sharded:
        for L_fn, h, dev in ((store._L.vc_knn_mst, store._h, False), (store._L.vc_knn_mst_dev, store._h, True),
                             (sharded._L.vc_sharded_knn_mst, sharded._h, False), (sharded._L.vc_sharded_knn_mst_dev, sharded._h, True)):
            st = vc.VcKnnMstStats(7, 7, 7, 7, 7, 7, 7)
            out = (p(edges), p(labels), p(hist))
            for args in ((None, p(g), None, 12, 10, 1, 64, 0, 1) + out,                    # a null handle
                         (h, None, None, 12, 10, 1, 64, 0, 1) + out,                       # null rows
                         (h, p(g), None, 12, 10, 1, 64, 0, 1, None, p(labels), p(hist)),   # null edges
                         (h, p(g), None, 0, 0, 1, 64, 0, 1) + out,                         # k out of range
                         (h, p(g), None, KG.MAX_K, 10, 1, 64, 0, 1) + out,
                         (h, p(g), None, 12, 0, 1, 64, 0, 1) + out,                        # kk out of range
                         (h, p(g), None, 12, 13, 1, 64, 0, 1) + out,
                         (h, p(g), None, 12, 10, 2, 64, 0, 1) + out,                       # VC_KNN_REVERSE
                         (h, p(g), None, 12, 10, 3, 64, 0, 1) + out,
                         (h, p(g), None, 12, 10, 0x80000001, 64, 0, 1) + out,
                         (h, p(g), None, 12, 10, 1, 64, 2, 1) + out,                       # an unknown weight kind
                         (h, p(g), None, 12, 10, 1, 64, 0, 0) + out,                       # min_pts under DISTANCE must be 1
                         (h, p(g), None, 12, 10, 1, 64, 0, 2) + out,
                         (h, p(g), None, 12, 10, 1, 64, 1, 0) + out,                       # min_pts under REACHABILITY: 1 .. k + 1
                         (h, p(g), None, 12, 10, 1, 64, 1, 14) + out):
                assert L_fn(*args, C.byref(st), *((None,) if dev else ())) == vc.VC_ERR_INVALID, (dev, args)
                assert np.all(edges == STALE) and np.all(labels == STALE) and np.all(hist == STALE)
                assert st.as_dict() == dict.fromkeys(KM.MST_STATS, 7)
        count = C.c_uint64(7)
        for L_fn, h, dev in ((store._L.vc_mst_cut, store._h, False), (store._L.vc_mst_cut_dev, store._h, True),
                             (sharded._L.vc_sharded_mst_cut, sharded._h, False), (sharded._L.vc_sharded_mst_cut_dev, sharded._h, True)):
            for args in ((None, p(edges), 5, 3, p(labels)), (h, None, 5, 3, p(labels)), (h, p(edges), 5, 3, None)):
                assert L_fn(*args, C.byref(count), *((None,) if dev else ())) == vc.VC_ERR_INVALID, (dev, args)
                assert np.all(labels == STALE) and count.value == 7
        with pytest.raises(vc.VcError) as err:                                             # through the wrappers
            store.knn_mst(rows, counts, 13, KM.MUTUAL)
        assert err.value.code == vc.VC_ERR_INVALID
        with pytest.raises(vc.VcError) as err:
            store.knn_mst(rows, counts, 10, KM.REVERSE)
        assert err.value.code == vc.VC_ERR_INVALID and "VC_KNN_MUTUAL or VC_KNN_EITHER" in str(err.value)


def test_too_many_items_are_refused_before_the_rows_are_read(vc):
    """N kk > 2^31 - 1 with a one-word dummy for the rows: the refusal comes before the pointer is dereferenced"""
    n, k = 262177, 8191
    assert not KM.items_ok(n, k) and KM.items_ok(n - 1, k)
    dummy, edges = np.zeros(1, dtype=np.uint64), np.full(4, STALE, dtype=np.uint64)
    with vc.Engine(64, capacity=n, n_tables=2) as store:
        store.add_synthetic(n, seed=3, kind=vc.SYNTH_UNIFORM)
        assert len(store) == n
        for L_fn, extra in ((store._L.vc_knn_mst, ()), (store._L.vc_knn_mst_dev, (None,))):
            for flags in (KM.MUTUAL, KM.EITHER):
                assert L_fn(store._h, dummy.ctypes.data, None, k, k, flags, KM.NO_CAP, KM.DISTANCE, 1, edges.ctypes.data, None, None, None, *extra) == vc.VC_ERR_INVALID
        assert np.all(edges == STALE) and "2^31 - 1" in store._L.vc_last_error(store._h).decode()


def test_a_corrupted_graph_is_refused_on_the_device(vc):
    """a count above k, a foreign id, the row's own id: VC_ERR_INVALID, the pads intact, and the handle goes on"""
    import torch
    id_base, k, kk = 300, 12, 10
    codes, rows, counts = KM.graph("small", k, id_base)
    n = len(codes)
    broken = counts.copy()
    broken[n - 1] = k + 1
    foreign = rows.copy()
    foreign[5, 1] = (foreign[5, 1] & np.uint64(0xFFFFFFFF00000000)) | np.uint64(n + id_base)
    own = rows.copy()
    own[n // 2, kk - 1] = (own[n // 2, kk - 1] & np.uint64(0xFFFFFFFF00000000)) | np.uint64(n // 2 + id_base)
    with _make(vc, codes, id_base=id_base) as store:
        for flags in (KM.MUTUAL, KM.EITHER):
            for r, c in ((rows, broken), (foreign, counts), (own, counts), (own, None)):
                for kind, min_pts in ((KM.DISTANCE, 1), (KM.REACHABILITY, 4)):
                    with pytest.raises(vc.VcError) as err:
                        _mst(store, r, c, kk, flags, kind=kind, min_pts=min_pts)          # (_inner inside is not reached: the call raises)
                    torch.cuda.synchronize()
                    assert err.value.code == vc.VC_ERR_INVALID
                    with pytest.raises(vc.VcError) as err:
                        store.knn_mst(r, c, kk, flags, weight_kind=kind, min_pts=min_pts)
                    assert err.value.code == vc.VC_ERR_INVALID
            _ok(store, rows, counts, kk, flags, KM.model("small", k, kk, flags, id_base=id_base), ("after the refusal", flags))
