"""HDBSCAN-style clusters from a spanning forest: vc_mst_condense* and its vc_sharded_* forms.

The expectation is condense_common.py's model -- a plain loop over the levels, straight from the contract's table of cases -- pinned by
test_mst_condense_cpu.py against a top-down formulation over knn_mst_common.cut_model and, for the selection, against a brute force
over all antichains; the same file pins the figures of the forests used here, so no comparison below is vacuous.  Nodes, labels, node,
own, leave and the statistics are integer functions of the edge set per weight and the arguments, so every comparison is exact equality
on every word; device outputs are pre-filled with a stale pattern and padded, so nodes[0 .. n_nodes) and the record arrays are proven
written and nodes[n_nodes ..) and the words around every output proven untouched.  One device.

Not tested: the sharded forms across real devices, forests of more than 9000 records, and min_cluster_size near 2^31 on a store that
large (the limits themselves are refused below and checked in tests/cpp/condense_plan_test.cc)."""
import ctypes as C

import numpy as np
import pytest

import condense_common as CC
import knn_graph_common as KG
import knn_mst_common as KM

pytestmark = pytest.mark.gpu

PAD = 4          # stale 64-bit words kept on both sides of every device output
STALE = KM.STALE64
NODE_WORDS = 6   # 64-bit words of a vc_condensed_node


def _codes(n, bits, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (n, bits // 8), dtype=np.uint8)


def _make(vc, n, bits=64, id_base=0, shards=0):
    if shards:
        e = vc.ShardedEngine(bits, capacity=n + 10, n_shards=shards, devices=[0], id_base=id_base, n_tables=KG.TABLES[bits])
    else:
        e = vc.Engine(bits, capacity=max(n, 1), id_base=id_base, n_tables=KG.TABLES[bits])
    if n:
        e.add_codes(_codes(n, bits))
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


def _edges_dev(edges):
    return _to_dev(edges.view(np.uint64) if len(edges) else np.zeros(2, dtype=np.uint64))


def _condense(store, n, d_edges, n_edges, mcs, root_weight=0, method=CC.EOM, with_node=True, with_own=True, with_leave=True, with_stats=True):
    """vc_mst_condense_dev on stale-filled outputs: (the whole node buffer as 64-bit words [6 (max(N, 1) - 1)], labels [N], node, own,
    leave [N] | None, stats | None); an output that was not asked for must still be stale"""
    import torch
    cap, words = max(n, 1) - 1, (n + 1) // 2
    d_n, d_l, d_s, d_o, d_v = _stale(NODE_WORDS * cap), _stale(words), _stale(words), _stale(words), _stale(words)
    torch.cuda.synchronize()
    at = lambda buf, given=True: buf.data_ptr() + 8 * PAD if given else None
    try:
        st = store.mst_condense_dev(d_edges.data_ptr() if n_edges else None, n_edges, mcs, at(d_n), at(d_l), at(d_s, with_node), at(d_o, with_own), at(d_v, with_leave),
                                    root_weight=root_weight, method=method, with_stats=with_stats)
    finally:
        torch.cuda.synchronize()
    out = [_inner(d_n, NODE_WORDS * cap, "nodes")]
    for buf, given, what in ((d_l, True, "labels"), (d_s, with_node, "node"), (d_o, with_own, "own"), (d_v, with_leave, "leave")):
        raw = _inner(buf, words, what)
        if given:
            if n % 2:
                assert raw.view(np.uint32)[n] == np.array([STALE]).view(np.uint32)[1], (what, "the word behind the array")
            out.append(raw.view(np.uint32)[:n].copy())
        else:
            assert np.all(raw == STALE), (what, "not asked for")
            out.append(None)
    return out + [st]


def _ok(store, n, edges, mcs, want, what, d_edges=None, **kw):
    """a call that must succeed: nodes[0 .. n_nodes), the record arrays and the stats are the model's, nodes[n_nodes ..) is still stale"""
    got = _condense(store, n, _edges_dev(edges) if d_edges is None else d_edges, len(edges), mcs, **kw)
    m = len(want[0])
    got[0], rest = got[0][:NODE_WORDS * m].view(CC.NODE), got[0][NODE_WORDS * m:]
    CC.same(got, want, what)
    assert np.all(rest == STALE), (what, "beyond n_nodes")
    return got


def _all_stale(vc, store, n, d_edges, n_edges, mcs, what, **kw):
    """a call the device refuses: VC_ERR_INVALID and not one output word written"""
    import torch
    cap, words = max(n, 1) - 1, (n + 1) // 2
    bufs = [_stale(NODE_WORDS * cap)] + [_stale(words) for _ in range(4)]
    torch.cuda.synchronize()
    with pytest.raises(vc.VcError) as err:
        store.mst_condense_dev(d_edges.data_ptr(), n_edges, mcs, *[b.data_ptr() + 8 * PAD for b in bufs], **kw)
    torch.cuda.synchronize()
    assert err.value.code == vc.VC_ERR_INVALID, what
    for b in bufs:
        assert np.all(b.cpu().numpy().view(np.uint64) == STALE), (what, "an output word was written")
    return str(err.value)


# ---- 1. the two forests at every parameter --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mcs", [2, 5, 25])
@pytest.mark.parametrize("name", ["attach", "ruler"])
def test_the_forests_against_the_model(vc, name, mcs):
    """min_cluster_size 2, 5, 25; root_weight 0, the largest weight + 1, bits + 1; both methods"""
    n, bits, edges = CC.forest(name)
    top = int(edges["weight"].max())
    with _make(vc, n, bits) as store:
        d_e = _edges_dev(edges)
        for root_weight in (0, top + 1, bits + 1):
            for method in (CC.EOM, CC.LEAF):
                got = _ok(store, n, edges, mcs, CC.model(name, mcs, root_weight, method), (name, mcs, root_weight, method), d_edges=d_e, root_weight=root_weight,
                          method=method)
                assert got[5]["n_clustered"] + got[5]["n_noise"] == n and got[5]["n_nodes"] <= CC.node_bound(n, mcs)
        if mcs == 5:   # every optional output NULL and given
            want = CC.model(name, mcs)
            for mask in range(16):
                kw = dict(with_node=bool(mask & 1), with_own=bool(mask & 2), with_leave=bool(mask & 4), with_stats=bool(mask & 8))
                _ok(store, n, edges, mcs, want, (name, "optional", mask), d_edges=d_e, **kw)


def test_a_high_id_base(vc):
    for id_base in (1000, 2 ** 32 - 5000):
        n, bits, edges = CC.forest("attach", id_base)
        with _make(vc, n, bits, id_base=id_base) as store:
            for mcs, root_weight, method in ((5, 0, CC.EOM), (2, 65, CC.EOM), (5, 65, CC.LEAF)):
                got = _ok(store, n, edges, mcs, CC.model("attach", mcs, root_weight, method, id_base), ("id_base", id_base, mcs), root_weight=root_weight, method=method)
                assert int(got[1].min()) >= id_base and int(got[0]["rep"].min()) >= id_base
                plain = CC.model("attach", mcs, root_weight, method)
                assert np.array_equal(got[1].astype(np.int64) - id_base, plain[1]) and np.array_equal(got[2], plain[2])   # the ids shift, nothing else


def test_the_order_within_a_weight_changes_no_word(vc):
    for name, mcs in (("attach", 5), ("ruler", 2), ("attach", 2)):
        n, bits, edges = CC.forest(name)
        with _make(vc, n, bits) as store:
            want = CC.model(name, mcs, 65)
            for seed in (1, 2, 3):
                mixed = CC.shuffled_within_weights(edges, seed)
                assert not np.array_equal(mixed, edges) and np.array_equal(mixed["weight"], edges["weight"])
                _ok(store, n, mixed, mcs, want, (name, "shuffled", seed), root_weight=65)


# ---- 2. the real pipeline: graph -> spanning forest -> clusters, without leaving the device ---------------------------------------------------------
def test_the_pipeline_on_the_device(vc):
    import torch
    codes, rows, counts = KM.graph("clustered", 12)
    n, mcs = len(codes), 5
    with vc.Engine(64, capacity=n, n_tables=KG.TABLES[64]) as store:
        store.add_codes(codes)
        d_r, d_c = _to_dev(rows), _to_dev(counts)
        for flags in (KM.MUTUAL, KM.EITHER):
            want_edges, _, _, mst = KM.model("clustered", 12, 10, flags, weight_kind=KM.REACHABILITY, min_pts=5)
            d_e = _to_dev(np.zeros(2 * (n - 1), dtype=np.uint64))
            st = store.knn_mst_dev(d_r.data_ptr(), d_c.data_ptr(), 12, 10, d_e.data_ptr(), flags=flags, weight_kind=KM.REACHABILITY, min_pts=5)
            M, top = st["n_tree"], st["max_weight"]
            assert M == len(want_edges) and top == mst["max_weight"]
            for root_weight in (0, top + 1):
                for method in (CC.EOM, CC.LEAF):
                    want = CC.condense_model(n, want_edges, mcs, root_weight, method)
                    got = _ok(store, n, want_edges, mcs, want, ("pipeline", flags, root_weight, method), d_edges=d_e, root_weight=root_weight, method=method)
                    assert got[5]["n_nodes"] > 0
            # every root is selected here once it has a weight to end at: the labels are the cut's at the top height wherever a component
            # has mcs records
            want = CC.condense_model(n, want_edges, mcs, top + 1, CC.EOM)
            assert np.all((want[0]["flags"][(want[0]["flags"] & CC.ROOT) != 0] & CC.SELECTED) != 0) and want[5]["n_selected"] == want[5]["n_roots"] > 0
            got = _ok(store, n, want_edges, mcs, want, ("pipeline, the top", flags), d_edges=d_e, root_weight=top + 1)
            d_l = _to_dev(np.zeros(n, dtype=np.uint32))
            store.mst_cut_dev(d_e.data_ptr(), M, top, d_l.data_ptr())
            torch.cuda.synchronize()
            cut = d_l.cpu().numpy().view(np.uint32)
            sizes = np.bincount(cut, minlength=n)[cut]
            assert np.array_equal(got[1][sizes >= mcs], cut[sizes >= mcs]) and np.any(sizes >= mcs) and np.all(got[2][sizes < mcs] == CC.NONE)


# ---- 3. every level of a 512-bit code, the duplicates, tiny stores ----------------------------------------------------------------------------------
def test_one_chain_of_512_levels(vc):
    n, bits, edges = CC.forest("thermo")
    assert len(np.unique(edges["weight"])) == 512 and int(edges["weight"].max()) >= 511
    with _make(vc, n, bits) as store:
        for mcs, root_weight, method in ((2, 0, CC.EOM), (2, 513, CC.EOM), (3, 513, CC.LEAF), (40, 0, CC.EOM)):
            got = _ok(store, n, edges, mcs, CC.model("thermo", mcs, root_weight, method), ("thermo", mcs, root_weight), root_weight=root_weight, method=method)
            assert got[5]["n_levels"] == 512


def test_the_duplicates_one_level_of_weight_zero(vc):
    """8300 copies of one code: the level of weight 0 makes one component of thousands of singletons, every size into one word"""
    edges = KM.model("dup", KG.DUP_K, KG.DUP_K, KM.EITHER)[0]
    n = KG.DUP_N
    assert int((edges["weight"] == 0).sum()) > 8000
    with _make(vc, n, 64) as store:
        for mcs, root_weight in ((5, 0), (5, 3), (2, 65)):
            got = _ok(store, n, edges, mcs, CC.condense_model(n, edges, mcs, root_weight), ("dup", mcs, root_weight), root_weight=root_weight)
            assert int(got[0]["size"].max()) > 8000 and int(got[0]["form"].min()) == 0


def test_tiny_stores_and_no_edges(vc):
    none = np.zeros(0, dtype=CC.EDGE)
    for m in (1, 2):
        with _make(vc, m, id_base=40) as store:
            got = _ok(store, m, none, 2, CC.condense_model(m, none, 2, id_base=40), ("no edge", m))
            assert len(got[0]) == 0 and got[1].tolist() == list(range(40, 40 + m)) and np.all(got[2] == CC.NONE) and got[5] == dict(CC.zero_stats(), n_noise=m)
            if m == 2:
                pair = CC.to_edges([(1, 0, 7)], 40)
                for mcs, root_weight in ((2, 0), (2, 8), (3, 8), (2, 65)):
                    got = _ok(store, m, pair, mcs, CC.condense_model(m, pair, mcs, root_weight, id_base=40), ("pair", mcs, root_weight), root_weight=root_weight)
                assert got[1].tolist() == [40, 40] and got[0][0]["stability"] == 2 * (65 - 7) and got[5]["n_levels"] == 1
                host = store.mst_condense(pair, 2, 65)
                CC.same(host, CC.condense_model(m, pair, 2, 65, id_base=40), "pair, host form")
    n, bits, edges = CC.forest("attach")
    with _make(vc, n, bits) as store:                                              # a large store without an edge
        got = _ok(store, n, none, 5, CC.condense_model(n, none, 5), "no edge, 3000 records")
        assert np.array_equal(got[1], np.arange(n, dtype=np.uint32)) and got[5]["n_noise"] == n
    with vc.Engine(64, capacity=4, n_tables=2) as store:                           # N == 0: VC_OK, zero stats
        nodes, labels, node, own, leave, st = store.mst_condense(none, 2)
        assert len(nodes) == 0 and len(labels) == 0 and st == CC.zero_stats()
        assert store.mst_condense_dev(None, 0, 2, _stale(1).data_ptr(), _stale(1).data_ptr()) == CC.zero_stats()


# ---- 4. the labels downstream, the host forms, three shards, call history -------------------------------------------------------------------------
def test_the_labels_feed_group_summary_unchanged(vc):
    """d_labels goes into vc_group_summary_dev as it lies on the device"""
    import torch
    n, bits, edges = CC.forest("attach")
    want = CC.model("attach", 5, 65)
    with _make(vc, n, bits) as store:
        words = (n + 1) // 2
        d_l, d_n, d_g = _stale(words), _stale(NODE_WORDS * (n - 1)), _to_dev(np.zeros(3 * n, dtype=np.uint64))
        d_e = _edges_dev(edges)
        store.mst_condense_dev(d_e.data_ptr(), len(edges), 5, d_n.data_ptr() + 8 * PAD, d_l.data_ptr() + 8 * PAD, root_weight=65)
        rc, count = store.group_summary_dev(d_l.data_ptr() + 8 * PAD, n, d_g.data_ptr())
        torch.cuda.synchronize()
        assert rc == vc.VC_OK and np.array_equal(_inner(d_l, words, "labels").view(np.uint32)[:n], want[1])
        groups = d_g.cpu().numpy().view(vc.GROUP_DTYPE)[:count]
        assert np.array_equal(groups["label"], np.unique(want[1]))
        selected = want[0][(want[0]["flags"] & CC.SELECTED) != 0]
        big = groups[np.isin(groups["label"], selected["rep"])]
        assert len(big) == len(selected) == want[5]["n_selected"] and int(groups["size"].sum()) == n


def test_the_host_forms_and_three_shards(vc):
    n, bits, edges = CC.forest("ruler")
    with _make(vc, n, bits) as store, _make(vc, n, bits, shards=3) as sharded:
        for mcs, root_weight, method in ((2, 0, CC.EOM), (5, 65, CC.EOM), (2, 65, CC.LEAF), (25, 40, CC.EOM)):
            want = CC.model("ruler", mcs, root_weight, method)
            single = _ok(store, n, edges, mcs, want, ("device", mcs), root_weight=root_weight, method=method)
            CC.same(store.mst_condense(edges, mcs, root_weight, method), single, ("host", mcs))
            got = store.mst_condense(edges, mcs, root_weight, method, with_node=False, with_own=False, with_leave=False)
            assert got[2] is None and got[3] is None and got[4] is None and np.array_equal(got[1], single[1])
            got = store.mst_condense(edges, mcs, root_weight, method, with_node=False, with_own=False)     # leave without own
            assert got[3] is None and np.array_equal(got[4], single[4])
            CC.same(_ok(sharded, n, edges, mcs, want, ("sharded", mcs), root_weight=root_weight, method=method), single, ("sharded", mcs))
            CC.same(sharded.mst_condense(edges, mcs, root_weight, method), single, ("sharded host", mcs))
        # the host form writes n_nodes nodes and no more
        want = CC.model("ruler", 5)
        m = len(want[0])
        assert 0 < m < n - 1
        e = np.ascontiguousarray(edges)
        for L_fn, h in ((store._L.vc_mst_condense, store._h), (sharded._L.vc_sharded_mst_condense, sharded._h)):
            nodes, labels, st = np.full(NODE_WORDS * (n - 1), STALE, dtype=np.uint64), np.zeros(n, dtype=np.uint32), vc.VcMstCondenseStats()
            assert L_fn(h, e.ctypes.data, len(e), 5, 0, CC.EOM, nodes.ctypes.data, labels.ctypes.data, None, None, None, C.byref(st)) == vc.VC_OK
            assert np.array_equal(nodes[:NODE_WORDS * m].view(CC.NODE), want[0]) and np.all(nodes[NODE_WORDS * m:] == STALE) and st.n_nodes == m
            assert np.array_equal(labels, want[1])


def test_two_shapes_in_a_row_on_one_handle(vc):
    """the grow-only scratch leaves nothing behind: a large call, a small one, the large one again, other readers of the edges in between"""
    n, bits, edges = CC.forest("attach")
    few = edges[:40]
    with _make(vc, n, bits) as store:
        d_e = _edges_dev(edges)
        for step, (part, mcs, root_weight) in enumerate(((edges, 5, 0), (few, 2, 0), (edges, 5, 0), (edges, 25, 65), (few, 2, 65), (edges, 2, 65), (edges, 5, 0))):
            want = CC.model("attach", mcs, root_weight) if part is edges else CC.condense_model(n, part, mcs, root_weight)
            _ok(store, n, part, mcs, want, ("history", step), d_edges=d_e, root_weight=root_weight)
            assert store.mst_cut(edges, 10)[1] == n - int((edges["weight"] <= 10).sum())


# ---- 5. errors ------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_untouched(vc):
    """all four entry points; nothing is dereferenced before the checks, so host addresses serve the device forms too"""
    n, bits, edges = CC.forest("ruler")
    e, p = np.ascontiguousarray(edges), lambda a: a.ctypes.data
    nodes, labels, extra = np.full(NODE_WORDS * n, STALE, dtype=np.uint64), np.full(n, STALE, dtype=np.uint64), np.full(n, STALE, dtype=np.uint64)
    with _make(vc, n, bits) as store, _make(vc, n, bits, shards=3) as sharded:
        for L_fn, h, dev in ((store._L.vc_mst_condense, store._h, False), (store._L.vc_mst_condense_dev, store._h, True),
                             (sharded._L.vc_sharded_mst_condense, sharded._h, False), (sharded._L.vc_sharded_mst_condense_dev, sharded._h, True)):
            st = vc.VcMstCondenseStats(7, 7, 7, 7, 7, 7, 7, 7, 7)
            out = (p(nodes), p(labels), p(extra), p(extra), p(extra))
            for args in ((None, p(e), len(e), 5, 0, 0) + out,                              # a null handle
                         (h, None, len(e), 5, 0, 0) + out,                                 # null edges with n_edges > 0
                         (h, p(e), len(e), 5, 0, 0, None) + out[1:],                       # null nodes
                         (h, p(e), len(e), 5, 0, 0, p(nodes), None) + out[2:],             # null labels
                         (h, p(e), n, 5, 0, 0) + out,                                      # more edges than a forest has
                         (h, p(e), 2 ** 40, 5, 0, 0) + out,
                         (h, p(e), len(e), 0, 0, 0) + out,                                 # min_cluster_size out of range
                         (h, p(e), len(e), 1, 0, 0) + out,
                         (h, p(e), len(e), 2 ** 31 + 1, 0, 0) + out,
                         (h, p(e), len(e), 0xFFFFFFFF, 0, 0) + out,
                         (h, p(e), len(e), 5, bits + 2, 0) + out,                          # root_weight above bits + 1
                         (h, p(e), len(e), 5, 0xFFFFFFFF, 0) + out,
                         (h, p(e), len(e), 5, 0, 2) + out,                                 # an unknown method
                         (h, p(e), len(e), 5, 0, 0x80000000) + out):
                assert L_fn(*args, C.byref(st), *((None,) if dev else ())) == vc.VC_ERR_INVALID, (dev, args)
                assert np.all(nodes == STALE) and np.all(labels == STALE) and np.all(extra == STALE)
                assert st.as_dict() == dict.fromkeys(CC.STATS, 7)
        with pytest.raises(vc.VcError) as err:                                             # through the wrappers
            store.mst_condense(edges, 1)
        assert err.value.code == vc.VC_ERR_INVALID and "min_cluster_size" in str(err.value)
        with pytest.raises(vc.VcError) as err:
            sharded.mst_condense(edges, 5, method=2)
        assert err.value.code == vc.VC_ERR_INVALID
        CC.same(store.mst_condense(edges, 2 ** 31), CC.condense_model(n, edges, 2 ** 31), "the largest min_cluster_size: no node")


def test_a_broken_edge_list_is_refused_on_the_device(vc):
    """an end outside the store, a == b, a weight above bits, descending weights, a root weight not above the last weight: VC_ERR_INVALID
    with every output word still stale; a cycle: VC_ERR_INVALID found when the levels are through, which this library also does before
    it writes an output word; and the handle goes on"""
    id_base = 300
    n, bits, edges = CC.forest("attach", id_base)
    top, mid = int(edges["weight"].max()), len(edges) // 2
    broken = []
    for bad_id in (id_base - 1, id_base + n, 0, 0xFFFFFFFF):
        for end in ("a", "b"):
            e = edges.copy()
            e[mid][end] = bad_id
            broken.append((e, 0, ("foreign", bad_id, end)))
    for at in (0, mid, len(edges) - 1):
        e = edges.copy()
        e[at]["b"] = e[at]["a"]
        broken.append((e, 0, ("loop", at)))
    e = edges.copy()
    e[len(e) - 1]["weight"] = bits + 1
    broken.append((e, 0, "a weight above bits"))
    e = edges.copy()
    e[mid]["weight"] = int(e[mid]["weight"]) + 1
    assert e[mid]["weight"] > e[mid + 1]["weight"]
    broken.append((e, 0, "descending"))
    e = edges.copy()
    e[[0, len(e) - 1]] = e[[len(e) - 1, 0]]
    broken.append((e, 0, "the first and the last exchanged"))
    broken += [(edges, top, "root_weight == the last weight"), (edges, 1, "root_weight below the last weight")]
    with _make(vc, n, bits, id_base=id_base) as store:
        for e, root_weight, what in broken:
            _all_stale(vc, store, n, _edges_dev(e), len(e), 5, what, root_weight=root_weight)
            with pytest.raises(vc.VcError) as err:
                store.mst_condense(e, 5, root_weight)
            assert err.value.code == vc.VC_ERR_INVALID, what
        # a cycle: without its first edge the forest has two components; an edge of it a second time, or an edge between the first
        # and the last record of the larger component, makes n - 1 edges again, ascending, and closes a cycle
        rest = edges[1:]
        parts = KM.cut_model(n, rest, KM.NO_CAP, id_base)[0]
        inside = np.flatnonzero(parts == np.bincount(parts).argmax())
        other = np.zeros(1, dtype=CC.EDGE)
        other[0] = (id_base + int(inside[0]), id_base + int(inside[-1]), top, 0)
        assert KM.cut_model(n, rest, KM.NO_CAP, id_base)[1] == 2 and len(inside) > 2
        for e, what in ((np.concatenate([rest, rest[-1:]]), "an edge twice"), (np.concatenate([rest, other]), "a closing edge")):
            assert len(e) == n - 1 and np.all(np.diff(e["weight"].astype(np.int64)) >= 0)
            assert "cycle" in _all_stale(vc, store, n, _edges_dev(e), len(e), 5, what), what
            with pytest.raises(vc.VcError) as err:
                store.mst_condense(e, 5)
            assert err.value.code == vc.VC_ERR_INVALID, what
        _ok(store, n, edges, 5, CC.model("attach", 5, 0, CC.EOM, id_base), "after the refusals")
