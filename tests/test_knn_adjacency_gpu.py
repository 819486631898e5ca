"""The reverse, mutual and symmetrised k-NN graph in CSR form: vc_knn_adjacency* and its vc_sharded_* forms.

The expectation is knn_adjacency_common.py's numpy model -- knn_graph_common's edge sets, the (target, dist, neighbour) triples,
np.lexsort -- pinned against plain loops by test_knn_adjacency_cpu.py, which also shows that the inputs below reach segments longer
than a sub-tile of the sort, the merge's block team, thousands of empty segments, both distance passes and three key passes.
Offsets, segments and statistics are integer functions of the graph and the call, so every comparison is exact equality on every
word; device outputs are pre-filled with a stale pattern and padded, so every word of offsets[0 .. N] and adj[0 .. T) is proven
written and adj[T .. cap) and the words around both outputs proven untouched.  One device.

Not tested: the sharded forms across real devices, N kk near 2^31 - 1 on the device (the limit itself is refused below and checked
in tests/cpp/knn_adjacency_plan_test.cc), and rows that are no vc_knn_graph* rows beyond the three the device refuses."""
import ctypes as C
import functools

import numpy as np
import pytest

import knn_adjacency_common as KA
import knn_graph_common as KG

pytestmark = pytest.mark.gpu

PAD = 3          # stale words kept on both sides of every device output
STALE = KA.STALE64


def _make(vc, codes, id_base=0, shards=0, index=False):
    bits = codes.shape[1] * 8
    if shards:
        e = vc.ShardedEngine(bits, capacity=len(codes) + 10, n_shards=shards, devices=[0], id_base=id_base, n_tables=KG.TABLES[bits])
    else:
        e = vc.Engine(bits, capacity=max(len(codes), 1), id_base=id_base, n_tables=KG.TABLES[bits])
    if len(codes):
        e.add_codes(codes)
    if index:
        e.build_index()
    return e


def _to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    signed = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(a.view(signed).copy()).cuda()


def _stale(n_words):
    return _to_dev(np.full(n_words + 2 * PAD, STALE, dtype=np.uint64))


def _inner(buf, n_words, what):
    """the n_words words between the pads of a synchronised buffer; the pads must still be stale"""
    raw = buf.cpu().numpy().view(np.uint64)
    assert np.all(raw[:PAD] == STALE) and np.all(raw[PAD + n_words:] == STALE), (what, "words around the output")
    return raw[PAD:PAD + n_words]


def _adj(store, rows, counts, kk, flags, max_dist=KA.NO_CAP, cap=None, with_stats=True, with_adj=True):
    """vc_knn_adjacency_dev on stale-filled outputs: (rc, offsets [N + 1], the whole adj buffer [cap], stats | None)"""
    import torch
    n, k = rows.shape
    cap = KA.bound(n, kk, flags) if cap is None else cap
    d_r, d_c = _to_dev(rows if n else np.zeros((1, 1), dtype=np.uint64)), _to_dev(counts) if counts is not None else None
    d_o, d_a = _stale(n + 1), _stale(cap)
    torch.cuda.synchronize()
    rc, st = store.knn_adjacency_dev(d_r.data_ptr(), d_c.data_ptr() if counts is not None else None, k, kk, d_a.data_ptr() + 8 * PAD if with_adj else None,
                                     cap if with_adj else 0, d_o.data_ptr() + 8 * PAD, flags=flags, max_dist=max_dist, with_stats=with_stats)
    torch.cuda.synchronize()
    return rc, _inner(d_o, n + 1, "offsets"), _inner(d_a, cap, "adj"), st


def _ok(vc, store, rows, counts, kk, flags, want, what, max_dist=KA.NO_CAP, cap=None):
    """a call that must succeed: offsets, adj[0 .. T) and the stats are the model's, adj[T .. cap) is still stale"""
    rc, offsets, adj, st = _adj(store, rows, counts, kk, flags, max_dist, cap)
    assert rc == vc.VC_OK, (what, rc)
    T = int(want[0][-1])
    KA.same_adjacency((offsets, adj[:T], st), want, what)
    assert np.all(adj[T:] == STALE), (what, "beyond T")
    return offsets, adj[:T], st


@functools.lru_cache(maxsize=None)
def _graph(name, k, id_base=0):
    codes = {"clustered": lambda: KG.clustered_case(64, n=2000), "dup": KG.dup_case, "hub": lambda: KG.hub_case()[0],
             "c256": lambda: KA.complement_case(256), "c512": lambda: KA.complement_case(512), "small": lambda: KG.clustered_case(64, n=700)}[name]()
    rows, counts = KG.model_rows(codes, k, id_base)
    rows.setflags(write=False)
    return codes, rows, counts


@functools.lru_cache(maxsize=None)
def _models(name, k, kk, max_dist=KA.NO_CAP, id_base=0):
    _, rows, counts = _graph(name, k, id_base)
    return KA.adjacency_models(rows, counts, kk, max_dist, id_base)


# ---- 1. the sweep ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kk", [10, 1])
def test_sweep_against_the_model(vc, kk):
    """20 000 items cross a block of the sort (kk = 10), 2 000 do not (kk = 1); all three flags, with and without the cap, counts
    given and NULL"""
    codes, rows, counts = _graph("clustered", 12)
    with _make(vc, codes) as store:
        for max_dist in (KA.NO_CAP, 64 // 4):
            for flags in KA.FLAGS:
                for given in (counts, None):
                    _ok(vc, store, rows, given, kk, flags, _models("clustered", 12, kk, max_dist)[flags], (kk, max_dist, flags, given is None), max_dist)


# ---- 2. hubs -----------------------------------------------------------------------------------------------------------------------------------
def test_the_duplicates_hubs_and_empty_segments(vc):
    """dup_case() at k = kk = 5: a segment of 8 525 words -- a run over three sub-tiles of the sort, the merge's block team -- and
    8 550 empty segments"""
    codes, rows, counts = _graph("dup", KG.DUP_K)
    with _make(vc, codes) as store:
        for flags in KA.FLAGS:
            want = _models("dup", KG.DUP_K, KG.DUP_K)[flags]
            _ok(vc, store, rows, counts, KG.DUP_K, flags, want, ("dup", flags))
        assert _models("dup", KG.DUP_K, KG.DUP_K)[KA.REVERSE][2]["max_degree"] == 8525


def test_the_hub_set_and_short_rows(vc):
    codes, rows, counts = _graph("hub", KG.HUB_K)
    with _make(vc, codes) as store:
        for flags in KA.FLAGS:
            for kk in (KG.HUB_K, 3):
                _ok(vc, store, rows, counts, kk, flags, _models("hub", KG.HUB_K, kk)[flags], ("hub", kk, flags))
        n, k = len(codes), 100
        assert n == 71 < k
        _, wide, wide_counts = _graph("hub", k)
        assert np.all(wide_counts == n - 1)                                    # every row holds the whole store
        for flags in KA.FLAGS:
            want = _models("hub", k, k)[flags]
            assert np.all(np.diff(want[0].astype(np.int64)) == n - 1)          # so every record is in every segment
            _ok(vc, store, wide, wide_counts, k, flags, want, ("short rows", flags))
            _ok(vc, store, wide, None, k, flags, want, ("short rows, no counts", flags))


# ---- 3. two distance passes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c256", "c512"])
def test_distances_on_both_sides_of_256(vc, name):
    codes, rows, counts = _graph(name, 100)
    with _make(vc, codes) as store:
        for flags in KA.FLAGS:
            _ok(vc, store, rows, counts, 100, flags, _models(name, 100, 100)[flags], (name, flags))
            _ok(vc, store, rows, counts, 100, flags, _models(name, 100, 100, 255)[flags], (name, flags, "one pass under the cap"), 255)


# ---- 4. three key passes ---------------------------------------------------------------------------------------------------------------------------
def test_a_store_above_two_key_bytes(vc):
    """66 000 random codes at k = kk = 2: the keys take three passes.  The rows are the engine's own LINEAR graph, 200 of them
    checked against the model; the expectation is the model over those rows"""
    n, k = 66000, 2
    codes = np.random.default_rng(66).integers(0, 256, size=(n, 8), dtype=np.uint8)
    assert KA.key_passes(n) == 3
    with _make(vc, codes) as store:
        rows, counts = store.knn_graph(k, mode=KG.LINEAR)
        for first in range(100, n, n // 8):
            KG.same_graph((rows[first:first + 25], counts[first:first + 25]), KG.model_rows(codes, k, first=first, count=25), ("linear graph", first))
        want = KA.adjacency_models(rows, counts, k)
        for flags in KA.FLAGS:
            _ok(vc, store, rows, counts, k, flags, want[flags], ("66000", flags))


# ---- 5. agreement with vc_cluster_knn_dev ------------------------------------------------------------------------------------------------------
def test_agreement_with_cluster_knn_on_the_same_graph(vc):
    import torch
    codes, rows, counts = _graph("small", 12)
    n = len(codes)
    with _make(vc, codes) as store:
        d_r, d_c = _to_dev(rows), _to_dev(counts)
        for kk, max_dist in ((10, KA.NO_CAP), (4, 2)):
            got = {}
            for flags in KA.FLAGS:
                rc, offsets, adj, st = _adj(store, rows, counts, kk, flags, max_dist)
                assert rc == vc.VC_OK
                got[flags] = (offsets, adj[:int(offsets[n])], st)
            for flags in (KG.MUTUAL, KG.EITHER):
                d_l, d_d = _to_dev(np.zeros(n, dtype=np.uint32)), _to_dev(np.zeros(n, dtype=np.uint32))
                cl = store.cluster_knn_dev(d_r.data_ptr(), d_c.data_ptr(), 12, kk, d_l.data_ptr(), d_d.data_ptr(), flags=flags, max_dist=max_dist)
                torch.cuda.synchronize()
                labels, deg = d_l.cpu().numpy().view(np.uint32), d_d.cpu().numpy().view(np.uint32)
                assert np.array_equal(np.diff(got[KA.REVERSE][0].astype(np.int64)), deg), (kk, "in-degrees")
                assert all(got[f][2]["n_edges"] == cl["n_edges"] for f in KA.FLAGS) and got[KA.REVERSE][2]["max_degree"] == cl["max_in_degree"]
                assert got[KA.REVERSE][2]["n_entries"] == cl["n_edges"] and got[KA.MUTUAL][2]["n_entries"] == 2 * cl["n_mutual"]
                assert got[KA.EITHER][2]["n_entries"] == 2 * (cl["n_edges"] - cl["n_mutual"])
                assert np.array_equal(KA.components(*got[flags][:2]), labels), (kk, flags, "components")


# ---- 6. the exact-MIH graph --------------------------------------------------------------------------------------------------------------------
def test_the_exact_mih_graph_with_a_high_id_base(vc):
    id_base, k, kk = 2 ** 32 - 5000, 12, 10
    codes = KG.clustered_case(128, n=700)
    with _make(vc, codes, id_base=id_base, index=True) as store:
        rows, counts = store.knn_graph(k, mode=KG.MIH_EXACT)
        KG.same_graph((rows, counts), KG.model_rows(codes, k, id_base), "mih graph")
        want = KA.adjacency_models(rows, counts, kk, KA.NO_CAP, id_base)
        for flags in KA.FLAGS:
            _, adj, _ = _ok(vc, store, rows, counts, kk, flags, want[flags], ("mih", flags))
            assert int((adj & np.uint64(0xFFFFFFFF)).min()) >= id_base


# ---- 7. capacity -------------------------------------------------------------------------------------------------------------------------------
def test_the_capacity_protocol(vc):
    codes, rows, counts = _graph("small", 12)
    n, kk = len(codes), 10
    with _make(vc, codes) as store:
        for flags in KA.FLAGS:
            want = _models("small", 12, kk)[flags]
            T = want[2]["n_entries"]
            assert 0 < T <= KA.bound(n, kk, flags)
            rc, offsets, adj, st = _adj(store, rows, counts, kk, flags, cap=T - 1)
            assert rc == vc.VC_ERR_CAPACITY and np.array_equal(offsets, want[0]) and int(offsets[n]) == T and st == want[2], flags
            assert np.all(adj == STALE)                                         # adj is untouched
            _ok(vc, store, rows, counts, kk, flags, want, ("cap = T", flags), cap=T)
            rc, offsets, _, st = _adj(store, rows, counts, kk, flags, with_adj=False)       # the sizing call
            assert rc == vc.VC_ERR_CAPACITY and np.array_equal(offsets, want[0]) and st == want[2], flags
            rc, offsets, adj, st = _adj(store, rows, counts, kk, flags, with_stats=False)    # stats may be NULL
            assert rc == vc.VC_OK and st is None and np.array_equal(offsets, want[0]) and np.array_equal(adj[:T], want[1])
            rc, offsets, adj, st = _adj(store, rows, counts, kk, flags, cap=T - 1, with_stats=False)
            assert rc == vc.VC_ERR_CAPACITY and st is None and np.array_equal(offsets, want[0]) and np.all(adj == STALE)
        # nothing listed at all: T = 0 fits a sizing call
        none = np.full_like(rows, KG.INF)
        none[:, :] = (np.uint64(60) << np.uint64(32)) | rows[:, :] & np.uint64(0xFFFFFFFF)
        for flags in KA.FLAGS:
            rc, offsets, _, st = _adj(store, none, counts, kk, flags, max_dist=3, with_adj=False)
            assert rc == vc.VC_OK and np.all(offsets == 0) and st == dict(n_edges=0, n_entries=0, n_empty=n, max_degree=0)


# ---- 8. the host form and three shards -------------------------------------------------------------------------------------------------------------
def test_the_host_form_and_three_shards(vc):
    codes, rows, counts = _graph("small", 12)
    with _make(vc, codes) as store, _make(vc, codes, shards=3) as sharded:
        for kk, flags, max_dist in ((10, KA.REVERSE, KA.NO_CAP), (10, KA.EITHER, KA.NO_CAP), (10, KA.MUTUAL, KA.NO_CAP), (5, KA.EITHER, 2), (1, KA.REVERSE, 16)):
            want = _models("small", 12, kk, max_dist)[flags]
            single = _ok(vc, store, rows, counts, kk, flags, want, ("device", kk, flags), max_dist)
            KA.same_adjacency(store.knn_adjacency(rows, counts, kk, flags, max_dist), single, ("host", kk, flags))
            KA.same_adjacency(store.knn_adjacency(rows, None, kk, flags, max_dist), single, ("host, no counts", kk, flags))
            KA.same_adjacency(_ok(vc, sharded, rows, counts, kk, flags, want, ("sharded", kk, flags), max_dist), single, ("sharded", kk, flags))
            KA.same_adjacency(sharded.knn_adjacency(rows, counts, kk, flags, max_dist), single, ("sharded host", kk, flags))
        # the host form's capacity protocol: the offsets come home, adj stays as it was
        want = _models("small", 12, 10)[KA.EITHER]
        n, T = len(codes), want[2]["n_entries"]
        for L_fn, h in ((store._L.vc_knn_adjacency, store._h), (sharded._L.vc_sharded_knn_adjacency, sharded._h)):
            offsets, adj, st = np.full(n + 1, STALE, dtype=np.uint64), np.full(T, STALE, dtype=np.uint64), vc.VcKnnAdjacencyStats()
            g, c = np.ascontiguousarray(rows), np.ascontiguousarray(counts)
            assert L_fn(h, g.ctypes.data, c.ctypes.data, 12, 10, KA.EITHER, KA.NO_CAP, adj.ctypes.data, T - 1, offsets.ctypes.data, C.byref(st)) == vc.VC_ERR_CAPACITY
            assert np.array_equal(offsets, want[0]) and np.all(adj == STALE) and st.as_dict() == want[2]
            assert L_fn(h, g.ctypes.data, c.ctypes.data, 12, 10, KA.EITHER, KA.NO_CAP, None, 0, offsets.ctypes.data, None) == vc.VC_ERR_CAPACITY
            assert L_fn(h, g.ctypes.data, c.ctypes.data, 12, 10, KA.EITHER, KA.NO_CAP, adj.ctypes.data, T, offsets.ctypes.data, None) == vc.VC_OK
            assert np.array_equal(adj, want[1])


# ---- 9. call history -------------------------------------------------------------------------------------------------------------------------------
def test_call_history_leaves_every_word_the_same(vc):
    codes, rows, counts = _graph("small", 12)
    with _make(vc, codes) as store:
        first = {}
        for step, (kk, flags) in enumerate(((10, KA.EITHER), (3, KA.REVERSE), (10, KA.MUTUAL), (10, KA.REVERSE), (3, KA.EITHER), (10, KA.EITHER), (3, KA.REVERSE),
                                            (10, KA.MUTUAL), (3, KA.MUTUAL), (10, KA.REVERSE))):
            got = _ok(vc, store, rows, counts, kk, flags, _models("small", 12, kk)[flags], ("history", step, kk, flags))
            if (kk, flags) in first:
                assert np.array_equal(got[0], first[kk, flags][0]) and np.array_equal(got[1], first[kk, flags][1]) and got[2] == first[kk, flags][2]
            first.setdefault((kk, flags), got)
            if step % 2:                                                       # other readers of the graph in between
                assert store.cluster_knn(rows, counts, 5)[2]["n_edges"] == 5 * len(codes)
            else:
                assert store.cluster_snn(rows, counts, 10, 3)[3]["n_edges"] == 10 * len(codes)


# ---- 10. errors --------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_untouched(vc):
    """all four entry points; nothing is dereferenced before the checks, so host addresses serve the device forms too"""
    codes, rows, counts = _graph("small", 12)
    n, p = len(codes), lambda a: a.ctypes.data
    g = np.ascontiguousarray(rows)
    adj, offs = np.full(2 * n * 12, STALE, dtype=np.uint64), np.full(n + 1, STALE, dtype=np.uint64)
    with _make(vc, codes) as store, _make(vc, codes, shards=3) as sharded:
        for L_fn, h, dev in ((store._L.vc_knn_adjacency, store._h, False), (store._L.vc_knn_adjacency_dev, store._h, True),
                             (sharded._L.vc_sharded_knn_adjacency, sharded._h, False), (sharded._L.vc_sharded_knn_adjacency_dev, sharded._h, True)):
            st = vc.VcKnnAdjacencyStats(7, 7, 7, 7, 7)
            for args in ((None, p(g), None, 12, 10, 2, 64, p(adj), len(adj), p(offs)),            # a null handle
                         (h, None, None, 12, 10, 2, 64, p(adj), len(adj), p(offs)),                # null rows
                         (h, p(g), None, 12, 10, 2, 64, p(adj), len(adj), None),                   # null offsets
                         (h, p(g), None, 12, 10, 2, 64, None, 1, p(offs)),                         # null adj with a capacity
                         (h, p(g), None, 0, 0, 2, 64, p(adj), len(adj), p(offs)),                  # k out of range
                         (h, p(g), None, KG.MAX_K, 10, 2, 64, p(adj), len(adj), p(offs)),
                         (h, p(g), None, 12, 0, 2, 64, p(adj), len(adj), p(offs)),                 # kk out of range
                         (h, p(g), None, 12, 13, 2, 64, p(adj), len(adj), p(offs)),                # kk > k
                         (h, p(g), None, 12, 10, 3, 64, p(adj), len(adj), p(offs)),                # flags = 3
                         (h, p(g), None, 12, 10, 0x80000001, 64, p(adj), len(adj), p(offs))):
                assert L_fn(*args, C.byref(st), *((None,) if dev else ())) == vc.VC_ERR_INVALID, (dev, args)
                assert np.all(adj == STALE) and np.all(offs == STALE)
                assert (st.n_edges, st.n_entries, st.n_empty, st.max_degree) == (7, 7, 7, 7)
        with pytest.raises(vc.VcError) as err:                                                      # through the wrappers
            _adj(store, rows, counts, 13, KA.REVERSE)
        assert err.value.code == vc.VC_ERR_INVALID


def test_too_many_items_are_refused_before_the_rows_are_read(vc):
    """N kk > 2^31 - 1 with a one-word dummy for the rows: the refusal comes before the pointer is dereferenced"""
    n, k = 262177, 8191
    assert not KA.items_ok(n, k) and KA.items_ok(n - 1, k)
    dummy, offs = np.zeros(1, dtype=np.uint64), np.full(4, STALE, dtype=np.uint64)
    with vc.Engine(64, capacity=n, n_tables=2) as store:
        store.add_synthetic(n, seed=3, kind=vc.SYNTH_UNIFORM)
        assert len(store) == n
        for L_fn, extra in ((store._L.vc_knn_adjacency, ()), (store._L.vc_knn_adjacency_dev, (None,))):
            for flags in KA.FLAGS:
                assert L_fn(store._h, dummy.ctypes.data, None, k, k, flags, KA.NO_CAP, None, 0, offs.ctypes.data, None, *extra) == vc.VC_ERR_INVALID
        assert np.all(offs == STALE) and "2^31 - 1" in store._L.vc_last_error(store._h).decode()


def test_a_corrupted_graph_is_refused_with_both_outputs_stale(vc):
    id_base, k, kk = 300, 12, 10
    codes = KG.clustered_case(64, n=700)
    n = len(codes)
    rows, counts = KG.model_rows(codes, k, id_base)
    want = KA.adjacency_models(rows, counts, kk, KA.NO_CAP, id_base)
    broken = counts.copy()
    broken[n - 1] = k + 1                                                      # a count of k + 1
    foreign = rows.copy()
    foreign[5, 1] = (foreign[5, 1] & np.uint64(0xFFFFFFFF00000000)) | np.uint64(n + id_base)    # an id equal to N + id_base
    own = rows.copy()
    own[n // 2, kk - 1] = (own[n // 2, kk - 1] & np.uint64(0xFFFFFFFF00000000)) | np.uint64(n // 2 + id_base)   # the row's own id
    with _make(vc, codes, id_base=id_base) as store:
        for flags in KA.FLAGS:
            for r, c in ((rows, broken), (foreign, counts), (own, counts), (own, None)):
                import torch
                d_r, d_c = _to_dev(r), _to_dev(c) if c is not None else None
                d_o, d_a = _stale(n + 1), _stale(KA.bound(n, kk, flags))
                torch.cuda.synchronize()
                with pytest.raises(vc.VcError) as err:
                    store.knn_adjacency_dev(d_r.data_ptr(), d_c.data_ptr() if c is not None else None, k, kk, d_a.data_ptr() + 8 * PAD, KA.bound(n, kk, flags),
                                            d_o.data_ptr() + 8 * PAD, flags=flags)
                torch.cuda.synchronize()
                assert err.value.code == vc.VC_ERR_INVALID
                assert np.all(d_o.cpu().numpy().view(np.uint64) == STALE) and np.all(d_a.cpu().numpy().view(np.uint64) == STALE), (flags, "an output word was written")
                _ok(vc, store, rows, counts, kk, flags, want[flags], ("after the refusal", flags))


# ---- 11. tiny stores ---------------------------------------------------------------------------------------------------------------------------
def test_tiny_stores(vc):
    codes, _ = KG.hub_case()
    for m in (2, 1):
        rows, counts = KG.model_rows(codes[:m], 3, 40)
        with _make(vc, codes[:m], id_base=40) as store:
            for flags in KA.FLAGS:
                want = KA.adjacency_model(rows, counts, 3, flags, KA.NO_CAP, 40)
                for given in (counts, None):
                    got = _ok(vc, store, rows, given, 3, flags, want, ("tiny", m, flags))
                    if m == 1:
                        assert got[0].tolist() == [0, 0] and len(got[1]) == 0 and got[2] == dict(KA.zero_stats(), n_empty=1)
                    else:
                        d = int(rows[0, 0]) >> 32
                        assert got[0].tolist() == [0, 1, 2] and got[1].tolist() == [(d << 32) | 41, (d << 32) | 40]
                KA.same_adjacency(store.knn_adjacency(rows, counts, 3, flags), want, ("tiny host", m, flags))
    with vc.Engine(64, capacity=4, n_tables=2) as store:                       # N == 0: VC_OK, zero stats, offsets[0] = 0
        for flags in KA.FLAGS:
            offsets, adj, st = store.knn_adjacency(np.zeros((0, 3), dtype=np.uint64), None, 3, flags)
            assert offsets.tolist() == [0] and len(adj) == 0 and st == KA.zero_stats()
            rc, offsets, adj, st = _adj(store, np.zeros((0, 3), dtype=np.uint64), None, 3, flags, cap=2)
            assert rc == vc.VC_OK and offsets.tolist() == [0] and np.all(adj == STALE) and st == KA.zero_stats()
