"""One result per label group in k-NN search: vc_search_knn_distinct, vc_search_knn_distinct_dev and their vc_sharded_* forms.

The expectation is distinct_common.py's numpy model -- the round protocol over a brute-force sorted list, pinned against the
minimum-per-label formulation and against plain loops by test_distinct_cpu.py, which also shows that the crafted cases reach what they
are there for.  Rows, row labels, counts and statistics are integer functions of the codes, the labels and the call, so every comparison
is exact equality on every output word; device outputs are pre-filled with a stale pattern, so every word is proven written and the
words around an output proven untouched.  One device; N <= 9000.

Not tested: a count of UINT32_MAX passed on from the search underneath (nothing provokes a give-up on purpose), and the sharded form
across real devices."""
import ctypes as C

import numpy as np
import pytest

import distinct_common as DC
import groups_common as GC

pytestmark = pytest.mark.gpu

PAD = 3          # stale words kept on both sides of every device output


def _make(vc, codes, id_base=0, shards=0, capacity=None, n_tables=0):
    bits, capacity = codes.shape[1] * 8, capacity or max(len(codes), 1)
    if shards:
        e = vc.ShardedEngine(bits, capacity=capacity, n_shards=shards, devices=[0], id_base=id_base, n_tables=n_tables)
    else:
        e = vc.Engine(bits, capacity=capacity, id_base=id_base, n_tables=n_tables)
    if len(codes):
        e.add_codes(codes)
    if n_tables:
        e.build_index()
    return e


def _to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    signed = {1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(a.view(signed).copy()).cuda()


def _stale(n_words, dtype):
    return _to_dev(np.full(n_words + 2 * PAD, DC.STALE if dtype == np.uint64 else DC.STALE32, dtype=dtype))


def _inner(buf, n_words, dtype, what):
    """the n_words words between the pads of a synchronised buffer; the pads must still be stale"""
    raw = buf.cpu().numpy().view(dtype)
    stale = DC.STALE if dtype == np.uint64 else DC.STALE32
    assert np.all(raw[:PAD] == stale) and np.all(raw[PAD + n_words:] == stale), (what, "words around the output")
    return raw[PAD:PAD + n_words]


def _dev(store, queries, k, labels, mode=0, k_first=0, with_labels=True, with_counts=True, with_stats=True, stream=None, d_labels=None):
    """the device form on stale-filled outputs: (rows, row_labels | None, counts | None, stats | None)"""
    import torch
    nq = len(queries)
    d_q = _to_dev(queries)
    d_l = _to_dev(np.asarray(labels, dtype=np.uint32)) if d_labels is None else d_labels
    d_o, d_r, d_c = _stale(nq * k, np.uint64), _stale(nq * k, np.uint32) if with_labels else None, _stale(nq, np.uint32) if with_counts else None
    torch.cuda.synchronize()
    ptr = lambda b, size: b.data_ptr() + size * PAD if b is not None else None
    st = store.search_knn_distinct_dev(d_q.data_ptr(), nq, k, d_l.data_ptr(), ptr(d_o, 8), ptr(d_r, 4), ptr(d_c, 4), mode=mode, k_first=k_first,
                                       with_stats=with_stats, stream=stream)
    assert (st is None) == (not with_stats)
    torch.cuda.synchronize()
    return (_inner(d_o, nq * k, np.uint64, "rows").reshape(nq, k), _inner(d_r, nq * k, np.uint32, "row labels").reshape(nq, k) if with_labels else None,
            _inner(d_c, nq, np.uint32, "counts") if with_counts else None, st)


def _same(got, want, what):
    """a device result with some outputs left out against the model's"""
    rows, rls, counts, st = got
    DC.same_run((rows, rls if rls is not None else want[1], counts if counts is not None else want[2], st), want, what)


def _plain_knn(store, queries, k, mode=0):
    import torch
    nq = len(queries)
    d_q, d_o, d_c = _to_dev(queries), _stale(nq * k, np.uint64), _stale(nq, np.uint32)
    torch.cuda.synchronize()
    store.search_knn_dev(d_q.data_ptr(), nq, k, d_o.data_ptr() + 8 * PAD, d_c.data_ptr() + 4 * PAD, mode=mode)
    torch.cuda.synchronize()
    return _inner(d_o, nq * k, np.uint64, "plain rows").reshape(nq, k), _inner(d_c, nq, np.uint32, "plain counts")


# ---- 1. singletons ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [64, 128])
def test_singletons_are_the_plain_search(vc, bits):
    """labels equal the id: the row is bit for bit vc_search_knn_dev at k, in one round"""
    n, id_base = 2048, 1000
    codes = GC.uniform_codes(n, bits, 3 + bits)
    queries = GC.uniform_codes(70, bits, 4 + bits)
    labels = np.arange(n, dtype=np.uint32) + id_base
    lists = DC.sorted_lists(codes, queries, id_base)
    with _make(vc, codes, id_base=id_base) as store:
        for k in (1, 10, 64):
            want = DC.protocol_model(lists, labels, k, k, id_base)
            got = _dev(store, queries, k, labels, k_first=k)
            DC.same_run(got, want, (bits, k))
            rows, counts = _plain_knn(store, queries, k)
            assert np.array_equal(got[0], rows) and np.array_equal(got[2], counts) and np.array_equal(got[1], (rows & np.uint64(0xFFFFFFFF)).astype(np.uint32))
            assert got[3] == {"n_rounds": 1, "k_last": k, "n_searched": 70, "n_truncated": 0, "n_short": 0}


# ---- 2. one group -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [0, 3])
def test_one_group(vc, shards):
    """every record has label 7: one entry per row; k' doubles until it exceeds N = 300, then every query is short"""
    bits, n, k = 64, 300, 4
    codes = GC.uniform_codes(n, bits, 21)
    queries = codes[:5] ^ np.uint8(1)
    labels = np.full(n, 7, dtype=np.uint32)
    want = DC.protocol_model(DC.sorted_lists(codes, queries), labels, k)
    assert want[3] == {"n_rounds": 7, "k_last": 512, "n_searched": 35, "n_truncated": 0, "n_short": 5} and np.all(want[2] == 1)
    with _make(vc, codes, shards=shards) as store:
        DC.same_run(_dev(store, queries, k, labels), want, shards)
        DC.same_run(store.search_knn_distinct(queries, k, labels, with_stats=True), want, (shards, "host form"))


# ---- 3. duplicate-heavy data: the retry compaction and the index map ---------------------------------------------------------------------
@pytest.mark.parametrize("bits", [64, 128, 256, 512])
def test_duplicate_heavy(vc, bits):
    """257 queries, of which some finish in round 0 and the others need 1 .. 4 more (pinned on the model by test_distinct_cpu.py)"""
    codes, labels, queries = DC.dup_case(bits)
    want = DC.dup_expect(bits)
    with _make(vc, codes) as store:
        DC.same_run(_dev(store, queries, DC.DUP_K, labels), want, bits)
        if bits == 64:
            _same(_dev(store, queries, DC.DUP_K, labels, with_labels=False, with_counts=False, with_stats=False), want, "rows only")
            sub = slice(3, 200, 7)                                          # another batch on the same handle
            DC.same_run(_dev(store, queries[sub], DC.DUP_K, labels), DC.protocol_model(DC.dup_lists(bits)[sub], labels, DC.DUP_K), "a sub-batch")


# ---- 4. the size classes of the collapse kernel, both sides of their edges ----------------------------------------------------------------
@pytest.mark.parametrize("k_first", [64, 65, 1024, 1025, 8192])
def test_size_class_edges(vc, k_first):
    bits, k = 64, 32
    codes, labels, queries = DC.dup_case(bits)
    with _make(vc, codes) as store:
        DC.same_run(_dev(store, queries, k, labels, k_first=k_first), DC.dup_expect(bits, k, k_first), k_first)


# ---- 5. truncation ------------------------------------------------------------------------------------------------------------------------
def test_truncation(vc):
    """8600 records of one label lie nearest: at k = 2 the widest row still holds one group; at k = 1 the first round ends it"""
    codes, labels, queries = DC.truncation_case()
    lists = DC.truncation_lists()
    with _make(vc, codes) as store:
        want = DC.protocol_model(lists, labels, 2)
        assert np.all(want[2] == (1 | DC.TRUNCATED)) and want[3]["n_truncated"] == 3 and want[3]["k_last"] == 8192
        got = _dev(store, queries, 2, labels)
        DC.same_run(got, want, "k = 2")
        assert np.all(got[2] == (1 | vc.DISTINCT_TRUNCATED)) and np.all(got[0][:, 1] == DC.INF) and np.all(got[1][:, 0] == 5)
        DC.same_run(_dev(store, queries, 2, labels, k_first=8192), DC.protocol_model(lists, labels, 2, 8192), "k = 2 at once")
        want = DC.protocol_model(lists, labels, 1)
        assert want[3] == {"n_rounds": 1, "k_last": 2, "n_searched": 3, "n_truncated": 0, "n_short": 0}
        DC.same_run(_dev(store, queries, 1, labels), want, "k = 1")


# ---- 6. hostile label values --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,k_first", [(10, 0), (32, 1025), (32, 8192), (64, 64)])
def test_hostile_label_values(vc, k, k_first):
    """0, 0xFFFFFFFF, 0xFFFFFFFE, values that differ only above bit 16 or only in the low 4 bits: only equality matters"""
    bits = 64
    codes, labels, queries = DC.dup_case(bits)
    hostile = DC.hostile_labels(labels)
    assert {0, 0xFFFFFFFF, 0xFFFFFFFE} <= set(hostile.tolist())
    with _make(vc, codes) as store:
        DC.same_run(_dev(store, queries, k, hostile, k_first=k_first), DC.dup_expect(bits, k, k_first, 0, True), (k, k_first))


# ---- 7. ties ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [64, 128])
def test_ties(vc, bits):
    """records of different labels at equal distance: heads in id order, a group's head its smallest (dist, id)"""
    codes, labels, queries = DC.ties_case(bits)
    lists = DC.sorted_lists(codes, queries, 50)
    with _make(vc, codes, id_base=50) as store:
        for k, k_first in ((8, 0), (14, 14), (14, 100), (3, 3)):
            DC.same_run(_dev(store, queries, k, labels, k_first=k_first), DC.protocol_model(lists, labels, k, k_first, 50), (bits, k, k_first))


# ---- 8. k_first is a tuning knob ----------------------------------------------------------------------------------------------------------
def test_k_first_independence(vc):
    bits, k = 128, DC.DUP_K
    codes, labels, queries = DC.dup_case(bits)
    with _make(vc, codes) as store:
        runs = {}
        for k_first in (k, 0, 8 * k, 8192):
            runs[k_first] = _dev(store, queries, k, labels, k_first=k_first)
            DC.same_run(runs[k_first], DC.dup_expect(bits, k, k_first), k_first)
        for k_first, got in runs.items():
            for a, b in zip(got[:3], runs[0][:3]):
                assert np.array_equal(a, b), k_first
        assert len({tuple(sorted(r[3].items())) for r in runs.values()}) == 4        # the statistics differ


# ---- 9. exact MIH equals the linear scan ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,n_tables,shards", [(64, 2, 0), (128, 4, 0), (64, 4, 3)])
def test_mode_agreement(vc, bits, n_tables, shards):
    """rows, row labels and counts are the same words in both modes, for every k_first.  The statistics are each mode's own: a row of
    exact MIH is sure only below its last distance (the ties there are genuine, not the smallest ids), so a full row counts up to
    that distance only and a query may take a round more than over the linear scan -- the model's tie_cut"""
    codes, labels, queries = DC.dup_case(bits)
    with _make(vc, codes, n_tables=n_tables, shards=shards) as store:
        for k_first in (0, DC.DUP_K, 33):
            want, want_mih = DC.dup_expect(bits, DC.DUP_K, k_first), DC.dup_expect(bits, DC.DUP_K, k_first, 0, False, True)
            assert all(np.array_equal(a, b) for a, b in zip(want[:3], want_mih[:3])) and want_mih[3]["n_searched"] > want[3]["n_searched"]
            mih = _dev(store, queries, DC.DUP_K, labels, mode=vc.MODE_MIH_EXACT, k_first=k_first)
            lin = _dev(store, queries, DC.DUP_K, labels, mode=vc.MODE_LINEAR, k_first=k_first)
            DC.same_run(mih, want_mih, (bits, k_first, "exact MIH"))
            DC.same_run(lin, want, (bits, k_first, "linear"))
            assert all(np.array_equal(a, b) for a, b in zip(mih[:3], lin[:3]))
        DC.same_run(store.search_knn_distinct(queries[:40], DC.DUP_K, labels, mode=vc.MODE_MIH_EXACT, with_stats=True),
                    DC.protocol_model(DC.dup_lists(bits)[:40], labels, DC.DUP_K, tie_cut=True), (bits, "exact MIH, host form"))


# ---- 10. the pipeline: labels from the groupers --------------------------------------------------------------------------------------------
def test_labels_from_cluster_radius_and_group_index(vc):
    import torch
    bits = 64
    codes, _, queries = DC.dup_case(bits)
    lists = DC.dup_lists(bits)
    with _make(vc, codes, n_tables=2) as store:
        d_labels = _to_dev(np.zeros(len(codes), dtype=np.uint32))
        store.cluster_radius_dev(2, d_labels.data_ptr(), mode=vc.MODE_MIH_EXACT)       # the labels never leave the device
        torch.cuda.synchronize()
        labels = d_labels.cpu().numpy().view(np.uint32)
        assert 1 < len(np.unique(labels)) < len(codes)
        DC.same_run(_dev(store, queries, DC.DUP_K, labels, mode=vc.MODE_MIH_EXACT, d_labels=d_labels), DC.protocol_model(lists, labels, DC.DUP_K, tie_cut=True),
                    "cluster_radius")
        group_index = store.group_summary(labels)[3]
        want = DC.protocol_model(lists, group_index, DC.DUP_K)
        got = _dev(store, queries, DC.DUP_K, group_index)
        DC.same_run(got, want, "group_index")
        assert np.array_equal(got[0], _dev(store, queries, DC.DUP_K, labels)[0])       # the same partition under other names: the same rows


# ---- 11. sub-batches -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [0, 3])
def test_sub_batches(vc, monkeypatch, shards):
    """VC_DISTINCT_SCRATCH = 20 480 bytes: 128 queries per sub-batch at k' = 20, 8 at k' = 320 -- the rows are unchanged"""
    bits = 64
    codes, labels, queries = DC.dup_case(bits)
    monkeypatch.setenv("VC_DISTINCT_SCRATCH", "20480")
    with _make(vc, codes, shards=shards) as store:                          # (the knob is read when the handle is made)
        monkeypatch.delenv("VC_DISTINCT_SCRATCH")
        DC.same_run(_dev(store, queries, DC.DUP_K, labels), DC.dup_expect(bits), shards)
        DC.same_run(_dev(store, queries, 32, labels, k_first=8192), DC.dup_expect(bits, 32, 8192), (shards, "one row per sub-batch"))


# ---- 12. the host form, the caller's streams -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [0, 3])
def test_host_form_and_streams(vc, shards):
    import torch
    bits = 128
    codes, labels, queries = DC.dup_case(bits)
    want = DC.dup_expect(bits)
    with _make(vc, codes, shards=shards) as store:
        DC.same_run(store.search_knn_distinct(queries, DC.DUP_K, labels, with_stats=True), want, "ascending")
        got = store.search_knn_distinct(queries, DC.DUP_K, labels, order=vc.ORDER_FARTHEST_FIRST)
        rows, rls = DC.reverse_valid(*want[:3])
        DC.same_run(got, (rows, rls, want[2]), "farthest first")
        side = torch.cuda.Stream()
        DC.same_run(_dev(store, queries, DC.DUP_K, labels, stream=side.cuda_stream), want, "a caller's stream")
        DC.same_run(_dev(store, queries, DC.DUP_K, labels, stream=vc.STREAM_OWN), want, "VC_STREAM_OWN")
    codes, labels, queries = DC.truncation_case()
    if not shards:
        with _make(vc, codes) as store:                                     # a flagged count: the valid part is the count without its flag
            want = DC.protocol_model(DC.truncation_lists(), labels, 2, 4096)
            got = store.search_knn_distinct(queries, 2, labels, order=vc.ORDER_FARTHEST_FIRST, k_first=4096, with_stats=True)
            DC.same_run(got, want, "one entry turned round")


# ---- 13. the sharded store -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [64, 128])
def test_three_shards_equal_the_single_engine(vc, bits):
    codes, labels, queries = DC.dup_case(bits)
    with _make(vc, codes, id_base=7) as one, _make(vc, codes, id_base=7, shards=3, capacity=len(codes) + 5) as store:
        for k, k_first in ((DC.DUP_K, 0), (32, 65)):
            a, b = _dev(one, queries, k, labels, k_first=k_first), _dev(store, queries, k, labels, k_first=k_first)
            DC.same_run(b, a, (bits, k, "sharded == single"))
            DC.same_run(b, DC.dup_expect(bits, k, k_first, 7), (bits, k, "sharded == model"))


# ---- 14. a warm handle -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [0, 3])
def test_warm_handle(vc, shards):
    """the same call twice, a larger one that grows the buffers, the first again: the same bits"""
    bits = 64
    codes, labels, queries = DC.dup_case(bits)
    small = DC.protocol_model(DC.dup_lists(bits)[:33], labels, 5)
    with _make(vc, codes, shards=shards) as store:
        first = _dev(store, queries[:33], 5, labels)
        DC.same_run(first, small, "cold")
        DC.same_run(_dev(store, queries[:33], 5, labels), small, "again")
        DC.same_run(_dev(store, queries, 32, labels, k_first=8192), DC.dup_expect(bits, 32, 8192), "a larger call")
        DC.same_run(store.search_knn_distinct(queries, DC.DUP_K, labels, with_stats=True), DC.dup_expect(bits), "host form")
        again = _dev(store, queries[:33], 5, labels)
        for a, b in zip(first[:3], again[:3]):
            assert np.array_equal(a, b)
        assert first[3] == again[3]


# ---- 15. errors and the empty store ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [0, 2])
def test_errors_leave_the_outputs_untouched(vc, shards):
    import torch
    bits, n, nq, k = 64, 500, 4, 5
    codes = GC.uniform_codes(n, bits, 11)
    queries = np.ascontiguousarray(codes[:nq])
    labels = (np.arange(n, dtype=np.uint32) // 3).astype(np.uint32)
    L = vc.load_library()
    fn, fn_dev = (L.vc_sharded_search_knn_distinct, L.vc_sharded_search_knn_distinct_dev) if shards else (L.vc_search_knn_distinct, L.vc_search_knn_distinct_dev)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    with _make(vc, codes[:400], shards=shards, capacity=n, n_tables=4) as store:
        out, rl, cnt = np.full(nq * k, DC.STALE, dtype=np.uint64), np.full(nq * k, DC.STALE32, dtype=np.uint32), np.full(nq, DC.STALE32, dtype=np.uint32)
        st = vc.VcDistinctStats(n_rounds=77, k_last=77, n_searched=77, n_truncated=77, n_short=77)
        h, q, lab, lin, mih = store._h, p(queries), p(labels), vc.MODE_LINEAR, vc.MODE_MIH_EXACT
        #      handle q  nq  k  mode order labels k_first out
        bad = [(None, q, nq, k, lin, 0, lab, 0, p(out)), (h, None, nq, k, lin, 0, lab, 0, p(out)), (h, q, nq, k, lin, 0, None, 0, p(out)),
               (h, q, nq, k, lin, 0, lab, 0, None), (h, q, 0, k, lin, 0, lab, 0, p(out)), (h, q, nq, 0, lin, 0, lab, 0, p(out)),
               (h, q, nq, 8193, lin, 0, lab, 0, p(out)), (h, q, nq, k, lin, 0, lab, k - 1, p(out)), (h, q, nq, k, lin, 0, lab, 8193, p(out)),
               (h, q, nq, k, vc.MODE_MIH_APPROX, 0, lab, 0, p(out)), (h, q, nq, k, 3, 0, lab, 0, p(out)), (h, q, nq, k, lin, 2, lab, 0, p(out))]
        for args in bad:
            assert fn(*args, p(rl), p(cnt), C.byref(st)) == vc.VC_ERR_INVALID, args
        d_q, d_l = _to_dev(queries), _to_dev(labels)
        d_o, d_r, d_c = _stale(nq * k, np.uint64), _stale(nq * k, np.uint32), _stale(nq, np.uint32)
        torch.cuda.synchronize()
        for args in bad[:-1]:                                               # (the device form has no order)
            hh, qq, n_q, kk, mode, _, ll, kf, oo = args
            dev_args = (hh, d_q.data_ptr() if qq is not None else None, n_q, kk, mode, d_l.data_ptr() if ll is not None else None, kf,
                        d_o.data_ptr() if oo is not None else None)
            assert fn_dev(*dev_args, d_r.data_ptr(), d_c.data_ptr(), C.byref(st), None) == vc.VC_ERR_INVALID, args

        def untouched():
            torch.cuda.synchronize()
            assert np.all(out == DC.STALE) and np.all(rl == DC.STALE32) and np.all(cnt == DC.STALE32)
            for buf, dt in ((d_o, np.uint64), (d_r, np.uint32), (d_c, np.uint32)):
                assert np.all(buf.cpu().numpy().view(dt) == (DC.STALE if dt == np.uint64 else DC.STALE32))
            assert (st.n_rounds, st.k_last, st.n_searched, st.n_truncated, st.n_short) == (77,) * 5

        untouched()
        want = DC.protocol_model(DC.sorted_lists(codes[:400], queries), labels[:400], k, tie_cut=True)
        DC.same_run(store.search_knn_distinct(queries, k, labels[:400], mode=mih, with_stats=True), want, "a current index")
        store.add_codes(codes[400:])                                        # the index is stale now: it counts as none
        assert fn(h, q, nq, k, mih, 0, lab, 0, p(out), p(rl), p(cnt), C.byref(st)) == vc.VC_ERR_STATE
        assert fn_dev(h, d_q.data_ptr(), nq, k, mih, d_l.data_ptr(), 0, d_o.data_ptr(), d_r.data_ptr(), d_c.data_ptr(), C.byref(st), None) == vc.VC_ERR_STATE
        untouched()
        with pytest.raises(vc.VcError):
            store.search_knn_distinct(queries, k, labels, mode=vc.MODE_MIH_APPROX)
        want = DC.protocol_model(DC.sorted_lists(codes, queries), labels, k)
        DC.same_run(store.search_knn_distinct(queries, k, labels, with_stats=True), want, "the handle still works")
        DC.same_run(store.search_knn_distinct(queries, k, labels, k_first=8192, with_stats=True), DC.protocol_model(DC.sorted_lists(codes, queries), labels, k, 8192),
                    "k_first = VC_MAX_K is legal")


@pytest.mark.parametrize("shards", [0, 2])
def test_the_empty_store(vc, shards):
    """N == 0: VC_OK, counts 0, padded rows, zero labels and zero stats"""
    bits, nq, k = 64, 3, 4
    queries = GC.uniform_codes(nq, bits, 2)
    with _make(vc, np.zeros((0, bits // 8), np.uint8), shards=shards, capacity=16) as store:
        want = (np.full((nq, k), DC.INF, dtype=np.uint64), np.zeros((nq, k), dtype=np.uint32), np.zeros(nq, dtype=np.uint32), DC.zero_stats())
        DC.same_run(_dev(store, queries, k, np.zeros(1, dtype=np.uint32)), want, "device form")
        DC.same_run(store.search_knn_distinct(queries, k, np.zeros(0, dtype=np.uint32), with_stats=True), want, "host form")
