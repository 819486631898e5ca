"""Scoped k-NN: vc_search_knn_scoped, vc_search_knn_scoped_dev and their vc_sharded_* forms.

The expectation is scope_common.py's numpy model -- per query the brute-force sorted list over the records of its own scope, and the
plan of vc_scope_plan.hpp for the statistics -- pinned against plain loops by test_scope_cpu.py, which also shows that the crafted
cases reach what they are there for.  Rows, counts and statistics are integer functions of the codes, the scopes and the call, so
every comparison is exact equality on every output word; device outputs are pre-filled with a stale pattern, so every word is proven
written and the words around an output proven untouched.  One device; N <= 9000 (the large scope has 8800 records, so that the
small scopes next to it fit under that bound).

Not tested: the sharded form across real devices, and anything at N above 9000 (tools/bench_scoped.py asserts equality there)."""
import ctypes as C

import numpy as np
import pytest

import distinct_common as DC
import filter_common as FC
import scope_common as SC

pytestmark = pytest.mark.gpu

PAD = 3          # stale words kept on both sides of every device output


def _make(vc, codes, id_base=0, shards=0, capacity=None):
    bits, capacity = codes.shape[1] * 8, capacity or max(len(codes), 1)
    if shards:
        e = vc.ShardedEngine(bits, capacity=capacity, n_shards=shards, devices=[0], id_base=id_base)
    else:
        e = vc.Engine(bits, capacity=capacity, id_base=id_base)
    if len(codes):
        e.add_codes(codes)
    return e


def _make_env(vc, monkeypatch, codes, env, **kw):
    """a handle made under environment knobs, which are read when the handle is made"""
    for name, val in env.items():
        monkeypatch.setenv(name, str(val))
    store = _make(vc, codes, **kw)
    for name in env:
        monkeypatch.delenv(name)
    return store


def _to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    signed = {1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(a.view(signed).copy()).cuda()


def _stale(n_words, dtype):
    return _to_dev(np.full(n_words + 2 * PAD, SC.STALE if dtype == np.uint64 else SC.STALE32, dtype=dtype))


def _inner(buf, n_words, dtype, what):
    """the n_words words between the pads of a synchronised buffer; the pads must still be stale"""
    raw = buf.cpu().numpy().view(dtype)
    stale = SC.STALE if dtype == np.uint64 else SC.STALE32
    assert np.all(raw[:PAD] == stale) and np.all(raw[PAD + n_words:] == stale), (what, "words around the output")
    return raw[PAD:PAD + n_words]


def _dev(store, queries, k, scope, qscope, with_counts=True, with_stats=True, stream=None):
    """the device form on stale-filled outputs: (rows, counts | None, stats | None)"""
    import torch
    nq = len(queries)
    d_q, d_s, d_qs = _to_dev(queries), _to_dev(np.asarray(scope, dtype=np.uint32)), _to_dev(np.asarray(qscope, dtype=np.uint32))
    d_o, d_c = _stale(nq * k, np.uint64), _stale(nq, np.uint32) if with_counts else None
    torch.cuda.synchronize()
    st = store.search_knn_scoped_dev(d_q.data_ptr(), nq, k, d_s.data_ptr(), d_qs.data_ptr(), d_o.data_ptr() + 8 * PAD,
                                     d_c.data_ptr() + 4 * PAD if with_counts else None, with_stats=with_stats, stream=stream)
    assert (st is None) == (not with_stats)
    torch.cuda.synchronize()
    return _inner(d_o, nq * k, np.uint64, "rows").reshape(nq, k), _inner(d_c, nq, np.uint32, "counts") if with_counts else None, st


def _plain_knn(store, queries, k):
    import torch
    nq = len(queries)
    d_q, d_o, d_c = _to_dev(queries), _stale(nq * k, np.uint64), _stale(nq, np.uint32)
    torch.cuda.synchronize()
    store.search_knn_dev(d_q.data_ptr(), nq, k, d_o.data_ptr() + 8 * PAD, d_c.data_ptr() + 4 * PAD, mode=0)
    torch.cuda.synchronize()
    return _inner(d_o, nq * k, np.uint64, "plain rows").reshape(nq, k), _inner(d_c, nq, np.uint32, "plain counts")


def _filtered_equal(store, query, k, scope, value):
    import torch
    d_q, d_s, d_o, d_c = _to_dev(query), _to_dev(np.asarray(scope, dtype=np.uint32)), _stale(k, np.uint64), _stale(1, np.uint32)
    torch.cuda.synchronize()
    store.search_knn_filtered_dev(d_q.data_ptr(), 1, k, d_s.data_ptr(), d_o.data_ptr() + 8 * PAD, d_c.data_ptr() + 4 * PAD, kind=FC.EQUAL, value=int(value), mode=0)
    torch.cuda.synchronize()
    return _inner(d_o, k, np.uint64, "filtered row"), _inner(d_c, 1, np.uint32, "filtered count")[0]


@pytest.fixture(scope="module")
def seven64():
    """the shared reference of the 64-bit seven-scope case at id_base 0"""
    codes, queries, scope, qscope = SC.seven_case(64)
    return codes, queries, scope, qscope, DC.sorted_lists(codes, queries)


# ---- 1. one scope ----------------------------------------------------------------------------------------------------------------------------
def test_one_scope_is_the_plain_linear_search(vc):
    codes, queries = FC.uniform_case(64)
    n, nq = len(codes), len(queries)
    lists = DC.sorted_lists(codes, queries)
    scope, qscope = np.full(n, 0xABCD0123, dtype=np.uint32), np.full(nq, 0xABCD0123, dtype=np.uint32)
    with _make(vc, codes) as store:
        for k in (1, 10, 64):
            got = _dev(store, queries, k, scope, qscope)
            SC.same_run(got, SC.model(lists, scope, qscope, k), k)
            rows, counts = _plain_knn(store, queries, k)                   # bit for bit the plain linear search
            assert np.array_equal(got[0], rows) and np.array_equal(got[1], counts)
            assert got[2]["n_scopes"] == 1 and got[2]["n_matched"] == n and got[2]["n_pairs"] == n * nq and got[2]["n_windows"] == 1


# ---- 2. against two references -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [64, 128, 256, 512])
def test_seven_scopes_against_the_model_and_the_filtered_call(vc, bits):
    codes, queries, scope, qscope = SC.seven_case(bits)
    id_base, k = 1000, 10
    lists = DC.sorted_lists(codes, queries, id_base)
    with _make(vc, codes, id_base=id_base) as store:
        got = _dev(store, queries, k, scope, qscope)
        SC.same_run(got, SC.model(lists, scope, qscope, k, id_base, W=bits // 64), bits)
        for value in np.unique(qscope):                                     # one filtered call per distinct value, on the same handle
            for q in np.nonzero(qscope == value)[0]:
                row, count = _filtered_equal(store, queries[q:q + 1], k, scope, value)
                assert np.array_equal(got[0][q], row) and got[1][q] == count, (bits, value, q)


# ---- 3. segment edges ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [64, 512])
def test_segment_edges(vc, bits):
    k = 10
    codes, queries, scope, qscope = SC.edge_case(bits, k)
    lists = DC.sorted_lists(codes, queries)
    with _make(vc, codes) as store:
        want = SC.model(lists, scope, qscope, k, W=bits // 64)
        got = _dev(store, queries, k, scope, qscope)
        SC.same_run(got, want, bits)
        assert got[2]["n_empty"] == 2
        twins = [i for i in range(len(queries)) if any(j != i and qscope[j] == qscope[i] and np.array_equal(queries[j], queries[i]) for j in range(len(queries)))]
        assert len(twins) == 2 and np.array_equal(got[0][twins[0]], got[0][twins[1]]) and got[1][twins[0]] == got[1][twins[1]]
        perm = np.random.default_rng(2).permutation(len(queries))          # a permuted call returns permuted rows
        again = _dev(store, np.ascontiguousarray(queries[perm]), k, scope, qscope[perm])
        assert np.array_equal(again[0], got[0][perm]) and np.array_equal(again[1], got[1][perm]) and again[2] == got[2]


# ---- 4. hostile values -----------------------------------------------------------------------------------------------------------------------------
def test_hostile_scope_values(vc):
    codes, queries, scope, qscope = SC.hostile_case()
    lists = DC.sorted_lists(codes, queries)
    with _make(vc, codes) as store:
        for k in (3, 100, 400):
            got = _dev(store, queries, k, scope, qscope)
            SC.same_run(got, SC.model(lists, scope, qscope, k), k)
        assert np.all(got[1][qscope == 0x7FFFFFFF] == 0) and got[2]["n_empty"] == 3 and got[2]["n_scopes"] == len(SC.HOSTILE) - 1
        assert got[2]["n_matched"] == np.count_nonzero(scope != 0xFFFFFFFE)


# ---- 5. ties -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,ties", [(64, 63), (64, 64), (64, 65), (64, 600), (512, 100)])
def test_ties_go_to_the_smaller_id_of_the_own_scope(vc, bits, ties):
    codes, queries, scope, qscope, k = SC.tie_case(bits, ties)
    lists = DC.sorted_lists(codes, queries)
    with _make(vc, codes) as store:
        for kk in (k, 1, ties, ties + 3):
            got = _dev(store, queries, kk, scope, qscope)
            SC.same_run(got, SC.model(lists, scope, qscope, kk, W=bits // 64), (bits, ties, kk))
        got = _dev(store, queries, k, scope, qscope)
        assert np.array_equal(got[0][0], np.arange(k, dtype=np.uint64) * np.uint64(2))          # distance 0, the k smallest even ids
        assert np.array_equal(got[0][1], np.arange(k, dtype=np.uint64) * np.uint64(2) + np.uint64(1))


# ---- 6. large k ----------------------------------------------------------------------------------------------------------------------------------------
def test_large_k(vc):
    codes, queries, scope, qscope = SC.large_case()
    lists = DC.sorted_lists(codes, queries)
    with _make(vc, codes) as store:
        got = _dev(store, queries, 8192, scope, qscope)
        SC.same_run(got, SC.model(lists, scope, qscope, 8192), "k = 8192")
        assert np.all(got[1][qscope == 77] == 8192) and np.all(got[1][qscope == 1] == 120)
        small = qscope != 77                                                  # k larger than every scope
        got = _dev(store, np.ascontiguousarray(queries[small]), 200, scope, qscope[small])
        SC.same_run(got, SC.model([L for L, s in zip(lists, small) if s], scope, qscope[small], 200), "k above every scope")
        assert got[2]["n_short"] == np.count_nonzero(small) and np.all(got[1] < 200)


# ---- 7. windows and sub-batches ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [64, 256])
def test_windows_and_sub_batches(vc, monkeypatch, bits):
    codes, queries, scope, qscope = SC.seven_case(bits, nq=300)
    lists = DC.sorted_lists(codes, queries)
    W = bits // 64
    with _make(vc, codes) as plain, _make_env(vc, monkeypatch, codes, {"VC_SCOPE_WINDOW": 256}) as windowed, \
            _make_env(vc, monkeypatch, codes, {"VC_SCOPE_WINDOW": 256, "VC_SCOPE_SCRATCH": 4096}) as both, \
            _make_env(vc, monkeypatch, codes, {"VC_SCOPE_WINDOW": 1 << 25, "VC_SCOPE_SCRATCH": 1}) as single:
        for k in (10, 300):                                                   # k above the window: windows shorter than the row
            base = _dev(plain, queries, k, scope, qscope)
            SC.same_run(base, SC.model(lists, scope, qscope, k, W=W), (bits, k))
            for store, kw in ((windowed, dict(window=256)), (both, dict(window=256, scratch=4096)), (single, dict(window=1 << 25, scratch=1))):
                got = _dev(store, queries, k, scope, qscope)
                want = SC.model(lists, scope, qscope, k, W=W, **kw)
                SC.same_run(got, want, (bits, k, kw))
                assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])
                assert got[2]["n_windows"] == want[2]["n_windows"] > 1
        assert base[2]["n_windows"] == 1


# ---- 8. three shards on one device ------------------------------------------------------------------------------------------------------------------------
def test_three_shards_equal_the_single_engine(vc):
    codes, queries, scope, qscope = SC.seven_case(128)
    k = 10
    for id_base in (0, 7):
        want = SC.model(DC.sorted_lists(codes, queries, id_base), scope, qscope, k, id_base, W=2)
        with _make(vc, codes, id_base=id_base) as one, _make(vc, codes, id_base=id_base, shards=3, capacity=len(codes) + 5) as store:
            a, b = _dev(one, queries, k, scope, qscope), _dev(store, queries, k, scope, qscope)
            SC.same_run(b, a, (id_base, "sharded == single"))
            SC.same_run(b, want, (id_base, "sharded == model"))
            SC.same_run(store.search_knn_scoped(queries, k, scope, qscope, with_stats=True), want, (id_base, "host form"))


# ---- 9. the host form and a warm handle --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [0, 3])
def test_host_form_streams_and_a_warm_handle(vc, seven64, shards):
    import torch
    codes, queries, scope, qscope, lists = seven64
    with _make(vc, codes, shards=shards) as store:
        for k in (10, 30):
            want = SC.model(lists, scope, qscope, k)
            SC.same_run(store.search_knn_scoped(queries, k, scope, qscope, with_stats=True), want, "ascending")
            rows, counts = store.search_knn_scoped(queries, k, scope, qscope, order=vc.ORDER_FARTHEST_FIRST)
            SC.same_run((rows, counts), (SC.reverse_valid(want[0], want[1]), want[1]), "farthest first")
            side = torch.cuda.Stream()
            SC.same_run(_dev(store, queries, k, scope, qscope, stream=side.cuda_stream), want, "a caller's stream")
            SC.same_run(_dev(store, queries, k, scope, qscope, stream=vc.STREAM_OWN), want, "VC_STREAM_OWN")
            got = _dev(store, queries, k, scope, qscope, with_counts=False, with_stats=False)
            assert got[1] is None and got[2] is None and np.array_equal(got[0], want[0])
        assert np.any(want[1] < 30)
        # a warm handle: small, a different and larger scoped call (the buffers grow), a filtered call, small again
        first = _dev(store, queries[:5], 3, scope, qscope[:5])
        SC.same_run(first, SC.model(lists[:5], scope, qscope[:5], 3), "cold")
        other = np.where(scope == 3, np.uint32(900), scope)
        SC.same_run(_dev(store, queries, 200, other, qscope), SC.model(lists, other, qscope, 200), "a larger call")
        store.search_knn_filtered(queries, 64, scope, kind=FC.EQUAL, value=3)
        again = _dev(store, queries[:5], 3, scope, qscope[:5])
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and first[2] == again[2]


# ---- 10. errors and the empty store --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [0, 2])
def test_errors_leave_the_outputs_untouched(vc, shards):
    import torch
    bits, n, nq, k = 64, 500, 4, 5
    codes = FC.uniform_case(bits)[0][:n]
    queries = np.ascontiguousarray(codes[:nq])
    scope, qscope = (np.arange(n, dtype=np.uint32) % 3).astype(np.uint32), np.array([0, 1, 2, 1], dtype=np.uint32)
    L = vc.load_library()
    fn, fn_dev = (L.vc_sharded_search_knn_scoped, L.vc_sharded_search_knn_scoped_dev) if shards else (L.vc_search_knn_scoped, L.vc_search_knn_scoped_dev)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    with _make(vc, codes, shards=shards) as store:
        out, cnt = np.full(nq * k, SC.STALE, dtype=np.uint64), np.full(nq, SC.STALE32, dtype=np.uint32)
        st = vc.VcScopeStats(n_matched=77, n_pairs=77, n_scopes=77, n_windows=77, n_short=77, n_empty=77)
        h, q, s, qs = store._h, p(queries), p(scope), p(qscope)
        #      handle q  nq  k  order scope qscope flags out
        bad = [(None, q, nq, k, 0, s, qs, 0, p(out)), (h, None, nq, k, 0, s, qs, 0, p(out)), (h, q, nq, k, 0, None, qs, 0, p(out)),
               (h, q, nq, k, 0, s, None, 0, p(out)), (h, q, nq, k, 0, s, qs, 0, None), (h, q, 0, k, 0, s, qs, 0, p(out)),
               (h, q, nq, 0, 0, s, qs, 0, p(out)), (h, q, nq, 8193, 0, s, qs, 0, p(out)), (h, q, nq, k, 0, s, qs, 1, p(out)),
               (h, q, nq, k, 0, s, qs, 0x80000000, p(out)), (h, q, nq, k, 2, s, qs, 0, p(out))]
        for args in bad:
            assert fn(*args, p(cnt), C.byref(st)) == vc.VC_ERR_INVALID, args
        d_q, d_s, d_qs = _to_dev(queries), _to_dev(scope), _to_dev(qscope)
        d_o, d_c = _stale(nq * k, np.uint64), _stale(nq, np.uint32)
        torch.cuda.synchronize()
        for args in bad[:-1]:                                               # (the device form has no order)
            hh, qq, n_q, kk, _, ss, qss, flags, oo = args
            dev_args = (hh, d_q.data_ptr() if qq is not None else None, n_q, kk, d_s.data_ptr() if ss is not None else None,
                        d_qs.data_ptr() if qss is not None else None, flags, d_o.data_ptr() if oo is not None else None)
            assert fn_dev(*dev_args, d_c.data_ptr(), C.byref(st), None) == vc.VC_ERR_INVALID, args
        torch.cuda.synchronize()
        assert np.all(out == SC.STALE) and np.all(cnt == SC.STALE32)
        for buf, dt in ((d_o, np.uint64), (d_c, np.uint32)):
            assert np.all(buf.cpu().numpy().view(dt) == (SC.STALE if dt == np.uint64 else SC.STALE32))
        assert all(getattr(st, name) == 77 for name in SC.STAT_NAMES)
        SC.same_run(store.search_knn_scoped(queries, k, scope, qscope, with_stats=True), SC.model(DC.sorted_lists(codes, queries), scope, qscope, k),
                    "the handle still works")


@pytest.mark.parametrize("shards", [0, 2])
def test_the_empty_store(vc, shards):
    """N == 0: VC_OK, counts 0, padded rows and zero stats"""
    bits, nq, k = 64, 3, 4
    queries = FC.uniform_case(bits)[1][:nq]
    qscope = np.array([0, 5, 0xFFFFFFFF], dtype=np.uint32)
    with _make(vc, np.zeros((0, bits // 8), np.uint8), shards=shards, capacity=16) as store:
        want = (np.full((nq, k), SC.INF, dtype=np.uint64), np.zeros(nq, dtype=np.uint32), SC.zero_stats())
        SC.same_run(_dev(store, queries, k, np.zeros(1, dtype=np.uint32), qscope), want, "device form")
        SC.same_run(store.search_knn_scoped(queries, k, np.zeros(0, dtype=np.uint32), qscope, with_stats=True), want, "host form")
