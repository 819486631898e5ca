"""Filtered k-NN: vc_search_knn_filtered, vc_search_knn_filtered_dev and their vc_sharded_* forms.

The expectation is filter_common.py's numpy model -- the brute-force sorted list over the allowed records, and the round protocol for
the statistics -- pinned against plain loops by test_filter_cpu.py, which also shows that the crafted cases reach what they are there
for.  Rows, counts and statistics are integer functions of the codes, the filter and the call, so every comparison is exact equality
on every output word; device outputs are pre-filled with a stale pattern, so every word is proven written and the words around an
output proven untouched.  One device; N <= 9000.

Not tested: a count of UINT32_MAX passed on from the search underneath (nothing provokes a give-up on purpose), and the sharded form
across real devices."""
import ctypes as C

import numpy as np
import pytest

import distinct_common as DC
import filter_common as FC

pytestmark = pytest.mark.gpu

PAD = 3          # stale words kept on both sides of every device output
ROUTES = (0, 1, 2)


def _make(vc, codes, id_base=0, shards=0, capacity=None, n_tables=0, flags=0):
    bits, capacity = codes.shape[1] * 8, capacity or max(len(codes), 1)
    if shards:
        e = vc.ShardedEngine(bits, capacity=capacity, n_shards=shards, devices=[0], id_base=id_base, n_tables=n_tables, flags=flags)
    else:
        e = vc.Engine(bits, capacity=capacity, id_base=id_base, n_tables=n_tables, flags=flags)
    if len(codes):
        e.add_codes(codes)
    if n_tables:
        e.build_index()
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
    return _to_dev(np.full(n_words + 2 * PAD, FC.STALE if dtype == np.uint64 else FC.STALE32, dtype=dtype))


def _inner(buf, n_words, dtype, what):
    """the n_words words between the pads of a synchronised buffer; the pads must still be stale"""
    raw = buf.cpu().numpy().view(dtype)
    stale = FC.STALE if dtype == np.uint64 else FC.STALE32
    assert np.all(raw[:PAD] == stale) and np.all(raw[PAD + n_words:] == stale), (what, "words around the output")
    return raw[PAD:PAD + n_words]


def _dev(store, queries, k, sel, kind=FC.MASK, value=0, mode=0, k_first=0, with_counts=True, with_stats=True, stream=None, d_sel=None):
    """the device form on stale-filled outputs: (rows, counts | None, stats | None)"""
    import torch
    nq = len(queries)
    d_q = _to_dev(queries)
    d_s = _to_dev(np.asarray(sel, dtype=np.uint32)) if d_sel is None else d_sel
    d_o, d_c = _stale(nq * k, np.uint64), _stale(nq, np.uint32) if with_counts else None
    torch.cuda.synchronize()
    st = store.search_knn_filtered_dev(d_q.data_ptr(), nq, k, d_s.data_ptr(), d_o.data_ptr() + 8 * PAD, d_c.data_ptr() + 4 * PAD if with_counts else None,
                                       kind=kind, value=value, mode=mode, k_first=k_first, with_stats=with_stats, stream=stream)
    assert (st is None) == (not with_stats)
    torch.cuda.synchronize()
    return _inner(d_o, nq * k, np.uint64, "rows").reshape(nq, k), _inner(d_c, nq, np.uint32, "counts") if with_counts else None, st


def _plain_knn(store, queries, k, mode=0):
    import torch
    nq = len(queries)
    d_q, d_o, d_c = _to_dev(queries), _stale(nq * k, np.uint64), _stale(nq, np.uint32)
    torch.cuda.synchronize()
    store.search_knn_dev(d_q.data_ptr(), nq, k, d_o.data_ptr() + 8 * PAD, d_c.data_ptr() + 4 * PAD, mode=mode)
    torch.cuda.synchronize()
    return _inner(d_o, nq * k, np.uint64, "plain rows").reshape(nq, k), _inner(d_c, nq, np.uint32, "plain counts")


@pytest.fixture(scope="module")
def uniform64():
    """the shared reference of the 64-bit cases: codes, queries and the sorted lists at id_base 0"""
    codes, queries = FC.uniform_case(64)
    return codes, queries, DC.sorted_lists(codes, queries)


# ---- 1. all allowed, none allowed, fewer than k allowed ------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_all_none_and_few_allowed(vc, monkeypatch, uniform64, route):
    codes, queries, lists = uniform64
    n, nq = len(codes), len(queries)
    with _make_env(vc, monkeypatch, codes, {"VC_FILTER_ROUTE": route}) as store:
        everyone = np.ones(n, dtype=bool)
        for k in (1, 10, 64):
            got = _dev(store, queries, k, FC.sel_for(everyone, FC.MASK))
            FC.same_run(got, FC.model(lists, everyone, k, route=route), (route, k))
            rows, counts = _plain_knn(store, queries, k)                   # bit for bit the plain linear search
            assert np.array_equal(got[0], rows) and np.array_equal(got[1], counts)
        nobody = np.zeros(n, dtype=bool)
        got = _dev(store, queries, 7, FC.sel_for(nobody, FC.MASK))
        assert np.all(got[0] == FC.INF) and np.all(got[1] == 0)
        FC.same_run(got, FC.model(lists, nobody, 7, route=route), (route, "none"))
        assert got[2]["routes"] == 0 and got[2]["n_allowed"] == 0
        few = np.zeros(n, dtype=bool)
        few[[5, 77, n - 1]] = True
        got = _dev(store, queries, 7, FC.sel_for(few, FC.MASK))
        FC.same_run(got, FC.model(lists, few, 7, route=route), (route, "A < k"))
        assert np.all(got[1] == 3) and got[2]["n_short"] == nq and np.all(got[0][:, 3:] == FC.INF)


# ---- 2. selectivities, at every code width, under every route -------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [64, 128, 256, 512])
def test_selectivities(vc, monkeypatch, bits):
    codes, queries = FC.uniform_case(bits)
    id_base, k, n = 1000, 10, len(codes)
    lists = DC.sorted_lists(codes, queries, id_base)
    masks = {one_in: FC.random_mask(n, one_in, 40 + one_in) for one_in in (2, 16, 256)}
    runs = {}
    for route in ROUTES:
        with _make_env(vc, monkeypatch, codes, {"VC_FILTER_ROUTE": route}, id_base=id_base) as store:
            for one_in, allowed in masks.items():
                got = _dev(store, queries, k, FC.sel_for(allowed, FC.MASK))
                FC.same_run(got, FC.model(lists, allowed, k, id_base=id_base, route=route, W=bits // 64), (bits, route, one_in))
                runs[route, one_in] = got
                if route == 2:
                    assert got[2]["routes"] == FC.RAN_PRE and got[2]["n_rounds"] == 0
                if route == 1:
                    assert got[2]["routes"] & FC.RAN_POST and got[2]["n_rounds"] >= 1
    for one_in in masks:                                                     # the same words on every route
        for route in (1, 2):
            assert np.array_equal(runs[route, one_in][0], runs[0, one_in][0]) and np.array_equal(runs[route, one_in][1], runs[0, one_in][1])
    assert runs[0, 2][2]["routes"] == FC.RAN_POST and runs[0, 256][2]["routes"] == FC.RAN_PRE      # the plan's own choice at both ends


# ---- 3. every kind on the same allowed set ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [1, 2])
def test_every_kind_means_the_same_set(vc, monkeypatch, route):
    codes, queries = FC.uniform_case(64, n=4001)                           # N is no multiple of 32
    id_base, k, n = 0xFFFFF000 - 4001, 12, 4001                            # ids run up to just below 2^32 - 4096
    lists = DC.sorted_lists(codes, queries, id_base)
    allowed = FC.random_mask(n, 5, 9)
    want = FC.model(lists, allowed, k, id_base=id_base, route=route)
    rng = np.random.default_rng(4)
    high = (rng.integers(1, 1 << 16, size=n).astype(np.uint32) << np.uint32(16)) | np.uint32(0xBEEF)     # values that differ only in high bits
    with _make_env(vc, monkeypatch, codes, {"VC_FILTER_ROUTE": route}, id_base=id_base) as store:
        cases = [("mask", FC.MASK, 0, FC.sel_for(allowed, FC.MASK, other=high)),
                 ("mask of all ones", FC.MASK, 0, FC.sel_for(allowed, FC.MASK, other=np.full(n, 0xFFFFFFFF, dtype=np.uint32))),
                 ("bits, junk in the tail", FC.BITS, 0, FC.sel_for(allowed, FC.BITS, junk=0xFFFFFFFF)),
                 ("bits", FC.BITS, 0, FC.sel_for(allowed, FC.BITS)),
                 ("roots", FC.ROOTS, 0, FC.sel_for(allowed, FC.ROOTS, id_base)),
                 ("roots among zeros", FC.ROOTS, 0, FC.sel_for(allowed, FC.ROOTS, id_base, other=np.zeros(n, dtype=np.uint32)))]
        for value in (0, 0xFFFFFFFF, 0x0001BEEF):
            far = np.where(high == np.uint32(value), np.uint32(0x0002BEEF), high)
            cases.append(("equal %#x" % value, FC.EQUAL, value, FC.sel_for(allowed, FC.EQUAL, value=value, other=far)))
            cases.append(("not equal %#x" % value, FC.NOT_EQUAL, value, FC.sel_for(allowed, FC.NOT_EQUAL, value=value, other=far)))
        for what, kind, value, sel in cases:
            assert np.array_equal(FC.allowed_of(sel, kind, value, n, id_base), allowed), what
            FC.same_run(_dev(store, queries, k, sel, kind=kind, value=value, k_first=40), FC.model(lists, allowed, k, id_base=id_base, route=route, k_first=40), what)
        assert want[2]["n_allowed"] == np.count_nonzero(allowed)


# ---- 4. ties ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,A", [(64, 63), (64, 64), (64, 65), (64, 1300), (512, 200), (128, 700)])
def test_ties_go_to_the_smaller_id(vc, monkeypatch, bits, A):
    """duplicate-heavy codes, the k-th distance holds more allowed records than the row takes, every allowed record has a disallowed
    copy one id below; windows of 63, 64 and 65 ids, and tie groups that span several wave-slices"""
    codes, allowed, queries, k = FC.tie_case(bits, A)
    lists = DC.sorted_lists(codes, queries)
    sel = FC.sel_for(allowed, FC.BITS, junk=0xFFFFFFFF)
    for route in (1, 2):
        with _make_env(vc, monkeypatch, codes, {"VC_FILTER_ROUTE": route}) as store:
            for kk in (k, 1, A, A + 3):
                if kk > FC.MAX_K:
                    continue
                FC.same_run(_dev(store, queries, kk, sel, kind=FC.BITS), FC.model(lists, allowed, kk, route=route, W=bits // 64), (bits, A, route, kk))


# ---- 5. the fallback -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tables", [0, 2])
def test_fallback_after_the_widest_row(vc, monkeypatch, n_tables):
    """the 8600 nearest records are disallowed: the rounds (VC_FILTER_ROUTE = 1) reach k' = 8192, every query goes to the pre-filter
    route, rows exact and full"""
    codes, sel, queries, allowed = FC.fallback_case()
    lists, k = DC.truncation_lists(), 5
    with _make_env(vc, monkeypatch, codes, {"VC_FILTER_ROUTE": 1}, n_tables=n_tables) as store:
        mode = vc.MODE_MIH_EXACT if n_tables else vc.MODE_LINEAR
        want = FC.model(lists, allowed, k, tie_cut=bool(n_tables), route=1)
        got = _dev(store, queries, k, sel, kind=FC.NOT_EQUAL, value=5, mode=mode)
        FC.same_run(got, want, n_tables)
        assert got[2]["k_last"] == 8192 and got[2]["n_rounds"] > 1 and got[2]["n_fallback"] == len(queries) and got[2]["routes"] == FC.RAN_POST | FC.RAN_PRE
        assert np.all(got[1] == k) and np.all(got[0] != FC.INF)
        FC.same_run(_dev(store, queries, k, sel, kind=FC.NOT_EQUAL, value=5, mode=mode, k_first=8192),
                    FC.model(lists, allowed, k, tie_cut=bool(n_tables), k_first=8192, route=1), "at once")


# ---- 6. windows --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [64, 256])
def test_windows_are_merged(vc, monkeypatch, bits):
    codes, queries = FC.uniform_case(bits)
    lists = DC.sorted_lists(codes, queries)
    allowed = FC.random_mask(len(codes), 2, 12)
    A = int(np.count_nonzero(allowed))
    assert 1800 < A < 2200
    with _make_env(vc, monkeypatch, codes, {"VC_FILTER_ROUTE": 2, "VC_FILTER_WINDOW": 256}) as store:
        for k in (10, 300):                                                  # k above the window: windows shorter than the row
            got = _dev(store, queries, k, FC.sel_for(allowed, FC.MASK))
            FC.same_run(got, FC.model(lists, allowed, k, route=2, window=256, W=bits // 64), (bits, k))
            assert got[2]["n_windows"] == (A + 255) // 256 > 6


# ---- 7. sub-batches ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [1, 2])
def test_sub_batches(vc, monkeypatch, uniform64, route):
    """VC_FILTER_SCRATCH = 256 bytes: one query per sub-batch of the rounds (a k' row is larger), and at 4 slices per window 8 queries
    per sub-batch of the subset scan"""
    codes, queries, lists = uniform64
    allowed = FC.random_mask(len(codes), 2, 12) if route == 1 else np.ones(len(codes), dtype=bool)
    with _make_env(vc, monkeypatch, codes, {"VC_FILTER_ROUTE": route, "VC_FILTER_SCRATCH": 256, "VC_FILTER_WINDOW": 2048}) as store:
        got = _dev(store, queries, 10, FC.sel_for(allowed, FC.MASK))
        FC.same_run(got, FC.model(lists, allowed, 10, route=route, scratch=256, window=2048), route)
        if route == 2:
            assert got[2]["n_windows"] == 2 * ((len(queries) + 7) // 8) == 10


# ---- 8. modes ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,n_tables", [(64, 2), (128, 4)])
def test_exact_mih_equals_linear(vc, bits, n_tables):
    codes, labels, queries = DC.dup_case(bits)
    lists = DC.dup_lists(bits)
    allowed = (labels % 3) != 0                                            # whole groups in and out
    k = 10
    with _make(vc, codes, n_tables=n_tables) as store:
        for k_first in (0, k, 33, 8192):
            want = FC.model(lists, allowed, k, k_first=k_first, W=bits // 64)
            lin = _dev(store, queries, k, labels % 3, kind=FC.NOT_EQUAL, value=0, k_first=k_first)
            mih = _dev(store, queries, k, labels % 3, kind=FC.NOT_EQUAL, value=0, k_first=k_first, mode=vc.MODE_MIH_EXACT)
            FC.same_run(lin, want, (bits, k_first, "linear"))
            FC.same_run(mih, FC.model(lists, allowed, k, k_first=k_first, tie_cut=True, W=bits // 64), (bits, k_first, "exact MIH"))
            assert np.array_equal(lin[0], mih[0]) and np.array_equal(lin[1], mih[1])


def test_refused_modes(vc):
    codes, queries = FC.uniform_case(64)
    sel = np.ones(len(codes), dtype=np.uint32)
    with _make(vc, codes, n_tables=4) as store:
        with pytest.raises(vc.VcError) as err:
            store.search_knn_filtered(queries, 5, sel, mode=vc.MODE_MIH_APPROX)
        assert err.value.code == vc.VC_ERR_INVALID
        store.search_knn_filtered(queries, 5, sel, mode=vc.MODE_MIH_EXACT)
    for n_tables, flags in ((4, vc.FLAG_REF_SIGNEXT_KEYS), (2, vc.FLAG_REF_STOP_LITERAL4)):
        for shards in (0, 2):
            with _make(vc, codes, n_tables=n_tables, flags=flags, shards=shards) as store:
                with pytest.raises(vc.VcError) as err:
                    store.search_knn_filtered(queries, 5, sel, mode=vc.MODE_MIH_EXACT)
                assert err.value.code == vc.VC_ERR_INVALID
                store.search_knn_filtered(queries, 5, sel, mode=vc.MODE_LINEAR)      # the linear scan is not affected
    with _make(vc, codes, n_tables=4, flags=vc.FLAG_REF_STOP_LITERAL4) as store:      # the literal 4 is exact from four tables on
        store.search_knn_filtered(queries, 5, sel, mode=vc.MODE_MIH_EXACT)


# ---- 9. three shards on one device ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [1, 2])
def test_three_shards_equal_the_single_engine(vc, monkeypatch, route):
    codes, queries = FC.uniform_case(128)
    id_base, k = 7, 10
    lists = DC.sorted_lists(codes, queries, id_base)
    allowed = FC.random_mask(len(codes), 4, 3)
    sel = FC.sel_for(allowed, FC.BITS)
    want = FC.model(lists, allowed, k, id_base=id_base, route=route, W=2)
    env = {"VC_FILTER_ROUTE": route}
    with _make_env(vc, monkeypatch, codes, env, id_base=id_base, n_tables=4) as one, \
            _make_env(vc, monkeypatch, codes, env, id_base=id_base, shards=3, capacity=len(codes) + 5, n_tables=4) as store:
        for mode in (vc.MODE_LINEAR, vc.MODE_MIH_EXACT):
            a, b = _dev(one, queries, k, sel, kind=FC.BITS, mode=mode), _dev(store, queries, k, sel, kind=FC.BITS, mode=mode)
            FC.same_run(b[:2], a[:2], (route, mode, "sharded == single"))
            FC.same_run(b[:2], want[:2], (route, mode, "sharded == model"))
            if mode == vc.MODE_LINEAR:
                assert a[2] == want[2] == b[2]
        for h in (one, store):
            FC.same_run(h.search_knn_filtered(queries, k, sel, kind=FC.BITS, with_stats=True), want, (route, "host form"))


# ---- 10. the pipeline: leaders' labels stay on the device ----------------------------------------------------------------------------------------
def test_roots_of_leaders_equal_a_retained_store(vc):
    import torch
    bits, k = 64, 10
    codes, _, queries = DC.dup_case(bits)
    with _make(vc, codes, n_tables=2) as store, _make(vc, codes, n_tables=2) as cut:
        d_labels = _to_dev(np.zeros(len(codes), dtype=np.uint32))
        store.leaders_radius_dev(2, d_labels.data_ptr(), mode=vc.MODE_MIH_EXACT)
        torch.cuda.synchronize()
        labels = d_labels.cpu().numpy().view(np.uint32)
        leaders = labels == np.arange(len(codes), dtype=np.uint32)
        assert 1 < np.count_nonzero(leaders) < len(codes)
        got = _dev(store, queries, k, None, kind=FC.ROOTS, mode=vc.MODE_MIH_EXACT, d_sel=d_labels)
        FC.same_run(got[:2], FC.model_rows(DC.dup_lists(bits), leaders, k), "the model")
        n_kept, new_ids = cut.retain(labels, vc.RETAIN_ROOTS, with_map=True)
        assert n_kept == np.count_nonzero(leaders)
        rows, counts = _plain_knn(cut, queries, k)
        old_of = np.nonzero(leaders)[0].astype(np.uint64)                   # new id j was old id old_of[j]
        assert np.array_equal(new_ids[leaders], np.arange(n_kept, dtype=np.uint32))
        mapped = np.where(rows == FC.INF, FC.INF, (rows & ~np.uint64(0xFFFFFFFF)) | old_of[np.minimum(rows & np.uint64(0xFFFFFFFF), np.uint64(n_kept - 1)).astype(np.int64)])
        assert np.array_equal(got[0], mapped) and np.array_equal(got[1], counts)


# ---- 11. handle behaviour ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [0, 3])
def test_host_form_streams_and_a_warm_handle(vc, uniform64, shards):
    import torch
    codes, queries, lists = uniform64
    dense, sparse = FC.random_mask(len(codes), 2, 5), FC.random_mask(len(codes), 256, 6)
    with _make(vc, codes, shards=shards) as store:
        for allowed, k in ((dense, 10), (sparse, 30)):                       # the plan's route at both ends; the sparse rows are short
            sel = FC.sel_for(allowed, FC.MASK)
            want = FC.model(lists, allowed, k)
            FC.same_run(store.search_knn_filtered(queries, k, sel, with_stats=True), want, "ascending")
            rows, counts = store.search_knn_filtered(queries, k, sel, order=vc.ORDER_FARTHEST_FIRST)
            FC.same_run((rows, counts), (FC.reverse_valid(want[0], want[1]), want[1]), "farthest first")
            side = torch.cuda.Stream()
            FC.same_run(_dev(store, queries, k, sel, stream=side.cuda_stream), want, "a caller's stream")
            FC.same_run(_dev(store, queries, k, sel, stream=vc.STREAM_OWN), want, "VC_STREAM_OWN")
            got = _dev(store, queries, k, sel, with_counts=False, with_stats=False)
            assert got[1] is None and got[2] is None and np.array_equal(got[0], want[0])
        assert np.any(FC.model_rows(lists, sparse, 30)[1] < 30)
        # a warm handle: small, larger (the buffers grow), small again
        sel = FC.sel_for(sparse, FC.MASK)
        first = _dev(store, queries[:5], 3, sel)
        FC.same_run(first, FC.model(lists[:5], sparse, 3), "cold")
        FC.same_run(_dev(store, queries, 64, FC.sel_for(dense, FC.MASK), k_first=8192), FC.model(lists, dense, 64, k_first=8192), "a larger call")
        FC.same_run(_dev(store, queries, 200, sel), FC.model(lists, sparse, 200), "a larger sparse call")
        again = _dev(store, queries[:5], 3, sel)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and first[2] == again[2]


# ---- 12. errors and the empty store ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [0, 2])
def test_errors_leave_the_outputs_untouched(vc, shards):
    import torch
    bits, n, nq, k = 64, 500, 4, 5
    codes = FC.uniform_case(bits)[0][:n]
    queries = np.ascontiguousarray(codes[:nq])
    sel = (np.arange(n, dtype=np.uint32) % 3).astype(np.uint32)
    L = vc.load_library()
    fn, fn_dev = (L.vc_sharded_search_knn_filtered, L.vc_sharded_search_knn_filtered_dev) if shards else (L.vc_search_knn_filtered, L.vc_search_knn_filtered_dev)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    with _make(vc, codes[:400], shards=shards, capacity=n, n_tables=4) as store:
        out, cnt = np.full(nq * k, FC.STALE, dtype=np.uint64), np.full(nq, FC.STALE32, dtype=np.uint32)
        st = vc.VcFilterStats(n_allowed=77, routes=77, n_rounds=77, k_last=77, n_windows=77, n_searched=77, n_fallback=77, n_short=77)
        h, q, s, lin, mih = store._h, p(queries), p(sel), vc.MODE_LINEAR, vc.MODE_MIH_EXACT
        #      handle q  nq  k  mode order sel kind value k_first out
        bad = [(None, q, nq, k, lin, 0, s, 0, 0, 0, p(out)), (h, None, nq, k, lin, 0, s, 0, 0, 0, p(out)), (h, q, nq, k, lin, 0, None, 0, 0, 0, p(out)),
               (h, q, nq, k, lin, 0, s, 0, 0, 0, None), (h, q, 0, k, lin, 0, s, 0, 0, 0, p(out)), (h, q, nq, 0, lin, 0, s, 0, 0, 0, p(out)),
               (h, q, nq, 8193, lin, 0, s, 0, 0, 0, p(out)), (h, q, nq, k, lin, 0, s, 0, 0, k - 1, p(out)), (h, q, nq, k, lin, 0, s, 0, 0, 8193, p(out)),
               (h, q, nq, k, lin, 0, s, 5, 0, 0, p(out)), (h, q, nq, k, lin, 0, s, 0xFFFFFFFF, 0, 0, p(out)),
               (h, q, nq, k, vc.MODE_MIH_APPROX, 0, s, 0, 0, 0, p(out)), (h, q, nq, k, 3, 0, s, 0, 0, 0, p(out)), (h, q, nq, k, lin, 2, s, 0, 0, 0, p(out))]
        for args in bad:
            assert fn(*args, p(cnt), C.byref(st)) == vc.VC_ERR_INVALID, args
        d_q, d_s = _to_dev(queries), _to_dev(sel)
        d_o, d_c = _stale(nq * k, np.uint64), _stale(nq, np.uint32)
        torch.cuda.synchronize()
        for args in bad[:-1]:                                               # (the device form has no order)
            hh, qq, n_q, kk, mode, _, ss, kind, value, kf, oo = args
            dev_args = (hh, d_q.data_ptr() if qq is not None else None, n_q, kk, mode, d_s.data_ptr() if ss is not None else None, kind, value, kf,
                        d_o.data_ptr() if oo is not None else None)
            assert fn_dev(*dev_args, d_c.data_ptr(), C.byref(st), None) == vc.VC_ERR_INVALID, args

        def untouched():
            torch.cuda.synchronize()
            assert np.all(out == FC.STALE) and np.all(cnt == FC.STALE32)
            for buf, dt in ((d_o, np.uint64), (d_c, np.uint32)):
                assert np.all(buf.cpu().numpy().view(dt) == (FC.STALE if dt == np.uint64 else FC.STALE32))
            assert all(getattr(st, name) == 77 for name in FC.STAT_NAMES)

        untouched()
        lists = DC.sorted_lists(codes[:400], queries)
        allowed = sel[:400] == 1
        FC.same_run(store.search_knn_filtered(queries, k, sel[:400], kind=FC.EQUAL, value=1, mode=mih, with_stats=True),
                    FC.model(lists, allowed, k, tie_cut=True), "a current index")
        store.add_codes(codes[400:])                                        # the index is stale now: it counts as none
        assert fn(h, q, nq, k, mih, 0, s, FC.EQUAL, 1, 0, p(out), p(cnt), C.byref(st)) == vc.VC_ERR_STATE
        assert fn_dev(h, d_q.data_ptr(), nq, k, mih, d_s.data_ptr(), FC.EQUAL, 1, 0, d_o.data_ptr(), d_c.data_ptr(), C.byref(st), None) == vc.VC_ERR_STATE
        untouched()
        FC.same_run(store.search_knn_filtered(queries, k, sel, kind=FC.EQUAL, value=1, with_stats=True),
                    FC.model(DC.sorted_lists(codes, queries), sel == 1, k), "the handle still works")


@pytest.mark.parametrize("shards", [0, 2])
def test_the_empty_store(vc, shards):
    """N == 0: VC_OK, counts 0, padded rows and zero stats"""
    bits, nq, k = 64, 3, 4
    queries = FC.uniform_case(bits)[1][:nq]
    with _make(vc, np.zeros((0, bits // 8), np.uint8), shards=shards, capacity=16) as store:
        want = (np.full((nq, k), FC.INF, dtype=np.uint64), np.zeros(nq, dtype=np.uint32), FC.zero_stats())
        FC.same_run(_dev(store, queries, k, np.zeros(1, dtype=np.uint32)), want, "device form")
        FC.same_run(store.search_knn_filtered(queries, k, np.zeros(0, dtype=np.uint32), with_stats=True), want, "host form")
