"""Device-side seeding: vc_seed_centres, vc_seed_centres_dev and their vc_sharded_* forms.

The expectation is seed_common.py's numpy model of the header's rule (pinned against plain loops, and the five crafted cases against
what they are there for, by test_seed_cpu.py).  Centres, picks, assignment and statistics are integer functions of the codes, K, the
method and `seed`, so every comparison is exact equality on every output word; output buffers are pre-filled with a stale pattern, so
every word is proven written and the words around an output proven untouched.  One device; N <= 262 149."""
import ctypes as C

import numpy as np
import pytest

import assign_common as AC
import groups_common as GC
import seed_common as SC

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
    return e


def _stale(n_words):
    import torch
    t = torch.from_numpy(np.full(n_words + 2 * PAD, SC.STALE, dtype=np.uint64).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _inner(buf, n_words, what):
    """the n_words words between the pads of a synchronised buffer; the pads must still be stale"""
    raw = buf.cpu().numpy().view(np.uint64)
    assert np.all(raw[:PAD] == SC.STALE) and np.all(raw[PAD + n_words:] == SC.STALE), (what, "words around the output")
    return raw[PAD:PAD + n_words]


def _dev(store, k, method, seed, with_picks=True, with_assign=True, with_stats=True, stream=None, sync=True):
    """the device form on stale-filled outputs: (centres, picks | None, assign | None, stats | None), or the buffers with sync=False"""
    import torch
    n, words = len(store), store.nbytes // 8
    d_c, d_p, d_a = _stale(k * words), _stale(k) if with_picks else None, _stale(n) if with_assign else None
    ptr = lambda b: b.data_ptr() + 8 * PAD if b is not None else None
    st = store.seed_centres_dev(k, ptr(d_c), ptr(d_p), ptr(d_a), method=method, seed=seed, with_stats=with_stats, stream=stream)
    assert (st is None) == (not with_stats)
    if not sync:
        return d_c, d_p, d_a, st
    torch.cuda.synchronize()
    return _collect(store, k, d_c, d_p, d_a, st)


def _collect(store, k, d_c, d_p, d_a, st, what=None):
    return (_inner(d_c, k * (store.nbytes // 8), what).view(np.uint8).reshape(k, store.nbytes),
            _inner(d_p, k, what) if d_p is not None else None, _inner(d_a, len(store), what) if d_a is not None else None, st)


def _check_all_forms(store, k, method, seed, want, what=None):
    """host form with and without assign; device form with every output, and with picks, assign and stats NULL"""
    SC.same_run(store.seed_centres(k, method, seed, with_assign=True), want, (what, "host form"))
    got = store.seed_centres(k, method, seed)
    assert got[2] is None
    SC.same_run(got, want, (what, "host form, no assign"))
    SC.same_run(_dev(store, k, method, seed), want, (what, "device form"))
    SC.same_run(_dev(store, k, method, seed, with_picks=False, with_assign=False, with_stats=False), want, (what, "device form, centres only"))


# ---- 1. the five crafted cases at every width, both methods ----------------------------------------------------------------------------
@pytest.mark.parametrize("method", SC.METHODS)
@pytest.mark.parametrize("bits", SC.WIDTHS)
@pytest.mark.parametrize("number", SC.CASES)
def test_the_crafted_cases(vc, number, bits, method):
    """ties (1), more seeds than distinct codes (2), planted records at the ends of the blocks (3), K = N (4), 257 blocks with the
    weighted pick in the last one (5)"""
    codes, k, seed = SC.case_codes(number, bits), SC.case_k(number), SC.case_seed(number, bits, method)
    want = SC.case_expect(number, bits, method)
    with _make(vc, codes) as store:
        _check_all_forms(store, k, method, seed, want, what=(number, bits, method))
        if number == 5:
            return
        SC.same_run(_dev(store, k, method, seed, with_assign=False), want, (number, bits, method, "picks and stats, best in the scratch"))
        SC.same_run(_dev(store, k, method, seed, with_picks=False, with_stats=False), want, (number, bits, method, "assign only"))


@pytest.mark.parametrize("method", SC.METHODS)
def test_case_3_weighted_under_every_edge_seed(vc, method):
    """the seeds under which the weighted mode picks each planted record (test_seed_cpu.py pins that they do), and K = 1"""
    bits = 64
    codes, k = SC.case_codes(3, bits), SC.case_k(3)
    with _make(vc, codes) as store:
        for seed in SC.EDGE_SEEDS:
            want = SC.case_expect(3, bits, method, 0, seed)
            SC.same_run(store.seed_centres(k, method, seed, with_assign=True), want, (method, seed))
        SC.same_run(_dev(store, 1, method, 5), SC.seed_model(codes, 1, method, 5), (method, "K = 1"))
        big = 0xFEDCBA9876543210                                           # `seed` is 64 bits wide
        SC.same_run(_dev(store, k, method, big), SC.seed_model(codes, k, method, big), (method, "a 64-bit seed"))


# ---- 2. what the seeds are for -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", SC.METHODS)
@pytest.mark.parametrize("bits", [64, 128])
def test_assign_is_assign_nearest_and_kmajority_takes_the_seeds(vc, bits, method):
    codes = GC.clustered_codes(4096, bits, 69 + bits, centres=40, flips=3)
    k, seed = 40, 3
    want = SC.seed_model(codes, k, method, seed)
    with _make(vc, codes) as store:
        centres, picks, assign, st = store.seed_centres(k, method, seed, with_assign=True)
        SC.same_run((centres, picks, assign, st), want, (bits, method))
        assert np.array_equal(store.assign_nearest(centres), assign)        # the same strict < in ascending index, on the same handle
        AC.same_run(store.kmajority(k, seeds=centres), AC.kmajority_model(codes, centres), (bits, method, "kmajority from the seeds"))
        assert np.array_equal(store.get_codes(SC.index_of(picks)), centres)


# ---- 3. id_base and shards ---------------------------------------------------------------------------------------------------------------
LAYOUTS = [(0, None), (3, 4650), (3, 3076), (2, 3073)]


@pytest.mark.parametrize("method", SC.METHODS)
@pytest.mark.parametrize("shards,capacity", LAYOUTS)
def test_id_base_and_shards(vc, shards, capacity, method):
    """case 3 with id_base = 1000.  Capacity 4650 in three shards: boundaries at 1550 and 3100 -- the first inside block 1, the third
    shard empty; 3076: boundaries 1025 and 2050, the planted records 1023 | 1024 and 2047 in different shards than their blocks'
    other records; two shards of 1536 and 1537.  Sharded == model, which the single engine equals as well."""
    bits = 128
    codes, k, seed = SC.case_codes(3, bits), SC.case_k(3), SC.case_seed(3, bits, method)
    want = SC.case_expect(3, bits, method, 1000)
    assert np.array_equal(SC.index_of(want[1]) - 1000, SC.index_of(SC.case_expect(3, bits, method)[1]))
    with _make(vc, codes, id_base=1000, shards=shards, capacity=capacity) as store:
        if shards:
            ranges = [store.shard_range(g) for g in range(shards)]
            assert all((r[0] - 1000) % SC.B for r in ranges[1:]), ranges     # no boundary on a block's
            assert (ranges[-1][0] - 1000 >= len(codes)) == (capacity == 4650), ranges     # the last shard's range starts behind the last record
        _check_all_forms(store, k, method, seed, want, what=(shards, capacity, method))
        if shards and method == SC.WEIGHTED:
            for s in (0, 1, 2, 3):
                SC.same_run(store.seed_centres(k, method, s, with_assign=True), SC.case_expect(3, bits, method, 1000, s), (shards, capacity, "seed", s))


@pytest.mark.parametrize("method", SC.METHODS)
@pytest.mark.parametrize("number,bits", [(1, 64), (2, 256), (4, 512), (5, 64)])
def test_the_other_cases_over_three_shards(vc, number, bits, method):
    """ties across the shard boundaries (1), the exhausted store (2: every shard reports total 0), K = N (4), and the long scan (5): the
    root finds the last shard from the totals and that shard's pick launch its last block"""
    codes, k, seed = SC.case_codes(number, bits), SC.case_k(number), SC.case_seed(number, bits, method)
    want = SC.case_expect(number, bits, method)
    with _make(vc, codes, shards=3, capacity=len(codes) + (7 if number != 5 else 0)) as store:
        SC.same_run(store.seed_centres(k, method, seed, with_assign=True), want, (number, bits, method, "host form"))
        SC.same_run(_dev(store, k, method, seed), want, (number, bits, method, "device form"))


# ---- 4. a warm handle ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [0, 3])
def test_large_small_large_and_neighbouring_calls(vc, shards):
    """grow-only scratch: a large K, a small one, the large one again, with and without the caller's assign; vc_kmajority and
    vc_group_summary, whose scratch lies next to this call's, in between -- every result unchanged"""
    bits = 64
    codes = GC.clustered_codes(4096, bits, 811, centres=60, flips=4)
    with _make(vc, codes, shards=shards, capacity=4099 if shards else None) as store:
        first = {}
        for step, (k, method) in enumerate([(300, SC.WEIGHTED), (2, SC.FARTHEST), (300, SC.WEIGHTED), (300, SC.FARTHEST), (5, SC.WEIGHTED), (300, SC.FARTHEST)]):
            want = first.setdefault((k, method), SC.seed_model(codes, k, method, 9))
            SC.same_run(_dev(store, k, method, 9, with_assign=step % 2 == 0), want, (shards, step, "device form"))
            centres, picks, assign, st = store.seed_centres(k, method, 9, with_assign=True)
            SC.same_run((centres, picks, assign, st), want, (shards, step, "host form"))
            if step in (1, 4):
                AC.same_run(store.kmajority(k, seeds=centres, max_iters=3), AC.kmajority_model(codes, centres, 3), (shards, step, "kmajority"))
            else:
                labels = SC.index_of(picks)[SC.index_of(assign)].astype(np.uint32)      # every record labelled with its seed's id
                GC.same(store.group_summary(labels), GC.model(codes, labels), (shards, step, "group_summary"))


def test_two_calls_on_two_streams_without_a_wait_between(vc):
    import torch
    bits = 128
    codes = SC.case_codes(1, bits)
    want_a, want_b = SC.seed_model(codes, 12, SC.WEIGHTED, 1), SC.seed_model(codes, 9, SC.FARTHEST, 2)
    with _make(vc, codes) as store:
        side = torch.cuda.Stream()
        for _ in range(3):
            a = _dev(store, 12, SC.WEIGHTED, 1, with_stats=False, stream=None, sync=False)       # with stats NULL the host waits for nothing
            b = _dev(store, 9, SC.FARTHEST, 2, with_stats=False, stream=side.cuda_stream, sync=False)
            torch.cuda.synchronize()
            SC.same_run(_collect(store, 12, *a), want_a, "null stream")
            SC.same_run(_collect(store, 9, *b), want_b, "side stream")


@pytest.mark.parametrize("shards", [0, 2])
def test_records_appended_between_two_calls(vc, shards):
    """no index is needed and a stale one does not matter: only the codes are read"""
    bits, n_old = 64, 3000
    codes = SC.case_codes(1, bits)
    with _make(vc, codes[:n_old], shards=shards, capacity=len(codes) + 1, n_tables=4) as store:
        store.build_index()
        for method in SC.METHODS:
            SC.same_run(store.seed_centres(8, method, 4, with_assign=True), SC.seed_model(codes[:n_old], 8, method, 4), (shards, method, "before"))
        store.add_codes(codes[n_old:])
        for method in SC.METHODS:
            SC.same_run(store.seed_centres(8, method, 4, with_assign=True), SC.seed_model(codes, 8, method, 4), (shards, method, "appended, index stale"))
            SC.same_run(_dev(store, 8, method, 4), SC.seed_model(codes, 8, method, 4), (shards, method, "appended, device form"))


# ---- 5. errors and the empty store -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [0, 2])
def test_errors_leave_the_outputs_untouched(vc, shards):
    import torch
    bits, n, k = 64, 100, 5
    codes = GC.uniform_codes(n, bits, 11)
    L = vc.load_library()
    fn, fn_dev = (L.vc_sharded_seed_centres, L.vc_sharded_seed_centres_dev) if shards else (L.vc_seed_centres, L.vc_seed_centres_dev)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    with _make(vc, codes, shards=shards) as store:
        centres = np.full((n + 1) * (bits // 64), SC.STALE, dtype=np.uint64)
        picks, assign = np.full(n + 1, SC.STALE, dtype=np.uint64), np.full(n, SC.STALE, dtype=np.uint64)
        st = vc.VcSeedStats(cost=77, radius=77, n_zero_picks=77)
        bad = [(None, k, 0, 1, p(centres)), (store._h, k, 0, 1, None), (store._h, 0, 0, 1, p(centres)), (store._h, n + 1, 1, 1, p(centres)),
               (store._h, k, 2, 1, p(centres)), (store._h, k, 0xFFFFFFFF, 1, p(centres))]
        for args in bad:
            assert fn(*args, p(picks), p(assign), C.byref(st)) == vc.VC_ERR_INVALID, args
            assert fn(*args, None, None, None) == vc.VC_ERR_INVALID, args
        assert (st.cost, st.radius, st.n_zero_picks) == (77, 77, 77)
        d_c, d_p, d_a = _stale((n + 1) * (bits // 64)), _stale(n + 1), _stale(n)
        ptr = lambda b: b.data_ptr() + 8 * PAD
        bad_dev = [(None, k, 0, 1, ptr(d_c)), (store._h, k, 0, 1, None), (store._h, 0, 0, 1, ptr(d_c)), (store._h, n + 1, 1, 1, ptr(d_c)),
                   (store._h, k, 2, 1, ptr(d_c))]
        for args in bad_dev:
            assert fn_dev(*args, ptr(d_p), ptr(d_a), C.byref(st), None) == vc.VC_ERR_INVALID, args
        torch.cuda.synchronize()
        assert np.all(centres == SC.STALE) and np.all(picks == SC.STALE) and np.all(assign == SC.STALE)
        for buf in (d_c, d_p, d_a):
            assert np.all(buf.cpu().numpy().view(np.uint64) == SC.STALE)
        assert (st.cost, st.radius, st.n_zero_picks) == (77, 77, 77)
        with pytest.raises(vc.VcError):
            store.seed_centres(k, method=2)
        for method in SC.METHODS:                                           # K = N is legal; the handle still works
            SC.same_run(store.seed_centres(n, method, 6, with_assign=True), SC.seed_model(codes, n, method, 6), (shards, method, "K = N"))


@pytest.mark.parametrize("shards", [0, 2])
def test_the_empty_store(vc, shards):
    import torch
    bits, k = 64, 3
    L = vc.load_library()
    fn, fn_dev = (L.vc_sharded_seed_centres, L.vc_sharded_seed_centres_dev) if shards else (L.vc_seed_centres, L.vc_seed_centres_dev)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    with _make(vc, np.zeros((0, bits // 8), np.uint8), shards=shards, capacity=16) as store:
        for method in SC.METHODS:
            centres, picks = np.full(k, SC.STALE, dtype=np.uint64), np.full(k, SC.STALE, dtype=np.uint64)
            st = vc.VcSeedStats(cost=9, radius=9, n_zero_picks=9)
            assert fn(store._h, k, method, 1, p(centres), p(picks), None, C.byref(st)) == vc.VC_OK          # K > N == 0 is no error
            assert st.as_dict() == SC.zero_stats() and np.all(centres == SC.STALE) and np.all(picks == SC.STALE)
            d_c, d_p = _stale(k), _stale(k)
            st = vc.VcSeedStats(cost=9, radius=9, n_zero_picks=9)
            assert fn_dev(store._h, k, method, 1, d_c.data_ptr(), d_p.data_ptr(), d_p.data_ptr(), C.byref(st), None) == vc.VC_OK
            torch.cuda.synchronize()
            assert st.as_dict() == SC.zero_stats()
            assert np.all(d_c.cpu().numpy().view(np.uint64) == SC.STALE) and np.all(d_p.cpu().numpy().view(np.uint64) == SC.STALE)
            assert fn(store._h, 0, method, 1, p(centres), None, None, None) == vc.VC_ERR_INVALID
