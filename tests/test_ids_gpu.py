"""Queries named by id on the device: vc_get_codes_dev, vc_search_knn_ids, vc_search_knn_ids_dev and their vc_sharded_* forms
(image_search_client::search_image_by_id for a batch, image_search_client.h:12-27; ID -> BinaryCode, linear_search.cc:45-46).

Shapes, id lists and the engine-free expectations are ids_common.py's; what they are made to exercise is pinned without a GPU
by test_ids_cpu.py.  Everything runs on one device except the last test."""
import ctypes as C

import numpy as np
import pytest

import ids_common as I

pytestmark = pytest.mark.gpu

KMAX = max(I.KS_GROUPS) + 1


def _st(s):
    return (s.radius, s.n_results, s.n_main_reads, s.n_sub_reads, s.n_local_reads, s.n_candidates)


def _make(vc, name, flags=0, devices=(0,), indexed=True, cand_cap=0):
    s = I.SHAPES[name]
    if s["shards"]:
        e = vc.ShardedEngine(s["bits"], capacity=s["capacity"], n_shards=s["shards"], n_tables=s["m"], devices=list(devices),
                             id_base=s["id_base"], flags=flags, cand_cap=cand_cap)
    else:
        e = vc.Engine(s["bits"], capacity=s["capacity"], n_tables=s["m"], id_base=s["id_base"], flags=flags, cand_cap=cand_cap)
    e.add_codes(I.codes_of(name))
    if indexed:
        e.build_index()
    return e


@pytest.fixture(scope="module")
def stores(vc):
    """every store of the module, made once: stores(name, flagged)"""
    made = {}

    def get(name, flagged=False):
        if (name, flagged) not in made:
            made[(name, flagged)] = _make(vc, name, (vc.FLAG_GLOBAL_STOP | vc.FLAG_GLOBAL_APPROX) if flagged else 0)
        return made[(name, flagged)]
    yield get
    for e in made.values():
        e.close()


class Dev:
    """a batch's device buffers (torch), and the device form of a by-id call read back"""

    def __init__(self, ids, k):
        import torch
        self.torch, self.nq, self.k = torch, len(ids), k
        self.ids = torch.from_numpy(np.ascontiguousarray(ids).view(np.int32)).cuda()
        self.out = torch.full((self.nq * k,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")   # (stale contents must not survive)
        self.cnt = torch.full((self.nq,), 0x5A5A, dtype=torch.int32, device="cuda")
        self.stats = torch.full((self.nq * 40,), 0x5A, dtype=torch.uint8, device="cuda")

    def run(self, store, mode, id_flags, stats=True, counts=True):
        store.search_knn_ids_dev(self.ids.data_ptr(), self.nq, self.k, self.out.data_ptr(), self.cnt.data_ptr() if counts else None,
                                 self.stats.data_ptr() if stats else None, mode=mode, id_flags=id_flags)
        self.torch.cuda.synchronize()
        rows = self.out.cpu().numpy().view(np.uint64).reshape(self.nq, self.k)
        cnt = self.cnt.cpu().numpy().view(np.uint32)
        raw = self.stats.cpu().numpy().reshape(-1, 40)
        st = [tuple(int(x) for x in r[:8].view(np.uint32)) + tuple(int(x) for x in r[8:].view(np.uint64)) for r in raw]
        return rows, cnt, st


def _gathered(name, ids):
    """the codes vc_get_code returns for the resident ids of a list (the host copy of the records), and which they are"""
    found = I.resident(name, ids)
    pos = ids[found].astype(np.int64) - I.SHAPES[name]["id_base"]
    return found, I.codes_of(name)[pos]


# ---- 1. get_codes_dev ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(I.SHAPES))
def test_get_codes_dev(vc, stores, name):
    import torch
    s, store = I.SHAPES[name], stores(name)
    for length in I.LIST_LENGTHS:
        ids = I.id_list(name, length)
        d_ids = torch.from_numpy(ids.view(np.int32)).cuda()
        d_codes = torch.full((length, s["bits"] // 8), 0x5A, dtype=torch.uint8, device="cuda")
        d_found = torch.full((length,), 7, dtype=torch.int32, device="cuda")
        store.get_codes_dev(d_ids.data_ptr(), length, d_codes.data_ptr(), d_found.data_ptr())
        torch.cuda.synchronize()
        found, codes = _gathered(name, ids)
        exp = np.zeros((length, s["bits"] // 8), dtype=np.uint8)
        exp[found] = codes
        assert np.array_equal(d_found.cpu().numpy(), found.astype(np.int32))
        assert np.array_equal(d_codes.cpu().numpy(), exp)
        for i in np.flatnonzero(found)[:5]:                                  # the host copy IS what vc_get_code returns
            assert np.array_equal(store.get_code(int(ids[i])), exp[i])
        d_codes.fill_(0x5A)
        store.get_codes_dev(d_ids.data_ptr(), length, d_codes.data_ptr(), None)      # d_found may be NULL
        torch.cuda.synchronize()
        assert np.array_equal(d_codes.cpu().numpy(), exp)


# ---- 2. LINEAR against brute force --------------------------------------------------------------------------------------------
_brute = {}


def _brute_top(oracle, name, qid):
    """the KMAX smallest (dist, id) of the record with global id qid over all records, None if it is not resident -- numpy only"""
    s = I.SHAPES[name]
    key = (s["bits"], int(qid) - s["id_base"])
    if key not in _brute:
        row = I.brute_row(oracle.np_distances, I.codes_of(name), 0, key[1], KMAX, False)
        _brute[key] = row
    row = _brute[key]
    return None if row is None else row + np.uint64(s["id_base"])


def _linear_expect(oracle, name, qid, k, exclude):
    top = _brute_top(oracle, name, qid)
    if top is None:
        return np.zeros(0, dtype=np.uint64)
    # self removed BY ID from the full order: the k smallest over all items except the query's own record
    return top[top != np.uint64(qid)][:k] if exclude else top[:k]


@pytest.mark.parametrize("name", list(I.SHAPES))
def test_linear_rows_are_brute_force(vc, oracle, stores, name):
    s, store = I.SHAPES[name], stores(name)
    for length in I.LIST_LENGTHS:
        ids = I.id_list(name, length)
        found = I.resident(name, ids)
        for k in s["ks"]:
            dev = Dev(ids, k)
            for id_flags in (0, vc.IDS_EXCLUDE_SELF):
                rows, cnt, st = dev.run(store, vc.MODE_LINEAR, id_flags)
                for i, qid in enumerate(ids):
                    exp = _linear_expect(oracle, name, qid, k, bool(id_flags))
                    assert cnt[i] == len(exp), (length, k, id_flags, i)
                    assert np.array_equal(rows[i], I.padded(exp, k)), (length, k, id_flags, i)
                    assert st[i] == ((0, len(exp), 0, 0, 0, s["n"]) if found[i] else (0,) * 6)
                    if id_flags and found[i]:
                        assert int(qid) not in set((rows[i][:cnt[i]] & np.uint64(0xFFFFFFFF)).tolist())


# ---- 3. the MIH modes -----------------------------------------------------------------------------------------------------------
_mih = {}


@pytest.fixture(scope="module", autouse=True)
def _close_oracles():
    """the oracles of _mih_expect live as long as the module"""
    yield
    for key in [k for k in _mih if k[0] == "oracle"]:
        _mih.pop(key).close()


def _mih_expect(oracle, name, qid, kp, approximate):
    """MihOracle.find over the union for the record qid with kp results: (canonical row, radius, n_sub_reads, n_candidates).
    The oracle's tie order at the k-th distance is not the contract, so the row is the canonical one -- the kp smallest among
    the items the loop has seen when it stops where the oracle stops -- and the oracle's own row is compared by distance."""
    s = I.SHAPES[name]
    pos = int(qid) - s["id_base"]
    key = (s["bits"], s["m"], pos, kp, approximate)
    if key not in _mih:
        codes = I.codes_of(name)
        okey = ("oracle", s["bits"], s["m"])
        if okey not in _mih:
            _mih[okey] = oracle.MihOracle(codes, s["m"], key_mode=1, id_base=0)
        mkey = ("minsub", s["bits"], s["m"], pos)
        if mkey not in _mih:
            _mih[mkey] = (oracle.np_sub_distances(codes, codes[pos], s["m"]).min(axis=1), oracle.np_distances(codes, codes[pos]))
        minsub, d = _mih[mkey]
        ores, ost = _mih[okey].find(codes[pos], kp, approximate=approximate, stop_mult=min(s["m"], 4))
        seen = np.flatnonzero(minsub <= ost.radius)
        row = np.sort(oracle.pack(d[seen], seen.astype(np.uint64)))[:kp]
        assert np.array_equal(row >> I.SH, np.sort(ores) >> I.SH)
        _mih[key] = (row, ost.radius, ost.n_sub_reads, ost.n_distinct)
    row, radius, sub, cand = _mih[key]
    return row + np.uint64(s["id_base"]), radius, sub, cand


def _check_against_oracle(vc, oracle, store, name, ids, k, mode):
    found = I.resident(name, ids)
    dev = Dev(ids, k)
    for id_flags in (0, vc.IDS_EXCLUDE_SELF):
        rows, cnt, st = dev.run(store, mode, id_flags)
        for i, qid in enumerate(ids):
            if not found[i]:
                assert cnt[i] == 0 and np.all(rows[i] == I.PACK_INF) and st[i] == (0,) * 6
                continue
            row, radius, sub, cand = _mih_expect(oracle, name, qid, k + (1 if id_flags else 0), mode == vc.MODE_MIH_APPROX)
            exp = I.strip_row(row, qid, k) if id_flags else row
            assert np.array_equal(rows[i], I.padded(exp, k)), (k, id_flags, i, qid)
            assert cnt[i] == len(exp)
            assert st[i] == (radius, len(exp), 0, sub, 0, cand), (k, id_flags, i, qid)


def _check_against_the_call_underneath(vc, store, name, ids, k, mode):
    """rows, counts and statistics bit for bit those of search_knn, same mode, k (or k + 1, stripped on the host), queried with
    the codes of the resident ids"""
    found, codes = _gathered(name, ids)
    dev = Dev(ids, k)
    for id_flags in (0, vc.IDS_EXCLUDE_SELF):
        kp = k + (1 if id_flags else 0)
        rows, cnt, st = dev.run(store, mode, id_flags)
        ref, rcnt, rst = store.search_knn(codes, kp, mode=mode, with_stats=True)
        j = 0
        for i, qid in enumerate(ids):
            if not found[i]:
                assert cnt[i] == 0 and np.all(rows[i] == I.PACK_INF) and st[i] == (0,) * 6
                continue
            exp = ref[j][:rcnt[j]]
            exp = I.strip_row(exp, qid, k) if id_flags else exp
            assert np.array_equal(rows[i], I.padded(exp, k)), (k, id_flags, i, qid)
            assert cnt[i] == len(exp)
            assert st[i] == (rst[j].radius, len(exp)) + _st(rst[j])[2:], (k, id_flags, i, qid)
            j += 1


MODES = ["MIH_EXACT", "MIH_APPROX"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", I.SINGLE)
def test_mih_single_engine_against_the_oracle(vc, oracle, stores, name, mode):
    store = stores(name)
    for length in (1, 64):
        for k in I.SHAPES[name]["ks"]:
            _check_against_oracle(vc, oracle, store, name, I.id_list(name, length), k, getattr(vc, "MODE_" + mode))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", I.SHARDED)
def test_mih_sharded_with_the_global_flags_against_the_oracle(vc, oracle, stores, name, mode):
    """VC_FLAG_GLOBAL_STOP | VC_FLAG_GLOBAL_APPROX: the store answers as one engine over the union, so the oracle over the union
    is the expectation -- statistics included"""
    store = stores(name, flagged=True)
    for length in (1, 64):
        for k in I.SHAPES[name]["ks"]:
            _check_against_oracle(vc, oracle, store, name, I.id_list(name, length), k, getattr(vc, "MODE_" + mode))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", I.SHARDED)
def test_mih_sharded_without_the_flags_equals_search_knn(vc, stores, name, mode):
    """without the flags the statistics are per-shard sums: the expectation is ShardedEngine.search_knn on the gathered codes.
    MIH_APPROX runs the k of I.unflagged_approx_ks: without VC_FLAG_GLOBAL_APPROX every shard collects 20 (k + 1) candidates of
    its OWN, and a shard that holds fewer records than that (H8's hold 750 or 500) walks all 2^32 keys of every table -- the call
    underneath and the by-id call alike, for hours (measured: H8 / MIH_APPROX with k up to 100 was stopped after 300 s)."""
    store = stores(name)
    ks = I.SHAPES[name]["ks"] if mode == "MIH_EXACT" else I.unflagged_approx_ks(name)
    for length in (1, 64):
        for k in ks:
            _check_against_the_call_underneath(vc, store, name, I.id_list(name, length), k, getattr(vc, "MODE_" + mode))


@pytest.mark.parametrize("mode", ["LINEAR"] + MODES)
@pytest.mark.parametrize("name,flagged", [(n, False) for n in I.SHAPES] + [(n, True) for n in I.SHARDED])
def test_long_list_equals_the_call_underneath(vc, stores, name, flagged, mode):
    """257 ids = more than one block of every new kernel: bit for bit the rows of search_knn on the codes get_code returns"""
    k = I.SHAPES[name]["ks"][1]
    _check_against_the_call_underneath(vc, stores(name, flagged), name, I.id_list(name, 257), k, getattr(vc, "MODE_" + mode))


# ---- 4. the host form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S64", "S128", "S512", "H3", "H8"])
def test_host_form(vc, stores, name):
    store = stores(name)
    L = vc.load_library()
    fn = L.vc_sharded_search_knn_ids if I.SHAPES[name]["shards"] else L.vc_search_knn_ids
    ids = I.id_list(name, 64)
    for mode in (vc.MODE_LINEAR, vc.MODE_MIH_EXACT, vc.MODE_MIH_APPROX):
        for k in (I.SHAPES[name]["ks"][:3] if mode != vc.MODE_MIH_APPROX else I.unflagged_approx_ks(name)[:3]):
            dev = Dev(ids, k)
            for id_flags in (0, vc.IDS_EXCLUDE_SELF):
                rows, cnt, st = dev.run(store, mode, id_flags)
                got, gcnt, gst = store.search_knn_ids(ids, k, mode=mode, id_flags=id_flags, with_stats=True)
                assert np.array_equal(got, rows) and np.array_equal(gcnt, cnt) and [_st(x) for x in gst] == st
                far, fcnt, fst = store.search_knn_ids(ids, k, mode=mode, order=vc.ORDER_FARTHEST_FIRST, id_flags=id_flags, with_stats=True)
                assert np.array_equal(fcnt, cnt) and [_st(x) for x in fst] == st
                for i in range(len(ids)):                                    # farthest first = the stripped row reversed
                    assert np.array_equal(far[i][:cnt[i]], rows[i][:cnt[i]][::-1])
                    assert np.all(far[i][cnt[i]:] == I.PACK_INF)
                bare = np.empty((len(ids), k), dtype=np.uint64)              # counts = NULL and stats = NULL are accepted
                assert fn(store._h, ids.ctypes.data_as(C.c_void_p), len(ids), k, mode, vc.ORDER_ASCENDING, id_flags,
                          bare.ctypes.data_as(C.c_void_p), None, None) == vc.VC_OK
                assert np.array_equal(bare, rows)


def test_device_form_without_counts_and_stats(vc, stores):
    for name in ("S128", "H3"):
        ids = I.id_list(name, 64)
        dev = Dev(ids, 6)
        rows, _, _ = dev.run(stores(name), vc.MODE_MIH_EXACT, vc.IDS_EXCLUDE_SELF)
        dev2 = Dev(ids, 6)
        rows2, cnt2, _ = dev2.run(stores(name), vc.MODE_MIH_EXACT, vc.IDS_EXCLUDE_SELF, stats=False, counts=False)
        assert np.array_equal(rows, rows2)
        assert np.all(cnt2 == 0x5A5A)                                        # untouched


# ---- 5. the argument contract ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S128", "H3"])
def test_argument_contract(vc, stores, name):
    store, L = stores(name), vc.load_library()
    sharded = bool(I.SHAPES[name]["shards"])
    host = L.vc_sharded_search_knn_ids if sharded else L.vc_search_knn_ids
    devf = L.vc_sharded_search_knn_ids_dev if sharded else L.vc_search_knn_ids_dev
    codesf = L.vc_sharded_get_codes_dev if sharded else L.vc_get_codes_dev
    ids = I.id_list(name, 64)
    k = 6
    dev = Dev(ids, k)
    out = np.empty((64, k), dtype=np.uint64)
    p_ids, p_out = ids.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    d_ids, d_out = dev.ids.data_ptr(), dev.out.data_ptr()
    INV = vc.VC_ERR_INVALID
    # k = VC_MAX_K is fine without the flag's k + 1 -- and refused with it
    assert host(store._h, p_ids, 64, 8192, vc.MODE_LINEAR, 0, vc.IDS_EXCLUDE_SELF, p_out, None, None) == INV
    assert devf(store._h, d_ids, 64, 8192, vc.MODE_LINEAR, vc.IDS_EXCLUDE_SELF, d_out, None, None, None) == INV
    assert host(store._h, p_ids, 64, 8193, vc.MODE_LINEAR, 0, 0, p_out, None, None) == INV
    for bad in (2, 0x80000000, 3):                                           # unknown id_flags bits
        assert host(store._h, p_ids, 64, k, vc.MODE_LINEAR, 0, bad, p_out, None, None) == INV
        assert devf(store._h, d_ids, 64, k, vc.MODE_LINEAR, bad, d_out, None, None, None) == INV
    assert host(store._h, p_ids, 0, k, vc.MODE_LINEAR, 0, 0, p_out, None, None) == INV          # nq = 0
    assert devf(store._h, d_ids, 0, k, vc.MODE_LINEAR, 0, d_out, None, None, None) == INV
    assert codesf(store._h, d_ids, 0, d_out, None, None) == INV
    assert host(store._h, None, 64, k, vc.MODE_LINEAR, 0, 0, p_out, None, None) == INV          # null pointers
    assert host(store._h, p_ids, 64, k, vc.MODE_LINEAR, 0, 0, None, None, None) == INV
    assert devf(store._h, None, 64, k, vc.MODE_LINEAR, 0, d_out, None, None, None) == INV
    assert devf(store._h, d_ids, 64, k, vc.MODE_LINEAR, 0, None, None, None, None) == INV
    assert codesf(store._h, None, 64, d_out, None, None) == INV
    assert codesf(store._h, d_ids, 64, None, None, None) == INV
    assert host(None, p_ids, 64, k, vc.MODE_LINEAR, 0, 0, p_out, None, None) == INV
    assert host(store._h, p_ids, 64, 0, vc.MODE_LINEAR, 0, 0, p_out, None, None) == INV         # k = 0, unknown mode, unknown order
    assert host(store._h, p_ids, 64, k, 3, 0, 0, p_out, None, None) == INV
    assert host(store._h, p_ids, 64, k, vc.MODE_LINEAR, 2, 0, p_out, None, None) == INV
    # the handle still works
    rows, cnt, _ = dev.run(store, vc.MODE_LINEAR, 0)
    assert np.all(cnt[I.resident(name, ids)] == k)


@pytest.mark.parametrize("name", ["S128", "H3"])
def test_mih_before_build_index_is_a_state_error(vc, name):
    ids = I.id_list(name, 64)
    with _make(vc, name, indexed=False) as store:
        for mode in (vc.MODE_MIH_EXACT, vc.MODE_MIH_APPROX):
            with pytest.raises(vc.VcError) as ei:
                store.search_knn_ids(ids, 6, mode=mode)
            assert ei.value.code == vc.VC_ERR_STATE
            with pytest.raises(vc.VcError) as ei:
                Dev(ids, 6).run(store, mode, 0)
            assert ei.value.code == vc.VC_ERR_STATE
        rows, cnt = store.search_knn_ids(ids, 6, mode=vc.MODE_LINEAR)       # LINEAR needs no index
        assert np.all(cnt[I.resident(name, ids)] == 6)


# ---- 6. history independence ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S128", "H3"])
def test_history_independence(vc, name):
    """the same id batch before and after a larger host-pointer search_knn and a radius call on the same handle: the by-id
    scratch is the handle's own, and nothing of another call's shapes or contents shows in the result"""
    ids = I.id_list(name, 64)
    codes = I.codes_of(name)
    with _make(vc, name) as store:
        def batch():
            res = []
            for mode in (vc.MODE_LINEAR, vc.MODE_MIH_EXACT, vc.MODE_MIH_APPROX):
                k = 39 if mode != vc.MODE_MIH_APPROX else I.unflagged_approx_ks(name)[-1]
                for id_flags in (0, vc.IDS_EXCLUDE_SELF):
                    rows, cnt, st = Dev(ids, k).run(store, mode, id_flags)
                    got, gcnt, gst = store.search_knn_ids(ids, k, mode=mode, id_flags=id_flags, with_stats=True)
                    res.append((rows.copy(), cnt.copy(), st, got, gcnt, [_st(x) for x in gst]))
            return res
        before = batch()
        store.search_knn(codes[:300], 120, mode=vc.MODE_MIH_EXACT, with_stats=True)      # more queries, larger k
        store.search_knn(codes[:300], 120, mode=vc.MODE_LINEAR)
        store.search_radius(codes[1000:1040], 6, mode=vc.MODE_MIH_EXACT, cap_per_query=4096)
        Dev(I.id_list(name, 257), 100).run(store, vc.MODE_LINEAR, vc.IDS_EXCLUDE_SELF)    # and a larger by-id call
        after = batch()
        for b, a in zip(before, after):
            assert np.array_equal(b[0], a[0]) and np.array_equal(b[1], a[1]) and b[2] == a[2]
            assert np.array_equal(b[3], a[3]) and np.array_equal(b[4], a[4]) and b[5] == a[5]


# ---- a LINEAR batch whose device-side ring-overflow recovery gives up -----------------------------------------------------------
def test_host_form_recovers_on_the_host_when_the_device_gives_up(vc, oracle, monkeypatch):
    """rings of 4 entries against the group of 40 identical codes: the rows overflow; the first recover launch is made to give
    up (test knob, bounded spin), so the host form answers the batch through the host-form k-NN of its handle kind, whose
    host-driven recovery always ends, and strips on the host -- the same rows.  The fallback is one driver for both kinds, so
    the sharded shape H3 runs it too; its shards each sabotage their own first recover launch."""
    monkeypatch.setenv("VC_RECOVER_TEST_FAIL", "1")
    monkeypatch.setenv("VC_RECOVER_SPIN_LIMIT", "200")
    k = 6
    for name in ("S128", "H3"):
        base = I.SHAPES[name]["id_base"]
        ids = np.array([base + I.GROUP40[0], base + I.GROUP40[39], 0xFFFFFFFF, base + I.GROUP7[3]], dtype=np.uint32)
        with _make(vc, name, cand_cap=4) as store:
            for id_flags in (vc.IDS_EXCLUDE_SELF, 0):                         # (the knob sabotages the first launch only)
                got, cnt = store.search_knn_ids(ids, k, mode=vc.MODE_LINEAR, id_flags=id_flags)
                for i, qid in enumerate(ids):
                    exp = _linear_expect(oracle, name, qid, k, bool(id_flags))
                    assert cnt[i] == len(exp) and np.array_equal(got[i], I.padded(exp, k)), (name, id_flags, i)
            if name == "S128":
                assert store.device_status() == 1


# ---- 7. two devices -------------------------------------------------------------------------------------------------------------
def test_two_devices(vc, oracle):
    """H3 over devices 0 and 1: the ids travel to the second device, its shards' slots come back by peer copies.  Skipped on a
    one-GPU box, as test_two_devices is elsewhere: it runs wherever two devices are visible."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (the cross-device leg of the sharded gather)")
    name = "H3"
    with _make(vc, name, devices=(0, 1)) as store:
        torch.cuda.set_device(store.root_device)
        ids = I.id_list(name, 257)
        found, codes = _gathered(name, ids)
        d_ids = torch.from_numpy(ids.view(np.int32)).cuda()
        d_codes = torch.zeros((257, 16), dtype=torch.uint8, device="cuda")
        d_found = torch.zeros((257,), dtype=torch.int32, device="cuda")
        store.get_codes_dev(d_ids.data_ptr(), 257, d_codes.data_ptr(), d_found.data_ptr())
        torch.cuda.synchronize()
        exp = np.zeros((257, 16), dtype=np.uint8)
        exp[found] = codes
        assert np.array_equal(d_codes.cpu().numpy(), exp) and np.array_equal(d_found.cpu().numpy(), found.astype(np.int32))
        for mode in (vc.MODE_LINEAR, vc.MODE_MIH_EXACT):
            _check_against_the_call_underneath(vc, store, name, ids, 6, mode)
