"""Greedy leader dedup on the device: vc_leaders_radius, vc_leaders_radius_dev and their vc_sharded_* forms -- record i is a leader
iff no leader with a smaller id lies within the radius; labels = own id for a leader, else the smallest-id leader within the radius.

Shapes and data are ids_common.py's plus the thermometer set T512, the engine-free expectation leaders_common.py's (two host methods
that test_leaders_cpu.py pins against each other).  The label is a function of the data and the radius only, so every comparison is
np.array_equal on the labels and equality on n_pairs and n_leaders; n_rounds is a diagnostic and only bounded.  Everything runs on
one device except the two-device test."""
import ctypes as C

import numpy as np
import pytest

import cluster_common as CC
import ids_common as I
import leaders_common as LC
import radius_ids_common as R

pytestmark = pytest.mark.gpu

MODES = ["LINEAR", "MIH_EXACT"]
STALE = 0xDEADBEEF


def _make(vc, name, devices=(0,), indexed=True, n_first=None, codes=None):
    s = I.SHAPES[name]
    if s["shards"]:
        e = vc.ShardedEngine(s["bits"], capacity=s["capacity"], n_shards=s["shards"], n_tables=s["m"], devices=list(devices), id_base=s["id_base"])
    else:
        e = vc.Engine(s["bits"], capacity=s["capacity"], n_tables=s["m"], id_base=s["id_base"])
    e.add_codes(I.codes_of(name)[:n_first] if codes is None else codes)
    if indexed:
        e.build_index()
    return e


@pytest.fixture(scope="module")
def stores(vc):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _make(vc, name)
        return made[name]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def thermometer(vc):
    t = LC.T512
    e = vc.Engine(t["bits"], capacity=t["capacity"], n_tables=t["m"], id_base=t["id_base"])
    e.add_codes(LC.t512_codes())
    e.build_index()
    yield e
    e.close()


def _buffer(n, init=None):
    """a device label buffer of n entries, every one stale; the first len(init) hold `init`"""
    import torch
    buf = torch.from_numpy(np.full(n, STALE, dtype=np.uint32).view(np.int32)).cuda()
    if init is not None and len(init):
        buf[:len(init)] = torch.from_numpy(np.ascontiguousarray(init, dtype=np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    return buf


def _read(buf):
    import torch
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(np.uint32)


def _dev(store, radius, mode, batch=0, init=None, stream=None):
    """the device form read back: (labels, n_pairs, n_leaders, n_rounds)"""
    buf = _buffer(len(store), init)
    stats = store.leaders_radius_dev(radius, buf.data_ptr(), mode=mode, batch=batch, n_labelled=0 if init is None else len(init), stream=stream)
    return (_read(buf),) + stats


def _n_batches(n, batch, n_labelled=0):
    batch = batch or 4096
    return -(-(n - n_labelled) // batch)


def _check(got, name, radius, n_labelled=0, what=None, batch=0):
    labels, n_pairs, n_leaders, n_rounds = got
    want = LC.expect(name, radius)
    assert np.array_equal(labels, want), (name, radius, what)
    assert n_pairs == CC.n_pairs(name, radius, n_labelled), (name, radius, what)
    assert n_leaders == LC.n_leaders(want), (name, radius, what)
    assert n_rounds >= _n_batches(len(want), batch, n_labelled), (name, radius, what)      # at least one round per batch


# ---- 1. one engine: every shape, mode, radius and batch size ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", I.SINGLE)
def test_single_engine(vc, stores, name, mode):
    """every code width, an id_base above zero, S512's id range that ends at 2^32 (labels and ids with the top bit); batch sizes: the
    default, one id per search (S256 only: no batch has a neighbour inside it, the past settles everything), one that does not
    divide N, one beyond N"""
    store, m, n = stores(name), getattr(vc, "MODE_" + mode), I.SHAPES[name]["n"]
    batches = (0, 257, n + 5) + ((1,) if name == "S256" else ())
    for radius in LC.RADII[name]:
        for batch in batches:
            got = _dev(store, radius, m, batch=batch)
            _check(got, name, radius, what=batch, batch=batch)
            if batch == 1:
                assert got[3] == n                                                  # one round per batch, none more
    if name == "S512":
        assert int(LC.expect(name, 3).min()) >= 2 ** 31 and I.SHAPES[name]["id_base"] + I.SHAPES[name]["capacity"] == 2 ** 32


# ---- 2. the thermometer: chains of rounds ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_thermometer(vc, thermometer, mode):
    """T512, label[i] = id_base + i - i % (R + 1).  One batch needs 513, 342, 172 rounds: the driver goes on after every group's
    read-back.  Batches of 100: the chains cross batch boundaries, the past settles what it can.  Batches of 1: the past alone."""
    m, n = getattr(vc, "MODE_" + mode), LC.T512["n"]
    for radius in LC.T512_RADII:
        want = LC.t512_expect(radius)
        n_pairs = len(LC.t512_pairs(radius))
        host_rounds = LC.rounds(n, LC.t512_pairs(radius))[1]
        for batch in (0, 100, 1):
            labels, pairs, leaders, n_rounds = _dev(thermometer, radius, m, batch=batch)
            assert np.array_equal(labels, want), (radius, batch)
            assert pairs == n_pairs and leaders == -(-n // (radius + 1)), (radius, batch)
            if batch == 0:
                assert n_rounds == host_rounds and n_rounds > vc.LEADER_ROUND_GROUP, (radius, n_rounds)
            else:
                assert _n_batches(n, batch) <= n_rounds <= n + _n_batches(n, batch), (radius, batch, n_rounds)


# ---- 3. one leader -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_a_radius_of_all_bits_gives_one_leader(vc, stores, mode):
    name = "S256"
    s, store = I.SHAPES[name], stores(name)
    n = s["n"]
    for radius in (s["bits"], s["bits"] + 44):
        for batch in (0, 257):
            labels, n_pairs, n_leaders, n_rounds = _dev(store, radius, getattr(vc, "MODE_" + mode), batch=batch)
            assert np.all(labels == np.uint32(s["id_base"])) and n_pairs == n * (n - 1) // 2 and n_leaders == 1
            assert n_rounds >= 2 + (_n_batches(n, batch) - 1)                       # 2 in the leader's batch, 1 in every other


# ---- 4. the incremental form ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["S128", "S512"])
def test_incremental(vc, name, mode):
    """engine A holds the first 60 %, is labelled, receives the rest and vc_update_index, and goes on from its labels: bit for bit the
    call from scratch, and the incoming entries are not written"""
    s, m = I.SHAPES[name], getattr(vc, "MODE_" + mode)
    n, k, base = s["n"], CC.n_old(name), s["id_base"]
    with _make(vc, name, n_first=k) as store:
        old = {}
        for radius in (3, 6):
            labels, n_pairs, n_leaders, _ = _dev(store, radius, m)
            want = (LC.old_labels(name, radius) + base).astype(np.uint32)
            assert np.array_equal(labels, want) and n_leaders == LC.n_leaders(want)
            assert np.array_equal(labels, LC.expect(name, radius)[:k])              # the prefix property
            assert n_pairs == CC.n_pairs(name, radius) - CC.n_pairs(name, radius, k)
            old[radius] = labels
        store.add_codes(I.codes_of(name)[k:])
        assert len(store) == n
        if mode == "MIH_EXACT":                                                     # a stale index counts as none; nothing is written
            buf = _buffer(n, old[3])
            before = _read(buf).copy()
            with pytest.raises(vc.VcError) as ei:
                store.leaders_radius_dev(3, buf.data_ptr(), mode=m, n_labelled=k)
            assert ei.value.code == vc.VC_ERR_STATE and np.array_equal(_read(buf), before)
        store.update_index()
        for radius in (3, 6):
            got = _dev(store, radius, m, init=old[radius])                          # the tail of the buffer is 0xDEADBEEF
            _check(got, name, radius, n_labelled=k, what="incremental")
            assert np.array_equal(got[0][:k], old[radius])                          # the first k entries: untouched
            scratch = _dev(store, radius, m)
            _check(scratch, name, radius, what="from scratch")
            assert np.array_equal(got[0], scratch[0]) and got[2] == scratch[2]
            _check(_dev(store, radius, m, batch=300, init=old[radius]), name, radius, n_labelled=k, what="incremental, batch 300", batch=300)
            again = _dev(store, radius, m, init=got[0])                             # n_labelled == N: writes nothing and counts
            assert np.array_equal(again[0], got[0]) and again[1] == 0 and again[2] == got[2] and again[3] == 0
            host = store.leaders_radius(radius, mode=m, labels=old[radius])         # the host form: only the tail comes home
            assert np.array_equal(host[0], got[0]) and host[1:3] == got[1:3]


# ---- 5. sharded -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", I.SHARDED)
def test_sharded(vc, stores, name, mode):
    """H3 and H8 hold S128's records: labels are S128's plus id_base; shard 7 of H8 is empty, GROUP7 spans H3's boundary 1999 | 2000"""
    store, m, base = stores(name), getattr(vc, "MODE_" + mode), I.SHAPES[name]["id_base"]
    for radius in (0, 3, 6):
        want = (LC.labels_of("S128", radius) + base).astype(np.uint32)
        for batch in (0, 1001):
            got = _dev(store, radius, m, batch=batch)
            assert np.array_equal(got[0], want)
            _check(got, name, radius, what=batch, batch=batch)
        host = store.leaders_radius(radius, mode=m, batch=1001)
        assert np.array_equal(host[0], want) and host[1:] == got[1:]
    labels = _dev(store, 0, m)[0]
    assert set(labels[list(I.GROUP7)].tolist()) == {base + 37} and set(labels[list(I.GROUP40)].tolist()) == {base + 100}


def test_sharded_incremental(vc):
    """through vc_sharded_update_index: the appended records fill shard 1 and reach shard 2 of H3"""
    name, radius = "H3", 3
    s = I.SHAPES[name]
    n, k, base = s["n"], CC.n_old(name), s["id_base"]
    with _make(vc, name, n_first=k) as store:
        old = _dev(store, radius, vc.MODE_MIH_EXACT)[0]
        assert np.array_equal(old, (LC.old_labels(name, radius) + base).astype(np.uint32))
        store.add_codes(I.codes_of(name)[k:])
        buf = _buffer(n, old)
        with pytest.raises(vc.VcError) as ei:
            store.leaders_radius_dev(radius, buf.data_ptr(), mode=vc.MODE_MIH_EXACT, n_labelled=k)
        assert ei.value.code == vc.VC_ERR_STATE and np.all(_read(buf)[k:] == np.uint32(STALE))
        store.update_index()
        for mode in (vc.MODE_MIH_EXACT, vc.MODE_LINEAR):
            got = _dev(store, radius, mode, init=old)
            _check(got, name, radius, n_labelled=k)
            assert np.array_equal(got[0][:k], old)
            host = store.leaders_radius(radius, mode=mode, labels=old)
            _check(host, name, radius, n_labelled=k)


# ---- 6. host form == device form; streams -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S128", "H3"])
def test_host_form_and_streams(vc, stores, name):
    import torch
    store, L = stores(name), vc.load_library()
    n = I.SHAPES[name]["n"]
    sharded = bool(I.SHAPES[name]["shards"])
    for mode in (vc.MODE_LINEAR, vc.MODE_MIH_EXACT):
        for radius in (0, 6):
            dev = _dev(store, radius, mode)
            _check(dev, name, radius)
            host = store.leaders_radius(radius, mode=mode, batch=777)
            assert np.array_equal(host[0], dev[0]) and host[1:3] == dev[1:3]
            _check(_dev(store, radius, mode, stream=vc.STREAM_OWN), name, radius, what="own stream")
            side = torch.cuda.Stream()
            buf = _buffer(n)
            with torch.cuda.stream(side):
                stats = store.leaders_radius_dev(radius, buf.data_ptr(), mode=mode, stream=side.cuda_stream)
            side.synchronize()
            _check((_read(buf),) + stats, name, radius, what="side stream")
    # stats == NULL is accepted, by both forms
    want = LC.expect(name, 3)
    buf = _buffer(n)
    devf = L.vc_sharded_leaders_radius_dev if sharded else L.vc_leaders_radius_dev
    hostf = L.vc_sharded_leaders_radius if sharded else L.vc_leaders_radius
    assert devf(store._h, 3, vc.MODE_MIH_EXACT, 0, 0, buf.data_ptr(), None, None) == vc.VC_OK
    assert np.array_equal(_read(buf), want)
    out = np.full(n, STALE, dtype=np.uint32)
    assert hostf(store._h, 3, vc.MODE_MIH_EXACT, 0, 0, out.ctypes.data_as(C.c_void_p), None) == vc.VC_OK
    assert np.array_equal(out, want)


# ---- 7. the argument contract -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S128", "H3"])
def test_argument_contract(vc, stores, name):
    store, L = stores(name), vc.load_library()
    s = I.SHAPES[name]
    sharded, n = bool(s["shards"]), s["n"]
    devf = L.vc_sharded_leaders_radius_dev if sharded else L.vc_leaders_radius_dev
    hostf = L.vc_sharded_leaders_radius if sharded else L.vc_leaders_radius
    buf = _buffer(n)
    out = np.full(n, STALE, dtype=np.uint32)
    p_out, d_out = out.ctypes.data_as(C.c_void_p), buf.data_ptr()
    st = vc.VcLeaderStats(7, 7, 7)
    INV, LIN = vc.VC_ERR_INVALID, vc.MODE_LINEAR
    for mode in (vc.MODE_MIH_APPROX, 3):                                            # MIH_APPROX and an unknown mode
        assert hostf(store._h, 3, mode, 0, 0, p_out, C.byref(st)) == INV
        assert devf(store._h, 3, mode, 0, 0, d_out, C.byref(st), None) == INV
    assert hostf(store._h, 3, LIN, 0, 0, None, C.byref(st)) == INV                  # null labels
    assert devf(store._h, 3, LIN, 0, 0, None, C.byref(st), None) == INV
    assert hostf(store._h, 3, LIN, 0, n + 1, p_out, C.byref(st)) == INV             # n_labelled > N
    assert devf(store._h, 3, LIN, 0, n + 1, d_out, C.byref(st), None) == INV
    assert hostf(None, 3, LIN, 0, 0, p_out, C.byref(st)) == INV
    assert devf(None, 3, LIN, 0, 0, d_out, C.byref(st), None) == INV
    assert np.all(out == np.uint32(STALE)) and np.all(_read(buf) == np.uint32(STALE))      # checked before any work
    with _make(vc, name, indexed=False) as bare:                                    # MIH without an index
        assert hostf(bare._h, 3, vc.MODE_MIH_EXACT, 0, 0, p_out, C.byref(st)) == vc.VC_ERR_STATE
        assert devf(bare._h, 3, vc.MODE_MIH_EXACT, 0, 0, d_out, C.byref(st), None) == vc.VC_ERR_STATE
        assert np.all(out == np.uint32(STALE)) and np.all(_read(buf) == np.uint32(STALE))
        _check(_dev(bare, 3, LIN), name, 3, what="LINEAR needs no index")
    with _make(vc, name, indexed=False, n_first=0) as empty:                        # an empty store: VC_OK, zero stats, nothing written
        assert len(empty) == 0
        for mode in (LIN, vc.MODE_MIH_EXACT):
            st = vc.VcLeaderStats(7, 7, 7)
            assert devf(empty._h, 3, mode, 0, 0, d_out, C.byref(st), None) == vc.VC_OK and (st.n_pairs, st.n_leaders, st.n_rounds) == (0, 0, 0)
            st = vc.VcLeaderStats(7, 7, 7)
            assert hostf(empty._h, 3, mode, 0, 0, p_out, C.byref(st)) == vc.VC_OK and (st.n_pairs, st.n_leaders, st.n_rounds) == (0, 0, 0)
        assert hostf(empty._h, 3, LIN, 0, 1, p_out, C.byref(st)) == INV
        labels, n_pairs, n_leaders, n_rounds = empty.leaders_radius(3)
        assert len(labels) == 0 and (n_pairs, n_leaders, n_rounds) == (0, 0, 0)
        assert np.all(out == np.uint32(STALE)) and np.all(_read(buf) == np.uint32(STALE))
    _check(_dev(store, 3, vc.MODE_MIH_EXACT), name, 3, what="the handle answers afterwards")


# ---- 8. history independence --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S128", "H3"])
def test_history_independence(vc, name):
    """one handle answers leaders calls at R = 6, 0, 16, 3 between cluster, by-id radius and by-id k-NN calls, then the same calls in
    another order: the batch buffers are shared with vc_cluster_radius* and every word of them is written before it is read -- every
    repetition returns the same bits and every call in between its own expected result"""
    import torch
    s = I.SHAPES[name]
    ids = I.id_list(name, 64)
    res = I.resident(name, ids)
    codes = I.codes_of(name)

    with _make(vc, name) as store:
        def leaders(radius, mode, batch=0):
            got = _dev(store, radius, mode, batch=batch)
            _check(got, name, radius, what="history", batch=batch)
            return got

        def cluster(radius=6):
            buf = _buffer(len(store))
            n_pairs, n_clusters = store.cluster_radius_dev(radius, buf.data_ptr(), mode=vc.MODE_MIH_EXACT)
            want = CC.expect(name, radius)
            assert np.array_equal(_read(buf), want) and n_pairs == CC.n_pairs(name, radius) and n_clusters == CC.n_clusters(want)

        def radius_ids():
            offs, flat, _ = R.expect_batch(name, ids, 6, vc.IDS_ONLY_GREATER)
            d_ids = torch.from_numpy(ids.view(np.int32)).cuda()
            out = torch.zeros(len(flat) + 1, dtype=torch.int64, device="cuda")
            o = torch.zeros(len(ids) + 1, dtype=torch.int64, device="cuda")
            assert store.search_radius_ids_dev(d_ids.data_ptr(), len(ids), 6, out.data_ptr(), len(flat), o.data_ptr(), mode=vc.MODE_MIH_EXACT,
                                               id_flags=vc.IDS_ONLY_GREATER) == vc.VC_OK
            torch.cuda.synchronize()
            assert np.array_equal(o.cpu().numpy().view(np.uint64), offs) and np.array_equal(out.cpu().numpy().view(np.uint64)[:-1], flat)

        def knn_ids():
            k = 6
            d_ids = torch.from_numpy(ids.view(np.int32)).cuda()
            out = torch.zeros((len(ids), k), dtype=torch.int64, device="cuda")
            store.search_knn_ids_dev(d_ids.data_ptr(), len(ids), k, out.data_ptr(), mode=vc.MODE_LINEAR, id_flags=vc.IDS_EXCLUDE_SELF)
            torch.cuda.synchronize()
            rows = out.cpu().numpy().view(np.uint64)
            for i in np.flatnonzero(res)[::7]:
                assert np.array_equal(rows[i], I.brute_row(I.distances, codes, s["id_base"], ids[i], k, True)), i

        first = {}
        for radius, between in zip((6, 0, 16, 3), (cluster, knn_ids, radius_ids, lambda: cluster(3))):
            for mode in (vc.MODE_MIH_EXACT, vc.MODE_LINEAR):
                first[radius, mode] = leaders(radius, mode)
            between()
        for radius, between in zip((3, 16, 0, 6), (knn_ids, lambda: cluster(0), radius_ids, cluster)):     # the big scratch first this time
            for mode in (vc.MODE_LINEAR, vc.MODE_MIH_EXACT):
                got = leaders(radius, mode)
                assert np.array_equal(got[0], first[radius, mode][0]) and got[1:] == first[radius, mode][1:]
                between()
        small = leaders(6, vc.MODE_MIH_EXACT, batch=311)                             # another batch size on the used scratch
        assert np.array_equal(small[0], first[6, vc.MODE_MIH_EXACT][0])


# ---- 9. end to end with removal -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S128", "H3"])
def test_leaders_then_retain(vc, name):
    """leaders_radius, then retain(labels, RETAIN_ROOTS): the survivors are the leaders in order, no two of them within the radius, and
    the handle equals a fresh one fed the leaders' codes"""
    s, radius = I.SHAPES[name], 6
    n, base = s["n"], s["id_base"]
    codes = I.codes_of(name)
    want = LC.expect(name, radius)
    keep = want == (np.arange(n, dtype=np.int64) + base).astype(np.uint32)
    with _make(vc, name) as store, _make(vc, name, codes=codes[keep]) as fresh:
        labels, n_pairs, n_leaders, _ = store.leaders_radius(radius, mode=vc.MODE_MIH_EXACT)
        assert np.array_equal(labels, want) and n_leaders == int(keep.sum()) and 1 < n_leaders < n
        n_kept, new_ids = store.retain(labels, kind=vc.RETAIN_ROOTS)
        assert n_kept == n_leaders == len(store) == len(fresh)
        assert np.all(new_ids[(labels.astype(np.int64) - base)] != np.uint32(0xFFFFFFFF))      # every record's leader survived
        for j in (0, 1, n_kept // 2, n_kept - 1):                                   # the survivors' codes are the leaders', in order
            assert np.array_equal(store.get_code(base + j), codes[keep][j])
        own = (np.arange(n_kept, dtype=np.int64) + base).astype(np.uint32)
        for mode in (vc.MODE_MIH_EXACT, vc.MODE_LINEAR):                            # a second pass finds nothing to drop
            again = store.leaders_radius(radius, mode=mode)
            assert np.array_equal(again[0], own) and again[1] == 0 and again[2] == n_kept
        q = codes[[0, n // 2, n - 1]]
        for h_mode in (vc.MODE_MIH_EXACT,):
            a = [x.tolist() for x in store.search_radius(q, 8, mode=h_mode, cap_per_query=1 << 13)]
            b = [x.tolist() for x in fresh.search_radius(q, 8, mode=h_mode, cap_per_query=1 << 13)]
            assert a == b
            ra, ca = store.search_knn(q, 10, mode=h_mode)[:2]
            rb, cb = fresh.search_knn(q, 10, mode=h_mode)[:2]
            assert np.array_equal(ra, rb) and np.array_equal(ca, cb)


# ---- 10. two devices ------------------------------------------------------------------------------------------------------------------
def test_two_devices(vc):
    """H3 over devices 0 and 1: the batch's ids and queries travel to the second device, its shards' results come back by peer
    copies, the decision runs on the root.  Skipped on a one-GPU box, as test_two_devices is elsewhere."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (the cross-device leg of the sharded gather and radius search)")
    name = "H3"
    with _make(vc, name, devices=(0, 1)) as store:
        torch.cuda.set_device(store.root_device)
        for mode in (vc.MODE_LINEAR, vc.MODE_MIH_EXACT):
            for radius in (0, 3, 6):
                _check(_dev(store, radius, mode, batch=1001), name, radius, batch=1001)
                _check(store.leaders_radius(radius, mode=mode), name, radius)
