"""Density clustering on the device: vc_dbscan_radius, vc_dbscan_radius_dev and their vc_sharded_* forms -- DBSCAN over the radius
graph in one walk of the radius search.

Shapes and data are ids_common.py's plus the planted shape of dbscan_common.py, whose engine-free expectation (two host methods
that test_dbscan_cpu.py pins against each other) every result is compared with.  The result is a function of the data, the radius
and min_pts only, so every comparison is np.array_equal on labels and degrees plus equality on all five statistics.  Everything
runs on one device except the two-device test."""
import ctypes as C

import numpy as np
import pytest

import cluster_common as CC
import dbscan_common as DC
import ids_common as I
import leaders_common as LC
import radius_ids_common as R

pytestmark = pytest.mark.gpu

MODES = ["LINEAR", "MIH_EXACT"]
STALE = 0xDEADBEEF


def _make(vc, name, devices=(0,), indexed=True, n_first=None, codes=None):
    s = DC.shape(name)
    if s["shards"]:
        e = vc.ShardedEngine(s["bits"], capacity=s["capacity"], n_shards=s["shards"], n_tables=s["m"], devices=list(devices), id_base=s["id_base"])
    else:
        e = vc.Engine(s["bits"], capacity=s["capacity"], n_tables=s["m"], id_base=s["id_base"])
    e.add_codes(DC.codes_of(name)[:n_first] if codes is None else codes)
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


def _buffer(n):
    """a device buffer of n uint32, every one stale"""
    import torch
    buf = torch.from_numpy(np.full(n, STALE, dtype=np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    return buf


def _read(buf):
    import torch
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(np.uint32)


def _dev(store, radius, min_pts, mode, batch=0, with_degrees=True, stream=None):
    """the device form on stale-filled buffers, read back: (labels, degrees | None, stats)"""
    lab = _buffer(len(store))
    deg = _buffer(len(store)) if with_degrees else None
    stats = store.dbscan_radius_dev(radius, min_pts, lab.data_ptr(), deg.data_ptr() if with_degrees else None, mode=mode, batch=batch, stream=stream)
    return _read(lab), (_read(deg) if with_degrees else None), stats


def _same(got, want, what=None):
    assert np.array_equal(got[0], want[0]), what
    assert got[1] is None or np.array_equal(got[1], want[1]), what
    assert got[2] == want[2], (what, got[2], want[2])


def _check(got, name, radius, min_pts, what=None):
    _same(got, DC.expect(name, radius, min_pts), (name, radius, min_pts, what))


# ---- 1. one engine: every shape, mode, radius, min_pts and batch size -----------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", I.SINGLE + ("P64",))
def test_single_engine(vc, stores, name, mode):
    """every code width, an id_base above zero, S512's ids that end at 2^32 (labels with the top bit), the planted bridges; batch
    sizes: the default, one that does not divide N, one beyond N, and one id per search (S256 and the planted shape only)"""
    store, m, n = stores(name), getattr(vc, "MODE_" + mode), DC.shape(name)["n"]
    batches = (0, 257, n + 5) + ((1,) if name in ("S256", "P64") else ())
    for radius in DC.RADII + ((DC.PLANT_R,) if name == "P64" else ()):
        for min_pts in DC.MIN_PTS + ((DC.PLANT_MIN_PTS,) if name == "P64" else ()):
            for batch in batches:
                _check(_dev(store, radius, min_pts, m, batch=batch), name, radius, min_pts, what=batch)
            _check(store.dbscan_radius(radius, min_pts, mode=m, batch=300), name, radius, min_pts, what="host form")
    _check(_dev(store, 3, 8, m, with_degrees=False), name, 3, 8, what="d_degrees NULL")
    _check(_dev(store, 6, 3, m, batch=257, with_degrees=False), name, 6, 3, what="d_degrees NULL again")
    L = vc.load_library()                                                               # the host form without degrees, without stats
    out = np.full(n, STALE, dtype=np.uint32)
    assert L.vc_dbscan_radius(store._h, 3, 8, m, 0, out.ctypes.data_as(C.c_void_p), None, None) == vc.VC_OK
    assert np.array_equal(out, DC.expect(name, 3, 8)[0])


# ---- 2. the special values of min_pts and of the radius -------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["S64", "S128", "S512", "P64"])
def test_min_pts_1_and_2_are_the_cluster_call(vc, stores, name, mode):
    """bit for bit vc_cluster_radius_dev on the same handle; min_pts = 2 reports the isolated records as noise"""
    store, m, n = stores(name), getattr(vc, "MODE_" + mode), DC.shape(name)["n"]
    own = (np.arange(n, dtype=np.int64) + DC.shape(name)["id_base"]).astype(np.uint32)
    for radius in (0, 3, 6):
        buf = _buffer(n)
        n_pairs, n_clusters = store.cluster_radius_dev(radius, buf.data_ptr(), mode=m)
        single = _read(buf)
        one = _dev(store, radius, 1, m)
        assert np.array_equal(one[0], single)
        assert one[2] == dict(n_pairs=n_pairs, n_clusters=n_clusters, n_core=n, n_border=0, n_noise=0)
        two = _dev(store, radius, 2, m, batch=257)
        isolated = int(np.count_nonzero(two[1] == 1))
        assert np.array_equal(two[0], single) and np.array_equal(two[1], one[1])
        assert two[2] == dict(n_pairs=n_pairs, n_clusters=n_clusters - isolated, n_core=n - isolated, n_border=0, n_noise=isolated)
        assert np.all(two[0][two[1] == 1] == own[two[1] == 1])
    labels, degrees, stats = _dev(store, 3, n + 1, m)                                   # min_pts > N: everything is noise
    assert np.array_equal(labels, own) and np.array_equal(degrees, DC.expect(name, 3, 1)[1])
    assert stats == dict(n_pairs=len(DC.pairs_of(name, 3)), n_clusters=0, n_core=0, n_border=0, n_noise=n)


@pytest.mark.parametrize("mode", MODES)
def test_a_radius_of_all_bits_gives_one_cluster_of_cores(vc, stores, mode):
    name = "S256"
    s, store = I.SHAPES[name], stores(name)
    n = s["n"]
    for radius in (s["bits"], s["bits"] + 44):
        labels, degrees, stats = _dev(store, radius, 64, getattr(vc, "MODE_" + mode))
        assert np.all(labels == np.uint32(s["id_base"])) and np.all(degrees == np.uint32(n))
        assert stats == dict(n_pairs=n * (n - 1) // 2, n_clusters=1, n_core=n, n_border=0, n_noise=0)


# ---- 3. the anchor rule on the planted bridges ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["P64", "PH3"])
def test_planted_bridges(vc, stores, name, mode):
    """a contested border takes the label of its SMALLEST-ID core neighbour, whether it is met from above or from below, inside one
    batch or across batches (and shards); two copies of it are cores and weld the two groups"""
    store, m, base = stores(name), getattr(vc, "MODE_" + mode), DC.shape(name)["id_base"]
    want = {"x_below": 15, "x_between": 100, "x_above": 40, "rules_disagree": 61}
    for batch in (0,) + DC.PLANT_BATCHES:
        got = _dev(store, DC.PLANT_R, DC.PLANT_MIN_PTS, m, batch=batch)
        _check(got, name, DC.PLANT_R, DC.PLANT_MIN_PTS, what=batch)
        labels, degrees, stats = got
        for k in DC.CONTESTED:
            br = DC.BRIDGES[k]
            x = br["x"][0]
            assert degrees[x] == 3 and labels[x] == np.uint32(base + want[k]), (k, batch)
            assert set(labels[list(br["a"])].tolist()) == {base + min(br["a"])} and set(labels[list(br["b"])].tolist()) == {base + min(br["b"])}
        br = DC.BRIDGES["x_twice"]
        members = list(br["a"] + br["b"] + br["x"])
        assert np.all(degrees[list(br["x"])] == 4) and np.all(labels[members] == np.uint32(base + min(members))), batch
        assert stats == dict(n_pairs=73, n_clusters=9, n_core=42, n_border=4, n_noise=404)


# ---- 4. sharded -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", I.SHARDED + ("PH3",))
def test_sharded(vc, stores, name, mode):
    """H3 and H8 hold S128's records (shard 7 of H8 is empty), PH3 the planted ones with a bridge astride the boundary 199 | 200"""
    store, m = stores(name), getattr(vc, "MODE_" + mode)
    cases = [(0, 8), (3, 3), (3, 8), (6, 64)] + ([(DC.PLANT_R, DC.PLANT_MIN_PTS)] if name == "PH3" else [])
    for radius, min_pts in cases:
        for batch in (0, 1001):
            _check(_dev(store, radius, min_pts, m, batch=batch), name, radius, min_pts, what=batch)
        _check(_dev(store, radius, min_pts, m, batch=257, with_degrees=False), name, radius, min_pts, what="d_degrees NULL")
        _check(store.dbscan_radius(radius, min_pts, mode=m), name, radius, min_pts, what="host form")
    if name != "PH3":
        base = I.SHAPES[name]["id_base"]
        want = DC.expect("S128", 3, 8)
        got = _dev(store, 3, 8, m)
        assert np.array_equal(got[0], (want[0].astype(np.int64) + base).astype(np.uint32)) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def test_two_devices(vc):
    """H3 over devices 0 and 1: the batch's ids and queries travel to the second device, its shards' results come back by peer
    copies, the three kernels run on the root.  Skipped on a one-GPU box, as test_two_devices is elsewhere."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (the cross-device leg of the sharded gather and radius search)")
    name = "H3"
    with _make(vc, name, devices=(0, 1)) as store:
        torch.cuda.set_device(store.root_device)
        for mode in (vc.MODE_LINEAR, vc.MODE_MIH_EXACT):
            for radius, min_pts in ((0, 8), (3, 8), (6, 64)):
                _check(_dev(store, radius, min_pts, mode, batch=1001), name, radius, min_pts)
                _check(store.dbscan_radius(radius, min_pts, mode=mode), name, radius, min_pts)


# ---- 5. a long-lived handle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S128", "H3"])
def test_history_independence(vc, name):
    """one handle answers dbscan calls between cluster, leaders and by-id radius calls, at varying batch and min_pts, then again in
    another order: the batch buffers are shared by the three groupers and every word of them is written before it is read -- every
    repetition returns the same bits and every call in between its own expected result"""
    import torch
    ids = I.id_list(name, 64)

    with _make(vc, name) as store:
        n = len(store)

        def dbscan(radius, min_pts, mode, batch=0, with_degrees=True):
            got = _dev(store, radius, min_pts, mode, batch=batch, with_degrees=with_degrees)
            _check(got, name, radius, min_pts, what="history")
            return got

        def cluster(radius=6, batch=0):
            buf = _buffer(n)
            n_pairs, n_clusters = store.cluster_radius_dev(radius, buf.data_ptr(), mode=vc.MODE_MIH_EXACT, batch=batch)
            want = CC.expect(name, radius)
            assert np.array_equal(_read(buf), want) and n_pairs == CC.n_pairs(name, radius) and n_clusters == CC.n_clusters(want)

        def leaders(radius=3, batch=0):
            buf = _buffer(n)
            n_pairs, n_leaders, _ = store.leaders_radius_dev(radius, buf.data_ptr(), mode=vc.MODE_MIH_EXACT, batch=batch)
            want = LC.expect(name, radius)
            assert np.array_equal(_read(buf), want) and n_pairs == CC.n_pairs(name, radius) and n_leaders == LC.n_leaders(want)

        def radius_ids():
            offs, flat, _ = R.expect_batch(name, ids, 6, vc.IDS_ONLY_GREATER)
            d_ids = torch.from_numpy(ids.view(np.int32)).cuda()
            out = torch.zeros(len(flat) + 1, dtype=torch.int64, device="cuda")
            o = torch.zeros(len(ids) + 1, dtype=torch.int64, device="cuda")
            assert store.search_radius_ids_dev(d_ids.data_ptr(), len(ids), 6, out.data_ptr(), len(flat), o.data_ptr(), mode=vc.MODE_MIH_EXACT,
                                               id_flags=vc.IDS_ONLY_GREATER) == vc.VC_OK
            torch.cuda.synchronize()
            assert np.array_equal(o.cpu().numpy().view(np.uint64), offs) and np.array_equal(out.cpu().numpy().view(np.uint64)[:-1], flat)

        first = {}
        plan = ((6, 8), (0, 3), (3, 64), (3, 8))
        for (radius, min_pts), between in zip(plan, (cluster, leaders, radius_ids, lambda: cluster(3, batch=700))):
            for mode in (vc.MODE_MIH_EXACT, vc.MODE_LINEAR):
                first[radius, min_pts, mode] = dbscan(radius, min_pts, mode)
            between()
        for (radius, min_pts), between in zip(plan[::-1], (lambda: leaders(6, batch=311), radius_ids, lambda: cluster(0), leaders)):
            for mode, batch in ((vc.MODE_LINEAR, 257), (vc.MODE_MIH_EXACT, 1001)):
                _same(dbscan(radius, min_pts, mode, batch=batch), first[radius, min_pts, mode], "repeated")
                between()
        _same(dbscan(6, 8, vc.MODE_MIH_EXACT, batch=311, with_degrees=False), first[6, 8, vc.MODE_MIH_EXACT], "NULL degrees on used scratch")
        _same(store.dbscan_radius(3, 64, mode=vc.MODE_MIH_EXACT), first[3, 64, vc.MODE_MIH_EXACT], "host form")


# ---- 6. the argument contract ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S128", "H3"])
def test_argument_contract(vc, stores, name):
    store, L = stores(name), vc.load_library()
    s = I.SHAPES[name]
    sharded, n = bool(s["shards"]), s["n"]
    devf = L.vc_sharded_dbscan_radius_dev if sharded else L.vc_dbscan_radius_dev
    hostf = L.vc_sharded_dbscan_radius if sharded else L.vc_dbscan_radius
    d_lab, d_deg = _buffer(n), _buffer(n)
    lab, deg = np.full(n, STALE, dtype=np.uint32), np.full(n, STALE, dtype=np.uint32)
    p_lab, p_deg = lab.ctypes.data_as(C.c_void_p), deg.ctypes.data_as(C.c_void_p)
    st = vc.VcDbscanStats(7, 7, 7, 7, 7)
    INV, LIN = vc.VC_ERR_INVALID, vc.MODE_LINEAR

    def untouched():
        return all(np.all(x == np.uint32(STALE)) for x in (lab, deg, _read(d_lab), _read(d_deg)))

    for mode in (vc.MODE_MIH_APPROX, 3):                                            # MIH_APPROX and an unknown mode
        assert hostf(store._h, 3, 8, mode, 0, p_lab, p_deg, C.byref(st)) == INV
        assert devf(store._h, 3, 8, mode, 0, d_lab.data_ptr(), d_deg.data_ptr(), C.byref(st), None) == INV
    for mode in (LIN, vc.MODE_MIH_EXACT):
        assert hostf(store._h, 3, 0, mode, 0, p_lab, p_deg, C.byref(st)) == INV         # min_pts == 0
        assert devf(store._h, 3, 0, mode, 0, d_lab.data_ptr(), d_deg.data_ptr(), C.byref(st), None) == INV
    assert hostf(store._h, 3, 8, LIN, 0, None, p_deg, C.byref(st)) == INV               # null labels
    assert devf(store._h, 3, 8, LIN, 0, None, d_deg.data_ptr(), C.byref(st), None) == INV
    assert hostf(None, 3, 8, LIN, 0, p_lab, p_deg, C.byref(st)) == INV                  # null handle
    assert devf(None, 3, 8, LIN, 0, d_lab.data_ptr(), d_deg.data_ptr(), C.byref(st), None) == INV
    assert untouched()                                                                  # checked before any work
    with _make(vc, name, indexed=False) as bare:                                        # MIH without an index
        assert hostf(bare._h, 3, 8, vc.MODE_MIH_EXACT, 0, p_lab, p_deg, C.byref(st)) == vc.VC_ERR_STATE
        assert devf(bare._h, 3, 8, vc.MODE_MIH_EXACT, 0, d_lab.data_ptr(), d_deg.data_ptr(), C.byref(st), None) == vc.VC_ERR_STATE
        assert untouched()
        _check(_dev(bare, 3, 8, LIN), name, 3, 8, what="LINEAR needs no index")
    with _make(vc, name, indexed=False, n_first=0) as empty:                            # an empty store: VC_OK, zero stats, nothing written
        assert len(empty) == 0
        for mode in (LIN, vc.MODE_MIH_EXACT):
            st = vc.VcDbscanStats(7, 7, 7, 7, 7)
            assert devf(empty._h, 3, 8, mode, 0, d_lab.data_ptr(), d_deg.data_ptr(), C.byref(st), None) == vc.VC_OK and not any(st.as_dict().values())
            st = vc.VcDbscanStats(7, 7, 7, 7, 7)
            assert hostf(empty._h, 3, 8, mode, 0, p_lab, p_deg, C.byref(st)) == vc.VC_OK and not any(st.as_dict().values())
        assert hostf(empty._h, 3, 0, LIN, 0, p_lab, p_deg, C.byref(st)) == INV
        labels, degrees, stats = empty.dbscan_radius(3, 8)
        assert len(labels) == 0 and len(degrees) == 0 and not any(stats.values())
        assert untouched()
    _check(_dev(store, 3, 8, vc.MODE_MIH_EXACT), name, 3, 8, what="the handle answers afterwards")


@pytest.mark.parametrize("name", ["S128", "H3"])
def test_a_stale_index_counts_as_none(vc, name):
    """add_codes leaves the index stale: VC_ERR_STATE and nothing written; update_index, and the result is a fresh handle's"""
    s = I.SHAPES[name]
    n, k = s["n"], CC.n_old(name)
    with _make(vc, name, n_first=k) as store, _make(vc, name) as fresh:
        _same(_dev(store, 3, 8, vc.MODE_MIH_EXACT), DC.expect_codes(I.codes_of(name)[:k], 3, 8, s["id_base"]), "the first 60 % alone")
        store.add_codes(I.codes_of(name)[k:])
        assert len(store) == n
        d_lab, d_deg = _buffer(n), _buffer(n)
        with pytest.raises(vc.VcError) as ei:
            store.dbscan_radius_dev(3, 8, d_lab.data_ptr(), d_deg.data_ptr(), mode=vc.MODE_MIH_EXACT)
        assert ei.value.code == vc.VC_ERR_STATE and np.all(_read(d_lab) == np.uint32(STALE)) and np.all(_read(d_deg) == np.uint32(STALE))
        with pytest.raises(vc.VcError) as ei:
            store.dbscan_radius(3, 8, mode=vc.MODE_MIH_EXACT)
        assert ei.value.code == vc.VC_ERR_STATE
        _check(_dev(store, 3, 8, vc.MODE_LINEAR), name, 3, 8, what="LINEAR does not need the index")
        store.update_index()
        for radius, min_pts in ((3, 8), (6, 64)):
            got = _dev(store, radius, min_pts, vc.MODE_MIH_EXACT)
            _check(got, name, radius, min_pts, what="after update_index")
            _same(_dev(fresh, radius, min_pts, vc.MODE_MIH_EXACT), got, "a fresh handle")


# ---- 7. end to end with removal -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S128", "H3"])
def test_dbscan_then_retain(vc, name):
    """retain(labels, RETAIN_ROOTS) keeps one representative per cluster and every noise record; a second dbscan on the survivors
    equals the expectation computed from the surviving codes"""
    s, radius, min_pts = I.SHAPES[name], 3, 8
    n, base = s["n"], s["id_base"]
    codes = I.codes_of(name)
    want = DC.expect(name, radius, min_pts)
    keep = want[0] == (np.arange(n, dtype=np.int64) + base).astype(np.uint32)
    with _make(vc, name) as store:
        labels, degrees, stats = store.dbscan_radius(radius, min_pts, mode=vc.MODE_MIH_EXACT)
        _same((labels, degrees, stats), want, "before")
        assert stats["n_clusters"] > 0 and stats["n_border"] > 0 and stats["n_noise"] > 0
        n_kept, new_ids = store.retain(labels, kind=vc.RETAIN_ROOTS)
        assert n_kept == len(store) == stats["n_clusters"] + stats["n_noise"] == int(keep.sum())
        assert np.array_equal(new_ids != np.uint32(0xFFFFFFFF), keep)
        survivors = DC.expect_codes(codes[keep], radius, min_pts, base)
        for mode in (vc.MODE_MIH_EXACT, vc.MODE_LINEAR):
            _same(_dev(store, radius, min_pts, mode), survivors, "the survivors, device form")
            _same(store.dbscan_radius(radius, min_pts, mode=mode, batch=257), survivors, "the survivors, host form")


# ---- 8. one walk ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S64", "S128"])
def test_one_walk_of_the_radius_search(vc, name):
    """the density rule needs no second search: on one handle, at the same batch, a dbscan call and a cluster call launch the MIH
    radius search equally often.  vc_get_timing's mih_launches counts every launch of the MIH routes of the radius search; the
    LINEAR route feeds neither counter (scan_launches counts the k-NN scan's events only), so MIH mode is what can be compared."""
    with _make(vc, name) as store:
        n = len(store)
        buf = _buffer(n)
        for radius, batch in ((3, 257), (6, 1001)):
            n_batches = -(-n // batch)
            store.cluster_radius_dev(radius, buf.data_ptr(), mode=vc.MODE_MIH_EXACT, batch=batch)      # the work ring has its final size now
            store.timing()
            _dev(store, radius, 8, vc.MODE_MIH_EXACT, batch=batch)
            walk = store.timing().mih_launches
            store.cluster_radius_dev(radius, buf.data_ptr(), mode=vc.MODE_MIH_EXACT, batch=batch)
            assert walk == store.timing().mih_launches and walk >= n_batches, (radius, batch, walk)
