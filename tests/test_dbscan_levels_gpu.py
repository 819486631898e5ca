"""Density clustering at every radius in one walk: vc_dbscan_levels, vc_dbscan_levels_dev and their vc_sharded_* forms.

Shapes and data are ids_common.py's, levels_common's even-parity store and dbscan_common's planted shape; the engine-free expectation
is dbscan_levels_common.py's: one dbscan_common.dbscan per level over the pairs of distance <= r, the core distances from the sorted
distances (test_dbscan_levels_cpu.py pins both against the device's scheme run on the host).  Labels, core distances and counters
are functions of the data, the level and min_pts only, so every comparison is np.array_equal.  Everything runs on one device except
the two-device test."""
import ctypes as C

import numpy as np
import pytest

import dbscan_common as DC
import dbscan_levels_common as DL
import ids_common as I
import levels_common as LC

pytestmark = pytest.mark.gpu

MODES = ["LINEAR", "MIH_EXACT"]
STALE = 0xDEADBEEF


def _make(vc, name, devices=(0,), indexed=True, n_first=None):
    s = DL.shape(name)
    if s["shards"]:
        e = vc.ShardedEngine(s["bits"], capacity=s["capacity"], n_shards=s["shards"], n_tables=s["m"], devices=list(devices), id_base=s["id_base"])
    else:
        e = vc.Engine(s["bits"], capacity=s["capacity"], n_tables=s["m"], id_base=s["id_base"])
    e.add_codes((DC.codes_of(name) if name in DC.PLANTED else LC.codes_of(name))[:n_first])
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


def _buffer(*shape):
    """a device buffer of uint32, every one stale"""
    import torch
    buf = torch.from_numpy(np.full(shape, STALE, dtype=np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    return buf


def _read(buf):
    import torch
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(np.uint32)


def _sevens(vc):
    return vc.VcDbscanLevelsStats(*[(7,) * 64] * 5)


def _whole(st):
    """the WHOLE stats record, all 64 entries of every row"""
    return {f: np.array(getattr(st, f)[:], dtype=np.uint64) for f in DL.FIELDS}


def _devf(vc, store):
    L = vc.load_library()
    return L.vc_sharded_dbscan_levels_dev if isinstance(store, vc.ShardedEngine) else L.vc_dbscan_levels_dev


def _hostf(vc, store):
    L = vc.load_library()
    return L.vc_sharded_dbscan_levels if isinstance(store, vc.ShardedEngine) else L.vc_dbscan_levels


def _dev(vc, store, R, min_pts, mode, batch=0, with_cd=True, stream=None):
    """the device form through the C ABI on stale-filled buffers, read back: (labels [R + 1, N], core_dist [N] | None, stats); the
    stats record comes in filled with sevens"""
    lab = _buffer(R + 1, len(store))
    cd = _buffer(len(store)) if with_cd else None
    st = _sevens(vc)
    rc = _devf(vc, store)(store._h, R, min_pts, mode, batch, lab.data_ptr(), cd.data_ptr() if with_cd else None, C.byref(st), stream)
    assert rc == vc.VC_OK, rc
    return _read(lab), (_read(cd) if with_cd else None), _whole(st)


def _check(got, name, R, min_pts, data=None, what=None):
    """levels 0 .. R, the core distances and all five counter rows against dbscan_levels_common; the entries above R are 0"""
    labels, cd, stats = got
    want = DL.expect(data or name, min_pts, R, base=DL.shape(name)["id_base"])
    msg = (name, R, min_pts, what)
    assert labels.shape == want[0].shape and np.array_equal(labels, want[0]), msg
    assert cd is None or np.array_equal(cd, want[1]), msg
    for f in DL.FIELDS:
        assert np.array_equal(stats[f][:R + 1], want[2][f]), msg + (f, stats[f][:R + 1], want[2][f])
        assert not stats[f][R + 1:].any(), msg + (f,)


def _same(a, b):
    assert np.array_equal(a[0], b[0]) and (a[1] is None or b[1] is None or np.array_equal(a[1], b[1]))
    assert all(np.array_equal(a[2][f], b[2][f]) for f in DL.FIELDS)


# ---- 1. one engine: every shape and mode ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", I.SINGLE)
def test_single_engine(vc, stores, name, mode):
    """every code width, an id_base above zero, S512's ids that end at 2^32 (labels with the top bit); the default batch and one that
    does not divide N.  All buffers come in stale."""
    store, m, R = stores(name), getattr(vc, "MODE_" + mode), LC.max_radius(name)
    _check(_dev(vc, store, R, 3, m), name, R, 3)
    _check(_dev(vc, store, R, 8, m, batch=257), name, R, 8, what=257)


# ---- 2. level r is vc_dbscan_radius at r, on the same handle; min_pts 1 is vc_cluster_levels ---------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_agreement_with_the_per_radius_calls(vc, stores, mode):
    store, m, n, R = stores("S64"), getattr(vc, "MODE_" + mode), I.SHAPES["S64"]["n"], LC.max_radius("S64")
    for min_pts in (1, 3, 64):
        labels, cd, stats = _dev(vc, store, R, min_pts, m)
        for r in range(R + 1):
            lab, deg = _buffer(n), _buffer(n)
            st = store.dbscan_radius_dev(r, min_pts, lab.data_ptr(), deg.data_ptr(), mode=m)
            assert np.array_equal(labels[r], _read(lab)), (min_pts, r)
            assert np.array_equal(cd <= r, _read(deg) >= min_pts), (min_pts, r)
            assert st == dict(n_pairs=int(stats["n_pairs"][:r + 1].sum()), n_clusters=int(stats["n_clusters"][r]), n_core=int(stats["n_core"][r]),
                              n_border=int(stats["n_border"][r]), n_noise=int(stats["n_noise"][r])), (min_pts, r)
    labels, cd, stats = _dev(vc, store, R, 1, m)
    single = _buffer(R + 1, n)
    n_pairs, n_clusters = store.cluster_levels_dev(R, single.data_ptr(), mode=m)
    assert np.array_equal(labels, _read(single)) and not cd.any()
    assert np.array_equal(stats["n_pairs"][:R + 1], n_pairs) and np.array_equal(stats["n_clusters"][:R + 1], n_clusters)
    assert np.all(stats["n_core"][:R + 1] == n) and not stats["n_border"].any() and not stats["n_noise"].any()


# ---- 3. the planted bridges: contested borders, batch borders ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_planted_bridges(vc, stores, mode):
    """one id per search, X with a0 and b0 in one batch of 7, a batch border of 257 between X and b0: the core launch of a batch
    precedes its edge launch, and an anchor is lowered from a later batch"""
    store, m, base = stores("P64"), getattr(vc, "MODE_" + mode), DC.PLANTED["P64"]["id_base"]
    for min_pts in (DC.PLANT_MIN_PTS, 5):
        for batch in DC.PLANT_BATCHES:
            got = _dev(vc, store, 4, min_pts, m, batch=batch)
            _check(got, "P64", 4, min_pts, what=batch)
    labels = _dev(vc, store, 4, DC.PLANT_MIN_PTS, m, batch=7)[0]
    for key in DC.CONTESTED:                                                          # at PLANT_R the contested X goes with min(a0, b0)
        br = DC.BRIDGES[key]
        x, a0, b0 = br["x"][0], br["a"][0], br["b"][0]
        assert labels[DC.PLANT_R][x] == labels[DC.PLANT_R][min(a0, b0)] != base + x, key
    br = DC.BRIDGES["rules_disagree"]
    assert labels[DC.PLANT_R][br["x"][0]] == base + min(br["b"]) != base + min(br["a"] + br["b"])


# ---- 4. levels that only the cascade and the prefix minimum write; records that never become a core ------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_empty_levels_and_core_never(vc, stores, mode):
    store, R = stores("EVEN"), 7
    for batch in (0, 64):
        got = _dev(vc, store, R, 64, getattr(vc, "MODE_" + mode), batch=batch)
        _check(got, "EVEN", R, 64, what=batch)
    labels, cd, stats = got
    assert np.count_nonzero(cd == vc.CORE_NEVER) == 27 and not np.any(cd[cd != vc.CORE_NEVER] % 2)
    for r in (1, 3, 5, 7):
        assert stats["n_pairs"][r] == 0 and np.array_equal(labels[r], labels[r - 1]), r
    assert stats["n_border"][7] == 27 and stats["n_noise"][7] == 0                      # the 27 are borders through the prefix minimum


# ---- 5. edge cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_edge_cases(vc, stores, mode):
    store, m, s = stores("S64"), getattr(vc, "MODE_" + mode), I.SHAPES["S64"]
    n, R = s["n"], LC.max_radius("S64")
    own = (np.arange(n, dtype=np.int64) + s["id_base"]).astype(np.uint32)
    got = _dev(vc, store, 0, 3, m)                                                    # max_radius 0: one level
    _check(got, "S64", 0, 3)
    assert got[0].shape == (1, n) and np.array_equal(got[0][0], DC.expect("S64", 0, 3)[0])
    labels, cd, stats = _dev(vc, store, R, 2 ** 32 - 1, m, batch=257)                 # no record has 2^32 - 1 neighbours: all noise
    assert np.all(labels == own) and np.all(cd == vc.CORE_NEVER)
    assert np.array_equal(stats["n_pairs"][:R + 1], LC.histogram("S64")) and np.all(stats["n_noise"][:R + 1] == n)
    assert not stats["n_clusters"].any() and not stats["n_core"].any() and not stats["n_border"].any() and not stats["n_noise"][R + 1:].any()
    _check(_dev(vc, store, R, 8, m, with_cd=False), "S64", R, 8, what="d_core_dist NULL")
    _check(_dev(vc, store, R, 3, m, batch=1001, with_cd=False), "S64", R, 3, what="d_core_dist NULL again")
    out = np.full((R + 1, n), STALE, dtype=np.uint32)                                 # the host form without core_dist, without stats
    assert _hostf(vc, store)(store._h, R, 8, m, 0, out.ctypes.data_as(C.c_void_p), None, None) == vc.VC_OK
    assert np.array_equal(out, DL.expect("S64", 8)[0])


def test_the_cap(vc, stores):
    """max_radius = 63 is the last legal one: 64 levels, every pair of the store; 64 is refused before any work"""
    store, n = stores("EVEN"), LC.EVEN["n"]
    got = _dev(vc, store, 63, 8, vc.MODE_LINEAR)
    _check(got, "EVEN", 63, 8)
    assert int(got[2]["n_pairs"].sum()) == n * (n - 1) // 2 and got[2]["n_clusters"][63] == 1 and got[2]["n_core"][63] == n
    lab, cd, st = _buffer(65, n), _buffer(n), _sevens(vc)
    out, out_cd = np.full((65, n), STALE, dtype=np.uint32), np.full(n, STALE, dtype=np.uint32)
    for mode in (vc.MODE_LINEAR, vc.MODE_MIH_EXACT):
        for R in (64, 65, 2 ** 32 - 1):
            assert _devf(vc, store)(store._h, R, 8, mode, 0, lab.data_ptr(), cd.data_ptr(), C.byref(st), None) == vc.VC_ERR_INVALID
            assert _hostf(vc, store)(store._h, R, 8, mode, 0, out.ctypes.data_as(C.c_void_p), out_cd.ctypes.data_as(C.c_void_p), C.byref(st)) == vc.VC_ERR_INVALID
    assert np.all(_read(lab) == np.uint32(STALE)) and np.all(_read(cd) == np.uint32(STALE)) and np.all(out == np.uint32(STALE)) and np.all(out_cd == np.uint32(STALE))
    with pytest.raises(vc.VcError) as ei:
        store.dbscan_levels(64, 8)
    assert ei.value.code == vc.VC_ERR_INVALID


# ---- 6. the argument contract -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S64", "H3"])
def test_argument_contract(vc, stores, name):
    store = stores(name)
    s = I.SHAPES[name]
    n, R, data = s["n"], 3, "S128" if s["shards"] else name
    devf, hostf = _devf(vc, store), _hostf(vc, store)
    lab, cd = _buffer(R + 1, n), _buffer(n)
    out, out_cd = np.full((R + 1, n), STALE, dtype=np.uint32), np.full(n, STALE, dtype=np.uint32)
    p_out, p_cd, d_out, d_cd = out.ctypes.data_as(C.c_void_p), out_cd.ctypes.data_as(C.c_void_p), lab.data_ptr(), cd.data_ptr()
    st = _sevens(vc)
    INV, LIN = vc.VC_ERR_INVALID, vc.MODE_LINEAR

    def untouched():
        return (np.all(out == np.uint32(STALE)) and np.all(out_cd == np.uint32(STALE)) and np.all(_read(lab) == np.uint32(STALE))
                and np.all(_read(cd) == np.uint32(STALE)))

    for mode in (vc.MODE_MIH_APPROX, 3):                                            # MIH_APPROX and an unknown mode
        assert hostf(store._h, R, 3, mode, 0, p_out, p_cd, C.byref(st)) == INV
        assert devf(store._h, R, 3, mode, 0, d_out, d_cd, C.byref(st), None) == INV
    for mode in (LIN, vc.MODE_MIH_EXACT):
        assert hostf(store._h, R, 3, mode, 0, None, p_cd, C.byref(st)) == INV       # null labels
        assert devf(store._h, R, 3, mode, 0, None, d_cd, C.byref(st), None) == INV
        assert hostf(store._h, R, 0, mode, 0, p_out, p_cd, C.byref(st)) == INV      # min_pts 0
        assert devf(store._h, R, 0, mode, 0, d_out, d_cd, C.byref(st), None) == INV
        assert hostf(store._h, vc.LEVELS_MAX, 3, mode, 0, p_out, p_cd, C.byref(st)) == INV      # max_radius beyond the cap
        assert devf(store._h, vc.LEVELS_MAX, 3, mode, 0, d_out, d_cd, C.byref(st), None) == INV
    assert hostf(None, R, 3, LIN, 0, p_out, p_cd, C.byref(st)) == INV
    assert devf(None, R, 3, LIN, 0, d_out, d_cd, C.byref(st), None) == INV
    assert untouched()                                                              # checked before any work
    with _make(vc, name, indexed=False) as bare:                                    # MIH without an index
        assert hostf(bare._h, R, 3, vc.MODE_MIH_EXACT, 0, p_out, p_cd, C.byref(st)) == vc.VC_ERR_STATE
        assert devf(bare._h, R, 3, vc.MODE_MIH_EXACT, 0, d_out, d_cd, C.byref(st), None) == vc.VC_ERR_STATE
        assert untouched()
        _check(_dev(vc, bare, R, 3, LIN), name, R, 3, data=data, what="LINEAR needs no index")
    with _make(vc, name, n_first=s["n"] // 2) as half:                              # a stale index counts as none
        half.add_codes(I.codes_of(name)[s["n"] // 2:])
        assert len(half) == n
        assert hostf(half._h, R, 3, vc.MODE_MIH_EXACT, 0, p_out, p_cd, C.byref(st)) == vc.VC_ERR_STATE
        assert devf(half._h, R, 3, vc.MODE_MIH_EXACT, 0, d_out, d_cd, C.byref(st), None) == vc.VC_ERR_STATE
        assert untouched()
    with _make(vc, name, indexed=False, n_first=0) as empty:                        # an empty store: VC_OK, zero stats, nothing written
        assert len(empty) == 0
        for mode in (LIN, vc.MODE_MIH_EXACT):
            st = _sevens(vc)
            assert devf(empty._h, R, 3, mode, 0, d_out, d_cd, C.byref(st), None) == vc.VC_OK and not any(v.any() for v in _whole(st).values())
            st = _sevens(vc)
            assert hostf(empty._h, R, 3, mode, 0, p_out, p_cd, C.byref(st)) == vc.VC_OK and not any(v.any() for v in _whole(st).values())
        assert hostf(empty._h, R, 0, LIN, 0, p_out, p_cd, C.byref(st)) == INV
        labels, core_dist, stats = empty.dbscan_levels(R, 3)
        assert labels.shape == (R + 1, 0) and core_dist.shape == (0,) and not any(v.any() for v in stats.values())
        assert untouched()
    assert devf(store._h, R, 3, LIN, 0, d_out, d_cd, None, None) == vc.VC_OK        # stats == NULL is accepted
    want = DL.expect(data, 3, R, base=s["id_base"])
    assert np.array_equal(_read(lab), want[0]) and np.array_equal(_read(cd), want[1])


# ---- 7. sharded -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", I.SHARDED)
def test_sharded(vc, stores, name, mode):
    """H3 and H8 hold S128's records: the levels are S128's plus id_base; shard 7 of H8 is empty"""
    store, m, R = stores(name), getattr(vc, "MODE_" + mode), LC.max_radius(name)
    _check(_dev(vc, store, R, 3, m), name, R, 3, data="S128")
    got = _dev(vc, store, R, 8, m, batch=1001)
    _check(got, name, R, 8, data="S128", what=1001)
    labels, core_dist, stats = store.dbscan_levels(R, 8, mode=m)
    assert np.array_equal(labels, got[0]) and np.array_equal(core_dist, got[1])
    assert all(np.array_equal(stats[f], got[2][f][:R + 1]) for f in DL.FIELDS)


@pytest.mark.parametrize("mode", MODES)
def test_sharded_planted(vc, stores, mode):
    """PH3: the X of "x_above" is the first record of shard 1, its anchors lie in shard 0"""
    store, m = stores("PH3"), getattr(vc, "MODE_" + mode)
    assert DC.BRIDGES["x_above"]["x"][0] == 200
    for min_pts in (DC.PLANT_MIN_PTS, 5):
        for batch in (0, 7):
            _check(_dev(vc, store, 4, min_pts, m, batch=batch), "PH3", 4, min_pts, what=batch)


def test_two_devices(vc):
    """H3 over devices 0 and 1: the kernels run on the root with global ids.  Skipped on a one-GPU box, as test_two_devices is elsewhere."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (the cross-device leg of the sharded gather and radius search)")
    name = "H3"
    R = LC.max_radius(name)
    with _make(vc, name, devices=(0, 1)) as store:
        torch.cuda.set_device(store.root_device)
        for mode in (vc.MODE_LINEAR, vc.MODE_MIH_EXACT):
            _check(_dev(vc, store, R, 8, mode, batch=1001), name, R, 8, data="S128")
            host = store.dbscan_levels(R, 8, mode=mode)
            assert np.array_equal(host[0], DL.expect("S128", 8, R, base=I.SHAPES[name]["id_base"])[0])


# ---- 8. one walk ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S64", "S128"])
def test_one_walk_of_the_radius_search(vc, name):
    """all levels need no second search: on one handle, at the same batch, the call and ONE vc_dbscan_radius_dev at max_radius launch
    the MIH radius search equally often (vc_get_timing's mih_launches, as test_dbscan_gpu.py compares it)"""
    with _make(vc, name) as store:
        n = len(store)
        lab = _buffer(n)
        for R, batch in ((3, 257), (6, 1001)):
            n_batches = -(-n // batch)
            store.dbscan_radius_dev(R, 8, lab.data_ptr(), None, mode=vc.MODE_MIH_EXACT, batch=batch)      # the work ring has its final size now
            store.timing()
            _dev(vc, store, R, 8, vc.MODE_MIH_EXACT, batch=batch)
            walk = store.timing().mih_launches
            store.dbscan_radius_dev(R, 8, lab.data_ptr(), None, mode=vc.MODE_MIH_EXACT, batch=batch)
            assert walk == store.timing().mih_launches and walk >= n_batches, (R, batch, walk)


# ---- 9. host form == device form; streams; a warm handle ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S256", "H3"])
def test_host_form_streams_and_a_warm_handle(vc, stores, name):
    import torch
    store = stores(name)
    s = I.SHAPES[name]
    n, R, data, min_pts = s["n"], LC.max_radius(name), "S128" if s["shards"] else name, 8
    for mode in (vc.MODE_LINEAR, vc.MODE_MIH_EXACT):
        dev = _dev(vc, store, R, min_pts, mode)
        _check(dev, name, R, min_pts, data=data)
        out, out_cd = np.full((R + 1, n), STALE, dtype=np.uint32), np.full(n, STALE, dtype=np.uint32)      # the C host form
        st = _sevens(vc)
        assert _hostf(vc, store)(store._h, R, min_pts, mode, 777, out.ctypes.data_as(C.c_void_p), out_cd.ctypes.data_as(C.c_void_p), C.byref(st)) == vc.VC_OK
        _check((out, out_cd, _whole(st)), name, R, min_pts, data=data, what="host form")
        labels, core_dist, stats = store.dbscan_levels(R, min_pts, mode=mode)       # the Python host path
        assert np.array_equal(labels, dev[0]) and np.array_equal(core_dist, dev[1]) and all(np.array_equal(stats[f], dev[2][f][:R + 1]) for f in DL.FIELDS)
        _check(_dev(vc, store, R, min_pts, mode, stream=vc.STREAM_OWN), name, R, min_pts, data=data, what="own stream")
        side = torch.cuda.Stream()
        lab, cd = _buffer(R + 1, n), _buffer(n)
        with torch.cuda.stream(side):
            stats = store.dbscan_levels_dev(R, min_pts, lab.data_ptr(), cd.data_ptr(), mode=mode, stream=side.cuda_stream)
        side.synchronize()
        assert np.array_equal(_read(lab), dev[0]) and np.array_equal(_read(cd), dev[1]) and all(np.array_equal(stats[f], dev[2][f][:R + 1]) for f in DL.FIELDS)
        # the batch buffers are shared with vc_dbscan_radius, vc_cluster_levels and the by-id radius search: calls in between change nothing
        labels6, degrees6, stats6 = store.dbscan_radius(6, min_pts, mode=mode)
        assert np.array_equal(labels6, dev[0][6]) and np.array_equal(degrees6 >= min_pts, dev[1] <= 6) and stats6["n_clusters"] == int(dev[2]["n_clusters"][6])
        _same(_dev(vc, store, R, min_pts, mode, batch=500), dev)
        single = store.cluster_levels(3, mode=mode)[0]
        ids = (np.arange(0, n, 97, dtype=np.int64) + s["id_base"]).astype(np.uint32)
        store.search_radius_ids(ids, 4, mode=mode, cap_per_query=n)
        again = _dev(vc, store, R, 1, mode)                                         # min_pts 1: single linkage
        assert np.array_equal(again[0][:4], single) and not again[1].any()
        small = _dev(vc, store, 2, min_pts, mode, with_cd=False)                    # a smaller call on the warm handle
        assert np.array_equal(small[0], dev[0][:3]) and all(np.array_equal(small[2][f][:3], dev[2][f][:3]) for f in DL.FIELDS)
        _same(_dev(vc, store, R, min_pts, mode), dev)
