"""Single-linkage clusters at every radius in one walk: vc_cluster_levels, vc_cluster_levels_dev and their vc_sharded_* forms.

Shapes and data are ids_common.py's (plus levels_common's even-parity store), the engine-free expectation levels_common.py's: one
union-find per level over the pairs of distance <= r (test_levels_cpu.py pins it against cluster_common and against the device's
scheme run on the host).  A label is a function of the data and the level only, so every comparison is np.array_equal on the labels
and equality on the counters.  Everything runs on one device except the two-device test."""
import ctypes as C

import numpy as np
import pytest

import cluster_common as CC
import ids_common as I
import levels_common as LC

pytestmark = pytest.mark.gpu

MODES = ["LINEAR", "MIH_EXACT"]
STALE = 0xDEADBEEF


def _make(vc, name, devices=(0,), indexed=True, n_first=None):
    s = LC.shape(name)
    if s["shards"]:
        e = vc.ShardedEngine(s["bits"], capacity=s["capacity"], n_shards=s["shards"], n_tables=s["m"], devices=list(devices), id_base=s["id_base"])
    else:
        e = vc.Engine(s["bits"], capacity=s["capacity"], n_tables=s["m"], id_base=s["id_base"])
    e.add_codes(LC.codes_of(name)[:n_first])
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


def _buffer(levels, n, init=None):
    """a device label buffer of levels x n entries, every one stale; of every level the first init.shape[1] hold `init`"""
    import torch
    host = np.full((levels, n), STALE, dtype=np.uint32)
    if init is not None:
        host[:, :init.shape[1]] = init
    buf = torch.from_numpy(host.view(np.int32)).cuda()
    torch.cuda.synchronize()
    return buf


def _read(buf):
    import torch
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(np.uint32)


def _devf(vc, store):
    L = vc.load_library()
    return L.vc_sharded_cluster_levels_dev if isinstance(store, vc.ShardedEngine) else L.vc_cluster_levels_dev


def _hostf(vc, store):
    L = vc.load_library()
    return L.vc_sharded_cluster_levels if isinstance(store, vc.ShardedEngine) else L.vc_cluster_levels


def _dev(vc, store, R, mode, batch=0, init=None, stream=None):
    """the device form through the C ABI, read back: (labels [R + 1, N], n_pairs [64], n_clusters [64]) -- the WHOLE stats record,
    which comes in filled with sevens"""
    buf = _buffer(R + 1, len(store), init)
    st = vc.VcLevelsStats((7,) * 64, (7,) * 64)
    rc = _devf(vc, store)(store._h, R, mode, batch, 0 if init is None else init.shape[1], buf.data_ptr(), C.byref(st), stream)
    assert rc == vc.VC_OK, rc
    return _read(buf), np.array(st.n_pairs[:], dtype=np.uint64), np.array(st.n_clusters[:], dtype=np.uint64)


def _check(got, name, R, n_labelled=0, base=None, data=None, what=None):
    """levels 0 .. R and both counter arrays against levels_common; the entries above R are 0"""
    labels, n_pairs, n_clusters = got
    data = data or name
    want = LC.expect(data, R, base=LC.shape(name)["id_base"] if base is None else base)
    assert labels.shape == want.shape and np.array_equal(labels, want), (name, R, what)
    assert np.array_equal(n_pairs[:R + 1], LC.histogram(data, R, n_labelled)), (name, R, what)
    assert np.array_equal(n_clusters[:R + 1], LC.cluster_counts(want)), (name, R, what)
    assert not n_pairs[R + 1:].any() and not n_clusters[R + 1:].any(), (name, R, what)
    assert np.all(labels[1:] <= labels[:-1])                                         # the levels are nested


# ---- 1. one engine: every shape, mode and batch size ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", I.SINGLE)
def test_single_engine(vc, stores, name, mode):
    """every code width, an id_base above zero, S512's ids that end at 2^32 (labels with the top bit); batch sizes: the default, one
    that does not divide N, one beyond N, one id per search (S256 only).  The label buffer comes in stale."""
    store, m, n, R = stores(name), getattr(vc, "MODE_" + mode), I.SHAPES[name]["n"], LC.max_radius(name)
    assert R == 2 * I.SHAPES[name]["flips"]
    for batch in (0, 257, n + 5) + ((1,) if name == "S256" else ()):
        _check(_dev(vc, store, R, m, batch=batch), name, R, what=batch)


# ---- 2. level r is vc_cluster_radius at r, on the same handle -----------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", I.SINGLE)
def test_agreement_with_cluster_radius(vc, stores, name, mode):
    import torch
    store, m, n, R = stores(name), getattr(vc, "MODE_" + mode), I.SHAPES[name]["n"], LC.max_radius(name)
    labels, n_pairs, n_clusters = _dev(vc, store, R, m)
    for radius in CC.RADII[name]:
        buf = torch.from_numpy(np.full(n, STALE, dtype=np.uint32).view(np.int32)).cuda()
        pairs_r, clusters_r = store.cluster_radius_dev(radius, buf.data_ptr(), mode=m)
        assert np.array_equal(labels[radius], _read(buf)), radius
        assert int(n_clusters[radius]) == clusters_r and int(n_pairs[:radius + 1].sum()) == pairs_r, radius


# ---- 3. max_radius = 0: one level, the groups of identical codes -------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_max_radius_zero(vc, stores, mode):
    m = getattr(vc, "MODE_" + mode)
    for name in I.SINGLE:
        got = _dev(vc, stores(name), 0, m)
        _check(got, name, 0)
        assert got[0].shape == (1, I.SHAPES[name]["n"]) and np.array_equal(got[0][0], CC.expect(name, 0))
    lab = _dev(vc, stores("S128"), 0, m)[0][0]
    assert set(lab[list(I.GROUP7)].tolist()) == {37} and set(lab[list(I.GROUP40)].tolist()) == {100}


# ---- 4. levels without pairs of their own: only the cascade writes them -------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_empty_levels(vc, stores, mode):
    """even-popcount codes: every distance is even, so the odd levels repeat the level below"""
    store, R = stores("EVEN"), 7
    for batch in (0, 64):
        got = _dev(vc, store, R, getattr(vc, "MODE_" + mode), batch=batch)
        _check(got, "EVEN", R, what=batch)
        labels, n_pairs, _ = got
        for r in (1, 3, 5, 7):
            assert n_pairs[r] == 0 and np.array_equal(labels[r], labels[r - 1]), r
        assert all(n_pairs[r] > 0 and not np.array_equal(labels[r], labels[r - 1]) for r in (2, 4))


# ---- 5. the cap and the argument contract -------------------------------------------------------------------------------------------
def test_the_cap(vc, stores):
    """max_radius = 63 is the last legal one: 64 levels, every pair of the store; 64 is refused before any work"""
    store, n = stores("EVEN"), LC.EVEN["n"]
    got = _dev(vc, store, 63, vc.MODE_LINEAR)
    _check(got, "EVEN", 63)
    assert int(got[1].sum()) == n * (n - 1) // 2 and got[2][63] == 1
    buf = _buffer(65, n)
    st = vc.VcLevelsStats((7,) * 64, (7,) * 64)
    out = np.full((65, n), STALE, dtype=np.uint32)
    for mode in (vc.MODE_LINEAR, vc.MODE_MIH_EXACT):
        for R in (64, 65, 2 ** 32 - 1):
            assert _devf(vc, store)(store._h, R, mode, 0, 0, buf.data_ptr(), C.byref(st), None) == vc.VC_ERR_INVALID
            assert _hostf(vc, store)(store._h, R, mode, 0, 0, out.ctypes.data_as(C.c_void_p), C.byref(st)) == vc.VC_ERR_INVALID
    assert np.all(_read(buf) == np.uint32(STALE)) and np.all(out == np.uint32(STALE))
    with pytest.raises(vc.VcError) as ei:
        store.cluster_levels(64)
    assert ei.value.code == vc.VC_ERR_INVALID


@pytest.mark.parametrize("name", ["S64", "H3"])
def test_argument_contract(vc, stores, name):
    store = stores(name)
    s = I.SHAPES[name]
    n, R = s["n"], 3
    devf, hostf = _devf(vc, store), _hostf(vc, store)
    buf = _buffer(R + 1, n)
    out = np.full((R + 1, n), STALE, dtype=np.uint32)
    p_out, d_out = out.ctypes.data_as(C.c_void_p), buf.data_ptr()
    st = vc.VcLevelsStats((7,) * 64, (7,) * 64)
    INV, LIN = vc.VC_ERR_INVALID, vc.MODE_LINEAR
    for mode in (vc.MODE_MIH_APPROX, 3):                                            # MIH_APPROX and an unknown mode
        assert hostf(store._h, R, mode, 0, 0, p_out, C.byref(st)) == INV
        assert devf(store._h, R, mode, 0, 0, d_out, C.byref(st), None) == INV
    assert hostf(store._h, R, LIN, 0, 0, None, C.byref(st)) == INV                  # null labels
    assert devf(store._h, R, LIN, 0, 0, None, C.byref(st), None) == INV
    assert hostf(store._h, R, LIN, 0, n + 1, p_out, C.byref(st)) == INV             # n_labelled > N
    assert devf(store._h, R, LIN, 0, n + 1, d_out, C.byref(st), None) == INV
    assert hostf(None, R, LIN, 0, 0, p_out, C.byref(st)) == INV
    assert devf(None, R, LIN, 0, 0, d_out, C.byref(st), None) == INV
    assert np.all(out == np.uint32(STALE)) and np.all(_read(buf) == np.uint32(STALE))      # checked before any work
    with _make(vc, name, indexed=False) as bare:                                    # MIH without an index
        assert hostf(bare._h, R, vc.MODE_MIH_EXACT, 0, 0, p_out, C.byref(st)) == vc.VC_ERR_STATE
        assert devf(bare._h, R, vc.MODE_MIH_EXACT, 0, 0, d_out, C.byref(st), None) == vc.VC_ERR_STATE
        assert np.all(out == np.uint32(STALE)) and np.all(_read(buf) == np.uint32(STALE))
    with _make(vc, name, n_first=s["n"] // 2) as half:                              # a stale index counts as none
        half.add_codes(I.codes_of(name)[s["n"] // 2:])
        assert len(half) == n
        assert hostf(half._h, R, vc.MODE_MIH_EXACT, 0, 0, p_out, C.byref(st)) == vc.VC_ERR_STATE
        assert devf(half._h, R, vc.MODE_MIH_EXACT, 0, 0, d_out, C.byref(st), None) == vc.VC_ERR_STATE
        assert np.all(out == np.uint32(STALE)) and np.all(_read(buf) == np.uint32(STALE))
        data = "S128" if s["shards"] else name
        _check(_dev(vc, half, R, LIN), name, R, data=data, what="LINEAR needs no index")
    with _make(vc, name, indexed=False, n_first=0) as empty:                        # an empty store: VC_OK, zero stats, nothing written
        assert len(empty) == 0
        for mode in (LIN, vc.MODE_MIH_EXACT):
            st = vc.VcLevelsStats((7,) * 64, (7,) * 64)
            assert devf(empty._h, R, mode, 0, 0, d_out, C.byref(st), None) == vc.VC_OK and not any(st.n_pairs[:]) and not any(st.n_clusters[:])
            st = vc.VcLevelsStats((7,) * 64, (7,) * 64)
            assert hostf(empty._h, R, mode, 0, 0, p_out, C.byref(st)) == vc.VC_OK and not any(st.n_pairs[:]) and not any(st.n_clusters[:])
        assert hostf(empty._h, R, LIN, 0, 1, p_out, C.byref(st)) == INV
        labels, n_pairs, n_clusters = empty.cluster_levels(R)
        assert labels.shape == (R + 1, 0) and not n_pairs.any() and not n_clusters.any()
        assert np.all(out == np.uint32(STALE)) and np.all(_read(buf) == np.uint32(STALE))
    assert devf(store._h, R, LIN, 0, 0, d_out, None, None) == vc.VC_OK              # stats == NULL is accepted
    assert np.array_equal(_read(buf), LC.expect("S128" if s["shards"] else name, R, base=s["id_base"]))


# ---- 6. the incremental form --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["S128", "S512"])
def test_incremental(vc, name, mode):
    """an engine holds the first 60 %, its levels are computed, it receives the rest and vc_update_index, and goes on from its labels
    re-laid to the new stride: bit for bit the call from scratch, at every level"""
    s, m = I.SHAPES[name], getattr(vc, "MODE_" + mode)
    n, k, base, R = s["n"], CC.n_old(name), s["id_base"], LC.max_radius(name)
    with _make(vc, name, n_first=k) as store:
        old, old_pairs, old_clusters = _dev(vc, store, R, m)
        want_old = (LC.old_labels(name, k) + base).astype(np.uint32)
        assert np.array_equal(old, want_old) and np.array_equal(old_clusters[:R + 1], LC.cluster_counts(want_old))
        assert np.array_equal(old_pairs[:R + 1], LC.histogram(name) - LC.histogram(name, n_labelled=k))
        store.add_codes(I.codes_of(name)[k:])
        store.update_index()
        assert len(store) == n
        got = _dev(vc, store, R, m, init=old)                                       # the tail of every level is 0xDEADBEEF
        _check(got, name, R, n_labelled=k, what="incremental")
        assert not np.array_equal(got[0][:, :k], old)                               # old records changed their label
        scratch = _dev(vc, store, R, m)
        _check(scratch, name, R, what="from scratch")
        assert np.array_equal(got[0], scratch[0]) and np.array_equal(got[2], scratch[2])
        _check(_dev(vc, store, R, m, batch=300, init=old), name, R, n_labelled=k, what="incremental, batch 300")
        again = _dev(vc, store, R, m, init=got[0])                                  # n_labelled == N: re-flatten and count
        assert np.array_equal(again[0], got[0]) and not again[1].any() and np.array_equal(again[2], got[2])
        host = store.cluster_levels(R, mode=m, labels=old)                          # the binding re-lays the rows itself
        assert np.array_equal(host[0], got[0]) and np.array_equal(host[1], got[1][:R + 1]) and np.array_equal(host[2], got[2][:R + 1])


# ---- 7. sharded -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", I.SHARDED)
def test_sharded(vc, stores, name, mode):
    """H3 and H8 hold S128's records: the levels are S128's plus id_base; shard 7 of H8 is empty, GROUP7 spans H3's boundary 1999 | 2000"""
    store, m, base, R = stores(name), getattr(vc, "MODE_" + mode), I.SHAPES[name]["id_base"], LC.max_radius(name)
    for batch in (0, 1001):
        got = _dev(vc, store, R, m, batch=batch)
        _check(got, name, R, data="S128", what=batch)
    host = store.cluster_levels(R, mode=m)
    assert np.array_equal(host[0], got[0]) and np.array_equal(host[1], got[1][:R + 1]) and np.array_equal(host[2], got[2][:R + 1])
    assert set(got[0][0][list(I.GROUP7)].tolist()) == {base + 37} and set(got[0][0][list(I.GROUP40)].tolist()) == {base + 100}


def test_sharded_incremental(vc):
    """through vc_sharded_update_index: the appended records fill shard 1 and reach shard 2 of H3"""
    name = "H3"
    s = I.SHAPES[name]
    n, k, base, R = s["n"], CC.n_old(name), s["id_base"], LC.max_radius(name)
    with _make(vc, name, n_first=k) as store:
        old = _dev(vc, store, R, vc.MODE_MIH_EXACT)[0]
        assert np.array_equal(old, (LC.old_labels("S128", k) + base).astype(np.uint32))
        store.add_codes(I.codes_of(name)[k:])
        buf = _buffer(R + 1, n, old)
        before = _read(buf).copy()
        assert _devf(vc, store)(store._h, R, vc.MODE_MIH_EXACT, 0, k, buf.data_ptr(), None, None) == vc.VC_ERR_STATE
        assert np.array_equal(_read(buf), before)
        store.update_index()
        _check(_dev(vc, store, R, vc.MODE_MIH_EXACT, init=old), name, R, n_labelled=k, data="S128")
        host = store.cluster_levels(R, mode=vc.MODE_LINEAR, labels=old)
        assert np.array_equal(host[0], LC.expect("S128", R, base=base)) and np.array_equal(host[1], LC.histogram("S128", R, k))


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
            _check(_dev(vc, store, R, mode, batch=1001), name, R, data="S128")
            host = store.cluster_levels(R, mode=mode)
            assert np.array_equal(host[0], LC.expect("S128", R, base=I.SHAPES[name]["id_base"]))


# ---- 8. host form == device form; streams; a warm handle ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S256", "H3"])
def test_host_form_streams_and_a_warm_handle(vc, stores, name):
    import torch
    store = stores(name)
    s = I.SHAPES[name]
    n, R, data = s["n"], LC.max_radius(name), "S128" if s["shards"] else name
    for mode in (vc.MODE_LINEAR, vc.MODE_MIH_EXACT):
        dev = _dev(vc, store, R, mode)
        _check(dev, name, R, data=data)
        out = np.full((R + 1, n), STALE, dtype=np.uint32)                           # the C host form
        st = vc.VcLevelsStats((7,) * 64, (7,) * 64)
        assert _hostf(vc, store)(store._h, R, mode, 777, 0, out.ctypes.data_as(C.c_void_p), C.byref(st)) == vc.VC_OK
        _check((out, np.array(st.n_pairs[:], dtype=np.uint64), np.array(st.n_clusters[:], dtype=np.uint64)), name, R, data=data, what="host form")
        host = store.cluster_levels(R, mode=mode)                                   # the Python host path
        assert np.array_equal(host[0], dev[0]) and np.array_equal(host[1], dev[1][:R + 1]) and np.array_equal(host[2], dev[2][:R + 1])
        _check(_dev(vc, store, R, mode, stream=vc.STREAM_OWN), name, R, data=data, what="own stream")
        side = torch.cuda.Stream()
        buf = _buffer(R + 1, n)
        with torch.cuda.stream(side):
            n_pairs, n_clusters = store.cluster_levels_dev(R, buf.data_ptr(), mode=mode, stream=side.cuda_stream)
        side.synchronize()
        assert np.array_equal(_read(buf), dev[0]) and np.array_equal(n_pairs, dev[1][:R + 1]) and np.array_equal(n_clusters, dev[2][:R + 1])
        # the batch buffers are shared with vc_cluster_radius and vc_dbscan_radius: calls in between change nothing
        labels6, pairs6, clusters6 = store.cluster_radius(6, mode=mode)
        assert np.array_equal(labels6, dev[0][6]) and pairs6 == int(dev[1][:7].sum()) and clusters6 == int(dev[2][6])
        again = _dev(vc, store, R, mode, batch=500)
        assert all(np.array_equal(a, b) for a, b in zip(again, dev))
        labels1 = store.dbscan_radius(3, 1, mode=mode)[0]                           # min_pts 1: single linkage
        assert np.array_equal(labels1, dev[0][3])
        small = _dev(vc, store, 2, mode)                                            # a smaller call on the warm handle
        assert np.array_equal(small[0], dev[0][:3]) and np.array_equal(small[1][:3], dev[1][:3]) and np.array_equal(small[2][:3], dev[2][:3])
        again = _dev(vc, store, R, mode)
        assert all(np.array_equal(a, b) for a, b in zip(again, dev))
