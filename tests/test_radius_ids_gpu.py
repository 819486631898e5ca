"""Radius search for queries named by id on the device: vc_search_radius_ids, vc_search_radius_ids_dev and their vc_sharded_*
forms ("which records lie within R of these records"; search_R_neighbors, search_worker.cc:222-264, behind
search_image_by_id's id -> code read, image_search_client.h:12-27).

Shapes, data and id lists are ids_common.py's, the engine-free expectation radius_ids_common.py's; what they are made to
exercise is pinned without a GPU by test_radius_ids_cpu.py.  Everything runs on one device except the two-device test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ids_common as I
import radius_ids_common as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A5A5A5A5A5A5A5A
MODES = ["LINEAR", "MIH_EXACT"]


def _make(vc, name, devices=(0,), indexed=True):
    s = I.SHAPES[name]
    if s["shards"]:
        e = vc.ShardedEngine(s["bits"], capacity=s["capacity"], n_shards=s["shards"], n_tables=s["m"], devices=list(devices), id_base=s["id_base"])
    else:
        e = vc.Engine(s["bits"], capacity=s["capacity"], n_tables=s["m"], id_base=s["id_base"])
    e.add_codes(I.codes_of(name))
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


def _lists(name):
    return [I.id_list(name, length) for length in I.LIST_LENGTHS] + [R.edge_list(name)]


def _dev(store, ids, radius, mode, id_flags, cap, stream=None, with_buffer=True):
    """the device form read back: (rc, offsets [nq + 1], the whole output buffer of cap + 1 entries, the last a sentinel)"""
    import torch
    nq = len(ids)
    d_ids = torch.from_numpy(np.ascontiguousarray(ids).view(np.int32)).cuda()
    out = torch.full((cap + 1,), SENTINEL, dtype=torch.int64, device="cuda")       # (stale contents must not survive)
    offs = torch.full((nq + 1,), 0x5A5A, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc = store.search_radius_ids_dev(d_ids.data_ptr(), nq, radius, out.data_ptr() if with_buffer else None, cap, offs.data_ptr(), mode=mode,
                                     id_flags=id_flags, stream=stream)
    torch.cuda.synchronize()
    return rc, offs.cpu().numpy().view(np.uint64), out.cpu().numpy().view(np.uint64)


def _check_dev(vc, store, name, ids, radius, mode, id_flags, cap=None):
    offs, flat, _ = R.expect_batch(name, ids, radius, id_flags)
    T = len(flat)
    rc, o, out = _dev(store, ids, radius, mode, id_flags, T if cap is None else cap)
    assert rc == vc.VC_OK, (name, radius, mode, id_flags, len(ids))
    assert np.array_equal(o, offs), (name, radius, mode, id_flags, len(ids))
    assert np.array_equal(out[:T], flat), (name, radius, mode, id_flags, len(ids))
    assert np.all(out[T:] == np.uint64(SENTINEL))                                  # nothing behind the total
    return out[:T]


def _check_host(vc, store, name, ids, radius, mode, id_flags):
    _, _, segs = R.expect_batch(name, ids, radius, id_flags)
    got = store.search_radius_ids(ids, radius, mode=mode, id_flags=id_flags, cap_per_query=8)      # (small: most batches retry once)
    assert len(got) == len(segs)
    for i, (g, e) in enumerate(zip(got, segs)):
        assert np.array_equal(g, e), (name, radius, mode, id_flags, len(ids), i)


def _radius_dev_on_codes(vc, store, name, ids, radius, mode):
    """vc_get_codes_dev + vc_search_radius_dev on the same ids: (found, offsets, flat) -- zero rows for the ids that are not resident"""
    import torch
    nq, nbytes = len(ids), I.SHAPES[name]["bits"] // 8
    d_ids = torch.from_numpy(np.ascontiguousarray(ids).view(np.int32)).cuda()
    d_codes = torch.zeros((nq, nbytes), dtype=torch.uint8, device="cuda")
    d_found = torch.zeros((nq,), dtype=torch.int32, device="cuda")
    store.get_codes_dev(d_ids.data_ptr(), nq, d_codes.data_ptr(), d_found.data_ptr())
    offs = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    rc = store.search_radius_dev(d_codes.data_ptr(), nq, radius, None, 0, offs.data_ptr(), mode=mode)
    torch.cuda.synchronize()
    total = int(offs[nq].item())
    out = torch.zeros(max(total, 1), dtype=torch.int64, device="cuda")
    assert store.search_radius_dev(d_codes.data_ptr(), nq, radius, out.data_ptr(), total, offs.data_ptr(), mode=mode) == vc.VC_OK
    torch.cuda.synchronize()
    return d_found.cpu().numpy().astype(bool), offs.cpu().numpy().view(np.uint64), out.cpu().numpy().view(np.uint64)[:total]


# ---- 1. one engine: every shape, radius, mode, flag set and list ----------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", I.SINGLE)
def test_single_engine(vc, stores, name, mode):
    store, m = stores(name), getattr(vc, "MODE_" + mode)
    for ids in _lists(name):
        for radius in R.RADII[name]:
            for id_flags in R.FLAG_SETS:
                got = _check_dev(vc, store, name, ids, radius, m, id_flags)
                _check_host(vc, store, name, ids, radius, m, id_flags)
                if id_flags == 0:      # bit for bit the segments of the call underneath on the gathered codes
                    found, uo, uflat = _radius_dev_on_codes(vc, store, name, ids, radius, m)
                    assert np.array_equal(found, I.resident(name, ids))
                    under = [uflat[int(uo[i]):int(uo[i + 1])] for i in np.flatnonzero(found)]
                    assert np.array_equal(got, np.concatenate(under) if under else np.zeros(0, dtype=np.uint64))


# ---- 2. chunk boundaries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_a_segment_across_several_chunks(vc, stores, mode):
    """S128 at R = 16: the longest segment of the list of 257 holds 2 540 entries -- three chunks of 1 024, the last one partly
    filled -- on its own, in the list, and as every query of a batch (all chunks full but every third)"""
    name, store, m = "S128", stores("S128"), getattr(vc, "MODE_" + mode)
    ids = I.id_list(name, 257)
    lens = np.array([len(R.expect(name, q, 16)) for q in ids])
    assert lens.max() == 2540
    longest = ids[int(lens.argmax())]
    for batch in (np.array([longest], dtype=np.uint32), np.array([longest, 0xFFFFFFFF, longest, longest], dtype=np.uint32), ids):
        for id_flags in R.FLAG_SETS:
            _check_dev(vc, store, name, batch, 16, m, id_flags)
            # room for the uncompacted total: the call does not wait for T, the result is the same
            raw = int(sum(len(R.expect(name, q, 16)) for q in batch))
            _check_dev(vc, store, name, batch, 16, m, id_flags, cap=raw)


# ---- 3. scan boundaries: every id of the store in one call ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_all_ids_list_every_pair_exactly_once(vc, stores, mode):
    """5 000 queries cross the tiles of 1 024 of both block-level scans; ONLY_GREATER over all resident ids lists every unordered
    pair within the radius exactly once"""
    name, store, m = "S128", stores("S128"), getattr(vc, "MODE_" + mode)
    n = I.SHAPES[name]["n"]
    ids = np.arange(n, dtype=np.uint32)
    for radius in (0, 2):
        want = R.brute_pairs(name, radius)
        rc, offs, out = _dev(store, ids, radius, m, vc.IDS_ONLY_GREATER, len(want))
        assert rc == vc.VC_OK and int(offs[n]) == len(want)
        lens = np.diff(offs.astype(np.int64))
        assert np.all(lens >= 0)
        flat = out[:len(want)]
        owner = np.repeat(ids.astype(np.uint64), lens)
        assert np.all((flat & R.LOW) > owner)
        same = owner[1:] == owner[:-1]
        assert np.all(flat[1:][same] > flat[:-1][same])                             # ascending packed inside every segment
        pairs = (owner << I.SH) | (flat & R.LOW)
        assert len(np.unique(pairs)) == len(pairs) and np.array_equal(np.sort(pairs), want)
        for q in (0, 1023, 1024, 2048, n - 1):                                      # and the segments themselves, around the tiles
            assert np.array_equal(flat[int(offs[q]):int(offs[q + 1])], R.expect(name, q, radius, vc.IDS_ONLY_GREATER))


# ---- 4. sharded ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", I.SHARDED)
def test_sharded(vc, stores, name, mode):
    """H3 and H8 hold S128's records: shard 7 of H8 is empty, 1999 | 2000 is a shard boundary inside GROUP7"""
    store, m = stores(name), getattr(vc, "MODE_" + mode)
    for ids in _lists(name):
        for radius in (0, 6, 16):
            for id_flags in R.FLAG_SETS:
                _check_dev(vc, store, name, ids, radius, m, id_flags)
                _check_host(vc, store, name, ids, radius, m, id_flags)
    base = I.SHAPES[name]["id_base"]
    group = np.array([base + p for p in I.GROUP7], dtype=np.uint32)
    got = store.search_radius_ids(group, 0, mode=m, id_flags=vc.IDS_ONLY_GREATER)
    assert [len(g) for g in got] == [6, 5, 4, 3, 2, 1, 0]                           # the group's pairs once, across the shards


# ---- 5. the capacity protocol -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S128", "H3"])
def test_capacity_protocol(vc, stores, name):
    store = stores(name)
    ids = I.id_list(name, 64)
    for mode in (vc.MODE_LINEAR, vc.MODE_MIH_EXACT):
        for id_flags in R.FLAG_SETS:
            offs, flat, _ = R.expect_batch(name, ids, 6, id_flags)
            T, raw = len(flat), len(R.expect_batch(name, ids, 6, 0)[1])
            assert T > 1
            _check_dev(vc, store, name, ids, 6, mode, id_flags, cap=T)              # out_cap = T: VC_OK
            rc, o, out = _dev(store, ids, 6, mode, id_flags, T - 1)                 # one short: the sizes, d_out untouched
            assert rc == vc.VC_ERR_CAPACITY and np.array_equal(o, offs) and np.all(out == np.uint64(SENTINEL))
            rc, o, out = _dev(store, ids, 6, mode, id_flags, 0, with_buffer=False)  # out_cap = 0 with d_out = NULL asks for the sizes
            assert rc == (vc.VC_ERR_CAPACITY if T else vc.VC_OK) and np.array_equal(o, offs)
            if id_flags:                                                            # between T and the uncompacted total
                assert T < raw
                _check_dev(vc, store, name, ids, 6, mode, id_flags, cap=(T + raw) // 2)
            # the host form: the same protocol on host buffers
            L = vc.load_library()
            fn = L.vc_sharded_search_radius_ids if I.SHAPES[name]["shards"] else L.vc_search_radius_ids
            ho = np.zeros(len(ids) + 1, dtype=np.uint64)
            hout = np.full(T, SENTINEL, dtype=np.uint64)
            p_ids = ids.ctypes.data_as(C.c_void_p)
            assert fn(store._h, p_ids, len(ids), 6, mode, id_flags, hout.ctypes.data_as(C.c_void_p), T - 1, ho.ctypes.data_as(C.c_void_p)) == vc.VC_ERR_CAPACITY
            assert np.array_equal(ho, offs) and np.all(hout == np.uint64(SENTINEL))
            ho[:] = 0
            assert fn(store._h, p_ids, len(ids), 6, mode, id_flags, None, 0, ho.ctypes.data_as(C.c_void_p)) == vc.VC_ERR_CAPACITY
            assert np.array_equal(ho, offs)
            assert fn(store._h, p_ids, len(ids), 6, mode, id_flags, hout.ctypes.data_as(C.c_void_p), T, ho.ctypes.data_as(C.c_void_p)) == vc.VC_OK
            assert np.array_equal(ho, offs) and np.array_equal(hout, flat)
    # a batch of ids that are all missing: T = 0, VC_OK also without a buffer
    gone = np.array([0xFFFFFFFF, 0xFFFFFFFF], dtype=np.uint32)
    rc, o, out = _dev(store, gone, 6, vc.MODE_LINEAR, 0, 0, with_buffer=False)
    assert rc == vc.VC_OK and np.all(o == 0)


# ---- 6. the argument contract -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S128", "H3"])
def test_argument_contract(vc, stores, name):
    import torch
    store, L = stores(name), vc.load_library()
    sharded = bool(I.SHAPES[name]["shards"])
    host = L.vc_sharded_search_radius_ids if sharded else L.vc_search_radius_ids
    devf = L.vc_sharded_search_radius_ids_dev if sharded else L.vc_search_radius_ids_dev
    ids = I.id_list(name, 64)
    out, offs = np.full(64, SENTINEL, dtype=np.uint64), np.zeros(65, dtype=np.uint64)
    p_ids, p_out, p_offs = (a.ctypes.data_as(C.c_void_p) for a in (ids, out, offs))
    t_ids = torch.from_numpy(ids.view(np.int32)).cuda()
    t_out = torch.full((64,), SENTINEL, dtype=torch.int64, device="cuda")
    t_offs = torch.zeros(65, dtype=torch.int64, device="cuda")
    d_ids, d_out, d_offs = t_ids.data_ptr(), t_out.data_ptr(), t_offs.data_ptr()
    INV, LIN = vc.VC_ERR_INVALID, vc.MODE_LINEAR
    for bad in (0x4, 0x80000000, 0x4 | vc.IDS_EXCLUDE_SELF):                        # unknown id_flags bits
        assert host(store._h, p_ids, 64, 3, LIN, bad, p_out, 64, p_offs) == INV
        assert devf(store._h, d_ids, 64, 3, LIN, bad, d_out, 64, d_offs, None) == INV
    for mode in (2, 3):                                                             # MIH_APPROX and an unknown mode
        assert host(store._h, p_ids, 64, 3, mode, 0, p_out, 64, p_offs) == INV
        assert devf(store._h, d_ids, 64, 3, mode, 0, d_out, 64, d_offs, None) == INV
    assert host(store._h, p_ids, 0, 3, LIN, 0, p_out, 64, p_offs) == INV             # nq = 0
    assert devf(store._h, d_ids, 0, 3, LIN, 0, d_out, 64, d_offs, None) == INV
    assert host(store._h, None, 64, 3, LIN, 0, p_out, 64, p_offs) == INV             # null pointers
    assert host(store._h, p_ids, 64, 3, LIN, 0, p_out, 64, None) == INV
    assert host(store._h, p_ids, 64, 3, LIN, 0, None, 64, p_offs) == INV
    assert host(None, p_ids, 64, 3, LIN, 0, p_out, 64, p_offs) == INV
    assert devf(store._h, None, 64, 3, LIN, 0, d_out, 64, d_offs, None) == INV
    assert devf(store._h, d_ids, 64, 3, LIN, 0, d_out, 64, None, None) == INV
    assert devf(store._h, d_ids, 64, 3, LIN, 0, None, 64, d_offs, None) == INV
    assert devf(None, d_ids, 64, 3, LIN, 0, d_out, 64, d_offs, None) == INV
    torch.cuda.synchronize()
    assert np.all(out == np.uint64(SENTINEL)) and bool((t_out == SENTINEL).all()) and bool((t_offs == 0).all())      # checked before any work
    # vc_search_knn_ids* keeps refusing the radius calls' bit
    knn = L.vc_sharded_search_knn_ids if sharded else L.vc_search_knn_ids
    rows = np.empty((64, 3), dtype=np.uint64)
    assert knn(store._h, p_ids, 64, 3, LIN, 0, vc.IDS_ONLY_GREATER, rows.ctypes.data_as(C.c_void_p), None, None) == INV
    # the handle answers correctly afterwards
    for id_flags in R.FLAG_SETS:
        _check_dev(vc, store, name, ids, 3, vc.MODE_MIH_EXACT, id_flags)


@pytest.mark.parametrize("name", ["S128", "H3"])
def test_mih_before_build_index_is_a_state_error(vc, name):
    ids = I.id_list(name, 64)
    with _make(vc, name, indexed=False) as store:
        with pytest.raises(vc.VcError) as ei:
            store.search_radius_ids(ids, 3, mode=vc.MODE_MIH_EXACT)
        assert ei.value.code == vc.VC_ERR_STATE
        with pytest.raises(vc.VcError) as ei:
            _dev(store, ids, 3, vc.MODE_MIH_EXACT, 0, 1 << 16)
        assert ei.value.code == vc.VC_ERR_STATE
        for id_flags in R.FLAG_SETS:                                                # LINEAR needs no index
            _check_dev(vc, store, name, ids, 3, vc.MODE_LINEAR, id_flags)
            _check_host(vc, store, name, ids, 3, vc.MODE_LINEAR, id_flags)
        store.build_index()
        _check_dev(vc, store, name, ids, 3, vc.MODE_MIH_EXACT, vc.IDS_ONLY_GREATER)


# ---- 7. history independence --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S128", "H3"])
def test_history_independence(vc, name):
    """the same batch before and after a larger by-id radius call, a k-NN by-id call and a host search_radius on the same handle:
    the scratch is the handle's own and every word of it is written before it is read -- identical bits"""
    ids = I.id_list(name, 64)
    codes = I.codes_of(name)
    with _make(vc, name) as store:
        def batch():
            res = []
            for mode in (vc.MODE_LINEAR, vc.MODE_MIH_EXACT):
                for id_flags in R.FLAG_SETS:
                    T = len(R.expect_batch(name, ids, 6, id_flags)[1])
                    rc, o, out = _dev(store, ids, 6, mode, id_flags, T)
                    assert rc == vc.VC_OK
                    res.append((o, out, store.search_radius_ids(ids, 6, mode=mode, id_flags=id_flags)))
            return res
        before = batch()
        big = I.id_list(name, 257)
        assert _dev(store, big, 16, vc.MODE_MIH_EXACT, 0, 600000)[0] == vc.VC_OK      # a larger by-id radius call: every scratch buffer regrows
        store.search_knn_ids(big, 100, mode=vc.MODE_LINEAR, id_flags=vc.IDS_EXCLUDE_SELF)
        store.search_radius(codes[1000:1040], 6, mode=vc.MODE_MIH_EXACT, cap_per_query=4096)
        after = batch()
        for b, a in zip(before, after):
            assert np.array_equal(b[0], a[0]) and np.array_equal(b[1], a[1])
            assert len(b[2]) == len(a[2]) and all(np.array_equal(x, y) for x, y in zip(b[2], a[2]))


# ---- 8. streams -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S128", "H3"])
def test_streams(vc, stores, name):
    """the device form on a torch side stream (two batches back to back, read after one stream synchronise) and on VC_STREAM_OWN"""
    import torch
    store = stores(name)
    a, b = I.id_list(name, 64), I.id_list(name, 257)
    for mode in (vc.MODE_LINEAR, vc.MODE_MIH_EXACT):
        for id_flags in (0, vc.IDS_ONLY_GREATER):
            exp = [R.expect_batch(name, ids, 6, id_flags) for ids in (a, b)]
            side = torch.cuda.Stream()
            bufs = []
            for ids, (offs, flat, _) in zip((a, b), exp):
                bufs.append((torch.from_numpy(ids.view(np.int32)).cuda(), torch.full((len(flat) + 1,), SENTINEL, dtype=torch.int64, device="cuda"),
                             torch.zeros(len(ids) + 1, dtype=torch.int64, device="cuda")))
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                for d_ids, out, offs in bufs:
                    assert store.search_radius_ids_dev(d_ids.data_ptr(), d_ids.numel(), 6, out.data_ptr(), out.numel() - 1, offs.data_ptr(), mode=mode,
                                                       id_flags=id_flags, stream=side.cuda_stream) == vc.VC_OK
            side.synchronize()
            for (offs, flat, _), (_, out, o) in zip(exp, bufs):
                assert np.array_equal(o.cpu().numpy().view(np.uint64), offs)
                assert np.array_equal(out.cpu().numpy().view(np.uint64)[:-1], flat) and int(out[-1].item()) == SENTINEL
            offs, flat, _ = exp[0]
            rc, o, out = _dev(store, a, 6, mode, id_flags, len(flat), stream=vc.STREAM_OWN)
            assert rc == vc.VC_OK and np.array_equal(o, offs) and np.array_equal(out[:-1], flat)


# ---- 9. two devices -------------------------------------------------------------------------------------------------------------------
def test_two_devices(vc):
    """H3 over devices 0 and 1: the ids and queries travel to the second device, its shards' results come back by peer copies.
    Skipped on a one-GPU box, as test_two_devices is elsewhere: it runs wherever two devices are visible."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (the cross-device leg of the sharded gather and radius search)")
    name = "H3"
    with _make(vc, name, devices=(0, 1)) as store:
        torch.cuda.set_device(store.root_device)
        for ids in (I.id_list(name, 257), R.edge_list(name)):
            for mode in (vc.MODE_LINEAR, vc.MODE_MIH_EXACT):
                for id_flags in R.FLAG_SETS:
                    _check_dev(vc, store, name, ids, 6, mode, id_flags)
                    _check_host(vc, store, name, ids, 6, mode, id_flags)


# ---- 10. the host C++ layer -----------------------------------------------------------------------------------------------------------
def test_image_search_client_within(vc, tmp_path):
    """image_search_client::search_image_by_id_within through a C++ caller on S128: a planted id (six twins at distance 0, the
    image itself left out by default), the same with VC_IDS_ONLY_GREATER, and an id that is not in the database"""
    name = "S128"
    s = I.SHAPES[name]
    (tmp_path / "lsh.code").write_bytes(I.codes_of(name).tobytes())
    exe = tmp_path / "radius_by_id_test"
    lib = os.path.join(ROOT, "verticut_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "radius_by_id_test.cc"),
                           "-I", os.path.join(ROOT, "verticut_amd", "host"), "-L", lib, "-lverticut_gpu",
                           "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib", "-L/opt/rocm/lib"])
    ids = [I.GROUP7[3], 4999, 77777]
    for id_flags in (vc.IDS_EXCLUDE_SELF, vc.IDS_ONLY_GREATER, 0):
        p = subprocess.run([str(exe), str(tmp_path / "lsh.code"), str(s["n"]), str(s["bits"]), str(s["m"]), "6", str(id_flags)] + [str(i) for i in ids],
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        lines = p.stdout.strip().splitlines()
        assert len(lines) == len(ids)
        for qid, line in zip(ids, lines):
            head, _, rest = line.partition(" :")
            assert head == "id %d" % qid
            got = [tuple(int(x) for x in pair.split(":")) for pair in rest.split()]
            exp = R.expect(name, qid, 6, id_flags)
            assert got == [(int(v & R.LOW), int(v >> I.SH)) for v in exp], (id_flags, qid)      # (image id, distance), nearest first
        assert lines[2] == "id 77777 :"                                             # not in the database: an empty list
    twins = [int(v & R.LOW) for v in R.expect(name, I.GROUP7[3], 0, vc.IDS_EXCLUDE_SELF)]
    assert twins == [p for p in I.GROUP7 if p != I.GROUP7[3]]
