"""Nearest of K given codes on the device: vc_assign_nearest, vc_assign_nearest_dev and their vc_sharded_* forms.

The expectation is assign_common.py's numpy model of the header's contract (pinned against plain loops by test_assign_cpu.py).  Every
output word is an integer function of the codes, the centres and the range, so every comparison is exact equality, and the words of
an output buffer outside the range must keep what they held.  Everything runs on one device; N <= 8192."""
import ctypes as C

import numpy as np
import pytest

import assign_common as AC
import groups_common as GC

pytestmark = pytest.mark.gpu

N = 4097
KS = (1, 2, 63, 64, 65, 257, 1000)
KNOBS = [(None, None), (64, None), (None, 3), (64, 3), (1, 2)]     # (VC_ASSIGN_TILE, VC_ASSIGN_SLICES)


def _make(vc, monkeypatch, codes, tile=None, slices=None, id_base=0, shards=0, capacity=None, n_tables=0):
    """the knobs are read when the handle is created"""
    for name, value in (("VC_ASSIGN_TILE", tile), ("VC_ASSIGN_SLICES", slices)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))
    bits, capacity = codes.shape[1] * 8, capacity or max(len(codes), 1)
    if shards:
        e = vc.ShardedEngine(bits, capacity=capacity, n_shards=shards, devices=[0], id_base=id_base, n_tables=n_tables)
    else:
        e = vc.Engine(bits, capacity=capacity, id_base=id_base, n_tables=n_tables)
    if len(codes):
        e.add_codes(codes)
    return e


def _upload(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _buffer(n_words):
    return _upload(np.full(max(n_words, 1), AC.STALE, dtype=np.uint64))


def _read(buf):
    import torch
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(np.uint64)


def _dev(store, centres, first, count, pad=3, stream=None):
    """the device form into the middle of a stale-filled buffer: (the count words, the words around them)"""
    d_c, d_out = _upload(centres), _buffer(count + 2 * pad)
    store.assign_nearest_dev(d_c.data_ptr(), len(centres), first, count, d_out.data_ptr() + 8 * pad, stream=stream)
    raw = _read(d_out)
    return raw[pad:pad + count], np.r_[raw[:pad], raw[pad + count:]]


def _check_both_forms(store, centres, want, first=0, count=None, what=None):
    count = len(want) - first if count is None else count
    exp = want[first:first + count]
    got = store.assign_nearest(centres, first, count)
    assert got.dtype == np.uint64 and np.array_equal(got, exp), (what, "host form")
    got, around = _dev(store, centres, first, count)
    assert np.array_equal(got, exp), (what, "device form")
    assert np.all(around == AC.STALE), (what, "words outside the range")


# ---- 1. every width and every K against the model -------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", AC.WIDTHS)
def test_host_and_device_form_against_the_model(vc, monkeypatch, bits):
    """K from one centre to more than a tile of 512-bit centres holds (256), N = 4097: one record in the last block at every width"""
    codes = AC.assign_case(bits, N, KS[0])[0]
    with _make(vc, monkeypatch, codes) as store:
        for k in KS:
            centres = AC.assign_case(bits, N, k)[1]
            want = AC.assign_expect(bits, N, k)
            _check_both_forms(store, centres, want, what=(bits, k))
            _check_both_forms(store, centres, want, 5, N - 9, what=(bits, k, "inner range"))


# ---- 2. ranges ---------------------------------------------------------------------------------------------------------------------------
def test_ranges(vc, monkeypatch):
    bits, k = 128, 65
    codes, centres = AC.assign_case(bits, N, k)
    want = AC.assign_expect(bits, N, k)
    with _make(vc, monkeypatch, codes) as store:
        for first, count in ((0, 0), (0, 1), (N - 1, 1), (63, 130), (1, N - 1), (N, 0)):
            _check_both_forms(store, centres, want, first, count, what=(first, count))
        L, out = vc.load_library(), np.full(N + 1, AC.STALE, dtype=np.uint64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        for first, count in ((0, N + 1), (1, N), (N, 1), (N + 1, 0), (1 << 63, 1 << 63)):
            assert L.vc_assign_nearest(store._h, p(centres), k, first, count, p(out)) == vc.VC_ERR_INVALID, (first, count)
            d_c, d_out = _upload(centres), _buffer(N + 1)
            assert L.vc_assign_nearest_dev(store._h, d_c.data_ptr(), k, first, count, d_out.data_ptr(), None) == vc.VC_ERR_INVALID, (first, count)
            assert np.all(_read(d_out) == AC.STALE) and np.all(out == AC.STALE)


# ---- 3. the tile and slice paths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,slices", KNOBS)
@pytest.mark.parametrize("bits", AC.WIDTHS)
def test_tiles_and_slices(vc, monkeypatch, bits, tile, slices):
    """K = 257 at tiles of 64: five tiles, the last holds one centre -- the one a planted record equals; two identical centres in
    different tiles and different slices, nearest for planted records: the smaller index wins on every path.  K = 2 with three slices
    asked for: fewer centres than slices.  Every knob setting gives the model's words, hence the same ones."""
    codes, centres = AC.tie_case(bits)
    want = AC.assign_model(codes, centres)
    for i in AC.TIE_RECORDS:
        assert want[i] == np.uint64(AC.TIE_P | 1 << 32)
    assert want[AC.HIT_RECORD] == np.uint64(AC.HIT_CENTRE)
    with _make(vc, monkeypatch, codes, tile, slices) as store:
        _check_both_forms(store, centres, want, what=(bits, tile, slices))
        _check_both_forms(store, centres, want, 60, 2000, what=(bits, tile, slices, "range"))
        two = np.stack([centres[AC.TIE_Q], centres[AC.TIE_P]])             # equal again: index 0 wins everywhere they are nearest
        want2 = AC.assign_model(codes, two)
        assert np.all(AC.index_of(want2) == 0)
        _check_both_forms(store, two, want2, what=(bits, tile, slices, "K = 2"))
        _check_both_forms(store, centres[:1], AC.assign_model(codes, centres[:1]), what=(bits, tile, slices, "K = 1"))


# ---- 4. the path this call replaces ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [64, 128])
def test_equals_a_k1_linear_search_over_the_centres(vc, monkeypatch, bits):
    n, k = 2048, 300
    codes = GC.clustered_codes(n, bits, 500 + bits, centres=30, flips=4)
    centres = codes[np.random.default_rng(bits).choice(n, size=k, replace=False)]      # near-duplicates among them: ties of distance
    assert len(AC.tie_witnesses(codes, centres)) > 0
    with _make(vc, monkeypatch, codes) as store, vc.Engine(bits, capacity=k, id_base=0) as holder:
        holder.add_codes(centres)
        rows, counts = holder.search_knn(codes, 1, mode=vc.MODE_LINEAR)
        assert np.all(counts == 1)
        got = store.assign_nearest(centres)
        assert np.array_equal(got, rows[:, 0]) and np.array_equal(got, AC.assign_model(codes, centres))
        got, _ = _dev(store, centres, 0, n)
        assert np.array_equal(got, rows[:, 0])


# ---- 5. id_base and shards -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards,capacity", [(0, None), (2, 4099), (3, 4099), (3, 9000)])
def test_id_base_and_shards(vc, monkeypatch, shards, capacity):
    """capacity 4099: shard boundaries at 2049, or 1366 and 2732 -- no multiple of 64; capacity 9000 in three shards: the last is empty.
    Ranges inside one shard, across one boundary, across two; all equal to the model, hence to the single engine"""
    bits, k = 128, 257
    codes, centres = AC.assign_case(bits, N, k)
    want = AC.assign_expect(bits, N, k)
    with _make(vc, monkeypatch, codes, id_base=1000, shards=shards, capacity=capacity) as store:
        if shards:
            ranges = [store.shard_range(g) for g in range(shards)]
            assert all(r[0] % 64 and (r[0] - 1000) % 64 for r in ranges[1:]), ranges
        for first, count in ((0, N), (1000, 2500), (10, 100), (2040, 20), (1300, 1500), (N - 1, 1), (N, 0)):
            _check_both_forms(store, centres, want, first, count, what=(shards, capacity, first, count))


def test_sharded_knobs(vc, monkeypatch):
    codes, centres = AC.tie_case(64)
    want = AC.assign_model(codes, centres)
    with _make(vc, monkeypatch, codes, tile=64, slices=3, shards=3, capacity=4099) as store:
        _check_both_forms(store, centres, want, what="three shards, tiles of 64, three slices")


# ---- 6. streams and the handle's history -----------------------------------------------------------------------------------------------------
def test_two_calls_on_two_streams_without_a_wait_between(vc, monkeypatch):
    import torch
    bits = 64
    codes = AC.assign_case(bits, N, 257)[0]
    cen_a, cen_b = AC.assign_case(bits, N, 257)[1], AC.assign_case(bits, N, 1000)[1]
    with _make(vc, monkeypatch, codes, slices=3) as store:
        side = torch.cuda.Stream()
        d_a, d_b, out_a, out_b = _upload(cen_a), _upload(cen_b), _buffer(N), _buffer(N)
        for _ in range(3):
            store.assign_nearest_dev(d_a.data_ptr(), 257, 0, N, out_a.data_ptr(), stream=None)
            store.assign_nearest_dev(d_b.data_ptr(), 1000, 0, N, out_b.data_ptr(), stream=side.cuda_stream)
        assert np.array_equal(_read(out_a), AC.assign_expect(bits, N, 257)) and np.array_equal(_read(out_b), AC.assign_expect(bits, N, 1000))


def test_large_small_large_and_appended_records(vc, monkeypatch):
    """grow-only staging: a large K, a small one, the large one again -- every result unchanged; then records are appended and, with the
    index left stale, the new range assigns correctly and the old range's words are what they were"""
    bits, n_old = 64, 3000
    codes = AC.assign_case(bits, N, 1000)[0]
    with _make(vc, monkeypatch, codes[:n_old], capacity=N, n_tables=4) as store:
        store.build_index()
        for k in (1000, 2, 1000, 65):
            centres = AC.assign_case(bits, N, k)[1]
            assert np.array_equal(store.assign_nearest(centres), AC.assign_expect(bits, N, k)[:n_old]), k
        store.add_codes(codes[n_old:])
        centres, want = AC.assign_case(bits, N, 1000)[1], AC.assign_expect(bits, N, 1000)
        _check_both_forms(store, centres, want, n_old, N - n_old, what="the appended records")
        _check_both_forms(store, centres, want, what="everything, index stale")
        store.update_index()
        _check_both_forms(store, centres, want, what="index current again")


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [0, 2])
def test_errors_leave_the_output_untouched(vc, monkeypatch, shards):
    bits, n, k = 64, 300, 7
    codes, centres = AC.assign_case(bits, n, k)
    L = vc.load_library()
    fn, fn_dev = (L.vc_sharded_assign_nearest, L.vc_sharded_assign_nearest_dev) if shards else (L.vc_assign_nearest, L.vc_assign_nearest_dev)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    with _make(vc, monkeypatch, codes, shards=shards) as store:
        out, d_c, d_out = np.full(n, AC.STALE, dtype=np.uint64), _upload(centres), _buffer(n)
        bad = [(None, p(centres), k, 0, n, p(out)), (store._h, None, k, 0, n, p(out)), (store._h, p(centres), 0, 0, n, p(out)),
               (store._h, p(centres), k, 0, n + 1, p(out)), (store._h, p(centres), k, n, 1, p(out)), (store._h, p(centres), k, 0, n, None)]
        for args in bad:
            assert fn(*args) == vc.VC_ERR_INVALID, args
        bad_dev = [(None, d_c.data_ptr(), k, 0, n, d_out.data_ptr()), (store._h, None, k, 0, n, d_out.data_ptr()), (store._h, d_c.data_ptr(), 0, 0, n, d_out.data_ptr()),
                   (store._h, d_c.data_ptr(), k, 1, n, d_out.data_ptr()), (store._h, d_c.data_ptr(), k, 0, n, None)]
        for args in bad_dev:
            assert fn_dev(*args, None) == vc.VC_ERR_INVALID, args
        assert np.all(out == AC.STALE) and np.all(_read(d_out) == AC.STALE)
        assert fn(store._h, p(centres), k, 0, 0, None) == vc.VC_OK and fn(store._h, p(centres), k, n, 0, None) == vc.VC_OK      # count == 0: nothing to write
        assert fn_dev(store._h, d_c.data_ptr(), k, 5, 0, None, None) == vc.VC_OK
        assert np.array_equal(store.assign_nearest(centres), AC.assign_model(codes, centres))                                   # the handle still works
    empty = vc.ShardedEngine(bits, capacity=16, n_shards=2, devices=[0]) if shards else vc.Engine(bits, capacity=16)
    with empty:
        assert fn(empty._h, p(centres), k, 0, 0, None) == vc.VC_OK and fn(empty._h, p(centres), k, 0, 1, p(out)) == vc.VC_ERR_INVALID
        assert len(empty.assign_nearest(centres)) == 0
