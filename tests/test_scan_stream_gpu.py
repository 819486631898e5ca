"""GPU parity of the prefix-sorted scan stream (vc_build_scan_stream, vc_scan_kernel_stream): rows and counts of linear k-NN
bit for bit against brute force in numpy and against the same engine before the build -- every size at which the chunk, granule
or padding arithmetic changes, every small tile, data that stresses the header (clustered, equal keys), ring overflow with device
recovery, crafted records that pass the lower bound and must fail the exact check, tie order, routing, byte accounting,
invalidation, a refused build, and the sharded serving loop that turns the stream on.

k = N + 5 is run where the API admits it (k <= VC_MAX_K = 8192); beyond that the call is refused with VC_ERR_INVALID with and
without a stream, which is asserted instead."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INF = np.uint64(0xFFFFFFFFFFFFFFFF)
ID_BASE = 1000
MAX_K = 8192
SIZES = [1, 255, 256, 257, 2047, 2048, 2049, 100_003, 1 << 20]


def _popcount(x):
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(x)
    return np.unpackbits(x.view(np.uint8).reshape(x.shape + (8,)), axis=-1).sum(axis=-1)


def _packed_all(codes, q, id_base=ID_BASE):
    """[nq][N] packed dist << 32 | id of every record, unsorted"""
    c = np.ascontiguousarray(codes).view(np.uint64)          # [N][2]
    qq = np.ascontiguousarray(q).view(np.uint64)             # [nq][2]
    ids = np.arange(codes.shape[0], dtype=np.uint64) + np.uint64(id_base)
    out = np.empty((q.shape[0], codes.shape[0]), dtype=np.uint64)
    for i in range(q.shape[0]):
        d = _popcount(c[:, 0] ^ qq[i, 0]).astype(np.uint64) + _popcount(c[:, 1] ^ qq[i, 1]).astype(np.uint64)
        out[i] = (d << np.uint64(32)) | ids
    return out


def _sorted_rows(packed):
    """brute force once per data set: every row fully sorted, shared by all k and nq of the data set"""
    return np.sort(packed, axis=1)


def _expect(srt, nq, k):
    n = srt.shape[1]
    out = np.full((nq, k), INF, dtype=np.uint64)
    out[:, : min(k, n)] = srt[:nq, : min(k, n)]
    return out, np.full(nq, min(k, n), dtype=np.uint32)


def _ks(n):
    return [1, 100, n + 5]


def _uniform(n, rng):
    return rng.integers(0, 256, size=(n, 16), dtype=np.uint8)


def _clustered(n, rng):
    centres = rng.integers(0, 256, size=(max(n // 500, 1), 16), dtype=np.uint8)
    c = centres[rng.integers(0, centres.shape[0], size=n)].copy()
    rows = np.arange(n)
    for _ in range(6):                                   # up to 6 flipped bits per record
        b = rng.integers(0, 128, size=n)
        on = rng.integers(0, 2, size=n).astype(np.uint8)
        c[rows, b // 8] ^= (on << (b % 8).astype(np.uint8)).astype(np.uint8)
    return c


def _equal_keys(n, rng):
    c = _uniform(n, rng)
    c[:, :4] = np.frombuffer(np.uint32(0xC0FFEE42).tobytes(), dtype=np.uint8)   # bytes 0..3 are the key: full mask everywhere
    return c


def _queries(codes, rng, nq=8):
    """half near-duplicates of records (one of them exact), half uniform"""
    q = rng.integers(0, 256, size=(nq, 16), dtype=np.uint8)
    for i in range(0, nq, 2):
        q[i] = codes[rng.integers(0, codes.shape[0])]
        for b in rng.integers(0, 128, size=i):
            q[i, b // 8] ^= np.uint8(1 << (b % 8))
    return q


def _check_all_tiles(vc, e, codes, q, ks, stream):
    """nq = 1..8 x ks against brute force; returns the rows for the before / after comparison"""
    srt = _sorted_rows(_packed_all(codes, q))
    got_all = {}
    for k in ks:
        if k > MAX_K:
            with pytest.raises(vc.VcError) as ex:
                e.search_knn(q[:1], k)
            assert ex.value.code == vc.VC_ERR_INVALID
            continue
        for nq in range(1, 9):
            before = e.scan_stream_info()["launches"]
            got, cnt = e.search_knn(q[:nq], k)
            exp, ecnt = _expect(srt, nq, k)
            assert np.array_equal(cnt, ecnt), (codes.shape[0], nq, k, stream)
            assert np.array_equal(got, exp), (codes.shape[0], nq, k, stream)
            after = e.scan_stream_info()["launches"]
            assert after == before + (1 if stream else 0), (nq, k, before, after)   # one tile of nq <= 8 queries: one stream launch
            got_all[(nq, k)] = got
    return got_all


def _before_and_after(vc, codes, q, ks, **engine_kw):
    with vc.Engine(128, capacity=codes.shape[0], id_base=ID_BASE, **engine_kw) as e:
        e.add_codes(codes)
        assert e.scan_stream_info()["built"] == 0
        plain = _check_all_tiles(vc, e, codes, q, ks, stream=False)
        e.build_scan_stream()
        info = e.scan_stream_info()
        n = codes.shape[0]
        n_pad = (n + 2047) // 2048 * 2048
        assert info["built"] == 1 and info["items"] == n and info["granules"] == n_pad // 256 and info["launches"] == 0
        assert info["bytes"] == 4 * (4 * ((n_pad + 8191) // 8192 * 8192) + n_pad + 2 * (n_pad // 256))
        streamed = _check_all_tiles(vc, e, codes, q, ks, stream=True)
        assert plain.keys() == streamed.keys()
        for key in plain:
            assert np.array_equal(plain[key], streamed[key]), key


@pytest.mark.parametrize("n", SIZES)
def test_uniform_every_size_tile_and_k(vc, n):
    rng = np.random.default_rng(n)
    codes = _uniform(n, rng)
    _before_and_after(vc, codes, _queries(codes, rng), _ks(n))


@pytest.mark.parametrize("n,blocks", [(3 * 2048, 1), (7 * 2048 - 5, 1), (7 * 2048 - 5, 2), (6 * 2048 + 1, 2)])
def test_one_block_walks_several_chunks(vc, n, blocks):
    """the persistent grid capped to one or two blocks: every exit of the chunk loop, both register buffers re-used, the parked
    prefetch cursor and the header prefetch of the next chunk, at a few thousand codes"""
    rng = np.random.default_rng(n + blocks)
    codes = _uniform(n, rng)
    _before_and_after(vc, codes, _queries(codes, rng), [1, 100], scan_blocks=blocks)


@pytest.mark.parametrize("n", [257, 2049, 100_003])
@pytest.mark.parametrize("make", [_clustered, _equal_keys], ids=["clustered", "equal_keys"])
def test_clustered_and_equal_keys(vc, make, n):
    rng = np.random.default_rng(7 * n + 1)
    codes = make(n, rng)
    _before_and_after(vc, codes, _queries(codes, rng), _ks(n))


@pytest.mark.parametrize("n", [2049, 100_003])
def test_identical_codes_overflow_the_ring_and_are_recovered_on_the_device(vc, n):
    """every record ties at distance 0..: the ring (cand_cap 256 -> 4 k entries at k = 100) overflows, the device recovery keeps the smallest ids"""
    rng = np.random.default_rng(n + 3)
    codes = np.repeat(_uniform(1, rng), n, axis=0)
    q = _queries(codes, rng)
    _before_and_after(vc, codes, q, [1, 100], cand_cap=256)
    with vc.Engine(128, capacity=n, id_base=ID_BASE, cand_cap=256) as e:
        e.add_codes(codes)
        e.build_scan_stream()
        got, cnt = e.search_knn(q[:8], 100)
        assert np.all(cnt == 100) and e.device_status() == 0
        assert np.array_equal(got[0] & np.uint64(0xFFFFFFFF), np.arange(100, dtype=np.uint64) + np.uint64(ID_BASE))


def _crafted(n, rng):
    """uniform records plus, for j = 1..32, a record whose 96 streamed bits equal the query's and whose key differs from the
    query's in its j LOWEST bits (bits no granule header of a few hundred granules knows): its lower bound is 0, its distance j.
    Distance 10 occurs three times (ids spread over the store), so at k = 11 the k-th distance is a tie that the id decides."""
    codes = _uniform(n, rng)
    q = rng.integers(0, 256, size=(8, 16), dtype=np.uint8)
    qkey = int(q[0, :4].copy().view(np.uint32)[0])
    js = list(range(1, 33)) + [10, 10]
    pos = sorted(int(p) for p in rng.choice(n, size=len(js), replace=False))
    order = rng.permutation(len(js))
    for p, j in zip(pos, (js[o] for o in order)):
        codes[p] = q[0]
        codes[p, :4] = np.frombuffer(np.uint32(qkey ^ ((1 << j) - 1) & 0xFFFFFFFF).tobytes(), dtype=np.uint8)
    return codes, q


@pytest.mark.parametrize("n", [2049, 100_003])
def test_bound_passes_and_the_exact_check_decides(vc, n):
    rng = np.random.default_rng(n + 17)
    codes, q = _crafted(n, rng)
    d0 = _packed_all(codes, q[:1])[0] >> np.uint64(32)
    assert sorted(d0[d0 <= 32].tolist()) == sorted(list(range(1, 33)) + [10, 10])    # the crafted records, nothing else that near
    # k = 9 / 10 / 11 / 12: the threshold settles at 9 and at the three-way tie at distance 10 (one, two, all three of them wanted)
    _before_and_after(vc, codes, q, [9, 10, 11, 12, 34, 100])
    with vc.Engine(128, capacity=n, id_base=ID_BASE) as e:
        e.add_codes(codes)
        e.build_scan_stream()
        got, _ = e.search_knn(q[:1], 11)
        tie_ids = np.sort(np.nonzero(d0 == 10)[0])
        assert [int(x >> np.uint64(32)) for x in got[0]] == list(range(1, 10)) + [10, 10]
        assert [int(x & np.uint64(0xFFFFFFFF)) - ID_BASE for x in got[0][9:]] == tie_ids[:2].tolist()   # the two LOWEST ids of the tie


def test_routing_and_byte_accounting(vc, monkeypatch):
    n = 100_003
    rng = np.random.default_rng(5)
    codes = _uniform(n, rng)
    n_pad = (n + 2047) // 2048 * 2048
    with vc.Engine(128, capacity=n, id_base=ID_BASE) as e:
        e.add_codes(codes)
        q = _queries(codes, rng, nq=9)
        e.timing()
        e.search_knn(q[:8], 10)
        t = e.timing()
        assert t.scan_launches == 1 and t.scan_bytes == n * 16                       # no stream: what it always reported
        e.build_scan_stream()
        e.search_knn(q[:8], 10)
        t = e.timing()
        assert t.scan_launches == 1 and t.scan_bytes == n_pad * 12 + (n_pad // 256) * 8
        assert e.scan_stream_info()["launches"] == 1
        got9, _ = e.search_knn(q, 10)                                                # nine queries in one tile: the store's columns
        t = e.timing()
        assert e.scan_stream_info()["launches"] == 1 and t.scan_launches == 1 and t.scan_bytes == n * 16
        srt = _sorted_rows(_packed_all(codes, q))
        assert np.array_equal(got9, _expect(srt, 9, 10)[0])
        # the calls that ride on the k-NN search keep the store's columns too
        e.search_knn_ids(np.array([ID_BASE + 5, ID_BASE + 77], dtype=np.uint32), 10)
        e.search_knn_filtered(q[:2], 10, np.ones(n, dtype=np.uint32))
        e.search_radius(q[:2], 20)
        assert e.scan_stream_info()["launches"] == 1
    with vc.Engine(128, capacity=n, id_base=ID_BASE, query_tile=8) as e:             # 9 queries as tiles of 8 + 1: both from the stream
        e.add_codes(codes)
        e.build_scan_stream()
        got, _ = e.search_knn(q, 10)
        assert e.scan_stream_info()["launches"] == 2
        assert np.array_equal(got, got9)
    for bits in (64, 256):
        with vc.Engine(bits, capacity=1000) as e:
            e.add_synthetic(1000, seed=3)
            with pytest.raises(vc.VcError) as ex:
                e.build_scan_stream()
            assert ex.value.code == vc.VC_ERR_INVALID
            e.search_knn(np.zeros((2, bits // 8), dtype=np.uint8), 5)
            assert e.scan_stream_info() == dict(built=0, items=0, granules=0, bytes=0, launches=0, bound_passes=0, exact_passes=0)
    # host-driven recovery (no device recovery, identical codes, a small ring): the search's own tile streams, its probes do not
    monkeypatch.setenv("VC_DEVICE_RECOVER", "0")
    same = np.repeat(_uniform(1, rng), 5000, axis=0)
    with vc.Engine(128, capacity=5000, id_base=ID_BASE, cand_cap=64) as e:
        e.add_codes(same)
        e.build_scan_stream()
        e.timing()
        got, cnt = e.search_knn(same[:1], 20)
        t = e.timing()
        assert np.all(cnt == 20) and np.array_equal(got[0] & np.uint64(0xFFFFFFFF), np.arange(20, dtype=np.uint64) + np.uint64(ID_BASE))
        assert t.scan_launches > 1 and e.scan_stream_info()["launches"] == 1


def test_a_change_of_the_store_drops_the_stream(vc):
    rng = np.random.default_rng(23)
    n0, n1 = 3000, 2500
    codes = _uniform(n0 + n1, rng)
    q = _queries(codes, rng)
    with vc.Engine(128, capacity=n0 + n1, id_base=ID_BASE) as e:
        e.add_codes(codes[:n0])
        e.build_scan_stream()
        assert e.scan_stream_info()["built"] == 1
        e.add_codes(codes[n0:])
        assert e.scan_stream_info()["built"] == 0                                    # dropped, and nothing rebuilds it unasked
        srt = _sorted_rows(_packed_all(codes, q))
        got, cnt = e.search_knn(q, 100)
        assert np.array_equal(got, _expect(srt, 8, 100)[0]) and e.scan_stream_info()["built"] == 0
        e.build_scan_stream()
        info = e.scan_stream_info()
        assert info["built"] == 1 and info["items"] == n0 + n1
        got, cnt = e.search_knn(q, 100)
        assert np.array_equal(got, _expect(srt, 8, 100)[0]) and e.scan_stream_info()["launches"] == 1
        e.build_scan_stream()                                                        # building again replaces it
        assert e.scan_stream_info()["launches"] == 0
        keep = np.ones(n0 + n1, dtype=np.uint32)
        keep[::3] = 0
        e.retain(keep)
        assert e.scan_stream_info()["built"] == 0
        kept = codes[keep != 0]
        got, cnt = e.search_knn(q, 100)
        assert np.array_equal(got, _expect(_sorted_rows(_packed_all(kept, q)), 8, 100)[0])
        e.build_scan_stream()
        got2, _ = e.search_knn(q, 100)
        assert np.array_equal(got2, got) and e.scan_stream_info()["launches"] == 1


def test_a_refused_build_leaves_the_engine_serving(vc, monkeypatch):
    monkeypatch.setenv("VC_SCAN_STREAM_FREE", "100000")       # the memory rule is told of 100 KB free: 55 KB do not hold 20 B x 20 000
    rng = np.random.default_rng(29)
    codes = _uniform(20_000, rng)
    q = _queries(codes, rng)
    with vc.Engine(128, capacity=20_000, id_base=ID_BASE) as e:
        e.add_codes(codes)
        with pytest.raises(vc.VcError) as ex:
            e.build_scan_stream()
        assert ex.value.code == vc.VC_ERR_NOMEM
        assert e.scan_stream_info()["built"] == 0
        got, cnt = e.search_knn(q, 100)
        assert np.array_equal(got, _expect(_sorted_rows(_packed_all(codes, q)), 8, 100)[0])


@pytest.mark.parametrize("switch", ["1", "0"])
def test_sharded_search_turns_the_stream_on(vc, monkeypatch, switch):
    import torch
    from verticut_amd.sharded import ShardedSearch
    monkeypatch.setenv("VC_SCAN_STREAM", switch)
    rng = np.random.default_rng(31)
    n, k = 50_000, 100
    codes = _uniform(n, rng)
    q = _queries(codes, rng)
    srt = _sorted_rows(_packed_all(codes, q, id_base=0))
    ss = ShardedSearch(128, n, rank=0, world=1, device=0, query_tile=8)
    try:
        ss.add_codes_global(codes)
        assert ss.backend.engine.scan_stream_info()["built"] == 0
        dq = torch.from_numpy(q).cuda()
        for rep in range(2):
            rows, cnt = ss.search(dq, k)
            torch.cuda.synchronize()
            assert np.array_equal(rows.cpu().numpy().view(np.uint64), _expect(srt, 8, k)[0])
            assert np.all(cnt.cpu().numpy() == k)
            info = ss.backend.engine.scan_stream_info()
            assert info["built"] == int(switch) and info["launches"] == (rep + 1) * int(switch)
    finally:
        ss.close()
