"""GPU parity of the stream kernel's exact check (vc_scan_slow_stream in vc_scan.hip) where it is entered often and late:
every check compares rows and counts bit for bit with brute force in numpy and with the same engine before
build_scan_stream(), for tiles of 1..8 queries, with ID_BASE added to the ids.  The cases sit where a check that is deferred
and batched per wave (tried and measured in DESIGN 4.1.2; 64 entries per wave) has its edges, and hold for the inline check as
well: near records only in the ragged last chunk of a block's walk, 63 / 64 / 65 candidates of one wave over consecutive chunks
of one block, fires in which every record of a wave-load is a candidate and the ring overflows, near records of eight queries
interleaved in sorted order, and the clean hand-back of the state between two calls.

A wave of a 256-thread block owns granule w (sorted positions [256 w, 256 w + 256)) and granule 4 + w of every 2048-record
chunk; the crafted stores place their near records by key, and each test checks in numpy that they landed where it says."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INF = np.uint64(0xFFFFFFFFFFFFFFFF)
ID_BASE = 1000
N_RAGGED = 3 * 2048 + 17


def _popcount(x):
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(x)
    return np.unpackbits(x.view(np.uint8).reshape(x.shape + (8,)), axis=-1).sum(axis=-1)


def _sorted_rows(codes, q):
    """brute force once per data set: [nq][N] packed dist << 32 | id, every row sorted"""
    c = np.ascontiguousarray(codes).view(np.uint64)
    qq = np.ascontiguousarray(q).view(np.uint64)
    ids = np.arange(codes.shape[0], dtype=np.uint64) + np.uint64(ID_BASE)
    out = np.empty((q.shape[0], codes.shape[0]), dtype=np.uint64)
    for i in range(q.shape[0]):
        d = _popcount(c[:, 0] ^ qq[i, 0]).astype(np.uint64) + _popcount(c[:, 1] ^ qq[i, 1]).astype(np.uint64)
        out[i] = (d << np.uint64(32)) | ids
    return np.sort(out, axis=1)


def _expect(srt, nq, k):
    n = srt.shape[1]
    out = np.full((nq, k), INF, dtype=np.uint64)
    out[:, : min(k, n)] = srt[:nq, : min(k, n)]
    return out, np.full(nq, min(k, n), dtype=np.uint32)


def _all_tiles(e, srt, q, ks, stream):
    got_all = {}
    for k in ks:
        for nq in range(1, 9):
            before = e.scan_stream_info()["launches"]
            got, cnt = e.search_knn(q[:nq], k)
            exp, ecnt = _expect(srt, nq, k)
            assert np.array_equal(cnt, ecnt), (nq, k, stream)
            assert np.array_equal(got, exp), (nq, k, stream)
            assert e.scan_stream_info()["launches"] == before + (1 if stream else 0), (nq, k)
            got_all[(nq, k)] = got
    return got_all


def _before_and_after(vc, codes, q, ks, **engine_kw):
    srt = _sorted_rows(codes, q)
    with vc.Engine(128, capacity=codes.shape[0], id_base=ID_BASE, **engine_kw) as e:
        e.add_codes(codes)
        plain = _all_tiles(e, srt, q, ks, stream=False)
        e.build_scan_stream()
        assert e.scan_stream_info()["built"] == 1
        streamed = _all_tiles(e, srt, q, ks, stream=True)
        for key in plain:
            assert np.array_equal(plain[key], streamed[key]), key
        assert e.device_status() == 0


def _keys(codes):
    return np.ascontiguousarray(codes[:, :4]).view(np.uint32)[:, 0]


def _set_key(rec, key):
    rec[:4] = np.frombuffer(np.uint32(key & 0xFFFFFFFF).tobytes(), dtype=np.uint8)


def _sorted_pos(codes):
    """sorted position of every record; the tests keep all keys distinct, so the order does not depend on the sort's tie rule"""
    keys = _keys(codes)
    assert np.unique(keys).size == keys.size
    pos = np.empty(keys.size, dtype=np.int64)
    pos[np.argsort(keys, kind="stable")] = np.arange(keys.size)
    return pos


def _spread_background(n, rng, shift):
    """uniform records whose keys are spread evenly: the i-th smallest key lies in [i * 2^shift + 128, (i + 1) * 2^shift), so a
    key's sorted position can be read off its value, and the 128 keys from i * 2^shift on are free for crafted records"""
    assert n << shift <= 1 << 32
    codes = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    keys = (np.arange(n, dtype=np.uint64) << np.uint64(shift)) + rng.integers(128, 1 << shift, size=n).astype(np.uint64)
    codes[:, :4] = keys.astype(np.uint32).view(np.uint8).reshape(n, 4)
    return codes[rng.permutation(n)]          # ids carry no order


def _flip_tail_bits(rec, nbits, rng):
    for b in rng.choice(96, size=nbits, replace=False):
        rec[4 + b // 8] ^= np.uint8(1 << (b % 8))


@pytest.mark.parametrize("k", [1, 100])
def test_near_records_only_in_the_ragged_last_chunk(vc, k):
    """Uniform codes, one block; the 17 records of the ragged fourth chunk (the largest keys) are the near records of the eight
    queries, two per query and three of the first: the exact check finds them in the last pass of the chunk loop, behind which
    nothing follows but the kernel's exit."""
    rng = np.random.default_rng(101)
    n = N_RAGGED
    codes = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    codes[:, 3] &= 0x7F                                        # background keys below 2^31
    q = rng.integers(0, 256, size=(8, 16), dtype=np.uint8)
    near = rng.choice(n, size=17, replace=False)
    for j, p in enumerate(near):
        i = j % 8
        _set_key(q[i], 0xFFFFFF00 + i)                         # the query's key and its records' keys: the top of the key range
        codes[p] = q[i]
        _set_key(codes[p], 0xFFFFFF00 + 8 * (j // 8 + 1) + i)  # distinct keys, one to two low bits off the query's
        _flip_tail_bits(codes[p], j // 8, rng)
    pos = _sorted_pos(codes)
    assert sorted(pos[near].tolist()) == list(range(3 * 2048, n))         # exactly the ragged chunk
    srt = _sorted_rows(codes, q)
    assert np.all((srt[:, :2] >> np.uint64(32)) <= 4) and np.all((srt[:, 3] >> np.uint64(32)) > 20)
    _before_and_after(vc, codes, q, [k], scan_blocks=1)


@pytest.mark.parametrize("second", [23, 24, 25])
def test_one_wave_meets_63_64_65_candidates_over_consecutive_chunks(vc, second):
    """One block, one query with 40 + second + 3 near records in wave 0's first granule of chunks 0, 1 and 2 and k = their
    number, so the bootstrap threshold (the whole store is its sample) admits exactly them: wave 0 has seen 40 candidates
    after chunk 0 and 63, 64 or 65 after chunk 1 -- one below, at and one above a wave's width -- before chunk 2 adds three.
    Those counts are exact for the one-query tile; the larger tiles add seven uniform queries with candidates of their own,
    and must give the same rows all the same."""
    rng = np.random.default_rng(200 + second)
    n = N_RAGGED
    counts = [40, second, 3]
    n_near = sum(counts)
    codes = _spread_background(n - n_near, rng, 19)
    q = rng.integers(0, 256, size=(8, 16), dtype=np.uint8)
    qlow = 0x15
    _set_key(q[0], qlow)
    # chunk c starts at the 2048 c-th background key, 2048 c * 2^19; the near records before it shift that by less than a
    # granule, and their own keys (low 6 bits varied) lie below every background key from there on
    bases = [0, 2048 << 19, 4096 << 19]
    near = np.repeat(q[:1], n_near, axis=0)
    j = 0
    for base, cnt in zip(bases, counts):
        for s in range(cnt):
            _set_key(near[j], base | (qlow ^ s))               # distance popcount(s) (+ 1 for the chunk's bit) <= 7
            j += 1
    codes = np.concatenate([codes, near])
    perm = rng.permutation(n)
    codes = codes[perm]
    is_near = perm >= n - n_near
    pos = _sorted_pos(codes)[is_near]
    chunk, wave = pos // 2048, (pos % 1024) // 256
    assert np.all(wave == 0) and np.all(pos % 2048 < 256)
    assert [int((chunk == c).sum()) for c in range(3)] == counts
    srt = _sorted_rows(codes, q)
    d0 = srt[0] >> np.uint64(32)
    assert d0[n_near - 1] <= 7 and d0[n_near] > 20             # the near records, nothing else that near
    _before_and_after(vc, codes, q, [n_near], scan_blocks=1)


@pytest.mark.parametrize("n,blocks", [(2049, 1), (2049, 2), (7 * 2048 - 5, 1), (7 * 2048 - 5, 2)])
def test_identical_codes_fill_every_wave_load_and_overflow_the_ring(vc, n, blocks):
    """every record passes every test: each wave-load holds 1024 candidates and the store n entries for a 256-entry ring; the
    device recovery keeps the lowest ids."""
    rng = np.random.default_rng(n + blocks)
    codes = np.repeat(rng.integers(0, 256, size=(1, 16), dtype=np.uint8), n, axis=0)
    q = rng.integers(0, 256, size=(8, 16), dtype=np.uint8)
    q[0] = codes[0]
    q[2] = codes[0]
    q[2, 7] ^= 0x11
    _before_and_after(vc, codes, q, [1, 100], cand_cap=256, scan_blocks=blocks)
    with vc.Engine(128, capacity=n, id_base=ID_BASE, cand_cap=256, scan_blocks=blocks) as e:
        e.add_codes(codes)
        e.build_scan_stream()
        got, cnt = e.search_knn(q, 100)
        assert np.all(cnt == 100) and e.device_status() == 0
        for i in range(8):
            assert np.array_equal(got[i] & np.uint64(0xFFFFFFFF), np.arange(100, dtype=np.uint64) + np.uint64(ID_BASE))


def _interleaved(n, rng):
    """Eight queries with 14 near records each at distances 1..12, 10, 10 (a three-way tie at distance 10).  Query i's key is
    KB + i and its s-th record's key KB + 8 s + i, so in sorted order the 112 records interleave query by query inside one
    stretch of 112 positions: neighbouring lanes of one wave-load hold survivors of all eight."""
    dist = list(range(1, 13)) + [10, 10]
    shift = 19 if n < 8000 else 15
    codes = _spread_background(n - 8 * len(dist), rng, shift)
    q = rng.integers(0, 256, size=(8, 16), dtype=np.uint8)
    kb = 700 << shift                                          # the 128 free keys in front of the 700th background key
    near = []
    for i in range(8):
        _set_key(q[i], kb + i)
        for s, d in enumerate(dist):
            rec = q[i].copy()
            _set_key(rec, kb + 8 * s + i)                      # key distance popcount(s) <= 3
            _flip_tail_bits(rec, d - bin(s).count("1"), rng)
            near.append(rec)
    codes = np.concatenate([codes, np.array(near, dtype=np.uint8)])
    return codes[rng.permutation(n)], q, dist, kb


@pytest.mark.parametrize("n,blocks", [(N_RAGGED, 1), (100_003, 0)])
def test_survivors_of_several_queries_interleave_in_one_wave_load(vc, n, blocks):
    rng = np.random.default_rng(n + 41)
    codes, q, dist, kb = _interleaved(n, rng)
    srt = _sorted_rows(codes, q)
    d = srt >> np.uint64(32)
    assert np.all(np.sort(d[:, :14], axis=1) == np.sort(np.array(dist))) and np.all(d[:, 14] > 14)   # per query: its own records, nothing else that near
    near_pos = np.sort(_sorted_pos(codes)[_keys(codes) >> np.uint32(7) == kb >> 7])
    assert near_pos.size == 112 and near_pos[0] == 700 and near_pos[-1] == 811      # one stretch of sorted positions: waves 2 and 3 of chunk 0
    # k = 9 / 10 / 11 / 12: the threshold settles at 9 and at the three-way tie at distance 10 (one, two, all three wanted)
    _before_and_after(vc, codes, q, [9, 10, 11, 12], **({"scan_blocks": blocks} if blocks else {}))


def test_two_consecutive_calls_give_equal_rows(vc):
    rng = np.random.default_rng(77)
    codes, q, _, _ = _interleaved(N_RAGGED, rng)
    srt = _sorted_rows(codes, q)
    with vc.Engine(128, capacity=codes.shape[0], id_base=ID_BASE, scan_blocks=1) as e:
        e.add_codes(codes)
        e.build_scan_stream()
        for k in (11, 100):
            first, c1 = e.search_knn(q, k)
            second, c2 = e.search_knn(q, k)
            assert np.array_equal(first, second) and np.array_equal(c1, c2)
            assert np.array_equal(first, _expect(srt, 8, k)[0])
        assert e.device_status() == 0 and e.scan_stream_info()["launches"] == 4
