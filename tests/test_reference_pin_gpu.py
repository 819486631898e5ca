"""The device kernels against the reference's own golden vectors, with no oracle in between.

tests/golden/primitives.json and tests/golden/reference_sweep.npz were written from the reference's image_tools.h (Hamming
distance, rule a1; binaryToInt, rule a2) and bitmap.cc (rule a7).  test_oracle_cpu.py pins the CPU oracle to them; the
tests here pin what the GPU computes to the same values, so that a mistake the oracle and a kernel share (byte order,
sign extension, full-width popcounts, the bitmap's bit layout) cannot pass both suites.

Widths the engine cannot hold are left out: Hamming pairs of 3, 7, 12, 13 and 18 bytes (codes are 64/128/256/512 bits)
and binaryToInt substrings of 3 bytes (24 bits divides none of those widths).  Of a bitmap trace only the final state is
pinned: the device bitmap is built from the keys, not mutated, so the interleaved `gets` stay a CPU check.
"""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SH = np.uint64(32)
ID_BASE = 0xF0000000          # ids with the top bit set: a sign-extended or truncated id shows


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "primitives.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def sweep():
    with np.load(os.path.join(GOLDEN, "reference_sweep.npz")) as z:
        return {name: z[name] for name in z.files}


def _hex(h):
    return np.frombuffer(bytes.fromhex(h), dtype=np.uint8)


def _ham_pairs(golden, sweep, nb):
    """(a, b, dist) of every golden Hamming pair of nb bytes: primitives.json first, then the sweep"""
    cases = [c for c in golden["hamming"] if len(c["a"]) == 2 * nb]
    a = np.concatenate([np.stack([_hex(c["a"]) for c in cases]), sweep["ham_a_%d" % nb]])
    b = np.concatenate([np.stack([_hex(c["b"]) for c in cases]), sweep["ham_b_%d" % nb]])
    d = np.concatenate([np.array([c["dist"] for c in cases]), sweep["ham_d_%d" % nb]]).astype(np.int64)
    assert a.shape == b.shape == (len(d), nb) and 0 in d and 8 * nb in d   # the extremes are in the fixtures
    return np.ascontiguousarray(a), np.ascontiguousarray(b), d


def _pair_distances(rows, n, id_base):
    """rows[i] = packed results of query i over a database of n records: the distance reported for record i, and the
    check that every record comes back exactly once in ascending order"""
    out = np.empty(len(rows), dtype=np.int64)
    for i, r in enumerate(rows):
        r = np.asarray(r, dtype=np.uint64)
        assert len(r) == n and np.all(r[1:] > r[:-1]), i
        ids = (r & np.uint64(0xFFFFFFFF)).astype(np.int64) - id_base
        assert np.array_equal(np.sort(ids), np.arange(n)), i
        out[i] = int(r[np.flatnonzero(ids == i)[0]] >> SH)
    return out


@pytest.mark.parametrize("nb", [8, 16, 32, 64])
def test_hamming_distance_matches_golden(vc, golden, sweep, nb):
    """a1: the distance the device reports for (query a[i], record b[i]) is the reference's hamming(a[i], b[i]) -- linear
    k-NN (host and device-pointer API), linear radius, MIH-exact k-NN and MIH radius over 16-bit substrings, and three
    shards of one device; the fixtures hold distance 0 and distance = bits."""
    import torch
    a, b, dist = _ham_pairs(golden, sweep, nb)
    n, bits = len(dist), 8 * nb
    with vc.Engine(bits, capacity=n, n_tables=bits // 16, id_base=ID_BASE) as e:
        e.add_codes(b)
        out, cnt = e.search_knn(a, n)
        assert np.all(cnt == n)
        assert np.array_equal(_pair_distances(out, n, ID_BASE), dist)
        d_q = torch.from_numpy(a).cuda()
        d_out = torch.empty((n, n), dtype=torch.int64, device="cuda")
        d_cnt = torch.empty((n,), dtype=torch.int32, device="cuda")
        e.search_knn_dev(d_q.data_ptr(), n, n, d_out.data_ptr(), d_cnt.data_ptr())
        torch.cuda.synchronize()
        assert np.all(d_cnt.cpu().numpy() == n)
        assert np.array_equal(_pair_distances(d_out.cpu().numpy().view(np.uint64), n, ID_BASE), dist)
        assert np.array_equal(_pair_distances(e.search_radius(a, bits), n, ID_BASE), dist)
        e.build_index()
        out, cnt = e.search_knn(a, n, mode=vc.MODE_MIH_EXACT)
        assert np.all(cnt == n)
        assert np.array_equal(_pair_distances(out, n, ID_BASE), dist)
        rad = e.search_radius(a, bits, mode=vc.MODE_MIH_EXACT)
        assert np.array_equal(_pair_distances(rad, n, ID_BASE), dist)
    with vc.ShardedEngine(bits, capacity=n, n_shards=3, devices=[0], id_base=ID_BASE) as s:
        s.add_codes(b)
        out, cnt = s.search_knn(a, n)
        assert np.all(cnt == n)
        assert np.array_equal(_pair_distances(out, n, ID_BASE), dist)


@pytest.mark.parametrize("ln", [1, 2, 4])
def test_bucket_keys_match_golden_binary_to_int(vc, golden, sweep, ln):
    """a2: a record whose table-t substring holds the golden bytes sits in bucket binaryToInt(bytes) -- the golden value,
    sign extension included -- with VC_FLAG_REF_SIGNEXT_KEYS, and in bucket value & (2^s - 1) (never in the sign-extended
    one) without it.  Substrings of 8, 16 and 32 bits in 128-bit codes; every table, the last one included."""
    raw = [_hex(c["bytes"]) for c in golden["binary_to_int"] if len(c["bytes"]) == 2 * ln] + list(sweep["b2i_in_%d" % ln])
    val = [c["value"] for c in golden["binary_to_int"] if len(c["bytes"]) == 2 * ln] + [int(v) for v in sweep["b2i_out_%d" % ln]]
    raw, val = np.stack(raw).astype(np.uint8), np.array(val, dtype=np.uint64)
    n_cases, bits, s = len(val), 128, 8 * ln
    m = bits // s
    assert np.any(val >> np.uint64(s - 1) & np.uint64(1)) and np.any(val >> np.uint64(s - 1) & np.uint64(1) == 0)
    # record r, table t holds case (r + 5 t) mod n_cases, at bytes [t*ln, (t+1)*ln) -- the substring MihOracle.key reads
    case = (np.arange(n_cases)[:, None] + 5 * np.arange(m)[None, :]) % n_cases
    codes = raw[case].reshape(n_cases, bits // 8)
    mask = (1 << s) - 1
    for flags in (vc.FLAG_REF_SIGNEXT_KEYS, 0):
        with vc.Engine(bits, capacity=n_cases, n_tables=m, flags=flags, id_base=ID_BASE) as e:
            e.add_codes(codes)
            e.build_index()
            for t in range(m):
                golden_keys = val[case[:, t]]
                for v in np.unique(golden_keys):
                    v = int(v)
                    members = ID_BASE + np.flatnonzero(golden_keys == v)       # ascending: append order
                    key = v if flags else v & mask
                    got = e.get_bucket(t, key, with_codes=False)
                    assert got is not None and np.array_equal(got[0], members), (flags, t, hex(v))
                    assert e.bitmap_test(t, key) == 1, (flags, t, hex(v))
                    if v != v & mask:                     # top bit set, s < 32: the other mode's key names no bucket
                        other = v & mask if flags else v
                        assert e.get_bucket(t, other, with_codes=False) is None, (flags, t, hex(v))
                        assert e.bitmap_test(t, other) == 0, (flags, t, hex(v))


@pytest.mark.parametrize("idx", range(12))
def test_occupancy_bitmap_matches_golden_trace(vc, golden, idx):
    """a7: the final bitmap of a bitmap.cc trace, as a set of table-0 keys, is what the device builds -- byte for byte
    through vc_bitmap_read (LSB-first uint32 words), zero beyond the trace, and bit for bit through vc_bitmap_test."""
    tr = golden["bitmap"][idx]
    nbytes = tr["n_bytes"]
    raw = _hex(tr["raw"])
    assert len(raw) == nbytes
    keys = np.flatnonzero(np.unpackbits(raw, bitorder="little"))                # bit v = byte v/8, bit v%8
    assert len(keys)
    s = 8 if nbytes == 4 else 16                                                # a bitmap of 2^s >= 8 * n_bytes bits
    bits = 64
    codes = np.zeros((len(keys), bits // 8), dtype=np.uint8)
    codes[:, : s // 8] = keys.astype("<u2").view(np.uint8).reshape(-1, 2)[:, : s // 8]   # binaryToInt: low byte first
    with vc.Engine(bits, capacity=len(codes), n_tables=bits // s, flags=vc.FLAG_USE_BITMAP) as e:
        e.add_codes(codes)
        e.build_index()
        words = e.bitmap_read(0, 0, (1 << s) // 32)
        assert words[: nbytes // 4].view(np.uint8).tobytes().hex() == tr["raw"]
        assert not np.any(words[nbytes // 4:])
        expect = np.unpackbits(raw, bitorder="little")
        for v in range(8 * nbytes):
            assert e.bitmap_test(0, v) == expect[v], v
