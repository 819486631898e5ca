"""Shared by test_ids_cpu.py and test_ids_gpu.py (vc_get_codes_dev, vc_search_knn_ids*, vc_sharded_*_ids*): the shapes, their
data, the id lists and the engine-free expectations.

The new kernels (gather, strip, the sharded OR-merge) can only go wrong at edges, so the shapes are small: every code width
(W = 1, 2, 4, 8 words), an engine filled below its capacity, id ranges that start above zero, end at 2^32 or use the top bit,
shards that are partly filled or empty, ids missing on either side of the resident range, repeated ids, and two planted groups
of identical codes that put a query's own record first, in the middle, at the end of the k + 1 row, or not in it at all.

Clustered data with FEW centres on purpose: the approximate loop stops once 20 k candidates are seen, so k + 1 = 101 needs 2 020
records near the query (two clusters of 2 500) -- otherwise it walks shells of C(32, r) keys, which neither the oracle nor a
test of seconds can afford.  For the same reason the shapes without planted groups run k in {1, 6} only.
"""
import numpy as np

SH = np.uint64(32)
PACK_INF = np.uint64(0xFFFFFFFFFFFFFFFF)
LIST_LENGTHS = (1, 64, 257)
KS_GROUPS = (1, 6, 39, 100)          # against the groups of 7 and 40
KS_PLAIN = (1, 6)

# name: bits, m, n, capacity, id_base, centres, flips, shards (0 = one engine), ks
SHAPES = {
    "S64": dict(bits=64, m=2, n=3000, capacity=4096, id_base=1000, centres=4, flips=4, shards=0, ks=KS_PLAIN),
    "S128": dict(bits=128, m=4, n=5000, capacity=5000, id_base=0, centres=2, flips=8, shards=0, ks=KS_GROUPS),
    "S256": dict(bits=256, m=8, n=1500, capacity=2048, id_base=77, centres=3, flips=8, shards=0, ks=KS_PLAIN),
    # the capacity ends at 2^32: 0xFFFFFFFF is a legal id of this engine that is not resident
    "S512": dict(bits=512, m=16, n=1500, capacity=1600, id_base=2 ** 32 - 1600, centres=3, flips=8, shards=0, ks=KS_PLAIN),
    # S128's data over shards on one device: 3 x 2 000 ids (the last shard holds 1 000), 8 x 750 (shard 6 holds 500, shard 7 none)
    "H3": dict(bits=128, m=4, n=5000, capacity=6000, id_base=2 ** 31 + 5, centres=2, flips=8, shards=3, ks=KS_GROUPS),
    "H8": dict(bits=128, m=4, n=5000, capacity=6000, id_base=2 ** 31 + 5, centres=2, flips=8, shards=8, ks=KS_GROUPS),
}
SINGLE = ("S64", "S128", "S256", "S512")
SHARDED = ("H3", "H8")

# planted in the 128-bit data (positions = ids relative to id_base); 1999 | 2000 is a shard boundary of H3
GROUP7 = (37, 412, 1999, 2000, 3333, 4001, 4990)
GROUP40 = tuple(100 + 113 * i for i in range(40))
PLANTED_QUERIES = (GROUP7[0], GROUP7[3], GROUP7[6], GROUP40[0], GROUP40[20], GROUP40[39])

_POP = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint32)
_cache = {}


def codes_of(name):
    """the records of a shape, in id order (H3 / H8 share S128's)"""
    s = SHAPES[name]
    key = (s["bits"], s["n"], s["centres"], s["flips"])
    if key not in _cache:
        bits, n = s["bits"], s["n"]
        rng = np.random.default_rng(bits * 1000 + n)
        centres = rng.integers(0, 256, size=(s["centres"], bits // 8), dtype=np.uint8)
        codes = centres[rng.integers(0, s["centres"], size=n)].copy()
        for i in range(n):
            for b in rng.choice(bits, size=int(rng.integers(0, s["flips"] + 1)), replace=False):
                codes[i, b // 8] ^= np.uint8(1 << (b % 8))
        if bits == 128:
            for group, seed in ((GROUP7, 7), (GROUP40, 40)):     # a member of cluster 0 / 1 with a flip pattern of its own
                c = centres[seed % 2].copy()
                for b in np.random.default_rng(seed).choice(bits, size=s["flips"], replace=False):
                    c[b // 8] ^= np.uint8(1 << (b % 8))
                codes[list(group)] = c
        codes.setflags(write=False)
        _cache[key] = codes
    return _cache[key]


def shard_bounds(name):
    """[lo, hi) of the resident records of every shard, relative to id_base (one engine: one range)"""
    s = SHAPES[name]
    g, cap, n = max(s["shards"], 1), s["capacity"], s["n"]
    return [(min(n, cap * i // g), min(n, cap * (i + 1) // g)) for i in range(g)]


def unflagged_approx_ks(name):
    """the k of a shape that MIH_APPROX can run WITHOUT VC_FLAG_GLOBAL_APPROX: a shard then stops at 20 (k + 1) candidates of its
    own, and one that holds fewer records than that never stops -- it walks all 2^32 keys of every 32-bit table.  So: the k for
    which the smallest non-empty shard holds 20 (k + 1) records of the query's cluster (an even share of the shard's records
    per centre; members of a cluster differ in at most 2 x flips bits, so their minimum substring distance is small).  One
    engine: every k of the shape."""
    s = SHAPES[name]
    if not s["shards"]:
        return s["ks"]
    smallest = min(hi - lo for lo, hi in shard_bounds(name) if hi > lo)
    return tuple(k for k in s["ks"] if 20 * (k + 1) <= smallest // s["centres"]) or s["ks"][:1]


def resident(name, ids):
    s = SHAPES[name]
    rel = np.asarray(ids, dtype=np.int64) - s["id_base"]
    return (rel >= 0) & (rel < s["n"])


def id_list(name, length):
    """uint32 ids: length 1 = the last resident id; 64 and 257 = the first and last id of every non-empty shard (or of the engine),
    one id below id_base (where there is one), one in [id_base + n, id_base + capacity) (where the capacity leaves room),
    0xFFFFFFFF, an id three times, the planted ids (128-bit data), then random ids -- one in eight of them not resident."""
    s = SHAPES[name]
    base, n, cap = s["id_base"], s["n"], s["capacity"]
    if length == 1:
        return np.array([base + n - 1], dtype=np.uint32)
    ids = []
    for lo, hi in shard_bounds(name):
        if hi > lo:
            ids += [base + lo, base + hi - 1]
    if base > 0:
        ids.append(base - 1)
    if cap > n:
        ids.append(base + n)
    ids.append(0xFFFFFFFF)
    ids += [base + n // 3] * 3
    if s["bits"] == 128:
        ids += [base + p for p in PLANTED_QUERIES]
    assert len(ids) <= 64
    rng = np.random.default_rng(length + n)
    while len(ids) < length:
        if len(ids) % 8 == 7:
            ids.append(int(rng.integers(0, 2 ** 32)))            # (resident only by accident)
        else:
            ids.append(base + int(rng.integers(0, n)))
    return np.array(ids, dtype=np.uint32)


def distances(codes, q):
    """full Hamming distances of every record to q (byte table; the GPU tests use oracle.np_distances instead)"""
    return _POP[np.bitwise_xor(codes, q[None, :])].sum(axis=1, dtype=np.uint32)


def pack(dist, ids):
    return (dist.astype(np.uint64) << SH) | ids.astype(np.uint64)


def brute_row(dist_fn, codes, id_base, qid, k, exclude_self):
    """the k smallest (dist, id) over ALL records -- all records but the query's own when exclude_self -- for the record with
    global id qid; None when qid is not resident.  Engine-free: distances and a sort."""
    pos = int(qid) - id_base
    if not 0 <= pos < len(codes):
        return None
    ids = np.arange(len(codes), dtype=np.uint64) + np.uint64(id_base)
    d = dist_fn(codes, codes[pos])
    if exclude_self:
        keep = ids != np.uint64(qid)
        d, ids = d[keep], ids[keep]
    return np.sort(pack(d, ids))[:k]


def strip_row(row, qid, k):
    """the contract of VC_IDS_EXCLUDE_SELF on the host: `row` (ascending, k + 1 entries at most) without the entry (0, qid),
    cut to k"""
    row = np.asarray(row, dtype=np.uint64)
    return row[row != np.uint64(qid)][:k]


def self_position(name, qid, k):
    """where the query's own record sits in its k + 1 row: 'first', 'mid', 'last', or 'absent'"""
    s = SHAPES[name]
    row = brute_row(distances, codes_of(name), s["id_base"], qid, k + 1, False)
    at = np.flatnonzero(row == np.uint64(qid))
    if len(at) == 0:
        return "absent"
    return "first" if at[0] == 0 else ("last" if at[0] == len(row) - 1 else "mid")


def padded(row, k):
    out = np.full(k, PACK_INF, dtype=np.uint64)
    out[:len(row)] = row
    return out
