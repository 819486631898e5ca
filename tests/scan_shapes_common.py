"""Shared by test_scan_shapes_cpu.py and test_scan_shapes_gpu.py: the compiled set of vc_scan_kernel, the four database
sizes that walk a block through its chunk loop, two kinds of seeded data per size and the brute-force expectation.
Nothing here touches the engine or the oracle: the CPU suite checks on exactly these inputs that the cases bite (which
chunk, pair slot, lane and pair half every expected row draws from), the GPU suite runs them.

Layout the verify kernel gives an ordinal i (vc_scan.hip): chunk = i // C with C = 2 * BLK * U; inside the chunk pair
slot u = r // (2 * BLK), lane (thread) = r % (2 * BLK) // 2, pair half = r % 2.  Block b of a grid of G walks the chunks
b, b + G, b + 2G, ...

Planted data.  The issue asks for every planted row to hold item n - 1 and a plant from every chunk, slot, half, lane 0
and lane BLK - 1.  One item cannot be near two queries that are far apart (its distances to the all-zero and the all-ones
code add up to B), and a short database has fewer first / last lanes than 13 queries would each need.  So the planted
queries form a cluster -- a base code and ten codes one bit away from it -- and the plants are near-duplicates of the
base: each is within 0..6 bits of every cluster query and so belongs to all eleven rows.  The all-zero and the all-ones
query carry a few plants of their own at free ordinals; their rows otherwise come from the uniform background.
"""
import functools

import numpy as np

PACK_INF = np.uint64(0xFFFFFFFFFFFFFFFF)
BITS = (64, 128, 256, 512)
SIZES = ("short", "long", "solo", "wide")
KINDS = ("planted", "dense")
NQ = 15                          # queries per data set; the general form uses the first 13, the small form 8..15
N_CLUSTER = NQ - 2               # queries 2..: the base code and codes one bit away; 0 = all-zero, 1 = all-ones
K_PLANTED = (1, 100)
K_DENSE = 37
MAX_N = 28672
DENSE_CENTRES = 5
SEED = 20261


def general_shapes():
    """(bits, U, BLK, NB) of every vc_scan_kernel<W, U, BLK, NB> that launch_scan_w instantiates: U * W <= 8"""
    return [(bits, u, blk, nb) for bits in BITS for u in (1, 2, 4) if u * (bits // 64) <= 8
            for blk in (256, 512) for nb in (1, 2, 3)]


def small_unroll(bits):
    """UD of the small-tile form vc_scan_kernel<W, UD, 256, 2, QT, MW>"""
    w = bits // 64
    return 4 if w <= 2 else (2 if w <= 4 else 1)


def small_forms():
    return [(bits, qt) for bits in BITS for qt in range(1, 9)]


class Size(tuple):
    """(name, n, scan_blocks, capacity, id_base, chunk)"""
    __slots__ = ()
    name = property(lambda s: s[0])
    n = property(lambda s: s[1])
    scan_blocks = property(lambda s: s[2])
    capacity = property(lambda s: s[3])
    id_base = property(lambda s: s[4])
    chunk = property(lambda s: s[5])

    @property
    def nchunks(self):
        return -(-self.n // self.chunk)

    def grid(self, resident=1 << 30):
        """blocks launched: the request (0 = every resident block), never more than chunks"""
        return min(self.nchunks, self.scan_blocks or resident)

    def chunks_per_block(self):
        g = self.grid()
        return [len(range(b, self.nchunks, g)) for b in range(g)]


def size(name, u, blk):
    c = 2 * blk * u
    if name == "short":
        return Size((name, 2 * c + 1, 2, 2 * c + 1, 0xFFFF0000, c))
    if name == "wide":
        return Size((name, 2 * c + 1, 0, 2 * c + 1, 0, c))
    n = 6 * c + c - 1
    return Size((name, n, 2 if name == "long" else 1, n + 5000, 0, c))


def locate(i, u, blk):
    """ordinal -> (chunk, pair slot, lane, pair half)"""
    c = 2 * blk * u
    r = i % c
    return i // c, r // (2 * blk), r % (2 * blk) // 2, r % 2


def ordinal(chunk, slot, lane, half, u, blk):
    return chunk * 2 * blk * u + slot * 2 * blk + 2 * lane + half


def _flipped(code, positions):
    out = code.copy()
    for b in positions:
        out[b // 8] ^= np.uint8(1 << (b % 8))
    return out


class Data:
    """codes [n, bits/8] uint8, queries [NQ, bits/8] uint8, plants {ordinal: flips from the base code} (planted kind)"""

    def __init__(self, codes, queries, plants=None, ties=None):
        self.codes, self.queries, self.plants, self.ties = codes, queries, plants or {}, ties or []
        self.codes.setflags(write=False)
        self.queries.setflags(write=False)


def _planted(bits, u, blk, n, seed):
    rng = np.random.default_rng(seed)
    nb = bits // 8
    c = 2 * blk * u
    nchunks = -(-n // c)
    codes = rng.integers(0, 256, size=(n, nb), dtype=np.uint8)          # background: distances near bits / 2
    base = rng.integers(0, 256, size=nb, dtype=np.uint8)
    qbits = rng.choice(bits, size=N_CLUSTER - 1, replace=False)         # query 2 is the base, 3.. are one bit away
    queries = np.zeros((NQ, nb), dtype=np.uint8)
    queries[1] = 0xFF
    queries[2] = base
    for i in range(N_CLUSTER - 1):
        queries[3 + i] = _flipped(base, [qbits[i]])

    other = np.setdiff1d(np.arange(bits), qbits)                        # plants leave the queries' own bits alone: a plant d bits
    plants = {}                                                         # from the base is d + 1 bits from queries 3..

    def plant(i, d):
        if i < n and i not in plants:
            plants[i] = d
            codes[i] = _flipped(base, rng.choice(other, size=d, replace=False))

    plant(n - 1, 1)
    for ch in range(nchunks):
        plant(ch * c, 1 + ch % 5)                                       # the chunk's first and last item
        plant(ch * c + c - 1, 1 + (ch + 2) % 5)
        for s in range(u):                                              # lane 0 and lane BLK - 1 of every slot, in opposite
            for li, lane in enumerate((0, blk - 1)):                    # halves that swap from slot to slot and chunk to chunk
                plant(ordinal(ch, s, lane, (ch + s + li) % 2, u, blk), 1 + (3 * ch + s + 2 * li) % 5)
        # one more at an offset that no other chunk uses: stale registers of the previous chunk miss it
        plant(ordinal(ch, ch % u, 1 + (37 * ch + 11) % (blk - 2), (ch // u) % 2, u, blk), 1 + ch % 5)
    assert len(plants) + NQ < 100                                       # every plant fits every cluster row of 100

    taken = set(plants)

    def free_in_chunk(ch, start):
        lo, hi = ch * c, min(n, (ch + 1) * c)
        i = lo + start % (hi - lo)
        while i in taken:
            i = lo + (i - lo + 3) % (hi - lo)
        taken.add(i)
        return i

    roomy = [ch for ch in range(nchunks) if min(n, (ch + 1) * c) - ch * c >= 64]
    exact = {}
    for q in range(NQ):                                                 # an exact duplicate per query: the k = 1 answer
        ch = roomy[q % len(roomy)]
        i = free_in_chunk(ch, 977 * q + 131)
        codes[i] = queries[q]
        exact[q] = i
    for q in (0, 1):                                                    # near-duplicates of the two constant queries
        for d in (1, 2, 3):
            i = free_in_chunk(roomy[(q + d) % len(roomy)], 613 * d + 57 * q)
            codes[i] = _flipped(queries[q], rng.choice(bits, size=d, replace=False))
    # tie group: 7 bits from the base = 8 bits from the other cluster queries; more of them than a row of 100 has room for
    ties = []
    free = np.array([i for i in range(n) if i not in taken])
    for i in rng.choice(free, size=160, replace=False):
        codes[i] = _flipped(base, rng.choice(other, size=7, replace=False))
        ties.append(int(i))
    d = Data(codes, queries, plants, sorted(ties))
    d.exact = exact
    return d


def _dense(bits, n, seed):
    """a handful of centres, every item a centre with 1..3 flipped bits (five per centre with none): a third of a centre's
    items lie at or under the k-th distance of its query, so most waves of most chunks append"""
    rng = np.random.default_rng(seed)
    nb = bits // 8
    centres = rng.integers(0, 256, size=(DENSE_CENTRES, nb), dtype=np.uint8)
    which = rng.integers(0, DENSE_CENTRES, size=n)
    flips = rng.integers(1, 4, size=n)
    for ce in range(DENSE_CENTRES):
        flips[rng.choice(np.flatnonzero(which == ce), size=5, replace=False)] = 0
    codes = centres[which].copy()
    pos = rng.integers(0, bits, size=(n, 3))
    for _ in range(64):                                                 # three distinct bit positions per item
        bad = np.flatnonzero((pos[:, 0] == pos[:, 1]) | (pos[:, 0] == pos[:, 2]) | (pos[:, 1] == pos[:, 2]))
        if bad.size == 0:
            break
        pos[bad] = rng.integers(0, bits, size=(bad.size, 3))
    assert bad.size == 0
    for t in range(3):
        rows = np.flatnonzero(flips > t)
        codes[rows, pos[rows, t] // 8] ^= (1 << (pos[rows, t] % 8)).astype(np.uint8)
    queries = centres[np.arange(NQ) % DENSE_CENTRES].copy()
    return Data(codes, queries)


@functools.lru_cache(maxsize=None)
def data(bits, u, blk, size_name, kind):
    """the data set of a (shape, size, kind); short and wide share theirs (same n), long and solo too"""
    n = size(size_name, u, blk).n
    tag = 0 if size_name in ("short", "wide") else 1
    seed = SEED + 1000 * bits + 100 * u + blk + 7 * tag
    return _planted(bits, u, blk, n, seed) if kind == "planted" else _dense(bits, n, seed + 3)


def distances(codes, queries):
    """[nq, n] integer Hamming distances: popcount of the XOR over the whole code"""
    cw = np.ascontiguousarray(codes).view(np.uint64)
    qw = np.ascontiguousarray(queries).view(np.uint64)
    out = np.empty((qw.shape[0], cw.shape[0]), dtype=np.uint64)
    for q0 in range(0, qw.shape[0], 128):
        x = cw[None, :, :] ^ qw[q0:q0 + 128, None, :]
        if hasattr(np, "bitwise_count"):
            out[q0:q0 + 128] = np.bitwise_count(x).sum(axis=2, dtype=np.uint64)
        else:
            out[q0:q0 + 128] = np.unpackbits(x.view(np.uint8), axis=2).sum(axis=2, dtype=np.uint64)
    return out


def expect(codes, queries, k, id_base=0):
    """rows [nq, k] of dist << 32 | id_base + ordinal, ascending, PACK_INF behind counts[i] entries; counts [nq]"""
    n = codes.shape[0]
    packed = (distances(codes, queries) << np.uint64(32)) | (np.uint64(id_base) + np.arange(n, dtype=np.uint64))[None, :]
    packed.sort(axis=1)
    rows = np.full((packed.shape[0], k), PACK_INF, dtype=np.uint64)
    rows[:, :min(k, n)] = packed[:, :k]
    return rows, np.full(packed.shape[0], min(k, n), dtype=np.uint32)


def calls(kind):
    """(first query, nq, k) of the searches a general-form case makes on one engine: 13 queries = tiles of 11 and 2 under
    query_tile = 11, one query = the min(q + 1, last) edge of the query prefetch"""
    if kind == "planted":
        return [(0, 13, 1), (0, 13, 100), (2, 1, 100), (1, 1, 1)]
    return [(0, 13, K_DENSE), (3, 1, K_DENSE)]


def small_calls(kind):
    """the small-tile case's searches: 8 queries, then 9..15 = a full tile and a tail tile of QT = nq - 8"""
    if kind == "planted":
        return [(0, nq, K_PLANTED[nq % 2]) for nq in range(8, 16)]
    return [(0, nq, K_DENSE) for nq in range(8, 16)]


def large_tile_queries(d, bits, nq, seed):
    """nq queries for the large-tile cases: the data set's queries in turn, with 0..2 flipped bits"""
    rng = np.random.default_rng(seed)
    q = d.queries[np.arange(nq) % NQ].copy()
    for i in range(nq):
        for b in rng.choice(bits, size=(i // NQ) % 3, replace=False):
            q[i, b // 8] ^= np.uint8(1 << (b % 8))
    return q


def parse_trace(err):
    """the [scan shape] lines of a captured stderr as dicts of ints"""
    out = []
    for line in err.splitlines():
        if line.startswith("[scan shape] "):
            out.append({k: int(v) for k, v in (f.split("=") for f in line[len("[scan shape] "):].split())})
    return out
