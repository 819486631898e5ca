"""Shared by test_sharded_global_approx_cpu.py and test_sharded_global_approx_gpu.py (VC_FLAG_GLOBAL_APPROX): the data of
the clustered and the crafted cases, and the numpy model of the approximate rule.

The model is the order-independent reading of search_worker.cc:93-157 that test_oracle_cpu.py pins against MihOracle: the
loop stops after the first shell r in which the distinct items of shells 0..r -- the items whose minimum substring distance
is <= r -- reach 20 k, else after the last shell; the answer is the k smallest (dist, id) among them; table 0 issues
C(S, 0) + .. + C(S, r) gets.  It holds for masked keys (key_mode = 1) without the bitmap.  The CPU file checks it against
MihOracle wherever the oracle can afford the shells, and uses it for what the oracle cannot walk: a shard that holds fewer
than 20 k items near the query runs into shells of C(32, r) probes."""
import math

import numpy as np

FACTOR = 20                                   # APPROXIMATE_FACTOR, search_worker.h:14
SH = np.uint64(32)

CLUSTERED_SHAPES = ((128, 4), (64, 2), (256, 8), (64, 4))
CLUSTERED_SHARDS = (1, 3, 8)
CLUSTERED_KS = (1, 5)
CLUSTERED_N, CLUSTERED_ID_BASE, CLUSTERED_NQ = 20_000, 1234, 10


def near_queries(codes, rng, nq, flips):
    q = codes[rng.integers(0, codes.shape[0], size=nq)].copy()
    for i in range(nq):
        for b in rng.choice(codes.shape[1] * 8, size=int(rng.integers(0, flips + 1)), replace=False):
            q[i, b // 8] ^= np.uint8(1 << (b % 8))
    return q


def clustered_case(oracle, bits, m):
    """the codes and the near queries of the (bits, m) case, the same whatever the number of shards"""
    codes = oracle.gen_codes(CLUSTERED_N, bits, 7, kind=1, n_centres=60, max_flips=bits // 16)
    return codes, near_queries(codes, np.random.default_rng(bits * 10 + m), CLUSTERED_NQ, bits // 16)


def shard_bounds(capacity, n_shards, n):
    """[lo, hi) of the records every id-range shard holds when n records fill a store of this capacity in id order"""
    return [(min(n, capacity * g // n_shards), min(n, capacity * (g + 1) // n_shards)) for g in range(n_shards)]


class Approx:
    """what the approximate loop returns for one query over `codes`: radius, n_sub_reads, n_distinct, rows (ascending)"""

    def __init__(self, oracle, codes, q, k, m, id_base=0):
        S = codes.shape[1] * 8 // m
        if len(codes):
            minsub = oracle.np_sub_distances(codes, q, m).min(axis=1)
        else:
            minsub = np.zeros(0, dtype=np.uint32)
        cum = np.cumsum(np.bincount(minsub, minlength=S + 1))
        hit = np.flatnonzero(cum >= FACTOR * k)
        self.radius = int(hit[0]) if len(hit) else S
        self.n_distinct = int(cum[self.radius])
        self.n_sub_reads = sum(math.comb(S, r) for r in range(self.radius + 1))
        ids = np.flatnonzero(minsub <= self.radius)
        d = oracle.np_distances(codes[ids], q) if len(ids) else np.zeros(0, dtype=np.uint32)
        self.rows = np.sort(oracle.pack(d, ids.astype(np.uint64) + np.uint64(id_base)))[:k]
        self.cum = cum                        # cum[r]: distinct items of shells 0..r

    def stats(self):
        return (self.radius, self.n_sub_reads, self.n_distinct)

    def stop(self):
        """where the loop stopped and what it had seen: the statistics that tell two stop decisions apart"""
        return (self.radius, self.n_distinct)


class Unflagged:
    """the store without the flag: every shard runs the loop to its own stop; rows merged, the widest radius, summed reads and
    candidates (vc_sharded_stats_kernel).  Empty shards are never asked."""

    def __init__(self, oracle, codes, q, k, m, bounds, id_base=0):
        self.shards = [Approx(oracle, codes[lo:hi], q, k, m, id_base + lo) for lo, hi in bounds if hi > lo]
        self.radius = max(s.radius for s in self.shards)
        self.n_sub_reads = sum(s.n_sub_reads for s in self.shards)
        self.n_distinct = sum(s.n_distinct for s in self.shards)
        self.rows = np.sort(np.concatenate([s.rows for s in self.shards]))[:k]

    def stop(self):
        """(n_sub_reads is left out on purpose: summed over G shards it differs from the union's whatever the shards do)"""
        return (self.radius, self.n_distinct)


def canonical(oracle, codes, q, k, radius, m, id_base):
    """the k smallest (dist, id) among the items whose minimum substring distance is <= radius"""
    d = oracle.np_distances(codes, q)
    ids = np.nonzero(oracle.np_sub_distances(codes, q, m).min(axis=1) <= radius)[0]
    return np.sort(oracle.pack(d[ids], ids.astype(np.uint64) + np.uint64(id_base)))[:k]


# ---- crafted thresholds: 128 bit / 4 tables, 3 000 uniform filler codes in 3 shards of 1 000, the all-zero query, k = 2 -> the
# loop stops at 40 distinct candidates.  Planted items have chosen substring distances; the filler has no 32-bit substring
# within 3 bits of zero (asserted by the CPU file), so the counts of shells 0..3 are the planted ones.
CR_BITS, CR_M, CR_K, CR_N, CR_SHARDS, CR_ID_BASE = 128, 4, 2, 3000, 3, 100
CR_PER_SHARD = CR_N // CR_SHARDS
CR_STOP = FACTOR * CR_K
CR_CASES = [(r, hit, place) for r in (0, 1, 2, 3) for hit in (True, False) for place in ("one", "spread", "late")]
CR_BEST, CR_TIE = (0, 1, 1, 1), ((0, 2, 2, 2), (2, 0, 2, 2))   # shell-0 items: distance 3, and two at distance 6 = the k-th


def crafted_radius(r_star, hit):
    """hit: the count reaches exactly 40 in shell r_star; else 39 there, and shell r_star + 1 brings it beyond"""
    return r_star if hit else r_star + 1


def _subs(r, i):
    """i-th ordinary item of shell r: table i % 4 at distance r, the others 3..5 beyond it (full distance >= 4 r + 9 > 6)"""
    t = i % 4
    far = iter(r + 3 + (i + j) % 3 for j in range(3))
    return tuple(r if tt == t else next(far) for tt in range(4))


def _shard_of(place, i):
    """where the i-th planted item of the union's shells goes"""
    if place == "one":
        return 1
    if place == "spread":
        return i % 3                                       # at most 15 of the <= 45 planted items per shard
    return 0 if i % 3 != 2 else 1 + (i // 3) % 2           # "late": two thirds in shard 0 (< 40 up to the union's stop)


def crafted(r_star, hit, place):
    """(codes, planted) -- planted: [(position, substring distances)]; the tie pair are planted[1] and planted[2].
    Shells below r_star hold 5 items each, shell r_star the rest to 40 (hit) or 39; a miss adds 3 in shell r_star + 1.
    'late' adds 14 items to shard 0 in the shell behind the union's stop: with its share of the others shard 0 reaches 40
    by itself there, one shell later than the union."""
    quota = {r: 5 for r in range(r_star)}
    quota[r_star] = (CR_STOP if hit else CR_STOP - 1) - 5 * r_star
    if not hit:
        quota[r_star + 1] = 3
    items = []
    for r in sorted(quota):
        special = (CR_BEST,) + CR_TIE if r == 0 else ()
        items += list(special) + [_subs(r, i) for i in range(quota[r] - len(special))]
    fill = [0] * CR_SHARDS
    planted = []
    for i, subs in enumerate(items):
        g = _shard_of(place, i)
        planted.append((g * CR_PER_SHARD + 17 + 3 * fill[g], subs))
        fill[g] += 1
    if place == "late":
        behind = crafted_radius(r_star, hit) + 1
        assert fill[0] < CR_STOP <= fill[0] + 14
        for i in range(14):
            planted.append((17 + 3 * fill[0], _subs(behind, i)))
            fill[0] += 1
    nb, sb = CR_BITS // 8, CR_BITS // 8 // CR_M
    codes = np.random.default_rng(1000 + r_star).integers(0, 256, size=(CR_N, nb), dtype=np.uint8)
    for pos, subs in planted:
        c = np.zeros(nb, dtype=np.uint8)
        for t, b in enumerate(subs):
            word = np.zeros(sb * 8, dtype=np.uint8)
            word[:b] = 1
            c[t * sb:(t + 1) * sb] = np.packbits(word, bitorder="little")
        codes[pos] = c
    return codes, planted


def crafted_query():
    return np.zeros((1, CR_BITS // 8), dtype=np.uint8)
