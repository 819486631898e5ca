"""The expectation of vc_seed_centres*: a numpy model of the header's rule, engine-free, a plain-loop version of it for small inputs,
and the crafted inputs of test_seed_cpu.py (which pins what they reach) and test_seed_gpu.py (which compares every output word with
the model, bit for bit)."""
import functools

import numpy as np

import groups_common as GC

WIDTHS = GC.WIDTHS
FARTHEST, WEIGHTED = 0, 1
METHODS = (FARTHEST, WEIGHTED)
B = 1024                                      # VC_SEED_BLOCK_RECORDS of csrc/vc_seed_plan.hpp: records per block of the round kernel
PICK_TRIP = 256                               # VC_SEED_BLOCK: partials per trip of the pick kernel's loop
STALE = np.uint64(0xA5A5A5A5A5A5A5A5)         # what output buffers hold before a call
MASK = (1 << 64) - 1
_POP = np.array([bin(x).count("1") for x in range(256)], dtype=np.int64)


def draw(seed, t):
    """output number t (from 0) of SplitMix64 started at `seed`, by stepping the state as the header writes it"""
    x = seed & MASK
    for _ in range(t + 1):
        x = (x + 0x9E3779B97F4A7C15) & MASK
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        z ^= z >> 31
    return z


def dist_to(codes, code):
    """int64 [N]: Hamming distances of every record to one code"""
    return _POP[codes ^ code[None, :]].sum(axis=1)


def zero_stats():
    return {"cost": 0, "radius": 0, "n_zero_picks": 0}


def seed_model(codes, k, method, seed, id_base=0, trace=None):
    """(centres uint8 [k, bits / 8], picks uint64 [k], assign uint64 [N], stats) as the header's loop defines them.  trace: a list that
    gets one dict per decided pick -- the record, and how many records shared the maximum (farthest) or the block of 1024 records the
    running sum crossed the target in (weighted)"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    n = len(codes)
    centres, picks = np.zeros((k, codes.shape[1]), np.uint8), np.zeros(k, np.uint64)
    if n == 0:
        return centres, picks, np.zeros(0, np.uint64), zero_stats()
    best_d, best_i = np.full(n, 1 << 40, np.int64), np.zeros(n, np.int64)
    s, pick_dist, n_zero = draw(seed, 0) % n, 0, 0
    for t in range(k):
        centres[t] = codes[s]
        picks[t] = (id_base + s) | pick_dist << 32
        n_zero += t >= 1 and pick_dist == 0
        d = dist_to(codes, codes[s])
        lower = d < best_d                                    # strict: the earlier seed keeps a tie
        best_d[lower], best_i[lower] = d[lower], t
        if t == k - 1:
            break
        if method == FARTHEST:
            s = int(np.argmax(best_d))                        # the first maximum: the smallest i on a tie
            if trace is not None:
                trace.append({"record": s, "n_at_max": int(np.count_nonzero(best_d == best_d[s]))})
        else:
            total = int(best_d.sum())
            if total == 0:
                s = 0
            else:
                target = draw(seed, t + 1) % total
                s = int(np.searchsorted(np.cumsum(best_d), target, side="right"))    # the smallest i with cum[i] > target
            if trace is not None:
                trace.append({"record": s, "block": s // B, "total": total})
        pick_dist = int(best_d[s])
    assign = best_i.astype(np.uint64) | best_d.astype(np.uint64) << np.uint64(32)
    return centres, picks, assign, {"cost": int(best_d.sum()), "radius": int(best_d.max()), "n_zero_picks": int(n_zero)}


def seed_naive(codes, k, method, seed, id_base=0):
    """the same rule by plain loops, for small inputs: what seed_model is pinned against"""
    n = len(codes)
    rows = [[int(x) for x in r] for r in codes]
    hd = lambda a, b: sum(bin(x ^ y).count("1") for x, y in zip(a, b))
    best = [(None, None)] * n
    s, pick_dist, centres, picks, n_zero = draw(seed, 0) % n, 0, [], [], 0
    for t in range(k):
        centres.append(rows[s])
        picks.append((id_base + s) | pick_dist << 32)
        if t >= 1 and pick_dist == 0:
            n_zero += 1
        for i in range(n):
            d = hd(rows[i], rows[s])
            if best[i][0] is None or d < best[i][0]:
                best[i] = (d, t)
        if t == k - 1:
            break
        if method == FARTHEST:
            s = 0
            for i in range(n):
                if best[i][0] > best[s][0]:
                    s = i
        else:
            total = sum(b[0] for b in best)
            s = 0
            if total:
                target, run = draw(seed, t + 1) % total, 0
                for i in range(n):
                    run += best[i][0]
                    if run > target:
                        s = i
                        break
        pick_dist = best[s][0]
    return (np.array(centres, np.uint8).reshape(k, -1), np.array(picks, np.uint64), np.array([b[1] | b[0] << 32 for b in best], np.uint64),
            {"cost": sum(b[0] for b in best), "radius": max(b[0] for b in best), "n_zero_picks": n_zero})


def index_of(packed):
    return (packed & np.uint64(0xFFFFFFFF)).astype(np.int64)


def dist_of(packed):
    return (packed >> np.uint64(32)).astype(np.int64)


def same_run(got, want, what=None):
    """centres, picks, assign (None in `got`: not asked for) and the statistics, every word"""
    for name, g, w in zip(("centres", "picks", "assign"), got, want):
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, name)
    if got[3] is not None:
        assert {key: int(v) for key, v in got[3].items()} == want[3], (what, got[3], want[3])


# ---- the crafted inputs: what each is for is pinned in test_seed_cpu.py ---------------------------------------------------------------
CASES = (1, 2, 3, 4, 5)
EDGE_RECORDS = (0, B - 1, B, 2 * B - 1, 3 * B - 1, 3 * B)    # case 3: the ends of the blocks; 3 B is the lone record of the last block
EDGE_FLIPS = (3, 6, 1, 5, 2, 4)                              # their distances to the common code, over disjoint bits
EDGE_SEEDS = range(32)                                       # the weighted mode picks every planted record under at least one of these


def _set_bits(code, first, count):
    for b in range(first, first + count):
        code[b // 8] ^= np.uint8(1 << (b % 8))


@functools.lru_cache(maxsize=None)
def case_codes(number, bits):
    rng = np.random.default_rng(7000 + 10 * bits + number)
    nbytes = bits // 8
    if number == 1:      # ties: 16 codes at most, so every maximum and every running sum is shared by many records
        codes = np.tile(rng.integers(0, 256, size=nbytes, dtype=np.uint8), (4099, 1))
        codes[:, :2] = rng.integers(0, 4, size=(4099, 2), dtype=np.uint8)
    elif number == 2:    # exhaustion: 5 distinct codes, more seeds asked for than there are
        codes = GC.uniform_codes(5, bits, 7100 + bits)[rng.integers(0, 5, size=300)]
        codes[:5] = GC.uniform_codes(5, bits, 7100 + bits)            # (every one of the five occurs)
    elif number == 3:    # edges: one code everywhere but at the ends of the blocks
        codes = np.tile(rng.integers(0, 256, size=nbytes, dtype=np.uint8), (3 * B + 1, 1))
        at = 0
        for i, flips in zip(EDGE_RECORDS, EDGE_FLIPS):
            _set_bits(codes[i], at, flips)
            at += flips
    elif number == 4:    # K = N over distinct codes
        codes = GC.uniform_codes(50, bits, 7200 + bits)
        assert len(np.unique(codes, axis=0)) == 50
    elif number == 5:    # long scan: 257 blocks, so the pick kernel's loop over the partials takes a second trip
        codes = GC.uniform_codes(256 * B + 5, bits, 7300 + bits)
    else:
        raise ValueError(number)
    codes = np.ascontiguousarray(codes)
    codes.setflags(write=False)
    return codes


LONG_SCAN_SEEDS = {64: 62511, 128: 185752, 256: 96509, 512: 38008}     # what long_scan_seed finds; test_seed_cpu.py checks what they reach


@functools.lru_cache(maxsize=None)
def long_scan_seed(bits):
    """the smallest `seed` under which case 5's first weighted pick falls into the last block (number 256: five records).  The sum of
    the distances of all records to record s is, per bit, the count of records that differ from s there, so a candidate costs O(bits);
    the search still takes seconds, so its results are kept in LONG_SCAN_SEEDS."""
    if bits in LONG_SCAN_SEEDS:
        return LONG_SCAN_SEEDS[bits]
    codes = case_codes(5, bits)
    n = len(codes)
    ones = np.unpackbits(codes, axis=1, bitorder="little").sum(axis=0, dtype=np.int64)
    tail = codes[256 * B:]
    for seed in range(1 << 20):
        s = draw(seed, 0) % n
        sbits = np.unpackbits(codes[s], bitorder="little").astype(bool)
        total = int(np.where(sbits, n - ones, ones).sum())
        if draw(seed, 1) % total >= total - int(dist_to(tail, codes[s]).sum()):
            return seed
    raise AssertionError("no seed below 2^20 reaches the last block")


def case_k(number):
    return {1: 10, 2: 9, 3: 7, 4: 50, 5: 8}[number]


def case_seed(number, bits, method):
    """the `seed` of a case: case 3 wants a first record that is none of the planted ones, case 5 (weighted) the last block"""
    if number == 5 and method == WEIGHTED:
        return long_scan_seed(bits)
    if number == 3:
        n = 3 * B + 1
        return next(s for s in range(1, 100) if draw(s, 0) % n not in EDGE_RECORDS)
    return 11 * number


@functools.lru_cache(maxsize=None)
def case_expect(number, bits, method, id_base=0, seed=None):
    """(centres, picks, assign, stats, trace) of a case by the model"""
    trace = []
    seed = case_seed(number, bits, method) if seed is None else seed
    got = seed_model(case_codes(number, bits), case_k(number), method, seed, id_base, trace)
    for x in got[:3]:
        x.setflags(write=False)
    return got + (trace,)
