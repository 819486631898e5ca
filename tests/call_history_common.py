"""Shared by test_call_history_cpu.py and test_call_history_gpu.py: the data sets, the pool of distinct queries, the
call alphabet and the three orders of one multiset of calls.  Everything is seeded: the CPU suite checks the properties
the GPU sequences rely on (the far batches really stop in shell 2 or later, the shuffled order really holds the named
adjacent pairs) on exactly the data and calls the GPU suite runs."""
import numpy as np

LINEAR, EXACT, APPROX = 0, 1, 2
POOL = 20                       # distinct queries per kind; a batch tiles them
KINDS = ("near", "far", "uniform")

# (bits, m) -> n, centres, max_flips: clusters of 2 000-3 000 items, so approximate mode (20 k candidates) stops in an early shell
SHAPES = {
    (128, 4): (48_000, 16, 4),
    (64, 2): (40_000, 16, 3),
    (64, 4): (40_000, 16, 3),
    (256, 8): (30_000, 12, 6),
    (64, 8): (30_000, 12, 3),
}
SEED = 41


def make_codes(vo, bits, m, n=None):
    nn, centres, flips = SHAPES[(bits, m)]
    return vo.gen_codes(n or nn, bits, SEED, kind=1, n_centres=centres, max_flips=flips)


def _flip(row, positions):
    for b in positions:
        row[b // 8] ^= np.uint8(1 << (b % 8))


def make_queries(codes, bits, m, seed=0):
    """[3 * POOL, bits/8]: POOL near-duplicates (0..2 flipped bits), POOL far queries (a database item with 2 or 3 flipped
    bits in EVERY substring: its own shells 0 and 1 are empty of it), POOL uniform-random ones."""
    rng = np.random.default_rng(1000 * bits + m + seed)
    s = bits // m
    n = codes.shape[0]
    near = codes[rng.integers(0, n, size=POOL)].copy()
    for i in range(POOL):
        _flip(near[i], rng.choice(bits, size=int(rng.integers(0, 3)), replace=False))
    far = codes[rng.integers(0, n, size=POOL)].copy()
    for i in range(POOL):
        for t in range(m):
            _flip(far[i], t * s + rng.choice(s, size=int(rng.integers(2, 4)), replace=False))
    uni = rng.integers(0, 256, size=(POOL, bits // 8), dtype=np.uint8)
    return np.concatenate([near, far, uni])


def batch_index(kind, nq, start):
    """indices into make_queries() of a batch of nq queries of one kind"""
    return KINDS.index(kind) * POOL + (start + np.arange(nq)) % POOL


class Call(tuple):
    """(form, mode, k, nq, order, stats, kind, stream, radius, start)
    form: knn | knn_dev | knn_dev_stats | radius | radius_dev | radius_dev_small (out_cap too small: VC_ERR_CAPACITY)
    stream: own | null | side | set_side (vc_set_stream(side), host form, back to VC_STREAM_OWN)"""
    __slots__ = ()
    form = property(lambda c: c[0])
    mode = property(lambda c: c[1])
    k = property(lambda c: c[2])
    nq = property(lambda c: c[3])
    order = property(lambda c: c[4])
    stats = property(lambda c: c[5])
    kind = property(lambda c: c[6])
    stream = property(lambda c: c[7])
    radius = property(lambda c: c[8])
    start = property(lambda c: c[9])

    @property
    def is_radius(self):
        return self.form.startswith("radius")

    @property
    def size(self):
        """what the scratch of the call grows with: nq * k (a radius search's tile is carved with k = 1)"""
        return self.nq * (1 if self.is_radius else self.k)


def knn(form, mode, k, nq, kind, stream="own", order=0, stats=True, start=0):
    return Call((form, mode, k, nq, order, stats, kind, stream, 0, start))


def rad(form, mode, radius, nq, kind, stream="own", start=0):
    return Call((form, mode, 0, nq, 0, False, kind, stream, radius, start))


K_VALUES = (1, 7, 100, 1000, 3500)
NQ_VALUES = (1, 5, 33, 700, 9000)
MAX_ROWS = 2_500_000            # nq * k of one call (20 MB of rows, every one of them compared)


def named_calls(m):
    """the calls the named adjacent pairs and the route evidence are made of"""
    return {
        "far": knn("knn", EXACT, 7, 700, "far"),                          # >= 64 far queries: group_hint -> 3
        "near": knn("knn", EXACT, 7, 700, "near", stats=False),
        "radius": rad("radius", EXACT, 8, 33, "near"),
        "knn_big": knn("knn", EXACT, 1000, 33, "near"),
        "lin": knn("knn", LINEAR, 100, 33, "uniform", order=1),
        "mih": knn("knn_dev_stats", EXACT, 100, 33, "near", stream="null"),
        "dev_side": knn("knn_dev", EXACT, 100, 700, "near", stream="side", stats=False),
        "host": knn("knn", APPROX, 7, 5, "near"),
        "tiles": knn("knn", EXACT, 100, 9000, "near"),                    # three launches under VC_MIH_QTILE=4096
        "switch": knn("knn", EXACT, 100, 700, "uniform"),                 # the cost model's switch to the verify kernel
        "lds": knn("knn_dev_stats", EXACT, 3500, 700, "near", stream="side"),   # out of the in-block route by its LDS request
        "cap": rad("radius_dev_small", EXACT, 8, 700, "near", stream="side"),
        "lin_big": knn("knn_dev_stats", LINEAR, 100, 9000, "near", stream="null"),
        "set_side": knn("knn", EXACT, 100, 33, "far", stream="set_side"),
        "rad_wide": rad("radius_dev", EXACT, 2 * m + 2, 700, "near", stream="null"),
        "rad_lin": rad("radius", LINEAR, 0, 700, "near", stream="set_side"),
        "one": knn("knn", EXACT, 1, 1, "uniform", order=1),
        "approx_dev": knn("knn_dev_stats", APPROX, 100, 33, "near", stream="side"),
    }


PAIRS = (("far", "near"), ("near", "far"), ("radius", "knn_big"), ("knn_big", "radius"), ("lin", "mih"), ("dev_side", "host"))


def drawn_calls(m, seed, count=10):
    """`count` more distinct calls drawn from the alphabet by a seeded generator"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        kind = KINDS[rng.integers(0, 3)]
        start = int(rng.integers(0, POOL))
        stream = ("own", "null", "side", "set_side")[rng.integers(0, 4)]
        if rng.integers(0, 3) == 0:                                        # a radius search
            form = "radius" if stream in ("own", "set_side") else "radius_dev"
            c = rad(form, (LINEAR, EXACT)[rng.integers(0, 2)], (0, 8, 2 * m + 2)[rng.integers(0, 3)],
                    int(NQ_VALUES[rng.integers(0, 4)]), kind, stream, start)
        else:
            mode = (LINEAR, EXACT, APPROX)[rng.integers(0, 3)]
            k = int(K_VALUES[rng.integers(0, 5)])
            nq = int(NQ_VALUES[rng.integers(0, 5)])
            if mode == APPROX:                                             # expectation = MihOracle.find: near queries, k <= 100
                kind, k = "near", min(k, 100)
            if nq * k > MAX_ROWS:
                continue
            if stream in ("own", "set_side"):
                c = knn("knn", mode, k, nq, kind, stream, int(rng.integers(0, 2)), bool(rng.integers(0, 2)), start)
            else:
                c = knn(("knn_dev", "knn_dev_stats")[rng.integers(0, 2)], mode, k, nq, kind, stream, start=start)
        if c not in out:
            out.append(c)
    return out


def multiset(m, seed):
    named = named_calls(m)
    calls = list(named.values())
    for c in drawn_calls(m, seed):
        if c not in calls:
            calls.append(c)
    return named, calls


def orders(m, seed):
    """{'descending' | 'ascending' | 'shuffled': [Call]}: every distinct call twice in each"""
    named, calls = multiset(m, seed)
    twice = [(c, occ) for occ in range(2) for c in calls]
    desc = [c for c, _ in sorted(twice, key=lambda co: (-co[0].size, co[1]))]
    asc = [c for c, _ in sorted(twice, key=lambda co: (co[0].size, co[1]))]
    rest = list(calls) + list(calls)
    units = []
    for a, b in PAIRS:
        rest.remove(named[a])
        rest.remove(named[b])
        units.append([named[a], named[b]])
    units += [[c] for c in rest]
    rng = np.random.default_rng(seed + 1)
    shuffled = [c for i in rng.permutation(len(units)) for c in units[i]]
    return {"descending": desc, "ascending": asc, "shuffled": shuffled}


def has_adjacent(seq, a, b):
    return any(x == a and y == b for x, y in zip(seq, seq[1:]))
