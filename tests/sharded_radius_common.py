"""Shared by test_sharded_radius_dev_cpu.py and test_sharded_radius_dev_gpu.py: the shapes, their seeded data and queries,
the engine-free expectation (numpy brute force over the union) and a numpy model of the rank merge.  The CPU suite checks on
exactly the data the GPU suite runs that the inputs do what the GPU tests rely on."""
import functools

import numpy as np

SEED, ID_BASE = 34, 3
VC_SORT_CAP = 8192       # csrc/vc_common.hpp
MIH_RADIUS_TILE = 4096   # csrc/vc_mih.hip

# name -> bits, m, n, centres, flips, radius, shards, capacity, nq
SHAPES = {
    "interleaved": (64, 2, 30_000, 40, 6, 9, 3, 35_000, 8),     # 1: every planted query in all 3 shards, empty trailing shard
    "heavy": (64, 4, 30_000, 2, 3, 8, 8, 30_000, 8),            # 2: ~15 000 neighbours per query, segments of ~1 900
    "max_shards": (128, 4, 24_000, 40, 6, 9, 16, 27_000, 8),    # 3: VC_MAX_SHARDS, the last one empty, empty middle segments
    "one_shard": (64, 2, 20_000, 200, 6, 9, 1, 20_000, 8),      # 4: the merge degenerates to a copy
    "many_light": (64, 2, 8_000, 200, 6, 9, 3, 8_000, 4_099),   # 5: crosses MIH_RADIUS_TILE and the offsets kernel's tile loop
}


def planted_queries(codes, rng, nq, flips):
    """as test_sharded_native_gpu._queries: database items with up to `flips` flipped bits"""
    q = codes[rng.integers(0, codes.shape[0], size=nq)].copy()
    for i in range(nq):
        for b in rng.choice(codes.shape[1] * 8, size=int(rng.integers(0, flips + 1)), replace=False):
            q[i, b // 8] ^= np.uint8(1 << (b % 8))
    return q


def make(vo, name, seed=0):
    """(codes, queries) of a shape: nq - 1 planted queries (up to 4 flips) and one uniform-random query at the end"""
    bits, _, n, centres, flips, _, shards, _, nq = SHAPES[name]
    codes = vo.gen_codes(n, bits, SEED, kind=1, n_centres=centres, max_flips=flips)
    rng = np.random.default_rng(bits + shards + seed)
    q = np.concatenate([planted_queries(codes, rng, nq - 1, 4), rng.integers(0, 256, size=(1, bits // 8), dtype=np.uint8)])
    return codes, q


def expected_rows(vo, codes, queries, radius):
    """per query: the ascending packed neighbours within `radius`, numpy brute force over the union"""
    rows = []
    for q in queries:
        d = vo.np_distances(codes, q)
        ids = np.nonzero(d <= radius)[0]
        rows.append(np.sort(vo.pack(d[ids], ids.astype(np.uint64) + np.uint64(ID_BASE))))
    return rows


@functools.lru_cache(maxsize=None)
def case(vo, name, seed=0):
    """(codes, queries, expected rows) of a shape, computed once per session and shared: treat as read-only"""
    codes, q = make(vo, name, seed)
    return codes, q, expected_rows(vo, codes, q, SHAPES[name][5])


def shard_bounds(capacity, shards):
    """[lo, hi) of every shard's ids relative to id_base: capacity * g / G"""
    return [(capacity * g // shards, capacity * (g + 1) // shards) for g in range(shards)]


def shard_segments(row, capacity, shards):
    """a query's expected row split into the shards' ascending segments (what every shard's radius search returns)"""
    ids = (row & np.uint64(0xFFFFFFFF)).astype(np.int64) - ID_BASE
    return [row[(ids >= lo) & (ids < hi)] for lo, hi in shard_bounds(capacity, shards)]


def rank_merge(segments):
    """the merge kernel's rule: the place of element i of list g is i + sum over the other lists of lower_bound(list, value)"""
    total = sum(len(s) for s in segments)
    out = np.zeros(total, dtype=np.uint64)
    hit = np.zeros(total, dtype=np.int64)
    for g, seg in enumerate(segments):
        pos = np.arange(len(seg), dtype=np.int64)
        for g2, other in enumerate(segments):
            if g2 != g:
                pos += np.searchsorted(other, seg, "left")
        out[pos] = seg
        hit[pos] += 1
    assert np.all(hit == 1)          # every place written exactly once
    return out
