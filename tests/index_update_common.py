"""Shared data of the index-update tests (vc_update_index): codes whose substrings take CHOSEN key values, and a numpy model of
the update.

A table's key of a record is the little-endian value of its substring (substring t = bytes [t s/8, (t+1) s/8)), so a database is
written down as an [n, m] array of keys.  The old part draws its keys from a small pool (duplicate-heavy buckets, all even
values); the appended part holds, per table, every way a new entry can meet the old index:
  (a) entries for keys that already have a bucket;
  (b) new keys below the smallest old key, key 0 among them;
  (c) new keys strictly between old keys (odd values);
  (d) new keys above the largest old key, 2^s - 1 among them;
  (e) many new entries for ONE key: for a key with an old bucket and for a new key;
  (f) s = 32: new keys on both sides of a 128-key line edge (..127 / ..128) and of a 256-key block edge (..255 / ..256) inside blocks
      that hold old keys, and one in a block that held none.
The planted entries need room: the cases are complete from PLANT_MIN_OLD old and PLANT_MIN_NEW new records on; shorter parts get a
prefix of the plan (which starts with keys 0 and 2^s - 1)."""
import functools
from collections import namedtuple

import numpy as np

SHAPES = ((64, 8), (64, 4), (128, 8), (256, 16), (64, 2), (128, 4), (256, 8), (512, 16))     # (bits, tables): s = 8, 16 x 3, 32 x 4
FILE_SHAPES = ((64, 8), (64, 4), (128, 8), (256, 16), (64, 2))        # whole index files are compared (32-bit tables: > 0.5 GB each)
SWEEP_SHAPES = ((64, 8), (64, 4), (64, 2))                            # one shape per substring width for the tile-edge sweep
SWEEP_N0 = (255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385)
SWEEP_DELTA = 777
PAIRS = ((0, 500), (1, 1), (5000, 1), (5000, 0), (300, 20000))        # (n0, delta) of every shape
POOL = 48                    # old keys per table (s = 32: two more, next to the planted edges)
PLANT_MIN_OLD, PLANT_MIN_NEW = 255, 500
MANY = 40                    # entries of case (e)
EDGE_BASE = 0x40000000       # s = 32: the blocks [EDGE_BASE, +256) and [+256, +512) hold old keys; the line edge is at +128
EMPTY_BLOCK_KEY = 0x70000101 # s = 32: a key whose 256-key block holds no old key

Plan = namedtuple("Plan", "pool below between above many_old many_new edges empty_block")


def cases():
    """every (bits, m, n0, delta) the GPU test runs: PAIRS at every shape, the sweep at one shape per substring width"""
    out = [(b, m, n0, d) for b, m in SHAPES for n0, d in PAIRS]
    out += [(b, m, n0, SWEEP_DELTA) for b, m in SWEEP_SHAPES for n0 in SWEEP_N0]
    return out


@functools.lru_cache(maxsize=None)
def plan(bits, m, t):
    """the key values of table t: the old pool and the new-only keys of cases (b) .. (f)"""
    s = bits // m
    rng = np.random.default_rng(100000 * bits + 100 * m + t)
    top = 1 << s
    if s == 8:
        pool = [16 + 4 * i for i in range(POOL)]
    else:
        pool = set()
        while len(pool) < POOL:
            v = int(rng.integers(top // 16, top - top // 16)) & ~1
            if s == 32 and (EDGE_BASE - 512 <= v < EDGE_BASE + 1024 or (v >> 8) == (EMPTY_BLOCK_KEY >> 8)):
                continue
            pool.add(v)
        if s == 32:
            pool |= {EDGE_BASE + 100, EDGE_BASE + 300}
        pool = sorted(pool)
    lo, hi = pool[0], pool[-1]
    between = [((a + b) // 2) | 1 for a, b in zip(pool, pool[1:]) if b - a >= 4][:: max(1, len(pool) // 8)]
    edges = (EDGE_BASE + 127, EDGE_BASE + 128, EDGE_BASE + 255, EDGE_BASE + 256) if s == 32 else ()
    return Plan(tuple(pool), (0, lo // 2 | 1), tuple(between), (top - 1, hi + (top - hi) // 2 | 1), pool[len(pool) // 3], between[0] + 0,
                edges, EMPTY_BLOCK_KEY if s == 32 else None)


def _planted(p):
    """the appended part's planted keys of one table, most telling first"""
    out = [0, p.above[0], p.below[1], p.above[1]]
    out += list(p.edges) + ([p.empty_block] if p.empty_block is not None else [])
    out += list(p.between)
    out += [p.many_old] * MANY + [p.many_new] * MANY
    return out


@functools.lru_cache(maxsize=None)
def keys(bits, m, n0, delta):
    """([n0, m], [delta, m]) uint32 keys of the old and of the appended records"""
    rng = np.random.default_rng(1000003 * bits + 10007 * m + 31 * n0 + delta)
    old = np.empty((n0, m), dtype=np.uint32)
    new = np.empty((delta, m), dtype=np.uint32)
    for t in range(m):
        p = plan(bits, m, t)
        pool = np.array(p.pool, dtype=np.uint32)
        col = pool[rng.integers(0, len(pool), n0)]
        col[: min(n0, len(pool))] = pool[: min(n0, len(pool))]    # every pool key has a bucket once there is room
        old[:, t] = col[rng.permutation(n0)]
        planted = np.array(_planted(p)[:delta], dtype=np.uint32)
        fresh = np.array(p.between + p.below + p.above, dtype=np.uint32)
        rest = delta - len(planted)
        fill = np.where(rng.random(rest) < 0.9, pool[rng.integers(0, len(pool), rest)], fresh[rng.integers(0, len(fresh), rest)])
        new[:, t] = np.concatenate([planted, fill.astype(np.uint32)])[rng.permutation(delta)]
    for a in (old, new):
        a.setflags(write=False)
    return old, new


def codes_of(key_rows, bits, m):
    """[n, m] keys -> [n, bits / 8] code bytes"""
    s = bits // m
    dt = {8: np.uint8, 16: np.dtype("<u2"), 32: np.dtype("<u4")}[s]
    return np.ascontiguousarray(key_rows.astype(dt)).view(np.uint8).reshape(len(key_rows), bits // 8)


def codes(bits, m, n0, delta):
    """(old codes, appended codes)"""
    old, new = keys(bits, m, n0, delta)
    return codes_of(old, bits, m), codes_of(new, bits, m)


# ---------------------------------------------------------------- numpy model of a table
Table = namedtuple("Table", "ids offsets bitmap_keys n_unique")     # ranked (s = 32): offsets[U + 1] + sorted distinct keys; direct: offsets[2^s + 1]


def table_from_scratch(k, s):
    """the table vc_build_index builds from the keys k of records 0 .. n - 1: a stable sort by key"""
    k = np.asarray(k, dtype=np.uint64)
    ids = np.argsort(k, kind="stable").astype(np.uint32)
    distinct = np.unique(k)
    if s < 32:
        offsets = np.searchsorted(k[ids], np.arange((1 << s) + 1, dtype=np.uint64), side="left").astype(np.uint32)
        return Table(ids, offsets, distinct, 0)
    offsets = np.append(np.searchsorted(k[ids], distinct, side="left"), len(k)).astype(np.uint32)
    return Table(ids, offsets, distinct, len(distinct))


def update_model(old, k_new, n0, s):
    """The update rule: `old` = the table of records [0, n0), k_new = the keys of records n0 ..; returns the merged table built WITHOUT
    sorting an old entry: sort the new pairs, one insert point each, old position p -> p + #{j : ins[j] <= p}, new j -> ins[j] + j."""
    k_new = np.asarray(k_new, dtype=np.uint64)
    d = len(k_new)
    order = np.argsort(k_new, kind="stable")
    kd, idd = k_new[order], (n0 + order).astype(np.uint32)
    if s < 32:
        ins = old.offsets[kd.astype(np.int64) + 1].astype(np.int64)
    else:
        rank = np.searchsorted(old.bitmap_keys, kd, side="left")                  # set bits below the key
        bit = np.isin(kd, old.bitmap_keys)
        ins = old.offsets[rank + bit].astype(np.int64)
    assert np.all(np.diff(ins) >= 0)
    ids = np.full(n0 + d, 0xFFFFFFFF, dtype=np.uint32)
    p = np.arange(n0, dtype=np.int64)
    ids[p + np.searchsorted(ins, p, side="right")] = old.ids
    ids[ins + np.arange(d)] = idd
    distinct = np.union1d(old.bitmap_keys, kd)
    if s < 32:
        offsets = (old.offsets + np.searchsorted(kd, np.arange((1 << s) + 1, dtype=np.uint64), side="left")).astype(np.uint32)
        return Table(ids, offsets, distinct, 0)
    head = np.append(True, kd[1:] != kd[:-1]) if d else np.zeros(0, dtype=bool)
    nb = np.nonzero(head & ~bit)[0]                                               # first entries of the new buckets, key order
    nb_rank, nb_pos = rank[nb], ins[nb] + nb
    U = old.n_unique
    offsets = np.full(U + len(nb) + 1, 0xFFFFFFFF, dtype=np.uint32)
    r = np.arange(U + 1, dtype=np.int64)
    offsets[r + np.searchsorted(nb_rank, r, side="right")] = old.offsets + np.searchsorted(ins, old.offsets, side="right")
    offsets[nb_rank + np.arange(len(nb))] = nb_pos
    return Table(ids, offsets, distinct, U + len(nb))
