"""Shared data of the removal tests (vc_retain*): databases, named keep masks and a numpy model of the filter.

The databases are those of the index-update tests (index_update_common): their planted keys hold every bucket situation -- duplicate-
heavy buckets, keys 0 and 2^s - 1, both sides of a 128-key line edge and of a 256-key block edge, a block with a single key.  A mask
is a bool array over the records, True = the record survives.

Size sweep: the first N rows of a fixed row permutation of the (300, 20000) database.  The sizes sit on the edges of what the code
walks in steps: the keep bitmap's 64-record word, its 256-record rank block, 2048 / 4096 / 16384 (the update's merge tile, the sort's
sub-tile and block), and 8192 -- the tile of the exclusive scan (vc_sort.hip SCAN_ITEMS) that the filter runs over N + 1 flags, which
the list of the issue did not have."""
import functools

import numpy as np

import index_update_common as U

DATABASES = ((0, 500), (300, 20000), (5000, 1))           # (n0, delta) of index_update_common.codes
SWEEP_DB = (300, 20000)
SWEEP_N = (63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385)
MASKS = ("all", "none", "only_first", "only_last", "drop_first", "drop_last", "every_other", "first_half", "second_half", "sparse",
         "dense", "bucket_edges", "whole_buckets")
# the sweep runs the masks whose keep words, rank blocks and scan tiles differ with N at the tail: an alternating pattern, a seeded
# sparse and a seeded dense one, and the one that cuts the last record (the last, partial bitmap word)
SWEEP_MASKS = ("every_other", "sparse", "dense", "drop_last")
GONE = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def db_keys(bits, m, n0, d):
    a = np.concatenate(U.keys(bits, m, n0, d))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def db_codes(bits, m, n0, d):
    a = np.concatenate(U.codes(bits, m, n0, d))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _sweep_rows(bits, m):
    return np.random.default_rng(424242 + bits * 100 + m).permutation(sum(SWEEP_DB))


def sweep_keys(bits, m, n):
    return db_keys(bits, m, *SWEEP_DB)[_sweep_rows(bits, m)[:n]]


def sweep_codes(bits, m, n):
    return np.ascontiguousarray(db_codes(bits, m, *SWEEP_DB)[_sweep_rows(bits, m)[:n]])


def vanish_set(bits, m, t):
    """the keys of table t whose buckets the mask `whole_buckets` removes whole"""
    p = U.plan(bits, m, t)
    s = bits // m
    out = {0, (1 << s) - 1, p.many_old, p.between[0]}
    if s == 32:
        out |= set(p.edges) | {p.empty_block}
    return sorted(out)


def mask(name, keys, bits, m):
    """the named keep mask over the records whose [n, m] keys are given"""
    n = len(keys)
    keep = np.ones(n, dtype=bool)
    rng = np.random.default_rng(7919 * n + 31 * bits + m)
    if name == "all":
        pass
    elif name == "none":
        keep[:] = False
    elif name == "only_first":
        keep[1:] = False
    elif name == "only_last":
        keep[:-1] = False
    elif name == "drop_first":
        keep[0] = False
    elif name == "drop_last":
        keep[-1] = False
    elif name == "every_other":
        keep[1::2] = False
    elif name == "first_half":
        keep[n // 2:] = False
    elif name == "second_half":
        keep[: n // 2] = False
    elif name == "sparse":
        keep = rng.random(n) >= 0.01
    elif name == "dense":
        keep = rng.random(n) < 0.01
    elif name == "bucket_edges":
        col = keys[:, 0]
        order = np.argsort(col, kind="stable")
        starts = np.nonzero(np.append(True, col[order][1:] != col[order][:-1]))[0]
        ends = np.append(starts[1:], n)
        for a, b in zip(starts, ends):
            if b - a >= 3:
                keep[order[[a, (a + b) // 2, b - 1]]] = False
    elif name == "whole_buckets":
        for t in range(m):
            keep &= ~np.isin(keys[:, t], np.array(vanish_set(bits, m, t), dtype=keys.dtype))
    else:
        raise KeyError(name)
    return keep


def new_ids_model(keep, id_base):
    """new_ids of vc_retain: the new global id of every old record, GONE for a removed one"""
    keep = np.asarray(keep, dtype=bool)
    out = np.full(len(keep), GONE, dtype=np.uint32)
    out[keep] = (id_base + np.arange(int(keep.sum()), dtype=np.int64)).astype(np.uint32)
    return out


def retain_model(table, keep, s):
    """The filter rule: `table` = the U.Table of all records, keep = the mask; the table of the survivors built WITHOUT sorting --
    S = the exclusive scan of the entries' keep flags, ids_new[S[p]] = new_local(ids[p]), offsets through S, buckets that lost
    every entry dropped."""
    keep = np.asarray(keep, dtype=bool)
    new_local = np.cumsum(keep) - keep                      # set bits strictly below i
    flags = keep[table.ids]
    S = np.append(0, np.cumsum(flags)).astype(np.int64)
    ids = new_local[table.ids[flags]].astype(np.uint32)
    K = int(S[-1])
    if s < 32:
        offsets = S[table.offsets].astype(np.uint32)
        distinct = np.nonzero(offsets[1:] > offsets[:-1])[0].astype(np.uint64)
        return U.Table(ids, offsets, distinct, 0)
    off = table.offsets.astype(np.int64)
    alive = S[off[1:]] > S[off[:-1]]
    offsets = np.append(S[off[:-1]][alive], K).astype(np.uint32)
    return U.Table(ids, offsets, table.bitmap_keys[alive], int(alive.sum()))


def same_table(a, b):
    return (np.array_equal(a.ids, b.ids) and np.array_equal(a.offsets, b.offsets) and
            np.array_equal(np.asarray(a.bitmap_keys, dtype=np.uint64), np.asarray(b.bitmap_keys, dtype=np.uint64)) and a.n_unique == b.n_unique)


def cases():
    """every (bits, m, kind, size, mask) the GPU test runs: kind "db" with size = (n0, delta), kind "sweep" with size = N"""
    out = [(b, m, "db", db, mk) for b, m in U.SHAPES for db in DATABASES for mk in MASKS]
    out += [(b, m, "sweep", n, mk) for b, m in U.SWEEP_SHAPES for n in SWEEP_N for mk in SWEEP_MASKS]
    return out


def case_keys(bits, m, kind, size):
    return db_keys(bits, m, *size) if kind == "db" else sweep_keys(bits, m, size)


def case_codes(bits, m, kind, size):
    return db_codes(bits, m, *size) if kind == "db" else sweep_codes(bits, m, size)
