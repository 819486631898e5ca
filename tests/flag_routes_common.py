"""Shared by test_flag_routes_cpu.py and test_flag_routes_gpu.py: the reference-fidelity flags (VC_FLAG_USE_BITMAP,
VC_FLAG_REF_SIGNEXT_KEYS, VC_FLAG_REF_STOP_LITERAL4) crossed with the MIH execution routes, at five small shapes.  Shapes,
seeded data, the flag sets that bite at each shape, the route table and the engine-free expectation (MihOracle.find =
SearchWorker::find, search_worker.cc:159-264, plus the engine's canonical tie rule) live here; nothing in this module
touches the engine, so the CPU suite pins on exactly this data that every flag and every route has something to get wrong.

Expectations are computed once per (shape, flag set, mode) and shared by every route: they are never modified."""
import functools
from collections import namedtuple
from math import comb

import numpy as np

SH = np.uint64(32)
NQ = 16
FLIPS = (0, 1, 2, 3, 4, 6, 8, 10)                # query i gets FLIPS[i % 8] distinct flipped bits
BITMAP, SIGNEXT, LITERAL4 = 1, 2, 4              # VC_FLAG_USE_BITMAP, VC_FLAG_REF_SIGNEXT_KEYS, VC_FLAG_REF_STOP_LITERAL4
CODE_SEED = 34

Shape = namedtuple("Shape", "bits m n centres flips k k_approx")
SHAPES = {
    "A": Shape(128, 4, 30000, 150, 10, 20, 5),    # 4 x 32 bit: every shell class of a grouped pass and the shell beyond it
    "B": Shape(64, 2, 30000, 150, 6, 20, 5),      # 2 x 32 bit: the stop multiplier bites, radii 5-6 are handed over
    "C": Shape(64, 4, 30000, 150, 6, 20, 5),      # 4 x 16 bit: direct-key scan, sign extension changes rows
    "D": Shape(64, 8, 20000, 100, 4, 10, None),   # 8 x 8 bit: sign extension changes the statistics only
    "E": Shape(128, 8, 30000, 150, 8, 20, None),  # 8 x 16 bit, two words per code
}

# only the sets that bite: signext does nothing at s = 32, literal4 nothing at m >= 4
FLAG_SETS = {
    "A": ("bitmap",),
    "B": ("bitmap", "literal4", "literal4+bitmap"),
    "C": ("bitmap", "signext", "signext+literal4", "signext+literal4+bitmap"),     # signext+literal4 = VC_REF_QUIRKS=1
    "D": ("signext", "signext+bitmap"),
    "E": ("signext+bitmap",),
}

# route name -> environment read at vc_create
ROUTES = {
    "default": {},
    "host_loop": {"VC_MIH_HOST_LOOP": "1"},       # every shell through the multi-block kernels
    "budget1": {"VC_MIH_BUDGET": "1"},            # shell 0 in the query kernel, then the hand-over
    "bcodes0": {"VC_MIH_BCODES": "0"},            # <= 16-bit substrings verify through the id gather
    "switch2": {"VC_MIH_SWITCH": "2"},            # the scan switch forced wherever the planner allows it
    "group1": {"VC_MIH_GROUP": "1"},              # shells sharing the query kernel's first pass
    "group2": {"VC_MIH_GROUP": "2"},
    "group3": {"VC_MIH_GROUP": "3"},
    "lines1": {"VC_MIH_LINES": "1"},              # directory lines of the 32-bit tables
    "bent0": {"VC_MIH_BENT": "0"},                # 32-bit substrings of <= 128-bit codes verify through the id gather
    "bent0_lines1": {"VC_MIH_BENT": "0", "VC_MIH_LINES": "1"},
}
ALL_SHAPES = ("default", "host_loop", "budget1", "bcodes0", "switch2")
ROUTES_OF = {
    "A": ALL_SHAPES + ("group1", "group2", "group3", "lines1", "bent0", "bent0_lines1"),
    "B": ALL_SHAPES + ("group1", "group2", "group3", "lines1", "bent0", "bent0_lines1"),
    "C": ALL_SHAPES,
    "D": ALL_SHAPES,
    "E": ("default", "host_loop"),
}

# the sharded store: (shape, flag set, shards)
SHARDED = (("C", "signext+literal4+bitmap", 3), ("B", "literal4+bitmap", 4))


def cases():
    """every (shape, flag set, route) cell"""
    return [(s, f, r) for s in SHAPES for f in FLAG_SETS[s] for r in ROUTES_OF[s]]


def case_id(case):
    return "-".join(case)


def flag_bits(name):
    return sum({"bitmap": BITMAP, "signext": SIGNEXT, "literal4": LITERAL4}[p] for p in name.split("+") if p)


def oracle_settings(shape_id, flags, approximate=False):
    """(key_mode, use_bitmap, stop_mult) of MihOracle for a flag set; approximate mode stops on the heap size, and the
    oracle is given the literal 4 there as test_mih_approximate_parity does"""
    m = SHAPES[shape_id].m
    fb = flag_bits(flags)
    return (0 if fb & SIGNEXT else 1, bool(fb & BITMAP), 4 if (fb & LITERAL4 or approximate) else min(m, 4))


def switch_forbidden(shape_id, flags):
    """knn_plan's switch_ok: the scan switch reproduces the radius loop only without bitmap counters, with masked keys and
    with the exact stop multiplier min(m, 4)"""
    fb = flag_bits(flags)
    return bool(fb & (BITMAP | SIGNEXT)) or bool(fb & LITERAL4 and SHAPES[shape_id].m < 4)


@functools.lru_cache(maxsize=None)
def _codes(vo, shape_id):
    sh = SHAPES[shape_id]
    c = vo.gen_codes(sh.n, sh.bits, CODE_SEED, kind=1, n_centres=sh.centres, max_flips=sh.flips)
    c.setflags(write=False)
    return c


def make_codes(vo, shape_id):
    return _codes(vo, shape_id)


@functools.lru_cache(maxsize=None)
def _queries(vo, shape_id):
    sh = SHAPES[shape_id]
    codes = _codes(vo, shape_id)
    rng = np.random.default_rng(sh.bits + sh.m)
    q = codes[rng.integers(0, sh.n, NQ)].copy()
    for i in range(NQ):
        for b in rng.choice(sh.bits, size=FLIPS[i % 8], replace=False):
            q[i, b // 8] ^= np.uint8(1 << (b % 8))
    s = sh.bits // sh.m
    if s < 32:
        q[::2, s // 8 - 1] ^= 0x80                # the top bit of substring 0: where sign extension bites
    q.setflags(write=False)
    return q


def make_queries(vo, shape_id):
    """[NQ, bits/8]: database items with 0..10 flipped bits; every other query has the top bit of substring 0 flipped"""
    return _queries(vo, shape_id)


# ---- the engine's contract, engine-free
def reach_min_subdist(vo, codes, q, m, signext):
    """min over tables of the substring distance; with sign-extended keys a table only reaches items whose
    substring top bit equals the query's (Pilaf/image_tools.h:13)."""
    sub = vo.np_sub_distances(codes, q, m).astype(np.int64)
    if signext:
        nlb = codes.shape[1] // m
        x = np.bitwise_xor(codes, q[None, :]).reshape(codes.shape[0], m, nlb)
        top_differs = (x[:, :, nlb - 1] & 0x80) != 0
        sub[top_differs] = 10 ** 6
    return sub.min(axis=1)


def canonical_mih(vo, codes, q, m, k, radius, signext, id_base=0):
    """the k smallest (dist, id) among the items reachable within `radius`, and how many are reachable"""
    seen = reach_min_subdist(vo, codes, q, m, signext) <= radius
    d = vo.np_distances(codes, q)
    ids = np.arange(codes.shape[0], dtype=np.uint64) + np.uint64(id_base)
    packed = np.sort(vo.pack(d[seen], ids[seen]))
    return packed[:k], int(seen.sum())


def check_contract(got, oracle_res):
    """distance multiset + id set below the k-th distance."""
    o = np.sort(oracle_res)
    assert len(got) == len(o)
    assert np.array_equal(got >> SH, o >> SH)
    if len(o):
        dk = o[-1] >> SH
        assert set(got[(got >> SH) < dk].tolist()) == set(o[(o >> SH) < dk].tolist())


def leaves(s, radius):
    """keys of shells 0..radius of one s-bit table: what the reference counts per rank without looking at the data"""
    return sum(comb(s, r) for r in range(radius + 1))


# one query's expectation.  stats = (radius, n_results, n_sub_reads, n_local_reads, n_candidates): the fields of a 40-byte
# vc_query_stats record next to n_main_reads, which is always 0; n_candidates is the oracle's distinct-candidate count
Expect = namedtuple("Expect", "oracle_row row stats")


def _expect_rows(vo, codes, q, m, k, key_mode, use_bitmap, stop_mult, approximate, id_base):
    mo = vo.MihOracle(codes, m, key_mode=key_mode, id_base=id_base)
    out = []
    for i in range(q.shape[0]):
        ores, ost = mo.find(q[i], k, approximate=approximate, use_bitmap=use_bitmap, stop_mult=stop_mult)
        row, reachable = canonical_mih(vo, codes, q[i], m, k, ost.radius, key_mode == 0, id_base)
        assert ost.n_main_reads == 0 and reachable == ost.n_distinct      # the oracle and the numpy reach rule agree
        out.append(Expect(np.sort(ores), row, (ost.radius, ost.n_results, ost.n_sub_reads, ost.n_local_reads, ost.n_distinct)))
    mo.close()
    return out


@functools.lru_cache(maxsize=None)
def expect(vo, shape_id, flags, approximate=False):
    """[NQ] Expect of one engine over the whole shape"""
    sh = SHAPES[shape_id]
    key_mode, use_bitmap, stop_mult = oracle_settings(shape_id, flags, approximate)
    k = sh.k_approx if approximate else sh.k
    return _expect_rows(vo, _codes(vo, shape_id), _queries(vo, shape_id), sh.m, k, key_mode, use_bitmap, stop_mult, approximate, 0)


def split_ranges(n, shards, id_base=0):
    """(first id, count) of every shard of a store filled to its capacity n; the GPU suite checks them against
    ShardedEngine.shard_range"""
    return [(id_base + n * g // shards, n * (g + 1) // shards - n * g // shards) for g in range(shards)]


def expect_sharded(vo, shape_id, flags, ranges):
    """Every shard runs SearchWorker::find to its own stop rule over its id range (first id, count): rows = the k smallest
    of the shards' rows, radius = the maximum, n_sub_reads / n_local_reads / n_candidates = the sums."""
    sh = SHAPES[shape_id]
    key_mode, use_bitmap, stop_mult = oracle_settings(shape_id, flags)
    codes, q = _codes(vo, shape_id), _queries(vo, shape_id)
    parts = [_expect_rows(vo, codes[first:first + cnt], q, sh.m, sh.k, key_mode, use_bitmap, stop_mult, False, first)
             for first, cnt in ranges if cnt]
    out = []
    for i in range(NQ):
        ps = [p[i] for p in parts]
        row = np.sort(np.concatenate([p.row for p in ps]))[:sh.k]
        orow = np.sort(np.concatenate([p.oracle_row for p in ps]))[:sh.k]
        st = (max(p.stats[0] for p in ps), len(row), sum(p.stats[2] for p in ps), sum(p.stats[3] for p in ps),
              sum(p.stats[4] for p in ps))
        out.append(Expect(orow, row, st))
    return out
