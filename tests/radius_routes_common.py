"""Shared by test_radius_routes_cpu.py and test_radius_routes_gpu.py: the fixed-radius search (vc_search_radius, vc_search_radius_dev,
vc_sharded_search_radius[_dev]) on each of the four routes radius_search_device can take (vc_mih.hip radius_route: mih_query_kernel
in MQ_MODE_RADIUS, mih_bucket_stream_kernel, one mih_probe_kernel launch per shell, the verify kernel with a fixed threshold),
crossed with VC_FLAG_USE_BITMAP and VC_FLAG_REF_SIGNEXT_KEYS, at seven shapes that cover every word count (1, 2, 4, 8) and every
substring width (8, 16, 32), from R = 0 down to the deepest shell a route can be asked for.

Shapes, seeded data with planted boundary items, the radius lists, the route knobs, the expected route of every (shape, R) under
default knobs as a literal, a model of radius_plan / radius_route for the forced routes, and the engine-free closed-form expectation
live here.  Nothing in this module touches the engine; test_radius_routes_cpu.py pins on exactly this data that every cell of the
GPU suite has something to get wrong.  Expectations are computed once, shared and never modified."""
import functools
import os
import re
from collections import namedtuple
from math import comb

import numpy as np

SH = np.uint64(32)
BITMAP, SIGNEXT = 1, 2                           # VC_FLAG_USE_BITMAP, VC_FLAG_REF_SIGNEXT_KEYS
CAND_CAP = 512                                   # vc_config.cand_cap of every engine: the work ring starts at max(512, 4096) entries
RING_START = 4096
NQ = 6
N_SHARDS = 3
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "verticut_amd", "csrc", "vc_mih.hip")

# per_dist ball items at every full distance 0..ball_to around each of the four ball centres
Shape = namedtuple("Shape", "bits m n id_base ball_to per_dist seed")
SHAPES = {
    "64/8": Shape(64, 8, 8192, 77, 64, 3, 1),                     # W = 1, 8 x 8 bit: the largest n, probes x avg_bucket = MQ_ENTRY_BUDGET at R = bits
    "64/4": Shape(64, 4, 6001, 0, 64, 3, 2),                      # W = 1, 4 x 16 bit
    "64/2": Shape(64, 2, 4099, 1 << 20, 64, 3, 3),                # W = 1, 2 x 32 bit
    "128/4": Shape(128, 4, 5003, (1 << 32) - 1 - 5003, 128, 3, 4),   # W = 2, 4 x 32 bit; the last id is 2^32 - 2
    "256/16": Shape(256, 16, 7001, 123456789, 256, 3, 5),         # W = 4, 16 x 16 bit
    "512/64": Shape(512, 64, 6007, 5, 512, 2, 6),                 # W = 8, 64 x 8 bit
    "512/16": Shape(512, 16, 4500, 3000000000, 128, 3, 7),        # W = 8, 16 x 32 bit: the widest mask set in LDS
}
N_SHAPES = 7
assert len(SHAPES) == N_SHAPES


def sbits(sid):
    return SHAPES[sid].bits // SHAPES[sid].m


# ---- radius_plan / radius_route (vc_mih.hip), as arithmetic
Limits = namedtuple("Limits", "MS_MAXP MQ_ENTRY_BUDGET MQ_RADIUS_BUDGET MIH_RADIUS_TILE")
LIMITS = Limits(2048, 65536, 4000000, 4096)      # test_radius_routes_cpu.py reads the same names from the source
SCAN_FLOOR = 1 << 20                             # vc_radius_search: the scan answers a plan of more than max(n, 2^20) probes


def source_limits():
    txt = open(SRC).read()
    return Limits(*(int(re.search(r"#define\s+%s\s+(\d+)" % name, txt).group(1)) for name in Limits._fields))


Plan = namedtuple("Plan", "R rq ra rsub n_big small_shells probes")


def radius_plan(bits, m, R):
    """R = m q + a after clamping to bits: tables 0..a search substring radius q, the others q - 1 (not at all when q = 0)"""
    s = bits // m
    R = min(R, bits)
    rq, ra = divmod(R, m)
    rsub, n_big, small = min(s, rq), min(m, ra + 1), (min(s, rq - 1) + 1 if rq else 0)
    probes = sum((m if r < small else n_big) * comb(s, r) for r in range(rsub + 1))
    return Plan(R, rq, ra, rsub, n_big, small, probes)


def table_radii(bits, m, R):
    """[m] substring radius of every table, -1 = not searched"""
    p = radius_plan(bits, m, R)
    return np.array([p.rq if t <= p.ra else p.rq - 1 for t in range(m)], dtype=np.int64)


def uses_index(bits, m, n, R):
    return radius_plan(bits, m, R).probes <= max(n, SCAN_FLOOR)


# route name -> environment read at vc_create ("linear" is mode = VC_MODE_LINEAR, no knob)
ROUTES = {
    "default": {},
    "host_loop": {"VC_MIH_HOST_LOOP": "1"},
    "stream2": {"VC_MIH_STREAM": "2"},                               # <= 16-bit substrings leave the query kernel at every size
    "stream0": {"VC_MIH_STREAM": "0"},
    "bcodes0": {"VC_MIH_BCODES": "0", "VC_MIH_STREAM": "2"},         # out of the query kernel, and no bucket-order codes to stream
    "linear": {},                                                    # mode = VC_MODE_LINEAR
}
NARROW_ROUTES = ("default", "host_loop", "stream2", "stream0", "bcodes0", "linear")
WIDE_ROUTES = ("default", "host_loop", "linear")                     # 32-bit substrings: the stream knobs and the code copies do not exist


def routes_of(sid):
    return NARROW_ROUTES if sbits(sid) < 32 else WIDE_ROUTES


def model_route(bits, m, n, R, route):
    """radius_route + the scan decision of vc_radius_search for a store of n records under a route's knobs"""
    s = bits // m
    if route == "linear" or not uses_index(bits, m, n, R):
        return "linear_scan"
    if route == "host_loop":
        return "host_shells"
    p = radius_plan(bits, m, R)
    inblock = p.probes <= LIMITS.MQ_RADIUS_BUDGET and p.rsub <= 16 and p.probes * (n / 2.0 ** s) <= LIMITS.MQ_ENTRY_BUDGET
    if route in ("stream2", "bcodes0") and s <= 16:
        inblock = False
    if inblock:
        return "query_kernel"
    stream = route != "stream0" and s <= 16 and p.probes <= LIMITS.MS_MAXP and route != "bcodes0"
    return "stream" if stream else "host_shells"


# ---- radii
def shallow_radii(m):
    return sorted({0, 1, m - 1, m, m + 1, 2 * m - 1, 2 * m} | {2 * m + a for a in range(min(m, 4))})


def index_edge(sid):
    """32-bit substrings: (the last R whose plan stays within max(n, 2^20) probes, the first R beyond)"""
    sh = SHAPES[sid]
    R = 0
    while uses_index(sh.bits, sh.m, sh.n, R + 1):
        R += 1
    return R, R + 1


# (shape, R) -> the queries sent at that R; every other R sends all six.  Shell 16 of 16-bit substrings costs 2^16 probes a table.
ONE_QUERY = {("64/4", 64): (0,), ("256/16", 256): (0,)}

RADII = {
    "64/8": shallow_radii(8) + [35, 63, 64, 69],                     # shell 4 (a = 3), all tables at 7, shell 8 = bits, clamped
    "64/4": shallow_radii(4) + [18, 27, 64],                         # shells 4 (a = 2) and 6 (a = 3); shell 16 = bits on one query
    "64/2": shallow_radii(2) + [11, 12, 64],                         # the last R on the index (shell 5), the first on the scan, bits
    "128/4": shallow_radii(4) + [23, 24, 128],
    "256/16": shallow_radii(16) + [69, 107, 256],                    # shells 4 (a = 5) and 6 (a = 11); shell 16 = bits on one query
    "512/64": shallow_radii(64) + [259, 511, 512, 517],              # shell 4 (a = 3), all tables at 7, shell 8 = bits, clamped
    "512/16": shallow_radii(16) + [80, 81, 512],
}

# the route radius_search_device takes under default knobs, per (shape, R): literals; test_radius_routes_cpu.py checks them against
# model_route with the limits read from the source
Q, S, H, L = "query_kernel", "stream", "host_shells", "linear_scan"
DEFAULT_ROUTE = {
    "64/8": {R: Q for R in RADII["64/8"]},                           # 2 048 probes x 32 entries = MQ_ENTRY_BUDGET exactly: still in the block
    "64/4": {R: Q for R in RADII["64/4"]},
    "64/2": {0: Q, 1: Q, 2: Q, 3: Q, 4: Q, 5: Q, 11: Q, 12: L, 64: L},
    "128/4": {0: Q, 1: Q, 3: Q, 4: Q, 5: Q, 7: Q, 8: Q, 9: Q, 10: Q, 11: Q, 23: Q, 24: L, 128: L},
    "256/16": {0: Q, 1: Q, 15: Q, 16: Q, 17: Q, 31: Q, 32: Q, 33: Q, 34: Q, 35: Q, 69: Q, 107: Q, 256: H},
    "512/64": {0: Q, 1: Q, 63: Q, 64: Q, 65: Q, 127: Q, 128: Q, 129: Q, 130: Q, 131: Q, 259: H, 511: H, 512: H, 517: H},
    "512/16": {0: Q, 1: Q, 15: Q, 16: Q, 17: Q, 31: Q, 32: Q, 33: Q, 34: Q, 35: Q, 80: Q, 81: L, 512: L},
}


def expected_route(sid, R, route, n=None):
    sh = SHAPES[sid]
    if route == "default" and n is None:
        return DEFAULT_ROUTE[sid][R]
    return model_route(sh.bits, sh.m, sh.n if n is None else n, R, route)


def walk(sid):
    """the radius list ascending, then in a seeded shuffle"""
    up = list(RADII[sid])
    rng = np.random.default_rng(1000 + SHAPES[sid].seed)
    return up + [up[i] for i in rng.permutation(len(up))]


def queries_at(sid, R):
    return ONE_QUERY.get((sid, R), tuple(range(NQ)))


# ---- flag sets and cells
FLAG_SETS = ("", "bitmap", "signext", "signext+bitmap")


def flag_bits(name):
    return sum({"bitmap": BITMAP, "signext": SIGNEXT}[p] for p in name.split("+") if p)


def cases():
    """every (shape, flag set, route) cell.  Below 32-bit substrings: four flag sets x six routes.  At 32 bits sign extension is the
    identity: two flag sets x three routes, and one cell with both flags on the default route that must change nothing."""
    out = []
    for sid in SHAPES:
        if sbits(sid) < 32:
            out += [(sid, f, r) for f in FLAG_SETS for r in routes_of(sid)]
        else:
            out += [(sid, f, r) for f in ("", "bitmap") for r in routes_of(sid)] + [(sid, "signext+bitmap", "default")]
    return out


def case_id(case):
    return "-".join((case[0], case[1] or "noflags", case[2]))


SHARDED = tuple((sid, f) for sid in ("64/4", "128/4") for f in FLAG_SETS)
TILE_LEGS = (("64/4", "default", Q), ("64/4", "stream2", S))          # (shape, route, the route the trace must name)
TILE_R = 5
TILE_COPIES = 4097


# ---- data
def _flip(code, nlb, t, bits_in_sub):
    for b in bits_in_sub:
        code[t * nlb + b // 8] ^= np.uint8(1 << (b % 8))


def _item(rng, centre, m, s, subs, top=()):
    """a copy of `centre` with subs[t] flipped bits in substring t; the substring's top bit is among them exactly for t in `top`"""
    nlb = s // 8
    c = centre.copy()
    for t, d in enumerate(subs):
        d = int(d)
        assert 0 <= d <= s
        if t in top:
            assert d >= 1
            low = rng.choice(s - 1, size=d - 1, replace=False) if d > 1 else []
            _flip(c, nlb, t, [s - 1] + [int(b) for b in low])
        else:
            pool = s if d == s else s - 1                        # (the top bit stays as it is unless the whole substring flips)
            _flip(c, nlb, t, [int(b) for b in rng.choice(pool, size=d, replace=False)])
    return c


def _ball(rng, centre, sh):
    """per_dist items at every full distance 0..ball_to, the flips dealt to the substrings in three ways in turn: anywhere, packed into
    as few tables as a random table order allows, dealt round to all tables"""
    s = sh.bits // sh.m
    out = []
    for d in range(sh.ball_to + 1):
        for j in range(sh.per_dist):
            way = (d + j) % 3
            if way == 0:
                pos = rng.choice(sh.bits, size=d, replace=False)
                subs = np.bincount(pos // s, minlength=sh.m)
                c = centre.copy()
                for b in pos:
                    c[b // 8] ^= np.uint8(1 << (b % 8))
                out.append(c)
                continue
            order = rng.permutation(sh.m)
            subs = np.zeros(sh.m, dtype=np.int64)
            if way == 1:
                left = d
                for t in order:
                    subs[t] = min(s, left)
                    left -= subs[t]
            else:
                subs[:] = d // sh.m
                subs[order[: d % sh.m]] += 1
            rank = rng.random((sh.m, s)).argsort(axis=1).argsort(axis=1)      # per table: a random order of its bits
            out.append(centre ^ np.packbits(rank < subs[:, None], axis=1, bitorder="little").reshape(-1))
    return out


def _planted(rng, centre, sh):
    """the boundary items of every shallow R (R < m, shell 1, shell 2 with every remainder) around one centre;
    test_radius_routes_cpu.py finds each kind again by its definition"""
    m, s = sh.m, sh.bits // sh.m
    out = []
    if s < 32:
        # the top bit of every substring differs: no sign-extended key reaches it at any radius, R = bits included
        out += [_item(rng, centre, m, s, [d] * m, top=tuple(range(m))) for d in (1, 2)]
    for R in shallow_radii(m):
        q, a = divmod(R, m)
        big, small = list(range(a + 1)), list(range(a + 1, m))
        if q == 0:
            # zero-distance substring only in the last searched table (a) and beyond: inside R, found through table a alone
            out.append(_item(rng, centre, m, s, [1] * a + [0] * (m - a)))
            if small:
                # zero-distance substring only in a table beyond a: full distance m - 1 > R, and no searched table reaches it
                subs = [1] * m
                subs[small[-1]] = 0
                out.append(_item(rng, centre, m, s, subs))
            continue
        # reachable through exactly one big table, at that table's radius; every small table at exactly q: full distance R
        for t in (big[0], big[-1]):
            subs = [q + 1 if u <= a else q for u in range(m)]
            subs[t] = q
            out.append(_item(rng, centre, m, s, subs))
            if s < 32:
                out.append(_item(rng, centre, m, s, subs, top=(t,)))          # the same, the reaching substring differs in its top bit
        # reachable only through a big table below its radius, a small table at exactly q
        subs = [q + 1 if u <= a else q for u in range(m)]
        subs[big[-1]] = q - 1
        out.append(_item(rng, centre, m, s, subs))
        if small:
            # reachable through exactly one small table at radius q - 1: full distance R
            for t in (small[0], small[-1]):
                subs = [q + 1 if u <= a else q for u in range(m)]
                subs[t] = q - 1
                out.append(_item(rng, centre, m, s, subs))
                if s < 32 and q >= 2:
                    out.append(_item(rng, centre, m, s, subs, top=(t,)))
        # several tables reach it: the first and the last at distance 0
        subs = [1] * m
        subs[0] = subs[m - 1] = 0
        if sum(subs) <= R:
            out.append(_item(rng, centre, m, s, subs))
        # full distance exactly R + 1 with one table in reach (outside R all the same)
        subs = [q + 1 if u <= a else q for u in range(m)]
        subs[0] = q
        subs[m - 1] += 1
        out.append(_item(rng, centre, m, s, subs))
        if s < 32:
            # table 0 is the lowest-index minimum and differs in its top bit; table 1 reaches it as well
            subs = [q + 1 if u <= a else q for u in range(m)]
            subs[0] = subs[1] = min(1, q)
            if sum(subs) <= R:
                out.append(_item(rng, centre, m, s, subs, top=(0,)))
    return out


@functools.lru_cache(maxsize=None)
def _data(sid):
    sh = SHAPES[sid]
    s, nb = sh.bits // sh.m, sh.bits // 8
    nlb = s // 8
    rng = np.random.default_rng(20240 + sh.seed)
    centres = rng.integers(0, 256, size=(4, nb), dtype=np.uint8)
    centres[3, nlb - 1::nlb] |= 0x80                             # the fourth centre: the top bit of every substring set
    special = []
    for i, c in enumerate(centres):
        special += _ball(rng, c, sh)
        if i in (0, 3):
            special += _planted(rng, c, sh)
    assert len(special) < sh.n - 1000, (sid, len(special))
    codes = rng.integers(0, 256, size=(sh.n, nb), dtype=np.uint8)
    codes[: len(special)] = np.array(special, dtype=np.uint8)
    codes = codes[rng.permutation(sh.n)]
    q = np.empty((NQ, nb), dtype=np.uint8)
    q[0], q[1], q[2], q[5] = centres[0], centres[1], centres[2], centres[3]
    q[3] = codes[sh.n // 2]
    q[3, 0] ^= 1                                                 # a near-duplicate of a record
    q[4] = rng.integers(0, 256, size=nb, dtype=np.uint8)         # uniform: few neighbours until deep
    codes.setflags(write=False)
    q.setflags(write=False)
    return codes, q


def make_codes(sid):
    return _data(sid)[0]


def make_queries(sid):
    """[6, bits/8]: three ball centres, a near-duplicate of a record, a uniform query, a ball centre whose substrings' top bits are all set"""
    return _data(sid)[1]


Geometry = namedtuple("Geometry", "dist sub topdiff")


@functools.lru_cache(maxsize=None)
def geometry(sid, qi):
    """of query qi against every record: full distances [n], substring distances [n, m], 'the substring's top bit differs' [n, m]"""
    sh = SHAPES[sid]
    codes, q = _data(sid)
    nlb = sh.bits // sh.m // 8
    x = np.bitwise_xor(codes, q[qi][None, :])
    sub = np.unpackbits(x, axis=1).reshape(sh.n, sh.m, -1).sum(axis=2).astype(np.int64)
    topdiff = (x.reshape(sh.n, sh.m, nlb)[:, :, nlb - 1] & 0x80) != 0
    for a in (sub, topdiff):
        a.setflags(write=False)
    return Geometry(sub.sum(axis=1), sub, topdiff)


# ---- the expectation: closed form, no key enumeration
def reach(sid, qi, R, signext):
    """[n, m] bool: table t reaches the record -- sub_t <= r_t, and under sign-extended keys of substrings below 32 bit the top bits
    of that substring agree too (a flipped top bit changes every bit above it in the key: no enumerated key has them)"""
    sh = SHAPES[sid]
    g = geometry(sid, qi)
    ok = g.sub <= table_radii(sh.bits, sh.m, R)[None, :]
    if signext and sbits(sid) < 32:
        ok &= ~g.topdiff
    return ok


def _pack(sid, qi, keep, lo=0, hi=None):
    sh = SHAPES[sid]
    g = geometry(sid, qi)
    idx = np.flatnonzero(keep[lo:hi]) + lo
    return np.sort((g.dist[idx].astype(np.uint64) << SH) | (idx.astype(np.uint64) + np.uint64(sh.id_base)))


@functools.lru_cache(maxsize=None)
def brute(sid, qi, R):
    r = _pack(sid, qi, geometry(sid, qi).dist <= R)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def closed_form(sid, qi, R, signext):
    """what the index returns: dist <= R and some table reaches the record; ascending packed dist << 32 | id_base + ordinal"""
    r = _pack(sid, qi, (geometry(sid, qi).dist <= min(R, SHAPES[sid].bits)) & reach(sid, qi, R, signext).any(axis=1))
    r.setflags(write=False)
    return r


def expect(sid, flags, route, R, qi, part=None):
    """the row of query qi at radius R from one engine (part = (first ordinal, count): from one shard of a store).  The scan knows no
    keys: LINEAR mode and a radius the scan answers give the brute force whatever the flags."""
    sh = SHAPES[sid]
    n = sh.n if part is None else part[1]
    if route == "linear" or not uses_index(sh.bits, sh.m, n, R):
        row = brute(sid, qi, R)
    else:
        row = closed_form(sid, qi, R, bool(flag_bits(flags) & SIGNEXT))
    if part is not None:
        ids = (row & np.uint64(0xFFFFFFFF)).astype(np.int64) - sh.id_base
        row = row[(ids >= part[0]) & (ids < part[0] + part[1])]
    return row


def split_ranges(n, shards):
    """(first ordinal, count) of every shard of a store filled to its capacity n"""
    return [(n * g // shards, n * (g + 1) // shards - n * g // shards) for g in range(shards)]


def expect_sharded(sid, flags, R, qi):
    """reachability is per record, so the union of the shards' rows is the closed form over the union -- shard by shard, since every
    shard decides by its own size whether the scan answers"""
    return np.sort(np.concatenate([expect(sid, flags, "default", R, qi, part) for part in split_ranges(SHAPES[sid].n, N_SHARDS)]))
