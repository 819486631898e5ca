"""Pinned without a GPU: the data, radii and route tables of test_radius_routes_gpu.py (radius_routes_common.py) make every route,
flag, table radius and boundary of the fixed-radius search matter, and the closed-form expectation the GPU rows are compared with
equals MihOracle.radius (search_R_neighbors' shell enumeration with the pigeonhole split, oracle/vc_oracle.cc) in both key modes."""
import numpy as np
import pytest

import radius_routes_common as F

ORACLE_PROBES = 1_100_000        # the oracle enumerates every key: pinned wherever one query's plan stays within about 10^6 probes


def test_the_seven_shapes_and_their_cells():
    """every word count 1, 2, 4, 8 and substring width 8, 16, 32; n within 4 000..8 192; one id range from 0 and one ending just below
    2^32; 4 x 24 + 3 x 7 = 117 cells, each once; the flag values are the ABI's"""
    from verticut_amd import engine
    assert (F.BITMAP, F.SIGNEXT) == (engine.FLAG_USE_BITMAP, engine.FLAG_REF_SIGNEXT_KEYS)
    assert len(F.SHAPES) == F.N_SHAPES == len(F.RADII) == len(F.DEFAULT_ROUTE) == 7
    assert sorted((sh.bits // 64, F.sbits(sid)) for sid, sh in F.SHAPES.items()) == [(1, 8), (1, 16), (1, 32), (2, 32), (4, 16), (8, 8), (8, 32)]
    assert all(4000 <= sh.n <= 8192 for sh in F.SHAPES.values())
    ends = [sh.id_base + sh.n for sh in F.SHAPES.values()]
    assert max(ends) == (1 << 32) - 1 and any(sh.id_base == 0 for sh in F.SHAPES.values())
    cases = F.cases()
    assert len(cases) == len({F.case_id(c) for c in cases}) == 4 * 24 + 3 * 7
    for sid in F.SHAPES:
        narrow = F.sbits(sid) < 32
        for fl in (F.FLAG_SETS if narrow else ("", "bitmap")):
            for route in (("default", "host_loop", "stream2", "stream0", "bcodes0", "linear") if narrow else ("default", "host_loop", "linear")):
                assert (sid, fl, route) in cases
        assert narrow or (sid, "signext+bitmap", "default") in cases
    assert all(F.SHAPES[sid].n >= 3 * 1000 for sid, _ in F.SHARDED) and {sid for sid, _ in F.SHARDED} == {"64/4", "128/4"}
    assert F.TILE_COPIES * F.NQ > F.LIMITS.MIH_RADIUS_TILE


def test_limits_are_the_sources():
    assert F.source_limits() == F.LIMITS
    txt = open(F.SRC).read()
    assert "std::max<uint64_t>(n, 1u << 20)" in txt and F.SCAN_FLOOR == 1 << 20      # vc_radius_search's scan decision
    assert "std::max(ix->cap, 4096u)" in txt and F.RING_START == max(F.CAND_CAP, 4096)


def test_radius_lists():
    """shallow: 0, 1, m - 1, m, m + 1, 2m - 1, 2m and every remainder 0..min(m, 4) - 1 at shell 2; deep: per substring width"""
    for sid, sh in F.SHAPES.items():
        m, s, radii = sh.m, F.sbits(sid), F.RADII[sid]
        assert radii == sorted(set(radii)) and set(F.DEFAULT_ROUTE[sid]) == set(radii)
        assert {0, 1, m - 1, m, m + 1, 2 * m - 1, 2 * m} <= set(radii)
        assert {F.radius_plan(sh.bits, m, R).ra for R in radii if R // m == 2} >= set(range(min(m, 4)))
        shells = {F.radius_plan(sh.bits, m, R).rsub for R in radii}
        assert sh.bits in radii
        if s == 8:
            assert {4, 7, 8} <= shells and sh.bits + 5 in radii
            assert F.radius_plan(sh.bits, m, sh.bits + 5) == F.radius_plan(sh.bits, m, sh.bits)
        elif s == 16:
            assert {4, 6, 16} <= shells and F.ONE_QUERY[(sid, sh.bits)] == (0,)
        else:
            last, first = F.index_edge(sid)
            assert last in radii and first in radii and first == last + 1
            edge = max(sh.n, 1 << 20)
            assert F.radius_plan(sh.bits, m, last).probes <= edge < F.radius_plan(sh.bits, m, first).probes
            assert F.radius_plan(sh.bits, m, last).rsub in (4, 5)
        # the ball reaches past the deepest shell the index is asked for
        deepest = max(F.radius_plan(sh.bits, m, R).rsub for R in radii if F.uses_index(sh.bits, m, sh.n, R))
        assert sh.ball_to >= min(sh.bits, (deepest + 1) * m)
        w = F.walk(sid)
        assert w[: len(radii)] == radii and sorted(w[len(radii):]) == radii and w[len(radii):] != radii
    assert set(F.ONE_QUERY) == {("64/4", 64), ("256/16", 256)}


def test_default_routes_are_the_models():
    """the literal route table equals radius_route's arithmetic with the limits of the source"""
    for sid, sh in F.SHAPES.items():
        for R in F.RADII[sid]:
            assert F.DEFAULT_ROUTE[sid][R] == F.model_route(sh.bits, sh.m, sh.n, R, "default"), (sid, R)


def test_every_route_is_reached():
    """Over the radius list of a shape the knobs reach every route that exists at its substring width -- all four at 8 and 16 bits,
    three at 32 bits (the stream kernel serves <= 16-bit substrings) -- whatever the flag set, and each forced route is the one
    its knob names.  Under default knobs three routes are reached: the stream route needs probes <= MS_MAXP with
    probes x n / 2^s > MQ_ENTRY_BUDGET, which is n > 8 192 at 8-bit substrings and far more at 16 -- beyond the sizes of this suite,
    so only VC_MIH_STREAM=2 takes a cell there."""
    cases = F.cases()
    for width, want in ((8, {F.Q, F.S, F.H, F.L}), (16, {F.Q, F.S, F.H, F.L}), (32, {F.Q, F.H, F.L})):
        for fl in F.FLAG_SETS:
            got = {F.expected_route(sid, R, route) for sid, f, route in cases if f == fl and F.sbits(sid) == width for R in F.RADII[sid]}
            if width == 32 and "signext" in fl:
                continue                                           # (the one 'changes nothing' cell)
            assert got == want, (width, fl, got)
    default = {F.DEFAULT_ROUTE[sid][R] for sid in F.SHAPES for R in F.RADII[sid]}
    assert default == {F.Q, F.H, F.L}
    assert F.LIMITS.MS_MAXP * 8192 / 2 ** 8 <= F.LIMITS.MQ_ENTRY_BUDGET
    for sid, sh in F.SHAPES.items():
        assert all(F.model_route(sh.bits, sh.m, sh.n, R, "default") != F.S for R in range(sh.bits + 1))
        # default knobs cross a route change on one handle wherever the table has one
        for R in F.RADII[sid]:
            assert F.expected_route(sid, R, "host_loop") == (F.H if F.uses_index(sh.bits, sh.m, sh.n, R) else F.L)
            assert F.expected_route(sid, R, "linear") == F.L
            if F.sbits(sid) < 32:
                p = F.radius_plan(sh.bits, sh.m, R).probes
                assert F.expected_route(sid, R, "stream2") == (F.S if p <= F.LIMITS.MS_MAXP else F.H)
                assert F.expected_route(sid, R, "bcodes0") == F.H
                assert F.expected_route(sid, R, "stream0") == F.DEFAULT_ROUTE[sid][R] != F.S
    assert {F.DEFAULT_ROUTE["512/64"][R] for R in F.RADII["512/64"]} == {F.Q, F.H}          # query kernel -> host shells as R grows
    assert {F.DEFAULT_ROUTE["256/16"][R] for R in F.RADII["256/16"]} == {F.Q, F.H}
    for sid in ("64/2", "128/4", "512/16"):
        assert {F.DEFAULT_ROUTE[sid][R] for R in F.RADII[sid]} == {F.Q, F.L}                # MIH <-> scan: the work buffers start over
    # both ends of the stream knob at both narrow widths: streamed shallow, host shells deep
    for sid in ("64/4", "256/16", "512/64"):
        assert {F.expected_route(sid, R, "stream2") for R in F.RADII[sid]} == {F.S, F.H}
    assert {F.expected_route("64/8", R, "stream2") for R in F.RADII["64/8"]} == {F.S}       # shell 8 of 8 tables is 2 041 probes: streamed
    for sid, route, name in F.TILE_LEGS:
        assert F.expected_route(sid, F.TILE_R, route) == name and F.TILE_R in F.RADII[sid]


def test_queries_follow_the_recipe():
    for sid, sh in F.SHAPES.items():
        codes, q = F.make_codes(sid), F.make_queries(sid)
        s = F.sbits(sid)
        assert codes.shape == (sh.n, sh.bits // 8) and q.shape == (F.NQ, sh.bits // 8)
        d = [F.geometry(sid, i).dist for i in range(F.NQ)]
        for i in (0, 1, 2, 5):                                     # ball centres: items at every full distance 0..ball_to
            assert set(range(sh.ball_to + 1)) <= set(d[i].tolist())
        assert d[3].min() == 1                                     # the near-duplicate
        assert d[4].min() > sh.bits // 8                           # uniform: nothing near
        assert np.all(q[5].reshape(sh.m, s // 8)[:, -1] & 0x80)    # the top bit of every substring
        # the ring: R = bits returns every record, more than the 4 096 entries the ring starts with
        assert sh.n > F.RING_START and all(len(F.brute(sid, i, sh.bits)) == sh.n for i in range(F.NQ))
        # the ball's flips are dealt in many ways: at full distance 2m some item has an untouched table, some item none
        sub = F.geometry(sid, 0).sub[d[0] == 2 * sh.m]
        assert (sub.min(axis=1) == 0).any() and (sub.min(axis=1) >= 1).any() and len({tuple(r) for r in sub.tolist()}) >= 3


def _kinds(sid, qi, R):
    """which boundary kinds query qi finds at radius R, by their definitions"""
    sh = F.SHAPES[sid]
    m, s = sh.m, F.sbits(sid)
    g = F.geometry(sid, qi)
    p = F.radius_plan(sh.bits, m, R)
    rt = F.table_radii(sh.bits, m, R)
    big = np.arange(m) <= p.ra
    inside = g.dist <= R
    ok = F.reach(sid, qi, R, False)
    n_reach = ok.sum(axis=1)
    assert np.array_equal(inside, inside & (n_reach > 0))          # the pigeonhole: masked keys reach everything inside R
    at_radius = ok & (g.sub == rt[None, :])
    kinds = set()
    if (g.dist == R).any():
        kinds.add("at R")
    if (g.dist == R + 1).any():
        kinds.add("at R + 1")
    one = inside & (n_reach == 1)
    if (one & (at_radius & big[None, :]).any(axis=1)).any():
        kinds.add("one big table at its radius")
    if p.rq >= 1 and (one & (at_radius & ~big[None, :]).any(axis=1)).any():
        kinds.add("one small table at its radius")
    if (inside & ((g.sub == p.rq) & ~big[None, :]).any(axis=1) & ~(ok & ~big[None, :]).any(axis=1)).any():
        kinds.add("small table at q, big table only")
    if (inside & (n_reach >= 2)).any():
        kinds.add("several tables")
    if p.rq == 0:
        zero_beyond = ((g.sub == 0) & ~big[None, :]).any(axis=1)
        if (zero_beyond & ~((g.sub == 0) & big[None, :]).any(axis=1) & ~inside).any():
            kinds.add("zero only beyond a: outside")
        if (zero_beyond & one).any():
            kinds.add("zero beyond a, one searched table: inside")
    if s < 32:
        ext = F.reach(sid, qi, R, True)
        if (inside & ~ext.any(axis=1)).any():
            kinds.add("lost under sign extension")
        first_min = g.sub.argmin(axis=1)
        rows = np.arange(sh.n)
        if (inside & ok[rows, first_min] & g.topdiff[rows, first_min] & ext.any(axis=1)).any():
            kinds.add("top bit differs in the first minimum, found through another table")
    return kinds


@pytest.mark.parametrize("sid", list(F.SHAPES))
def test_every_boundary_kind_is_present(sid):
    """around the first centre and around the centre whose substrings' top bits are set; each kind at some tested R whose plan the
    oracle test below enumerates; the exact-distance and several-table kinds at every tested R below the ball's end"""
    sh = F.SHAPES[sid]
    want = {"at R", "at R + 1", "one big table at its radius", "one small table at its radius", "small table at q, big table only",
            "several tables", "zero beyond a, one searched table: inside"}
    want.add("zero only beyond a: outside")
    if F.sbits(sid) < 32:
        want |= {"lost under sign extension", "top bit differs in the first minimum, found through another table"}
    for qi in (0, 5):
        found = {}
        for R in F.RADII[sid]:
            if F.radius_plan(sh.bits, sh.m, R).probes <= ORACLE_PROBES and F.uses_index(sh.bits, sh.m, sh.n, R):
                found[R] = _kinds(sid, qi, R)
                if R < sh.ball_to:
                    assert {"at R", "at R + 1"} <= found[R], (sid, qi, R)
        assert want <= set().union(*found.values()), (sid, qi, want - set().union(*found.values()))
        # shell 1 and shell 2 both hold the one-table kinds
        for shell in (1, 2):
            here = set().union(*(k for R, k in found.items() if R // sh.m == shell))
            assert {"one big table at its radius", "one small table at its radius", "small table at q, big table only"} <= here, (sid, qi, shell)


@pytest.mark.parametrize("sid", list(F.SHAPES))
def test_closed_form_equals_the_oracle(oracle, sid):
    """MihOracle.radius in both key modes over every (query, R) of the walk whose plan stays within ORACLE_PROBES, the deep ones
    included (shell 8 of 8-bit, shell 16 of 16-bit, the last index-side R of 32-bit substrings); with masked keys both equal the
    brute force dist <= R, and so does the closed form at every R however deep"""
    sh = F.SHAPES[sid]
    codes, q = F.make_codes(sid), F.make_queries(sid)
    ids = np.arange(sh.n, dtype=np.uint64) + np.uint64(sh.id_base)
    pinned = set()
    for key_mode in (0, 1):
        mo = oracle.MihOracle(codes, sh.m, key_mode=key_mode, id_base=sh.id_base)
        for R in F.RADII[sid]:
            p = F.radius_plan(sh.bits, sh.m, R)
            for qi in F.queries_at(sid, R):
                exp = F.closed_form(sid, qi, R, key_mode == 0)
                if key_mode == 1:
                    assert np.array_equal(exp, np.sort(oracle.pack(oracle.np_distances(codes, q[qi]), ids)[F.geometry(sid, qi).dist <= R]))
                    assert np.array_equal(exp, F.brute(sid, qi, R))
                if p.probes > ORACLE_PROBES:
                    continue
                got, probes = mo.radius(q[qi], p.R)                 # (the clamp to `bits` is the engine's)
                assert probes == p.probes, (sid, R)
                assert np.array_equal(got, exp), (sid, key_mode, R, qi)
                assert len(np.unique(exp & np.uint64(0xFFFFFFFF))) == len(exp)
                pinned.add(R)
        mo.close()
    deep = {R for R in F.RADII[sid] if F.uses_index(sh.bits, sh.m, sh.n, R)}
    assert pinned >= deep                                           # everything the index answers is pinned; the scan's radii are the brute force


@pytest.mark.parametrize("sid", [s for s in F.SHAPES if F.sbits(s) < 32])
def test_sign_extension_removes_results(sid):
    """below 32-bit substrings the flag loses neighbours at some tested R -- shallow and deep, for the plain centre and for the one
    whose keys are all negative -- and never adds one; in LINEAR mode it changes nothing"""
    sh = F.SHAPES[sid]
    for qi in (0, 5):
        lost = {R: len(F.closed_form(sid, qi, R, False)) - len(F.closed_form(sid, qi, R, True)) for R in F.RADII[sid] if qi in F.queries_at(sid, R)}
        assert all(v >= 0 for v in lost.values())
        assert any(v > 0 for R, v in lost.items() if R <= 2 * sh.m + 3) and any(v > 0 for R, v in lost.items() if R > 2 * sh.m + 3), (sid, qi, lost)
        for R in lost:
            assert set(F.closed_form(sid, qi, R, True).tolist()) <= set(F.closed_form(sid, qi, R, False).tolist())
            assert np.array_equal(F.expect(sid, "signext", "linear", R, qi), F.brute(sid, qi, R))
    assert len(F.expect(sid, "signext", "default", sh.bits, 0)) < sh.n        # even R = bits leaves records unreached


@pytest.mark.parametrize("sid", [s for s in F.SHAPES if F.sbits(s) == 32])
def test_sign_extension_is_the_identity_at_32_bits(sid):
    for R in F.RADII[sid]:
        for qi in range(F.NQ):
            assert np.array_equal(F.expect(sid, "signext+bitmap", "default", R, qi), F.expect(sid, "", "default", R, qi))


@pytest.mark.parametrize("sid", list(F.SHAPES))
def test_the_bitmap_has_both_answers(sid):
    """VC_FLAG_USE_BITMAP puts a bitmap test in front of every probe and must not change a row.  From 16-bit substrings on the
    queries probe set bits (the centres' own keys) and clear ones (the uniform query's key in some table, keys one flip away);
    at 8 bits and these sizes every one of the 256 keys of a table is taken, so the test always passes there."""
    sh = F.SHAPES[sid]
    s = F.sbits(sid)
    sub4, sub0 = F.geometry(sid, 4).sub, F.geometry(sid, 0).sub
    assert (sub0 == 0).any(axis=0).all()
    if s >= 16:
        assert not (sub4 == 0).any(axis=0).all()
    else:
        codes = F.make_codes(sid)
        assert all(len(np.unique(codes[:, t])) == 256 for t in range(sh.m))
    for R in F.RADII[sid][:4]:
        assert np.array_equal(F.expect(sid, "bitmap", "default", R, 0), F.expect(sid, "", "default", R, 0))


@pytest.mark.parametrize("sid,fl", F.SHARDED)
def test_sharded_expectation_is_the_union(sid, fl):
    """three shards of consecutive ordinals; every shard holds part of every ball, and the rows of the parts add up to the one
    engine's row wherever one engine and its shards agree on index or scan -- which at these sizes is everywhere"""
    sh = F.SHAPES[sid]
    ranges = F.split_ranges(sh.n, F.N_SHARDS)
    assert ranges[0][0] == 0 and sum(c for _, c in ranges) == sh.n
    for R in F.RADII[sid]:
        assert all(F.uses_index(sh.bits, sh.m, c, R) == F.uses_index(sh.bits, sh.m, sh.n, R) for _, c in ranges)
        for qi in F.queries_at(sid, R):
            assert np.array_equal(F.expect_sharded(sid, fl, R, qi), F.expect(sid, fl, "default", R, qi))
    R = 2 * sh.m
    parts = [len(F.expect(sid, fl, "default", R, 0, part)) for part in ranges]
    assert all(c > 0 for c in parts)
