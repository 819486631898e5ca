"""Pinned without a GPU, on the oracle alone (MihOracle.find = SearchWorker::find, search_worker.cc:159-264): the data of
test_flag_routes_gpu.py makes every reference-fidelity flag and every execution route matter, so that no GPU case there can
pass vacuously.  The conditions are the ones the GPU suite relies on; the figures observed with the committed seeds stand in
the docstrings."""
import numpy as np
import pytest

import flag_routes_common as F

SH = np.uint64(32)


def _stats(ex, field):
    return [e.stats[field] for e in ex]


RADIUS, N_RESULTS, N_SUB, N_LOCAL, N_CAND = range(5)


def test_every_cell_of_the_tables_is_a_case():
    """5 shapes x their flag sets x their routes = 76 cells (A 1 x 11, B 3 x 11, C 4 x 5, D 2 x 5, E 1 x 2), each once, and the
    flag values are the ABI's"""
    from verticut_amd import engine
    assert (F.BITMAP, F.SIGNEXT, F.LITERAL4) == (engine.FLAG_USE_BITMAP, engine.FLAG_REF_SIGNEXT_KEYS, engine.FLAG_REF_STOP_LITERAL4)
    cases = F.cases()
    ids = [F.case_id(c) for c in cases]
    assert len(cases) == 76 and len(set(ids)) == 76
    for sid in F.SHAPES:
        for fl in F.FLAG_SETS[sid]:
            for knob in ("default", "host_loop", "budget1", "bcodes0", "switch2") if sid != "E" else ("default", "host_loop"):
                assert (sid, fl, knob) in cases
            assert F.switch_forbidden(sid, fl)                         # every listed set keeps the scan switch off
    for sid in "AB":
        for fl in F.FLAG_SETS[sid]:
            for knob in ("group1", "group2", "group3", "lines1", "bent0", "bent0_lines1"):
                assert (sid, fl, knob) in cases
    assert all(set(F.ROUTES[r]) <= {"VC_MIH_HOST_LOOP", "VC_MIH_BUDGET", "VC_MIH_BCODES", "VC_MIH_SWITCH", "VC_MIH_GROUP", "VC_MIH_LINES",
                                    "VC_MIH_BENT"} for r in F.ROUTES)
    # the {id, code} records exist at 32-bit substrings of <= 128-bit codes only: the routes without them are listed for A and B alone
    assert F.ROUTES["bent0"] == {"VC_MIH_BENT": "0"} and F.ROUTES["bent0_lines1"] == {"VC_MIH_BENT": "0", "VC_MIH_LINES": "1"}
    assert {sid for sid, _, r in cases if r in ("bent0", "bent0_lines1")} == {"A", "B"}
    for sid in "AB":
        assert F.SHAPES[sid].bits // F.SHAPES[sid].m == 32 and F.SHAPES[sid].bits <= 128
    for sid in "CDE":
        assert "bent0" not in F.ROUTES_OF[sid] and "bent0_lines1" not in F.ROUTES_OF[sid]
    # a flag is listed only where it bites: signext below 32-bit substrings, literal4 below 4 tables
    for sid, sets in F.FLAG_SETS.items():
        sh = F.SHAPES[sid]
        for fl in sets:
            assert not (F.flag_bits(fl) & F.SIGNEXT) or sh.bits // sh.m < 32
            assert not (F.flag_bits(fl) & F.LITERAL4) or sh.m < 4 or F.flag_bits(fl) & F.SIGNEXT   # (VC_REF_QUIRKS sets both)
    assert F.oracle_settings("B", "literal4+bitmap") == (1, True, 4) and F.oracle_settings("B", "bitmap") == (1, True, 2)
    assert F.oracle_settings("C", "signext+literal4") == (0, False, 4) and F.oracle_settings("D", "signext", True) == (0, False, 4)


def test_queries_follow_the_recipe(oracle):
    """query i is a database item with FLIPS[i % 8] flipped bits, plus the top bit of substring 0 for every other query of a
    shape with substrings under 32 bits"""
    for sid, sh in F.SHAPES.items():
        codes, q = F.make_codes(oracle, sid), F.make_queries(oracle, sid)
        assert codes.shape == (sh.n, sh.bits // 8) and q.shape == (F.NQ, sh.bits // 8)
        s = sh.bits // sh.m
        base = q.copy()
        if s < 32:
            base[::2, s // 8 - 1] ^= 0x80
        for i in range(F.NQ):
            assert int(oracle.np_distances(codes, base[i]).min()) <= F.FLIPS[i % 8]


def test_shape_a_covers_every_shell_class_of_a_grouped_pass(oracle):
    """Exact radii [0,1,2,2,2,3,2,3,1,1,2,2,1,3,3,3]: shells 0, 1 and 2 are the classes of a pass grouped to depth 3
    (VC_MIH_GROUP=1..3), shell 3 lies behind it.  Approximate (k = 5): [0,1,2,2,2,1,2,3,1,1,2,2,2,2,3,3]."""
    for approx in (False, True):
        assert set(_stats(F.expect(oracle, "A", "bitmap", approx), RADIUS)) == {0, 1, 2, 3}


def test_shape_b_stops_earlier_under_the_literal_multiplier_and_is_handed_over(oracle):
    """Multiplier min(m, 4) = 2: radii [0,0,3,2,1,5,5,6,0,0,0,2,2,5,5,5]; the literal 4: [0,0,2,2,1,4,3,6,0,0,0,1,1,3,5,5], 6 of
    16 queries stop earlier (never later), and their rows are the worse ones of a smaller reach.  Radii 5-6 need 2 x 242 825
    probes and more, beyond any budget the query kernel is given for 16 queries: the hand-over happens without a knob."""
    two, four = F.expect(oracle, "B", "bitmap"), F.expect(oracle, "B", "literal4+bitmap")
    r2, r4 = _stats(two, RADIUS), _stats(four, RADIUS)
    assert max(r2) >= 5 and max(r4) >= 5
    assert all(b <= a for a, b in zip(r2, r4))
    assert sum(a != b for a, b in zip(r2, r4)) >= 4
    assert sum(a != b for a, b in zip(_stats(two, N_CAND), _stats(four, N_CAND))) >= 4
    assert _stats(F.expect(oracle, "B", "literal4"), RADIUS) == r4
    assert F.leaves(32, 5) == 242825


@pytest.mark.parametrize("sid,fl,approx", [("C", "signext", False), ("C", "signext", True), ("D", "signext", False), ("E", "signext+bitmap", False)])
def test_sign_extended_keys_change_what_a_query_reaches(oracle, sid, fl, approx):
    """key_mode 0 (binaryToInt's sign extension, Pilaf/image_tools.h:13) against masked keys, same stop rule.  Observed:
    C exact: rows of 5 queries, n_candidates of 12; C approximate: rows of 6, n_candidates of 10; D: n_candidates of 13, rows of
    none (the statistics are the witness); E: n_candidates of 11."""
    sh = F.SHAPES[sid]
    key_mode, use_bitmap, stop_mult = F.oracle_settings(sid, fl, approx)
    assert key_mode == 0
    ext = F.expect(oracle, sid, fl, approx)
    mo = oracle.MihOracle(F.make_codes(oracle, sid), sh.m, key_mode=1)
    differs = 0
    for i, q in enumerate(F.make_queries(oracle, sid)):
        ores, ost = mo.find(q, sh.k_approx if approx else sh.k, approximate=approx, use_bitmap=use_bitmap, stop_mult=stop_mult)
        differs += ost.n_distinct != ext[i].stats[N_CAND] or not np.array_equal(np.sort(ores) >> SH, ext[i].oracle_row >> SH)
    assert differs >= 4, differs


BITMAP_SETS = [(sid, fl, approx) for sid in F.SHAPES for fl in F.FLAG_SETS[sid] if F.flag_bits(fl) & F.BITMAP
               for approx in ((False, True) if F.SHAPES[sid].k_approx else (False,))]


@pytest.mark.parametrize("sid,fl,approx", BITMAP_SETS)
def test_bitmap_counters(oracle, sid, fl, approx):
    """with the bitmap attached (search_worker.cc:238-245) n_local_reads counts every leaf of shells 0..radius of table 0 and
    n_sub_reads the set bits among them -- fewer for at least one query (in fact for most); without it n_sub_reads is the
    leaf count and n_local_reads stays 0, and neither rows nor radius nor candidates depend on the bitmap"""
    sh = F.SHAPES[sid]
    s = sh.bits // sh.m
    ex = F.expect(oracle, sid, fl, approx)
    assert all(e.stats[N_LOCAL] == F.leaves(s, e.stats[RADIUS]) for e in ex)
    assert all(e.stats[N_SUB] <= e.stats[N_LOCAL] for e in ex) and any(e.stats[N_SUB] < e.stats[N_LOCAL] for e in ex)
    plain = "+".join(p for p in fl.split("+") if p != "bitmap")
    for e, p in zip(ex, F.expect(oracle, sid, plain, approx)):
        assert (p.stats[N_SUB], p.stats[N_LOCAL]) == (e.stats[N_LOCAL], 0)
        assert np.array_equal(e.row, p.row) and (e.stats[RADIUS], e.stats[N_CAND]) == (p.stats[RADIUS], p.stats[N_CAND])


def test_sign_extension_changes_the_bitmap_hits(oracle):
    """n_sub_reads under the bitmap with sign-extended keys against masked keys: C differs for 12 queries, E for 13"""
    c_ext, c_msk = F.expect(oracle, "C", "signext+literal4+bitmap"), F.expect(oracle, "C", "bitmap")
    assert sum(a.stats[N_SUB] != b.stats[N_SUB] for a, b in zip(c_ext, c_msk)) >= 4
    sh = F.SHAPES["E"]
    mo = oracle.MihOracle(F.make_codes(oracle, "E"), sh.m, key_mode=1)
    msk = [mo.find(q, sh.k, use_bitmap=True, stop_mult=4)[1].n_sub_reads for q in F.make_queries(oracle, "E")]
    assert sum(a.stats[N_SUB] != b for a, b in zip(F.expect(oracle, "E", "signext+bitmap"), msk)) >= 4


def test_the_canonical_rows_honour_the_contract(oracle):
    """the expectation the GPU rows are compared with bit for bit -- the k smallest (dist, id) among the items reachable
    within the oracle's radius -- has the oracle's distances and its ids below the k-th distance, for every flag set"""
    for sid, sh in F.SHAPES.items():
        for fl in F.FLAG_SETS[sid]:
            for approx in ((False, True) if sh.k_approx else (False,)):
                for e in F.expect(oracle, sid, fl, approx):
                    F.check_contract(e.row, e.oracle_row)
                    assert len(e.row) == e.stats[N_RESULTS] == (sh.k_approx if approx else sh.k)
                    assert np.all(e.row[1:] > e.row[:-1])


@pytest.mark.parametrize("sid,fl,shards", F.SHARDED)
def test_shards_stop_by_their_own_rule(oracle, sid, fl, shards):
    """The sharded expectation is not the single engine's: a shard holds a third or a quarter of every cluster, so it walks
    further (C on 3 shards: the radius grows for 4 queries; B on 4 shards: for all 16, up to shell 7) and the summed counters
    differ for every query.  The ranges are even, every shard holds more than k items, and the merged rows still honour
    the contract of the merged oracle rows."""
    sh = F.SHAPES[sid]
    ranges = F.split_ranges(sh.n, shards)
    assert ranges[0][0] == 0 and sum(c for _, c in ranges) == sh.n and all(c > sh.k for _, c in ranges)
    assert all(ranges[g][0] + ranges[g][1] == ranges[g + 1][0] for g in range(shards - 1))
    ex, one = F.expect_sharded(oracle, sid, fl, ranges), F.expect(oracle, sid, fl)
    assert all(a.stats[RADIUS] >= b.stats[RADIUS] for a, b in zip(ex, one))
    assert sum(a.stats[RADIUS] > b.stats[RADIUS] for a, b in zip(ex, one)) >= 4
    assert all(a.stats[N_LOCAL] > b.stats[N_LOCAL] for a, b in zip(ex, one))
    assert sum(a.stats[N_SUB] != b.stats[N_SUB] for a, b in zip(ex, one)) >= 4
    for e in ex:
        F.check_contract(e.row, e.oracle_row)
        assert len(e.row) == sh.k
