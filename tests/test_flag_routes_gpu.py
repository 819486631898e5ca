"""The reference-fidelity flags on every MIH execution route.  VC_FLAG_USE_BITMAP, VC_FLAG_REF_SIGNEXT_KEYS and
VC_FLAG_REF_STOP_LITERAL4 are read in the multi-block probe kernel, in the query kernel's owner rule, granule scan and
direct-key scan, in both statistics exports, in the planner's scan-switch decision and in the sharded statistics reduction;
the routes (VC_MIH_HOST_LOOP, VC_MIH_BUDGET, VC_MIH_BCODES, VC_MIH_SWITCH, VC_MIH_GROUP, VC_MIH_LINES, VC_MIH_BENT) decide which of these
places a query passes.  Every (shape, flag set, route) cell of flag_routes_common.py builds one engine and serves 16 queries in
exact and approximate mode, through the host-pointer and the device-resident call; every query is compared with
MihOracle.find (SearchWorker::find, search_worker.cc:159-264) -- never with another GPU route.  test_flag_routes_cpu.py pins on
the same data that each flag changes radii, rows or counters there, and that the radii cover the shells the routes differ in."""
import numpy as np
import pytest

import flag_routes_common as F

pytestmark = pytest.mark.gpu


def _host_stats(st):
    return [(s.radius, s.n_results, s.n_main_reads, s.n_sub_reads, s.n_local_reads, s.n_candidates) for s in st]


def _dev_stats(t):
    """device buffer of 40-byte vc_query_stats records -> (radius, n_results, n_main_reads, n_sub_reads, n_local_reads, n_candidates)"""
    raw = t.cpu().numpy().view(np.uint8).reshape(-1, 40)
    out = []
    for r in raw:
        u32, u64 = r[:8].view(np.uint32), r[8:].view(np.uint64)
        out.append((int(u32[0]), int(u32[1]), int(u64[0]), int(u64[1]), int(u64[2]), int(u64[3])))
    return out


def _check(got, cnt, stats, expected, where):
    """rows, counts and statistics of one call against the oracle's, query by query"""
    assert len(expected) == len(got) == len(cnt) == len(stats)
    for i, ex in enumerate(expected):
        radius, n_results, n_sub, n_local, n_cand = ex.stats
        g = got[i, : cnt[i]]
        assert cnt[i] == n_results, (where, i)
        F.check_contract(g, ex.oracle_row)                        # distance multiset + id set below the k-th distance
        assert np.array_equal(g, ex.row), (where, i)              # the whole row: the canonical tie rule within the oracle's radius
        assert np.all(got[i, cnt[i]:] == np.uint64(0xFFFFFFFFFFFFFFFF)), (where, i)
        assert stats[i] == (radius, n_results, 0, n_sub, n_local, n_cand), (where, i, stats[i], ex.stats)


def _search_dev(torch, h, q, k, mode, sharded=False):
    """the device-resident call on torch's current stream: (rows, counts, statistics)"""
    nq = len(q)
    dq = torch.from_numpy(np.array(q)).cuda()                   # (a copy: the shared queries are read-only)
    out = torch.full((nq, k), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    cnt = torch.full((nq,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    stat = torch.full((nq, 5), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if sharded:
        h.search_knn_dev(dq.data_ptr(), nq, k, out.data_ptr(), cnt.data_ptr(), d_stats=stat.data_ptr(), mode=mode, stream=stream)
    else:
        h.search_knn_dev_stats(dq.data_ptr(), nq, k, out.data_ptr(), cnt.data_ptr(), stat.data_ptr(), mode=mode, stream=stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64), cnt.cpu().numpy().view(np.uint32), _dev_stats(stat)


def _legs(vc, sh):
    return [(vc.MODE_MIH_EXACT, sh.k, False)] + ([(vc.MODE_MIH_APPROX, sh.k_approx, True)] if sh.k_approx else [])


@pytest.mark.parametrize("case", F.cases(), ids=F.case_id)
def test_flag_set_on_route(vc, oracle, monkeypatch, case):
    import torch
    sid, fl, route = case
    sh = F.SHAPES[sid]
    for name, value in F.ROUTES[route].items():                   # the knobs are read at vc_create
        monkeypatch.setenv(name, value)
    codes, q = F.make_codes(oracle, sid), F.make_queries(oracle, sid)
    with vc.Engine(sh.bits, capacity=sh.n, n_tables=sh.m, flags=F.flag_bits(fl)) as e:
        e.add_codes(codes)
        e.build_index()
        e.timing()                                                # the witnesses below count the MIH calls alone
        for mode, k, approx in _legs(vc, sh):
            expected = F.expect(oracle, sid, fl, approx)
            got, cnt, st = e.search_knn(q, k, mode=mode, with_stats=True)
            _check(got, cnt, _host_stats(st), expected, (case, "host", approx))
            dgot, dcnt, dst = _search_dev(torch, e, q, k, mode)
            assert np.array_equal(dgot, got) and np.array_equal(dcnt, cnt), (case, approx)
            assert dst == _host_stats(st), (case, approx)
        t = e.timing()
    radii = [ex.stats[0] for ex in F.expect(oracle, sid, fl)]
    # route witnesses.  mih_launches counts the launches of mih_query_kernel (timed_query_launch; the multi-block probe
    # kernels are not counted), scan_launches the verify kernel's
    if route == "host_loop":
        assert t.mih_launches == 0 and max(radii) >= 1            # every shell went through the multi-block kernels
    else:
        assert t.mih_launches >= 1 and t.mih_queries > 0 and t.mih_probes > 0
    if route == "budget1":
        assert max(radii) >= 1                                    # some query left the query kernel after shell 0
    if route == "switch2":
        assert F.switch_forbidden(sid, fl) and t.scan_launches == 0   # quirks and bitmap counters keep the radius loop


@pytest.mark.parametrize("sid", ["A", "B"])
def test_forced_switch_takes_these_queries_when_no_flag_forbids_it(vc, oracle, monkeypatch, sid):
    """The counterpart of the switch2 cases above: the same data without a flag under VC_MIH_SWITCH=2 does reach the scan
    switch (the queries beyond the query kernel's shells are answered by the verify kernel, stop rule replayed), so
    scan_launches == 0 in a flagged case is the planner's decision and not a lack of opportunity."""
    sh = F.SHAPES[sid]
    monkeypatch.setenv("VC_MIH_SWITCH", "2")
    with vc.Engine(sh.bits, capacity=sh.n, n_tables=sh.m) as e:
        e.add_codes(F.make_codes(oracle, sid))
        e.build_index()
        e.timing()
        got, cnt, st = e.search_knn(F.make_queries(oracle, sid), sh.k, mode=vc.MODE_MIH_EXACT, with_stats=True)
        t = e.timing()
    assert not F.switch_forbidden(sid, "") and t.scan_launches >= 1
    _check(got, cnt, _host_stats(st), F.expect(oracle, sid, ""), (sid, "switch2 without flags"))


@pytest.mark.parametrize("sid,fl,shards,route", [pytest.param(s, f, g, "default", id="-".join((s, f, "%dshards" % g))) for s, f, g in F.SHARDED]
                         + [pytest.param("B", "literal4+bitmap", 4, "bent0", id="B-literal4+bitmap-4shards-bent0")])
def test_flag_set_over_shards(vc, oracle, monkeypatch, sid, fl, shards, route):
    """Each shard stops by its own rule, so the expectation is one MihOracle per shard's id range: rows = the k smallest of
    the shards' rows, radius = the maximum, n_sub_reads / n_local_reads / n_candidates = the sums (vc_sharded_stats_kernel),
    through the host-pointer and the device-resident call.  The bent0 case: every shard without its {id, code} records."""
    import torch
    sh = F.SHAPES[sid]
    assert (sid, fl, shards) in F.SHARDED
    for name, value in F.ROUTES[route].items():                   # the knobs are read when the store is created
        monkeypatch.setenv(name, value)
    q = F.make_queries(oracle, sid)
    with vc.ShardedEngine(sh.bits, capacity=sh.n, n_shards=shards, n_tables=sh.m, devices=[0], flags=F.flag_bits(fl)) as s:
        s.add_codes(F.make_codes(oracle, sid))
        s.build_index()
        ranges = [s.shard_range(g) for g in range(shards)]
        assert ranges == F.split_ranges(sh.n, shards)             # the ranges test_flag_routes_cpu.py pins
        expected = F.expect_sharded(oracle, sid, fl, ranges)
        got, cnt, st = s.search_knn(q, sh.k, mode=vc.MODE_MIH_EXACT, with_stats=True)
        _check(got, cnt, _host_stats(st), expected, (sid, fl, shards, "host"))
        dgot, dcnt, dst = _search_dev(torch, s, q, sh.k, vc.MODE_MIH_EXACT, sharded=True)
        _check(dgot, dcnt, dst, expected, (sid, fl, shards, "dev"))
