"""VC_FLAG_GLOBAL_APPROX: approximate MIH over id-range shards with the stop decision of ONE SearchWorker over the union (the
reference's master fills one heap of knn * APPROXIMATE_FACTOR distinct candidates from all ranks and broadcasts is_stop,
search_worker.cc:104-139).  Rows, counts and all six statistics fields equal one vc_engine holding the union, bit for bit; the
statistics equal the oracle's SearchWorker, the rows the canonical form (the k smallest packed values among the items whose
minimum substring distance is <= the radius).  All on one device.  What the data is made to exercise is pinned without a GPU
by test_sharded_global_approx_cpu.py."""
import contextlib
import os
import re
import subprocess

import numpy as np
import pytest

import sharded_global_approx_common as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _st(s):
    return (s.radius, s.n_results, s.n_main_reads, s.n_sub_reads, s.n_local_reads, s.n_candidates)


@contextlib.contextmanager
def _pair(vc, codes, bits, m, shards, id_base, flags=0, capacity=None):
    """the flagged store and one engine over the same records"""
    n = len(codes)
    with vc.ShardedEngine(bits, capacity=capacity or n, n_shards=shards, n_tables=m, devices=[0], id_base=id_base,
                          flags=vc.FLAG_GLOBAL_APPROX | flags) as s, \
            vc.Engine(bits, capacity=max(n, 1), n_tables=m, id_base=id_base, flags=flags) as one:
        for e in (s, one):
            if n:
                e.add_codes(codes)
            e.build_index()
        yield s, one


def _assert_same(vc, s, one, q, k, mode=None):
    """host form, both orders: rows, counts and statistics identical to the other engine's"""
    mode = vc.MODE_MIH_APPROX if mode is None else mode
    got, cnt, st = s.search_knn(q, k, mode=mode, with_stats=True)
    ref, rcnt, rst = one.search_knn(q, k, mode=mode, with_stats=True)
    assert np.array_equal(cnt, rcnt)
    assert np.array_equal(got, ref)
    assert [_st(x) for x in st] == [_st(x) for x in rst]
    far, fcnt = s.search_knn(q, k, mode=mode, order=vc.ORDER_FARTHEST_FIRST)
    rfar, _ = one.search_knn(q, k, mode=mode, order=vc.ORDER_FARTHEST_FIRST)
    assert np.array_equal(fcnt, rcnt) and np.array_equal(far, rfar)
    for i in range(len(q)):
        assert np.array_equal(far[i][:cnt[i]], got[i][:cnt[i]][::-1])
    return got, cnt, st


def _assert_oracle(oracle, mo, codes, q, k, m, id_base, got, cnt, st, rows=True):
    for i in range(len(q)):
        ores, ost = mo.find(q[i], k, approximate=True)
        assert (st[i].radius, st[i].n_sub_reads, st[i].n_candidates) == (ost.radius, ost.n_sub_reads, ost.n_distinct)
        assert np.array_equal(got[i][:cnt[i]] >> A.SH, np.sort(ores) >> A.SH)          # by distance: its tie order is not the contract
        if rows:
            assert np.array_equal(got[i][:cnt[i]], A.canonical(oracle, codes, q[i], k, st[i].radius, m, id_base))


@pytest.fixture(scope="module")
def clustered(oracle):
    """codes, queries and the oracle of every (bits, m) case, made once"""
    cache = {}

    def get(bits, m, key_mode=1):
        if (bits, m, key_mode) not in cache:
            codes, q = A.clustered_case(oracle, bits, m)
            cache[(bits, m, key_mode)] = (codes, q, oracle.MihOracle(codes, m, key_mode=key_mode, id_base=A.CLUSTERED_ID_BASE))
        return cache[(bits, m, key_mode)]
    return get


@pytest.mark.parametrize("bits,m,shards", [pytest.param(b, m, g, id="%d-%d-%d" % (b, m, g)) for g in A.CLUSTERED_SHARDS
                                           for b, m in A.CLUSTERED_SHAPES])
def test_equal_to_one_engine_over_the_union(vc, oracle, clustered, bits, m, shards):
    codes, q, mo = clustered(bits, m)
    with _pair(vc, codes, bits, m, shards, A.CLUSTERED_ID_BASE) as (s, one):
        for k in A.CLUSTERED_KS:
            got, cnt, st = _assert_same(vc, s, one, q, k)
            _assert_oracle(oracle, mo, codes, q, k, m, A.CLUSTERED_ID_BASE, got, cnt, st)


def test_sign_extended_keys(vc, oracle, clustered):
    """VC_FLAG_REF_SIGNEXT_KEYS is allowed: shards and union share the key function, whatever it cannot reach"""
    bits, m = 64, 4
    codes, q, mo = clustered(bits, m, key_mode=0)
    with _pair(vc, codes, bits, m, 3, A.CLUSTERED_ID_BASE, flags=vc.FLAG_REF_SIGNEXT_KEYS) as (s, one):
        for k in A.CLUSTERED_KS:
            got, cnt, st = _assert_same(vc, s, one, q, k)
            _assert_oracle(oracle, mo, codes, q, k, m, A.CLUSTERED_ID_BASE, got, cnt, st, rows=False)


@pytest.mark.parametrize("r_star,hit,place", A.CR_CASES, ids=["r%d-%s-%s" % (r, "hit" if h else "miss", p) for r, h, p in A.CR_CASES])
def test_crafted_thresholds(vc, oracle, r_star, hit, place):
    """the union's count reaches exactly 40 in shell r_star (the search stops there) or 39 (it goes one shell on), with the
    planted items in one shard, spread so that no shard reaches 40, or with a shard that reaches 40 by itself one shell later"""
    codes, planted = A.crafted(r_star, hit, place)
    q = A.crafted_query()
    mo = oracle.MihOracle(codes, A.CR_M, key_mode=1, id_base=A.CR_ID_BASE)
    with _pair(vc, codes, A.CR_BITS, A.CR_M, A.CR_SHARDS, A.CR_ID_BASE) as (s, one):
        got, cnt, st = _assert_same(vc, s, one, q, A.CR_K)
        _assert_oracle(oracle, mo, codes, q, A.CR_K, A.CR_M, A.CR_ID_BASE, got, cnt, st)
        assert st[0].radius == A.crafted_radius(r_star, hit)
        if hit:
            assert st[0].n_candidates == A.CR_STOP
        # two planted items tie at the k-th distance (in different shards unless everything is in one): the smaller id wins
        tie = sorted(A.CR_ID_BASE + planted[i][0] for i in (1, 2))
        assert cnt[0] == A.CR_K and int(got[0][1]) == (6 << 32) | tie[0]


def test_capped_run_leaves_by_both_ways(vc, oracle, monkeypatch, capfd):
    """A capped approximate run ends an open query in one of two places (vc_mih_search): in the hand-over, when the query kernel
    ran every shell of the cap, or in the commit of the cap's shell when that shell ran through the multi-block kernels.  One
    query gives the query kernel shells 0..2 at 128 / 4, so the rounds of a crafted case that stops in shell 4 take both: caps
    0..2 end in the hand-over (a kernel line with the query still open and no shell line behind it), caps 3 and 4 in the
    commit of shells 3 and 4.  VC_MIH_TRACE shows which; a change of the in-block budget that drops one way fails here."""
    codes, _ = A.crafted(3, False, "spread")                        # no shard stops by itself: every shard is open at every cap
    q = A.crafted_query()
    with vc.Engine(A.CR_BITS, capacity=A.CR_N, n_tables=A.CR_M, id_base=A.CR_ID_BASE) as one:
        one.add_codes(codes)
        one.build_index()
        ref, rcnt, rst = one.search_knn(q, A.CR_K, mode=vc.MODE_MIH_APPROX, with_stats=True)
        monkeypatch.setenv("VC_MIH_TRACE", "1")                     # read when an engine is created: the shards', not `one`'s
        with vc.ShardedEngine(A.CR_BITS, capacity=A.CR_N, n_shards=A.CR_SHARDS, n_tables=A.CR_M, devices=[0], id_base=A.CR_ID_BASE,
                              flags=vc.FLAG_GLOBAL_APPROX) as s:
            s.add_codes(codes)
            s.build_index()
            capfd.readouterr()
            got, cnt, st = s.search_knn(q, A.CR_K, mode=vc.MODE_MIH_APPROX, with_stats=True)
            err = capfd.readouterr().err
    assert np.array_equal(got, ref) and np.array_equal(cnt, rcnt) and [_st(x) for x in st] == [_st(x) for x in rst]
    assert st[0].radius == 4
    seen = []
    for ln in err.splitlines():
        kern = re.match(r"\[vc_mih\] shells 0\.\.(\d+) in the query kernel \(group \d+\): (\d+) queries, (\d+) continue", ln)
        shell = re.match(r"\[vc_mih\] shell r=(\d+) keys=\d+ active=(\d+) -> next=(\d+)", ln)
        if kern:
            seen.append(("kernel",) + tuple(int(x) for x in kern.groups()))
        elif shell:
            seen.append(("shell",) + tuple(int(x) for x in shell.groups()))
    G = A.CR_SHARDS
    want = []
    for t in range(5):                                              # the round capped at t, shard after shard
        one_shard = [("kernel", min(t, 2), 1, 1)]                   # shells 0..min(t, 2) in the block, the query still open
        one_shard += [("shell", r, 1, 1 if r < t else 0) for r in range(3, t + 1)]   # the cap's shell ends it (last_shell)
        want += one_shard * G
    assert seen == want


def test_never_reaching_20k(vc, oracle):
    """64 bit / 8 tables (S = 8): the loop ends after the last shell"""
    bits, m, id_base = 64, 8, 3
    rng = np.random.default_rng(8)
    codes = oracle.gen_codes(3000, bits, 6, kind=1, n_centres=40, max_flips=6)
    q = np.concatenate([A.near_queries(codes, rng, 6, 4), rng.integers(0, 256, size=(2, bits // 8), dtype=np.uint8)])
    # 1 500 records, k = 100: 2 000 candidates do not exist -- every query ends at S with full rows
    with _pair(vc, codes[:1500], bits, m, 3, id_base) as (s, one):
        got, cnt, st = _assert_same(vc, s, one, q, 100)
        assert all(x.radius == bits // m and x.n_candidates == 1500 for x in st) and np.all(cnt == 100)
        mo = oracle.MihOracle(codes[:1500], m, key_mode=1, id_base=id_base)
        _assert_oracle(oracle, mo, codes[:1500], q, 100, m, id_base, got, cnt, st)
    # a union smaller than k (7 records, capacity 50, 4 shards); empty trailing shards (3 000 records, capacity 12 000)
    for n_rec, cap, k in ((7, 50, 20), (3000, 12000, 20), (3000, 12000, 100)):
        with _pair(vc, codes[:n_rec], bits, m, 4, id_base, capacity=cap) as (s, one):
            got, cnt, st = _assert_same(vc, s, one, q, k)
            mo = oracle.MihOracle(codes[:n_rec], m, key_mode=1, id_base=id_base)
            _assert_oracle(oracle, mo, codes[:n_rec], q, k, m, id_base, got, cnt, st)
            if n_rec < k:
                assert all(x.radius == bits // m and x.n_candidates == n_rec for x in st) and np.all(cnt == n_rec)


def test_nothing_ingested(vc):
    """a store without records answers what the unflagged store answers"""
    bits, m, k = 64, 8, 5
    q = np.random.default_rng(2).integers(0, 256, size=(3, bits // 8), dtype=np.uint8)
    with vc.ShardedEngine(bits, capacity=100, n_shards=4, n_tables=m, devices=[0], flags=vc.FLAG_GLOBAL_APPROX) as a, \
            vc.ShardedEngine(bits, capacity=100, n_shards=4, n_tables=m, devices=[0]) as b:
        for s in (a, b):
            s.build_index()
        _assert_same(vc, a, b, q, k)
        assert np.all(a.search_knn(q, k, mode=vc.MODE_MIH_APPROX)[1] == 0)


def _stats_array(t):
    raw = t.cpu().numpy().view(np.uint8).reshape(-1, 40)
    return [tuple(int(x) for x in r[:8].view(np.uint32)) + tuple(int(x) for x in r[8:].view(np.uint64)) for r in raw]


def test_device_form_equals_host_form(vc, oracle, clustered):
    import torch
    bits, m, k = 128, 4, 5
    codes, q, _ = clustered(bits, m)
    nq = len(q)
    with vc.ShardedEngine(bits, capacity=len(codes), n_shards=8, n_tables=m, devices=[0], id_base=9, flags=vc.FLAG_GLOBAL_APPROX) as s:
        s.add_codes(codes)
        s.build_index()
        href, hcnt, hst = s.search_knn(q, k, mode=vc.MODE_MIH_APPROX, with_stats=True)
        want_st = [_st(x) for x in hst]
        assert len({x.radius for x in hst}) > 1                     # the queries of a call settle in different rounds
        dq = torch.from_numpy(q).cuda()
        dq2 = torch.from_numpy(q[::-1].copy()).cuda()
        side = torch.cuda.Stream()

        def call(dqueries, stream, counts=True, stats=True):
            out = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
            cnt = torch.zeros((nq,), dtype=torch.int32, device="cuda") if counts else None
            stat = torch.zeros((nq, 5), dtype=torch.int64, device="cuda") if stats else None
            with torch.cuda.stream(stream):
                s.search_knn_dev(dqueries.data_ptr(), nq, k, out.data_ptr(), cnt.data_ptr() if counts else None,
                                 d_stats=stat.data_ptr() if stats else None, mode=vc.MODE_MIH_APPROX, stream=stream.cuda_stream)
            stream.synchronize()
            return (out.cpu().numpy().view(np.uint64), cnt.cpu().numpy().view(np.uint32) if counts else None,
                    _stats_array(stat) if stats else None)

        for stream in (torch.cuda.current_stream(), side):
            for counts, stats in ((True, True), (True, False), (False, True), (False, False)):
                out, cnt, st = call(dq, stream, counts, stats)
                assert np.array_equal(out, href)
                assert cnt is None or np.array_equal(cnt, hcnt)
                assert st is None or st == want_st
        # two calls back to back, then the first repeated: same bits
        first = call(dq, side)
        second = call(dq2, side)
        again = call(dq, side)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and first[2] == again[2]
        assert np.array_equal(second[0], href[::-1]) and np.array_equal(second[1], hcnt[::-1]) and second[2] == want_st[::-1]


def test_flags(vc, oracle, clustered):
    G, A_ = vc.FLAG_GLOBAL_STOP, vc.FLAG_GLOBAL_APPROX
    for bits, n_tables, flags in ((128, 0, 0), (128, 4, vc.FLAG_USE_BITMAP), (128, 4, vc.FLAG_USE_BITMAP | G)):
        with pytest.raises(vc.VcError) as ei:
            vc.ShardedEngine(bits, capacity=1000, n_shards=2, n_tables=n_tables, devices=[0], flags=A_ | flags)
        assert ei.value.code == vc.VC_ERR_INVALID
    for flags in (vc.FLAG_REF_SIGNEXT_KEYS, vc.FLAG_REF_STOP_LITERAL4, G):
        with vc.ShardedEngine(64, capacity=1000, n_shards=2, n_tables=4, devices=[0], flags=A_ | flags):
            pass
    # k = 3: every shard of four finds its own 60 candidates by shell 4, and where it stops differs from the union's stop
    # (the model of sharded_global_approx_common.py: radius or summed candidates differ for 9 of the 10 near queries)
    bits, m, k = 128, 4, 3
    codes, q, _ = clustered(bits, m)
    q = np.concatenate([q, np.random.default_rng(5).integers(0, 256, size=(2, bits // 8), dtype=np.uint8)])

    def store(flags):
        s = vc.ShardedEngine(bits, capacity=len(codes), n_shards=4, n_tables=m, devices=[0], flags=flags)
        s.add_codes(codes)
        s.build_index()
        return s

    with store(0) as plain, store(G) as gs, store(A_) as ga, store(A_ | G) as both, \
            vc.Engine(bits, capacity=len(codes), n_tables=m, flags=A_) as flagged_one, vc.Engine(bits, capacity=len(codes), n_tables=m) as one:
        for e in (flagged_one, one):
            e.add_codes(codes)
            e.build_index()
        near = q[:A.CLUSTERED_NQ]
        for mode in (vc.MODE_LINEAR, vc.MODE_MIH_EXACT):
            _assert_same(vc, flagged_one, one, q, k, mode)          # a plain engine ignores the flag
        _assert_same(vc, flagged_one, one, near, k, vc.MODE_MIH_APPROX)
        _assert_same(vc, gs, plain, near, k, vc.MODE_MIH_APPROX)    # without the new flag MIH_APPROX is as it was
        _, _, pst = plain.search_knn(near, k, mode=vc.MODE_MIH_APPROX, with_stats=True)
        _, _, ost = one.search_knn(near, k, mode=vc.MODE_MIH_APPROX, with_stats=True)
        stop = lambda st: [(x.radius, x.n_candidates) for x in st]  # (the summed n_sub_reads would differ whatever the shards do)
        assert sum(a != b for a, b in zip(stop(pst), stop(ost))) >= 5   # ... which is not where one engine stops
        _assert_same(vc, ga, one, near, k, vc.MODE_MIH_APPROX)
        _assert_same(vc, both, one, near, k, vc.MODE_MIH_APPROX)
        for mode in (vc.MODE_LINEAR, vc.MODE_MIH_EXACT):            # the other searches do not look at the new flag
            _assert_same(vc, ga, plain, q, k, mode)
        _assert_same(vc, both, gs, q, k, vc.MODE_MIH_EXACT)
        for mode in (vc.MODE_LINEAR, vc.MODE_MIH_EXACT):
            want = plain.search_radius(q, 12, mode=mode)
            for s in (ga, both):
                have = s.search_radius(q, 12, mode=mode)
                assert all(np.array_equal(x, y) for x, y in zip(have, want))
        import torch
        dq = torch.from_numpy(q).cuda()
        res = []
        for s in (plain, ga):
            offs = torch.zeros((len(q) + 1,), dtype=torch.int64, device="cuda")
            out = torch.zeros((4096,), dtype=torch.int64, device="cuda")
            stream = torch.cuda.current_stream()
            assert s.search_radius_dev(dq.data_ptr(), len(q), 12, out.data_ptr(), out.numel(), offs.data_ptr(),
                                       mode=vc.MODE_MIH_EXACT, stream=stream.cuda_stream) == vc.VC_OK
            stream.synchronize()
            o = offs.cpu().numpy()
            res.append((o, out.cpu().numpy()[:o[-1]]))
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


def test_routing_evidence(vc, oracle, clustered, monkeypatch, capfd):
    """under VC_MIH_GS_TRACE the flagged call prints one [vc_ga] line per round, caps 0, 1, 2, .. up to the batch's largest radius;
    the unflagged store prints none"""
    monkeypatch.setenv("VC_MIH_GS_TRACE", "1")                      # read when a sharded store is created
    bits, m, k = 128, 4, 1
    codes, q, _ = clustered(bits, m)
    line = re.compile(r"^\[vc_ga\] round (\d+): (\d+) open -> (\d+) open  [\d.]+ us$", flags=re.M)
    for flags in (vc.FLAG_GLOBAL_APPROX, 0):
        with vc.ShardedEngine(bits, capacity=len(codes), n_shards=4, n_tables=m, devices=[0], flags=flags) as s:
            s.add_codes(codes)
            s.build_index()
            capfd.readouterr()
            _, _, st = s.search_knn(q, k, mode=vc.MODE_MIH_APPROX, with_stats=True)
            rounds = [tuple(int(x) for x in r) for r in line.findall(capfd.readouterr().err)]
        if not flags:
            assert rounds == []
            continue
        assert [r[0] for r in rounds] == list(range(len(rounds)))
        assert rounds[0][1] == len(q) and rounds[-1][2] == 0
        assert all(a[2] == b[1] for a, b in zip(rounds, rounds[1:]))
        assert rounds[-1][0] == max(x.radius for x in st)
        for t, n_in, n_out in rounds:                               # a round settles the queries whose radius is its cap
            assert n_in - n_out == sum(x.radius == t for x in st)


def test_driver_prints_one_search_worker(vc, oracle, tmp_path):
    """distributed-image-search in approximate mode with VC_SHARDS=3 VC_GLOBAL_APPROX=1 prints what the one-engine run prints"""
    driver = os.path.join(ROOT, "verticut_amd", "bin", "distributed-image-search")
    n, bits, m, k = 30000, 128, 4, 5
    rng = np.random.default_rng(5)
    codes = oracle.gen_codes(n, bits, 34, kind=1, n_centres=150, max_flips=8)
    q = codes[rng.integers(0, n, size=6)].copy()
    q[:, 3] ^= 0x12
    (tmp_path / "lsh.code").write_bytes(codes.tobytes())
    (tmp_path / "query.code").write_bytes(q.tobytes())
    args = [driver, str(tmp_path / "lsh.code"), str(n), str(bits), str(bits // m), str(k), "pilaf", "0", "1", "-1",
            str(tmp_path / "query.code")]

    def run(**extra):
        env = {key: v for key, v in os.environ.items() if key not in ("VC_SHARDS", "VC_GLOBAL_STOP", "VC_GLOBAL_APPROX", "VC_REF_QUIRKS")}
        env.update(VC_PRINT_RESULTS="1", VC_DEVICES="0", **extra)
        p = subprocess.run(args, capture_output=True, text=True, timeout=300, env=env)
        return p.returncode, [ln for ln in p.stdout.splitlines() if not ln.startswith("while :")], p.stderr

    rc1, one, err1 = run()
    rc3, sharded, err3 = run(VC_SHARDS="3", VC_GLOBAL_APPROX="1")
    assert rc1 == 0 and rc3 == 0, err1 + err3
    assert len(re.findall(r"^query \d+$", "\n".join(one), flags=re.M)) == len(q)
    assert sharded == one
    rc, quirks, err = run(VC_SHARDS="3", VC_GLOBAL_APPROX="1", VC_REF_QUIRKS="1")
    rc1q, one_q, err1q = run(VC_REF_QUIRKS="1")
    assert rc == 0 and rc1q == 0 and quirks == one_q, err + err1q   # the reference's quirks do not break the argument
