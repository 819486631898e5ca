"""VC_FLAG_GLOBAL_STOP: exact MIH over id-range shards with the stop decision of ONE SearchWorker over the union (the
reference's master tests the merged heap and broadcasts is_stop, search_worker.cc:179-207).  Rows, counts and all five
statistics equal one vc_engine holding the union, and the oracle's SearchWorker; all on one device."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SH = np.uint64(32)


def _queries(codes, rng, nq, flips):
    q = codes[rng.integers(0, codes.shape[0], size=nq)].copy()
    for i in range(nq):
        for b in rng.choice(codes.shape[1] * 8, size=int(rng.integers(0, flips + 1)), replace=False):
            q[i, b // 8] ^= np.uint8(1 << (b % 8))
    return q


def _canonical(oracle, codes, q, k, radius, m, id_base):
    """the k smallest (dist, id) among the items whose minimum substring distance is <= radius"""
    d = oracle.np_distances(codes, q)
    ids = np.nonzero(oracle.np_sub_distances(codes, q, m).min(axis=1) <= radius)[0]
    return np.sort(oracle.pack(d[ids], ids.astype(np.uint64) + np.uint64(id_base)))[:k]


def _st(s):
    return (s.radius, s.n_results, s.n_main_reads, s.n_sub_reads, s.n_local_reads, s.n_candidates)


def _assert_same(vc, s, one, q, k):
    """host form, both orders: rows, counts and statistics identical to the single engine's"""
    got, cnt, st = s.search_knn(q, k, mode=vc.MODE_MIH_EXACT, with_stats=True)
    ref, rcnt, rst = one.search_knn(q, k, mode=vc.MODE_MIH_EXACT, with_stats=True)
    assert np.array_equal(cnt, rcnt)
    assert np.array_equal(got, ref)
    assert [_st(x) for x in st] == [_st(x) for x in rst]
    far, fcnt = s.search_knn(q, k, mode=vc.MODE_MIH_EXACT, order=vc.ORDER_FARTHEST_FIRST)
    rfar, _ = one.search_knn(q, k, mode=vc.MODE_MIH_EXACT, order=vc.ORDER_FARTHEST_FIRST)
    assert np.array_equal(fcnt, rcnt) and np.array_equal(far, rfar)
    return got, cnt, st


# one more 128-bit / 4-table case without the {id, code} records (VC_MIH_BENT=0: every shard and the single engine verify through
# the id gather, as an index does when memory is short); the cases that had no such parameter keep their ids
@pytest.mark.parametrize("bits,m,shards,bent", [pytest.param(b, m, g, None, id="%d-%d-%d" % (b, m, g)) for g in (1, 3, 8)
                                                for b, m in ((128, 4), (64, 2), (256, 8), (64, 4))]
                         + [pytest.param(128, 4, 3, "0", id="128-4-3-bent0")])
def test_equal_to_one_engine_over_the_union(vc, oracle, monkeypatch, bits, m, shards, bent):
    if bent is not None:
        monkeypatch.setenv("VC_MIH_BENT", bent)                         # read when an engine or a sharded store is created
    n, id_base = 20_000, 1234
    rng = np.random.default_rng(bits * 10 + m + shards)
    codes = oracle.gen_codes(n, bits, 7, kind=1, n_centres=60, max_flips=bits // 16)
    near = _queries(codes, rng, 10, bits // 16)
    q = np.concatenate([near, rng.integers(0, 256, size=(3, bits // 8), dtype=np.uint8)])
    mo = oracle.MihOracle(codes, m, key_mode=1, id_base=id_base)
    with vc.ShardedEngine(bits, capacity=n, n_shards=shards, n_tables=m, devices=[0], id_base=id_base,
                          flags=vc.FLAG_GLOBAL_STOP) as s, vc.Engine(bits, capacity=n, n_tables=m, id_base=id_base) as one:
        s.add_codes(codes)
        s.build_index()
        one.add_codes(codes)
        one.build_index()
        for k in (1, 20, 100):
            got, cnt, st = _assert_same(vc, s, one, q, k)
            for i in range(len(q)):
                assert np.array_equal(got[i][:cnt[i]], _canonical(oracle, codes, q[i], k, st[i].radius, m, id_base))
            for i in range(len(near)):      # the oracle's SearchWorker (the uniform queries walk too many shells for it)
                ost = mo.find(q[i], k, stop_mult=min(m, 4))[1]
                assert (st[i].radius, st[i].n_sub_reads, st[i].n_candidates) == (ost.radius, ost.n_sub_reads, ost.n_distinct)


def _stats_array(t):
    raw = t.cpu().numpy().view(np.uint8).reshape(-1, 40)
    return [tuple(int(x) for x in r[:8].view(np.uint32)) + tuple(int(x) for x in r[8:].view(np.uint64)) for r in raw]


def test_device_form_equals_host_form(vc, oracle):
    import torch
    n, bits, m, k = 30_000, 128, 4, 50
    rng = np.random.default_rng(3)
    codes = oracle.gen_codes(n, bits, 11, kind=1, n_centres=100, max_flips=8)
    q = np.concatenate([_queries(codes, rng, 14, 8), rng.integers(0, 256, size=(2, bits // 8), dtype=np.uint8)])
    nq = len(q)
    with vc.ShardedEngine(bits, capacity=n, n_shards=8, n_tables=m, devices=[0], id_base=9, flags=vc.FLAG_GLOBAL_STOP) as s:
        s.add_codes(codes)
        s.build_index()
        href, hcnt, hst = s.search_knn(q, k, mode=vc.MODE_MIH_EXACT, with_stats=True)
        dq = torch.from_numpy(q).cuda()
        side = torch.cuda.Stream()
        for stream in (torch.cuda.current_stream(), side):
            out = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
            cnt = torch.zeros((nq,), dtype=torch.int32, device="cuda")
            stat = torch.zeros((nq, 5), dtype=torch.int64, device="cuda")
            with torch.cuda.stream(stream):
                s.search_knn_dev(dq.data_ptr(), nq, k, out.data_ptr(), cnt.data_ptr(), d_stats=stat.data_ptr(),
                                 mode=vc.MODE_MIH_EXACT, stream=stream.cuda_stream)
            stream.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint64), href)
            assert np.array_equal(cnt.cpu().numpy().view(np.uint32), hcnt)
            assert _stats_array(stat) == [(x.radius, x.n_results, x.n_main_reads, x.n_sub_reads, x.n_local_reads, x.n_candidates)
                                          for x in hst]


def _crafted(bits, m, items, n_fill, seed):
    """uniform filler, then codes whose substrings differ from the all-zero query in the given numbers of bits"""
    nb, sb = bits // 8, bits // 8 // m
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, size=(n_fill, nb), dtype=np.uint8)
    for pos, subs in items:
        c = np.zeros(nb, dtype=np.uint8)
        for t, b in enumerate(subs):
            word = np.zeros(sb * 8, dtype=np.uint8)
            word[:b] = 1
            c[t * sb:(t + 1) * sb] = np.packbits(word, bitorder="little")
        codes[pos] = c
    return codes


@pytest.mark.parametrize("r0", [2, 6])            # 2: decided by a capped confirm round; 6: by the union scan
@pytest.mark.parametrize("early", [True, False])
def test_ties_at_the_threshold(vc, oracle, r0, early):
    """D = m r0: the union loop stops at r0 - 1 when the items below D plus the ties at D with a substring below r0 make k"""
    bits, m, k, n, shards, id_base = 128, 4, 4, 3000, 3, 100
    below = [(5, (1, 0, 0, 0)), (1500, (0, 1, 0, 0))]
    flat = [(10, (r0,) * 4), (999, (r0,) * 4), (1000, (r0,) * 4)]     # every substring at r0: only shell r0 sees them
    low = [(1999, (r0 - 1, r0, r0, r0 + 1)), (2000, (r0, r0 - 1, r0 + 1, r0)), (2500, (r0 + 1, r0, r0, r0 - 1))]
    codes = _crafted(bits, m, below + flat + (low if early else low[:1]), n, seed=r0)
    q = np.zeros((1, bits // 8), dtype=np.uint8)
    with vc.ShardedEngine(bits, capacity=n, n_shards=shards, n_tables=m, devices=[0], id_base=id_base,
                          flags=vc.FLAG_GLOBAL_STOP) as s, vc.Engine(bits, capacity=n, n_tables=m, id_base=id_base) as one:
        s.add_codes(codes)
        s.build_index()
        one.add_codes(codes)
        one.build_index()
        got, cnt, st = _assert_same(vc, s, one, q, k)
        ost = oracle.MihOracle(codes, m, key_mode=1, id_base=id_base).find(q[0], k, stop_mult=4)[1]
        assert (st[0].radius, st[0].n_sub_reads, st[0].n_candidates) == (ost.radius, ost.n_sub_reads, ost.n_distinct)
        assert st[0].radius == (r0 - 1 if early else r0)
        assert np.array_equal(got[0], _canonical(oracle, codes, q[0], k, st[0].radius, m, id_base))
        lin, _ = s.search_knn(q, k)
        assert np.array_equal(got[0], lin[0]) != early        # the early stop returns other ties than LINEAR


def test_routing_evidence(vc, oracle):
    """near-duplicate queries the single engine stops at radius <= 1 launch no verify kernel on any shard; uniform queries
    reach the union scan"""
    n, bits, m, k, shards = 40_000, 128, 4, 10, 8
    rng = np.random.default_rng(21)
    codes = oracle.gen_codes(n, bits, 5, kind=1, n_centres=200, max_flips=4)
    q = _queries(codes, rng, 64, 2)
    with vc.ShardedEngine(bits, capacity=n, n_shards=shards, n_tables=m, devices=[0], flags=vc.FLAG_GLOBAL_STOP) as s, \
            vc.Engine(bits, capacity=n, n_tables=m) as one:
        s.add_codes(codes)
        s.build_index()
        one.add_codes(codes)
        one.build_index()
        _, _, rst = one.search_knn(q, k, mode=vc.MODE_MIH_EXACT, with_stats=True)
        assert max(x.radius for x in rst) <= 1
        for g in range(shards):
            s.shard(g).timing()                                         # reset
        _assert_same(vc, s, one, q, k)
        assert all(s.shard(g).timing().scan_launches == 0 for g in range(shards))
        u = rng.integers(0, 256, size=(4, bits // 8), dtype=np.uint8)
        _assert_same(vc, s, one, u, k)
        assert sum(s.shard(g).timing().scan_launches for g in range(shards)) > 0


def test_refused_combinations(vc):
    for bits, n_tables, flags in ((128, 0, 0), (128, 4, vc.FLAG_REF_SIGNEXT_KEYS), (64, 2, vc.FLAG_REF_STOP_LITERAL4),
                                  (128, 4, vc.FLAG_USE_BITMAP)):
        with pytest.raises(vc.VcError) as ei:
            vc.ShardedEngine(bits, capacity=1000, n_shards=2, n_tables=n_tables, devices=[0], flags=vc.FLAG_GLOBAL_STOP | flags)
        assert ei.value.code == vc.VC_ERR_INVALID
    with vc.ShardedEngine(128, capacity=1000, n_shards=2, n_tables=4, devices=[0], flags=vc.FLAG_GLOBAL_STOP | vc.FLAG_REF_STOP_LITERAL4):
        pass                                                            # the literal 4 with 4 tables is min(m, 4): exact
    with vc.Engine(128, capacity=1000, n_tables=4, flags=vc.FLAG_GLOBAL_STOP):
        pass                                                            # a plain engine accepts and ignores it


def test_other_modes_unchanged_and_small_unions(vc, oracle):
    bits, m, k = 128, 4, 20
    rng = np.random.default_rng(4)
    codes = oracle.gen_codes(5000, bits, 6, kind=1, n_centres=40, max_flips=6)
    q = np.concatenate([_queries(codes, rng, 6, 4), rng.integers(0, 256, size=(2, bits // 8), dtype=np.uint8)])
    with vc.ShardedEngine(bits, capacity=5000, n_shards=4, n_tables=m, devices=[0], flags=vc.FLAG_GLOBAL_STOP) as a, \
            vc.ShardedEngine(bits, capacity=5000, n_shards=4, n_tables=m, devices=[0]) as b:
        for s in (a, b):
            s.add_codes(codes)
            s.build_index()
        for mode in (vc.MODE_LINEAR, vc.MODE_MIH_APPROX):
            ra, ca, sa = a.search_knn(q, k, mode=mode, with_stats=True)
            rb, cb, sb = b.search_knn(q, k, mode=mode, with_stats=True)
            assert np.array_equal(ra, rb) and np.array_equal(ca, cb) and [_st(x) for x in sa] == [_st(x) for x in sb]
    # empty trailing shards (capacity above the record count), and a union with fewer than k records (R = S)
    for n_rec, cap in ((3000, 12000), (7, 50)):
        with vc.ShardedEngine(bits, capacity=cap, n_shards=4, n_tables=m, devices=[0], id_base=3, flags=vc.FLAG_GLOBAL_STOP) as s, \
                vc.Engine(bits, capacity=n_rec, n_tables=m, id_base=3) as one:
            s.add_codes(codes[:n_rec])
            s.build_index()
            one.add_codes(codes[:n_rec])
            one.build_index()
            _, cnt, st = _assert_same(vc, s, one, q, k)
            if n_rec < k:
                assert all(x.radius == bits // m and x.n_candidates == n_rec for x in st) and np.all(cnt == n_rec)


def test_driver_prints_one_search_worker(vc, oracle, tmp_path):
    """distributed-image-search with VC_SHARDS=3 VC_GLOBAL_STOP=1 prints what the one-engine run prints"""
    driver = os.path.join(ROOT, "verticut_amd", "bin", "distributed-image-search")
    n, bits, m, k = 30000, 128, 4, 10
    rng = np.random.default_rng(5)
    codes = oracle.gen_codes(n, bits, 34, kind=1, n_centres=150, max_flips=8)
    q = np.concatenate([codes[rng.integers(0, n, size=5)], rng.integers(0, 256, size=(1, bits // 8), dtype=np.uint8)])
    q[:5, 3] ^= 0x12
    (tmp_path / "lsh.code").write_bytes(codes.tobytes())
    (tmp_path / "query.code").write_bytes(q.tobytes())
    args = [driver, str(tmp_path / "lsh.code"), str(n), str(bits), str(bits // m), str(k), "pilaf", "0", "0", "-1",
            str(tmp_path / "query.code")]

    def run(**extra):
        env = {key: v for key, v in os.environ.items() if key not in ("VC_SHARDS", "VC_GLOBAL_STOP", "VC_REF_QUIRKS")}
        env.update(VC_PRINT_RESULTS="1", VC_DEVICES="0", **extra)
        p = subprocess.run(args, capture_output=True, text=True, timeout=300, env=env)
        return p.returncode, [ln for ln in p.stdout.splitlines() if not ln.startswith("while :")], p.stderr

    rc1, one, err1 = run()
    rc3, sharded, err3 = run(VC_SHARDS="3", VC_GLOBAL_STOP="1")
    assert rc1 == 0 and rc3 == 0, err1 + err3
    assert len(re.findall(r"^query \d+$", "\n".join(one), flags=re.M)) == len(q)
    assert sharded == one
    rc, _, err = run(VC_SHARDS="3", VC_GLOBAL_STOP="1", VC_REF_QUIRKS="1")
    assert rc != 0 and "VC_GLOBAL_STOP" in err
