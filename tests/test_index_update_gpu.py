"""vc_update_index on the GPU: an index brought up to date by merging the appended records (handle U) is BIT FOR BIT the index
vc_build_index builds from all records (handle F) -- as saved files where a file is small enough, else bucket by bucket and bitmap
word by bitmap word --, for every way a new entry can meet the old index (index_update_common), every index layout, any call
history, across save / load, over shards and through the C++ host layer.  The VC_MIH_TRACE line "index updated: ..." is the
witness of the route an update took."""
import filecmp
import os
import re
import subprocess

import numpy as np
import pytest

import flag_routes_common as F
import index_update_common as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("VC_MIH_BCODES", "VC_MIH_BENT", "VC_MIH_LINES", "VC_MIH_STREAM", "VC_MIH_UPDATE")


def _update_lines(err):
    """the 'index updated' lines of a captured stderr -> [(n, added, route, bent, bcodes, lines)]"""
    found = re.findall(r"\[vc_mih\] index updated: n=(\d+) added=(\d+) route=(\w+) bent=(\w+) bcodes=([01]) lines=([01])\n", err)
    return [(int(n), int(a), r, b, int(bc), int(ln)) for n, a, r, b, bc, ln in found]


def _clean_env(monkeypatch, **env):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("VC_MIH_TRACE", "1")
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def _start(e, old):
    """add the old records and build; a handle that refuses an index of nothing gets its first record by add alone"""
    if len(old):
        e.add_codes(old)
    e.build_index()


def _same_files(a, b):
    same = filecmp.cmp(a, b, shallow=False)
    os.unlink(a)
    os.unlink(b)
    return same


def _compare_views(u, f, bits, m, key_cols, planted, id_base, where):
    """U against F and against the stable sort: every occurring key's bucket in every table, the bitmap words around the planted
    keys, a few absent keys"""
    s = bits // m
    for t in range(m):
        col = key_cols[:, t]
        order = np.argsort(col, kind="stable")
        for key in np.unique(col).tolist():
            exp = (order[np.searchsorted(col[order], key, "left"): np.searchsorted(col[order], key, "right")] + id_base).astype(np.uint32)
            gu, gf = u.get_bucket(t, key, with_codes=False), f.get_bucket(t, key, with_codes=False)
            assert gu is not None and gf is not None, (where, t, key)
            assert gu[2] == gf[2] == len(exp) and np.array_equal(gu[0], exp) and np.array_equal(gf[0], exp), (where, t, key)
        words = (1 << s) // 32
        for key in planted[t]:
            w0 = max(0, (key >> 5) - 1)
            cnt = min(3, words - w0)
            assert np.array_equal(u.bitmap_read(t, w0, cnt), f.bitmap_read(t, w0, cnt)), (where, t, key)
            assert u.bitmap_test(t, key) == 1, (where, t, key)
        present = set(col.tolist())
        for key in (2, 5, (1 << s) - 2, (1 << (s - 1)) + 1):
            if key not in present:
                assert u.bitmap_test(t, key) == 0 and f.bitmap_test(t, key) == 0 and u.get_bucket(t, key) is None, (where, t, key)


def _planted_keys(bits, m, new_k):
    out = []
    for t in range(m):
        p = U.plan(bits, m, t)
        want = set((0,) + p.below + p.above + p.between + p.edges + ((p.empty_block,) if p.empty_block is not None else ()))
        out.append(sorted(want & set(new_k[:, t].tolist())))
    return out


def _update_and_compare(vc, capfd, tmp_path, bits, m, n0, d, id_base=0):
    old_c, new_c = U.codes(bits, m, n0, d)
    old_k, new_k = U.keys(bits, m, n0, d)
    where = (bits, m, n0, d, id_base)
    with vc.Engine(bits, capacity=n0 + d, n_tables=m, id_base=id_base) as u, vc.Engine(bits, capacity=n0 + d, n_tables=m, id_base=id_base) as f:
        _start(u, old_c)
        if d:
            u.add_codes(new_c)
        capfd.readouterr()
        u.update_index()
        lines = _update_lines(capfd.readouterr().err)
        assert len(lines) == 1 and lines[0][:3] == (n0 + d, d, "merge" if d else "none"), (where, lines)
        f.add_codes(np.concatenate([old_c, new_c]))
        f.build_index()
        if (bits, m) in U.FILE_SHAPES:
            u.save_index(tmp_path / "u.vcidx")
            f.save_index(tmp_path / "f.vcidx")
            assert _same_files(tmp_path / "u.vcidx", tmp_path / "f.vcidx"), where
        else:
            _compare_views(u, f, bits, m, np.concatenate([old_k, new_k]), _planted_keys(bits, m, new_k), id_base, where)


PAIR_CASES = [(b, m, n0, d) for b, m in U.SHAPES for n0, d in U.PAIRS]
SWEEP_CASES = [(b, m, n0, U.SWEEP_DELTA) for b, m in U.SWEEP_SHAPES for n0 in U.SWEEP_N0]


@pytest.mark.parametrize("bits,m,n0,d", PAIR_CASES + SWEEP_CASES, ids=["%d-%d-%d+%d" % c for c in PAIR_CASES + SWEEP_CASES])
def test_updated_index_is_the_built_index(vc, monkeypatch, capfd, tmp_path, bits, m, n0, d):
    """1. add n0, build, add delta, update == add n0 + delta, build; the trace names the merge (nothing to do: none)"""
    _clean_env(monkeypatch)
    assert (bits, m, n0, d) in U.cases()
    _update_and_compare(vc, capfd, tmp_path, bits, m, n0, d)


@pytest.mark.parametrize("bits,m", [(64, 4), (128, 4)])
def test_updated_index_with_an_id_base(vc, monkeypatch, capfd, tmp_path, bits, m):
    """1. the same under id_base != 0: the tables hold local ids, the views add the base"""
    _clean_env(monkeypatch)
    _update_and_compare(vc, capfd, tmp_path, bits, m, 300, 20000, id_base=1000000)


@pytest.mark.parametrize("bits,m", [(64, 8), (64, 4), (64, 2)])
def test_repeated_updates(vc, monkeypatch, capfd, tmp_path, bits, m):
    """2. build at n0, three add + update rounds of different sizes, searches in between: the file of one build"""
    _clean_env(monkeypatch)
    old_c, new_c = U.codes(bits, m, 300, 20000)
    both = np.concatenate([old_c, new_c])
    cuts = (300, 301, 4500, 20300)
    q = both[[5, 310, 20000]]
    with vc.Engine(bits, capacity=len(both), n_tables=m) as u, vc.Engine(bits, capacity=len(both), n_tables=m) as f:
        u.add_codes(both[: cuts[0]])
        u.build_index()
        for a, b in zip(cuts, cuts[1:]):
            u.search_knn(q, 10, mode=vc.MODE_MIH_EXACT)
            u.search_radius(q[:1], 2, mode=vc.MODE_MIH_EXACT, cap_per_query=1 << 15)
            u.add_codes(both[a:b])
            capfd.readouterr()
            u.update_index()
            assert [ln[:3] for ln in _update_lines(capfd.readouterr().err)] == [(b, b - a, "merge")]
        f.add_codes(both)
        f.build_index()
        got, exp = u.search_knn(q, 10, mode=vc.MODE_MIH_EXACT, with_stats=True), f.search_knn(q, 10, mode=vc.MODE_MIH_EXACT, with_stats=True)
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and _host_stats(got[2]) == _host_stats(exp[2])
        u.save_index(tmp_path / "u.vcidx")
        f.save_index(tmp_path / "f.vcidx")
        assert _same_files(tmp_path / "u.vcidx", tmp_path / "f.vcidx")


def _host_stats(st):
    return [(s.radius, s.n_results, s.n_main_reads, s.n_sub_reads, s.n_local_reads, s.n_candidates) for s in st]


# ---------------------------------------------------------------- 3. every layout
def _layout_cells():
    import test_index_policy_gpu as P
    return [c for c in P.CELLS if (c[0], c[1]) in ((64, 2), (128, 4), (64, 4), (128, 8))]


N0_LAYOUT = 19000


@pytest.mark.parametrize("bits,m,layout", _layout_cells(), ids=["%d-%d-%s" % (b, m, "-".join(ly)) for b, m, ly in _layout_cells()])
def test_every_layout_after_an_update(vc, oracle, monkeypatch, capfd, bits, m, layout):
    """3. the knob routes of test_index_policy_gpu, on its database: 19 000 records built, 11 000 appended and merged.  The trace
    shows the layout the knobs name (records merged, not gathered again); exact k-NN (k = 20, 2 000), approximate k-NN and the radius
    sweep R = 0 .. 2m + 2 give the oracle's rows, counts and statistics and handle F's, bit for bit."""
    import torch
    import test_index_policy_gpu as P
    from test_flag_routes_gpu import _check
    _clean_env(monkeypatch, **dict(P.LAYOUT_ENV[ly] for ly in layout))
    codes, base, q = P._data(oracle, bits, m)
    where = (bits, m, layout)
    bcodes, bent, lines = P._cell_layout(bits, m, layout)
    approx = F._expect_rows(oracle, codes, q, m, 5, 1, False, 4, True, 0)
    with vc.Engine(bits, capacity=P.N, n_tables=m) as u, vc.Engine(bits, capacity=P.N, n_tables=m) as f:
        u.add_codes(codes[:N0_LAYOUT])
        u.build_index()
        u.add_codes(codes[N0_LAYOUT:])
        capfd.readouterr()
        u.update_index()
        assert _update_lines(capfd.readouterr().err) == [(P.N, P.N - N0_LAYOUT, "merge", "merge" if bent else "0", bcodes, lines)], where
        f.add_codes(codes)
        f.build_index()
        assert P._layout_line(capfd.readouterr().err, "built")[4:] == (bcodes, bent, lines), where
        for k, nq in ((P.K_SMALL, F.NQ), (P.K_BIG, P.NQ_BIG)):
            got = P._check_knn(torch, vc, u, q[:nq], k, P._knn_expect(oracle, bits, m, k, nq), (where, k))
            exp = f.search_knn(q[:nq], k, mode=vc.MODE_MIH_EXACT, with_stats=True)
            assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and got[2] == _host_stats(exp[2]), (where, k)
        got = u.search_knn(q, 5, mode=vc.MODE_MIH_APPROX, with_stats=True)
        exp = f.search_knn(q, 5, mode=vc.MODE_MIH_APPROX, with_stats=True)
        _check(got[0], got[1], _host_stats(got[2]), approx, (where, "approx"))
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and _host_stats(got[2]) == _host_stats(exp[2]), where
        P._check_radius_sweep(vc, u, base, P._radius_expect(oracle, bits, m), where)
        P._check_radius_sweep(vc, f, base, P._radius_expect(oracle, bits, m), (where, "F"))


@pytest.mark.parametrize("sid,fl", [("C", "signext"), ("A", "bitmap")])
def test_reference_flags_after_an_update(vc, oracle, monkeypatch, capfd, sid, fl):
    """3. VC_FLAG_REF_SIGNEXT_KEYS (16-bit keys) and VC_FLAG_USE_BITMAP (32-bit keys) on an updated index: MihOracle's rows and
    statistics, exact and approximate"""
    from test_flag_routes_gpu import _check
    _clean_env(monkeypatch)
    sh = F.SHAPES[sid]
    codes, q = F.make_codes(oracle, sid), F.make_queries(oracle, sid)
    with vc.Engine(sh.bits, capacity=sh.n, n_tables=sh.m, flags=F.flag_bits(fl)) as u:
        u.add_codes(codes[:21000])
        u.build_index()
        u.add_codes(codes[21000:])
        u.update_index()
        assert [ln[2] for ln in _update_lines(capfd.readouterr().err)] == ["merge"]
        for mode, k, approx in ((vc.MODE_MIH_EXACT, sh.k, False), (vc.MODE_MIH_APPROX, sh.k_approx, True)):
            got, cnt, st = u.search_knn(q, k, mode=mode, with_stats=True)
            _check(got, cnt, _host_stats(st), F.expect(oracle, sid, fl, approx), (sid, fl, approx))


# ---------------------------------------------------------------- 4. handle history
@pytest.mark.parametrize("sid", ["C", "A"])
def test_handle_history(vc, oracle, monkeypatch, tmp_path, sid):
    """4. searches, an add (every index consumer answers VC_ERR_STATE, the linear scan serves on), the update, the same and new
    searches: a fresh handle's results bit for bit; a NEW record queried by id without itself"""
    _clean_env(monkeypatch)
    sh = F.SHAPES[sid]
    codes, q = F.make_codes(oracle, sid), F.make_queries(oracle, sid)
    n0 = 17000
    with vc.Engine(sh.bits, capacity=sh.n, n_tables=sh.m) as u, vc.Engine(sh.bits, capacity=sh.n, n_tables=sh.m) as f:
        u.add_codes(codes[:n0])
        u.build_index()
        u.search_knn(q, sh.k, mode=vc.MODE_MIH_EXACT, with_stats=True)
        u.search_radius(q[:2], 3, mode=vc.MODE_MIH_EXACT, cap_per_query=1 << 15)
        u.add_codes(codes[n0:])
        key0 = int.from_bytes(codes[0, : sh.bits // sh.m // 8].tobytes(), "little")
        for call in (lambda: u.search_knn(q, sh.k, mode=vc.MODE_MIH_EXACT), lambda: u.search_knn(q, sh.k, mode=vc.MODE_MIH_APPROX),
                     lambda: u.get_bucket(0, key0), lambda: u.save_index(tmp_path / "stale.vcidx"), lambda: u.bitmap_test(0, key0),
                     lambda: u.search_radius(q[:1], 2, mode=vc.MODE_MIH_EXACT),
                     lambda: u.search_knn_ids(np.array([3, 5], dtype=np.uint32), 5, mode=vc.MODE_MIH_EXACT)):
            with pytest.raises(vc.VcError) as ei:
                call()
            assert ei.value.code == vc.VC_ERR_STATE
        lin = u.search_knn(q, sh.k, mode=vc.MODE_LINEAR)           # the scan needs no index: all records, stale index or not
        u.update_index()
        f.add_codes(codes)
        f.build_index()
        flin = f.search_knn(q, sh.k, mode=vc.MODE_LINEAR)
        assert np.array_equal(lin[0], flin[0]) and np.array_equal(lin[1], flin[1])
        new_ids = np.array([n0, n0 + 1, sh.n - 1, 7], dtype=np.uint32)
        for h_calls in (
            lambda h: h.search_knn(q, sh.k, mode=vc.MODE_MIH_EXACT, with_stats=True),
            lambda h: h.search_knn(q, sh.k_approx, mode=vc.MODE_MIH_APPROX, with_stats=True),
            lambda h: h.search_knn(codes[n0: n0 + 8], 7, mode=vc.MODE_MIH_EXACT, with_stats=True),
            lambda h: h.search_knn_ids(new_ids, 6, mode=vc.MODE_MIH_EXACT, id_flags=vc.IDS_EXCLUDE_SELF, with_stats=True),
        ):
            got, exp = h_calls(u), h_calls(f)
            assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and _host_stats(got[2]) == _host_stats(exp[2])
        rows, cnt, _ = u.search_knn_ids(new_ids, 6, mode=vc.MODE_MIH_EXACT, id_flags=vc.IDS_EXCLUDE_SELF, with_stats=True)
        for i, gid in enumerate(new_ids):
            assert cnt[i] == 6 and gid not in (rows[i] & np.uint64(0xFFFFFFFF)).tolist()
        for R in (0, 2, 5):
            for a, b in zip(u.search_radius(q[:4], R, mode=vc.MODE_MIH_EXACT, cap_per_query=1 << 15),
                            f.search_radius(q[:4], R, mode=vc.MODE_MIH_EXACT, cap_per_query=1 << 15)):
                assert np.array_equal(a, b)


# ---------------------------------------------------------------- 5. the rebuild route
@pytest.mark.parametrize("bits,m", [(64, 4), (64, 2)])
def test_rebuild_route_gives_the_same_file(vc, monkeypatch, capfd, tmp_path, bits, m):
    """5. VC_MIH_UPDATE=0: vc_update_index rebuilds (the trace says so) and the file is the merge route's"""
    old_c, new_c = U.codes(bits, m, 4097, U.SWEEP_DELTA)
    paths = {}
    for route, env in (("merge", {}), ("rebuild", {"VC_MIH_UPDATE": "0"})):
        _clean_env(monkeypatch, **env)
        with vc.Engine(bits, capacity=len(old_c) + len(new_c), n_tables=m) as e:
            e.add_codes(old_c)
            e.build_index()
            e.add_codes(new_c)
            capfd.readouterr()
            e.update_index()
            assert [ln[:3] for ln in _update_lines(capfd.readouterr().err)] == [(len(old_c) + len(new_c), len(new_c), route)]
            paths[route] = tmp_path / (route + ".vcidx")
            e.save_index(paths[route])
    assert _same_files(paths["merge"], paths["rebuild"])


# ---------------------------------------------------------------- 6. persistence
@pytest.mark.parametrize("bits,m", [(64, 4), (64, 2)])
def test_update_of_a_loaded_index(vc, monkeypatch, capfd, tmp_path, bits, m):
    """6. load_index, add, update == a build of everything; the updated file passes the loader's device validation"""
    _clean_env(monkeypatch)
    old_c, new_c = U.codes(bits, m, 4096, U.SWEEP_DELTA)
    both = np.concatenate([old_c, new_c])
    with vc.Engine(bits, capacity=len(both), n_tables=m) as a:
        a.add_codes(old_c)
        a.build_index()
        a.save_index(tmp_path / "old.vcidx")
    with vc.Engine(bits, capacity=len(both), n_tables=m) as u, vc.Engine(bits, capacity=len(both), n_tables=m) as f:
        u.add_codes(old_c)
        u.load_index(tmp_path / "old.vcidx")
        os.unlink(tmp_path / "old.vcidx")
        u.add_codes(new_c)
        capfd.readouterr()
        u.update_index()
        assert [ln[:3] for ln in _update_lines(capfd.readouterr().err)] == [(len(both), len(new_c), "merge")]
        u.save_index(tmp_path / "u.vcidx")
        f.add_codes(both)
        f.build_index()
        f.save_index(tmp_path / "f.vcidx")
        assert filecmp.cmp(tmp_path / "u.vcidx", tmp_path / "f.vcidx", shallow=False)
        os.unlink(tmp_path / "f.vcidx")
        exp = f.search_knn(both[[1, 4500]], 10, mode=vc.MODE_MIH_EXACT)
    with vc.Engine(bits, capacity=len(both), n_tables=m) as third:
        third.add_codes(both)
        third.load_index(tmp_path / "u.vcidx")                    # (offsets, ranks, ids, bucket membership: validated on the device)
        os.unlink(tmp_path / "u.vcidx")
        got = third.search_knn(both[[1, 4500]], 10, mode=vc.MODE_MIH_EXACT)
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])


# ---------------------------------------------------------------- 7. sharded
def _sharded_results(vc, h, q, sh):
    out = []
    for mode, k in ((vc.MODE_LINEAR, sh.k), (vc.MODE_MIH_EXACT, sh.k), (vc.MODE_MIH_APPROX, sh.k_approx)):
        rows, cnt, st = h.search_knn(q, k, mode=mode, with_stats=True)
        out.append((rows.tolist(), cnt.tolist(), _host_stats(st)))
    for mode in (vc.MODE_LINEAR, vc.MODE_MIH_EXACT):
        out.append([r.tolist() for r in h.search_radius(q[:4], 4, mode=mode, cap_per_query=1 << 14)])
    return out


@pytest.mark.parametrize("sid,flags", [("C", 0), ("A", 0), ("A", "stop"), ("C", "approx")])
def test_sharded_update(vc, oracle, monkeypatch, capfd, sid, flags):
    """7. three shards on device 0, 12 000 records built (shard 0 full, shard 1 begun, shard 2 empty), 10 000 appended across the
    boundary of shards 1 and 2: shard 0 has nothing to do, shard 1 merges, shard 2 builds; every search equals a fresh store's"""
    _clean_env(monkeypatch)
    sh = F.SHAPES[sid]
    codes, q = F.make_codes(oracle, sid), F.make_queries(oracle, sid)
    fl = {0: 0, "stop": vc.FLAG_GLOBAL_STOP, "approx": vc.FLAG_GLOBAL_APPROX}[flags]
    n0, n1 = 12000, 22000
    mk = lambda: vc.ShardedEngine(sh.bits, capacity=sh.n, n_shards=3, n_tables=sh.m, devices=[0], flags=fl)
    u, f = mk(), mk()
    try:
        assert [u.shard_range(g) for g in range(3)] == [(0, 10000), (10000, 10000), (20000, 10000)]
        u.add_codes(codes[:n0])
        u.build_index()
        _sharded_results(vc, u, q, sh)
        u.add_codes(codes[n0:n1])
        with pytest.raises(vc.VcError) as ei:
            u.search_knn(q, sh.k, mode=vc.MODE_MIH_EXACT)
        assert ei.value.code == vc.VC_ERR_STATE
        capfd.readouterr()
        u.update_index()
        err = capfd.readouterr().err
        assert [ln[:3] for ln in _update_lines(err)] == [(10000, 0, "none"), (10000, 8000, "merge")], err
        assert re.findall(r"index built: n=(\d+)", err) == ["2000"], err
        f.add_codes(codes[:n1])
        f.build_index()
        assert _sharded_results(vc, u, q, sh) == _sharded_results(vc, f, q, sh)
        assert len(u) == len(f) == n1
    finally:
        u.close()
        f.close()


# ---------------------------------------------------------------- 8. the host layer


def test_host_layer_put_then_update(vc, tmp_path):
    """8. GpuProxy::put(ID, BinaryCode) in a loop, Backend::update_index(), get(HashIndex): the bucket with the new record last"""
    from verticut_amd import build as vb
    src = os.path.join(ROOT, "tests", "cpp", "put_update_test.cc")
    exe = tmp_path / "put_update"
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-o", str(exe), str(src), "-I", vb.HOST, "-L", vb.LIBDIR, "-lverticut_gpu",
                           "-Wl,-rpath," + vb.LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib", "-L/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert out.stdout.strip() == "bucket " + " ".join(str(i) for i in list(range(0, 40, 4)) + [42])
