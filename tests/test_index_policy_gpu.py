"""Every index layout the MIH memory policy can choose (csrc/vc_mih_policy.hpp; tests/cpp/mih_policy_test.cc has its arithmetic).
An index may or may not hold bucket-order code copies (bcodes: <= 16-bit substrings), {id, code} records (bent: 32-bit substrings
of <= 128-bit codes) and directory lines (lines: 32-bit substrings); what it gets depends on the free device memory, which never
bites at a test's size, so without a knob the suite only ever sees bcodes=1 / bent=1 / lines=0.  Here every outcome is forced
through VC_MIH_BCODES, VC_MIH_BENT and VC_MIH_LINES, the VC_MIH_TRACE line "index built: ..." proves which index a case got, and
every row and statistic is compared with MihOracle.find (SearchWorker::find, search_worker.cc:159-264) or numpy brute force --
equality between two layouts is only ever asserted on top of that."""
import filecmp
import functools
import re

import numpy as np
import pytest

import flag_routes_common as F
from test_mih_limits_gpu import buf_entries, limits

# (the GPU tests are marked one by one: the two tests on the cases themselves run without a GPU)

ERASED = np.uint64(0xFFFFFFFFFFFFFFFF)
KNOBS = ("VC_MIH_BCODES", "VC_MIH_BENT", "VC_MIH_LINES", "VC_MIH_STREAM")


def _layout_line(err, how):
    """the last 'index built' / 'index loaded' line of a captured stderr -> (n, sbits, m, W, bcodes, bent, lines)"""
    found = re.findall(r"\[vc_mih\] index %s: n=(\d+) sbits=(\d+) m=(\d+) W=(\d+) bcodes=([01]) bent=([01]) lines=([01])\n" % how, err)
    assert found, err
    return tuple(int(x) for x in found[-1])


def _host_stats(st):
    return [(s.radius, s.n_results, s.n_main_reads, s.n_sub_reads, s.n_local_reads, s.n_candidates) for s in st]


def _search_dev(torch, e, q, k, mode):
    """the device-resident call on torch's current stream: (rows, counts, statistics as _host_stats gives them)"""
    nq = len(q)
    dq = torch.from_numpy(np.array(q)).cuda()
    out = torch.full((nq, k), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    cnt = torch.full((nq,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    stat = torch.full((nq, 5), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    e.search_knn_dev_stats(dq.data_ptr(), nq, k, out.data_ptr(), cnt.data_ptr(), stat.data_ptr(), mode=mode,
                           stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    stats = []
    for r in stat.cpu().numpy().view(np.uint8).reshape(-1, 40):      # 40-byte vc_query_stats records
        u32, u64 = r[:8].view(np.uint32), r[8:].view(np.uint64)
        stats.append((int(u32[0]), int(u32[1]), int(u64[0]), int(u64[1]), int(u64[2]), int(u64[3])))
    return out.cpu().numpy().view(np.uint64), cnt.cpu().numpy().view(np.uint32), stats


# ---------------------------------------------------------------- (a) the witness: the index says what it holds
# what the trace line must show on a route, written out by route NAME: the environment itself comes from F.ROUTES, so a knob
# misspelt there builds the default index and fails here
def _expected_layout(sid, route):
    sh = F.SHAPES[sid]
    s = sh.bits // sh.m
    bcodes, bent, lines = int(s <= 16), int(s == 32 and sh.bits <= 128), 0
    if route == "bcodes0":
        bcodes = 0
    if route in ("lines1", "bent0_lines1") and s == 32:
        lines = 1
    if route in ("bent0", "bent0_lines1"):
        bent = 0
    return bcodes, bent, lines


INDEX_ROUTES = ("default", "bcodes0", "lines1", "bent0", "bent0_lines1")        # the routes of F.ROUTES that shape the index
WITNESS = [(sid, r) for sid in F.SHAPES for r in INDEX_ROUTES if r in F.ROUTES_OF[sid]]
_saved = {}


def _default_index_file(vc, oracle, tmp_path_factory, sid):
    """the index of a shape saved once, from an engine created without any knob"""
    if sid not in _saved:
        sh = F.SHAPES[sid]
        path = tmp_path_factory.mktemp("index_" + sid) / "default.vcidx"
        with vc.Engine(sh.bits, capacity=sh.n, n_tables=sh.m) as e:
            e.add_codes(F.make_codes(oracle, sid))
            e.build_index()
            e.save_index(path)
        _saved[sid] = path
    return _saved[sid]


def test_the_witness_cases_cover_every_index_shaping_route():
    """every route of the table whose environment names an index knob is a witness case at every shape that lists it: 5 + 5 + 2 + 2 + 1"""
    shaping = {r for r, env in F.ROUTES.items() if not env or set(env) & {"VC_MIH_BCODES", "VC_MIH_BENT", "VC_MIH_LINES"}}
    assert shaping == set(INDEX_ROUTES)
    assert len(WITNESS) == 15 and all((sid, r) in WITNESS for sid in F.SHAPES for r in F.ROUTES_OF[sid] if r in shaping)
    assert {sid for sid, r in WITNESS if r != "default" and _expected_layout(sid, r) == _expected_layout(sid, "default")} <= {"A", "B"}
    assert all(_expected_layout(sid, "bcodes0") == _expected_layout(sid, "default") for sid in "AB")     # no copies to lose at 32 bits


@pytest.mark.gpu
@pytest.mark.parametrize("sid,route", WITNESS, ids=["-".join(c) for c in WITNESS])
def test_index_reports_its_layout(vc, oracle, monkeypatch, capfd, tmp_path, tmp_path_factory, sid, route):
    """The VC_MIH_TRACE line of a build shows exactly the layout the route asks for; the index file saved under the default,
    loaded under the route's environment into a second engine with the same records, shows that layout again (the derived
    structures are not in the file: a load derives them by the same policy), and the file a bent0_lines1 engine saves is byte for
    byte the default engine's."""
    sh = F.SHAPES[sid]
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    default_file = _default_index_file(vc, oracle, tmp_path_factory, sid) if route != "default" else None
    monkeypatch.setenv("VC_MIH_TRACE", "1")
    for name, value in F.ROUTES[route].items():                   # read at vc_create
        monkeypatch.setenv(name, value)
    codes = F.make_codes(oracle, sid)
    head = (sh.n, sh.bits // sh.m, sh.m, sh.bits // 64)
    capfd.readouterr()
    with vc.Engine(sh.bits, capacity=sh.n, n_tables=sh.m) as e:
        e.add_codes(codes)
        e.build_index()
        assert _layout_line(capfd.readouterr().err, "built") == head + _expected_layout(sid, route), (sid, route)
        if route == "bent0_lines1":
            e.save_index(tmp_path / "own.vcidx")
            assert filecmp.cmp(tmp_path / "own.vcidx", default_file, shallow=False)
    if default_file is not None:
        with vc.Engine(sh.bits, capacity=sh.n, n_tables=sh.m) as e2:
            e2.add_codes(codes)
            e2.load_index(default_file)
            assert _layout_line(capfd.readouterr().err, "loaded") == head + _expected_layout(sid, route), (sid, route)
            q = F.make_queries(oracle, sid)[:4]                   # the loaded index serves: rows of the oracle's, query by query
            got, cnt, st = e2.search_knn(q, sh.k, mode=vc.MODE_MIH_EXACT, with_stats=True)
            for i, ex in enumerate(F.expect(oracle, sid, "")[:4]):
                assert np.array_equal(got[i, : cnt[i]], ex.row) and (st[i].radius, st[i].n_candidates) == (ex.stats[0], ex.stats[4])


@pytest.mark.gpu
def test_records_cannot_be_forced_onto_wide_codes(vc, oracle, monkeypatch, capfd):
    """VC_MIH_BENT=1 at 256 bit / 8 tables: the {id, code} records exist for codes of at most two words, the index has none"""
    monkeypatch.setenv("VC_MIH_TRACE", "1")
    monkeypatch.setenv("VC_MIH_BENT", "1")
    n = 5000
    codes = oracle.gen_codes(n, 256, 9, kind=1, n_centres=50, max_flips=6)
    capfd.readouterr()
    with vc.Engine(256, capacity=n, n_tables=8) as e:
        e.add_codes(codes)
        e.build_index()
        assert _layout_line(capfd.readouterr().err, "built") == (n, 32, 8, 4, 0, 0, 0)


# ---------------------------------------------------------------- (c) every layout on what the flag routes do not run
N = 30000
N_EVERY, N_BIG, N_BIG_CENTRES = 6000, 12500, 4
# k = 2 000 is the largest round k whose candidates the query kernel still buffers (3 k + 1 024 <= 8 192 entries); k = 2 400 is past
# that step (16 384), so the multi-block kernels take the call and mih_probe_kernel reads the entries
K_SMALL, K_BIG, K_MULTI, NQ_BIG = 20, 2000, 2400, 4
LAYOUT_ENV = {"bent1": ("VC_MIH_BENT", "1"), "bent0": ("VC_MIH_BENT", "0"), "lines0": ("VC_MIH_LINES", "0"), "lines1": ("VC_MIH_LINES", "1"),
              "bcodes1": ("VC_MIH_BCODES", "1"), "bcodes0": ("VC_MIH_BCODES", "0")}
CELLS = ([(bits, m, (b, ln)) for bits, m in ((64, 2), (128, 4)) for b in ("bent1", "bent0") for ln in ("lines0", "lines1")]
         + [(256, 8, ("lines0",)), (256, 8, ("lines1",))]
         + [(bits, m, (b,)) for bits, m in ((64, 4), (128, 8)) for b in ("bcodes1", "bcodes0")])
RELOADED = {(128, 4, ("bent0", "lines0")), (128, 4, ("bent0", "lines1")), (64, 4, ("bcodes0",))}


def _cell_layout(bits, m, layout):
    s = bits // m
    return (int(s <= 16 and "bcodes0" not in layout), int(s == 32 and bits <= 128 and "bent0" not in layout), int("lines1" in layout))


@functools.lru_cache(maxsize=None)
def _data(vo, bits, m):
    """One database per shape, 30 000 records in a fixed random order:
    - 6 000 at EVERY distance 0 .. 2m+3 around one base code, flips spread over the substrings (the data of
      test_radius_search_every_remainder_of_the_pigeonhole_split): the radius sweep's query is the base code;
    - 12 500 in 4 clusters of ~3 100 within 5 flips of their centre: a query there has 2 400 neighbours within a few shells, so
      k = 2 000 and k = 2 400 stop where the oracle can still follow;
    - 11 500 in 115 clusters within 6 flips: the k = 20 queries, 0 .. 10 flips away from a record (F.FLIPS), stop in shells 0 .. 3.
    Returns (codes, base, queries [16]); queries 0..3 come from the big clusters."""
    rng = np.random.default_rng(1000 * bits + m)
    base = vo.gen_codes(1, bits, 5)[0]
    every = np.tile(base, (N_EVERY, 1))
    for i in range(N_EVERY):
        for b in rng.choice(bits, size=int(rng.integers(0, 2 * m + 4)), replace=False):
            every[i, b // 8] ^= np.uint8(1 << (b % 8))
    big = vo.gen_codes(N_BIG, bits, 51, kind=1, n_centres=N_BIG_CENTRES, max_flips=5)
    small = vo.gen_codes(N - N_EVERY - N_BIG, bits, 52, kind=1, n_centres=115, max_flips=6)
    parts = np.concatenate([every, big, small])
    perm = rng.permutation(N)
    codes = np.ascontiguousarray(parts[perm])
    where = np.empty(N, dtype=np.int64)
    where[perm] = np.arange(N)                                    # row of parts -> row of codes
    src = np.concatenate([N_EVERY + rng.integers(0, N_BIG, NQ_BIG), N_EVERY + N_BIG + rng.integers(0, len(small), F.NQ - NQ_BIG)])
    q = codes[where[src]].copy()
    for i in range(F.NQ):
        for b in rng.choice(bits, size=(1, 2, 3, 0)[i] if i < NQ_BIG else F.FLIPS[i % 8], replace=False):
            q[i, b // 8] ^= np.uint8(1 << (b % 8))
    for a in (codes, base, q):
        a.setflags(write=False)
    return codes, base, q


@functools.lru_cache(maxsize=None)
def _knn_expect(vo, bits, m, k, nq):
    """[nq] (canonical row, (radius, n_results, 0, n_sub_reads, n_local_reads, n_candidates)) from MihOracle.find"""
    codes, _, q = _data(vo, bits, m)
    mo = vo.MihOracle(codes, m, key_mode=1)
    out = []
    for i in range(nq):
        ores, ost = mo.find(q[i], k, stop_mult=min(m, 4))
        row, reachable = F.canonical_mih(vo, codes, q[i], m, k, ost.radius, False)
        assert reachable == ost.n_distinct and ost.n_main_reads == 0
        F.check_contract(row, ores)
        out.append((row, (ost.radius, ost.n_results, 0, ost.n_sub_reads, ost.n_local_reads, ost.n_distinct)))
    mo.close()
    return out


@functools.lru_cache(maxsize=None)
def _radius_expect(vo, bits, m):
    """[2m+3] sorted packed (distance, id) of everything within R of the base code, R = 0 .. 2m+2: numpy brute force"""
    codes, base, _ = _data(vo, bits, m)
    d = vo.np_distances(codes, base)
    out = []
    for R in range(2 * m + 3):
        ids = np.nonzero(d <= R)[0]
        out.append(np.sort(vo.pack(d[ids], ids.astype(np.uint64))))
    return out


def _check_knn(torch, vc, e, q, k, expected, where):
    """host and device call against the oracle: whole rows by the canonical tie rule, counts, every statistic"""
    got, cnt, st = e.search_knn(q, k, mode=vc.MODE_MIH_EXACT, with_stats=True)
    dgot, dcnt, dst = _search_dev(torch, e, q, k, vc.MODE_MIH_EXACT)
    for rows, counts, stats, call in ((got, cnt, _host_stats(st), "host"), (dgot, dcnt, dst, "dev")):
        assert len(rows) == len(expected)
        for i, (row, exp_stats) in enumerate(expected):
            assert counts[i] == len(row) == exp_stats[1], (where, call, i)
            assert np.array_equal(rows[i, : counts[i]], row), (where, call, i)
            assert np.all(rows[i, counts[i]:] == ERASED), (where, call, i)
            assert stats[i] == exp_stats, (where, call, i, stats[i], exp_stats)
    return got, cnt, _host_stats(st)


def _check_radius_sweep(vc, e, base, expected, where):
    for R, exp in enumerate(expected):
        got = e.search_radius(base[None, :], R, mode=vc.MODE_MIH_EXACT, cap_per_query=1 << 15)[0]
        assert np.array_equal(got, exp), (where, R, len(got), len(exp))


def test_the_layout_cells_have_something_to_get_wrong(oracle):
    """Needs no GPU result: on every shape's database the k = 20 queries stop in at least three different shells, k = 2 000 fills
    the query kernel's largest candidate buffer and k = 2 400 is past it, the sweep's results grow with every R and every
    remainder of R over the tables occurs."""
    assert len(CELLS) == 14 and len(set(CELLS)) == 14 and RELOADED <= set(CELLS)
    L = limits()
    assert buf_entries(L, K_BIG) == 8192 and buf_entries(L, K_MULTI) == 16384
    for bits, m in sorted({(b, m) for b, m, _ in CELLS}):
        small = _knn_expect(oracle, bits, m, K_SMALL, F.NQ)
        assert len({s[0] for _, s in small}) >= 3, (bits, m)
        for k in (K_BIG, K_MULTI):
            assert all(len(row) == k for row, _ in _knn_expect(oracle, bits, m, k, NQ_BIG)), (bits, m, k)
        sizes = [len(r) for r in _radius_expect(oracle, bits, m)]
        assert len(sizes) == 2 * m + 3 and all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[-1] < 1 << 15, (bits, m, sizes)


@pytest.mark.gpu
@pytest.mark.parametrize("bits,m,layout", CELLS, ids=["%d-%d-%s" % (b, m, "-".join(ly)) for b, m, ly in CELLS])
def test_every_layout_serves_every_route(vc, oracle, monkeypatch, capfd, tmp_path, bits, m, layout):
    """One engine per (shape, layout): exact k-NN with k = 20, k = 2 000 (the query kernel's largest candidate buffer) and
    k = 2 400 (past it -- the multi-block kernels: mih_probe_kernel reads its entries through vc_load_entry) on the host and
    the device call against MihOracle.find, radius search for every
    R = 0 .. 2m+2 against numpy.  <= 16-bit shapes sweep once more under VC_MIH_STREAM=2: the bucket-streaming kernel with the code
    copies, the per-shell probe launches without them -- the route an index takes when the copies do not fit.  Three cells reach
    the same engine state by load_index as well."""
    import torch
    where = (bits, m, layout)
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("VC_MIH_TRACE", "1")
    for name, value in (LAYOUT_ENV[ly] for ly in layout):
        monkeypatch.setenv(name, value)
    codes, base, q = _data(oracle, bits, m)
    small, sweep = _knn_expect(oracle, bits, m, K_SMALL, F.NQ), _radius_expect(oracle, bits, m)
    line = (N, bits // m, m, bits // 64) + _cell_layout(bits, m, layout)
    capfd.readouterr()
    with vc.Engine(bits, capacity=N, n_tables=m) as e:
        e.add_codes(codes)
        e.build_index()
        assert _layout_line(capfd.readouterr().err, "built") == line, where
        built = _check_knn(torch, vc, e, q, K_SMALL, small, where)
        e.timing()
        _check_knn(torch, vc, e, q[:NQ_BIG], K_BIG, _knn_expect(oracle, bits, m, K_BIG, NQ_BIG), (where, K_BIG))
        assert e.timing().mih_launches >= 1                       # the query kernel, on its 8 192-entry buffer
        _check_knn(torch, vc, e, q[:NQ_BIG], K_MULTI, _knn_expect(oracle, bits, m, K_MULTI, NQ_BIG), (where, K_MULTI))
        assert e.timing().mih_launches == 0                       # no query-kernel launch: 16 384 entries are not buffered in LDS
        _check_radius_sweep(vc, e, base, sweep, where)
        if where in RELOADED:
            e.save_index(tmp_path / "index.vcidx")
    if where in RELOADED:
        with vc.Engine(bits, capacity=N, n_tables=m) as e2:
            e2.add_codes(codes)
            e2.load_index(tmp_path / "index.vcidx")
            assert _layout_line(capfd.readouterr().err, "loaded") == line, where
            loaded = _check_knn(torch, vc, e2, q, K_SMALL, small, (where, "loaded"))
            assert np.array_equal(loaded[0], built[0]) and np.array_equal(loaded[1], built[1]) and loaded[2] == built[2]
            _check_radius_sweep(vc, e2, base, sweep, (where, "loaded"))
    if bits // m <= 16:
        monkeypatch.setenv("VC_MIH_STREAM", "2")                  # read at vc_create: a second engine
        with vc.Engine(bits, capacity=N, n_tables=m) as e3:
            e3.add_codes(codes)
            e3.build_index()
            assert _layout_line(capfd.readouterr().err, "built") == line, where
            e3.timing()
            _check_radius_sweep(vc, e3, base, sweep, (where, "stream"))
            t = e3.timing()
        if "bcodes1" in layout:
            assert t.mih_launches >= 1 and t.mih_entries >= t.mih_hits > 0     # mih_bucket_stream_kernel ran and read entries
        else:
            assert t.mih_launches == 0                            # no copies, no stream route: one probe launch per shell
