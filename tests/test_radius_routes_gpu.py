"""The fixed-radius search on every route, flag, code width and depth.  radius_search_device (vc_mih.hip) answers a call through
mih_query_kernel in MQ_MODE_RADIUS, through mih_bucket_stream_kernel, through one mih_probe_kernel launch per shell or through the
verify kernel with a fixed threshold; each has its own copy of the pigeonhole split (n_big, small_shells, the tables left out while
R < m) and of the keep-everything ring (cap, doubling and repeat, vc_sort_compact_segments_kernel), and reads
VC_FLAG_REF_SIGNEXT_KEYS and VC_FLAG_USE_BITMAP in its own place.

Every (shape, flag set, route) cell of radius_routes_common.py builds one engine (cand_cap = 512: the ring starts at 4 096 entries)
and walks the shape's whole radius list twice on that handle -- ascending, then shuffled -- from R = 0 to R = bits and beyond, so
that route changes, MIH <-> scan buffer resets and the ring sizes earlier calls left behind are crossed both ways.  Each step
goes through vc_search_radius (first into a buffer that is too small: VC_ERR_CAPACITY and its offsets) and vc_search_radius_dev
(a side stream as torch's current one, poisoned buffers), all six queries in one call, and every row, every offset and the words
behind the total are compared bit for bit with the closed form of radius_routes_common.py (which test_radius_routes_cpu.py pins to
MihOracle.radius) -- never with another GPU route.  The VC_MIH_TRACE line of every attempt names the route, the clamped radius,
the plan's probes and the ring's capacity: all four are checked on every call."""
import ctypes as C
import re

import numpy as np
import pytest

import radius_routes_common as F

pytestmark = pytest.mark.gpu
POISON = 0x5A5A5A5A5A5A5A5A
TRACE = re.compile(r"\[vc_mih\] radius search: R=(\d+) probes=(\d+) cap=(\d+) route=(\w+)")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _attempts(capfd):
    """(R, probes, cap, route) of every attempt traced since the last look"""
    return [(int(a), int(b), int(c), d) for a, b, c, d in TRACE.findall(capfd.readouterr().err)]


class Ring:
    """the work ring of one handle (VcRadiusWork): it starts at 4 096 entries a query on the index and at 65 536 on the scan, doubles
    until the largest row fits, keeps its size for later calls and starts over when the tile shape flips between index and scan"""

    def __init__(self):
        self.scan, self.cap = None, 0

    def call(self, route, largest):
        scan = route == F.L
        if scan != self.scan:
            self.scan, self.cap = scan, 0
        first = last = max(self.cap, 65536 if scan else F.RING_START)
        while last < largest:
            last *= 2
        self.cap = last
        return first, last


def _check_trace(lines, sid, R, route_name, ring, rows, where):
    sh = F.SHAPES[sid]
    p = F.radius_plan(sh.bits, sh.m, R)
    assert lines, where
    for r, probes, cap, name in lines:
        assert (r, name) == (p.R, route_name), (where, lines)
        assert probes == (0 if route_name == F.L else p.probes), (where, lines)
    if ring is not None:
        first, last = ring.call(route_name, max(len(r) for r in rows))
        caps = [c for _, _, c, _ in lines]
        assert caps[0] == first and caps[-1] == last and caps == sorted(caps) and set(caps) <= {first << i for i in range(8)}, (where, caps, first, last)
        assert (len(set(caps)) > 1) == (last > first), (where, caps)


def _offsets(rows):
    return np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)


def _check_rows(flat, offs, rows, total_cap, where):
    """every row in full, the offsets, the total, and nothing written behind the total"""
    want = _offsets(rows)
    assert np.array_equal(offs[: len(want)], want), (where, offs[: len(want)], want)
    total = int(want[-1])
    assert np.array_equal(flat[:total], np.concatenate(rows)), where
    assert total_cap >= total and np.all(flat[total:] == np.uint64(POISON)), where


def _host_call(vc, h, fn, q, R, mode, rows, where):
    """the host-pointer call: a buffer of half the total first (VC_ERR_CAPACITY, the offsets already valid), then with room to spare"""
    nq, total = len(q), int(_offsets(rows)[-1])
    assert total > 0
    small = np.full(max(total // 2, 1), POISON, dtype=np.uint64)
    offs = np.full(nq + 2, POISON, dtype=np.uint64)
    assert fn(h, _p(q), nq, R, mode, _p(small), total // 2, _p(offs)) == vc.VC_ERR_CAPACITY, where
    assert np.array_equal(offs[: nq + 1], _offsets(rows)) and offs[nq + 1] == np.uint64(POISON), (where, "capacity leg")
    out = np.full(total + 8, POISON, dtype=np.uint64)
    offs = np.full(nq + 2, POISON, dtype=np.uint64)
    assert fn(h, _p(q), nq, R, mode, _p(out), total + 8, _p(offs)) == vc.VC_OK, where
    assert offs[nq + 1] == np.uint64(POISON), where
    _check_rows(out, offs, rows, total + 8, (where, "host"))


def _dev_call(vc, torch, side, e, q, R, mode, rows, where):
    """the device-resident call with exactly enough room, on a side stream that is torch's current one; every buffer poisoned"""
    nq, total = len(q), int(_offsets(rows)[-1])
    with torch.cuda.stream(side):
        dq = torch.from_numpy(q).cuda()
        out = torch.full((total + 8,), POISON, dtype=torch.int64, device="cuda")
        offs = torch.full((nq + 2,), POISON, dtype=torch.int64, device="cuda")
        rc = e.search_radius_dev(dq.data_ptr(), nq, R, out.data_ptr(), total, offs.data_ptr(), mode=mode,
                                 stream=torch.cuda.current_stream().cuda_stream)
        side.synchronize()
    assert rc == vc.VC_OK, where
    o = offs.cpu().numpy().view(np.uint64)
    assert o[nq + 1] == np.uint64(POISON), where
    _check_rows(out.cpu().numpy().view(np.uint64), o, rows, total, (where, "dev"))


def _set_route(monkeypatch, route):
    monkeypatch.setenv("VC_MIH_TRACE", "1")
    for name, value in F.ROUTES[route].items():                    # the knobs are read when an engine is created
        monkeypatch.setenv(name, value)


@pytest.mark.parametrize("case", F.cases(), ids=F.case_id)
def test_radius_walk_on_route(vc, monkeypatch, capfd, case):
    import torch
    sid, fl, route = case
    sh = F.SHAPES[sid]
    _set_route(monkeypatch, route)
    mode = vc.MODE_LINEAR if route == "linear" else vc.MODE_MIH_EXACT
    side = torch.cuda.Stream()
    queries = F.make_queries(sid)
    seen = set()
    with vc.Engine(sh.bits, capacity=sh.n, n_tables=sh.m, flags=F.flag_bits(fl), id_base=sh.id_base, cand_cap=F.CAND_CAP) as e:
        e.add_codes(F.make_codes(sid))
        e.build_index()
        capfd.readouterr()
        ring = Ring()
        for step, R in enumerate(F.walk(sid)):
            qis = F.queries_at(sid, R)
            q = np.ascontiguousarray(queries[list(qis)])
            rows = [F.expect(sid, fl, route, R, qi) for qi in qis]
            name = F.expected_route(sid, R, route)
            where = (case, step, R)
            _host_call(vc, e._h, e._L.vc_search_radius, q, R, mode, rows, where)
            lines = _attempts(capfd)
            _check_trace(lines, sid, R, name, ring, rows, where)
            _dev_call(vc, torch, side, e, q, R, mode, rows, where)
            _check_trace(_attempts(capfd), sid, R, name, ring, rows, where)
            seen.add(name)
    assert seen == {F.expected_route(sid, R, route) for R in F.RADII[sid]}


@pytest.mark.parametrize("sid,fl", F.SHARDED, ids=["-".join((s, f or "noflags")) for s, f in F.SHARDED])
def test_radius_walk_over_shards(vc, monkeypatch, capfd, sid, fl):
    """three shards on device 0 through vc_sharded_search_radius and vc_sharded_search_radius_dev, the radius list ascending:
    reachability is per record, so the rows are the closed form over the union; every shard's attempts name the route of a
    store of its size"""
    import torch
    sh = F.SHAPES[sid]
    _set_route(monkeypatch, "default")
    side = torch.cuda.Stream()
    queries = F.make_queries(sid)
    with vc.ShardedEngine(sh.bits, capacity=sh.n, n_shards=F.N_SHARDS, n_tables=sh.m, devices=[0], flags=F.flag_bits(fl), id_base=sh.id_base,
                          cand_cap=F.CAND_CAP) as s:
        s.add_codes(F.make_codes(sid))
        s.build_index()
        ranges = F.split_ranges(sh.n, F.N_SHARDS)
        assert [s.shard_range(g) for g in range(F.N_SHARDS)] == [(sh.id_base + first, cnt) for first, cnt in ranges]
        capfd.readouterr()
        for R in F.RADII[sid]:
            qis = F.queries_at(sid, R)
            q = np.ascontiguousarray(queries[list(qis)])
            rows = [F.expect_sharded(sid, fl, R, qi) for qi in qis]
            names = {F.expected_route(sid, R, "default", n=cnt) for _, cnt in ranges}
            assert len(names) == 1
            where = (sid, fl, R)
            _host_call(vc, s._h, s._L.vc_sharded_search_radius, q, R, vc.MODE_MIH_EXACT, rows, where)
            lines = _attempts(capfd)
            assert len(lines) >= F.N_SHARDS
            _check_trace(lines, sid, R, names.pop(), None, rows, where)
            _dev_call(vc, torch, side, s, q, R, vc.MODE_MIH_EXACT, rows, where)
            assert len(_attempts(capfd)) >= F.N_SHARDS


@pytest.mark.parametrize("sid,route,name", F.TILE_LEGS, ids=[r for _, r, _ in F.TILE_LEGS])
def test_batch_across_radius_tiles(vc, monkeypatch, capfd, sid, route, name):
    """4 097 copies of the six queries in one call: six full tiles of MIH_RADIUS_TILE queries and a last one of six, whose segments
    the offsets kernel places behind the earlier tiles'; every row checked"""
    import torch
    sh = F.SHAPES[sid]
    _set_route(monkeypatch, route)
    R = F.TILE_R
    q = np.ascontiguousarray(np.tile(F.make_queries(sid), (F.TILE_COPIES, 1)))
    rows = [F.expect(sid, "", route, R, qi) for qi in range(F.NQ)] * F.TILE_COPIES
    assert len(q) == len(rows) == F.TILE_COPIES * F.NQ and len(q) % F.LIMITS.MIH_RADIUS_TILE == F.NQ
    with vc.Engine(sh.bits, capacity=sh.n, n_tables=sh.m, id_base=sh.id_base, cand_cap=F.CAND_CAP) as e:
        e.add_codes(F.make_codes(sid))
        e.build_index()
        capfd.readouterr()
        _host_call(vc, e._h, e._L.vc_search_radius, q, R, vc.MODE_MIH_EXACT, rows, (sid, route))
        _check_trace(_attempts(capfd), sid, R, name, Ring(), rows, (sid, route))
        _dev_call(vc, torch, torch.cuda.Stream(), e, q, R, vc.MODE_MIH_EXACT, rows, (sid, route))
        _check_trace(_attempts(capfd), sid, R, name, None, rows, (sid, route))
