"""vc_sharded_search_radius_dev: the radius search over shards for callers that keep queries and results in HBM
(search_R_neighbors on every rank + gather_vectors + the master's dedup, search_worker.cc:177-199,222-264).  Every shard searches
its id range into its own buffer, two kernels on the root device make the union: its offsets, and a rank merge that places every
value by binary searches in the other shards' segments.  Every row is compared with a numpy brute force over the union and with
the host-pointer forms (ShardedEngine.search_radius, one Engine.search_radius), in both modes.  The shapes, their data and what
they guarantee are in sharded_radius_common.py / test_sharded_radius_dev_cpu.py."""
import contextlib

import numpy as np
import pytest

import sharded_radius_common as rc

pytestmark = pytest.mark.gpu
SENTINEL = np.int64(0x5A5A5A5A5A5A5A5A)


@contextlib.contextmanager
def _store(vc, oracle, name, devices=(0,), build=True, single=False):
    """ShardedEngine over a shape's data (+ one Engine over the union when `single`)"""
    bits, m, n, _, _, _, shards, capacity, _ = rc.SHAPES[name]
    codes = rc.case(oracle, name)[0]
    with contextlib.ExitStack() as st:
        s = st.enter_context(vc.ShardedEngine(bits, capacity=capacity, n_shards=shards, n_tables=m, devices=list(devices), id_base=rc.ID_BASE))
        s.add_codes(codes)
        one = None
        if single:
            one = st.enter_context(vc.Engine(bits, capacity=n, n_tables=m, id_base=rc.ID_BASE))
            one.add_codes(codes)
        if build:
            s.build_index()
            if one:
                one.build_index()
        yield (s, one) if single else s


def _rows(out, offs):
    """device tensors -> (list of per-query uint64 arrays, offsets); the caller has synchronised"""
    o = offs.cpu().numpy().view(np.uint64)
    flat = out.cpu().numpy().view(np.uint64)
    assert o[0] == 0 and np.all(o[1:] >= o[:-1])
    return [flat[int(o[i]):int(o[i + 1])] for i in range(len(o) - 1)], o


def _offsets_of(rows):
    return np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)


def _search(vc, s, torch, q, radius, mode, device="cuda"):
    """the two-pass use of the call: ask with no room (VC_ERR_CAPACITY, the needed counts in d_offsets), then with exactly enough"""
    dq = torch.from_numpy(q).to(device)
    offs = torch.zeros(len(q) + 1, dtype=torch.int64, device=device)
    r = s.search_radius_dev(dq.data_ptr(), len(q), radius, None, 0, offs.data_ptr(), mode=mode)
    torch.cuda.synchronize()
    total = int(offs[-1].item())
    assert r == (vc.VC_ERR_CAPACITY if total else vc.VC_OK)
    out = torch.full((total + 1,), SENTINEL, dtype=torch.int64, device=device)
    assert s.search_radius_dev(dq.data_ptr(), len(q), radius, out.data_ptr(), total, offs.data_ptr(), mode=mode) == vc.VC_OK
    torch.cuda.synchronize()
    assert int(out[total].item()) == SENTINEL
    return _rows(out[:total], offs)[0]


def _same(got, exp):
    return len(got) == len(exp) and all(np.array_equal(g, e) for g, e in zip(got, exp))


@pytest.mark.parametrize("name", ["interleaved", "heavy", "max_shards", "one_shard", "many_light"])
def test_rows_equal_the_union(vc, oracle, name):
    """shapes 1-5 in both modes: the numpy brute force over the union, the host-pointer call over the same shards and one engine
    over the union all give the rows the device-resident call gives (many_light: also a call of one query)"""
    import torch
    _, q, exp = rc.case(oracle, name)
    radius = rc.SHAPES[name][5]
    with _store(vc, oracle, name, single=True) as (s, one):
        for mode in (vc.MODE_MIH_EXACT, vc.MODE_LINEAR):
            got = _search(vc, s, torch, q, radius, mode)
            assert _same(got, exp)
            cap = max(len(r) for r in exp) + 1
            assert _same(s.search_radius(q, radius, mode=mode, cap_per_query=cap), got)
            assert _same(one.search_radius(q, radius, mode=mode, cap_per_query=cap), got)
            if name == "many_light":
                assert _same(_search(vc, s, torch, q[:1], radius, mode), exp[:1])


def test_capacity_contract(vc, oracle):
    """shape 1: too little room -> VC_ERR_CAPACITY, d_offsets = the needed counts, d_out untouched in every word (also with no
    buffer at all); exactly enough room -> VC_OK and nothing written behind d_out[total]"""
    import torch
    _, q, exp = rc.case(oracle, "interleaved")
    radius, nq = rc.SHAPES["interleaved"][5], len(q)
    want = _offsets_of(exp)
    total = int(want[-1])
    with _store(vc, oracle, "interleaved") as s:
        dq = torch.from_numpy(q).cuda()
        for mode in (vc.MODE_MIH_EXACT, vc.MODE_LINEAR):
            for cap, with_buffer in ((0, False), (total - 1, True)):
                out = torch.full((total + 1,), SENTINEL, dtype=torch.int64, device="cuda")
                offs = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
                r = s.search_radius_dev(dq.data_ptr(), nq, radius, out.data_ptr() if with_buffer else None, cap, offs.data_ptr(), mode=mode)
                torch.cuda.synchronize()
                assert r == vc.VC_ERR_CAPACITY
                assert np.array_equal(offs.cpu().numpy().view(np.uint64), want)
                assert bool((out == SENTINEL).all())
            out = torch.full((total + 1,), SENTINEL, dtype=torch.int64, device="cuda")
            offs = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
            assert s.search_radius_dev(dq.data_ptr(), nq, radius, out.data_ptr(), total, offs.data_ptr(), mode=mode) == vc.VC_OK
            torch.cuda.synchronize()
            assert int(out[total].item()) == SENTINEL
            got, o = _rows(out[:total], offs)
            assert np.array_equal(o, want) and _same(got, exp)


def test_streams_and_call_history(vc, oracle):
    """shape 1 on torch's current stream and on a side stream: two different batches back to back, nothing waited for in between,
    both right after one synchronise.  Then a heavy call on the same handle -- a handle holds one database, so it is shape 1's
    data at radius 64: every record is a neighbour of every query, 30 000 per row, which regrows every buffer of the path by two
    orders of magnitude and sends both modes through the scan -- and shape 1's call again: the same rows as the first time."""
    import torch
    codes, qa, expa = rc.case(oracle, "interleaved")
    _, qb, expb = rc.case(oracle, "interleaved", 1)
    radius, nq = rc.SHAPES["interleaved"][5], len(qa)
    assert not np.array_equal(qa, qb)
    with _store(vc, oracle, "interleaved") as s:
        dqa, dqb = torch.from_numpy(qa).cuda(), torch.from_numpy(qb).cuda()
        for mode in (vc.MODE_MIH_EXACT, vc.MODE_LINEAR):
            first = None
            for stream in (torch.cuda.current_stream(), torch.cuda.Stream()):
                bufs = [(torch.full((int(_offsets_of(e)[-1]) + 1,), SENTINEL, dtype=torch.int64, device="cuda"),
                         torch.zeros(nq + 1, dtype=torch.int64, device="cuda")) for e in (expa, expb)]
                torch.cuda.synchronize()
                with torch.cuda.stream(stream):
                    for dq, (out, offs) in zip((dqa, dqb), bufs):
                        assert s.search_radius_dev(dq.data_ptr(), nq, radius, out.data_ptr(), out.numel() - 1, offs.data_ptr(), mode=mode,
                                                   stream=stream.cuda_stream) == vc.VC_OK
                stream.synchronize()
                for exp, (out, offs) in zip((expa, expb), bufs):
                    assert int(out[-1].item()) == SENTINEL
                    assert _same(_rows(out[:-1], offs)[0], exp)
                first = first or [r.copy() for r in _rows(bufs[0][0][:-1], bufs[0][1])[0]]
            heavy = _search(vc, s, torch, qa, 64, mode)
            everything = np.arange(len(codes), dtype=np.uint64) + np.uint64(rc.ID_BASE)
            for i in range(nq):
                assert np.array_equal(heavy[i], np.sort(oracle.pack(oracle.np_distances(codes, qa[i]), everything)))
            assert _same(_search(vc, s, torch, qa, radius, mode), first)


def test_shard_side_regrow(vc, oracle):
    """a fresh handle whose first call is the heavy shape 2: every shard finds ~13 000 results where its buffer starts with 64 per
    query, grows it to the reported total inside the call and repeats; the rows are exact, and a light call and the heavy one
    again on the grown buffers give the same"""
    import torch
    _, q, exp = rc.case(oracle, "heavy")
    radius = rc.SHAPES["heavy"][5]
    for mode in (vc.MODE_MIH_EXACT, vc.MODE_LINEAR):
        with _store(vc, oracle, "heavy") as s:
            assert _same(_search(vc, s, torch, q, radius, mode), exp)
            assert _same(_search(vc, s, torch, q[-1:], radius, mode), exp[-1:])
            assert _same(_search(vc, s, torch, q, radius, mode), exp)


def test_refusals(vc, oracle):
    import torch
    _, q, _ = rc.case(oracle, "interleaved")
    radius, nq = rc.SHAPES["interleaved"][5], len(q)
    dq = torch.from_numpy(q).cuda()
    offs = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    out = torch.zeros(16, dtype=torch.int64, device="cuda")
    L = vc.load_library()
    assert L.vc_sharded_search_radius_dev(None, dq.data_ptr(), nq, radius, vc.MODE_LINEAR, out.data_ptr(), 16, offs.data_ptr(), None) == vc.VC_ERR_INVALID
    with _store(vc, oracle, "interleaved", build=False) as s:
        def code(*a, **kw):
            with pytest.raises(vc.VcError) as ei:
                s.search_radius_dev(*a, **kw)
            return ei.value.code
        assert code(None, nq, radius, out.data_ptr(), 16, offs.data_ptr(), mode=vc.MODE_LINEAR) == vc.VC_ERR_INVALID
        assert code(dq.data_ptr(), nq, radius, out.data_ptr(), 16, None, mode=vc.MODE_LINEAR) == vc.VC_ERR_INVALID
        assert code(dq.data_ptr(), 0, radius, out.data_ptr(), 16, offs.data_ptr(), mode=vc.MODE_LINEAR) == vc.VC_ERR_INVALID
        assert code(dq.data_ptr(), nq, radius, None, 16, offs.data_ptr(), mode=vc.MODE_LINEAR) == vc.VC_ERR_INVALID
        assert code(dq.data_ptr(), nq, radius, out.data_ptr(), 16, offs.data_ptr(), mode=vc.MODE_MIH_APPROX) == vc.VC_ERR_INVALID
        assert code(dq.data_ptr(), nq, radius, out.data_ptr(), 16, offs.data_ptr(), mode=vc.MODE_MIH_EXACT) == vc.VC_ERR_STATE   # no build_index yet
        torch.cuda.synchronize()
        assert bool((out == 0).all())


def test_two_devices(vc, oracle):
    """shape 1 across two GPUs: the queries travel by peer copy, the lanes run on host threads, the remote shards' offsets and
    results reach the root by peer copies under either exchange setting.  Skipped on a one-GPU box, like
    test_two_devices_both_exchanges: it runs wherever two devices are visible."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (the cross-device leg of vc_sharded_search_radius_dev has not run on hardware yet)")
    _, q, exp = rc.case(oracle, "interleaved")
    radius = rc.SHAPES["interleaved"][5]
    with torch.cuda.device(0), _store(vc, oracle, "interleaved", devices=(0, 1)) as s:
        assert s.root_device == 0
        for mode in (vc.MODE_MIH_EXACT, vc.MODE_LINEAR):
            for _ in range(2):
                assert _same(_search(vc, s, torch, q, radius, mode, device="cuda:0"), exp)
