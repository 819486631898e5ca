"""Long-lived handles: a result depends only on the database and the call, never on the calls made before it.

Every other GPU test creates an engine, makes one to three calls and destroys it.  Here ONE handle per shape answers a long
seeded sequence of heterogeneous calls (call_history_common.py: form x mode x k x nq x order x stats x query kind x stream x
radius), the same multiset of calls in three orders -- descending by nq * k (everything after the first call runs inside grown
buffers full of another layout's data), ascending (every call grows something) and shuffled (with the named adjacent pairs:
far -> near batches and back, radius -> larger k and back, LINEAR -> MIH, device form on a side stream -> host form) -- and

  (a) EVERY row of EVERY call equals an expectation computed without the engine: the numpy model of the exact radius loop
      (oracle.MihExactModel, pinned against the oracle's SearchWorker::find in test_call_history_cpu.py), brute-force distances
      for LINEAR and the radius searches, MihOracle.find for approximate mode;
  (b) every later occurrence of a call -- in the same handle and in the other two orders -- returns bit-identical rows, counts,
      offsets and statistics.

Batches tile a pool of 60 distinct queries, so the expectation is computed once per distinct query and compared for every row.
The cross-call state this walks over: ensure_tile's carving of d_tile (k-NN and radius layouts), the ring allocated at the first
hand-over, the MihCounters block and its mapped sequence numbers, the radius totals, VcMihIndex::group_hint, the engine's
grow() buffers with the recovery barrier, and the sharded driver's DevBuf::grow.
"""
import ctypes as C
import hashlib

import numpy as np
import pytest

import call_history_common as H

pytestmark = pytest.mark.gpu

SH = np.uint64(32)
INF = np.uint64(0xFFFFFFFFFFFFFFFF)
STAT_FIELDS = ("radius", "n_results", "n_main_reads", "n_sub_reads", "n_local_reads", "n_candidates")


# ----------------------------------------------------------------------------- expectations (no engine involved)
class Expect:
    """per distinct query of the pool: the sorted (dist, id) of the whole database and the exact model, built once"""

    def __init__(self, oracle, codes, queries, m, id_base):
        self.vo, self.codes, self.q, self.m, self.id_base = oracle, codes, queries, m, id_base
        self.n = codes.shape[0]
        self._model, self._exact, self._approx, self._mo = {}, {}, {}, None

    def model(self, i):
        if i not in self._model:
            self._model[i] = self.vo.MihExactModel(self.codes, self.q[i], self.m, self.id_base)
        return self._model[i]

    def linear(self, i, k):
        row = self.model(i).packed[:k]
        return row, (0, len(row), 0, 0, 0, self.n)

    def exact(self, i, k):
        if (i, k) not in self._exact:
            row, st = self.model(i).find(k)
            self._exact[(i, k)] = (row, tuple(st[f] for f in STAT_FIELDS))
        return self._exact[(i, k)]

    def approx(self, i, k):
        """MihOracle.find decides the radius and the counters; the row is the engine's canonical rule at that radius"""
        if (i, k) not in self._approx:
            if self._mo is None:
                self._mo = self.vo.MihOracle(self.codes, self.m, key_mode=1, id_base=self.id_base)
            ores, ost = self._mo.find(self.q[i], k, approximate=True, stop_mult=4)
            mdl = self.model(i)
            row = mdl.packed[np.flatnonzero(mdl.minsub <= ost.radius)[:k]]
            assert np.array_equal(row >> SH, np.sort(ores) >> SH)
            self._approx[(i, k)] = (row, (ost.radius, len(row), 0, ost.n_sub_reads, 0, ost.n_distinct))
        return self._approx[(i, k)]

    def knn(self, mode, i, k):
        return (self.linear, self.exact, self.approx)[mode](i, k)

    def within(self, i, radius):
        p = self.model(i).packed
        return p[: int(np.searchsorted(p, np.uint64((radius + 1) << 32)))]


def _padded(rows, k):
    out = np.full((len(rows), k), INF, dtype=np.uint64)
    for j, r in enumerate(rows):
        out[j, : len(r)] = r
    return out


def expected_knn(exp, c, idx):
    """rows [nq, k] (INF behind the count), counts [nq], statistics [nq, 6] of a k-NN call, tiled from the distinct queries"""
    distinct = sorted(set(idx.tolist()))
    per = [exp.knn(c.mode, i, c.k) for i in distinct]
    pos = np.searchsorted(distinct, idx)
    rows = _padded([p[0] for p in per], c.k)[pos]
    counts = np.array([len(p[0]) for p in per], dtype=np.uint32)[pos]
    stats = np.array([p[1] for p in per], dtype=np.uint64)[pos]
    return rows, counts, stats


def expected_radius(exp, c, idx):
    distinct = sorted(set(idx.tolist()))
    per = [exp.within(i, c.radius) for i in distinct]
    pos = np.searchsorted(distinct, idx)
    lens = np.array([len(p) for p in per], dtype=np.uint64)[pos]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    flat = np.concatenate([per[j] for j in pos]) if len(pos) else np.empty(0, dtype=np.uint64)
    return flat.astype(np.uint64), offs


def _stats_host(stats):
    return np.array([[getattr(s, f) for f in STAT_FIELDS] for s in stats], dtype=np.uint64)


def _stats_dev(t):
    raw = np.ascontiguousarray(t.cpu().numpy()).view(np.uint8).reshape(-1, 40)
    return np.concatenate([raw[:, :8].copy().view(np.uint32).astype(np.uint64), raw[:, 8:].copy().view(np.uint64)], axis=1)


def _digest(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(b"-" if a is None else np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _assert_rows(got, want, what):
    """every row of the call; the message names the first entry that differs"""
    if not np.array_equal(got, want):
        assert got.shape == want.shape, (what, got.shape, want.shape)
        diff = (got != want).reshape(len(got), -1)
        rows = np.flatnonzero(diff.any(axis=1))
        r, col = int(rows[0]), int(np.flatnonzero(diff[rows[0]])[0])
        raise AssertionError("%s: %d of %d rows differ; first at row %d, column %d: got %#x, want %#x" % (
            what, len(rows), len(got), r, col, int(got.reshape(len(got), -1)[r, col]), int(want.reshape(len(got), -1)[r, col])))


# ----------------------------------------------------------------------------- one call on one handle
class Runner:
    """issues a Call on an Engine or a ShardedEngine and returns what came back as numpy arrays"""

    def __init__(self, vc, handle, queries, sharded=False):
        import torch
        self.torch, self.vc, self.h, self.q, self.sharded = torch, vc, handle, queries, sharded
        self.side = torch.cuda.Stream()
        self.dq = torch.from_numpy(queries).cuda()
        torch.cuda.synchronize()

    def _stream(self, c):
        return {"null": None, "side": self.side.cuda_stream}[c.stream]

    def _host_stream(self, c, on):
        if c.stream == "set_side":                       # vc_set_stream: the host-pointer calls move to a torch side stream ...
            self.h.set_stream(C.c_void_p(self.side.cuda_stream) if on else self.vc.STREAM_OWN)   # ... and back to the engine's own

    def knn(self, c, idx):
        torch = self.torch
        if c.form == "knn":
            self._host_stream(c, True)
            try:
                res = self.h.search_knn(self.q[idx], c.k, mode=c.mode, order=c.order, with_stats=c.stats)
            finally:
                self._host_stream(c, False)
            return res[0], res[1], (_stats_host(res[2]) if c.stats else None)
        dq = self.dq[torch.from_numpy(idx).cuda()].contiguous()
        out = torch.full((c.nq, c.k), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")   # never-valid fill: every entry must be written
        cnt = torch.full((c.nq,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        stat = torch.full((c.nq, 5), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda") if c.form == "knn_dev_stats" else None
        torch.cuda.synchronize()
        if self.sharded:
            self.h.search_knn_dev(dq.data_ptr(), c.nq, c.k, out.data_ptr(), cnt.data_ptr(),
                                  d_stats=stat.data_ptr() if stat is not None else None, mode=c.mode, stream=self._stream(c))
        elif stat is not None:
            self.h.search_knn_dev_stats(dq.data_ptr(), c.nq, c.k, out.data_ptr(), cnt.data_ptr(), stat.data_ptr(), mode=c.mode,
                                        stream=self._stream(c))
        else:
            self.h.search_knn_dev(dq.data_ptr(), c.nq, c.k, out.data_ptr(), cnt.data_ptr(), mode=c.mode, stream=self._stream(c))
        torch.cuda.synchronize()
        return (out.cpu().numpy().view(np.uint64), cnt.cpu().numpy().view(np.uint32), _stats_dev(stat) if stat is not None else None)

    def radius_host(self, c, idx, cap):
        """raw vc_search_radius / vc_sharded_search_radius: (rc, out, offsets)"""
        q = np.ascontiguousarray(self.q[idx])
        offs = np.zeros(c.nq + 1, dtype=np.uint64)
        out = np.full(max(cap, 1), INF, dtype=np.uint64)
        fn = self.h._L.vc_sharded_search_radius if self.sharded else self.h._L.vc_search_radius
        self._host_stream(c, True)
        try:
            rc = fn(self.h._h, q.ctypes.data_as(C.c_void_p), c.nq, c.radius, c.mode, out.ctypes.data_as(C.c_void_p), cap,
                    offs.ctypes.data_as(C.c_void_p))
        finally:
            self._host_stream(c, False)
        return rc, out, offs

    def radius_dev(self, c, idx, cap):
        torch = self.torch
        dq = self.dq[torch.from_numpy(idx).cuda()].contiguous()
        d_off = torch.full((c.nq + 1,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        d_out = torch.full((max(cap, 1),), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        rc = self.h.search_radius_dev(dq.data_ptr(), c.nq, c.radius, d_out.data_ptr(), cap, d_off.data_ptr(), mode=c.mode,
                                      stream=self._stream(c))
        torch.cuda.synchronize()
        return rc, d_out.cpu().numpy().view(np.uint64), d_off.cpu().numpy().view(np.uint64)


def run_and_check(vc, run, c, expect_knn, expect_radius, seen, key, evidence=None):
    """property (a) for every row of the call, property (b) against every earlier occurrence of it (`seen`: digests by call)"""
    idx = H.batch_index(c.kind, c.nq, c.start)
    what = "%s %r" % (key, tuple(c))
    timer = getattr(run.h, "timing", None)
    if timer:
        timer()                                                            # reset: the evidence below is this call's own
    if c.is_radius:
        flat, offs = expect_radius(c, idx)
        total = int(offs[-1])
        small = c.form.endswith("_small")
        if small:
            assert total >= 2, what
        cap = total // 2 if small else total + 10
        rc, out, got_offs = (run.radius_dev if c.form.startswith("radius_dev") else run.radius_host)(c, idx, cap)
        assert rc == (vc.VC_ERR_CAPACITY if small else vc.VC_OK), (what, rc)
        _assert_rows(got_offs, offs, what + " offsets")                   # too small: the needed counts are in the offsets
        if not small:
            _assert_rows(out[:total], flat, what + " results")
        dig = _digest(got_offs, None if small else out[:total])
    else:
        rows, counts, stats = expect_knn(c, idx)
        if c.order == 1:
            assert np.all(counts == c.k), what
            rows = rows[:, ::-1]
        got, cnt, st = run.knn(c, idx)
        _assert_rows(cnt, counts, what + " counts")
        _assert_rows(got, rows, what + " rows")
        if st is not None:
            for f, name in enumerate(STAT_FIELDS):                          # field by field
                _assert_rows(st[:, f], stats[:, f], what + " statistics." + name)
        if c.form == "knn_dev_stats":                                       # the device statistics equal the host form's too
            hc = H.knn("knn", c.mode, c.k, c.nq, c.kind, "own", 0, True, c.start)
            hgot, hcnt, hst = run.knn(hc, idx)
            _assert_rows(hgot, got, what + " host-form rows")
            _assert_rows(hcnt, cnt, what + " host-form counts")
            _assert_rows(hst, st, what + " host-form statistics")
        dig = _digest(got, cnt, st)
        if evidence is not None and st is not None:
            evidence.setdefault("radii", {})[c] = st[:, 0]
    if timer and evidence is not None:
        t = timer()
        evidence.setdefault("timing", {})[c] = (t.mih_launches, t.scan_launches)
    assert seen.setdefault((key, c), dig) == dig, what + ": differs from an earlier occurrence of the same call"


# ----------------------------------------------------------------------------- single engines: the full alphabet
CONFIGS = {
    # name: bits, m, id_base (None: the top of the id range), knobs
    "128x4": (128, 4, 1000, {}),
    "64x2": (64, 2, 77, {}),
    "64x4": (64, 4, 500_000, {}),
    "64x4-stream": (64, 4, 500_000, {"VC_MIH_STREAM": "2"}),             # the bucket-streaming kernel for every radius search
    "256x8": (256, 8, 3, {}),
    "128x4-top-ids": (128, 4, None, {}),                                  # packed ids at the top of the 32-bit range
}
_cache = {}
_seen = {}          # (config, call) -> digest of what it returned: across the three orders, each on a fresh handle


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_expectations():
    """the cached models hold MihOracle handles: released here, while the oracle library is still loaded"""
    yield
    _cache.clear()


def _config(oracle, name):
    bits, m, id_base, knobs = CONFIGS[name]
    key = (bits, m, id_base)
    if key not in _cache:
        _cache.clear()                                                    # one data set's models at a time
        codes = H.make_codes(oracle, bits, m)
        base = 2 ** 32 - len(codes) if id_base is None else id_base
        q = H.make_queries(codes, bits, m)
        _cache[key] = (codes, q, base, Expect(oracle, codes, q, m, base))
    return (bits, m, knobs) + _cache[key]


@pytest.mark.parametrize("order", ["descending", "ascending", "shuffled"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_any_order_of_the_calls_returns_the_same(vc, oracle, monkeypatch, name, order):
    bits, m, knobs, codes, q, id_base, exp = _config(oracle, name)
    monkeypatch.setenv("VC_MIH_QTILE", "4096")                            # knobs are read at vc_create
    for kn, v in knobs.items():
        monkeypatch.setenv(kn, v)
    seq = H.orders(m, seed=m)[order]
    named = H.named_calls(m)
    evidence = {}
    with vc.Engine(bits, capacity=len(codes), n_tables=m, id_base=id_base) as e:
        e.add_codes(codes)
        e.build_index()
        run = Runner(vc, e, q)
        for c in seq:
            run_and_check(vc, run, c, lambda c, idx: expected_knn(exp, c, idx), lambda c, idx: expected_radius(exp, c, idx),
                          _seen, name, evidence)
            assert e.device_status() == 0
    # route evidence: the sequence really took the routes it is meant to walk over
    far = evidence["radii"][named["far"]]
    if bits // m == 32:
        assert evidence["timing"][named["tiles"]][0] >= 3                 # 9000 queries = three launches, the last one partial
        assert evidence["timing"][named["switch"]][1] > 0                 # uniform queries: the cost model switched to the verify kernel
        assert int((far >= 2).sum()) * 10 >= len(far) * 6                 # the far batch is one that moves group_hint to 3


# ----------------------------------------------------------------------------- the scan fallback's tile, the clean state's layout
def test_fallback_tile_and_group_layout_do_not_leak(vc, oracle, monkeypatch, capfd):
    """query_tile = 4 and every exact MIH query handed to the verify kernel (VC_MIH_SWITCH=2), which scans in tiles of 32 whatever
    the engine's tile is.  LINEAR calls before and after it keep the engine's tile -- every verify launch of theirs names qt <= 4 --
    and three group layouts follow each other on one state buffer (GQ 5, GQ 40 in the fallback, GQ 64 in two groups): a state
    handed back clean for one layout is not taken for clean by the next.  Both orders of the calls return the same, exact rows."""
    import scan_shapes_common as S
    bits, m, id_base, k = 128, 4, 300, 10
    monkeypatch.setenv("VC_MIH_SWITCH", "2")                              # knobs are read at vc_create
    monkeypatch.setenv("VC_SCAN_SHAPE_TRACE", "1")
    codes = H.make_codes(oracle, bits, m, n=20_000)
    q = H.make_queries(codes, bits, m)
    exp = Expect(oracle, codes, q, m, id_base)
    # (uniform queries: their k-th distance lies shells beyond the query kernel's own, so they do reach the forced switch)
    calls = [H.knn("knn", H.LINEAR, k, 5, "near"), H.knn("knn", H.EXACT, k, 40, "uniform"), H.knn("knn_dev", H.LINEAR, k, 70, "far", stream="null")]
    for i in range(len(q)):                                               # LINEAR rows: the oracle's scan, not the model's sort
        assert np.array_equal(exp.linear(i, k)[0], oracle.linear_knn(codes, q[i], k, id_base=id_base))
    seen = {}
    for seq in (calls, calls[::-1]):
        with vc.Engine(bits, capacity=len(codes), n_tables=m, id_base=id_base, query_tile=4) as e:
            e.add_codes(codes)
            e.build_index()
            run = Runner(vc, e, q)
            for c in seq:
                capfd.readouterr()
                run_and_check(vc, run, c, lambda c, idx: expected_knn(exp, c, idx), None, seen, "tile")
                tiles = [t["qt"] for t in S.parse_trace(capfd.readouterr().err)]
                print("%r: verify tiles %s" % (tuple(c), tiles))
                if c.mode == H.LINEAR:
                    want = [4] * (c.nq // 4) + [c.nq % 4] * (c.nq % 4 != 0)       # (a group of 64 is whole tiles: 70 = 16 x 4, then 4 + 2)
                    assert tiles == want, (tuple(c), tiles)
                else:
                    # the forced switch hands all 40 unfinished queries over at once: one group of 40 in the fallback's tile of 32
                    assert tiles == [32, 8], (tuple(c), tiles)
                assert e.device_status() == 0


# ----------------------------------------------------------------------------- ring-overflow history
def test_ring_overflow_history(vc, oracle):
    """duplicate-heavy clusters behind a small candidate ring: LINEAR batches whose rows overflow the ring (thousands of ties at the
    k-th distance: device-side recovery, barrier words, d_rec) alternate with batches that do not (lone codes, k = 1), and with
    exact MIH batches whose shells overflow the work ring and go through the redo round (k = 3500: every shell in the multi-block
    kernels).  Every row exact, vc_device_status 0 throughout."""
    bits, m, id_base = 128, 4, 40
    dup = oracle.gen_codes(80_000, bits, 34, kind=1, n_centres=8, max_flips=2)       # ~10 000 items per cluster (test_mih_overflow_recovery)
    codes = np.concatenate([dup, oracle.gen_codes(3000, bits, 9)])                   # + lone codes
    rng = np.random.default_rng(12)
    near = dup[rng.integers(0, len(dup), size=H.POOL)].copy()
    near[::2, 3] ^= 0x10
    lone = codes[len(dup) + rng.integers(0, 3000, size=H.POOL)].copy()
    q = np.concatenate([near, lone, rng.integers(0, 256, size=(H.POOL, bits // 8), dtype=np.uint8)])   # kinds: near, "far" = lone, uniform
    exp = Expect(oracle, codes, q, m, id_base)
    for i in range(len(q)):                                               # LINEAR rows: the oracle's scan, not the model's sort
        assert np.array_equal(exp.linear(i, 100)[0], oracle.linear_knn(codes, q[i], 100, id_base=id_base))
    over = [H.knn("knn", H.LINEAR, 100, 33, "near"), H.knn("knn_dev", H.LINEAR, 100, 700, "uniform", stream="side"),
            H.knn("knn_dev_stats", H.LINEAR, 7, 5, "near", stream="null"), H.knn("knn", H.LINEAR, 1000, 33, "uniform", order=1)]
    calm = [H.knn("knn", H.LINEAR, 1, 33, "far"), H.knn("knn_dev", H.LINEAR, 1, 5, "far", stream="null")]
    mih = [H.knn("knn", H.EXACT, 100, 33, "near"), H.knn("knn", H.EXACT, 3500, 5, "near"),
           H.knn("knn_dev_stats", H.EXACT, 1000, 33, "near", stream="side"), H.knn("knn", H.EXACT, 1, 700, "far", stats=False)]
    seq = []
    for r in range(3):
        for j in range(4):
            seq += [over[(j + r) % 4], calm[j % 2], mih[(j + 2 * r) % 4]]
    seen = {}
    with vc.Engine(bits, capacity=len(codes), n_tables=m, id_base=id_base, cand_cap=512) as e:
        e.add_codes(codes)
        e.build_index()
        run = Runner(vc, e, q)
        for c in seq:
            run_and_check(vc, run, c, lambda c, idx: expected_knn(exp, c, idx), None, seen, "ring")
            assert e.device_status() == 0


# ----------------------------------------------------------------------------- ingest history
def test_ingest_history(vc, oracle):
    """vc_add_codes in three uneven pieces with a LINEAR search after each (the staging buffer and the scan's state grow with the
    database under a live handle), each equal to the oracle over the prefix; then vc_build_index and MIH calls"""
    bits, m, id_base = 128, 4, 123
    codes = H.make_codes(oracle, bits, m, n=30_000)
    q = H.make_queries(codes, bits, m)
    idx = np.arange(len(q))
    with vc.Engine(bits, capacity=len(codes), n_tables=m, id_base=id_base) as e:
        done = 0
        for piece, k in ((7000, 100), (1, 1000), (22_999, 7)):
            e.add_codes(codes[done:done + piece])
            done += piece
            assert len(e) == done
            got, cnt = e.search_knn(q, k)
            want = np.stack([oracle.linear_knn(codes[:done], q[i], k, id_base=id_base) for i in idx])
            _assert_rows(cnt, np.full(len(q), k, dtype=np.uint32), "prefix %d counts" % done)
            _assert_rows(got, want, "prefix %d rows" % done)
            with pytest.raises(vc.VcError) as ei:                         # no index over this prefix yet
                e.search_knn(q[:1], 5, mode=vc.MODE_MIH_EXACT)
            assert ei.value.code == vc.VC_ERR_STATE
        e.build_index()
        exp = Expect(oracle, codes, q, m, id_base)
        run = Runner(vc, e, q)
        seen = {}
        for c in (H.knn("knn", H.EXACT, 100, 33, "near"), H.knn("knn", H.EXACT, 7, 700, "far"), H.knn("knn", H.LINEAR, 100, 33, "near"),
                  H.rad("radius", H.EXACT, 8, 33, "near"), H.knn("knn", H.EXACT, 100, 33, "near")):
            run_and_check(vc, run, c, lambda c, idx: expected_knn(exp, c, idx), lambda c, idx: expected_radius(exp, c, idx), seen, "ingest")


# ----------------------------------------------------------------------------- sharded handles
class ShardedExpect:
    """the union's expectation (LINEAR, radius, exact mode with VC_FLAG_GLOBAL_STOP) and the shards' own (every shard runs to its
    own stop rule: merged rows, the widest radius, summed reads and candidates)"""

    def __init__(self, oracle, codes, queries, m, id_base, ranges, global_stop):
        self.union = Expect(oracle, codes, queries, m, id_base)
        self.parts = [Expect(oracle, codes[lo - id_base: lo - id_base + cnt], queries, m, lo) for lo, cnt in ranges if cnt]
        self.global_stop = global_stop
        self._merged = {}

    def knn(self, mode, i, k):
        if mode == H.LINEAR or (mode == H.EXACT and self.global_stop):
            return self.union.knn(mode, i, k)
        if (mode, i, k) not in self._merged:
            per = [p.knn(mode, i, k) for p in self.parts]
            row = np.sort(np.concatenate([r for r, _ in per]))[:k]
            st = np.array([s for _, s in per], dtype=np.uint64)
            stats = (int(st[:, 0].max()), len(row), 0, int(st[:, 3].sum()), int(st[:, 4].sum()), int(st[:, 5].sum()))
            if mode == H.EXACT:                                           # exact for every shard: the union's distances
                assert np.array_equal(row >> SH, self.union.exact(i, k)[0] >> SH)
            self._merged[(mode, i, k)] = (row, stats)
        return self._merged[(mode, i, k)]

    def within(self, i, radius):
        return self.union.within(i, radius)


def sharded_calls():
    """the smaller alphabet: host and device forms, d_stats on and off, LINEAR / EXACT / APPROX, radius searches with the
    VC_ERR_CAPACITY case, k in {1, 100, 1000}, nq in {1, 33, 700}"""
    return [
        H.knn("knn", H.EXACT, 100, 700, "near"), H.knn("knn", H.EXACT, 1000, 33, "near", stats=False, order=1),
        H.knn("knn", H.EXACT, 1, 1, "uniform"), H.knn("knn_dev_stats", H.EXACT, 100, 33, "far", stream="side"),
        H.knn("knn_dev", H.EXACT, 1, 700, "far", stream="null"), H.knn("knn_dev_stats", H.EXACT, 1000, 1, "uniform", stream="null"),
        H.knn("knn", H.EXACT, 100, 33, "uniform"),
        H.knn("knn", H.LINEAR, 1000, 700, "near", order=1), H.knn("knn_dev_stats", H.LINEAR, 100, 33, "uniform", stream="side"),
        H.knn("knn", H.LINEAR, 1, 1, "far"),
        H.knn("knn", H.APPROX, 1, 33, "near"), H.knn("knn_dev_stats", H.APPROX, 1, 700, "near", stream="side"),
        H.rad("radius", H.EXACT, 8, 33, "near"), H.rad("radius", H.LINEAR, 10, 700, "near"), H.rad("radius", H.EXACT, 0, 1, "uniform"),
        H.rad("radius_small", H.EXACT, 8, 700, "near"),
    ]


def sharded_orders():
    calls = sharded_calls()
    twice = [(c, occ) for occ in range(2) for c in calls]
    perm = np.random.default_rng(7).permutation(len(twice))
    return {"descending": [c for c, _ in sorted(twice, key=lambda co: (-co[0].size, co[1]))],
            "ascending": [c for c, _ in sorted(twice, key=lambda co: (co[0].size, co[1]))],
            "shuffled": [twice[i][0] for i in perm]}


_sharded_seen = {}


@pytest.mark.parametrize("order", ["descending", "ascending", "shuffled"])
@pytest.mark.parametrize("global_stop", [False, True])
@pytest.mark.parametrize("shards,capacity", [(3, 24_000), (8, 64_000)])        # 8 shards: capacity above the record count, five stay empty
def test_sharded_any_order_of_the_calls_returns_the_same(vc, oracle, shards, capacity, global_stop, order):
    bits, m, n, id_base = 128, 4, 24_000, 2000
    codes = H.make_codes(oracle, bits, m, n=n)
    q = H.make_queries(codes, bits, m)
    with vc.ShardedEngine(bits, capacity=capacity, n_shards=shards, n_tables=m, devices=[0], id_base=id_base,
                          flags=vc.FLAG_GLOBAL_STOP if global_stop else 0) as s:
        s.add_codes(codes[:5000])
        s.add_codes(codes[5000:])
        s.build_index()
        assert len(s) == n
        slices = [s.shard_range(g) for g in range(shards)]                # the id range a shard may hold: capacity / shards wide
        assert slices[0][0] == id_base and all(cnt == capacity // shards for _, cnt in slices)
        ranges = [(lo, len(s.shard(g))) for g, (lo, _) in enumerate(slices)]   # ... and the records it does hold
        assert all(cnt == min(max(id_base + n - lo, 0), capacity // shards) for lo, cnt in ranges)   # filled one after the other
        assert sum(cnt for _, cnt in ranges) == n and (shards == 3 or sum(cnt == 0 for _, cnt in ranges) == 5)
        key = (shards, global_stop)
        if key not in _cache:
            _cache.clear()
            _cache[key] = ShardedExpect(oracle, codes, q, m, id_base, ranges, global_stop)
        exp = _cache[key]
        run = Runner(vc, s, q, sharded=True)
        for c in sharded_orders()[order]:
            run_and_check(vc, run, c, lambda c, idx: expected_knn(exp, c, idx), lambda c, idx: expected_radius(exp, c, idx),
                          _sharded_seen, "sharded-%d-%s" % (shards, "global" if global_stop else "own"))
