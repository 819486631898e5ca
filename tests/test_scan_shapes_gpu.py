"""Every compiled shape of vc_scan_kernel inside its multi-chunk loop.  Engine(scan_blocks=...) caps the grid at one or two
blocks over databases of three or seven chunks, so a block walks up to seven chunks: every exit of the loop, the re-use of
each register buffer, the parked prefetch cursor and the rare path under a tile in flight -- the state a 1e9-row pass is
in, at no more than 28 672 codes.  Every row and count of every call is compared bit for bit with the numpy brute force
of scan_shapes_common (whose inputs test_scan_shapes_cpu.py pins), and VC_SCAN_SHAPE_TRACE=1 shows on stderr which
instantiation each launch really ran, its grid and its chunk count."""
import numpy as np
import pytest

import scan_shapes_common as S

pytestmark = pytest.mark.gpu

DB_OF_NB = {1: 0, 2: 2, 3: 3}    # third field of VC_SCAN_SHAPE (vc_scan_pick_shape): 0 -> one buffer, 1 / 2 -> two, 3 -> three


def _search_twice(e, capfd, q, k, exp, what):
    """one search compared with the expectation, then the same search again on the same engine: identical bits.
    Returns the [scan shape] lines of the first call."""
    rows, counts = exp
    capfd.readouterr()
    got, cnt = e.search_knn(q, k)
    trace = S.parse_trace(capfd.readouterr().err)
    assert np.array_equal(cnt, counts), what
    if not np.array_equal(got, rows):
        bad = np.argwhere(got != rows)
        r, c = (int(x) for x in bad[0])
        raise AssertionError("%s: %d entries differ, first at row %d slot %d: got dist %d id %d, expected dist %d id %d" % (
            what, len(bad), r, c, got[r, c] >> np.uint64(32), got[r, c] & np.uint64(0xFFFFFFFF),
            rows[r, c] >> np.uint64(32), rows[r, c] & np.uint64(0xFFFFFFFF)))
    again, cnt2 = e.search_knn(q, k)
    assert np.array_equal(again, got) and np.array_equal(cnt2, cnt), what + " (repeated)"
    return trace


def _check_trace(trace, tiles, sz, w, u, blk, nb, small, what):
    """one line per verify launch, in launch order: the instantiation, the grid and the chunk count"""
    assert [t["qt"] for t in trace] == tiles, (what, trace)
    for t in trace:
        assert (t["W"], t["U"], t["BLK"], t["NB"]) == (w, u, blk, nb), (what, t)
        assert t["QT"] == (t["qt"] if small else 0), (what, t)
        assert t["grid"] == (sz.scan_blocks or sz.nchunks), (what, t)
        assert t["nchunks"] == sz.nchunks == -(-sz.n // (2 * blk * u)), (what, t)
    return {(t["W"], t["U"], t["BLK"], t["NB"], t["QT"]) for t in trace}


@pytest.fixture(scope="module")
def expected():
    """the numpy expectation of (bits, U, BLK, size, kind, first query, nq, k), computed once and shared"""
    cache = {}

    def get(bits, u, blk, size_name, kind, first, nq, k):
        key = (bits, u, blk, size_name, kind, first, nq, k)
        if key not in cache:
            d = S.data(bits, u, blk, size_name, kind)
            rows, counts = S.expect(d.codes, d.queries[first:first + nq], k, S.size(size_name, u, blk).id_base)
            rows.setflags(write=False)
            counts.setflags(write=False)
            cache[key] = (rows, counts)
        return cache[key]
    return get


@pytest.mark.parametrize("bits,u,blk,nb", S.general_shapes())
def test_general_form_shape(vc, monkeypatch, capfd, expected, bits, u, blk, nb):
    monkeypatch.setenv("VC_SCAN_SHAPE", "%d,%d,%d" % (u, blk, DB_OF_NB[nb]))
    monkeypatch.setenv("VC_SCAN_SMALL", "0")
    monkeypatch.setenv("VC_SCAN_SHAPE_TRACE", "1")
    launched = set()
    for size_name in S.SIZES:
        sz = S.size(size_name, u, blk)
        for kind in S.KINDS:
            d = S.data(bits, u, blk, size_name, kind)
            with vc.Engine(bits, capacity=sz.capacity, id_base=sz.id_base, scan_blocks=sz.scan_blocks, query_tile=11) as e:
                e.add_codes(d.codes)
                assert len(e) == sz.n
                for first, nq, k in S.calls(kind):
                    what = "W=%d U=%d BLK=%d NB=%d %s %s q%d+%d k=%d" % (bits // 64, u, blk, nb, size_name, kind, first, nq, k)
                    trace = _search_twice(e, capfd, d.queries[first:first + nq], k,
                                          expected(bits, u, blk, size_name, kind, first, nq, k), what)
                    launched |= _check_trace(trace, [11, 2] if nq == 13 else [nq], sz, bits // 64, u, blk, nb, False, what)
    print("launched (W, U, BLK, NB, QT):", sorted(launched))
    assert launched == {(bits // 64, u, blk, nb, 0)}


@pytest.mark.parametrize("tau_fold", [None, "0", "1"])
@pytest.mark.parametrize("bits", S.BITS)
def test_small_tile_form(vc, monkeypatch, capfd, expected, bits, tau_fold):
    """query_tile = 8 and 8..15 queries: a full tile and a tail tile of every QT = 1..7.  VC_TAU_FOLD unset and 0 are the
    product's path (thresholds cut by vc_tau_init_kernel); 1 makes the kernel's own prologue cut them."""
    if tau_fold is None:
        monkeypatch.delenv("VC_TAU_FOLD", raising=False)
    else:
        monkeypatch.setenv("VC_TAU_FOLD", tau_fold)
    monkeypatch.setenv("VC_SCAN_SHAPE_TRACE", "1")
    u = S.small_unroll(bits)
    launched = set()
    for size_name in S.SIZES:
        sz = S.size(size_name, u, 256)
        for kind in S.KINDS:
            d = S.data(bits, u, 256, size_name, kind)
            seen = set()
            with vc.Engine(bits, capacity=sz.capacity, id_base=sz.id_base, scan_blocks=sz.scan_blocks, query_tile=8) as e:
                e.add_codes(d.codes)
                for first, nq, k in S.small_calls(kind):
                    what = "W=%d small %s %s nq=%d k=%d fold=%s" % (bits // 64, size_name, kind, nq, k, tau_fold)
                    trace = _search_twice(e, capfd, d.queries[first:first + nq], k,
                                          expected(bits, u, 256, size_name, kind, first, nq, k), what)
                    shapes = _check_trace(trace, [8] if nq == 8 else [8, nq - 8], sz, bits // 64, u, 256, 2, True, what)
                    seen |= {s[4] for s in shapes}
                    launched |= shapes
            assert seen == set(range(1, 9)), (size_name, kind, seen)
    print("launched (W, U, BLK, NB, QT):", sorted(launched))


@pytest.mark.parametrize("bits,nq", [(512, 640), (256, 4096)])
def test_default_pick_large_tiles(vc, monkeypatch, capfd, bits, nq):
    """no shape knob: a query tile above 40 KB of LDS (256 bits x 4096 is the config-5 tile) makes the picker take BLK = 512,
    and the tile is staged by a loop longer than the block; two blocks over the three chunks of a `short` database"""
    monkeypatch.setenv("VC_SCAN_SHAPE_TRACE", "1")
    u, k = S.small_unroll(bits), 10
    sz = S.size("short", u, 512)
    d = S.data(bits, u, 512, "short", "planted")
    q = S.large_tile_queries(d, bits, nq, 5)
    exp = S.expect(d.codes, q, k, sz.id_base)
    with vc.Engine(bits, capacity=sz.capacity, id_base=sz.id_base, scan_blocks=2, query_tile=nq) as e:
        e.add_codes(d.codes)
        what = "W=%d default pick, tile of %d" % (bits // 64, nq)
        trace = _search_twice(e, capfd, q, k, exp, what)
        print("launched (W, U, BLK, NB, QT):", sorted(_check_trace(trace, [nq], sz, bits // 64, u, 512, 2, False, what)))
