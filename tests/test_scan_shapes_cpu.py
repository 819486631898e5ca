"""The cases of test_scan_shapes_gpu.py bite, checked without a GPU on the generator and the numpy expectation alone: the
sizes walk a block through every exit of the verify kernel's chunk loop, every planted row draws from every chunk, pair
slot, pair half, first and last lane and from item n - 1, the ties at the k-th distance outnumber the row's room and
straddle chunks and blocks, and no candidate ring can overflow.  Conditions on the inputs, not measurements."""
import numpy as np
import pytest

import scan_shapes_common as S

SH = np.uint64(32)
TILES = sorted({(bits, u, blk) for bits, u, blk, _ in S.general_shapes()})
CLUSTER = range(2, S.NQ)


def test_the_parametrisation_is_the_compiled_set():
    g = S.general_shapes()
    assert len(g) == len(set(g)) == 54
    assert set(g) == {(64 * w, u, blk, nb) for w in (1, 2, 4, 8) for u in (1, 2, 4) for blk in (256, 512) for nb in (1, 2, 3)
                      if u * w <= 8}
    assert [sum(1 for s in g if s[0] == b) for b in S.BITS] == [18, 18, 12, 6]
    s = S.small_forms()
    assert len(s) == len(set(s)) == 32 and {qt for _, qt in s} == set(range(1, 9))
    assert [S.small_unroll(b) for b in S.BITS] == [4, 4, 2, 1]
    assert all((bits, S.small_unroll(bits), 256, 2) in g for bits in S.BITS)   # the small form's tile is a general shape's too
    assert len(TILES) == 18


@pytest.mark.parametrize("bits,u,blk", TILES)
def test_sizes_walk_every_exit_of_the_chunk_loop(bits, u, blk):
    c = 2 * blk * u
    sz = {name: S.size(name, u, blk) for name in S.SIZES}
    assert sz["short"].chunks_per_block() == [2, 1] and sz["long"].chunks_per_block() == [4, 3]
    assert sz["solo"].chunks_per_block() == [7] and sz["wide"].chunks_per_block() == [1, 1, 1]
    assert {x for s in sz.values() for x in s.chunks_per_block()} == {1, 2, 3, 4, 7}
    assert sz["short"].n % 2 == 1 and sz["short"].n % c == 1            # the last chunk holds one item: the pair (n - 1, n) straddles n
    assert sz["long"].n % c == c - 1 and sz["solo"].n == sz["long"].n   # the last chunk lacks one item
    assert (sz["wide"].n, sz["wide"].scan_blocks, sz["wide"].grid(resident=256)) == (sz["short"].n, 0, 3)
    for s in sz.values():
        assert s.chunk == c and s.n <= S.MAX_N <= 65536                  # a ring of the default 65 536 entries cannot overflow
        assert s.nchunks == -(-s.n // c) and s.grid(resident=256) == (s.scan_blocks or s.nchunks)
        assert s.id_base + s.capacity <= 1 << 32 and s.capacity >= s.n
        assert (s.id_base == 0xFFFF0000) == (s.name == "short")
        assert (s.capacity == s.n + 5000) == (s.name in ("long", "solo"))
        # the last chunk's reach stays inside a column (the engine pads the column stride to 8192 items)
        assert s.nchunks * c <= -(-s.capacity // 8192) * 8192
    assert sz["long"].capacity > sz["long"].nchunks * c - 1             # rows beyond n inside the last chunk's reach exist


@pytest.mark.parametrize("size_name", ["short", "long"])
@pytest.mark.parametrize("bits,u,blk", TILES)
def test_planted_rows_draw_from_every_corner(bits, u, blk, size_name):
    sz = S.size(size_name, u, blk)
    d = S.data(bits, u, blk, size_name, "planted")
    n, nchunks = sz.n, sz.nchunks
    assert d.codes.shape == (n, bits // 8) and d.queries.shape == (S.NQ, bits // 8)
    assert not d.queries[0].any() and (d.queries[1] == 0xFF).all()
    dist = S.distances(d.codes, d.queries)
    # plants are 0..6 bits from every cluster query, the background is far from all of them
    pl = np.array(sorted(d.plants))
    assert dist[2:, pl].max() <= 6 and n - 1 in d.plants
    back = np.ones(n, dtype=bool)
    back[pl] = False
    back[d.ties] = False
    back[list(d.exact.values())] = False
    assert dist[2:, back].min() > 9 or bits == 64 and dist[2:, back].min() > 8
    # the offset of the extra plant differs from chunk to chunk
    extra = [S.ordinal(ch, ch % u, 1 + (37 * ch + 11) % (blk - 2), (ch // u) % 2, u, blk) for ch in range(nchunks)]
    assert len({e % sz.chunk for e in extra}) == nchunks and all(e in d.plants for e in extra if e < n)

    rows, counts = S.expect(d.codes, d.queries, 100, sz.id_base)
    assert (counts == 100).all() and (rows[:, 1:] > rows[:, :-1]).all()
    for q in CLUSTER:
        ids = (rows[q] & np.uint64(0xFFFFFFFF)).astype(np.int64) - sz.id_base
        planted = [int(i) for i in ids if int(i) in d.plants]
        loc = [S.locate(i, u, blk) for i in planted]
        assert n - 1 in planted and set(planted) == set(d.plants)
        assert {l[0] for l in loc} == set(range(nchunks))
        assert {l[1] for l in loc} == set(range(u))
        assert {l[3] for l in loc} == {0, 1}
        assert {0, blk - 1} <= {l[2] for l in loc}
        assert any(e in planted for e in extra)
        # the first and the last item of some chunk
        assert any(i % sz.chunk == 0 for i in planted) and any(i % sz.chunk == sz.chunk - 1 for i in planted)
        # ties at the k-th distance: strictly more than the row admits, over two chunks and both blocks, cut inside the group
        dk = int(rows[q, -1] >> SH)
        tied = np.flatnonzero(dist[q] == dk)
        admitted = int(((rows[q] >> SH) == dk).sum())
        assert 0 < admitted < tied.size
        tied_chunks = {int(i) // sz.chunk for i in tied}
        assert len(tied_chunks) >= 2 and {ch % 2 for ch in tied_chunks} == {0, 1}
        in_row = tied[:admitted]
        assert np.array_equal(in_row + sz.id_base, (rows[q, -admitted:] & np.uint64(0xFFFFFFFF)).astype(np.int64))   # the smallest ids
        assert int(in_row[0]) // sz.chunk != int(tied[-1]) // sz.chunk   # the group straddles a chunk boundary

    # k = 1: every query's answer is its exact duplicate, and over a call the answers come from every chunk that has room
    rows1, _ = S.expect(d.codes, d.queries, 1, sz.id_base)
    assert [int(r) for r in rows1[:, 0]] == [sz.id_base + d.exact[q] for q in range(S.NQ)]
    roomy = nchunks - (1 if n % sz.chunk == 1 else 0)
    assert {d.exact[q] // sz.chunk for q in range(13)} == set(range(roomy))


@pytest.mark.parametrize("size_name", ["short", "long"])
@pytest.mark.parametrize("bits,u,blk", TILES)
def test_dense_rows_append_from_most_waves(bits, u, blk, size_name):
    sz = S.size(size_name, u, blk)
    d = S.data(bits, u, blk, size_name, "dense")
    dist = S.distances(d.codes, d.queries)
    rows, counts = S.expect(d.codes, d.queries, S.K_DENSE, sz.id_base)
    assert (counts == S.K_DENSE).all()
    wave_items = 64 * 2                                                  # items of one wave in one pair slot
    for q in range(S.NQ):
        dk = int(rows[q, -1] >> SH)
        assert 1 <= dk <= 3
        under = np.flatnonzero(dist[q] <= dk)
        assert under.size > S.K_DENSE and under.size >= sz.n // 32 and under.size <= sz.n <= 65536
        assert (dist[q] == dk).sum() > ((rows[q] >> SH) == dk).sum() > 0     # ties cut at the k-th distance
        assert {int(i) // sz.chunk for i in under} >= set(range(sz.nchunks - (1 if sz.n % sz.chunk == 1 else 0)))
        waves = {int(i) // wave_items for i in under}
        assert len(waves) * 2 > sz.n // wave_items                      # more than half of all (wave, slot) tiles append


@pytest.mark.parametrize("bits,u,nq", [(512, 1, 640), (256, 2, 4096)])
def test_large_tile_inputs(bits, u, nq):
    """the default pick's BLK = 512 cases: a query tile above 40 KB of LDS on a `short` database for BLK = 512"""
    assert nq * (bits // 8 + 4) > 40 * 1024 and nq * (bits // 8 + 4) <= 160 * 1024
    assert u == S.small_unroll(bits)
    sz = S.size("short", u, 512)
    assert sz.chunks_per_block() == [2, 1] and sz.n <= S.MAX_N
    d = S.data(bits, u, 512, "short", "planted")
    q = S.large_tile_queries(d, bits, nq, 5)
    assert q.shape == (nq, bits // 8) and np.array_equal(q[:S.NQ], d.queries)
    rows, counts = S.expect(d.codes, q, 10, sz.id_base)
    assert (counts == 10).all() and (rows[:, 1:] > rows[:, :-1]).all()
    # cluster queries: the ten nearest are plants and exact duplicates, drawn from both blocks' chunks over the call
    chunks = set()
    for i in range(2, nq, 97):
        if i % S.NQ >= 2:
            ids = (rows[i] & np.uint64(0xFFFFFFFF)).astype(np.int64) - sz.id_base
            assert (rows[i] >> SH).max() <= 8
            chunks |= {int(j) // sz.chunk for j in ids}
    assert {0, 1} <= chunks


def test_calls_cover_the_tiles_the_issue_names():
    for kind in S.KINDS:
        assert {nq for _, nq, _ in S.calls(kind)} == {13, 1}
        assert sorted(nq for _, nq, _ in S.small_calls(kind)) == list(range(8, 16))
        assert all(f + nq <= S.NQ for f, nq, _ in S.calls(kind) + S.small_calls(kind))
    assert {k for _, _, k in S.calls("planted")} == set(S.K_PLANTED) == {k for _, _, k in S.small_calls("planted")}
    assert {k for _, _, k in S.calls("dense")} == {S.K_DENSE}
    line = "[scan shape] W=2 U=4 BLK=256 NB=2 QT=0 grid=2 nchunks=7 qt=11"
    assert S.parse_trace("noise\n" + line + "\n") == [dict(W=2, U=4, BLK=256, NB=2, QT=0, grid=2, nchunks=7, qt=11)]
