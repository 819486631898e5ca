"""The weighted label vote on the device: vc_knn_vote*, vc_label_propagate* and their vc_sharded_* forms.

The expectation is vote_common.py's dict-loop model, pinned against an independent formulation by test_vote_cpu.py, which also shows
that the labelled inputs make each of the three rules decide.  Labels, votes, totals and statistics are integer functions of the
segments and the labels, so every comparison is exact equality on every word; device outputs are pre-filled with a stale pattern and
padded, so every output word is proven written and the words around it proven untouched.  The mixed graphs stay within the team
shape (at most 52 entries a segment); the table shapes and the long shape are reached by rows of k = 8191 over a store of 8 200
uniform codes and by hand-made CSR stars on the same store.  One device.

Not tested: the sharded forms across real devices, segments whose tally comes near 32 bits on the device (the limit is checked in
tests/cpp/vote_plan_test.cc), more than 65 535 long segments."""
import ctypes as C
import functools

import numpy as np
import pytest

import knn_adjacency_common as KA
import knn_graph_common as KG
import vote_common as V

pytestmark = pytest.mark.gpu

PAD = 3          # stale words kept on both sides of every device output
STALE = V.STALE32
BIG_N, BIG_K = 8200, 8191


def _make(vc, codes, id_base=0, shards=0, index=False):
    bits = codes.shape[1] * 8
    if shards:
        e = vc.ShardedEngine(bits, capacity=len(codes) + 10, n_shards=shards, devices=[0], id_base=id_base, n_tables=KG.TABLES[bits])
    else:
        e = vc.Engine(bits, capacity=max(len(codes), 1), id_base=id_base, n_tables=KG.TABLES[bits])
    if len(codes):
        e.add_codes(codes)
    if index:
        e.build_index()
    return e


def _to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    signed = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(a.view(signed).reshape(-1).copy()).cuda()


def _stale(n_words):
    return _to_dev(np.full(n_words + 2 * PAD, STALE, dtype=np.uint32))


def _inner(buf, n_words, what):
    """the n_words words between the pads of a synchronised buffer; the pads must still be stale"""
    raw = buf.cpu().numpy().view(np.uint32)
    assert np.all(raw[:PAD] == STALE) and np.all(raw[PAD + n_words:] == STALE), (what, "words around the output")
    return raw[PAD:PAD + n_words]


def _vote(store, rows, counts, kk, labels, kind=V.COUNT, max_dist=V.NO_CAP, with_votes=True, d_rows=None):
    """vc_knn_vote_dev on stale-filled outputs: (label, votes | None, total | None, stats); d_rows: rows that are in HBM already"""
    import torch
    n_rows, k = rows.shape
    d_r = d_rows if d_rows is not None else _to_dev(rows if rows.size else np.zeros(1, dtype=np.uint64))
    d_c = _to_dev(counts) if counts is not None else None
    d_l = _to_dev(labels if len(labels) else np.zeros(1, dtype=np.uint32))
    outs = [_stale(n_rows) for _ in range(3)]
    ptr = [o.data_ptr() + 4 * PAD for o in outs]
    torch.cuda.synchronize()
    st = store.knn_vote_dev(d_r.data_ptr(), d_c.data_ptr() if counts is not None else None, n_rows, k, kk, d_l.data_ptr(), ptr[0], ptr[1] if with_votes else None,
                            ptr[2] if with_votes else None, weight_kind=kind, max_dist=max_dist)
    torch.cuda.synchronize()
    got = [_inner(o, n_rows, name) for o, name in zip(outs, ("label", "votes", "total"))]
    if not with_votes:
        assert np.all(got[1] == STALE) and np.all(got[2] == STALE)
        return got[0], None, None, st
    return got[0], got[1], got[2], st


def _propagate(store, offsets, adj, labels, kind=V.COUNT, flags=0, max_iters=V.MAX_ITERS, with_votes=True, outs=None):
    """vc_label_propagate_dev on stale-filled outputs: (labels, votes | None, total | None, stats)"""
    import torch
    n = len(labels)
    d_o, d_a = _to_dev(offsets), _to_dev(adj if len(adj) else np.zeros(1, dtype=np.uint64))
    d_l = _to_dev(labels if n else np.zeros(1, dtype=np.uint32))
    outs = [_stale(n) for _ in range(3)] if outs is None else outs
    ptr = [o.data_ptr() + 4 * PAD for o in outs]
    torch.cuda.synchronize()
    st = store.label_propagate_dev(d_o.data_ptr(), d_a.data_ptr() if len(adj) else None, len(adj), d_l.data_ptr(), ptr[0], ptr[1] if with_votes else None,
                                   ptr[2] if with_votes else None, weight_kind=kind, flags=flags, max_iters=max_iters)
    torch.cuda.synchronize()
    got = [_inner(o, n, name) for o, name in zip(outs, ("labels", "votes", "total"))]
    if not with_votes:
        assert np.all(got[1] == STALE) and np.all(got[2] == STALE)
        return got[0], None, None, st
    return got[0], got[1], got[2], st


# ---- 1. the sweep ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [64, 128])
def test_vote_sweep_against_the_model(vc, bits):
    """both widths, kk in {1, 3, 10} (P = 8 and 16 lanes a row), both weight kinds, no cap / a cap that cuts rows / 0"""
    codes, rows, counts = V.graph(bits)
    labels = V.seeded_labels(bits)
    with _make(vc, codes) as store:
        for kk in (1, 3, 10):
            for kind in (V.COUNT, V.CLOSENESS):
                for cap in (V.NO_CAP, bits // 8, 0):
                    V.same_vote(_vote(store, rows, counts, kk, labels, kind, cap), V.vote_expected(bits, kk, kind, cap), (bits, kk, kind, cap))
        got = _vote(store, rows, counts, 10, labels, with_votes=False)
        assert np.array_equal(got[0], V.vote_expected(bits, 10, V.COUNT)[0]) and got[3] == V.vote_expected(bits, 10, V.COUNT)[3]
        # an entry equal to the row's own id is an ordinary entry: every row gets its own id as its nearest entry
        own = np.concatenate([np.arange(700, dtype=np.uint64)[:, None], rows[:, :9]], axis=1)
        V.same_vote(_vote(store, own, counts, 10, labels), V.vote_model(own, counts, 10, labels, bits=bits), "own ids")


# ---- 2. null counts and short rows -----------------------------------------------------------------------------------------------------------------
def test_null_counts_and_short_rows(vc):
    codes, rows, counts = V.graph(64)
    labels = V.seeded_labels(64)
    with _make(vc, codes) as store:
        for kk in (3, 10):
            V.same_vote(_vote(store, rows, None, kk, labels), V.vote_expected(64, kk, V.COUNT), ("no counts", kk))
        short = counts.copy()
        short[::3] = np.arange(len(short[::3])) % 4                           # rows of 0 .. 3 entries among full ones
        V.same_vote(_vote(store, rows, short, 10, labels, V.CLOSENESS), V.vote_model(rows, short, 10, labels, V.CLOSENESS), "counts below kk")
    hub = KG.hub_case()[0]
    n, k = len(hub), 100
    assert n - 1 < k
    wide, wide_counts = KG.model_rows(hub, k)
    hub_labels = (np.arange(n) % 3).astype(np.uint32)
    hub_labels[::4] = V.NONE
    with _make(vc, hub) as store:
        for kk in (k, 64, 65):                                                # the count (70) cuts every row: P = 64 and the wave's table
            want = V.vote_model(wide, wide_counts, kk, hub_labels, V.CLOSENESS)
            V.same_vote(_vote(store, wide, wide_counts, kk, hub_labels, V.CLOSENESS), want, ("short rows", kk))
        # rows of a search hold min(k, N) entries, the record itself among them: counts = NULL stands for exactly that
        found, cnt = store.search_knn_ids(np.arange(n, dtype=np.uint32), k)
        assert np.all(cnt == n) and np.all(found[:, 0] >> np.uint64(32) == 0)
        V.same_vote(_vote(store, found, None, k, hub_labels), V.vote_model(found, None, k, hub_labels, n=n), "search rows, no counts")


# ---- 3. the classifier: search then vote, the rows never leave HBM -------------------------------------------------------------------------------------
def test_the_classifier_votes_over_search_rows_in_hbm(vc):
    import torch
    codes, _, _ = V.graph(128)
    labels = V.seeded_labels(128)
    rng = np.random.default_rng(12)
    queries = codes[rng.choice(700, 33, replace=False)].copy()
    queries[:, 0] ^= 0x11                                                     # 33 queries that are no records
    with _make(vc, codes) as store:
        for q, what in ((queries, "foreign queries"), (codes[:33].copy(), "records as queries")):
            d_q = torch.from_numpy(q.copy()).cuda()
            d_rows, d_cnt = _to_dev(np.zeros(33 * 10, dtype=np.uint64)), _to_dev(np.zeros(33, dtype=np.uint32))
            store.search_knn_dev(d_q.data_ptr(), 33, 10, d_rows.data_ptr(), d_cnt.data_ptr())
            torch.cuda.synchronize()
            rows = d_rows.cpu().numpy().view(np.uint64).reshape(33, 10)
            assert np.array_equal(rows, store.search_knn(q, 10)[0])
            if what == "records as queries":
                assert np.all(rows[:, 0] >> np.uint64(32) == 0)              # own-id entries are present
            for kind in (V.COUNT, V.CLOSENESS):
                want = V.vote_model(rows, None, 10, labels, kind, bits=128)
                V.same_vote(_vote(store, rows, None, 10, labels, kind, d_rows=d_rows), want, (what, kind))
                assert want[3]["n_voted"] + want[3]["n_unlabelled"] == 33


# ---- 4. the team boundaries and the table at its bound --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _big():
    """8 200 uniform 64-bit codes and six full rows of k = 8191"""
    rng = np.random.default_rng(77)
    codes = rng.integers(0, 256, (BIG_N, 8), dtype=np.uint8)
    rows = np.concatenate([KG.model_rows(codes, BIG_K, first=f, count=2)[0] for f in (0, 4000, BIG_N - 2)])
    rows.setflags(write=False)
    return codes, rows


@pytest.fixture(scope="module")
def big_store(vc):
    with _make(vc, _big()[0]) as store:
        yield store


def _big_labels(name):
    rng = np.random.default_rng(3)
    if name == "distinct":
        labels = rng.permutation(BIG_N).astype(np.uint32) * np.uint32(7919)   # every label once: the table fills to its half-full bound
        assert len(np.unique(labels)) == BIG_N and V.NONE not in labels
        return labels
    if name == "one":
        return np.full(BIG_N, 5, dtype=np.uint32)                             # one slot takes every add
    labels = rng.integers(0, 40, BIG_N).astype(np.uint32)
    labels[rng.random(BIG_N) < 0.3] = V.NONE
    return labels


@pytest.mark.parametrize("name", ["distinct", "one", "mixed"])
def test_row_lengths_at_every_team_boundary(vc, big_store, name):
    """64 | 65: lanes to the wave's table; 256 | 257: the wave to the block; 1024 | 1025: the 16 KiB to the 128 KiB table; 8191: full"""
    _, rows = _big()
    labels = _big_labels(name)
    assert np.all(rows != KG.INF)
    for kk in (64, 65, 256, 257, 1024, 1025, BIG_K):
        for kind in (V.COUNT, V.CLOSENESS) if name == "mixed" or kk == BIG_K else (V.COUNT,):
            V.same_vote(_vote(big_store, rows, None, kk, labels, kind), V.vote_model(rows, None, kk, labels, kind), (name, kk, kind))
    counts = np.array([64, 65, 1024, 1025, BIG_K, 0], dtype=np.uint32)        # every length in one launch, through the counts
    V.same_vote(_vote(big_store, rows, counts, BIG_K, labels, V.CLOSENESS), V.vote_model(rows, counts, BIG_K, labels, V.CLOSENESS), (name, "counts"))
    if name == "distinct":
        want = V.vote_model(rows, None, BIG_K, labels)
        assert np.all(want[1] == 1) and np.all(want[2] == BIG_K) and want[3]["n_ties"] == len(rows)   # 8 191 labels at the top tally: rule 3 all the way


# ---- 5. propagation against the model ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [64, 128])
def test_propagation_on_the_three_adjacencies(vc, bits):
    """the semi-supervised and the community form on the EITHER, MUTUAL and REVERSE adjacency, max_iters 1, 2 and 64"""
    codes, _, _ = V.graph(bits)
    with _make(vc, codes) as store:
        for flags in (KA.EITHER, KA.MUTUAL, KA.REVERSE):
            offsets, adj = V.adjacency(bits, flags)
            for form in ("seeded", "community"):
                labels, lp_flags = V.form_input(bits, form)
                for max_iters in (1, 2, V.MAX_ITERS):
                    want = V.propagate_expected(bits, flags, form, max_iters)[0]
                    V.same_vote(_propagate(store, offsets, adj, labels, V.COUNT, lp_flags, max_iters), want, (bits, flags, form, max_iters))
        offsets, adj = V.adjacency(bits, KA.EITHER)
        want = V.propagate_expected(bits, KA.EITHER, "seeded", 3, V.CLOSENESS)[0]
        V.same_vote(_propagate(store, offsets, adj, V.seeded_labels(bits), V.CLOSENESS, V.CLAMP, 3), want, (bits, "closeness"))
        got = _propagate(store, offsets, adj, V.seeded_labels(bits), V.CLOSENESS, V.CLAMP, 3, with_votes=False)
        assert np.array_equal(got[0], want[0]) and got[3] == want[3]


def test_the_converged_case_the_capped_case_and_the_continuation(vc):
    codes, _, _ = V.graph(128)
    offsets, adj = V.adjacency(128, KA.EITHER)
    with _make(vc, codes) as store:
        want, _ = V.propagate_expected(128, KA.EITHER, "sparse", V.MAX_ITERS)
        assert want[3]["converged"] == 1 and want[3]["n_iters"] < V.MAX_ITERS
        V.same_vote(_propagate(store, offsets, adj, V.sparse_seeds(128), V.COUNT, V.CLAMP), want, "converged")
        want, _ = V.propagate_expected(128, KA.EITHER, "seeded", V.MAX_ITERS)
        assert want[3]["converged"] == 0 and want[3]["n_iters"] == V.MAX_ITERS and want[3]["n_changed_last"] > 0
        V.same_vote(_propagate(store, offsets, adj, V.seeded_labels(128), V.COUNT, V.CLAMP), want, "capped")
        # labels_out fed back in continues the same sequence (the community form has no seeds to remember)
        whole, _ = V.propagate_expected(128, KA.EITHER, "community", 5)
        first = _propagate(store, offsets, adj, V.community_labels(700), max_iters=2)
        V.same_vote(first, V.propagate_expected(128, KA.EITHER, "community", 2)[0], "two rounds")
        second = _propagate(store, offsets, adj, first[0].copy(), max_iters=3)
        assert np.array_equal(second[0], whole[0]) and np.array_equal(second[1], whole[1]) and np.array_equal(second[2], whole[2])
        assert second[3]["n_iters"] == 3 and second[3]["n_changed_last"] == whole[3]["n_changed_last"] and second[3]["n_ties_last"] == whole[3]["n_ties_last"]
        # the community labels are resident ids: they feed vc_group_summary unchanged
        done = _propagate(store, offsets, adj, V.community_labels(700))
        assert done[3]["converged"] == 1
        groups = store.group_summary(done[0])[0]
        assert np.array_equal(groups["label"], np.unique(done[0])) and 1 < len(groups) < 700


@pytest.mark.parametrize("bits", [64, 128])
def test_one_round_without_the_clamp_is_the_vote_over_the_same_segments(vc, bits):
    """apart from records with no voting entry, which keep their label.  In the community form no record's current label occurs in its
    own segment, so rule 2 never decides in round 1 and the two calls agree word for word; with class labels they agree wherever the
    record is unlabelled (nothing for rule 2 to prefer)"""
    codes, _, _ = V.graph(bits)
    offsets, adj = V.adjacency(bits, KA.EITHER)
    rows, deg = V.padded_rows(offsets, adj)
    with _make(vc, codes) as store:
        for labels, mask in ((V.community_labels(700), np.ones(700, dtype=bool)), (V.seeded_labels(bits), V.seeded_labels(bits) == V.NONE),
                             (V.sparse_seeds(bits), V.sparse_seeds(bits) == V.NONE)):
            for kind in (V.COUNT, V.CLOSENESS):
                lp = _propagate(store, offsets, adj, labels, kind, 0, 1)
                vote = _vote(store, rows, deg, rows.shape[1], labels, kind)
                voted = vote[0] != V.NONE
                assert np.array_equal(lp[0][voted & mask], vote[0][voted & mask]) and np.array_equal(lp[0][~voted], labels[~voted])
                assert np.array_equal(lp[1][mask], vote[1][mask]) and np.array_equal(lp[2], vote[2]) and (voted & mask).sum() > 100
        assert (~voted).sum() > 0                                            # with 40 seeds many a segment has no voting entry


# ---- 6. hand-made CSR: empty segments, stars into the long path, two hubs, the bipartite flip -----------------------------------------------------------
def _csr(segments):
    """lists of (dist, id) per record -> (offsets, adj), every segment ascending in the packed word"""
    offsets = np.zeros(len(segments) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in segments])
    adj = np.array([w for s in segments for w in sorted((d << 32) | j for d, j in s)], dtype=np.uint64)
    return offsets, adj


def _star(hubs, degree):
    """records `hubs` list records hub + 1 .. hub + degree (mod N) at distances 0 .. 6, and are listed back; the rest is empty"""
    segments = [[] for _ in range(BIG_N)]
    for hub in hubs:
        for t in range(1, degree + 1):
            j = (hub + t) % BIG_N
            segments[hub].append((t % 7, j))
            segments[j].append((t % 7, hub))
    return _csr(segments)


@pytest.mark.parametrize("degree", [V.BIG_MAX, V.BIG_MAX + 1])
def test_a_star_crosses_into_the_long_path(vc, big_store, degree):
    """a hub of 8 192 entries is the last the 128 KiB table takes, 8 193 the first of the long path; all-distinct labels fill the
    table to its bound and make 8 19x labels tie, one label sends every add to one slot"""
    offsets, adj = _star([0], degree)
    assert V.bin_of(degree) == (6 if degree == V.BIG_MAX else 7) and int(offsets[1]) == degree
    for name in ("distinct", "one", "mixed"):
        labels = _big_labels(name)
        for kind, flags, max_iters in ((V.COUNT, 0, 2), (V.CLOSENESS, V.CLAMP, 3)):
            want = V.propagate_model(offsets, adj, labels, kind, flags, max_iters)
            V.same_vote(_propagate(big_store, offsets, adj, labels, kind, flags, max_iters), want, (name, degree, kind, flags))
    want = V.propagate_model(offsets, adj, _big_labels("distinct"), V.COUNT, 0, 1)
    nearest = int(adj[0]) & 0xFFFFFFFF
    assert want[1][0] == 1 and want[2][0] == degree and want[0][0] == _big_labels("distinct")[nearest]   # rule 3: the hub takes its nearest entry's label


def test_two_hubs_at_once_and_empty_segments(vc, big_store):
    offsets, adj = _star([0, 4100], V.BIG_MAX + 1)                            # two long segments, their tables side by side; each hub lists the other, so both hold that entry twice
    deg = np.diff(offsets.astype(np.int64))
    assert (deg > V.BIG_MAX).sum() == 2 and (deg == 0).sum() == 0 and deg.max() == V.BIG_MAX + 2
    for name in ("distinct", "mixed"):
        labels = _big_labels(name)
        want = V.propagate_model(offsets, adj, labels, V.CLOSENESS, 0, 3)
        V.same_vote(_propagate(big_store, offsets, adj, labels, V.CLOSENESS, 0, 3), want, ("two hubs", name))
    # a hub of 300 and one of 2 000 among 8 000 empty segments: the wave's table, the block's 16 KiB and 128 KiB tables in one round
    segments = [[] for _ in range(BIG_N)]
    for hub, degree in ((10, 300), (20, 2000), (30, 700), (40, 65), (50, 64), (60, 33), (70, 17), (80, 9), (90, 1)):
        segments[hub] = [((3 * t) % 11, (hub + 7 * t) % BIG_N) for t in range(1, degree + 1)]
    offsets, adj = _csr(segments)
    assert sorted(set(V.bin_of(d) for d in np.diff(offsets.astype(np.int64)))) == [0, 1, 2, 3, 4, 5, 6]
    for name in ("mixed", "distinct"):
        labels = _big_labels(name)
        want = V.propagate_model(offsets, adj, labels, V.CLOSENESS, 0, 2)
        assert want[3]["n_iters"] == 2
        V.same_vote(_propagate(big_store, offsets, adj, labels, V.CLOSENESS, 0, 2), want, ("every bin", name))
    # no entry at all: everybody keeps its label, one round, converged
    labels = _big_labels("mixed")
    got = _propagate(big_store, np.zeros(BIG_N + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), labels)
    assert np.array_equal(got[0], labels) and not got[1].any() and not got[2].any()
    assert got[3] == dict(n_iters=1, converged=1, n_changed_last=0, n_labelled=int((labels != V.NONE).sum()), n_ties_last=0)


def test_a_two_colour_bipartite_graph_flips_for_ever(vc):
    codes, _, _ = V.graph(64)
    offsets, adj = _csr([[(1, i ^ 1)] for i in range(700)])
    colours = (np.arange(700) % 2).astype(np.uint32)
    with _make(vc, codes) as store:
        for max_iters in (1, 2, 7, V.MAX_ITERS):
            got = _propagate(store, offsets, adj, colours, max_iters=max_iters)
            assert got[3] == dict(n_iters=max_iters, converged=0, n_changed_last=700, n_labelled=700, n_ties_last=0), max_iters
            assert np.array_equal(got[0], colours ^ np.uint32(max_iters % 2)) and np.all(got[1] == 1) and np.all(got[2] == 1)
        fixed = _propagate(store, offsets, adj, colours, flags=V.CLAMP)          # clamped, nothing moves -- and the outvoted seeds are visible
        assert fixed[3]["converged"] == 1 and fixed[3]["n_iters"] == 1 and np.array_equal(fixed[0], colours) and np.all(fixed[1] == 1)


# ---- 7. the host forms, three shards, call history ----------------------------------------------------------------------------------------------------------
def test_the_host_forms_and_three_shards(vc):
    codes, rows, counts = V.graph(64)
    labels = V.seeded_labels(64)
    offsets, adj = V.adjacency(64, KA.EITHER)
    with _make(vc, codes) as store, _make(vc, codes, shards=3) as sharded:
        for kk, kind, cap in ((10, V.COUNT, V.NO_CAP), (3, V.CLOSENESS, V.NO_CAP), (10, V.CLOSENESS, 8)):
            want = V.vote_expected(64, kk, kind, cap)
            V.same_vote(store.knn_vote(rows, counts, kk, labels, kind, cap), want, ("host", kk))
            V.same_vote(store.knn_vote(rows, None, kk, labels, kind, cap), want, ("host, no counts", kk))
            V.same_vote(sharded.knn_vote(rows, counts, kk, labels, kind, cap), want, ("sharded host", kk))
            V.same_vote(_vote(sharded, rows, counts, kk, labels, kind, cap), want, ("sharded device", kk))
            got = store.knn_vote(rows, counts, kk, labels, kind, cap, with_votes=False)
            assert got[1] is None and got[2] is None and np.array_equal(got[0], want[0])
        for form, max_iters in (("seeded", 4), ("community", V.MAX_ITERS), ("sparse", 2)):
            lab, lp_flags = V.form_input(64, form)
            want = V.propagate_expected(64, KA.EITHER, form, max_iters)[0]
            V.same_vote(store.label_propagate(offsets, adj, lab, V.COUNT, lp_flags, max_iters), want, ("host", form))
            V.same_vote(sharded.label_propagate(offsets, adj, lab, V.COUNT, lp_flags, max_iters), want, ("sharded host", form))
            V.same_vote(_propagate(sharded, offsets, adj, lab, V.COUNT, lp_flags, max_iters), want, ("sharded device", form))
            got = store.label_propagate(offsets, adj, lab, V.COUNT, lp_flags, max_iters, with_votes=False)
            assert got[1] is None and got[2] is None and np.array_equal(got[0], want[0])


def test_call_history_big_then_small_leaves_every_word_the_same(vc, big_store):
    """the grow-only scratch leaves nothing behind: long tables, then tiny calls, then the long tables again, both calls mixed"""
    _, rows = _big()
    star, star_adj = _star([0], V.BIG_MAX + 1)
    tiny, tiny_adj = _csr([[(1, (i + 1) % BIG_N)] for i in range(BIG_N)])
    labels = _big_labels("mixed")
    first = {}
    for step, what in enumerate(("star", "vote big", "ring", "vote small", "star", "ring", "vote big", "vote small", "star")):
        if what == "star":
            got = _propagate(big_store, star, star_adj, labels, V.CLOSENESS, 0, 2)
        elif what == "ring":
            got = _propagate(big_store, tiny, tiny_adj, labels, V.COUNT, V.CLAMP, 3)
        elif what == "vote big":
            got = _vote(big_store, rows, None, BIG_K, labels, V.CLOSENESS)
        else:
            got = _vote(big_store, rows, None, 5, labels)
        if what in first:
            V.same_vote(got, first[what], (step, what))
        first.setdefault(what, got)
    V.same_vote(first["star"], V.propagate_model(star, star_adj, labels, V.CLOSENESS, 0, 2), "star")
    V.same_vote(first["ring"], V.propagate_model(tiny, tiny_adj, labels, V.COUNT, V.CLAMP, 3), "ring")
    V.same_vote(first["vote small"], V.vote_model(rows, None, 5, labels), "vote small")


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_untouched(vc):
    """all eight entry points; nothing is dereferenced before the checks, so host addresses serve the device forms too"""
    codes, rows, counts = V.graph(64)
    offsets, adj = V.adjacency(64, KA.EITHER)
    n, p = len(codes), lambda a: a.ctypes.data
    g, lab, off, ad = np.ascontiguousarray(rows), np.ascontiguousarray(V.seeded_labels(64)), np.ascontiguousarray(offsets), np.ascontiguousarray(adj)
    outs = [np.full(n, STALE, dtype=np.uint32) for _ in range(3)]
    o = tuple(p(x) for x in outs)
    with _make(vc, codes) as store, _make(vc, codes, shards=3) as sharded:
        for L_fn, h, dev in ((store._L.vc_knn_vote, store._h, False), (store._L.vc_knn_vote_dev, store._h, True),
                             (sharded._L.vc_sharded_knn_vote, sharded._h, False), (sharded._L.vc_sharded_knn_vote_dev, sharded._h, True)):
            st = vc.VcKnnVoteStats(7, 7, 7, 7)
            for args in ((None, p(g), None, n, 10, 10, 64, p(lab), 0) + o,                 # a null handle
                         (h, None, None, n, 10, 10, 64, p(lab), 0) + o,                    # null rows
                         (h, p(g), None, n, 10, 10, 64, None, 0) + o,                      # null labels
                         (h, p(g), None, n, 10, 10, 64, p(lab), 0, None, o[1], o[2]),      # null out_label
                         (h, p(g), None, n, 0, 0, 64, p(lab), 0) + o,                      # k out of range
                         (h, p(g), None, n, V.MAX_K + 1, 10, 64, p(lab), 0) + o,
                         (h, p(g), None, n, 10, 0, 64, p(lab), 0) + o,                     # kk out of range
                         (h, p(g), None, n, 10, 11, 64, p(lab), 0) + o,
                         (h, p(g), None, n, 10, 10, 64, p(lab), 2) + o,                    # an unknown weight kind
                         (h, p(g), None, n, 10, 10, 64, p(lab), 0xFFFFFFFF) + o):
                assert L_fn(*args, C.byref(st), *((None,) if dev else ())) == vc.VC_ERR_INVALID, (dev, args)
                assert all(np.all(x == STALE) for x in outs) and st.as_dict() == dict.fromkeys(V.VOTE_STATS, 7)
        for L_fn, h, dev in ((store._L.vc_label_propagate, store._h, False), (store._L.vc_label_propagate_dev, store._h, True),
                             (sharded._L.vc_sharded_label_propagate, sharded._h, False), (sharded._L.vc_sharded_label_propagate_dev, sharded._h, True)):
            st = vc.VcLabelPropagateStats(7, 7, 7, 7, 7)
            T = len(ad)
            for args in ((None, p(off), p(ad), T, p(lab), 0, 0, 5) + o,                    # a null handle
                         (h, None, p(ad), T, p(lab), 0, 0, 5) + o,                         # null offsets
                         (h, p(off), None, T, p(lab), 0, 0, 5) + o,                        # null adj with entries
                         (h, p(off), p(ad), T, None, 0, 0, 5) + o,                         # null labels_in
                         (h, p(off), p(ad), T, p(lab), 0, 0, 5, None, o[1], o[2]),         # null labels_out
                         (h, p(off), p(ad), T, p(lab), 2, 0, 5) + o,                       # an unknown weight kind
                         (h, p(off), p(ad), T, p(lab), 0, 2, 5) + o,                       # an unknown flag
                         (h, p(off), p(ad), T, p(lab), 0, 0x80000001, 5) + o,
                         (h, p(off), p(ad), T, p(lab), 0, 0, 0) + o,                       # max_iters out of range
                         (h, p(off), p(ad), T, p(lab), 0, 0, V.MAX_ITERS + 1) + o):
                assert L_fn(*args, C.byref(st), *((None,) if dev else ())) == vc.VC_ERR_INVALID, (dev, args)
                assert all(np.all(x == STALE) for x in outs) and st.as_dict() == dict.fromkeys(V.LP_STATS, 7)
        with pytest.raises(vc.VcError) as err:                                             # through the wrappers
            store.knn_vote(rows, counts, 11, lab)
        assert err.value.code == vc.VC_ERR_INVALID and "kk must be in 1..k" in str(err.value)
        with pytest.raises(vc.VcError) as err:
            store.label_propagate(offsets, adj, lab, max_iters=65)
        assert err.value.code == vc.VC_ERR_INVALID and "max_iters" in str(err.value)


def test_a_corrupted_input_is_refused_on_the_device(vc):
    """vote: a count of UINT32_MAX, a foreign id, d > bits under CLOSENESS.  propagate: a foreign id, d > bits under CLOSENESS, a
    decreasing offset, a first offset that is not 0, a wrong n_entries -- and every output word stays stale.  The handle goes on."""
    import torch
    id_base = 300
    codes, rows, counts = V.graph(64)
    rows = rows + np.uint64(id_base)
    labels = V.seeded_labels(64)
    n = len(codes)
    voting = int(np.nonzero(labels[(rows[5, :10] & np.uint64(0xFFFFFFFF)).astype(np.int64) - id_base] != V.NONE)[0][0])
    broken = counts.copy()
    broken[n - 1] = 0xFFFFFFFF
    foreign = rows.copy()
    foreign[5, 1] = (foreign[5, 1] & np.uint64(0xFFFFFFFF00000000)) | np.uint64(n + id_base)
    below = rows.copy()
    below[6, 0] = (below[6, 0] & np.uint64(0xFFFFFFFF00000000)) | np.uint64(id_base - 1)
    far = rows.copy()
    far[5, voting] = (np.uint64(65) << np.uint64(32)) | (far[5, voting] & np.uint64(0xFFFFFFFF))
    with _make(vc, codes, id_base=id_base) as store:
        good = V.vote_model(rows, counts, 10, labels, V.CLOSENESS, id_base=id_base)
        for r, c, kinds in ((rows, broken, (V.COUNT, V.CLOSENESS)), (foreign, counts, (V.COUNT, V.CLOSENESS)), (below, None, (V.COUNT,)), (far, counts, (V.CLOSENESS,))):
            for kind in kinds:
                with pytest.raises(vc.VcError) as err:
                    _vote(store, r, c, 10, labels, kind)
                torch.cuda.synchronize()
                assert err.value.code == vc.VC_ERR_INVALID
                with pytest.raises(vc.VcError) as err:
                    store.knn_vote(r, c, 10, labels, kind)
                assert err.value.code == vc.VC_ERR_INVALID
        V.same_vote(_vote(store, far, counts, 10, labels, V.COUNT), V.vote_model(far, counts, 10, labels, V.COUNT, id_base=id_base), "d > bits is no error under COUNT")
        V.same_vote(_vote(store, rows, counts, 10, labels, V.CLOSENESS), good, "after the refusals")
        offsets, adj = KA.adjacency_model(rows, counts, 10, KA.EITHER, id_base=id_base)[:2]
        T = len(adj)
        want = V.propagate_model(offsets, adj, labels, V.CLOSENESS, V.CLAMP, 3, id_base=id_base)
        V.same_vote(_propagate(store, offsets, adj, labels, V.CLOSENESS, V.CLAMP, 3), want, "the sound input")
        bad_id, bad_d, down, start, short = adj.copy(), adj.copy(), offsets.copy(), offsets.copy(), offsets.copy()
        bad_id[T // 2] = (bad_id[T // 2] & np.uint64(0xFFFFFFFF00000000)) | np.uint64(n + id_base)
        bad_d[T // 3] = (np.uint64(65) << np.uint64(32)) | (bad_d[T // 3] & np.uint64(0xFFFFFFFF))
        down[n // 2] = down[n // 2 + 1] + np.uint64(1)
        start[0] = 1
        short[n] = T - 1
        for o, a, t, kinds in ((offsets, bad_id, T, (V.COUNT, V.CLOSENESS)), (offsets, bad_d, T, (V.CLOSENESS,)), (down, adj, T, (V.COUNT,)), (start, adj, T, (V.COUNT,)),
                               (short, adj, T, (V.COUNT,)), (offsets, adj[:T - 1], T - 1, (V.COUNT,)), (offsets, np.r_[adj, adj[:1]], T + 1, (V.COUNT,))):
            for kind in kinds:
                outs = [_stale(n) for _ in range(3)]
                with pytest.raises(vc.VcError) as err:
                    _propagate(store, o, a, labels, kind, V.CLAMP, 3, outs=outs)
                torch.cuda.synchronize()
                assert err.value.code == vc.VC_ERR_INVALID
                for buf in outs:
                    assert np.all(buf.cpu().numpy().view(np.uint32) == STALE)               # no output word was written
                with pytest.raises(vc.VcError) as err:
                    store.label_propagate(o, a, labels, kind, V.CLAMP, 3)
                assert err.value.code == vc.VC_ERR_INVALID
        V.same_vote(_propagate(store, offsets, bad_d, labels, V.COUNT, V.CLAMP, 3), V.propagate_model(offsets, bad_d, labels, V.COUNT, V.CLAMP, 3, id_base=id_base),
                    "d > bits is no error under COUNT")
        V.same_vote(_propagate(store, offsets, adj, labels, V.CLOSENESS, V.CLAMP, 3), want, "after the refusals")


# ---- 9. tiny stores and a high id base --------------------------------------------------------------------------------------------------------------------
def test_tiny_stores(vc):
    rng = np.random.default_rng(1)
    with _make(vc, np.zeros((0, 8), dtype=np.uint8)) as store:                             # N = 0
        got = store.label_propagate(np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
        assert len(got[0]) == 0 and got[3] == V.zero_lp_stats()
        got = store.knn_vote(np.zeros((0, 3), dtype=np.uint64), None, 3, np.zeros(0, dtype=np.uint32))
        assert len(got[0]) == 0 and got[3] == V.zero_vote_stats()
        got = store.knn_vote(np.zeros((4, 3), dtype=np.uint64), None, 3, np.zeros(0, dtype=np.uint32))   # rows over an empty store hold min(k, 0) = 0 entries
        assert np.all(got[0] == V.NONE) and got[3] == dict(n_voted=0, n_unlabelled=4, n_ties=0, n_entries=0)
    for n in (1, 2):
        codes = rng.integers(0, 256, (n, 8), dtype=np.uint8)
        rows, counts = KG.model_rows(codes, 3, 40)
        offsets, adj = KA.adjacency_model(rows, counts, 3, KA.EITHER, id_base=40)[:2]
        with _make(vc, codes, id_base=40) as store:
            for labels in (np.arange(n, dtype=np.uint32) + 40, np.array([V.NONE, 9][:n], dtype=np.uint32), np.full(n, V.NONE, dtype=np.uint32)):
                V.same_vote(_vote(store, rows, counts, 3, labels, V.CLOSENESS), V.vote_model(rows, counts, 3, labels, V.CLOSENESS, id_base=40), ("vote", n))
                V.same_vote(store.knn_vote(rows, counts, 3, labels), V.vote_model(rows, counts, 3, labels, id_base=40), ("host vote", n))
                for flags in (0, V.CLAMP):
                    want = V.propagate_model(offsets, adj, labels, V.COUNT, flags, 4, id_base=40)
                    V.same_vote(_propagate(store, offsets, adj, labels, V.COUNT, flags, 4), want, ("propagate", n, flags))
                    V.same_vote(store.label_propagate(offsets, adj, labels, V.COUNT, flags, 4), want, ("host propagate", n, flags))
            V.same_vote(_vote(store, np.zeros((0, 3), dtype=np.uint64), None, 3, labels), (np.zeros(0), np.zeros(0), np.zeros(0), V.zero_vote_stats()), "no rows")


def test_a_high_id_base_with_an_exact_mih_graph(vc):
    """ids near 2^32: graph -> adjacency -> vote and propagate, every id word above 2^31"""
    id_base = 0xFFFFF000
    codes, _, _ = V.graph(64)
    n = len(codes)
    labels = V.seeded_labels(64)
    with _make(vc, codes, id_base=id_base, index=True) as store:
        rows, counts = store.knn_graph(V.K, mode=vc.MODE_MIH_EXACT)
        assert np.array_equal(rows, KG.model_rows(codes, V.K, id_base)[0])
        offsets, adj, _ = store.knn_adjacency(rows, counts, V.K, KA.EITHER)
        for kind in (V.COUNT, V.CLOSENESS):
            V.same_vote(_vote(store, rows, counts, V.K, labels, kind), V.vote_model(rows, counts, V.K, labels, kind, id_base=id_base), ("vote", kind))
            want = V.propagate_model(offsets, adj, labels, kind, V.CLAMP, 5, id_base=id_base)
            V.same_vote(_propagate(store, offsets, adj, labels, kind, V.CLAMP, 5), want, ("seeded", kind))
        ids = V.community_labels(n, id_base)
        want = V.propagate_model(offsets, adj, ids, V.COUNT, 0, V.MAX_ITERS, id_base=id_base)
        got = _propagate(store, offsets, adj, ids)
        V.same_vote(got, want, "community")
        assert got[3]["converged"] == 1 and np.all(got[0] >= id_base)
        assert np.array_equal(got[0] - np.uint32(id_base), V.propagate_expected(64, KA.EITHER, "community", V.MAX_ITERS)[0][0])   # the layout does not matter
