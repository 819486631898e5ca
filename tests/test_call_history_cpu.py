"""The expectation the call-history GPU suite compares every row with, pinned without a GPU: the numpy model of the exact
radius loop (oracle.MihExactModel) against the oracle's SearchWorker::find (MihOracle.find, search_worker.cc:170-207), and the
properties of the seeded call sequences that test_call_history_gpu.py relies on."""
import numpy as np
import pytest

import call_history_common as H

SH = np.uint64(32)


def _check(oracle, mo, codes, q, m, k, id_base):
    row, st = oracle.np_mih_exact(codes, q, m, k, id_base=id_base)
    ores, ost = mo.find(q, k, stop_mult=min(m, 4))
    o = np.sort(ores)
    assert (st["radius"], st["n_sub_reads"], st["n_candidates"]) == (ost.radius, ost.n_sub_reads, ost.n_distinct)
    assert (st["n_local_reads"], st["n_main_reads"], st["n_results"]) == (ost.n_local_reads, ost.n_main_reads, len(o))
    # rows: the oracle's heap keeps whichever ties at the k-th distance came first, the model the smallest ids
    assert len(row) == len(o) and np.array_equal(row >> SH, o >> SH)
    if len(o):
        dk = o[-1] >> SH
        assert np.array_equal(row[(row >> SH) < dk], o[(o >> SH) < dk])
    assert np.all(row[1:] > row[:-1])
    return st


@pytest.mark.parametrize("bits,m", [(128, 4), (64, 2), (256, 8), (64, 4), (64, 8)])
def test_model_equals_the_oracle(oracle, bits, m):
    """near-duplicate queries at every shape; uniform-random ones where every shell is cheap for the oracle (16- and 8-bit
    substrings), so the model's late stops are pinned too; id_base at the top of the id range"""
    codes = H.make_codes(oracle, bits, m)
    q = H.make_queries(codes, bits, m)
    id_base = 2 ** 32 - len(codes) if bits == 128 else 1000
    mo = oracle.MihOracle(codes, m, key_mode=1, id_base=id_base)
    cheap = bits // m <= 16
    late = 0
    for i in list(range(0, H.POOL, 2)) + ([2 * H.POOL + j for j in range(6)] if cheap else []):
        model = oracle.MihExactModel(codes, q[i], m, id_base)
        for k in (1, 7, 100) + ((1000, 3500) if cheap else ()):
            st = _check(oracle, mo, codes, q[i], m, k, id_base)
            assert model.find(k)[1] == st                 # one model per query answers every k
            late += st["radius"] >= 2
    if cheap:
        assert late > 0


def test_model_with_fewer_items_than_k(oracle):
    """the loop never stops: radius = s, the row is the whole database"""
    codes = H.make_codes(oracle, 64, 4, n=50)
    q = H.make_queries(codes, 64, 4)
    mo = oracle.MihOracle(codes, 4, key_mode=1, id_base=9)
    for i in (0, 2 * H.POOL):
        st = _check(oracle, mo, codes, q[i], 4, 100, 9)
        assert st["radius"] == 16 and st["n_candidates"] == 50 and st["n_results"] == 50
    row, st = oracle.np_mih_exact(codes[:0], q[0], 4, 5)
    assert len(row) == 0 and st["radius"] == 16 and st["n_candidates"] == 0


@pytest.mark.parametrize("bits,m", [(128, 4), (64, 2)])
def test_far_batches_stop_in_shell_two_or_later(oracle, bits, m):
    """the condition under which VcMihIndex::group_hint moves to 3: >= 60 % of a batch of >= 64 queries over 32-bit substrings
    stops in shell 2 or later.  The far batch of the GPU sequences, judged by the model."""
    codes = H.make_codes(oracle, bits, m)
    q = H.make_queries(codes, bits, m)
    far = H.named_calls(m)["far"]
    idx = H.batch_index(far.kind, far.nq, far.start)
    radius = {i: oracle.np_mih_exact(codes, q[i], m, far.k)[1]["radius"] for i in set(idx.tolist())}
    late = sum(radius[i] >= 2 for i in idx.tolist())
    assert far.nq >= 64 and late * 10 >= far.nq * 6, (late, far.nq)
    near = H.named_calls(m)["near"]
    nidx = H.batch_index(near.kind, near.nq, near.start)
    nrad = {i: oracle.np_mih_exact(codes, q[i], m, near.k)[1]["radius"] for i in set(nidx.tolist())}
    assert sum(nrad[i] <= 1 for i in nidx.tolist()) * 10 >= near.nq * 6      # and the near batch moves it back to 2


@pytest.mark.parametrize("m", [2, 4, 8])
def test_orders_of_the_call_multiset(m):
    named, calls = H.multiset(m, seed=m)
    orders = H.orders(m, seed=m)
    assert set(orders) == {"descending", "ascending", "shuffled"}
    for name, seq in orders.items():
        assert sorted(seq) == sorted(calls + calls), name                  # the same multiset, every call twice
    sizes = [c.size for c in orders["descending"]]
    assert sizes == sorted(sizes, reverse=True) and [c.size for c in orders["ascending"]] == sorted(sizes)
    for a, b in H.PAIRS:
        assert H.has_adjacent(orders["shuffled"], named[a], named[b]), (a, b)
    # the alphabet is covered
    assert {c.form for c in calls} == {"knn", "knn_dev", "knn_dev_stats", "radius", "radius_dev", "radius_dev_small"}
    assert {c.k for c in calls if not c.is_radius} == set(H.K_VALUES)
    assert {c.nq for c in calls} == set(H.NQ_VALUES)
    assert {c.radius for c in calls if c.is_radius} == {0, 8, 2 * m + 2}
    assert {c.stream for c in calls} == {"own", "null", "side", "set_side"}
    assert {c.mode for c in calls} == {H.LINEAR, H.EXACT, H.APPROX} and {c.kind for c in calls} == set(H.KINDS)
    assert {c.order for c in calls if c.form == "knn"} == {0, 1} and {c.stats for c in calls if c.form == "knn"} == {True, False}
