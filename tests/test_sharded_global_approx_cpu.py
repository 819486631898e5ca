"""VC_FLAG_GLOBAL_APPROX without a GPU: the data of test_sharded_global_approx_gpu.py does what it was made for.
(a) every crafted case stops in the shell it was designed to stop in, with the designed number of distinct candidates;
(b) the data discriminates: the store WITHOUT the flag (every id-range shard to its own stop, rows merged, widest radius,
    summed candidates) differs from one SearchWorker over the union -- in radius or summed candidate count for every
    clustered case at k >= 5 (the summed n_sub_reads differ for any data, so they are not compared), in radius or rows for
    every crafted case in which no single shard reaches 20 k by itself.
A later change of the data that stops exercising the rule fails here.

The union is judged by MihOracle; the shards by the numpy model of sharded_global_approx_common.py, which is checked against
MihOracle here on the union of every case and on every shard whose own stop the oracle can afford (a shard that holds
fewer than 20 k items near the query walks into shells of C(32, r) probes: that is why the flag exists)."""
import math

import numpy as np
import pytest

import sharded_global_approx_common as A

AFFORDABLE = 200_000          # probes per table the oracle is asked to walk in one find


def _affordable(S, radius):
    return sum(math.comb(S, r) for r in range(radius + 1)) <= AFFORDABLE


def _agree(oracle, mo, model, q, k):
    """MihOracle and the model: statistics, and rows by distance (the oracle's heap order among ties is not the contract)"""
    ores, ost = mo.find(q, k, approximate=True)
    assert (ost.radius, ost.n_sub_reads, ost.n_distinct) == model.stats()
    assert np.array_equal(np.sort(ores) >> A.SH, model.rows >> A.SH)


@pytest.mark.parametrize("bits,m", A.CLUSTERED_SHAPES)
def test_clustered_cases_discriminate(oracle, bits, m):
    codes, q = A.clustered_case(oracle, bits, m)
    S = bits // m
    mo = oracle.MihOracle(codes, m, key_mode=1, id_base=A.CLUSTERED_ID_BASE)
    for k in A.CLUSTERED_KS:
        union = [A.Approx(oracle, codes, q[i], k, m, A.CLUSTERED_ID_BASE) for i in range(len(q))]
        for i, u in enumerate(union):
            assert u.n_distinct >= A.FACTOR * k and _affordable(S, u.radius)    # 20 k well inside the neighbourhood
            _agree(oracle, mo, u, q[i], k)
        for shards in A.CLUSTERED_SHARDS:
            bounds = A.shard_bounds(len(codes), shards, len(codes))
            model = [A.Unflagged(oracle, codes, q[i], k, m, bounds, A.CLUSTERED_ID_BASE) for i in range(len(q))]
            differ = sum(model[i].stop() != union[i].stop() for i in range(len(q)))
            print("%d/%d shards %d k %d: radius or candidates differ for %d of %d queries" % (bits, m, shards, k, differ, len(q)))
            if shards == 1:
                assert differ == 0
            elif k >= 5:
                assert differ > 0
    mo.close()


def test_shard_model_is_the_oracle_on_shards(oracle):
    """the issue's shape: 128 / 4, 3 id-range shards, k = 5 -- one MihOracle per shard with its id_base, where affordable"""
    bits, m, k, shards = 128, 4, 5, 3
    codes, q = A.clustered_case(oracle, bits, m)
    checked = 0
    for lo, hi in A.shard_bounds(len(codes), shards, len(codes)):
        mo = oracle.MihOracle(codes[lo:hi], m, key_mode=1, id_base=A.CLUSTERED_ID_BASE + lo)
        for i in range(len(q)):
            model = A.Approx(oracle, codes[lo:hi], q[i], k, m, A.CLUSTERED_ID_BASE + lo)
            if _affordable(bits // m, model.radius):
                _agree(oracle, mo, model, q[i], k)
                checked += 1
        mo.close()
    assert checked == 27          # of 30 shard-queries: three walk beyond what the oracle is asked to afford


@pytest.mark.parametrize("r_star,hit,place", A.CR_CASES, ids=["r%d-%s-%s" % (r, "hit" if h else "miss", p) for r, h, p in A.CR_CASES])
def test_crafted_cases_stop_where_designed(oracle, r_star, hit, place):
    codes, planted = A.crafted(r_star, hit, place)
    q = A.crafted_query()[0]
    radius = A.crafted_radius(r_star, hit)
    bounds = A.shard_bounds(A.CR_N, A.CR_SHARDS, A.CR_N)
    is_planted = np.zeros(A.CR_N, dtype=bool)
    is_planted[[p for p, _ in planted]] = True
    assert len({p for p, _ in planted}) == len(planted)
    minsub = oracle.np_sub_distances(codes, q, A.CR_M).min(axis=1)
    assert minsub[~is_planted].min() > 3                            # the filler stays out of shells 0..3
    assert all(int(minsub[p]) == min(subs) for p, subs in planted)
    # (a) the union stops where designed
    u = A.Approx(oracle, codes, q, A.CR_K, A.CR_M, A.CR_ID_BASE)
    mo = oracle.MihOracle(codes, A.CR_M, key_mode=1, id_base=A.CR_ID_BASE)
    _agree(oracle, mo, u, q, A.CR_K)
    mo.close()
    assert u.radius == radius
    if hit:
        assert u.n_distinct == A.CR_STOP and (r_star == 0 or u.cum[r_star - 1] == 5 * r_star)
    else:
        assert u.cum[r_star] == A.CR_STOP - 1
        assert u.n_distinct == A.CR_STOP + 2 + int(np.sum(minsub[~is_planted] <= radius))
    # the tie at the k-th distance: the smaller id wins
    tie = sorted(A.CR_ID_BASE + planted[i][0] for i in (1, 2))
    assert [int(v >> A.SH) for v in u.rows] == [3, 6] and int(u.rows[1] & np.uint64(0xFFFFFFFF)) == tie[0]
    if place != "one":
        assert (tie[0] - A.CR_ID_BASE) // A.CR_PER_SHARD != (tie[1] - A.CR_ID_BASE) // A.CR_PER_SHARD
    # the placement is what its name says
    model = A.Unflagged(oracle, codes, q, A.CR_K, A.CR_M, bounds, A.CR_ID_BASE)
    alone = [s.cum[radius] for s in model.shards]                   # every shard's own count where the union stops
    if place == "one":
        assert alone[1] >= A.CR_STOP and alone[0] + alone[2] == int(np.sum(minsub[~is_planted] <= radius))
        assert model.shards[1].radius == radius
    elif place == "spread":
        assert max(int(s.cum[3]) for s in model.shards) < A.CR_STOP
    else:
        assert max(alone) < A.CR_STOP and model.shards[0].radius == radius + 1
    # (b) no single shard reaches 20 k where the union does: the unflagged store answers something else
    if max(alone) < A.CR_STOP:
        assert model.radius != u.radius or not np.array_equal(model.rows, u.rows)
