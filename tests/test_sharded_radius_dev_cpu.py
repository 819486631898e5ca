"""The rank merge behind vc_sharded_search_radius_dev, modelled in numpy, on the shapes tests/test_sharded_radius_dev_gpu.py
runs: a query's union is a merge of the shards' ascending, id-disjoint segments, and the place of every value follows from
ranks alone -- own index + sum of lower_bound in the other segments.  Also pins what the GPU tests rely on in their inputs: if
the generator or the query recipe ever changes, the assertion that fails here names the GPU test that lost its teeth."""
import numpy as np
import pytest

import sharded_radius_common as rc


def _segments(name, rows):
    _, _, _, _, _, _, shards, capacity, _ = rc.SHAPES[name]
    return [rc.shard_segments(r, capacity, shards) for r in rows]


@pytest.mark.parametrize("name", sorted(rc.SHAPES))
def test_rank_merge_model_equals_the_sorted_union(oracle, name):
    _, _, rows = rc.case(oracle, name)
    for row, segs in zip(rows, _segments(name, rows)):
        assert sum(len(s) for s in segs) == len(row)                       # the shards' id ranges cover the union
        assert all(np.all(s[1:] > s[:-1]) for s in segs)                   # ascending and distinct within a shard
        merged = rc.rank_merge(segs)
        assert np.array_equal(merged, np.sort(np.concatenate(segs))) and np.array_equal(merged, row)
    one = rc.case(oracle, "many_light")[2][:1]                             # nq = 1
    assert np.array_equal(rc.rank_merge(_segments("many_light", one)[0]), one[0])


def test_shard_id_ranges_are_capacity_g_over_G():
    assert rc.shard_bounds(35_000, 3) == [(0, 11_666), (11_666, 23_333), (23_333, 35_000)]
    for name, (_, _, n, _, _, _, shards, capacity, _) in rc.SHAPES.items():
        b = rc.shard_bounds(capacity, shards)
        assert b[0][0] == 0 and b[-1][1] == capacity and all(b[g][1] == b[g + 1][0] for g in range(shards - 1)) and n <= capacity


def test_shape_1_interleaves_every_planted_query_across_all_shards(oracle):
    """test_rows_equal_the_union[interleaved], the capacity and the stream tests: the plain concatenation is not sorted"""
    _, _, rows = rc.case(oracle, "interleaved")
    counts = [len(r) for r in rows]
    assert min(counts[:-1]) == 440 and max(counts) == 741 and counts[-1] == 0    # the uniform query has no neighbour
    for segs in _segments("interleaved", rows)[:-1]:
        assert all(len(s) for s in segs)
        cat = np.concatenate(segs)
        assert not np.all(cat[1:] > cat[:-1])
        assert all(segs[g][0] < segs[g - 1][-1] for g in range(1, len(segs)))     # every shard starts below its predecessor's end
    n, capacity, shards = rc.SHAPES["interleaved"][2], rc.SHAPES["interleaved"][7], rc.SHAPES["interleaved"][6]
    assert rc.shard_bounds(capacity, shards)[-1][0] < n < capacity               # the last shard is partly filled ...
    assert rc.SHAPES["max_shards"][2] <= rc.shard_bounds(27_000, 16)[-1][0]      # ... and shape 3's is empty


def test_shape_2_has_heavy_queries_next_to_an_empty_one(oracle):
    """test_rows_equal_the_union[heavy], the call-history and the regrow tests: rows above VC_SORT_CAP spanning many merge chunks,
    shard results beyond the shards' starting buffers (64 entries per query)"""
    _, q, rows = rc.case(oracle, "heavy")
    counts = [len(r) for r in rows]
    assert sorted(counts) == [0, 9630, 14974, 14974, 14974, 14974, 15026, 15026]
    assert sum(c > rc.VC_SORT_CAP for c in counts) == 7 and counts[-1] == 0 and counts[-2] > rc.VC_SORT_CAP
    per_shard = np.array([[len(s) for s in segs] for segs in _segments("heavy", rows)])
    assert per_shard[:-1].min() > 1024 and per_shard[:-1].max() < 2048           # segments of ~1 900: several chunks of 1 024 each
    assert np.all(per_shard.sum(axis=0) > 64 * len(q))                           # every shard outgrows its first buffer


def test_shape_3_has_empty_segments_in_the_middle_and_an_empty_last_shard(oracle):
    """test_rows_equal_the_union[max_shards]"""
    _, _, rows = rc.case(oracle, "max_shards")
    counts = [len(r) for r in rows]
    assert min(counts[:-1]) == 9 and max(counts) == 631
    per_shard = np.array([[len(s) for s in segs] for segs in _segments("max_shards", rows)])
    assert np.all(per_shard[:, -1] == 0)                                         # shard 15 holds no record at all
    sparse = per_shard[counts.index(9)]
    assert np.count_nonzero(sparse) == 7
    filled = np.nonzero(sparse)[0]
    assert np.any(sparse[filled[0]:filled[-1]] == 0)                             # zero-length segments between filled ones


def test_shape_5_crosses_the_query_tiles(oracle):
    """test_rows_equal_the_union[many_light]: more queries than MIH_RADIUS_TILE and than the offsets kernel's 1 024-thread tile,
    light rows, some of them empty"""
    _, q, rows = rc.case(oracle, "many_light")
    counts = np.array([len(r) for r in rows])
    assert len(q) == 4099 > rc.MIH_RADIUS_TILE and counts.max() < 100 and np.count_nonzero(counts == 0) >= 1


def test_merge_grid_and_regrow_arithmetic(tmp_path):
    """tests/cpp/sharded_radius_plan_test.cc: the host driver's index arithmetic (block bases, running totals, the regrow sizes)
    as a stand-alone program over csrc/vc_sharded_radius.hpp -- the program one builds with -fsanitize=address,undefined"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "sharded_radius_plan_test"
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-o", str(exe), os.path.join(root, "tests", "cpp", "sharded_radius_plan_test.cc")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "all checks hold" in p.stdout, p.stdout + p.stderr
