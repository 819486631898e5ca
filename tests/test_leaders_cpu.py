"""Greedy leader dedup, without a GPU: the ABI surface, the code objects of the kernels, and the expectation of test_leaders_gpu.py
-- that its two methods agree, that the result has the three properties the call promises, that the data makes the difference to
single linkage matter, and how many rounds the eager rule needs."""
import ctypes
import os
import re

import numpy as np
import pytest

import cluster_common as CC
import ids_common as I
import leaders_common as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vc_leaders_radius", "vc_leaders_radius_dev", "vc_sharded_leaders_radius", "vc_sharded_leaders_radius_dev"]


def test_header_declares_and_library_exports_the_new_names(vc):
    txt = open(os.path.join(ROOT, "include", "verticut_gpu.h")).read()
    assert re.search(r"#define\s+VC_ABI_VERSION\s+2\b", txt)             # entry points are only added
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"typedef struct vc_leader_stats\s*\{\s*uint64_t n_pairs;\s*uint64_t n_leaders;\s*uint64_t n_rounds;\s*\}\s*vc_leader_stats;", code)
    L = ctypes.CDLL(vc.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(L, name), name
        assert name in vc.EXPORTS
    assert ctypes.sizeof(vc.VcLeaderStats) == 24 and vc.VcLeaderStats.n_leaders.offset == 8 and vc.VcLeaderStats.n_rounds.offset == 16
    for cls in (vc.Engine, vc.ShardedEngine):
        for meth in ("leaders_radius", "leaders_radius_dev"):
            assert callable(getattr(cls, meth))
    host = open(os.path.join(ROOT, "verticut_amd", "host", "verticut_host.hpp")).read()
    assert re.search(r"virtual int leaders_radius\([^)]*\)\s*=\s*0;", host)
    assert len(re.findall(r"int leaders_radius\([^)]*\)\s*override", host)) == 2
    assert "return vc_leaders_radius(h_," in host and "return vc_sharded_leaders_radius(h_," in host
    # the group of rounds between two read-backs: one constant, mirrored
    internal = open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_internal.hpp")).read()
    group = int(re.search(r"#define\s+VC_LEADER_ROUND_GROUP\s+(\d+)u", internal).group(1))
    assert group == vc.LEADER_ROUND_GROUP and 1 <= group < min(LC.rounds(LC.T512["n"], LC.t512_pairs(r))[1] for r in LC.T512_RADII)


def test_leaders_kernels_use_no_scratch_and_two_words_of_lds(vc):
    """vc_leaders.o holds the round kernel twice (round 1 and the later rounds), the assign and the count kernel: no scratch, no
    spills -- a wave walks its query's segment and reduces across its lanes; LDS holds only the round kernel's two block sums"""
    from verticut_amd import build as vb
    assert "vc_leaders.hip" in vb.SOURCES
    res = vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_leaders.o"))
    assert len(res) == 4, sorted(res)
    for kernel, count in (("vc_leaders_round_kernel", 2), ("vc_leaders_assign_kernel", 1), ("vc_leaders_count_kernel", 1)):      # (mangled names)
        assert sum(kernel in name for name in res) == count, (kernel, sorted(res))
    for name, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == (16 if "vc_leaders_round_kernel" in name else 0), (name, r)


# Eager rounds per shape at its radii (0, 3, 6, last), as leaders_common.rounds counts them: S64 2 / 10 / 7 / 2, S128 2 / 6 / 10 / 2,
# S256 2 / 5 / 6 / 2, S512 2 / 5 / 8 / 2.  Asserted is only the bound that keeps the GPU test's shapes cheap.
MAX_ROUNDS = 64


@pytest.mark.parametrize("name", I.SINGLE)
def test_the_two_expectation_methods_agree(name):
    n = I.SHAPES[name]["n"]
    own = np.arange(n)
    k = CC.n_old(name)
    for radius in LC.RADII[name]:
        pairs = CC.pairs_of(name, radius)
        lab = LC.labels_of(name, radius)
        by_rounds, n_rounds = LC.rounds(n, pairs)
        assert np.array_equal(lab, by_rounds), radius
        print(name, radius, "eager rounds", n_rounds)
        assert 2 <= n_rounds < MAX_ROUNDS, (radius, n_rounds)
        # the three properties
        assert np.all(lab <= own) and np.array_equal(lab[lab], lab)                # a label is a leader, itself labelled with itself
        assert LC.far_members(lab, pairs) == 0                                      # every dropped record is within R of its label
        assert LC.close_leaders(lab, pairs) == 0                                    # no two leaders within R
        a, b = CC.split(pairs)
        smallest = np.full(n, n, dtype=np.int64)
        lead = lab[a] == a
        np.minimum.at(smallest, b[lead], a[lead])
        assert np.array_equal(lab[lab != own], smallest[lab != own])                # the SMALLEST leader within R
        assert LC.n_leaders(lab) == int(np.count_nonzero(lab == own))
        # the prefix property: the first 60 % alone decide as they do among all
        assert 0 < k < n and np.array_equal(LC.old_labels(name, radius), lab[:k]), radius


def test_the_data_makes_the_feature_matter():
    """single linkage chains: members of a component far from its label; the leaders have none"""
    name, radius = "S128", 6
    pairs = CC.pairs_of(name, radius)
    assert CC.figures(name, radius) == (180, 177, 2459, 3608)
    assert LC.far_members(CC.labels_of(name, radius), pairs) == 3608
    lab = LC.labels_of(name, radius)
    assert LC.far_members(lab, pairs) == 0
    assert LC.n_leaders(lab) > 180 and not np.array_equal(lab, CC.labels_of(name, radius))
    # the label is the minimum over ALL leader neighbours, not the leader that dropped the record first: the assign pass matters
    a, b = CC.split(pairs)
    n_lead = np.bincount(b[lab[a] == a], minlength=len(lab))
    assert np.count_nonzero(n_lead > 1) > 0


@pytest.mark.parametrize("radius", LC.T512_RADII)
def test_thermometer_closed_form(radius):
    n = LC.T512["n"]
    codes = LC.t512_codes()
    assert codes.shape == (n, 64) and not codes[0].any() and np.all(codes[n - 1] == 0xFF)
    for i in (0, 1, 7, 8, 9, 300, 512):
        d = I.distances(codes, codes[i])
        assert np.array_equal(d, np.abs(np.arange(n) - i))                          # |i - j| bits apart
    pairs = LC.t512_pairs(radius)
    want = LC.t512_labels(radius)
    assert np.array_equal(LC.greedy(n, pairs), want)
    lab, n_rounds = LC.rounds(n, pairs)
    assert np.array_equal(lab, want)
    assert n_rounds == {1: 513, 2: 342, 5: 172}[radius]                             # one batch: a chain through every record
    assert np.array_equal(LC.t512_expect(radius), (want + 5).astype(np.uint32))


def _pairs(*edges):
    return np.sort(np.array([(min(a, b) << 32) | max(a, b) for a, b in edges], dtype=np.uint64))


def test_hand_made_graph():
    """a path 0-1-2-3-4: leaders 0, 2, 4, decided in rounds 1, 3, 5.  6 is adjacent to the leader 5 and to the dropped 3.  7 is adjacent
    to the leaders 5 and 2: round 2 drops it on 5, 2 becomes a leader only in round 3, and the label is 2 -- the assign pass.  8 is alone"""
    n = 9
    pairs = _pairs((0, 1), (1, 2), (2, 3), (3, 4), (5, 6), (3, 6), (5, 7), (2, 7))
    want = np.array([0, 0, 2, 2, 4, 5, 5, 2, 8])
    assert np.array_equal(LC.greedy(n, pairs), want)
    lab, n_rounds = LC.rounds(n, pairs)
    assert np.array_equal(lab, want) and n_rounds == 5
    assert LC.far_members(want, pairs) == 0 and LC.close_leaders(want, pairs) == 0 and LC.n_leaders(want) == 5
