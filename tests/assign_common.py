"""The expectation of vc_assign_nearest* and vc_kmajority*: numpy models of the header's two contracts, engine-free, plain-loop
versions of both for small inputs, and the crafted inputs of test_assign_cpu.py (which pins what they reach), test_assign_gpu.py and
test_kmajority_gpu.py (which compare every output with the models, bit for bit)."""
import functools

import numpy as np

import groups_common as GC

WIDTHS = GC.WIDTHS
MAX_ITERS = 64
STALE = np.uint64(0xA5A5A5A5A5A5A5A5)        # what output buffers hold before a call


def _bits(codes):
    return np.unpackbits(np.ascontiguousarray(codes, dtype=np.uint8), axis=1, bitorder="little").astype(np.float32)


def distances(codes, centres):
    """int64 [N, K] Hamming distances by bit matrices (float32 products of 0 / 1 sums up to 512: exact)"""
    r, c = _bits(codes), _bits(centres)
    return (r.sum(axis=1)[:, None] + c.sum(axis=1)[None, :] - 2.0 * (r @ c.T)).astype(np.int64)


def assign_model(codes, centres, first=0, count=None):
    """packed uint64 [count]: centre index | distance << 32, the smallest (distance, index) -- argmin takes the first minimum"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    count = len(codes) - first if count is None else count
    if count == 0:
        return np.zeros(0, np.uint64)
    d = distances(codes[first:first + count], centres)
    idx = np.argmin(d, axis=1)
    return (d[np.arange(count), idx].astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)


def assign_naive(codes, centres):
    out = []
    for r in codes:
        best = None
        for c, cen in enumerate(centres):
            d = sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(r, cen))
            if best is None or d < best[0]:
                best = (d, c)
        out.append(best[1] | best[0] << 32)
    return np.array(out, dtype=np.uint64)


def index_of(packed):
    return (packed & np.uint64(0xFFFFFFFF)).astype(np.int64)


def dist_of(packed):
    return (packed >> np.uint64(32)).astype(np.int64)


def zero_stats():
    return {"n_iters": 0, "converged": 0, "n_empty": 0, "cost_final": 0, "cost": np.zeros(MAX_ITERS, np.uint64), "n_changed": np.zeros(MAX_ITERS, np.uint64)}


def kmajority_model(codes, seeds, max_iters=MAX_ITERS, id_base=0, assign=assign_model, update=GC.model):
    """(centres, assign, labels, stats) as the header's loop defines them; the update step is the centroid of groups_common.model"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    C = np.array(seeds, dtype=np.uint8).reshape(len(seeds), codes.shape[1])
    n, st, prev = len(codes), zero_stats(), None
    if n == 0:
        return C, np.zeros(0, np.uint64), np.zeros(0, np.uint32), st
    for t in range(max_iters):
        a = assign(codes, C)
        idx = index_of(a)
        st["cost"][t] = dist_of(a).sum()
        st["n_changed"][t] = n if prev is None else np.count_nonzero(idx != prev)
        st["n_iters"] = t + 1
        if st["n_changed"][t] == 0:
            st["converged"] = 1
            break
        groups, cents = update(codes, (idx + id_base).astype(np.uint32), id_base)[:2]
        C[groups["label"].astype(np.int64) - id_base] = cents     # a centre without a member has no group: it keeps its code
        prev = idx
    a = assign(codes, C)
    st["cost_final"] = int(dist_of(a).sum())
    st["n_empty"] = len(C) - len(np.unique(index_of(a)))
    return C, a, (index_of(a) + id_base).astype(np.uint32), st


def kmajority_naive(codes, seeds, max_iters=MAX_ITERS, id_base=0):
    return kmajority_model(codes, seeds, max_iters, id_base, assign=assign_naive, update=GC.naive)


def same_stats(got, want, what=None):
    assert set(got) == set(want), what
    for key in want:
        if key in ("cost", "n_changed"):
            assert np.array_equal(np.asarray(got[key], dtype=np.uint64), want[key]), (what, key, got[key], want[key])
        else:
            assert int(got[key]) == int(want[key]), (what, key, got[key], want[key])


def same_run(got, want, what=None):
    for name, g, w in zip(("centres", "assign", "labels"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, name)
    same_stats(got[3], want[3], what)


def tie_witnesses(codes, centres):
    """records whose smallest distance is reached by two centres of different index: where the tie rule decides"""
    d = distances(codes, centres)
    return np.flatnonzero((d == d.min(axis=1)[:, None]).sum(axis=1) > 1)


# ---- the crafted k-majority cases: (codes, seeds); what each is for is pinned in test_assign_cpu.py -----------------------------------
CASES = (1, 2, 3, 4)


@functools.lru_cache(maxsize=None)
def case(number):
    if number == 1:      # clustered, one duplicate seed: a centre that stays empty, index ties
        codes = GC.clustered_codes(4096, 64, 69, centres=40, flips=3)
        seeds = codes[:40].copy()
    elif number == 2:    # the same at 128 bits: two duplicate seeds, more empty centres
        codes = GC.clustered_codes(4096, 128, 133, centres=40, flips=3)
        seeds = codes[:40].copy()
    elif number == 3:    # uniform codes: not converged at the cap of 64 rounds
        codes = GC.uniform_codes(4096, 256, 265)
        seeds = codes[:64].copy()
    elif number == 4:    # every record its own centre: cost 0
        codes = GC.uniform_codes(1000, 64, 73)
        seeds = codes.copy()
    else:
        raise ValueError(number)
    codes.setflags(write=False)
    seeds.setflags(write=False)
    return codes, seeds


@functools.lru_cache(maxsize=None)
def case_expect(number, max_iters=MAX_ITERS, id_base=0):
    codes, seeds = case(number)
    got = kmajority_model(codes, seeds, max_iters, id_base)
    for x in got[:3]:
        x.setflags(write=False)
    return got


# ---- the crafted assign inputs ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def assign_case(bits, n, k, seed=0):
    """uniform codes and centres"""
    codes, centres = GC.uniform_codes(n, bits, 3000 + bits + seed), GC.uniform_codes(k, bits, 4000 + bits + k + seed)
    codes.setflags(write=False)
    centres.setflags(write=False)
    return codes, centres


@functools.lru_cache(maxsize=None)
def assign_expect(bits, n, k, seed=0):
    out = assign_model(*assign_case(bits, n, k, seed))
    out.setflags(write=False)
    return out


TIE_P, TIE_Q = 3, 200             # identical centres: tiles of 64 put them into tiles 0 and 3, three slices of 257 into slices 0 and 2
TIE_RECORDS = (0, 63, 64, 2047, 2048, 4096)     # planted at one flipped bit from them; 4096 is the lone record of the last block
HIT_RECORD, HIT_CENTRE = 77, 256  # a record equal to the last centre (the one-centre tile at VC_ASSIGN_TILE=64): distance 0


@functools.lru_cache(maxsize=None)
def tie_case(bits, n=4097, k=257):
    codes, centres = (x.copy() for x in assign_case(bits, n, k))
    centres[TIE_Q] = centres[TIE_P]
    for j, i in enumerate(TIE_RECORDS):
        codes[i] = centres[TIE_P]
        codes[i, j % codes.shape[1]] ^= np.uint8(1 << (j % 8))
    codes[HIT_RECORD] = centres[HIT_CENTRE]
    codes.setflags(write=False)
    centres.setflags(write=False)
    return codes, centres
