"""The MIH query kernel at the capacity limits of its LDS structures (vc_mih.hip mih_query_kernel and what surrounds it).

Every limit has an overflow path that only runs once the structure is full: the hit list (MQ_HMAX, drained at MQ_HFLUSH),
the drain's entry -> bucket bitmap (MQ_BMW words), the k-NN candidate buffer (buf_entries, mq_compact / mq_select_exact),
the replay's tie buffer (MR_TIES: the query is "unresolved" and rejoins the radius loop) and the stream kernel's probe list
(MS_MAXP).  The limits are read from the source, the data is crafted in numpy so that it lands just below, at, just above
and far past a limit, and a CPU test checks that it does.  Every GPU case compares with a plain reference (numpy brute
force, oracle.MihOracle) and proves with a device counter or a trace line that it reached its limit.

The GPU tests are marked one by one: test_generators_reach_their_limits runs without a GPU."""
import math
import os
import re
from itertools import combinations

import numpy as np
import pytest

SH = np.uint64(32)
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "verticut_amd", "csrc", "vc_mih.hip")
_BINOM = np.array([[math.comb(c, i) for i in range(34)] for c in range(34)], dtype=np.int64)


# ------------------------------------------------------------------ limits read from the source
def limits():
    txt = open(SRC).read()

    def d(name):
        m = re.search(r"#define\s+%s\s+(\d+)u?\b" % name, txt)
        assert m, name
        return int(m.group(1))

    L = {n: d(n) for n in ("MQ_BLK", "MQ_G", "MQ_HMAX", "MQ_BMW", "MQ_EPT", "MQ_MAX_GROUP", "MQ_LO_RADIUS", "MQ_LO_KNN",
                           "MQ_GPT_KNN", "MR_TIES", "MS_MAXP")}
    L["MQ_HFLUSH"] = L["MQ_HMAX"] // 2
    L["MQ_ROUND"] = L["MQ_BLK"] * L["MQ_EPT"]
    L["BMW_ENTRIES"] = L["MQ_BMW"] * 32
    return L


def buf_entries(L, k):
    """the query kernel's candidate buffer for k (vc_mih_search)"""
    b = 1024
    while b < L["MQ_MAX_GROUP"] * k + L["MQ_ROUND"]:
        b <<= 1
    return b


def granules_per_pass(L, lo):
    gw = (1 << lo) // 32
    g32 = 1 if gw >= 16 else (L["MQ_GPT_KNN"] if gw == 4 else 16 // gw)
    return L["MQ_BLK"] * g32


# ------------------------------------------------------------------ keys, codes, popcounts
def popc(x):
    return np.bitwise_count(np.asarray(x, dtype=np.uint64)).astype(np.int64)


def colex(x, nbits):
    """rank of each bit pattern among the patterns of its popcount in colex order (mq_unrank / vc_next_comb order)"""
    x = np.asarray(x, dtype=np.int64)
    rank = np.zeros_like(x)
    cnt = np.zeros_like(x)
    for c in range(nbits):
        b = (x >> c) & 1
        cnt += b
        rank += b * _BINOM[c, cnt]
    return rank


def codes_from_keys(keys, sbits):
    """[n, m] substring keys -> row-major codes (substring t = bits t*s .. t*s+s-1 of the little-endian code)"""
    dt = {32: "<u4", 16: "<u2"}[sbits]
    return np.ascontiguousarray(keys.astype(dt)).view(np.uint8).reshape(keys.shape[0], -1)


def keys_of(codes, m):
    nb = codes.shape[1] // m
    return np.ascontiguousarray(codes).view({4: "<u4", 2: "<u2"}[nb]).reshape(codes.shape[0], m).astype(np.int64)


def rand_weight(rng, n, w, sbits):
    """n random sbits-bit masks of popcount w"""
    out = np.zeros(n, dtype=np.int64)
    for i in range(n):
        for b in rng.choice(sbits, size=w, replace=False):
            out[i] |= 1 << int(b)
    return out


# ------------------------------------------------------------------ the scans' pass structure (hit-list model)
def _passes_granule(L, keys, qk, tables, lo, r_lo, r_hi, ball):
    """hits of every pass of one scan32 call: a pass is granules_per_pass consecutive granules of the tables' item space
    (table-major; per table the segments (shell r, |hi| = h) of plan32, hi patterns in colex order)"""
    hi_bits = 32 - lo
    segs = []
    for r in range(r_lo, r_hi + 1):
        for h in range(0, min(r, hi_bits) + 1):
            if not ball and r - h > lo:
                continue
            segs.append((r, h))
    start, s0 = {}, 0
    for r, h in segs:
        start[(r, h)] = s0
        s0 += math.comb(hi_bits, h)
    per_table, gpp = s0, granules_per_pass(L, lo)
    hits = np.zeros((per_table * len(tables) + gpp - 1) // gpp, dtype=np.int64)
    for ti, t in enumerate(tables):
        e = np.unique(keys[:, t]) ^ qk[t]
        h, j = popc(e >> lo), popc(e & ((1 << lo) - 1))
        for r, hh in segs:
            sel = (h == hh) & ((j <= r - hh) if ball else (j == r - hh))
            idx = ti * per_table + start[(r, hh)] + colex(e[sel] >> lo, hi_bits)
            np.add.at(hits, idx // gpp, 1)
    return [int(x) for x in hits]


def _passes_direct(L, keys, qk, tables, r, sbits):
    """hits of every pass of one scan_direct(r) call: MQ_BLK * MQ_G keys per pass, table-major, colex order"""
    nkeys, kpp = math.comb(sbits, r), L["MQ_BLK"] * L["MQ_G"]
    hits = np.zeros((nkeys * len(tables) + kpp - 1) // kpp, dtype=np.int64)
    for ti, t in enumerate(tables):
        e = np.unique(keys[:, t]) ^ qk[t]
        e = e[popc(e) == r]
        np.add.at(hits, (ti * nkeys + colex(e, sbits)) // kpp, 1)
    return [int(x) for x in hits]


def hitlist_peak(L, seq):
    """replay the append loop over a sequence of pass hit counts ("D" = a drain between shells): the largest value the
    hit-list counter reaches (> MQ_HMAX: hits did not fit and were appended again after a drain in the middle of a pass)"""
    nh = peak = 0
    for hits in seq:
        if hits == "D":
            nh = 0
            continue
        peak = max(peak, nh + hits)
        while hits:
            tot = nh + hits
            hits -= max(0, min(hits, L["MQ_HMAX"] - nh))
            nh = 0 if tot >= L["MQ_HFLUSH"] else tot
            if tot <= L["MQ_HMAX"]:
                break
    return peak


def radius_plan(bits, m, R):
    """vc_search_radius's pigeonhole split: (substring radius of tables 0..n_big-1, n_big, small_shells)"""
    s = bits // m
    rq, ra = R // m, R % m
    return min(s, rq), min(m, ra + 1), (min(s, rq - 1) + 1 if rq else 0)


def radius_hit_seq(L, keys, qk, bits, m, R):
    rsub, n_big, small = radius_plan(bits, m, R)
    s = bits // m
    if s == 32:
        lo = L["MQ_LO_RADIUS"]
        seq = _passes_granule(L, keys, qk, range(n_big), lo, rsub, rsub, True)
        if n_big < m and small:
            seq += _passes_granule(L, keys, qk, range(n_big, m), lo, small - 1, small - 1, True)
        return seq
    seq = []
    for r in range(rsub + 1):
        seq += _passes_direct(L, keys, qk, range(m if r < small else n_big), r, s)
    return seq


def knn_hit_seq(L, keys, qk, m, group, last_shell):
    """32-bit substrings: passes of shells 0 .. last_shell, the first `group` shells in one pass, a drain after each"""
    lo, seq, r = L["MQ_LO_KNN"], [], 0
    while r <= last_shell:
        r_hi = min(group - 1, last_shell) if r == 0 else r
        seq += _passes_granule(L, keys, qk, range(m), lo, r, r_hi, False) + ["D"]
        r = r_hi + 1
    return seq


def probed_keys(keys, qk, radii):
    """non-empty buckets a search probes: distinct occupied keys of table t within substring distance radii[t]"""
    return sum(int((popc(np.unique(keys[:, t]) ^ qk[t]) <= rt).sum()) for t, rt in enumerate(radii))


# ------------------------------------------------------------------ crafted data
def radius_ball32(L, n_ball, seed, n_bg=20000):
    """128-bit codes, m = 4, R = 12 (table 0 searches the 3-ball, tables 1..3 the 2-ball): n_ball records whose table-0
    key lies in the FIRST pass of the table-0 granule scan (|hi| = 0, 1, 2 in colex order, low part within the ball),
    the other three substrings at distance 3 each -- full distance <= 12, owned by table 0 and by no other table's ball"""
    rng = np.random.default_rng(seed)
    lo = L["MQ_LO_RADIUS"]
    hi_bits, gpp, R = 32 - lo, granules_per_pass(L, lo), 12
    lows = {w: [x for x in range(1 << lo) if bin(x).count("1") <= w] for w in range(4)}
    es, idx = [], 0
    for h in range(4):
        his = sorted(combinations(range(hi_bits), h), key=lambda c: c[::-1])
        for c in his:
            if idx < gpp:
                hi = sum(1 << b for b in c)
                es += [(hi << lo) | x for x in lows[3 - h]]
            idx += 1
    assert n_ball <= len(es)
    qk = rng.integers(0, 1 << 32, size=4, dtype=np.int64)
    keys = np.empty((n_ball + n_bg, 4), dtype=np.int64)
    keys[:n_ball, 0] = qk[0] ^ np.array(es[:n_ball], dtype=np.int64)
    for t in range(1, 4):
        keys[:n_ball, t] = qk[t] ^ rand_weight(rng, n_ball, 3, 32)
    keys[n_ball:] = rng.integers(0, 1 << 32, size=(n_bg, 4), dtype=np.int64)
    perm = rng.permutation(keys.shape[0])
    return codes_from_keys(keys[perm], 32), codes_from_keys(qk[None], 32)[0], R


def radius_direct16(L, n_low, n_s3, seed):
    """64-bit codes, m = 4, R = 15 (every table searches shells 0..3 of its 16-bit keys, no drain between shells): n_low
    occupied keys of shells 0..2 (carried in the hit list, < MQ_HFLUSH), then n_s3 keys of the first pass of shell 3 --
    the pass that meets the carried hits.  Other substrings at distance 4: every record within R, owned by its own table."""
    rng = np.random.default_rng(seed)
    kpp = L["MQ_BLK"] * L["MQ_G"]
    allk = np.arange(1 << 16, dtype=np.int64)
    w = popc(allk)
    low = [(t, int(e)) for r in range(3) for t in range(4) for e in allk[w == r]]
    e3 = allk[w == 3]
    e3 = e3[np.argsort(colex(e3, 16))]                              # the enumeration order of scan_direct
    s3 = [(t, int(e)) for t in range(4) for e in e3][:kpp]
    assert n_low <= len(low) and n_s3 <= len(s3)
    pick = [low[i] for i in rng.choice(len(low), size=n_low, replace=False)] + s3[:n_s3]
    qk = rng.integers(0, 1 << 16, size=4, dtype=np.int64)
    keys = np.empty((len(pick), 4), dtype=np.int64)
    for i, (t, e) in enumerate(pick):
        for tt in range(4):
            keys[i, tt] = qk[tt] ^ (e if tt == t else int(rand_weight(rng, 1, 4, 16)[0]))
    return codes_from_keys(keys[rng.permutation(len(pick))], 16), codes_from_keys(qk[None], 16)[0], 15


def knn_ball32(n_ball, seed, n_bg=20000):
    """128-bit codes, m = 4: n_ball records whose key in ONE table t lies in the 2-ball of the query's (w <= 1 keys of every
    table first, then w = 2), the other three substrings at distance 3: full distance w + 9, owned by table t.  With k = 10
    the k-th distance is 10, so an exact query runs shells 0..2 and stops there (10 <= 3 * 4)."""
    rng = np.random.default_rng(seed)
    w1 = [(t, e) for t in range(4) for e in [0] + [1 << b for b in range(32)]]
    w2 = [(t, (1 << a) | (1 << b)) for t in range(4) for a, b in combinations(range(32), 2)]
    w2 = [w2[i] for i in rng.permutation(len(w2))]
    pick = (w1 + w2)[:n_ball]
    assert len(pick) == n_ball
    qk = rng.integers(0, 1 << 32, size=4, dtype=np.int64)
    keys = np.empty((n_ball + n_bg, 4), dtype=np.int64)
    for i, (t, e) in enumerate(pick):
        f = rand_weight(rng, 4, 3, 32)
        for tt in range(4):
            keys[i, tt] = qk[tt] ^ (e if tt == t else int(f[tt]))
    keys[n_ball:] = rng.integers(0, 1 << 32, size=(n_bg, 4), dtype=np.int64)
    return codes_from_keys(keys[rng.permutation(keys.shape[0])], 32), codes_from_keys(qk[None], 32)[0]


def heavy_bucket32(n_heavy, seed, n_bg=20000):
    """128-bit codes, m = 4: n_heavy records share the query's table-0 key, one bit differs in each other substring
    (distance 3, owned by table 0): the shell-0 drain holds n_heavy entries and an exact query stops after shell 0"""
    rng = np.random.default_rng(seed)
    qk = rng.integers(0, 1 << 32, size=4, dtype=np.int64)
    keys = np.empty((n_heavy + n_bg, 4), dtype=np.int64)
    keys[:n_heavy, 0] = qk[0]
    for t in range(1, 4):
        keys[:n_heavy, t] = qk[t] ^ (np.int64(1) << rng.integers(0, 32, size=n_heavy))
    keys[n_heavy:] = rng.integers(0, 1 << 32, size=(n_bg, 4), dtype=np.int64)
    return codes_from_keys(keys[rng.permutation(keys.shape[0])], 32), codes_from_keys(qk[None], 32)[0]


def ties32(n_ties, seed, n_bg=20000):
    """128-bit codes, m = 4: n_ties records at full distance D = 8 = 2 m whose substring distances are (3, 3, 1, 1) in a
    random table order -- not all equal D / m, so the replay counts each as a tie shell 1 has seen"""
    rng = np.random.default_rng(seed)
    qk = rng.integers(0, 1 << 32, size=4, dtype=np.int64)
    keys = np.empty((n_ties + n_bg, 4), dtype=np.int64)
    for i in range(n_ties):
        ws = rng.permutation([3, 3, 1, 1])
        for t in range(4):
            keys[i, t] = qk[t] ^ int(rand_weight(rng, 1, int(ws[t]), 32)[0])
    keys[n_ties:] = rng.integers(0, 1 << 32, size=(n_bg, 4), dtype=np.int64)
    return codes_from_keys(keys[rng.permutation(keys.shape[0])], 32), codes_from_keys(qk[None], 32)[0]


def replay_ties(codes, q, m, k):
    """(k-th distance D, ties at D whose substring distances are not all D / m) -- what mih_replay_kernel counts"""
    from oracle import vc_oracle as vo
    d = vo.np_distances(codes, q).astype(np.int64)
    D = int(np.sort(d)[k - 1])
    sub = vo.np_sub_distances(codes, q, m).astype(np.int64)
    return D, int(((d == D) & ~(sub == D // m).all(axis=1)).sum())


def stream_probes(bits, m, R):
    rsub, n_big, small = radius_plan(bits, m, R)
    return sum((m if r < small else n_big) * math.comb(bits // m, r) for r in range(rsub + 1))


# every case is sized from the parsed limits: a retune of a constant moves the boundaries with it
_L = limits()
_H, _F = _L["MQ_HMAX"], _L["MQ_HFLUSH"]
RADIUS32_BALLS = [_H // 2, _H - 1, _H, _H + 1, 2 * _H + 252]          # table-0 hits in the first pass of the radius scan
KNN32_BALLS = [_H - 1, _H, _H + 1, 4 * 529]                          # hits of the grouped first pass (shells 0..2, 4 tables)
DIRECT16 = [(_F - 13, _H - _F + 12), (_F - 13, _H - _F + 13), (_F - 13, _H - _F + 14), (_F - 1, _H)]   # carried + next pass
DRAIN_ENTRIES = [_L["BMW_ENTRIES"] - 1, _L["BMW_ENTRIES"], _L["BMW_ENTRIES"] + 1, 20000]
TIES = [_L["MR_TIES"] - 1, _L["MR_TIES"], _L["MR_TIES"] + 1, _L["MR_TIES"] + 808]


# ------------------------------------------------------------------ CPU: the generators land where they claim
def test_generators_reach_their_limits(oracle):
    L = limits()
    H = L["MQ_HMAX"]
    assert L["MQ_HFLUSH"] * 2 == H and L["MQ_ROUND"] == 1024 and L["BMW_ENTRIES"] == 8192   # the sizes quoted below
    # the generators' keys are the engine's / oracle's bucket keys (rule a12, masked)
    codes, q, R = radius_ball32(L, 1025, 1)
    mo = oracle.MihOracle(codes[:50], 4, key_mode=1)
    K = keys_of(codes, 4)
    assert all(mo.key(codes[i], t) == K[i, t] for i in range(50) for t in range(4))
    mo.close()
    # hit list, 32-bit radius search: the first pass of table 0 holds n_ball hits, nothing else in it, then drains
    for n in RADIUS32_BALLS:
        codes, q, R = radius_ball32(L, n, 1)
        K, qk = keys_of(codes, 4), keys_of(q[None], 4)[0]
        seq = radius_hit_seq(L, K, qk, 128, 4, R)
        assert seq[0] == n and hitlist_peak(L, seq) == n
        d = oracle.np_distances(codes, q)
        assert (d <= R).sum() >= n                               # every ball record is a result
    # 32-bit k-NN: group 3 holds the whole 2-ball in one pass; groups 1 and 2 its shell 2 (132 keys of shells 0..1 fewer)
    for n in KNN32_BALLS:
        codes, q = knn_ball32(n, 2)
        K, qk = keys_of(codes, 4), keys_of(q[None], 4)[0]
        assert hitlist_peak(L, knn_hit_seq(L, K, qk, 4, 3, 2)) == n
        for g in (1, 2):
            assert hitlist_peak(L, knn_hit_seq(L, K, qk, 4, g, 2)) == n - 4 * 33
        assert probed_keys(K, qk, [2] * 4) == n
        D, _ = replay_ties(codes, q, 4, 10)
        assert D == 10                                           # stops in shell 2
    assert max(RADIUS32_BALLS) > 2 * H and max(KNN32_BALLS) > 2 * H and max(a + b for a, b in DIRECT16) == H + L["MQ_HFLUSH"] - 1
    # 16-bit radius search: hits of shells 0..2 carried, then the first pass of shell 3
    for n_low, n_s3 in DIRECT16:
        codes, q, R = radius_direct16(L, n_low, n_s3, 3)
        K, qk = keys_of(codes, 4), keys_of(q[None], 4)[0]
        seq = radius_hit_seq(L, K, qk, 64, 4, R)
        assert hitlist_peak(L, seq) == n_low + n_s3
        assert (oracle.np_distances(codes, q) <= R).all()
    # drain bitmap: the shell-0 drain holds exactly n entries (four shell-0 buckets)
    for n in DRAIN_ENTRIES:
        codes, q = heavy_bucket32(n, 4)
        K, qk = keys_of(codes, 4), keys_of(q[None], 4)[0]
        assert sum(int((K[:, t] == qk[t]).sum()) for t in range(4)) == n
    # candidate buffer: k at and one past each power-of-two step; the heavy bucket's survivors overfill every buffer
    for P in (2048, 4096, 8192):
        k = (P - L["MQ_ROUND"]) // L["MQ_MAX_GROUP"]
        assert buf_entries(L, k) == P and buf_entries(L, k + 1) == 2 * P
        assert 20000 > P
    # replay ties: below, at and above MR_TIES ties at D = 8
    for n in TIES:
        codes, q = ties32(n, 5, n_bg=2000)
        D, nt = replay_ties(codes, q, 4, 10)
        assert (D, nt) == (8, n)
    # stream routing: R = 13 fits MS_MAXP, R = 14 does not
    assert stream_probes(64, 4, 13) == 1668 <= L["MS_MAXP"] < stream_probes(64, 4, 14) == 2228


# ------------------------------------------------------------------ GPU helpers
# The 128-bit / 4-table cases below drain their entries either from the {id, code} records (VcTableView::bent, what an index of
# this size gets: VC_MIH_BENT "1") or through the id gather of vc_load_entry (what it gets when memory is short: "0").  The limits,
# the expectations and the device counters do not depend on the layout; the cases that had no such parameter keep their ids.
def _with_bent(cases):
    """[(values, id)] -> every case under VC_MIH_BENT "1" (id kept) and "0" (id + "-bent0")"""
    return ([pytest.param(*v, "1", id=i) for v, i in cases] + [pytest.param(*v, "0", id=i + "-bent0") for v, i in cases])


def _engine(vc, codes, bits, m, **kw):
    e = vc.Engine(bits, capacity=codes.shape[0], n_tables=m, **kw)
    e.add_codes(codes)
    e.build_index()
    return e


def _radius_ref(oracle, codes, q, R):
    d = oracle.np_distances(codes, q)
    sel = d <= R
    return np.sort(oracle.pack(d[sel], np.nonzero(sel)[0]))


def _knn_checked(vc, oracle, e, mo, codes, q, k):
    """one exact k-NN query against MihOracle: contract, canonical rule at the radius, radius / n_sub_reads / n_candidates,
    linear-scan distances.  Returns (row, (radius, n_sub_reads, n_candidates))"""
    got, cnt, st = e.search_knn(q[None], k, mode=vc.MODE_MIH_EXACT, with_stats=True)
    g, s = got[0, : cnt[0]], st[0]
    ores, ost = mo.find(q, k, stop_mult=4)
    o = np.sort(ores)
    assert np.array_equal(g >> SH, o >> SH)
    dk = o[-1] >> SH
    assert set(g[(g >> SH) < dk].tolist()) == set(o[(o >> SH) < dk].tolist())
    assert (s.radius, s.n_sub_reads, s.n_candidates) == (ost.radius, ost.n_sub_reads, ost.n_distinct)
    seen = oracle.np_sub_distances(codes, q, 4).min(axis=1) <= ost.radius
    d = oracle.np_distances(codes, q)
    exp = np.sort(oracle.pack(d[seen], np.nonzero(seen)[0]))[:k]
    assert np.array_equal(g, exp)
    assert s.n_candidates == int(seen.sum())
    lin, lcnt = e.search_knn(q[None], k, mode=vc.MODE_LINEAR)
    assert np.array_equal(g >> SH, lin[0, : lcnt[0]] >> SH)
    return g, (s.radius, s.n_sub_reads, s.n_candidates)


# ------------------------------------------------------------------ GPU: hit list
@pytest.mark.gpu
@pytest.mark.parametrize("n_ball,bent", _with_bent([((n,), str(n)) for n in RADIUS32_BALLS]))
def test_hit_list_radius_granule_scan(vc, oracle, monkeypatch, n_ball, bent):
    """32-bit granule scan of the radius search: the first pass of table 0 holds n_ball hits (MQ_HMAX - 1 .. > 2 MQ_HMAX)"""
    L = limits()
    monkeypatch.setenv("VC_MIH_BENT", bent)
    codes, q, R = radius_ball32(L, n_ball, 1)
    K, qk = keys_of(codes, 4), keys_of(q[None], 4)[0]
    rsub, n_big, small = radius_plan(128, 4, R)
    with _engine(vc, codes, 128, 4) as e:
        e.timing()
        got = e.search_radius(q[None], R, mode=vc.MODE_MIH_EXACT, cap_per_query=8192)[0]
        t = e.timing()
        assert np.array_equal(got, _radius_ref(oracle, codes, q, R))
        assert t.mih_launches >= 1 and t.mih_queries == 1             # the query kernel ran it
        assert t.mih_hits == probed_keys(K, qk, [rsub] * n_big + [small - 1] * (4 - n_big))
    assert hitlist_peak(L, radius_hit_seq(L, K, qk, 128, 4, R)) == n_ball


@pytest.mark.gpu
@pytest.mark.parametrize("n_low,n_s3", DIRECT16)
def test_hit_list_radius_direct_keys(vc, oracle, n_low, n_s3):
    """<= 16-bit direct keys: hits of shells 0..2 carried into the first pass of shell 3.  A pass probes at most MQ_HMAX keys,
    so the list peaks at MQ_HFLUSH - 1 + MQ_HMAX: 'far past' is 1.5 x here, never 2 x."""
    L = limits()
    codes, q, R = radius_direct16(L, n_low, n_s3, 3)
    K, qk = keys_of(codes, 4), keys_of(q[None], 4)[0]
    with _engine(vc, codes, 64, 4) as e:
        e.timing()
        got = e.search_radius(q[None], R, mode=vc.MODE_MIH_EXACT, cap_per_query=4096)[0]
        t = e.timing()
        assert np.array_equal(got, _radius_ref(oracle, codes, q, R))
        assert t.mih_launches >= 1 and t.mih_hits == n_low + n_s3
    assert hitlist_peak(L, radius_hit_seq(L, K, qk, 64, 4, R)) == n_low + n_s3


@pytest.mark.gpu
@pytest.mark.parametrize("n_ball,lines,bent", _with_bent([((n, ln), "%d-%s" % (n, ln)) for ln in ("0", "1") for n in KNN32_BALLS]))
def test_hit_list_knn_grouping(vc, oracle, monkeypatch, n_ball, lines, bent):
    """exact k-NN over the 2-ball: VC_MIH_GROUP = 3 puts all n_ball hits in one pass, 1 and 2 put n_ball - 132 in the
    shell-2 pass.  The three give identical rows and statistics, equal to MihOracle's."""
    L = limits()
    k = 10
    codes, q = knn_ball32(n_ball, 2)
    K, qk = keys_of(codes, 4), keys_of(q[None], 4)[0]
    mo = oracle.MihOracle(codes, 4, key_mode=1)
    monkeypatch.setenv("VC_MIH_LINES", lines)
    monkeypatch.setenv("VC_MIH_BENT", bent)
    res = []
    for group in (1, 2, 3):
        monkeypatch.setenv("VC_MIH_GROUP", str(group))
        with _engine(vc, codes, 128, 4) as e:
            e.timing()
            row, st = _knn_checked(vc, oracle, e, mo, codes, q, k)
            t = e.timing()
            assert st[0] == 2 and t.mih_queries == 1 and t.mih_hits == n_ball   # shells 0..2, every ball key drained
            res.append((row.tolist(), st))
        peak = hitlist_peak(L, knn_hit_seq(L, K, qk, 4, group, 2))
        assert peak == (n_ball if group == 3 else n_ball - 132)
    assert res[0] == res[1] == res[2]


# ------------------------------------------------------------------ GPU: drain bitmap and candidate buffer
@pytest.mark.gpu
@pytest.mark.parametrize("n,bent", _with_bent([((n,), str(n)) for n in DRAIN_ENTRIES]))
def test_drain_entry_bitmap(vc, oracle, monkeypatch, n, bent):
    """a k-NN drain of n entries: <= MQ_BMW * 32 map entries to buckets through the LDS bitmap, more by binary search.
    VC_MIH_GROUP=1: shell 0 alone in the first pass (a grouped pass would add the 3 n shell-1 entries of tables 1..3).
    No counter says which mapping ran; the entry count does."""
    monkeypatch.setenv("VC_MIH_GROUP", "1")
    monkeypatch.setenv("VC_MIH_BENT", bent)
    k = 10
    codes, q = heavy_bucket32(n, 4)
    mo = oracle.MihOracle(codes, 4, key_mode=1)
    with _engine(vc, codes, 128, 4) as e:
        e.timing()
        _, st = _knn_checked(vc, oracle, e, mo, codes, q, k)
        t = e.timing()
    assert st[0] == 0 and st[2] == n                                  # stopped after shell 0, every entry verified
    assert t.mih_queries == 1 and t.mih_entries == n and t.mih_hits == 1   # ONE drain of n entries


@pytest.mark.gpu
@pytest.mark.parametrize("step,past,bent", _with_bent([((st, pa), "%d-%d" % (pa, st)) for st in (2048, 4096, 8192) for pa in (0, 1)]))
def test_candidate_buffer_steps(vc, oracle, monkeypatch, step, past, bent):
    """k at and one past each buf_entries step.  The shell-0 bucket yields 20 000 survivors under an open threshold, more
    than any buffer: mq_compact runs (and keeps everything: no threshold yet), then mq_select_exact.  The device has no
    counter for either; the witness is the data (survivors > buf_entries) and the in-kernel route (mih_launches)."""
    L = limits()
    monkeypatch.setenv("VC_MIH_GROUP", "2")                           # shells 0 and 1 share the first pass: two classes
    monkeypatch.setenv("VC_MIH_BENT", bent)
    k = (step - L["MQ_ROUND"]) // L["MQ_MAX_GROUP"] + past
    buf = buf_entries(L, k)
    assert buf == step * (2 if past else 1) and 20000 > buf
    codes, q = heavy_bucket32(20000, 6)
    mo = oracle.MihOracle(codes, 4, key_mode=1)
    with _engine(vc, codes, 128, 4) as e:
        e.timing()
        _, st = _knn_checked(vc, oracle, e, mo, codes, q, k)
        t = e.timing()
    assert st[0] == 0 and st[2] == 20000
    assert (t.mih_launches >= 1) == (buf <= 8192)                     # buffers beyond 8 192 run in the multi-block kernels


# ------------------------------------------------------------------ GPU: replay -> rejoin
def _trace_count(err, pattern):
    m = re.findall(pattern, err)
    assert m, err
    return int(m[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["host_loop", "hand_over"])
@pytest.mark.parametrize("n_ties", TIES)
def test_replay_tie_buffer(vc, oracle, monkeypatch, capfd, n_ties, route):
    """n_ties ties at D = 8 (D % m == 0, substrings not all 2): up to MR_TIES the replay resolves the query, past it the
    query is unresolved and rejoins the radius loop.  Rows and statistics equal MihOracle's either way."""
    L = limits()
    k = 10
    monkeypatch.setenv("VC_MIH_TRACE", "1")
    monkeypatch.setenv("VC_MIH_SWITCH", "2")
    if route == "host_loop":
        monkeypatch.setenv("VC_MIH_HOST_LOOP", "1")
    else:
        monkeypatch.setenv("VC_MIH_BUDGET", "1")                     # the query kernel runs shell 0 only, then hands over
    codes, q = ties32(n_ties, 5)
    assert replay_ties(codes, q, 4, k) == (8, n_ties)
    mo = oracle.MihOracle(codes, 4, key_mode=1)
    with _engine(vc, codes, 128, 4) as e:
        capfd.readouterr()
        _, st = _knn_checked(vc, oracle, e, mo, codes, q, k)
        t = e.timing()
    err = capfd.readouterr().err
    assert st[0] == 1 and t.scan_launches >= 1
    back = (_trace_count(err, r"shell r=0: \d+ queries answered by the verify kernel \(cost model\), (\d+) continue")
            if route == "host_loop" else _trace_count(err, r"answered by the verify kernel, (\d+) came back"))
    assert back == (1 if n_ties > L["MR_TIES"] else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["host_loop", "hand_over"])
def test_replay_ring_overflow(vc, oracle, monkeypatch, capfd, route):
    """cand_cap = 64 and 500 ties: the scan's ring overflows (raw > lin_cap), the query is unresolved and rejoins"""
    k = 10
    monkeypatch.setenv("VC_MIH_TRACE", "1")
    monkeypatch.setenv("VC_MIH_SWITCH", "2")
    if route == "host_loop":
        monkeypatch.setenv("VC_MIH_HOST_LOOP", "1")
    else:
        monkeypatch.setenv("VC_MIH_BUDGET", "1")
    codes, q = ties32(500, 7)
    mo = oracle.MihOracle(codes, 4, key_mode=1)
    with _engine(vc, codes, 128, 4, cand_cap=64) as e:
        capfd.readouterr()
        _, st = _knn_checked(vc, oracle, e, mo, codes, q, k)
    err = capfd.readouterr().err
    assert st[0] == 1
    back = (_trace_count(err, r"shell r=0: \d+ queries answered by the verify kernel \(cost model\), (\d+) continue")
            if route == "host_loop" else _trace_count(err, r"answered by the verify kernel, (\d+) came back"))
    assert back == 1


# ------------------------------------------------------------------ GPU: stream routing
@pytest.mark.gpu
@pytest.mark.parametrize("R", [13, 14])
def test_stream_routing_probe_limit(vc, oracle, monkeypatch, R):
    """64-bit, m = 4 radius search at R = 13 (1 668 probes: streamed) and R = 14 (2 228 > MS_MAXP: multi-block shells).
    VC_MIH_STREAM=2 keeps this small database out of the query kernel, as the entry budget does for ~4 M records."""
    L = limits()
    monkeypatch.setenv("VC_MIH_STREAM", "2")
    n = 200000
    rng = np.random.default_rng(R)
    codes = oracle.gen_codes(n, 64, 21, kind=1, n_centres=100, max_flips=10)
    q = codes[rng.integers(0, n, size=4)].copy()
    for i in range(len(q)):
        for b in rng.choice(64, size=3, replace=False):
            q[i, b // 8] ^= np.uint8(1 << (b % 8))
    with _engine(vc, codes, 64, 4) as e:
        e.timing()
        got = e.search_radius(q, R, mode=vc.MODE_MIH_EXACT, cap_per_query=1 << 16)
        t = e.timing()
    streamed = stream_probes(64, 4, R) <= L["MS_MAXP"]
    assert streamed == (R == 13)
    assert (t.mih_launches >= 1) == streamed                          # the stream kernel is a timed MIH launch, probe shells are not
    for i in range(len(q)):
        exp = _radius_ref(oracle, codes, q[i], R)
        assert len(exp) > 0 and np.array_equal(got[i], exp)
