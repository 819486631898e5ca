"""The expectation of vc_group_summary*: a numpy model of the header's contract, engine-free, and the crafted inputs of
test_groups_cpu.py (which pins what they reach) and test_groups_gpu.py (which compares every output with the model, bit for bit)."""
import functools

import numpy as np

GROUP_FIELDS = ("label", "size", "rep", "rep_dist", "max_dist", "reserved")
GROUP_DTYPE = np.dtype([(f, "<u4") for f in GROUP_FIELDS])
WIDTHS = (64, 128, 256, 512)
SMALL_WINDOW = 2048          # VC_GROUP_WINDOW of the windowed cases
TIER_SIZES = (1, 2, 3, 64, 65, 1024, 1025, 2049)


def model(codes, labels, id_base=0):
    """codes uint8 [N, bits / 8], labels [N] -> (groups, centroids, rep_labels, group_index) as the header defines them"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    n, nbytes = len(labels), codes.shape[1]
    if n == 0:
        return np.zeros(0, GROUP_DTYPE), np.zeros((0, nbytes), np.uint8), np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    keys = np.asarray(labels).astype(np.int64) - id_base
    assert keys.min() >= 0 and keys.max() < n
    order = np.argsort(keys, kind="stable")                       # groups by ascending label, members by ascending id
    sk = keys[order]
    head = np.r_[True, sk[1:] != sk[:-1]]
    starts = np.flatnonzero(head)
    sizes = np.diff(np.r_[starts, n])
    of = np.cumsum(head) - 1                                      # group number per sorted position
    bits = np.unpackbits(codes[order], axis=1, bitorder="little").astype(np.int64)
    cent = (2 * np.add.reduceat(bits, starts, axis=0) > sizes[:, None]).astype(np.int64)   # strict majority: a tie gives 0
    dist = np.abs(bits - cent[of]).sum(axis=1)
    packed = (dist << 32) | (order + id_base)                     # smallest (distance, id)
    best = np.minimum.reduceat(packed, starts)
    groups = np.zeros(len(starts), GROUP_DTYPE)
    groups["label"], groups["size"] = sk[starts] + id_base, sizes
    groups["rep"], groups["rep_dist"] = best & 0xFFFFFFFF, best >> 32
    groups["max_dist"] = np.maximum.reduceat(dist, starts)
    rep_labels, group_index = np.empty(n, np.uint32), np.empty(n, np.uint32)
    rep_labels[order], group_index[order] = groups["rep"][of], of
    return groups, np.packbits(cent.astype(np.uint8), axis=1, bitorder="little"), rep_labels, group_index


def naive(codes, labels, id_base=0):
    """the same by plain loops, for small inputs: what model() is pinned against"""
    n, nbits = len(labels), codes.shape[1] * 8
    bit = lambda i, b: (int(codes[i, b // 8]) >> (b % 8)) & 1
    out, cents, rep_labels, group_index = [], [], [0] * n, [0] * n
    for g, lab in enumerate(sorted(set(int(x) for x in labels))):
        members = [i for i in range(n) if int(labels[i]) == lab]
        cent = [1 if 2 * sum(bit(i, b) for i in members) > len(members) else 0 for b in range(nbits)]
        dist = {i: sum(bit(i, b) != cent[b] for b in range(nbits)) for i in members}
        rep = min(members, key=lambda i: (dist[i], i))
        out.append((lab, len(members), rep + id_base, dist[rep], max(dist.values()), 0))
        cents.append([sum(cent[8 * k + j] << j for j in range(8)) for k in range(nbits // 8)])
        for i in members:
            rep_labels[i], group_index[i] = rep + id_base, g
    return (np.array(out, dtype=GROUP_DTYPE), np.array(cents, dtype=np.uint8).reshape(len(out), nbits // 8),
            np.array(rep_labels, dtype=np.uint32), np.array(group_index, dtype=np.uint32))


def same(got, want, what=None):
    for name, g, w in zip(("groups", "centroids", "rep_labels", "group_index"), got, want):
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, name)


def uniform_codes(n, bits, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, bits // 8), dtype=np.uint8)


def partition(sizes, seed, id_base=0):
    """labels of a partition whose groups have these sizes IN SORTED ORDER (group g takes the sorted positions behind group g - 1):
    the members are scattered over the ids at random and the label values are random ids, ascending with g -- so a label is in
    general no member of its group.  Returns (labels uint32 [N], starts)."""
    rng = np.random.default_rng(seed)
    n = int(sum(sizes))
    values = np.sort(rng.choice(n, size=len(sizes), replace=False))
    labels = np.empty(n, np.int64)
    labels[rng.permutation(n)] = np.repeat(values, sizes)
    return (labels + id_base).astype(np.uint32), np.r_[0, np.cumsum(sizes)]


def _fill(sizes, upto, pieces):
    """appends groups of the sizes `pieces` in turn, then singletons, until the groups cover exactly `upto` positions"""
    k = 0
    while sum(sizes) < upto:
        s = pieces[k % len(pieces)] if k < 4 * len(pieces) else 1
        sizes.append(s if sum(sizes) + s <= upto else 1)
        k += 1
    assert sum(sizes) == upto


@functools.lru_cache(maxsize=None)
def tier_sizes():
    """every size at which the code takes another path, laid out against windows of 2048 positions: a pair astride 2047 | 2048, a
    group of 65 astride 4096, the group of 2049 from 4159 on -- its chunks start in windows 2, 2 and 3 and its second chunk lies
    astride 6144"""
    sizes = [1025, 3, 64, 1, 2, 65]
    _fill(sizes, 2047, (1, 2, 1, 3, 1, 7))
    sizes += [2, 1024]                       # 2047 .. 2048, then 2049 .. 3072
    _fill(sizes, 4094, (3, 2, 63, 66, 128, 129, 4, 5))
    sizes += [65, 2049]                      # 4094 .. 4158, 4159 .. 6207
    sizes += [1, 2, 3, 1, 1, 6]
    return tuple(sizes)


@functools.lru_cache(maxsize=None)
def tier_case(bits, id_base=0):
    """(codes, labels) of the tier-and-window cases at one code width: uniform codes, the partition of tier_sizes(), and three
    crafted spots -- the first pair's members differ in two bits, one each way (a tie of distance); every even group of 4 .. 1024
    members has bit 0 set in exactly half of them; the first group of 3 holds the same code twice; the group of 2049 holds its own
    centroid twice, at ids that are not its smallest"""
    sizes = tier_sizes()
    labels, starts = partition(sizes, 1000 + bits, id_base)
    codes = uniform_codes(len(labels), bits, 2000 + bits)
    order = np.argsort(labels, kind="stable")
    for g, s in enumerate(sizes):
        members = order[starts[g]:starts[g + 1]]
        if s % 2 == 0 and 4 <= s <= 1024:
            codes[members, 0] &= 0xFE
            codes[members[::2], 0] |= 1
    m2 = order[starts[sizes.index(2)]:starts[sizes.index(2) + 1]]
    codes[m2[1]] = codes[m2[0]]
    codes[m2[0], 0] = (codes[m2[0], 0] & 0xFC) | 1
    codes[m2[1], 0] = (codes[m2[1], 0] & 0xFC) | 2
    g3 = sizes.index(3)
    m3 = order[starts[g3]:starts[g3 + 1]]
    codes[m3[2]] = codes[m3[1]]
    gb = sizes.index(2049)
    mb = order[starts[gb]:starts[gb + 1]]
    for _ in range(8):                       # (two members moved onto the centroid may move the centroid: repeat until it stands)
        cent = model(codes[mb], np.zeros(len(mb), np.uint32))[1][0]
        if np.array_equal(codes[mb[700]], cent) and np.array_equal(codes[mb[1500]], cent):
            break
        codes[mb[700]] = codes[mb[1500]] = cent
    codes.setflags(write=False)
    labels.setflags(write=False)
    return codes, labels


@functools.lru_cache(maxsize=None)
def tier_expect(bits, id_base=0):
    codes, labels = tier_case(bits, id_base)
    return model(codes, labels, id_base)


def clustered_codes(n, bits, seed, centres=40, flips=3):
    """centres + at most `flips` flipped bits each: near-duplicate groups for the end-to-end cases"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(centres, bits // 8), dtype=np.uint8)
    codes = base[rng.integers(0, centres, size=n)].copy()
    for i in range(n):
        for b in rng.integers(0, bits, size=rng.integers(0, flips + 1)):
            codes[i, b // 8] ^= np.uint8(1 << (b % 8))
    return codes
