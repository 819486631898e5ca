"""The model of vc_mst_condense*, shared by test_mst_condense_cpu.py (which pins it against a top-down formulation over
knn_mst_common.cut_model and the selection against a brute force over all antichains) and test_mst_condense_gpu.py.  A plain loop over
the levels, written straight from the contract's table of cases: the components before a level, the groups the level's edges make
of them, big and small children, the node that forms, goes on or does not exist.  Also a mirror of vc_mst_condense_plan.hpp and the
forests the GPU tests run on."""
import functools

import numpy as np

import knn_mst_common as KM

EOM, LEAF = 0, 1
NONE = 0xFFFFFFFF
SELECTED, KEEP, ROOT = 1, 2, 4
MAX_MCS = 2 ** 31
EDGE = KM.EDGE
NODE = np.dtype([("parent", np.uint32), ("rep", np.uint32), ("form", np.uint32), ("end", np.uint32), ("size", np.uint32), ("n_children", np.uint32),
                 ("flags", np.uint32), ("pad", np.uint32), ("stability", np.uint64), ("best", np.uint64)])   # vc_condensed_node
STATS = ("n_nodes", "n_leaves", "n_roots", "n_selected", "n_clustered", "n_noise", "total_stability", "n_levels")
NAMES = ["vc_mst_condense", "vc_mst_condense_dev", "vc_sharded_mst_condense", "vc_sharded_mst_condense_dev"]


def zero_stats():
    return dict.fromkeys(STATS, 0)


# ---- the plan (vc_mst_condense_plan.hpp) ----------------------------------------------------------------------------------------------------
def words4(words):
    return (words * 4 + 7) & ~7


def node_bound(n, mcs):
    return 2 * (n // mcs) - 1 if n >= mcs else 0


def work_bytes(n):
    return 12 * words4(n)


def tree_bytes(n):
    m = max(n - 1, 1)
    return m * 40 + 4 * words4(m) + m * 8


def sort_bytes(n):
    m = max(n - 1, 1)
    return 2 * (m * 8 + words4(m))


def stage_total(n, n_edges):
    return max(n_edges * 16 + max(n - 1, 0) * 48 + 4 * words4(n), 8)


# ---- the tree --------------------------------------------------------------------------------------------------------------------------------
def tree_model(n, edges, mcs, root_weight, id_base=0):
    """the condensed tree bottom-up.  Returns (nodes: list of dicts parent / rep / form / end / size / children / sum_leave / root in the
    order of creation, own [n] as indices into that list or NONE, leave [n], the number of levels)"""
    members = {i: [i] for i in range(n)}       # root position -> the records of its component
    where = list(range(n))                      # record -> root position
    carried = {}                                # root position -> the node its component carries
    nodes, own, leave = [], [NONE] * n, [NONE] * n
    weights = [int(w) for w in edges["weight"]]
    levels = sorted(set(weights))
    for w in levels:
        # the groups of previous components that the edges of weight w join: a small union-find over the previous roots
        up = {}

        def find(x):
            while up.setdefault(x, x) != x:
                up[x] = up[up[x]]
                x = up[x]
            return x

        for e, ew in zip(edges, weights):
            if ew == w:
                ra, rb = find(where[int(e["a"]) - id_base]), find(where[int(e["b"]) - id_base])
                if ra != rb:
                    up[max(ra, rb)] = min(ra, rb)
        groups = {}
        for old in list(up):
            groups.setdefault(find(old), []).append(old)
        for new_root, olds in groups.items():
            big = [o for o in olds if len(members[o]) >= mcs]
            small = [o for o in olds if len(members[o]) < mcs]
            total = sum(len(members[o]) for o in olds)
            node = None
            if len(big) >= 2:
                node = len(nodes)
                nodes.append(dict(parent=NONE, rep=NONE, form=w, end=NONE, size=total, children=[carried[o] for o in big], sum_leave=w * total, root=False))
                for o in big:
                    nodes[carried[o]].update(parent=node, end=w, rep=o + id_base)
            elif len(big) == 1:
                node = carried[big[0]]
                grown = sum(len(members[o]) for o in small)
                nodes[node]["size"] += grown
                nodes[node]["sum_leave"] += w * grown
            elif total >= mcs:
                node = len(nodes)
                nodes.append(dict(parent=NONE, rep=NONE, form=w, end=NONE, size=total, children=[], sum_leave=w * total, root=False))
            if node is not None:
                for o in (small if big else olds):
                    for p in members[o]:
                        own[p], leave[p] = node, w
            merged = sorted(p for o in olds for p in members[o])
            for o in olds:
                del members[o]
                carried.pop(o, None)
            members[new_root] = merged
            for p in merged:
                where[p] = new_root
            if node is not None:
                carried[new_root] = node
    for root, node in carried.items():
        nodes[node].update(end=root_weight, rep=root + id_base, root=True)
    return nodes, own, leave, len(levels)


def stability(node, root_weight):
    """end * size - the sum of the leave levels; none for a root under root_weight 0"""
    return 0 if node["root"] and root_weight == 0 else node["end"] * node["size"] - node["sum_leave"]


def select(parents, stabilities, allowed, method):
    """parents[i] > i or NONE.  Returns (keep, best, selected) lists: the ascending excess-of-mass pass, then the choice top-down"""
    m = len(parents)
    sub, keep, best = [0] * m, [False] * m, [0] * m
    n_children = [0] * m
    for i in range(m):
        keep[i] = allowed[i] and stabilities[i] >= sub[i]        # a tie goes to the parent
        best[i] = stabilities[i] if keep[i] else sub[i]
        if parents[i] != NONE:
            assert parents[i] > i
            sub[parents[i]] += best[i]
            n_children[parents[i]] += 1
    cand = keep if method == EOM else [allowed[i] and n_children[i] == 0 for i in range(m)]
    selected, covered = [False] * m, [False] * m
    for i in range(m - 1, -1, -1):
        above = parents[i] != NONE and covered[parents[i]]
        selected[i] = cand[i] and not above
        covered[i] = above or selected[i]
    return keep, best, selected


def condense_model(n, edges, mcs, root_weight=0, method=EOM, id_base=0):
    """(nodes NODE [n_nodes], labels uint32 [n], node [n], own [n], leave [n], stats dict) of the contract"""
    raw, own_raw, leave, n_levels = tree_model(n, edges, mcs, root_weight, id_base)
    order = sorted(range(len(raw)), key=lambda j: (raw[j]["form"], raw[j]["rep"]))
    assert len({(raw[j]["form"], raw[j]["rep"]) for j in order}) == len(raw)          # the order is strict
    number = {j: t for t, j in enumerate(order)}
    m = len(raw)
    parents = [number[raw[j]["parent"]] if raw[j]["parent"] != NONE else NONE for j in order]
    stabilities = [stability(raw[j], root_weight) for j in order]
    allowed = [not (raw[j]["root"] and root_weight == 0) for j in order]
    keep, best, selected = select(parents, stabilities, allowed, method)
    nodes = np.zeros(m, dtype=NODE)
    for t, j in enumerate(order):
        r = raw[j]
        flags = (SELECTED if selected[t] else 0) | (KEEP if keep[t] else 0) | (ROOT if r["root"] else 0)
        nodes[t] = (parents[t], r["rep"], r["form"], r["end"], r["size"], len(r["children"]), flags, 0, stabilities[t], best[t])
    sel_anc = [NONE] * m
    for t in range(m - 1, -1, -1):
        sel_anc[t] = t if selected[t] else (sel_anc[parents[t]] if parents[t] != NONE else NONE)
    own = np.array([number[j] if j != NONE else NONE for j in own_raw], dtype=np.uint32).reshape(n)
    node = np.array([sel_anc[o] if o != NONE else NONE for o in own.tolist()], dtype=np.uint32).reshape(n)
    labels = np.array([int(nodes[s]["rep"]) if s != NONE else id_base + i for i, s in enumerate(node.tolist())], dtype=np.uint32).reshape(n)
    clustered = int((node != NONE).sum())
    st = dict(n_nodes=m, n_leaves=sum(1 for r in raw if not r["children"]), n_roots=sum(1 for r in raw if r["root"]), n_selected=sum(selected),
              n_clustered=clustered, n_noise=n - clustered, total_stability=sum(s for s, c in zip(stabilities, selected) if c), n_levels=n_levels)
    return nodes, labels, node, own, np.array(leave, dtype=np.uint32).reshape(n), st


def depth(nodes):
    """the longest chain of nodes, a root counting 1"""
    d = [1] * len(nodes)
    for t in range(len(nodes) - 1, -1, -1):
        if int(nodes[t]["parent"]) != NONE:
            d[t] = d[int(nodes[t]["parent"])] + 1
    return max(d, default=0)


def same(got, want, what=None):
    """every word: nodes, labels, node, own, leave (None = not asked for) and the stats"""
    assert got[0].dtype == NODE and len(got[0]) == len(want[0]), (what, "n_nodes", len(got[0]), len(want[0]))
    for field in NODE.names:
        assert np.array_equal(got[0][field], want[0][field]), (what, "nodes", field)
    for at, name in ((1, "labels"), (2, "node"), (3, "own"), (4, "leave")):
        if got[at] is not None:
            assert np.array_equal(got[at], want[at]), (what, name)
    if got[5] is not None:
        assert got[5] == want[5], (what, got[5], want[5])


# ---- the inputs -----------------------------------------------------------------------------------------------------------------------------
def to_edges(triples, id_base=0):
    """(a, b, weight) positions -> EDGE records ascending in weight (stable); dist is a word the call must not read"""
    out = np.zeros(len(triples), dtype=EDGE)
    for t, (a, b, w) in enumerate(sorted(triples, key=lambda e: e[2])):
        out[t] = (a + id_base, b + id_base, w, 0xDEAD)
    return out


@functools.lru_cache(maxsize=None)
def forest(name, id_base=0):
    """(n, bits, edges): "attach" -- record i hangs on a random earlier one at a random weight 0 .. 64, every height with small and big
    joins; "ruler" -- four chains of 512 whose weights follow the ruler sequence, a balanced tree with ties between a parent and its
    children; "thermo" -- one chain of 513 records with the weights 0 .. 512 in a random place each, every level of a 512-bit code"""
    rng = np.random.default_rng(5)
    if name == "attach":
        n, bits = 3000, 64
        triples = [(i, int(rng.integers(0, i)), int(rng.integers(0, 65))) for i in range(1, n)]
    elif name == "ruler":
        n, bits = 2048, 64
        tz = lambda i: (i & -i).bit_length() - 1
        triples = [(i, i - 1, min(64, 4 * tz(i) + int(rng.integers(0, 3)))) for i in range(1, n) if i % 512]
    elif name == "thermo":
        n, bits = 513, 512
        weights = rng.permutation(513)[:512]
        triples = [(i, i - 1, int(weights[i - 1])) for i in range(1, n)]
    else:
        raise KeyError(name)
    edges = to_edges(triples, id_base)
    edges.setflags(write=False)
    return n, bits, edges


@functools.lru_cache(maxsize=None)
def model(name, mcs, root_weight=0, method=EOM, id_base=0):
    n, _, edges = forest(name, id_base)
    return condense_model(n, edges, mcs, root_weight, method, id_base)


def shuffled_within_weights(edges, seed):
    """the same edges with every weight class randomly permuted and the two ends of some edges swapped"""
    rng = np.random.default_rng(seed)
    out = edges.copy()
    for w in np.unique(edges["weight"]):
        at = np.flatnonzero(edges["weight"] == w)
        out[at] = edges[rng.permutation(at)]
    swap = rng.random(len(out)) < 0.5
    out["a"][swap], out["b"][swap] = out["b"][swap].copy(), out["a"][swap].copy()
    return out
