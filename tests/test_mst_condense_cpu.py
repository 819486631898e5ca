"""vc_mst_condense* without a GPU: the ABI surface, the code objects of the kernels, the plan arithmetic under the sanitizers, and the
expectation of test_mst_condense_gpu.py -- that the model's bottom-up loop and a top-down formulation over knn_mst_common.cut_model
agree on every input and on all small forests, that its selection is the best antichain a brute force finds, and the figures of the
forests the GPU tests run on."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import condense_common as CC
import knn_graph_common as KG
import knn_mst_common as KM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_new_names(vc):
    txt = open(os.path.join(ROOT, "include", "verticut_gpu.h")).read()
    assert re.search(r"#define\s+VC_ABI_VERSION\s+2\b", txt)             # entry points are only added
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"typedef struct vc_condensed_node\s*\{\s*uint32_t parent;\s*uint32_t rep;\s*uint32_t form;\s*uint32_t end;\s*uint32_t size;\s*uint32_t n_children;"
                     r"\s*uint32_t flags;\s*uint32_t pad;\s*uint64_t stability;\s*uint64_t best;\s*\}\s*vc_condensed_node;", code)
    assert re.search(r"typedef struct vc_mst_condense_stats\s*\{\s*uint64_t n_nodes;\s*uint64_t n_leaves;\s*uint64_t n_roots;\s*uint64_t n_selected;\s*uint64_t n_clustered;"
                     r"\s*uint64_t n_noise;\s*uint64_t total_stability;\s*uint32_t n_levels;\s*uint32_t pad;\s*\}\s*vc_mst_condense_stats;", code)
    for name, value in (("VC_CONDENSE_EOM", "0u"), ("VC_CONDENSE_LEAF", "1u"), ("VC_CONDENSE_NONE", "0xFFFFFFFFu"), ("VC_CONDENSE_SELECTED", "1u"),
                        ("VC_CONDENSE_KEEP", "2u"), ("VC_CONDENSE_ROOT", "4u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), code), name
    assert code.index("vc_label_propagate_stats* stats);") < code.index("VC_CONDENSE_EOM") < code.index("vc_device_status")   # after the vc_label_propagate* block
    assert code.index("int vc_sharded_label_propagate(") < code.index("int vc_sharded_mst_condense_dev(")
    L = ctypes.CDLL(vc.LIB_PATH)
    for name in CC.NAMES:
        assert hasattr(L, name), name
        assert name in vc.EXPORTS
    args = (r"uint64_t n_edges,\s*uint32_t min_cluster_size,\s*uint32_t root_weight,\s*uint32_t method,\s*vc_condensed_node\* %snodes,\s*uint32_t\* %slabels,"
            r"\s*uint32_t\* %snode,\s*uint32_t\* %sown,\s*uint32_t\* %sleave,\s*vc_mst_condense_stats\* stats")
    for name in ("vc_mst_condense_dev", "vc_sharded_mst_condense_dev"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*const vc_mst_edge\* d_edges,\s*%s,\s*void\* stream\)" % (name, args % (("d_",) * 5)), code), name
    for name in ("vc_mst_condense", "vc_sharded_mst_condense"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*const vc_mst_edge\* edges,\s*%s\)" % (name, args % (("",) * 5)), code), name
    flat = " ".join(txt.split()).replace(" * ", " ")
    for phrase in ("NOT OFFERED: an incremental form; the condensed tree and stability selection (host work on N - 1 edges); N kk above 2^31 - 1.",
                   "vc_mst_condense* below takes these edges as they are", "only a, b and weight are read", "must be a FOREST over the N resident records",
                   "the order of the edges WITHIN one weight influences no output word", "min_cluster_size (mcs) lies in 2 .. 2^31",
                   "A component of size >= mcs always carries exactly one live cluster", "two or more big children", "exactly one big child",
                   "rep(C) is the smallest global id of C's component at its end", "stability(C) = end(C) size(C) - the sum of leave(p)",
                   "A root under root_weight == 0 has stability 0 and is never selected", "ascending by (form, rep)", "a tie going to the parent",
                   "words beyond n_nodes are untouched", "otherwise the record's OWN global id", "ERRORS, checked before any work", "NO OUTPUT WORD WRITTEN",
                   "the components at the end must number N - n_edges", "n_edges == 0 gives no nodes and identity labels", "WAITS: three small read-backs",
                   "no shard is touched"):
        assert " ".join(phrase.split()) in flat, phrase
    assert vc.VC_ABI_VERSION == 2 and (vc.CONDENSE_EOM, vc.CONDENSE_LEAF, vc.CONDENSE_NONE) == (CC.EOM, CC.LEAF, CC.NONE)
    assert (vc.CONDENSE_SELECTED, vc.CONDENSE_KEEP, vc.CONDENSE_ROOT) == (CC.SELECTED, CC.KEEP, CC.ROOT)
    st = vc.VcMstCondenseStats
    assert ctypes.sizeof(st) == 64 and [getattr(st, n).offset for n in CC.STATS] == [0, 8, 16, 24, 32, 40, 48, 56]
    assert st().as_dict() == CC.zero_stats()
    assert vc.CONDENSED_NODE == CC.NODE and vc.CONDENSED_NODE.itemsize == 48
    assert [vc.CONDENSED_NODE.fields[f][1] for f in CC.NODE.names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40]
    for cls in (vc.Engine, vc.ShardedEngine):
        for meth in ("mst_condense", "mst_condense_dev"):
            assert callable(getattr(cls, meth)), (cls, meth)
    host = open(os.path.join(ROOT, "verticut_amd", "host", "verticut_host.hpp")).read()
    assert re.search(r"virtual int mst_condense\([^)]*\)\s*=\s*0;", host) and len(re.findall(r"int mst_condense\([^)]*\)\s*override", host)) == 2
    for call in ("return vc_mst_condense(h_,", "return vc_sharded_mst_condense(h_,"):
        assert call in host, call
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "5.23" in design and "vc_mst_condense" in design and "unmeasured" in design
    for doc in ("README.md", "INTEGRATION.md", os.path.join("profiles", "README.md")):
        assert "vc_mst_condense" in open(os.path.join(ROOT, doc)).read() or "mst_condense" in open(os.path.join(ROOT, doc)).read(), doc
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_mst_condense.py"))


def test_condense_kernels_use_no_scratch_and_no_lds(vc):
    from verticut_amd import build as vb
    assert "vc_mst_condense.hip" in vb.SOURCES and "vc_mst_condense_plan.hpp" in vb.HEADERS
    res = vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_mst_condense.o"))
    kernels = ("vc_cond_init_kernel", "vc_cond_plan_kernel", "vc_cond_unite_kernel", "vc_cond_tally_kernel", "vc_cond_decide_kernel", "vc_cond_apply_kernel",
               "vc_cond_settle_kernel", "vc_cond_roots_kernel", "vc_cond_keys_kernel", "vc_cond_rank_kernel", "vc_cond_write_kernel", "vc_cond_fold_kernel",
               "vc_cond_select_kernel", "vc_cond_label_kernel")
    for kernel in kernels:
        assert sum(kernel in name for name in res) == 1, (kernel, sorted(res))
    assert len(res) == len(kernels), sorted(res)
    for name, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == 0, (name, r)
    text = open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_mst_condense.hip")).read()
    for word in ("hipLaunchCooperativeKernel", "grid_group", "__shared__", "getenv", "asm"):
        assert word not in text, word
    assert '#include "vc_forest.hpp"' in text and "cl_unite(" in text and "void cl_unite" not in text   # vc_forest.hpp's union, not a copy
    assert "vc_radix_sort_items(" in text                                                               # vc_sort.hip's sort, not a copy


def test_plan_arithmetic_under_the_sanitizers(tmp_path):
    """tests/cpp/condense_plan_test.cc over csrc/vc_mst_condense_plan.hpp, host code only, a stand-alone program with AddressSanitizer and
    UBSan; the figures it prints are those of the model's mirror"""
    src = os.path.join(ROOT, "tests", "cpp", "condense_plan_test.cc")
    exe = tmp_path / "condense_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           src, "-I", os.path.join(ROOT, "verticut_amd", "csrc")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert out.stdout.startswith("condense plan ok: NODE 48 STAT 64 WORK_NODE 40 RECORD_WORDS 12\n")
    for n in (1, 2, 513, 2048, 3000, 9000, 1000000):
        line = "SCRATCH %d %d %d %d %d" % (n, CC.work_bytes(n), CC.tree_bytes(n), CC.sort_bytes(n), CC.stage_total(n, n - 1))
        assert re.search("^%s$" % line, out.stdout, flags=re.M), line
    for mcs in (2, 5, 25):
        assert re.search(r"^BOUND %d %d$" % (mcs, CC.node_bound(3000, mcs)), out.stdout, flags=re.M), mcs


# ---- the model is the contract: a second formulation, top-down ------------------------------------------------------------------------------------
def top_down(n, edges, mcs, root_weight, id_base=0):
    """the condensed tree from the components at every height (knn_mst_common.cut_model), from the top: a cluster is followed downwards
    through the one part of size >= mcs it keeps, splits where two or more such parts appear at the next lower height, and was formed
    where none does.  Returns {(form, rep): (parent key | None, end, size, n_children, stability, root)}, own [n] as keys | None,
    leave [n]; the stability is the plain sum over the members of end - leave."""
    heights = sorted({int(w) for w in edges["weight"]})
    parts = []                                                   # parts[t]: the components at heights[t] as {root position: members}
    for h in heights:
        labels = KM.cut_model(n, edges, h, id_base)[0]
        comp = {}
        for i, root in enumerate(labels.tolist()):
            comp.setdefault(root - id_base, []).append(i)
        parts.append(comp)
    nodes, own, leave = {}, [None] * n, [NONE] * n
    # the recursion is written with an explicit stack: chains are hundreds of levels deep
    where = []                                                    # where[t][record] = its root at heights[t]
    for comp in parts:
        w = [0] * n
        for root, members in comp.items():
            for p in members:
                w[p] = root
        where.append(w)
    stack = [(len(heights) - 1, root, root_weight, None, True) for root, members in (parts[-1] if parts else {}).items() if len(members) >= mcs]
    while stack:
        t, root, end, parent, is_root = stack.pop()
        members = parts[t][root]
        rep, size = min(members) + id_base, len(members)
        left = []                                                 # (record, the height at which it left the cluster)
        current = members
        while True:
            h = heights[t]
            pieces = {}
            for p in current:
                pieces.setdefault(where[t - 1][p] if t else p, []).append(p)
            big = [r for r, m in pieces.items() if len(m) >= mcs]
            if len(big) == 1:                                     # goes on downwards; the small parts leave here
                for r, m in pieces.items():
                    if r != big[0]:
                        left += [(p, h) for p in m]
                current, t = pieces[big[0]], t - 1
                continue
            left += [(p, h) for p in current]                     # formed here: everybody still inside leaves at h
            form, children = h, big
            break
        key = (form, rep)
        assert key not in nodes
        assert len(left) == size
        nodes[key] = (parent, end, size, len(children), 0 if is_root and root_weight == 0 else sum(end - at for _, at in left), is_root)
        small = {p for r, m in pieces.items() if r not in children for p in m} if children else set(current)
        for p, at in left:
            if at != form or p in small:
                own[p], leave[p] = key, at
        for r in children:
            stack.append((t - 1, r, form, key, False))
    return nodes, own, leave


NONE = CC.NONE


def _agree(n, edges, mcs, root_weight, id_base=0):
    """the model's tree, stabilities, own and leave against top_down's"""
    nodes, _, _, own, leave, st = CC.condense_model(n, edges, mcs, root_weight, CC.EOM, id_base)
    want, want_own, want_leave = top_down(n, edges, mcs, root_weight, id_base)
    keys = [(int(x["form"]), int(x["rep"])) for x in nodes]
    assert keys == sorted(want), (n, mcs, root_weight)
    for t, x in enumerate(nodes):
        parent, end, size, n_children, stability, is_root = want[keys[t]]
        assert (keys[int(x["parent"])] if int(x["parent"]) != NONE else None) == parent and int(x["parent"]) > t
        assert (int(x["end"]), int(x["size"]), int(x["n_children"]), int(x["stability"]), bool(int(x["flags"]) & CC.ROOT)) == (end, size, n_children, stability, is_root), (keys[t],)
        assert int(x["end"]) > int(x["form"]) or is_root
    assert [keys[o] if o != NONE else None for o in own.tolist()] == want_own and leave.tolist() == want_leave
    assert st["n_levels"] == len(set(edges["weight"].tolist())) and st["n_roots"] == sum(1 for v in want.values() if v[5])
    return nodes, st


EXHAUSTIVE_N = 5      # forests of up to this many records run under EVERY assignment of the weights


def _small_forests(max_n=7, max_weight=3):
    """every forest over up to max_n records as a parent array (record i hangs on an earlier one or on nothing): 5 913 of them.  Those of
    up to EXHAUSTIVE_N records come under every assignment of the weights 0 .. max_weight (10 581 weighted forests); those of 6 and 7
    records under ONE assignment drawn at random each (all of them would be 20 million)"""
    rng = np.random.default_rng(17)
    for n in range(1, max_n + 1):
        for parents in itertools.product(*[range(-1, i) for i in range(1, n)]):
            pairs = [(i + 1, p) for i, p in enumerate(parents) if p >= 0]
            if n <= EXHAUSTIVE_N:
                choices = itertools.product(range(max_weight + 1), repeat=len(pairs))
            else:
                choices = [tuple(int(x) for x in rng.integers(0, max_weight + 1, len(pairs)))]
            for weights in choices:
                yield n, CC.to_edges([(a, b, w) for (a, b), w in zip(pairs, weights)])


def test_the_model_agrees_with_the_top_down_formulation_on_all_small_forests():
    """Every forest structure of up to 7 records with weights in 0 .. 3 -- exhaustively in the weights up to 5 records, one random
    assignment each at 6 and 7.  Up to 4 records every (min_cluster_size, root_weight) of {2, 3} x {0, 4} is tried on every weighted
    forest; above, the pairs (and min_cluster_size 4) take turns from one forest to the next."""
    pairs = ((2, 0), (3, 4), (2, 4), (3, 0))
    turns = itertools.cycle(pairs + ((4, 4),))
    seen = nodes_seen = split = 0
    for n, edges in _small_forests():
        for mcs, root_weight in (pairs if n <= 4 else (next(turns),)):
            nodes, _ = _agree(n, edges, mcs, root_weight)
            seen += 1
            nodes_seen += len(nodes)
            split += len(nodes) >= 3
    assert seen > 18000 and nodes_seen > 9000 and split > 300


def test_the_model_agrees_with_the_top_down_formulation_on_the_gpu_inputs():
    for name, cases in (("attach", ((2, 0), (5, 0), (25, 65))), ("ruler", ((2, 0), (2, 65), (5, 57))), ("thermo", ((2, 0), (40, 513)))):
        n, bits, edges = CC.forest(name)
        for mcs, root_weight in cases:
            _agree(n, edges, mcs, root_weight)
    n, _, edges = CC.forest("attach", 300)
    _agree(n, edges, 5, 65, 300)
    codes = KM.graph("clustered", 12)[0]
    for flags in (KM.MUTUAL, KM.EITHER):
        edges = KM.model("clustered", 12, 10, flags, weight_kind=KM.REACHABILITY, min_pts=5)[0]
        for root_weight in (0, int(edges["weight"].max()) + 1):
            _agree(len(codes), edges, 5, root_weight)
    edges = KM.model("dup", KG.DUP_K, KG.DUP_K, KM.EITHER)[0]
    _agree(KG.DUP_N, edges, 5, 3)


# ---- the selection: the best antichain, by brute force --------------------------------------------------------------------------------------------
def _brute_force_selection(parents, stabilities, allowed):
    """of all antichains of allowed nodes the one of the largest total stability; among equal totals the one that covers the most nodes
    (a tie goes to the parent, and a parent covers what its children cover and itself).  Sets of nodes are bit masks."""
    m = len(parents)
    above = [0] * m                                   # the ancestors of i
    for i in range(m - 1, -1, -1):
        if parents[i] != NONE:
            above[i] = above[parents[i]] | 1 << parents[i]
    banned = sum(1 << i for i in range(m) if not allowed[i])
    best_score, best = None, []
    for mask in range(1 << m):
        if mask & banned:
            continue
        total, ok = 0, True
        for i in range(m):
            if mask >> i & 1:
                if above[i] & mask:
                    ok = False
                    break
                total += stabilities[i]
        if not ok:
            continue
        score = (total, sum(1 for i in range(m) if (above[i] | 1 << i) & mask))
        if best_score is None or score > best_score:
            best_score, best = score, [mask]
        elif score == best_score:
            best.append(mask)
    assert len(best) == 1, "of two antichains with the largest total one covers more"
    return [i for i in range(m) if best[0] >> i & 1]


def test_the_selection_is_the_best_antichain():
    """on the condensed trees of random forests of 2 .. 15 nodes (at most eight of 14 or 15: a tree of 15 has 32 768 subsets), and on the
    same trees with random stabilities full of ties"""
    rng = np.random.default_rng(23)
    trees = with_choice = internal = large = 0
    while trees < 150 or large < 8:
        n = int(rng.integers(8, 40))
        triples = [(i, int(rng.integers(0, i)), int(rng.integers(0, 6))) for i in range(1, n) if rng.random() < 0.93]
        for root_weight in (0, 6):
            nodes = CC.condense_model(n, CC.to_edges(triples), 2, root_weight)[0]
            m = len(nodes)
            if not 2 <= m <= 15 or (m >= 14 and large >= 8) or (m < 14 and trees >= 150):
                continue
            large += m >= 14
            parents = [int(p) for p in nodes["parent"]]
            allowed = [not (int(f) & CC.ROOT and root_weight == 0) for f in nodes["flags"]]
            for stabilities in ([int(s) for s in nodes["stability"]], [int(s) if a else 0 for s, a in zip(rng.integers(0, 4, m), allowed)]):
                keep, best, selected = CC.select(parents, stabilities, allowed, CC.EOM)
                chosen = [i for i in range(m) if selected[i]]
                assert chosen == _brute_force_selection(parents, stabilities, allowed), (parents, stabilities, allowed)
                assert sum(stabilities[i] for i in chosen) == sum(best[i] for i in range(m) if parents[i] == NONE)
                trees += 1
                with_choice += any(selected[i] != keep[i] for i in range(m))
                internal += any(selected[i] and any(p == i for p in parents) for i in range(m))
    assert with_choice > 20 and internal > 20 and large == 8
    # the leaf method: the leaves, but for a lone root under root_weight 0
    parents, stabilities = [2, 2, NONE, NONE], [5, 1, 9, 4]
    assert CC.select(parents, stabilities, [True, True, False, False], CC.LEAF)[2] == [True, True, False, False]
    assert CC.select(parents, stabilities, [True] * 4, CC.LEAF)[2] == [True, True, False, True]
    assert CC.select(parents, stabilities, [True] * 4, CC.EOM)[2] == [False, False, True, True]
    assert CC.select(parents, [5, 4, 9, 4], [True] * 4, CC.EOM)[:2] == ([True, True, True, True], [5, 4, 9, 4])     # 9 == 5 + 4: the tie goes to the parent
    assert CC.select(parents, [5, 5, 9, 4], [True] * 4, CC.EOM)[2] == [True, True, False, True]


# ---- the pins: the figures of the forests test_mst_condense_gpu.py runs on -------------------------------------------------------------------------
def _ties(nodes):
    """the parents whose stability EQUALS the sum of their children's best"""
    sub = np.zeros(len(nodes), dtype=np.uint64)
    for x in nodes:
        if int(x["parent"]) != NONE:
            sub[int(x["parent"])] += x["best"]
    return int(((nodes["n_children"] > 0) & (nodes["stability"] == sub)).sum())


def test_the_attach_forest():
    n, bits, edges = CC.forest("attach")
    assert (n, bits, len(edges)) == (3000, 64, 2999) and np.all(np.diff(edges["weight"].astype(np.int64)) >= 0)
    nodes, labels, node, own, leave, st = CC.model("attach", 5)
    assert (st["n_levels"], st["n_nodes"], st["n_noise"], st["n_roots"]) == (65, 271, 1095, 1) and CC.depth(nodes) - 1 == 38
    assert CC.depth(nodes) >= 10 and st["n_noise"] >= 100
    assert int((nodes["n_children"] >= 3).sum()) == 33                                             # multiway nodes
    selected = (nodes["flags"] & CC.SELECTED) != 0
    assert int((selected & (nodes["n_children"] > 0)).sum()) == 8                                  # selected nodes that have children
    raw = CC.tree_model(n, edges, 5, 0)[0]
    assert sum(1 for r in raw if r["sum_leave"] != r["form"] * r["size"]) == 158                   # clusters that absorbed small components
    assert st["n_nodes"] <= CC.node_bound(n, 5) and st["n_selected"] == int(selected.sum()) == 168 and st["n_clustered"] + st["n_noise"] == n
    assert np.all(labels[node == NONE] == np.flatnonzero(node == NONE)) and np.all(own[node != NONE] != NONE)
    assert int(((own != NONE) & (node == NONE)).sum()) > 0                                         # records of a cluster that was not chosen are noise
    leaf = CC.model("attach", 5, 0, CC.LEAF)
    assert leaf[5]["n_selected"] == leaf[5]["n_leaves"] == 190 and np.array_equal(leaf[0]["stability"], nodes["stability"]) and not np.array_equal(leaf[1], labels)
    assert CC.model("attach", 2)[5]["n_nodes"] > CC.model("attach", 5)[5]["n_nodes"] > CC.model("attach", 25)[5]["n_nodes"] > 3
    high = CC.model("attach", 5, 65)
    assert int(edges["weight"].max()) == 64 and int(nodes[-1]["stability"]) == 0 and int(high[0][-1]["stability"]) > 0 and high[5]["n_roots"] == 1


def test_the_ruler_forest():
    n, bits, edges = CC.forest("ruler")
    assert (n, bits, len(edges)) == (2048, 64, 2044)
    nodes, labels, node, own, leave, st = CC.model("ruler", 2)
    assert (st["n_roots"], st["n_noise"], st["n_levels"]) == (4, 0, 26) and st["n_nodes"] == 2044 <= CC.node_bound(n, 2)
    assert _ties(nodes) == 67                                                                      # the tie rule is exercised
    assert np.all((nodes["flags"][(nodes["flags"] & CC.ROOT) != 0] & (CC.KEEP | CC.SELECTED)) == 0)   # no whole component under root_weight 0
    top = CC.model("ruler", 2, 65)
    chosen = np.flatnonzero((top[0]["flags"] & CC.SELECTED) != 0)
    assert top[5]["n_selected"] == 4 and np.all((top[0]["flags"][chosen] & CC.ROOT) != 0)          # exactly the four roots
    assert sorted(set(top[1].tolist())) == [0, 512, 1024, 1536]


def test_the_chain_the_duplicates_and_the_degenerate_cases():
    n, bits, edges = CC.forest("thermo")
    assert (n, bits) == (513, 512) and len(np.unique(edges["weight"])) == 512
    assert CC.model("thermo", 2)[5]["n_levels"] == 512 and CC.depth(CC.model("thermo", 2)[0]) > 10
    none = np.zeros(0, dtype=CC.EDGE)
    for m in (0, 1, 2, 9):
        nodes, labels, node, own, leave, st = CC.condense_model(m, none, 2, id_base=40)
        assert len(nodes) == 0 and labels.tolist() == list(range(40, 40 + m)) and st == dict(CC.zero_stats(), n_noise=m)
    pair = CC.to_edges([(1, 0, 7)], 40)
    assert CC.condense_model(2, pair, 2, 0, id_base=40)[1].tolist() == [40, 41]                    # a lone root under root_weight 0: noise
    nodes, labels, *_ = CC.condense_model(2, pair, 2, 8, id_base=40)
    assert labels.tolist() == [40, 40] and tuple(nodes[0]) == (NONE, 40, 7, 8, 2, 0, CC.SELECTED | CC.KEEP | CC.ROOT, 0, 2, 2)
    # the order within a weight and the direction of an edge change nothing
    n, _, edges = CC.forest("attach")
    mixed = CC.shuffled_within_weights(edges, 1)
    assert not np.array_equal(mixed, edges)
    CC.same(CC.condense_model(n, mixed, 5, 65), CC.model("attach", 5, 65), "shuffled")
