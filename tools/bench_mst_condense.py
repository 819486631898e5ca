"""The condensed tree of a spanning forest and its selection (vc_mst_condense_dev) against its floor and the path it replaces: clustered
synthetic 64-bit codes (the store of bench_knn_mst.py: 1e6 records, 16 per centre, up to 6 flipped bits), m = 2, the graph built once
per k by vc_knn_graph_dev in exact MIH, the forest by vc_knn_mst_dev under VC_MST_REACHABILITY with min_pts 5, one engine, k = kk = 10
and k = kk = 100, both flags; min_cluster_size 5, root_weight = the largest weight + 1, VC_CONDENSE_EOM.

  condense_mutual / _either   vc_mst_condense_dev with nodes, labels, node, own and leave, buffers warm
  cut_mutual / cut_either     vc_mst_cut_dev at the top height on the same edges: ONE union pass and a flatten, the floor of a level
  host                        the replaced path, once per flag: the edges copied home, then the condensation on the host -- a Python
                              loop over the levels with a union-find in lists (the tests' model is a plainer loop and slower).  The
                              model runs under an alarm of --host-limit seconds (60): reported as a time only when it ends within
                              it; otherwise the JSON says that it did not.

Per k one child process under its own `timeout`, the next only after the one before succeeded.  In it, before anything is timed, for
both flags: EVERY word of the device's nodes, labels, node, own, leave and statistics == the host model's over the whole store
(asserted).  Where the model ran into its alarm, the same assertion is made on a store of --prefix (1e5) records built the same way,
whose model gets ten times the limit, and the JSON says so.  Then the device legs interleaved, a host clock around each ending in a
device synchronise, medians of --reps with min .. max.  No ratio is fixed in advance.  Prints one JSON line; --out also writes it to a file.

    python tools/bench_mst_condense.py [--n 1e6] [--ks 10,100] [--reps 7] [--out profiles/mst_condense_bench.json]
"""
import argparse
import json
import os
import signal
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NONE = 0xFFFFFFFF


def host_condense(n, a, b, w, mcs, root_weight):
    """the contract on the host, VC_CONDENSE_EOM: (nodes as a dict of arrays in the order (form, rep), labels, node, own, leave, stats)"""
    parent, size = list(range(n)), [1] * n
    carried, members = {}, {}                    # root -> its node; root -> the records of a component that has no node (and two records or more)
    form, rep, end, sz, nch, sum_leave, par, is_root = [], [], [], [], [], [], [], []
    own, leave = [NONE] * n, [NONE] * n

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    def new_node(weight, total, children):
        form.append(weight); rep.append(NONE); end.append(NONE); sz.append(total); nch.append(children); sum_leave.append(weight * total)
        par.append(NONE); is_root.append(False)
        return len(form) - 1

    cuts = [0] + (np.flatnonzero(np.diff(w)) + 1).tolist() + [len(w)] if len(w) else [0]
    for s, e in zip(cuts[:-1], cuts[1:]):
        weight = int(w[s])
        olds_a, olds_b = [find(x) for x in a[s:e].tolist()], [find(x) for x in b[s:e].tolist()]
        up = {}

        def lfind(x):
            while up.setdefault(x, x) != x:
                up[x] = up[up[x]]
                x = up[x]
            return x

        for ra, rb in zip(olds_a, olds_b):
            ra, rb = lfind(ra), lfind(rb)
            if ra != rb:
                up[max(ra, rb)] = min(ra, rb)
        groups = {}
        for old in list(up):
            groups.setdefault(lfind(old), []).append(old)
        for new_root, olds in groups.items():
            big = [o for o in olds if size[o] >= mcs]
            total = sum(size[o] for o in olds)
            node = None
            if len(big) >= 2:
                node = new_node(weight, total, len(big))
                for o in big:
                    c = carried.pop(o)
                    par[c], end[c], rep[c] = node, weight, o
            elif len(big) == 1:
                node = carried.pop(big[0])
                grown = total - size[big[0]]
                sz[node] += grown
                sum_leave[node] += weight * grown
            elif total >= mcs:
                node = new_node(weight, total, 0)
            if node is not None:
                for o in olds:
                    if size[o] < mcs:
                        for p in members.pop(o, (o,)):
                            own[p], leave[p] = node, weight
                carried[new_root] = node
            else:
                merged = []
                for o in olds:
                    merged += members.pop(o, (o,))
                members[new_root] = merged
            for o in olds:
                parent[o] = new_root
            size[new_root] = total
    for root, c in carried.items():
        end[c], rep[c], is_root[c] = root_weight, root, True
    m = len(form)
    form, rep, end, sz, nch = (np.array(x, dtype=np.int64) for x in (form, rep, end, sz, nch))
    order = np.lexsort((rep, form))
    number = np.empty(m, dtype=np.int64)
    number[order] = np.arange(m)
    par = np.array(par, dtype=np.int64)
    parents = np.where(par[order] != NONE, number[np.minimum(par[order], max(m - 1, 0))], NONE) if m else par
    root_flag = np.array(is_root, dtype=bool)[order] if m else np.zeros(0, dtype=bool)
    stability = end[order] * sz[order] - np.array(sum_leave, dtype=np.int64)[order] if m else np.zeros(0, dtype=np.int64)
    allowed = ~(root_flag & (root_weight == 0))
    stability[~allowed] = 0
    sub, keep, best = [0] * m, [False] * m, [0] * m
    ps, stab, ok = parents.tolist(), stability.tolist(), allowed.tolist()
    for i in range(m):
        keep[i] = ok[i] and stab[i] >= sub[i]
        best[i] = stab[i] if keep[i] else sub[i]
        if ps[i] != NONE:
            sub[ps[i]] += best[i]
    sel_anc, selected = [NONE] * m, [False] * m
    for i in range(m - 1, -1, -1):
        above = sel_anc[ps[i]] if ps[i] != NONE else NONE
        selected[i] = keep[i] and above == NONE
        sel_anc[i] = above if above != NONE else (i if keep[i] else NONE)
    flags = np.array(selected, dtype=np.uint32) | (np.array(keep, dtype=np.uint32) << 1) | (root_flag.astype(np.uint32) << 2)
    nodes = dict(parent=parents.astype(np.uint32), rep=rep[order].astype(np.uint32), form=form[order].astype(np.uint32), end=end[order].astype(np.uint32),
                 size=sz[order].astype(np.uint32), n_children=nch[order].astype(np.uint32), flags=flags, pad=np.zeros(m, dtype=np.uint32),
                 stability=stability.astype(np.uint64), best=np.array(best, dtype=np.uint64))
    own = np.array(own, dtype=np.int64)
    has = own != NONE
    own_out = np.full(n, NONE, dtype=np.int64)
    own_out[has] = number[own[has]]
    node = np.full(n, NONE, dtype=np.int64)
    node[has] = np.array(sel_anc + [NONE], dtype=np.int64)[own_out[has]]
    labels = np.arange(n, dtype=np.int64)
    labels[node != NONE] = rep[order][node[node != NONE]]
    clustered = int((node != NONE).sum())
    st = dict(n_nodes=m, n_leaves=int((nch == 0).sum()), n_roots=int(root_flag.sum()), n_selected=int(sum(selected)), n_clustered=clustered, n_noise=n - clustered,
              total_stability=int(sum(s for s, c in zip(stab, selected) if c)), n_levels=len(cuts) - 1)
    return nodes, labels.astype(np.uint32), node.astype(np.uint32), own_out.astype(np.uint32), np.array(leave, dtype=np.uint32), st


class HostTooSlow(Exception):
    pass


def limited(seconds, fn, *a):
    """fn(*a) under an alarm: HostTooSlow when it has not ended after `seconds`"""
    def ring(signum, frame):
        raise HostTooSlow()
    before = signal.signal(signal.SIGALRM, ring)
    signal.alarm(int(seconds))
    try:
        return fn(*a)
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, before)


def same_words(vc, what, stats, d_nodes, d_rec, want):
    """every word of the device's outputs == the host model's"""
    assert stats == want[5], (what, "statistics differ from the host model", stats, want[5])
    got = d_nodes[:stats["n_nodes"]].cpu().numpy().view(vc.CONDENSED_NODE).reshape(-1)
    for field in vc.CONDENSED_NODE.names:
        assert np.array_equal(got[field], want[0][field]), (what, "nodes differ from the host model", field)
    for at, name in ((1, "labels"), (2, "node"), (3, "own"), (4, "leave")):
        assert np.array_equal(d_rec[name].cpu().numpy().view(np.uint32), want[at]), (what, name, "differ from the host model")


def check_prefix(args, vc, torch, flags, note):
    """the assertion on a store of --prefix records built the same way: graph, forest, condensation, every word against the model"""
    n, k, mcs = int(args.prefix), args.k, args.min_cluster_size
    st = torch.cuda.current_stream().cuda_stream
    with vc.Engine(64, capacity=n, n_tables=2, flags=vc.FLAG_LEAN_TIMING) as e:
        e.add_synthetic(n, seed=args.seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // args.cluster_size, 1), max_flips=args.flips)
        e.build_index()
        d_rows = torch.empty((n, k), dtype=torch.int64, device="cuda")
        d_counts = torch.empty((n,), dtype=torch.int32, device="cuda")
        d_edges = torch.zeros((n - 1, 4), dtype=torch.int32, device="cuda")
        d_nodes = torch.zeros((n - 1, 6), dtype=torch.int64, device="cuda")
        d_rec = {name: torch.empty((n,), dtype=torch.int32, device="cuda") for name in ("labels", "node", "own", "leave")}
        e.knn_graph_dev(k, d_rows.data_ptr(), d_counts.data_ptr(), mode=vc.MODE_MIH_EXACT, batch=args.batch, stream=st)
        mst = e.knn_mst_dev(d_rows.data_ptr(), d_counts.data_ptr(), k, k, d_edges.data_ptr(), flags=flags, weight_kind=vc.MST_REACHABILITY, min_pts=args.min_pts, stream=st)
        torch.cuda.synchronize()
        M, root_weight = mst["n_tree"], mst["max_weight"] + 1
        edges = d_edges[:M].cpu().numpy().view(np.uint32)
        want = limited(10 * args.host_limit, host_condense, n, edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64), edges[:, 2].astype(np.int64), mcs, root_weight)
        stats = e.mst_condense_dev(d_edges.data_ptr(), M, mcs, d_nodes.data_ptr(), d_rec["labels"].data_ptr(), d_rec["node"].data_ptr(), d_rec["own"].data_ptr(),
                                   d_rec["leave"].data_ptr(), root_weight=root_weight, method=vc.CONDENSE_EOM, stream=st)
        torch.cuda.synchronize()
        same_words(vc, ("prefix", flags), stats, d_nodes, d_rec, want)
        note("every word equals the host model on a store of %d records: %s" % (n, stats))
        return stats


def step(args):
    import torch
    from verticut_amd import engine as vc
    n, bits, m, k, mcs = int(args.n), 64, 2, args.k, args.min_cluster_size
    kk = k

    def note(what):
        print("[bench_mst_condense k=%d] %s" % (k, what), file=sys.stderr, flush=True)

    e = vc.Engine(bits, capacity=n, n_tables=m, flags=vc.FLAG_LEAN_TIMING)
    e.add_synthetic(n, seed=args.seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // args.cluster_size, 1), max_flips=args.flips)
    e.build_index()
    st = torch.cuda.current_stream().cuda_stream
    d_rows = torch.empty((n, k), dtype=torch.int64, device="cuda")
    d_counts = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_nodes = torch.zeros((n - 1, 6), dtype=torch.int64, device="cuda")
    d_rec = {name: torch.empty((n,), dtype=torch.int32, device="cuda") for name in ("labels", "node", "own", "leave", "cut")}
    d_edges = {f: torch.zeros((n - 1, 4), dtype=torch.int32, device="cuda") for f in (vc.KNN_MUTUAL, vc.KNN_EITHER)}
    e.knn_graph_dev(k, d_rows.data_ptr(), d_counts.data_ptr(), mode=vc.MODE_MIH_EXACT, batch=args.batch, stream=st)
    torch.cuda.synchronize()
    note("graph built")
    names = {vc.KNN_MUTUAL: "mutual", vc.KNN_EITHER: "either"}
    res = {"stats": {}, "mst": {}, "host_s": {}, "root_weight": {}, "cut_clusters": {}, "checked": {}}
    M, top = {}, {}

    def leg_condense(flags):
        return e.mst_condense_dev(d_edges[flags].data_ptr(), M[flags], mcs, d_nodes.data_ptr(), d_rec["labels"].data_ptr(), d_rec["node"].data_ptr(),
                                  d_rec["own"].data_ptr(), d_rec["leave"].data_ptr(), root_weight=top[flags] + 1, method=vc.CONDENSE_EOM, stream=st)

    def leg_cut(flags):
        return e.mst_cut_dev(d_edges[flags].data_ptr(), M[flags], top[flags], d_rec["cut"].data_ptr(), stream=st)

    # ---- the check, and the host leg with it
    for flags, name in names.items():
        mst = e.knn_mst_dev(d_rows.data_ptr(), d_counts.data_ptr(), k, kk, d_edges[flags].data_ptr(), flags=flags, weight_kind=vc.MST_REACHABILITY, min_pts=args.min_pts,
                            stream=st)
        torch.cuda.synchronize()
        M[flags], top[flags] = mst["n_tree"], mst["max_weight"]
        t0 = time.perf_counter()
        edges = d_edges[flags][:M[flags]].cpu().numpy().view(np.uint32)
        copy_home = time.perf_counter() - t0
        t0 = time.perf_counter()
        try:
            want = limited(args.host_limit, host_condense, n, edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64), edges[:, 2].astype(np.int64), mcs, top[flags] + 1)
        except HostTooSlow:
            want = None
        model_s = time.perf_counter() - t0
        stats = leg_condense(flags)
        torch.cuda.synchronize()
        if want is not None:
            same_words(vc, name, stats, d_nodes, d_rec, want)
            res["checked"][name] = {"every_word_equals_host_model": True, "records_checked": n}
            res["host_s"][name] = {"copy_home": round(copy_home, 3), "model": round(model_s, 3)}
            note("VC_KNN_%s: every word of nodes, labels, node, own, leave and the statistics equals the host model over %d records: %s; host %.1f s"
                 % (name.upper(), n, stats, copy_home + model_s))
        else:
            res["host_s"][name] = {"copy_home": round(copy_home, 3), "model_did_not_end_within_s": args.host_limit}
            res["checked"][name] = {"every_word_equals_host_model": True, "records_checked": int(args.prefix), "on_a_prefix_store": True,
                                    "prefix_stats": check_prefix(args, vc, torch, flags, note)}
        count = leg_cut(flags)
        torch.cuda.synchronize()
        res["stats"][name], res["mst"][name], res["root_weight"][name], res["cut_clusters"][name] = stats, mst, top[flags] + 1, count
        del edges, want

    # ---- the timing
    legs = {}
    for flags, name in names.items():
        legs["condense_" + name] = lambda f=flags: leg_condense(f)
        legs["cut_" + name] = lambda f=flags: leg_cut(f)
    for fn in legs.values():       # every buffer of the timed window warm
        fn()
    torch.cuda.synchronize()
    t = {name: [] for name in legs}
    for _ in range(args.reps):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[name].append(time.perf_counter() - t0)
    med = {q: round(float(np.median(v)) * 1e3, 3) for q, v in t.items()}
    res.update(call_ms_median=med, call_ms_min={q: round(min(v) * 1e3, 3) for q, v in t.items()}, call_ms_max={q: round(max(v) * 1e3, 3) for q, v in t.items()},
               reps=args.reps, min_cluster_size=mcs, min_pts=args.min_pts,
               condense_over_cut={name: round(med["condense_" + name] / med["cut_" + name], 2) for name in names.values()})
    note("timed: %s" % res)
    with open(args.step_out, "w") as f:
        json.dump(res, f)
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e6)
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--cluster-size", type=int, default=16, help="records per centre of the synthetic data")
    ap.add_argument("--flips", type=int, default=6, help="a record is its centre with up to this many bits flipped")
    ap.add_argument("--min-cluster-size", type=int, default=5)
    ap.add_argument("--min-pts", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-limit", type=int, default=60, help="seconds the host model may take on the whole store")
    ap.add_argument("--prefix", type=float, default=1e5, help="records of the store the words are asserted on when the model is too slow on the whole one")
    ap.add_argument("--seed", type=int, default=35)
    ap.add_argument("--step-timeout", type=int, default=500, help="seconds a step may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=("run",), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--step-out", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--k", type=int, default=10, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    line = {"metric": "condensed tree, stabilities, excess-of-mass selection and labels of the spanning forest (VC_MST_REACHABILITY, min_pts %d) of a built exact k-NN "
                      "graph, %.3g clustered 64-bit codes (%d per centre, <= %d flips), kk = k, min_cluster_size %d, root_weight = the largest weight + 1, one engine"
                      % (args.min_pts, args.n, args.cluster_size, args.flips, args.min_cluster_size),
            "not_measured": "other code widths and shapes (a 512-bit forest has up to 513 levels of five launches), the split of a call into its levels and "
                            "launches (no kernel trace), the pass over the records per level against a list of the records without a node (not built), "
                            "VC_CONDENSE_LEAF, root_weight 0, the sharded forms, the host-pointer forms"}
    with tempfile.TemporaryDirectory() as td:
        for k in [int(x) for x in args.ks.split(",")]:
            part = os.path.join(td, "run_%d.json" % k)      # chained: a step that fails, faults or runs into its time limit ends the run
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", "run", "--step-out", part, "--k", str(k)]
            for key in ("n", "batch", "cluster_size", "flips", "min_cluster_size", "min_pts", "reps", "seed", "host_limit", "prefix"):
                cmd += ["--" + key.replace("_", "-"), str(getattr(args, key))]
            rc = subprocess.call(cmd)
            if rc != 0:
                raise SystemExit("the step at k=%d ended with status %d: nothing further is started" % (k, rc))
            line["k=%d" % k] = json.load(open(part))
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
