"""The minimum spanning forest of a built k-NN graph (vc_knn_mst_dev) against its floor and the path it replaces: clustered synthetic
64-bit codes (the store of bench_knn_graph.py: 1e6 records, 16 per centre, up to 6 flipped bits), m = 2, the graph built once per k by
vc_knn_graph_dev in exact MIH, one engine, k = kk = 10 and k = kk = 100, no cap, VC_MST_DISTANCE, both flags.

  mst_mutual / mst_either     vc_knn_mst_dev with edges, labels and histogram, buffers warm
  cluster_mutual / _either    vc_cluster_knn_dev on the same graph, flags and handle: ONE pass over the N kk entries, the floor any reader
                              of the graph pays; the forest costs about one such pass per round over a shrinking list
  cut_mutual / cut_either     vc_mst_cut_dev on the forest at the median weight of its edges
  host                        the replaced path, once per flag: the rows copied home, then the forest on the host.  NOT a Python Kruskal
                              loop, which would take minutes here: a vectorised numpy Boruvka under the same strict order.  The order is
                              strict, so the forest is unique and Kruskal keeps exactly these edges; the host figure is therefore a LOWER
                              bound of what a host Kruskal in Python would take, and says so in the JSON.

Per k one child process under its own `timeout`, the next only after the one before succeeded.  In it, before anything is timed, for
both flags: EVERY word of the device's edges, labels and histogram == the host model's (asserted; the whole store, which covers any
sample of components), the statistics and totals == the model's, the labels == vc_cluster_knn_dev's, and vc_mst_cut_dev at the timed
height == the host's cut of the model's edges.  The host model also gives the live-list length at the start of every round; the
device's rounds are reported beside the model's.  Then the device legs interleaved, a host clock around each ending in a device
synchronise, medians of --reps with min .. max.  No ratio is fixed in advance.  Prints one JSON line; --out also writes it to a file.

    python tools/bench_knn_mst.py [--n 1e6] [--ks 10,100] [--reps 7] [--out profiles/knn_mst_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOW = np.uint64(0xFFFFFFFF)
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
S32 = np.uint64(32)


def _merge(comp, u, v):
    """comp (the smallest id of every record's component) after the components u[t] and v[t] are joined, by label propagation with
    pointer jumping over the component ids"""
    lab = np.arange(len(comp), dtype=np.int64)
    while True:
        m = np.minimum(lab[u], lab[v])
        new = lab.copy()
        np.minimum.at(new, u, m)
        np.minimum.at(new, v, m)
        new = new[new]
        if np.array_equal(new, lab):
            return lab[comp]
        lab = new


def host_forest(rows, kk, either):
    """the contract on the host for full rows, VC_MST_DISTANCE, no cap: (keys of the forest edges ascending, labels, the listed entries,
    the graph's edges, rounds that hooked, live-list length at the start of every round)"""
    n, k = rows.shape
    sub = rows[:, :kk]
    j = (sub & LOW).astype(np.int64)
    d = sub >> S32
    i = np.repeat(np.arange(n, dtype=np.int64), kk).reshape(n, kk)
    back = ((d << S32) | i.astype(np.uint64)) <= rows[:, kk - 1][j]           # j lists i: the one compare
    below = i < j
    home = (below | ~back) if either else (back & below)                     # THE HOME RULE
    key = ((d << S32) | (i * kk + np.arange(kk, dtype=np.int64)[None, :]).astype(np.uint64))[home]
    a, b = i[home], j[home]
    n_graph = int(home.sum())
    del sub, j, d, i, back, below, home
    flat = rows.reshape(-1)
    comp = np.arange(n, dtype=np.int64)
    picked, live_counts, rounds = [], [], 0
    while True:
        ca, cb = comp[a], comp[b]
        alive = ca != cb
        key, a, b, ca, cb = key[alive], a[alive], b[alive], ca[alive], cb[alive]
        live_counts.append(int(len(key)))
        if len(key) == 0:
            break
        best = np.full(n, NONE, dtype=np.uint64)
        np.minimum.at(best, ca, key)
        np.minimum.at(best, cb, key)
        picks = np.unique(best[best != NONE])
        picked.append(picks)
        rounds += 1
        idx = (picks & LOW).astype(np.int64)
        pa = idx // kk
        pb = (flat[pa * k + idx % kk] & LOW).astype(np.int64)
        comp = _merge(comp, comp[pa], comp[pb])
    keys = np.sort(np.concatenate(picked)) if picked else np.zeros(0, dtype=np.uint64)
    return keys, comp.astype(np.uint32), n * kk, n_graph, rounds, live_counts


def keys_to_edges(keys, rows, kk):
    """[M, 4] uint32 (a, b, weight, dist) of the forest edges with these keys"""
    k = rows.shape[1]
    idx = (keys & LOW).astype(np.int64)
    a = idx // kk
    v = rows.reshape(-1)[a * k + idx % kk]
    return np.stack([a.astype(np.uint32), (v & LOW).astype(np.uint32), (keys >> S32).astype(np.uint32), (v >> S32).astype(np.uint32)], axis=1)


def step(args):
    import torch
    from verticut_amd import engine as vc
    n, bits, m, k = int(args.n), 64, 2, args.k
    kk = k

    def note(what):
        print("[bench_knn_mst k=%d] %s" % (k, what), file=sys.stderr, flush=True)

    e = vc.Engine(bits, capacity=n, n_tables=m, flags=vc.FLAG_LEAN_TIMING)
    e.add_synthetic(n, seed=args.seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // args.cluster_size, 1), max_flips=args.flips)
    e.build_index()
    st = torch.cuda.current_stream().cuda_stream
    d_rows = torch.empty((n, k), dtype=torch.int64, device="cuda")
    d_counts = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_labels = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_cl = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_cut = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_hist = torch.empty((bits + 1,), dtype=torch.int64, device="cuda")
    d_edges = {f: torch.zeros((n - 1, 4), dtype=torch.int32, device="cuda") for f in (vc.KNN_MUTUAL, vc.KNN_EITHER)}
    e.knn_graph_dev(k, d_rows.data_ptr(), d_counts.data_ptr(), mode=vc.MODE_MIH_EXACT, batch=args.batch, stream=st)
    torch.cuda.synchronize()
    note("graph built")
    assert np.all(d_counts.cpu().numpy().view(np.uint32) == min(k, n - 1)) and n > k

    def leg_mst(flags):
        return e.knn_mst_dev(d_rows.data_ptr(), d_counts.data_ptr(), k, kk, d_edges[flags].data_ptr(), d_labels.data_ptr(), d_hist.data_ptr(), flags=flags, stream=st)

    def leg_cluster(flags):
        return e.cluster_knn_dev(d_rows.data_ptr(), d_counts.data_ptr(), k, kk, d_cl.data_ptr(), None, flags=flags, stream=st)

    # ---- the check, and the host leg with it
    t0 = time.perf_counter()
    rows = d_rows.cpu().numpy().view(np.uint64)
    copy_home = time.perf_counter() - t0
    names = {vc.KNN_MUTUAL: "mutual", vc.KNN_EITHER: "either"}
    res = {"stats": {}, "model": {}, "host_s": {"copy_home": round(copy_home, 3)}, "cut_height": {}, "cut_clusters": {}}
    M = {}
    for flags, name in names.items():
        t0 = time.perf_counter()
        keys, labels, n_listed, n_graph, rounds, live = host_forest(rows, kk, flags == vc.KNN_EITHER)
        res["host_s"]["forest_" + name] = round(time.perf_counter() - t0, 3)
        want = keys_to_edges(keys, rows, kk)
        stats = leg_mst(flags)
        torch.cuda.synchronize()
        M[flags] = len(want)
        got = d_edges[flags][:M[flags]].cpu().numpy().view(np.uint32)
        assert stats["n_tree"] == M[flags] and np.array_equal(got, want), (name, "edges differ from the host model", stats, M[flags])
        assert np.array_equal(d_labels.cpu().numpy().view(np.uint32), labels), (name, "labels differ from the host model")
        hist = np.bincount(want[:, 2], minlength=bits + 1).astype(np.uint64)
        assert np.array_equal(d_hist.cpu().numpy().view(np.uint64), hist), (name, "histogram differs from the host model")
        assert (stats["n_edges"], stats["n_graph_edges"], stats["n_clusters"], stats["total_weight"], stats["max_weight"]) == \
            (n_listed, n_graph, n - M[flags], int(want[:, 2].astype(np.int64).sum()), int(want[:, 2].max()) if M[flags] else 0), (name, stats)
        cl = leg_cluster(flags)
        torch.cuda.synchronize()
        assert np.array_equal(d_cl.cpu().numpy().view(np.uint32), labels) and cl["n_clusters"] == stats["n_clusters"] and cl["n_edges"] == stats["n_edges"], name
        height = int(np.median(want[:, 2])) if M[flags] else 0
        count = e.mst_cut_dev(d_edges[flags].data_ptr(), M[flags], height, d_cut.data_ptr(), stream=st)
        torch.cuda.synchronize()
        below = want[want[:, 2] <= height]
        cut = _merge(np.arange(n, dtype=np.int64), below[:, 0].astype(np.int64), below[:, 1].astype(np.int64)).astype(np.uint32)
        assert np.array_equal(d_cut.cpu().numpy().view(np.uint32), cut) and count == n - len(below) == n - int(hist[:height + 1].sum()), (name, "cut", height)
        res["stats"][name], res["cut_height"][name], res["cut_clusters"][name] = stats, height, count
        res["model"][name] = {"rounds": rounds, "live_at_round_start": live, "weight_hist_nonzero": {int(w): int(c) for w, c in enumerate(hist) if c}}
        note("VC_KNN_%s: every word of edges, labels, histogram equals the host model; labels equal vc_cluster_knn_dev's; the cut at %d equals the host's: %s, "
             "model rounds %d, live %s" % (name.upper(), height, stats, rounds, live))
    del rows

    # ---- the timing
    legs = {}
    for flags, name in names.items():
        legs["mst_" + name] = lambda f=flags: leg_mst(f)
        legs["cluster_" + name] = lambda f=flags: leg_cluster(f)
        legs["cut_" + name] = lambda f=flags, nm=name: e.mst_cut_dev(d_edges[f].data_ptr(), M[f], res["cut_height"][nm], d_cut.data_ptr(), stream=st)
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
    res.update(checked={"every_word_of_edges_labels_hist_equals_host_model": True, "labels_equal_cluster_knn_dev": True, "cut_equals_host": True, "records_checked": n},
               call_ms_median=med, call_ms_min={q: round(min(v) * 1e3, 3) for q, v in t.items()}, call_ms_max={q: round(max(v) * 1e3, 3) for q, v in t.items()},
               reps=args.reps, items=n * kk,
               mst_over_cluster_knn={name: round(med["mst_" + name] / med["cluster_" + name], 2) for name in names.values()},
               host_over_mst={name: round((res["host_s"]["copy_home"] + res["host_s"]["forest_" + name]) * 1e3 / med["mst_" + name], 1) for name in names.values()},
               host_note="the host forest is a vectorised numpy Boruvka, not a Python Kruskal loop: a lower bound of the replaced path")
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=35)
    ap.add_argument("--step-timeout", type=int, default=500, help="seconds a step may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=("run",), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--step-out", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--k", type=int, default=10, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    line = {"metric": "minimum spanning forest in Kruskal order of a built exact k-NN graph, %.3g clustered 64-bit codes (%d per centre, <= %d flips), "
                      "kk = k, no cap, VC_MST_DISTANCE, one engine" % (args.n, args.cluster_size, args.flips),
            "not_measured": "other code widths and shapes, VC_MST_REACHABILITY, a cap, the sharded forms, the host-pointer forms, compaction of the live list "
                            "every round against every second round (only every round exists), grouped read-backs (one per round exists), the split of a "
                            "call into its launches (no kernel trace), a host Kruskal written as a Python loop"}
    with tempfile.TemporaryDirectory() as td:
        for k in [int(x) for x in args.ks.split(",")]:
            part = os.path.join(td, "run_%d.json" % k)      # chained: a step that fails, faults or runs into its time limit ends the run
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", "run", "--step-out", part, "--k", str(k)]
            for key in ("n", "batch", "cluster_size", "flips", "reps", "seed"):
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
