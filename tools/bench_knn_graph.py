"""The exact k-NN graph of the store (vc_knn_graph_dev) and its components (vc_cluster_knn_dev) against the path they replace: clustered
synthetic 64-bit codes (the store of the other tools: 1e6 records, 16 per centre, up to 6 flipped bits), m = 2, exact MIH, batches of
4 096 ids, one engine, k = 10 and k = 100.

  graph        vc_knn_graph_dev from scratch in VC_MODE_MIH_EXACT: per batch fill ids, gather, rounds of search + settle, one wait per
               round; the N x k settled rows stay in HBM.  k_first = 0: the first round asks for 2 (k + 1)
  graph_k_first_k2   the same with k_first = k + 2, the smallest k' at which a full exact-MIH row can be settled (at k + 1 the last entry
               itself lies at the last distance, so at most k - 1 others lie below it): a cheap first round, more queries go on
  loop         the walk in the same batch size through vc_search_knn_ids_dev(VC_IDS_EXCLUDE_SELF) at k -- the device loop alone; its
               rows are NOT settled (ties at the last distance are any members), so it is a lower bound of the replaced path
  loop_home    that loop with every batch's rows copied home
  cluster_knn  vc_cluster_knn_dev at kk = k, VC_KNN_MUTUAL, no cap, on the built graph: it moves N x k x 8 bytes, GB/s against that

Per k two steps, each a child process under its own `timeout`, the next only after the one before succeeded:
  check   rows and counts of `graph` == a VC_MODE_LINEAR build (asserted); labels and in-degrees of `cluster_knn` == a numpy model over
          the rows (asserted); n_searched / N, n_linear, k_last reported
  time    the five legs interleaved, a host clock around each leg ending in a device synchronise, medians of --reps with min .. max
No ratio is fixed in advance.  Prints one JSON line; --out also writes it to a file.

    python tools/bench_knn_graph.py [--n 1e6] [--ks 10,100] [--reps 7] [--out profiles/knn_graph_bench.json]
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
from tools.bench_cluster import host_union_find  # noqa: E402

LOW = np.uint64(0xFFFFFFFF)


def host_model(rows):
    """(labels, in_degree, n_mutual) of the full graph at kk = k, VC_KNN_MUTUAL, no cap: edges as sorted keys, no one-compare trick"""
    n, k = rows.shape
    src = np.repeat(np.arange(n, dtype=np.uint64), k)
    dst = rows.reshape(-1) & LOW
    deg = np.bincount(dst.astype(np.int64), minlength=n).astype(np.uint32)
    keys = np.sort((src << np.uint64(32)) | dst)
    back = (dst << np.uint64(32)) | src
    pos = np.searchsorted(keys, back)
    mutual = keys[np.minimum(pos, len(keys) - 1)] == back
    a, b = src[mutual].astype(np.int64), dst[mutual].astype(np.int64)
    once = a < b
    return host_union_find(n, a[once], b[once]), deg, int(once.sum())


def step(args):
    import torch
    from verticut_amd import engine as vc
    n, bits, m, B, k = int(args.n), 64, 2, args.batch, args.k

    def note(what):
        print("[bench_knn_graph k=%d] %s" % (k, what), file=sys.stderr, flush=True)

    e = vc.Engine(bits, capacity=n, n_tables=m, flags=vc.FLAG_LEAN_TIMING)
    e.add_synthetic(n, seed=args.seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // args.cluster_size, 1), max_flips=args.flips)
    e.build_index()
    note("engine built")
    st = torch.cuda.current_stream().cuda_stream
    d_rows = torch.empty((n, k), dtype=torch.int64, device="cuda")
    d_counts = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_labels = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_deg = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_ids = torch.arange(n, dtype=torch.int32, device="cuda")       # (n < 2^31 here)
    d_loop = torch.empty((B, k), dtype=torch.int64, device="cuda")
    starts = list(range(0, n, B))

    def leg_graph(mode=vc.MODE_MIH_EXACT, k_first=0):
        return e.knn_graph_dev(k, d_rows.data_ptr(), d_counts.data_ptr(), mode=mode, batch=B, k_first=k_first, stream=st)

    def leg_loop(home=False):
        for lo in starts:
            nq = min(B, n - lo)
            e.search_knn_ids_dev(d_ids[lo:].data_ptr(), nq, k, d_loop.data_ptr(), mode=vc.MODE_MIH_EXACT, id_flags=vc.IDS_EXCLUDE_SELF, stream=st)
            if home:
                d_loop[:nq].cpu()

    def leg_cluster():
        return e.cluster_knn_dev(d_rows.data_ptr(), d_counts.data_ptr(), k, k, d_labels.data_ptr(), d_deg.data_ptr(), stream=st)

    if args.step == "check":
        stats = leg_graph()
        torch.cuda.synchronize()
        rows, counts = d_rows.cpu().numpy().view(np.uint64), d_counts.cpu().numpy().view(np.uint32)
        tight = leg_graph(k_first=k + 2)
        torch.cuda.synchronize()
        assert np.array_equal(rows, d_rows.cpu().numpy().view(np.uint64)), "the rows at k_first = k + 2 differ from those at the default"
        lin = leg_graph(vc.MODE_LINEAR)
        torch.cuda.synchronize()
        assert np.array_equal(rows, d_rows.cpu().numpy().view(np.uint64)), "the exact-MIH rows differ from the LINEAR build"
        assert np.array_equal(counts, d_counts.cpu().numpy().view(np.uint32)) and np.all(counts == min(k, n - 1))
        assert np.all(rows[:, 1:] > rows[:, :-1]) and not np.any((rows & LOW) == np.arange(n, dtype=np.uint64)[:, None])
        note("rows equal the LINEAR build: %s" % stats)
        cst = leg_cluster()      # (on the LINEAR build's rows: the same words)
        torch.cuda.synchronize()
        labels, deg, n_mutual = host_model(rows)
        assert np.array_equal(d_labels.cpu().numpy().view(np.uint32).astype(np.int64), labels), "labels differ from the host model"
        assert np.array_equal(d_deg.cpu().numpy().view(np.uint32), deg), "in-degrees differ from the host model"
        assert cst["n_edges"] == n * min(k, n - 1) and cst["n_mutual"] == n_mutual and cst["n_clusters"] == len(np.unique(labels)) and cst["max_in_degree"] == int(deg.max())
        res = {"rows_equal_linear_build": True, "labels_and_in_degrees_equal_host_model": True, "graph_stats": stats, "graph_k_first_k2_stats": tight,
               "linear_stats": lin, "searched_per_record": round(stats["n_searched"] / n, 4),
               "searched_per_record_k_first_k2": round(tight["n_searched"] / n, 4), "cluster_knn_stats": cst}
        note("labels and in-degrees equal the host model: %s" % cst)
    else:
        legs = {"graph": leg_graph, "graph_k_first_k2": lambda: leg_graph(k_first=k + 2), "loop": leg_loop, "loop_home": lambda: leg_loop(True), "cluster_knn": leg_cluster}
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
        res = {"call_ms_median": {q: round(float(np.median(v)) * 1e3, 3) for q, v in t.items()},
               "call_ms_min": {q: round(min(v) * 1e3, 3) for q, v in t.items()},
               "call_ms_max": {q: round(max(v) * 1e3, 3) for q, v in t.items()}, "reps": args.reps, "batches": len(starts)}
        med = res["call_ms_median"]
        res["graph_over_loop"] = round(med["graph"] / med["loop"], 3)
        res["graph_over_loop_home"] = round(med["graph"] / med["loop_home"], 3)
        res["graph_k_first_k2_over_loop"] = round(med["graph_k_first_k2"] / med["loop"], 3)
        res["cluster_knn_GBps_of_rows"] = round(n * k * 8 / (med["cluster_knn"] * 1e-3) / 1e9, 2)
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
    ap.add_argument("--step-timeout", type=int, default=400, help="seconds a step may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=("check", "time"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--step-out", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--k", type=int, default=10, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    line = {"metric": "exact k-NN graph and its mutual components, %.3g clustered 64-bit codes (%d per centre, <= %d flips), m=2, exact MIH, "
                      "batches of %d ids, one engine" % (args.n, args.cluster_size, args.flips, args.batch)}
    with tempfile.TemporaryDirectory() as td:
        for k in [int(x) for x in args.ks.split(",")]:
            line["k=%d" % k] = {}
            for name in ("check", "time"):      # chained: a step that fails, faults or runs into its time limit ends the run
                part = os.path.join(td, "%s_%d.json" % (name, k))
                cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--step-out", part, "--k", str(k)]
                for key in ("n", "batch", "cluster_size", "flips", "reps", "seed"):
                    cmd += ["--" + key.replace("_", "-"), str(getattr(args, key))]
                rc = subprocess.call(cmd)
                if rc != 0:
                    raise SystemExit("step %s at k=%d ended with status %d: nothing further is started" % (name, k, rc))
                line["k=%d" % k][name] = json.load(open(part))
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
