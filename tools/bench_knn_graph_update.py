"""A built k-NN graph brought up to date after an append (vc_update_index + vc_knn_graph_update_dev) against the path it replaces, the
build over the whole store (vc_knn_graph_dev): the store of tools/bench_knn_graph.py -- 1e6 clustered 64-bit codes (16 per centre, up
to 6 flipped bits), m = 2, exact MIH, batches of 4 096 ids, one engine -- with appends of 1e3, 1e4 and 1e5 records of the same
distribution (the generator's next records), k = 10 and k = 100.

Per k one child process under its own `timeout`, the next only after the one before succeeded.  The child builds the graph of the
first n records once and keeps a copy in HBM.  Per append size and repetition, on the same handle:
  1. the old rows and counts are copied into the front of the N x k buffer and the records are appended            (not timed)
  2. update   vc_update_index, then vc_knn_graph_update_dev in VC_MODE_MIH_EXACT                                    (timed, both parts)
  3. rebuild  vc_knn_graph_dev over the whole store into a second buffer                                            (timed)
  4. vc_retain_dev takes the appended records away again: the store and its index are as before step 1             (not timed)
A host clock around each leg ending in a device synchronise; the first repetition is the warm-up, in which rows and counts of the two
buffers are asserted equal; medians of --reps with min .. max.  THE ONE CONDITION (asserted): at 1e4 appended records the update's
median lies below the rebuild's median of the same run.  Nothing else is fixed in advance.

--trace-csv merges the kernel times of a `rocprofv3 --kernel-trace --stats --output-format csv` run of the update alone (a run of its
own: `rocprofv3 ... -- python tools/bench_knn_graph_update.py --step trace --k 10 --appends 10000 --step-out X`) into --out: the join,
merge, copy and scan launches, and the count pass's pair-words/s -- nb x nw x W over a launch -- next to the rate
profiles/kmajority_bench.json records for vc_assign_kernel, whose data flow it has.

Not measured: other widths, the sharded forms, the host form, VC_MODE_LINEAR, other knobs than the defaults.

    python tools/bench_knn_graph_update.py [--n 1e6] [--ks 10,100] [--appends 1000,10000,100000] [--reps 7] [--out profiles/knn_graph_update_bench.json]
"""
import argparse
import csv
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OLD_BATCH, WINDOW = 1 << 18, 1024          # the defaults of vc_knn_graph_update_plan.hpp, which the runs use


def step(args):
    import torch
    from verticut_amd import engine as vc
    n, bits, m, B, k = int(args.n), 64, 2, args.batch, args.k
    appends = [int(float(x)) for x in args.appends.split(",")]
    cap = n + max(appends)

    def note(what):
        print("[bench_knn_graph_update k=%d] %s" % (k, what), file=sys.stderr, flush=True)

    def synth(count):
        e.add_synthetic(count, seed=args.seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // args.cluster_size, 1), max_flips=args.flips)

    e = vc.Engine(bits, capacity=cap, n_tables=m, flags=vc.FLAG_LEAN_TIMING)
    synth(n)
    e.build_index()
    st = torch.cuda.current_stream().cuda_stream
    d_old = torch.empty((n, k), dtype=torch.int64, device="cuda")
    d_old_counts = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_rows = torch.empty((cap, k), dtype=torch.int64, device="cuda")
    d_counts = torch.empty((cap,), dtype=torch.int32, device="cuda")
    d_rows2 = torch.empty((cap, k), dtype=torch.int64, device="cuda")
    d_counts2 = torch.empty((cap,), dtype=torch.int32, device="cuda")
    d_keep = torch.zeros((cap,), dtype=torch.int32, device="cuda")
    d_keep[:n] = 1
    e.knn_graph_dev(k, d_old.data_ptr(), d_old_counts.data_ptr(), mode=vc.MODE_MIH_EXACT, batch=B, stream=st)
    torch.cuda.synchronize()
    note("engine and the graph of the first %d records built" % n)
    res = {}
    for n_new in appends:
        N = n + n_new
        t = {"update_index": [], "graph_update": [], "update": [], "rebuild": []}
        stats = None
        reps = 1 if args.step == "trace" else args.reps + 1
        for rep in range(reps):
            d_rows[:n].copy_(d_old)
            d_counts[:n].copy_(d_old_counts)
            synth(n_new)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.update_index()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            stats = e.knn_graph_update_dev(k, n, d_rows.data_ptr(), d_counts.data_ptr(), mode=vc.MODE_MIH_EXACT, batch=B, stream=st)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if args.step != "trace":
                e.knn_graph_dev(k, d_rows2.data_ptr(), d_counts2.data_ptr(), mode=vc.MODE_MIH_EXACT, batch=B, stream=st)
                torch.cuda.synchronize()
            t3 = time.perf_counter()
            if rep == 0 and args.step != "trace":      # the warm-up: every buffer of the timed window has its size, and the words are compared
                assert torch.equal(d_rows[:N], d_rows2[:N]), "the updated rows differ from the build over the whole store"
                assert torch.equal(d_counts[:N], d_counts2[:N]), "the updated counts differ from the build over the whole store"
                note("append %d: rows and counts equal the build from scratch: %s" % (n_new, stats))
            elif args.step != "trace":
                for name, dt in (("update_index", t1 - t0), ("graph_update", t2 - t1), ("update", t2 - t0), ("rebuild", t3 - t2)):
                    t[name].append(dt)
            kept = e.retain_dev(d_keep.data_ptr(), vc.RETAIN_MASK, None, stream=st)
            torch.cuda.synchronize()
            assert kept == n and len(e) == n
        one = {"n_new": n_new, "stats": stats, "rows_and_counts_equal_rebuild": args.step != "trace"}
        if args.step != "trace":
            one.update({"call_ms_median": {q: round(float(np.median(v)) * 1e3, 3) for q, v in t.items()},
                        "call_ms_min": {q: round(min(v) * 1e3, 3) for q, v in t.items()},
                        "call_ms_max": {q: round(max(v) * 1e3, 3) for q, v in t.items()}, "reps": args.reps})
            med = one["call_ms_median"]
            one["update_over_rebuild"] = round(med["update"] / med["rebuild"], 5)
            one["new_rows_ms_at_the_build_price"] = round(med["rebuild"] * n_new / N, 3)      # the build's per-record price times the new records
            one["join_pair_words"] = float(n) * n_new                                            # (W = 1)
            note("append %d timed: %s" % (n_new, one))
        res["append=%d" % n_new] = one
    with open(args.step_out, "w") as f:
        json.dump(res, f)
    e.close()


ASSIGN_RATE_G = 4521.47      # vc_assign_kernel at 64 bits, K = 4 096, pair-words/s in units of 1e9 (profiles/kmajority_bench.json)


def merge_trace(path, line, n, appends):
    """the kernel statistics (csv) of a `rocprofv3 --kernel-trace --stats` run of --step trace -> the update's launches"""
    rows = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = re.search(r"vc_kgraph_\w+(?:<[^>]*>)?|scan_\w+_kernel|mih_query_kernel|vc_scan_kernel", row["Name"])
            if name:
                key = name.group(0)
                rows[key] = {"calls": int(row["Calls"]) + rows.get(key, {}).get("calls", 0),
                             "total_us": round(float(row["TotalDurationNs"]) / 1e3 + rows.get(key, {}).get("total_us", 0.0), 1)}
    for v in rows.values():
        v["avg_us"] = round(v["total_us"] / v["calls"], 3)
    out = {"kernels": rows, "appends": appends, "how": "rocprofv3 --kernel-trace --stats over --step trace at k = 10 (a run of its own: the build of the old "
                                                        "graph, one update per append size, no rebuild)"}
    count = [v for key, v in rows.items() if "join_kernel" in key and "false" in key]
    if count:                                                                # every count pass of the run: n x n_new pair-words per append (W = 1)
        pw = float(n) * sum(appends)
        out["join_count_pass"] = {"pair_words": pw, "total_us": count[0]["total_us"], "pair_words_per_s_G": round(pw / count[0]["total_us"] / 1e3, 1),
                                  "vc_assign_kernel_pair_words_per_s_G": ASSIGN_RATE_G,
                                  "fraction_of_assign": round(pw / count[0]["total_us"] / 1e3 / ASSIGN_RATE_G, 4)}
    line["trace"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e6)
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--appends", default="1000,10000,100000")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--cluster-size", type=int, default=16, help="records per centre of the synthetic data")
    ap.add_argument("--flips", type=int, default=6, help="a record is its centre with up to this many bits flipped")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=35)
    ap.add_argument("--step-timeout", type=int, default=500, help="seconds a step may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-csv", default=None, help="kernel_stats.csv of a rocprofv3 run of --step trace: merged into --out, nothing is run")
    ap.add_argument("--step", choices=("time", "trace"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--step-out", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--k", type=int, default=10, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    if args.trace_csv:
        line = json.load(open(args.out))
        merge_trace(args.trace_csv, line, int(args.n), [int(float(x)) for x in args.appends.split(",")])
        with open(args.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
        print(json.dumps(line["trace"]))
        return
    line = {"metric": "vc_update_index + vc_knn_graph_update_dev against vc_knn_graph_dev over the whole store, %.3g clustered 64-bit codes (%d per centre, "
                      "<= %d flips) + the appended records, m=2, exact MIH, batches of %d ids, old batches of %d, windows of %d, one engine"
                      % (args.n, args.cluster_size, args.flips, args.batch, OLD_BATCH, WINDOW)}
    with tempfile.TemporaryDirectory() as td:
        for k in [int(x) for x in args.ks.split(",")]:
            part = os.path.join(td, "time_%d.json" % k)      # chained: a step that fails, faults or runs into its time limit ends the run
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", "time", "--step-out", part, "--k", str(k)]
            for key in ("n", "appends", "batch", "cluster_size", "flips", "reps", "seed"):
                cmd += ["--" + key.replace("_", "-"), str(getattr(args, key))]
            rc = subprocess.call(cmd)
            if rc != 0:
                raise SystemExit("the step at k=%d ended with status %d: nothing further is started" % (k, rc))
            line["k=%d" % k] = json.load(open(part))
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
    for k, part in line.items():      # THE ONE CONDITION, after the figures are safe
        one = part.get("append=10000") if isinstance(part, dict) else None
        if one:
            med = one["call_ms_median"]
            assert med["update"] < med["rebuild"], "%s: update %s ms is not below the rebuild's %s ms at 1e4 appended records" % (k, med["update"], med["rebuild"])


if __name__ == "__main__":
    main()
