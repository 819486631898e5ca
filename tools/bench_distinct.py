"""One result per label group (vc_search_knn_distinct_dev) on the store of the clustering benches -- clustered synthetic 64-bit codes, one
engine, 1e6 records, two tables, exact MIH -- with the labels vc_cluster_radius_dev makes at R = 8, 4096 resident queries, k = 100.

  distinct    vc_search_knn_distinct_dev, labels resident, row labels and counts asked for, stats asked for
  plain       vc_search_knn_dev at k = 100 on the same handle: it answers the other question (the nearest records, copies included) and
              marks the floor
  host        the path replaced: the same searches at the same k' sequence (vc_search_knn_dev), rows, counts and all labels copied
              home, the rows collapsed with numpy (first occurrence per label, row by row), the unfinished queries searched again
  searches    the searches of the device call alone -- the same k' and the same retry queries, gathered beforehand -- so that
              distinct - searches bounds what the collapse, the scan, the gather and the wait per round cost together

The rows, row labels and counts of `distinct` are asserted equal to those of `host`, every word, in the same run.  A host clock around
each leg ending in a device synchronise, legs alternated, medians of --reps with min and max as the spread.  No time or ratio is fixed
in advance.

--trace-csv merges the kernel times of a `rocprofv3 --kernel-trace --stats --output-format csv` run of the distinct leg alone (a run of
its own: `rocprofv3 ... -- python tools/bench_distinct.py --step --only distinct --step-out X`) into --out: the time of the collapse
launches per call and their share of the call's median.

The measurement is one child process under its own `timeout`; nothing is repeated after a failure.  Prints one JSON line; --out also
writes it.  Not measured: the sharded forms, other widths, N, k and label sources, VC_MODE_LINEAR, more than one GPU.

    python tools/bench_distinct.py [--n 1e6] [--nq 4096] [--k 100] [--reps 7] [--out profiles/distinct_bench.json]
"""
import argparse
import csv
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MAX_K = 8192
INF = np.uint64(0xFFFFFFFFFFFFFFFF)


def collapse_home(rows, counts, labels, id_base, k, kp):
    """numpy, row by row: (kept entries, their labels, count or None for a query that goes on) per row of a round at k'"""
    out = []
    for row, cnt in zip(rows, counts):
        row = row[:cnt]
        if cnt == kp and kp < MAX_K:         # exact MIH: a full row is sure only below its last distance (the header's sure prefix)
            row = row[(row >> np.uint64(32)) < (row[-1] >> np.uint64(32))]
        labs = labels[(row & np.uint64(0xFFFFFFFF)).astype(np.int64) - id_base]
        pos = np.sort(np.unique(labs, return_index=True)[1])
        d = len(pos)
        if d >= k:
            out.append((row[pos[:k]], labs[pos[:k]], k))
        elif cnt < kp:
            out.append((row[pos], labs[pos], d))
        elif kp >= MAX_K:
            out.append((row[pos], labs[pos], d | 0x80000000))
        else:
            out.append(None)
    return out


def step(args):
    import torch
    from verticut_amd import engine as vc
    n, nq, k, bits = int(args.n), args.nq, args.k, 64
    words = bits // 64

    def note(what):
        print("[bench_distinct] %s" % what, file=sys.stderr, flush=True)

    e = vc.Engine(bits, capacity=n, n_tables=2, flags=vc.FLAG_LEAN_TIMING)
    e.add_synthetic(n, seed=args.seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // args.cluster_size, 1), max_flips=args.flips)
    e.build_index()
    st = torch.cuda.current_stream().cuda_stream
    i32, i64 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.int64, device="cuda")
    d_labels = torch.empty((n,), **i32)
    t0 = time.perf_counter()
    n_pairs, n_clusters = e.cluster_radius_dev(args.radius, d_labels.data_ptr(), mode=vc.MODE_MIH_EXACT, stream=st)
    torch.cuda.synchronize()
    note("labels: %d clusters at R = %d in %.1f ms" % (n_clusters, args.radius, (time.perf_counter() - t0) * 1e3))
    ids = torch.from_numpy((np.arange(nq, dtype=np.int64) * (n // nq)).astype(np.int32)).cuda()
    d_q = torch.empty((nq, words), **i64)
    e.get_codes_dev(ids.data_ptr(), nq, d_q.data_ptr(), stream=st)
    d_out, d_rl, d_cnt = torch.empty((nq, k), **i64), torch.empty((nq, k), **i32), torch.empty((nq,), **i32)
    d_rows, d_rcnt = torch.empty((nq * 2 * k,), **i64), torch.empty((nq,), **i32)   # grown below if a later round needs more
    res = {"bits": bits, "n": n, "nq": nq, "k": k, "radius": args.radius, "n_clusters": int(n_clusters), "k_first": args.k_first}
    stats = {}

    def leg_distinct():
        stats["last"] = e.search_knn_distinct_dev(d_q.data_ptr(), nq, k, d_labels.data_ptr(), d_out.data_ptr(), d_rl.data_ptr(), d_cnt.data_ptr(),
                                                  mode=vc.MODE_MIH_EXACT, k_first=args.k_first, stream=st)

    def leg_plain():
        e.search_knn_dev(d_q.data_ptr(), nq, k, d_out.data_ptr(), d_cnt.data_ptr(), mode=vc.MODE_MIH_EXACT, stream=st)

    rounds = []          # what the host path saw: (k', queries searched, indices of the queries searched)

    def leg_host(record=False):
        nonlocal d_rows
        labels = d_labels.cpu().numpy().view(np.uint32)                      # all labels home, as a caller without the device call has to
        rows_out, rl_out, cnt_out = np.full((nq, k), INF, dtype=np.uint64), np.zeros((nq, k), dtype=np.uint32), np.zeros(nq, dtype=np.uint32)
        todo, kp, d_cur = np.arange(nq), (args.k_first or min(MAX_K, 2 * k)), d_q
        while len(todo):
            m = len(todo)
            if d_rows.numel() < m * kp:
                d_rows = torch.empty((m * kp,), **i64)
            e.search_knn_dev(d_cur.data_ptr(), m, kp, d_rows.data_ptr(), d_rcnt.data_ptr(), mode=vc.MODE_MIH_EXACT, stream=st)
            rows = d_rows[:m * kp].cpu().numpy().view(np.uint64).reshape(m, kp)
            counts = d_rcnt[:m].cpu().numpy().view(np.uint32)
            if record:
                rounds.append((kp, m, todo.copy()))
            again = []
            for i, got in zip(todo, collapse_home(rows, counts, labels, e.id_base, k, kp)):
                if got is None:
                    again.append(i)
                else:
                    w = min(len(got[0]), k)
                    rows_out[i, :w], rl_out[i, :w], cnt_out[i] = got[0][:w], got[1][:w], got[2]
            todo = np.array(again, dtype=np.int64)
            if len(todo):
                d_cur = d_q[torch.from_numpy(todo).cuda()].contiguous()
                kp = min(MAX_K, 2 * kp)
        return rows_out, rl_out, cnt_out

    legs = {"distinct": leg_distinct}
    if args.only != "distinct":
        want = leg_host(record=True)
        leg_distinct()
        torch.cuda.synchronize()
        got = (d_out.cpu().numpy().view(np.uint64), d_rl.cpu().numpy().view(np.uint32), d_cnt.cpu().numpy().view(np.uint32))
        for name, g, w in zip(("rows", "row_labels", "counts"), got, want):
            assert np.array_equal(g, w), "the device call's %s differ from the host path's" % name
        res["equals_host_path"] = True
        res["rounds"] = [{"k_prime": kp, "n_searched": m} for kp, m, _ in rounds]
        assert stats["last"]["n_rounds"] == len(rounds) and stats["last"]["n_searched"] == sum(m for _, m, _ in rounds)
        subsets = [d_q if j == 0 else d_q[torch.from_numpy(idx).cuda()].contiguous() for j, (_, _, idx) in enumerate(rounds)]
        if d_rows.numel() < max(m * kp for kp, m, _ in rounds):
            d_rows = torch.empty((max(m * kp for kp, m, _ in rounds),), **i64)

        def leg_searches():
            for (kp, m, _), sub in zip(rounds, subsets):
                e.search_knn_dev(sub.data_ptr(), m, kp, d_rows.data_ptr(), d_rcnt.data_ptr(), mode=vc.MODE_MIH_EXACT, stream=st)

        legs.update({"plain": leg_plain, "host": leg_host, "searches": leg_searches})
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    note("first calls done: %s" % stats.get("last"))
    t = {name: [] for name in legs}
    for _ in range(args.reps):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[name].append(time.perf_counter() - t0)
    res.update({"call_ms_median": {key: round(float(np.median(v)) * 1e3, 4) for key, v in t.items()},
                "call_ms_min": {key: round(min(v) * 1e3, 4) for key, v in t.items()},
                "call_ms_max": {key: round(max(v) * 1e3, 4) for key, v in t.items()}, "reps": args.reps, "stats": stats["last"]})
    med = res["call_ms_median"]
    if args.only != "distinct":
        res["distinct_over_plain"] = round(med["distinct"] / med["plain"], 3)
        res["host_over_distinct"] = round(med["host"] / med["distinct"], 3)
        res["beside_the_searches_ms"] = round(med["distinct"] - med["searches"], 4)
        res["beside_the_searches_share"] = round((med["distinct"] - med["searches"]) / med["distinct"], 4)
        res["beside_the_searches_note"] = ("distinct - searches: the collapse launches, the scan and gather, the copy of 24 bytes and the wait per round "
                                           "together; an upper bound of the collapse kernel's share, not its time")
    note("timed: %s" % res)
    with open(args.step_out, "w") as f:
        json.dump(res, f)
    e.close()


def merge_trace(path, res):
    """the kernel statistics (csv) of a `rocprofv3 --kernel-trace --stats` run of one --step of --only distinct -> the collapse
    launches' time and their share of the kernel time of the run"""
    rows = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "vc_distinct_" in row["Name"]:
                rows[row["Name"]] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 3), "min_us": round(float(row["MinNs"]) / 1e3, 3),
                                     "max_us": round(float(row["MaxNs"]) / 1e3, 3), "total_us": round(float(row["TotalDurationNs"]) / 1e3, 1)}
    is_collapse = lambda key: "wave_kernel" in key or "table_kernel" in key
    collapse = sum(v["total_us"] for key, v in rows.items() if is_collapse(key))
    # one collapse launch per round here (a round's rows fit the scratch budget), so the launches count the calls of the traced run
    n_calls = sum(v["calls"] for key, v in rows.items() if is_collapse(key)) / res["stats"]["n_rounds"]
    res["kernel_trace"] = {"kernels": rows, "calls_traced": n_calls, "collapse_us_per_call": round(collapse / n_calls, 1),
                           "new_kernels_us_per_call": round(sum(v["total_us"] for v in rows.values()) / n_calls, 1),
                           "collapse_share_of_call": round(collapse / n_calls / (res["call_ms_median"]["distinct"] * 1e3), 5),
                           "how": "rocprofv3 --kernel-trace --stats over one --step of --only distinct (a run of its own, first call included); "
                                  "the share is the collapse launches' time per call over the call's median of the untraced run"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e6)
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--k-first", type=int, default=0, help="k' of the first round (0 = 2 k)")
    ap.add_argument("--radius", type=int, default=8, help="of vc_cluster_radius_dev, which makes the labels")
    ap.add_argument("--cluster-size", type=int, default=16, help="records per centre of the synthetic data")
    ap.add_argument("--flips", type=int, default=6, help="a record is its centre with up to this many bits flipped")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=35, help="of the synthetic data")
    ap.add_argument("--only", default="all", choices=("all", "distinct"), help="distinct: the device call alone (for a profiler run)")
    ap.add_argument("--step-timeout", type=int, default=400, help="seconds the measurement may take")
    ap.add_argument("--trace-csv", default=None, help="the *_kernel_stats.csv a rocprofv3 --kernel-trace --stats run of one --step of --only distinct wrote: "
                                                     "merged into --out")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--step-out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    if args.trace_csv:
        line = json.load(open(args.out))
        merge_trace(args.trace_csv, line["run"])
        with open(args.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
        return print(json.dumps(line))
    line = {"metric": "vc_search_knn_distinct_dev (exact MIH, k = %d, labels of vc_cluster_radius_dev at R = %d) against vc_search_knn_dev at the same k and "
                      "against the host path it replaces (the same searches, rows and labels home, numpy collapse, retry loop); %.3g clustered 64-bit codes "
                      "(%d per centre, <= %d flips), two tables, %d resident queries, one engine; not measured: the sharded forms, other widths, N, k and "
                      "label sources, VC_MODE_LINEAR, more than one GPU" % (args.k, args.radius, args.n, args.cluster_size, args.flips, args.nq)}
    with tempfile.TemporaryDirectory() as td:
        part = os.path.join(td, "run.json")
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", "--step-out", part, "--only", args.only]
        for key in ("n", "nq", "k", "k_first", "radius", "cluster_size", "flips", "reps", "seed"):
            cmd += ["--" + key.replace("_", "-"), str(getattr(args, key))]
        rc = subprocess.call(cmd)
        if rc != 0:
            raise SystemExit("the measurement ended with status %d" % rc)
        line["run"] = json.load(open(part))
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
