"""Filtered k-NN (vc_search_knn_filtered_dev) on the store of the clustering benches -- clustered synthetic 64-bit codes, one engine,
1e6 records, two tables, exact MIH -- with random VC_FILTER_BITS masks at A/N = 1, 1/4, 1/16, 1/64, 1/256, 1/4096, 1/65536, 4096
resident queries, k = 100.

  filtered    vc_search_knn_filtered_dev on three handles over the same records: VC_FILTER_ROUTE = 1 (post-filter first), 2 (pre-filter
              only) and 0 (the plan's choice), the mask resident as bits, counts and stats asked for
  plain       vc_search_knn_dev at k = 100 on the same handle: the unfiltered question; marks the floor of the post-filter route
  host        the path replaced: vc_search_knn_dev at the plan's k' = clamp(2 ceil(k N / A), k, 8192), rows and counts home, the rows
              filtered with numpy against the mask, the unfinished queries searched again at 2 k' up to 8192 -- beyond which that
              path has no answer (`host_unanswered`)

The rows of every route are asserted equal to each other, and for a sample of queries to a numpy brute force over all codes, in the
same run.  A host clock around each call ending in a device synchronise, medians of --reps after a warm-up call with min and max as
the spread; a leg whose warm-up call takes longer than --slow-ms runs --slow-reps repetitions instead (recorded as `reps`).  From
the forced-route times the crossover of the two routes is read in units of the plan's threshold, 2 ceil(k N / A), and the automatic
route is compared with the faster forced route at every selectivity.  No time or ratio is fixed in advance.

The pair rate: at A/N = 1 the pre-filter route is three walks over N codes for every query; 3 nq N W pair-words over the call's
median is a lower bound of the walk kernels' rate (gather, list, cut, select and the launches included), set against the rate
profiles/kmajority_bench.json records for vc_assign_kernel -- the same data flow without the placement work.  --trace-csv merges the
kernel times of a `rocprofv3 --kernel-trace --stats --output-format csv` run of `--step --only pre` (a run of its own) into --out.

The measurement is one child process under its own `timeout`; nothing is repeated after a failure.  Prints one JSON line; --out also
writes it.  Not measured: the sharded forms, VC_MODE_LINEAR, other widths, N, k and filter kinds, the host form, more than one GPU.

    python tools/bench_filtered.py [--n 1e6] [--nq 4096] [--k 100] [--reps 7] [--out profiles/filtered_bench.json]
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
MAX_K = 8192
INF = np.uint64(0xFFFFFFFFFFFFFFFF)
ONE_IN = (1, 4, 16, 64, 256, 4096, 65536)
_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint64)


def step(args):
    import torch
    from verticut_amd import engine as vc
    n, nq, k, bits = int(args.n), args.nq, args.k, 64

    def note(what):
        print("[bench_filtered] %s" % what, file=sys.stderr, flush=True)

    routes = (2,) if args.only == "pre" else (1, 2, 0)
    eng = {}
    for route in routes:                                                    # the knob is read when the handle is made
        os.environ["VC_FILTER_ROUTE"] = str(route)
        e = vc.Engine(bits, capacity=n, n_tables=2, flags=vc.FLAG_LEAN_TIMING)
        e.add_synthetic(n, seed=args.seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // args.cluster_size, 1), max_flips=args.flips)
        e.build_index()
        eng[route] = e
    del os.environ["VC_FILTER_ROUTE"]
    e0 = eng[routes[-1]]
    st = torch.cuda.current_stream().cuda_stream
    i32, i64 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.int64, device="cuda")
    ids = torch.from_numpy((np.arange(nq, dtype=np.int64) * (n // nq)).astype(np.int32)).cuda()
    d_q = torch.empty((nq, 1), **i64)
    e0.get_codes_dev(ids.data_ptr(), nq, d_q.data_ptr(), stream=st)
    d_out, d_cnt = torch.empty((nq, k), **i64), torch.empty((nq,), **i32)
    d_rows, d_rcnt = torch.empty((nq * MAX_K,), **i64), torch.empty((nq,), **i32)
    torch.cuda.synchronize()
    queries = d_q.cpu().numpy().view(np.uint8).reshape(nq, 8)
    all_ids = torch.arange(n, dtype=torch.int32, device="cuda")
    d_codes = torch.empty((n, 1), **i64)
    e0.get_codes_dev(all_ids.data_ptr(), n, d_codes.data_ptr(), stream=st)
    torch.cuda.synchronize()
    codes = d_codes.cpu().numpy().view(np.uint8).reshape(n, 8)
    sample = list(range(0, nq, max(nq // args.check, 1)))[:args.check]
    rng = np.random.default_rng(args.seed)
    res = {"bits": bits, "n": n, "nq": nq, "k": k, "reps": args.reps, "selectivities": []}

    def timed(fn, slow_ok=True):
        fn()                                                                 # the warm-up call (buffers grow here)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        first = time.perf_counter() - t0
        reps = args.slow_reps if slow_ok and first * 1e3 > args.slow_ms else args.reps
        t = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": round(float(np.median(t)), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4), "reps": reps}

    if args.only != "pre":
        res["plain"] = timed(lambda: e0.search_knn_dev(d_q.data_ptr(), nq, k, d_out.data_ptr(), d_cnt.data_ptr(), mode=vc.MODE_MIH_EXACT, stream=st))
        note("plain: %s" % res["plain"])
    for one_in in (ONE_IN if args.only != "pre" else (1,)):
        allowed = np.ones(n, dtype=bool) if one_in == 1 else rng.integers(0, one_in, size=n) == 0
        if not allowed.any():
            allowed[n // 2] = True
        A = int(np.count_nonzero(allowed))
        d_bits = torch.from_numpy(np.packbits(allowed, bitorder="little").view(np.uint8).copy()).cuda()
        if d_bits.numel() % 4:
            d_bits = torch.cat([d_bits, torch.zeros(4 - d_bits.numel() % 4, dtype=torch.uint8, device="cuda")])
        entry = {"one_in": one_in, "n_allowed": A, "threshold_units": int(2 * ((k * n + A - 1) // A)), "routes": {}}
        rows_by_route, stats = {}, {}
        for route in routes:
            e = eng[route]

            def leg():
                stats[route] = e.search_knn_filtered_dev(d_q.data_ptr(), nq, k, d_bits.data_ptr(), d_out.data_ptr(), d_cnt.data_ptr(), kind=vc.FILTER_BITS,
                                                         mode=vc.MODE_MIH_EXACT, stream=st)

            entry["routes"][str(route)] = dict(timed(leg), stats=None)
            entry["routes"][str(route)]["stats"] = stats[route]
            rows_by_route[route] = (d_out.cpu().numpy().view(np.uint64).copy(), d_cnt.cpu().numpy().view(np.uint32).copy())
            note("A/N = 1/%d route %d: %s" % (one_in, route, entry["routes"][str(route)]))
        first = rows_by_route[routes[0]]
        for route in routes[1:]:
            assert np.array_equal(rows_by_route[route][0], first[0]) and np.array_equal(rows_by_route[route][1], first[1]), "the routes' rows differ"
        idx = np.nonzero(allowed)[0]
        for qi in sample:                                                    # numpy brute force over the allowed codes
            d = _POP8[codes[idx] ^ queries[qi][None, :]].sum(axis=1, dtype=np.uint64)
            want = np.sort(d << np.uint64(32) | idx.astype(np.uint64))[:k]
            assert np.array_equal(first[0][qi][:len(want)], want) and first[1][qi] == len(want) and np.all(first[0][qi][len(want):] == INF), "a row differs from the brute force"
        entry["rows_equal_brute_force_sample"] = len(sample)
        if args.only != "pre":
            unanswered = {}

            def leg_host():
                mask = allowed                                               # the mask lives at home on this path
                rows_out, cnt_out = np.full((nq, k), INF, dtype=np.uint64), np.zeros(nq, dtype=np.uint32)
                todo, kp, d_cur = np.arange(nq), max(k, min(MAX_K, 2 * ((k * n + A - 1) // A))), d_q
                while len(todo):
                    m = len(todo)
                    e0.search_knn_dev(d_cur.data_ptr(), m, kp, d_rows.data_ptr(), d_rcnt.data_ptr(), mode=vc.MODE_MIH_EXACT, stream=st)
                    rows = d_rows[:m * kp].cpu().numpy().view(np.uint64).reshape(m, kp)
                    counts = d_rcnt[:m].cpu().numpy().view(np.uint32)
                    again = []
                    for i, row, cnt in zip(todo, rows, counts):
                        row = row[:cnt]
                        if cnt == kp:                                        # exact MIH: a full row is sure only below its last distance
                            row = row[(row >> np.uint64(32)) < (row[-1] >> np.uint64(32))]
                        kept = row[mask[(row & np.uint64(0xFFFFFFFF)).astype(np.int64)]]
                        if len(kept) >= k or cnt < kp:
                            w = min(len(kept), k)
                            rows_out[i, :w], cnt_out[i] = kept[:w], w
                        else:
                            again.append(i)
                    todo = np.array(again, dtype=np.int64)
                    if kp >= MAX_K:
                        break
                    if len(todo):
                        d_cur = d_q[torch.from_numpy(todo).cuda()].contiguous()
                        kp = min(MAX_K, 2 * kp)
                unanswered["n"] = int(len(todo))
                return rows_out, cnt_out, todo

            entry["host"] = timed(leg_host)
            rows_out, cnt_out, todo = leg_host()
            entry["host_unanswered"] = unanswered["n"]
            done = np.setdiff1d(np.arange(nq), todo)
            assert np.array_equal(rows_out[done], first[0][done]) and np.array_equal(cnt_out[done], first[1][done]), "the host path's rows differ"
            note("A/N = 1/%d host: %s unanswered %d" % (one_in, entry["host"], unanswered["n"]))
        res["selectivities"].append(entry)
    if args.only != "pre":
        # the automatic route against the faster forced route, within the spread of the repetitions
        worst = 0.0
        for entry in res["selectivities"]:
            r = entry["routes"]
            best = min(("1", "2"), key=lambda x: r[x]["median_ms"])
            spread = max(r[x]["max_ms"] - r[x]["min_ms"] for x in ("0", best))   # min .. max of the repetitions of the two legs compared
            entry["faster_forced_route"] = int(best)
            entry["auto_minus_faster_ms"] = round(r["0"]["median_ms"] - r[best]["median_ms"], 4)
            entry["spread_ms"] = round(spread, 4)
            entry["auto_within_spread"] = bool(entry["auto_minus_faster_ms"] <= spread)
            worst = max(worst, spread / r[best]["median_ms"])
        res["largest_relative_spread"] = round(worst, 4)
        post_wins = [e_["threshold_units"] for e_ in res["selectivities"] if e_["faster_forced_route"] == 1]
        pre_wins = [e_["threshold_units"] for e_ in res["selectivities"] if e_["faster_forced_route"] == 2]
        res["crossover"] = {"post_filter_faster_up_to_units": max(post_wins) if post_wins else None, "pre_filter_faster_from_units": min(pre_wins) if pre_wins else None,
                            "units": "2 ceil(k N / A), what the plan compares with VC_FILTER_POST_MAX_K"}
    full = next(e_ for e_ in res["selectivities"] if e_["one_in"] == 1)["routes"]["2"]
    pw = 3.0 * nq * n * (bits // 64)
    ref = json.load(open(os.path.join(ROOT, "profiles", "kmajority_bench.json")))["shapes"][0]["assign_kernel"]["pair_words_per_s_G"]
    res["subset_scan"] = {"pair_words": pw, "call_ms_median": full["median_ms"], "pair_words_per_s_G": round(pw / full["median_ms"] / 1e6, 1),
                          "vc_assign_kernel_pair_words_per_s_G": ref, "fraction_of_assign": round(pw / full["median_ms"] / 1e6 / ref, 4),
                          "how": "three walks x nq x N x W pair-words over the median of the whole pre-filter call at A/N = 1 (keep set, list, gather, "
                                 "cuts, bases, select and launches included): a lower bound of the walk kernels' rate"}
    note("timed: %s" % json.dumps(res)[:400])
    with open(args.step_out, "w") as f:
        json.dump(res, f)
    for e in eng.values():
        e.close()


def merge_trace(path, res):
    """the kernel statistics (csv) of a `rocprofv3 --kernel-trace --stats` run of one --step of --only pre -> the walk kernels' times"""
    rows = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "vc_filter_" in row["Name"]:
                rows[re.search(r"vc_filter_\w+(?:<\d+>)?", row["Name"]).group(0)] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 3), "min_us": round(float(row["MinNs"]) / 1e3, 3),
                                                   "max_us": round(float(row["MaxNs"]) / 1e3, 3), "total_us": round(float(row["TotalDurationNs"]) / 1e3, 1)}
    walks = {key: v for key, v in rows.items() if any(w in key for w in ("hist_kernel", "count_kernel", "place_kernel"))}
    pw_walk = float(res["nq"]) * res["n"] * (res["bits"] // 64)
    ref = res["subset_scan"]["vc_assign_kernel_pair_words_per_s_G"]
    out = {"kernels": rows, "how": "rocprofv3 --kernel-trace --stats over one --step of --only pre (a run of its own, warm-up calls included)"}
    for key, v in walks.items():
        if "count_kernel" in key or "place_kernel" in key:                  # one launch per call covers the whole window
            v["pair_words_per_s_G"] = round(pw_walk / v["avg_us"] / 1e3, 1)
            v["fraction_of_assign"] = round(pw_walk / v["avg_us"] / 1e3 / ref, 4)
    hist = [v for key, v in walks.items() if "hist_kernel" in key]
    if hist:                                                                 # two launches per call: the prefix and the rest
        per_call = 2 * sum(v["total_us"] for v in hist) / sum(v["calls"] for v in hist)
        out["hist_us_per_call"] = round(per_call, 1)
        out["hist_pair_words_per_s_G"] = round(pw_walk / per_call / 1e3, 1)
        out["hist_fraction_of_assign"] = round(pw_walk / per_call / 1e3 / ref, 4)
    res["kernel_trace"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e6)
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--cluster-size", type=int, default=16, help="records per centre of the synthetic data")
    ap.add_argument("--flips", type=int, default=6, help="a record is its centre with up to this many bits flipped")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--slow-ms", type=float, default=3000.0, help="a leg whose warm call takes longer runs --slow-reps repetitions")
    ap.add_argument("--slow-reps", type=int, default=3)
    ap.add_argument("--check", type=int, default=8, help="queries whose rows are compared with a numpy brute force")
    ap.add_argument("--seed", type=int, default=35, help="of the synthetic data and the masks")
    ap.add_argument("--only", default="all", choices=("all", "pre"), help="pre: the pre-filter route at A/N = 1 alone (for a profiler run)")
    ap.add_argument("--step-timeout", type=int, default=900, help="seconds the measurement may take")
    ap.add_argument("--trace-csv", default=None, help="the *_kernel_stats.csv of a rocprofv3 run of one --step of --only pre: merged into --out")
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
    line = {"metric": "vc_search_knn_filtered_dev (exact MIH, k = %d, random VC_FILTER_BITS masks at A/N = 1 .. 1/65536) under VC_FILTER_ROUTE 1, 2 and 0 against "
                      "vc_search_knn_dev at the same k and against the host path it replaces (search at the plan's k', rows home, numpy filter, repeat); "
                      "%.3g clustered 64-bit codes (%d per centre, <= %d flips), two tables, %d resident queries, one engine; not measured: the sharded "
                      "forms, VC_MODE_LINEAR, other widths, N, k and filter kinds, more than one GPU" % (args.k, args.n, args.cluster_size, args.flips, args.nq)}
    with tempfile.TemporaryDirectory() as td:
        part = os.path.join(td, "run.json")
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", "--step-out", part, "--only", args.only]
        for key in ("n", "nq", "k", "cluster_size", "flips", "reps", "slow_ms", "slow_reps", "check", "seed"):
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
