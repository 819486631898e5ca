"""Scoped k-NN (vc_search_knn_scoped_dev) on the store of bench_filtered.py -- clustered synthetic 64-bit codes, one engine, 1e6
records -- with 4096 resident queries, k = 100, under scope layouts of the store:

  equal U     U equal scopes (record i carries i mod U after a shuffle), U = 1, 16, 64, 256, 4096, 65536; every query draws its scope
              uniformly from the U
  skewed      scope j holds 2^j records, j = 0 .. 19 (the last one what is left of N); every query draws one of the 20 uniformly

Each layout is compared with THE PATH THE CALL REPLACES: the loop of vc_search_knn_filtered_dev(VC_FILTER_EQUAL, value,
VC_MODE_LINEAR), one call per distinct query scope, on the same handle, with the queries split by value and the per-value outputs
allocated outside the clock (the loop at its best).  The rows of the two paths are asserted equal in the same run.  At U = 1 the
single filtered call and vc_search_knn_dev (linear) are timed as well.  A host clock around calls that end in a device synchronise,
medians of --reps after a warm-up, with min and max.

THE ONE CONDITION, fixed before anything was measured: for every equal layout with at least 64 distinct query scopes the scoped
call's MEDIAN is below the loop's MINIMUM.  `condition` records the verdict per layout and overall; nothing else is a target.

Pairs: n_pairs (the statistics: the distances the answers need) against the pairs the walk kernels compute -- per wave-slice its
positions times the sorted queries of the slots it touches, from the plan (tests/scope_common.py's arithmetic) -- and their ratio.
--trace-csv merges the kernel times of a `rocprofv3 --kernel-trace --stats --output-format csv` run of `--step --only U` (a run of
its own) into --out, with the walk kernels' pair-word rates beside vc_filter_count_kernel's and vc_assign_kernel's.

The measurement is one child process under its own `timeout`; nothing is repeated after a failure.  Prints one JSON line; --out also
writes it.  Not measured: the sharded and host forms, other widths, N and k, more than one GPU.

    python tools/bench_scoped.py [--n 1e6] [--nq 4096] [--k 100] [--reps 7] [--out profiles/scoped_bench.json]
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
EQUAL_U = (1, 16, 64, 256, 4096, 65536)
FILTER_COUNT_RATE_G = 3050.0      # vc_filter_count_kernel, DESIGN.md 5.14 (profiles/filtered_kernel_stats.csv)
SLICE_LEN = 512                   # 64-bit codes: vc_filter_slice_len(1)


def layouts(n, nq, rng, only):
    out = []
    for U in EQUAL_U:
        if only not in ("all", str(U)):
            continue
        scope = (np.arange(n, dtype=np.uint32) % np.uint32(U))[rng.permutation(n)]
        out.append(("equal %d" % U, U, scope, rng.integers(0, U, size=nq).astype(np.uint32)))
    if only in ("all", "skewed"):
        scope = np.minimum(np.floor(np.log2(np.arange(n, dtype=np.float64) + 1)), 19).astype(np.uint32)[rng.permutation(n)]
        out.append(("skewed", 20, scope, rng.integers(0, 20, size=nq).astype(np.uint32)))
    return out


def computed_pairs(scope, qscope, window=1 << 20):
    """the pairs the walk kernels compute in one walk: per slice its positions x the sorted queries of the slots between its ends"""
    uniq, per_q = np.unique(qscope, return_counts=True)
    qrun = np.concatenate([[0], np.cumsum(per_q)])
    sizes = np.bincount(np.searchsorted(uniq, scope[np.isin(scope, uniq)]), minlength=len(uniq))
    seg = np.concatenate([[0], np.cumsum(sizes)])
    A, total = int(seg[-1]), 0
    for w0 in range(0, A, window):
        wn = min(window, A - w0)
        p0 = w0 + np.arange(0, wn, SLICE_LEN)
        p1 = np.minimum(p0 + SLICE_LEN, w0 + wn)
        u0, u1 = np.searchsorted(seg[1:], p0, side="right"), np.searchsorted(seg[1:], p1 - 1, side="right")
        total += int(((p1 - p0) * (qrun[u1 + 1] - qrun[u0])).sum())
    return total


def step(args):
    import torch
    from verticut_amd import engine as vc
    n, nq, k, bits = int(args.n), args.nq, args.k, 64

    def note(what):
        print("[bench_scoped] %s" % what, file=sys.stderr, flush=True)

    e = vc.Engine(bits, capacity=n, flags=vc.FLAG_LEAN_TIMING)
    e.add_synthetic(n, seed=args.seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // args.cluster_size, 1), max_flips=args.flips)
    st = torch.cuda.current_stream().cuda_stream
    i32, i64 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.int64, device="cuda")
    ids = torch.from_numpy((np.arange(nq, dtype=np.int64) * (n // nq)).astype(np.int32)).cuda()
    d_q = torch.empty((nq, 1), **i64)
    e.get_codes_dev(ids.data_ptr(), nq, d_q.data_ptr(), stream=st)
    d_out, d_cnt = torch.empty((nq, k), **i64), torch.empty((nq,), **i32)
    torch.cuda.synchronize()
    rng = np.random.default_rng(args.seed)
    res = {"bits": bits, "n": n, "nq": nq, "k": k, "reps": args.reps, "layouts": []}

    def timed(fn):
        fn()                                                                 # the warm-up call (buffers grow here)
        torch.cuda.synchronize()
        t = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": round(float(np.median(t)), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}

    for name, U, scope, qscope in layouts(n, nq, rng, args.only):
        d_scope, d_qscope = torch.from_numpy(scope.view(np.int32).copy()).cuda(), torch.from_numpy(qscope.view(np.int32).copy()).cuda()
        stats = {}

        def leg_scoped():
            stats["s"] = e.search_knn_scoped_dev(d_q.data_ptr(), nq, k, d_scope.data_ptr(), d_qscope.data_ptr(), d_out.data_ptr(), d_cnt.data_ptr(), stream=st)

        entry = {"layout": name, "scopes_in_store": U, "scoped": timed(leg_scoped)}
        entry["stats"] = stats["s"]
        rows, counts = d_out.cpu().numpy().view(np.uint64).copy(), d_cnt.cpu().numpy().view(np.uint32).copy()
        cp = computed_pairs(scope, qscope)
        entry["pairs"] = {"n_pairs": stats["s"]["n_pairs"], "computed_per_walk": cp, "computed_over_needed": round(cp / max(stats["s"]["n_pairs"], 1), 3)}
        note("%s scoped: %s %s" % (name, entry["scoped"], entry["pairs"]))
        if args.only == "all" or args.loop:
            # the loop of the parent's call: queries split by value and outputs allocated outside the clock
            values = np.unique(qscope)
            parts = []
            for v in values:
                idx = np.nonzero(qscope == v)[0]
                parts.append((int(v), idx, d_q[torch.from_numpy(idx).cuda()].contiguous(), torch.empty((len(idx), k), **i64), torch.empty((len(idx),), **i32)))
            torch.cuda.synchronize()

            def leg_loop():
                for v, idx, q_v, o_v, c_v in parts:
                    e.search_knn_filtered_dev(q_v.data_ptr(), len(idx), k, d_scope.data_ptr(), o_v.data_ptr(), c_v.data_ptr(), kind=vc.FILTER_EQUAL, value=v,
                                              mode=vc.MODE_LINEAR, with_stats=False, stream=st)

            entry["loop"] = dict(timed(leg_loop), calls=len(values))
            for v, idx, q_v, o_v, c_v in parts:
                assert np.array_equal(o_v.cpu().numpy().view(np.uint64), rows[idx]) and np.array_equal(c_v.cpu().numpy().view(np.uint32), counts[idx]), \
                    "the scoped rows differ from the filtered loop's (%s, value %d)" % (name, v)
            entry["rows_equal_loop"] = True
            entry["speedup_median"] = round(entry["loop"]["median_ms"] / entry["scoped"]["median_ms"], 2)
            if name.startswith("equal") and len(values) >= 64:
                entry["condition_scoped_median_below_loop_min"] = bool(entry["scoped"]["median_ms"] < entry["loop"]["min_ms"])
            note("%s loop: %s" % (name, entry["loop"]))
        if name == "equal 1":
            entry["plain_linear"] = timed(lambda: e.search_knn_dev(d_q.data_ptr(), nq, k, d_out.data_ptr(), d_cnt.data_ptr(), mode=vc.MODE_LINEAR, stream=st))
            prow = d_out.cpu().numpy().view(np.uint64)
            assert np.array_equal(prow, rows), "the scoped rows at one scope differ from vc_search_knn_dev's"
            entry["rows_equal_plain"] = True
            note("plain: %s" % entry["plain_linear"])
        res["layouts"].append(entry)
    verdicts = [x["condition_scoped_median_below_loop_min"] for x in res["layouts"] if "condition_scoped_median_below_loop_min" in x]
    res["condition"] = {"rule": "every equal layout with >= 64 distinct query scopes: scoped median < loop minimum", "layouts": len(verdicts),
                        "holds": bool(verdicts) and all(verdicts)}
    with open(args.step_out, "w") as f:
        json.dump(res, f)
    e.close()


def merge_trace(path, res, layout):
    """the kernel statistics (csv) of a `rocprofv3 --kernel-trace --stats` run of one --step --only <layout> -> per-kernel times and the
    walks' pair-word rates"""
    rows = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            m = re.search(r"vc_scope_\w+(?:<[\d, ]+>)?", row["Name"])
            if m:
                rows[m.group(0)] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 3), "min_us": round(float(row["MinNs"]) / 1e3, 3),
                                    "max_us": round(float(row["MaxNs"]) / 1e3, 3), "total_us": round(float(row["TotalDurationNs"]) / 1e3, 1)}
    entry = next(x for x in res["layouts"] if x["layout"] == layout)
    ref = json.load(open(os.path.join(ROOT, "profiles", "kmajority_bench.json")))["shapes"][0]["assign_kernel"]["pair_words_per_s_G"]
    pw = float(entry["pairs"]["computed_per_walk"]) * (res["bits"] // 64)
    for key, v in rows.items():
        if "walk_kernel" in key:
            v["pair_words_per_s_G"] = round(pw / v["avg_us"] / 1e3, 1)
            v["fraction_of_filter_count"] = round(pw / v["avg_us"] / 1e3 / FILTER_COUNT_RATE_G, 4)
            v["fraction_of_assign"] = round(pw / v["avg_us"] / 1e3 / ref, 4)
    res.setdefault("kernel_trace", {})[layout] = {"kernels": rows, "pair_words_per_walk": pw, "vc_filter_count_kernel_G": FILTER_COUNT_RATE_G,
                                                  "vc_assign_kernel_G": ref,
                                                  "how": "rocprofv3 --kernel-trace --stats over one --step of --only <layout> (a run of its own, warm-up included)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e6)
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--cluster-size", type=int, default=16, help="records per centre of the synthetic data")
    ap.add_argument("--flips", type=int, default=6, help="a record is its centre with up to this many bits flipped")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=35, help="of the synthetic data and the layouts")
    ap.add_argument("--only", default="all", help="one layout alone, without the loop (for a profiler run): 1, 16, 64, 256, 4096, 65536 or skewed")
    ap.add_argument("--loop", action="store_true", help="with --only: time the loop as well")
    ap.add_argument("--step-timeout", type=int, default=900, help="seconds the measurement may take")
    ap.add_argument("--trace-csv", default=None, help="the *_kernel_stats.csv of a rocprofv3 run of one --step --only <layout>: merged into --out")
    ap.add_argument("--trace-layout", default="equal 64")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--step-out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    if args.trace_csv:
        line = json.load(open(args.out))
        merge_trace(args.trace_csv, line["run"], args.trace_layout)
        with open(args.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
        return print(json.dumps(line))
    line = {"metric": "vc_search_knn_scoped_dev (k = %d) against the loop of vc_search_knn_filtered_dev(VC_FILTER_EQUAL, VC_MODE_LINEAR), one call per distinct "
                      "query scope, on the same handle; %.3g clustered 64-bit codes (%d per centre, <= %d flips), %d resident queries, one engine; equal "
                      "scopes U = 1 .. 65536 and one skewed layout; not measured: the sharded and host forms, other widths, N and k, more than one GPU"
                      % (args.k, args.n, args.cluster_size, args.flips, args.nq)}
    with tempfile.TemporaryDirectory() as td:
        part = os.path.join(td, "run.json")
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", "--step-out", part, "--only", args.only]
        if args.loop:
            cmd.append("--loop")
        for key in ("n", "nq", "k", "cluster_size", "flips", "reps", "seed"):
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
