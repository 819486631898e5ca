"""DBSCAN at every radius 0 .. R from one walk (vc_dbscan_levels_dev) against what it replaces, a loop of vc_dbscan_radius_dev calls,
on tools/bench_dbscan.py's data and parameters: clustered synthetic 64-bit codes, R = 8, m = 2, exact MIH, one engine, 1e6 records in
62 500 clusters of about 16, batches of 4 096 ids, min_pts = 4.

  levels       vc_dbscan_levels_dev at max_radius = R: per batch fill ids, gather, radius search at R, the batch's core distances, one
               edge launch that puts a pair into the forest of max(distance, both core distances), lowers the anchor candidates and
               counts the pair; then R cascade launches and one finish pass over all levels
  dbscan_R     ONE vc_dbscan_radius_dev at radius R on the same handle (existing code): the same batches and searches
  loop         vc_dbscan_radius_dev at r = 0, 1, .. R: R + 1 walks -- what a caller runs today to see every level

Two steps, each a child process under its own `timeout`, the second only after the first succeeded:
  check   level r of `levels` == the labels of vc_dbscan_radius_dev(r, min_pts) for every r = 0 .. R, core_dist <= r exactly where its
          degrees reach min_pts, all five statistics equal (all asserted); written down: the five counter rows
  time    the three legs interleaved, a host clock around each leg ending in a device synchronise, medians of --reps
No time is fixed in advance.  levels / loop below 1 is what justifies the call; the walks at small r are cheaper than the one at R,
so the factor is not R + 1.  levels / dbscan_R is the price of the core distances, the per-level select, the histogram, the cascade
and the finish pass over R + 1 levels; a value near 2 would mean a hidden second walk.  Prints one JSON line; --out also writes it.

    python tools/bench_dbscan_levels.py [--n 1e6] [--reps 7] [--out profiles/dbscan_levels_bench.json]
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

FIELDS = ("n_pairs", "n_clusters", "n_core", "n_border", "n_noise")


def step(args):
    import torch
    from verticut_amd import engine as vc
    n, bits, m, B, R, min_pts = int(args.n), 64, 2, args.batch, args.radius, args.min_pts
    mode = vc.MODE_MIH_EXACT

    def note(what):
        print("[bench_dbscan_levels] %s" % what, file=sys.stderr, flush=True)

    e = vc.Engine(bits, capacity=n, n_tables=m, flags=vc.FLAG_LEAN_TIMING)
    e.add_synthetic(n, seed=args.seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // args.cluster_size, 1), max_flips=args.flips)
    e.build_index()
    note("engine built")
    st = torch.cuda.current_stream().cuda_stream
    d_levels = torch.empty((R + 1, n), dtype=torch.int32, device="cuda")
    d_core = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_labels = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_degrees = torch.empty((n,), dtype=torch.int32, device="cuda")
    batches = (n + B - 1) // B

    def leg_levels():
        return e.dbscan_levels_dev(R, min_pts, d_levels.data_ptr(), d_core.data_ptr(), mode=mode, batch=B, stream=st)

    def leg_dbscan(r=R):
        return e.dbscan_radius_dev(r, min_pts, d_labels.data_ptr(), d_degrees.data_ptr(), mode=mode, batch=B, stream=st)

    def leg_loop():
        return [leg_dbscan(r) for r in range(R + 1)]

    if args.step == "check":
        stats = leg_levels()
        torch.cuda.synchronize()
        levels = d_levels.cpu().numpy().view(np.uint32)
        core = d_core.cpu().numpy().view(np.uint32)
        for r in range(R + 1):
            st_r = leg_dbscan(r)
            torch.cuda.synchronize()
            assert np.array_equal(levels[r], d_labels.cpu().numpy().view(np.uint32)), "level %d differs from vc_dbscan_radius_dev(%d)" % (r, r)
            assert np.array_equal(core <= r, d_degrees.cpu().numpy().view(np.uint32) >= min_pts), "level %d: core_dist <= r is not degrees >= min_pts" % r
            got = {f: int(stats[f][r]) for f in FIELDS[1:]}
            got["n_pairs"] = int(stats["n_pairs"][:r + 1].sum())
            assert got == st_r, "level %d: statistics %s, vc_dbscan_radius_dev gives %s" % (r, got, st_r)
        res = {"every_level_equals_dbscan_radius": True, "levels": R + 1, "batches": batches, "min_pts": min_pts,
               "core_never": int(np.count_nonzero(core == vc.CORE_NEVER))}
        res.update({f: [int(x) for x in stats[f]] for f in FIELDS})
        note("levels equal: %s" % res)
    else:
        legs = {"levels": leg_levels, "dbscan_R": leg_dbscan, "loop": leg_loop}
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
        res = {"call_ms_median": {k: round(float(np.median(v)) * 1e3, 3) for k, v in t.items()},
               "call_ms_min": {k: round(min(v) * 1e3, 3) for k, v in t.items()},
               "call_ms_max": {k: round(max(v) * 1e3, 3) for k, v in t.items()}, "reps": args.reps, "batches": batches}
        med = res["call_ms_median"]
        res["levels_over_loop"] = round(med["levels"] / med["loop"], 3)
        res["levels_over_dbscan_R"] = round(med["levels"] / med["dbscan_R"], 3)
        res["extra_us_per_batch"] = round((med["levels"] - med["dbscan_R"]) * 1e3 / batches, 1)
        note("timed: %s" % res)
    with open(args.step_out, "w") as f:
        json.dump(res, f)
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e6)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--radius", type=int, default=8, help="max_radius of the levels call, the last radius of the loop")
    ap.add_argument("--min-pts", type=int, default=4)
    ap.add_argument("--cluster-size", type=int, default=16, help="records per centre of the synthetic data")
    ap.add_argument("--flips", type=int, default=6, help="a record is its centre with up to this many bits flipped")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=35)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a step may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=("check", "time"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--step-out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    line = {"metric": "DBSCAN at every radius 0 .. %d from one walk against %d calls of vc_dbscan_radius_dev, min_pts %d, %.3g clustered 64-bit "
                      "codes (%d per centre, <= %d flips), m=2, exact MIH, batches of %d ids, one engine"
                      % (args.radius, args.radius + 1, args.min_pts, args.n, args.cluster_size, args.flips, args.batch)}
    with tempfile.TemporaryDirectory() as td:
        for name in ("check", "time"):      # chained: a step that fails, faults or runs into its time limit ends the run
            part = os.path.join(td, name + ".json")
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--step-out", part]
            for k in ("n", "batch", "radius", "min_pts", "cluster_size", "flips", "reps", "seed"):
                cmd += ["--" + k.replace("_", "-"), str(getattr(args, k))]
            rc = subprocess.call(cmd)
            if rc != 0:
                raise SystemExit("step %s ended with status %d: nothing further is started" % (name, rc))
            line[name] = json.load(open(part))
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
