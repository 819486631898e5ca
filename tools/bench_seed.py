"""Device-side seeding (vc_seed_centres_dev) on the store of the clustering benches -- clustered synthetic codes, one engine, 1e6
records, at 64 and at 128 bits, K = 4096 -- against the host path it replaces, and what the seeds do to vc_kmajority_dev.

  seed        vc_seed_centres_dev, VC_SEED_FARTHEST and VC_SEED_WEIGHTED, K = 4096, picks and assign asked for, stats NULL (the host
              waits for nothing); total time and microseconds per round
  host        the path replaced: every code copied home (vc_get_codes_dev of all ids, then the device-to-host copy), then the numpy model
              of the rule (tests/seed_common.py: per round one pass over the N records).  Run at K = --host-k (64) only and reported per
              round; a figure for K = 4096 is EXTRAPOLATED from it (rounds cost the same: each is one pass), not run.  The device
              form's outputs at the same K are asserted equal to the model's, every word, in the same run
  kmajority   vc_kmajority_dev (max_iters = --rounds) from three seedings: the default of Engine.kmajority (ids spread evenly over the
              store), farthest, weighted: cost_final, n_empty, n_iters, time

A host clock around each leg ending in a device synchronise, legs alternated, medians of --reps with min and max as the spread.  No
time or ratio is fixed in advance.

--trace-csv merges the kernel times of a `rocprofv3 --kernel-trace --stats --output-format csv` run of the seeding legs alone (a run
of its own: `rocprofv3 ... -- python tools/bench_seed.py --step --only seed --bits 64 --step-out X`) into that width of --out: the
time of a round launch, and the bytes a round moves -- N x bits / 8 of codes and 8 N of best read, the changed words of best written
(not counted: at most 8 N) -- over it, against the 8 TB/s HBM peak.  At these sizes codes and best (16 and 24 MB) fit the Infinity
Cache, so that share says how far the launch is from a streaming kernel, not where the bytes came from.

Each width is one child process under its own `timeout`; nothing is repeated after a failure.  Prints one JSON line; --out also
writes it.  Not measured: the sharded forms, other N and K, more than one GPU.

    python tools/bench_seed.py [--n 1e6] [--k 4096] [--reps 7] [--out profiles/seed_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK_GBS = 8000.0
WIDTHS = [64, 128]
METHODS = (("farthest", 0), ("weighted", 1))


def step(args):
    import torch
    import seed_common as SC
    from verticut_amd import engine as vc
    n, bits, k, hk = int(args.n), args.bits, args.k, args.host_k
    nbytes, words = bits // 8, bits // 64

    def note(what):
        print("[bench_seed %d] %s" % (bits, what), file=sys.stderr, flush=True)

    e = vc.Engine(bits, capacity=n, flags=vc.FLAG_LEAN_TIMING)
    e.add_synthetic(n, seed=args.seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // args.cluster_size, 1), max_flips=args.flips)
    st = torch.cuda.current_stream().cuda_stream
    i32, i64 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.int64, device="cuda")
    d_cen = {name: torch.empty((k * words,), **i64) for name, _ in METHODS}
    d_picks, d_assign = torch.empty((k,), **i64), torch.empty((n,), **i64)
    d_all, d_codes = torch.arange(n, **i32), torch.empty((n, words), **i64)
    res = {"bits": bits, "k": k, "n": n, "seed": args.rng_seed}

    def leg_seed(name, method, kk=k):
        e.seed_centres_dev(kk, d_cen[name].data_ptr(), d_picks.data_ptr(), d_assign.data_ptr(), method=method, seed=args.rng_seed, with_stats=False, stream=st)

    legs = {"seed_" + name: (lambda name=name, method=method: leg_seed(name, method)) for name, method in METHODS}
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    note("engine built, first seeding calls done")

    if args.only != "seed":
        # the host path, once per method at K = host_k, its outputs against the device form's at the same K
        host = {}
        for name, method in METHODS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.get_codes_dev(d_all.data_ptr(), n, d_codes.data_ptr(), stream=st)
            codes = d_codes.cpu().numpy().view(np.uint8).reshape(n, nbytes)
            t1 = time.perf_counter()
            want = SC.seed_model(codes, hk, method, args.rng_seed, e.id_base)
            t2 = time.perf_counter()
            stats = e.seed_centres_dev(hk, d_cen[name].data_ptr(), d_picks.data_ptr(), d_assign.data_ptr(), method=method, seed=args.rng_seed, stream=st)
            torch.cuda.synchronize()
            got = (d_cen[name][:hk * words].cpu().numpy().view(np.uint8).reshape(hk, nbytes), d_picks[:hk].cpu().numpy().view(np.uint64),
                   d_assign.cpu().numpy().view(np.uint64), stats)
            SC.same_run(got, want, (bits, name))
            host[name] = {"k": hk, "copy_home_ms": round((t1 - t0) * 1e3, 2), "model_ms": round((t2 - t1) * 1e3, 2),
                          "model_ms_per_round": round((t2 - t1) * 1e3 / hk, 3), "equals_device_form": True,
                          "extrapolated_ms_at_k": round((t1 - t0) * 1e3 + (t2 - t1) * 1e3 / hk * k, 1)}
            note("host path %s: %s" % (name, host[name]))
        res["host_path"] = host
        res["host_path_note"] = "run at K = %d and reported per round; extrapolated_ms_at_k = copy_home_ms + model_ms_per_round x %d was NOT run" % (hk, k)
        # k-majority from three seedings
        d_seeds, d_lab = torch.empty((k * words,), **i64), torch.empty((n,), **i32)
        spread = torch.from_numpy((np.arange(k, dtype=np.int64) * n // k).astype(np.int32)).cuda()
        d_spread = torch.empty((k * words,), **i64)
        e.get_codes_dev(spread.data_ptr(), k, d_spread.data_ptr(), stream=st)
        for name, _ in METHODS:
            legs["seed_" + name]()
        torch.cuda.synchronize()
        sources, km = {"spread_ids": d_spread, "farthest": d_cen["farthest"].clone(), "weighted": d_cen["weighted"].clone()}, {}

        def leg_km(name):
            d_seeds.copy_(sources[name])
            km[name] = e.kmajority_dev(k, d_seeds.data_ptr(), d_assign.data_ptr(), d_lab.data_ptr(), max_iters=args.rounds, stream=st)

        for name in sources:
            legs["kmajority_from_" + name] = lambda name=name: leg_km(name)

    for fn in legs.values():
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
    res.update({"call_ms_median": {key: round(float(np.median(v)) * 1e3, 4) for key, v in t.items()},
                "call_ms_min": {key: round(min(v) * 1e3, 4) for key, v in t.items()},
                "call_ms_max": {key: round(max(v) * 1e3, 4) for key, v in t.items()}, "reps": args.reps})
    res["us_per_round"] = {name: round(res["call_ms_median"]["seed_" + name] * 1e3 / k, 3) for name, _ in METHODS}
    res["launches_per_call"] = {"farthest": k + 2, "weighted": 2 * k + 1}
    if args.only != "seed":
        res["seed_stats"] = {name: e.seed_centres_dev(k, d_cen[name].data_ptr(), None, None, method=method, seed=args.rng_seed, stream=st) for name, method in METHODS}
        res["kmajority"] = {name: {"max_iters": args.rounds, "n_iters": int(s["n_iters"]), "converged": int(s["converged"]), "n_empty": int(s["n_empty"]),
                                   "cost_first_round": int(s["cost"][0]), "cost_final": int(s["cost_final"]),
                                   "call_ms_median": res["call_ms_median"]["kmajority_from_" + name]} for name, s in km.items()}
        res["seeding_over_kmajority"] = {name: round(res["call_ms_median"]["seed_" + name] / res["call_ms_median"]["kmajority_from_" + name], 3) for name, _ in METHODS}
    note("timed: %s" % res)
    with open(args.step_out, "w") as f:
        json.dump(res, f)
    e.close()


def merge_trace(path, res):
    """the kernel statistics (csv) of a `rocprofv3 --kernel-trace --stats` run of one --step of --only seed -> the round launch's time
    and its bytes against the HBM peak"""
    rows = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "vc_seed_" in row["Name"]:
                rows[row["Name"]] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 3), "min_us": round(float(row["MinNs"]) / 1e3, 3),
                                     "max_us": round(float(row["MaxNs"]) / 1e3, 3)}
    n, bits = res["n"], res["bits"]
    rnd = next(v for key, v in rows.items() if "vc_seed_round_kernel" in key)
    bytes_round = n * bits // 8 + 8 * n
    res["kernel_trace"] = {"kernels": rows, "round_bytes_read": bytes_round, "round_gb_per_s": round(bytes_round / (rnd["avg_us"] * 1e-6) / 1e9, 1),
                           "share_of_hbm_peak": round(bytes_round / (rnd["avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4), "hbm_peak_gb_per_s": HBM_PEAK_GBS,
                           "how": "rocprofv3 --kernel-trace --stats over one --step of --only seed (a run of its own, first calls included); bytes = the codes "
                                  "and best read once per round (the changed words written are not counted); both fit the Infinity Cache at this size"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e6)
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--host-k", type=int, default=64, help="K of the host path (it is reported per round)")
    ap.add_argument("--cluster-size", type=int, default=16, help="records per centre of the synthetic data")
    ap.add_argument("--flips", type=int, default=6, help="a record is its centre with up to this many bits flipped")
    ap.add_argument("--rounds", type=int, default=10, help="max_iters of the k-majority legs")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=35, help="of the synthetic data")
    ap.add_argument("--rng-seed", type=int, default=1, help="the `seed` of vc_seed_centres_dev")
    ap.add_argument("--only", default="all", choices=("all", "seed"), help="seed: the seeding legs alone (for a profiler run)")
    ap.add_argument("--widths", default=None, help="bits,... (default %s)" % ",".join(str(b) for b in WIDTHS))
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds one width may take")
    ap.add_argument("--trace-csv", default=None, help="the *_kernel_stats.csv a rocprofv3 --kernel-trace --stats run of one --step of --only seed wrote, "
                                                     "with --trace-bits: merged into that width of --out")
    ap.add_argument("--trace-bits", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--step-out", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--bits", type=int, default=64, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    if args.trace_csv:
        line = json.load(open(args.out))
        merge_trace(args.trace_csv, next(sh for sh in line["widths"] if sh["bits"] == args.trace_bits))
        with open(args.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
        return print(json.dumps(line))
    widths = [int(x) for x in args.widths.split(",")] if args.widths else WIDTHS
    line = {"metric": "vc_seed_centres_dev (farthest-first and distance-weighted, K = %d) against the host path it replaces (all codes home + the numpy model, "
                      "run at K = %d, extrapolated beyond), and vc_kmajority_dev (%d rounds) from three seedings; %.3g clustered codes (%d per centre, <= %d "
                      "flips), one engine; not measured: the sharded forms, other N and K, more than one GPU" % (args.k, args.host_k, args.rounds, args.n, args.cluster_size, args.flips),
            "widths": []}
    with tempfile.TemporaryDirectory() as td:
        for bits in widths:
            part = os.path.join(td, "run_%d.json" % bits)
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", "--step-out", part, "--bits", str(bits),
                   "--only", args.only]
            for key in ("n", "k", "host_k", "cluster_size", "flips", "rounds", "reps", "seed", "rng_seed"):
                cmd += ["--" + key.replace("_", "-"), str(getattr(args, key))]
            rc = subprocess.call(cmd)
            if rc != 0:
                raise SystemExit("the run of width %d ended with status %d" % (bits, rc))
            line["widths"].append(json.load(open(part)))
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
