"""vc_retain_dev with the index FILTERED to the survivors (the default) against the same call taking a full vc_build_index afterwards
(VC_MIH_RETAIN=0), both from the SAME state: an engine with a current MIH index over n clustered 128-bit codes (n/1000 centres,
<= 11 flips, m = 4) and a seeded keep mask in device memory that removes a fraction of the records.

A state cannot be rewound, so every repetition makes its own: create, add n, build -- then ONE timed call, a host clock around it
(the call waits inside).  The two legs alternate, one warm-up state each per fraction, then --reps repetitions; median,
interquartile range and full range per leg.  VC_MIH_RETAIN is read at vc_create.  Prints one JSON line (and writes it to --out).

    python tools/bench_retain.py [--n 1e8] [--fractions 0.01,0.5] [--reps 5] [--out profiles/retain_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BITS, M, W = 128, 4, 2


def note(what):
    print("[bench_retain] %s" % what, file=sys.stderr, flush=True)


def summary(ms):
    q = statistics.quantiles(ms, n=4, method="inclusive") if len(ms) > 1 else [ms[0]] * 3
    return {"median_ms": statistics.median(ms), "iqr_ms": q[2] - q[0], "min_ms": min(ms), "max_ms": max(ms), "runs_ms": [round(x, 3) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e8)
    ap.add_argument("--fractions", default="0.01,0.5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=34)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("VC_STRIDE_TRIES", "1")                 # (the column-stride probe of vc_create is not what is measured)
    import torch
    from verticut_amd import engine as vc
    n = int(args.n)
    result = {"bench": "retain", "bits": BITS, "n_tables": M, "n": n, "reps": args.reps, "device": torch.cuda.get_device_name(0), "sweeps": []}
    gen = torch.Generator(device="cuda")
    for frac in [float(f) for f in args.fractions.split(",")]:
        gen.manual_seed(args.seed)
        d_sel = (torch.rand(n, device="cuda", generator=gen) >= frac).to(torch.int32)
        kept_expect = int(d_sel.sum().item())
        runs = {"filter": [], "rebuild": []}
        for rep in range(-1, args.reps):                          # rep -1: the warm-up of both legs
            for leg in ("filter", "rebuild"):
                if leg == "filter":
                    os.environ.pop("VC_MIH_RETAIN", None)
                else:
                    os.environ["VC_MIH_RETAIN"] = "0"
                e = vc.Engine(BITS, capacity=n, n_tables=M)
                e.add_synthetic(n, seed=args.seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // 1000, 1), max_flips=11)
                e.build_index()
                torch.cuda.synchronize()
                time.sleep(0.25)                                  # (let the driver finish reclaiming the previous state's memory)
                t0 = time.perf_counter()
                kept = e.retain_dev(d_sel.data_ptr())
                ms = (time.perf_counter() - t0) * 1e3
                assert kept == kept_expect == len(e)
                e.close()
                if rep >= 0:
                    runs[leg].append(ms)
        row = {"removed_fraction": frac, "kept": kept_expect, "filter": summary(runs["filter"]), "rebuild": summary(runs["rebuild"])}
        # per table: the filter reads ids[] and writes the survivors' (flags + scan in between: 3 x 4 n), the records likewise; the
        # rebuild moves every surviving (key, id) pair through four radix passes and gathers the records again
        row["filter_bytes_per_table"] = 4 * n + 4 * kept_expect + 3 * 4 * n + 16 * W * (n + kept_expect)
        row["rebuild_bytes_per_table"] = 4 * 2 * 8 * kept_expect + (4 + 8 * W + 16 * W) * kept_expect
        note("removed %.2f: filter %.1f ms, rebuild %.1f ms (iqr %.1f)" % (frac, row["filter"]["median_ms"], row["rebuild"]["median_ms"], row["rebuild"]["iqr_ms"]))
        result["sweeps"].append(row)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
