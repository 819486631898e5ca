"""vc_update_index against the only way there was before it, vc_build_index, both from the SAME stale state: an engine with an MIH
index over n clustered 128-bit codes (n/1000 centres, <= 11 flips, m = 4) to which delta records were then added.

A state cannot be rewound (records are only ever appended), so every repetition makes its own: create, add n, build, add delta --
then ONE timed call, a host clock around it (both calls end in a stream synchronise).  The two legs alternate, one warm-up state
each per delta, then --reps repetitions; median, interquartile range and full range per leg.  The whole sweep runs once per --bent setting
(VC_MIH_BENT is read at vc_create).  Bytes by the formulas of DESIGN.md 4.3.2.  Prints one JSON line (and writes it to --out).

    python tools/bench_update.py [--n 1e8] [--deltas 1e4,1e6,1e7] [--reps 9] [--bent auto,0] [--out profiles/index_update_bench.json]
    python tools/bench_update.py --one --n 1e8 --deltas 1e6      # one state, one update: the run to put under a kernel trace
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
    print("[bench_update] %s" % what, file=sys.stderr, flush=True)


def stale_state(vc, n, delta, seed):
    e = vc.Engine(BITS, capacity=n + delta, n_tables=M)
    e.add_synthetic(n, seed=seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // 1000, 1), max_flips=11)
    e.build_index()
    e.add_synthetic(delta, seed=seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // 1000, 1), max_flips=11)
    return e


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def bytes_moved(n, delta, bent):
    """per table, by DESIGN.md 4.3.2: the merge reads and writes ids[] (and the 16 W-byte records) once; the rebuild moves every
    (key, id) pair in and out of each of the four 8-bit radix passes and gathers the records again"""
    total = n + delta
    merge = 2 * 4 * total + (2 * 16 * W * total if bent else 0) + 4 * 8 * delta * 2
    rebuild = 4 * 2 * 8 * total + ((4 + 8 * W + 16 * W) * total if bent else 0)
    return {"merge_bytes_per_table": merge, "rebuild_bytes_per_table": rebuild}


def summary(ms):
    """median, the full range, and the interquartile range: a repetition allocates and frees tens of GB, and single runs of EITHER
    leg stall for 0.1 .. 5 s while the driver reclaims what the previous repetition's engine returned -- the range shows those
    stalls, the interquartile range is the spread of the runs without them"""
    q = statistics.quantiles(ms, n=4, method="inclusive")
    return {"median_ms": statistics.median(ms), "iqr_ms": q[2] - q[0], "min_ms": min(ms), "max_ms": max(ms), "runs_ms": [round(x, 3) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e8)
    ap.add_argument("--deltas", default="1e4,1e6,1e7")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--bent", default="auto,0")
    ap.add_argument("--seed", type=int, default=34)
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("VC_STRIDE_TRIES", "1")                 # (the column-stride probe of vc_create is not what is measured)
    import torch
    from verticut_amd import engine as vc
    n = int(args.n)
    deltas = [int(float(d)) for d in args.deltas.split(",")]

    if args.one:
        e = stale_state(vc, n, deltas[0], args.seed)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        ms = timed(e.update_index)
        print(json.dumps({"n": n, "delta": deltas[0], "update_ms": ms, "free_before": free0, "free_after": torch.cuda.mem_get_info()[0]}))
        e.close()
        return

    result = {"bench": "index_update", "bits": BITS, "n_tables": M, "n": n, "reps": args.reps, "device": torch.cuda.get_device_name(0), "sweeps": []}
    for bent in args.bent.split(","):
        if bent == "auto":
            os.environ.pop("VC_MIH_BENT", None)
        else:
            os.environ["VC_MIH_BENT"] = bent
        for delta in deltas:
            runs = {"update": [], "rebuild": []}
            for rep in range(-1, args.reps):                      # rep -1: the warm-up of both legs
                for leg in ("update", "rebuild"):
                    e = stale_state(vc, n, delta, args.seed)
                    torch.cuda.synchronize()
                    time.sleep(0.25)                              # (let the driver finish reclaiming the previous state's memory)
                    ms = timed(e.update_index if leg == "update" else e.build_index)
                    e.close()
                    if rep >= 0:
                        runs[leg].append(ms)
            row = {"bent": bent, "delta": delta, "update": summary(runs["update"]), "rebuild": summary(runs["rebuild"])}
            row.update(bytes_moved(n, delta, bent != "0"))
            gain = row["rebuild"]["median_ms"] - row["update"]["median_ms"]
            spread = row["rebuild"]["iqr_ms"]
            row["update_faster_by_more_than_rebuild_iqr"] = gain > spread
            row["update_faster_by_more_than_rebuild_range"] = gain > row["rebuild"]["max_ms"] - row["rebuild"]["min_ms"]
            note("bent=%s delta=%d update %.1f ms rebuild %.1f ms (iqr %.1f)" % (bent, delta, row["update"]["median_ms"],
                                                                                    row["rebuild"]["median_ms"], spread))
            result["sweeps"].append(row)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
