"""A built k-NN graph brought up to date after a removal (vc_retain_dev + vc_knn_graph_retain_dev) against what a caller must do
without it, vc_retain_dev + the build over the whole store (vc_knn_graph_dev): the store of tools/bench_knn_graph.py -- 1e6 clustered
64-bit codes (16 per centre, up to 6 flipped bits), m = 2, exact MIH, batches of 4 096 ids, one engine -- at k = 10 and k = 100, with
0.1 %, 1 % and 10 % of the records removed at random, and the dedup case: VC_RETAIN_ROOTS on the labels of vc_cluster_radius_dev at
R = 8, which keeps one record per group.

Per k one child process under its own `timeout`, the next only after the one before succeeded.  The child builds the graph of the whole
store once and keeps it in HBM.  Per case and repetition, on a FRESH handle with the same records (vc_retain* cannot be undone), whose search and graph
buffers one batch of vc_knn_graph_dev has warmed:
  1. retain     vc_retain_dev with the map                                                                            (timed)
  2. translate  vc_knn_graph_retain_dev on a graph in which every entry of a removed record was replaced by the nearest surviving id
                below it, so that no row is short and nothing is searched: the translate pass alone, with the real graph's traffic;
                twice, the first run warms the call's own buffers                                                     (the second timed)
  3. carry      the old rows and counts copied into the work buffer (not timed), then vc_knn_graph_retain_dev in VC_MODE_MIH_EXACT (timed)
  4. rebuild    vc_knn_graph_dev over the K survivors into a second buffer                                            (timed)
A host clock around each leg ending in a device synchronise; the first repetition is the warm-up, in which rows and counts [0, K) of
the two buffers are asserted equal; medians of --reps with min .. max.  NO SPEED-UP IS ASSERTED: the figures say where the call pays
(retain + carry below retain + rebuild) and where it stops paying.

Per case: S / K (n_rows_short / n_rows_kept) beside 1 - (1 - f)^k; the bytes the translate pass moves -- n_old k 8 read, K k 8 written
twice, K k 4 of gathers (and K k 8 read by the copy back, listed apart) -- and their rate as a share of the 8 TB/s HBM peak.

Not measured: other widths, the sharded forms, the host form, VC_MODE_LINEAR, other knobs than the defaults.

    python tools/bench_knn_graph_retain.py [--n 1e6] [--ks 10,100] [--fractions 0.001,0.01,0.1] [--reps 5] [--out profiles/knn_graph_retain_bench.json]
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

HBM_PEAK = 8e12          # bytes/s
DEDUP_RADIUS = 8


def step(args):
    import torch
    from verticut_amd import engine as vc
    n, bits, m, B, k = int(args.n), 64, 2, args.batch, args.k
    fractions = [float(x) for x in args.fractions.split(",")]

    def note(what):
        print("[bench_knn_graph_retain k=%d] %s" % (k, what), file=sys.stderr, flush=True)

    def fresh():
        e = vc.Engine(bits, capacity=n, n_tables=m, flags=vc.FLAG_LEAN_TIMING)
        e.add_synthetic(n, seed=args.seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // args.cluster_size, 1), max_flips=args.flips)
        e.build_index()
        return e

    e = fresh()
    st = torch.cuda.current_stream().cuda_stream
    d_old = torch.empty((n, k), dtype=torch.int64, device="cuda")
    d_old_counts = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_rows = torch.empty((n, k), dtype=torch.int64, device="cuda")
    d_counts = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_rows2 = torch.empty((n, k), dtype=torch.int64, device="cuda")
    d_counts2 = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_map = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_labels = torch.empty((n,), dtype=torch.int32, device="cuda")
    t0 = time.perf_counter()
    e.knn_graph_dev(k, d_old.data_ptr(), d_old_counts.data_ptr(), mode=vc.MODE_MIH_EXACT, batch=B, stream=st)
    torch.cuda.synchronize()
    build_old_ms = (time.perf_counter() - t0) * 1e3
    e.cluster_radius_dev(DEDUP_RADIUS, d_labels.data_ptr(), mode=vc.MODE_MIH_EXACT, batch=B, stream=st)
    torch.cuda.synchronize()
    note("engine, the graph of the %d records (%.0f ms) and the labels at R = %d built" % (n, build_old_ms, DEDUP_RADIUS))
    rng = np.random.default_rng(args.seed)
    cases = []
    for f in fractions:
        keep = np.ones(n, dtype=np.int32)
        keep[rng.choice(n, size=int(round(f * n)), replace=False)] = 0
        cases.append(("random %g" % f, f, torch.from_numpy(keep).cuda(), vc.RETAIN_MASK))
    cases.append(("dedup R=%d" % DEDUP_RADIUS, None, d_labels, vc.RETAIN_ROOTS))
    res = {"build_of_the_old_graph_ms": round(build_old_ms, 1)}
    for name, f, d_sel, kind in cases:
        t = {"retain": [], "carry": [], "rebuild": [], "translate_alone": []}
        stats = K = d_fake = None
        for rep in range(args.reps + 1):
            e.close()
            e = fresh()
            e.knn_graph_dev(k, d_rows2.data_ptr(), d_counts2.data_ptr(), mode=vc.MODE_MIH_EXACT, batch=B, count=B, stream=st)   # warms the search's and the graph's buffers
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            K = e.retain_dev(d_sel.data_ptr(), kind, d_map.data_ptr(), stream=st)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if rep == 0:
                # the graph of step 5: a removed id becomes the nearest surviving id below it (the first survivor for the ids before it)
                live = d_map.cpu().numpy() != -1
                near = np.maximum.accumulate(np.where(live, np.arange(n), -1))
                near[near < 0] = int(np.argmax(live))
                ids = d_old & 0xFFFFFFFF
                d_fake = (d_old - ids) + torch.from_numpy(near).cuda()[ids]
                del ids
            for again in range(2):      # the first of the two warms this call's own buffers and is not timed
                d_rows.copy_(d_fake)
                d_counts.copy_(d_old_counts)
                torch.cuda.synchronize()
                t4 = time.perf_counter()
                alone = e.knn_graph_retain_dev(k, n, d_map.data_ptr(), d_rows.data_ptr(), d_counts.data_ptr(), mode=vc.MODE_MIH_EXACT, batch=B, stream=st)
                torch.cuda.synchronize()
                t5 = time.perf_counter()
                assert alone["n_rows_short"] == 0 and alone["repair"]["n_searched"] == 0 and alone["n_rows_kept"] == K
            d_rows.copy_(d_old)
            d_counts.copy_(d_old_counts)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            stats = e.knn_graph_retain_dev(k, n, d_map.data_ptr(), d_rows.data_ptr(), d_counts.data_ptr(), mode=vc.MODE_MIH_EXACT, batch=B, stream=st)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            e.knn_graph_dev(k, d_rows2.data_ptr(), d_counts2.data_ptr(), mode=vc.MODE_MIH_EXACT, batch=B, stream=st)
            torch.cuda.synchronize()
            t6 = time.perf_counter()
            if rep == 0:      # the warm-up: the words are compared
                assert K == len(e) == stats["n_rows_kept"]
                assert torch.equal(d_rows[:K], d_rows2[:K]), "the carried rows differ from the build over the survivors"
                assert torch.equal(d_counts[:K], d_counts2[:K]), "the carried counts differ from the build over the survivors"
                note("%s: K = %d, rows and counts equal the build from scratch: %s" % (name, K, stats))
            if rep:
                for leg, dt in (("retain", t1 - t0), ("carry", t3 - t2), ("rebuild", t6 - t3), ("translate_alone", t5 - t4)):
                    t[leg].append(dt)
        med = {q: round(float(np.median(v)) * 1e3, 3) for q, v in t.items()}
        moved = n * k * 8 + 2 * K * k * 8 + K * k * 4
        one = {"fraction_removed": f if f is not None else round(1 - K / n, 6), "K": K, "stats": stats, "rows_and_counts_equal_rebuild": True,
               "S_over_K": round(stats["n_rows_short"] / K, 5), "S_over_K_expected_for_random": round(1 - (1 - f) ** k, 5) if f is not None else None,
               "call_ms_median": med, "call_ms_min": {q: round(min(v) * 1e3, 3) for q, v in t.items()},
               "call_ms_max": {q: round(max(v) * 1e3, 3) for q, v in t.items()}, "reps": args.reps,
               "retain_plus_carry_ms": round(med["retain"] + med["carry"], 3), "retain_plus_rebuild_ms": round(med["retain"] + med["rebuild"], 3),
               "new_over_today": round((med["retain"] + med["carry"]) / (med["retain"] + med["rebuild"]), 5),
               "carry_over_rebuild": round(med["carry"] / med["rebuild"], 5),
               "expected_carry_ms_S_over_K_times_rebuild_plus_translate": round(stats["n_rows_short"] / K * med["rebuild"] + med["translate_alone"], 3),
               "translate_bytes": {"old_rows_read": n * k * 8, "new_rows_written_twice": 2 * K * k * 8, "gathers": K * k * 4, "total": moved,
                                   "copy_back_read_listed_apart": K * k * 8},
               "translate_TB_per_s": round(moved / (med["translate_alone"] / 1e3) / 1e12, 4),
               "translate_share_of_hbm_peak": round(moved / (med["translate_alone"] / 1e3) / HBM_PEAK, 4)}
        note("%s timed: %s" % (name, one))
        res[name] = one
        del d_fake
    with open(args.step_out, "w") as f:
        json.dump(res, f)
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e6)
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--fractions", default="0.001,0.01,0.1")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--cluster-size", type=int, default=16, help="records per centre of the synthetic data")
    ap.add_argument("--flips", type=int, default=6, help="a record is its centre with up to this many bits flipped")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=35)
    ap.add_argument("--step-timeout", type=int, default=500, help="seconds a step may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=("time",), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--step-out", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--k", type=int, default=10, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    line = {"metric": "vc_retain_dev + vc_knn_graph_retain_dev against vc_retain_dev + vc_knn_graph_dev over the survivors, %.3g clustered 64-bit codes "
                      "(%d per centre, <= %d flips), m=2, exact MIH, batches of %d ids, the default VC_KGRAPH_SCRATCH, one engine; ms, medians of %d after a "
                      "warm-up in which rows and counts were asserted equal" % (args.n, args.cluster_size, args.flips, args.batch, args.reps),
            "hbm_peak_bytes_per_s": HBM_PEAK}
    with tempfile.TemporaryDirectory() as td:
        for k in [int(x) for x in args.ks.split(",")]:
            part = os.path.join(td, "time_%d.json" % k)      # chained: a step that fails, faults or runs into its time limit ends the run
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", "time", "--step-out", part, "--k", str(k)]
            for key in ("n", "fractions", "batch", "cluster_size", "flips", "reps", "seed"):
                cmd += ["--" + key.replace("_", "-"), str(getattr(args, key))]
            rc = subprocess.call(cmd)
            if rc != 0:
                raise SystemExit("the step at k=%d ended with status %d: nothing further is started" % (k, rc))
            line["k=%d" % k] = json.load(open(part))
            if args.out:                                     # what is measured is safe before the next step starts
                with open(args.out, "w") as f:
                    f.write(json.dumps(line, indent=1) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
