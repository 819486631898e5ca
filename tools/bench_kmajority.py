"""Nearest of K codes on the device (vc_assign_nearest_dev) against the path the library offered before it, and k-majority rounds
(vc_kmajority_dev), on the store of the clustering benches: clustered synthetic codes, one engine, 1e6 records, at 64 and at 128 bits,
K = 256 and 4096.  The centres are the centroids vc_group_summary_dev gives for a DBSCAN labelling (radius 8, min_pts 4, exact MIH) of
the same store, cut to K, or padded to K with the codes of records spread evenly over the store.

  assign      vc_assign_nearest_dev over all records
  knn1        the path replaced: a second handle holds the centres; per 4096 ids vc_get_codes_dev on the store, then
              vc_search_knn_dev(k = 1, VC_MODE_LINEAR) on the second handle
  kmajority   vc_kmajority_dev, max_iters = --rounds, seeded with the same centres

The outputs of `assign` and `knn1` are asserted equal in the same run, before anything is timed; the returned pair of `kmajority` is
asserted to satisfy assign == vc_assign_nearest(centres).  A host clock around each leg ending in a device synchronise, legs
alternated, medians of --reps with min and max as the spread.  No time or ratio is fixed in advance.

Kernel figures of vc_assign_kernel: pair-words (one record word against one centre word) per second over the call time of `assign`,
and the share of the VALU issue rate that follows from VALU_PER_PAIR_WORD -- the VALU instructions per pair-word counted by hand in
the saved ISA of the kernel (hipcc --save-temps), see the table below.  That rate is the bound: the HBM traffic is N x bits / 8
bytes once.  --trace-db merges the kernel times of a `rocprofv3 --kernel-trace --stats` run of the k-majority leg alone (a run of
its own: `rocprofv3 ... -- python tools/bench_kmajority.py --step --step-out X --bits 64 --k 4096 --only kmajority`) into the result:
the split of a call into assign, update (vc_groups_run's kernels, its sort, scans and gather), bookkeeping, and what is left of the
wall time -- host waits and launch gaps.

Each (bits, K) shape is one child process under its own `timeout`.  Prints one JSON line; --out also writes it.

    python tools/bench_kmajority.py [--n 1e6] [--reps 7] [--out profiles/kmajority_bench.json]
"""
import argparse
import json
import os
import sqlite3
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VALU_PEAK_GOPS = 39321.6   # bench.py's VALU_PEAK_GOPS: 256 CUs x 64 lanes x 2.4 GHz 32-bit lane-ops/s
# vc_assign_kernel's inner loop in the saved ISA (two centres per trip).  64 bits, 8 records per thread: 32 v_xor_b32, 32
# v_bcnt_u32_b32 (one chain of two per pair, the second with the accumulator operand), 16 v_cmp, 32 v_cndmask_b32, 3 v_mov_b32 (the
# two centre indices, the LDS address) = 115 for 16 pair-words.  128 bits, 4 records: 32 + 32 (a chain of two per 64-bit word), 8
# v_add_u32 joining a pair's two chains, 8 v_cmp, 16 v_cndmask, 3 v_mov = 99 for 16 pair-words.  (256 bits: 87 for 16, 512 bits: 159
# for 32 -- the compare / select share shrinks with the width.)
VALU_PER_PAIR_WORD = {64: 115 / 16, 128: 99 / 16}
SHAPES = [(64, 256), (64, 4096), (128, 256), (128, 4096)]
CHUNK = 4096


def step(args):
    import torch
    from verticut_amd import engine as vc
    n, bits, k = int(args.n), args.bits, args.k
    nbytes, m = bits // 8, bits // 32

    def note(what):
        print("[bench_kmajority %d/%d] %s" % (bits, k, what), file=sys.stderr, flush=True)

    e = vc.Engine(bits, capacity=n, n_tables=m, flags=vc.FLAG_LEAN_TIMING)
    e.add_synthetic(n, seed=args.seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // args.cluster_size, 1), max_flips=args.flips)
    e.build_index()
    st = torch.cuda.current_stream().cuda_stream
    i32, i64 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.int64, device="cuda")
    d_labels = torch.empty((n,), **i32)
    d_groups, d_cents = torch.empty((n, 6), **i32), torch.empty((n, bits // 32), **i32)
    d_all = torch.arange(n, **i32)
    e.dbscan_radius_dev(args.radius, args.min_pts, d_labels.data_ptr(), None, mode=vc.MODE_MIH_EXACT, batch=CHUNK, stream=st)
    rc, G = e.group_summary_dev(d_labels.data_ptr(), n, d_groups.data_ptr(), d_cents.data_ptr(), stream=st)
    assert rc == vc.VC_OK
    torch.cuda.synchronize()
    cents = d_cents[:G].cpu().numpy().view(np.uint8).reshape(G, nbytes)
    if G >= k:
        centres = cents[:k].copy()
    else:
        ids = torch.from_numpy((np.arange(k - G, dtype=np.int64) * n // (k - G)).astype(np.int32)).cuda()
        d_pad = torch.empty((k - G, bits // 32), **i32)
        e.get_codes_dev(ids.data_ptr(), k - G, d_pad.data_ptr(), stream=st)
        centres = np.concatenate([cents, d_pad.cpu().numpy().view(np.uint8).reshape(k - G, nbytes)])
    note("engine built, %d DBSCAN groups, %d centres" % (G, k))
    del d_groups, d_cents
    holder = vc.Engine(bits, capacity=k, id_base=0, flags=vc.FLAG_LEAN_TIMING)
    holder.add_codes(centres)
    d_centres = torch.from_numpy(centres.view(np.int64).reshape(-1).copy()).cuda()
    d_seeds = torch.empty_like(d_centres)
    d_a, d_b, d_c = torch.empty((n,), **i64), torch.empty((n,), **i64), torch.empty((n,), **i64)
    d_q = torch.empty((CHUNK, bits // 32), **i32)
    d_klab = torch.empty((n,), **i32)

    def leg_assign():
        e.assign_nearest_dev(d_centres.data_ptr(), k, 0, n, d_a.data_ptr(), stream=st)

    def leg_knn1():
        for pos in range(0, n, CHUNK):
            nq = min(CHUNK, n - pos)
            e.get_codes_dev(d_all.data_ptr() + 4 * pos, nq, d_q.data_ptr(), stream=st)
            holder.search_knn_dev(d_q.data_ptr(), nq, 1, d_b.data_ptr() + 8 * pos, mode=vc.MODE_LINEAR, stream=st)

    km = {}

    def leg_kmajority():
        d_seeds.copy_(d_centres)
        km["stats"] = e.kmajority_dev(k, d_seeds.data_ptr(), d_c.data_ptr(), d_klab.data_ptr(), max_iters=args.rounds, stream=st)

    legs = {"kmajority": leg_kmajority} if args.only == "kmajority" else {"assign": leg_assign, "knn1": leg_knn1, "kmajority": leg_kmajority}
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    res = {"bits": bits, "k": k, "n": n, "dbscan_groups": int(G)}
    if args.only != "kmajority":
        assert torch.equal(d_a, d_b), "vc_assign_nearest_dev differs from the k = 1 linear search over the centres"
        res["assign_equals_knn1"] = True
        e.assign_nearest_dev(d_seeds.data_ptr(), k, 0, n, d_a.data_ptr(), stream=st)
        torch.cuda.synchronize()
        assert torch.equal(d_a, d_c), "the assignment vc_kmajority_dev returned is not vc_assign_nearest of its centres"
        res["kmajority_pair_consistent"] = True
        note("outputs equal")
    t = {name: [] for name in legs}
    for _ in range(args.reps):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[name].append(time.perf_counter() - t0)
    stats = km["stats"]
    rounds = int(stats["n_iters"])
    res.update({"call_ms_median": {key: round(float(np.median(v)) * 1e3, 4) for key, v in t.items()},
                "call_ms_min": {key: round(min(v) * 1e3, 4) for key, v in t.items()},
                "call_ms_max": {key: round(max(v) * 1e3, 4) for key, v in t.items()}, "reps": args.reps,
                "kmajority": {"max_iters": args.rounds, "n_iters": rounds, "converged": int(stats["converged"]), "n_empty": int(stats["n_empty"]),
                              "cost": [int(x) for x in stats["cost"][:rounds]], "cost_final": int(stats["cost_final"]),
                              "n_changed": [int(x) for x in stats["n_changed"][:rounds]]}})
    med = res["call_ms_median"]
    res["kmajority"]["ms_per_round"] = round(med["kmajority"] / max(rounds, 1), 4)
    if "assign" in med:
        res["knn1_over_assign"] = round(med["knn1"] / med["assign"], 2)
        res["knn1_over_assign_spread"] = [round(res["call_ms_min"]["knn1"] / res["call_ms_max"]["assign"], 2), round(res["call_ms_max"]["knn1"] / res["call_ms_min"]["assign"], 2)]
        pw = n * k * (bits // 64) / (med["assign"] * 1e-3)
        res["assign_kernel"] = {"pair_words_per_s_G": round(pw / 1e9, 2), "valu_per_pair_word": round(VALU_PER_PAIR_WORD[bits], 4),
                                "valu_lane_ops_per_s_G": round(pw * VALU_PER_PAIR_WORD[bits] / 1e9, 1), "valu_peak_G": VALU_PEAK_GOPS,
                                "share_of_valu_issue_rate": round(pw * VALU_PER_PAIR_WORD[bits] / 1e9 / VALU_PEAK_GOPS, 4),
                                "hbm_bytes_once": n * nbytes,
                                "how": "pair-words over the median call time of `assign` (host clock, launch included); VALU instructions per pair-word counted in "
                                       "the saved ISA; the VALU issue rate is the bound, the codes are read from HBM once"}
    note("timed: %s" % res)
    with open(args.step_out, "w") as f:
        json.dump(res, f)
    holder.close()
    e.close()


def split_from_trace(path, res):
    """the kernel-trace database of a `rocprofv3 --kernel-trace --stats` run of one --step of `--only kmajority` -> kernel time per
    vc_kmajority_dev call, split into assign, update (vc_groups_run's kernels, its sort, scans and gather) and bookkeeping.  Only the
    dispatches from the first vc_assign_kernel on count: what comes before is the set-up of the store and the centres."""
    db = sqlite3.connect(path)
    t0 = db.execute("select min(start) from kernels where name like '%vc_assign_kernel%'").fetchone()[0]
    ms, launches = dict.fromkeys(("assign", "update", "bookkeeping", "copies_and_fills"), 0.0), {}
    for name, cnt, total in db.execute("select name, count(*), sum(duration) from kernels where start >= ? group by name", (t0,)):
        key = ("assign" if "vc_assign_" in name else "bookkeeping" if "vc_kmaj_" in name else
               "update" if any(x in name for x in ("vc_groups_", "rs_", "scan_", "vc_ids_gather")) else "copies_and_fills")
        ms[key] += total / 1e6
        launches[key] = launches.get(key, 0) + cnt
    calls = db.execute("select count(*) from kernels where name like '%vc_kmaj_empty_kernel%'").fetchone()[0]
    per_launch = db.execute("select avg(duration), min(duration), max(duration) from kernels where name like '%vc_assign_kernel%'").fetchone()
    res["kernel_trace"] = {"calls_traced": calls, "kernel_ms_per_call": {key: round(v / max(calls, 1), 4) for key, v in ms.items()},
                           "launches_per_call": {key: round(v / max(calls, 1), 2) for key, v in launches.items()},
                           "vc_assign_kernel_ms": {"mean": round(per_launch[0] / 1e6, 4), "min": round(per_launch[1] / 1e6, 4), "max": round(per_launch[2] / 1e6, 4)},
                           "how": "rocprofv3 --kernel-trace --stats over one --step of --only kmajority (a run of its own, warm-up call included); the wall time "
                                  "of a call less these kernel times is host waits and launch gaps"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e6)
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--min-pts", type=int, default=4)
    ap.add_argument("--cluster-size", type=int, default=16, help="records per centre of the synthetic data")
    ap.add_argument("--flips", type=int, default=6, help="a record is its centre with up to this many bits flipped")
    ap.add_argument("--rounds", type=int, default=10, help="max_iters of the k-majority leg")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=35)
    ap.add_argument("--only", default="all", choices=("all", "kmajority"), help="kmajority: that leg alone (for a profiler run)")
    ap.add_argument("--shapes", default=None, help="bits:K,... (default %s)" % ",".join("%d:%d" % s for s in SHAPES))
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds one shape may take")
    ap.add_argument("--trace-db", default=None, help="the database a rocprofv3 --kernel-trace --stats run of one --step of --only kmajority wrote, with "
                                                    "--trace-shape bits:K: merged into that shape of --out")
    ap.add_argument("--trace-shape", default="64:4096")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--step-out", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--bits", type=int, default=64, help=argparse.SUPPRESS)
    ap.add_argument("--k", type=int, default=256, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    if args.trace_db:
        line = json.load(open(args.out))
        bits, k = (int(x) for x in args.trace_shape.split(":"))
        split_from_trace(args.trace_db, next(sh for sh in line["shapes"] if (sh["bits"], sh["k"]) == (bits, k)))
        with open(args.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
        return print(json.dumps(line))
    shapes = [tuple(int(x) for x in s.split(":")) for s in args.shapes.split(",")] if args.shapes else SHAPES
    line = {"metric": "vc_assign_nearest_dev over all records against get_codes + k = 1 linear search in calls of %d ids, and vc_kmajority_dev (%d rounds), %.3g "
                      "clustered codes (%d per centre, <= %d flips), one engine; sharded forms: not timed" % (CHUNK, args.rounds, args.n, args.cluster_size, args.flips),
            "shapes": []}
    with tempfile.TemporaryDirectory() as td:
        for bits, k in shapes:
            part = os.path.join(td, "run_%d_%d.json" % (bits, k))
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", "--step-out", part, "--bits", str(bits),
                   "--k", str(k), "--only", args.only]
            for key in ("n", "radius", "min_pts", "cluster_size", "flips", "rounds", "reps", "seed"):
                cmd += ["--" + key.replace("_", "-"), str(getattr(args, key))]
            rc = subprocess.call(cmd)
            if rc != 0:
                raise SystemExit("the run of shape %d:%d ended with status %d" % (bits, k, rc))
            line["shapes"].append(json.load(open(part)))
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
