"""Approximate MIH k-NN over 8 id-range shards on ONE device, with and without VC_FLAG_GLOBAL_APPROX, against one engine holding
everything: 1e8 clustered 128-bit codes (n/1000 centres, <= 11 flips), m = 4, top-100, calls of 4 096 near-duplicate queries
(bench.py's knn_mih generator: a database item with 0-4 flipped bits).  Three legs in one process, timed interleaved, call
after call: the single engine, the flagged store, the unflagged store (today's behaviour: every shard runs to its own 20 k).
Every leg has a time limit of its own: before its timed calls a leg answers --probe queries, and a leg whose full call would
not fit the limit by that measure is not run -- the estimate is its result; a leg that runs stops calling once the limit is
spent.  The flagged rows, counts and statistics are asserted equal to the single engine's.  Prints one JSON line with
queries/s and a flagged call's per-round wall times (the [vc_ga] lines of a store created with VC_MIH_GS_TRACE set).

    python tools/bench_sharded_approx.py [--n 1e8] [--calls 6] [--leg-limit 60]
"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_sharded_mih import captured_stderr, near_queries  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e8)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--probe", type=int, default=64, help="queries of the call that prices a leg")
    ap.add_argument("--leg-limit", type=float, default=60.0, help="seconds a leg may spend on its timed calls")
    ap.add_argument("--seed", type=int, default=34)
    args = ap.parse_args()
    import torch
    from verticut_amd import engine as vc
    n, bits, m, k, Q = int(args.n), 128, 4, args.k, args.queries
    mode = vc.MODE_MIH_APPROX
    synth = dict(seed=args.seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // 1000, 1), max_flips=11)

    def note(what):   # progress on stderr: a run of several minutes says where it is
        print("[bench_sharded_approx] %s" % what, file=sys.stderr, flush=True)

    def store(flags):
        s = vc.ShardedEngine(bits, capacity=n, n_shards=args.shards, n_tables=m, devices=[0], flags=flags)
        s.add_synthetic(n, **synth)
        s.build_index()
        note("store with flags 0x%x built" % flags)
        return s

    one = vc.Engine(bits, capacity=n, n_tables=m, flags=vc.FLAG_LEAN_TIMING)
    one.add_synthetic(n, **synth)
    one.build_index()
    legs = {"single": one, "flagged": store(vc.FLAG_GLOBAL_APPROX), "unflagged": store(0)}
    rng = np.random.default_rng(args.seed + 3)
    host_q = [near_queries(one, n, Q, bits, 4, rng) for _ in range(2)]
    dev_q = [torch.from_numpy(h).cuda() for h in host_q]
    d_out = torch.empty((Q, k), dtype=torch.int64, device="cuda")
    d_cnt = torch.empty((Q,), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def timed(eng, i, nq=Q):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.search_knn_dev(dev_q[i % 2].data_ptr(), nq, k, d_out.data_ptr(), d_cnt.data_ptr(), mode=mode, stream=st)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    # the price of a leg: a small call (also the warm-up: buffers grown, code objects loaded), scaled to a full one
    estimate, spent = {}, {}
    for name, eng in legs.items():
        timed(eng, 0, args.probe)
        estimate[name] = timed(eng, 1, args.probe) * Q / args.probe
        note("%s: a call is estimated at %.3f s" % (name, estimate[name]))
        spent[name] = 0.0
    runs = {name: estimate[name] <= args.leg_limit for name in legs}
    t = {name: [] for name in legs}
    for name, eng in legs.items():
        if runs[name]:
            timed(eng, 0)   # full-size warm-up
    for i in range(args.calls):
        for name, eng in legs.items():
            if runs[name] and spent[name] < args.leg_limit:
                t[name].append(timed(eng, i))
                spent[name] += t[name][-1]
        note("call %d timed" % i)
    # the flagged store answers exactly what the single engine answers
    got, cnt, gst = legs["flagged"].search_knn(host_q[0], k, mode=mode, with_stats=True)
    ref, rcnt, rst = one.search_knn(host_q[0], k, mode=mode, with_stats=True)
    key = lambda x: (x.radius, x.n_results, x.n_sub_reads, x.n_local_reads, x.n_candidates)
    equal = bool(np.array_equal(got, ref) and np.array_equal(cnt, rcnt) and [key(x) for x in gst] == [key(x) for x in rst])
    assert equal, "flagged sharded rows / statistics differ from the single engine"
    unflagged_radius = None
    if runs["unflagged"]:
        _, _, ust = legs["unflagged"].search_knn(host_q[0], k, mode=mode, with_stats=True)
        unflagged_radius = np.bincount([x.radius for x in ust]).tolist()
    legs["unflagged"].close()
    # VC_MIH_GS_TRACE is read when a sharded store is created: the per-round times come from a store of their own, built
    # after the timed calls, so that those run without the trace
    os.environ["VC_MIH_GS_TRACE"] = "1"
    try:
        traced = store(vc.FLAG_GLOBAL_APPROX)
    finally:
        del os.environ["VC_MIH_GS_TRACE"]
    captured_stderr(lambda: timed(traced, 0), "[vc_ga]")   # warm-up
    rounds = captured_stderr(lambda: timed(traced, 0), "[vc_ga]")
    traced.close()
    qps = {name: Q / float(np.median(v)) for name, v in t.items() if v}
    per_round = []
    for ln in rounds:
        us = re.search(r"([0-9.]+) us$", ln)
        per_round.append({"line": ln, "us": float(us.group(1)) if us else None})
    print(json.dumps({
        "metric": "approximate MIH top-%d, %d shards on one device, %.3g clustered 128-bit codes, m=4, calls of %d near-duplicate queries"
                  % (k, args.shards, n, Q),
        "queries_per_s": {name: round(v, 1) for name, v in qps.items()},
        "flagged_over_unflagged": round(qps["flagged"] / qps["unflagged"], 2) if "flagged" in qps and "unflagged" in qps else None,
        "flagged_over_single": round(qps["flagged"] / qps["single"], 3) if "flagged" in qps and "single" in qps else None,
        "leg_limit_s": args.leg_limit,
        "estimated_call_s": {name: round(v, 3) for name, v in estimate.items()},
        "not_run_over_limit": [name for name in legs if not runs[name]],
        "call_ms": {name: [round(x * 1e3, 2) for x in v] for name, v in t.items()},
        "flagged_rounds_per_call": len(per_round),
        "flagged_rounds": per_round,
        "radius_histogram_single": np.bincount([x.radius for x in rst]).tolist(),
        "radius_histogram_unflagged": unflagged_radius,
        "rows_and_stats_equal_single": equal,
    }))
    legs["flagged"].close()
    one.close()


if __name__ == "__main__":
    main()
