"""Exact MIH k-NN over 8 id-range shards on ONE device, with and without VC_FLAG_GLOBAL_STOP, against one engine holding
everything: 1e8 clustered 128-bit codes (n/1000 centres, <= 11 flips), m = 4, top-100, calls of 4 096 near-duplicate queries
(bench.py's knn_mih generator: a database item with 0-4 flipped bits).  The three are timed interleaved, call after call, in
one process; the flagged rows, counts and statistics are asserted equal to the single engine's.  Prints one JSON line with
queries/s and a flagged call's per-round wall times (the VC_MIH_GS_TRACE lines of a store created with that knob set).

    python tools/bench_sharded_mih.py [--n 1e8] [--calls 6] [--unflagged-calls 2]
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def near_queries(e, n, nq, bits, max_flips, rng):
    q = np.empty((nq, bits // 8), dtype=np.uint8)
    for i in range(nq):
        c = e.get_code(int(rng.integers(0, n)))
        for b in rng.choice(bits, size=int(rng.integers(0, max_flips + 1)), replace=False):
            c[b // 8] ^= np.uint8(1 << (b % 8))
        q[i] = c
    return q


def captured_stderr(fn, prefix="[vc_gs]"):
    """run fn() with stderr captured; returns the trace lines that start with `prefix` (default: the sharded global stop's)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+") as f:
        os.dup2(f.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        return [ln.strip() for ln in f if ln.startswith(prefix)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e8)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--unflagged-calls", type=int, default=2)
    ap.add_argument("--seed", type=int, default=34)
    args = ap.parse_args()
    import torch
    from verticut_amd import engine as vc
    n, bits, m, k, Q = int(args.n), 128, 4, args.k, args.queries
    synth = dict(seed=args.seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // 1000, 1), max_flips=11)
    one = vc.Engine(bits, capacity=n, n_tables=m, flags=vc.FLAG_LEAN_TIMING)
    flagged = vc.ShardedEngine(bits, capacity=n, n_shards=args.shards, n_tables=m, devices=[0], flags=vc.FLAG_GLOBAL_STOP)
    plain = vc.ShardedEngine(bits, capacity=n, n_shards=args.shards, n_tables=m, devices=[0])
    for s in (one, flagged, plain):
        s.add_synthetic(n, **synth)
        s.build_index()
    rng = np.random.default_rng(args.seed + 3)
    host_q = [near_queries(one, n, Q, bits, 4, rng) for _ in range(2)]
    dev_q = [torch.from_numpy(h).cuda() for h in host_q]
    d_out = torch.empty((Q, k), dtype=torch.int64, device="cuda")
    d_cnt = torch.empty((Q,), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(eng, i):
        eng.search_knn_dev(dev_q[i % 2].data_ptr(), Q, k, d_out.data_ptr(), d_cnt.data_ptr(), mode=vc.MODE_MIH_EXACT, stream=st)

    def timed(eng, i):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call(eng, i)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for eng in (one, flagged, plain):   # warm-up: buffers grown, code objects loaded
        call(eng, 0)
    t = {"single": [], "flagged": [], "unflagged": []}
    for i in range(args.calls):
        t["single"].append(timed(one, i))
        t["flagged"].append(timed(flagged, i))
        if i < args.unflagged_calls:
            t["unflagged"].append(timed(plain, i))
    # VC_MIH_GS_TRACE is read when a sharded store is created: the per-round times come from a store of their own, built
    # after the timed calls, so that those run without the trace
    os.environ["VC_MIH_GS_TRACE"] = "1"
    try:
        traced = vc.ShardedEngine(bits, capacity=n, n_shards=args.shards, n_tables=m, devices=[0], flags=vc.FLAG_GLOBAL_STOP)
    finally:
        del os.environ["VC_MIH_GS_TRACE"]
    traced.add_synthetic(n, **synth)
    traced.build_index()
    captured_stderr(lambda: call(traced, 0))   # warm-up
    rounds = captured_stderr(lambda: timed(traced, 0))
    traced.close()
    # the flagged store answers exactly what the single engine answers
    got, cnt, gst = flagged.search_knn(host_q[0], k, mode=vc.MODE_MIH_EXACT, with_stats=True)
    ref, rcnt, rst = one.search_knn(host_q[0], k, mode=vc.MODE_MIH_EXACT, with_stats=True)
    key = lambda x: (x.radius, x.n_results, x.n_sub_reads, x.n_local_reads, x.n_candidates)
    equal = bool(np.array_equal(got, ref) and np.array_equal(cnt, rcnt) and [key(x) for x in gst] == [key(x) for x in rst])
    assert equal, "flagged sharded rows / statistics differ from the single engine"
    qps = {name: Q / float(np.median(v)) for name, v in t.items() if v}
    per_round = []
    for ln in rounds:
        us = re.search(r"([0-9.]+) us$", ln)
        per_round.append({"line": ln, "us": float(us.group(1)) if us else None})
    print(json.dumps({
        "metric": "exact MIH top-%d, %d shards on one device, %.3g clustered 128-bit codes, m=4, calls of %d near-duplicate queries"
                  % (k, args.shards, n, Q),
        "queries_per_s": {name: round(v, 1) for name, v in qps.items()},
        "flagged_over_unflagged": round(qps["flagged"] / qps["unflagged"], 2) if "unflagged" in qps else None,
        "flagged_over_single": round(qps["flagged"] / qps["single"], 3),
        "call_ms": {name: [round(x * 1e3, 2) for x in v] for name, v in t.items()},
        "flagged_rounds": per_round,
        "radius_histogram_single": np.bincount([x.radius for x in rst]).tolist(),
        "rows_and_stats_equal_single": equal,
    }))
    for s in (flagged, plain, one):
        s.close()


if __name__ == "__main__":
    main()
