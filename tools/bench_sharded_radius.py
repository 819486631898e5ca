"""Radius search over 8 id-range shards on ONE device, host-pointer form against device-resident form against one engine:
BASELINE configs[1]'s shape with the data and queries of `bench.py --workload c2` (64-bit codes from vc_add_synthetic(n, seed),
queries = database items with 0-8 flipped bits, radius 8, exact MIH), m = 2 and m = 4, calls of 1 024 queries.

    (A) vc_sharded_search_radius       host pointers: per-shard results cross to the host, are concatenated there into a padded
                                       ring, uploaded and re-sorted on the root
    (B) vc_sharded_search_radius_dev   queries, results and offsets stay in HBM; rank merge on the root
    (C) vc_search_radius_dev           one engine over the union: no sharding cost, the floor

The three outputs are first compared word for word; then every leg is warmed and the legs alternate A, B, C for --rounds rounds
of at least --seconds each, a host clock around calls that end in a synchronise.  Prints one JSON line (and writes it to --out):
queries/s per leg as the median over the rounds, with the rounds' spread.

    python tools/bench_sharded_radius.py [--n 1e8] [--tables 2,4] [--rounds 5] [--seconds 1.0] [--legs A,B,C] [--out FILE]
"""
import argparse
import json
import os
import sys
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


def run_shape(args, m, legs):
    import torch
    from verticut_amd import engine as vc
    n, bits, Q, radius = int(args.n), 64, args.queries, 8
    one = vc.Engine(bits, capacity=n, n_tables=m, flags=vc.FLAG_LEAN_TIMING)
    sh = vc.ShardedEngine(bits, capacity=n, n_shards=args.shards, n_tables=m, devices=[0])
    for s in (one, sh):
        s.add_synthetic(n, seed=args.seed)
        s.build_index()
    rng = np.random.default_rng(args.seed + 2)
    host_q = [near_queries(one, n, Q, bits, radius, rng) for _ in range(2)]
    dev_q = [torch.from_numpy(h).cuda() for h in host_q]
    out_cap = Q * 64
    d_out = {leg: torch.zeros((out_cap,), dtype=torch.int64, device="cuda") for leg in "BC"}
    d_off = {leg: torch.zeros((Q + 1,), dtype=torch.int64, device="cuda") for leg in "BC"}
    h_out, h_off = np.zeros(out_cap, dtype=np.uint64), np.zeros(Q + 1, dtype=np.uint64)
    st = torch.cuda.current_stream().cuda_stream
    L = vc.load_library()

    def call(leg, i):
        if leg == "A":     # the raw C call: the wrapper's list building is not part of the path
            rc = L.vc_sharded_search_radius(sh._h, host_q[i % 2].ctypes.data, Q, radius, vc.MODE_MIH_EXACT, h_out.ctypes.data, out_cap, h_off.ctypes.data)
        else:
            eng = sh if leg == "B" else one
            rc = eng.search_radius_dev(dev_q[i % 2].data_ptr(), Q, radius, d_out[leg].data_ptr(), out_cap, d_off[leg].data_ptr(),
                                       mode=vc.MODE_MIH_EXACT, stream=st)
        if rc != vc.VC_OK:    # a truncated result must never be timed as if it were complete
            raise SystemExit("leg %s: returned %d (results do not fit out_cap = %d)" % (leg, rc, out_cap))

    # the three outputs, word for word
    for leg in "ABC":
        call(leg, 0)
    torch.cuda.synchronize()
    offs = {"A": h_off.copy(), "B": d_off["B"].cpu().numpy().view(np.uint64), "C": d_off["C"].cpu().numpy().view(np.uint64)}
    total = int(offs["C"][Q])
    outs = {"A": h_out[:total].copy(), "B": d_out["B"].cpu().numpy().view(np.uint64)[:total], "C": d_out["C"].cpu().numpy().view(np.uint64)[:total]}
    equal = all(np.array_equal(offs[x], offs["C"]) and np.array_equal(outs[x], outs["C"]) for x in "AB")
    assert equal, "the three legs' outputs differ"

    def round_of(leg, seconds):
        torch.cuda.synchronize()
        calls, t0 = 0, time.perf_counter()
        while True:
            call(leg, calls)
            torch.cuda.synchronize()
            calls += 1
            dt = time.perf_counter() - t0
            if dt >= seconds:
                return Q * calls / dt

    for leg in legs:           # warm-up: buffers grown, code objects loaded
        round_of(leg, 0.2)
    qps = {leg: [] for leg in legs}
    for _ in range(args.rounds):
        for leg in legs:
            qps[leg].append(round_of(leg, args.seconds))
    res = {}
    for leg in legs:
        v = np.array(qps[leg])
        res[leg] = {"queries_per_s": round(float(np.median(v)), 1), "min": round(float(v.min()), 1), "max": round(float(v.max()), 1),
                    "spread_pct": round(float((v.max() - v.min()) / np.median(v) * 100), 2), "rounds": [round(float(x), 1) for x in v]}
    line = {"m": m, "substring_bits": bits // m, "mean_neighbours_per_query": total / Q, "total_per_call": total,
            "merge_algorithmic_bytes_per_call": total * 16 + (args.shards + 1) * (Q + 1) * 8,
            "outputs_equal": bool(equal), "legs": res}
    if "A" in res and "B" in res:
        line["B_over_A"] = round(res["B"]["queries_per_s"] / res["A"]["queries_per_s"], 3)
    if "C" in res and "B" in res:
        line["B_over_C"] = round(res["B"]["queries_per_s"] / res["C"]["queries_per_s"], 3)
    sh.close()
    one.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e8)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--tables", default="2,4")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--legs", default="A,B,C", help="legs to time (all three are always run once and compared)")
    ap.add_argument("--seed", type=int, default=34)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    legs = [x for x in args.legs.split(",") if x in ("A", "B", "C")]
    result = {
        "metric": "queries/s, all neighbours within Hamming distance 8 (exact MIH), 64-bit codes, %.3g-code DB, %d shards on one device, "
                  "calls of %d queries" % (args.n, args.shards, args.queries),
        "legs": {"A": "vc_sharded_search_radius (host pointers)", "B": "vc_sharded_search_radius_dev", "C": "vc_search_radius_dev, one engine"},
        "method": "legs alternate, %d rounds of >= %.1f s each, host clock around calls that end in a synchronise; median, min, max over rounds"
                  % (args.rounds, args.seconds),
        "shapes": [run_shape(args, int(m), legs) for m in args.tables.split(",")],
    }
    text = json.dumps(result)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
