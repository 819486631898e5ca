"""Batched by-id k-NN against the same search on codes already in HBM, and against the single-id loop it replaces: 1e8 clustered
128-bit codes (n/1000 centres, <= 11 flips), m = 4, exact MIH top-100, one engine.

  ids        calls of 4 096 random resident ids through vc_search_knn_ids_dev (gather + search + found mask)
  ids_self   the same with VC_IDS_EXCLUDE_SELF (gather + search with k + 1 + strip)
  codes      vc_search_knn_dev on the SAME codes, gathered once by vc_get_codes_dev and left in HBM
  loop       --loop-ids ids through get_code + one single-query search_knn each: the only by-id path before the batched call

The three batched legs are timed interleaved, call after call, two id sets alternating, a host clock around a call that ends in a
device synchronise; their rows are asserted equal (ids == codes; ids_self == the codes leg with k + 1, stripped on the host).
Prints one JSON line.

    python tools/bench_ids.py [--n 1e8] [--calls 200] [--loop-ids 200]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e8)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--loop-ids", type=int, default=200)
    ap.add_argument("--seed", type=int, default=34)
    args = ap.parse_args()
    import torch
    from verticut_amd import engine as vc
    n, bits, m, k, Q = int(args.n), 128, 4, args.k, args.queries
    mode = vc.MODE_MIH_EXACT

    def note(what):
        print("[bench_ids] %s" % what, file=sys.stderr, flush=True)

    e = vc.Engine(bits, capacity=n, n_tables=m, flags=vc.FLAG_LEAN_TIMING)
    e.add_synthetic(n, seed=args.seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // 1000, 1), max_flips=11)
    e.build_index()
    note("engine built")
    rng = np.random.default_rng(args.seed + 5)
    host_ids = [rng.integers(0, n, size=Q, dtype=np.uint32) for _ in range(2)]
    d_ids = [torch.from_numpy(h.view(np.int32)).cuda() for h in host_ids]
    d_codes = [torch.empty((Q, bits // 8), dtype=torch.uint8, device="cuda") for _ in range(2)]
    st = torch.cuda.current_stream().cuda_stream
    for i in range(2):
        e.get_codes_dev(d_ids[i].data_ptr(), Q, d_codes[i].data_ptr(), None, stream=st)
    d_out = torch.empty((Q, k + 1), dtype=torch.int64, device="cuda")
    d_cnt = torch.empty((Q,), dtype=torch.int32, device="cuda")

    def leg_ids(i, flags=0):
        e.search_knn_ids_dev(d_ids[i].data_ptr(), Q, k, d_out.data_ptr(), d_cnt.data_ptr(), mode=mode, id_flags=flags, stream=st)

    def leg_codes(i, kk=k):
        e.search_knn_dev(d_codes[i].data_ptr(), Q, kk, d_out.data_ptr(), d_cnt.data_ptr(), mode=mode, stream=st)

    legs = {"ids": leg_ids, "ids_self": lambda i: leg_ids(i, vc.IDS_EXCLUDE_SELF), "codes": leg_codes}

    def timed(fn, i):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(i)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def rows(fn, i, kk):
        fn(i)
        torch.cuda.synchronize()
        return d_out.cpu().numpy().view(np.uint64).reshape(-1)[:Q * kk].reshape(Q, kk).copy(), d_cnt.cpu().numpy().view(np.uint32).copy()

    # the legs answer the same thing (also the warm-up of every shape the timed window uses)
    ref, rcnt = rows(leg_codes, 0, k)
    got, gcnt = rows(leg_ids, 0, k)
    assert np.array_equal(got, ref) and np.array_equal(gcnt, rcnt), "by-id rows differ from the rows of the gathered codes"
    ref1, _ = rows(lambda i: leg_codes(i, k + 1), 0, k + 1)
    got, gcnt = rows(legs["ids_self"], 0, k)
    for q in range(Q):
        r = ref1[q]
        assert np.array_equal(got[q], r[r != np.uint64(host_ids[0][q])][:k]), "self-excluded rows differ from the stripped k + 1 rows"
    for fn in legs.values():
        timed(fn, 1)
    note("rows equal, legs warm")
    t = {name: [] for name in legs}
    for c in range(args.calls):
        for name, fn in legs.items():
            t[name].append(timed(fn, c % 2))
    note("batched legs timed")
    # the single-id path: W synchronous 8-byte copies, then a single-query call that uploads the code again
    loop_ids = rng.integers(0, n, size=args.loop_ids, dtype=np.uint32)
    for gid in loop_ids[:8]:
        e.search_knn(e.get_code(int(gid)), k, mode=mode)
    t0 = time.perf_counter()
    for gid in loop_ids:
        e.search_knn(e.get_code(int(gid)), k, mode=mode)
    loop_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    for gid in loop_ids:
        e.get_code(int(gid))
    get_s = time.perf_counter() - t0
    med = {name: float(np.median(v)) for name, v in t.items()}
    print(json.dumps({
        "metric": "exact MIH top-%d by id, %.3g clustered 128-bit codes, m=4, calls of %d resident ids, one engine" % (k, n, Q),
        "queries_per_s": {name: round(Q / v, 1) for name, v in med.items()},
        "call_ms_median": {name: round(v * 1e3, 3) for name, v in med.items()},
        "call_ms_min": {name: round(min(v) * 1e3, 3) for name, v in t.items()},
        "ids_minus_codes_us": round((med["ids"] - med["codes"]) * 1e6, 1),
        "ids_self_minus_codes_us": round((med["ids_self"] - med["codes"]) * 1e6, 1),
        "calls": args.calls,
        "loop": {"ids": int(args.loop_ids), "queries_per_s": round(args.loop_ids / loop_s, 1),
                 "us_per_id": round(loop_s / args.loop_ids * 1e6, 1), "get_code_us_per_id": round(get_s / args.loop_ids * 1e6, 1)},
        "batched_over_loop": round(Q / med["ids"] / (args.loop_ids / loop_s), 1),
        "rows_equal": True,
    }))
    e.close()


if __name__ == "__main__":
    main()
