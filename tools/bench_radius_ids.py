"""Radius search by id against the same search on codes already gathered: BASELINE configs[1], the shape of `bench.py --workload c2`
(1e8 uniform 64-bit codes, all neighbours within R = 8, m = 2, exact MIH), calls of 4 096 random resident ids, one engine.

  ids          vc_search_radius_ids_dev with id_flags = 0 (gather + radius search + count / scans / copy)
  ids_greater  the same with VC_IDS_ONLY_GREATER
  codes        vc_get_codes_dev + vc_search_radius_dev on the same ids -- what a caller whose ids all exist had before

The three legs are timed interleaved, call after call, two id sets alternating, a host clock around a call that ends in a device
synchronise; medians of --calls calls.  In the same run the segments of `ids` are asserted equal to those of `codes`, and those of
`ids_greater` to the `ids` segments filtered on the host.  What `ids` may cost over `codes`: the count launch, the two scans and the
plan launch, the copy launch, at most one extra wait (none here: the output buffer holds the uncompacted total) and one extra pass
over the results (16 bytes per entry).  The tool prices that pass at --hbm-gbs and measures the marginal cost of a tiny launch
(back-to-back one-element fills on the same stream) so that the two can be set against the measured difference.
Prints one JSON line; --out also writes it to a file.

    python tools/bench_radius_ids.py [--n 1e8] [--calls 20] [--out profiles/radius_ids_bench.json]
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
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--seed", type=int, default=34)
    ap.add_argument("--hbm-gbs", type=float, default=4000.0, help="rate the extra pass over the results is priced at")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from verticut_amd import engine as vc
    n, bits, m, Q, radius = int(args.n), 64, 2, args.queries, args.radius
    mode = vc.MODE_MIH_EXACT

    def note(what):
        print("[bench_radius_ids] %s" % what, file=sys.stderr, flush=True)

    e = vc.Engine(bits, capacity=n, n_tables=m, flags=vc.FLAG_LEAN_TIMING)
    e.add_synthetic(n, seed=args.seed)
    e.build_index()
    note("engine built")
    rng = np.random.default_rng(args.seed + 5)
    host_ids = [rng.integers(0, n, size=Q, dtype=np.uint32) for _ in range(2)]
    d_ids = [torch.from_numpy(h.view(np.int32)).cuda() for h in host_ids]
    d_codes = torch.empty((Q, bits // 8), dtype=torch.uint8, device="cuda")
    out_cap = Q * 64
    d_out = torch.empty((out_cap,), dtype=torch.int64, device="cuda")
    d_off = torch.empty((Q + 1,), dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def leg_ids(i, flags=0):
        if e.search_radius_ids_dev(d_ids[i].data_ptr(), Q, radius, d_out.data_ptr(), out_cap, d_off.data_ptr(), mode=mode, id_flags=flags,
                                   stream=st) != vc.VC_OK:
            raise SystemExit("results do not fit out_cap = %d" % out_cap)

    def leg_codes(i):
        e.get_codes_dev(d_ids[i].data_ptr(), Q, d_codes.data_ptr(), None, stream=st)
        if e.search_radius_dev(d_codes.data_ptr(), Q, radius, d_out.data_ptr(), out_cap, d_off.data_ptr(), mode=mode, stream=st) != vc.VC_OK:
            raise SystemExit("results do not fit out_cap = %d" % out_cap)

    legs = {"ids": leg_ids, "ids_greater": lambda i: leg_ids(i, vc.IDS_ONLY_GREATER), "codes": leg_codes}

    def timed(fn, i):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(i)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def segments(fn, i):
        fn(i)
        torch.cuda.synchronize()
        offs = d_off.cpu().numpy().view(np.uint64).copy()
        return offs, d_out.cpu().numpy().view(np.uint64)[:int(offs[Q])].copy()

    # the legs answer the same thing (also the warm-up of every buffer the timed window uses)
    entries = {}
    for i in range(2):
        ro, rf = segments(leg_codes, i)
        go, gf = segments(leg_ids, i)
        assert np.array_equal(go, ro) and np.array_equal(gf, rf), "by-id segments differ from the segments of the gathered codes"
        owner = np.repeat(host_ids[i].astype(np.uint64), np.diff(go.astype(np.int64)))
        keep = (gf & np.uint64(0xFFFFFFFF)) > owner
        want_lens = np.bincount(np.repeat(np.arange(Q), np.diff(go.astype(np.int64)))[keep], minlength=Q)
        bo, bf = segments(legs["ids_greater"], i)
        assert np.array_equal(np.diff(bo.astype(np.int64)), want_lens) and np.array_equal(bf, gf[keep]), \
            "ONLY_GREATER segments differ from the host-filtered segments"
        entries[i] = {"ids": int(go[Q]), "ids_greater": int(bo[Q])}
    note("segments equal, legs warm: %s" % entries)
    t = {name: [] for name in legs}
    for c in range(args.calls):
        for name, fn in legs.items():
            t[name].append(timed(fn, c % 2))
    note("legs timed")
    # marginal cost of a tiny launch on this box: 1 000 one-element fills back to back, one synchronise
    one = torch.zeros(1, dtype=torch.int32, device="cuda")
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(1000):
            one.fill_(1)
        torch.cuda.synchronize()
        tiny_us = (time.perf_counter() - t0) * 1e3
    med = {name: float(np.median(v)) for name, v in t.items()}
    mean_entries = float(np.mean([entries[i]["ids"] for i in range(2)]))
    pass_us = mean_entries * 16 / (args.hbm_gbs * 1e9) * 1e6
    line = {
        "metric": "exact MIH radius-%d search by id, %.3g uniform 64-bit codes, m=2, calls of %d resident ids, one engine" % (radius, n, Q),
        "call_ms_median": {name: round(v * 1e3, 3) for name, v in med.items()},
        "call_ms_min": {name: round(min(v) * 1e3, 3) for name, v in t.items()},
        "queries_per_s": {name: round(Q / v, 1) for name, v in med.items()},
        "entries_per_call": entries,
        "ids_minus_codes_us": round((med["ids"] - med["codes"]) * 1e6, 1),
        "ids_greater_minus_codes_us": round((med["ids_greater"] - med["codes"]) * 1e6, 1),
        "allowance_us": {"extra_pass_16B_per_entry_at_%g_GBs" % args.hbm_gbs: round(pass_us, 3), "tiny_launch": round(tiny_us, 2),
                         "pass_plus_four_launches": round(pass_us + 4 * tiny_us, 2)},
        "calls": args.calls,
        "out_cap": out_cap,
        "segments_equal": True,
    }
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
    e.close()


if __name__ == "__main__":
    main()
