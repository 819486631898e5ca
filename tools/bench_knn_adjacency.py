"""The reverse, mutual and symmetrised k-NN graph in CSR form (vc_knn_adjacency_dev) against its floor and the path it replaces:
clustered synthetic 64-bit codes (the store of bench_knn_graph.py: 1e6 records, 16 per centre, up to 6 flipped bits), m = 2, the
graph built once per k by vc_knn_graph_dev in exact MIH, one engine, k = kk = 10 and k = kk = 100, no cap.

  reverse / mutual / either   vc_knn_adjacency_dev with the output sized by the bound, buffers warm
  sizing                      the VC_KNN_REVERSE call with adj_cap = 0: the count pass, the scan and the wait -- no item, no sort
  cluster_knn                 vc_cluster_knn_dev on the same graph and handle: one edge pass, the floor any reader of the graph pays
  host                        the replaced path, once: the rows copied home, the (target, dist, source) triples of VC_KNN_REVERSE
                              ordered by np.lexsort, the offsets by bincount and cumsum

Per k one child process under its own `timeout`, the next only after the one before succeeded.  In it, before anything is timed:
VC_KNN_REVERSE's offsets, segments and statistics == the host's (asserted, every word); VC_KNN_MUTUAL and VC_KNN_EITHER against the
host on --sample targets spread over the store (the verified reverse segment intersected / united with the target's own row; every
word of those segments asserted) and their totals against vc_cluster_knn_dev's n_edges and n_mutual (asserted).  Then the device
legs interleaved, a host clock around each ending in a device synchronise, medians of --reps with min .. max.
`beyond_count_ms` = reverse - sizing is what the items, the sort and the copy out cost together; the sort's passes move
passes x items x 24 bytes plus the histogram reads, so `sort_bytes_per_s_at_least` = that traffic / beyond_count_ms is a LOWER bound
on the sort's rate (no kernel trace was taken).  No ratio is fixed in advance.  Prints one JSON line; --out also writes it to a file.

    python tools/bench_knn_adjacency.py [--n 1e6] [--ks 10,100] [--reps 7] [--out profiles/knn_adjacency_bench.json]
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

LOW = np.uint64(0xFFFFFFFF)
PEAK = 8e12   # bytes per second of HBM, the figure the other tools compare with


def host_reverse(rows):
    """(offsets [n + 1], adj [n k]) of VC_KNN_REVERSE for full rows without a cap, by np.lexsort"""
    n, k = rows.shape
    flat = rows.reshape(-1)
    tgt = (flat & LOW).astype(np.int64)
    dist = flat >> np.uint64(32)
    src = np.repeat(np.arange(n, dtype=np.uint64), k)
    order = np.lexsort((src, dist, tgt))
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(np.bincount(tgt, minlength=n))
    return offsets, ((dist << np.uint64(32)) | src)[order]


def step(args):
    import torch
    from verticut_amd import engine as vc
    n, bits, m, k = int(args.n), 64, 2, args.k
    kk = k

    def note(what):
        print("[bench_knn_adjacency k=%d] %s" % (k, what), file=sys.stderr, flush=True)

    e = vc.Engine(bits, capacity=n, n_tables=m, flags=vc.FLAG_LEAN_TIMING)
    e.add_synthetic(n, seed=args.seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // args.cluster_size, 1), max_flips=args.flips)
    e.build_index()
    st = torch.cuda.current_stream().cuda_stream
    d_rows = torch.empty((n, k), dtype=torch.int64, device="cuda")
    d_counts = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_labels = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_deg = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_offsets = torch.empty((n + 1,), dtype=torch.int64, device="cuda")
    d_adj = torch.empty((2 * n * kk,), dtype=torch.int64, device="cuda")
    e.knn_graph_dev(k, d_rows.data_ptr(), d_counts.data_ptr(), mode=vc.MODE_MIH_EXACT, batch=args.batch, stream=st)
    torch.cuda.synchronize()
    note("graph built")
    assert np.all(d_counts.cpu().numpy().view(np.uint32) == min(k, n - 1)) and n > k

    def leg_adj(flags, cap=None):
        cap = (2 if flags == vc.KNN_EITHER else 1) * n * kk if cap is None else cap
        return e.knn_adjacency_dev(d_rows.data_ptr(), d_counts.data_ptr(), k, kk, d_adj.data_ptr() if cap else None, cap, d_offsets.data_ptr(), flags=flags, stream=st)

    def leg_cluster():
        return e.cluster_knn_dev(d_rows.data_ptr(), d_counts.data_ptr(), k, kk, d_labels.data_ptr(), d_deg.data_ptr(), stream=st)

    def fetch(flags):
        rc, stats = leg_adj(flags)
        torch.cuda.synchronize()
        assert rc == vc.VC_OK
        offsets = d_offsets.cpu().numpy().view(np.uint64)
        return offsets, d_adj[:int(offsets[n])].cpu().numpy().view(np.uint64), stats

    # ---- the check, and the host leg with it
    t0 = time.perf_counter()
    rows = d_rows.cpu().numpy().view(np.uint64)
    t1 = time.perf_counter()
    want_offsets, want_adj = host_reverse(rows)
    t2 = time.perf_counter()
    host = {"copy_home": t1 - t0, "lexsort_and_offsets": t2 - t1}
    note("host path: %s" % host)
    cl = leg_cluster()
    torch.cuda.synchronize()
    offsets, adj, stats = fetch(vc.KNN_REVERSE)
    assert np.array_equal(offsets, want_offsets) and np.array_equal(adj, want_adj), "VC_KNN_REVERSE differs from the host's lexsort"
    deg = np.diff(want_offsets.astype(np.int64))
    assert stats == {"n_edges": n * kk, "n_entries": n * kk, "n_empty": int((deg == 0).sum()), "max_degree": int(deg.max())}, stats
    assert np.array_equal(d_deg.cpu().numpy().view(np.uint32), deg) and cl["n_edges"] == n * kk
    note("VC_KNN_REVERSE equals the host path on every word: %s" % stats)
    all_stats = {"reverse": stats}
    sample = np.unique(np.linspace(0, n - 1, args.sample).astype(np.int64))
    sample = np.unique(np.concatenate([sample, np.argsort(deg)[-16:]]))          # and the largest hubs
    for name, flags in (("mutual", vc.KNN_MUTUAL), ("either", vc.KNN_EITHER)):
        offsets, adj, stats = fetch(flags)
        want_T = 2 * cl["n_mutual"] if flags == vc.KNN_MUTUAL else 2 * (cl["n_edges"] - cl["n_mutual"])
        assert stats["n_entries"] == want_T == int(offsets[n]) and stats["n_edges"] == cl["n_edges"], (name, stats, cl)
        for j in sample.tolist():
            rev = want_adj[int(want_offsets[j]):int(want_offsets[j + 1])]
            own = rows[j]
            if flags == vc.KNN_MUTUAL:
                seg = own[np.isin(own & LOW, rev & LOW)]
            else:
                seg = np.sort(np.concatenate([own, rev[~np.isin(rev & LOW, own & LOW)]]))
            assert np.array_equal(adj[int(offsets[j]):int(offsets[j + 1])], seg), (name, j)
        all_stats[name] = stats
        note("VC_KNN_%s: totals equal vc_cluster_knn_dev's, %d sampled segments equal the host's: %s" % (name.upper(), len(sample), stats))
    del rows, want_adj, adj

    # ---- the timing
    legs = {"reverse": lambda: leg_adj(vc.KNN_REVERSE), "mutual": lambda: leg_adj(vc.KNN_MUTUAL), "either": lambda: leg_adj(vc.KNN_EITHER),
            "sizing": lambda: leg_adj(vc.KNN_REVERSE, 0), "cluster_knn": leg_cluster}
    for fn in legs.values():       # every buffer of the timed window warm
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
    res = {"checked": {"reverse_equals_host_lexsort_every_word": True, "mutual_either_totals_equal_cluster_knn": True, "mutual_either_sampled_segments": int(len(sample))},
           "stats": all_stats, "cluster_knn_stats": cl,
           "call_ms_median": {q: round(float(np.median(v)) * 1e3, 3) for q, v in t.items()},
           "call_ms_min": {q: round(min(v) * 1e3, 3) for q, v in t.items()},
           "call_ms_max": {q: round(max(v) * 1e3, 3) for q, v in t.items()}, "reps": args.reps,
           "host_s": {q: round(v, 3) for q, v in host.items()}, "host_s_total": round(sum(host.values()), 3)}
    med = res["call_ms_median"]
    items = n * kk
    dist_passes, key_passes = (int(bits).bit_length() + 7) // 8, (int(n).bit_length() + 7) // 8
    traffic = items * (dist_passes * (24 + 8) + key_passes * (24 + 4))
    beyond = med["reverse"] - med["sizing"]
    res.update(items=items, sort_passes=dist_passes + key_passes, sort_bytes=traffic, beyond_count_ms=round(beyond, 3),
               beyond_count_share=round(beyond / med["reverse"], 3), sort_bytes_per_s_at_least=round(traffic / (beyond * 1e-3), 0),
               sort_share_of_peak_at_least=round(traffic / (beyond * 1e-3) / PEAK, 3),
               over_cluster_knn={q: round(med[q] / med["cluster_knn"], 2) for q in ("reverse", "mutual", "either", "sizing")},
               host_over_reverse=round(res["host_s_total"] * 1e3 / med["reverse"], 1))
    note("timed: %s" % res)
    with open(args.step_out, "w") as f:
        json.dump(res, f)
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e6)
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--cluster-size", type=int, default=16, help="records per centre of the synthetic data")
    ap.add_argument("--flips", type=int, default=6, help="a record is its centre with up to this many bits flipped")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=35)
    ap.add_argument("--sample", type=int, default=2000, help="targets whose mutual and symmetrised segments the host rebuilds")
    ap.add_argument("--step-timeout", type=int, default=400, help="seconds a step may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=("run",), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--step-out", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--k", type=int, default=10, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    line = {"metric": "reverse / mutual / symmetrised k-NN graph in CSR form of a built exact k-NN graph, %.3g clustered 64-bit codes (%d per centre, <= %d flips), "
                      "kk = k, no cap, one engine" % (args.n, args.cluster_size, args.flips),
            "not_measured": "other shapes and code widths, the sharded forms, the host-pointer form, a last pass written straight into d_adj instead of the "
                            "copy of T words (only the copy exists), the split of beyond_count_ms into item writes, sort passes and copy (no kernel trace)"}
    with tempfile.TemporaryDirectory() as td:
        for k in [int(x) for x in args.ks.split(",")]:
            part = os.path.join(td, "run_%d.json" % k)      # chained: a step that fails, faults or runs into its time limit ends the run
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", "run", "--step-out", part, "--k", str(k)]
            for key in ("n", "batch", "cluster_size", "flips", "reps", "seed", "sample"):
                cmd += ["--" + key.replace("_", "-"), str(getattr(args, key))]
            rc = subprocess.call(cmd)
            if rc != 0:
                raise SystemExit("the step at k=%d ended with status %d: nothing further is started" % (k, rc))
            line["k=%d" % k] = json.load(open(part))
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
