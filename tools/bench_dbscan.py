"""Density clustering on the device (vc_dbscan_radius_dev) against the single-linkage clustering next to it (vc_cluster_radius_dev, the
yardstick: existing code over the same radius searches), on tools/bench_cluster.py's data and parameters: clustered synthetic
64-bit codes, all neighbours within R = 8, m = 2, exact MIH, one engine, 1e6 records in 62 500 clusters of about 16, batches of
4 096 ids, min_pts = 4.

  dbscan       vc_dbscan_radius_dev: per batch fill ids, gather, radius search, then the degree and the edge launch over the raw
               result; one finish pass at the end
  cluster      vc_cluster_radius_dev from scratch on the same handle: the same batches and searches, one union launch per batch

Two steps, each a child process under its own `timeout`, the second only after the first succeeded:
  check   labels and degrees of `dbscan` == a host DBSCAN over the pairs that vc_search_radius_ids_dev + VC_IDS_ONLY_GREATER lists
          (asserted), n_pairs == their number, all five statistics (asserted); written down: the three kind counts and the clusters
          beside the single-linkage count
  time    the two legs interleaved, a host clock around each leg ending in a device synchronise, medians of --reps
No time is fixed in advance: both legs spend their time in the same radius searches -- ONE walk each -- and the dbscan call adds one
small launch per batch and the finish pass.  A ratio near 2 would mean a second walk.  Prints one JSON line; --out also writes it.

    python tools/bench_dbscan.py [--n 1e6] [--reps 7] [--out profiles/dbscan_bench.json]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
LOW = np.uint64(0xFFFFFFFF)


def host_dbscan(n, a, b, min_pts):
    """(labels, degrees) by the rule: the degree counts the record itself; cores are united by bench_cluster.host_union_find over
    the core-core pairs; a non-core record with a core neighbour takes the label of its smallest-id core neighbour.  (a, b): every
    pair once, a < b."""
    from bench_cluster import host_union_find
    deg = 1 + np.bincount(a, minlength=n) + np.bincount(b, minlength=n)
    core = deg >= min_pts
    cc = core[a] & core[b]
    lab = host_union_find(n, a[cc], b[cc])
    anchor = np.full(n, n, dtype=np.int64)
    up, down = core[a] & ~core[b], ~core[a] & core[b]
    np.minimum.at(anchor, b[up], a[up])
    np.minimum.at(anchor, a[down], b[down])
    border = ~core & (anchor < n)
    lab[border] = lab[anchor[border]]
    return lab, deg


def step(args):
    import torch
    from verticut_amd import engine as vc
    n, bits, m, B, radius, min_pts = int(args.n), 64, 2, args.batch, args.radius, args.min_pts
    mode = vc.MODE_MIH_EXACT

    def note(what):
        print("[bench_dbscan] %s" % what, file=sys.stderr, flush=True)

    e = vc.Engine(bits, capacity=n, n_tables=m, flags=vc.FLAG_LEAN_TIMING)
    e.add_synthetic(n, seed=args.seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // args.cluster_size, 1), max_flips=args.flips)
    e.build_index()
    note("engine built")
    st = torch.cuda.current_stream().cuda_stream
    d_labels = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_degrees = torch.empty((n,), dtype=torch.int32, device="cuda")
    starts = list(range(0, n, B))

    def leg_dbscan():
        return e.dbscan_radius_dev(radius, min_pts, d_labels.data_ptr(), d_degrees.data_ptr(), mode=mode, batch=B, stream=st)

    def leg_cluster():
        return e.cluster_radius_dev(radius, d_labels.data_ptr(), mode=mode, batch=B, stream=st)

    if args.step == "check":
        stats = leg_dbscan()
        torch.cuda.synchronize()
        labels = d_labels.cpu().numpy().view(np.uint32).astype(np.int64)
        degrees = d_degrees.cpu().numpy().view(np.uint32).astype(np.int64)
        c_pairs, n_clusters = leg_cluster()
        torch.cuda.synchronize()
        # the pairs, batch by batch, through the by-id radius search (sizes call first, then the batch's pairs come home)
        d_ids = torch.arange(n, dtype=torch.int32, device="cuda")       # (n < 2^31 here)
        d_off = torch.empty((B + 1,), dtype=torch.int64, device="cuda")
        d_out = torch.empty((1,), dtype=torch.int64, device="cuda")
        qa, qb = [], []
        for lo in starts:
            nq = min(B, n - lo)
            e.search_radius_ids_dev(d_ids[lo:].data_ptr(), nq, radius, None, 0, d_off.data_ptr(), mode=mode, id_flags=vc.IDS_ONLY_GREATER, stream=st)
            torch.cuda.synchronize()
            total = int(d_off[nq].item())
            if total > d_out.numel():
                d_out = torch.empty((total,), dtype=torch.int64, device="cuda")
            if e.search_radius_ids_dev(d_ids[lo:].data_ptr(), nq, radius, d_out.data_ptr(), d_out.numel(), d_off.data_ptr(), mode=mode,
                                       id_flags=vc.IDS_ONLY_GREATER, stream=st) != vc.VC_OK:
                raise SystemExit("pairs do not fit the buffer")
            offs = d_off[:nq + 1].cpu().numpy().view(np.uint64).astype(np.int64)
            qa.append(np.repeat(np.arange(lo, lo + nq, dtype=np.int64), np.diff(offs)))
            qb.append((d_out[:total].cpu().numpy().view(np.uint64) & LOW).astype(np.int64))
        a, b = np.concatenate(qa), np.concatenate(qb)
        assert np.all(b > a) and len(a) == stats["n_pairs"] == c_pairs, "the loop lists %d pairs, the calls examined %d and %d" % (len(a), stats["n_pairs"], c_pairs)
        note("%d pairs at home" % len(a))
        want, deg = host_dbscan(n, a, b, min_pts)
        assert np.array_equal(degrees, deg), "degrees differ from the host count over the loop's pairs"
        assert np.array_equal(labels, want), "labels differ from the host DBSCAN over the loop's pairs"
        own = np.arange(n)
        core = deg >= min_pts
        host = {"n_pairs": len(a), "n_clusters": int((core & (want == own)).sum()), "n_core": int(core.sum()),
                "n_border": int((~core & (want != own)).sum()), "n_noise": int((~core & (want == own)).sum())}
        assert stats == host, "statistics %s, the host counts %s" % (stats, host)
        res = {"labels_and_degrees_equal_host_dbscan": True, "min_pts": min_pts, "batches": len(starts)}
        res.update(stats)
        res["cluster_n_clusters"] = int(n_clusters)
        res["largest_degree"] = int(deg.max())
        note("labels equal: %s" % res)
    else:
        legs = {"dbscan": leg_dbscan, "cluster": leg_cluster}
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
        res = {"call_ms_median": {k: round(float(np.median(v)) * 1e3, 3) for k, v in t.items()},
               "call_ms_min": {k: round(min(v) * 1e3, 3) for k, v in t.items()},
               "call_ms_max": {k: round(max(v) * 1e3, 3) for k, v in t.items()}, "reps": args.reps, "batches": len(starts)}
        med = res["call_ms_median"]
        res["dbscan_over_cluster"] = round(med["dbscan"] / med["cluster"], 3)
        res["extra_us_per_batch"] = round((med["dbscan"] - med["cluster"]) * 1e3 / len(starts), 1)
        note("timed: %s" % res)
    with open(args.step_out, "w") as f:
        json.dump(res, f)
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e6)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--min-pts", type=int, default=4)
    ap.add_argument("--cluster-size", type=int, default=16, help="records per centre of the synthetic data")
    ap.add_argument("--flips", type=int, default=6, help="a record is its centre with up to this many bits flipped")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=35)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a step may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=("check", "time"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--step-out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    line = {"metric": "DBSCAN (min_pts = %d) of the radius-%d graph against its connected components, %.3g clustered 64-bit codes (%d per centre, "
                      "<= %d flips), m=2, exact MIH, batches of %d ids, one engine" % (args.min_pts, args.radius, args.n, args.cluster_size, args.flips, args.batch)}
    with tempfile.TemporaryDirectory() as td:
        for name in ("check", "time"):      # chained: a step that fails, faults or runs into its time limit ends the run
            part = os.path.join(td, name + ".json")
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--step-out", part]
            for k in ("n", "batch", "radius", "min_pts", "cluster_size", "flips", "reps", "seed"):
                cmd += ["--" + k.replace("_", "-"), str(getattr(args, k))]
            rc = subprocess.call(cmd)
            if rc != 0:
                raise SystemExit("step %s ended with status %d: nothing further is started" % (name, rc))
            line[name] = json.load(open(part))
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
