"""Shared-nearest-neighbour clustering of a built k-NN graph (vc_cluster_snn_dev) against its floor and the path it replaces: clustered
synthetic 64-bit codes (the store of bench_knn_graph.py: 1e6 records, 16 per centre, up to 6 flipped bits), m = 2, the graph built
once by vc_knn_graph_dev in exact MIH, one engine, k = kk = 10 and k = kk = 100, VC_KNN_MUTUAL, no cap, min_shared = kk / 2.

  snn          vc_cluster_snn_dev with the weights and the histogram written: N * kk list intersections of kk probes each
  snn_labels   the same with d_shared and d_hist NULL
  cluster_knn  vc_cluster_knn_dev on the same graph: the same edges without the intersections -- the floor
  host         the replaced path, once: the rows copied home, the intersections in numpy (a membership table per chunk of rows, one
               gather per chunk).  N * kk^2 probes are 10^10 at kk = 100, so the intersections run over about --host-probes / kk^2
               evenly spaced rows when that is fewer than N, and their time is scaled
               to N rows: the JSON says `host_rows` and `host_intersect_extrapolated`.  The timed host leg is the copy and the
               intersections alone; the mutual test and the union-find, which the labels need on top, run in the check step

Per k two steps, each a child process under its own `timeout`, the next only after the one before succeeded:
  check   weights of `snn` == the host intersections on the host's rows (asserted); histogram == the count of the weights (the host's
          where it has all rows, else the device's own -- said in the JSON); labels == a host union-find over the mutual pairs at or
          above the threshold (asserted); the five statistics (asserted)
  time    the three device legs interleaved, a host clock around each ending in a device synchronise, medians of --reps with
          min .. max; then the host leg once
No ratio is fixed in advance.  Prints one JSON line; --out also writes it to a file.

    python tools/bench_snn.py [--n 1e6] [--ks 10,100] [--reps 7] [--out profiles/snn_bench.json]
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
from tools.bench_cluster import host_union_find  # noqa: E402

LOW = np.uint64(0xFFFFFFFF)
NONE = 0xFFFFFFFF


def host_rows(n, kk, budget):
    """the rows the host intersects: all of them, or every step-th so that about budget / kk^2 are taken"""
    want = max(int(budget) // (kk * kk), 1)
    return np.arange(n, dtype=np.int64) if want >= n else np.arange(0, n, -(-n // want), dtype=np.int64)


def host_intersections(ids, sel, chunk=128):
    """shared[r, jj] = |S_i & S_j| for i = sel[r], j = ids[i, jj]: per chunk of rows a membership table [chunk, N] of bytes, set at the
    rows' own ids, read at their neighbours' ids in one gather, cleared again"""
    n, kk = ids.shape
    out = np.empty((len(sel), kk), dtype=np.uint32)
    table = np.zeros((chunk, n), dtype=np.uint8)
    for lo in range(0, len(sel), chunk):
        own = ids[sel[lo:lo + chunk]]                                   # [c, kk]
        c = len(own)
        r = np.arange(c)[:, None]
        table[r, own] = 1
        out[lo:lo + c] = table[r[:, :, None], ids[own]].sum(axis=2, dtype=np.uint32)   # ids[own]: [c, kk, kk], row j's list for every entry
        table[r, own] = 0
    return out


def host_mutual(ids):
    """mutual[i, jj]: row ids[i, jj] lists i in turn -- edges as sorted keys, no one-compare trick"""
    n, kk = ids.shape
    src = np.repeat(np.arange(n, dtype=np.uint64), kk)
    dst = ids.reshape(-1).astype(np.uint64)
    keys = np.sort((src << np.uint64(32)) | dst)
    back = (dst << np.uint64(32)) | src
    pos = np.searchsorted(keys, back)
    return (keys[np.minimum(pos, len(keys) - 1)] == back).reshape(n, kk)


def step(args):
    import torch
    from verticut_amd import engine as vc
    n, bits, m, k = int(args.n), 64, 2, args.k
    kk, min_shared = k, k // 2

    def note(what):
        print("[bench_snn k=%d] %s" % (k, what), file=sys.stderr, flush=True)

    e = vc.Engine(bits, capacity=n, n_tables=m, flags=vc.FLAG_LEAN_TIMING)
    e.add_synthetic(n, seed=args.seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // args.cluster_size, 1), max_flips=args.flips)
    e.build_index()
    st = torch.cuda.current_stream().cuda_stream
    d_rows = torch.empty((n, k), dtype=torch.int64, device="cuda")
    d_counts = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_labels = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_deg = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_shared = torch.empty((n, kk), dtype=torch.int32, device="cuda")
    d_hist = torch.empty((kk,), dtype=torch.int64, device="cuda")
    e.knn_graph_dev(k, d_rows.data_ptr(), d_counts.data_ptr(), mode=vc.MODE_MIH_EXACT, batch=args.batch, stream=st)
    torch.cuda.synchronize()
    note("graph built")

    def leg_snn(weights=True):
        return e.cluster_snn_dev(d_rows.data_ptr(), d_counts.data_ptr(), k, kk, min_shared, d_labels.data_ptr(), d_shared.data_ptr() if weights else None,
                                 d_hist.data_ptr() if weights else None, stream=st)

    def leg_cluster():
        return e.cluster_knn_dev(d_rows.data_ptr(), d_counts.data_ptr(), k, kk, d_labels.data_ptr(), d_deg.data_ptr(), stream=st)

    def leg_host(with_mutual=True):
        """(seconds by part, ids, sel, shared of sel, mutual | None)"""
        t0 = time.perf_counter()
        rows = d_rows.cpu().numpy().view(np.uint64)
        t1 = time.perf_counter()
        ids = (rows & LOW).astype(np.int64)
        sel = host_rows(n, kk, args.host_probes)
        shared = host_intersections(ids, sel)
        t2 = time.perf_counter()
        mutual = host_mutual(ids) if with_mutual else None
        t3 = time.perf_counter()
        return {"copy_home": t1 - t0, "intersect": (t2 - t1) * n / len(sel), "mutual": t3 - t2}, ids, sel, shared, mutual

    if args.step == "check":
        assert np.all(d_counts.cpu().numpy().view(np.uint32) == min(k, n - 1)) and n > k
        stats = leg_snn()
        torch.cuda.synchronize()
        got_shared = d_shared.cpu().numpy().view(np.uint32)
        got_hist = d_hist.cpu().numpy().view(np.uint64)
        got_labels = d_labels.cpu().numpy().view(np.uint32).astype(np.int64)
        _, ids, sel, shared, mutual = leg_host()
        full = len(sel) == n
        assert np.array_equal(got_shared[sel], shared), "weights differ from the host intersections"
        note("weights equal the host intersections on %d rows" % len(sel))
        weights = shared if full else got_shared          # every entry is listed here: no cap, counts == k
        assert not np.any(weights == NONE) and int(weights.max()) < kk
        assert np.array_equal(got_hist, np.bincount(weights.reshape(-1).astype(np.int64), minlength=kk).astype(np.uint64)), "histogram differs"
        src = np.repeat(np.arange(n, dtype=np.int64), kk).reshape(n, kk)
        join = mutual & (weights >= min_shared) & (src < ids)
        labels = host_union_find(n, src[join], ids[join])
        assert np.array_equal(got_labels, labels), "labels differ from the host union-find"
        want = {"n_edges": n * kk, "n_mutual": int((mutual & (src < ids)).sum()), "n_joined": int(join.sum()), "n_clusters": len(np.unique(labels)),
                "max_shared": int(weights.max())}
        assert stats == want, (stats, want)
        labels_only = leg_snn(False)
        torch.cuda.synchronize()
        assert labels_only == stats and np.array_equal(d_labels.cpu().numpy().view(np.uint32).astype(np.int64), labels)
        res = {"weights_equal_host_intersections": True, "host_rows": int(len(sel)), "histogram_equals_count_of": "host weights" if full else "device weights",
               "labels_equal_host_union_find_over": "host weights" if full else "device weights", "stats_equal_host": True, "snn_stats": stats,
               "min_shared": min_shared, "hist": [int(x) for x in got_hist]}
        note("labels, histogram and statistics equal the host model: %s" % stats)
    else:
        legs = {"snn": leg_snn, "snn_labels": lambda: leg_snn(False), "cluster_knn": leg_cluster}
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
        parts, ids, sel, shared, _ = leg_host(False)     # the copy and the intersections; the mutual test and the union-find come on top (check step)
        del parts["mutual"]
        res = {"call_ms_median": {q: round(float(np.median(v)) * 1e3, 3) for q, v in t.items()},
               "call_ms_min": {q: round(min(v) * 1e3, 3) for q, v in t.items()},
               "call_ms_max": {q: round(max(v) * 1e3, 3) for q, v in t.items()}, "reps": args.reps,
               "host_s": {q: round(v, 3) for q, v in parts.items()}, "host_s_total": round(sum(parts.values()), 3), "host_rows": int(len(sel)),
               "host_intersect_extrapolated": bool(len(sel) != n)}
        med = res["call_ms_median"]
        res["probes"] = n * kk * kk
        res["snn_probes_per_s"] = round(n * kk * kk / (med["snn"] * 1e-3), 0)
        res["host_probes_per_s"] = round(n * kk * kk / parts["intersect"], 0)
        res["snn_over_cluster_knn"] = round(med["snn"] / med["cluster_knn"], 2)
        res["host_over_snn"] = round(res["host_s_total"] * 1e3 / med["snn"], 1)
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
    ap.add_argument("--host-probes", type=float, default=1e9, help="set probes the host intersects; fewer than N kk^2: every step-th row, time scaled")
    ap.add_argument("--step-timeout", type=int, default=400, help="seconds a step may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=("check", "time"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--step-out", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--k", type=int, default=10, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    line = {"metric": "shared-nearest-neighbour clusters of a built exact k-NN graph, %.3g clustered 64-bit codes (%d per centre, <= %d flips), "
                      "kk = k, VC_KNN_MUTUAL, no cap, min_shared = kk / 2, one engine" % (args.n, args.cluster_size, args.flips)}
    with tempfile.TemporaryDirectory() as td:
        for k in [int(x) for x in args.ks.split(",")]:
            line["k=%d" % k] = {}
            for name in ("check", "time"):      # chained: a step that fails, faults or runs into its time limit ends the run
                part = os.path.join(td, "%s_%d.json" % (name, k))
                cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--step-out", part, "--k", str(k)]
                for key in ("n", "batch", "cluster_size", "flips", "reps", "seed", "host_probes"):
                    cmd += ["--" + key.replace("_", "-"), str(getattr(args, key))]
                rc = subprocess.call(cmd)
                if rc != 0:
                    raise SystemExit("step %s at k=%d ended with status %d: nothing further is started" % (name, k, rc))
                line["k=%d" % k][name] = json.load(open(part))
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
