"""Near-duplicate clustering on the device (vc_cluster_radius_dev) against what a caller did before it existed: clustered synthetic
64-bit codes at BASELINE configs[1]'s parameters (all neighbours within R = 8, m = 2, exact MIH), one engine.  Default size: 1e6
records in 62 500 clusters of about 16 (centre + up to 6 flipped bits, so members of a cluster are up to 12 bits apart and a
component is not a clique); a whole run stays well under a minute.

  cluster      vc_cluster_radius_dev from scratch: per batch of 4 096 ids fill ids, gather, radius search, union over the raw
               result; one flatten, one wait for the statistics
  loop         the same walk in the same batch size through vc_search_radius_ids_dev with VC_IDS_ONLY_GREATER -- the device loop
               alone, the pairs stay in HBM and nothing is clustered yet
  loop_home    that loop with every batch's offsets and pairs copied home (what a host union-find needs)

Two steps, each a child process under its own `timeout`, the second only after the first succeeded:
  check   labels of `cluster` == a host union-find over the pairs of `loop_home` (asserted), n_pairs == their number
  time    the three legs interleaved, a host clock around each leg ending in a device synchronise, medians of --reps
No ratio is fixed in advance: the expectation to confirm or refute is cluster <= loop, since it skips the compaction.
Prints one JSON line; --out also writes it to a file.

    python tools/bench_cluster.py [--n 1e6] [--reps 7] [--out profiles/cluster_bench.json]
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


def host_union_find(n, a, b):
    """labels = smallest id of each component: rounds of (hook the larger root under the smaller, for every pair at once; pointer
    jumping) until no pair joins two roots"""
    lab = np.arange(n, dtype=np.int64)
    while True:
        ra, rb = lab[a], lab[b]
        live = ra != rb
        if not live.any():
            return lab
        a, b, ra, rb = a[live], b[live], ra[live], rb[live]
        hi, lo = np.maximum(ra, rb), np.minimum(ra, rb)
        order = np.argsort(hi, kind="stable")
        hi, lo = hi[order], lo[order]
        start = np.flatnonzero(np.r_[True, hi[1:] != hi[:-1]])
        lab[hi[start]] = np.minimum(lab[hi[start]], np.minimum.reduceat(lo, start))
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt


def step(args):
    import torch
    from verticut_amd import engine as vc
    n, bits, m, B, radius = int(args.n), 64, 2, args.batch, args.radius
    mode = vc.MODE_MIH_EXACT

    def note(what):
        print("[bench_cluster] %s" % what, file=sys.stderr, flush=True)

    e = vc.Engine(bits, capacity=n, n_tables=m, flags=vc.FLAG_LEAN_TIMING)
    e.add_synthetic(n, seed=args.seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // args.cluster_size, 1), max_flips=args.flips)
    e.build_index()
    note("engine built")
    st = torch.cuda.current_stream().cuda_stream
    d_labels = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_ids = torch.arange(n, dtype=torch.int32, device="cuda")       # (n < 2^31 here)
    d_off = torch.empty((B + 1,), dtype=torch.int64, device="cuda")
    starts = list(range(0, n, B))

    def leg_cluster():
        return e.cluster_radius_dev(radius, d_labels.data_ptr(), mode=mode, batch=B, stream=st)

    # size the loop's output buffer once, from the sizes call of every batch (not timed)
    cap = 0
    for lo in starts:
        nq = min(B, n - lo)
        rc = e.search_radius_ids_dev(d_ids[lo:].data_ptr(), nq, radius, None, 0, d_off.data_ptr(), mode=mode, id_flags=vc.IDS_ONLY_GREATER, stream=st)
        torch.cuda.synchronize()
        cap = max(cap, int(d_off[nq].item()))
    d_out = torch.empty((max(cap, 1),), dtype=torch.int64, device="cuda")
    note("largest batch holds %d pairs" % cap)

    def leg_loop(home=None):
        for lo in starts:
            nq = min(B, n - lo)
            if e.search_radius_ids_dev(d_ids[lo:].data_ptr(), nq, radius, d_out.data_ptr(), cap, d_off.data_ptr(), mode=mode,
                                       id_flags=vc.IDS_ONLY_GREATER, stream=st) != vc.VC_OK:
                raise SystemExit("pairs do not fit the buffer")
            if home is not None:
                offs = d_off[:nq + 1].cpu().numpy().view(np.uint64)
                home.append((lo, offs, d_out[:int(offs[nq])].cpu().numpy().view(np.uint64)))

    if args.step == "check":
        n_pairs, n_clusters = leg_cluster()
        torch.cuda.synchronize()
        labels = d_labels.cpu().numpy().view(np.uint32).astype(np.int64)
        home = []
        leg_loop(home)
        a = np.concatenate([np.repeat(np.arange(lo, lo + len(offs) - 1, dtype=np.int64), np.diff(offs.astype(np.int64))) for lo, offs, _ in home])
        b = np.concatenate([flat for _, _, flat in home])
        b = (b & LOW).astype(np.int64)
        assert np.all(b > a) and len(a) == n_pairs, "the loop lists %d pairs, the call examined %d" % (len(a), n_pairs)
        want = host_union_find(n, a, b)
        assert np.array_equal(labels, want), "labels differ from the host union-find over the loop's pairs"
        _, sizes = np.unique(want, return_counts=True)
        assert len(sizes) == n_clusters
        member = np.flatnonzero(want != np.arange(n))
        direct = np.isin((want[member].astype(np.uint64) << np.uint64(32)) | member.astype(np.uint64), (a.astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64))
        res = {"labels_equal_host_union_find": True, "n_pairs": int(n_pairs), "n_clusters": int(n_clusters), "largest_cluster": int(sizes.max()),
               "singletons": int((sizes == 1).sum()), "members_not_adjacent_to_their_label": int((~direct).sum()), "largest_batch_pairs": cap}
        note("labels equal: %s" % res)
    else:
        legs = {"cluster": leg_cluster, "loop": leg_loop, "loop_home": lambda: leg_loop([])}
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
        res["cluster_over_loop"] = round(med["cluster"] / med["loop"], 3)
        res["cluster_over_loop_home"] = round(med["cluster"] / med["loop_home"], 3)
        note("timed: %s" % res)
    with open(args.step_out, "w") as f:
        json.dump(res, f)
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e6)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--radius", type=int, default=8)
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
    line = {"metric": "connected components of the radius-%d graph, %.3g clustered 64-bit codes (%d per centre, <= %d flips), m=2, exact MIH, "
                      "batches of %d ids, one engine" % (args.radius, args.n, args.cluster_size, args.flips, args.batch)}
    with tempfile.TemporaryDirectory() as td:
        for name in ("check", "time"):      # chained: a step that fails, faults or runs into its time limit ends the run
            part = os.path.join(td, name + ".json")
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--step-out", part]
            for k in ("n", "batch", "radius", "cluster_size", "flips", "reps", "seed"):
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
