"""Label groups summarised on the device (vc_group_summary_dev) against the call that made the labels (vc_dbscan_radius_dev, the scale
it is to be compared with) and against the host path it replaces, on the benches' standing shape: clustered synthetic 64-bit codes,
R = 8, m = 2, exact MIH, one engine, 1e6 records, labels from vc_dbscan_radius_dev with min_pts = 4.

  summary      vc_group_summary_dev on the DBSCAN labels: groups, centroids, rep_labels, group_index, groups_cap = N
  dbscan       vc_dbscan_radius_dev on the same handle
  host         the path replaced: N codes (vc_get_codes_dev of all ids) and N labels copied home, then numpy -- a stable sort,
               unpackbits, add.reduceat for the votes, the distances, minimum.reduceat for the representatives
  singletons   summary on hand-made labels: every record its own group
  one_group    summary on hand-made labels: one group of N
  gather       vc_get_codes_dev of the ids in the summary's sorted order alone: the codes per second it fetches (one 64-byte
               sector each at 64 bits), next to the random-sector ceiling bench.py prices the MIH kernels against

Every output of the three summary legs is asserted equal to the numpy result in the same run, before anything is timed.  A host
clock around each leg ending in a device synchronise, legs interleaved, medians of --reps.  No time or ratio is fixed in advance.
The run is one child process under its own `timeout`.  Prints one JSON line; --out also writes it.

    python tools/bench_groups.py [--n 1e6] [--reps 7] [--out profiles/groups_bench.json]
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
SECTOR_PEAK_G = 54.0   # bench.py's SECTOR_PEAK_G: tools/ubench_sectors.hip, independent random-sector loads over a 2 GB footprint


def host_summary(codes, labels):
    """(label, size, rep, rep_dist, max_dist per group; centroids; rep_labels; group_index) by the header's rule, id_base 0"""
    n = len(labels)
    order = np.argsort(labels, kind="stable")
    sk = labels[order]
    head = np.r_[True, sk[1:] != sk[:-1]]
    starts = np.flatnonzero(head)
    sizes = np.diff(np.r_[starts, n])
    of = np.cumsum(head) - 1
    bits = np.unpackbits(codes[order], axis=1, bitorder="little")
    cent = (2 * np.add.reduceat(bits, starts, axis=0, dtype=np.int32) > sizes[:, None]).astype(np.uint8)
    dist = (bits ^ cent[of]).sum(axis=1, dtype=np.int64)
    best = np.minimum.reduceat((dist << 32) | order, starts)
    rep = best & 0xFFFFFFFF
    rep_labels, group_index = np.empty(n, np.int64), np.empty(n, np.int64)
    rep_labels[order], group_index[order] = rep[of], of
    return ((sk[starts], sizes, rep, best >> 32, np.maximum.reduceat(dist, starts)), np.packbits(cent, axis=1, bitorder="little"), rep_labels,
            group_index)


def step(args):
    import torch
    from verticut_amd import engine as vc
    n, bits, m, radius, min_pts = int(args.n), 64, 2, args.radius, args.min_pts
    mode = vc.MODE_MIH_EXACT

    def note(what):
        print("[bench_groups] %s" % what, file=sys.stderr, flush=True)

    e = vc.Engine(bits, capacity=n, n_tables=m, flags=vc.FLAG_LEAN_TIMING)
    e.add_synthetic(n, seed=args.seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // args.cluster_size, 1), max_flips=args.flips)
    e.build_index()
    note("engine built")
    st = torch.cuda.current_stream().cuda_stream
    i32 = dict(dtype=torch.int32, device="cuda")
    d_labels, d_degrees = torch.empty((n,), **i32), torch.empty((n,), **i32)
    d_groups, d_cents = torch.empty((n, 6), **i32), torch.empty((n, bits // 32), **i32)
    d_rep, d_gi = torch.empty((n,), **i32), torch.empty((n,), **i32)
    d_all = torch.arange(n, **i32)                                    # (n < 2^31 here)
    d_codes = torch.empty((n, bits // 32), **i32)

    def leg_dbscan():
        return e.dbscan_radius_dev(radius, min_pts, d_labels.data_ptr(), d_degrees.data_ptr(), mode=mode, batch=args.batch, stream=st)

    def summary_on(d_lab):
        def leg():
            rc, G = e.group_summary_dev(d_lab.data_ptr(), n, d_groups.data_ptr(), d_cents.data_ptr(), d_rep.data_ptr(), d_gi.data_ptr(), stream=st)
            assert rc == vc.VC_OK
            return G
        return leg

    def home(t):
        return t.cpu().numpy().view(np.uint32)

    def leg_host():
        e.get_codes_dev(d_all.data_ptr(), n, d_codes.data_ptr(), stream=st)
        codes = d_codes.cpu().numpy().view(np.uint8).reshape(n, bits // 8)
        return host_summary(codes, home(d_labels).astype(np.int64))

    stats = leg_dbscan()
    torch.cuda.synchronize()
    e.get_codes_dev(d_all.data_ptr(), n, d_codes.data_ptr(), stream=st)
    codes = d_codes.cpu().numpy().view(np.uint8).reshape(n, bits // 8).copy()
    d_single, d_one = d_all.flip(0).contiguous(), torch.full((n,), n // 2, **i32)
    checked = {}
    for name, d_lab in (("summary", d_labels), ("singletons", d_single), ("one_group", d_one)):
        G = summary_on(d_lab)()
        torch.cuda.synchronize()
        (lab, size, rep, rep_dist, max_dist), cent, rep_labels, group_index = host_summary(codes, home(d_lab).astype(np.int64))
        got = home(d_groups)[:G]
        assert G == len(lab), "%s: %d groups, the host counts %d" % (name, G, len(lab))
        for k, want in enumerate((lab, size, rep, rep_dist, max_dist, np.zeros(G, np.int64))):
            assert np.array_equal(got[:, k], want), "%s: groups field %d differs from the host result" % (name, k)
        assert np.array_equal(home(d_cents)[:G].view(np.uint8).reshape(G, bits // 8), cent), "%s: centroids differ" % name
        assert np.array_equal(home(d_rep), rep_labels) and np.array_equal(home(d_gi), group_index), "%s: rep_labels / group_index differ" % name
        checked[name] = {"groups": int(G), "largest": int(size.max()), "groups_of_1_or_2": int((size <= 2).sum()), "groups_above_1024": int((size > 1024).sum()),
                         "representative_is_not_the_label": int((rep != lab).sum()), "mean_max_dist": round(float(max_dist.mean()), 3)}
        note("%s equal to the host result: %s" % (name, checked[name]))
    order = torch.from_numpy(np.argsort(home(d_labels), kind="stable").astype(np.int32)).cuda()

    def leg_gather():
        e.get_codes_dev(order.data_ptr(), n, d_codes.data_ptr(), stream=st)

    legs = {"summary": summary_on(d_labels), "dbscan": leg_dbscan, "host": leg_host, "singletons": summary_on(d_single), "one_group": summary_on(d_one),
            "gather": leg_gather}
    for fn in legs.values():
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
    res = {"outputs_equal_numpy": True, "dbscan_stats": stats, "checked": checked,
           "call_ms_median": {k: round(float(np.median(v)) * 1e3, 3) for k, v in t.items()},
           "call_ms_min": {k: round(min(v) * 1e3, 3) for k, v in t.items()},
           "call_ms_max": {k: round(max(v) * 1e3, 3) for k, v in t.items()}, "reps": args.reps}
    med = res["call_ms_median"]
    res["summary_over_dbscan"] = round(med["summary"] / med["dbscan"], 4)
    res["host_over_summary"] = round(med["host"] / med["summary"], 2)
    g_codes = n / (med["gather"] * 1e-3) / 1e9
    res["gather"] = {"codes_per_s_G": round(g_codes, 3), "useful_bytes_per_s_G": round(g_codes * bits / 8, 2), "sector_bytes_per_s_G": round(g_codes * 64, 2),
                     "sectors_per_code": bits // 64, "random_sector_ceiling_G_per_s": SECTOR_PEAK_G, "of_the_ceiling": round(g_codes * (bits // 64) / SECTOR_PEAK_G, 4),
                     "how": "vc_get_codes_dev of the N ids in sorted order, host clock; the ceiling is bench.py's SECTOR_PEAK_G (tools/ubench_sectors.hip)"}
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
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds the run may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--step-out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    line = {"metric": "group summary of DBSCAN labels (min_pts = %d, radius %d) against the DBSCAN call and the host path it replaces, %.3g clustered "
                      "64-bit codes (%d per centre, <= %d flips), m=2, exact MIH, one engine" % (args.min_pts, args.radius, args.n, args.cluster_size, args.flips)}
    with tempfile.TemporaryDirectory() as td:
        part = os.path.join(td, "run.json")
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", "--step-out", part]
        for k in ("n", "batch", "radius", "min_pts", "cluster_size", "flips", "reps", "seed"):
            cmd += ["--" + k.replace("_", "-"), str(getattr(args, k))]
        rc = subprocess.call(cmd)
        if rc != 0:
            raise SystemExit("the run ended with status %d" % rc)
        line.update(json.load(open(part)))
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
