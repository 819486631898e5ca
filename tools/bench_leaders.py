"""Greedy leader dedup on the device (vc_leaders_radius_dev) against the single-linkage clustering next to it (vc_cluster_radius_dev,
the yardstick: existing code over the same radius searches), on tools/bench_cluster.py's data and parameters: clustered synthetic
64-bit codes, all neighbours within R = 8, m = 2, exact MIH, one engine, 1e6 records in 62 500 clusters of about 16, batches of
4 096 ids.

  leaders      vc_leaders_radius_dev from scratch: per batch fill ids, gather, radius search, then the decision rounds over the raw
               result (groups of rounds between two read-backs of the undecided counter) and the assign pass; one count at the end
  cluster      vc_cluster_radius_dev from scratch on the same handle: the same batches and searches, one union launch per batch

Two steps, each a child process under its own `timeout`, the second only after the first succeeded:
  check   labels of `leaders` == a host greedy pass over the pairs that vc_search_radius_ids_dev + VC_IDS_ONLY_GREATER lists
          (asserted), n_pairs == their number, n_rounds == a host model of the rounds batch by batch (asserted); written down: the
          leaders, the rounds per batch (mean and max), the members not within R of their label for both calls
  time    the two legs interleaved, a host clock around each leg ending in a device synchronise, medians of --reps
No ratio is fixed in advance: both legs spend their time in the same radius searches, the leaders call adds its round launches and
one wait per group of rounds.  Prints one JSON line; --out also writes it to a file.

    python tools/bench_leaders.py [--n 1e6] [--reps 7] [--out profiles/leaders_bench.json]
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


def host_greedy(n, a, b):
    """labels by the sequential rule: in id order, a record is kept iff no kept record so far is adjacent; a dropped record takes its
    smallest kept neighbour.  (a, b): every pair once, a < b."""
    order = np.argsort(b, kind="stable")
    nb = a[order].tolist()
    start = np.zeros(n + 1, dtype=np.int64)
    start[1:] = np.cumsum(np.bincount(b, minlength=n))
    start = start.tolist()
    lab = list(range(n))
    leader = [False] * n
    for i in range(n):
        best = -1
        for v in nb[start[i]:start[i + 1]]:
            if leader[v] and (best < 0 or v < best):
                best = v
        if best < 0:
            leader[i] = True
        else:
            lab[i] = best
    return np.array(lab, dtype=np.int64)


def host_rounds_per_batch(n, a, b, batch, lab):
    """the rounds that have work, per batch, by the device's schedule run on all batches at once: round 1 drops a record on a
    leader below its batch (final: lab[v] == v) and keeps one without a smaller neighbour inside its batch; every later round is
    the eager rule on the state the previous round left"""
    first = (np.arange(n) // batch) * batch
    n_batches = (n + batch - 1) // batch
    leader_final = lab == np.arange(n)
    past = a < first[b]
    past_drop = np.bincount(b[past & leader_final[a]], minlength=n) > 0
    ia, ib = a[~past], b[~past]
    has_inside = np.bincount(ib, minlength=n) > 0
    U, L, D = 0, 1, 2
    state = np.full(n, U, dtype=np.int8)
    state[past_drop] = D
    state[~past_drop & ~has_inside] = L
    rounds = np.ones(n_batches, dtype=np.int64)
    while True:
        und = state == U
        open_batches = np.unique(np.flatnonzero(und) // batch)
        if len(open_batches) == 0:
            break
        rounds[open_batches] += 1
        live = und[ib]
        ia, ib = ia[live], ib[live]
        sa = state[ia]
        has_leader = np.bincount(ib[sa == L], minlength=n) > 0
        blocked = np.bincount(ib[sa == U], minlength=n) > 0
        state[und & has_leader] = D
        state[und & ~has_leader & ~blocked] = L
    assert np.array_equal(state == L, leader_final)
    return rounds


def far_members(lab, a, b):
    """members (label != own id) that are not within R of their label"""
    member = np.flatnonzero(lab != np.arange(len(lab)))
    link = (lab[member].astype(np.uint64) << np.uint64(32)) | member.astype(np.uint64)
    return int((~np.isin(link, (a.astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64))).sum())


def step(args):
    import torch
    from verticut_amd import engine as vc
    n, bits, m, B, radius = int(args.n), 64, 2, args.batch, args.radius
    mode = vc.MODE_MIH_EXACT

    def note(what):
        print("[bench_leaders] %s" % what, file=sys.stderr, flush=True)

    e = vc.Engine(bits, capacity=n, n_tables=m, flags=vc.FLAG_LEAN_TIMING)
    e.add_synthetic(n, seed=args.seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // args.cluster_size, 1), max_flips=args.flips)
    e.build_index()
    note("engine built")
    st = torch.cuda.current_stream().cuda_stream
    d_labels = torch.empty((n,), dtype=torch.int32, device="cuda")
    starts = list(range(0, n, B))

    def leg_leaders():
        return e.leaders_radius_dev(radius, d_labels.data_ptr(), mode=mode, batch=B, stream=st)

    def leg_cluster():
        return e.cluster_radius_dev(radius, d_labels.data_ptr(), mode=mode, batch=B, stream=st)

    if args.step == "check":
        n_pairs, n_leaders, n_rounds = leg_leaders()
        torch.cuda.synchronize()
        labels = d_labels.cpu().numpy().view(np.uint32).astype(np.int64)
        c_pairs, n_clusters = leg_cluster()
        torch.cuda.synchronize()
        c_labels = d_labels.cpu().numpy().view(np.uint32).astype(np.int64)
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
        assert np.all(b > a) and len(a) == n_pairs == c_pairs, "the loop lists %d pairs, the calls examined %d and %d" % (len(a), n_pairs, c_pairs)
        note("%d pairs at home" % len(a))
        want = host_greedy(n, a, b)
        assert np.array_equal(labels, want), "labels differ from the host greedy pass over the loop's pairs"
        assert n_leaders == int((want == np.arange(n)).sum())
        rounds = host_rounds_per_batch(n, a, b, B, want)
        assert int(rounds.sum()) == n_rounds, "the host model counts %d rounds, the call %d" % (int(rounds.sum()), n_rounds)
        lead = want == np.arange(n)
        res = {"labels_equal_host_greedy": True, "n_pairs": int(n_pairs), "n_leaders": int(n_leaders), "n_rounds": int(n_rounds),
               "batches": len(starts), "rounds_per_batch_mean": round(float(rounds.mean()), 2), "rounds_per_batch_max": int(rounds.max()),
               "rounds_per_batch_histogram": {str(k): int(v) for k, v in zip(*np.unique(rounds, return_counts=True))},
               "round_group": vc.LEADER_ROUND_GROUP,
               "leaders_members_not_within_r_of_their_label": far_members(want, a, b),
               "leader_pairs_within_r": int((lead[a] & lead[b]).sum()),
               "cluster_n_clusters": int(n_clusters), "cluster_members_not_within_r_of_their_label": far_members(c_labels, a, b)}
        assert res["leaders_members_not_within_r_of_their_label"] == 0 and res["leader_pairs_within_r"] == 0
        note("labels equal: %s" % res)
    else:
        legs = {"leaders": leg_leaders, "cluster": leg_cluster}
        for fn in legs.values():       # every buffer of the timed window warm
            fn()
        torch.cuda.synchronize()
        t = {name: [] for name in legs}
        n_rounds = 0
        for _ in range(args.reps):
            for name, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                t[name].append(time.perf_counter() - t0)
                if name == "leaders":
                    n_rounds = out[2]
        res = {"call_ms_median": {k: round(float(np.median(v)) * 1e3, 3) for k, v in t.items()},
               "call_ms_min": {k: round(min(v) * 1e3, 3) for k, v in t.items()},
               "call_ms_max": {k: round(max(v) * 1e3, 3) for k, v in t.items()}, "reps": args.reps, "batches": len(starts)}
        med = res["call_ms_median"]
        res["leaders_over_cluster"] = round(med["leaders"] / med["cluster"], 3)
        res["extra_us_per_batch"] = round((med["leaders"] - med["cluster"]) * 1e3 / len(starts), 1)
        res["extra_us_per_round_with_work"] = round((med["leaders"] - med["cluster"]) * 1e3 / max(n_rounds, 1), 1)
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
    line = {"metric": "greedy leaders of the radius-%d graph against its connected components, %.3g clustered 64-bit codes (%d per centre, <= %d flips), "
                      "m=2, exact MIH, batches of %d ids, one engine" % (args.radius, args.n, args.cluster_size, args.flips, args.batch)}
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
