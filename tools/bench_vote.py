"""The k-NN label vote (vc_knn_vote_dev) and label propagation (vc_label_propagate_dev) against their floor and the path they replace:
clustered synthetic 64-bit codes (the store of bench_knn_graph.py: 1e6 records, 16 per centre, up to 6 flipped bits), m = 2, the
graph built once per k by vc_knn_graph_dev in exact MIH and turned round by vc_knn_adjacency_dev, one engine, k = kk = 10 and 100.

  vote_count / vote_closeness    vc_knn_vote_dev over the graph's rows, 40 % of the records labelled with one of 16 classes (the class
                                 of a record: its component in the mutual graph of its first 10 entries, mod 16; --noise of the tags
                                 are replaced by a random class, so that segments hold several labels and ties occur)
  round_<flag>                   vc_label_propagate_dev(max_iters = 1) on the VC_KNN_EITHER / MUTUAL / REVERSE adjacency: the plan
                                 pass and ONE round per bin mix (the mix is reported)
  semi / community               vc_label_propagate_dev on the VC_KNN_EITHER adjacency to convergence or VC_LP_MAX_ITERS: --seeds
                                 clamped seeds / labels = ids; n_iters reported, per_round_ms = (call - round_either) / (n_iters - 1)
  cluster_knn                    vc_cluster_knn_dev (VC_KNN_MUTUAL, kk = k) on the same graph and handle: the one-gather-per-entry floor
  host                           the replaced path, once: rows (or CSR) and labels copied home and tallied in numpy -- one stable sort
                                 of (segment, label) keys, np.add.reduceat, np.maximum.reduceat over the winner keys

Per k one child process under its own `timeout`, the next only after the one before succeeded.  In it, before anything is timed,
every output word (labels, votes, totals, statistics) of both vote kinds is asserted equal to the host model over the whole store;
propagation is asserted round by round over the whole store (every round up to --check-rounds of each form, and the last round from
the device's own labels one round earlier).  Then the device legs interleaved, a host clock around each ending in a device
synchronise, medians of --reps with min .. max.  No ratio is fixed in advance.  Prints one JSON line; --out also writes it.

    python tools/bench_vote.py [--n 1e6] [--ks 10,100] [--reps 7] [--out profiles/knn_vote_bench.json]
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
NONE = 0xFFFFFFFF
BIN_TOPS = (8, 16, 32, 64, 256, 1024, 8192)
BIN_NAMES = ("P8", "P16", "P32", "P64", "WAVE", "SMALL", "BIG", "LONG")


def host_tally(seg, pos, words, labels, current, kind, bits, n_segs):
    """The vote rule for flat entries (segment number ascending, position within the segment, packed word) under `labels`; current:
    [n_segs] labels or None.  Returns (winner, votes, total uint32 [n_segs], has [n_segs] bool, ties [n_segs] bool)."""
    lab = labels[(words & LOW).astype(np.int64)]
    keep = lab != NONE
    seg, pos, lab = seg[keep], pos[keep], lab[keep].astype(np.uint64)
    wt = (np.uint64(bits + 1) - (words[keep] >> np.uint64(32))) if kind else np.ones(len(seg), dtype=np.uint64)
    order = np.argsort((seg.astype(np.uint64) << np.uint64(32)) | lab, kind="stable")     # runs of (segment, label), positions ascending within
    seg, pos, lab, wt = seg[order], pos[order], lab[order], wt[order]
    start = np.nonzero(np.r_[True, (seg[1:] != seg[:-1]) | (lab[1:] != lab[:-1])])[0] if len(seg) else np.zeros(0, dtype=np.int64)
    winner, votes, total = np.full(n_segs, NONE, dtype=np.uint32), np.zeros(n_segs, dtype=np.uint32), np.zeros(n_segs, dtype=np.uint32)
    has, ties = np.zeros(n_segs, dtype=bool), np.zeros(n_segs, dtype=bool)
    if not len(start):
        return winner, votes, total, has, ties
    tally = np.add.reduceat(wt, start)
    rseg, rlab, rpos = seg[start], lab[start], pos[start].astype(np.uint64)
    is_cur = (rlab == current[rseg].astype(np.uint64)) if current is not None else np.zeros(len(start), dtype=bool)
    key = (tally << np.uint64(32)) | (is_cur.astype(np.uint64) << np.uint64(31)) | (np.uint64(0x7FFFFFFF) - rpos)
    first = np.nonzero(np.r_[True, rseg[1:] != rseg[:-1]])[0]
    segs = rseg[first]
    best = np.maximum.reduceat(key, first)
    best_of_run = np.repeat(best, np.diff(np.r_[first, len(start)]))
    won = key == best_of_run
    at_top = np.add.reduceat((tally == (best_of_run >> np.uint64(32))).astype(np.int64), first)
    winner[rseg[won]] = rlab[won].astype(np.uint32)
    votes[segs] = (best >> np.uint64(32)).astype(np.uint32)
    total[segs] = np.add.reduceat(tally, first).astype(np.uint32)
    has[segs] = True
    ties[segs] = (at_top > 1) & ((best & np.uint64(0x80000000)) == 0)
    return winner, votes, total, has, ties


def flat_rows(rows):
    n, k = rows.shape
    return np.repeat(np.arange(n, dtype=np.int64), k), np.tile(np.arange(k, dtype=np.int64), n), rows.reshape(-1)


def flat_csr(offsets, adj):
    n = len(offsets) - 1
    deg = np.diff(offsets.astype(np.int64))
    seg = np.repeat(np.arange(n, dtype=np.int64), deg)
    return seg, np.arange(len(adj), dtype=np.int64) - offsets[:-1].astype(np.int64)[seg], adj


def host_round(flat, labels, seeds, kind, bits):
    """one synchronous round: (new labels, votes, total, changed, ties)"""
    winner, votes, total, has, ties = host_tally(*flat, labels, labels, kind, bits, len(labels))
    new = np.where(has, winner, labels)
    if seeds is not None:
        new = np.where(seeds != NONE, seeds, new)
    return new.astype(np.uint32), votes, total, int((new != labels).sum()), int(ties.sum())


def step(args):
    import torch
    from verticut_amd import engine as vc
    n, bits, m, k = int(args.n), 64, 2, args.k
    kk = k

    def note(what):
        print("[bench_vote k=%d] %s" % (k, what), file=sys.stderr, flush=True)

    def dev(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]).copy()).cuda()

    def home(t, dtype):
        return t.cpu().numpy().view(dtype)

    e = vc.Engine(bits, capacity=n, n_tables=m, flags=vc.FLAG_LEAN_TIMING)
    e.add_synthetic(n, seed=args.seed, kind=vc.SYNTH_CLUSTERED, n_centres=max(n // args.cluster_size, 1), max_flips=args.flips)
    e.build_index()
    st = torch.cuda.current_stream().cuda_stream
    d_rows = torch.empty((n, k), dtype=torch.int64, device="cuda")
    d_counts = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_comp = torch.empty((n,), dtype=torch.int32, device="cuda")
    e.knn_graph_dev(k, d_rows.data_ptr(), d_counts.data_ptr(), mode=vc.MODE_MIH_EXACT, batch=args.batch, stream=st)
    torch.cuda.synchronize()
    note("graph built")
    assert np.all(home(d_counts, np.uint32) == min(k, n - 1)) and n > k

    def leg_cluster(kk_cut=kk):
        return e.cluster_knn_dev(d_rows.data_ptr(), d_counts.data_ptr(), k, kk_cut, d_comp.data_ptr(), None, stream=st)

    leg_cluster(min(kk, 10))
    torch.cuda.synchronize()
    comp = home(d_comp, np.uint32)
    rng = np.random.default_rng(args.seed)
    classes = (comp % np.uint32(16)).astype(np.uint32)                         # a class per component of the mutual graph of the first 10 entries
    noisy = np.where(rng.random(n) < args.noise, rng.integers(0, 16, n).astype(np.uint32), classes)   # some records carry a wrong tag: segments with several labels, ties
    vote_labels = np.where(rng.random(n) < 0.4, noisy, np.uint32(NONE)).astype(np.uint32)
    seeds = np.full(n, NONE, dtype=np.uint32)
    at = rng.choice(n, size=min(args.seeds, n), replace=False)
    seeds[at] = noisy[at]
    ids = np.arange(n, dtype=np.uint32)
    d_vote_labels, d_seeds, d_ids = dev(vote_labels), dev(seeds), dev(ids)
    d_out = [torch.empty((n,), dtype=torch.int32, device="cuda") for _ in range(3)]

    adjs = {}
    for name, flags in (("either", vc.KNN_EITHER), ("mutual", vc.KNN_MUTUAL), ("reverse", vc.KNN_REVERSE)):
        cap = (2 if flags == vc.KNN_EITHER else 1) * n * kk
        d_off, d_adj = torch.empty((n + 1,), dtype=torch.int64, device="cuda"), torch.empty((cap,), dtype=torch.int64, device="cuda")
        rc, stats = e.knn_adjacency_dev(d_rows.data_ptr(), d_counts.data_ptr(), k, kk, d_adj.data_ptr(), cap, d_off.data_ptr(), flags=flags, stream=st)
        torch.cuda.synchronize()
        assert rc == vc.VC_OK
        deg = np.diff(home(d_off, np.uint64).astype(np.int64))
        mix = np.bincount(np.searchsorted(BIN_TOPS, deg), minlength=8)
        adjs[name] = (d_off, d_adj, stats["n_entries"], {b: int(c) for b, c in zip(BIN_NAMES, mix) if c}, int(deg.max()))
    note("adjacencies built: %s" % {q: (v[2], v[3]) for q, v in adjs.items()})

    def leg_vote(kind):
        return e.knn_vote_dev(d_rows.data_ptr(), d_counts.data_ptr(), n, k, kk, d_vote_labels.data_ptr(), d_out[0].data_ptr(), d_out[1].data_ptr(), d_out[2].data_ptr(),
                              weight_kind=kind, stream=st)

    def leg_lp(name, d_labels, flags, max_iters, kind=vc.VOTE_COUNT):
        d_off, d_adj, T = adjs[name][:3]
        return e.label_propagate_dev(d_off.data_ptr(), d_adj.data_ptr(), T, d_labels.data_ptr(), d_out[0].data_ptr(), d_out[1].data_ptr(), d_out[2].data_ptr(),
                                     weight_kind=kind, flags=flags, max_iters=max_iters, stream=st)

    def outputs():
        torch.cuda.synchronize()
        return [home(t, np.uint32).copy() for t in d_out]

    # ---- the check, and the host leg with it
    host, checked = {}, {}
    t0 = time.perf_counter()
    rows, lab_home = home(d_rows, np.uint64), home(d_vote_labels, np.uint32)
    t1 = time.perf_counter()
    flat = flat_rows(rows)
    for name, kind in (("count", vc.VOTE_COUNT), ("closeness", vc.VOTE_CLOSENESS)):
        t2 = time.perf_counter()
        winner, votes, total, has, ties = host_tally(*flat, lab_home, None, kind, bits, n)
        t3 = time.perf_counter()
        stats = leg_vote(kind)
        got = outputs()
        assert np.array_equal(got[0], winner) and np.array_equal(got[1], votes) and np.array_equal(got[2], total), "vc_knn_vote_dev differs from the host (%s)" % name
        want = {"n_voted": int(has.sum()), "n_unlabelled": int((~has).sum()), "n_ties": int(ties.sum()), "n_entries": int((lab_home[(flat[2] & LOW).astype(np.int64)] != NONE).sum())}
        assert stats == want, (stats, want)
        host["vote_" + name] = {"copy_home": round(t1 - t0, 3), "tally": round(t3 - t2, 3)}
        checked["vote_" + name] = stats
        note("vote %s equals the host on every word: %s" % (name, stats))
    del rows, flat
    t0 = time.perf_counter()
    d_off, d_adj, T = adjs["either"][:3]
    offsets, adj = home(d_off, np.uint64), home(d_adj[:T], np.uint64)
    t1 = time.perf_counter()
    flat = flat_csr(offsets, adj)
    host["propagate_copy_home"] = round(t1 - t0, 3)
    forms = {}
    for form, d_labels, lp_flags, first in (("semi", d_seeds, vc.LP_CLAMP_SEEDS, seeds), ("community", d_ids, 0, ids)):
        full = leg_lp("either", d_labels, lp_flags, vc.LP_MAX_ITERS)
        final = outputs()
        labels, clamp, rounds_checked, round_s = first, (first if lp_flags else None), 0, []
        for r in range(1, min(args.check_rounds, full["n_iters"]) + 1):   # the device's round r from its own labels after r - 1 rounds
            t2 = time.perf_counter()
            new, votes, total, changed, ties = host_round(flat, labels, clamp, vc.VOTE_COUNT, bits)
            round_s.append(time.perf_counter() - t2)
            stats = leg_lp("either", d_labels, lp_flags, r)
            got = outputs()
            assert np.array_equal(got[0], new) and np.array_equal(got[1], votes) and np.array_equal(got[2], total), "round %d of %s differs from the host" % (r, form)
            assert (stats["n_iters"], stats["n_changed_last"], stats["n_ties_last"], stats["n_labelled"]) == (r, changed, ties, int((new != NONE).sum())), (form, r, stats)
            labels, rounds_checked = new, rounds_checked + 1
        if full["n_iters"] > rounds_checked:                              # and the last round, from the device's labels one round earlier
            leg_lp("either", d_labels, lp_flags, full["n_iters"] - 1)
            before = outputs()[0]
            new, votes, total, changed, ties = host_round(flat, before, clamp, vc.VOTE_COUNT, bits)
            assert np.array_equal(final[0], new) and np.array_equal(final[1], votes) and np.array_equal(final[2], total), "the last round of %s differs from the host" % form
            assert (full["n_changed_last"], full["n_ties_last"], full["converged"]) == (changed, ties, int(changed == 0)), (form, full)
        else:
            assert np.array_equal(final[0], labels)
        forms[form] = dict(full, labels_in_the_end=int(len(np.unique(final[0]))), rounds_checked_against_host=rounds_checked + (full["n_iters"] > rounds_checked))
        host["propagate_" + form] = {"round_s": round(float(np.median(round_s)), 3), "rounds": full["n_iters"],
                                     "extrapolated_total_s": round(host["propagate_copy_home"] + float(np.median(round_s)) * full["n_iters"], 3)}
        note("%s: %s" % (form, forms[form]))
    del flat, offsets, adj

    # ---- the timing
    legs = {"vote_count": lambda: leg_vote(vc.VOTE_COUNT), "vote_closeness": lambda: leg_vote(vc.VOTE_CLOSENESS),
            "round_either": lambda: leg_lp("either", d_seeds, vc.LP_CLAMP_SEEDS, 1), "round_mutual": lambda: leg_lp("mutual", d_seeds, vc.LP_CLAMP_SEEDS, 1),
            "round_reverse": lambda: leg_lp("reverse", d_seeds, vc.LP_CLAMP_SEEDS, 1),
            "round_either_closeness": lambda: leg_lp("either", d_seeds, vc.LP_CLAMP_SEEDS, 1, vc.VOTE_CLOSENESS),
            "semi": lambda: leg_lp("either", d_seeds, vc.LP_CLAMP_SEEDS, vc.LP_MAX_ITERS), "community": lambda: leg_lp("either", d_ids, 0, vc.LP_MAX_ITERS),
            "cluster_knn": leg_cluster}
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
    res = {"checked": {"vote_every_word_equals_host": True, "propagate_rounds_equal_host_every_word": {q: v["rounds_checked_against_host"] for q, v in forms.items()}},
           "vote_stats": checked, "propagate_stats": forms, "adjacency": {q: {"n_entries": v[2], "bins": v[3], "max_degree": v[4]} for q, v in adjs.items()},
           "call_ms_median": {q: round(float(np.median(v)) * 1e3, 3) for q, v in t.items()},
           "call_ms_min": {q: round(min(v) * 1e3, 3) for q, v in t.items()},
           "call_ms_max": {q: round(max(v) * 1e3, 3) for q, v in t.items()}, "reps": args.reps, "host_s": host}
    med = res["call_ms_median"]
    res["per_round_ms"] = {q: round((med[q] - med["round_either"]) / (forms[q]["n_iters"] - 1), 3) for q in ("semi", "community") if forms[q]["n_iters"] > 1}
    res["over_cluster_knn"] = {q: round(med[q] / med["cluster_knn"], 2) for q in med if q != "cluster_knn"}
    res["per_round_over_cluster_knn"] = {q: round(v / med["cluster_knn"], 2) for q, v in res["per_round_ms"].items()}
    res["host_over_device"] = {"vote_count": round((host["vote_count"]["copy_home"] + host["vote_count"]["tally"]) * 1e3 / med["vote_count"], 1),
                               "semi": round(host["propagate_semi"]["extrapolated_total_s"] * 1e3 / med["semi"], 1),
                               "community": round(host["propagate_community"]["extrapolated_total_s"] * 1e3 / med["community"], 1)}
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
    ap.add_argument("--seeds", type=int, default=5000, help="hand-tagged records of the semi-supervised form")
    ap.add_argument("--noise", type=float, default=0.1, help="share of the tags replaced by a random class")
    ap.add_argument("--check-rounds", type=int, default=3, help="rounds of each form the host model repeats over the whole store (and always the last)")
    ap.add_argument("--step-timeout", type=int, default=500, help="seconds a step may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=("run",), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--step-out", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--k", type=int, default=10, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    line = {"metric": "k-NN label vote over the rows and label propagation over the CSR adjacency of a built exact k-NN graph, %.3g clustered 64-bit codes "
                      "(%d per centre, <= %d flips), kk = k, no cap, one engine; 40 %% of the records labelled for the vote, %d clamped seeds for the semi-supervised "
                      "form, 16 classes, %.0f %% of the tags wrong" % (args.n, args.cluster_size, args.flips, args.seeds, 100 * args.noise),
            "host_sample": "the host tally ran over the WHOLE store for both vote kinds and for every checked round; the host's propagation total is its median "
                           "round times the device's n_iters plus the copy home (extrapolated from the checked rounds)",
            "not_measured": "other code widths, the team boundaries (kk of 64 / 65, 256 / 257, 1024 / 1025), the 128 KiB table and the long path at scale, the "
                            "sharded forms, the host-pointer forms, rounds grouped per read-back (not built), a kernel trace"}
    with tempfile.TemporaryDirectory() as td:
        for k in [int(x) for x in args.ks.split(",")]:
            part = os.path.join(td, "run_%d.json" % k)      # chained: a step that fails, faults or runs into its time limit ends the run
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", "run", "--step-out", part, "--k", str(k)]
            for key in ("n", "batch", "cluster_size", "flips", "reps", "seed", "seeds", "noise", "check_rounds"):
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
