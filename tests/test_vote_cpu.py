"""vc_knn_vote* and vc_label_propagate* without a GPU: the ABI surface, the code objects of the kernels, the plan arithmetic under the
sanitizers, and the expectation of test_vote_gpu.py -- that the dict-loop model of vote_common.py agrees with an independent
formulation (sort the voting entries by label, np.add.reduceat, an argmax over explicit (tally, is-current, -first position) tuples),
and that the labelled inputs make each of the three rules matter."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import knn_adjacency_common as KA
import vote_common as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_new_names(vc):
    txt = open(os.path.join(ROOT, "include", "verticut_gpu.h")).read()
    assert re.search(r"#define\s+VC_ABI_VERSION\s+2\b", txt)             # entry points are only added
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"typedef struct vc_knn_vote_stats\s*\{\s*uint64_t n_voted;\s*uint64_t n_unlabelled;\s*uint64_t n_ties;\s*uint64_t n_entries;\s*\}"
                     r"\s*vc_knn_vote_stats;", code)
    assert re.search(r"typedef struct vc_label_propagate_stats\s*\{\s*uint32_t n_iters;\s*uint32_t converged;\s*uint64_t n_changed_last;\s*uint64_t n_labelled;"
                     r"\s*uint64_t n_ties_last;\s*\}\s*vc_label_propagate_stats;", code)
    for name, value in (("VC_VOTE_NONE", "0xFFFFFFFFu"), ("VC_VOTE_COUNT", "0u"), ("VC_VOTE_CLOSENESS", "1u"), ("VC_LP_CLAMP_SEEDS", "1u"), ("VC_LP_MAX_ITERS", "64u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), code), name
    assert code.index("vc_knn_mst_stats;") < code.index("VC_VOTE_NONE") < code.index("vc_device_status")   # after the vc_knn_mst* block
    L = ctypes.CDLL(vc.LIB_PATH)
    for name in V.VOTE_NAMES:
        assert hasattr(L, name), name
        assert name in vc.EXPORTS
    for name in ("vc_knn_vote_dev", "vc_sharded_knn_vote_dev"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*const uint64_t\* d_rows,\s*const uint32_t\* d_counts,\s*uint64_t n_rows,\s*uint32_t k,\s*uint32_t kk,"
                         r"\s*uint32_t max_dist,\s*const uint32_t\* d_labels,\s*uint32_t weight_kind,\s*uint32_t\* d_out_label,\s*uint32_t\* d_out_votes,"
                         r"\s*uint32_t\* d_out_total,\s*vc_knn_vote_stats\* stats,\s*void\* stream\)" % name, code), name
    for name in ("vc_knn_vote", "vc_sharded_knn_vote"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*const uint64_t\* rows,\s*const uint32_t\* counts,\s*uint64_t n_rows,\s*uint32_t k,\s*uint32_t kk,"
                         r"\s*uint32_t max_dist,\s*const uint32_t\* labels,\s*uint32_t weight_kind,\s*uint32_t\* out_label,\s*uint32_t\* out_votes,"
                         r"\s*uint32_t\* out_total,\s*vc_knn_vote_stats\* stats\)" % name, code), name
    for name in ("vc_label_propagate_dev", "vc_sharded_label_propagate_dev"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*const uint64_t\* d_offsets,\s*const uint64_t\* d_adj,\s*uint64_t n_entries,\s*const uint32_t\* d_labels_in,"
                         r"\s*uint32_t weight_kind,\s*uint32_t flags,\s*uint32_t max_iters,\s*uint32_t\* d_labels_out,\s*uint32_t\* d_votes,\s*uint32_t\* d_total,"
                         r"\s*vc_label_propagate_stats\* stats,\s*void\* stream\)" % name, code), name
    for name in ("vc_label_propagate", "vc_sharded_label_propagate"):
        assert re.search(r"\bint\s+%s\s*\(\s*vc_\w+\*\s*\w+,\s*const uint64_t\* offsets,\s*const uint64_t\* adj,\s*uint64_t n_entries,\s*const uint32_t\* labels_in,"
                         r"\s*uint32_t weight_kind,\s*uint32_t flags,\s*uint32_t max_iters,\s*uint32_t\* labels_out,\s*uint32_t\* votes,\s*uint32_t\* total,"
                         r"\s*vc_label_propagate_stats\* stats\)" % name, code), name
    flat = " ".join(txt.split()).replace(" * ", " ")
    for phrase in ("THE VOTE RULE, shared by both calls", "Such an entry does not vote".lower(), "bits + 1 - d under VC_VOTE_CLOSENESS", "(1) the larger tally",
                   "(2) then the segment's CURRENT label", "(3) then the label whose first occurrence in the segment comes earliest",
                   "winner VC_VOTE_NONE, votes = 0 and total = 0", "The order is strict, so every output word is a function of the segment and the labels",
                   "holds ANY rows whose ids are resident", "then holds min(k, N) entries", "An entry equal to a record's own id is an ordinary entry",
                   "Rounds are double-buffered", "they are also written for clamped seeds", "ERRORS, checked before any work, outputs untouched",
                   "THE OUTPUTS ARE THEN UNDEFINED", "NO OUTPUT WORD WRITTEN", "does not fit 32 bits", "n_rows == 0 and N == 0 give VC_OK and zero stats",
                   "one for the plan, then one small read-back per round", "no shard is touched", "NOT OFFERED: caller-given edge weights",
                   "asynchronous propagation", "an incremental form after vc_add_codes or vc_retain*", "more than 64 rounds per call"):
        assert " ".join(phrase.split()) in flat, phrase
    assert vc.VC_ABI_VERSION == 2
    assert (vc.VOTE_NONE, vc.VOTE_COUNT, vc.VOTE_CLOSENESS, vc.LP_CLAMP_SEEDS, vc.LP_MAX_ITERS) == (V.NONE, V.COUNT, V.CLOSENESS, V.CLAMP, V.MAX_ITERS)
    st = vc.VcKnnVoteStats
    assert ctypes.sizeof(st) == 32 and [getattr(st, n).offset for n in V.VOTE_STATS] == [0, 8, 16, 24] and st().as_dict() == V.zero_vote_stats()
    st = vc.VcLabelPropagateStats
    assert ctypes.sizeof(st) == 32 and [getattr(st, n).offset for n in V.LP_STATS] == [0, 4, 8, 16, 24] and st().as_dict() == V.zero_lp_stats()
    for cls in (vc.Engine, vc.ShardedEngine):
        for meth in ("knn_vote", "knn_vote_dev", "label_propagate", "label_propagate_dev"):
            assert callable(getattr(cls, meth)), (cls, meth)
    host = open(os.path.join(ROOT, "verticut_amd", "host", "verticut_host.hpp")).read()
    assert re.search(r"virtual int knn_vote\([^)]*\)\s*=\s*0;", host) and re.search(r"virtual int label_propagate\([^)]*\)\s*=\s*0;", host)
    assert len(re.findall(r"int knn_vote\([^)]*\)\s*override", host)) == 2 and len(re.findall(r"int label_propagate\([^)]*\)\s*override", host)) == 2
    for call in ("return vc_knn_vote(h_,", "return vc_sharded_knn_vote(h_,", "return vc_label_propagate(h_,", "return vc_sharded_label_propagate(h_,"):
        assert call in host, call
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "5.22" in design and "vc_knn_vote" in design and "vc_label_propagate" in design
    for doc in ("README.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "vc_knn_vote" in text and "vc_label_propagate" in text, doc
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_vote.py"))


def test_the_plan_mirror_is_the_header(vc):
    text = open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_vote_plan.hpp")).read()

    def const(name):
        m = re.search(r"#define\s+%s\s+(0x[0-9A-Fa-f]+|\d+)u?\b" % name, text)
        assert m, name
        return int(m.group(1), 0)
    assert (const("VC_VOTE_TEAM_MIN"), const("VC_VOTE_TEAM_MAX"), const("VC_VOTE_WAVE_MAX"), const("VC_VOTE_SMALL_MAX"), const("VC_VOTE_BIG_MAX")) == \
        (V.TEAM_MIN, V.TEAM_MAX, V.WAVE_MAX, V.SMALL_MAX, V.BIG_MAX)
    assert (const("VC_VOTE_MIN_SLOTS"), const("VC_VOTE_SLOT_BYTES"), const("VC_VOTE_LONG_AUX_BYTES"), const("VC_VOTE_STAT_BYTES"), const("VC_VOTE_PLAN_STAT_BYTES"),
            const("VC_VOTE_BLOCK")) == (V.MIN_SLOTS, V.SLOT_BYTES, V.LONG_AUX_BYTES, V.STAT_BYTES, V.PLAN_STAT_BYTES, V.BLOCK)
    assert (const("VC_VOTE_LABEL_NONE"), const("VC_VOTE_KIND_COUNT"), const("VC_VOTE_KIND_CLOSENESS"), const("VC_VOTE_CLAMP"), const("VC_VOTE_MAX_ITERS")) == \
        (V.NONE, V.COUNT, V.CLOSENESS, V.CLAMP, V.MAX_ITERS)
    names = re.search(r"enum VcVoteBin \{([^}]*)\}", text).group(1).replace("\n", " ").split(",")
    assert [n.strip().replace("VC_VOTE_BIN_", "") for n in names[:-1]] == list(V.BIN_NAMES) and names[-1].strip() == "VC_VOTE_BINS" and V.BINS == len(V.BIN_NAMES)
    assert V.BIG_MAX == V.MAX_K                                           # the row view never leaves the LDS table
    assert [V.bin_of(x) for x in (0, 8, 9, 16, 17, 32, 33, 64, 65, 256, 257, 1024, 1025, 8192, 8193, 10 ** 9)] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7]
    assert (V.lds_bytes(256), V.lds_bytes(1024), V.lds_bytes(8192)) == (4 << 10, 16 << 10, 128 << 10)


def test_vote_kernels_use_no_scratch_memory_and_the_lds_they_say(vc):
    from verticut_amd import build as vb
    assert "vc_vote.hip" in vb.SOURCES and "vc_vote_plan.hpp" in vb.HEADERS
    res = vb.kernel_resources(os.path.join(vb.LIBDIR, "vc_vote.o"))
    kernels = ("vc_vote_team_kernelILj8E", "vc_vote_team_kernelILj16E", "vc_vote_team_kernelILj32E", "vc_vote_team_kernelILj64E", "vc_vote_table_kernelILj64E",
               "vc_vote_table_kernelILj256E", "vc_vote_long_insert_kernel", "vc_vote_long_key_kernel", "vc_vote_long_top_kernel", "vc_vote_long_finish_kernel",
               "vc_vote_plan_count_kernel", "vc_vote_plan_entries_kernel", "vc_vote_plan_fill_kernel", "vc_vote_plan_finish_kernel")
    for kernel in kernels:
        assert sum(kernel in name for name in res) == 1, (kernel, sorted(res))
    assert len(res) == len(kernels), sorted(res)
    for name, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        if "team" in name or "long" in name or "entries" in name or "plan_finish" in name:
            assert r["group_segment_fixed_size"] == 0, (name, r)         # no LDS: the team shape is shuffles only
        else:
            assert r["group_segment_fixed_size"] <= 256, (name, r)       # reduction words only: the table is dynamic LDS
    text = open(os.path.join(ROOT, "verticut_amd", "csrc", "vc_vote.hip")).read()
    for word in ("hipLaunchCooperativeKernel", "grid_group", "getenv", "asm"):
        assert word not in text, word


def test_plan_arithmetic_under_the_sanitizers(tmp_path):
    """tests/cpp/vote_plan_test.cc over csrc/vc_vote_plan.hpp, host code only, with AddressSanitizer and UBSan; the figures it prints
    are those of the model's mirror"""
    src = os.path.join(ROOT, "tests", "cpp", "vote_plan_test.cc")
    exe = tmp_path / "vote_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           src, "-I", os.path.join(ROOT, "verticut_amd", "csrc")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert out.stdout.endswith("vote plan ok: TEAM %d WAVE %d SMALL %d BIG %d MIN_SLOTS %d BINS %d STAT %d\n" %
                               (V.TEAM_MAX, V.WAVE_MAX, V.SMALL_MAX, V.BIG_MAX, V.MIN_SLOTS, V.BINS, V.STAT_BYTES))
    for length in (1, 65, 1024, 8192, 8193):
        assert re.search(r"^TABLE %d %d %d$" % (length, V.slots(length), V.slots(length).bit_length() - 1), out.stdout, flags=re.M), length
    for n in (1, 2, 700, 8200, 1000000):
        line = "SCRATCH %d %d %d" % (n, V.lp_bytes(n), V.long_bytes(2, V.slots(8193) + V.slots(n)))
        assert re.search("^%s$" % line, out.stdout, flags=re.M), line
    for with_counts in (False, True):
        assert re.search(r"^STAGE %d %d$" % (with_counts, V.vote_stage_total(33, 10, 701, with_counts)), out.stdout, flags=re.M)
    assert re.search(r"^LPSTAGE %d$" % V.lp_stage_total(701, 12345), out.stdout, flags=re.M)
    assert V.length_ok(0xFFFFFFFF // 65, 64) and not V.length_ok(0xFFFFFFFF // 65 + 1, 64) and V.lp_stat_bytes() == 128 + 64 * 64 and V.long_cap(8193) == 2
    assert V.key(3, True, 0) > V.key(3, False, 0) > V.key(3, False, 1) > V.key(2, True, 0)


# ---- the model is the contract: an independent formulation ---------------------------------------------------------------------------------------
def _reduceat_segment(words, labels, kind, bits, current=V.NONE, id_base=0):
    """(winner, votes, total, rule): the voting entries sorted by label (stably, so a run's first element is the first occurrence),
    np.add.reduceat over the runs, an argmax over explicit (tally, is-current, -first position) tuples"""
    words = np.asarray(words, dtype=np.uint64)
    ids = (words & np.uint64(0xFFFFFFFF)).astype(np.int64) - id_base
    labs = labels[ids].astype(np.int64) if len(ids) else np.zeros(0, dtype=np.int64)
    keep = labs != V.NONE
    if not keep.any():
        return V.NONE, 0, 0, 0
    pos = np.nonzero(keep)[0]
    labs = labs[keep]
    dist = (words[keep] >> np.uint64(32)).astype(np.int64)
    wts = (bits + 1 - dist) if kind == V.CLOSENESS else np.ones(len(dist), dtype=np.int64)
    order = np.argsort(labs, kind="stable")
    starts = np.nonzero(np.r_[True, np.diff(labs[order]) != 0])[0]
    tallies = np.add.reduceat(wts[order], starts)
    tuples = [(int(t), int(labs[order][s] == current), -int(pos[order][s])) for t, s in zip(tallies, starts)]
    best = max(range(len(tuples)), key=lambda i: tuples[i])
    top = [t for t in tuples if t[0] == tuples[best][0]]
    rule = 1 if len(top) == 1 else (2 if tuples[best][1] else 3)
    return int(labs[order][starts[best]]), tuples[best][0], int(wts.sum()), rule


@pytest.mark.parametrize("bits", [64, 128])
def test_the_model_agrees_with_the_reduceat_formulation(bits):
    _, rows, counts = V.graph(bits)
    labels = V.seeded_labels(bits)
    rng = np.random.default_rng(bits)
    for kind in (V.COUNT, V.CLOSENESS):
        for kk, cap in ((1, V.NO_CAP), (3, V.NO_CAP), (10, V.NO_CAP), (10, bits // 8), (10, 0)):
            for r in range(len(rows)):
                seg = V.row_segment(rows[r], counts[r], kk, cap)
                cur = int(rng.integers(0, V.N_CLASSES)) if r % 3 else V.NONE
                got = V.vote_segment(seg, labels, kind, bits, cur)
                assert got[:4] == _reduceat_segment(seg, labels, kind, bits, cur), (kind, kk, cap, r)
    offsets, adj = V.adjacency(bits, KA.EITHER)
    (want, votes, total, st), _ = V.propagate_expected(bits, KA.EITHER, "community", 2)
    lab = V.community_labels(700)
    for _ in range(2):
        new = lab.copy()
        for i in range(700):
            win, _, _, rule = _reduceat_segment(adj[int(offsets[i]):int(offsets[i + 1])], lab, V.COUNT, bits, int(lab[i]))
            if rule:
                new[i] = win
        lab = new
    assert np.array_equal(lab, want)


def test_hand_made_segments_spell_the_three_rules():
    labels = np.array([7, 7, 9, 9, V.NONE, 3], dtype=np.uint32)
    seg = [(1 << 32) | 2, (2 << 32) | 0, (2 << 32) | 3, (3 << 32) | 1, (3 << 32) | 4, (5 << 32) | 5]   # labels 9 7 9 7 - 3
    assert V.vote_segment(seg, labels, V.COUNT, 64) == (9, 2, 5, 3, 5)                       # 9 and 7 tie at 2: 9 comes first
    assert V.vote_segment(seg, labels, V.COUNT, 64, current=7) == (7, 2, 5, 2, 5)            # the current label breaks the tie
    assert V.vote_segment(seg, labels, V.COUNT, 64, current=3) == (9, 2, 5, 3, 5)            # a current label below the top does not
    assert V.vote_segment(seg, labels, V.CLOSENESS, 64) == (9, 64 + 63, 64 + 63 + 63 + 62 + 60, 1, 5)
    assert V.vote_segment(seg[4:5], labels, V.COUNT, 64) == (V.NONE, 0, 0, 0, 0) and V.vote_segment([], labels, V.COUNT, 64) == (V.NONE, 0, 0, 0, 0)
    assert V.vote_segment(seg[5:], labels, V.CLOSENESS, 64, current=1) == (3, 60, 60, 1, 1)


# ---- the inputs make each rule matter (conditions, not counts) -------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [64, 128])
def test_the_vote_inputs_reach_ties_empty_rows_and_weight_dependent_winners(bits):
    assert V.vote_expected(bits, 3, V.COUNT)[3]["n_ties"] > 0                                # rule 3 decides rows at kk = 3
    assert V.vote_expected(bits, 1, V.COUNT)[3]["n_unlabelled"] > 0 and V.vote_expected(bits, 10, V.COUNT)[3]["n_unlabelled"] > 0
    assert V.vote_expected(bits, 10, V.COUNT)[3]["n_voted"] > 0
    assert np.any(V.vote_expected(bits, 10, V.COUNT)[0] != V.vote_expected(bits, 10, V.CLOSENESS)[0])
    capped = V.vote_expected(bits, 10, V.COUNT, bits // 8)[3]
    assert 0 < capped["n_entries"] < V.vote_expected(bits, 10, V.COUNT)[3]["n_entries"]     # the cap cuts rows
    labels = V.seeded_labels(bits)
    assert 0.5 < float((labels == V.NONE).mean()) < 0.7 and len(np.unique(labels)) == V.N_CLASSES + 1


def test_the_propagation_inputs_reach_rule_2_convergence_and_the_cap():
    for bits in (64, 128):
        (labels, _, _, st), trace = V.propagate_expected(bits, KA.EITHER, "community", V.MAX_ITERS)
        assert st["converged"] == 1 and st["n_iters"] < V.MAX_ITERS and 1 < len(np.unique(labels)) < 700
        assert any(t[2] > 0 for t in trace)                                                  # rule 2 decides records in some round
        (_, _, _, st), trace = V.propagate_expected(bits, KA.EITHER, "seeded", V.MAX_ITERS)
        assert st["converged"] == 0 and st["n_iters"] == V.MAX_ITERS and st["n_changed_last"] > 0   # still changing at max_iters
        assert any(t[2] > 0 for t in trace)
    (_, _, _, st), _ = V.propagate_expected(128, KA.EITHER, "sparse", V.MAX_ITERS)
    assert st["converged"] == 1 and 1 < st["n_iters"] < V.MAX_ITERS                          # a seeded semi-supervised case converges
    seeds = V.sparse_seeds(128)
    (labels, _, _, _), _ = V.propagate_expected(128, KA.EITHER, "sparse", V.MAX_ITERS)
    assert np.array_equal(labels[seeds != V.NONE], seeds[seeds != V.NONE])                   # the clamp
    for flags in (KA.EITHER, KA.MUTUAL, KA.REVERSE):                                          # every adjacency stays in the team shape here
        offsets, _ = V.adjacency(64, flags)
        assert int(np.diff(offsets.astype(np.int64)).max()) <= V.TEAM_MAX
