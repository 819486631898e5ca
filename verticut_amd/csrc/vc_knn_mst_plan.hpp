// Plan arithmetic of vc_knn_mst* and vc_mst_cut* (vc_knn_mst.hip): the argument checks, the 2^31 - 1 limit on the items, the 64-bit
// edge key and its unpacking, the bound on the live list, the scratch bytes, the bit counts of the final sort, the bound on the rounds
// and the staging layouts of the host forms.  Plain C++ with no HIP in it, so that tests/cpp/knn_mst_plan_test.cc checks it on the CPU;
// the kernels and the driver call exactly these functions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VC_MST_FN __host__ __device__ inline
#else
#define VC_MST_FN inline
#endif

#define VC_MST_MUTUAL 0u                  // = VC_KNN_MUTUAL
#define VC_MST_EITHER 1u                  // = VC_KNN_EITHER
#define VC_MST_KIND_DISTANCE 0u           // = VC_MST_DISTANCE
#define VC_MST_KIND_REACHABILITY 1u       // = VC_MST_REACHABILITY
#define VC_MST_MAX_ITEMS 0x7FFFFFFFull    // N kk of a call: the home index takes the key's low word, the sort's positions are 32-bit
#define VC_MST_STAT_BYTES 48u             // the device's block, see VcMstStat in vc_knn_mst.hip
#define VC_MST_HOST_STAT_BYTES 48u        // sizeof(vc_knn_mst_stats)
#define VC_MST_EDGE_BYTES 16u             // sizeof(vc_mst_edge)
#define VC_MST_BLOCK 256u                 // threads of a block of every launch
#define VC_MST_MAX_BITS 512u              // the widest code: the histogram of the write launch has this many + 1 LDS counters
#define VC_MST_NONE 0xFFFFFFFFFFFFFFFFull // best[] of a component that no live edge leaves

// ---- the arguments (k already checked by vc_kgraph_k_ok) ----------------------------------------------------------------------------------
VC_MST_FN bool vc_mst_kk_ok(uint32_t k, uint32_t kk) { return kk >= 1 && kk <= k; }
VC_MST_FN bool vc_mst_flags_ok(uint32_t flags) { return flags == VC_MST_MUTUAL || flags == VC_MST_EITHER; }   // VC_KNN_REVERSE is no undirected graph
VC_MST_FN bool vc_mst_kind_ok(uint32_t kind) { return kind <= VC_MST_KIND_REACHABILITY; }
// min_pts counts the record itself: 1 .. k + 1 under REACHABILITY, 1 under DISTANCE
VC_MST_FN bool vc_mst_min_pts_ok(uint32_t kind, uint32_t k, uint32_t min_pts) {
  return kind == VC_MST_KIND_REACHABILITY ? (min_pts >= 1 && min_pts <= k + 1) : min_pts == 1;
}
VC_MST_FN bool vc_mst_items_ok(uint64_t n, uint32_t kk) { return n == 0 || n <= VC_MST_MAX_ITEMS / kk; }   // n kk <= 2^31 - 1, no overflow

// ---- the weight.  The core distance of a row: 0 at min_pts 1; else the distance of entry min_pts - 2, or `bits` when the row is
// shorter.  `entry` is that word of the row (read only when the row holds it)
VC_MST_FN bool vc_mst_core_held(uint32_t count, uint32_t min_pts) { return count + 1 >= min_pts; }   // min_pts >= 2
VC_MST_FN uint32_t vc_mst_weight(uint32_t d, uint32_t core_a, uint32_t core_b) {
  const uint32_t c = core_a > core_b ? core_a : core_b;
  return d > c ? d : c;
}

// ---- the key of an edge: weight << 32 | home index, home index = pos(a) * kk + jj with jj the position of b in row a.  Rows ascend in
// (dist, id), so under one weight and one home end the index orders by (dist, b): the key's order is the contract's (weight, a, dist, b)
VC_MST_FN uint64_t vc_mst_key(uint32_t weight, uint64_t pos_a, uint32_t kk, uint32_t jj) { return ((uint64_t)weight << 32) | (pos_a * kk + jj); }
VC_MST_FN uint32_t vc_mst_key_weight(uint64_t key) { return (uint32_t)(key >> 32); }
VC_MST_FN uint32_t vc_mst_key_home(uint64_t key) { return (uint32_t)key; }
VC_MST_FN uint32_t vc_mst_home_pos(uint32_t home, uint32_t kk) { return home / kk; }
VC_MST_FN uint32_t vc_mst_home_entry(uint32_t home, uint32_t kk) { return home % kk; }
// THE HOME RULE, from the entry (i lists j): the smaller id if it lists the other, otherwise the larger.  `back` = j lists i.
// MUTUAL: the pair is an edge iff back, and its home entry is the smaller end's.  EITHER: every listed entry is an edge; its home
// entry is the smaller end's if that end lists, so the larger end's entry is home only when the smaller does not list back.
VC_MST_FN bool vc_mst_is_home(uint32_t flags, bool i_below_j, bool back) { return flags == VC_MST_MUTUAL ? (back && i_below_j) : (i_below_j || !back); }

// ---- the rounds: every round that hooks halves the components that still have an edge out, so at most ceil(log2 n) rounds hook; the
// driver runs one more that finds nothing
VC_MST_FN uint32_t vc_mst_bitlength(uint64_t x) {
  uint32_t b = 0;
  while (x) { ++b; x >>= 1; }
  return b;
}
VC_MST_FN uint32_t vc_mst_ceil_log2(uint64_t n) { return n <= 1 ? 0u : vc_mst_bitlength(n - 1); }
VC_MST_FN uint32_t vc_mst_round_bound(uint64_t n) { return vc_mst_ceil_log2(n) + 1; }

// ---- the final sort of the picked edges: key = weight (0 .. bits), the value's high word = home index (below n kk)
VC_MST_FN uint32_t vc_mst_weight_bits(uint32_t bits) { return vc_mst_bitlength(bits); }
VC_MST_FN uint32_t vc_mst_home_bits(uint64_t n, uint32_t kk) { return vc_mst_bitlength(n * kk); }

// ---- the scratch of a call, in bytes.  The live list: two buffers (a round reads one and writes the survivors to the other) of
// (key u64, pos b u32) -- a home entry each, so at most n kk of them, half that under MUTUAL (a pair has two listed entries, one home).
// The forest: the parents, the round's snapshot of the component ids (u32 each) and best (u64).  The picked list: two (weight u32,
// home << 32 u64) pairs of n - 1 items for the sort
VC_MST_FN uint64_t vc_mst_live_bound(uint64_t n, uint32_t kk, uint32_t flags) { return flags == VC_MST_MUTUAL ? n * kk / 2 : n * kk; }
VC_MST_FN uint64_t vc_mst_words4(uint64_t words) { return (words * 4 + 7) & ~7ull; }   // bytes of a 32-bit array, the next one 8-byte aligned
VC_MST_FN uint64_t vc_mst_live_cap(uint64_t n, uint32_t kk, uint32_t flags) {          // what a buffer holds: no empty buffer
  const uint64_t L = vc_mst_live_bound(n, kk, flags);
  return L ? L : 1;
}
VC_MST_FN uint64_t vc_mst_live_bytes(uint64_t n, uint32_t kk, uint32_t flags) {
  const uint64_t L = vc_mst_live_cap(n, kk, flags);
  return 2 * (L * 8 + vc_mst_words4(L));
}
VC_MST_FN uint64_t vc_mst_forest_bytes(uint64_t n) { return n * 8 + 2 * vc_mst_words4(n); }
VC_MST_FN uint64_t vc_mst_pick_items(uint64_t n) { return n ? n - 1 : 0; }           // a forest of n records has at most n - 1 edges
VC_MST_FN uint64_t vc_mst_pick_cap(uint64_t n) { return n > 1 ? n - 1 : 1; }
VC_MST_FN uint64_t vc_mst_pick_bytes(uint64_t n) {
  const uint64_t m = vc_mst_pick_cap(n);
  return 2 * (m * 8 + vc_mst_words4(m));
}

// ---- the host forms' staging, every part 8-byte aligned.  vc_knn_mst: rows [n][k] | edges [n - 1] | hist [bits + 1] | labels [n] |
// counts [n].  vc_mst_cut: edges [n_edges] | labels [n]
struct VcMstStage {
  uint64_t rows, edges, hist, labels, counts, total;
  VcMstStage(uint64_t n, uint32_t k, uint32_t bits, bool with_counts) {
    uint64_t o = 0;
    rows = o;    o += n * k * 8;
    edges = o;   o += vc_mst_pick_items(n) * VC_MST_EDGE_BYTES;
    hist = o;    o += ((uint64_t)bits + 1) * 8;
    labels = o;  o += (n * 4 + 7) & ~7ull;
    counts = o;  o += with_counts ? (n * 4 + 7) & ~7ull : 0;
    total = o;
  }
};
struct VcMstCutStage {
  uint64_t edges, labels, total;
  VcMstCutStage(uint64_t n, uint64_t n_edges) {
    edges = 0;
    labels = n_edges * VC_MST_EDGE_BYTES;
    total = labels + ((n * 4 + 7) & ~7ull);
  }
};
