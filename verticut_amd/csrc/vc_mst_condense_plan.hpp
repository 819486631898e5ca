// Plan arithmetic of vc_mst_condense* (vc_mst_condense.hip): the argument checks, the bound on the nodes, the level table compacted
// from the plan pass's first-edge table, the tags of the per-level claims, the bit counts of the node sort, the stability, the scratch
// bytes and the staging layout of the host form.  Plain C++ with no HIP in it, so that tests/cpp/condense_plan_test.cc checks it on the
// CPU; the kernels and the driver call exactly these functions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VC_COND_FN __host__ __device__ inline
#else
#define VC_COND_FN inline
#endif

#define VC_COND_EOM 0u                    // = VC_CONDENSE_EOM
#define VC_COND_LEAF 1u                   // = VC_CONDENSE_LEAF
#define VC_COND_NONE 0xFFFFFFFFu          // = VC_CONDENSE_NONE
#define VC_COND_SELECTED 1u               // = VC_CONDENSE_SELECTED
#define VC_COND_KEEP 2u                   // = VC_CONDENSE_KEEP
#define VC_COND_ROOT 4u                   // = VC_CONDENSE_ROOT
#define VC_COND_MAX_MCS 0x80000000u       // min_cluster_size lies in 2 .. 2^31
#define VC_COND_MAX_BITS 512u             // the widest code: a forest has at most this many + 1 levels
#define VC_COND_NODE_BYTES 48u            // sizeof(vc_condensed_node)
#define VC_COND_HOST_STAT_BYTES 64u       // sizeof(vc_mst_condense_stats)
#define VC_COND_STAT_BYTES 56u            // the device's block, see VcCondStat in vc_mst_condense.hip
#define VC_COND_WORK_NODE_BYTES 40u       // a node while the levels run, see CdNode in vc_mst_condense.hip
#define VC_COND_EDGE_BYTES 16u            // sizeof(vc_mst_edge)
#define VC_COND_BLOCK 256u                // threads of a block of every launch
#define VC_COND_RECORD_WORDS 12u          // 32-bit words of scratch per record, see vc_cond_work_bytes
#define VC_COND_NODE_WORDS 4u             // 32-bit words of scratch per node beside the working node and one 64-bit word, see vc_cond_tree_bytes

// ---- the arguments --------------------------------------------------------------------------------------------------------------------------
VC_COND_FN bool vc_cond_mcs_ok(uint32_t mcs) { return mcs >= 2 && mcs <= VC_COND_MAX_MCS; }
VC_COND_FN bool vc_cond_root_weight_ok(uint32_t root_weight, uint32_t bits) { return root_weight <= bits + 1; }
VC_COND_FN bool vc_cond_method_ok(uint32_t method) { return method <= VC_COND_LEAF; }
VC_COND_FN uint64_t vc_cond_edge_cap(uint64_t n) { return n ? n - 1 : 0; }   // a forest of n records has at most n - 1 edges: max(n, 1) - 1
VC_COND_FN bool vc_cond_edges_ok(uint64_t n, uint64_t n_edges) { return n_edges <= vc_cond_edge_cap(n); }
// what the device checks of the root weight once the largest weight is known: 0, or above every edge
VC_COND_FN bool vc_cond_root_above(uint32_t root_weight, uint32_t last_weight) { return root_weight == 0 || root_weight > last_weight; }

// ---- the nodes.  Every node but a leaf has two or more children, and the leaves are disjoint sets of at least mcs records: at most
// floor(n / mcs) leaves and one node fewer inside.  The caller's d_nodes holds max(n, 1) - 1 records, which is never less.
VC_COND_FN uint64_t vc_cond_node_bound(uint64_t n, uint32_t mcs) {
  const uint64_t leaves = n / mcs;
  return leaves ? 2 * leaves - 1 : 0;
}
VC_COND_FN uint64_t vc_cond_node_cap(uint64_t n) { return vc_cond_edge_cap(n); }

// ---- the levels.  The plan pass leaves first[w] = the index of the first edge of weight w, VC_COND_NONE where there is none; the list
// ascends, so level w is the edges first[w] .. the next first (or n_edges).  Compacted into rows on the host; returns the rows written
struct VcCondLevel {
  uint32_t weight, first, count;
};
inline uint32_t vc_cond_levels(const uint32_t* first, uint32_t bits, uint64_t n_edges, VcCondLevel* out) {
  uint32_t rows = 0;
  for (uint32_t w = 0; w <= bits; ++w) {
    if (first[w] == VC_COND_NONE) continue;
    if (rows) out[rows - 1].count = first[w] - out[rows - 1].first;
    out[rows++] = VcCondLevel{w, first[w], 0};
  }
  if (rows) out[rows - 1].count = (uint32_t)n_edges - out[rows - 1].first;
  return rows;
}
// the tags of level l = 0, 1, .. in the two claim arrays: a record's old root is claimed twice a level (the tally, then the apply
// launch), a new root once; all are above every earlier level's and above the zero the arrays start with
VC_COND_FN uint32_t vc_cond_tag_tally(uint32_t level) { return 2 * level + 1; }
VC_COND_FN uint32_t vc_cond_tag_apply(uint32_t level) { return 2 * level + 2; }
VC_COND_FN uint32_t vc_cond_tag_new(uint32_t level) { return level + 1; }

// ---- the stability of a node: end * size - the sum of the leave levels, which is form * size at formation + w * absorbed at every w.
// A root under root_weight 0 has none.  size < 2^32 and end <= 513: no overflow
VC_COND_FN uint64_t vc_cond_stability(uint32_t end, uint32_t size, uint64_t sum_leave, bool root, uint32_t root_weight) {
  return root && root_weight == 0 ? 0 : (uint64_t)end * size - sum_leave;
}
// may the node be chosen at all?  Not a root under root_weight 0
VC_COND_FN bool vc_cond_allowed(bool root, uint32_t root_weight) { return !(root && root_weight == 0); }
VC_COND_FN bool vc_cond_keep(uint64_t stability, uint64_t sub, bool allowed) { return allowed && stability >= sub; }   // a tie goes to the parent

// ---- the sort of the nodes by (form, rep): key = form (0 .. bits), the value's high word = rep (a global id)
VC_COND_FN uint32_t vc_cond_bitlength(uint64_t x) {
  uint32_t b = 0;
  while (x) { ++b; x >>= 1; }
  return b;
}
VC_COND_FN uint32_t vc_cond_form_bits(uint32_t bits) { return vc_cond_bitlength(bits); }
VC_COND_FN uint32_t vc_cond_rep_bits(uint32_t id_base, uint64_t n) { return n ? vc_cond_bitlength((uint64_t)id_base + n - 1) : 1; }

// ---- the scratch of a call, in bytes.  Per record twelve words: the forest, the snapshot, the component's size and node, the level's
// three sums and its decision, the two claim arrays, own and leave.  The plan: first[bits + 1].  Per node of the cap: the working node,
// then for the finish the rank, the selected ancestor, the candidate word, the children still missing, and the 64-bit sum of their
// best.  The sort: two (form u32, rep << 32 | index u64) pairs
VC_COND_FN uint64_t vc_cond_words4(uint64_t words) { return (words * 4 + 7) & ~7ull; }
VC_COND_FN uint64_t vc_cond_work_bytes(uint64_t n) { return VC_COND_RECORD_WORDS * vc_cond_words4(n); }
VC_COND_FN uint64_t vc_cond_plan_bytes(uint32_t bits) { return vc_cond_words4((uint64_t)bits + 1); }
VC_COND_FN uint64_t vc_cond_scratch_nodes(uint64_t n) { return n > 1 ? n - 1 : 1; }   // no empty buffer
VC_COND_FN uint64_t vc_cond_tree_bytes(uint64_t n) {
  const uint64_t m = vc_cond_scratch_nodes(n);
  return m * VC_COND_WORK_NODE_BYTES + VC_COND_NODE_WORDS * vc_cond_words4(m) + m * 8;
}
VC_COND_FN uint64_t vc_cond_sort_bytes(uint64_t n) {
  const uint64_t m = vc_cond_scratch_nodes(n);
  return 2 * (m * 8 + vc_cond_words4(m));
}

// ---- the host form's staging, every part 8-byte aligned: edges [n_edges] | nodes [max(n, 1) - 1] | labels [n] | node [n] | own [n] |
// leave [n]; the three optional arrays take their place whether asked for or not
struct VcCondStage {
  uint64_t edges, nodes, labels, node, own, leave, total;
  VcCondStage(uint64_t n, uint64_t n_edges) {
    uint64_t o = 0;
    edges = o;   o += n_edges * VC_COND_EDGE_BYTES;
    nodes = o;   o += vc_cond_node_cap(n) * VC_COND_NODE_BYTES;
    labels = o;  o += vc_cond_words4(n);
    node = o;    o += vc_cond_words4(n);
    own = o;     o += vc_cond_words4(n);
    leave = o;   o += vc_cond_words4(n);
    total = o ? o : 8;
  }
};
