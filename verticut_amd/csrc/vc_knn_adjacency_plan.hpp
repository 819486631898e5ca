// Plan arithmetic of vc_knn_adjacency* (vc_knn_adjacency.hip): the argument checks, the 2^31 - 1 limit on the items, the passes of the
// sort, the bound on T, the scratch bytes, the lanes that serve a row of the mutual compaction, the boundary between the two teams of
// the merge and the staging layout of the host form.  Plain C++ with no HIP in it, so that tests/cpp/knn_adjacency_plan_test.cc checks
// it on the CPU; the kernels and the driver call exactly these functions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VC_ADJ_FN __host__ __device__ inline
#else
#define VC_ADJ_FN inline
#endif

#define VC_ADJ_MUTUAL 0u                  // = VC_KNN_MUTUAL
#define VC_ADJ_EITHER 1u                  // = VC_KNN_EITHER
#define VC_ADJ_REVERSE 2u                 // = VC_KNN_REVERSE
#define VC_ADJ_MAX_ITEMS 0x7FFFFFFFull    // N kk of a call: the scans and the sort's positions are 32-bit
#define VC_ADJ_STAT_BYTES 32u             // the device's block: edges | entries | empty segments | the longest segment, the error word
#define VC_ADJ_BLOCK 256u                 // threads of a block of every launch
#define VC_ADJ_WAVE 64u
// THE BOUNDARY between the two teams of the merge (VC_KNN_EITHER): a segment of up to this many words is merged by ONE WAVE (four
// records share a block), a longer one by the BLOCK.  Chosen from the code, not from a measurement: at 1024 a lane of the wave takes
// 16 words with one binary search each; a hub of thousands would hold its wave for as many searches while three waves idle.
#define VC_ADJ_TEAM_DEGREE 1024u
// static LDS of the sort's instantiations, from vc_sort.hip's arrays: the per-wave digit counters (4 x 256), the digit starts (257),
// the running offsets (256), the wave sums (4), and the staged sub-tile of 4096 keys and values
#define VC_ADJ_SORT_TILE 4096u
#define VC_ADJ_SORT_LDS_FIXED ((4u * 256u + 257u + 256u + 4u) * 4u)
#define VC_ADJ_SORT_LDS_BYTES (VC_ADJ_SORT_LDS_FIXED + VC_ADJ_SORT_TILE * (4u + 8u))   // 48 KiB of staging: 55316
#define VC_ADJ_SORT_LDS_LIMIT 65536u      // what a block may declare statically

// ---- the arguments (k already checked by vc_kgraph_k_ok) ----------------------------------------------------------------------------------
VC_ADJ_FN bool vc_adj_kk_ok(uint32_t k, uint32_t kk) { return kk >= 1 && kk <= k; }
VC_ADJ_FN bool vc_adj_flags_ok(uint32_t flags) { return flags <= VC_ADJ_REVERSE; }
VC_ADJ_FN bool vc_adj_items_ok(uint64_t n, uint32_t kk) { return n == 0 || n <= VC_ADJ_MAX_ITEMS / kk; }   // n kk <= 2^31 - 1, no overflow
VC_ADJ_FN bool vc_adj_sorts(uint32_t flags) { return flags != VC_ADJ_MUTUAL; }                            // VC_KNN_MUTUAL is row-local
// T never exceeds this
VC_ADJ_FN uint64_t vc_adj_bound(uint64_t n, uint32_t kk, uint32_t flags) { return (flags == VC_ADJ_EITHER ? 2ull : 1ull) * n * kk; }

// ---- the sort: by dist (digits of value >> 32), then by the target position; the sentinel key n sorts last -------------------------------
VC_ADJ_FN uint32_t vc_adj_bitlength(uint64_t x) {
  uint32_t b = 0;
  while (x) { ++b; x >>= 1; }
  return b;
}
// no listed entry is farther than min(max_dist, bits)
VC_ADJ_FN uint32_t vc_adj_dist_bits(uint32_t max_dist, uint32_t bits) { return vc_adj_bitlength(max_dist < bits ? max_dist : bits); }
VC_ADJ_FN uint32_t vc_adj_key_bits(uint64_t n) { return vc_adj_bitlength(n); }   // keys 0 .. n
VC_ADJ_FN uint32_t vc_adj_passes(uint32_t bits) { return (bits + 7) / 8; }
VC_ADJ_FN uint32_t vc_adj_sort_passes(uint64_t n, uint32_t max_dist, uint32_t bits) {
  return vc_adj_passes(vc_adj_dist_bits(max_dist, bits)) + vc_adj_passes(vc_adj_key_bits(n));
}

// ---- the scratch of a call, in bytes.  The items: two pairs of (key [n kk] u32, value [n kk] u64), 24 n kk -- none under
// VC_KNN_MUTUAL and none in a sizing call (adj_cap == 0).  The counters: n + 1 words, twice under VC_KNN_EITHER (the in-part and the
// whole segment), then the scan's work words.  Not bounded by VC_KGRAPH_SCRATCH: a sort cannot be chunked. ------------------------------
VC_ADJ_FN uint64_t vc_adj_key_bytes(uint64_t n, uint32_t kk, uint32_t flags, uint64_t adj_cap) {
  return vc_adj_sorts(flags) && adj_cap ? 2ull * 4 * n * kk : 0;
}
VC_ADJ_FN uint64_t vc_adj_val_bytes(uint64_t n, uint32_t kk, uint32_t flags, uint64_t adj_cap) {
  return vc_adj_sorts(flags) && adj_cap ? 2ull * 8 * n * kk : 0;
}
VC_ADJ_FN uint64_t vc_adj_item_bytes(uint64_t n, uint32_t kk, uint32_t flags, uint64_t adj_cap) {
  return vc_adj_key_bytes(n, kk, flags, adj_cap) + vc_adj_val_bytes(n, kk, flags, adj_cap);
}
VC_ADJ_FN uint32_t vc_adj_counter_arrays(uint32_t flags) { return flags == VC_ADJ_EITHER ? 2u : 1u; }
VC_ADJ_FN uint64_t vc_adj_counter_words(uint64_t n, uint32_t flags) { return vc_adj_counter_arrays(flags) * (n + 1); }

// ---- the mutual compaction: P lanes serve a row, 64 / P rows share a wave; P is the power of two >= kk, at most the wave ---------------
VC_ADJ_FN uint32_t vc_adj_row_lanes(uint32_t kk) {
  uint32_t p = 1;
  while (p < kk && p < VC_ADJ_WAVE) p <<= 1;
  return p;
}
// ---- the merge: who serves a segment of `degree` words
VC_ADJ_FN bool vc_adj_block_team(uint32_t degree) { return degree > VC_ADJ_TEAM_DEGREE; }

// ---- the host form's staging: rows [n][k] | offsets [n + 1] | adj [cap] | counts [n], every part 8-byte aligned; cap is the caller's
// adj_cap cut to the bound, which T never exceeds
struct VcAdjStage {
  uint64_t rows, offsets, adj, counts, cap, total;
  VcAdjStage(uint64_t n, uint32_t k, uint32_t kk, uint32_t flags, uint64_t adj_cap, bool with_counts) {
    const uint64_t bound = vc_adj_bound(n, kk, flags);
    cap = adj_cap < bound ? adj_cap : bound;
    uint64_t o = 0;
    rows = o;     o += n * k * 8;
    offsets = o;  o += (n + 1) * 8;
    adj = o;      o += cap * 8;
    counts = o;   o += with_counts ? (n * 4 + 7) & ~7ull : 0;
    total = o;
  }
};
