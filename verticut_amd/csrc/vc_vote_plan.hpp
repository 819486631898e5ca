// Plan arithmetic of vc_knn_vote* and vc_label_propagate* (vc_vote.hip): the argument checks, the weight of an entry, the 64-bit
// winner key and its unpacking, the team shape of a segment by its length, the table slots of the two table shapes, the degree bins of
// the propagate plan, the scratch bytes and the staging layouts of the host forms.  Plain C++ with no HIP in it, so that
// tests/cpp/vote_plan_test.cc checks it on the CPU; the kernels and the drivers call exactly these functions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VC_VOTE_FN __host__ __device__ inline
#else
#define VC_VOTE_FN inline
#endif

#define VC_VOTE_LABEL_NONE 0xFFFFFFFFu    // = VC_VOTE_NONE
#define VC_VOTE_KIND_COUNT 0u             // = VC_VOTE_COUNT
#define VC_VOTE_KIND_CLOSENESS 1u         // = VC_VOTE_CLOSENESS
#define VC_VOTE_CLAMP 1u                  // = VC_LP_CLAMP_SEEDS
#define VC_VOTE_MAX_ITERS 64u             // = VC_LP_MAX_ITERS
#define VC_VOTE_HOST_STAT_BYTES 32u       // sizeof(vc_knn_vote_stats)
#define VC_VOTE_LP_HOST_STAT_BYTES 32u    // sizeof(vc_label_propagate_stats)
#define VC_VOTE_STAT_BYTES 64u            // the device's block of one launch set, see VcVoteStat in vc_vote.hip
#define VC_VOTE_PLAN_STAT_BYTES 128u      // room for the propagate plan's block (VcVotePlanStat) in front of the rounds' blocks
#define VC_VOTE_BLOCK 256u                // threads of a block of the plan, team, block-table and long launches
#define VC_VOTE_WAVE 64u
// ---- the team shapes: a segment of up to VC_VOTE_TEAM_MAX entries is served by P lanes of a wave, P the power of two at or above
// its length (at least VC_VOTE_TEAM_MIN); up to VC_VOTE_WAVE_MAX by one wave with an LDS table; up to VC_VOTE_SMALL_MAX and
// VC_VOTE_BIG_MAX by a block with an LDS table; above that by the table in the handle's scratch
#define VC_VOTE_TEAM_MIN 8u
#define VC_VOTE_TEAM_MAX 64u
#define VC_VOTE_WAVE_MAX 256u
#define VC_VOTE_SMALL_MAX 1024u
#define VC_VOTE_BIG_MAX 8192u
#define VC_VOTE_MIN_SLOTS 64u             // no table is smaller
#define VC_VOTE_SLOT_BYTES 8u             // (label u32, tally u32)
#define VC_VOTE_LONG_BLOCKS 64u           // blocks that stride over one long segment
#define VC_VOTE_LONG_AUX_BYTES 16u        // per long segment: the best key u64, the total u32, the labels at the top tally u32

enum VcVoteBin { VC_VOTE_BIN_P8, VC_VOTE_BIN_P16, VC_VOTE_BIN_P32, VC_VOTE_BIN_P64, VC_VOTE_BIN_WAVE, VC_VOTE_BIN_SMALL, VC_VOTE_BIN_BIG, VC_VOTE_BIN_LONG,
                 VC_VOTE_BINS };

// ---- the arguments ----------------------------------------------------------------------------------------------------------------------
VC_VOTE_FN bool vc_vote_k_ok(uint32_t k, uint32_t max_k) { return k >= 1 && k <= max_k; }
VC_VOTE_FN bool vc_vote_kk_ok(uint32_t k, uint32_t kk) { return kk >= 1 && kk <= k; }
VC_VOTE_FN bool vc_vote_kind_ok(uint32_t kind) { return kind <= VC_VOTE_KIND_CLOSENESS; }
VC_VOTE_FN bool vc_vote_lp_flags_ok(uint32_t flags) { return (flags & ~VC_VOTE_CLAMP) == 0; }
VC_VOTE_FN bool vc_vote_iters_ok(uint32_t max_iters) { return max_iters >= 1 && max_iters <= VC_VOTE_MAX_ITERS; }
// rows without counts: every row holds min(k, n) entries (search rows, which may name the record itself)
VC_VOTE_FN uint32_t vc_vote_row_count(uint64_t n, uint32_t k) { return n < k ? (uint32_t)n : k; }
VC_VOTE_FN uint32_t vc_vote_row_entries(uint32_t kk, uint32_t count) { return count < kk ? count : kk; }

// ---- the weight of a voting entry at distance d (d <= bits under CLOSENESS, checked by the caller) --------------------------------------
VC_VOTE_FN uint32_t vc_vote_weight(uint32_t kind, uint32_t bits, uint32_t d) { return kind == VC_VOTE_KIND_CLOSENESS ? bits + 1 - d : 1u; }
// a segment's tally is a 32-bit sum: length * (bits + 1) must fit
VC_VOTE_FN bool vc_vote_length_ok(uint64_t length, uint32_t bits) { return length <= 0xFFFFFFFFull / ((uint64_t)bits + 1); }

// ---- THE KEY of a label's first occurrence at position pos of its segment: tally << 32 | is-current << 31 | (2^31 - 1 - pos).  Its
// order is the contract's: the larger tally, then the current label, then the earliest first occurrence.  A key of 0 is no label
// (a tally is at least 1).  pos stays below 2^31 because vc_vote_length_ok holds
VC_VOTE_FN uint64_t vc_vote_key(uint32_t tally, bool is_current, uint32_t pos) {
  return ((uint64_t)tally << 32) | (is_current ? 0x80000000ull : 0ull) | (uint64_t)(0x7FFFFFFFu - pos);
}
VC_VOTE_FN uint32_t vc_vote_key_tally(uint64_t key) { return (uint32_t)(key >> 32); }
VC_VOTE_FN bool vc_vote_key_current(uint64_t key) { return (key & 0x80000000ull) != 0; }
VC_VOTE_FN uint32_t vc_vote_key_pos(uint64_t key) { return 0x7FFFFFFFu - ((uint32_t)key & 0x7FFFFFFFu); }
// rule 3 decided: several labels hold the top tally and the current label is none of them
VC_VOTE_FN bool vc_vote_is_tie(uint64_t key, uint32_t labels_at_top) { return labels_at_top > 1 && !vc_vote_key_current(key); }

// ---- shapes ---------------------------------------------------------------------------------------------------------------------------------
VC_VOTE_FN uint32_t vc_vote_pow2_at_least(uint64_t x) {
  uint32_t p = 1;
  while ((uint64_t)p < x && p < 0x80000000u) p <<= 1;
  return p;
}
VC_VOTE_FN uint32_t vc_vote_team_lanes(uint32_t length) {   // length <= VC_VOTE_TEAM_MAX
  const uint32_t p = vc_vote_pow2_at_least(length);
  return p < VC_VOTE_TEAM_MIN ? VC_VOTE_TEAM_MIN : p;
}
VC_VOTE_FN uint32_t vc_vote_bin(uint64_t length) {
  if (length <= 8) return VC_VOTE_BIN_P8;
  if (length <= 16) return VC_VOTE_BIN_P16;
  if (length <= 32) return VC_VOTE_BIN_P32;
  if (length <= VC_VOTE_TEAM_MAX) return VC_VOTE_BIN_P64;
  if (length <= VC_VOTE_WAVE_MAX) return VC_VOTE_BIN_WAVE;
  if (length <= VC_VOTE_SMALL_MAX) return VC_VOTE_BIN_SMALL;
  if (length <= VC_VOTE_BIG_MAX) return VC_VOTE_BIN_BIG;
  return VC_VOTE_BIN_LONG;
}
// the longest segment of a bin (the long bin has none)
VC_VOTE_FN uint32_t vc_vote_bin_max(uint32_t bin) {
  return bin == VC_VOTE_BIN_P8 ? 8u : bin == VC_VOTE_BIN_P16 ? 16u : bin == VC_VOTE_BIN_P32 ? 32u : bin == VC_VOTE_BIN_P64 ? VC_VOTE_TEAM_MAX
         : bin == VC_VOTE_BIN_WAVE ? VC_VOTE_WAVE_MAX : bin == VC_VOTE_BIN_SMALL ? VC_VOTE_SMALL_MAX : VC_VOTE_BIG_MAX;
}
// the open-addressing table of a segment: a power of two of slots, at most half full
VC_VOTE_FN uint64_t vc_vote_slots(uint64_t length) {
  uint64_t s = VC_VOTE_MIN_SLOTS;
  while (s < 2 * length) s <<= 1;
  return s;
}
VC_VOTE_FN uint32_t vc_vote_slot_of(uint32_t label, uint32_t log2_slots) { return (label * 0x9E3779B1u) >> (32u - log2_slots); }   // log2_slots in 6 .. 31
VC_VOTE_FN uint32_t vc_vote_log2(uint64_t pow2) {
  uint32_t b = 0;
  while ((1ull << b) < pow2) ++b;
  return b;
}
// the LDS of a table launch whose longest segment is `bound`: 4 KiB / 16 KiB / 128 KiB at the three bins' bounds
VC_VOTE_FN uint32_t vc_vote_lds_bytes(uint32_t bound) { return (uint32_t)vc_vote_slots(bound) * VC_VOTE_SLOT_BYTES; }
VC_VOTE_FN uint32_t vc_vote_table_threads(uint32_t bound) { return bound <= VC_VOTE_WAVE_MAX ? VC_VOTE_WAVE : VC_VOTE_BLOCK; }

// ---- the propagate plan: a block of the count and fill launches serves VC_VOTE_BLOCK records; counts[bin * blocks + block] is scanned
// once, which gives every (bin, block) its place in the one list of n records
VC_VOTE_FN uint64_t vc_vote_plan_blocks(uint64_t n) { return (n + VC_VOTE_BLOCK - 1) / VC_VOTE_BLOCK; }
VC_VOTE_FN uint64_t vc_vote_plan_count_words(uint64_t n) { return VC_VOTE_BINS * vc_vote_plan_blocks(n); }
VC_VOTE_FN uint64_t vc_vote_words4(uint64_t words) { return (words * 4 + 7) & ~7ull; }
// scratch of a propagate call, without the long tables: the list [n], the two label buffers [n] each, the counts
VC_VOTE_FN uint64_t vc_vote_lp_bytes(uint64_t n) { return 3 * vc_vote_words4(n) + vc_vote_words4(vc_vote_plan_count_words(n)); }
// the long segments: the aux blocks, then the tables' label words and tally words
VC_VOTE_FN uint64_t vc_vote_long_bytes(uint64_t n_long, uint64_t slots) { return n_long * VC_VOTE_LONG_AUX_BYTES + slots * VC_VOTE_SLOT_BYTES; }
// a long segment holds more than VC_VOTE_BIG_MAX entries, so there are at most this many (no empty buffer)
VC_VOTE_FN uint64_t vc_vote_long_cap(uint64_t n_entries) { return n_entries / (VC_VOTE_BIG_MAX + 1) + 1; }
// the per-round counters of a propagate call: VC_VOTE_MAX_ITERS blocks of VC_VOTE_STAT_BYTES behind the plan's block
VC_VOTE_FN uint64_t vc_vote_lp_stat_bytes() { return VC_VOTE_PLAN_STAT_BYTES + (uint64_t)VC_VOTE_MAX_ITERS * VC_VOTE_STAT_BYTES; }

// ---- the host forms' staging, every part 8-byte aligned.  vc_knn_vote: rows [n_rows][k] | labels [n] | out label, votes, total
// [n_rows] each | counts [n_rows].  vc_label_propagate: offsets [n + 1] | adj [n_entries] | labels in, out, votes, total [n] each
struct VcVoteStage {
  uint64_t rows, labels, out_label, out_votes, out_total, counts, total;
  VcVoteStage(uint64_t n_rows, uint32_t k, uint64_t n, bool with_counts) {
    uint64_t o = 0;
    rows = o;       o += n_rows * k * 8;
    labels = o;     o += vc_vote_words4(n);
    out_label = o;  o += vc_vote_words4(n_rows);
    out_votes = o;  o += vc_vote_words4(n_rows);
    out_total = o;  o += vc_vote_words4(n_rows);
    counts = o;     o += with_counts ? vc_vote_words4(n_rows) : 0;
    total = o ? o : 8;
  }
};
struct VcVoteLpStage {
  uint64_t offsets, adj, labels_in, labels_out, votes, totals, total;
  VcVoteLpStage(uint64_t n, uint64_t n_entries) {
    uint64_t o = 0;
    offsets = o;     o += (n + 1) * 8;
    adj = o;         o += n_entries * 8;
    labels_in = o;   o += vc_vote_words4(n);
    labels_out = o;  o += vc_vote_words4(n);
    votes = o;       o += vc_vote_words4(n);
    totals = o;      o += vc_vote_words4(n);
    total = o;
  }
};
