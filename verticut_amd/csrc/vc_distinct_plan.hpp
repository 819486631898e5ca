// Plan arithmetic of vc_search_knn_distinct* (vc_distinct.hip): the k' schedule of the rounds, the size class and LDS bytes of the
// collapse kernel for a k', the verdict on a collapsed row, and the cut of a round into sub-batches.  Plain C++ with no HIP in it, so
// that tests/cpp/distinct_plan_test.cc checks it on the CPU; the kernels and the driver call exactly these functions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VC_DP_FN __host__ __device__ inline
#else
#define VC_DP_FN inline
#endif

#define VC_DISTINCT_MAX_K 8192u                        // = VC_MAX_K: the widest row the search underneath returns
#define VC_DISTINCT_TRUNCATED_BIT 0x80000000u          // = VC_DISTINCT_TRUNCATED
#define VC_DISTINCT_SCRATCH_DEFAULT (64ull << 20)      // bytes of row scratch per sub-batch (VC_DISTINCT_SCRATCH)
#define VC_DISTINCT_WAVE_MAX 64u                       // k' <= 64: one wave per query, no LDS
#define VC_DISTINCT_BLOCK_MAX 1024u                    // k' <= 1024: one block of 256 threads per query
#define VC_DISTINCT_WAVES_PER_BLOCK 4u                 // queries per block of the wave form

// ---- the schedule: k'_0 = k_first, or min(VC_MAX_K, 2k) for k_first == 0; k'_{j+1} = min(VC_MAX_K, 2 k'_j) ------------------------------
VC_DP_FN bool vc_distinct_k_first_ok(uint32_t k, uint32_t k_first) {   // k already checked: 1 .. VC_MAX_K
  return k_first == 0 || (k_first >= k && k_first <= VC_DISTINCT_MAX_K);
}
VC_DP_FN uint32_t vc_distinct_next_k(uint32_t kp) { return kp >= VC_DISTINCT_MAX_K / 2 ? VC_DISTINCT_MAX_K : 2 * kp; }
VC_DP_FN uint32_t vc_distinct_first_k(uint32_t k, uint32_t k_first) { return k_first ? k_first : vc_distinct_next_k(k); }

// ---- the collapse kernel's form for a k' ----------------------------------------------------------------------------------------------
enum { VC_DISTINCT_WAVE = 0, VC_DISTINCT_BLOCK = 1, VC_DISTINCT_TABLE = 2 };
VC_DP_FN int vc_distinct_class(uint32_t kp) {
  return kp <= VC_DISTINCT_WAVE_MAX ? VC_DISTINCT_WAVE : kp <= VC_DISTINCT_BLOCK_MAX ? VC_DISTINCT_BLOCK : VC_DISTINCT_TABLE;
}
VC_DP_FN uint32_t vc_distinct_threads(uint32_t kp) {   // threads per block
  return vc_distinct_class(kp) == VC_DISTINCT_TABLE ? 1024u : 256u;
}
// P: the row positions the block forms lay out, the smallest power of two >= max(k', 64); the first-occurrence table has 2 P slots
VC_DP_FN uint32_t vc_distinct_positions(uint32_t kp) {
  uint32_t p = 64;
  while (p < kp) p <<= 1;
  return p;
}
VC_DP_FN uint32_t vc_distinct_slots(uint32_t kp) { return 2 * vc_distinct_positions(kp); }
// dynamic LDS of a launch: P labels + 2 P slots of 4 bytes (the wave form: none); 96 KiB at k' = 8192
VC_DP_FN uint32_t vc_distinct_lds_bytes(uint32_t kp) {
  return vc_distinct_class(kp) == VC_DISTINCT_WAVE ? 0u : 12u * vc_distinct_positions(kp);
}
VC_DP_FN uint32_t vc_distinct_grid(uint32_t kp, uint32_t n) {   // blocks of a launch over n rows
  return vc_distinct_class(kp) == VC_DISTINCT_WAVE ? (n + VC_DISTINCT_WAVES_PER_BLOCK - 1) / VC_DISTINCT_WAVES_PER_BLOCK : n;
}
// the slot a label's probe chain starts at (slots: a power of two); every bit of the label reaches the low bits (fmix32 of MurmurHash3)
VC_DP_FN uint32_t vc_distinct_hash(uint32_t x, uint32_t slots) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x & (slots - 1);
}

// ---- the verdict on a collapsed row: d distinct labels among the `cnt` entries the search at k' returned -------------------------------
enum { VC_DISTINCT_FULL = 0, VC_DISTINCT_SHORT = 1, VC_DISTINCT_CUT = 2, VC_DISTINCT_RETRY = 3, VC_DISTINCT_PASSED = 4 };
struct VcDistinctVerdict {
  uint32_t status;   // VC_DISTINCT_*
  uint32_t count;    // the word for counts[] (any status but RETRY)
  uint32_t written;  // entries of the row that are results, the rest is padding
};
VC_DP_FN VcDistinctVerdict vc_distinct_verdict(uint32_t d, uint32_t cnt, uint32_t kp, uint32_t k) {
  const uint32_t w = d < k ? d : k;
  if (cnt == 0xFFFFFFFFu) return VcDistinctVerdict{VC_DISTINCT_PASSED, 0xFFFFFFFFu, w};   // the recovery underneath gave up: passed on
  if (d >= k) return VcDistinctVerdict{VC_DISTINCT_FULL, k, k};
  if (cnt < kp) return VcDistinctVerdict{VC_DISTINCT_SHORT, d, d};                          // the database is exhausted
  if (kp >= VC_DISTINCT_MAX_K) return VcDistinctVerdict{VC_DISTINCT_CUT, d | VC_DISTINCT_TRUNCATED_BIT, d};
  return VcDistinctVerdict{VC_DISTINCT_RETRY, 0, 0};
}
// entries of a row of the search underneath that are there to be read
VC_DP_FN uint32_t vc_distinct_row_entries(uint32_t cnt, uint32_t kp) { return cnt == 0xFFFFFFFFu || cnt > kp ? kp : cnt; }
// THE SURE PREFIX.  A row of exact MIH holds every record nearer than its last distance D, but at D only SOME of the records that
// tie there (genuine ones, not necessarily the smallest ids: the loop underneath stops once the k'-th distance is settled).  A head
// taken from those ties could be the wrong member, or the wrong group, of its distance.  So where a row is full and a wider one can
// still be asked for, only the entries nearer than D count (`tie_cut`); a row that is not full holds the whole database, and at
// the widest row the ties are all there is to go by.  Returns the distance entries must stay below, 0xFFFFFFFF for no cut.
VC_DP_FN uint32_t vc_distinct_sure_below(bool tie_cut, uint32_t cnt, uint32_t kp, uint32_t last_dist) {
  return tie_cut && cnt == kp && kp < VC_DISTINCT_MAX_K ? last_dist : 0xFFFFFFFFu;
}

// ---- sub-batches: the rows scratch holds at most `budget` bytes, but always one row ----------------------------------------------------
VC_DP_FN uint32_t vc_distinct_batch(uint64_t budget, uint32_t kp) {
  const uint64_t b = budget / (8ull * kp);
  return b < 1 ? 1u : b > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)b;
}
VC_DP_FN uint32_t vc_distinct_n_batches(uint32_t n, uint64_t budget, uint32_t kp) {
  const uint32_t b = vc_distinct_batch(budget, kp);
  return n / b + (n % b ? 1u : 0u);
}
// bytes of rows scratch a round of n queries at k' needs
VC_DP_FN uint64_t vc_distinct_rows_bytes(uint32_t n, uint64_t budget, uint32_t kp) {
  const uint32_t b = vc_distinct_batch(budget, kp);
  return 8ull * kp * (n < b ? n : b);
}
