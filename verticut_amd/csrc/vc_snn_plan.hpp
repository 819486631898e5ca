// Plan arithmetic of vc_cluster_snn* (vc_snn.hip): the argument checks, the size of a row's hash set, the team that serves a row, the
// lanes that serve one listed entry, the statistics block and the staging layout of the host form.  Plain C++ with no HIP in it, so
// that tests/cpp/snn_plan_test.cc checks it on the CPU; the kernels and the driver call exactly these functions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VC_SNN_FN __host__ __device__ inline
#else
#define VC_SNN_FN inline
#endif

#define VC_SNN_PLAN_MAX_KK 1024u          // = VC_SNN_MAX_KK: the widest neighbour list the call intersects
#define VC_SNN_PLAN_NONE 0xFFFFFFFFu      // = VC_SNN_NONE; also the empty slot of the set: a position of the store is below it
// THE BOUNDARY between the two team shapes: up to this kk ONE WAVE serves a row (its set is a private LDS slice, several rows share
// a block, no block barrier between them); above it ONE BLOCK does.  Chosen from the code, not from a measurement: at 128 a wave's
// pass over row j is at most two 8-byte loads per lane and its slice 1 KiB; beyond it the serial passes of one wave over the kk
// entries grow with kk^2 / 64 while the other waves of the block could share the same set.
#define VC_SNN_WAVE_KK 128u
#define VC_SNN_BLOCK 256u                 // threads of a block of either shape
#define VC_SNN_WAVE 64u
#define VC_SNN_FLAG_EITHER 1u             // = VC_KNN_EITHER, the only flag bit

// ---- the arguments (k already checked by vc_kgraph_k_ok) ----------------------------------------------------------------------------------
VC_SNN_FN bool vc_snn_kk_ok(uint32_t k, uint32_t kk) { return kk >= 1 && kk <= k && kk <= VC_SNN_PLAN_MAX_KK; }
VC_SNN_FN bool vc_snn_flags_ok(uint32_t flags) { return (flags & ~VC_SNN_FLAG_EITHER) == 0; }

// ---- the set of a row: open addressing over a power of two of slots, at least 2 kk of them, so that at most half are ever taken
// and a probe sequence always meets an empty slot, whatever the row holds --------------------------------------------------------------
VC_SNN_FN uint32_t vc_snn_pow2_at_least(uint32_t x) {
  uint32_t p = 1;
  while (p < x) p <<= 1;
  return p;
}
VC_SNN_FN uint32_t vc_snn_table_slots(uint32_t kk) { return vc_snn_pow2_at_least(2 * kk); }      // 2 .. 2048
VC_SNN_FN uint32_t vc_snn_table_shift(uint32_t kk) {                                             // 32 - log2(slots): 21 .. 31
  uint32_t s = vc_snn_table_slots(kk), sh = 32;
  while (s > 1) { s >>= 1; --sh; }
  return sh;
}
// the home slot of position x: the high bits of a multiplicative hash (any function gives the same outputs, the set is a set)
VC_SNN_FN uint32_t vc_snn_slot(uint32_t x, uint32_t shift) { return (x * 0x9E3779B1u) >> shift; }

// ---- the teams ------------------------------------------------------------------------------------------------------------------------------
VC_SNN_FN bool vc_snn_wave_team(uint32_t kk) { return kk <= VC_SNN_WAVE_KK; }
VC_SNN_FN uint32_t vc_snn_team_waves(uint32_t kk) { return vc_snn_wave_team(kk) ? 1u : VC_SNN_BLOCK / VC_SNN_WAVE; }
VC_SNN_FN uint32_t vc_snn_rows_per_block(uint32_t kk) { return VC_SNN_BLOCK / VC_SNN_WAVE / vc_snn_team_waves(kk); }
// lanes of a wave that stride over row j for ONE listed entry: a power of two, the whole wave from kk = 33 on; a wave takes
// 64 / lanes entries in one pass, so that short lists do not leave most of it idle
VC_SNN_FN uint32_t vc_snn_entry_lanes(uint32_t kk) {
  const uint32_t p = vc_snn_pow2_at_least(kk);
  return p > VC_SNN_WAVE ? VC_SNN_WAVE : p;
}
// static LDS of the two kernels: the sets of a block's teams, then the histogram counters
#define VC_SNN_WAVE_SLOTS (2u * VC_SNN_WAVE_KK)
#define VC_SNN_BLOCK_SLOTS (2u * VC_SNN_PLAN_MAX_KK)
#define VC_SNN_LDS_BYTES_WAVE (4u * (VC_SNN_BLOCK / VC_SNN_WAVE) * VC_SNN_WAVE_SLOTS + 4u * VC_SNN_WAVE_KK)      // 4608
#define VC_SNN_LDS_BYTES_BLOCK (4u * VC_SNN_BLOCK_SLOTS + 4u * VC_SNN_PLAN_MAX_KK)                               // 12288
VC_SNN_FN uint32_t vc_snn_grid(uint64_t n, uint32_t kk) {
  const uint64_t rpb = vc_snn_rows_per_block(kk), blocks = (n + rpb - 1) / rpb;
  return blocks < 1 ? 1u : blocks > 256u * 16u ? 256u * 16u : (uint32_t)blocks;
}

// ---- the device's statistics block, 40 bytes: edges | mutual pairs | joined pairs | clusters | the largest weight, the error word ----
#define VC_SNN_STAT_BYTES 40u

// ---- the staging of the host form, in bytes: rows [n][k] | counts [n] | weights [n][kk] | histogram [kk]; the labels have a
// buffer of their own.  Parts the caller does not pass take no room ------------------------------------------------------------------
struct VcSnnStage {
  uint64_t rows, counts, shared, hist, total;
  VcSnnStage(uint64_t n, uint32_t k, uint32_t kk, bool with_counts, bool with_shared, bool with_hist) {
    uint64_t o = 0;
    rows = o;    o += n * k * 8;
    counts = o;  o += with_counts ? (n * 4 + 7) & ~7ull : 0;
    shared = o;  o += with_shared ? (n * kk * 4 + 7) & ~7ull : 0;
    hist = o;    o += with_hist ? (uint64_t)kk * 8 : 0;
    total = o;
  }
};
