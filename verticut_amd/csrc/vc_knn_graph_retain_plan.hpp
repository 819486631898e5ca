// Plan arithmetic of vc_knn_graph_retain* (vc_knn_graph_retain.hip): the lanes a row takes in a wave, the rows a wave carries, the
// chunks of old rows that go through the out-of-place rows, the short rule and the scratch layout.  Plain C++ with no HIP in it, so
// that tests/cpp/knn_graph_retain_plan_test.cc checks it on the CPU; the kernels and the driver call exactly these functions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VC_KR_FN __host__ __device__ inline
#else
#define VC_KR_FN inline
#endif

#define VC_KGRET_WAVE 64u                          // = VC_WAVE
#define VC_KGRET_BLOCK 256u                        // threads per block of vc_kgraph_retain_kernel
#define VC_KGRET_STAT_BYTES 32u                    // the device's counters: see VC_KGRET_ST_*

// the device's counters, 64-bit words: the entries of surviving rows whose record was removed, the short rows (the kernel's tally),
// and one word of two halves: the length of the short list (low) and the error word (high)
enum { VC_KGRET_ST_DROPPED = 0, VC_KGRET_ST_SHORT = 1, VC_KGRET_ST_LIST = 2 };

// ---- the lane map.  A row takes a SEGMENT of P lanes, P the smallest power of two >= k, at most the wave; a wave carries 64 / P
// rows at once.  Lane l serves entry j0 + l % P of row l / P of the wave's group, j0 = 0, P, 2 P .. < k: one step for k <= 64, the
// chunk loop with a running base for a row wider than the wave -------------------------------------------------------------------------------
VC_KR_FN uint32_t vc_kgret_lanes(uint32_t k) {
  uint32_t p = 1;
  while (p < k && p < VC_KGRET_WAVE) p <<= 1;
  return p;
}
VC_KR_FN uint32_t vc_kgret_rows_per_wave(uint32_t k) { return VC_KGRET_WAVE / vc_kgret_lanes(k); }
VC_KR_FN uint32_t vc_kgret_steps(uint32_t k) { return (k + vc_kgret_lanes(k) - 1) / vc_kgret_lanes(k); }
// the lanes of segment r of a wave, as a ballot mask
VC_KR_FN uint64_t vc_kgret_segment_mask(uint32_t P, uint32_t r) { return (P >= 64 ? ~0ull : (1ull << P) - 1) << (r * P); }
// blocks of a launch over `rows` old rows
VC_KR_FN uint32_t vc_kgret_blocks(uint64_t rows, uint32_t k) {
  const uint64_t per_block = (uint64_t)(VC_KGRET_BLOCK / VC_KGRET_WAVE) * vc_kgret_rows_per_wave(k), b = (rows + per_block - 1) / per_block;
  return b < 1 ? 1u : b > 2048 ? 2048u : (uint32_t)b;
}

// ---- the chunks: the out-of-place rows hold at most `budget` bytes, but always one row; never more rows than the old graph has -----------
VC_KR_FN uint64_t vc_kgret_chunk_rows(uint64_t budget, uint32_t k, uint64_t n_old) {
  uint64_t b = budget / (8ull * k);
  if (b < 1) b = 1;
  return b < n_old ? b : (n_old ? n_old : 1);
}
// the out-of-place rows and their counts: rows [chunk][k] | counts [chunk]
VC_KR_FN uint64_t vc_kgret_rows_bytes(uint64_t chunk, uint32_t k) { return chunk * k * 8 + ((chunk * 4 + 7) & ~7ull); }

// ---- THE SHORT RULE.  A surviving row keeps m of its entries; they are the m smallest of the rebuilt row, which holds
// min(k, K - 1) entries, K the surviving count.  The row is short, and searched again, iff m is below that ---------------------------------
VC_KR_FN uint32_t vc_kgret_full(uint64_t K, uint32_t k) { return K == 0 ? 0u : (K - 1 < k ? (uint32_t)(K - 1) : k); }
VC_KR_FN bool vc_kgret_short(uint32_t m, uint64_t K, uint32_t k) { return m < vc_kgret_full(K, k); }

// ---- the scratch of a call beside the out-of-place rows, in bytes: the counters | live [n_old + 1] | rank [n_old + 1] | short
// [n_old] | srank [n_old] | the short list [K] | the scan's work (for n_old + 1 words).  Every word is written before it is read: the
// counters by a memset, live by the flag kernel (its last word is 0, so rank[n_old] is the live count), rank and srank by the scans,
// short by the translate kernel for every old row of every chunk, the list by the gather up to its length.
struct VcKgretWork {
  uint64_t stat, live, rank, shrt, srank, list, scan_work, total;
  VcKgretWork(uint64_t n_old, uint64_t K, uint64_t scan_words) {
    const uint64_t row4 = ((n_old + 1) * 4 + 7) & ~7ull;
    uint64_t o = 0;
    stat = o;       o += VC_KGRET_STAT_BYTES;
    live = o;       o += row4;
    rank = o;       o += row4;
    shrt = o;       o += row4;
    srank = o;      o += row4;
    list = o;       o += ((K ? K : 1) * 4 + 7) & ~7ull;
    scan_work = o;  o += (scan_words * 4 + 7) & ~7ull;
    total = o;
  }
};
