// Plan arithmetic of vc_knn_graph_update* (vc_knn_graph_update.hip): the record <-> (block, thread, r) map of the join kernel, its
// LDS tile, the knobs, the window and halving rule, the merge's sub-batches and the scratch layout.  Plain C++ with no HIP in it, so
// that tests/cpp/knn_graph_update_plan_test.cc checks it on the CPU; the kernels and the driver call exactly these functions.
#pragma once
#include <stdint.h>

#include "vc_assign_plan.hpp"

#if defined(__HIPCC__)
#define VC_KU_FN __host__ __device__ inline
#else
#define VC_KU_FN inline
#endif

#define VC_KGUPD_BLOCK 256u                        // threads per block of vc_kgraph_join_kernel
#define VC_KGUPD_LDS_WORDS 2048u                   // 64-bit words of the staged tile of new codes: 16 KiB, the join kernel's whole LDS
#define VC_KGUPD_OLD_BATCH_DEFAULT (1u << 18)      // old ids per batch (VC_KGRAPH_OLD_BATCH)
#define VC_KGUPD_OLD_BATCH_MAX (1u << 24)
#define VC_KGUPD_WINDOW_DEFAULT 1024u              // new records per window (VC_KGRAPH_WINDOW)
#define VC_KGUPD_WINDOW_MAX (1u << 20)
#define VC_KGUPD_GATHER_CHUNK (1u << 18)           // new ids per gather of the new records' codes
#define VC_KGUPD_STAT_BYTES 64u                    // the device's counters, 64-bit words: see VC_KGUPD_ST_*

// the device's counters: the hits and the affected records of the count pass in flight (zeroed before each), the old rows changed,
// the entries of old rows that name a new record, the error word
enum { VC_KGUPD_ST_HITS = 0, VC_KGUPD_ST_AFFECTED = 1, VC_KGUPD_ST_CHANGED = 2, VC_KGUPD_ST_INSERTED = 3, VC_KGUPD_ST_BAD = 4 };

// ---- the knobs: 0 or a value above the limit means the default ---------------------------------------------------------------------------
VC_KU_FN uint32_t vc_kgupd_old_batch(uint64_t knob) { return knob == 0 || knob > VC_KGUPD_OLD_BATCH_MAX ? VC_KGUPD_OLD_BATCH_DEFAULT : (uint32_t)knob; }
VC_KU_FN uint32_t vc_kgupd_window(uint64_t knob) { return knob == 0 || knob > VC_KGUPD_WINDOW_MAX ? VC_KGUPD_WINDOW_DEFAULT : (uint32_t)knob; }

// ---- the join kernel's map: vc_assign_kernel's.  Block b owns the batch's records [b * block_records, ...); its thread t owns
// b * block_records + r * VC_KGUPD_BLOCK + t, r < R = vc_assign_records(W) -------------------------------------------------------------------
static_assert(VC_KGUPD_BLOCK == VC_ASSIGN_BLOCK, "the map is vc_assign_record_of's");
VC_KU_FN constexpr uint32_t vc_kgupd_records(uint32_t W) { return vc_assign_records(W); }
VC_KU_FN constexpr uint32_t vc_kgupd_block_records(uint32_t W) { return VC_KGUPD_BLOCK * vc_kgupd_records(W); }
VC_KU_FN uint64_t vc_kgupd_record_of(uint32_t W, uint64_t block, uint32_t thread, uint32_t r) { return vc_assign_record_of(W, block, thread, r); }
VC_KU_FN uint32_t vc_kgupd_blocks(uint32_t nb, uint32_t W) { return (uint32_t)(((uint64_t)nb + vc_kgupd_block_records(W) - 1) / vc_kgupd_block_records(W)); }
// new records per LDS tile, and those of the tile that starts at t0 of a window of nw records
VC_KU_FN constexpr uint32_t vc_kgupd_tile(uint32_t W) { return VC_KGUPD_LDS_WORDS / W; }
VC_KU_FN uint32_t vc_kgupd_tile_records(uint32_t t0, uint32_t nw, uint32_t W) { return nw - t0 < vc_kgupd_tile(W) ? nw - t0 : vc_kgupd_tile(W); }

// ---- the threshold of an old record: the last entry of a full row, anything for a row that is not full -----------------------------------
VC_KU_FN uint64_t vc_kgupd_threshold(uint32_t count, uint32_t k, uint64_t last) { return count == k ? last : 0xFFFFFFFFFFFFFFFFull; }
// the count of a row after h hits
VC_KU_FN uint32_t vc_kgupd_count(uint32_t count, uint64_t h, uint32_t k) { return count + h < k ? (uint32_t)(count + h) : k; }

// ---- THE WINDOW RULE.  An old batch starts with windows of `window` new records (the last of the new records may be shorter).  The
// count pass of a window of nw records finds H hits.  The window is ACCEPTED when nw == 1, or when its hit list of 8 H bytes fits the
// budget and H fits 32 bits.  Otherwise it is REFUSED: the window size becomes nw / 2 (at least 1) for this window AND for the rest
// of this old batch, and the count pass runs again from the same first record.  So the size only shrinks inside a batch, a refused
// window of nw records is followed by at most log2(nw) more refusals, and a window of one record is never refused.  The next old
// batch starts again at `window`. ------------------------------------------------------------------------------------------------------------
VC_KU_FN bool vc_kgupd_accept(uint64_t H, uint64_t budget, uint32_t nw) { return nw <= 1 || (H <= 0xFFFFFFFFull && 8 * H <= budget); }
VC_KU_FN uint32_t vc_kgupd_halve(uint32_t nw) { return nw / 2 < 1 ? 1u : nw / 2; }
VC_KU_FN uint32_t vc_kgupd_window_records(uint64_t j0, uint64_t n_new, uint32_t size) { return n_new - j0 < size ? (uint32_t)(n_new - j0) : size; }

// ---- the merge's sub-batches: the out-of-place rows of one merge launch hold at most `budget` bytes, but always one row ---------------
VC_KU_FN uint32_t vc_kgupd_merge_sub(uint64_t budget, uint32_t k) {
  const uint64_t b = budget / (8ull * k);
  return b < 1 ? 1u : b > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)b;
}
VC_KU_FN uint64_t vc_kgupd_merge_bytes(uint64_t affected, uint64_t budget, uint32_t k) {
  const uint64_t b = vc_kgupd_merge_sub(budget, k);
  return 8ull * k * (affected < b ? affected : b);
}
// the hit list of an accepted window: at least one word, so that the buffer exists
VC_KU_FN uint64_t vc_kgupd_hits_bytes(uint64_t H) { return 8 * (H ? H : 1); }

// ---- the scratch of a call beside the new codes, the hit list and the merge rows, for old batches of at most nb records of W words
// and gathers of at most ng ids, in bytes: the counters | cnt [nb] | flag [nb] | offs [nb] | rank [nb] | the affected list [nb] | the
// new counts [nb] | hits of a block [blocks] | mark [nb] bytes | the scan's work | ids [max(nb, ng)] | found [max(nb, ng)] | the
// batch's codes [nb][W].  Every word is written before it is read: the counters by a memset (all at the start, the first two before
// every count pass), cnt, flag and the blocks' hits by every count pass, offs and rank by the scans, the list and the new counts by
// the list and merge kernels up to the affected count, mark by a memset per batch, ids by the init launch, found and the codes by the
// store's gather.
struct VcKgupdWork {
  uint64_t stat, cnt, flag, offs, rank, list, newcnt, blk, mark, scan_work, ids, found, q, total;
  VcKgupdWork(uint32_t nb, uint32_t ng, uint32_t W, uint64_t scan_words) {
    const uint64_t row4 = ((uint64_t)nb * 4 + 7) & ~7ull, big = nb > ng ? nb : ng, big4 = (big * 4 + 7) & ~7ull;
    uint64_t o = 0;
    stat = o;       o += VC_KGUPD_STAT_BYTES;
    cnt = o;        o += row4;
    flag = o;       o += row4;
    offs = o;       o += row4;
    rank = o;       o += row4;
    list = o;       o += row4;
    newcnt = o;     o += row4;
    blk = o;        o += ((uint64_t)vc_kgupd_blocks(nb, W) * 4 + 7) & ~7ull;
    mark = o;       o += ((uint64_t)nb + 7) & ~7ull;
    scan_work = o;  o += (scan_words * 4 + 7) & ~7ull;
    ids = o;        o += big4;
    found = o;      o += big4;
    q = o;          o += (uint64_t)nb * W * 8;
    total = o;
  }
};
