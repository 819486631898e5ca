// Multi-index-hashing side of the engine (vc_mih.hip): index build, bucket views, radius-incremental search.
#pragma once
#include "vc_internal.hpp"

struct VcMihIndex;

int vc_mih_build(VcMihIndex** out, const uint64_t* d_cols, uint64_t stride, uint64_t n, uint32_t W, uint32_t m,
                 uint32_t sbits, uint32_t id_base, uint32_t flags, uint32_t n_cu, uint32_t cand_cap, const VcKnobs& knobs,
                 hipStream_t s, std::string* err);
void vc_mih_free(VcMihIndex* ix);
// Index update (build_hash_tables.cc:40-70: get bucket, append, put): *ix covers records [0, n0) of the columns, which now hold
// n >= n0.  Appended ids exceed every indexed id and a bucket is in ascending id order (rule a12), so the index of all n records
// is the old one with each new entry appended to its key's bucket: per table a sort of the n - n0 new (key, id) pairs, one
// insert point per pair, and one streaming merge of ids[] (and of the {id, code} records).  Bit for bit what vc_mih_build gives
// from all n records.  The VcMihIndex object, its scratch and counters stay.  On failure *ix is the old index (still covering n0
// records) or, once a table has been touched, freed and null -- never half merged.
int vc_mih_update(VcMihIndex** ix, const uint64_t* d_cols, uint64_t stride, uint64_t n, hipStream_t s, std::string* err);
uint64_t vc_mih_records(const VcMihIndex* ix);   // records the index covers
// VC_MIH_TRACE: "[vc_mih] index updated: n=.. added=.. route=merge|rebuild|none bent=merge|gather|0 bcodes=.. lines=.."
void vc_mih_update_trace(const VcMihIndex* ix, uint64_t added, const char* route, const char* bent);
// Index removal, the mirror image of the update: the columns hold the ks.k survivors of the ks.n records *ix covers, compacted in
// order.  Deleting records and renumbering the survivors in order is a monotone map on ids and a bucket is an ascending id run, so
// the index of the survivors is the old one with the dead entries dropped and the ids translated: per table one scan of the
// entries' keep flags and one stable scatter -- nothing is sorted.  Bit for bit what vc_mih_build gives from the survivors.  The
// VcMihIndex object, its scratch and counters stay.  0 < ks.k <= ks.n.  On failure *ix is freed and null: never half filtered, and
// never the old index, which names records that are gone.
struct VcKeepSet;
int vc_mih_retain(VcMihIndex** ix, const VcKeepSet& ks, const uint64_t* d_cols, uint64_t stride, hipStream_t s, std::string* err);
// VC_MIH_TRACE: "[vc_mih] index retained: n=.. removed=.. route=filter|rebuild|none bent=filter|gather|0 bcodes=.. lines=.."
void vc_mih_retain_trace(const VcMihIndex* ix, uint64_t removed, const char* route, const char* bent);
// index persistence: the CSR tables + bitmaps of a built index, and back (the codes themselves travel as a code file)
int vc_mih_save(VcMihIndex* ix, const uint64_t* d_cols, uint64_t stride, const char* path, hipStream_t s, std::string* err);
int vc_mih_load(VcMihIndex** out, const char* path, const uint64_t* d_cols, uint64_t stride, uint64_t n, uint32_t W, uint32_t m,
                uint32_t sbits, uint32_t id_base, uint32_t flags, uint32_t n_cu, uint32_t cand_cap, const VcKnobs& knobs,
                hipStream_t s, std::string* err);
// sums and resets the measurement records of mih_query_kernel: device time of its launches (HIP events on the launch
// stream) and the algorithmic work counters {bucket probes, non-empty buckets, bucket entries verified, queries}
void vc_mih_timing(VcMihIndex* ix, float* ms, uint32_t* launches, uint64_t totals[4], hipStream_t s);
// Cost-model switch of the exact k-NN loop (the reference loops blindly to radius 32, search_worker.cc:170):
// when the shells a query still has to probe cost more than streaming the shard once, the engine answers it with the
// verify kernel and REPLAYS the stop rule of search_worker.cc:201-205 on the scan's candidates, so that results and
// statistics are those of the radius loop.  Where a resolved query is left: the front of its candidate ring + the
// statistics arrays of the search tile (mih_export_kernel and the statistics read-back then treat it like any other).
struct VcMihScanTarget {
  uint64_t* ring;            // [slot][cap]
  uint32_t cap;
  uint32_t* count;           // [slot] results written to the ring front
  uint32_t* radius;          // [slot] last shell the radius loop would have searched
  unsigned long long* seen;  // [slot] distinct items that loop would have verified (only when want_stats)
  unsigned long long* sub;   // [slot] table 0's bucket gets (closed form: every leaf of shells 0..radius)
  unsigned long long* loc;   // [slot] 0 (no bitmap attached on this path)
};
// d_q: the tile's queries ([slot][W]); d_list[0..n): slots to answer; d_unresolved / d_n_unresolved: slots the scan could
// not settle (ring overflow, too many ties) -- they continue in the radius loop.  Enqueued on s, no host sync.
typedef int (*vc_mih_scan_fn)(void* ctx, const uint64_t* d_q, const uint32_t* d_list, uint32_t n, uint32_t k, uint32_t stop_mult,
                              const VcMihScanTarget& tgt, bool want_stats, uint32_t* d_unresolved, uint32_t* d_n_unresolved,
                              hipStream_t s);
struct VcMihScanFallback {
  vc_mih_scan_fn fn = nullptr;
  void* ctx = nullptr;
  uint32_t n_cu = 0;
};
// kernels of that switch (vc_mih.hip), launched by the engine between its select and recover launches
hipError_t vc_launch_sort_compact_segments(uint64_t* d_ring, uint32_t cap, const uint32_t* d_count, const uint64_t* d_offs,
                                           uint64_t* d_out, uint64_t out_cap, uint32_t nq, hipStream_t s);
hipError_t vc_launch_gather_queries(const uint64_t* d_q, const uint32_t* d_list, uint32_t n, uint32_t W, uint64_t* d_out, hipStream_t s);
struct VcMihReplayArgs {
  const uint64_t* lin_ring;   // [gq][lin_cap] candidate rings of the scan (complete: every item at or below the k-th distance)
  const uint32_t* lin_count;  // raw ring cursors, lin_qs words apart
  const uint64_t* rows;       // [gq][k] select output (ascending, INF padded)
  const uint32_t* rows_cnt;   // [gq] (UINT32_MAX = ring overflowed)
  const uint64_t* queries;    // [gq][W] gathered queries
  const uint32_t* list;       // [gq] slots
  const uint64_t* cols;
  uint64_t stride;
  uint32_t lin_cap, lin_qs, gq, k, m, sbits, W, stop_mult, id_base;
  VcMihScanTarget tgt;
  uint32_t* unresolved;
  uint32_t* n_unresolved;
  uint32_t* resolved_flag;    // [gq] 1 = settled here
};
hipError_t vc_launch_mih_replay(const VcMihReplayArgs& a, hipStream_t s);
// seen[list[i]] = #{items whose minimum substring distance <= radius[list[i]]} for the queries with flag[i] != 0
hipError_t vc_launch_minsub_count(const uint64_t* cols, uint64_t stride, uint64_t n, uint32_t W, uint32_t m, uint32_t sbits,
                                  const uint64_t* d_queries, const uint32_t* d_list, const uint32_t* d_flag, uint32_t nq,
                                  const uint32_t* d_radius, unsigned long long* d_seen, uint32_t n_cu, hipStream_t s);

// ids[q][0..cnt[q]) = the items at full distance dist[q] with minimum substring distance <= radius[q], smallest ids first,
// at most need[q] (<= k) of them (the tie check of the sharded global stop's union scan).  d_chunk_scratch: nq * VC_TIE_CHUNKS words.
#define VC_TIE_CHUNKS 1024u
hipError_t vc_launch_tie_collect(const uint64_t* cols, uint64_t stride, uint64_t n, uint32_t W, uint32_t m, uint32_t sbits, uint32_t id_base,
                                 const uint64_t* d_queries, uint32_t nq, uint32_t k, const uint32_t* d_dist, const uint32_t* d_radius,
                                 const uint32_t* d_need, uint32_t* d_chunk_scratch, uint32_t* d_ids, uint32_t* d_cnt, hipStream_t s);

#define MIH_APPROX_FACTOR 20u   // search_worker.h:14: the approximate loop stops at k * 20 distinct candidates (vc_mih.hip, vc_sharded.hip)
// d_q [nq][W]; d_out [nq][k] ascending INF-padded; d_cnt [nq]; stats (host, may be null) filled after a sync.
// d_stats (device, may be null): the same records written by a kernel in stream order, no host wait for them.
// r_cap < sbits: either mode capped at shell r_cap (stop rule active, no scan switch); a query still open there ends with
// radius = r_cap and the k best of shells 0..r_cap.
int vc_mih_search(VcMihIndex* ix, const uint64_t* d_cols, uint64_t stride, uint64_t n, const uint64_t* d_q, uint32_t nq,
                  uint32_t k, bool approximate, uint64_t* d_out, uint32_t* d_cnt, vc_query_stats* stats, hipStream_t s,
                  std::string* err, const VcMihScanFallback* fb = nullptr, vc_query_stats* d_stats = nullptr,
                  uint32_t r_cap = 0xFFFFFFFFu);
// last shell the exact k-NN query kernel runs in one launch for a full batch (the in-block reach)
uint32_t vc_mih_knn_reach(const VcMihIndex* ix);
int vc_mih_bucket(VcMihIndex* ix, uint32_t table, uint32_t index, std::vector<uint32_t>* local_ids, hipStream_t s,
                  std::string* err);
int vc_mih_bitmap_test(VcMihIndex* ix, uint32_t table, uint32_t index, int* bit, hipStream_t s, std::string* err);
int vc_mih_bitmap_read(VcMihIndex* ix, uint32_t table, uint64_t word_off, uint64_t n_words, uint32_t* out, hipStream_t s,
                       std::string* err);
// grow-only device buffers of the radius search, owned by the engine (allocation costs more than a search)
struct VcRadiusTotals {   // vc_radius_offsets_kernel's running totals: `total` and `largest` in device memory (tot[0], tot[1]), all in the mapped copy
  unsigned long long total;     // entries of the call so far
  unsigned long long largest;   // largest segment of the call so far (beyond the ring's capacity: the call is repeated)
  unsigned long long seq;       // mapped host copy only: sequence number of the call that wrote the two
  unsigned long long unused;
};
struct VcRadiusWork {
  uint64_t *d_ring = nullptr, *d_compact = nullptr, *d_offs = nullptr;
  uint32_t* d_aux = nullptr;
  VcRadiusTotals* h_tot = nullptr;       // pinned, mapped: the last vc_radius_offsets_kernel of a call publishes there
  VcRadiusTotals* h_tot_dev = nullptr;
  unsigned long long seq = 0;
  size_t aux_words = 0, offs_cap = 0;
  uint64_t compact_cap = 0;
  uint32_t cap = 0, tq = 0;
};
void vc_radius_work_free(VcRadiusWork* w);

// All items within full distance <= radius, ascending per query; ix may be null when use_mih is false (linear scan).
// device_out = false: out / out_offsets are host memory (staged through the engine's buffers);
// device_out = true : out (out_cap entries) / out_offsets (nq + 1) are device memory, everything is enqueued on `s`
// and the host synchronises once at the end.
// total_out (may be null; device_out only): the entries the call found, also when they exceed out_cap (VC_ERR_CAPACITY).
int vc_radius_search(VcMihIndex* ix, bool use_mih, const uint64_t* d_cols, uint64_t stride, uint64_t n, uint32_t W,
                     uint32_t id_base, uint32_t n_cu, const VcKnobs* knobs, const uint64_t* d_q, uint32_t nq, uint32_t radius,
                     uint64_t* out, uint64_t out_cap, uint64_t* out_offsets, bool device_out, VcRadiusWork* work, hipStream_t s,
                     std::string* err, uint64_t* total_out = nullptr);
