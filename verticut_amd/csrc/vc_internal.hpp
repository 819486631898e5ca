// Host-side launcher declarations shared by the translation units of libverticut_gpu.so.
#pragma once
#include <functional>

#include "vc_common.hpp"
#include "vc_scan_stream_plan.hpp"

// Developer / test knobs from the environment, read ONCE per engine at vc_create (never on a launch path).
struct VcKnobs {
  uint32_t scan_wrap = 0, scan_diag = 0;      // VC_SCAN_WRAP / VC_SCAN_DIAG (diagnostic build only; results wrong by design)
  bool sample2_set = false;                   // VC_SAMPLE2: size of the second bootstrap stage
  uint64_t sample2 = 0;
  bool sample1_set = false;                   // VC_SAMPLE1: size of the first bootstrap stage
  uint64_t sample1 = 0;
  bool shape_set = false;                     // VC_SCAN_SHAPE "U,BLK,DB"
  int shape_u = 0, shape_blk = 0, shape_db = 0;
  uint32_t sample_blocks_per_cu = 4;          // VC_SAMPLE_BLOCKS_PER_CU (8 -> 4 in round 3: -1.5..6 us per 125 M-code step, two A/B pairs)
  bool recover_trace = false;                 // VC_RECOVER_TRACE
  bool mih_trace = false;                     // VC_MIH_TRACE
  bool device_recover = true;                 // VC_DEVICE_RECOVER=0: ring overflow handled by the host-driven fallback only
  int mih_bcodes = -1;                        // VC_MIH_BCODES: -1 auto, 0 / 1 forced
  int mih_bent = -1;                          // VC_MIH_BENT: id + code records in bucket order (32-bit substrings of 64-bit codes): -1 auto, 0 / 1
  int scan_small = 1;                         // VC_SCAN_SMALL=0: the general (LDS-streamed) query loop for every tile size
  uint64_t mih_budget = 0;                    // VC_MIH_BUDGET: probes per query run inside mih_query_kernel (0 = automatic)
  int resident_mb = -1;                       // VC_SCAN_RESIDENT_MB: database prefix kept in the Infinity Cache by the verify pass (-1 = default)
  bool scan_trace = false;                    // VC_SCAN_TRACE=1 (diagnostic build): per-block start / end times of the verify kernel
  int mih_host_loop = 0;                      // VC_MIH_HOST_LOOP=1: one host round trip per shell (the round-1 loop)
  int mih_phases = 0;                         // VC_MIH_PHASES=1 (dev): per-phase times of mih_query_kernel on stderr
  int mih_switch = 1;                         // VC_MIH_SWITCH=0: the exact k-NN loop never switches to the verify kernel; 2: always (tests)
  int mih_stream = 1;                         // VC_MIH_STREAM=0: radius search over <= 16-bit substrings through the per-shell probe kernels
  int tau_fold = 0;                           // VC_TAU_FOLD=1: small tiles cut the bootstrap histograms in the verify prologue instead of a
                                              // vc_tau_init_kernel launch (measured: the 1024 prologues cost 20 us, the launch 5 -- off)
  int mih_poll = 1;                           // VC_MIH_POLL=0: wait for the query kernel's counters with hipStreamSynchronize instead of polling
  int mih_lines = -1;                         // VC_MIH_LINES: directory lines of the 32-bit tables (VcTableView::lines): -1 auto, 0 / 1
  int mih_qtile = 0;                          // VC_MIH_QTILE: most queries of one mih_query_kernel launch (0 = default 16384; 4096 .. 65536)
  int mih_order = 1;                          // VC_MIH_ORDER=0: mih_query_kernel's blocks take the queries in batch order (no longest-first pre-pass, mih_order_kernel)
  uint32_t timing_every = 1;                  // not an environment knob: vc_config.timing_sample under VC_FLAG_LEAN_TIMING (set by vc_create) --
                                              // the MIH kernels' launches are bracketed by events only every N-th time as well
  int mih_group = 0;                          // VC_MIH_GROUP=1..3: shells sharing the query kernel's first pass (0 = adaptive)
  uint32_t recover_spin_limit = 0;            // VC_RECOVER_SPIN_LIMIT: bound of the recovery grid barrier's spin (0 = default, ~3 s)
  uint32_t recover_test_fail = 0;             // VC_RECOVER_TEST_FAIL=N (tests): the first N recover launches wait for a block that never comes
  bool stream_trace = false;                  // VC_STREAM_TRACE (dev): per-block start / look-up / end times of mih_bucket_stream_kernel on stderr
  uint32_t gs_cap = 1;                        // VC_MIH_GS_CAP (dev): cap of the sharded global stop's first round
  bool gs_trace = false;                      // VC_MIH_GS_TRACE (dev): per-round wall times of the sharded global stop on stderr
  int mih_update = 1;                         // VC_MIH_UPDATE=0: vc_update_index rebuilds the whole index (A/B runs, tests) instead of merging
  int mih_retain = 1;                         // VC_MIH_RETAIN=0: vc_retain* compacts the columns and rebuilds the whole index (A/B runs, tests) instead of filtering it
  uint32_t group_window = 1u << 20;           // VC_GROUP_WINDOW: sorted positions per gather of vc_group_summary* (a multiple of 1024, else ignored)
  bool scan_shape_trace = false;              // VC_SCAN_SHAPE_TRACE=1 (dev/tests): every verify launch names the instantiation it launched on stderr
  uint32_t assign_tile = 0;                   // VC_ASSIGN_TILE (tests): centres per LDS tile of vc_assign_kernel (0 = all that fit, vc_assign_plan.hpp)
  uint32_t assign_slices = 0;                 // VC_ASSIGN_SLICES (tests): forces the number of centre slices of a vc_assign_kernel launch (0 = the plan's)
  uint64_t distinct_scratch = 64ull << 20;    // VC_DISTINCT_SCRATCH: bytes of k' rows a sub-batch of vc_search_knn_distinct* may hold (vc_distinct_plan.hpp)
  uint32_t filter_route = 0;                  // VC_FILTER_ROUTE (tests, A/B runs): 0 the plan's route of vc_search_knn_filtered*, 1 post-filter first, 2 pre-filter only
  uint64_t filter_scratch = 64ull << 20;      // VC_FILTER_SCRATCH: bytes of k' rows / of per-slice counters a sub-batch of vc_search_knn_filtered* may hold (vc_filter_plan.hpp)
  uint32_t filter_window = 1u << 20;          // VC_FILTER_WINDOW: allowed ids per window of the pre-filter route (0 or above 2^24: the default)
  uint64_t scope_scratch = 64ull << 20;       // VC_SCOPE_SCRATCH: bytes of (query, slice) counters a sub-batch of vc_search_knn_scoped* may hold (vc_scope_plan.hpp)
  uint32_t scope_window = 1u << 20;           // VC_SCOPE_WINDOW: positions of the scope-sorted list per window (0 or above 2^24: the default)
  uint64_t kgraph_scratch = 64ull << 20;      // VC_KGRAPH_SCRATCH: bytes of k' rows a sub-batch of vc_knn_graph* may hold (vc_knn_graph_plan.hpp)
  uint64_t kgraph_old_batch = 0;              // VC_KGRAPH_OLD_BATCH: old ids per batch of vc_knn_graph_update* (0 or above 2^24: the default 2^18, vc_knn_graph_update_plan.hpp)
  uint64_t kgraph_window = 0;                 // VC_KGRAPH_WINDOW: new records per window of vc_knn_graph_update* (0 or above 2^20: the default 1024)
  bool stream_free_set = false;             // VC_SCAN_STREAM_FREE (tests): the free device memory, in bytes, that vc_build_scan_stream's memory rule is given
  uint64_t stream_free = 0;
};
void read_knobs(VcKnobs* k);   // vc_engine.hip: the one place that reads the environment (once per engine / sharded handle)

// ---- vc_scan.hip ------------------------------------------------------------------------------
// Scan-kernel shape chosen per launch: BLK threads, U column loads per thread per chunk.
struct VcScanShape {
  int blk;      // 256 or 512
  int unroll;   // U
  int dbuf;     // register buffers per lane: 1 (rely on other waves), 2 (prefetch next chunk), 3 (two chunks ahead)
  int small;    // tiles of <= 8 queries use the compile-time-unrolled form of the kernel
  size_t lds;   // bytes of LDS the general form stages its query tile in
  uint64_t chunk_items() const { return 2ull * blk * unroll; }
};
// 16 B loads in flight per thread per buffer = U*W; keep the two register buffers <= 64 VGPRs each.
constexpr int vc_scan_default_unroll(int W) { return W <= 2 ? 4 : (W <= 4 ? 2 : 1); }
// The small-tile rule: a tile of qt queries in this shape runs the compile-time-unrolled form of the verify kernel.
inline bool vc_scan_shape_is_small(const VcScanShape& sh, uint32_t W, uint32_t qt) {
  return sh.small && sh.blk == 256 && sh.dbuf == 2 && qt <= 8 && sh.unroll == vc_scan_default_unroll((int)W);
}
// n_items: 0, or the database size when the caller wants the tile shape fitted to a small database
VcScanShape vc_scan_pick_shape(uint32_t W, uint32_t qt, const VcKnobs* knobs, uint64_t n_items = 0);
// What a pass over n codes is in a shape: its chunks, and how many of them (a prefix of resident_mb megabytes) stay in the
// Infinity Cache (see the load in vc_scan_kernel).  The shape handed to vc_launch_scan is the one this was derived from.
inline void vc_scan_extent(const VcScanShape& sh, uint64_t n, uint32_t bits, uint64_t resident_mb, VcScanParams* p) {
  p->nchunks = (n + sh.chunk_items() - 1) / sh.chunk_items();
  p->resident = (resident_mb << 20) / (sh.chunk_items() * (bits / 8));
}

float vc_probe_stream_ms(const uint64_t* cols, uint64_t stride, uint32_t W, uint64_t items, uint64_t* d_sink, uint32_t n_cu,
                         hipStream_t s);
hipError_t vc_launch_fill_synth(uint64_t* cols, uint64_t stride, uint32_t W, uint64_t first_local, uint64_t n,
                                uint64_t first_gid, uint64_t seed, uint32_t kind, uint32_t n_centres,
                                uint32_t max_flips, hipStream_t s);
hipError_t vc_launch_rows_to_cols(const uint64_t* rows, uint64_t* cols, uint64_t stride, uint32_t W,
                                  uint64_t first_local, uint64_t n, hipStream_t s);
hipError_t vc_launch_gather_rows(const uint64_t* cols, uint64_t stride, uint32_t W, const uint32_t* d_local_ids,
                                 uint32_t n_ids, uint64_t* d_rows, hipStream_t s);
// One stage of the threshold bootstrap (two launches): histogram of the first s_items codes (refine: only
// distances <= tau[q]), then tau[q] = k-th smallest sampled distance.  shist [qt][hist_stride] must be zero.
struct VcSampleArgs {
  const uint64_t* cols;
  uint64_t stride, s_items;
  uint32_t W, bits, k;
  const uint64_t* queries;
  uint32_t qt;
  uint32_t* shist;
  uint32_t hist_stride;
  uint32_t* tau;
  uint32_t qs;              // words between consecutive queries' entries of tau[]
  bool refine;
  bool cut;                 // false: no vc_tau_init_kernel launch, the consumer cuts the histograms itself
  uint32_t n_cu, blocks_per_cu;
};
hipError_t vc_launch_sample_hist(const VcSampleArgs& a, hipStream_t s);
// true when a tile of qt queries runs the small-tile form of the verify kernel (which can cut the bootstrap histograms itself)
bool vc_scan_is_small(uint32_t W, uint32_t qt, const VcKnobs* knobs);
// grid = min(chunks, CUs x resident blocks per CU, want_blocks if non-zero); sh: the shape p.nchunks was derived from
hipError_t vc_launch_scan(const VcScanParams& p, const VcScanShape& sh, uint32_t W, uint32_t n_cu, uint32_t want_blocks,
                          const VcKnobs* knobs, hipStream_t s);
// ---- the prefix-sorted 96-bit scan stream of a 128-bit store (vc_scan_stream.hip; arithmetic: vc_scan_stream_plan.hpp) --------
struct VcScanStream {
  uint32_t* d_base = nullptr;   // the one allocation, carved by `plan`; null = not built
  uint32_t* d_diag = nullptr;   // diagnostic build: the last launch's two counters (VcScanParams::st_diag)
  VcStreamPlan plan{};
  uint64_t launches = 0;        // stream verify launches since the build
  bool built() const { return d_base != nullptr; }
};
// true when a tile of qt queries over 128-bit codes may take the stream form: the rule of the small-tile form
bool vc_scan_stream_tile(uint32_t qt, const VcKnobs* knobs);
// Builds the stream of the n records behind cols (W = 2) on s and waits for it; *out must be unbuilt.  have_free / free_bytes:
// what the memory rule is given.  hipErrorOutOfMemory: the rule or an allocation refused, nothing is held.
hipError_t vc_scan_stream_build(const uint64_t* cols, uint64_t stride, uint64_t n, bool have_free, uint64_t free_bytes, VcScanStream* out,
                                hipStream_t s);
void vc_scan_stream_free(VcScanStream* st);   // on the current device
// the stream form of the verify launch: p as for vc_launch_scan (its extent is replaced by the stream's), 1 <= p.qt <= 8
hipError_t vc_launch_scan_stream(VcScanParams p, const VcScanStream& st, uint64_t resident_mb, uint32_t n_cu, uint32_t want_blocks,
                                 const VcKnobs* knobs, hipStream_t s);
// ring -> sorted top-k (per query); out padded with VC_PACK_INF
// d_tau (nullable): final per-query distance thresholds of the scan -- farther entries are dropped before sorting
hipError_t vc_launch_select_ring(const uint64_t* d_buf, uint32_t cap, const uint32_t* d_count, const uint32_t* d_tau, uint32_t qs,
                                 uint32_t nq, uint32_t k, uint64_t* d_out, uint32_t* d_out_count, hipStream_t s);
// same, for the ring slots named in d_list (outputs indexed by slot)
hipError_t vc_launch_select_ring_list(const uint64_t* d_buf, uint32_t cap, const uint32_t* d_count, const uint32_t* d_list,
                                      uint32_t n_list, uint32_t k, uint64_t* d_out, uint32_t* d_out_count, hipStream_t s);
// Exact device-side recovery of the rows whose ring overflowed (count > cap), after vc_launch_select_ring on the same
// buffers: no-op launch when nothing overflowed.  scratch: VcRecoverScratch::words words, zero at first use
// (the kernel restores its barrier words itself).  nq <= VC_REC_MAXQ.  clean_copies > 0: as the last kernel of the step it also
// zeroes the step's state for these queries (ring cursors count, thresholds clean_tau, hist, and clean_copies
// partial histograms clean_shist + c * clean_copy_stride), so that the next step needs no memset.
struct VcRecoverArgs {
  const uint64_t* cols;
  uint64_t stride, n;
  uint32_t W, id_base, bits;
  const uint64_t* queries;
  uint32_t nq, k;
  uint64_t* ring;
  uint32_t cap;
  const uint32_t* count;
  const uint32_t* hist;
  uint32_t hist_stride, qs;
  uint32_t* scratch;
  uint64_t* out;
  uint32_t* out_count;
  uint32_t* clean_tau;
  uint32_t* clean_shist;
  uint64_t clean_copy_stride;
  uint32_t clean_copies;
  uint32_t n_cu, spin_limit;
  uint32_t absent;          // test knob: blocks the barrier waits for in vain
};
hipError_t vc_launch_recover(const VcRecoverArgs& a, hipStream_t s);
// ---- vc_sort.hip: the index builder's primitives (hand-written; no device library is linked) --------------------
// exclusive prefix sum of L uint32 (in place allowed); d_work: vc_scan_work_words(L) words
size_t vc_scan_work_words(uint64_t L);
hipError_t vc_exclusive_scan_u32(const uint32_t* d_in, uint32_t* d_out, uint64_t L, uint32_t* d_work, hipStream_t s);
// stable LSD radix sort of n (key, value) pairs by the low key_bits bits of the key (8-bit digits).  Input in
// (keys[0], vals[0]); the passes ping-pong between the two buffer pairs and the result is in pair
// (vc_radix_sort_passes(key_bits) & 1).  d_work: vc_radix_sort_work_words(n) words.
uint32_t vc_radix_sort_passes(uint32_t key_bits);
size_t vc_radix_sort_work_words(uint64_t n);
hipError_t vc_radix_sort_pairs(uint32_t* keys[2], uint32_t* vals[2], uint64_t n, uint32_t key_bits, uint32_t* d_work, hipStream_t s);
// the same kernels with a 64-bit payload: stable sort of n items by (the low key_bits bits of the key, the low hi_bits bits of
// value >> 32) -- the passes over the value's high word first, then the key's; items equal in both keep their input order.  Buffers,
// work words and ping-pong as above; the result is in pair (vc_radix_sort_item_passes(hi_bits, key_bits) & 1).
uint32_t vc_radix_sort_item_passes(uint32_t hi_bits, uint32_t key_bits);
hipError_t vc_radix_sort_items(uint32_t* keys[2], uint64_t* vals[2], uint64_t n, uint32_t hi_bits, uint32_t key_bits, uint32_t* d_work, hipStream_t s);
// n_lists x [nq][k] sorted lists -> merged top-k
hipError_t vc_launch_select_lists(const uint64_t* d_lists, uint32_t n_lists, uint32_t nq, uint32_t k, uint64_t* d_out,
                                  uint32_t* d_out_count, hipStream_t s);
// ---- a handle as the drivers below see it: one table of grow-only scratch and a view of its store ------------------
// Grow-only device scratch: the pointer and how many bytes are behind it.  It has no destructor on purpose: hipFree acts on
// the CURRENT device, so the owner binds the buffer's device and then releases it.
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  hipError_t regrow(size_t need) {   // at least `need` bytes (rounded up to 256), on the current device; the contents are lost when it grows
    if (need <= bytes) return hipSuccess;
    hipError_t r = p ? hipFree(p) : hipSuccess;
    p = nullptr;
    bytes = 0;
    if (r != hipSuccess) return r;
    need = (need + 255) & ~(size_t)255;
    if ((r = hipMalloc(&p, need)) != hipSuccess) { p = nullptr; return r; }
    bytes = need;
    return hipSuccess;
  }
  void release() { (void)hipFree(p); p = nullptr; bytes = 0; }
  template <class T> T* as() const { return (T*)p; }
};
// The scratch of the drivers that serve both handle kinds, family after family, one buffer per purpose.  An engine holds the table as
// it is, a sharded store on its root device.  A driver writes every word it reads, so what an earlier call left there never matters.
enum VcScratch {
  // the clustering calls over the radius-graph walk (vc_walk.hip).  The walk's own: a batch's ids, gathered queries, found words, the
  // nq + 1 offsets and the raw results of the search.  The consumers': the statistics; one word per record (dbscan's degrees / core
  // distances when the caller passes none); leaders' state words of a batch; the host forms' staged labels.  The five calls share them.
  VC_WALK_IDS, VC_WALK_Q, VC_WALK_FOUND, VC_WALK_ROFFS, VC_WALK_RAW, VC_WALK_STAT, VC_WALK_RECORD, VC_WALK_STATE, VC_WALK_HLAB,
  VC_GROUPS_SCRATCH, VC_GROUPS_WORK, VC_GROUPS_STAGE,         // vc_groups.hip: sort / numbering arrays; rows + big-group tables; the host form's staging
  VC_KMAJ_WORK, VC_KMAJ_STAGE,                                // vc_assign.hip: the round driver's arrays; the host forms' staging
  VC_SEED_WORK, VC_SEED_STAGE,                                // vc_seed.hip: slots, statistics, partials, best; the host forms' staging
  VC_DISTINCT_WORK, VC_DISTINCT_ROWS, VC_DISTINCT_STAGE,      // vc_distinct.hip: flags, maps, retry queries, counters; the k' rows; the host forms' staging
  // k-NN by id (vc_ids.hip): gathered queries, found words, the k' rows and counts of the search underneath; the host form's staged
  // ids, rows, counts and statistics
  VC_KIDS_Q, VC_KIDS_FOUND, VC_KIDS_ROWS, VC_KIDS_CNT, VC_KIDS_HIDS, VC_KIDS_HROWS, VC_KIDS_HCNT, VC_KIDS_HSTATS,
  // radius search by id (vc_ids_radius.hip): gathered queries, found words, the uncompacted results and offsets of the search underneath,
  // the compaction's counts (VcIdsRadiusWork); the host form's staged ids, results and offsets
  VC_RIDS_Q, VC_RIDS_FOUND, VC_RIDS_RAW, VC_RIDS_ROFFS, VC_RIDS_WORK, VC_RIDS_HIDS, VC_RIDS_HOUT, VC_RIDS_HOFFS,
  // filtered k-NN (vc_filter.hip): the keep set (bits, rank, scan work); the rounds' flags, maps and listed queries; the k' rows; the
  // pre-filter route's arrays of a window and a sub-batch; a window's gathered codes; the host forms' staging
  VC_FILTER_KEEP, VC_FILTER_WORK, VC_FILTER_ROWS, VC_FILTER_PRE, VC_FILTER_CODES, VC_FILTER_STAGE,
  // scoped k-NN (vc_scope.hip): the query side's sort and tables; the keep set; the listed records, their sort and the segment table;
  // a sub-batch's histograms, cuts and counters; its candidate, running and merge rows; a window's gathered codes; the host forms' staging
  VC_SCOPE_QUERY, VC_SCOPE_KEEP, VC_SCOPE_LIST, VC_SCOPE_WORK, VC_SCOPE_ROWS, VC_SCOPE_CODES, VC_SCOPE_STAGE,
  // the k-NN graph (vc_knn_graph.hip): a batch's ids, codes, flags, maps and retry codes (VcKgraphWork); the k' rows; the host forms'
  // staging; vc_cluster_knn*'s statistics block and its in-degrees when the caller passes none
  VC_KGRAPH_WORK, VC_KGRAPH_ROWS, VC_KGRAPH_STAGE, VC_KGRAPH_STAT, VC_KGRAPH_DEG,
  // the graph's update (vc_knn_graph_update.hip): an old batch's arrays (VcKgupdWork); the new records' codes; a window's hit list;
  // the out-of-place rows of a merge launch; the host forms' staging
  VC_KGRAPH_UPD_WORK, VC_KGRAPH_UPD_NEW, VC_KGRAPH_UPD_HITS, VC_KGRAPH_UPD_ROWS, VC_KGRAPH_UPD_STAGE,
  // the graph after a removal (vc_knn_graph_retain.hip): the flags, ranks and the short list (VcKgretWork); the out-of-place rows and
  // counts of a chunk; the host forms' staging
  VC_KGRAPH_RET_WORK, VC_KGRAPH_RET_ROWS, VC_KGRAPH_RET_STAGE,
  // shared-nearest-neighbour clusters (vc_snn.hip): the statistics block; the host forms' staging (VcSnnStage) and their labels
  VC_SNN_STAT, VC_SNN_STAGE, VC_SNN_HLAB,
  // the graph's adjacency (vc_knn_adjacency.hip): the statistics block; the counters and the scan's work; the two key and the two value
  // buffers of the items; the sort's work; the host forms' staging (VcAdjStage)
  VC_ADJ_STAT, VC_ADJ_COUNT, VC_ADJ_KEYS, VC_ADJ_VALS, VC_ADJ_SORT, VC_ADJ_STAGE,
  // the graph's spanning forest (vc_knn_mst.hip): the statistics block; best, the forest and the snapshot; the two live buffers; the two
  // key and value buffers of the picked list; the sort's work; the host forms' staging (VcMstStage, VcMstCutStage)
  VC_MST_STAT, VC_MST_FOREST, VC_MST_LIVE, VC_MST_PICK, VC_MST_SORT, VC_MST_STAGE,
  // the label vote and label propagation (vc_vote.hip): the plan's and the rounds' statistics blocks; the list, the two label buffers
  // and the bin counts; the scan's work; the long segments' table offsets; their tables; the host forms' staging (VcVoteStage, VcVoteLpStage)
  VC_VOTE_STAT, VC_VOTE_PLAN, VC_VOTE_SCAN, VC_VOTE_LONG_OFF, VC_VOTE_LONG, VC_VOTE_STAGE,
  // the condensed tree of a spanning forest (vc_mst_condense.hip): the statistics block; the plan's first-edge table; the twelve words
  // per record; the working nodes and the finish's words per node; the sort's two key and value buffers; its work; the host form's
  // staging (VcCondStage)
  VC_COND_STAT, VC_COND_PLAN, VC_COND_WORK, VC_COND_TREE, VC_COND_SORT, VC_COND_SORT_WORK, VC_COND_STAGE,
  VC_SCRATCH_BUFS
};
// buffer `which` of the handle's table, at least `bytes` large, on the current device; null when it cannot be had (the handle keeps the text)
typedef std::function<void*(int which, size_t bytes)> VcScratchAlloc;
// What a driver needs of a handle for one call (the search mode and the call's stream are the closures' own).  gather, search and knn
// enqueue on that stream and return a VC_* code with the device of the handle's buffers current; none waits, but for search returning
// VC_ERR_CAPACITY (*raw_total entries do not fit cap): then everything enqueued has been waited for, so that the raw buffer may be
// regrown.  A closure that fails has left its text in the handle.
// the handle's unchanged k-NN search of nq queries [nq][W] at kp into d_rows [nq][kp], d_cnt [nq] and d_stats (nullable)
typedef std::function<int(const uint64_t* d_q, uint32_t nq, uint32_t kp, uint64_t* d_rows, uint32_t* d_cnt, vc_query_stats* d_stats)> VcKnnSearch;
struct VcStoreView {
  uint64_t n;               // resident records
  uint32_t id_base, W;
  VcScratchAlloc alloc;
  std::function<size_t(int which)> held;   // the bytes behind buffer `which` now: an earlier call may have left more than this one asks for
  std::function<int(const uint32_t* d_ids, uint32_t nq, uint64_t* d_q, uint32_t* d_found)> gather;   // ids -> rows [nq][W] + found words (vc_launch_ids_gather's fill rule)
  std::function<int(const uint64_t* d_q, uint32_t nq, uint32_t radius, uint64_t* d_raw, uint64_t cap, uint64_t* d_roffs, uint64_t* raw_total)> search;
  VcKnnSearch knn;
};
// v.search into buffer raw_buf of the table (*d_raw, holding at least the initial 64 Ki entries), at the capacity the handle really
// holds; on VC_ERR_CAPACITY repeated once with the buffer grown to the total it reported.  *raw_total: the entries found.
#define VC_RAW_FIRST_BYTES ((size_t)8 << 16)
int vc_search_raw(const VcStoreView& v, int raw_buf, const uint64_t* d_q, uint32_t nq, uint32_t radius, uint64_t** d_raw, uint64_t* d_roffs, uint64_t* raw_total);
// the text and code of a failed HIP call inside a driver: "<who>: <call>: <error>"
int vc_hip_fail(std::string* err, const char* who, hipError_t r, const char* what);
#define VC_HIP_OR_FAIL(who, call)                                      \
  do {                                                                 \
    hipError_t _r = (call);                                            \
    if (_r != hipSuccess) return vc_hip_fail(err, who, _r, #call);     \
  } while (0)
// ---- vc_ids.hip: queries named by id ------------------------------------------------------------------------------
// ids (global) -> d_q [nq][W] + d_found [nq] (nullable): an id outside [id_base, id_base + n) gives a zero row and found = 0.
// fill_n != 0: an id outside [fill_base, fill_base + fill_n) (the whole store's resident range) gets local record 0's code as its
// row, still with found = 0 -- a cheap stand-in query for the search whose row is thrown away
hipError_t vc_launch_ids_gather(const uint64_t* cols, uint64_t stride, uint32_t W, uint32_t id_base, uint64_t n, uint32_t fill_base,
                                uint64_t fill_n, const uint32_t* d_ids, uint32_t nq, uint64_t* d_q, uint32_t* d_found, hipStream_t s);
// rows [nq][kp] / cnt of a search with kp = k + 1 (the entry (0, id) is dropped if present) or kp = k (pass-through) -> d_out
// [nq][k], d_out_cnt (nullable), d_stats[i].n_results (d_stats nullable: the search's records, rewritten in place); found = 0
// gives a VC_PACK_INF row, count 0 and a zero record.  rows and d_out must not overlap.
hipError_t vc_launch_ids_strip(const uint32_t* d_ids, const uint32_t* d_found, const uint64_t* d_rows, const uint32_t* d_cnt, uint32_t nq,
                               uint32_t kp, uint32_t k, uint64_t* d_out, uint32_t* d_out_cnt, vc_query_stats* d_stats, hipStream_t s);
// the shards' gathered slots ([nq][W] words | nq found words, slot_words apart; bit g of mask: slot g is filled) ORed into d_q / d_found
inline uint64_t vc_ids_slot_words(uint32_t nq, uint32_t W) { return (uint64_t)nq * W + ((uint64_t)nq + 1) / 2; }
hipError_t vc_launch_ids_merge(const uint64_t* d_slots, uint64_t slot_words, uint32_t mask, uint32_t nq, uint32_t W, uint64_t* d_q,
                               uint32_t* d_found, hipStream_t s);
// the strip kernel's rule on host memory (counts non-null)
void vc_ids_strip_host(const uint32_t* ids, const uint32_t* found, const uint64_t* rows, const uint32_t* cnt, uint32_t nq, uint32_t kp, uint32_t k,
                       uint64_t* out, uint32_t* counts, vc_query_stats* stats);
// k-NN by id of either handle kind (vc_search_knn_ids*, vc_sharded_search_knn_ids*) in two steps, so that a handle can keep the
// allocations out of what it times: the VC_KIDS_* buffers of nq queries at kp = vc_ids_kp reserved, then gather, v.knn at kp and
// strip on s, nothing waited for
inline uint32_t vc_ids_kp(uint32_t k, uint32_t id_flags) { return k + ((id_flags & VC_IDS_EXCLUDE_SELF) ? 1u : 0u); }
struct VcIdsKnnBufs {
  uint64_t* d_q;
  uint32_t* d_found;
  uint64_t* d_rows;
  uint32_t* d_cnt;
};
int vc_ids_knn_reserve(const VcStoreView& v, uint32_t nq, uint32_t kp, VcIdsKnnBufs* b);
int vc_ids_knn_run(const VcStoreView& v, const VcIdsKnnBufs& b, const uint32_t* d_ids, uint32_t nq, uint32_t kp, uint32_t k, uint64_t* d_out, uint32_t* d_counts,
                   vc_query_stats* d_stats, hipStream_t s, std::string* err);
// either handle's host form: ids staged, `run` (the handle's device step on s) into staged outputs, which come home; waits for them.
// A flagged row of a linear search -- the device-side recovery gave up -- has the batch answered again by host_knn (the handle's
// host-form k-NN of the gathered codes at kp, ascending) and stripped by the kernel's rule.  counts, stats nullable
struct VcIdsKnnHostArgs {
  const uint32_t* ids;
  uint32_t nq, kp, k, order;
  bool linear;              // the mode is VC_MODE_LINEAR
  uint64_t* out;
  uint32_t* counts;
  vc_query_stats* stats;
};
int vc_ids_knn_run_host(const VcStoreView& v, const VcIdsKnnHostArgs& a,
                        const std::function<int(const VcIdsKnnBufs& b, const uint32_t* d_ids, uint64_t* d_out, uint32_t* d_counts, vc_query_stats* d_stats)>& run,
                        const std::function<int(const uint64_t* codes, uint64_t* rows, uint32_t* counts)>& host_knn, hipStream_t s, std::string* err);
// ---- vc_ids_radius.hip: radius search by id.  The raw result of the radius search underneath (d_raw ascending per query, d_roffs its nq + 1 offsets) is
// compacted segment by segment -- an entry stays when its query's id is resident (d_found) and id_flags (VC_IDS_EXCLUDE_SELF,
// VC_IDS_ONLY_GREATER) keep it.  The work is cut into (query, chunk) items of VC_IDS_RCHUNK entries; w.items bounds their number.
#define VC_IDS_RCHUNK 1024u
inline uint64_t vc_ids_radius_items(uint32_t nq, uint64_t raw_total) { return (uint64_t)nq + raw_total / VC_IDS_RCHUNK; }
struct VcIdsRadiusWork {   // all words of the scratch are written by the count launches before anything reads them
  uint64_t items;          // vc_ids_radius_items(nq, the raw total): must fit 32 bits
  uint64_t* total;         // the compacted total T
  uint32_t *cs, *qsum;     // [nq + 1] chunk starts, [nq] kept entries per query
  uint32_t *chunk_cnt, *chunk_base;   // [items] kept entries of a chunk, and of the query's chunks before it
  static size_t bytes(uint32_t nq, uint64_t items) { return 8 + ((size_t)nq * 2 + 1 + items * 2) * 4; }
  VcIdsRadiusWork(void* p, uint32_t nq, uint64_t items_) : items(items_) {
    total = (uint64_t*)p;
    cs = (uint32_t*)(total + 1);
    qsum = cs + nq + 1;
    chunk_cnt = qsum + nq;
    chunk_base = chunk_cnt + items;
  }
};
// plan + count + chunk scan + offsets: d_offsets[0 .. nq] (the compacted prefix sums) and *w.total, nothing is waited for
hipError_t vc_launch_ids_radius_count(const VcIdsRadiusWork& w, const uint64_t* d_raw, const uint64_t* d_roffs, const uint32_t* d_ids,
                                      const uint32_t* d_found, uint32_t nq, uint32_t id_flags, uint64_t* d_offsets, hipStream_t s);
// the kept entries, in order, to d_out[d_offsets[q] ..): the caller has made sure that *w.total entries fit
hipError_t vc_launch_ids_radius_copy(const VcIdsRadiusWork& w, const uint64_t* d_raw, const uint64_t* d_roffs, const uint32_t* d_ids, uint32_t nq,
                                     uint32_t id_flags, const uint64_t* d_offsets, uint64_t* d_out, hipStream_t s);
// Radius search by id of either handle kind (vc_search_radius_ids*, vc_sharded_search_radius_ids*), the whole call on s with the
// device of the handle's buffers current: gather, vc_search_raw into VC_RIDS_RAW, count / offsets, and, once T is known to fit (one
// wait, only when the raw total exceeds out_cap), the copy.  VC_ERR_CAPACITY: d_offsets holds the needed counts.
int vc_ids_radius_run(const VcStoreView& v, const uint32_t* d_ids, uint32_t nq, uint32_t radius, uint32_t id_flags, uint64_t* d_out, uint64_t out_cap,
                      uint64_t* d_offsets, hipStream_t s, std::string* err);
// either handle's host form: ids staged, `run` (the handle's device step on s) into staged outputs; the offsets come home also on
// VC_ERR_CAPACITY, the results behind them; waits for both
int vc_ids_radius_run_host(const VcStoreView& v, const uint32_t* ids, uint32_t nq, uint64_t* out, uint64_t out_cap, uint64_t* out_offsets,
                           const std::function<int(const uint32_t* d_ids, uint64_t* d_out, uint64_t* d_offsets)>& run, hipStream_t s, std::string* err);
// ---- vc_walk.hip: the radius-graph walk under the five clustering calls (vc_cluster_radius*, vc_cluster_levels*, vc_leaders_radius*,
// vc_dbscan_radius*, vc_dbscan_levels*) of both handle kinds.  Every record from a first position on goes through the handle's radius
// search, batch by batch in ascending id order, and one consume step per batch folds the RAW result into the caller's arrays.
#define VC_CLUSTER_BATCH 4096u   // ids per radius search underneath when the caller passes batch = 0
inline uint32_t vc_walk_batch(uint32_t batch) { return batch ? batch : VC_CLUSTER_BATCH; }
struct VcWalkBatch {        // the raw result (ascending per query) of the queries first_id .. first_id + nq - 1, as it lies in the walk's buffers
  const uint64_t* d_raw;
  const uint64_t* d_roffs;  // nq + 1 offsets, d_roffs[nq] = raw_total
  uint32_t nq;
  uint64_t raw_total;
  uint32_t first_id;
};
// The positions first_pos .. v.n - 1 in batches of vc_walk_batch(batch): per batch the ids filled on the device, the gather, the search
// at `radius` (vc_search_raw into VC_WALK_RAW) and consume (a VC_* code; it may wait).  The walk itself waits for nothing.  err: the
// text of a failure of the walk's own; a closure's is in the handle.
int vc_walk_run(const VcStoreView& v, uint64_t first_pos, uint32_t batch, uint32_t radius, const std::function<int(const VcWalkBatch&)>& consume, hipStream_t s,
                std::string* err);
// the host forms' labels staged in VC_WALK_HLAB (*d_labels): `planes` planes of v.n words, of each the first n_labelled copied in
int vc_walk_stage_labels(const VcStoreView& v, const uint32_t* labels, size_t planes, uint64_t n_labelled, uint32_t** d_labels, hipStream_t s, std::string* err);
#define VC_WALK_HIP(call) VC_HIP_OR_FAIL("radius walk", call)
// The five consumers below come in two forms, both the whole call on s with the device of the handle's buffers current, n > 0:
// vc_*_run on device pointers -- statistics zeroed, labels initialised, the walk, the passes after the last batch, then the one wait
// for the statistics (stats: host memory, nullable) -- and vc_*_run_host on host pointers: labels staged, run, copied home, waited for.
// ---- vc_cluster.hip: near-duplicate clustering (vc_cluster_radius*).  d_labels [n] is the union-find forest in place: slot i holds
// the global id of the parent of record id_base + i, never greater than id_base + i.  Nothing here waits but the two run forms.
// d_dst[j] = first + j for j < count: the labels of the records that come in unlabelled, and the ids of a batch
hipError_t vc_launch_cluster_init(uint32_t* d_dst, uint64_t count, uint32_t first, hipStream_t s);
// unites every kept entry of the raw result (d_raw, its nq + 1 offsets d_roffs, total = d_roffs[nq]) of the queries first_id ..
// first_id + nq - 1 with its query: kept = id > the query's own, or id < first_new (= id_base + n_labelled); *d_n_pairs += the kept
hipError_t vc_launch_cluster_union(const uint64_t* d_raw, const uint64_t* d_roffs, uint32_t nq, uint64_t total, uint32_t first_id, uint64_t first_new,
                                   uint32_t id_base, uint32_t* d_labels, uint64_t* d_n_pairs, hipStream_t s);
// d_labels[i] = the root of record i (the smallest id of its component), in place; *d_n_clusters += the roots
hipError_t vc_launch_cluster_flatten(uint32_t* d_labels, uint64_t n, uint32_t id_base, uint64_t* d_n_clusters, hipStream_t s);
// the records from n_labelled on walked and united, one flatten over all n; VC_WALK_STAT: 2 x uint64 (pairs, clusters)
int vc_cluster_run(const VcStoreView& v, uint32_t radius, uint32_t batch, uint64_t n_labelled, uint32_t* d_labels, vc_cluster_stats* stats, hipStream_t s,
                   std::string* err);
int vc_cluster_run_host(const VcStoreView& v, uint32_t radius, uint32_t batch, uint64_t n_labelled, uint32_t* labels, vc_cluster_stats* stats, hipStream_t s,
                        std::string* err);
// ---- vc_leaders.hip: greedy leader dedup (vc_leaders_radius*).  d_labels [n]: slot i holds the global id of the smallest-id leader
// within the radius of record id_base + i, its own id for a leader; entries below the batch are final and only read.
#define VC_LEADER_ROUND_GROUP 4u           // decision rounds enqueued between two read-backs of the undecided counter
#define VC_LEADER_BATCH_MAX (1u << 29)     // a larger `batch` is cut to this: the round number shares the state word with two flags
#define VC_LEADER_STAT_BYTES 64u           // d_stat: 3 x uint64 (pairs, leaders, rounds that had work), then the 3 round counters (+ 1 pad)
// One batch: the raw result (d_raw, its nq + 1 offsets d_roffs) of the queries first_id .. first_id + nq - 1 is decided in rounds of
// at most VC_LEADER_ROUND_GROUP launches between two waits on `s` for the undecided counter, then the batch's labels are written.
// d_state: nq words of scratch, every one written by the first round.  d_stat[0] += the entries (query b, neighbour a < b),
// d_stat[2] += the rounds that had work.  *stuck: queries were still undecided after nq rounds (cannot happen; the caller reports it).
hipError_t vc_leaders_decide_batch(const uint64_t* d_raw, const uint64_t* d_roffs, uint32_t nq, uint32_t first_id, uint32_t id_base, uint32_t* d_labels,
                                   uint32_t* d_state, uint64_t* d_stat, hipStream_t s, bool* stuck);
// *d_n_leaders += the records i < n with d_labels[i] == id_base + i; nothing is waited for
hipError_t vc_launch_leaders_count(const uint32_t* d_labels, uint64_t n, uint32_t id_base, uint64_t* d_n_leaders, hipStream_t s);
// the records from n_labelled on walked in batches of at most VC_LEADER_BATCH_MAX and decided (a wait per group of rounds), one count
// over all n; the entries below n_labelled are only read, and the host form does not copy them back
int vc_leaders_run(const VcStoreView& v, uint32_t radius, uint32_t batch, uint64_t n_labelled, uint32_t* d_labels, vc_leader_stats* stats, hipStream_t s,
                   std::string* err);
int vc_leaders_run_host(const VcStoreView& v, uint32_t radius, uint32_t batch, uint64_t n_labelled, uint32_t* labels, vc_leader_stats* stats, hipStream_t s,
                        std::string* err);
// ---- vc_dbscan.hip: density clustering (vc_dbscan_radius*).  d_labels [n] starts as the own ids (vc_launch_cluster_init): a core's
// slot is the forest of vc_forest.hpp over the cores, a non-core's slot its smallest core neighbour seen so far, its own id for
// none; d_degrees [n] says which is which.  Nothing here waits.
#define VC_DBSCAN_STAT_BYTES 40u   // d_stat: 5 x uint64 in the order of vc_dbscan_stats (pairs, clusters, cores, borders, noise)
// One batch, two launches over the raw result (d_raw, its nq + 1 offsets d_roffs, total = d_roffs[nq]) of the queries first_id ..
// first_id + nq - 1: d_degrees[first_id - id_base + q] = the length of segment q, then every entry (own, v < own) unites two cores
// or lowers the non-core member's anchor to the core.  The degrees below first_id must be final.  *d_n_pairs += the entries v < own.
hipError_t vc_launch_dbscan_edges(const uint64_t* d_raw, const uint64_t* d_roffs, uint32_t nq, uint64_t total, uint32_t first_id, uint32_t id_base,
                                  uint32_t min_pts, uint32_t* d_degrees, uint32_t* d_labels, uint64_t* d_n_pairs, hipStream_t s);
// after the last batch, in place: d_labels[i] = the root of a core, the root of a border's anchor, the own id of noise;
// d_counts[0 .. 3] += the roots among the cores, the cores, the borders, the noise
hipError_t vc_launch_dbscan_finish(uint32_t* d_labels, const uint32_t* d_degrees, uint64_t n, uint32_t id_base, uint32_t min_pts, uint64_t* d_counts,
                                   hipStream_t s);
// every record walked from position 0, one finish pass; d_degrees null: the handle's own (VC_WALK_RECORD); degrees (host) nullable
int vc_dbscan_run(const VcStoreView& v, uint32_t radius, uint32_t min_pts, uint32_t batch, uint32_t* d_labels, uint32_t* d_degrees, vc_dbscan_stats* stats,
                  hipStream_t s, std::string* err);
int vc_dbscan_run_host(const VcStoreView& v, uint32_t radius, uint32_t min_pts, uint32_t batch, uint32_t* labels, uint32_t* degrees, vc_dbscan_stats* stats,
                       hipStream_t s, std::string* err);
// ---- vc_levels.hip: single-linkage clusters at every radius 0 .. max_radius in one walk (vc_cluster_levels*).  d_labels is level-major,
// (max_radius + 1) x n: level r at d_labels + r * n is a forest of vc_forest.hpp in place, as vc_cluster.hip's.  Nothing here waits.
#define VC_LEVELS_STAT_BYTES 1024u   // d_stat: vc_levels_stats as it lies (64 pair counters, then 64 cluster counters)
// every kept entry (vc_launch_cluster_union's keep rule) of distance d is united with its query in forest d only;
// d_n_pairs[d] += the kept entries of distance d
hipError_t vc_launch_levels_union(const uint64_t* d_raw, const uint64_t* d_roffs, uint32_t nq, uint64_t total, uint32_t first_id, uint64_t first_new,
                                  uint32_t id_base, uint64_t n, uint32_t max_radius, uint32_t* d_labels, uint64_t* d_n_pairs, hipStream_t s);
// after the last batch: max_radius launches, level r takes in the components of level r - 1
hipError_t vc_launch_levels_cascade(uint32_t* d_labels, uint64_t n, uint32_t id_base, uint32_t max_radius, hipStream_t s);
// d_labels[r * n + i] = the root of record i at level r, in place, every level in one launch; d_n_clusters[r] += the roots of level r
hipError_t vc_launch_levels_flatten(uint32_t* d_labels, uint64_t n, uint32_t id_base, uint32_t max_radius, uint64_t* d_n_clusters, hipStream_t s);
// the records from n_labelled on walked at max_radius (the first n_labelled of every level come in labelled), the cascade, one flatten
int vc_levels_run(const VcStoreView& v, uint32_t max_radius, uint32_t batch, uint64_t n_labelled, uint32_t* d_labels, vc_levels_stats* stats, hipStream_t s,
                  std::string* err);
int vc_levels_run_host(const VcStoreView& v, uint32_t max_radius, uint32_t batch, uint64_t n_labelled, uint32_t* labels, vc_levels_stats* stats, hipStream_t s,
                       std::string* err);
// ---- vc_dbscan_levels.hip: density clustering at every radius 0 .. max_radius in one walk (vc_dbscan_levels*).  d_labels is level-major,
// (max_radius + 1) x n, every slot starts as the own id (vc_launch_cluster_init per level); d_core_dist [n] says whether slot (r, i)
// is the forest of level r (d_core_dist[i] <= r) or record i's anchor candidate of exactly level r.  Nothing here waits.
#define VC_DBSCAN_LEVELS_STAT_BYTES 2560u   // d_stat: vc_dbscan_levels_stats as it lies (5 x 64 counters: pairs, clusters, cores, borders, noise)
// One batch, two launches over the raw result at max_radius of the queries first_id .. first_id + nq - 1: their core distances
// (the distance of entry min_pts - 1 of a segment, VC_CORE_NEVER for a shorter one), then every entry (own, v < own) of distance d
// is united in forest max(d, both core distances) and lowers the anchor candidates of its two ends.  The core distances below
// first_id must be final.  d_n_pairs[d] += the entries v < own of distance d.
hipError_t vc_launch_dbscan_levels_edges(const uint64_t* d_raw, const uint64_t* d_roffs, uint32_t nq, uint64_t total, uint32_t first_id, uint32_t id_base,
                                         uint64_t n, uint32_t max_radius, uint32_t min_pts, uint32_t* d_core_dist, uint32_t* d_labels, uint64_t* d_n_pairs,
                                         hipStream_t s);
// after the last batch: max_radius launches, the cores of level r - 1 carry their components into level r
hipError_t vc_launch_dbscan_levels_cascade(uint32_t* d_labels, const uint32_t* d_core_dist, uint64_t n, uint32_t id_base, uint32_t max_radius, hipStream_t s);
// d_labels[r * n + i] = the root of a core, the root of a border's anchor (the smallest candidate of the levels <= r), the own id of
// noise, in place, one launch; d_counts [4][VC_LEVELS_MAX]: [0][r] += the roots among the cores of level r, [1] cores, [2] borders, [3] noise
hipError_t vc_launch_dbscan_levels_finish(uint32_t* d_labels, const uint32_t* d_core_dist, uint64_t n, uint32_t id_base, uint32_t max_radius,
                                          uint64_t* d_counts, hipStream_t s);
// every record walked from position 0 at max_radius, the cascade, one finish pass; d_core_dist null: the handle's own (VC_WALK_RECORD);
// core_dist (host) nullable
int vc_dbscan_levels_run(const VcStoreView& v, uint32_t max_radius, uint32_t min_pts, uint32_t batch, uint32_t* d_labels, uint32_t* d_core_dist,
                         vc_dbscan_levels_stats* stats, hipStream_t s, std::string* err);
int vc_dbscan_levels_run_host(const VcStoreView& v, uint32_t max_radius, uint32_t min_pts, uint32_t batch, uint32_t* labels, uint32_t* core_dist,
                              vc_dbscan_levels_stats* stats, hipStream_t s, std::string* err);
// ---- vc_groups.hip: label groups summarised (vc_group_summary*, vc_sharded_group_summary*).  One driver for both handle kinds: the
// codes of a window's sorted ids come through `fetch` (vc_get_codes_dev / the sharded gather, enqueued on s, nothing waited for)
// as contiguous rows [nq][W].  The plan arithmetic is vc_groups_plan.hpp.
struct VcGroupsArgs {
  uint64_t n;               // resident records
  uint32_t id_base, W, window;   // window: VcKnobs::group_window
  const uint32_t* d_labels;
  uint64_t groups_cap;
  vc_group* d_groups;
  uint64_t* d_centroids;    // nullable, as d_rep_labels and d_group_index
  uint32_t* d_rep_labels;
  uint32_t* d_group_index;
  // the handle's grow-only buffer number `which`, at least `bytes` large, on the current device; null when it cannot be had (the
  // handle keeps the error text).  The driver writes every word it reads, so what an earlier call left there never matters.
  VcScratchAlloc alloc;
};
typedef std::function<int(const uint32_t* d_ids, uint32_t nq, uint64_t* d_rows)> VcGroupsFetch;
// the whole call on s with the device of the buffers current: one wait (error flag, G, items, big groups), scratch from a.alloc
int vc_groups_run(const VcGroupsArgs& a, const VcGroupsFetch& fetch, uint64_t* n_groups, hipStream_t s, std::string* err);
// the same for host pointers: labels staged, the outputs that are wanted staged and copied home, waited for (a's pointers are ignored)
int vc_groups_run_host(VcGroupsArgs a, const VcGroupsFetch& fetch, const uint32_t* labels, vc_group* groups, void* centroids, uint32_t* rep_labels,
                       uint32_t* group_index, uint64_t* n_groups, hipStream_t s, std::string* err);
// ---- vc_assign.hip: nearest of K given codes (vc_assign_nearest*) and the k-majority rounds on top of it (vc_kmajority*).  The plan
// arithmetic is vc_assign_plan.hpp.
// d_out[j] = c | dist << 32, c the centre (of K rows [W], 8-byte aligned) with the smallest (distance, index) for local record
// first + j, j < count; the caller has checked first + count <= the records behind cols.  One launch, or an init launch and one
// whose centre slices meet in atomicMin; nothing is waited for, no scratch.
hipError_t vc_launch_assign(const uint64_t* cols, uint64_t stride, uint32_t W, uint64_t first, uint64_t count, const uint64_t* d_centres, uint32_t K,
                            uint64_t* d_out, uint32_t n_cu, const VcKnobs* knobs, hipStream_t s);
// the handle's assign over a range fixed by the caller (all N records for the rounds), enqueued on the call's stream, nothing waited for
typedef std::function<int(const uint64_t* d_centres, uint64_t* d_out)> VcAssignAll;
// vc_assign_nearest for host pointers: centres staged, `run` into a staged output of `count` words, which comes home; waits for it
int vc_assign_run_host(const VcScratchAlloc& alloc, uint32_t W, const void* centres, uint32_t K, uint64_t count, uint64_t* out,
                       const VcAssignAll& run, hipStream_t s, std::string* err);
struct VcKmajArgs {
  uint32_t n_centres, max_iters;   // checked by the caller: 1 <= n_centres <= N, max_iters <= VC_KMAJ_MAX_ITERS
  uint64_t* d_centres;             // in: seeds, out: final
  uint64_t* d_assign;              // N packed
  uint32_t* d_labels;              // N, nullable
  VcScratchAlloc alloc;   // the handle's grow-only buffers VC_KMAJ_*
};
// One driver for both handle kinds, on s with the device of the buffers current.  g: the handle's VcGroupsArgs (n, id_base, W, window,
// alloc -- the pointers are set here); one wait per round and vc_groups_run's, one at the end.  stats nullable.
int vc_kmajority_run(const VcKmajArgs& k, VcGroupsArgs g, const VcAssignAll& assign_all, const VcGroupsFetch& fetch, vc_kmajority_stats* stats, hipStream_t s,
                     std::string* err);
// the same for host pointers (k's pointers are ignored): seeds staged, centres, assign and labels (nullable) come home, waited for
int vc_kmajority_run_host(VcKmajArgs k, const VcGroupsArgs& g, const VcAssignAll& assign_all, const VcGroupsFetch& fetch, void* centres, uint64_t* assign,
                          uint32_t* labels, vc_kmajority_stats* stats, hipStream_t s, std::string* err);
// ---- vc_seed.hip: device-side seeding (vc_seed_centres*, vc_sharded_seed_centres*).  The plan arithmetic -- generator, block ranges,
// slot word (dist << 32 | 0xFFFFFFFF - i), prefix search -- is vc_seed_plan.hpp.  Nothing here waits but vc_seed_run with stats.
// One round over the n records behind cols: best[i] lowered to (distance to the centre, t) where strictly smaller (t == 0: best counts
// as infinity), then the reduction of the NEW best for the next pick.  A slot is n_slot <= VC_SEED_SUBSLOTS words VC_SEED_SLOT_STRIDE
// apart whose maximum is the pick.  The centre is the record that slot d_slot_prev names (then its code goes to d_centre_out [W], the
// slot word to *d_slot_rec and id_base + index | dist << 32 to *d_pick_out, both nullable; the VC_SEED_SUBSLOTS words of d_slot_zero,
// nullable, are cleared), or the W words at d_code when that is not null (a shard: the root fetched them; none of those is used).
// Farthest: the blocks' maxima meet in atomicMax on the n_slot_next words of d_slot_next, which must be 0 before; weighted:
// d_partial[vc_seed_blocks(n)] gets the blocks' sums.  Both may be null: no reduction.
struct VcSeedRound {
  const uint64_t* cols;
  uint64_t stride, n;
  uint32_t W, id_base, t, method;
  const uint64_t* d_slot_prev;
  uint32_t n_slot_prev;
  const uint64_t* d_code;
  uint64_t* d_centre_out;
  uint64_t* d_pick_out;
  uint64_t* d_slot_rec;
  uint64_t* d_best;
  uint64_t* d_slot_next;
  uint32_t n_slot_next;
  uint64_t* d_slot_zero;
  uint32_t* d_partial;
};
hipError_t vc_launch_seed_round(const VcSeedRound& r, hipStream_t s);
// the weighted pick from a round's partials and best, one block: *d_total (nullable) = their sum; *d_slot (nullable) = the slot word of
// the smallest i whose running sum of distances exceeds rnd % total, of record 0 at distance 0 when the total is 0
hipError_t vc_launch_seed_pick(const uint32_t* d_partial, const uint64_t* d_best, uint64_t n, uint64_t rnd, uint64_t* d_slot, uint64_t* d_total, hipStream_t s);
// d_stat (two words, zero before = vc_seed_stats in memory): cost += the distances of best, radius = their maximum, n_zero_picks = the
// recorded slot words d_slots[1 .. K - 1] at distance 0 (d_slots nullable: left 0)
hipError_t vc_launch_seed_finish(const uint64_t* d_best, uint64_t n, const uint64_t* d_slots, uint32_t K, uint64_t* d_stat, hipStream_t s);
struct VcSeedArgs {
  const uint64_t* cols;
  uint64_t stride, n;
  uint32_t W, id_base;
  uint32_t n_centres, method;      // checked by the caller: 1 <= n_centres <= n, a known method
  uint64_t seed;
  uint64_t* d_centres;             // [n_centres][W]
  uint64_t* d_picks;               // nullable
  uint64_t* d_assign;              // nullable: then best lives in the handle's scratch
  VcScratchAlloc alloc;   // the handle's grow-only buffers VC_SEED_*
};
// the single engine's whole call on s; stats (host memory, nullable): one wait at the end for 16 bytes, none without
int vc_seed_run(const VcSeedArgs& a, vc_seed_stats* stats, hipStream_t s, std::string* err);
// either handle's host form: `run` (the device form on s) into staged outputs, which come home; waits for them.  picks, assign, stats nullable
struct VcSeedHostArgs {
  uint64_t n;
  uint32_t W, n_centres;
  void* centres;
  uint64_t* picks;
  uint64_t* assign;
  vc_seed_stats* stats;
  VcScratchAlloc alloc;
};
int vc_seed_run_host(const VcSeedHostArgs& a, const std::function<int(uint64_t* d_centres, uint64_t* d_picks, uint64_t* d_assign, vc_seed_stats* stats)>& run,
                     hipStream_t s, std::string* err);
// ---- vc_distinct.hip: one result per label group in k-NN search (vc_search_knn_distinct*, vc_sharded_search_knn_distinct*).  One
// driver for both handle kinds over the view's k-NN search; the plan arithmetic -- the k' schedule, the collapse kernel's
// form for a k', the verdict on a row, the sub-batches -- is vc_distinct_plan.hpp.
struct VcDistinctArgs {
  uint64_t n_labels;               // N, the resident records: d_labels has one word for each, indexed by id - id_base
  uint32_t id_base, W;
  const uint64_t* d_queries;       // [nq][W]
  uint32_t nq, k, k_first;         // checked by the caller: nq > 0, 1 <= k <= VC_MAX_K, vc_distinct_k_first_ok
  const uint32_t* d_labels;
  uint64_t* d_out;                 // [nq][k]
  uint32_t* d_row_labels;          // [nq][k], nullable
  uint32_t* d_counts;              // [nq], nullable
  uint64_t budget;                 // VcKnobs::distinct_scratch: bytes of rows scratch per sub-batch
  bool tie_cut;                    // the search underneath is exact MIH: its rows are sure only below their last distance (vc_distinct_sure_below)
  VcScratchAlloc alloc;   // the handle's grow-only buffers VC_DISTINCT_* (as VcGroupsArgs::alloc)
};
// the whole call on s with the device of the buffers current: one wait per round (24 bytes); stats (host memory) nullable
int vc_distinct_run(const VcDistinctArgs& a, const VcKnnSearch& search, vc_distinct_stats* stats, hipStream_t s, std::string* err);
// either handle's host form: queries and the N labels staged, `run` (the device form on s) into staged outputs, which come home;
// waits for them, then turns the valid part of every row round for VC_ORDER_FARTHEST_FIRST.  row_labels, counts, stats nullable
struct VcDistinctHostArgs {
  uint64_t n_labels;
  uint32_t W, nq, k, order;
  const void* queries;
  const uint32_t* labels;
  uint64_t* out;
  uint32_t* row_labels;
  uint32_t* counts;
  vc_distinct_stats* stats;
  VcScratchAlloc alloc;
};
int vc_distinct_run_host(const VcDistinctHostArgs& a, const std::function<int(const uint64_t* d_queries, const uint32_t* d_labels, uint64_t* d_out,
                                                                            uint32_t* d_row_labels, uint32_t* d_counts, vc_distinct_stats* stats)>& run,
                         hipStream_t s, std::string* err);
// ---- vc_filter.hip: k-NN among the allowed records (vc_search_knn_filtered*, vc_sharded_search_knn_filtered*).  One driver for both
// handle kinds over the view's knn, gather and alloc; the plan arithmetic -- the route, the k' schedule, the verdict on a row, the
// sub-batches, the windows and wave-slices of the subset scan, the cut of a histogram -- is vc_filter_plan.hpp.
struct VcFilterArgs {
  const uint64_t* d_queries;       // [nq][W]
  uint32_t nq, k, k_first;         // checked by the caller: nq > 0, 1 <= k <= VC_MAX_K, vc_distinct_k_first_ok
  const uint32_t* d_sel;           // N words, ceil(N / 32) for VC_FILTER_BITS
  uint32_t kind, value;            // checked by the caller: a known kind
  uint32_t bits;                   // the code width, 64 W
  uint64_t* d_out;                 // [nq][k]
  uint32_t* d_counts;              // [nq], nullable
  uint64_t budget;                 // VcKnobs::filter_scratch
  uint32_t window, route;          // VcKnobs::filter_window, filter_route
  bool tie_cut;                    // the search underneath is exact MIH: its rows are sure only below their last distance (vc_filter_sure_below)
};
// the whole call on s with the device of the buffers current: one wait for A, one per post-filter round; stats (host memory) nullable
int vc_filter_run(const VcStoreView& v, const VcFilterArgs& a, vc_filter_stats* stats, hipStream_t s, std::string* err);
// either handle's host form: queries and sel staged, `run` (the device form on s) into staged outputs, which come home; waits for
// them, then turns the valid part of every row round for VC_ORDER_FARTHEST_FIRST.  counts nullable
struct VcFilterHostArgs {
  uint32_t nq, k, order, kind;
  const void* queries;
  const uint32_t* sel;
  uint64_t* out;
  uint32_t* counts;
};
int vc_filter_run_host(const VcStoreView& v, const VcFilterHostArgs& a,
                       const std::function<int(const uint64_t* d_queries, const uint32_t* d_sel, uint64_t* d_out, uint32_t* d_counts)>& run, hipStream_t s,
                       std::string* err);
// ---- vc_scope.hip: k-NN inside each query's own scope (vc_search_knn_scoped*, vc_sharded_search_knn_scoped*).  One driver for both
// handle kinds over the view's gather and alloc; the plan arithmetic -- key bits, windows, the slice -> query-range rule, the counter
// layout, the sub-batches -- is vc_scope_plan.hpp.
struct VcScopeArgs {
  const uint64_t* d_queries;       // [nq][W]
  uint32_t nq, k;                  // checked by the caller: nq > 0, 1 <= k <= VC_MAX_K
  const uint32_t* d_scope;         // N words
  const uint32_t* d_qscope;        // nq words
  uint32_t bits;                   // the code width, 64 W
  uint64_t* d_out;                 // [nq][k]
  uint32_t* d_counts;              // [nq], nullable
  uint64_t budget;                 // VcKnobs::scope_scratch
  uint32_t window;                 // VcKnobs::scope_window
};
// the whole call on s with the device of the buffers current: one wait for U and A, one for the segment table; stats (host memory) nullable
int vc_scope_run(const VcStoreView& v, const VcScopeArgs& a, vc_scope_stats* stats, hipStream_t s, std::string* err);
// either handle's host form: queries, scope and qscope staged, `run` (the device form on s) into staged outputs, which come home;
// waits for them, then turns the valid part of every row round for VC_ORDER_FARTHEST_FIRST.  counts nullable
struct VcScopeHostArgs {
  uint32_t nq, k, order;
  const void* queries;
  const uint32_t* scope;
  const uint32_t* qscope;
  uint64_t* out;
  uint32_t* counts;
};
int vc_scope_run_host(const VcStoreView& v, const VcScopeHostArgs& a,
                      const std::function<int(const uint64_t* d_queries, const uint32_t* d_scope, const uint32_t* d_qscope, uint64_t* d_out, uint32_t* d_counts)>& run,
                      hipStream_t s, std::string* err);
// ---- vc_knn_graph.hip: the exact k-NN graph of the store (vc_knn_graph*, vc_sharded_knn_graph*) and its analysis (vc_cluster_knn*,
// vc_sharded_cluster_knn*).  One driver for both handle kinds over the view's gather, knn and alloc; the plan arithmetic -- the range,
// the k' schedule, the verdict on a row, the sub-batches, the scratch layout -- is vc_knn_graph_plan.hpp.
struct VcKgraphArgs {
  uint32_t k, k_first, batch;      // checked by the caller: vc_kgraph_k_ok, vc_kgraph_k_first_ok; batch as the caller passed it
  bool linear;                     // the mode is VC_MODE_LINEAR: one round at k + 1; else the view's knn is exact MIH
  uint64_t first, rows;            // the positions [first, first + rows) of the store, rows > 0 (vc_kgraph_range)
  uint64_t* d_rows;                // [rows][k]
  uint32_t* d_counts;              // [rows], nullable
  uint64_t budget;                 // VcKnobs::kgraph_scratch
  const uint32_t* d_id_list = nullptr;   // [rows] ascending global ids, device memory: the records to answer in place of the range (first is
                                   // then ignored), and d_rows / d_counts are those of the WHOLE store: record id's row goes to row id - id_base
};
// the whole call on s with the device of the buffers current: under exact MIH one wait per round of a batch (4 bytes), one at the end
// for the statistics when stats (host memory, nullable) is given.  linear_knn: the store's LINEAR k-NN, which answers the queries
// exact MIH leaves unsettled at k' = VC_MAX_K (in LINEAR mode the view's own)
int vc_knn_graph_run(const VcStoreView& v, const VcKnnSearch& linear_knn, const VcKgraphArgs& a, vc_knn_graph_stats* stats, hipStream_t s, std::string* err);
// either handle's host form (a's pointers are ignored): `run` (the device form on s) into staged rows and counts, which come home;
// waits for them.  A row the linear scan passed on (count UINT32_MAX) is answered again by host_knn -- the handle's host-form LINEAR
// k-NN of nq codes at k + 1, ascending -- and stripped by vc_ids_strip_host.  counts, stats nullable
int vc_knn_graph_run_host(const VcStoreView& v, const VcKgraphArgs& a, uint64_t* rows, uint32_t* counts, vc_knn_graph_stats* stats,
                          const std::function<int(uint64_t* d_rows, uint32_t* d_counts, vc_knn_graph_stats* stats)>& run,
                          const std::function<int(const uint64_t* codes, uint32_t nq, uint64_t* rows, uint32_t* counts)>& host_knn, hipStream_t s,
                          std::string* err);
// the second answer of vc_knn_graph_run_host alone: rows [a.rows][k] and cnt [a.rows] are the range's outputs in host memory
int vc_knn_graph_answer_again_host(const VcStoreView& v, const VcKgraphArgs& a, uint64_t* rows, uint32_t* cnt,
                                   const std::function<int(const uint64_t* codes, uint32_t nq, uint64_t* rows, uint32_t* counts)>& host_knn, hipStream_t s,
                                   std::string* err);
// ---- vc_knn_graph_update.hip: a built graph after vc_add_codes (vc_knn_graph_update*, vc_sharded_knn_graph_update*).  One driver for
// both handle kinds; the plan arithmetic -- the join kernel's map and tile, the window rule, the sub-batches, the scratch layout -- is
// vc_knn_graph_update_plan.hpp.
struct VcKgupdArgs {
  VcKgraphArgs build;              // of the new records' rows: first = n_old, rows = N - n_old > 0, its pointers those of row n_old
  uint64_t n_old;                  // checked by the caller: n_old < N
  uint64_t* d_rows;                // [N][k]: the first n_old rows are the graph as it was
  uint32_t* d_counts;              // [N], nullable
  uint64_t budget;                 // VcKnobs::kgraph_scratch: the hit list of a window, the out-of-place rows of a merge launch
  uint32_t old_batch, window;      // vc_kgupd_old_batch(VcKnobs::kgraph_old_batch), vc_kgupd_window(VcKnobs::kgraph_window)
};
// the whole call on s with the device of the buffers current: vc_knn_graph_run's waits for the new rows, one wait of 16 bytes per
// count pass of a window, one at the end for the statistics and the error word (VC_ERR_INVALID: an old count above k)
int vc_knn_graph_update_run(const VcStoreView& v, const VcKnnSearch& linear_knn, const VcKgupdArgs& a, vc_knn_graph_update_stats* stats, hipStream_t s,
                            std::string* err);
// either handle's host form (a's pointers are ignored): the old rows and counts staged up, `run` (the device form on s, which sets
// the pointers) on them, all N rows and counts home; waits for them.  host_knn as vc_knn_graph_run_host's.  counts, stats nullable
int vc_knn_graph_update_run_host(const VcStoreView& v, const VcKgupdArgs& a, uint64_t* rows, uint32_t* counts, vc_knn_graph_update_stats* stats,
                                 const std::function<int(uint64_t* d_rows, uint32_t* d_counts, vc_knn_graph_update_stats* stats)>& run,
                                 const std::function<int(const uint64_t* codes, uint32_t nq, uint64_t* rows, uint32_t* counts)>& host_knn, hipStream_t s,
                                 std::string* err);
// ---- vc_knn_graph_retain.hip: a built graph after vc_retain* (vc_knn_graph_retain*, vc_sharded_knn_graph_retain*).  One driver for both
// handle kinds; the plan arithmetic -- the lane map, the chunks, the short rule, the scratch layout -- is vc_knn_graph_retain_plan.hpp.
struct VcKgretArgs {
  VcKgraphArgs repair;             // of the short rows' searches: its pointers those of the WHOLE buffers [n_old][k] / [n_old] (counts nullable);
                                   // first, rows and d_id_list are set by the driver
  uint64_t n_old;                  // checked by the caller: 0 < K = v.n < n_old
  const uint32_t* d_new_ids;       // [n_old]: vc_retain*'s map
};
// the whole call on s with the device of the buffers current: one wait of 32 bytes for the short list's length, the error word
// (VC_ERR_INVALID) and the tallies, then vc_knn_graph_run's waits over the short list
int vc_knn_graph_retain_run(const VcStoreView& v, const VcKnnSearch& linear_knn, const VcKgretArgs& a, vc_knn_graph_retain_stats* stats, hipStream_t s,
                            std::string* err);
// either handle's host form (a's pointers are ignored): the old rows, counts and map staged up, `run` (the device form on s, which
// sets the pointers) on them, the K rows and counts home; waits for them.  host_knn as vc_knn_graph_run_host's.  counts, stats nullable
int vc_knn_graph_retain_run_host(const VcStoreView& v, const VcKgretArgs& a, const uint32_t* new_ids, uint64_t* rows, uint32_t* counts,
                                 vc_knn_graph_retain_stats* stats,
                                 const std::function<int(const uint32_t* d_new_ids, uint64_t* d_rows, uint32_t* d_counts, vc_knn_graph_retain_stats* stats)>& run,
                                 const std::function<int(const uint64_t* codes, uint32_t nq, uint64_t* rows, uint32_t* counts)>& host_knn, hipStream_t s,
                                 std::string* err);
struct VcKgraphClusterArgs {
  const uint64_t* d_rows;          // [n][k]: vc_knn_graph*'s rows over the whole store
  const uint32_t* d_counts;        // [n], nullable: then every row holds vc_kgraph_row_count(n, k) entries
  uint32_t k, kk, flags, max_dist; // checked by the caller: vc_kgraph_k_ok, 1 <= kk <= k, known flags
  uint32_t* d_labels;              // [n]
  uint32_t* d_in_degree;           // [n], nullable: then the handle's own (VC_KGRAPH_DEG)
};
// the whole call on s, v.n > 0: init, the edge launch, flatten, the largest in-degree, then the one wait for the statistics and the
// error word (VC_ERR_INVALID: a count above k or an id outside the store).  Only n, id_base and alloc of the view are used
int vc_cluster_knn_run(const VcStoreView& v, const VcKgraphClusterArgs& a, vc_cluster_knn_stats* stats, hipStream_t s, std::string* err);
// the same for host pointers (a's pointers are ignored): rows and counts staged, labels and in-degrees (nullable) come home, waited for
int vc_cluster_knn_run_host(const VcStoreView& v, VcKgraphClusterArgs a, const uint64_t* rows, const uint32_t* counts, uint32_t* labels, uint32_t* in_degree,
                            vc_cluster_knn_stats* stats, hipStream_t s, std::string* err);
// ---- vc_snn.hip: shared-nearest-neighbour clusters of a built graph (vc_cluster_snn*, vc_sharded_cluster_snn*).  One driver for both
// handle kinds; the plan arithmetic -- the argument checks, the set's size, the team shapes, the staging layout -- is vc_snn_plan.hpp.
struct VcSnnArgs {
  const uint64_t* d_rows;          // [n][k]: vc_knn_graph*'s rows over the whole store
  const uint32_t* d_counts;        // [n], nullable: then every row holds vc_kgraph_row_count(n, k) entries
  uint32_t k, kk, flags, max_dist; // checked by the caller: vc_kgraph_k_ok, vc_snn_kk_ok, vc_snn_flags_ok
  uint32_t min_shared;
  uint32_t* d_labels;              // [n]
  uint32_t* d_shared;              // [n][kk], nullable
  uint64_t* d_hist;                // [kk], nullable
};
// the whole call on s, v.n > 0: the memsets, init, the intersection launch, flatten, then the one wait for the statistics and the
// error word (VC_ERR_INVALID: a count above k, an id outside the store, a row's own id).  Only n, id_base and alloc of the view are used
int vc_cluster_snn_run(const VcStoreView& v, const VcSnnArgs& a, vc_cluster_snn_stats* stats, hipStream_t s, std::string* err);
// the same for host pointers (a's pointers are ignored): rows and counts staged; labels, weights and histogram (both nullable) come home, waited for
int vc_cluster_snn_run_host(const VcStoreView& v, VcSnnArgs a, const uint64_t* rows, const uint32_t* counts, uint32_t* labels, uint32_t* shared, uint64_t* hist,
                            vc_cluster_snn_stats* stats, hipStream_t s, std::string* err);
// ---- vc_knn_adjacency.hip: the reverse, mutual and symmetrised graph in CSR form (vc_knn_adjacency*, vc_sharded_knn_adjacency*).  One
// driver for both handle kinds; the plan arithmetic -- the argument checks, the passes, the scratch, the teams -- is vc_knn_adjacency_plan.hpp.
struct VcAdjArgs {
  const uint64_t* d_rows;          // [n][k]: vc_knn_graph*'s rows over the whole store
  const uint32_t* d_counts;        // [n], nullable: then every row holds vc_kgraph_row_count(n, k) entries
  uint32_t k, kk, flags, max_dist; // checked by the caller: vc_kgraph_k_ok, vc_adj_kk_ok, vc_adj_flags_ok, vc_adj_items_ok
  uint64_t* d_adj;                 // [adj_cap], null when adj_cap == 0
  uint64_t adj_cap;
  uint64_t* d_offsets;             // [n + 1]
};
// the whole call on s: every buffer grown, the enumerate (or mutual count) launch, the scans, the one wait for the statistics and the
// error word (VC_ERR_INVALID: a count above k, an id outside the store, a row's own id -- no output word written), the offsets,
// VC_ERR_CAPACITY where T > adj_cap (d_adj untouched), then the sort and the fill.  n == 0: offsets[0] = 0.  Only n, id_base, W and
// alloc of the view are used
int vc_knn_adjacency_run(const VcStoreView& v, const VcAdjArgs& a, vc_knn_adjacency_stats* stats, hipStream_t s, std::string* err);
// the same for host pointers (a's pointers are ignored): rows and counts staged; the offsets come home also on VC_ERR_CAPACITY, the
// T words of adj on VC_OK; waited for
int vc_knn_adjacency_run_host(const VcStoreView& v, VcAdjArgs a, const uint64_t* rows, const uint32_t* counts, uint64_t* adj, uint64_t* offsets,
                              vc_knn_adjacency_stats* stats, hipStream_t s, std::string* err);
// ---- vc_knn_mst.hip: the minimum spanning forest of a built graph in Kruskal order (vc_knn_mst*, vc_sharded_knn_mst*) and the cut of
// an edge list (vc_mst_cut*, vc_sharded_mst_cut*).  One driver for both handle kinds; the plan arithmetic -- the argument checks, the
// key, the home rule, the sizes, the round bound -- is vc_knn_mst_plan.hpp.
struct VcMstArgs {
  const uint64_t* d_rows;          // [n][k]: vc_knn_graph*'s rows over the whole store
  const uint32_t* d_counts;        // [n], nullable: then every row holds vc_kgraph_row_count(n, k) entries
  uint32_t k, kk, flags, max_dist; // checked by the caller: vc_kgraph_k_ok, vc_mst_kk_ok, vc_mst_flags_ok, vc_mst_items_ok
  uint32_t weight_kind, min_pts;   // vc_mst_kind_ok, vc_mst_min_pts_ok
  vc_mst_edge* d_edges;            // [max(n, 1) - 1]
  uint32_t* d_labels;              // [n], nullable
  uint64_t* d_hist;                // [bits + 1], nullable
};
// the whole call on s: init, the enumeration, the rounds (one wait each; the first brings the error word: VC_ERR_INVALID for a count
// above k, an id outside the store, a row's own id), the sort, the outputs, the last wait.  n == 0: the histogram zeroed.  Only n,
// id_base, W and alloc of the view are used
int vc_knn_mst_run(const VcStoreView& v, const VcMstArgs& a, vc_knn_mst_stats* stats, hipStream_t s, std::string* err);
// the same for host pointers (a's pointers are ignored): rows and counts staged; the M edges, the labels and the histogram (both
// nullable) come home, waited for
int vc_knn_mst_run_host(const VcStoreView& v, VcMstArgs a, const uint64_t* rows, const uint32_t* counts, vc_mst_edge* edges, uint32_t* labels, uint64_t* hist,
                        vc_knn_mst_stats* stats, hipStream_t s, std::string* err);
// the components under the edges of weight <= max_weight: init, one launch over the edges, flatten, one wait (VC_ERR_INVALID: an end
// outside the store).  n_clusters: host memory, nullable
int vc_mst_cut_run(const VcStoreView& v, const vc_mst_edge* d_edges, uint64_t n_edges, uint32_t max_weight, uint32_t* d_labels, uint64_t* n_clusters, hipStream_t s,
                   std::string* err);
int vc_mst_cut_run_host(const VcStoreView& v, const vc_mst_edge* edges, uint64_t n_edges, uint32_t max_weight, uint32_t* labels, uint64_t* n_clusters, hipStream_t s,
                        std::string* err);
// ---- vc_mst_condense.hip: the condensed tree of a spanning forest, its stabilities, the selection and the flat labels
// (vc_mst_condense*, vc_sharded_mst_condense*).  One driver for both handle kinds; the plan arithmetic -- the argument checks, the level
// table, the stability, the sizes -- is vc_mst_condense_plan.hpp.
struct VcCondenseArgs {
  const vc_mst_edge* d_edges;      // [n_edges]: a forest over the store, ascending in weight
  uint64_t n_edges;                // checked by the caller: vc_cond_edges_ok
  uint32_t min_cluster_size, root_weight, method;   // vc_cond_mcs_ok, vc_cond_root_weight_ok, vc_cond_method_ok
  vc_condensed_node* d_nodes;      // [max(n, 1) - 1]
  uint32_t* d_labels;              // [n]
  uint32_t* d_node;                // [n], nullable
  uint32_t* d_own;                 // [n], nullable
  uint32_t* d_leave;               // [n], nullable
};
// the whole call on s: the plan (THE FIRST WAIT: VC_ERR_INVALID for an edge or a root weight the contract refuses), the levels without
// a wait, the roots (the second wait: the node count; VC_ERR_INVALID for a cycle), the sort, the fold, the selection, the labels, the
// last wait.  No output word is written before the second wait.  Only n, id_base, W and alloc of the view are used
int vc_mst_condense_run(const VcStoreView& v, const VcCondenseArgs& a, vc_mst_condense_stats* stats, hipStream_t s, std::string* err);
// the same for host pointers (a's pointers are ignored): the edges staged; the n_nodes nodes, the labels and the three nullable
// arrays come home, waited for
int vc_mst_condense_run_host(const VcStoreView& v, VcCondenseArgs a, const vc_mst_edge* edges, vc_condensed_node* nodes, uint32_t* labels, uint32_t* node, uint32_t* own,
                             uint32_t* leave, vc_mst_condense_stats* stats, hipStream_t s, std::string* err);
// ---- vc_vote.hip: the weighted label tally of a segment -- the k-NN classifier over any rows (vc_knn_vote*, vc_sharded_knn_vote*) and
// synchronous label propagation over a CSR graph (vc_label_propagate*, vc_sharded_label_propagate*).  One driver per call for both
// handle kinds; the plan arithmetic -- the argument checks, the weight, the key, the team shapes, the sizes -- is vc_vote_plan.hpp.
struct VcVoteArgs {
  const uint64_t* d_rows;            // [n_rows][k]: any rows whose ids are resident
  const uint32_t* d_counts;          // [n_rows], nullable: then every row holds vc_vote_row_count(n, k) entries
  uint64_t n_rows;
  uint32_t k, kk, max_dist;          // checked by the caller: vc_vote_k_ok, vc_vote_kk_ok
  const uint32_t* d_labels;          // [n]
  uint32_t weight_kind;              // vc_vote_kind_ok
  uint32_t* d_out_label;             // [n_rows]
  uint32_t* d_out_votes;             // [n_rows], nullable
  uint32_t* d_out_total;             // [n_rows], nullable
};
// the whole call on s: one tally launch shaped by kk, ONE wait (the counters and the error word: VC_ERR_INVALID for a count above k, an
// id outside the store, a voting entry beyond the code width under CLOSENESS).  Only n, id_base, W and alloc of the view are used
int vc_knn_vote_run(const VcStoreView& v, const VcVoteArgs& a, vc_knn_vote_stats* stats, hipStream_t s, std::string* err);
// the same for host pointers (a's pointers are ignored): rows, counts and labels staged; the outputs (votes and total nullable) come
// home, waited for
int vc_knn_vote_run_host(const VcStoreView& v, VcVoteArgs a, const uint64_t* rows, const uint32_t* counts, const uint32_t* labels, uint32_t* out_label,
                         uint32_t* out_votes, uint32_t* out_total, vc_knn_vote_stats* stats, hipStream_t s, std::string* err);
struct VcLabelPropagateArgs {
  const uint64_t* d_offsets;         // [n + 1]
  const uint64_t* d_adj;             // [n_entries]
  uint64_t n_entries;
  const uint32_t* d_labels_in;       // [n]
  uint32_t weight_kind, flags, max_iters;   // checked by the caller: vc_vote_kind_ok, vc_vote_lp_flags_ok, vc_vote_iters_ok
  uint32_t* d_labels_out;            // [n]
  uint32_t* d_votes;                 // [n], nullable
  uint32_t* d_total;                 // [n], nullable
};
// the whole call on s: the plan (checks, bins, long tables; one wait, VC_ERR_INVALID before any output word is written), then the
// rounds, one read-back each; the copy into d_labels_out is enqueued behind the last one
int vc_label_propagate_run(const VcStoreView& v, const VcLabelPropagateArgs& a, vc_label_propagate_stats* stats, hipStream_t s, std::string* err);
// the same for host pointers (a's pointers are ignored): offsets, adj and labels_in staged; labels_out, votes and totals (both
// nullable) come home, waited for
int vc_label_propagate_run_host(const VcStoreView& v, VcLabelPropagateArgs a, const uint64_t* offsets, const uint64_t* adj, const uint32_t* labels_in,
                                uint32_t* labels_out, uint32_t* votes, uint32_t* totals, vc_label_propagate_stats* stats, hipStream_t s, std::string* err);
// ---- vc_retain.hip: removal of records (vc_retain*).  The keep set is VcKeepSet (vc_retain.hpp); nothing here waits.
struct VcKeepSet;
#define VC_RETAIN_FROM 2u   // internal kind: the records from `first_kept` on survive, sel is not read (a shard giving away a prefix of its records)
// sel -> d_bits (vc_keep_blocks(n) * 4 words) and d_rank (vc_keep_blocks(n) + 1 words, the last one = K); d_work: vc_scan_work_words(blocks + 1) words
hipError_t vc_launch_keep_bits(const uint32_t* d_sel, uint32_t kind, uint32_t id_base, uint64_t first_kept, uint64_t n, uint64_t* d_bits, uint32_t* d_rank,
                               uint32_t* d_work, uint32_t n_cu, hipStream_t s);
// d_new_ids[i] = id_base + new local id of record i, or UINT32_MAX for a removed one
hipError_t vc_launch_keep_map(const VcKeepSet& ks, uint32_t id_base, uint32_t* d_new_ids, uint32_t n_cu, hipStream_t s);
// one column compacted through d_scratch (round_up(n, 2) words): survivors in order at [0, K), zeros at [K, round_up(n, 2))
hipError_t vc_launch_keep_compact_column(const VcKeepSet& ks, uint64_t* d_col, uint64_t* d_scratch, uint32_t n_cu, hipStream_t s);
// ---- vc_engine.hip: what the sharded store's global stop (vc_sharded.hip) needs of a shard's engine
struct VcEngineView {
  const uint64_t* cols;   // column-major codes, word j of record i at cols[j * stride + i]
  uint64_t stride, n;
  uint32_t W, m, sbits, id_base, n_cu, reach;   // reach: vc_mih_knn_reach of the index (0 without one)
};
int vc_engine_view(vc_engine* e, VcEngineView* v);
int vc_engine_has_index(vc_engine* e);   // 1: an MIH index that covers every resident record
// MIH k-NN (mode: VC_MODE_MIH_EXACT or VC_MODE_MIH_APPROX) capped at shell r_cap (vc_mih_search's r_cap) on stream s: shells 0..r_cap
// with the mode's own stop rule active; a query still open at r_cap ends with radius = r_cap and the k best of what it has seen.
// d_stats as vc_search_knn_dev_stats
int vc_engine_knn_capped(vc_engine* e, const void* d_queries, uint32_t nq, uint32_t k, uint32_t mode, uint32_t r_cap, uint64_t* d_out,
                         uint32_t* d_counts, vc_query_stats* d_stats, hipStream_t s);
// vc_search_radius_dev on stream s with the shard's total returned to the host: *total = entries found, also when they exceed
// out_cap (VC_ERR_CAPACITY: the caller grows its buffer to *total and repeats, no read-back of the offsets)
int vc_engine_radius_dev(vc_engine* e, const void* d_queries, uint32_t nq, uint32_t radius, uint32_t mode, uint64_t* d_out, uint64_t out_cap,
                         uint64_t* d_offsets, uint64_t* total, hipStream_t s);
// what vc_sharded_retain* needs of a shard (vc_engine.hip), both on stream s and waited for: the records from local position
// first_kept on survive (vc_retain's column and index phases with the internal kind VC_RETAIN_FROM); and `count` records of `src`
// from its local position `first` on appended behind e's own (device or peer copies; e's index, if any, is stale afterwards)
int vc_engine_retain_from(vc_engine* e, uint64_t first_kept, hipStream_t s);
int vc_engine_append_from(vc_engine* e, vc_engine* src, uint64_t first, uint64_t count, hipStream_t s);
// the same over the gathered shard slots of vc_sharded_* (rows + counts per slot; a flagged shard row flags the merged row)
hipError_t vc_launch_select_slots(const uint64_t* d_base, uint64_t slot_words, uint32_t cnt_off_words, uint32_t n_lists, uint32_t nq,
                                  uint32_t k, uint64_t* d_out, uint32_t* d_out_count, hipStream_t s);
