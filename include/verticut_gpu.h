/* ============================================================================
 * verticut_gpu.h -- C ABI of the MI355X (gfx950) Hamming k-NN engine.
 *
 * Drop-in boundary for VertiCut's search hot path.  Every entry point names the reference
 * interface it replaces (paths relative to the reference tree).  Plain pointers and sizes
 * only: no C++ types, no torch types, no exceptions, no globals; one engine handle is
 * thread-compatible (one caller at a time, like SearchWorker, search_worker.h:35-50).
 *
 * Data model (reference semantics kept):
 *   code      B/8 raw bytes, B in {64,128,256,512}  (N_BINARY_BITS image_search_constants.h:10)
 *   id        uint32 = ordinal of the record in insertion order (+ id_base of the shard)
 *             (build_hash_tables.cc:55,61,69; image_search.proto:4,17)
 *   result    uint64 = id | (uint64)dist << 32      (search_worker.cc:12-13,254-256)
 *   table t   substring t = bytes [t*B/8/m, (t+1)*B/8/m) of the code, key = little-endian
 *             value (Pilaf/image_tools.h:12-18), one table per former MPI rank
 *             (search_worker.cc:99-101, build_hash_tables.cc:26,36-38)
 *
 * All functions return VC_OK (0) or a negative VC_ERR_* code; vc_last_error() gives text.
 * There is no CPU fallback anywhere behind this ABI: without a usable gfx950 device
 * vc_create fails with VC_ERR_NO_DEVICE.
 * ==========================================================================*/
#ifndef VERTICUT_GPU_H
#define VERTICUT_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VC_ABI_VERSION 2

/* ---- status codes (BaseProxy uses 0 = found/done, 1 = not found/fail: base_proxy.h:10-13) */
#define VC_OK 0
#define VC_NOT_FOUND 1          /* == PROXY_NOT_FOUND, only from vc_get_bucket / vc_get_code */
#define VC_ERR_INVALID (-1)     /* bad argument / configuration (reference: assert, search_worker.cc:75) */
#define VC_ERR_NO_DEVICE (-2)   /* no gfx950 device / HIP runtime failure at create */
#define VC_ERR_HIP (-3)         /* HIP call failed (text in vc_last_error) */
#define VC_ERR_NOMEM (-4)       /* device allocation failed */
#define VC_ERR_STATE (-5)       /* call order: e.g. MIH search before vc_build_index */
#define VC_ERR_CAPACITY (-6)    /* more codes than vc_config.capacity, or output buffer too small */

/* ---- search modes (which reference loop the call reproduces) */
#define VC_MODE_LINEAR 0      /* linear_search.cc:39-64  full scan + top-k            */
#define VC_MODE_MIH_EXACT 1   /* search_worker.cc:159-218 search_K_nearest_neighbors   */
#define VC_MODE_MIH_APPROX 2  /* search_worker.cc:93-157  ..._approximate_... (factor 20, search_worker.h:14) */

/* ---- vc_config.flags */
#define VC_FLAG_USE_BITMAP 0x1u        /* attach the bucket-occupancy bitmap (search_worker.cc:238-243);
                                          off = as shipped (:61-62), n_local_reads stays 0 */
#define VC_FLAG_REF_SIGNEXT_KEYS 0x2u  /* reproduce binaryToInt's sign-extended keys for substrings < 32 bit
                                          (Pilaf/image_tools.h:13): probes that flip the substring's top bit
                                          can never match, exactly as in the reference.  Off = masked keys
                                          (exact MIH for every substring width). */
#define VC_FLAG_REF_STOP_LITERAL4 0x4u /* stop rule "kth <= 4*radius" with the literal 4 (search_worker.cc:204)
                                          even when n_tables < 4.  Default: min(n_tables,4), identical to the
                                          reference whenever the reference itself is exact. */

#define VC_FLAG_LEAN_TIMING 0x8u       /* time only the verify-kernel launches (vc_timing.scan_*): no event pair around each
                                          search call, so vc_timing.total_ms / calls stay 0.  Each event record is a barrier
                                          packet in the stream (~4 us); a throughput loop that keeps its own clock sets this. */
#define VC_FLAG_GLOBAL_STOP 0x10u      /* sharded store (vc_sharded_config.engine.flags), VC_MODE_MIH_EXACT: the stop rule is decided on
                                          the MERGED rows, as the reference's master does (search_worker.cc:179-207), so rows, counts
                                          and statistics are those of one vc_engine holding the union.  A plain vc_engine ignores it
                                          (its stop is global already).  Refused (VC_ERR_INVALID) with
                                          n_tables == 0, VC_FLAG_USE_BITMAP, VC_FLAG_REF_SIGNEXT_KEYS, or VC_FLAG_REF_STOP_LITERAL4
                                          with n_tables < 4. */
#define VC_FLAG_GLOBAL_APPROX 0x20u    /* sharded store (vc_sharded_config.engine.flags), VC_MODE_MIH_APPROX: the loop stops where ONE
                                          engine over the union stops, as the reference's master does when it fills one heap of
                                          knn * APPROXIMATE_FACTOR distinct candidates from all ranks and broadcasts is_stop
                                          (search_worker.cc:104-139): after the first shell r* in which the distinct candidates of ALL
                                          shards together, shells 0..r*, reach 20 k -- else after the last shell.  Rows are the k
                                          smallest (dist, id) among the union's items whose minimum substring distance is <= r*,
                                          radius = r*, n_sub_reads = table 0's gets of shells 0..r*, n_candidates = the shards'
                                          distinct counts summed (the shards are id-disjoint): what one vc_engine holding the union
                                          returns.  Independent of VC_FLAG_GLOBAL_STOP (either or both may be set); MIH_EXACT, LINEAR
                                          and the radius searches do not look at it.  A plain vc_engine ignores it.  Refused
                                          (VC_ERR_INVALID) with n_tables == 0 or VC_FLAG_USE_BITMAP (the gets issued then depend on the
                                          union's bitmap); VC_FLAG_REF_SIGNEXT_KEYS and VC_FLAG_REF_STOP_LITERAL4 are allowed. */

/* ---- synthetic data kinds for vc_add_synthetic (the reference ships no data: .gitignore:7-8) */
#define VC_SYNTH_UNIFORM 0
#define VC_SYNTH_CLUSTERED 1

/* ---- streams: every `stream` argument is a hipStream_t; NULL is the HIP null (legacy default) stream -- what
 * PyTorch-ROCm's default stream is -- and VC_STREAM_OWN names the engine's private non-blocking stream, on which
 * the host-pointer calls run unless vc_set_stream says otherwise. */
#define VC_STREAM_OWN ((void*)(intptr_t)-1)

/* ---- output order for k-NN results */
#define VC_ORDER_ASCENDING 0       /* canonical: ascending packed (dist, id) */
#define VC_ORDER_FARTHEST_FIRST 1  /* as SearchWorker::find / linear_search print (search_worker.cc:210-216) */

typedef struct vc_engine vc_engine;

typedef struct vc_config {
  uint32_t abi_version;  /* VC_ABI_VERSION */
  uint32_t bits;         /* code width B: 64, 128, 256 or 512            (args_config.cc binary_bits) */
  uint32_t n_tables;     /* m, substring = B/m bits, 8..32, multiple of 8 (args_config.cc n_tables);
                            0 = linear-only engine */
  uint32_t flags;        /* VC_FLAG_* */
  uint64_t capacity;     /* max number of codes this engine (shard) will hold (image_total) */
  uint32_t id_base;      /* global id of local record 0 (shard offset; ids stay < 2^32) */
  int32_t device;        /* HIP device ordinal, -1 = current */
  uint32_t cand_cap;     /* per-query candidate ring entries, 0 = default (65536) */
  uint32_t scan_blocks;  /* 0 = default grid for the verify kernel (tuning knob) */
  uint32_t query_tile;   /* queries verified per DB pass; 0 = the engine chooses: 32 for databases of 256 MB and more, doubling
                            per halving below (at most 512: a small database's pass is priced by its launches, not its bytes).
                            8 = HBM-bound pass, see DESIGN.md 4.1 */
  uint32_t timing_sample;/* with VC_FLAG_LEAN_TIMING: time only every N-th verify launch (0/1 = every launch) */
  uint32_t reserved[4];
} vc_config;

/* Per-query statistics == SearchWorker::get_stat (search_worker.cc:24-30, search_worker.h:42-45). */
typedef struct vc_query_stats {
  uint32_t radius;        /* last substring shell searched (find's return value radius-1) */
  uint32_t n_results;     /* results written for this query (<= k) */
  uint64_t n_main_reads;  /* always 0 (never incremented in the reference) */
  uint64_t n_sub_reads;   /* bucket gets issued by table 0 (what rank 0's get_stat reports) */
  uint64_t n_local_reads; /* bitmap tests by table 0 (0 unless VC_FLAG_USE_BITMAP) */
  uint64_t n_candidates;  /* distinct DB items verified (owner-rule deduplicated) */
} vc_query_stats;

/* Device-side timing of every search call since the previous vc_get_timing(), measured with HIP events
 * recorded on the stream the kernels were launched on. */
typedef struct vc_timing {
  float total_ms;          /* sum over calls of the whole call's device span */
  float scan_ms;           /* sum over launches of the dominant verify kernel (vc_scan_kernel) */
  uint32_t scan_launches;
  uint32_t calls;
  uint64_t scan_bytes;     /* algorithmic bytes those launches read: N * B/8 per launch over the store's columns; per launch
                              over the scan stream (vc_build_scan_stream) the bytes THAT launch streams, padded records * 12
                              + granule headers * 8 */
  /* ABI 2 -- the MIH query kernel (mih_query_kernel: probe + verify + merge of the shells of a batch in one launch) */
  float mih_ms;            /* sum over its launches */
  uint32_t mih_launches;
  uint64_t mih_queries;    /* queries those launches served */
  uint64_t mih_probes;     /* bucket probes = keys enumerated (search_worker.cc:230-264 leaves), all tables */
  uint64_t mih_hits;       /* non-empty buckets looked up (PROXY_FOUND gets, search_worker.cc:246) */
  uint64_t mih_entries;    /* bucket entries verified (search_worker.cc:249-257) */
} vc_timing;

/* ---- lifetime ----------------------------------------------------------------------------
 * replaces: SearchWorker ctor (search_worker.cc:50-63) + BaseProxy::init/close (base_proxy.h:24-28) */
int vc_create(const vc_config* cfg, vc_engine** out);
int vc_destroy(vc_engine* e);
const char* vc_last_error(const vc_engine* e); /* never NULL; e may be NULL for create failures */
const char* vc_strerror(int code);
int vc_abi_version(void);

/* ---- ingest ------------------------------------------------------------------------------
 * replaces: build_hash_tables.cc:40-70 (records appended in file order, id = ordinal) and the
 * ID -> BinaryCode put path used by linear_search.cc:45-46.  `codes` = n * bits/8 raw bytes (host). */
int vc_add_codes(vc_engine* e, const void* codes, uint64_t n);
/* Same, generated on the device: item with global id g gets the code of the shared definition
 * (oracle/vc_oracle.cc gen_one) -- used by bench/tests for the BASELINE.json shapes. */
int vc_add_synthetic(vc_engine* e, uint64_t n, uint64_t seed, uint32_t kind, uint32_t n_centres, uint32_t max_flips);
int vc_size(const vc_engine* e, uint64_t* n);
/* The reference's on-disk inputs, honoured as they are:
 *   code file   headerless records of bits/8 bytes, id = ordinal  (build_hash_tables.cc:40-70, BINARY_CODE_FILE)
 *   bitmap file raw 2^substr_bits-bit LSB-first uint32 words of one table (generate_bitmap.cc:99-125,
 *               read back by bitmap_deamon.cc:41-65)
 * vc_load_code_file appends up to max_records records (0 = all) and reports how many were read;
 * vc_save_code_file writes the resident records back in id order; vc_write_bitmap_file needs vc_build_index. */
int vc_load_code_file(vc_engine* e, const char* path, uint64_t max_records, uint64_t* n_read);
int vc_save_code_file(vc_engine* e, const char* path);
int vc_write_bitmap_file(vc_engine* e, uint32_t table, const char* path);
/* Reads a bitmap file of that format (what bitmap_deamon.cc:41-65 loads) and checks it word for word against the
 * bitmap of the resident index: VC_OK = identical (the file belongs to this database), VC_ERR_STATE = it differs
 * (*n_mismatch_words, may be NULL, says in how many 32-bit words), VC_ERR_INVALID = wrong size / unreadable. */
int vc_read_bitmap_file(vc_engine* e, uint32_t table, const char* path, uint64_t* n_mismatch_words);
/* Index persistence (the step build_hash_tables.cc performs against the KV tier, kept on disk instead): the sorted id
 * runs, bucket offsets, occupancy bitmaps and rank directories of every table.  vc_load_index needs the same records
 * resident (vc_load_code_file / vc_add_codes) and refuses a file built for another shape (VC_ERR_STATE). */
int vc_save_index(vc_engine* e, const char* path);
int vc_load_index(vc_engine* e, const char* path);
/* ID -> BinaryCode get (linear_search.cc:45-46; by-id query path image_search_client.h:23-25).
 * id is a global id; out = bits/8 bytes.  VC_NOT_FOUND if id is not in this shard. */
int vc_get_code(vc_engine* e, uint32_t id, void* out);

/* ---- index -------------------------------------------------------------------------------
 * replaces: build_hash_tables.cc (bucket contents, rule a12) + generate_bitmap.cc:105-114
 * (bit v of table t set iff bucket (t,v) non-empty).  Must follow the last vc_add_* (or be brought up to
 * date by vc_update_index). */
int vc_build_index(vc_engine* e);
/* Brings the MIH index up to date with the records appended since it was built, loaded or last updated
 * (build_hash_tables.cc:40-70: get bucket, append, put).  The result is BIT FOR BIT the index
 * vc_build_index would build from all resident records.  No index yet -> behaves as vc_build_index;
 * index already current -> VC_OK, nothing done.
 * Appended ids exceed every indexed id, so each new entry goes to the END of its key's bucket: per table the
 * new (key, id) pairs are sorted and merged into the table in one streaming pass; no indexed entry is sorted
 * again.  vc_add_codes / vc_add_synthetic / vc_load_code_file therefore KEEP an existing index and mark it
 * stale: until the next vc_update_index / vc_build_index / vc_load_index every call that needs an index
 * returns VC_ERR_STATE exactly as if there were none -- only its device memory stays allocated.
 * If an update fails, the handle is left with that stale index or with none; vc_build_index works after either. */
int vc_update_index(vc_engine* e);

/* ---- scan stream: a second, derived layout of a 128-bit store for linear k-NN passes of 1..8 queries -----------------
 * The records sorted by their KEY -- the low 32 bits of code word 0, i.e. bytes 0..3 of a record -- as four uint32
 * columns, a position -> local id table and one {prefix, mask} header per 256 sorted records (the leading key bits they
 * share).  A linear pass of vc_search_knn / vc_search_knn_dev(_stats) with at most 8 queries per tile then streams 12 bytes
 * per record instead of 16: the header stands in for the key as a lower bound, and only the rare records that pass it read
 * their key.  Results are bit for bit those without the stream.  Larger tiles, other widths and every other call are served
 * from the store's own columns as before.
 * Cost: about 20.03 bytes per record held, plus sort temporaries of about 8 bytes per record during the call.  The build
 * runs on the engine's stream and waits for it.  VC_ERR_INVALID unless bits == 128; VC_ERR_NOMEM, engine unchanged, when
 * stream + temporaries exceed 55 % of the free device memory (the share an MIH index's bucket-order records may take) or an
 * allocation fails.  Building again replaces the stream.
 * Every call that changes the store -- vc_add_codes, vc_add_synthetic, vc_load_code_file, vc_retain* -- drops the stream and
 * frees it; searches then run as without it.  Nothing rebuilds it but this call, so no result depends on call history. */
int vc_build_scan_stream(vc_engine* e);
typedef struct vc_scan_stream_state {
  uint32_t built;          /* 0 / 1 */
  uint32_t reserved;
  uint64_t items;          /* records it covers */
  uint64_t granules;       /* headers (256 sorted records each, padding included) */
  uint64_t bytes;          /* device memory held */
  uint64_t launches;       /* verify launches served from the stream since the build */
  uint64_t bound_passes;   /* diagnostic build (VC_SCAN_DIAGNOSTICS) only, else 0: records of the LAST stream launch that */
  uint64_t exact_passes;   /* passed the lower bound / passed the exact check (summed over its queries) */
} vc_scan_stream_state;
int vc_scan_stream_info(vc_engine* e, vc_scan_stream_state* info);

/* HashIndex{table_id,index} -> Image_List get (search_worker.cc:224-246, base_proxy.h:18).
 * Writes up to cap (id, code) pairs in append (= id) order; *n = bucket length.
 * Returns VC_OK (PROXY_FOUND) or VC_NOT_FOUND.  ids / codes may be NULL. */
int vc_get_bucket(vc_engine* e, uint32_t table, uint32_t index, uint32_t* ids, void* codes, uint32_t cap, uint32_t* n);
/* ImageBitmap::get_idx (bitmap.cc:22-26) on table t's occupancy bitmap. *bit = 0/1. */
int vc_bitmap_test(vc_engine* e, uint32_t table, uint32_t index, int* bit);
/* Raw bitmap words (uint32, LSB-first, 2^substr_bits bits) as generate_bitmap.cc:122-125 writes them;
 * copies [word_off, word_off+n_words) to host memory. */
int vc_bitmap_read(vc_engine* e, uint32_t table, uint64_t word_off, uint64_t n_words, uint32_t* out);

/* ---- search ------------------------------------------------------------------------------
 * replaces: SearchWorker::find (search_worker.cc:65-89) / linear_search.cc:39-64 for a batch of
 * nq queries (nq * bits/8 raw bytes, host memory).
 *   out    nq * k packed results; query i owns out[i*k .. i*k+counts[i])
 *   counts nq entries (may be NULL): results found (< k only if the DB holds fewer items)
 *   stats  nq entries or NULL
 * Result set = the k smallest (dist, id) pairs among the items the mode's loop has seen
 * (LINEAR: all items).  Ties at the k-th distance resolve to the smallest ids.
 * Host memory: any.  Results of up to 512 KB cross in one copy through a pinned staging buffer of the engine; larger ones go
 * out by DMA directly when `out` is page-locked (hipHostMalloc / hipHostRegister: detected per call), else through two pinned
 * chunks with the DMA of one overlapping the host copy of the other -- a 16 384-query top-100 call returns 13 MB of rows:
 * 15 M queries/s into page-locked memory, 11 M into pageable (1e8 records, exact MIH).  `stats` costs the MIH modes four small
 * read-backs per launch and is skipped when NULL. */
int vc_search_knn(vc_engine* e, const void* queries, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order,
                  uint64_t* out, uint32_t* counts, vc_query_stats* stats);
/* Device-pointer variant for callers that keep queries/results in HBM (torch / multi-GPU merge).
 * d_queries: nq*bits/8 bytes; d_out: nq*k uint64, ascending, padded with UINT64_MAX; d_counts: nq uint32.
 * Asynchronous on `stream` and ordered like any other work enqueued there when mode == VC_MODE_LINEAR; the MIH
 * modes make the host wait until the batch's query kernel has finished (how many queries continue in the multi-block
 * shells decides what is enqueued next), so their rows are complete when the call returns; results are valid in
 * stream order in every mode.
 * Batch size, MIH modes: a call's queries run in launches of up to 16 384 (VC_MIH_QTILE) and a launch ends with its longest
 * query, i.e. carries a fixed tail of 60-90 us -- exact top-100 over 1e8 records: 14.4 M queries/s in calls of 4 096 queries,
 * 20.7 M in calls of 16 384; the radius search the same way (1 024 -> 4 096 queries per call: + 10 %).
 * A candidate-ring overflow (more than cand_cap items at or below the k-th distance: duplicate-heavy data,
 * linear_search.cc:113-117 mentions 250 000-entry buckets) is recovered exactly ON THE DEVICE in the same stream
 * (radix select over the position of the tied items), so a LINEAR row is always exact.  Only if that
 * recovery gives up (see vc_device_status) a query reports d_counts[i] == UINT32_MAX with an upper-bound row. */
int vc_search_knn_dev(vc_engine* e, const void* d_queries, uint32_t nq, uint32_t k, uint32_t mode,
                      uint64_t* d_out, uint32_t* d_counts, void* stream);
/* Same, plus SearchWorker::get_stat (search_worker.cc:24-30) for callers that stay on the device: d_stats (device
 * memory, nq records, may be NULL) is written by a kernel in stream order -- no host read-back, no extra wait.
 * LINEAR: n_candidates = records scanned, everything else 0.  n_results = d_counts[i]. */
int vc_search_knn_dev_stats(vc_engine* e, const void* d_queries, uint32_t nq, uint32_t k, uint32_t mode,
                            uint64_t* d_out, uint32_t* d_counts, vc_query_stats* d_stats, void* stream);
/* All items within full Hamming distance <= radius of each query (BASELINE config 2; built from
 * search_R_neighbors shells 0..radius/m, search_worker.cc:222-227).  mode LINEAR or MIH_EXACT.
 * out_offsets: nq+1 entries; results of query i at out[out_offsets[i] .. out_offsets[i+1]),
 * ascending packed.  VC_ERR_CAPACITY (with out_offsets filled with the needed counts) if out_cap is too small. */
int vc_search_radius(vc_engine* e, const void* queries, uint32_t nq, uint32_t radius, uint32_t mode,
                     uint64_t* out, uint64_t out_cap, uint64_t* out_offsets);

/* Device-pointer variant (queries and results stay in HBM): d_queries nq*bits/8 bytes, d_out out_cap packed values,
 * d_offsets nq+1 entries, all device memory.  The work is enqueued on `stream`; the host waits once, at the end, for the
 * total (and repeats the call internally with a larger work ring if a query outgrew it).  The copy into d_out may still be
 * running on `stream` when the call returns: the results are valid in stream order, a host reader copies behind it.
 * VC_ERR_CAPACITY if the results do not fit out_cap (d_offsets then holds the needed counts).
 * replaces: the same reference loop as vc_search_radius (search_worker.cc:222-264). */
int vc_search_radius_dev(vc_engine* e, const void* d_queries, uint32_t nq, uint32_t radius, uint32_t mode,
                         uint64_t* d_out, uint64_t out_cap, uint64_t* d_offsets, void* stream);

/* ---- queries named by id ------------------------------------------------------------------
 * replaces: image_search_client::search_image_by_id(id, knn, approximate) (image_search_client.h:12-27; its throughput tester
 * replays a file of query ids, image_search_test.cc:112-170) and the ID -> BinaryCode read (linear_search.cc:45-46), for a BATCH
 * of ids whose codes never leave HBM: a gather kernel turns the ids into the [nq][bits/64] query layout out of the column store,
 * the unchanged search runs on it, and a small kernel shapes the rows. */
#define VC_IDS_EXCLUDE_SELF 0x1u   /* row = the k nearest items OTHER than the query's own record */
#define VC_IDS_ONLY_GREATER 0x2u   /* radius-by-id calls only: a segment keeps the entries whose id exceeds the query's own */

/* ID -> BinaryCode for a batch, in HBM (linear_search.cc:45-46).  d_ids: nq global ids; d_codes: nq*bits/8 bytes; d_found: nq
 * uint32 (may be NULL), 1 = the id is resident, 0 = it is not (outside [id_base, id_base + vc_size)) and its code is all zero.
 * One launch on `stream`, nothing is waited for. */
int vc_get_codes_dev(vc_engine* e, const uint32_t* d_ids, uint32_t nq, void* d_codes, uint32_t* d_found, void* stream);
/* image_search_client::search_image_by_id for a batch (image_search_client.h:12-27).  ids: nq global ids (host memory); out,
 * counts, stats, order as vc_search_knn; id_flags: 0 or VC_IDS_EXCLUDE_SELF, any other bit gives VC_ERR_INVALID.
 *   id_flags == 0          rows, counts and statistics of a resident id are bit for bit those of vc_search_knn /
 *                          vc_search_knn_dev_stats in the same mode with the same k, queried with the code vc_get_code returns
 *                          for that id (so the row starts with the record itself, or with its duplicates of smaller id).
 *   VC_IDS_EXCLUDE_SELF    the row is that of the same call with k + 1, with the entry (distance 0, own id) removed if it is
 *                          present, cut to k.  The entry is found by value, not by position: duplicates with smaller ids precede
 *                          it, and with more than k of them it is not in the k + 1 row at all, which is then simply cut to k.
 *                          n_results and the count are those of the stripped row, the other statistics the k + 1 call's.  k may
 *                          be at most VC_MAX_K - 1 = 8191 then, else VC_ERR_INVALID.
 * A batch has no VC_NOT_FOUND: an id that is not resident gives count 0, a UINT64_MAX-padded row and zero statistics, and the call
 * still returns VC_OK.  Repeated ids are independent queries.  The scratch (gathered queries, k + 1 rows, counts, found words) is
 * grow-only buffers of the handle, separate from those of the other calls; a result depends on the database and the call only.
 * Bit 0x2 (VC_IDS_ONLY_GREATER) is refused here like any unknown bit.  Radius search by id is not offered by these k-NN calls: it
 * is vc_search_radius_ids / vc_search_radius_ids_dev below, which compact the variable-length result on the device. */
int vc_search_knn_ids(vc_engine* e, const uint32_t* ids, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order, uint32_t id_flags,
                      uint64_t* out, uint32_t* counts, vc_query_stats* stats);
/* The same for ids and results in HBM (search_image_by_id, image_search_client.h:12-27): d_ids nq uint32; d_out nq*k ascending,
 * UINT64_MAX padded; d_counts (may be NULL) and d_stats (may be NULL) as vc_search_knn_dev_stats.  Stream behaviour is exactly
 * that of vc_search_knn_dev_stats underneath, plus two small launches on `stream` (gather before, strip / found mask after):
 * VC_MODE_LINEAR waits for nothing on the host, the MIH modes wait as they do there; results are valid in stream order. */
int vc_search_knn_ids_dev(vc_engine* e, const uint32_t* d_ids, uint32_t nq, uint32_t k, uint32_t mode, uint32_t id_flags,
                          uint64_t* d_out, uint32_t* d_counts, vc_query_stats* d_stats, void* stream);

/* "Which records lie within `radius` of THESE records": vc_search_radius / vc_search_radius_dev for a batch of ids whose codes never
 * leave HBM (the near-duplicate question; search_R_neighbors, search_worker.cc:222-264, asked through search_image_by_id's id ->
 * code read, image_search_client.h:12-27).  mode VC_MODE_LINEAR or VC_MODE_MIH_EXACT; result layout as vc_search_radius_dev: offsets
 * has nq + 1 entries, query i owns out[offsets[i] .. offsets[i+1]), ascending packed (dist, id).
 * Errors are those of the radius call underneath and are checked before any work: VC_ERR_INVALID for another mode, nq == 0, null
 * ids / offsets, or out == NULL with out_cap != 0; VC_ERR_STATE in MIH mode without a current index.  id_flags: any combination of
 * VC_IDS_EXCLUDE_SELF and VC_IDS_ONLY_GREATER, any other bit gives VC_ERR_INVALID.
 *   id_flags == 0          the segment of a resident id is bit for bit that of vc_search_radius / vc_search_radius_dev in the same
 *                          mode and radius, queried with the code vc_get_code returns for that id.
 *   VC_IDS_EXCLUDE_SELF    that segment without the entry (0, own id).  The entry is matched by value, not by position (duplicates
 *                          with smaller ids precede it); it is always present for a resident id, its distance being 0 <= radius.
 *   VC_IDS_ONLY_GREATER    that segment without every entry whose id is <= the query's own id -- the own entry included, so adding
 *                          VC_IDS_EXCLUDE_SELF changes nothing.  Walking all resident ids in batches lists every unordered pair
 *                          within `radius` exactly once.  The kept entries stay in ascending packed order (a stable compaction).
 * A batch has no VC_NOT_FOUND: an id that is not resident (outside [id_base, id_base + vc_size)) owns an empty segment and the call
 * still returns VC_OK.  Repeated ids are independent queries.
 * Capacity, with T the compacted total: T > out_cap gives VC_ERR_CAPACITY, offsets then holds the compacted prefix sums
 * (offsets[nq] = T) and out is untouched -- the protocol of vc_search_radius_dev; out_cap = 0 with out = NULL asks for the sizes.
 * Device form: gather, the radius search underneath and the compaction (count, two scans, copy: 64-bit entries cut into chunks of
 * 1024 per query, so a long segment spreads over many blocks) are enqueued on `stream`.  The host waits where the radius search
 * underneath waits -- once per attempt for its total -- and at most once more, for T: not at all when the uncompacted total already
 * fits out_cap, since T <= that total.  The copy into d_out may still be running when the call returns; results are valid in
 * stream order.  The scratch (gathered queries, found words, the uncompacted results and their offsets, per-chunk counts) is
 * grow-only buffers of the handle, separate from those of every other call, every word written before it is read within a call: a
 * result depends on the database and the call only.  When the scratch for the uncompacted results is too small the call underneath
 * reports the size needed; the scratch grows and the search runs once more. */
int vc_search_radius_ids_dev(vc_engine* e, const uint32_t* d_ids, uint32_t nq, uint32_t radius, uint32_t mode, uint32_t id_flags,
                             uint64_t* d_out, uint64_t out_cap, uint64_t* d_offsets, void* stream);
/* The same for ids, results and offsets in host memory: the device form on the engine's stream plus the staged ids and the copy home
 * of the offsets (also with VC_ERR_CAPACITY) and the results; waits for them. */
int vc_search_radius_ids(vc_engine* e, const uint32_t* ids, uint32_t nq, uint32_t radius, uint32_t mode, uint32_t id_flags,
                         uint64_t* out, uint64_t out_cap, uint64_t* out_offsets);

/* "Which records are near-duplicates of each other", as a grouping: the connected components of the radius graph over ALL resident
 * records (two records are adjacent when their full Hamming distance is <= `radius`; a group is what chains of adjacent records
 * connect).  It replaces a walk of vc_search_radius_ids_dev with VC_IDS_ONLY_GREATER over all ids, the copy home of every pair and
 * a host union-find: the pairs never leave HBM, and the search's raw result is united as it lies, without the compaction.
 * labels: N = vc_size entries.  labels[i] = the GLOBAL id of the smallest-id record of the component of record id_base + i -- a
 * function of the database and the radius only, whatever `batch`, `mode` or the order the device worked in.
 * mode VC_MODE_LINEAR or VC_MODE_MIH_EXACT.  Errors are checked before any work and leave labels untouched: VC_ERR_INVALID for
 * another mode, null labels or n_labelled > N; VC_ERR_STATE in MIH mode without a current index (a stale one counts as none, as in
 * vc_search_radius_ids).  N == 0 gives VC_OK and zero stats; nothing is written.
 * batch: ids per radius search underneath, 0 = 4096; any value >= 1 is legal, larger than N too; the result does not depend on it.
 * n_labelled is the incremental form, the companion of vc_update_index: labels[0 .. n_labelled) come IN and entries from n_labelled
 * on are ignored and overwritten.  PRECONDITION: the incoming labels are what this call produced for the first n_labelled records
 * ALONE (a store that held exactly those records), at this same radius.  Only the ids id_base + n_labelled .. are queried; of a
 * query's entries those are united whose id exceeds the query's own or lies below id_base + n_labelled, so every pair with an old
 * member is seen from its new member and every new-new pair once.  The result is bit for bit that of a call from scratch
 * (n_labelled == 0) over all N records -- old groups that a new record bridges are merged.  n_labelled == N only re-flattens and
 * counts.
 * stats (host memory, may be NULL) is filled when the call returns.
 * Device form: d_labels IS the union-find forest, in place, and must not be touched by the caller during the call.  Everything is
 * enqueued on `stream`; the host waits where the radius search underneath waits -- once per batch and attempt, for its total -- and
 * once more at the end, for the stats.  Labels are valid in stream order.
 * The scratch (the batch's ids, gathered queries, found words, the raw results and their offsets, two counters) is grow-only
 * buffers of the handle, separate from those of every other call but vc_leaders_radius*, vc_dbscan_radius*, vc_cluster_levels* and vc_dbscan_levels*, which fill the same
 * batch buffers completely before they read them -- every word written before it is read within a call: a result depends on the database and the
 * call only.  The raw results grow to the LARGEST batch's total: on duplicate-heavy data that is
 * `batch` x the size of a group of duplicates (4096 ids into a bucket of 250 000 are 8 GB), so choose a smaller batch there. */
typedef struct vc_cluster_stats {
  uint64_t n_pairs;     /* unordered pairs {a < b} within `radius` that this call examined: all those with b >= n_labelled */
  uint64_t n_clusters;  /* components over ALL resident records after the call */
} vc_cluster_stats;
int vc_cluster_radius_dev(vc_engine* e, uint32_t radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* d_labels,
                          vc_cluster_stats* stats, void* stream);
/* The same for labels in host memory: the device form on the engine's stream plus the staged labels (the first n_labelled go in,
 * all N come home); waits for them. */
int vc_cluster_radius(vc_engine* e, uint32_t radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* labels,
                      vc_cluster_stats* stats);

/* "Drop the near-duplicates", as the one-pass rule of a dedup pipeline: walk the records in id order and keep a record iff no record
 * kept so far lies within `radius` of it.  It stands for one pass of a first-come dedup over the file order of
 * build_hash_tables.cc:40-70 (ids are the ordinals of the records), asked through search_R_neighbors, search_worker.cc:222-264.  The
 * kept records, the LEADERS, are the lexicographically first maximal independent set of the radius graph: every dropped record is
 * within `radius` of a leader, no two leaders are within `radius` of each other, and whether record i leads depends on the records
 * 0 .. i only.  vc_cluster_radius groups by single linkage instead: its components chain, and nothing bounds how far a member lies
 * from its label.
 * labels: N = vc_size entries.  Record id_base + i is a LEADER iff no leader with a smaller id lies within full Hamming distance
 * `radius` of it.  labels[i] = the record's own GLOBAL id for a leader, otherwise the global id of the SMALLEST-id leader within
 * `radius` (one exists and it is smaller than the record's own id): labels[i] <= id_base + i always.  The result is a function of
 * the database and the radius only, whatever `batch`, `mode`, the order the device worked in or the handle's history.
 * mode VC_MODE_LINEAR or VC_MODE_MIH_EXACT.  Errors are checked before any work and leave labels untouched: VC_ERR_INVALID for a
 * null handle, null labels, another mode or n_labelled > N; VC_ERR_STATE in MIH mode without a current index (a stale one counts as
 * none).  N == 0 gives VC_OK and zero stats; nothing is written.  stats (host memory, may be NULL) is filled when the call returns.
 * batch: ids per radius search underneath, 0 = 4096; any value >= 1 is legal, larger than N too (above 2^29 it is cut to 2^29); the
 * result does not depend on it.
 * n_labelled is the incremental form, the companion of vc_update_index: labels[0 .. n_labelled) come IN.  PRECONDITION: they are
 * this call's result for those records at this same radius -- by the prefix property that is the same for ANY store whose first
 * n_labelled records are these.  The incoming entries are READ ONLY: the call writes entries n_labelled .. N and not one byte below
 * (unlike vc_cluster_radius, where old labels change), and the result is bit for bit that of a call from scratch.  n_labelled == N
 * writes nothing and only counts.
 * How: the batches are taken in ascending id order, so every record below a batch is final and leads iff labels[v] == v.  Of a
 * query's entries only those with an id v below its own matter.  A batch is decided in synchronous ROUNDS over one state word per
 * query in scratch (never a sentinel inside labels: every 32-bit value is a legal id).  Round 1 also settles against the past: a
 * leader below the batch drops the query, and the smallest such is its label at once.  In a round an undecided query is DROPPED as
 * soon as one smaller neighbour of the batch is a decided leader, a LEADER when all of them are decided and dropped (or there is
 * none), and waits otherwise; a round reads the state the previous round left (a word stored in round r carries r and counts as
 * undecided to the readers of round r).  Every decision is the sequential pass's own, so the fixed point is unique; the smallest
 * undecided id is decided in every round, so a batch of nq ids ends after at most nq rounds -- the driver returns VC_ERR_HIP should
 * that bound ever be crossed.  After the last round the queries dropped inside the batch take the minimum over ALL their leader
 * neighbours.  No kernel waits for another block; rounds are separate launches, and a round launched behind the fixed point returns
 * on a device counter before it touches an entry.
 * Device form: everything is enqueued on `stream`; the host waits where the radius search underneath waits -- once per batch and
 * attempt, for its total -- once per group of 4 rounds of a batch, for the undecided counter, and once at the end, for the stats.
 * d_labels must not be touched by the caller during the call.  Labels are valid in stream order.
 * Scratch: the batch buffers (ids, gathered queries, found words, the raw results and their offsets) and the host form's staged
 * labels are THOSE OF vc_cluster_radius* -- both calls fill them completely before they read them; the state words, the statistics
 * and the round counters are this call's own.  All grow-only buffers of the handle, every word written before it is read within a
 * call; the note on the raw results' size at vc_cluster_radius holds here too.
 * Consuming the result: vc_retain* with VC_RETAIN_ROOTS accepts these labels as they are (a leader is labelled with itself) and
 * keeps exactly the leaders.  The survivors then are pairwise farther than `radius` apart, every removed record was within
 * `radius` of a survivor (the one its label named), and a second call at the same radius finds n_pairs == 0 and every record a
 * leader. */
typedef struct vc_leader_stats {
  uint64_t n_pairs;    /* unordered pairs {a < b} within `radius` with b >= n_labelled: the entries (query b, neighbour a < b) examined;
                          the same number vc_cluster_stats.n_pairs reports for the same arguments */
  uint64_t n_leaders;  /* records i with labels[i] == id_base + i over ALL N resident records after the call */
  uint64_t n_rounds;   /* decision rounds that had work, summed over the batches (at least one per batch): a diagnostic that depends
                          on `batch`, not part of the result */
} vc_leader_stats;
int vc_leaders_radius_dev(vc_engine* e, uint32_t radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* d_labels,
                          vc_leader_stats* stats, void* stream);
/* The same for labels in host memory: the device form on the engine's stream plus the staged labels (the first n_labelled go in,
 * the entries n_labelled .. N come home); waits for them. */
int vc_leaders_radius(vc_engine* e, uint32_t radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* labels,
                      vc_leader_stats* stats);

/* "Group the near-duplicates by density": DBSCAN over the radius graph.  It stands for search_R_neighbors, search_worker.cc:222-264,
 * asked for every record of the file order of build_hash_tables.cc:40-70 (ids are the ordinals of the records), followed by the
 * textbook density rule.  vc_cluster_radius takes ONE neighbour within `radius` as proof that two records belong together, so one
 * accidental near pair welds two groups; vc_leaders_radius does not chain but has no notion of noise.  Here:
 *   a record is a CORE iff at least min_pts records lie within `radius` of it;
 *   the CLUSTERS are the components of the graph whose vertices are the cores, two cores within `radius` being adjacent;
 *   a non-core record with at least one core within `radius` is a BORDER of the cluster of its smallest-id core neighbour
 *   (textbook DBSCAN leaves a border between two clusters to the visiting order; here the choice is fixed);
 *   every other record is NOISE.
 * N = vc_size.  degrees: N entries, may be NULL (the handle then uses grow-only scratch of its own).  degrees[i] = the number of
 * resident records within full Hamming distance `radius` of record id_base + i, the record ITSELF counted (scikit-learn's min_samples
 * convention) and exact duplicates once each; record i is a core iff degrees[i] >= min_pts.
 * labels: N entries.  Core: the smallest GLOBAL id among the cores of its component.  Border: the label of its smallest-id core
 * neighbour.  Noise: its own global id.
 * TELLING THE KINDS APART: no sentinel is used, every 32-bit value being a legal id.  With own = id_base + i:
 *   noise                        labels[i] == own and degrees[i] <  min_pts
 *   a cluster's representative   labels[i] == own and degrees[i] >= min_pts
 *   another core of a cluster    labels[i] != own and degrees[i] >= min_pts
 *   border                       labels[i] != own and degrees[i] <  min_pts
 * The result is a function of the database, `radius` and min_pts only, whatever `batch`, `mode`, the order the device worked in or
 * the handle's history.  min_pts == 1 makes every record a core: the labels are bit for bit those of vc_cluster_radius.  min_pts == 2
 * makes every record with a neighbour a core: the labels again equal vc_cluster_radius', the isolated records reported as noise.
 * min_pts > N makes every record noise: the labels are the identity and n_clusters == 0.
 * mode VC_MODE_LINEAR or VC_MODE_MIH_EXACT.  Errors are checked before any work and leave labels and degrees untouched:
 * VC_ERR_INVALID for a null handle, null labels, min_pts == 0 or another mode; VC_ERR_STATE in MIH mode without a current index (a
 * stale one counts as none).  N == 0 gives VC_OK and zero stats; nothing is written.  stats (host memory, may be NULL) is filled when
 * the call returns.  batch: as in vc_cluster_radius, 0 = 4096, any value >= 1 is legal; the result does not depend on it.
 * THERE IS NO n_labelled FORM: a new record can raise an old record to core, and the pairs of OLD records which that promotion
 * makes matter (two old cores to unite, an old border to anchor) are not seen again by a walk of the new records alone.  After
 * vc_add_codes + vc_update_index call again from scratch.
 * How: ONE walk of the radius search, as in vc_cluster_radius.  The batches are taken in ascending id order.  The degree of a
 * queried record is the length of its raw segment (the search returns every record within the radius exactly once, the query's own
 * included), so after a batch's degree launch every record up to the batch's end has its final degree.  Every unordered pair is
 * also seen from its LARGER member, and by then both degrees are known: the edge launch acts on the entries whose id is below the
 * query's own -- two cores are united in a lock-free forest over the cores (labels[] in place, the larger root hooked under the
 * smaller), exactly one core is noted by the other record as its anchor, the minimum kept.  After the last batch one finish pass
 * writes the roots and counts the kinds.  No kernel waits for another block.
 * Device form: everything is enqueued on `stream`; the host waits where the radius search underneath waits -- once per batch and
 * attempt, for its total -- and once at the end, for the stats.  d_labels and d_degrees must not be touched by the caller during
 * the call.  Results are valid in stream order.
 * Scratch: the batch buffers (ids, gathered queries, found words, the raw results and their offsets) and the host form's staged
 * labels are THOSE OF vc_cluster_radius* / vc_leaders_radius* -- every call fills them completely before it reads them; the degrees
 * of a call that passes none and the statistics are this call's own.  All grow-only buffers of the handle, every word written
 * before it is read within a call; the note on the raw results' size at vc_cluster_radius holds here too.
 * Consuming the result: vc_retain* with VC_RETAIN_ROOTS accepts these labels as they are.  It keeps one representative per cluster
 * and every noise record (both are labelled with themselves) and drops the borders and the other cores: n_clusters + n_noise
 * records survive. */
typedef struct vc_dbscan_stats {
  uint64_t n_pairs;     /* unordered pairs {a < b} within `radius`: every one examined once (== vc_cluster_stats.n_pairs at n_labelled 0) */
  uint64_t n_clusters;  /* components of the core graph */
  uint64_t n_core, n_border, n_noise;   /* sum to N */
} vc_dbscan_stats;
int vc_dbscan_radius_dev(vc_engine* e, uint32_t radius, uint32_t min_pts, uint32_t mode, uint32_t batch, uint32_t* d_labels,
                         uint32_t* d_degrees, vc_dbscan_stats* stats, void* stream);
/* The same for labels and degrees (may be NULL) in host memory: the device form on the engine's stream into staged buffers, which
 * then come home; waits for them. */
int vc_dbscan_radius(vc_engine* e, uint32_t radius, uint32_t min_pts, uint32_t mode, uint32_t batch, uint32_t* labels, uint32_t* degrees,
                     vc_dbscan_stats* stats);

/* "Which radius should I cluster at": the grouping of vc_cluster_radius at EVERY radius 0 .. max_radius from ONE walk of the radius
 * search, with the histogram of the pair distances -- the single-linkage dendrogram cut at every integer height.  Hamming distances
 * are integers and the raw result of the search at max_radius already holds every pair within every smaller radius, each entry with
 * its distance; a loop of max_radius + 1 vc_cluster_radius calls walks the store that many times.
 * labels: LEVEL-MAJOR, (max_radius + 1) * N entries with N = vc_size; labels[r * N + i] (index it in 64 bits) is the label of record
 * id_base + i at radius r.  Level r equals BIT FOR BIT what vc_cluster_radius* returns for radius = r with the same mode and
 * n_labelled and any batch -- the smallest GLOBAL id of the record's component -- stats->n_clusters[r] equals that call's n_clusters,
 * and n_pairs[0] + ... + n_pairs[r] its n_pairs.  The levels are nested: labels[r * N + i] <= labels[(r - 1) * N + i].
 * mode VC_MODE_LINEAR or VC_MODE_MIH_EXACT.  Errors are checked before any work and leave labels untouched: VC_ERR_INVALID for a
 * null handle, null labels, another mode, n_labelled > N or max_radius >= VC_LEVELS_MAX; VC_ERR_STATE in MIH mode without a current
 * index (a stale one counts as none).  N == 0 gives VC_OK and zero stats; nothing is written.  stats (host memory, may be NULL) is
 * filled when the call returns; its entries above max_radius are 0.
 * batch: as in vc_cluster_radius, 0 = 4096, any value >= 1 is legal; the result does not depend on it.
 * n_labelled is the incremental form, the companion of vc_update_index: for EVERY level r the entries labels[r * N .. r * N +
 * n_labelled) come IN -- the stride is the NEW N, so the caller re-lays the array of its earlier call -- and the entries behind them
 * are ignored and overwritten.  PRECONDITION: they are this call's level r for the first n_labelled records ALONE.  Only the ids
 * id_base + n_labelled .. are queried, with the keep rule of vc_cluster_radius.  The result is bit for bit that of a call from scratch;
 * n_pairs[d] counts the pairs {a < b} of distance d with b >= n_labelled.  n_labelled == N only re-flattens and counts.
 * How: one forest per level, in place in labels.  Per batch the walk of vc_cluster_radius at max_radius, then one launch over the raw
 * result: a kept entry of distance d is united in forest d ONLY (not in the forests d .. max_radius: one union per pair), and
 * counted in n_pairs[d].  After the last batch the cascade, one launch per level r = 1 .. max_radius: every record is united in
 * forest r with its root in forest r - 1, which is final by then -- by induction forest r connects exactly what the pairs of distance
 * <= r connect; the incoming labels of the incremental form are trees of their level like any other.  Then one launch flattens all
 * levels and counts their roots.  No kernel waits for another block.
 * Device form: d_labels holds the forests and must not be touched by the caller during the call.  Everything is enqueued on
 * `stream`; the host waits where the radius search underneath waits -- once per batch and attempt, for its total -- and once more at
 * the end, for the stats.  Labels are valid in stream order.
 * Scratch: the batch buffers (ids, gathered queries, found words, the raw results and their offsets) and the host form's staged
 * labels (grown to all levels) are THOSE OF vc_cluster_radius* -- every call fills them completely before it reads them; the 2 x 64
 * counters are this call's own.  All grow-only buffers of the handle, every word written before it is read within a call; the note
 * on the raw results' size at vc_cluster_radius holds here too, at max_radius. */
#define VC_LEVELS_MAX 64            /* levels 0 .. 63 */
typedef struct vc_levels_stats {    /* 1024 bytes */
  uint64_t n_pairs[VC_LEVELS_MAX];     /* [d] = unordered pairs {a < b}, b >= n_labelled, at distance EXACTLY d; 0 above max_radius */
  uint64_t n_clusters[VC_LEVELS_MAX];  /* [r] = components over ALL resident records at radius r; 0 above max_radius */
} vc_levels_stats;
int vc_cluster_levels_dev(vc_engine* e, uint32_t max_radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* d_labels,
                          vc_levels_stats* stats, void* stream);
/* The same for labels in host memory: the device form on the engine's stream plus the staged labels (of every level the first
 * n_labelled go in, all (max_radius + 1) * N come home); waits for them. */
int vc_cluster_levels(vc_engine* e, uint32_t max_radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* labels,
                      vc_levels_stats* stats);

/* "Which radius, and which min_pts, should I run DBSCAN at": the grouping of vc_dbscan_radius at EVERY radius 0 .. max_radius from
 * ONE walk of the radius search, with every record's CORE DISTANCE -- the k-distance that DBSCAN users plot to choose eps -- and the
 * histogram of the pair distances.  A loop of max_radius + 1 vc_dbscan_radius calls walks the store that many times.
 * labels: LEVEL-MAJOR, (max_radius + 1) * N entries with N = vc_size; labels[r * N + i] (index it in 64 bits) equals BIT FOR BIT what
 * vc_dbscan_radius* returns in labels[i] for radius = r with the same min_pts, either mode and any batch.  No sentinel appears in
 * labels.  vc_retain* with VC_RETAIN_ROOTS takes any one level, labels + r * N, as it is.
 * core_dist (N entries, may be NULL: the handle then uses scratch of its own): core_dist[i] = the distance from record id_base + i to
 * its min_pts-th nearest resident record, ITSELF COUNTED (so min_pts == 1 gives 0 everywhere), or VC_CORE_NEVER if fewer than min_pts
 * records lie within max_radius.  Record i is a core at level r iff core_dist[i] <= r -- the test that stands for vc_dbscan_radius's
 * degrees[i] >= min_pts; with it the kinds are told apart as there: a non-core record is a border at level r iff labels[r * N + i] !=
 * id_base + i, else noise.  min_pts == 1 makes every record a core at every level and labels equal to vc_cluster_levels*.
 * stats (host memory, may be NULL) is filled when the call returns; n_clusters, n_core, n_border and n_noise at [r] equal the
 * vc_dbscan_stats of vc_dbscan_radius(r, min_pts); every entry above max_radius is 0.
 * mode VC_MODE_LINEAR or VC_MODE_MIH_EXACT.  Errors are checked before any work and leave the outputs untouched: VC_ERR_INVALID for a
 * null handle, null labels, min_pts == 0, another mode or max_radius >= VC_LEVELS_MAX; VC_ERR_STATE in MIH mode without a current
 * index (a stale one counts as none).  N == 0 gives VC_OK and zero stats; nothing is written.
 * batch: as in vc_dbscan_radius, 0 = 4096, any value >= 1 is legal; the result does not depend on it.
 * There is NO n_labelled form, for vc_dbscan_radius's reason: a new record changes the degrees, hence the core distances, of the
 * old ones, so old records turn from border or noise into cores and the old labels are no starting point.
 * How: a pair {a, b} at distance d joins two cores at exactly the levels r >= w = max(d, core_dist[a], core_dist[b]) -- the
 * mutual-reachability distance, an integer here.  One forest per level over that level's cores, in place in labels.  Per batch the walk
 * of vc_dbscan_radius at max_radius, then two launches: the core distances of the batch's queries (entry min_pts - 1 of an ascending
 * segment), then, over the entries whose neighbour has the smaller id -- every pair once, both core distances final -- the union in
 * forest w ONLY and, where one end is no core yet at the level t at which the other becomes its core neighbour, a CAS minimum on that
 * end's anchor candidate of exactly level t.  After the last batch the cascade, one launch per level r = 1 .. max_radius: every core
 * of level r - 1 is united in forest r with its root in forest r - 1.  One last launch walks every record up the levels: a core
 * takes its root, a non-core the root of the smallest candidate of the levels <= r, or keeps its own id; it counts the kinds.  No
 * kernel waits for another block.
 * Device form: d_labels and d_core_dist hold the state and must not be touched by the caller during the call.  Everything is enqueued
 * on `stream`; the host waits where the radius search underneath waits -- once per batch and attempt, for its total -- and once more
 * at the end, for the stats.  Labels and core distances are valid in stream order.
 * Scratch: the batch buffers and the host form's staged labels (grown to all levels) are THOSE OF vc_cluster_radius* -- every call
 * fills them completely before it reads them; the core distances of a call that passes none (and of the host form) and the 5 x 64
 * counters are this call's own.  All grow-only buffers of the handle, every word written before it is read within a call; the note
 * on the raw results' size at vc_cluster_radius holds here too, at max_radius. */
#define VC_CORE_NEVER 0xFFFFFFFFu      /* core_dist: fewer than min_pts records within max_radius */
typedef struct vc_dbscan_levels_stats {   /* 2560 bytes; every entry above max_radius is 0 */
  uint64_t n_pairs[VC_LEVELS_MAX];     /* [d] = unordered pairs {a < b} at distance EXACTLY d (== vc_levels_stats.n_pairs at n_labelled 0) */
  uint64_t n_clusters[VC_LEVELS_MAX];  /* [r] == vc_dbscan_stats.n_clusters of vc_dbscan_radius(r, min_pts) */
  uint64_t n_core[VC_LEVELS_MAX], n_border[VC_LEVELS_MAX], n_noise[VC_LEVELS_MAX];   /* [r], sum to N */
} vc_dbscan_levels_stats;
int vc_dbscan_levels_dev(vc_engine* e, uint32_t max_radius, uint32_t min_pts, uint32_t mode, uint32_t batch, uint32_t* d_labels,
                         uint32_t* d_core_dist, vc_dbscan_levels_stats* stats, void* stream);
/* The same for labels and core_dist (may be NULL) in host memory: the device form on the engine's stream into staged buffers, which
 * then come home; waits for them. */
int vc_dbscan_levels(vc_engine* e, uint32_t max_radius, uint32_t min_pts, uint32_t mode, uint32_t batch, uint32_t* labels,
                     uint32_t* core_dist, vc_dbscan_levels_stats* stats);

/* "What is in each group": the step after vc_cluster_radius*, vc_leaders_radius* or vc_dbscan_radius*, which all stop at a labels
 * array.  Per group of equal labels: its size, its typical code and the member to keep.  The reference has nothing of the kind; the
 * call replaces the copy home of N codes and N labels, a host sort and a per-bit vote.
 * INPUT: labels, N = vc_size entries, every value in the resident id range [id_base, id_base + N).  Two records are in one group iff
 * their labels are equal.  Nothing else is assumed -- labels[l - id_base] == l need not hold, a label need not be a member of its own
 * group: the output of any of the three clustering calls qualifies, and so does any hand-made partition.
 * OUTPUT, with G the number of distinct labels and the groups numbered 0 .. G - 1 by ASCENDING label:
 *   groups[g]       the vc_group below.
 *   centroids       G rows of bits / 8 bytes in the byte layout of vc_add_codes / vc_get_code (8-byte aligned): bit b of row g is 1 iff
 *                   STRICTLY more than half of the members have bit b set -- a tie in an even-sized group gives 0.  This per-bit
 *                   majority code minimises the sum of Hamming distances to the members, exactly, in integers.
 *   rep             the member with the smallest (distance to the centroid, global id): a tie in distance goes to the smaller id.
 *   rep_labels[i]   the rep of record i's group, N entries.  By construction rep_labels[rep - id_base] == rep, so
 *                   vc_retain*(rep_labels, VC_RETAIN_ROOTS) keeps exactly the representatives; vc_retain* is unchanged.
 *   group_index[i]  g, the dense number of record i's group, N entries.
 * centroids, rep_labels and group_index may each be NULL; groups may be NULL only if groups_cap == 0.
 * CAPACITY, the protocol of the radius calls: *n_groups (may be NULL) = G always.  G > groups_cap returns VC_ERR_CAPACITY and NONE of
 * the four outputs is written (rep_labels and group_index do not depend on the cap, but they are not written either: the call ends
 * at its read-back).  G <= N, so groups_cap = N never fails.
 * ERRORS: VC_ERR_INVALID for a null handle, null labels with N > 0, null groups with groups_cap > 0 -- checked before any work; and
 * for a label outside the range, which is detected ON THE DEVICE by a flag word that comes home together with G: keys are clamped
 * before anything is addressed by them, so no address is ever formed from such a label; the outputs are untouched (*n_groups = 0).
 * N == 0 gives VC_OK and G = 0; nothing is read or written.  VC_ERR_NOMEM leaves the outputs untouched: the buffers are grown
 * before the first output word is written.
 * The result is a function of the codes and `labels` only: no order of lanes, no earlier call on the handle, no VC_GROUP_WINDOW and
 * no shard layout changes a bit of it.
 * How: the (label - id_base, id) pairs go through the index builder's stable radix sort, so a group's members lie contiguous in
 * ascending id order; head flags and three prefix sums number the groups, the work items and the big groups.  The codes of the sorted
 * ids are fetched by vc_get_codes_dev in windows of VC_GROUP_WINDOW positions (environment, read at vc_create; default 2^20, a multiple
 * of 1024) plus 1024 of overlap.  Groups of 1 .. 2 take one thread, of 3 .. 1024 one wave, larger ones one wave per 1024 members whose
 * vote counts, smallest (distance, id) and largest distance meet in integer atomics; only then a second walk of the windows happens.
 * Device form: everything is enqueued on `stream`; the host waits exactly ONCE, for 16 bytes -- G, the error flag and two counts that
 * size the launches behind it -- and one word per window.  d_labels must not be touched during the call; it may not overlap an output.
 * Outputs are valid in stream order.  The call is ordered behind the handle's previous call whatever its stream, like every call.
 * Scratch: three grow-only buffers of the handle, this call's own (no other call uses them), every word written before it is read
 * within a call: 24 N bytes and the sort's histograms; the row buffer (min(N, VC_GROUP_WINDOW + 1024) codes) with 4 * bits + bits / 8
 * + 16 bytes per group above 1024 members; the host form's staged labels and outputs.  Nothing is allocated or released by a call
 * that needs no more than an earlier one did; a call that needs more re-allocates the buffer, which waits for the device once.
 * A record count above 2^32 - 3 returns VC_ERR_INVALID (the prefix sums are 32-bit). */
typedef struct vc_group {       /* 24 bytes */
  uint32_t label;     /* the value shared by the members' labels[] entries */
  uint32_t size;      /* members */
  uint32_t rep;       /* GLOBAL id of the representative (a member) */
  uint32_t rep_dist;  /* Hamming distance representative -> centroid */
  uint32_t max_dist;  /* largest distance of a member to the centroid */
  uint32_t reserved;  /* 0 */
} vc_group;
int vc_group_summary_dev(vc_engine* e, const uint32_t* d_labels, uint64_t groups_cap, vc_group* d_groups, void* d_centroids,
                         uint32_t* d_rep_labels, uint32_t* d_group_index, uint64_t* n_groups, void* stream);
/* The same for labels and outputs in host memory: the device form on the engine's stream into staged buffers, of which the first G
 * groups and centroid rows and the two N-entry arrays come home; waits for them. */
int vc_group_summary(vc_engine* e, const uint32_t* labels, uint64_t groups_cap, vc_group* groups, void* centroids, uint32_t* rep_labels,
                     uint32_t* group_index, uint64_t* n_groups);

/* "Take these records out": the store and its index cut down to the surviving records, in place.  The reference has no delete
 * (its store has put and get only, base_proxy.h:18-22, and its index is one pass of build_hash_tables.cc over a code file); the call
 * stands for running build_hash_tables.cc:40-70 again over the code file without the removed records, and replaces the copy home of
 * the survivors, a second handle, vc_add_codes and vc_build_index.
 * N = vc_size before the call, K = the survivors.  sel: N words.  kind says how they are read:                                      */
#define VC_RETAIN_MASK  0u   /* record i survives iff sel[i] != 0 */
#define VC_RETAIN_ROOTS 1u   /* record i survives iff sel[i] == id_base + i: `sel` is a labels array of vc_cluster_radius*,
                                the survivors are the groups' representatives (of vc_leaders_radius*: the leaders; of
                                vc_dbscan_radius*: one representative per cluster and every noise record) */
/* new_ids (N words, may be NULL): new_ids[i] = the new GLOBAL id of old record id_base + i, or UINT32_MAX if it was removed -- the map
 * that carries labels, or any table keyed by id, across the call.  *n_kept (may be NULL) = K.
 * Afterwards vc_size == K, the survivors keep their relative order and survivor number j has global id id_base + j (ids stay ordinals
 * of the records in file order, build_hash_tables.cc:55,61,69).  capacity, id_base, flags and knobs are unchanged; the freed room
 * can be filled by vc_add_* again.  Every observable of the handle -- codes, every search with rows, counts, offsets and statistics,
 * clustering, the zero padding of the columns behind record K -- equals BIT FOR BIT that of a fresh handle of the same vc_config to
 * which the K surviving codes were added in order.
 * Index: a CURRENT index is filtered to the survivors (a bucket is an ascending id run and the renumbering is monotone, so the dead
 * entries are dropped and the ids translated; nothing is sorted) and is bit for bit the index vc_build_index builds from them,
 * derived structures chosen by the memory policy of a build of K records.  A STALE index (records added since it was built) serves
 * no one and is dropped, vc_build_index follows; no index before means no index after.  K == 0 drops the index (a store of nothing
 * has none): the handle equals a fresh empty one.  K == N changes nothing: new_ids is the identity, no column or index byte is
 * written.
 * Errors are checked before any work and leave the store, new_ids and *n_kept untouched: VC_ERR_INVALID for a null handle, null sel
 * with N > 0, kind > 1, new_ids overlapping sel.  N == 0 gives VC_OK and K = 0; nothing is read or written.
 * Device form: d_sel / d_new_ids are device memory.  Everything is enqueued on `stream`; the host waits inside the call (for K, which
 * sizes what follows, and per table as the MIH build waits).  When the call returns the store is in its new state for any later
 * call; d_new_ids is valid in stream order.
 * Failure: every allocation the column phase needs is made before the first column byte changes -- VC_ERR_NOMEM there leaves the store
 * as it was.  A failure in the index phase leaves the compacted records with NO index, never a half-filtered one; vc_build_index works
 * afterwards (the rule of vc_update_index).
 * Scratch: the keep bitmap (one bit per record), its rank directory, ONE scratch column (8 N bytes, the peak) and, per table, N + 1
 * scan words -- all call-scoped allocations, every word written before it is read.  The index object with its grow-only search
 * scratch and counters survives, as in vc_update_index. */
int vc_retain_dev(vc_engine* e, const uint32_t* d_sel, uint32_t kind, uint32_t* d_new_ids, uint64_t* n_kept, void* stream);
/* The same for sel / new_ids in host memory: the device form on the engine's stream plus the staged selection and the copy home of
 * the map; waits for them. */
int vc_retain(vc_engine* e, const uint32_t* sel, uint32_t kind, uint32_t* new_ids, uint64_t* n_kept);

/* "Which of my K codes is each record nearest to": the assign step of a vocabulary / coarse quantiser over the binary codes, and the
 * way to put records into EXISTING groups -- after vc_add_codes, `first = n_old, count = N - n_old` against the centroids of
 * vc_group_summary* is the companion of vc_update_index.  The reference has nothing of the kind; the call replaces a second handle
 * that holds the centres, vc_get_codes_dev and vc_search_knn_dev(k = 1, VC_MODE_LINEAR) in batches.
 * INPUT: centres, n_centres rows of bits / 8 bytes in the byte layout of vc_add_codes / the centroids of vc_group_summary* (8-byte
 * aligned in the device form); the records id_base + first .. id_base + first + count - 1 -- ordinals, used as n_labelled is.
 * OUTPUT: out[j] = c | (uint64_t)dist << 32 for record id_base + first + j: the project's packed result with the centre's INDEX in the
 * id field.  dist is the full Hamming distance to centre c, and c is the centre with the smallest (dist, index): a tie in distance
 * goes to the smaller index.  Hence out[j] is bit for bit row j of vc_search_knn(k = 1, VC_MODE_LINEAR) on a handle that holds the
 * centres with id_base = 0.
 * ERRORS, checked before any work, outputs untouched: VC_ERR_INVALID for a null handle, null centres, n_centres == 0, first + count >
 * N, null out with count > 0.  count == 0 returns VC_OK and nothing is read or written.  No index is needed and a stale one does not
 * matter: only the codes are read.
 * The result is a function of the codes, the centres and the range only: no knob, grid shape, shard layout or earlier call changes a
 * bit of it.
 * How: the transposed data flow of the verify kernel.  A thread keeps a few records in registers for the whole launch and the centres
 * stream past in LDS tiles (VC_ASSIGN_TILE, environment, read at vc_create: centres per tile, default all that fit in 16 KiB); per
 * pair and 64-bit word two XORs and two population counts, a strict < in ascending centre order.  When `count` is too small to fill
 * the device and the centres are many, they are cut into slices (VC_ASSIGN_SLICES forces their number) that meet in a 64-bit atomicMin
 * on `out`, set to all ones by an init launch -- the minimum of the packed value IS the (dist, index) rule, so this stays exact.
 * Device form: everything is enqueued on `stream`, the host waits for nothing; d_centres must stay untouched until the call has run.
 * The call is ordered behind the handle's previous call whatever its stream, like every call.  No scratch. */
int vc_assign_nearest_dev(vc_engine* e, const void* d_centres, uint32_t n_centres, uint64_t first, uint64_t count, uint64_t* d_out, void* stream);
/* The same for centres and out in host memory: the device form on the engine's stream on staged copies (a grow-only buffer of the
 * handle, shared with vc_kmajority's staging; every word written before it is read); waits for the result. */
int vc_assign_nearest(vc_engine* e, const void* centres, uint32_t n_centres, uint64_t first, uint64_t count, uint64_t* out);

/* A grouping with a CHOSEN number of groups: Lloyd iterations in Hamming space ("k-majority") over all N resident records -- assign
 * every record to the nearest centre (vc_assign_nearest), then move each centre to the per-bit majority of its members (the centroid
 * of vc_group_summary).  THE RULE, exact in integers:
 *   C = seeds; prev = none
 *   for t = 0 .. max_iters - 1:
 *       a = assign_nearest(C) over all N records; cost[t] = sum of dist(a)
 *       n_changed[t] = N if t == 0 else #{i : index(a[i]) != prev[i]};  n_iters = t + 1
 *       if n_changed[t] == 0: converged = 1; break
 *       for every centre c with at least one member in a: C[c] = per-bit STRICT majority of its members (a tie gives 0)
 *       a centre without a member keeps its code;  prev = index(a)
 *   assign = assign_nearest(C)            -- always: the returned pair satisfies assign == vc_assign_nearest(centres)
 *   labels[i] = id_base + index(assign[i]) -- a legal input of vc_group_summary* and, with its rep_labels, of vc_retain*
 * It terminates: the potential (sum of distances, sum of centre indices), ordered lexicographically, is never raised by an update in
 * its first term and is lowered strictly by an assign round that changes anything.
 * centres: in, the n_centres seeds (the caller chooses them; vc_seed_centres* below makes them on the device); out, the final centres.  assign: N
 * packed words.  labels: N words, may be NULL.  stats: host memory in both forms, may be NULL.
 * ERRORS, checked before any work, outputs untouched: VC_ERR_INVALID for a null handle, null centres or assign, n_centres == 0,
 * n_centres > N with N > 0 (the labels must be resident ids), max_iters > VC_KMAJ_MAX_ITERS.  N == 0 gives VC_OK and zero stats;
 * nothing is read or written.  max_iters == 0 is just the final assign: n_iters = 0, converged = 0.
 * Device form: everything is enqueued on `stream`; the host waits once per round for 16 bytes (cost and n_changed, reduced on the
 * device), once inside each update (vc_group_summary's wait) and once at the end for cost_final and n_empty.  Outputs are valid in
 * stream order.  Scratch: two grow-only buffers of the handle, this call's own (12 N bytes, 28 + bits / 8 bytes per centre, the
 * counters; the host form's staging), plus those of vc_group_summary*; every word written before it is read.
 * The result is a function of the codes and the seeds only: no knob, window, shard layout or earlier call changes a bit of it. */
#define VC_KMAJ_MAX_ITERS 64
typedef struct vc_kmajority_stats {      /* 1048 bytes */
  uint32_t n_iters, converged;           /* assign+update rounds run (<= max_iters); 1 = a round changed no assignment */
  uint64_t n_empty;                      /* centres without a member in the returned assignment */
  uint64_t cost_final;                   /* sum of the returned assignment's distances */
  uint64_t cost[VC_KMAJ_MAX_ITERS];      /* [t] = sum of distances of round t's assignment; 0 from n_iters on */
  uint64_t n_changed[VC_KMAJ_MAX_ITERS]; /* [t] = records whose centre index differs from round t-1's; [0] = N */
} vc_kmajority_stats;
int vc_kmajority_dev(vc_engine* e, uint32_t n_centres, uint32_t max_iters, void* d_centres, uint64_t* d_assign, uint32_t* d_labels,
                     vc_kmajority_stats* stats, void* stream);
/* The same for centres, assign and labels in host memory: the seeds staged, the device form on the engine's stream, the three arrays
 * come home; waits for them. */
int vc_kmajority(vc_engine* e, uint32_t n_centres, uint32_t max_iters, void* centres, uint64_t* assign, uint32_t* labels,
                 vc_kmajority_stats* stats);

/* Seeds for vc_kmajority* made on the device: K sequential rounds over all N resident records, one small launch each, no byte home.
 * Two standard seedings, both exact in integers.  VC_SEED_FARTHEST is the farthest-first traversal (Gonzalez, the 2-approximation of
 * k-centre); it is deterministic but for its first record, and its pick distances are the covering radii one reads to choose K.
 * VC_SEED_WEIGHTED samples a record with probability proportional to its Hamming distance to the nearest chosen seed -- for bit
 * vectors the squared Euclidean distance, so this is k-means++ for the cost vc_kmajority minimises.  THE RULE:
 *   N resident records with local index i; d(i, c) is the full Hamming distance; draw(t) is output number t (from 0) of SplitMix64
 *   started at the caller's `seed`: state x starts at seed, every output does x += 0x9E3779B97F4A7C15; z = x;
 *   z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; return z ^ z >> 31 -- all mod 2^64.
 *   best[i] = (dist = infinity, index = none) for every i
 *   s_0 = draw(0) % N ;  pick_dist_0 = 0
 *   for t = 0 .. K-1:
 *       centre t = code of record s_t
 *       for every i: if d(i, s_t) < dist(best[i]): best[i] = (d(i, s_t), t)      -- strict: the earlier seed keeps a tie
 *       if t == K-1: break
 *       VC_SEED_FARTHEST:  s_{t+1} = the i with the largest dist(best[i]), the SMALLEST i on a tie
 *       VC_SEED_WEIGHTED:  total = sum_i dist(best[i])
 *                          if total == 0: s_{t+1} = 0
 *                          else: target = draw(t+1) % total; s_{t+1} = the smallest i with sum_{j<=i} dist(best[j]) > target
 *       pick_dist_{t+1} = dist(best[s_{t+1}])           -- before seed t+1 is applied
 * OUTPUT: centres[t], K rows of bits / 8 bytes, the layout vc_kmajority takes as seeds (8-byte aligned in the device form).
 * picks[t] = (id_base + s_t) | pick_dist_t << 32, the project's packed word; may be NULL.  assign[i] = index | dist << 32 of best[i]
 * after the last seed; may be NULL.  stats: host memory in both forms, may be NULL; cost = the sum of dist(best), radius = its
 * maximum, n_zero_picks = #{t >= 1 : pick_dist_t == 0}.
 * Hence assign == vc_assign_nearest(centres) bit for bit (the same strict < in ascending index); in the farthest mode pick_dist_t
 * never rises for t >= 1 and radius <= pick_dist_{K-1}; a record at distance 0 from a seed is never picked while any record is
 * farther, and once every record coincides with a seed both methods pick record 0 at distance 0.
 * ERRORS, checked before any work, outputs untouched: VC_ERR_INVALID for a null handle, null centres, n_centres == 0, n_centres > N
 * with N > 0, a method other than the two.  N == 0 gives VC_OK and zero stats; nothing is read or written.  No index is needed and a
 * stale one does not matter: only the codes are read.
 * The result is a function of the codes, K, the method and `seed` only: no knob, grid shape, shard layout or earlier call changes a
 * bit of it.
 * How: a pick travels between launches as dist << 32 | (0xFFFFFFFF - i).  The round launch reads it, range-checks i, loads that
 * record's code (wave-uniform), records it into centres / picks, lowers best over its block's contiguous records and reduces the new
 * best: farthest, the blocks' maxima of that word meet in 64-bit atomicMax -- the maximum IS the rule -- spread over 16 words on
 * cache lines of their own, of which the next launch takes the maximum (a thousand blocks on one address measured 10 us a round);
 * weighted, a sum per block, from which a one-block pick launch finds the block and then the record that cross the target.  A last
 * launch reduces the statistics.  Blocks hand off only through atomics or through stores that a later launch reads.
 * Device form: everything is enqueued on `stream`; with stats == NULL the host waits for nothing, otherwise once, at the end, for 16
 * bytes; there is no wait per round.  The call is ordered behind the handle's previous call whatever its stream, like every call.
 * Scratch: two grow-only buffers of the handle, this call's own (8 K + 6 160 bytes, 4 bytes per 1024 records, 8 N bytes when
 * d_assign is NULL -- else best lives in d_assign; the host form's staging); every word written before it is read. */
#define VC_SEED_FARTHEST 0u
#define VC_SEED_WEIGHTED 1u
typedef struct vc_seed_stats {           /* 16 bytes */
  uint64_t cost;                         /* sum of dist(best) after the last seed */
  uint32_t radius, n_zero_picks;         /* max of dist(best); picks t >= 1 at distance 0 */
} vc_seed_stats;
int vc_seed_centres_dev(vc_engine* e, uint32_t n_centres, uint32_t method, uint64_t seed, void* d_centres, uint64_t* d_picks,
                        uint64_t* d_assign, vc_seed_stats* stats, void* stream);
/* The same for centres, picks and assign in host memory: the device form on the engine's stream into staged outputs, which come
 * home; waits for them. */
int vc_seed_centres(vc_engine* e, uint32_t n_centres, uint32_t method, uint64_t seed, void* centres, uint64_t* picks,
                    uint64_t* assign, vc_seed_stats* stats);

/* ---- one result per label group in k-NN search ----------------------------------------------------------------------------------
 * replaces: search_image_by_id / SearchWorker::find (image_search_client.h:12-27, search_worker.cc:65-89) for a front end that wants
 * the k nearest DISTINCT pictures: on near-duplicate-heavy data the plain top-k row is mostly copies of a few of them.  The
 * reference has no such call; the host loop it would take -- search with a guessed larger k, copy rows and labels home, collapse,
 * repeat -- is what this replaces.  Exact, batched; rows and labels never leave HBM in the device form.
 * labels: one uint32 per resident record, indexed by id - id_base (N = vc_size entries).  Only EQUALITY of two values matters: 0 and
 * 0xFFFFFFFF are labels like any other, nothing is validated.  The output of every grouper qualifies (vc_cluster_radius*,
 * vc_leaders_radius*, vc_dbscan_radius*, one level of the *_levels* calls, vc_kmajority*'s labels), and so does group_index of
 * vc_group_summary*, a class id or a user's album id.
 * RULE.  For a query q the HEAD of label L is the smallest packed (dist << 32 | id) over the records with label L.  Row i is the k
 * smallest heads of query i, ascending, padded with UINT64_MAX.  Equivalently: walk the ascending k-NN list of q and keep an entry
 * iff no earlier entry has its label -- the form the implementation takes, in ROUNDS:
 *   round j runs the UNCHANGED k-NN search (vc_search_knn_dev) at k'_j for the queries still unfinished, collapses each row of k'_j
 *   entries to the first occurrences of its labels and counts them, d.  A query is FINISHED when d >= k (its row: the first k kept
 *   entries, count k) or when the search returned fewer than k'_j entries (the database is exhausted: the row holds every group,
 *   count = d < k).  Otherwise it goes to round j + 1 with k'_{j+1} = min(VC_MAX_K, 2 k'_j).  A query still unfinished at
 *   k' = VC_MAX_K is TRUNCATED -- more than 8192 records of fewer than k groups lie nearest to it -- and gets the d heads found and
 *   count = d | VC_DISTINCT_TRUNCATED.  A count of UINT32_MAX from the search underneath (its ring-overflow recovery gave up, see
 *   vc_device_status) is passed on as it is, with the collapsed upper-bound row.
 * k_first sets k'_0; 0 means min(VC_MAX_K, 2 k), any other value must lie in k .. VC_MAX_K.  A finished row is THE SAME for every
 * k_first: a top-k' prefix that holds k distinct labels holds the k nearest heads as its first occurrences (a head not in the prefix
 * is farther than all k' entries).  k_first is a tuning knob only; the statistics differ.
 * This holds wherever the rows underneath are the true nearest records: VC_MODE_LINEAR always, VC_MODE_MIH_EXACT without
 * VC_FLAG_REF_SIGNEXT_KEYS and without VC_FLAG_REF_STOP_LITERAL4 at n_tables < 4.  Under those flags the row is the collapse of the
 * row the underlying call returns at the final k'.  VC_MODE_MIH_APPROX is refused: its 20 k candidate rule has no meaning for groups.
 * THE SURE PREFIX (VC_MODE_MIH_EXACT).  A row of exact MIH has the true distances and every record nearer than its last distance D,
 * but of the records that tie at D only some -- genuine ones, not necessarily the smallest ids (vc_search_knn's contract: "among the
 * items the mode's loop has seen").  A head taken from those ties could be the wrong member, or the wrong group, of its distance.
 * So in this mode a FULL row of a round with k' < VC_MAX_K counts only up to the entries nearer than D: d is the number of distinct
 * labels among those, and a query with d < k goes on.  A row that is not full holds the whole database and counts whole.  Rows, row
 * labels and counts are then word for word those of VC_MODE_LINEAR, for every k_first; n_rounds and n_searched can be larger than
 * there.  At k' = VC_MAX_K no wider row exists and the whole row counts: an entry at its last distance is a genuine member of a
 * genuine group of that distance, as in vc_search_knn.
 * OUTPUT: d_out nq * k packed; d_row_labels (nq * k, may be NULL) the label of every entry, 0 past the count; d_counts (nq, may be
 * NULL); stats (HOST memory in both forms, may be NULL).
 * ERRORS, checked before any work, outputs untouched: VC_ERR_INVALID for a null handle, queries, labels or out, nq == 0, k outside
 * 1 .. VC_MAX_K, a bad k_first, an approximate or unknown mode, a bad order (host form); VC_ERR_STATE in MIH mode without a current
 * index (a stale one counts as none).  N == 0 gives VC_OK with counts 0, padded rows and zero stats.
 * WAITS.  The device form makes the host wait ONCE PER ROUND, for the number of unfinished queries (24 bytes) -- in VC_MODE_LINEAR
 * too, where vc_search_knn_dev itself waits for nothing; the MIH mode's own waits inside the search come on top.  Results are valid
 * in stream order.
 * How: the collapse kernel has a form per size class of k' -- up to 64 entries one wave per query without LDS; above, one block per
 * query with the row's labels and a first-occurrence table of row positions in LDS (no label value is reserved as a marker); the
 * kept entries are placed by ballot and block sums, never by the order of atomics.  The retry list is the exclusive scan of a flag
 * per query, so it is ascending; a gather kernel compacts the retry queries; later rounds write straight into d_out through an
 * index map.  Hence every output word is a function of the database, the labels and the call only.
 * Scratch: three grow-only buffers of the handle, this call's own; every word written before it is read.  The k' rows of a round
 * take at most VC_DISTINCT_SCRATCH bytes (environment, read at vc_create; default 64 MiB; always at least one row): a round of n
 * queries runs in sub-batches of max(1, budget / (8 k')) queries, so a 4096-query call does not allocate 256 MiB at k' = 8192. */
#define VC_DISTINCT_TRUNCATED 0x80000000u
typedef struct vc_distinct_stats {   /* 32 bytes */
  uint32_t n_rounds;      /* search rounds run (>= 1 for nq > 0) */
  uint32_t k_last;        /* k' of the last round */
  uint64_t n_searched;    /* queries summed over rounds */
  uint64_t n_truncated;   /* queries that ended with VC_DISTINCT_TRUNCATED */
  uint64_t n_short;       /* queries that finished with count < k because the database holds fewer groups */
} vc_distinct_stats;
int vc_search_knn_distinct_dev(vc_engine* e, const void* d_queries, uint32_t nq, uint32_t k, uint32_t mode, const uint32_t* d_labels,
                               uint32_t k_first, uint64_t* d_out, uint32_t* d_row_labels, uint32_t* d_counts, vc_distinct_stats* stats,
                               void* stream);
/* The same for queries, labels and results in host memory: queries and the N labels are staged on the engine's stream ON EVERY CALL,
 * the device form runs into staged outputs, which come home; waits for them.  order as vc_search_knn: VC_ORDER_FARTHEST_FIRST
 * reverses the valid part of every row (and of its labels).  Callers who search repeatedly should keep the labels in HBM and use
 * the device form. */
int vc_search_knn_distinct(vc_engine* e, const void* queries, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order,
                           const uint32_t* labels, uint32_t k_first, uint64_t* out, uint32_t* row_labels, uint32_t* counts,
                           vc_distinct_stats* stats);

/* ---- k-NN among the records a filter allows: vc_search_knn_filtered* --------------------------------------------------------------------
 * "The k nearest among the records I allow": search only among the leaders or representatives of a grouper without cutting the
 * store down with vc_retain*; inside one album, class or cluster, or everywhere but in it; under a caller's keep mask (tombstones,
 * tenants, a date range computed elsewhere).  The reference has no such call; the host loop it would take -- search with a guessed
 * larger k, copy rows home, filter, repeat -- runs into VC_MAX_K for a selective filter and then has no exact answer at all.
 * THE FILTER is shared by all queries of the call (a filter per query is out of scope) (see vc_search_knn_scoped*).  Record i has global id id_base + i:
 *   VC_FILTER_MASK       sel[i] != 0                                                         N words
 *   VC_FILTER_ROOTS      sel[i] == id_base + i (a grouper's labels: one representative per   N words
 *                        group, as VC_RETAIN_ROOTS)
 *   VC_FILTER_EQUAL      sel[i] == value                                                     N words
 *   VC_FILTER_NOT_EQUAL  sel[i] != value                                                     N words
 *   VC_FILTER_BITS       bit i & 31 of sel[i >> 5]                                           ceil(N / 32) words; the bits of the last
 *                                                                                            word past N are ignored
 * `value` is read only by EQUAL and NOT_EQUAL.  Every 32-bit value is legal in sel and in value; nothing is validated but the kind.
 * THE RULE.  Row q holds the k smallest packed (dist << 32 | id) over the ALLOWED records, ascending, padded with UINT64_MAX;
 * counts[q] = min(k, A), A the number of allowed records.  Ties go to the smaller id: the linear scan's order.  Every output word
 * is a function of the codes, the filter and the call: not of mode, k_first, the route taken, the environment knobs below or what
 * earlier calls left in the handle.  There is no truncation flag: the call is exact for every A from 0 to N.  A count of UINT32_MAX
 * from the search underneath (its ring-overflow recovery gave up, see vc_device_status) is passed on as in vc_search_knn_distinct*.
 * MODES.  VC_MODE_LINEAR and VC_MODE_MIH_EXACT.  VC_MODE_MIH_APPROX is refused, and so is VC_MODE_MIH_EXACT on a handle with
 * VC_FLAG_REF_SIGNEXT_KEYS, or with VC_FLAG_REF_STOP_LITERAL4 at n_tables < 4: the rows underneath are not the true nearest
 * records there, so the result would depend on the route.
 * HOW.  sel becomes a bit per record and a rank directory (the keep set of vc_retain*); one host wait fetches A.  Then one of
 *   the POST-FILTER route (dense filters; keeps the speed of the index): rounds as in vc_search_knn_distinct* -- the UNCHANGED search
 *     at k' for the open queries, a strip kernel keeps the allowed entries of each row (under exact MIH only below the row's last
 *     distance, the sure prefix).  A query is finished with k kept entries or a row that was not full; else k' doubles up to
 *     VC_MAX_K, and a query still open there goes to the other route.  k_first sets k'_0; 0 means clamp(2 ceil(k N / A), k, VC_MAX_K).
 *     One host wait per round.
 *   the PRE-FILTER route (sparse filters, and the fallback): the allowed ids are listed ascending and taken in windows of
 *     VC_FILTER_WINDOW ids (default 2^20); a window's codes are gathered by id and scanned by brute force -- a histogram of the
 *     distances gives the k-th distance of every query, a count and a place walk put exactly the min(k, n) smallest (distance, id)
 *     into the row -- and the rows of further windows are merged in.  Exact for every A, no waits.
 * The plan takes the post-filter route when 2 ceil(k N / A) <= VC_FILTER_POST_MAX_K (vc_filter_plan.hpp), else the pre-filter route
 * answers the whole batch.  Environment, read once at vc_create: VC_FILTER_ROUTE (0 the plan's, 1 post-filter first, 2 pre-filter
 * only; tests and A/B runs), VC_FILTER_SCRATCH (bytes per sub-batch of k' rows and of per-slice counters, default 64 MiB, always
 * at least one query), VC_FILTER_WINDOW.
 * OUTPUT: d_out nq * k packed; d_counts (nq, may be NULL); stats (HOST memory in both forms, may be NULL).
 * ERRORS, checked before any work, outputs and stats untouched: VC_ERR_INVALID for a null handle, queries, sel or out, nq == 0, k
 * outside 1 .. VC_MAX_K, a bad k_first (0, or k .. VC_MAX_K), an unknown kind or mode, a refused mode, a bad order (host form);
 * VC_ERR_STATE in MIH mode without a current index (a stale one counts as none).  N == 0 gives VC_OK with counts 0, padded rows and
 * zero stats.
 * Scratch: grow-only buffers of the handle, this call's own; every word is written before it is read. */
#define VC_FILTER_MASK 0u
#define VC_FILTER_ROOTS 1u
#define VC_FILTER_EQUAL 2u
#define VC_FILTER_NOT_EQUAL 3u
#define VC_FILTER_BITS 4u
#define VC_FILTER_RAN_POST 1u
#define VC_FILTER_RAN_PRE 2u
typedef struct vc_filter_stats {   /* 48 bytes */
  uint64_t n_allowed;   /* A */
  uint32_t routes;      /* VC_FILTER_RAN_POST 1 | VC_FILTER_RAN_PRE 2 */
  uint32_t n_rounds;    /* post-filter search rounds run */
  uint32_t k_last;      /* k' of the last round, 0 without one */
  uint32_t n_windows;   /* subset windows scanned by the pre-filter route (per sub-batch of queries) */
  uint64_t n_searched;  /* queries summed over post-filter rounds */
  uint64_t n_fallback;  /* queries the post-filter rounds handed to the pre-filter route */
  uint64_t n_short;     /* queries with count < k (A < k) */
} vc_filter_stats;
int vc_search_knn_filtered_dev(vc_engine* e, const void* d_queries, uint32_t nq, uint32_t k, uint32_t mode, const uint32_t* d_sel,
                               uint32_t kind, uint32_t value, uint32_t k_first, uint64_t* d_out, uint32_t* d_counts,
                               vc_filter_stats* stats, void* stream);
/* The same for queries, sel and results in host memory: queries and sel are staged on the engine's stream ON EVERY CALL, the device
 * form runs into staged outputs, which come home; waits for them.  order as vc_search_knn: VC_ORDER_FARTHEST_FIRST reverses the
 * valid part of every row.  Callers who search repeatedly should keep sel in HBM, preferably as VC_FILTER_BITS (N / 8 bytes), and
 * use the device form. */
int vc_search_knn_filtered(vc_engine* e, const void* queries, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order,
                           const uint32_t* sel, uint32_t kind, uint32_t value, uint32_t k_first, uint64_t* out, uint32_t* counts,
                           vc_filter_stats* stats);

/* ---- k-NN inside each query's own scope: vc_search_knn_scoped* -----------------------------------------------------------------------------
 * "The k nearest records of MY tenant, album, class or cluster", for a batch in which every query brings its own value: a service
 * that batches the queries of many tenants, a labelling pass that asks for the nearest pictures of the same album for thousands of
 * pictures, a search inside a grouper's clusters.  With vc_search_knn_filtered* such a batch falls apart into one call -- one keep
 * set over all N records and one host wait -- per distinct value; this call answers it at once.
 * THE SCOPES.  scope holds N words, record i (global id id_base + i) carries scope[i]; qscope holds nq words, query q carries
 * qscope[q].  Every 32-bit value is legal in both arrays, 0, 0x80000000 and 0xFFFFFFFF included; nothing is validated.
 * THE RULE.  Row q holds the k smallest packed (dist << 32 | id) over the records with scope[i] == qscope[q], ascending, padded with
 * UINT64_MAX; counts[q] = min(k, S_q), S_q the number of records that carry the query's value -- 0 when none does.  Ties go to the
 * smaller id.  Every output word is a function of the codes, scope, qscope, the queries and k: not of the order of the queries, of
 * the other queries of the call, of the environment knobs below or of what earlier calls left in the handle.  Row q equals, word
 * for word, row 0 of vc_search_knn_filtered* called with VC_FILTER_EQUAL, value = qscope[q], VC_MODE_LINEAR and that one query.
 * There is no truncation flag and no mode argument: the call is exact brute force over the scope and needs no index.
 * flags is reserved and must be 0.  OUT OF SCOPE: VC_FILTER_NOT_EQUAL per query ("everywhere but my group") is a dense filter, which
 * needs the post-filter rounds of vc_search_knn_filtered*; and a form for queries named by id.
 * HOW.  The pairs (qscope[q], q) are sorted: the U distinct values ascending are the slots.  One pass over scope sets the bit of every
 * record whose value is one of them (a binary search) in a keep set; a host wait fetches U and A, the number of matched records.
 * Records that no query names cost nothing after this pass.  The A ids are listed ascending with their slots and sorted by slot with a
 * stable radix sort: slots ascend in the list and ids ascend within a slot, so every scope is a segment in id order.  A second host
 * wait fetches the segment table, 2 (U + 1) words.  The list is taken in windows of VC_SCOPE_WINDOW positions (default 2^20, 0 or
 * above 2^24 means the default) whose codes are gathered by id; a wave holds a slice of the window in registers and loops over the
 * sorted queries of the slots its slice touches, a pair counting only where the position's slot is the query's.  The selection is
 * the three walks of vc_search_knn_filtered*'s pre-filter route -- histogram, counts, placement by rank -- over per-(query, slice)
 * counters that a query owns only for the slices its segment touches; the queries are sub-batched so that these counters stay under
 * VC_SCOPE_SCRATCH bytes (default 64 MiB, always at least one query).  A segment that straddles windows has its rows merged.  Both
 * knobs are read once at vc_create.  COST: a slice that holds many tiny scopes computes a slice's worth of distances for every query of
 * its range although only the matching ones count; stats.n_pairs is the number the answer needs.
 * OUTPUT: d_out nq * k packed; d_counts (nq, may be NULL); stats (HOST memory in both forms, may be NULL).
 * ERRORS, checked before any work, outputs and stats untouched: VC_ERR_INVALID for a null handle, queries, scope, qscope or out,
 * nq == 0, k outside 1 .. VC_MAX_K, flags != 0, a bad order (host form).  N == 0 gives VC_OK with counts 0, padded rows and zero
 * stats.
 * Scratch: grow-only buffers of the handle, this call's own; every word is written before it is read. */
typedef struct vc_scope_stats {   /* 40 bytes */
  uint64_t n_matched;   /* A: records whose scope some query of the call names */
  uint64_t n_pairs;     /* sum over the queries of S_q: the distances the answer needs */
  uint32_t n_scopes;    /* U: distinct values in qscope */
  uint32_t n_windows;   /* windows of the sorted list scanned (per sub-batch of queries) */
  uint64_t n_short;     /* queries with count < k */
  uint64_t n_empty;     /* queries with S_q == 0 */
} vc_scope_stats;
int vc_search_knn_scoped_dev(vc_engine* e, const void* d_queries, uint32_t nq, uint32_t k, const uint32_t* d_scope,
                             const uint32_t* d_qscope, uint32_t flags, uint64_t* d_out, uint32_t* d_counts, vc_scope_stats* stats,
                             void* stream);
/* The same for queries, scope, qscope and results in host memory: all three inputs are staged on the engine's stream ON EVERY CALL,
 * the device form runs into staged outputs, which come home; waits for them.  order as vc_search_knn: VC_ORDER_FARTHEST_FIRST
 * reverses the valid part of every row.  Callers who search repeatedly should keep scope in HBM and use the device form. */
int vc_search_knn_scoped(vc_engine* e, const void* queries, uint32_t nq, uint32_t k, uint32_t order, const uint32_t* scope,
                         const uint32_t* qscope, uint32_t flags, uint64_t* out, uint32_t* counts, vc_scope_stats* stats);

/* ---- the exact k-NN graph of the store: vc_knn_graph* -------------------------------------------------------------------------------------
 * "For every resident record its k nearest other records": the input of UMAP / t-SNE maps, label propagation, hubness checks and
 * density-adaptive grouping (vc_cluster_knn* below).  The reference has no such call.  The host loop over vc_search_knn_ids_dev with
 * VC_IDS_EXCLUDE_SELF does not give a usable graph: under VC_MODE_MIH_EXACT the members of a row at its last distance are genuine but
 * not necessarily the smallest ids, so "j lists i" is not a function of the database; and every batch is a host round trip.
 * THE RULE.  The call covers the positions p in [first, first + count); count == 0 means "to the end" (as vc_assign_nearest).  Row
 * p - first holds the k smallest packed (dist << 32 | id) over all resident records OTHER than record id_base + p itself, ascending,
 * padded with UINT64_MAX; d_counts[p - first] = min(k, N - 1).  Ties go to the smaller id.  Duplicates of the record are ordinary
 * neighbours at distance 0.  Rows and counts are THE SAME WORDS in VC_MODE_LINEAR and VC_MODE_MIH_EXACT, for every batch, every
 * k_first and both handle kinds: a function of the database, k and the range only.  VC_MODE_MIH_APPROX is refused.
 * This holds wherever the rows underneath are the true nearest records: VC_MODE_LINEAR always, VC_MODE_MIH_EXACT without
 * VC_FLAG_REF_SIGNEXT_KEYS and without VC_FLAG_REF_STOP_LITERAL4 at n_tables < 4.  Under those flags a row is what the rule below
 * makes of the rows the underlying call returns.
 * k lies in 1 .. VC_MAX_K - 1.  batch: ids per search underneath, 0 means 4096, any value >= 1 is legal.
 * HOW.  Per batch of ids: the ids are made and their codes gathered on the device; then ROUNDS of the UNCHANGED k-NN search
 * (vc_search_knn_dev) at k', and after each a settle kernel that judges every row:
 *   - the entry equal to (uint64)own id -- distance 0, own id -- is dropped BY VALUE (binary search; vc_search_knn_ids' rule: with
 *     more than k' - 1 duplicates of smaller id it is not in the row at all);
 *   - a row that is not full (count < k') holds the whole store and is SETTLED;
 *   - VC_MODE_LINEAR runs one round at k' = k + 1, whose full rows are settled: the scan's order is (dist, id);
 *   - VC_MODE_MIH_EXACT starts at k' = k_first (0 means min(VC_MAX_K, 2 (k + 1)); any other value must lie in k + 1 .. VC_MAX_K)
 *     and doubles k' up to VC_MAX_K.  A full row is settled only if at least k entries other than the own record lie BELOW the
 *     row's last distance D -- the sure prefix of vc_search_knn_distinct*: the row holds every record nearer than D, of the ties
 *     at D only some.  A count above k', or of UINT32_MAX, is an unsettled full row.  (So k_first = k + 1 is legal but settles
 *     no full row: the last of k + 1 entries lies AT D, at most k - 1 others below it.  k + 2 is the smallest k' that can.);
 *   - a settled query gets its first k stripped entries and its count, written straight into the caller's rows; the others form the
 *     next round's list (an exclusive scan of a flag per query and a compacting gather: ascending, independent of block order);
 *   - a query still unsettled at k' = VC_MAX_K -- more than about 8191 records tie at or below its k-th distance -- is answered by
 *     the store's LINEAR k-NN at k + 1 and settled by the same kernel.  There is no truncation flag; stats.n_linear counts them.
 * A linear row whose count is UINT32_MAX (the scan's ring-overflow recovery gave up, see vc_device_status) is passed on as it is,
 * stripped, with that count, and counted in stats.n_gave_up; the host form answers such rows again through the handle's host k-NN.
 * The k' rows of a round take at most VC_KGRAPH_SCRATCH bytes (environment, read at create; default 64 MiB; always at least one
 * row): a round runs in sub-batches of max(1, budget / (8 k')) queries.
 * OUTPUT: d_rows count * k packed; d_counts (count words, may be NULL); stats (HOST memory in both forms, may be NULL).
 * ERRORS, checked before any work, outputs untouched: VC_ERR_INVALID for a null handle or rows, k outside 1 .. VC_MAX_K - 1, a bad
 * k_first, an approximate or unknown mode, first + count > N; VC_ERR_STATE in MIH mode without a current index.  N == 0, or an empty
 * range (first == N), gives VC_OK and zero stats.
 * WAITS.  VC_MODE_MIH_EXACT: once per round of a batch, for the length of the retry list (4 bytes), on top of the search's own; both
 * modes: once at the end for the statistics when stats is given.  Results are valid in stream order.
 * Scratch: grow-only buffers of the handle, this call's own; every word is written before it is read. */
typedef struct vc_knn_graph_stats {   /* 32 bytes */
  uint32_t n_rounds_max;  /* the most searches any record went through (the LINEAR answer after VC_MAX_K counts as one) */
  uint32_t k_last;        /* the largest k' any round ran at (k + 1 in VC_MODE_LINEAR) */
  uint64_t n_searched;    /* queries summed over the rounds of the mode's own search */
  uint64_t n_linear;      /* VC_MODE_MIH_EXACT: queries answered by the LINEAR k-NN after k' = VC_MAX_K */
  uint64_t n_gave_up;     /* rows the linear scan passed on with count UINT32_MAX */
} vc_knn_graph_stats;
int vc_knn_graph_dev(vc_engine* e, uint32_t k, uint32_t mode, uint32_t batch, uint64_t first, uint64_t count, uint32_t k_first,
                     uint64_t* d_rows, uint32_t* d_counts, vc_knn_graph_stats* stats, void* stream);
/* The same for rows and counts in host memory: nothing is staged but the outputs, which come home; waits for them.  There is no
 * `order` argument: graph rows are always ascending. */
int vc_knn_graph(vc_engine* e, uint32_t k, uint32_t mode, uint32_t batch, uint64_t first, uint64_t count, uint32_t k_first,
                 uint64_t* rows, uint32_t* counts, vc_knn_graph_stats* stats);

/* ---- a built k-NN graph after an append: vc_knn_graph_update* -----------------------------------------------------------------------------
 * vc_knn_graph* is the most expensive call of the library; after vc_add_codes of a few records to a large store this call brings a
 * built graph up to date without building it again.
 * PRECONDITION.  d_rows has room for N * k words and d_counts for N words, N the resident count now.  The first n_old rows and counts
 * are what vc_knn_graph* wrote when the store held exactly its first n_old records, over the full range, with this k; the records
 * [n_old, N) were appended since.  d_counts may be NULL: every old row then holds min(k, n_old - 1) entries, and no counts are
 * written.  In VC_MODE_MIH_EXACT the index must be current: the caller has run vc_update_index (or vc_build_index).
 * POSTCONDITION.  Rows and counts [0, N) are THE SAME WORDS as vc_knn_graph*(first = 0, count = N) writes for this store with this k,
 * in both modes, for every batch, k_first, window size, old-batch size and scratch budget, on both handle kinds -- under vc_knn_graph*'s
 * clause for the reference-fidelity flags, which governs the new records' rows.
 * k, mode, batch and k_first mean what they mean to vc_knn_graph* and govern the new records' rows only; the join below has no mode.
 * HOW.  1. The rows of the new records are vc_knn_graph* over [n_old, N), unchanged.  2. Old row i changes only where a new record j
 * has (dist(i, j) << 32 | id_j) < T_i, with T_i = row_i[k - 1] for a full row and UINT64_MAX otherwise: a threshold join of the old
 * records against the new ones, no search.  The new records' codes are gathered once.  The old records go by batches of
 * VC_KGRAPH_OLD_BATCH ids (environment, read at create; default 2^18; 0 or above 2^24 means the default), each against WINDOWS of
 * VC_KGRAPH_WINDOW new records (default 1024; 0 or above 2^20 means the default).  Per (old batch, window): a count pass of the join
 * kernel (old records in registers with their thresholds, read from the rows as they are now, so they tighten from window to window;
 * the window's codes in LDS tiles read as broadcasts); ONE WAIT of 16 bytes for the hits H and the affected records; if the hit list
 * of 8 H bytes exceeds VC_KGRAPH_SCRATCH and the window holds more than one record, the window is cut in half -- for the rest of this
 * old batch -- and counted again; two exclusive scans and a compacting gather (offsets, the ascending list of affected records); the
 * fill pass, which writes every record's hits at its own offset without atomics and which a block without a hit leaves at once; a
 * merge, one wave per affected record, that places the k smallest of row_i and its hits by rank counting into out-of-place rows
 * (sub-batches of max(1, VC_KGRAPH_SCRATCH / (8 k)) records), and a copy back.  3. One wait at the end for the stats and the error word.
 * STATS (HOST memory in both forms, may be NULL).  n_rows_changed and n_inserted are functions of the database, n_old and k only;
 * n_hits (the hits of the accepted count pass of every window), n_windows and n_halvings depend on the three knobs as well.
 * DEGENERATE.  n_old == N: VC_OK, nothing written, zero stats.  n_old == 0: a plain build.
 * ERRORS, checked before any work, outputs untouched: VC_ERR_INVALID for a null handle or rows, k outside 1 .. VC_MAX_K - 1, a bad
 * k_first, an approximate or unknown mode, n_old > N; VC_ERR_STATE in MIH mode without a current index (a stale index after
 * vc_add_codes counts as none).  An old count above k (UINT32_MAX included) is found ON THE DEVICE and gives VC_ERR_INVALID --
 * vc_cluster_knn*'s protocol: the error word comes home with the stats; THE OUTPUTS ARE THEN UNDEFINED.
 * Not offered: a form for vc_retain* in this call (a row that listed a removed record may need a search: that form is
 * vc_knn_graph_retain* below), graphs over a part of the range, and an automatic switch to a rebuild when the append is large -- the join costs n_old * n_new pair-words, which the caller weighs.
 * Scratch: grow-only buffers of the handle, this call's own; every word is written before it is read. */
typedef struct vc_knn_graph_update_stats {   /* 64 bytes */
  vc_knn_graph_stats build;   /* of the new records' rows: vc_knn_graph* over [n_old, N) */
  uint64_t n_rows_changed;    /* old rows of which at least one word changed */
  uint64_t n_inserted;        /* entries of old rows, after the call, whose id is a new record's */
  uint64_t n_hits;            /* pairs that passed a threshold, summed over the windows (depends on the knobs) */
  uint32_t n_windows;         /* (old batch, window) count passes run, retried ones included */
  uint32_t n_halvings;        /* windows cut in half because their hits exceeded the scratch budget */
} vc_knn_graph_update_stats;
int vc_knn_graph_update_dev(vc_engine* e, uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first,
                            uint64_t* d_rows, uint32_t* d_counts, vc_knn_graph_update_stats* stats, void* stream);
/* The same for rows and counts in host memory: the old rows and counts are staged up, all N rows and counts come home; waits for
 * them.  A new row that the linear scan passed on with count UINT32_MAX is answered again as vc_knn_graph does it. */
int vc_knn_graph_update(vc_engine* e, uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first,
                        uint64_t* rows, uint32_t* counts, vc_knn_graph_update_stats* stats);

/* ---- a built k-NN graph after a removal: vc_knn_graph_retain* ------------------------------------------------------------------------------
 * The other half of the store's life cycle: after vc_retain* swept tombstones, a grouper's duplicates or one tenant out of a large
 * store, this call brings a built graph up to date without building it again.
 * PRECONDITION.  vc_retain* has run; n_old is the record count before it and d_new_ids (n_old words) the map it wrote.  d_rows
 * (n_old * k words) and d_counts (n_old words) are what vc_knn_graph* wrote, over the full range and with this k, for the store as it
 * was before the removal.  d_counts may be NULL: every old row then holds min(k, n_old - 1) entries, and no counts are written.  In
 * VC_MODE_MIH_EXACT the index must be current; vc_retain* leaves a current index current.
 * POSTCONDITION.  K = vc_size now.  Rows and counts [0, K) are THE SAME WORDS as vc_knn_graph*(first = 0, count = K) writes for the
 * store now with this k, in both modes, for every batch, k_first and scratch budget, on both handle kinds -- under vc_knn_graph*'s
 * clause for the reference-fidelity flags, which governs the repaired rows.  Rows and counts [K, n_old) are unspecified afterwards.
 * Nothing outside the two buffers is written.
 * k, mode, batch and k_first mean what they mean to vc_knn_graph* and govern the repaired rows only; the translation has no mode.
 * WHY.  vc_retain* renumbers the survivors monotonically, so the order of (dist << 32 | id) among survivors is the same before and
 * after.  An old row whose entries all survive is, once its ids are translated, word for word the row a rebuild writes.  If some
 * entries died, the m that survive are exactly the m smallest entries of the rebuilt row, because every record the old row did not
 * list lies at or above the row's last entry.  Such a row is wrong only if it became SHORT: m < min(k, K - 1).  A row that held the
 * whole old store (count < k) holds the whole new store after the drop and is never short.
 * HOW.  1. The map is checked once: a live flag per word, an exclusive scan, and every live word compared with id_base + its rank.
 * 2. The old rows go by CHUNKS of max(1, VC_KGRAPH_SCRATCH / (8 k)) rows in ascending order.  The translate kernel skips the row of a
 * removed record, reads every entry's new id straight from the map, repacks the live entries as dist << 32 | new id in their old
 * order, pads the tail with UINT64_MAX and writes the row OUT OF PLACE with its new count; a copy puts the chunk's rows back at their
 * new positions, which lie at or before the chunk's own start, so nothing depends on block order.  3. The short flags are scanned and a
 * compacting gather gives the ascending list of the short rows' ids.  4. ONE WAIT for the length S of that list, the error word and
 * the tallies.  5. If S > 0, vc_knn_graph*'s driver runs over that id list -- batches, rounds, waits and the linear hand-over as in
 * vc_knn_graph* -- and writes each settled row and count to its own place.  6. One last wait fetches the repair's stats, and only
 * when stats is given.
 * STATS (HOST memory in both forms, may be NULL).  n_rows_kept, n_rows_short and n_entries_dropped are functions of the database
 * before, the removal and k only; `repair` depends on the knobs as vc_knn_graph_stats does.
 * DEGENERATE.  K == n_old: VC_OK, nothing written, the stats zero apart from n_rows_kept.  K == 0 or n_old == 0: VC_OK, nothing
 * written.  K == 1: count 0 and a UINT64_MAX row.
 * ERRORS, checked before any work, outputs untouched: VC_ERR_INVALID for a null handle, null rows or a null map, k outside
 * 1 .. VC_MAX_K - 1, a bad k_first, an approximate or unknown mode, n_old < vc_size; VC_ERR_STATE in MIH mode without a current
 * index.  Found ON THE DEVICE, giving VC_ERR_INVALID through the error word that comes home with the first wait -- vc_cluster_knn*'s
 * protocol; THE OUTPUTS ARE THEN UNDEFINED, but nothing outside the two buffers is read or written: an old count above k (UINT32_MAX
 * included), an entry whose id lies outside the old store, and a map that is not vc_retain*'s -- the live words must number exactly K,
 * and the j-th live word must equal id_base + j.
 * Not offered: graphs over a part of the range, and an automatic switch to a rebuild when most rows are short (after a dedup of a
 * clustered store nearly every row is): the call then costs the rebuild plus the translation, which the caller weighs.
 * Scratch: grow-only buffers of the handle, this call's own and vc_knn_graph*'s; every word is written before it is read. */
typedef struct vc_knn_graph_retain_stats {   /* 64 bytes */
  vc_knn_graph_stats repair;     /* of the searches that repaired the short rows (zero if none) */
  uint64_t n_rows_kept;          /* K */
  uint64_t n_rows_short;         /* surviving rows with m < min(k, K - 1): searched again */
  uint64_t n_entries_dropped;    /* entries of SURVIVING rows whose record was removed */
  uint64_t pad;
} vc_knn_graph_retain_stats;
int vc_knn_graph_retain_dev(vc_engine* e, uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first,
                            const uint32_t* d_new_ids, uint64_t* d_rows, uint32_t* d_counts,
                            vc_knn_graph_retain_stats* stats, void* stream);
/* The same for the map, rows and counts in host memory: all three are staged up, the K rows and counts come home; waits for them.  A
 * repaired row that the linear scan passed on with count UINT32_MAX is answered again as vc_knn_graph does it. */
int vc_knn_graph_retain(vc_engine* e, uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first,
                        const uint32_t* new_ids, uint64_t* rows, uint32_t* counts, vc_knn_graph_retain_stats* stats);

/* ---- components and in-degrees of the k-NN graph: vc_cluster_knn* -------------------------------------------------------------------------
 * Density-adaptive grouping: where one radius is too tight in sparse regions and too loose in dense ones, "i and j list each other
 * among their kk nearest" adapts to the local density.  Nothing is searched: the call reads a graph that vc_knn_graph* built and
 * touches the store only for N and id_base, so it may be run for any kk <= k, flag and cap on one graph build.
 * PRECONDITION.  d_rows (N * k) and d_counts (N) are what vc_knn_graph* wrote for this store over the full range first = 0, count = N
 * with this k.  d_counts may be NULL: every row then holds min(k, N - 1) entries, which is what vc_knn_graph* writes.  A count above k
 * (UINT32_MAX included) or an entry whose id is outside the store is found ON THE DEVICE and gives VC_ERR_INVALID -- vc_group_summary*'s
 * protocol: one wait for the error word together with the stats; the outputs are then undefined.
 * EDGES.  kk lies in 1 .. k.  Row i LISTS j iff j is among the first min(kk, count_i) entries of row i and dist(i, j) <= max_dist;
 * max_dist >= bits means no cap.  With count_j < kk (N - 1 < kk) every other record is in row j: every entry is listed.
 * OUTPUTS.  d_in_degree[j] (N words, may be NULL): the number of rows that list j, by exact integer atomics.  d_labels (N words):
 * the connected components of the graph in which i and j are joined
 *   VC_KNN_MUTUAL (flags 0)  iff each lists the other,
 *   VC_KNN_EITHER            iff one lists the other;
 * labels[i] is the smallest global id of record i's component, as vc_cluster_radius*: it feeds vc_group_summary*,
 * vc_retain*(VC_RETAIN_ROOTS), vc_search_knn_distinct* and the filtered and scoped calls unchanged.  stats (HOST memory in both forms,
 * may be NULL): n_edges the listed (directed) entries, n_mutual the unordered pairs that list each other (each counted once, from its
 * smaller member; under both flags), n_clusters the components, max_in_degree.
 * HOW.  Row j is exactly the min(k, N - 1) smallest packed (dist << 32 | id) over the other records and the distance is symmetric,
 * so "j lists i among its first m" is the ONE COMPARE (d << 32 | i) <= row_j[m - 1], m = min(kk, count_j): no search inside row j.
 * An init launch; one edge launch over the N * kk entries (the in-degree atomic, the compare, the union in the lock-free forest of
 * vc_cluster_radius*); the flatten-and-count pass; the largest in-degree.  Every output word is a function of the graph and the
 * call, not of the order in which the lanes ran.
 * ERRORS, checked before any work, outputs untouched: VC_ERR_INVALID for a null handle, rows or labels, k outside 1 .. VC_MAX_K - 1,
 * kk outside 1 .. k, unknown flags.  N == 0 gives VC_OK and zero stats.  WAITS: one, at the end.
 * Over a sharded store every pointer of the device form lives on the ROOT device. */
#define VC_KNN_MUTUAL 0u
#define VC_KNN_EITHER 1u
typedef struct vc_cluster_knn_stats {   /* 32 bytes */
  uint64_t n_edges;        /* listed entries (directed) */
  uint64_t n_mutual;       /* unordered pairs that list each other */
  uint64_t n_clusters;
  uint32_t max_in_degree;
  uint32_t pad;
} vc_cluster_knn_stats;
int vc_cluster_knn_dev(vc_engine* e, const uint64_t* d_rows, const uint32_t* d_counts, uint32_t k, uint32_t kk, uint32_t flags,
                       uint32_t max_dist, uint32_t* d_labels, uint32_t* d_in_degree, vc_cluster_knn_stats* stats, void* stream);
/* The same for host pointers: rows and counts are staged ON EVERY CALL, labels and in-degrees come home; waits for them. */
int vc_cluster_knn(vc_engine* e, const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags,
                   uint32_t max_dist, uint32_t* labels, uint32_t* in_degree, vc_cluster_knn_stats* stats);

/* ---- shared-nearest-neighbour clusters of the k-NN graph: vc_cluster_snn* -----------------------------------------------------------------
 * vc_cluster_knn* judges an edge by rank alone: on data with noise between the groups one stray mutual pair welds two groups
 * together.  Shared-nearest-neighbour clustering (Jarvis and Patrick, 1973) joins i and j only if their neighbour lists overlap in
 * at least min_shared records; the overlap counts themselves are the edge weights of community detection and of Jaccard-weighted
 * graph pipelines, and their histogram is what one reads min_shared from.  Nothing is searched and the store is touched only for N
 * and id_base.  The reference has no such call.
 * PRECONDITION AND "LISTS": exactly vc_cluster_knn*'s.  d_rows (N * k) and d_counts (N, may be NULL: every row then holds
 * min(k, N - 1) entries) are what vc_knn_graph* wrote over the full range with this k.  Row i LISTS j iff j is among the first
 * min(kk, count_i) entries of row i and dist(i, j) <= max_dist.  S_i is the set of records row i lists; the record itself is never
 * in its own set.  kk lies in 1 .. min(k, VC_SNN_MAX_KK).  flags is VC_KNN_MUTUAL or VC_KNN_EITHER and decides which pairs are
 * CANDIDATES: each lists the other / one lists the other.
 * OUTPUTS.  shared(i, j) = |S_i n S_j|, symmetric, in 0 .. kk - 1.
 *   d_shared (N * kk words, stride kk, may be NULL): word i * kk + jj is shared(i, j) when entry jj of row i is listed, VC_SNN_NONE
 *     otherwise.  Every word is written.
 *   d_hist (kk words of uint64_t, may be NULL): hist[s] = the listed (directed) entries with shared == s; it sums to n_edges.
 *   d_labels (N words, required): the components of the graph in which i and j are joined iff they are a candidate pair AND
 *     shared(i, j) >= min_shared; labels[i] is the smallest global id of the component, as vc_cluster_knn*, and feeds
 *     vc_group_summary*, vc_retain*(VC_RETAIN_ROOTS) and the distinct, filtered and scoped searches unchanged.
 *   stats (HOST memory in both forms, may be NULL): n_edges and n_mutual as vc_cluster_knn*; n_joined the unordered candidate pairs
 *     with shared >= min_shared, each counted once -- a mutual pair from its smaller member, a one-sided pair (VC_KNN_EITHER) from
 *     the row that lists it; n_clusters; max_shared over the listed entries, 0 if none.
 * min_shared == 0 gives vc_cluster_knn*'s labels, n_edges, n_mutual and n_clusters bit for bit; min_shared >= kk joins nothing.
 * Every output word is a function of the graph and the call, not of lane order, block order or the hash function used.
 * HOW.  One team of lanes per row -- a wave up to kk = 128, a block above -- puts S_i into an open-addressing set in LDS, at most
 * half full, then for each listed entry (d, j) strides over row j's first min(kk, count_j) entries with coalesced loads, tests the
 * cap and probes the set; a ballot's popcount is shared(i, j).  "j lists i" stays vc_cluster_knn*'s one compare.  The weights'
 * histogram is summed per block in LDS; the unions go into the lock-free forest of vc_cluster_radius*; then the flatten-and-count pass.
 * ERRORS, checked before any work, outputs untouched: VC_ERR_INVALID for a null handle, rows or labels, k outside 1 .. VC_MAX_K - 1,
 * kk outside 1 .. min(k, VC_SNN_MAX_KK), unknown flags.  Found ON THE DEVICE, VC_ERR_INVALID through vc_cluster_knn*'s protocol (the
 * error word comes home with the stats; THE OUTPUTS ARE THEN UNDEFINED, but nothing is read or written out of bounds): a count above
 * k, an entry whose id is outside the store, an entry whose id equals the row's own.  A row that lists one id twice is not a
 * vc_knn_graph* row: the result is then unspecified, but the call terminates and stays in bounds.
 * N == 0 gives VC_OK and zero stats; N == 1 gives the record its own label and all of d_shared VC_SNN_NONE.  WAITS: one, at the end.
 * Over a sharded store every pointer of the device form lives on the ROOT device and no shard is touched.
 * NOT OFFERED: closed neighbour sets (the record counted in its own set); a Jaccard threshold, which the caller derives from d_shared
 * and the counts; kk above 1024. */
#define VC_SNN_MAX_KK 1024u
#define VC_SNN_NONE   0xFFFFFFFFu
typedef struct vc_cluster_snn_stats {   /* 40 bytes */
  uint64_t n_edges;      /* listed entries (directed), as vc_cluster_knn* */
  uint64_t n_mutual;     /* unordered pairs that list each other, as vc_cluster_knn* */
  uint64_t n_joined;     /* unordered candidate pairs with shared >= min_shared, each counted once */
  uint64_t n_clusters;
  uint32_t max_shared;   /* over the listed entries; 0 if none */
  uint32_t pad;
} vc_cluster_snn_stats;
int vc_cluster_snn_dev(vc_engine* e, const uint64_t* d_rows, const uint32_t* d_counts, uint32_t k, uint32_t kk, uint32_t flags,
                       uint32_t max_dist, uint32_t min_shared, uint32_t* d_labels, uint32_t* d_shared, uint64_t* d_hist,
                       vc_cluster_snn_stats* stats, void* stream);
/* The same for host pointers: rows and counts are staged ON EVERY CALL; labels, weights and histogram come home; waits for them. */
int vc_cluster_snn(vc_engine* e, const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags,
                   uint32_t max_dist, uint32_t min_shared, uint32_t* labels, uint32_t* shared, uint64_t* hist,
                   vc_cluster_snn_stats* stats);

/* ---- the reverse, mutual and symmetrised k-NN graph in CSR form: vc_knn_adjacency* --------------------------------------------------------
 * Every call above walks the graph FORWARDS: row i tells whom i lists.  This call answers who lists j -- the ids behind
 * vc_cluster_knn*'s in_degree[j] -- and writes the adjacency of the mutual and of the symmetrised graph, the input of community
 * detection, label propagation, spectral and UMAP-style pipelines, in CSR.  Nothing is searched and the store is touched only for N,
 * id_base and the code width.  The reference has no such call.
 * PRECONDITION AND "LISTS": exactly vc_cluster_knn*'s.  d_rows (N * k) and d_counts (N, may be NULL: every row then holds
 * min(k, N - 1) entries) are what vc_knn_graph* wrote over the full range with this k.  Row i LISTS j iff j is among the first
 * min(kk, count_i) entries of row i and dist(i, j) <= max_dist; "j lists i" stays the one compare.  kk lies in 1 .. k.
 * OUTPUTS.  d_offsets has N + 1 words; segment j is d_adj[d_offsets[j] .. d_offsets[j + 1]) and holds the packed
 * dist << 32 | id of i for every record i of the set below, ASCENDING in the packed word: nearest first, ties to the smaller id -- the
 * order of a vc_knn_graph* row.  T = d_offsets[N].
 *   VC_KNN_REVERSE: every i that lists j.  The segment lengths are vc_cluster_knn*'s in_degree; T = n_edges.
 *   VC_KNN_MUTUAL:  every i that lists j and is listed by j: the adjacency of the graph vc_cluster_knn*(VC_KNN_MUTUAL) takes the
 *                   components of; T = 2 n_mutual.
 *   VC_KNN_EITHER:  every i that lists j or is listed by j, each once: the adjacency of the symmetrised graph;
 *                   T = 2 (n_edges - n_mutual).
 *   stats (HOST memory in both forms, may be NULL): n_edges as vc_cluster_knn*; n_entries = T; n_empty the records whose segment is
 *   empty; max_degree the longest segment.
 * Every word of d_offsets and of d_adj[0 .. T) is a function of the graph and the call only: not of lane or block order, of earlier
 * calls on the handle or of the shard layout.
 * CAPACITY, the protocol of the radius calls.  T <= N kk under VC_KNN_REVERSE and VC_KNN_MUTUAL, T <= 2 N kk under VC_KNN_EITHER.
 * T > adj_cap returns VC_ERR_CAPACITY: d_offsets is then filled (d_offsets[N] = T), d_adj is untouched, stats is filled.  adj_cap == 0
 * with a NULL d_adj is the sizing call: it costs the count pass only -- no item is written, nothing is sorted.
 * HOW.  VC_KNN_REVERSE and VC_KNN_EITHER: one thread per (record, entry < kk) writes a sort item -- key = the target's position,
 * value = dist << 32 | id of the source; under VC_KNN_EITHER only for the one-sided entries, the mutual ones being in the target's row
 * already -- and bumps the target's counter by an exact atomic; what is no item gets the key N and sorts to the end.  The counters
 * are scanned; ONE copy brings T, the statistics and the error word home.  Then a stable LSD radix sort of the items, first by the
 * distance (ceil(bitlength(min(max_dist, bits)) / 8) passes: one up to 128-bit codes, two above), then by the key
 * (ceil(bitlength(N) / 8) passes); the enumerate order is source-major, so stability yields the (target, dist, source id) order --
 * no segment-length limit and no ordering left to chance, whatever hubs the data hold.  VC_KNN_REVERSE copies the first T values out;
 * VC_KNN_EITHER merges each row's listed entries with the record's sorted run by rank counting, a wave per record, the block for a
 * segment above 1024 words.  VC_KNN_MUTUAL sorts nothing: segment i is the mutual entries of row i in row order, a ballot count and a
 * ballot compaction.
 * SCRATCH, in the handle's grow-only buffers: 24 N kk bytes for the two item buffer pairs (none under VC_KNN_MUTUAL and in a sizing
 * call), the sort's work words and (N + 1) counters, 2 (N + 1) under VC_KNN_EITHER.  It is NOT bounded by VC_KGRAPH_SCRATCH: a sort
 * cannot be chunked.
 * ERRORS, checked before any work, outputs untouched: VC_ERR_INVALID for a null handle, rows or offsets, a null adj with adj_cap > 0,
 * k outside 1 .. VC_MAX_K - 1, kk outside 1 .. k, flags above 2, N kk > 2^31 - 1 (this version's limit: the scans and the sort's
 * positions are 32-bit; the offsets are uint64_t so that lifting it changes no signature).  Found ON THE DEVICE, VC_ERR_INVALID: a
 * count above k, an entry whose id is outside the store, an entry whose id equals the row's own.  They come home through the error
 * word of the single wait, and NO OUTPUT WORD IS WRITTEN BEFORE THAT WAIT: d_offsets and d_adj are then untouched -- a stronger
 * promise than vc_cluster_knn*'s.  A row that is not ascending, lists an id twice or holds a distance above the code width is not a
 * vc_knn_graph* row: the result is then unspecified, but the call terminates and stays in bounds.
 * N == 0 gives VC_OK, zero stats and d_offsets[0] = 0.  VC_ERR_NOMEM leaves the outputs untouched: every buffer is grown before the
 * first launch.  WAITS: one in the device form.  Over a sharded store every pointer of the device form lives on the ROOT device and
 * no shard is touched; the result equals the single engine's word for word.
 * NOT OFFERED: segments ordered by neighbour id; a per-segment degree cap; N kk above 2^31 - 1; an incremental form after
 * vc_add_codes / vc_retain*; weights other than the distance (vc_cluster_snn*'s d_shared is indexed by row entry and can be joined
 * by the caller). */
#define VC_KNN_REVERSE 2u        /* beside VC_KNN_MUTUAL 0u and VC_KNN_EITHER 1u; accepted by vc_knn_adjacency* only */
typedef struct vc_knn_adjacency_stats {   /* 32 bytes */
  uint64_t n_edges;      /* listed entries (directed), as vc_cluster_knn* */
  uint64_t n_entries;    /* T = offsets[N] */
  uint64_t n_empty;      /* records whose segment is empty */
  uint32_t max_degree;   /* the longest segment */
  uint32_t pad;
} vc_knn_adjacency_stats;
int vc_knn_adjacency_dev(vc_engine* e, const uint64_t* d_rows, const uint32_t* d_counts, uint32_t k, uint32_t kk, uint32_t flags,
                         uint32_t max_dist, uint64_t* d_adj, uint64_t adj_cap, uint64_t* d_offsets,
                         vc_knn_adjacency_stats* stats, void* stream);
/* The same for host pointers: rows and counts are staged ON EVERY CALL; the offsets come home also on VC_ERR_CAPACITY, the T words of
 * adj on VC_OK; waits for the copy home. */
int vc_knn_adjacency(vc_engine* e, const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags,
                     uint32_t max_dist, uint64_t* adj, uint64_t adj_cap, uint64_t* offsets, vc_knn_adjacency_stats* stats);

/* ---- the minimum spanning forest of the k-NN graph in Kruskal order: vc_knn_mst*, vc_mst_cut* -------------------------------------------
 * vc_cluster_knn* gives the components at ONE cut.  The minimum spanning forest (MSF) of the mutual or symmetrised graph gives them
 * at EVERY cut: at most N - 1 edges, ascending, from which the labels at any height, the number of clusters at every height and --
 * under mutual-reachability weights -- the tree that HDBSCAN-style pipelines condense all follow without reading the N kk entries
 * again, and with no limit on the number of levels (vc_cluster_levels* stops at radius 63 and costs N words per level).
 * PRECONDITION AND "LISTS": exactly vc_cluster_knn*'s.  d_rows (N * k) and d_counts (N, may be NULL: every row then holds
 * min(k, N - 1) entries) are what vc_knn_graph* wrote over the full range with this k.  Row i LISTS j iff j is among the first
 * min(kk, count_i) entries of row i and dist(i, j) <= max_dist.  kk lies in 1 .. k, and N kk <= 2^31 - 1 (vc_knn_adjacency*'s limit:
 * an entry's index takes the low word of the edge key).
 * GRAPH.  flags is VC_KNN_MUTUAL or VC_KNN_EITHER: the undirected pair {i, j} is an edge iff each lists the other / iff one lists
 * the other.  VC_KNN_REVERSE is refused.
 * WEIGHT.  weight_kind = VC_MST_DISTANCE: w = dist(i, j); min_pts must be 1.  VC_MST_REACHABILITY: w = max(dist(i, j), c_i, c_j), the
 * mutual-reachability distance; min_pts lies in 1 .. k + 1 and counts the record itself, as vc_dbscan_levels*'s: c_i = 0 for
 * min_pts = 1, otherwise the distance of entry min_pts - 2 of row i, read from the k columns regardless of kk and max_dist; when
 * count_i < min_pts - 1, c_i = bits.  min_pts = 1 under VC_MST_REACHABILITY gives VC_MST_DISTANCE's output bit for bit.
 * THE ORDER, which makes every word a function of the graph and the call.  An edge is written as vc_mst_edge { a, b, weight, dist }
 * with global ids.  a is the HOME end: the smaller id if it lists the other, otherwise the larger (the larger then lists the smaller;
 * such one-sided edges exist only under VC_KNN_EITHER); b is the other end.  Edges are ordered lexicographically by
 * (weight, a, dist, b), which is the order of the 64-bit key weight << 32 | (pos(a) * kk + jj), jj the position of b in row a, because
 * rows ascend in (dist, id).  The order is strict, so the MSF is unique: the edges Kruskal keeps, taking edges ascending.
 * OUTPUTS of vc_knn_mst_dev.
 *   d_edges has room for max(N, 1) - 1 entries: the M forest edges, ascending in the order above; words beyond M are untouched.
 *   d_labels (N words, may be NULL): the components of the whole graph, smallest global id -- vc_cluster_knn*'s labels for the same
 *     kk, flags and max_dist, bit for bit.
 *   d_hist (bits + 1 words of uint64_t, may be NULL): hist[w] = forest edges of weight w; the clusters at height h are
 *     N - sum of hist[w] over w <= h.
 *   stats (HOST memory in both forms, may be NULL): n_edges the listed (directed) entries as vc_cluster_knn*, n_graph_edges the
 *     undirected edges of the chosen graph, n_tree = M, n_clusters = N - M, total_weight, max_weight, n_rounds the Boruvka rounds
 *     that hooked something -- implementation-defined, at most ceil(log2 N) + 1.
 * vc_mst_cut_dev: the components of the N records under the given edges of weight <= max_weight, smallest-id labels; it takes ANY
 * edge list, sorted or not (dist is not read).  An end outside the store gives VC_ERR_INVALID, found on the device.  On the MSF under
 * VC_MST_DISTANCE it equals vc_cluster_knn*(max_dist = min(the build's cap, max_weight)) bit for bit.  Its labels feed
 * vc_group_summary*, vc_retain*(VC_RETAIN_ROOTS), vc_search_knn_distinct* and the filtered and scoped calls unchanged.  *n_clusters
 * (HOST memory, may be NULL) gets the number of components.
 * HOW.  Boruvka on the device.  One thread per (record, entry < kk) validates the entry, does vc_cluster_knn*'s one compare and
 * appends every HOME entry to a compact live list (key, the other end) by ballot rank.  A round: every live edge whose ends lie in
 * two components offers its key to both by a 64-bit atomicMin behind a relaxed load, and survives into the other live buffer; every
 * component with a pick writes it to the picked list exactly once and unites the two trees in the lock-free forest of
 * vc_cluster_radius*; a flatten pass takes the round's snapshot.  The host reads the picked count and stops when a round hooked
 * nothing.  The strict order forbids cycles, and a chain of any length may hook in one round.  Then vc_knn_adjacency*'s stable radix
 * sort of the M picked edges by (weight, home index), and one launch writes the edges, the histogram and the sums.
 * SCRATCH, in the handle's grow-only buffers: 24 bytes per home entry (at most N kk of them, N kk / 2 under VC_KNN_MUTUAL) for the two
 * live buffers, 16 N for the forest, 24 N for the picked list and the sort's work words.
 * ERRORS, checked before any work, outputs untouched: VC_ERR_INVALID for a null handle, rows or edges, k outside 1 .. VC_MAX_K - 1,
 * kk outside 1 .. k, flags other than VC_KNN_MUTUAL / VC_KNN_EITHER, an unknown weight_kind, min_pts outside its range,
 * N kk > 2^31 - 1; vc_mst_cut*: a null handle or labels, null edges with n_edges > 0.  Found ON THE DEVICE, VC_ERR_INVALID through
 * vc_cluster_knn*'s protocol (THE OUTPUTS ARE THEN UNDEFINED, everything stays in bounds): a count above k, an entry whose id is
 * outside the store, an entry whose id equals the row's own.  N == 0 gives VC_OK and zero stats (d_hist zeroed); N == 1 gives M = 0
 * and the own label.
 * WAITS: one small read-back per round, plus one at the end; vc_mst_cut*: one.  Over a sharded store every pointer of the device
 * forms lives on the ROOT device and no shard is touched; the result equals the single engine's word for word.
 * NOT OFFERED: an incremental form; the condensed tree and stability selection (host work on N - 1 edges); N kk above 2^31 - 1.
 * (The condensed tree and its selection are a call of their own, on the device: vc_mst_condense* below takes these edges as they are.) */
#define VC_MST_DISTANCE 0u
#define VC_MST_REACHABILITY 1u
typedef struct vc_mst_edge {   /* 16 bytes */
  uint32_t a;        /* the home end, global id */
  uint32_t b;        /* the other end, global id */
  uint32_t weight;
  uint32_t dist;
} vc_mst_edge;
typedef struct vc_knn_mst_stats {   /* 48 bytes */
  uint64_t n_edges;        /* listed entries (directed), as vc_cluster_knn* */
  uint64_t n_graph_edges;  /* undirected edges of the chosen graph */
  uint64_t n_tree;         /* M */
  uint64_t n_clusters;     /* N - M */
  uint64_t total_weight;
  uint32_t max_weight;
  uint32_t n_rounds;       /* rounds that hooked something */
} vc_knn_mst_stats;
int vc_knn_mst_dev(vc_engine* e, const uint64_t* d_rows, const uint32_t* d_counts, uint32_t k, uint32_t kk, uint32_t flags,
                   uint32_t max_dist, uint32_t weight_kind, uint32_t min_pts, vc_mst_edge* d_edges, uint32_t* d_labels,
                   uint64_t* d_hist, vc_knn_mst_stats* stats, void* stream);
/* The same for host pointers: rows and counts are staged ON EVERY CALL; the M edges, the labels and the histogram (both may be NULL)
 * come home; waits for them.  M is stats->n_tree. */
int vc_knn_mst(vc_engine* e, const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags,
               uint32_t max_dist, uint32_t weight_kind, uint32_t min_pts, vc_mst_edge* edges, uint32_t* labels, uint64_t* hist,
               vc_knn_mst_stats* stats);
int vc_mst_cut_dev(vc_engine* e, const vc_mst_edge* d_edges, uint64_t n_edges, uint32_t max_weight, uint32_t* d_labels,
                   uint64_t* n_clusters, void* stream);
/* The same for host pointers: the edges are staged, the labels come home; waits for them. */
int vc_mst_cut(vc_engine* e, const vc_mst_edge* edges, uint64_t n_edges, uint32_t max_weight, uint32_t* labels,
               uint64_t* n_clusters);

/* ---- the weighted label vote of a segment: the k-NN classifier vc_knn_vote* and label propagation vc_label_propagate* ----------------------
 * Every call above groups records without supervision.  These two use labels the caller already has: "which album, class or tag does
 * this picture belong to?" is the majority label among its k nearest records (vc_knn_vote*, over the rows of any search or of a
 * graph, which never leave HBM), and a few thousand hand-tagged records tag the rest of the store along the adjacency of
 * vc_knn_adjacency* (vc_label_propagate*); started from labels[i] = id_base + i the second call is community detection by label
 * propagation.  Both are exact integers and a function of their inputs only.
 * THE VOTE RULE, shared by both calls.  A SEGMENT is an ordered list of packed entries dist << 32 | id, ascending in the packed word.
 * labels holds one uint32_t per resident record, indexed by id - id_base; VC_VOTE_NONE means "unlabelled": such an entry does not
 * vote.  The weight of a voting entry at distance d is 1 under VC_VOTE_COUNT and bits + 1 - d under VC_VOTE_CLOSENESS (at least 1,
 * the nearest weighs most).  tally[l] is the sum of the weights of the entries labelled l, total the sum of all tallies.  THE WINNER
 * is the label first in this strict order: (1) the larger tally; (2) then the segment's CURRENT label -- only vc_label_propagate*
 * has one: the standard damping of label propagation; (3) then the label whose first occurrence in the segment comes earliest, so
 * among tied labels the nearest neighbour's wins, ties in distance going to the smaller id, which is the segment order itself.  A
 * segment with no voting entry has winner VC_VOTE_NONE, votes = 0 and total = 0.  The order is strict, so every output word is a
 * function of the segment and the labels: it does not depend on lane or block order, on earlier calls on the handle or on the shard
 * layout.  A row is DECIDED BY RULE 3 when several labels hold the largest tally and the current label is none of them.
 * vc_knn_vote_dev.  d_rows (n_rows * k) holds ANY rows whose ids are resident: a graph of vc_knn_graph* (n_rows = N) or the rows of
 * vc_search_knn_dev and its distinct, filtered, scoped and ids forms for a batch of queries.  d_counts (n_rows) may be NULL: every row
 * then holds min(k, N) entries.  Row r's segment is its first min(kk, count_r) entries at distance <= max_dist.  kk lies in 1 .. k, k
 * in 1 .. VC_MAX_K.  An entry equal to a record's own id is an ordinary entry.  d_labels has N words.  d_out_label (n_rows) gets the
 * winners; d_out_votes and d_out_total (n_rows each, may be NULL) the winner's tally and the total: votes / total is the confidence,
 * and both stay integers.  stats (HOST memory in both forms, may be NULL): n_voted rows with a winner, n_unlabelled rows without one,
 * n_ties rows decided by rule 3, n_entries voting entries.
 * vc_label_propagate_dev.  d_offsets (N + 1 words) and d_adj are what vc_knn_adjacency* wrote for this store, with any flag;
 * n_entries must equal d_offsets[N].  Any CSR with non-decreasing offsets from 0, ascending segments and resident ids qualifies.
 * ROUNDS: L_0 = labels_in.  In round t every record i takes the winner of segment i under L_{t-1}, with current label L_{t-1}[i]; if
 * the segment has no voting entry, i keeps L_{t-1}[i].  With VC_LP_CLAMP_SEEDS in flags every record with labels_in[i] !=
 * VC_VOTE_NONE keeps labels_in[i] in every round: the semi-supervised form.  Without the flag and with labels_in[i] = id_base + i the
 * call is community detection by label propagation.  Rounds are double-buffered: no record ever reads a label written in the same
 * round, so the result does not depend on execution order.  The call stops after the first round that changes no label, or after
 * max_iters rounds (1 .. VC_LP_MAX_ITERS); synchronous propagation can oscillate, so the stats say which stop happened.
 * d_labels_out (N) holds L_T.  d_votes and d_total (N each, may be NULL) are the winner's tally and the total of the LAST round run,
 * that is under L_{T-1}; they are also written for clamped seeds, so a seed that its neighbourhood outvotes is visible.  stats:
 * n_iters = T, converged (0 or 1), n_changed_last, n_labelled the records with a label other than VC_VOTE_NONE in L_T, n_ties_last the
 * records whose vote in the last round was decided by rule 3 (clamped seeds included).  The labels feed vc_group_summary*, vc_retain*
 * and the distinct, filtered and scoped searches unchanged whenever they are resident ids, which the community form guarantees; the
 * caller's class values of the semi-supervised form are taken by the sel and scope consumers only.
 * HOW.  One tally routine serves both views.  Up to 64 entries a team of P lanes (P the power of two at or above the length) holds
 * the entries, `length` broadcast steps give every lane the tally of its label, and a butterfly max over the key (tally, is-current,
 * inverted position) of the first occurrences picks the winner: no LDS, no atomics.  Up to 8192 entries a wave or a block fills an
 * open-addressing table of (label, tally) slots in LDS, at most half full, and a second walk in order max-reduces the key.  Above
 * that -- CSR hubs -- the table lies in the handle's scratch and 64 blocks stride over the segment; there is no limit on a segment's
 * length other than the 32-bit tally.  vc_label_propagate* first runs a plan pass: offsets and entries validated, the records listed
 * per degree bin by one scan (no atomic cursor), the long tables laid out, ONE wait; then a round is one launch per non-empty bin.
 * ERRORS, checked before any work, outputs untouched: VC_ERR_INVALID for a null handle, rows, labels or out_label, k outside
 * 1 .. VC_MAX_K, kk outside 1 .. k, an unknown weight_kind; vc_label_propagate*: a null handle, offsets, adj (with n_entries > 0),
 * labels_in or labels_out, an unknown weight_kind or flag, max_iters outside 1 .. VC_LP_MAX_ITERS.  Found ON THE DEVICE by
 * vc_knn_vote*, VC_ERR_INVALID through vc_cluster_knn*'s protocol (THE OUTPUTS ARE THEN UNDEFINED, everything stays in bounds): a
 * count above k, an id outside the store, under VC_VOTE_CLOSENESS a voting entry with d > bits.  Found on the device by
 * vc_label_propagate* with NO OUTPUT WORD WRITTEN (the plan waits before the first round): d_offsets[0] != 0, decreasing offsets,
 * d_offsets[N] != n_entries, an id outside the store, d > bits under VC_VOTE_CLOSENESS, a segment so long that length * (bits + 1)
 * does not fit 32 bits.  n_rows == 0 and N == 0 give VC_OK and zero stats.
 * WAITS: vc_knn_vote*: one.  vc_label_propagate*: one for the plan, then one small read-back per round.  Over a sharded store every
 * pointer of the device forms lives on the ROOT device and no shard is touched; the result equals the single engine's word for word.
 * NOT OFFERED: caller-given edge weights such as vc_cluster_snn*'s d_shared; asynchronous propagation; an incremental form after
 * vc_add_codes or vc_retain*; more than 64 rounds per call -- a caller continues by passing labels_out back in. */
#define VC_VOTE_NONE 0xFFFFFFFFu
#define VC_VOTE_COUNT 0u
#define VC_VOTE_CLOSENESS 1u
#define VC_LP_CLAMP_SEEDS 1u
#define VC_LP_MAX_ITERS 64u
typedef struct vc_knn_vote_stats {   /* 32 bytes */
  uint64_t n_voted;        /* rows with a winner */
  uint64_t n_unlabelled;   /* rows without a winner */
  uint64_t n_ties;         /* rows whose winner was decided by rule 3 */
  uint64_t n_entries;      /* voting entries */
} vc_knn_vote_stats;
typedef struct vc_label_propagate_stats {   /* 32 bytes */
  uint32_t n_iters;          /* rounds run */
  uint32_t converged;        /* 1: the last round changed no label */
  uint64_t n_changed_last;   /* labels the last round changed */
  uint64_t n_labelled;       /* records with a label other than VC_VOTE_NONE in L_T */
  uint64_t n_ties_last;      /* records whose vote in the last round was decided by rule 3 */
} vc_label_propagate_stats;
int vc_knn_vote_dev(vc_engine* e, const uint64_t* d_rows, const uint32_t* d_counts, uint64_t n_rows, uint32_t k, uint32_t kk,
                    uint32_t max_dist, const uint32_t* d_labels, uint32_t weight_kind, uint32_t* d_out_label, uint32_t* d_out_votes,
                    uint32_t* d_out_total, vc_knn_vote_stats* stats, void* stream);
/* The same for host pointers: rows, counts and labels are staged ON EVERY CALL; the three outputs (votes and total may be NULL) come
 * home; waits for them. */
int vc_knn_vote(vc_engine* e, const uint64_t* rows, const uint32_t* counts, uint64_t n_rows, uint32_t k, uint32_t kk, uint32_t max_dist,
                const uint32_t* labels, uint32_t weight_kind, uint32_t* out_label, uint32_t* out_votes, uint32_t* out_total,
                vc_knn_vote_stats* stats);
int vc_label_propagate_dev(vc_engine* e, const uint64_t* d_offsets, const uint64_t* d_adj, uint64_t n_entries, const uint32_t* d_labels_in,
                           uint32_t weight_kind, uint32_t flags, uint32_t max_iters, uint32_t* d_labels_out, uint32_t* d_votes,
                           uint32_t* d_total, vc_label_propagate_stats* stats, void* stream);
/* The same for host pointers: offsets, adj and labels_in are staged on every call; labels_out, votes and total (both may be NULL)
 * come home; waits for them. */
int vc_label_propagate(vc_engine* e, const uint64_t* offsets, const uint64_t* adj, uint64_t n_entries, const uint32_t* labels_in,
                       uint32_t weight_kind, uint32_t flags, uint32_t max_iters, uint32_t* labels_out, uint32_t* votes, uint32_t* total,
                       vc_label_propagate_stats* stats);

/* ---- HDBSCAN-style clusters from a spanning forest: vc_mst_condense* ---------------------------------------------------------------------
 * vc_mst_cut* gives the components of a forest at ONE height the caller names.  This call gives the clusters that PERSIST, each at its
 * own density: the condensed tree of the forest, the stability of every node, the excess-of-mass (or leaf) selection and the flat
 * labels with noise -- on the device, in integers, every output word a function of the input.
 * INPUT.  d_edges[0 .. n_edges) are vc_mst_edge records as vc_knn_mst* writes them; only a, b and weight are read.  The list must be
 * a FOREST over the N resident records, non-decreasing in weight, every weight <= bits.  Any such list qualifies, not only a
 * vc_knn_mst* output, and the order of the edges WITHIN one weight influences no output word.  min_cluster_size (mcs) lies in
 * 2 .. 2^31.  root_weight is 0, or lies in 1 .. bits + 1 and is above every edge weight: the height at which the components of the
 * forest are deemed to merge.  method is VC_CONDENSE_EOM or VC_CONDENSE_LEAF.
 * THE TREE, bottom-up over the distinct weights w, ascending.  The components at height h are those of the edges of weight <= h.
 * When the edges of weight w are taken, each new component X is the union of a group of previous components (singletons included);
 * its children of size >= mcs are BIG, the others SMALL.  A component of size >= mcs always carries exactly one live cluster.
 *   two or more big children: their clusters END at w; a new node P FORMS at w with those clusters as its children, size |X|, and every
 *     record of X has leave level w in P; the small children's records get own = P, leave = w.
 *   exactly one big child: its cluster C continues as X, the same node, grown by the small children's records: own = C, leave = w.
 *   no big child and |X| >= mcs: a new LEAF node forms at w with size |X|; all its records get own = that node, leave = w.
 *   no big child and |X| < mcs: nothing.
 * A cluster alive when the edges run out is a ROOT: its end is root_weight and its parent VC_CONDENSE_NONE.  A record whose
 * component never reaches mcs has own = leave = VC_CONDENSE_NONE.  rep(C) is the smallest global id of C's component at its end.
 * STABILITY, the integer excess of mass in the distance domain: stability(C) = end(C) size(C) - the sum of leave(p) over the records
 * that ever joined C, which for a node formed at f is f size_at_formation + the sum of w absorbed_at_w.  A root under
 * root_weight == 0 has stability 0 and is never selected (per forest component, "no single cluster").
 * SELECTION.  Nodes are numbered ascending by (form, rep); the order is strict and children have smaller indices than parents.
 * Ascending: sub(C) = the sum of best(child); keep(C) = stability(C) >= sub(C), a tie going to the parent, and false for a root under
 * root_weight == 0; best(C) = keep ? stability : sub.  Then C is SELECTED iff keep(C) and no ancestor has keep.  Under
 * VC_CONDENSE_LEAF, C is selected iff it has no children (the same root rule); stability, best and the keep bit are written all the same.
 * OUTPUTS of vc_mst_condense_dev.
 *   d_nodes has room for max(N, 1) - 1 vc_condensed_node records (there are at most 2 floor(N / mcs) - 1): the n_nodes nodes in their
 *     order; words beyond n_nodes are untouched.  flags: VC_CONDENSE_SELECTED | VC_CONDENSE_KEEP | VC_CONDENSE_ROOT; pad is 0.
 *   d_labels (N words): rep of the selected node that is own(p) or an ancestor of it; otherwise the record's OWN global id -- noise,
 *     vc_dbscan_radius*'s convention, so the labels feed vc_group_summary*, vc_retain*(VC_RETAIN_ROOTS) and the distinct, filtered and
 *     scoped searches unchanged.
 *   d_node (N words, may be NULL): the index of that selected node, VC_CONDENSE_NONE for noise -- it tells a cluster's representative
 *     from a noise record.
 *   d_own, d_leave (N words each, may be NULL): own(p) as a node index and leave(p), the inputs of a GLOSH-style outlier score.
 *   stats (HOST memory in both forms, may be NULL): n_nodes, n_leaves (nodes without children), n_roots, n_selected, n_clustered and
 *     n_noise (they sum to N), total_stability over the selected nodes, n_levels the distinct weights.
 * HOW.  A plan launch validates every edge and notes the first edge of every weight; the host compacts that into at most bits + 1
 * levels.  Per level, with no wait: the level's edges are united in vc_cluster_radius*'s lock-free forest; every edge end claims its
 * previous component once and adds its size to the new root's sums (integer atomics); every new root applies the table above and
 * creates its node, in any order; the previous components are told; a pass over the records hands out own and leave and takes the
 * next snapshot.  Then the nodes are sorted by (form, rep) with vc_knn_adjacency*'s radix sort, one launch folds best upwards (the
 * last child to arrive serves the parent), one finds every node's selected ancestor, one writes the labels.
 * SCRATCH, in the handle's grow-only buffers: 48 bytes per record, 88 per node of the N - 1 the output may hold (the sort's two buffers among them), and the sort's work words.
 * ERRORS, checked before any work, outputs untouched: VC_ERR_INVALID for a null handle, labels or nodes, null edges with n_edges > 0,
 * n_edges > max(N, 1) - 1, mcs outside 2 .. 2^31, root_weight > bits + 1, an unknown method.  Found ON THE DEVICE, VC_ERR_INVALID
 * through the error word of the first wait with NO OUTPUT WORD WRITTEN: an end outside the store, a == b, a weight above bits,
 * descending weights, root_weight != 0 and not above the last weight.  A CYCLE (the components at the end must number N - n_edges)
 * is found at the second wait, also before any output word is written.  N == 0 gives VC_OK and zero stats; n_edges == 0 gives no
 * nodes and identity labels.
 * WAITS: three small read-backs -- the plan, the number of nodes (with the cycle check), the statistics.  Over a sharded store every
 * pointer of the device forms lives on the ROOT device and no shard is touched; the result equals the single engine's word for word.
 * NOT OFFERED: the outlier scores themselves, a cluster_selection_epsilon, max_cluster_size, soft memberships. */
#define VC_CONDENSE_EOM 0u
#define VC_CONDENSE_LEAF 1u
#define VC_CONDENSE_NONE 0xFFFFFFFFu
#define VC_CONDENSE_SELECTED 1u
#define VC_CONDENSE_KEEP 2u
#define VC_CONDENSE_ROOT 4u
typedef struct vc_condensed_node {   /* 48 bytes */
  uint32_t parent;       /* node index, VC_CONDENSE_NONE for a root */
  uint32_t rep;          /* smallest global id of the component at the node's end */
  uint32_t form;
  uint32_t end;
  uint32_t size;         /* records that ever joined */
  uint32_t n_children;
  uint32_t flags;
  uint32_t pad;
  uint64_t stability;
  uint64_t best;
} vc_condensed_node;
typedef struct vc_mst_condense_stats {   /* 64 bytes */
  uint64_t n_nodes;
  uint64_t n_leaves;
  uint64_t n_roots;
  uint64_t n_selected;
  uint64_t n_clustered;
  uint64_t n_noise;
  uint64_t total_stability;
  uint32_t n_levels;
  uint32_t pad;
} vc_mst_condense_stats;
int vc_mst_condense_dev(vc_engine* e, const vc_mst_edge* d_edges, uint64_t n_edges, uint32_t min_cluster_size, uint32_t root_weight,
                        uint32_t method, vc_condensed_node* d_nodes, uint32_t* d_labels, uint32_t* d_node, uint32_t* d_own,
                        uint32_t* d_leave, vc_mst_condense_stats* stats, void* stream);
/* The same for host pointers: the edges are staged ON EVERY CALL; the n_nodes nodes, the labels and the three optional arrays come
 * home; waits for them.  n_nodes is stats->n_nodes; without stats, count the nodes by pre-filling `nodes`. */
int vc_mst_condense(vc_engine* e, const vc_mst_edge* edges, uint64_t n_edges, uint32_t min_cluster_size, uint32_t root_weight,
                    uint32_t method, vc_condensed_node* nodes, uint32_t* labels, uint32_t* node, uint32_t* own, uint32_t* leave,
                    vc_mst_condense_stats* stats);

/* Sticky status of the asynchronous device path: *n_gave_up = calls since the previous vc_device_status() in which the
 * device-side ring-overflow recovery could not complete (its grid never met: the GPU was held by other kernels for
 * seconds); the affected queries kept d_counts[i] == UINT32_MAX.  0 in normal operation.  Synchronises the stream.
 * replaces: nothing in the reference (its find() is synchronous, search_worker.cc:65-89). */
int vc_device_status(vc_engine* e, uint32_t* n_gave_up);

/* ---- multi-GPU merge ---------------------------------------------------------------------
 * replaces: mpi_coordinator::gather_vectors + master-side heap (mpi_coordinator.cc:34-69,
 * search_worker.cc:179-199).  d_lists holds n_lists blocks of nq*k packed values (the all-gathered
 * per-shard top-k); UINT64_MAX marks an empty entry.  A list may be in any order, with its empty entries
 * anywhere and values repeated within it or across lists: ascending lists with the empty entries at the
 * tail (what the engine's rows are) take the fast merge, others are sorted first.  Writes the k smallest
 * values ascending to d_out (nq*k, UINT64_MAX padded) and the number of non-empty ones per query to
 * d_counts (may be NULL).  Asynchronous on `stream`; no engine needed. */
int vc_merge_topk_dev(const uint64_t* d_lists, uint32_t n_lists, uint32_t nq, uint32_t k,
                      uint64_t* d_out, uint32_t* d_counts, void* stream);

/* ---- one process, several GPUs --------------------------------------------------------------
 * replaces: the reference's distribution of this path -- `mpirun -n 4` ranks (run_distributed_search.py:74), the
 * per-radius MPI_Gather / Gatherv / Bcast between them (search_worker.cc:99-101,177,207; mpi_coordinator.cc:26-69)
 * and the master-side dedup + heap (search_worker.cc:179-199).
 * The database is split BY ID RANGE into n_shards shards (shard g holds ids [capacity*g/G, capacity*(g+1)/G) of the
 * id space that starts at engine.id_base; shard g lives on device_ids[g % n_devices]); every shard answers the whole
 * batch for its ids and the per-shard top-k rows (nq*k*8 bytes per shard -- the only inter-GPU traffic) are brought
 * together by ONE exchange per batch and merged by the kernel behind vc_merge_topk_dev on the first device:
 *   VC_EXCHANGE_RCCL       grouped ncclAllGather over xGMI (single-process ncclCommInitAll; one shard per device)
 *   VC_EXCHANGE_PEER_COPY  hipMemcpyPeerAsync into the root's gather buffer (also when shards share a device)
 *   VC_EXCHANGE_AUTO       RCCL when there is one shard per device, more than one device and librccl loads; else peer copy
 * LINEAR results are exactly those of one engine holding everything (the top-k of a union is the top-k of the parts'
 * top-k).  MIH modes: every shard runs to its OWN stop rule, which is exact for the shard, so exact-mode distances
 * equal the single-engine result; statistics report the widest radius and the summed reads / candidates.  With
 * VC_FLAG_GLOBAL_STOP in engine.flags, VC_MODE_MIH_EXACT instead stops where ONE engine over the union stops: the shards run
 * in capped rounds (shells 0..t, own stop rule active), a kernel on the root judges the merged rows (pigeonhole check +
 * the union's stop rule) and only undecided queries run again; queries beyond the shards' in-block shells are answered by
 * a scan of the union with the stop rule replayed.  Rows, counts and all statistics then equal one vc_engine's.  With
 * VC_FLAG_GLOBAL_APPROX, VC_MODE_MIH_APPROX does the same for the approximate rule (search_worker.cc:104-139): rounds capped at
 * shell t = 0, 1, 2, ... over the open queries, a kernel on the root adds the shards' distinct candidate counts and settles
 * a query in the first round whose sum reaches 20 k (or at the last shell).  As in every MIH mode the host waits inside the
 * call; results are valid in stream order. */
#define VC_MAX_SHARDS 16
#define VC_EXCHANGE_AUTO 0
#define VC_EXCHANGE_PEER_COPY 1
#define VC_EXCHANGE_RCCL 2

typedef struct vc_sharded vc_sharded;
typedef struct vc_sharded_config {
  uint32_t abi_version;            /* VC_ABI_VERSION */
  uint32_t n_shards;               /* G: 1..VC_MAX_SHARDS (the reference's `size`, search_worker.cc:58) */
  uint32_t n_devices;              /* entries of device_ids; 0 = devices 0..min(visible, n_shards)-1 */
  uint32_t exchange;               /* VC_EXCHANGE_* */
  int32_t device_ids[VC_MAX_SHARDS];
  vc_config engine;                /* per-shard template: bits, n_tables, flags, cand_cap, query_tile ...; capacity = TOTAL
                                      records over all shards, id_base = global id of record 0; `device` is ignored */
} vc_sharded_config;

int vc_sharded_create(const vc_sharded_config* cfg, vc_sharded** out);
int vc_sharded_destroy(vc_sharded* h);
const char* vc_sharded_last_error(const vc_sharded* h);     /* h may be NULL for create failures */
int vc_sharded_exchange(const vc_sharded* h, uint32_t* kind); /* the exchange in use: VC_EXCHANGE_PEER_COPY or _RCCL */
/* ingest in global id order (build_hash_tables.cc:40-70), routed to the shard that owns the id */
int vc_sharded_add_codes(vc_sharded* h, const void* codes, uint64_t n);
int vc_sharded_add_synthetic(vc_sharded* h, uint64_t n, uint64_t seed, uint32_t kind, uint32_t n_centres, uint32_t max_flips);
int vc_sharded_size(const vc_sharded* h, uint64_t* n);
int vc_sharded_build_index(vc_sharded* h);
/* vc_update_index per non-empty shard: update if it has an index, else build.  Appended ids fill the id-range
 * shards in order, so only the shard the store ended in and those after it have work to do. */
int vc_sharded_update_index(vc_sharded* h);
/* ID -> BinaryCode and HashIndex -> Image_List over all shards (a bucket = the shards' buckets in id order) */
int vc_sharded_get_code(vc_sharded* h, uint32_t id, void* out);
int vc_sharded_get_bucket(vc_sharded* h, uint32_t table, uint32_t index, uint32_t* ids, void* codes, uint32_t cap, uint32_t* n);
/* SearchWorker::find / linear_search for a batch over all shards; arguments as vc_search_knn */
int vc_sharded_search_knn(vc_sharded* h, const void* queries, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order,
                          uint64_t* out, uint32_t* counts, vc_query_stats* stats);
/* Device-resident, stream-ordered form: d_queries (nq*bits/8 bytes), d_out (nq*k), d_counts (nq, may be NULL) and
 * d_stats (nq records, may be NULL) are device memory on the ROOT device (vc_sharded_root_device: the first shard's),
 * `stream` a stream of that device (NULL = its null stream, VC_STREAM_OWN = the handle's own).  The queries reach every
 * other device by one peer copy, the shards of a device run one after the other on that device's stream and the devices
 * concurrently, rows + counts + statistics of a shard travel as one slot (one peer copy per remote shard or one grouped
 * ncclAllGather), the merge kernel reduces the shards' overflow flags on the device (a row whose shard-side recovery
 * gave up reports d_counts[i] == UINT32_MAX, exactly as vc_search_knn_dev does) and a small kernel the statistics.
 * LINEAR: nothing is waited for on the host -- results are valid in stream order.  MIH modes: as in vc_search_knn_dev the
 * host waits inside every shard for its query kernel (lanes of different devices then run on host threads).
 * replaces: search_worker.cc:99-101,177,207 + mpi_coordinator.cc:34-69 for callers that keep the batch in HBM. */
int vc_sharded_search_knn_dev(vc_sharded* h, const void* d_queries, uint32_t nq, uint32_t k, uint32_t mode,
                              uint64_t* d_out, uint32_t* d_counts, vc_query_stats* d_stats, void* stream);
int vc_sharded_root_device(const vc_sharded* h, int* device);
/* All items within full Hamming distance <= radius of each query over all shards; arguments, result layout and
 * VC_ERR_CAPACITY behaviour as vc_search_radius (host buffers).  Every shard searches its id range, the shards' results of a
 * query are brought together and ordered by the radius search's own segment sort on the root device.
 * replaces: search_R_neighbors on every rank + gather_vectors + the master-side dedup (search_worker.cc:177-199,222-264). */
int vc_sharded_search_radius(vc_sharded* h, const void* queries, uint32_t nq, uint32_t radius, uint32_t mode,
                             uint64_t* out, uint64_t out_cap, uint64_t* out_offsets);
/* Device-resident, stream-ordered form: arguments and result layout as vc_search_radius_dev, modes VC_MODE_LINEAR and
 * VC_MODE_MIH_EXACT; d_queries (nq*bits/8 bytes), d_out (out_cap packed values) and d_offsets (nq+1 entries) are device memory on
 * the ROOT device (vc_sharded_root_device), `stream` a stream of that device (NULL = its null stream, VC_STREAM_OWN = the
 * handle's own).  Results of query i, ascending packed, at d_out[d_offsets[i] .. d_offsets[i+1]): those of one vc_engine holding
 * the union, hence those of vc_sharded_search_radius.  VC_ERR_CAPACITY when the union's total exceeds out_cap: d_offsets then
 * holds the needed counts (d_offsets[nq] the total) and d_out is untouched.
 * The queries reach every other device by one peer copy; every non-empty shard runs its own radius search into a buffer of the
 * handle on its device (the shards of a device one after the other, the devices concurrently on host threads), and as in
 * vc_search_radius_dev each of these makes the host wait once for the shard's total -- one wait per shard and call; their sum is
 * the union's total, so nothing further is waited for.  A remote shard's offsets and results travel to the root by one
 * hipMemcpyPeerAsync each -- peer copies whatever vc_sharded_config.exchange says: the lengths vary and only the root needs
 * them -- and shards of the root device are read in place.  Two kernels on the root finish the call: the union's offsets, and a
 * rank merge that places every value by binary searches in the other shards' (ascending, id-disjoint) segments.  There is no
 * padded ring and no size limit besides memory: scratch is proportional to the results found.  The merge may still be running
 * on `stream` when the call returns; results are valid in stream order.
 * replaces: search_R_neighbors on every rank + gather_vectors + the master-side dedup (search_worker.cc:177-199,222-264;
 * mpi_coordinator.cc:34-69) for callers that keep the batch in HBM. */
int vc_sharded_search_radius_dev(vc_sharded* h, const void* d_queries, uint32_t nq, uint32_t radius, uint32_t mode,
                                 uint64_t* d_out, uint64_t out_cap, uint64_t* d_offsets, void* stream);
/* Queries named by id over all shards (search_image_by_id, image_search_client.h:12-27; ID -> BinaryCode, linear_search.cc:45-46):
 * contract, id_flags and batch rules as vc_get_codes_dev / vc_search_knn_ids / vc_search_knn_ids_dev, with "the call underneath"
 * = vc_sharded_search_knn / vc_sharded_search_knn_dev on the handle as it was created -- VC_FLAG_GLOBAL_STOP and
 * VC_FLAG_GLOBAL_APPROX included -- and ids global over the whole store.  Device pointers live on the ROOT device, `stream` is a
 * stream of that device.  Every non-empty shard gathers the ids IT owns into a [nq][bits/64] staging buffer on its own device
 * (zero rows for the others); a remote shard's buffer and found words reach the root by one hipMemcpyPeerAsync -- peer copies
 * whatever vc_sharded_config.exchange says, as in vc_sharded_search_radius_dev -- shards of the root device are read in place, and
 * one kernel on the root ORs the slots (the id ranges are disjoint).  The gather waits for nothing on the host. */
int vc_sharded_get_codes_dev(vc_sharded* h, const uint32_t* d_ids, uint32_t nq, void* d_codes, uint32_t* d_found, void* stream);
int vc_sharded_search_knn_ids(vc_sharded* h, const uint32_t* ids, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order,
                              uint32_t id_flags, uint64_t* out, uint32_t* counts, vc_query_stats* stats);
int vc_sharded_search_knn_ids_dev(vc_sharded* h, const uint32_t* d_ids, uint32_t nq, uint32_t k, uint32_t mode, uint32_t id_flags,
                                  uint64_t* d_out, uint32_t* d_counts, vc_query_stats* d_stats, void* stream);
/* Radius search by id over all shards: contract, id_flags, capacity protocol and batch rules as vc_search_radius_ids_dev /
 * vc_search_radius_ids, with "the call underneath" = vc_sharded_search_radius_dev and ids global over the whole store (an id is not
 * resident when no shard holds it).  Device pointers live on the ROOT device, `stream` is a stream of that device.  The ids are
 * gathered as in vc_sharded_get_codes_dev, the union's uncompacted result lands in a scratch buffer on the root, and the compaction
 * runs there.  VC_FLAG_GLOBAL_STOP and VC_FLAG_GLOBAL_APPROX play no part. */
int vc_sharded_search_radius_ids_dev(vc_sharded* h, const uint32_t* d_ids, uint32_t nq, uint32_t radius, uint32_t mode, uint32_t id_flags,
                                     uint64_t* d_out, uint64_t out_cap, uint64_t* d_offsets, void* stream);
int vc_sharded_search_radius_ids(vc_sharded* h, const uint32_t* ids, uint32_t nq, uint32_t radius, uint32_t mode, uint32_t id_flags,
                                 uint64_t* out, uint64_t out_cap, uint64_t* out_offsets);
/* Near-duplicate clustering over all shards: contract, modes, errors, batch, n_labelled (the companion of vc_sharded_update_index)
 * and stats as vc_cluster_radius_dev / vc_cluster_radius, with N = vc_sharded_size and ids global over the whole store -- the
 * resident ids are contiguous because the id-range shards fill in order.  d_labels lives on the ROOT device, `stream` is a stream
 * of that device.  The search underneath is vc_sharded_search_radius_dev into scratch on the root, the batch's ids are gathered as
 * in vc_sharded_get_codes_dev, and the union runs on the root.  VC_FLAG_GLOBAL_STOP and VC_FLAG_GLOBAL_APPROX play no part. */
int vc_sharded_cluster_radius_dev(vc_sharded* h, uint32_t radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* d_labels,
                                  vc_cluster_stats* stats, void* stream);
int vc_sharded_cluster_radius(vc_sharded* h, uint32_t radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* labels,
                              vc_cluster_stats* stats);
/* Greedy leader dedup over all shards: contract, modes, errors, batch, n_labelled (the companion of vc_sharded_update_index, incoming
 * entries read only), stats and scratch sharing as vc_leaders_radius_dev / vc_leaders_radius, with N = vc_sharded_size and ids global
 * over the whole store.  d_labels lives on the ROOT device, `stream` is a stream of that device.  The search underneath is
 * vc_sharded_search_radius_dev into scratch on the root, the batch's ids are gathered as in vc_sharded_get_codes_dev, and the
 * decision kernels run on the root.  VC_FLAG_GLOBAL_STOP and VC_FLAG_GLOBAL_APPROX play no part.  vc_sharded_retain* with
 * VC_RETAIN_ROOTS consumes the labels unchanged. */
int vc_sharded_leaders_radius_dev(vc_sharded* h, uint32_t radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* d_labels,
                                  vc_leader_stats* stats, void* stream);
int vc_sharded_leaders_radius(vc_sharded* h, uint32_t radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* labels,
                              vc_leader_stats* stats);
/* Density clustering over all shards: contract, kinds, modes, errors, batch, stats and scratch sharing as vc_dbscan_radius_dev /
 * vc_dbscan_radius (no n_labelled form either), with N = vc_sharded_size and ids global over the whole store.  d_labels and d_degrees
 * live on the ROOT device, `stream` is a stream of that device.  The search underneath is vc_sharded_search_radius_dev into scratch
 * on the root, the batch's ids are gathered as in vc_sharded_get_codes_dev, and the three kernels run on the root with global ids.
 * VC_FLAG_GLOBAL_STOP and VC_FLAG_GLOBAL_APPROX play no part.  vc_sharded_retain* with VC_RETAIN_ROOTS consumes the labels unchanged. */
int vc_sharded_dbscan_radius_dev(vc_sharded* h, uint32_t radius, uint32_t min_pts, uint32_t mode, uint32_t batch, uint32_t* d_labels,
                                 uint32_t* d_degrees, vc_dbscan_stats* stats, void* stream);
int vc_sharded_dbscan_radius(vc_sharded* h, uint32_t radius, uint32_t min_pts, uint32_t mode, uint32_t batch, uint32_t* labels,
                             uint32_t* degrees, vc_dbscan_stats* stats);
/* Single-linkage clusters at every radius over all shards: contract, layout, modes, errors, batch, n_labelled, stats and scratch
 * sharing as vc_cluster_levels_dev / vc_cluster_levels, with N = vc_sharded_size and ids global over the whole store.  d_labels
 * lives on the ROOT device, `stream` is a stream of that device.  The search underneath is vc_sharded_search_radius_dev into scratch
 * on the root, the batch's ids are gathered as in vc_sharded_get_codes_dev, and the kernels run on the root with global ids: level r
 * equals bit for bit vc_sharded_cluster_radius* at radius r.  VC_FLAG_GLOBAL_STOP and VC_FLAG_GLOBAL_APPROX play no part. */
int vc_sharded_cluster_levels_dev(vc_sharded* h, uint32_t max_radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* d_labels,
                                  vc_levels_stats* stats, void* stream);
int vc_sharded_cluster_levels(vc_sharded* h, uint32_t max_radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* labels,
                              vc_levels_stats* stats);
/* Density clustering at every radius over all shards: contract, layout, core distances, modes, errors, batch, stats and scratch
 * sharing as vc_dbscan_levels_dev / vc_dbscan_levels (no n_labelled form either), with N = vc_sharded_size and ids global over the
 * whole store.  d_labels and d_core_dist live on the ROOT device, `stream` is a stream of that device.  The search underneath is
 * vc_sharded_search_radius_dev into scratch on the root, the batch's ids are gathered as in vc_sharded_get_codes_dev, and the kernels
 * run on the root with global ids: level r equals bit for bit vc_sharded_dbscan_radius* at radius r.  VC_FLAG_GLOBAL_STOP and
 * VC_FLAG_GLOBAL_APPROX play no part.  vc_sharded_retain* with VC_RETAIN_ROOTS consumes any one level unchanged. */
int vc_sharded_dbscan_levels_dev(vc_sharded* h, uint32_t max_radius, uint32_t min_pts, uint32_t mode, uint32_t batch, uint32_t* d_labels,
                                 uint32_t* d_core_dist, vc_dbscan_levels_stats* stats, void* stream);
int vc_sharded_dbscan_levels(vc_sharded* h, uint32_t max_radius, uint32_t min_pts, uint32_t mode, uint32_t batch, uint32_t* labels,
                             uint32_t* core_dist, vc_dbscan_levels_stats* stats);
/* Label groups summarised over all shards: contract, capacity protocol, errors and scratch as vc_group_summary_dev / vc_group_summary,
 * with N = vc_sharded_size, ids global over the whole store and every pointer of the device form on the ROOT device, `stream` a stream
 * of that device.  The same kernels run on the root; only the rows of a window come through vc_sharded_get_codes_dev instead.
 * Scratch on top of vc_group_summary's (which lies on the root): that gather's own buffers, grow-only on the handle like those of
 * every by-id call -- per device n_shards slots of (VC_GROUP_WINDOW + 1024) x (bits / 8 + 4) bytes, so a small VC_GROUP_WINDOW is
 * the way to bound them with many shards and wide codes (16 shards x 512 bits at the default window: 1.1 GB).  As with every
 * vc_sharded_* call, two calls on one handle must not be in flight on different streams at once.  A group
 * may have its members in any shards: the result equals BIT FOR BIT that of one engine holding the same codes.
 * vc_sharded_retain*(rep_labels, VC_RETAIN_ROOTS) keeps exactly the representatives. */
int vc_sharded_group_summary_dev(vc_sharded* h, const uint32_t* d_labels, uint64_t groups_cap, vc_group* d_groups, void* d_centroids,
                                 uint32_t* d_rep_labels, uint32_t* d_group_index, uint64_t* n_groups, void* stream);
int vc_sharded_group_summary(vc_sharded* h, const uint32_t* labels, uint64_t groups_cap, vc_group* groups, void* centroids, uint32_t* rep_labels,
                             uint32_t* group_index, uint64_t* n_groups);
/* Nearest of K codes over all shards: contract and errors as vc_assign_nearest_dev / vc_assign_nearest, with N = vc_sharded_size,
 * `first` an ordinal of the whole store and every pointer of the device form on the ROOT device, `stream` a stream of that device.
 * The centres reach every other device by one peer copy; every non-empty shard assigns the part of the range it owns on its own
 * device (vc_assign_nearest_dev of its engine); a remote shard's slice of `out` travels to the root by one hipMemcpyPeerAsync behind
 * its lane's event, a root-device shard writes in place.  Nothing is waited for.  The result equals the single engine's bit for bit. */
int vc_sharded_assign_nearest_dev(vc_sharded* h, const void* d_centres, uint32_t n_centres, uint64_t first, uint64_t count, uint64_t* d_out,
                                  void* stream);
int vc_sharded_assign_nearest(vc_sharded* h, const void* centres, uint32_t n_centres, uint64_t first, uint64_t count, uint64_t* out);
/* k-majority over all shards: rule, errors, waits and scratch as vc_kmajority_dev / vc_kmajority with the pointers of the device form on
 * the ROOT device.  The same round driver runs on the root; the assign step is vc_sharded_assign_nearest_dev, the update step
 * vc_sharded_group_summary_dev's.  Centres, assign, labels and statistics equal the single engine's bit for bit. */
int vc_sharded_kmajority_dev(vc_sharded* h, uint32_t n_centres, uint32_t max_iters, void* d_centres, uint64_t* d_assign, uint32_t* d_labels,
                             vc_kmajority_stats* stats, void* stream);
int vc_sharded_kmajority(vc_sharded* h, uint32_t n_centres, uint32_t max_iters, void* centres, uint64_t* assign, uint32_t* labels,
                         vc_kmajority_stats* stats);
/* Seeding over all shards: rule, outputs and errors as vc_seed_centres_dev / vc_seed_centres with N = vc_sharded_size, i the ordinal
 * in the whole store (a shard's first ordinal plus the local index: shards are id ranges in order, so the store's prefix order is
 * the shards' order) and every pointer of the device form on the ROOT device.  Per round the root fetches the chosen record's code
 * from the shard that owns it (vc_sharded_get_codes_dev) straight into centres[t]; every non-empty shard runs the round launch over
 * its own records with that code; the root decides the next pick -- farthest: the maximum of the shards' slot words after
 * translation to store ordinals; weighted: from the shards' totals which shard, then that shard's pick launch with the rest of the
 * target.  WAITS: the root waits once per round for the shards' words (16 bytes each) and, in the weighted mode, a second time for
 * the owning shard's pick; once more at the end.  The result equals the single engine's bit for bit for any shard layout, empty
 * shards included. */
int vc_sharded_seed_centres_dev(vc_sharded* h, uint32_t n_centres, uint32_t method, uint64_t seed, void* d_centres, uint64_t* d_picks,
                                uint64_t* d_assign, vc_seed_stats* stats, void* stream);
int vc_sharded_seed_centres(vc_sharded* h, uint32_t n_centres, uint32_t method, uint64_t seed, void* centres, uint64_t* picks,
                            uint64_t* assign, vc_seed_stats* stats);
/* One result per label group over all shards: rule, outputs, errors, rounds and waits as vc_search_knn_distinct_dev /
 * vc_search_knn_distinct with N = vc_sharded_size and ids global over the whole store.  Every pointer of the device form lives on the
 * ROOT device, `stream` is a stream of that device; labels: all N entries on the root.  The search underneath is
 * vc_sharded_search_knn_dev on the handle as it was created (VC_FLAG_GLOBAL_STOP included); its merged rows are collapsed on the
 * root by the same kernels, so rows, labels, counts and statistics equal the single engine's bit for bit. */
int vc_sharded_search_knn_distinct_dev(vc_sharded* h, const void* d_queries, uint32_t nq, uint32_t k, uint32_t mode,
                                       const uint32_t* d_labels, uint32_t k_first, uint64_t* d_out, uint32_t* d_row_labels,
                                       uint32_t* d_counts, vc_distinct_stats* stats, void* stream);
int vc_sharded_search_knn_distinct(vc_sharded* h, const void* queries, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order,
                                   const uint32_t* labels, uint32_t k_first, uint64_t* out, uint32_t* row_labels, uint32_t* counts,
                                   vc_distinct_stats* stats);
/* borrow shard g's engine (bucket views, timing, files); its id range is [*first_id, *first_id + *n_ids) */
int vc_sharded_shard(vc_sharded* h, uint32_t shard, vc_engine** e, uint64_t* first_id, uint64_t* n_ids);

/* ---- measurement ------------------------------------------------------------------------- */
/* Sums and resets the event records (synchronises with the last recorded call). */
int vc_get_timing(const vc_engine* e, vc_timing* t);
/* Removal over all shards: contract, kinds, errors and failure rule as vc_retain_dev / vc_retain, with N = vc_sharded_size, ids
 * global over the whole store and d_sel / d_new_ids on the ROOT device.  The shards are id ranges filled in order, so after the
 * removal the survivors again fill shard 0, then shard 1, ...: records move from later shards to earlier ones and trailing shards may
 * become empty.  The handle equals, shard for shard, a fresh sharded handle of the same config fed the survivors in order.  Every
 * shard filters its own slice (vc_retain_dev); then, in ascending shard order, a shard receives what it lacks from the front of the
 * following shards (device / peer copies of column slices), which drop that prefix by the same filter.  When every non-empty shard
 * held a current index before, every non-empty shard holds one afterwards: filtered where records only left, brought up to date by
 * vc_update_index where records arrived.  The host waits inside the call.  Argument errors are checked before any work; a failure
 * after the first shard has changed leaves shards that are no longer filled in id order -- destroy the handle then. */
int vc_sharded_retain_dev(vc_sharded* h, const uint32_t* d_sel, uint32_t kind, uint32_t* d_new_ids, uint64_t* n_kept, void* stream);
int vc_sharded_retain(vc_sharded* h, const uint32_t* sel, uint32_t kind, uint32_t* new_ids, uint64_t* n_kept);

/* k-NN among the allowed records over all shards: filter, rule, modes, outputs, errors, routes and waits as
 * vc_search_knn_filtered_dev / vc_search_knn_filtered with N = vc_sharded_size and ids global over the whole store.  Every pointer of
 * the device form lives on the ROOT device; the keep set and every pass run there, the shards are reached only through the store's
 * own search and its gather by id.  The flags that refuse VC_MODE_MIH_EXACT are those of vc_sharded_config.engine. */
int vc_sharded_search_knn_filtered_dev(vc_sharded* h, const void* d_queries, uint32_t nq, uint32_t k, uint32_t mode, const uint32_t* d_sel,
                                       uint32_t kind, uint32_t value, uint32_t k_first, uint64_t* d_out, uint32_t* d_counts,
                                       vc_filter_stats* stats, void* stream);
int vc_sharded_search_knn_filtered(vc_sharded* h, const void* queries, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order,
                                   const uint32_t* sel, uint32_t kind, uint32_t value, uint32_t k_first, uint64_t* out, uint32_t* counts,
                                   vc_filter_stats* stats);

/* k-NN inside each query's own scope over all shards: scopes, rule, outputs, errors and waits as vc_search_knn_scoped_dev /
 * vc_search_knn_scoped with N = vc_sharded_size and ids global over the whole store.  Every pointer of the device form lives on the
 * ROOT device; every pass runs there, the shards are reached only through the store's gather by id. */
int vc_sharded_search_knn_scoped_dev(vc_sharded* h, const void* d_queries, uint32_t nq, uint32_t k, const uint32_t* d_scope,
                                     const uint32_t* d_qscope, uint32_t flags, uint64_t* d_out, uint32_t* d_counts, vc_scope_stats* stats,
                                     void* stream);
int vc_sharded_search_knn_scoped(vc_sharded* h, const void* queries, uint32_t nq, uint32_t k, uint32_t order, const uint32_t* scope,
                                 const uint32_t* qscope, uint32_t flags, uint64_t* out, uint32_t* counts, vc_scope_stats* stats);

/* The exact k-NN graph over all shards: rule, modes, outputs, errors, rounds and waits as vc_knn_graph_dev / vc_knn_graph with
 * N = vc_sharded_size and ids global over the whole store.  Every pointer of the device form lives on the ROOT device; the settle
 * passes run there, the shards are reached only through the store's own search and its gather by id. */
int vc_sharded_knn_graph_dev(vc_sharded* h, uint32_t k, uint32_t mode, uint32_t batch, uint64_t first, uint64_t count, uint32_t k_first,
                             uint64_t* d_rows, uint32_t* d_counts, vc_knn_graph_stats* stats, void* stream);
int vc_sharded_knn_graph(vc_sharded* h, uint32_t k, uint32_t mode, uint32_t batch, uint64_t first, uint64_t count, uint32_t k_first,
                         uint64_t* rows, uint32_t* counts, vc_knn_graph_stats* stats);
/* That graph after vc_sharded_add_codes: contract, steps, stats and errors as vc_knn_graph_update_dev / vc_knn_graph_update.  Every
 * pointer of the device form lives on the ROOT device, where the join, the merge and the scans run; the shards are reached only
 * through the store's own search and its gather by id, so an append that crosses a shard boundary is nothing special. */
int vc_sharded_knn_graph_update_dev(vc_sharded* h, uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first,
                                    uint64_t* d_rows, uint32_t* d_counts, vc_knn_graph_update_stats* stats, void* stream);
int vc_sharded_knn_graph_update(vc_sharded* h, uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first,
                                uint64_t* rows, uint32_t* counts, vc_knn_graph_update_stats* stats);
/* That graph after vc_sharded_retain*: contract, steps, stats and errors as vc_knn_graph_retain_dev / vc_knn_graph_retain.  Every
 * pointer of the device form lives on the ROOT device, where the translation and the scans run; the shards are reached only through
 * the store's own search and its gather by id, so a removal that moves records across a shard boundary is nothing special. */
int vc_sharded_knn_graph_retain_dev(vc_sharded* h, uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first,
                                    const uint32_t* d_new_ids, uint64_t* d_rows, uint32_t* d_counts,
                                    vc_knn_graph_retain_stats* stats, void* stream);
int vc_sharded_knn_graph_retain(vc_sharded* h, uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first,
                                const uint32_t* new_ids, uint64_t* rows, uint32_t* counts, vc_knn_graph_retain_stats* stats);
/* Components and in-degrees of that graph: as vc_cluster_knn_dev / vc_cluster_knn; the rows live on the ROOT device, no shard is
 * touched. */
int vc_sharded_cluster_knn_dev(vc_sharded* h, const uint64_t* d_rows, const uint32_t* d_counts, uint32_t k, uint32_t kk, uint32_t flags,
                               uint32_t max_dist, uint32_t* d_labels, uint32_t* d_in_degree, vc_cluster_knn_stats* stats, void* stream);
int vc_sharded_cluster_knn(vc_sharded* h, const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags,
                           uint32_t max_dist, uint32_t* labels, uint32_t* in_degree, vc_cluster_knn_stats* stats);
/* Shared-nearest-neighbour clusters of that graph: as vc_cluster_snn_dev / vc_cluster_snn; every pointer of the device form lives
 * on the ROOT device, no shard is touched. */
int vc_sharded_cluster_snn_dev(vc_sharded* h, const uint64_t* d_rows, const uint32_t* d_counts, uint32_t k, uint32_t kk, uint32_t flags,
                               uint32_t max_dist, uint32_t min_shared, uint32_t* d_labels, uint32_t* d_shared, uint64_t* d_hist,
                               vc_cluster_snn_stats* stats, void* stream);
int vc_sharded_cluster_snn(vc_sharded* h, const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags,
                           uint32_t max_dist, uint32_t min_shared, uint32_t* labels, uint32_t* shared, uint64_t* hist,
                           vc_cluster_snn_stats* stats);
/* The reverse, mutual or symmetrised graph in CSR form: as vc_knn_adjacency_dev / vc_knn_adjacency; every pointer of the device form
 * lives on the ROOT device, no shard is touched, and the words equal the single engine's. */
int vc_sharded_knn_adjacency_dev(vc_sharded* h, const uint64_t* d_rows, const uint32_t* d_counts, uint32_t k, uint32_t kk, uint32_t flags,
                                 uint32_t max_dist, uint64_t* d_adj, uint64_t adj_cap, uint64_t* d_offsets,
                                 vc_knn_adjacency_stats* stats, void* stream);
int vc_sharded_knn_adjacency(vc_sharded* h, const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags,
                             uint32_t max_dist, uint64_t* adj, uint64_t adj_cap, uint64_t* offsets, vc_knn_adjacency_stats* stats);
/* The minimum spanning forest and the cut of an edge list: as vc_knn_mst_dev / vc_knn_mst / vc_mst_cut_dev / vc_mst_cut; every pointer
 * of the device forms lives on the ROOT device, no shard is touched, and the words equal the single engine's. */
int vc_sharded_knn_mst_dev(vc_sharded* h, const uint64_t* d_rows, const uint32_t* d_counts, uint32_t k, uint32_t kk, uint32_t flags,
                           uint32_t max_dist, uint32_t weight_kind, uint32_t min_pts, vc_mst_edge* d_edges, uint32_t* d_labels,
                           uint64_t* d_hist, vc_knn_mst_stats* stats, void* stream);
int vc_sharded_knn_mst(vc_sharded* h, const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags,
                       uint32_t max_dist, uint32_t weight_kind, uint32_t min_pts, vc_mst_edge* edges, uint32_t* labels, uint64_t* hist,
                       vc_knn_mst_stats* stats);
int vc_sharded_mst_cut_dev(vc_sharded* h, const vc_mst_edge* d_edges, uint64_t n_edges, uint32_t max_weight, uint32_t* d_labels,
                           uint64_t* n_clusters, void* stream);
int vc_sharded_mst_cut(vc_sharded* h, const vc_mst_edge* edges, uint64_t n_edges, uint32_t max_weight, uint32_t* labels,
                       uint64_t* n_clusters);
/* The label vote and label propagation: as vc_knn_vote_dev / vc_knn_vote / vc_label_propagate_dev / vc_label_propagate; every pointer of
 * the device forms lives on the ROOT device, no shard is touched, and the words equal the single engine's. */
int vc_sharded_knn_vote_dev(vc_sharded* h, const uint64_t* d_rows, const uint32_t* d_counts, uint64_t n_rows, uint32_t k, uint32_t kk,
                            uint32_t max_dist, const uint32_t* d_labels, uint32_t weight_kind, uint32_t* d_out_label, uint32_t* d_out_votes,
                            uint32_t* d_out_total, vc_knn_vote_stats* stats, void* stream);
int vc_sharded_knn_vote(vc_sharded* h, const uint64_t* rows, const uint32_t* counts, uint64_t n_rows, uint32_t k, uint32_t kk, uint32_t max_dist,
                        const uint32_t* labels, uint32_t weight_kind, uint32_t* out_label, uint32_t* out_votes, uint32_t* out_total,
                        vc_knn_vote_stats* stats);
int vc_sharded_label_propagate_dev(vc_sharded* h, const uint64_t* d_offsets, const uint64_t* d_adj, uint64_t n_entries, const uint32_t* d_labels_in,
                                   uint32_t weight_kind, uint32_t flags, uint32_t max_iters, uint32_t* d_labels_out, uint32_t* d_votes,
                                   uint32_t* d_total, vc_label_propagate_stats* stats, void* stream);
int vc_sharded_label_propagate(vc_sharded* h, const uint64_t* offsets, const uint64_t* adj, uint64_t n_entries, const uint32_t* labels_in,
                               uint32_t weight_kind, uint32_t flags, uint32_t max_iters, uint32_t* labels_out, uint32_t* votes, uint32_t* total,
                               vc_label_propagate_stats* stats);
/* The condensed tree of a spanning forest and its selection: as vc_mst_condense_dev / vc_mst_condense; every pointer of the device form
 * lives on the ROOT device, no shard is touched, and the words equal the single engine's. */
int vc_sharded_mst_condense_dev(vc_sharded* h, const vc_mst_edge* d_edges, uint64_t n_edges, uint32_t min_cluster_size, uint32_t root_weight,
                                uint32_t method, vc_condensed_node* d_nodes, uint32_t* d_labels, uint32_t* d_node, uint32_t* d_own,
                                uint32_t* d_leave, vc_mst_condense_stats* stats, void* stream);
int vc_sharded_mst_condense(vc_sharded* h, const vc_mst_edge* edges, uint64_t n_edges, uint32_t min_cluster_size, uint32_t root_weight,
                            uint32_t method, vc_condensed_node* nodes, uint32_t* labels, uint32_t* node, uint32_t* own, uint32_t* leave,
                            vc_mst_condense_stats* stats);

/* Stream of the host-pointer calls (default VC_STREAM_OWN). */
int vc_set_stream(vc_engine* e, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VERTICUT_GPU_H */
