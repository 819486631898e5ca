// ============================================================================
// vc_engine.hip -- host side of the C ABI declared in include/verticut_gpu.h.
// Owns the HBM-resident code columns, the per-call work buffers and the launch sequence.
// No CPU compute path exists here: every search runs on the device or fails.
// ============================================================================
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>

#include "vc_distinct_plan.hpp"
#include "vc_filter_plan.hpp"
#include "vc_groups_plan.hpp"
#include "vc_internal.hpp"
#include "vc_knn_graph_plan.hpp"
#include "vc_snn_plan.hpp"
#include "vc_knn_adjacency_plan.hpp"
#include "vc_knn_mst_plan.hpp"
#include "vc_mst_condense_plan.hpp"
#include "vc_vote_plan.hpp"
#include "vc_knn_graph_update_plan.hpp"
#include "vc_mih.hpp"
#include "vc_retain.hpp"

// (the diagnostic build of vc_scan.hip counts the stream form's lower-bound and exact passes: build.py passes the flag to every unit)
#if defined(VC_SCAN_DIAGNOSTICS) && VC_SCAN_DIAGNOSTICS
#define VC_SCAN_STREAM_DIAG 1
#else
#define VC_SCAN_STREAM_DIAG 0
#endif

struct vc_engine {
  vc_config cfg;
  int device = 0;
  uint32_t bits = 0, W = 0, m = 0, sbits = 0, n_cu = 0;
  uint32_t cap = 65536, qtile = 32, scan_blocks = 0;
  bool qtile_auto = true;        // vc_config.query_tile == 0 and no VC_QUERY_TILE: the tile follows the database size (vc_linear_tile)
  uint64_t n = 0, stride = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  uint64_t* d_cols = nullptr;

  // grow-only work buffers
  void* d_stage = nullptr;      size_t stage_bytes = 0;   // ingest staging / query upload
  uint8_t* h_pin = nullptr;     size_t pin_bytes = 0;     // pinned host staging of the host-pointer search calls (queries | rows | counts)
  uint8_t* h_pipe = nullptr;    hipEvent_t pipe_ev[2] = {nullptr, nullptr};   // two pinned chunks: large result sets on their way to pageable memory
  uint64_t* d_q = nullptr;      size_t q_bytes = 0;       // queries [nq][W]
  uint32_t* d_state = nullptr;  size_t state_bytes = 0;   // per group: LinearState (vc_linear_plan.hpp)
  uint64_t* d_ring = nullptr;   size_t ring_bytes = 0;    // per tile: [qt][cap]
  uint64_t* d_out = nullptr;    size_t out_bytes = 0;     // [nq][k]
  uint32_t* d_cnt = nullptr;    size_t cnt_bytes = 0;     // [nq] result counts | [nq] raw ring counts
  // exact-MIH cost-model switch (mih_scan_fallback): gathered queries, their scan rows / counts / settled flags
  uint64_t* d_fq = nullptr;     size_t fq_bytes = 0;
  uint64_t* d_frows = nullptr;  size_t frows_bytes = 0;
  uint32_t* d_fcnt = nullptr;   size_t fcnt_bytes = 0;
  uint32_t* d_rec = nullptr;                              // scratch of the device-side ring-overflow recovery (zero at first use)
  // the scratch of the drivers this engine shares with the sharded store (VcScratch, vc_internal.hpp): the walk's, the groups',
  // k-majority's, seeding's, the distinct search's and the two by-id searches'
  DevBuf scratch[VC_SCRATCH_BUFS];
  CleanState clean;                                       // the last kernel of a linear step hands d_state back zeroed: no memset per step
  uint32_t scan_event_tick = 0;                           // VC_FLAG_LEAN_TIMING: only every timing_sample-th verify launch is timed
  VcKnobs knobs;                                          // environment knobs, read once at vc_create
  uint32_t recover_sabotage = 0;                          // test knob VC_RECOVER_TEST_FAIL: recover launches still to be made to give up

  // timing: event pairs recorded since the last vc_get_timing (calls: whole search calls, scans: verify launches)
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_calls, ev_scans;
  hipEvent_t cur_t0 = nullptr;
  // All search calls share the engine's work buffers, so a call must run after the previous one.  On the same stream
  // that is stream order; when the stream changes, the new call records an event at the tail of the previous stream
  // and waits for it (lazily: the common same-stream loop pays no event at all).
  hipEvent_t last_call = nullptr;
  hipStream_t last_stream = nullptr;
  bool last_stream_valid = false;
  uint64_t scan_bytes = 0;
  vc_timing last{};

  VcScanStream sstream;     // the prefix-sorted scan stream (vc_build_scan_stream); dropped by every call that changes the store
  VcMihIndex* mih = nullptr;
  uint64_t n_indexed = 0;   // records the index covers; n_indexed < n: the index is STALE (kept for vc_update_index, served to no one)
  VcRadiusWork radius_work;
  std::string err;
};

static thread_local std::string g_create_err;

static int fail(vc_engine* e, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (e) e->err = buf; else g_create_err = buf;
  return code;
}

#define VC_HIP(e, call)                                                                         \
  do {                                                                                          \
    hipError_t _r = (call);                                                                     \
    if (_r != hipSuccess)                                                                       \
      return fail(e, _r == hipErrorOutOfMemory ? VC_ERR_NOMEM : VC_ERR_HIP, "%s: %s (%s:%d)", #call, \
                  hipGetErrorString(_r), __FILE__, __LINE__);                                   \
  } while (0)

template <class T>
static int grow(vc_engine* e, T** p, size_t* have, size_t need) {
  if (need <= *have) return VC_OK;
  if (*p) VC_HIP(e, hipFree(*p));
  *p = nullptr;
  *have = 0;
  need = (need + 255) & ~(size_t)255;
  VC_HIP(e, hipMalloc((void**)p, need));
  *have = need;
  return VC_OK;
}

// device memory that lives as long as a scope
template <class T>
struct ScopedDev {
  T* p = nullptr;
  ScopedDev() = default;
  ScopedDev(const ScopedDev&) = delete;
  ScopedDev& operator=(const ScopedDev&) = delete;
  ~ScopedDev() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc((void**)&p, bytes); }
};

// environment knobs (developer / test switches): read here, once per engine (and once per sharded handle), never on a launch path
void read_knobs(VcKnobs* k) {
  if (const char* w = getenv("VC_SCAN_WRAP")) k->scan_wrap = (uint32_t)atoi(w);
  if (const char* w = getenv("VC_SCAN_DIAG")) k->scan_diag = (uint32_t)atoi(w);
  if (const char* w = getenv("VC_SCAN_TRACE")) k->scan_trace = atoi(w) != 0;
  if (const char* w = getenv("VC_SCAN_SHAPE_TRACE")) k->scan_shape_trace = atoi(w) != 0;
  if (const char* w = getenv("VC_SCAN_RESIDENT_MB")) k->resident_mb = std::max(0, atoi(w));
  if (const char* s2 = getenv("VC_SAMPLE2")) { k->sample2_set = true; k->sample2 = strtoull(s2, nullptr, 10); }
  if (const char* s1 = getenv("VC_SAMPLE1")) { k->sample1_set = true; k->sample1 = strtoull(s1, nullptr, 10); }
  if (const char* sh = getenv("VC_SCAN_SHAPE")) {
    int u = 0, b = 0, d = 2;
    if (sscanf(sh, "%d,%d,%d", &u, &b, &d) >= 1) { k->shape_set = true; k->shape_u = u; k->shape_blk = b; k->shape_db = d; }
  }
  if (const char* g = getenv("VC_SAMPLE_BLOCKS_PER_CU")) k->sample_blocks_per_cu = (uint32_t)std::max(1, atoi(g));
  k->recover_trace = getenv("VC_RECOVER_TRACE") != nullptr;
  k->mih_trace = getenv("VC_MIH_TRACE") != nullptr;
  if (const char* r = getenv("VC_DEVICE_RECOVER")) k->device_recover = atoi(r) != 0;
  if (const char* v = getenv("VC_MIH_BCODES")) k->mih_bcodes = atoi(v) != 0;
  if (const char* v = getenv("VC_MIH_BENT")) k->mih_bent = atoi(v) != 0;
  if (const char* v = getenv("VC_MIH_HOST_LOOP")) k->mih_host_loop = atoi(v);
  if (const char* v = getenv("VC_SCAN_SMALL")) k->scan_small = atoi(v);
  if (const char* v = getenv("VC_MIH_BUDGET")) k->mih_budget = strtoull(v, nullptr, 10);
  if (const char* v = getenv("VC_TAU_FOLD")) k->tau_fold = atoi(v);
  if (const char* v = getenv("VC_MIH_STREAM")) k->mih_stream = atoi(v);
  if (const char* v = getenv("VC_MIH_SWITCH")) k->mih_switch = atoi(v);
  if (const char* v = getenv("VC_MIH_PHASES")) k->mih_phases = atoi(v);
  if (const char* v = getenv("VC_MIH_GROUP")) k->mih_group = atoi(v);
  if (const char* v = getenv("VC_MIH_POLL")) k->mih_poll = atoi(v);
  if (const char* v = getenv("VC_MIH_LINES")) k->mih_lines = atoi(v);
  if (const char* v = getenv("VC_MIH_ORDER")) k->mih_order = atoi(v);
  if (const char* v = getenv("VC_MIH_QTILE")) k->mih_qtile = atoi(v);
  if (const char* v = getenv("VC_RECOVER_SPIN_LIMIT")) k->recover_spin_limit = (uint32_t)strtoul(v, nullptr, 10);
  if (const char* v = getenv("VC_RECOVER_TEST_FAIL")) k->recover_test_fail = (uint32_t)strtoul(v, nullptr, 10);
  k->stream_trace = getenv("VC_STREAM_TRACE") != nullptr;
  if (const char* v = getenv("VC_MIH_GS_CAP")) k->gs_cap = (uint32_t)std::max(0, atoi(v));
  k->gs_trace = getenv("VC_MIH_GS_TRACE") != nullptr;
  if (const char* v = getenv("VC_MIH_UPDATE")) k->mih_update = atoi(v);
  if (const char* v = getenv("VC_MIH_RETAIN")) k->mih_retain = atoi(v);
  if (const char* v = getenv("VC_GROUP_WINDOW")) {
    const uint64_t w = strtoull(v, nullptr, 10);
    if (vc_group_window_valid(w)) k->group_window = (uint32_t)w;
  }
  if (const char* v = getenv("VC_ASSIGN_TILE")) k->assign_tile = (uint32_t)strtoul(v, nullptr, 10);
  if (const char* v = getenv("VC_ASSIGN_SLICES")) k->assign_slices = (uint32_t)strtoul(v, nullptr, 10);
  if (const char* v = getenv("VC_DISTINCT_SCRATCH")) k->distinct_scratch = strtoull(v, nullptr, 10);
  if (const char* v = getenv("VC_FILTER_ROUTE")) k->filter_route = (uint32_t)strtoul(v, nullptr, 10);
  if (const char* v = getenv("VC_FILTER_SCRATCH")) k->filter_scratch = strtoull(v, nullptr, 10);
  if (const char* v = getenv("VC_FILTER_WINDOW")) k->filter_window = (uint32_t)strtoul(v, nullptr, 10);
  if (const char* v = getenv("VC_SCOPE_SCRATCH")) k->scope_scratch = strtoull(v, nullptr, 10);
  if (const char* v = getenv("VC_SCOPE_WINDOW")) k->scope_window = (uint32_t)strtoul(v, nullptr, 10);
  if (const char* v = getenv("VC_KGRAPH_SCRATCH")) k->kgraph_scratch = strtoull(v, nullptr, 10);
  if (const char* v = getenv("VC_KGRAPH_OLD_BATCH")) k->kgraph_old_batch = strtoull(v, nullptr, 10);
  if (const char* v = getenv("VC_KGRAPH_WINDOW")) k->kgraph_window = strtoull(v, nullptr, 10);
  if (const char* v = getenv("VC_SCAN_STREAM_FREE")) { k->stream_free_set = true; k->stream_free = strtoull(v, nullptr, 10); }
}

static int bind_device(vc_engine* e) {
  VC_HIP(e, hipSetDevice(e->device));
  return VC_OK;
}
// the index a call may consume: the built one while it covers every resident record, else none.  A stale index (records were added
// since) stays allocated for vc_update_index but every consumer sees "no index", exactly as if the add had freed it.
static VcMihIndex* live_index(const vc_engine* e) { return e->mih && e->n_indexed == e->n ? e->mih : nullptr; }
static void drop_index(vc_engine* e) {
  if (e->mih) vc_mih_free(e->mih);
  e->mih = nullptr;
  e->n_indexed = 0;
}
// the scan stream describes the store as it was built from: every call that changes the store drops it (device of e current)
static void drop_scan_stream(vc_engine* e) {
  if (e->sstream.built()) vc_scan_stream_free(&e->sstream);
}
static hipStream_t caller_stream(const vc_engine* e, void* stream) {   // NULL = the HIP null stream
  return stream == VC_STREAM_OWN ? e->own_stream : (hipStream_t)stream;
}

extern "C" {

int vc_abi_version(void) { return VC_ABI_VERSION; }

const char* vc_strerror(int code) {
  switch (code) {
    case VC_OK: return "ok";
    case VC_NOT_FOUND: return "not found";
    case VC_ERR_INVALID: return "invalid argument";
    case VC_ERR_NO_DEVICE: return "no usable gfx950 device";
    case VC_ERR_HIP: return "HIP runtime error";
    case VC_ERR_NOMEM: return "out of device memory";
    case VC_ERR_STATE: return "call made in the wrong state";
    case VC_ERR_CAPACITY: return "capacity exceeded";
  }
  return "unknown error";
}

const char* vc_last_error(const vc_engine* e) { return e ? e->err.c_str() : g_create_err.c_str(); }

int vc_create(const vc_config* cfg, vc_engine** out) {
  if (!cfg || !out) return fail(nullptr, VC_ERR_INVALID, "null argument");
  *out = nullptr;
  if (cfg->abi_version != VC_ABI_VERSION) return fail(nullptr, VC_ERR_INVALID, "abi_version %u != %u", cfg->abi_version, VC_ABI_VERSION);
  const uint32_t B = cfg->bits;
  if (!(B == 64 || B == 128 || B == 256 || B == 512)) return fail(nullptr, VC_ERR_INVALID, "bits must be 64/128/256/512");
  uint32_t sbits = 0;
  if (cfg->n_tables) {  // search_worker.cc:75 assert(nbytes % size == 0); binaryToInt handles <= 4 bytes
    if ((B / 8) % cfg->n_tables) return fail(nullptr, VC_ERR_INVALID, "code bytes not divisible by n_tables");
    sbits = B / cfg->n_tables;
    if (sbits < 8 || sbits > 32 || sbits % 8) return fail(nullptr, VC_ERR_INVALID, "substring must be 8..32 bits, multiple of 8");
  }
  if (cfg->capacity == 0 || cfg->capacity + (uint64_t)cfg->id_base > 0x100000000ull)
    return fail(nullptr, VC_ERR_INVALID, "capacity must be >0 and id_base+capacity <= 2^32 (ids are uint32)");

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(nullptr, VC_ERR_NO_DEVICE, "no HIP device visible");
  int dev = cfg->device;
  if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return fail(nullptr, VC_ERR_NO_DEVICE, "hipGetDevice failed");
  if (dev >= ndev) return fail(nullptr, VC_ERR_NO_DEVICE, "device %d out of range", dev);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return fail(nullptr, VC_ERR_NO_DEVICE, "hipGetDeviceProperties failed");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, VC_ERR_NO_DEVICE, "device %d is %s; this library carries gfx950 code only", dev, prop.gcnArchName);

  vc_engine* e = new vc_engine();
  e->cfg = *cfg;
  e->device = dev;
  e->bits = B;
  e->W = B / 64;
  e->m = cfg->n_tables;
  e->sbits = sbits;
  e->n_cu = (uint32_t)prop.multiProcessorCount;
  read_knobs(&e->knobs);
  if ((cfg->flags & VC_FLAG_LEAN_TIMING) && cfg->timing_sample > 1) e->knobs.timing_every = cfg->timing_sample;
  e->recover_sabotage = e->knobs.recover_test_fail;
  e->cap = cfg->cand_cap ? cfg->cand_cap : 65536u;
  // queries verified per database pass: 8 keeps the pass on the HBM side of the roofline (bench), larger tiles trade
  // bandwidth efficiency for queries/s until the popcount VALU ceiling; default for big batches: 32
  e->qtile = cfg->query_tile ? cfg->query_tile : 32u;
  e->qtile_auto = cfg->query_tile == 0;
  if (const char* s = getenv("VC_QUERY_TILE")) { e->qtile = (uint32_t)std::max(1, atoi(s)); e->qtile_auto = false; }
  e->scan_blocks = cfg->scan_blocks;
  if (const char* s = getenv("VC_SCAN_BLOCKS")) e->scan_blocks = (uint32_t)std::max(1, atoi(s));
  e->stride = (cfg->capacity + VC_PAD_ITEMS - 1) / VC_PAD_ITEMS * VC_PAD_ITEMS;

  int rc = bind_device(e);
  if (rc == VC_OK) {
    hipError_t r = hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking);
    // Column stride.  The verify kernel streams the W columns side by side, and how well the memory system keeps up
    // depends on the distance between the columns and on where the allocation landed: at 1e9 x 128-bit codes the
    // same kernel streams anywhere from 6.4 to 7.0 TB/s (tools/placement_probe3.py: a stride of exactly 2^30 items
    // is always fast there, 9 * 2^27 items is always slow at 1.2e9 codes, most strides are a lottery per allocation).
    // Nothing about the address hashing is documented, so a big multi-column database is allocated with room for a
    // few candidate strides and each is timed with a streaming read in the verify kernel's access pattern.
    std::vector<uint64_t> cand{e->stride};
    const bool stride_trace = getenv("VC_STRIDE_TRACE") != nullptr;
    const uint64_t col_min = e->stride * sizeof(uint64_t);
    int tries = 6;
    if (const char* t = getenv("VC_STRIDE_TRIES")) tries = std::max(1, atoi(t));   // 1 = take the first
    if (e->W >= 2 && col_min >= (256ull << 20) && tries > 1) {
      uint64_t p2 = VC_PAD_ITEMS;
      while (p2 < cfg->capacity) p2 <<= 1;
      if (p2 - e->stride <= e->stride / 12) cand.push_back(p2);                       // power of two, if it costs < 8 %
      for (int j = 1; (int)cand.size() < tries; ++j) cand.push_back(e->stride + (uint64_t)j * 4 * VC_PAD_ITEMS);   // + j * 256 KiB
    }
    if (const char* f = getenv("VC_STRIDE_FORCE")) {   // test knob: a given stride (items, multiple of 8192, >= capacity)
      const uint64_t fs = strtoull(f, nullptr, 10);
      if (fs >= e->stride && fs % VC_PAD_ITEMS == 0) {
        cand.assign(1, fs);
        e->stride = fs;
      }
    }
    const uint64_t stride_max = *std::max_element(cand.begin(), cand.end());
    const size_t col_bytes = stride_max * e->W * sizeof(uint64_t);
    if (r == hipSuccess) r = hipMalloc((void**)&e->d_cols, col_bytes);
    if (r == hipSuccess) r = hipMemsetAsync(e->d_cols, 0, col_bytes, e->own_stream);
    if (r == hipSuccess) r = hipStreamSynchronize(e->own_stream);
    if (r == hipSuccess && cand.size() > 1) {
      uint64_t* d_sink = nullptr;
      if (hipMalloc((void**)&d_sink, 8) == hipSuccess) {
        float best = -1.f;
        for (uint64_t st : cand) {
          const float ms = vc_probe_stream_ms(e->d_cols, st, e->W, cfg->capacity, d_sink, e->n_cu, e->own_stream);
          if (stride_trace) fprintf(stderr, "[vc stride] %llu items: %.3f ms\n", (unsigned long long)st, ms);
          if (ms > 0 && (best < 0 || ms < best)) {
            best = ms;
            e->stride = st;
          }
        }
        (void)hipFree(d_sink);
      }
    }
    if (r != hipSuccess) rc = fail(nullptr, r == hipErrorOutOfMemory ? VC_ERR_NOMEM : VC_ERR_HIP, "engine setup: %s", hipGetErrorString(r));
  } else {
    g_create_err = e->err;
  }
  if (rc != VC_OK) {
    vc_destroy(e);
    return rc;
  }
  e->stream = e->own_stream;
  *out = e;
  return VC_OK;
}

int vc_destroy(vc_engine* e) {
  if (!e) return VC_OK;
  (void)hipSetDevice(e->device);
  if (e->own_stream) (void)hipStreamSynchronize(e->own_stream);
  if (e->mih) vc_mih_free(e->mih);
  drop_scan_stream(e);
  vc_radius_work_free(&e->radius_work);
  (void)hipFree(e->d_cols);
  (void)hipFree(e->d_stage);
  if (e->h_pin) (void)hipHostFree(e->h_pin);
  if (e->h_pipe) (void)hipHostFree(e->h_pipe);
  for (hipEvent_t ev : e->pipe_ev)
    if (ev) (void)hipEventDestroy(ev);
  (void)hipFree(e->d_q);
  (void)hipFree(e->d_state);
  (void)hipFree(e->d_ring);
  (void)hipFree(e->d_out);
  (void)hipFree(e->d_cnt);
  (void)hipFree(e->d_rec);
  (void)hipFree(e->d_fq);
  (void)hipFree(e->d_frows);
  (void)hipFree(e->d_fcnt);
  for (DevBuf& b : e->scratch) b.release();
  for (hipEvent_t ev : e->ev_pool) (void)hipEventDestroy(ev);
  if (e->last_call) (void)hipEventDestroy(e->last_call);
  if (e->own_stream) (void)hipStreamDestroy(e->own_stream);
  delete e;
  return VC_OK;
}

int vc_set_stream(vc_engine* e, void* stream) {
  if (!e) return VC_ERR_INVALID;
  e->stream = caller_stream(e, stream);
  return VC_OK;
}

int vc_size(const vc_engine* e, uint64_t* n) {
  if (!e || !n) return VC_ERR_INVALID;
  *n = e->n;
  return VC_OK;
}

// ---- ingest (build_hash_tables.cc:40-70: append in file order, id = ordinal) ---------------------
int vc_add_codes(vc_engine* e, const void* codes, uint64_t n) {
  if (!e || (!codes && n)) return VC_ERR_INVALID;
  if (e->n + n > e->cfg.capacity) return fail(e, VC_ERR_CAPACITY, "add %llu codes: %llu + n > capacity %llu", (unsigned long long)n, (unsigned long long)e->n, (unsigned long long)e->cfg.capacity);
  int rc = bind_device(e);
  if (rc) return rc;
  drop_scan_stream(e);
  const size_t rec = e->bits / 8;
  const uint64_t batch = std::max<uint64_t>(1, (64ull << 20) / rec);
  const uint8_t* src = (const uint8_t*)codes;
  for (uint64_t off = 0; off < n; off += batch) {
    const uint64_t cnt = std::min(batch, n - off);
    if ((rc = grow(e, (uint8_t**)&e->d_stage, &e->stage_bytes, cnt * rec))) return rc;
    VC_HIP(e, hipMemcpyAsync(e->d_stage, src + off * rec, cnt * rec, hipMemcpyHostToDevice, e->stream));
    VC_HIP(e, vc_launch_rows_to_cols((const uint64_t*)e->d_stage, e->d_cols, e->stride, e->W, e->n + off, cnt, e->stream));
    VC_HIP(e, hipStreamSynchronize(e->stream));
  }
  e->n += n;   // (an index, if any, is stale from here on: live_index)
  return VC_OK;
}

int vc_add_synthetic(vc_engine* e, uint64_t n, uint64_t seed, uint32_t kind, uint32_t n_centres, uint32_t max_flips) {
  if (!e || kind > VC_SYNTH_CLUSTERED) return VC_ERR_INVALID;
  if (e->n + n > e->cfg.capacity) return fail(e, VC_ERR_CAPACITY, "add_synthetic beyond capacity");
  int rc = bind_device(e);
  if (rc) return rc;
  drop_scan_stream(e);
  VC_HIP(e, vc_launch_fill_synth(e->d_cols, e->stride, e->W, e->n, n, (uint64_t)e->cfg.id_base + e->n, seed, kind, n_centres, max_flips, e->stream));
  VC_HIP(e, hipStreamSynchronize(e->stream));
  e->n += n;   // (an index, if any, is stale from here on: live_index)
  return VC_OK;
}

// ---- the reference's file formats ------------------------------------------------------------------
int vc_load_code_file(vc_engine* e, const char* path, uint64_t max_records, uint64_t* n_read) {
  if (!e || !path) return VC_ERR_INVALID;
  FILE* fh = fopen(path, "rb");
  if (!fh) return fail(e, VC_ERR_INVALID, "Can't open file %s.", path);   // build_hash_tables.cc:30-33
  const size_t rec = e->bits / 8;
  const size_t batch = std::max<size_t>(1, (64u << 20) / rec);
  std::vector<char> buf(batch * rec);
  uint64_t total = 0;
  int rc = VC_OK;
  while (max_records == 0 || total < max_records) {
    const size_t want = max_records ? (size_t)std::min<uint64_t>(batch, max_records - total) : batch;
    const size_t got = fread(buf.data(), rec, want, fh);   // a trailing partial record is ignored, as fread(...,1,fh) does
    if (got == 0) break;
    if ((rc = vc_add_codes(e, buf.data(), got))) break;
    total += got;
  }
  fclose(fh);
  if (n_read) *n_read = total;
  return rc;
}

int vc_save_code_file(vc_engine* e, const char* path) {
  if (!e || !path) return VC_ERR_INVALID;
  int rc = bind_device(e);
  if (rc) return rc;
  FILE* fh = fopen(path, "wb");
  if (!fh) return fail(e, VC_ERR_INVALID, "Can't create file %s.", path);
  const size_t rec = e->bits / 8;
  const uint64_t batch = std::max<uint64_t>(1, (64ull << 20) / rec);
  std::vector<char> buf(batch * rec);
  std::vector<uint32_t> ids(batch);
  for (uint64_t off = 0; off < e->n; off += batch) {
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(batch, e->n - off);
    if ((rc = grow(e, (uint8_t**)&e->d_stage, &e->stage_bytes, (size_t)cnt * (rec + 4)))) break;
    uint32_t* d_ids = (uint32_t*)((uint8_t*)e->d_stage + (size_t)cnt * rec);
    for (uint32_t i = 0; i < cnt; ++i) ids[i] = (uint32_t)(off + i);
    hipError_t r = hipMemcpyAsync(d_ids, ids.data(), (size_t)cnt * 4, hipMemcpyHostToDevice, e->stream);
    if (r == hipSuccess) r = vc_launch_gather_rows(e->d_cols, e->stride, e->W, d_ids, cnt, (uint64_t*)e->d_stage, e->stream);
    if (r == hipSuccess) r = hipMemcpyAsync(buf.data(), e->d_stage, (size_t)cnt * rec, hipMemcpyDeviceToHost, e->stream);
    if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
    if (r != hipSuccess) { rc = fail(e, VC_ERR_HIP, "save: %s", hipGetErrorString(r)); break; }
    if (fwrite(buf.data(), rec, cnt, fh) != cnt) { rc = fail(e, VC_ERR_INVALID, "short write to %s", path); break; }
  }
  fclose(fh);
  return rc;
}

int vc_write_bitmap_file(vc_engine* e, uint32_t table, const char* path) {
  if (!e || !path) return VC_ERR_INVALID;
  if (!live_index(e)) return fail(e, VC_ERR_STATE, "no index built");
  if (table >= e->m) return VC_ERR_INVALID;
  int rc = bind_device(e);
  if (rc) return rc;
  FILE* fh = fopen(path, "wb");
  if (!fh) return fail(e, VC_ERR_INVALID, "Can't create file %s.", path);
  const uint64_t words = (1ull << e->sbits) / 32;
  const uint64_t batch = 16ull << 20;   // 64 MB of words per round
  std::vector<uint32_t> buf((size_t)std::min(words, batch));
  for (uint64_t off = 0; off < words && rc == VC_OK; off += batch) {
    const uint64_t cnt = std::min(batch, words - off);
    rc = vc_mih_bitmap_read(live_index(e), table, off, cnt, buf.data(), e->stream, &e->err);
    if (rc == VC_OK && fwrite(buf.data(), 4, cnt, fh) != cnt) rc = fail(e, VC_ERR_INVALID, "short write to %s", path);
  }
  fclose(fh);
  return rc;
}

// bitmap_deamon.cc:41-65 reads the files generate_bitmap.cc:99-125 wrote back into memory; here the file is checked word
// for word against the bitmap the index derived from the resident records (the two are equal exactly when the file was
// generated from the same code file), which is what "attaching" it means for an index whose rank directory depends on it
int vc_read_bitmap_file(vc_engine* e, uint32_t table, const char* path, uint64_t* n_mismatch_words) {
  if (!e || !path) return VC_ERR_INVALID;
  if (n_mismatch_words) *n_mismatch_words = 0;
  if (!live_index(e)) return fail(e, VC_ERR_STATE, "no index built");
  if (table >= e->m) return VC_ERR_INVALID;
  int rc = bind_device(e);
  if (rc) return rc;
  FILE* fh = fopen(path, "rb");
  if (!fh) return fail(e, VC_ERR_INVALID, "Can't open file %s.", path);   // bitmap_deamon.cc:48-51
  const uint64_t words = (1ull << e->sbits) / 32;
  const uint64_t batch = 16ull << 20;
  std::vector<uint32_t> file_w((size_t)std::min(words, batch)), dev_w((size_t)std::min(words, batch));
  uint64_t bad = 0;
  for (uint64_t off = 0; off < words && rc == VC_OK; off += batch) {
    const uint64_t cnt = std::min(batch, words - off);
    if (fread(file_w.data(), 4, cnt, fh) != cnt) { rc = fail(e, VC_ERR_INVALID, "%s is shorter than 2^%u bits", path, e->sbits); break; }
    rc = vc_mih_bitmap_read(live_index(e), table, off, cnt, dev_w.data(), e->stream, &e->err);
    for (uint64_t i = 0; i < cnt && rc == VC_OK; ++i) bad += file_w[i] != dev_w[i];
  }
  if (rc == VC_OK && fgetc(fh) != EOF) rc = fail(e, VC_ERR_INVALID, "%s is longer than 2^%u bits", path, e->sbits);
  fclose(fh);
  if (n_mismatch_words) *n_mismatch_words = bad;
  if (rc == VC_OK && bad) rc = fail(e, VC_ERR_STATE, "%s differs from the bitmap of the resident records in %llu words", path, (unsigned long long)bad);
  return rc;
}

int vc_save_index(vc_engine* e, const char* path) {
  if (!e || !path) return VC_ERR_INVALID;
  if (!live_index(e)) return fail(e, VC_ERR_STATE, "no index built");
  int rc = bind_device(e);
  if (rc) return rc;
  return vc_mih_save(live_index(e), e->d_cols, e->stride, path, e->stream, &e->err);
}

int vc_load_index(vc_engine* e, const char* path) {
  if (!e || !path) return VC_ERR_INVALID;
  if (e->m == 0) return fail(e, VC_ERR_STATE, "engine was created with n_tables = 0 (linear only)");
  int rc = bind_device(e);
  if (rc) return rc;
  drop_index(e);
  rc = vc_mih_load(&e->mih, path, e->d_cols, e->stride, e->n, e->W, e->m, e->sbits, e->cfg.id_base, e->cfg.flags, e->n_cu, e->cap,
                   e->knobs, e->stream, &e->err);
  if (rc == VC_OK) e->n_indexed = e->n;
  return rc;
}

int vc_get_code(vc_engine* e, uint32_t id, void* out) {
  if (!e || !out) return VC_ERR_INVALID;
  if (id < e->cfg.id_base || (uint64_t)id - e->cfg.id_base >= e->n) return VC_NOT_FOUND;
  int rc = bind_device(e);
  if (rc) return rc;
  const uint64_t local = id - e->cfg.id_base;
  uint64_t w[VC_MAX_W];
  for (uint32_t j = 0; j < e->W; ++j)
    VC_HIP(e, hipMemcpyAsync(&w[j], e->d_cols + j * e->stride + local, 8, hipMemcpyDeviceToHost, e->stream));
  VC_HIP(e, hipStreamSynchronize(e->stream));
  memcpy(out, w, e->bits / 8);
  return VC_OK;
}

// ---- timing helpers -----------------------------------------------------------------------------
// Events live in a grow-only pool and are handed out in pairs; vc_get_timing() sums every pair recorded since
// the previous vc_get_timing() and recycles them.  Beyond VC_MAX_TIMED pairs recording stops (sums stay valid).
#define VC_MAX_TIMED 8192
static hipEvent_t ev_take(vc_engine* e) {
  if (e->ev_used >= 2 * VC_MAX_TIMED) return nullptr;
  if (e->ev_used == e->ev_pool.size()) {
    hipEvent_t ev;
    if (hipEventCreate(&ev) != hipSuccess) return nullptr;
    e->ev_pool.push_back(ev);
  }
  return e->ev_pool[e->ev_used++];
}
static int ev_pair(vc_engine* e, hipEvent_t* a, hipEvent_t* b) {
  *a = ev_take(e);
  *b = *a ? ev_take(e) : nullptr;
  if (*a && !*b) { --e->ev_used; *a = nullptr; }
  return VC_OK;
}
static void timing_begin(vc_engine* e) {
  if (e->last_stream_valid && e->last_stream != e->stream) {
    if (!e->last_call && hipEventCreateWithFlags(&e->last_call, hipEventDisableTiming) != hipSuccess) e->last_call = nullptr;
    // the previous stream may be gone by now (the caller's to destroy): then everything it held has been submitted
    // and a device-wide wait is the safe fallback
    if (!e->last_call || hipEventRecord(e->last_call, e->last_stream) != hipSuccess ||
        hipStreamWaitEvent(e->stream, e->last_call, 0) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipDeviceSynchronize();
    }
  }
  e->cur_t0 = (e->cfg.flags & VC_FLAG_LEAN_TIMING) ? nullptr : ev_take(e);
  if (e->cur_t0) (void)hipEventRecord(e->cur_t0, e->stream);
}
static void timing_end(vc_engine* e) {
  e->last_stream = e->stream;
  e->last_stream_valid = true;
  if (!e->cur_t0) return;
  hipEvent_t t1 = ev_take(e);
  if (!t1) { --e->ev_used; e->cur_t0 = nullptr; return; }
  (void)hipEventRecord(t1, e->stream);
  e->ev_calls.emplace_back(e->cur_t0, t1);
  e->cur_t0 = nullptr;
}

int vc_get_timing(const vc_engine* ce, vc_timing* t) {
  vc_engine* e = const_cast<vc_engine*>(ce);
  if (!e || !t) return VC_ERR_INVALID;
  if (!e->ev_calls.empty() || !e->ev_scans.empty() || e->mih) {
    int rc = bind_device(e);
    if (rc) return rc;
    vc_timing lt{};
    if (e->mih) {
      uint64_t tot[4];
      vc_mih_timing(e->mih, &lt.mih_ms, &lt.mih_launches, tot, e->stream);
      lt.mih_probes = tot[0]; lt.mih_hits = tot[1]; lt.mih_entries = tot[2]; lt.mih_queries = tot[3];
    }
    for (auto& pr : e->ev_calls) {
      float ms = 0;
      VC_HIP(e, hipEventSynchronize(pr.second));
      (void)hipEventElapsedTime(&ms, pr.first, pr.second);
      lt.total_ms += ms;
      lt.calls++;
    }
    for (auto& pr : e->ev_scans) {
      float ms = 0;
      VC_HIP(e, hipEventSynchronize(pr.second));
      (void)hipEventElapsedTime(&ms, pr.first, pr.second);
      lt.scan_ms += ms;
      lt.scan_launches++;
    }
    lt.scan_bytes = e->scan_bytes;
    e->last = lt;
    e->ev_calls.clear();
    e->ev_scans.clear();
    e->ev_used = 0;
    e->scan_bytes = 0;
  }
  *t = e->last;
  return VC_OK;
}

// ---- LINEAR: linear_search.cc:39-64 for a batch of queries ------------------------------------------
struct LinearSearch;
struct LinearGroup {       // the queries of one bootstrap / select / recover: [g0, g0 + gq) of the batch
  uint32_t g0, gq;
  const uint64_t* dq;
  uint64_t* rows;          // [gq][k] ascending (INF padded)
  uint32_t* counts;        // [gq]
  bool fold;               // the verify prologue cuts the bootstrap histograms itself (no vc_tau_init_kernel)
};
struct LinearTile {        // the queries of one verify launch: [t0, t0 + qt) of the group
  uint32_t t0, qt;
  const uint64_t* dq;
  const uint64_t* d_limit;   // nullable: append only packed values <= limit[q] (host-driven recovery)
  const uint32_t* d_shist;   // set: the kernel's prologue cuts the bootstrap histograms itself
  uint64_t shist_cstride;
};
// runs between the select and the recover launch of a group: its rings and cursors are still intact
typedef std::function<int(const LinearSearch& ls, const LinearGroup& g)> LinearHook;

// One linear search call: the plan, the carved state and the launch sequence of a group as named steps.
struct LinearSearch {
  vc_engine* e;
  uint32_t k;
  LinearPlan plan;
  LinearState st;
  bool stream_ok = false;   // the call is a plain k-NN search (vc_search_knn, vc_search_knn_dev*): its small tiles may take the scan stream

  // tile: 0 = the engine's (vc_config.query_tile / VC_QUERY_TILE, else fitted to the database), or the caller's own
  LinearSearch(vc_engine* e_, uint32_t nq, uint32_t k_, uint32_t tile = 0)
      : e(e_), k(k_), plan(plan_in(e_, nq, k_, tile)), st(plan.GQ, plan.hs) {}

  static LinearPlanIn plan_in(const vc_engine* e, uint32_t nq, uint32_t k, uint32_t tile) {
    LinearPlanIn in{};
    in.n = e->n; in.bits = e->bits; in.nq = nq; in.k = k; in.ring_cap = e->cap;
    in.explicit_tile = tile ? tile : (e->qtile_auto ? 0u : e->qtile);
    in.sample1_set = e->knobs.sample1_set; in.sample1 = e->knobs.sample1;   // dev/test knob VC_SAMPLE1
    in.sample2_set = e->knobs.sample2_set; in.sample2 = e->knobs.sample2;   // dev/test knob VC_SAMPLE2
    return in;
  }
  uint32_t* state(size_t word_off) const { return e->d_state + word_off; }

  int open() {   // the engine's grow-only buffers, sized for the plan
    int rc;
    if ((rc = grow(e, &e->d_state, &e->state_bytes, st.state_words * 4))) return rc;
    if ((rc = grow(e, &e->d_ring, &e->ring_bytes, (size_t)plan.GQ * plan.cap * 8))) return rc;
    if (!e->d_rec && e->knobs.device_recover) {
      VC_HIP(e, hipMalloc((void**)&e->d_rec, VcRecoverScratch::words * 4));
      VC_HIP(e, hipMemsetAsync(e->d_rec, 0, VcRecoverScratch::words * 4, e->stream));
    }
    return VC_OK;
  }

  LinearGroup group(const uint64_t* d_q, uint32_t nq, uint32_t g0, uint64_t* d_out, uint32_t* d_cnt) const {
    LinearGroup g{g0, std::min(plan.GQ, nq - g0), d_q + (size_t)g0 * e->W, d_out + (size_t)g0 * k, d_cnt + g0, false};
    // small tiles: the verify kernel's prologue turns the sampled histograms into thresholds itself (one launch less and
    // no coherent read of the threshold lines by every block at start)
    g.fold = !plan.sample2 && e->knobs.tau_fold && vc_scan_is_small(e->W, std::min(plan.QT, g.gq), &e->knobs) &&
             (g.gq % plan.QT == 0 || vc_scan_is_small(e->W, g.gq % plan.QT, &e->knobs));
    return g;
  }
  LinearTile tile(const LinearGroup& g, uint32_t t0) const {
    return LinearTile{t0, std::min(plan.QT, g.gq - t0), g.dq + (size_t)t0 * e->W, nullptr,
                      g.fold ? state(st.at(t0).shist) : nullptr, g.fold ? st.shist_copy_stride(g.gq) : 0};
  }

  // per-step state: zero from the previous step's last kernel, or (first use, new buffer, other layout, after an error) memset now
  int prepare_state() {
    const bool clean = e->knobs.device_recover && e->clean.matches(e->d_state, st);
    e->clean.invalidate();
    if (clean) return VC_OK;
    VC_HIP(e, hipMemsetAsync(e->d_state, 0, e->state_bytes, e->stream));
    VC_HIP(e, hipMemsetAsync(state(st.tau), 0xFF, st.tau_words() * 4, e->stream));   // "no threshold yet"
    return VC_OK;
  }

  int bootstrap(const LinearGroup& g) {
    VcSampleArgs a{};
    a.cols = e->d_cols; a.stride = e->stride; a.s_items = plan.sample; a.W = e->W; a.bits = e->bits; a.k = k;
    a.queries = g.dq; a.qt = g.gq; a.shist = state(st.shist); a.hist_stride = st.hs; a.tau = state(st.tau); a.qs = VC_QUERY_LINE_WORDS;
    a.refine = false; a.cut = !g.fold; a.n_cu = e->n_cu; a.blocks_per_cu = e->knobs.sample_blocks_per_cu;
    VC_HIP(e, vc_launch_sample_hist(a, e->stream));
    if (!plan.sample2) return VC_OK;
    a.s_items = plan.sample2; a.shist = state(st.shist2); a.refine = true; a.cut = true;   // the refining stage
    VC_HIP(e, vc_launch_sample_hist(a, e->stream));
    return VC_OK;
  }

  VcScanParams scan_params(const LinearTile& t, const VcScanShape& sh) const {
    const LinearState::At at = st.at(t.t0);
    VcScanParams p{};
    vc_scan_extent(sh, e->n, e->bits, e->knobs.resident_mb < 0 ? VC_RESIDENT_MB_DEFAULT : (uint64_t)e->knobs.resident_mb, &p);
    p.cols = e->d_cols; p.stride = e->stride; p.n = e->n; p.id_base = e->cfg.id_base; p.bits = e->bits;
    p.qt = t.qt; p.k = k; p.cap = plan.cap; p.hist_stride = st.hs;
    p.queries = t.dq; p.qs = VC_QUERY_LINE_WORDS;
    p.tau = state(at.tau); p.count = state(at.count); p.hist = state(at.hist);
    p.buf = e->d_ring + (size_t)t.t0 * plan.cap;
    p.limit = t.d_limit;
    p.shist = t.d_shist; p.shist_cstride = t.shist_cstride; p.shist_copies = VC_SHIST_COPIES;
    p.wrap = e->knobs.scan_wrap;   // diagnostic build only, results are wrong by design
    p.diag = e->knobs.scan_diag;
    return p;
  }

  // Dev knob VC_SCAN_TRACE, diagnostic build only: the launch with a trace buffer attached -- when does every block of the
  // persistent grid start and end, what did the rare path do -- dumped on stderr.  Synchronises the stream.
  int dump_scan_trace(VcScanParams p, const VcScanShape& sh) {
    const uint32_t trace_blocks = 8192;
    const size_t bytes = trace_blocks * 16 + 256;   // + the rare-path counters
    ScopedDev<uint64_t> d_trace;
    VC_HIP(e, d_trace.alloc(bytes));
    VC_HIP(e, hipMemsetAsync(d_trace.p, 0, bytes, e->stream));
    p.trace = d_trace.p;
    VC_HIP(e, vc_launch_scan(p, sh, e->W, e->n_cu, e->scan_blocks, &e->knobs, e->stream));
    std::vector<uint64_t> h(trace_blocks * 2 + 32);
    VC_HIP(e, hipMemcpyAsync(h.data(), d_trace.p, bytes, hipMemcpyDeviceToHost, e->stream));
    VC_HIP(e, hipStreamSynchronize(e->stream));
    const uint32_t* c = (const uint32_t*)(h.data() + trace_blocks * 2);
    fprintf(stderr, "[scan trace] rare path: %u entries, %u of them appended %u items, %u re-cuts (%u queries)\n", c[0], c[1], c[2], c[3], p.qt);
    fprintf(stderr, "[scan trace] appended items by pass of the chunk loop:");
    for (int i = 0; i < 56; ++i) fprintf(stderr, " %u", c[8 + i]);
    fprintf(stderr, "\n");
    std::vector<double> start, end;
    uint64_t first = UINT64_MAX;
    for (uint32_t i = 0; i < trace_blocks; ++i)
      if (h[2 * i] && h[2 * i + 1]) first = std::min(first, h[2 * i]);
    // per XCD (blocks map to XCDs round-robin, blockIdx % 8): when does its last block end, and the mean end of its blocks
    double mx[8] = {}, sum[8] = {};
    uint32_t cnt[8] = {};
    for (uint32_t i = 0; i < trace_blocks; ++i) {
      if (!h[2 * i] || !h[2 * i + 1]) continue;
      const double en_us = (h[2 * i + 1] - first) * 0.01;   // 100 MHz -> us
      start.push_back((h[2 * i] - first) * 0.01);
      end.push_back(en_us);
      if (h[2 * i + 1] - first < (1ull << 40)) { mx[i & 7] = std::max(mx[i & 7], en_us); sum[i & 7] += en_us; ++cnt[i & 7]; }
    }
    fprintf(stderr, "[scan trace] per XCD last end / mean end us:");
    for (int x = 0; x < 8; ++x) fprintf(stderr, " %.0f/%.0f", mx[x], cnt[x] ? sum[x] / cnt[x] : 0.0);
    fprintf(stderr, "\n");
    if (start.empty()) return VC_OK;
    std::sort(start.begin(), start.end());
    std::sort(end.begin(), end.end());
    auto q = [](const std::vector<double>& v, double f) { return v[(size_t)(f * (v.size() - 1))]; };
    fprintf(stderr, "[scan trace] %zu blocks, qt %u: start us min/p50/p90/max %.1f %.1f %.1f %.1f | end us min/p10/p50/p90/p99/max %.1f %.1f %.1f %.1f %.1f %.1f\n",
            start.size(), p.qt, q(start, 0), q(start, .5), q(start, .9), q(start, 1), q(end, 0), q(end, .1), q(end, .5), q(end, .9), q(end, .99), q(end, 1));
    return VC_OK;
  }

  // The verify launch between two events.  VC_FLAG_LEAN_TIMING with vc_config.timing_sample = N > 1: only every N-th verify
  // launch is bracketed (an event record is a barrier packet, ~4-5 us each; a 125 M-code shard step is 0.35 ms)
  int timed_scan_launch(const VcScanParams& p, const VcScanShape& sh, bool over_stream = false) {
    hipEvent_t a = nullptr, b = nullptr;
    const uint32_t every = (e->cfg.flags & VC_FLAG_LEAN_TIMING) ? std::max(e->cfg.timing_sample, 1u) : 1u;
    if (e->scan_event_tick++ % every == 0) ev_pair(e, &a, &b);
    if (a) VC_HIP(e, hipEventRecord(a, e->stream));
    if (over_stream) {
      const uint64_t resident_mb = e->knobs.resident_mb < 0 ? VC_RESIDENT_MB_DEFAULT : (uint64_t)e->knobs.resident_mb;
      VC_HIP(e, vc_launch_scan_stream(p, e->sstream, resident_mb, e->n_cu, e->scan_blocks, &e->knobs, e->stream));
      e->sstream.launches++;
    } else if (e->knobs.scan_trace) {
      const int rc = dump_scan_trace(p, sh);
      if (rc) return rc;
    } else {
      VC_HIP(e, vc_launch_scan(p, sh, e->W, e->n_cu, e->scan_blocks, &e->knobs, e->stream));
    }
    if (a) {
      VC_HIP(e, hipEventRecord(b, e->stream));
      e->ev_scans.emplace_back(a, b);
      e->scan_bytes += over_stream ? vc_stream_scan_bytes(e->sstream.plan) : e->n * (e->bits / 8);
    }
    return VC_OK;
  }

  // one verify launch for a tile whose thresholds are set (or cut by the launch itself: LinearTile::d_shist)
  int verify(const LinearTile& t) {
    const VcScanShape sh = vc_scan_pick_shape(e->W, t.qt, &e->knobs, plan.shape_n(t.qt));
    // the scan stream serves the small tiles of a plain k-NN search over 128-bit codes; host-driven recovery probes
    // (d_limit) and everything else read the store's own columns
    const bool over_stream = stream_ok && e->sstream.built() && e->bits == 128 && !t.d_limit && vc_scan_stream_tile(t.qt, &e->knobs);
    return timed_scan_launch(scan_params(t, sh), sh, over_stream);
  }

  // rings -> rows and counts (UINT32_MAX == the ring overflowed: the row is only an upper bound until it is recovered)
  int select(const LinearGroup& g) {
    VC_HIP(e, vc_launch_select_ring(e->d_ring, plan.cap, state(st.count), state(st.tau), VC_QUERY_LINE_WORDS, g.gq, k, g.rows, g.counts, e->stream));
    return VC_OK;
  }

  // rows whose ring overflowed are recomputed exactly on the device: a no-op launch otherwise.  One launch serves VC_REC_MAXQ
  // queries (a group is larger only when one tile is: query_tile > 64); as the last kernel of the step it hands the chunk's
  // state back clean (the 16 partial histograms of a group of gq queries sit gq * hs words apart, which is what it is told)
  int recover(const LinearGroup& g) {
    if (!e->knobs.device_recover) return VC_OK;
    for (uint32_t c0 = 0; c0 < g.gq; c0 += VC_REC_MAXQ) {
      const LinearState::At at = st.at(c0);
      VcRecoverArgs a{};
      a.cols = e->d_cols; a.stride = e->stride; a.n = e->n; a.W = e->W; a.id_base = e->cfg.id_base; a.bits = e->bits;
      a.queries = g.dq + (size_t)c0 * e->W; a.nq = std::min(VC_REC_MAXQ, g.gq - c0); a.k = k;
      a.ring = e->d_ring + (size_t)c0 * plan.cap; a.cap = plan.cap;
      a.count = state(at.count); a.hist = state(at.hist); a.hist_stride = st.hs; a.qs = VC_QUERY_LINE_WORDS;
      a.scratch = e->d_rec; a.out = g.rows + (size_t)c0 * k; a.out_count = g.counts + c0;
      a.clean_tau = state(at.tau); a.clean_shist = state(at.shist);
      a.clean_copy_stride = st.shist_copy_stride(g.gq); a.clean_copies = VC_SHIST_COPIES;
      a.n_cu = e->n_cu; a.spin_limit = e->knobs.recover_spin_limit;
      a.absent = e->recover_sabotage ? (e->recover_sabotage--, 1u) : 0u;
      VC_HIP(e, vc_launch_recover(a, e->stream));
    }
    return VC_OK;
  }

  // the recover kernel handed the group's state back clean; the refining stage's histograms (dev knob) are not covered
  void hand_back_clean() {
    if (e->knobs.device_recover && !plan.sample2) e->clean.set(e->d_state, st);
  }

  // d_q: [nq][W] words on the device.  Results: d_out [nq][k] ascending (INF padded), d_cnt[0..nq) counts
  // (UINT32_MAX == the ring overflowed, the device-side recovery did not run or gave up, and the row is only an upper bound).
  int run(const uint64_t* d_q, uint32_t nq, uint64_t* d_out, uint32_t* d_cnt, const LinearHook* after_select = nullptr) {
    int rc = open();
    if (rc) return rc;
    for (uint32_t g0 = 0; g0 < nq; g0 += plan.GQ) {
      const LinearGroup g = group(d_q, nq, g0, d_out, d_cnt);
      if ((rc = prepare_state())) return rc;
      if ((rc = bootstrap(g))) return rc;
      for (uint32_t t0 = 0; t0 < g.gq; t0 += plan.QT)
        if ((rc = verify(tile(g, t0)))) return rc;
      if ((rc = select(g))) return rc;
      // (the exact-MIH switch replays the radius loop's stop rule here)
      if (after_select && (rc = (*after_select)(*this, g))) return rc;
      if ((rc = recover(g))) return rc;
      hand_back_clean();
    }
    return VC_OK;
  }
};

// ---- ring-overflow recovery, host-driven (the interval arithmetic: RecoverInterval, vc_linear_plan.hpp) ----------------
struct RecoverRec {
  uint32_t q;            // query index in the caller's batch
  RecoverInterval iv;
};
struct RecoverBufs {     // one tile's queries, limits, rows and counts
  ScopedDev<uint64_t> q, lim, rows;
  ScopedDev<uint32_t> cnt;
  int alloc(vc_engine* e, uint32_t QT, uint32_t k) {
    hipError_t r;
    if ((r = q.alloc((size_t)QT * e->W * 8)) != hipSuccess || (r = lim.alloc((size_t)QT * 8)) != hipSuccess ||
        (r = rows.alloc((size_t)QT * k * 8)) != hipSuccess || (r = cnt.alloc((size_t)QT * 4)) != hipSuccess)
      return fail(e, VC_ERR_HIP, "ring overflow recovery: hipMalloc: %s", hipGetErrorString(r));
    return VC_OK;
  }
};
struct RecoverRound {    // what one probing scan of a tile brings back
  std::vector<uint64_t> rows;   // [qt][k] the best of what fitted
  std::vector<uint32_t> cnt;    // [qt] their counts
  std::vector<uint32_t> raw;    // [qt] exact number of items <= probe
};

// one scan of qt queries appending only packed values <= their probes; synchronises the stream
static int recover_probe(LinearSearch& ls, RecoverBufs& b, const uint64_t* d_q, RecoverRec* recs, uint32_t qt, RecoverRound* r) {
  vc_engine* e = ls.e;
  const size_t W = e->W;
  const uint32_t k = ls.k;
  std::vector<uint64_t> lim(qt);
  std::vector<uint32_t> tau(qt);
  for (uint32_t i = 0; i < qt; ++i) {
    VC_HIP(e, hipMemcpyAsync(b.q.p + i * W, d_q + (size_t)recs[i].q * W, W * 8, hipMemcpyDeviceToDevice, e->stream));
    lim[i] = recs[i].iv.next_probe();
    tau[i] = (uint32_t)(lim[i] >> 32);
  }
  VC_HIP(e, hipMemsetAsync(e->d_state, 0, ls.st.state_words * 4, e->stream));
  VC_HIP(e, hipMemcpyAsync(b.lim.p, lim.data(), qt * 8, hipMemcpyHostToDevice, e->stream));
  VC_HIP(e, hipMemcpy2DAsync(ls.state(ls.st.tau), VC_QUERY_LINE_WORDS * 4, tau.data(), 4, 4, qt, hipMemcpyHostToDevice, e->stream));
  const LinearGroup g{0, qt, b.q.p, b.rows.p, b.cnt.p, false};
  LinearTile t = ls.tile(g, 0);
  t.d_limit = b.lim.p;
  int rc;
  if ((rc = ls.verify(t))) return rc;
  if ((rc = ls.select(g))) return rc;
  r->rows.resize((size_t)qt * k);
  r->cnt.resize(qt);
  r->raw.resize(qt);
  VC_HIP(e, hipMemcpyAsync(r->rows.data(), b.rows.p, r->rows.size() * 8, hipMemcpyDeviceToHost, e->stream));
  VC_HIP(e, hipMemcpyAsync(r->cnt.data(), b.cnt.p, qt * 4, hipMemcpyDeviceToHost, e->stream));
  VC_HIP(e, hipMemcpy2DAsync(r->raw.data(), 4, ls.state(ls.st.count), VC_QUERY_LINE_WORDS * 4, 4, qt, hipMemcpyDeviceToHost, e->stream));
  VC_HIP(e, hipStreamSynchronize(e->stream));
  return VC_OK;
}

// Rare: more than `cap` items at or below the k-th distance and no device-side recovery.  Every overflowed query keeps a
// RecoverInterval and is scanned again, a tile at a time, until its ring holds everything at or below its probe.
static int linear_recover(vc_engine* e, const uint64_t* d_q, uint32_t k, const std::vector<uint32_t>& over,
                          uint64_t* out /*host [nq][k]*/, uint32_t* cnt /*host [nq]*/) {
  LinearSearch ls(e, (uint32_t)over.size(), k);
  int rc = ls.open();
  if (rc) return rc;
  e->clean.invalidate();   // this path memsets the state itself and leaves it used
  const uint32_t QT = ls.plan.QT;
  RecoverBufs b;
  if ((rc = b.alloc(e, QT, k))) return rc;
  std::vector<RecoverRec> todo;
  for (uint32_t q : over) todo.push_back(RecoverRec{q, RecoverInterval(out[(size_t)q * k + k - 1])});
  const uint64_t want = std::min<uint64_t>(k, e->n);
  for (int round = 0; !todo.empty(); ++round) {
    if (round > VC_RECOVER_MAX_ROUNDS) return fail(e, VC_ERR_CAPACITY, "ring overflow recovery did not converge");
    std::vector<RecoverRec> next;
    for (size_t t0 = 0; t0 < todo.size(); t0 += QT) {
      const uint32_t qt = (uint32_t)std::min<size_t>(QT, todo.size() - t0);
      RecoverRound r;
      if ((rc = recover_probe(ls, b, d_q, &todo[t0], qt, &r))) return rc;
      for (uint32_t i = 0; i < qt; ++i) {
        RecoverRec rec = todo[t0 + i];
        if (e->knobs.recover_trace && i == 0)   // dev knob VC_RECOVER_TRACE
          fprintf(stderr, "[vc recover] round %d query %u: %s probe %016llx -> %llu items (cap %u)\n", round, rec.q,
                  rec.iv.bisect ? "bisect" : "bound ", (unsigned long long)rec.iv.probe, (unsigned long long)r.raw[i], ls.plan.cap);
        const RecoverInterval::Outcome o = rec.iv.update(r.raw[i], r.rows[(size_t)i * k + k - 1], ls.plan.cap, want);
        if (o != RecoverInterval::UNDERSHOOT) {   // a valid row
          memcpy(out + (size_t)rec.q * k, r.rows.data() + (size_t)i * k, (size_t)k * 8);
          cnt[rec.q] = r.cnt[i];
        }
        if (o != RecoverInterval::DONE) next.push_back(rec);
      }
    }
    todo.swap(next);
  }
  return VC_OK;
}

// Cost-model switch of the exact MIH k-NN loop (VcMihScanFallback, vc_mih.hpp): the listed queries are answered by the
// verify kernel in tiles of VC_FALLBACK_TILE and the stop rule of search_worker.cc:201-205 is replayed on each tile's
// candidates (mih_replay_kernel) between the select and the recover launch; with statistics wanted, one more pass over
// the shard counts the items the radius loop would have verified (minimum substring distance <= radius).
static int mih_scan_fallback(void* ctx, const uint64_t* d_q, const uint32_t* d_list, uint32_t n, uint32_t k, uint32_t stop_mult,
                             const VcMihScanTarget& tgt, bool want_stats, uint32_t* d_unresolved, uint32_t* d_n_unresolved, hipStream_t s) {
  vc_engine* e = (vc_engine*)ctx;
  int rc;
  if ((rc = grow(e, &e->d_fq, &e->fq_bytes, (size_t)n * e->W * 8))) return rc;
  if ((rc = grow(e, &e->d_frows, &e->frows_bytes, (size_t)n * k * 8))) return rc;
  if ((rc = grow(e, &e->d_fcnt, &e->fcnt_bytes, (size_t)n * 8))) return rc;
  uint32_t* d_flag = e->d_fcnt + n;
  VC_HIP(e, vc_launch_gather_queries(d_q, d_list, n, e->W, e->d_fq, s));
  const LinearHook replay = [&](const LinearSearch& ls, const LinearGroup& g) -> int {
    VcMihReplayArgs a{};
    a.lin_ring = e->d_ring; a.lin_count = ls.state(ls.st.count); a.rows = g.rows; a.rows_cnt = g.counts;
    a.queries = g.dq; a.list = d_list + g.g0; a.cols = e->d_cols; a.stride = e->stride;
    a.lin_cap = ls.plan.cap; a.lin_qs = VC_QUERY_LINE_WORDS; a.gq = g.gq; a.k = k; a.m = e->m; a.sbits = e->sbits; a.W = e->W;
    a.stop_mult = stop_mult; a.id_base = e->cfg.id_base; a.tgt = tgt; a.unresolved = d_unresolved; a.n_unresolved = d_n_unresolved;
    a.resolved_flag = d_flag + g.g0;
    VC_HIP(e, vc_launch_mih_replay(a, s));
    return VC_OK;
  };
  if ((rc = LinearSearch(e, n, k, VC_FALLBACK_TILE).run(e->d_fq, n, e->d_frows, e->d_fcnt, &replay))) return rc;
  if (want_stats)
    VC_HIP(e, vc_launch_minsub_count(e->d_cols, e->stride, e->n, e->W, e->m, e->sbits, e->d_fq, d_list, d_flag, n, tgt.radius, tgt.seen, e->n_cu, s));
  return VC_OK;
}

// Borrows a stream for one search call on device pointers and brackets the call with its timing events; the engine's own stream
// comes back on every return.
struct StreamCall {
  vc_engine* e;
  hipStream_t saved;
  StreamCall(vc_engine* e_, hipStream_t s) : e(e_), saved(e_->stream) {
    e->stream = s;
    timing_begin(e);
  }
  StreamCall(const StreamCall&) = delete;
  StreamCall& operator=(const StreamCall&) = delete;
  ~StreamCall() {
    timing_end(e);
    e->stream = saved;
  }
};

static int check_knn_args(vc_engine* e, const void* q, uint32_t nq, uint32_t k, uint32_t mode) {
  if (!e || !q || nq == 0) return VC_ERR_INVALID;
  if (k == 0 || k > VC_MAX_K) return fail(e, VC_ERR_INVALID, "k must be in 1..%u", VC_MAX_K);
  if (mode > VC_MODE_MIH_APPROX) return fail(e, VC_ERR_INVALID, "unknown mode %u", mode);
  if (mode != VC_MODE_LINEAR && !live_index(e)) return fail(e, VC_ERR_STATE, "MIH search needs vc_build_index() first (n_tables=%u)", e->m);
  return VC_OK;
}

int vc_search_knn_dev(vc_engine* e, const void* d_queries, uint32_t nq, uint32_t k, uint32_t mode, uint64_t* d_out,
                      uint32_t* d_counts, void* stream) {
  return vc_search_knn_dev_stats(e, d_queries, nq, k, mode, d_out, d_counts, nullptr, stream);
}

}  // extern "C"

// get_stat of a linear scan (vc_search_knn's host loop writes the same): every item was a candidate, nothing was probed
__global__ void vc_linear_stats_kernel(const uint32_t* __restrict__ cnt, uint32_t nq, uint64_t n, vc_query_stats* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  vc_query_stats o{};
  o.n_results = cnt[i];
  o.n_candidates = n;
  out[i] = o;
}

int vc_engine_view(vc_engine* e, VcEngineView* v) {
  if (!e || !v) return VC_ERR_INVALID;
  v->cols = e->d_cols;
  v->stride = e->stride;
  v->n = e->n;
  v->W = e->W;
  v->m = e->m;
  v->sbits = e->sbits;
  v->id_base = e->cfg.id_base;
  v->n_cu = e->n_cu;
  v->reach = live_index(e) ? vc_mih_knn_reach(live_index(e)) : 0;
  return VC_OK;
}

int vc_engine_knn_capped(vc_engine* e, const void* d_queries, uint32_t nq, uint32_t k, uint32_t mode, uint32_t r_cap, uint64_t* d_out,
                         uint32_t* d_counts, vc_query_stats* d_stats, hipStream_t s) {
  if (mode != VC_MODE_MIH_EXACT && mode != VC_MODE_MIH_APPROX) return VC_ERR_INVALID;
  int rc = check_knn_args(e, d_queries, nq, k, mode);
  if (rc) return rc;
  if (!d_out || !d_counts) return VC_ERR_INVALID;
  if ((rc = bind_device(e))) return rc;
  const StreamCall call(e, s);
  const VcMihScanFallback fb{mih_scan_fallback, e, e->n_cu};
  return vc_mih_search(live_index(e), e->d_cols, e->stride, e->n, (const uint64_t*)d_queries, nq, k, mode == VC_MODE_MIH_APPROX, d_out, d_counts, nullptr,
                       e->stream, &e->err, &fb, d_stats, r_cap);
}

int vc_engine_radius_dev(vc_engine* e, const void* d_queries, uint32_t nq, uint32_t radius, uint32_t mode, uint64_t* d_out, uint64_t out_cap,
                         uint64_t* d_offsets, uint64_t* total, hipStream_t s) {
  if (!e || !d_queries || !d_offsets || !total || (!d_out && out_cap) || nq == 0) return VC_ERR_INVALID;
  if (mode != VC_MODE_LINEAR && mode != VC_MODE_MIH_EXACT) return fail(e, VC_ERR_INVALID, "radius search: mode must be LINEAR or MIH_EXACT");
  if (mode == VC_MODE_MIH_EXACT && !live_index(e)) return fail(e, VC_ERR_STATE, "MIH search needs vc_build_index() first");
  int rc = bind_device(e);
  if (rc) return rc;
  const StreamCall call(e, s);
  *total = 0;
  return vc_radius_search(live_index(e), mode == VC_MODE_MIH_EXACT, e->d_cols, e->stride, e->n, e->W, e->cfg.id_base, e->n_cu, &e->knobs,
                          (const uint64_t*)d_queries, nq, radius, d_out, out_cap, d_offsets, true, &e->radius_work, e->stream, &e->err, total);
}

// the search of vc_search_knn_dev_stats on e->stream, inside the caller's StreamCall
static int knn_dev_run(vc_engine* e, const void* d_queries, uint32_t nq, uint32_t k, uint32_t mode, uint64_t* d_out, uint32_t* cnt,
                       vc_query_stats* d_stats, bool stream_ok = false) {
  int rc;
  if (mode == VC_MODE_LINEAR) {
    LinearSearch ls(e, nq, k);
    ls.stream_ok = stream_ok;
    rc = ls.run((const uint64_t*)d_queries, nq, d_out, cnt);
    if (rc == VC_OK && d_stats) {
      hipLaunchKernelGGL(vc_linear_stats_kernel, dim3((nq + 255) / 256), dim3(256), 0, e->stream, (const uint32_t*)cnt, nq, e->n, d_stats);
      if (hipGetLastError() != hipSuccess) rc = fail(e, VC_ERR_HIP, "vc_linear_stats_kernel launch failed");
    }
  } else {
    const VcMihScanFallback fb{mih_scan_fallback, e, e->n_cu};
    rc = vc_mih_search(live_index(e), e->d_cols, e->stride, e->n, (const uint64_t*)d_queries, nq, k, mode == VC_MODE_MIH_APPROX,
                       d_out, cnt, nullptr, e->stream, &e->err, &fb, d_stats);
  }
  return rc;
}

extern "C" {

int vc_search_knn_dev_stats(vc_engine* e, const void* d_queries, uint32_t nq, uint32_t k, uint32_t mode, uint64_t* d_out,
                            uint32_t* d_counts, vc_query_stats* d_stats, void* stream) {
  int rc = check_knn_args(e, d_queries, nq, k, mode);
  if (rc) return rc;
  if (!d_out) return VC_ERR_INVALID;
  if ((rc = bind_device(e))) return rc;
  if ((rc = grow(e, &e->d_cnt, &e->cnt_bytes, (size_t)nq * 8))) return rc;   // outside the timed bracket; grow() uses no stream
  const StreamCall call(e, caller_stream(e, stream));
  return knn_dev_run(e, d_queries, nq, k, mode, d_out, d_counts ? d_counts : e->d_cnt, d_stats, true);
}

}  // extern "C"

// ---- the engine as the drivers it shares with the sharded store see it ---------------------------------------------------------
static VcScratchAlloc scratch_alloc(vc_engine* e) {   // buffer `which` of the engine's table (VcScratch)
  return [e](int which, size_t bytes) -> void* {
    DevBuf& b = e->scratch[which];
    hipError_t r = b.regrow(bytes);
    if (r != hipSuccess) fail(e, r == hipErrorOutOfMemory ? VC_ERR_NOMEM : VC_ERR_HIP, "scratch buffer %d: %s", which, hipGetErrorString(r));
    return r == hipSuccess ? b.p : nullptr;
  };
}

// The view of one call, used inside the caller's StreamCall: everything goes to e->stream, the one device is current throughout.
static VcStoreView store_view(vc_engine* e, uint32_t mode) {
  VcStoreView v;
  v.n = e->n;
  v.id_base = e->cfg.id_base;
  v.W = e->W;
  v.alloc = scratch_alloc(e);
  v.held = [e](int which) { return e->scratch[which].bytes; };
  v.gather = [e](const uint32_t* d_ids, uint32_t nq, uint64_t* d_q, uint32_t* d_found) -> int {
    VC_HIP(e, vc_launch_ids_gather(e->d_cols, e->stride, e->W, e->cfg.id_base, e->n, e->cfg.id_base, e->n, d_ids, nq, d_q, d_found, e->stream));
    return VC_OK;
  };
  v.search = [e, mode](const uint64_t* d_q, uint32_t nq, uint32_t radius, uint64_t* d_raw, uint64_t cap, uint64_t* d_roffs, uint64_t* raw_total) {
    return vc_radius_search(live_index(e), mode == VC_MODE_MIH_EXACT, e->d_cols, e->stride, e->n, e->W, e->cfg.id_base, e->n_cu, &e->knobs, d_q, nq, radius,
                            d_raw, cap, d_roffs, true, &e->radius_work, e->stream, &e->err, raw_total);
  };
  v.knn = [e, mode](const uint64_t* d_q, uint32_t nq, uint32_t kp, uint64_t* d_rows, uint32_t* d_cnt, vc_query_stats* d_stats) {
    return knn_dev_run(e, d_q, nq, kp, mode, d_rows, d_cnt, d_stats);
  };
  return v;
}

// what a driver returned: its own text, if it left one, into the handle (a closure of the view has left its text there itself)
static int driver_done(vc_engine* e, int rc, const std::string& err) { return rc && !err.empty() ? fail(e, rc, "%s", err.c_str()) : rc; }
// An entry point after its checks: the device bound, `run` (a driver's vc_*_run or vc_*_run_host) on stream s inside a StreamCall.
template <class Run>
static int store_call(vc_engine* e, hipStream_t s, const Run& run) {
  int rc = bind_device(e);
  if (rc) return rc;
  const StreamCall call(e, s);
  std::string err;
  rc = run(e->stream, &err);
  return driver_done(e, rc, err);
}

// ---- queries named by id (vc_ids.hip) --------------------------------------------------------------------------------------
static int check_ids_args(vc_engine* e, const uint32_t* ids, uint32_t nq, uint32_t k, uint32_t mode, uint32_t id_flags) {
  int rc = check_knn_args(e, ids, nq, k, mode);
  if (rc) return rc;
  if (id_flags & ~VC_IDS_EXCLUDE_SELF) return fail(e, VC_ERR_INVALID, "unknown id_flags 0x%x", id_flags);
  if ((id_flags & VC_IDS_EXCLUDE_SELF) && k > VC_MAX_K - 1) return fail(e, VC_ERR_INVALID, "k must be in 1..%u with VC_IDS_EXCLUDE_SELF", VC_MAX_K - 1);
  return VC_OK;
}

extern "C" {

int vc_get_codes_dev(vc_engine* e, const uint32_t* d_ids, uint32_t nq, void* d_codes, uint32_t* d_found, void* stream) {
  if (!e || !d_ids || !d_codes || nq == 0) return VC_ERR_INVALID;
  int rc = bind_device(e);
  if (rc) return rc;
  VC_HIP(e, vc_launch_ids_gather(e->d_cols, e->stride, e->W, e->cfg.id_base, e->n, 0, 0, d_ids, nq, (uint64_t*)d_codes, d_found, caller_stream(e, stream)));
  return VC_OK;
}

int vc_search_knn_ids_dev(vc_engine* e, const uint32_t* d_ids, uint32_t nq, uint32_t k, uint32_t mode, uint32_t id_flags, uint64_t* d_out,
                          uint32_t* d_counts, vc_query_stats* d_stats, void* stream) {
  int rc = check_ids_args(e, d_ids, nq, k, mode, id_flags);
  if (rc) return rc;
  if (!d_out) return VC_ERR_INVALID;
  if ((rc = bind_device(e))) return rc;
  const uint32_t kp = vc_ids_kp(k, id_flags);
  const VcStoreView v = store_view(e, mode);
  VcIdsKnnBufs b;
  if ((rc = vc_ids_knn_reserve(v, nq, kp, &b))) return rc;   // outside the timed bracket, as vc_search_knn_dev_stats
  return store_call(e, caller_stream(e, stream), [&](hipStream_t s, std::string* err) {
    return vc_ids_knn_run(v, b, d_ids, nq, kp, k, d_out, d_counts, d_stats, s, err);
  });
}

int vc_search_knn_ids(vc_engine* e, const uint32_t* ids, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order, uint32_t id_flags,
                      uint64_t* out, uint32_t* counts, vc_query_stats* stats) {
  int rc = check_ids_args(e, ids, nq, k, mode, id_flags);
  if (rc) return rc;
  if (!out || order > VC_ORDER_FARTHEST_FIRST) return VC_ERR_INVALID;
  if ((rc = bind_device(e))) return rc;
  const uint32_t kp = vc_ids_kp(k, id_flags);
  const VcStoreView v = store_view(e, mode);
  hipStream_t s = e->stream;
  std::string err;
  rc = vc_ids_knn_run_host(v, VcIdsKnnHostArgs{ids, nq, kp, k, order, mode == VC_MODE_LINEAR, out, counts, stats},
                           [&](const VcIdsKnnBufs& b, const uint32_t* d_ids, uint64_t* d_out, uint32_t* d_counts, vc_query_stats* d_stats) {
                             return store_call(e, s, [&](hipStream_t cs, std::string* cerr) {
                               return vc_ids_knn_run(v, b, d_ids, nq, kp, k, d_out, d_counts, d_stats, cs, cerr);
                             });
                           },
                           [&](const uint64_t* codes, uint64_t* rows, uint32_t* rcnt) {
                             return vc_search_knn(e, codes, nq, kp, mode, VC_ORDER_ASCENDING, rows, rcnt, stats);
                           },
                           s, &err);
  return driver_done(e, rc, err);
}

}  // extern "C"

// ---- radius search for queries named by id (vc_ids_radius.hip) -------------------------------------------------------------------
static int check_radius_ids_args(vc_engine* e, const uint32_t* ids, uint32_t nq, uint32_t mode, uint32_t id_flags, const uint64_t* out,
                                 uint64_t out_cap, const uint64_t* offsets) {
  if (!e || !ids || !offsets || (!out && out_cap) || nq == 0) return VC_ERR_INVALID;
  if (mode != VC_MODE_LINEAR && mode != VC_MODE_MIH_EXACT) return fail(e, VC_ERR_INVALID, "radius search: mode must be LINEAR or MIH_EXACT");
  if (id_flags & ~(VC_IDS_EXCLUDE_SELF | VC_IDS_ONLY_GREATER)) return fail(e, VC_ERR_INVALID, "unknown id_flags 0x%x", id_flags);
  if (mode == VC_MODE_MIH_EXACT && !live_index(e)) return fail(e, VC_ERR_STATE, "MIH search needs vc_build_index() first");
  return VC_OK;
}

int vc_engine_has_index(vc_engine* e) { return e && live_index(e) ? 1 : 0; }

extern "C" {

int vc_search_radius_ids_dev(vc_engine* e, const uint32_t* d_ids, uint32_t nq, uint32_t radius, uint32_t mode, uint32_t id_flags, uint64_t* d_out,
                             uint64_t out_cap, uint64_t* d_offsets, void* stream) {
  int rc = check_radius_ids_args(e, d_ids, nq, mode, id_flags, d_out, out_cap, d_offsets);
  if (rc) return rc;
  return store_call(e, caller_stream(e, stream), [&](hipStream_t s, std::string* err) {
    return vc_ids_radius_run(store_view(e, mode), d_ids, nq, radius, id_flags, d_out, out_cap, d_offsets, s, err);
  });
}

int vc_search_radius_ids(vc_engine* e, const uint32_t* ids, uint32_t nq, uint32_t radius, uint32_t mode, uint32_t id_flags, uint64_t* out,
                         uint64_t out_cap, uint64_t* out_offsets) {
  int rc = check_radius_ids_args(e, ids, nq, mode, id_flags, out, out_cap, out_offsets);
  if (rc) return rc;
  if ((rc = bind_device(e))) return rc;
  const VcStoreView v = store_view(e, mode);
  hipStream_t s = e->stream;
  std::string err;
  rc = vc_ids_radius_run_host(v, ids, nq, out, out_cap, out_offsets,
                              [&](const uint32_t* d_ids, uint64_t* d_out, uint64_t* d_offsets) {
                                return store_call(e, s, [&](hipStream_t cs, std::string* cerr) {
                                  return vc_ids_radius_run(v, d_ids, nq, radius, id_flags, d_out, out_cap, d_offsets, cs, cerr);
                                });
                              },
                              s, &err);
  return driver_done(e, rc, err);
}

}  // extern "C"

// ---- the clustering calls over the radius-graph walk: near-duplicate clusters (vc_cluster.hip), clusters at every radius (vc_levels.hip),
// greedy leaders (vc_leaders.hip), density clustering at one radius (vc_dbscan.hip) and at every radius (vc_dbscan_levels.hip).  The
// drivers are theirs and vc_walk.hip's; here are the argument checks and the entry points. ------------------------
// what: the call's name in the texts.  A call at one radius passes max_radius = 0, one without min_pts 1, one that labels every record
// n_labelled = 0.
static int check_walk_args(vc_engine* e, const char* what, uint32_t max_radius, uint32_t min_pts, uint32_t mode, uint64_t n_labelled, const uint32_t* labels) {
  if (!e || !labels) return VC_ERR_INVALID;
  if (min_pts == 0) return fail(e, VC_ERR_INVALID, "%s: min_pts must be at least 1", what);
  if (mode != VC_MODE_LINEAR && mode != VC_MODE_MIH_EXACT) return fail(e, VC_ERR_INVALID, "%s: mode must be LINEAR or MIH_EXACT", what);
  if (max_radius >= VC_LEVELS_MAX) return fail(e, VC_ERR_INVALID, "%s: max_radius %u exceeds %u", what, max_radius, VC_LEVELS_MAX - 1);
  if (n_labelled > e->n) return fail(e, VC_ERR_INVALID, "%s: n_labelled %llu exceeds the %llu resident records", what, (unsigned long long)n_labelled, (unsigned long long)e->n);
  if (e->n && mode == VC_MODE_MIH_EXACT && !live_index(e)) return fail(e, VC_ERR_STATE, "MIH search needs vc_build_index() first");
  return VC_OK;
}

extern "C" {

int vc_cluster_radius_dev(vc_engine* e, uint32_t radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* d_labels,
                          vc_cluster_stats* stats, void* stream) {
  int rc = check_walk_args(e, "cluster", 0, 1, mode, n_labelled, d_labels);
  if (rc) return rc;
  if (stats) *stats = vc_cluster_stats{0, 0};
  if (e->n == 0) return VC_OK;
  return store_call(e, caller_stream(e, stream), [&](hipStream_t s, std::string* err) {
    return vc_cluster_run(store_view(e, mode), radius, batch, n_labelled, d_labels, stats, s, err);
  });
}

int vc_cluster_radius(vc_engine* e, uint32_t radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* labels, vc_cluster_stats* stats) {
  int rc = check_walk_args(e, "cluster", 0, 1, mode, n_labelled, labels);
  if (rc) return rc;
  if (stats) *stats = vc_cluster_stats{0, 0};
  if (e->n == 0) return VC_OK;
  return store_call(e, e->stream, [&](hipStream_t s, std::string* err) {
    return vc_cluster_run_host(store_view(e, mode), radius, batch, n_labelled, labels, stats, s, err);
  });
}

int vc_cluster_levels_dev(vc_engine* e, uint32_t max_radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* d_labels,
                          vc_levels_stats* stats, void* stream) {
  int rc = check_walk_args(e, "cluster levels", max_radius, 1, mode, n_labelled, d_labels);
  if (rc) return rc;
  if (stats) *stats = vc_levels_stats{};
  if (e->n == 0) return VC_OK;
  return store_call(e, caller_stream(e, stream), [&](hipStream_t s, std::string* err) {
    return vc_levels_run(store_view(e, mode), max_radius, batch, n_labelled, d_labels, stats, s, err);
  });
}

int vc_cluster_levels(vc_engine* e, uint32_t max_radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* labels, vc_levels_stats* stats) {
  int rc = check_walk_args(e, "cluster levels", max_radius, 1, mode, n_labelled, labels);
  if (rc) return rc;
  if (stats) *stats = vc_levels_stats{};
  if (e->n == 0) return VC_OK;
  return store_call(e, e->stream, [&](hipStream_t s, std::string* err) {
    return vc_levels_run_host(store_view(e, mode), max_radius, batch, n_labelled, labels, stats, s, err);
  });
}

int vc_leaders_radius_dev(vc_engine* e, uint32_t radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* d_labels,
                          vc_leader_stats* stats, void* stream) {
  int rc = check_walk_args(e, "leaders", 0, 1, mode, n_labelled, d_labels);
  if (rc) return rc;
  if (stats) *stats = vc_leader_stats{0, 0, 0};
  if (e->n == 0) return VC_OK;
  return store_call(e, caller_stream(e, stream), [&](hipStream_t s, std::string* err) {
    return vc_leaders_run(store_view(e, mode), radius, batch, n_labelled, d_labels, stats, s, err);
  });
}

int vc_leaders_radius(vc_engine* e, uint32_t radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* labels, vc_leader_stats* stats) {
  int rc = check_walk_args(e, "leaders", 0, 1, mode, n_labelled, labels);
  if (rc) return rc;
  if (stats) *stats = vc_leader_stats{0, 0, 0};
  if (e->n == 0) return VC_OK;
  return store_call(e, e->stream, [&](hipStream_t s, std::string* err) {
    return vc_leaders_run_host(store_view(e, mode), radius, batch, n_labelled, labels, stats, s, err);
  });
}

int vc_dbscan_radius_dev(vc_engine* e, uint32_t radius, uint32_t min_pts, uint32_t mode, uint32_t batch, uint32_t* d_labels, uint32_t* d_degrees,
                         vc_dbscan_stats* stats, void* stream) {
  int rc = check_walk_args(e, "dbscan", 0, min_pts, mode, 0, d_labels);
  if (rc) return rc;
  if (stats) *stats = vc_dbscan_stats{0, 0, 0, 0, 0};
  if (e->n == 0) return VC_OK;
  return store_call(e, caller_stream(e, stream), [&](hipStream_t s, std::string* err) {
    return vc_dbscan_run(store_view(e, mode), radius, min_pts, batch, d_labels, d_degrees, stats, s, err);
  });
}

int vc_dbscan_radius(vc_engine* e, uint32_t radius, uint32_t min_pts, uint32_t mode, uint32_t batch, uint32_t* labels, uint32_t* degrees,
                     vc_dbscan_stats* stats) {
  int rc = check_walk_args(e, "dbscan", 0, min_pts, mode, 0, labels);
  if (rc) return rc;
  if (stats) *stats = vc_dbscan_stats{0, 0, 0, 0, 0};
  if (e->n == 0) return VC_OK;
  return store_call(e, e->stream, [&](hipStream_t s, std::string* err) {
    return vc_dbscan_run_host(store_view(e, mode), radius, min_pts, batch, labels, degrees, stats, s, err);
  });
}

int vc_dbscan_levels_dev(vc_engine* e, uint32_t max_radius, uint32_t min_pts, uint32_t mode, uint32_t batch, uint32_t* d_labels, uint32_t* d_core_dist,
                         vc_dbscan_levels_stats* stats, void* stream) {
  int rc = check_walk_args(e, "dbscan levels", max_radius, min_pts, mode, 0, d_labels);
  if (rc) return rc;
  if (stats) *stats = vc_dbscan_levels_stats{};
  if (e->n == 0) return VC_OK;
  return store_call(e, caller_stream(e, stream), [&](hipStream_t s, std::string* err) {
    return vc_dbscan_levels_run(store_view(e, mode), max_radius, min_pts, batch, d_labels, d_core_dist, stats, s, err);
  });
}

int vc_dbscan_levels(vc_engine* e, uint32_t max_radius, uint32_t min_pts, uint32_t mode, uint32_t batch, uint32_t* labels, uint32_t* core_dist,
                     vc_dbscan_levels_stats* stats) {
  int rc = check_walk_args(e, "dbscan levels", max_radius, min_pts, mode, 0, labels);
  if (rc) return rc;
  if (stats) *stats = vc_dbscan_levels_stats{};
  if (e->n == 0) return VC_OK;
  return store_call(e, e->stream, [&](hipStream_t s, std::string* err) {
    return vc_dbscan_levels_run_host(store_view(e, mode), max_radius, min_pts, batch, labels, core_dist, stats, s, err);
  });
}

}  // extern "C"

// ---- label groups summarised (vc_groups.hip) ------------------------------------------------------------------------------------
// the codes of a window on e->stream, inside the caller's StreamCall
static VcGroupsFetch groups_fetch(vc_engine* e) {
  hipStream_t s = e->stream;
  return [e, s](const uint32_t* d_ids, uint32_t nq, uint64_t* d_rows) { return vc_get_codes_dev(e, d_ids, nq, d_rows, nullptr, (void*)s); };
}
static VcGroupsArgs groups_args(vc_engine* e, const uint32_t* d_labels, uint64_t groups_cap, vc_group* d_groups, void* d_centroids, uint32_t* d_rep_labels,
                                uint32_t* d_group_index) {
  return VcGroupsArgs{e->n, e->cfg.id_base, e->W, e->knobs.group_window, d_labels, groups_cap, d_groups, (uint64_t*)d_centroids, d_rep_labels, d_group_index,
                      scratch_alloc(e)};
}

extern "C" {

int vc_group_summary_dev(vc_engine* e, const uint32_t* d_labels, uint64_t groups_cap, vc_group* d_groups, void* d_centroids, uint32_t* d_rep_labels,
                         uint32_t* d_group_index, uint64_t* n_groups, void* stream) {
  if (!e || (!d_labels && e->n) || (!d_groups && groups_cap)) return VC_ERR_INVALID;
  if (n_groups) *n_groups = 0;
  if (e->n == 0) return VC_OK;
  int rc = bind_device(e);
  if (rc) return rc;
  const StreamCall call(e, caller_stream(e, stream));   // (orders the call behind the handle's previous one, whose buffers it may share)
  std::string err;
  rc = vc_groups_run(groups_args(e, d_labels, groups_cap, d_groups, d_centroids, d_rep_labels, d_group_index), groups_fetch(e), n_groups, e->stream, &err);
  return driver_done(e, rc, err);
}

int vc_group_summary(vc_engine* e, const uint32_t* labels, uint64_t groups_cap, vc_group* groups, void* centroids, uint32_t* rep_labels,
                     uint32_t* group_index, uint64_t* n_groups) {
  if (!e || (!labels && e->n) || (!groups && groups_cap)) return VC_ERR_INVALID;
  if (n_groups) *n_groups = 0;
  if (e->n == 0) return VC_OK;
  int rc = bind_device(e);
  if (rc) return rc;
  const StreamCall call(e, e->stream);
  std::string err;
  rc = vc_groups_run_host(groups_args(e, nullptr, groups_cap, nullptr, nullptr, nullptr, nullptr), groups_fetch(e), labels, groups, centroids, rep_labels,
                          group_index, n_groups, e->stream, &err);
  return driver_done(e, rc, err);
}

}  // extern "C"

// ---- nearest of K codes and k-majority (vc_assign.hip) ----------------------------------------------------------------------------
static int check_assign_args(vc_engine* e, const void* centres, uint32_t n_centres, uint64_t first, uint64_t count, const uint64_t* out) {
  if (!e || !centres || n_centres == 0 || first > e->n || count > e->n - first || (!out && count)) return VC_ERR_INVALID;
  return VC_OK;
}
static int check_kmajority_args(vc_engine* e, uint32_t n_centres, uint32_t max_iters, const void* centres, const uint64_t* assign) {
  if (!e || !centres || !assign || n_centres == 0 || (e->n && n_centres > e->n) || max_iters > VC_KMAJ_MAX_ITERS) return VC_ERR_INVALID;
  return VC_OK;
}
// the records [first, first + count) against the centres on e->stream, inside the caller's StreamCall
static VcAssignAll assign_range(vc_engine* e, uint32_t n_centres, uint64_t first, uint64_t count) {
  return [e, n_centres, first, count](const uint64_t* d_centres, uint64_t* d_out) -> int {
    VC_HIP(e, vc_launch_assign(e->d_cols, e->stride, e->W, first, count, d_centres, n_centres, d_out, e->n_cu, &e->knobs, e->stream));
    return VC_OK;
  };
}

extern "C" {

int vc_assign_nearest_dev(vc_engine* e, const void* d_centres, uint32_t n_centres, uint64_t first, uint64_t count, uint64_t* d_out, void* stream) {
  int rc = check_assign_args(e, d_centres, n_centres, first, count, d_out);
  if (rc || count == 0) return rc;
  if ((rc = bind_device(e))) return rc;
  const StreamCall call(e, caller_stream(e, stream));
  return assign_range(e, n_centres, first, count)((const uint64_t*)d_centres, d_out);
}

int vc_assign_nearest(vc_engine* e, const void* centres, uint32_t n_centres, uint64_t first, uint64_t count, uint64_t* out) {
  int rc = check_assign_args(e, centres, n_centres, first, count, out);
  if (rc || count == 0) return rc;
  if ((rc = bind_device(e))) return rc;
  const StreamCall call(e, e->stream);
  std::string err;
  rc = vc_assign_run_host(scratch_alloc(e), e->W, centres, n_centres, count, out, assign_range(e, n_centres, first, count), e->stream, &err);
  return driver_done(e, rc, err);
}

int vc_kmajority_dev(vc_engine* e, uint32_t n_centres, uint32_t max_iters, void* d_centres, uint64_t* d_assign, uint32_t* d_labels,
                     vc_kmajority_stats* stats, void* stream) {
  int rc = check_kmajority_args(e, n_centres, max_iters, d_centres, d_assign);
  if (rc) return rc;
  if (stats) *stats = vc_kmajority_stats{};
  if (e->n == 0) return VC_OK;
  if ((rc = bind_device(e))) return rc;
  const StreamCall call(e, caller_stream(e, stream));
  std::string err;
  rc = vc_kmajority_run(VcKmajArgs{n_centres, max_iters, (uint64_t*)d_centres, d_assign, d_labels, scratch_alloc(e)}, groups_args(e, nullptr, 0, nullptr, nullptr, nullptr, nullptr),
                        assign_range(e, n_centres, 0, e->n), groups_fetch(e), stats, e->stream, &err);
  return driver_done(e, rc, err);
}

int vc_kmajority(vc_engine* e, uint32_t n_centres, uint32_t max_iters, void* centres, uint64_t* assign, uint32_t* labels, vc_kmajority_stats* stats) {
  int rc = check_kmajority_args(e, n_centres, max_iters, centres, assign);
  if (rc) return rc;
  if (stats) *stats = vc_kmajority_stats{};
  if (e->n == 0) return VC_OK;
  if ((rc = bind_device(e))) return rc;
  const StreamCall call(e, e->stream);
  std::string err;
  rc = vc_kmajority_run_host(VcKmajArgs{n_centres, max_iters, nullptr, nullptr, nullptr, scratch_alloc(e)}, groups_args(e, nullptr, 0, nullptr, nullptr, nullptr, nullptr),
                             assign_range(e, n_centres, 0, e->n), groups_fetch(e), centres, assign, labels, stats, e->stream, &err);
  return driver_done(e, rc, err);
}

}  // extern "C"

// ---- device-side seeding (vc_seed.hip) --------------------------------------------------------------------------------------------
static int check_seed_args(vc_engine* e, uint32_t n_centres, uint32_t method, const void* centres) {
  if (!e || !centres || n_centres == 0 || (e->n && n_centres > e->n) || (method != VC_SEED_FARTHEST && method != VC_SEED_WEIGHTED)) return VC_ERR_INVALID;
  return VC_OK;
}
// the whole call on e->stream, inside the caller's StreamCall
static int seed_run(vc_engine* e, uint32_t n_centres, uint32_t method, uint64_t seed, uint64_t* d_centres, uint64_t* d_picks, uint64_t* d_assign,
                    vc_seed_stats* stats) {
  std::string err;
  const int rc = vc_seed_run(VcSeedArgs{e->d_cols, e->stride, e->n, e->W, e->cfg.id_base, n_centres, method, seed, d_centres, d_picks, d_assign, scratch_alloc(e)},
                             stats, e->stream, &err);
  return driver_done(e, rc, err);
}

extern "C" {

int vc_seed_centres_dev(vc_engine* e, uint32_t n_centres, uint32_t method, uint64_t seed, void* d_centres, uint64_t* d_picks, uint64_t* d_assign,
                        vc_seed_stats* stats, void* stream) {
  int rc = check_seed_args(e, n_centres, method, d_centres);
  if (rc) return rc;
  if (stats) *stats = vc_seed_stats{};
  if (e->n == 0) return VC_OK;
  if ((rc = bind_device(e))) return rc;
  const StreamCall call(e, caller_stream(e, stream));
  return seed_run(e, n_centres, method, seed, (uint64_t*)d_centres, d_picks, d_assign, stats);
}

int vc_seed_centres(vc_engine* e, uint32_t n_centres, uint32_t method, uint64_t seed, void* centres, uint64_t* picks, uint64_t* assign,
                    vc_seed_stats* stats) {
  int rc = check_seed_args(e, n_centres, method, centres);
  if (rc) return rc;
  if (stats) *stats = vc_seed_stats{};
  if (e->n == 0) return VC_OK;
  if ((rc = bind_device(e))) return rc;
  const StreamCall call(e, e->stream);
  std::string err;
  rc = vc_seed_run_host(VcSeedHostArgs{e->n, e->W, n_centres, centres, picks, assign, stats, scratch_alloc(e)},
                        [&](uint64_t* d_centres, uint64_t* d_picks, uint64_t* d_assign, vc_seed_stats* st) {
                          return seed_run(e, n_centres, method, seed, d_centres, d_picks, d_assign, st);
                        },
                        e->stream, &err);
  return driver_done(e, rc, err);
}

}  // extern "C"

// ---- one result per label group in k-NN search (vc_distinct.hip) --------------------------------------------------------------------
static int check_distinct_args(vc_engine* e, const void* q, uint32_t nq, uint32_t k, uint32_t mode, const uint32_t* labels, uint32_t k_first,
                               const uint64_t* out) {
  if (!e || !q || !labels || !out || nq == 0) return VC_ERR_INVALID;
  if (k == 0 || k > VC_MAX_K) return fail(e, VC_ERR_INVALID, "k must be in 1..%u", VC_MAX_K);
  if (!vc_distinct_k_first_ok(k, k_first)) return fail(e, VC_ERR_INVALID, "k_first must be 0 or in k..%u", VC_MAX_K);
  if (mode != VC_MODE_LINEAR && mode != VC_MODE_MIH_EXACT) return fail(e, VC_ERR_INVALID, "distinct search: mode must be LINEAR or MIH_EXACT");
  if (mode == VC_MODE_MIH_EXACT && !live_index(e)) return fail(e, VC_ERR_STATE, "MIH search needs vc_build_index() first (n_tables=%u)", e->m);
  return VC_OK;
}
// the whole call on e->stream, inside the caller's StreamCall
static int distinct_run(vc_engine* e, const uint64_t* d_queries, uint32_t nq, uint32_t k, uint32_t mode, const uint32_t* d_labels, uint32_t k_first,
                        uint64_t* d_out, uint32_t* d_row_labels, uint32_t* d_counts, vc_distinct_stats* stats) {
  std::string err;
  const int rc = vc_distinct_run(VcDistinctArgs{e->n, e->cfg.id_base, e->W, d_queries, nq, k, k_first, d_labels, d_out, d_row_labels, d_counts,
                                                e->knobs.distinct_scratch, mode == VC_MODE_MIH_EXACT, scratch_alloc(e)},
                                 store_view(e, mode).knn,
                                 stats, e->stream, &err);
  return driver_done(e, rc, err);
}

extern "C" {

int vc_search_knn_distinct_dev(vc_engine* e, const void* d_queries, uint32_t nq, uint32_t k, uint32_t mode, const uint32_t* d_labels, uint32_t k_first,
                               uint64_t* d_out, uint32_t* d_row_labels, uint32_t* d_counts, vc_distinct_stats* stats, void* stream) {
  int rc = check_distinct_args(e, d_queries, nq, k, mode, d_labels, k_first, d_out);
  if (rc) return rc;
  if ((rc = bind_device(e))) return rc;
  const StreamCall call(e, caller_stream(e, stream));
  return distinct_run(e, (const uint64_t*)d_queries, nq, k, mode, d_labels, k_first, d_out, d_row_labels, d_counts, stats);
}

int vc_search_knn_distinct(vc_engine* e, const void* queries, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order, const uint32_t* labels,
                           uint32_t k_first, uint64_t* out, uint32_t* row_labels, uint32_t* counts, vc_distinct_stats* stats) {
  int rc = check_distinct_args(e, queries, nq, k, mode, labels, k_first, out);
  if (rc) return rc;
  if (order > VC_ORDER_FARTHEST_FIRST) return VC_ERR_INVALID;
  if ((rc = bind_device(e))) return rc;
  const StreamCall call(e, e->stream);
  std::string err;
  rc = vc_distinct_run_host(VcDistinctHostArgs{e->n, e->W, nq, k, order, queries, labels, out, row_labels, counts, stats, scratch_alloc(e)},
                            [&](const uint64_t* d_q, const uint32_t* d_labels, uint64_t* d_out, uint32_t* d_rl, uint32_t* d_cnt, vc_distinct_stats* st) {
                              return distinct_run(e, d_q, nq, k, mode, d_labels, k_first, d_out, d_rl, d_cnt, st);
                            },
                            e->stream, &err);
  return driver_done(e, rc, err);
}

}  // extern "C"

// ---- k-NN among the allowed records (vc_filter.hip) -----------------------------------------------------------------------------------
static int check_filter_args(vc_engine* e, const void* q, uint32_t nq, uint32_t k, uint32_t mode, const uint32_t* sel, uint32_t kind, uint32_t k_first,
                             const uint64_t* out) {
  if (!e || !q || !sel || !out || nq == 0) return VC_ERR_INVALID;
  if (k == 0 || k > VC_MAX_K) return fail(e, VC_ERR_INVALID, "k must be in 1..%u", VC_MAX_K);
  if (!vc_distinct_k_first_ok(k, k_first)) return fail(e, VC_ERR_INVALID, "k_first must be 0 or in k..%u", VC_MAX_K);
  if (kind >= VC_FILTER_KINDS) return fail(e, VC_ERR_INVALID, "filtered search: unknown kind %u", kind);
  if (mode != VC_MODE_LINEAR && mode != VC_MODE_MIH_EXACT) return fail(e, VC_ERR_INVALID, "filtered search: mode must be LINEAR or MIH_EXACT");
  if (mode == VC_MODE_MIH_EXACT && ((e->cfg.flags & VC_FLAG_REF_SIGNEXT_KEYS) || ((e->cfg.flags & VC_FLAG_REF_STOP_LITERAL4) && e->m < 4)))
    return fail(e, VC_ERR_INVALID, "filtered search: MIH_EXACT rows are not the true nearest records under this handle's reference flags");
  if (mode == VC_MODE_MIH_EXACT && !live_index(e)) return fail(e, VC_ERR_STATE, "MIH search needs vc_build_index() first (n_tables=%u)", e->m);
  return VC_OK;
}
static VcFilterArgs filter_args(vc_engine* e, const uint64_t* d_queries, uint32_t nq, uint32_t k, uint32_t mode, const uint32_t* d_sel, uint32_t kind,
                                uint32_t value, uint32_t k_first, uint64_t* d_out, uint32_t* d_counts) {
  return VcFilterArgs{d_queries, nq, k, k_first, d_sel, kind, value, e->W * 64u, d_out, d_counts, e->knobs.filter_scratch, e->knobs.filter_window,
                      e->knobs.filter_route, mode == VC_MODE_MIH_EXACT};
}

extern "C" {

int vc_search_knn_filtered_dev(vc_engine* e, const void* d_queries, uint32_t nq, uint32_t k, uint32_t mode, const uint32_t* d_sel, uint32_t kind, uint32_t value,
                               uint32_t k_first, uint64_t* d_out, uint32_t* d_counts, vc_filter_stats* stats, void* stream) {
  const int rc = check_filter_args(e, d_queries, nq, k, mode, d_sel, kind, k_first, d_out);
  if (rc) return rc;
  return store_call(e, caller_stream(e, stream), [&](hipStream_t s, std::string* err) {
    return vc_filter_run(store_view(e, mode), filter_args(e, (const uint64_t*)d_queries, nq, k, mode, d_sel, kind, value, k_first, d_out, d_counts), stats, s, err);
  });
}

int vc_search_knn_filtered(vc_engine* e, const void* queries, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order, const uint32_t* sel, uint32_t kind,
                           uint32_t value, uint32_t k_first, uint64_t* out, uint32_t* counts, vc_filter_stats* stats) {
  const int rc = check_filter_args(e, queries, nq, k, mode, sel, kind, k_first, out);
  if (rc) return rc;
  if (order > VC_ORDER_FARTHEST_FIRST) return VC_ERR_INVALID;
  return store_call(e, e->stream, [&](hipStream_t s, std::string* err) {
    const VcStoreView v = store_view(e, mode);
    return vc_filter_run_host(v, VcFilterHostArgs{nq, k, order, kind, queries, sel, out, counts},
                              [&](const uint64_t* d_q, const uint32_t* d_sel, uint64_t* d_out, uint32_t* d_cnt) {
                                return vc_filter_run(v, filter_args(e, d_q, nq, k, mode, d_sel, kind, value, k_first, d_out, d_cnt), stats, s, err);
                              },
                              s, err);
  });
}

}  // extern "C"

// ---- k-NN inside each query's own scope (vc_scope.hip): exact brute force, no index, no mode ---------------------------------------------
static int check_scope_args(vc_engine* e, const void* q, uint32_t nq, uint32_t k, const uint32_t* scope, const uint32_t* qscope, uint32_t flags,
                            const uint64_t* out) {
  if (!e || !q || !scope || !qscope || !out || nq == 0) return VC_ERR_INVALID;
  if (k == 0 || k > VC_MAX_K) return fail(e, VC_ERR_INVALID, "k must be in 1..%u", VC_MAX_K);
  if (flags) return fail(e, VC_ERR_INVALID, "scoped search: flags is reserved and must be 0");
  return VC_OK;
}
static VcScopeArgs scope_args(vc_engine* e, const uint64_t* d_queries, uint32_t nq, uint32_t k, const uint32_t* d_scope, const uint32_t* d_qscope,
                              uint64_t* d_out, uint32_t* d_counts) {
  return VcScopeArgs{d_queries, nq, k, d_scope, d_qscope, e->W * 64u, d_out, d_counts, e->knobs.scope_scratch, e->knobs.scope_window};
}

extern "C" {

int vc_search_knn_scoped_dev(vc_engine* e, const void* d_queries, uint32_t nq, uint32_t k, const uint32_t* d_scope, const uint32_t* d_qscope, uint32_t flags,
                             uint64_t* d_out, uint32_t* d_counts, vc_scope_stats* stats, void* stream) {
  const int rc = check_scope_args(e, d_queries, nq, k, d_scope, d_qscope, flags, d_out);
  if (rc) return rc;
  return store_call(e, caller_stream(e, stream), [&](hipStream_t s, std::string* err) {
    return vc_scope_run(store_view(e, VC_MODE_LINEAR), scope_args(e, (const uint64_t*)d_queries, nq, k, d_scope, d_qscope, d_out, d_counts), stats, s, err);
  });
}

int vc_search_knn_scoped(vc_engine* e, const void* queries, uint32_t nq, uint32_t k, uint32_t order, const uint32_t* scope, const uint32_t* qscope,
                         uint32_t flags, uint64_t* out, uint32_t* counts, vc_scope_stats* stats) {
  const int rc = check_scope_args(e, queries, nq, k, scope, qscope, flags, out);
  if (rc) return rc;
  if (order > VC_ORDER_FARTHEST_FIRST) return VC_ERR_INVALID;
  return store_call(e, e->stream, [&](hipStream_t s, std::string* err) {
    const VcStoreView v = store_view(e, VC_MODE_LINEAR);
    return vc_scope_run_host(v, VcScopeHostArgs{nq, k, order, queries, scope, qscope, out, counts},
                             [&](const uint64_t* d_q, const uint32_t* d_scope, const uint32_t* d_qscope, uint64_t* d_out, uint32_t* d_cnt) {
                               return vc_scope_run(v, scope_args(e, d_q, nq, k, d_scope, d_qscope, d_out, d_cnt), stats, s, err);
                             },
                             s, err);
  });
}

}  // extern "C"

// ---- the exact k-NN graph of the store and its components (vc_knn_graph.hip) ---------------------------------------------------------------
static int check_kgraph_args(vc_engine* e, uint32_t k, uint32_t mode, uint64_t first, uint64_t count, uint32_t k_first, const uint64_t* rows, uint64_t* n_rows) {
  if (!e || !rows) return VC_ERR_INVALID;
  if (!vc_kgraph_k_ok(k)) return fail(e, VC_ERR_INVALID, "k-NN graph: k must be in 1..%u", VC_MAX_K - 1);
  if (!vc_kgraph_k_first_ok(k, k_first)) return fail(e, VC_ERR_INVALID, "k-NN graph: k_first must be 0 or in k+1..%u", VC_MAX_K);
  if (mode != VC_MODE_LINEAR && mode != VC_MODE_MIH_EXACT) return fail(e, VC_ERR_INVALID, "k-NN graph: mode must be LINEAR or MIH_EXACT");
  if (!vc_kgraph_range(e->n, first, count, n_rows))
    return fail(e, VC_ERR_INVALID, "k-NN graph: first %llu + count %llu exceeds the %llu resident records", (unsigned long long)first, (unsigned long long)count,
                (unsigned long long)e->n);
  if (e->n && mode == VC_MODE_MIH_EXACT && !live_index(e)) return fail(e, VC_ERR_STATE, "MIH search needs vc_build_index() first (n_tables=%u)", e->m);
  return VC_OK;
}
static VcKgraphArgs kgraph_args(vc_engine* e, uint32_t k, uint32_t mode, uint32_t batch, uint64_t first, uint64_t n_rows, uint32_t k_first, uint64_t* d_rows,
                                uint32_t* d_counts) {
  return VcKgraphArgs{k, k_first, batch, mode == VC_MODE_LINEAR, first, n_rows, d_rows, d_counts, e->knobs.kgraph_scratch};
}
static int check_cluster_knn_args(vc_engine* e, const uint64_t* rows, uint32_t k, uint32_t kk, uint32_t flags, const uint32_t* labels) {
  if (!e || !rows || !labels) return VC_ERR_INVALID;
  if (!vc_kgraph_k_ok(k)) return fail(e, VC_ERR_INVALID, "k-NN clusters: k must be in 1..%u", VC_MAX_K - 1);
  if (kk == 0 || kk > k) return fail(e, VC_ERR_INVALID, "k-NN clusters: kk must be in 1..k");
  if (flags & ~VC_KNN_EITHER) return fail(e, VC_ERR_INVALID, "k-NN clusters: unknown flags 0x%x", flags);
  return VC_OK;
}
static int check_cluster_snn_args(vc_engine* e, const uint64_t* rows, uint32_t k, uint32_t kk, uint32_t flags, const uint32_t* labels) {
  if (!e || !rows || !labels) return VC_ERR_INVALID;
  if (!vc_kgraph_k_ok(k)) return fail(e, VC_ERR_INVALID, "SNN clusters: k must be in 1..%u", VC_MAX_K - 1);
  if (!vc_snn_kk_ok(k, kk)) return fail(e, VC_ERR_INVALID, "SNN clusters: kk must be in 1..min(k, %u)", VC_SNN_MAX_KK);
  if (!vc_snn_flags_ok(flags)) return fail(e, VC_ERR_INVALID, "SNN clusters: unknown flags 0x%x", flags);
  return VC_OK;
}
static int check_knn_adjacency_args(vc_engine* e, const uint64_t* rows, uint32_t k, uint32_t kk, uint32_t flags, const uint64_t* adj, uint64_t adj_cap,
                                    const uint64_t* offsets) {
  if (!e || !rows || !offsets || (!adj && adj_cap)) return VC_ERR_INVALID;
  if (!vc_kgraph_k_ok(k)) return fail(e, VC_ERR_INVALID, "k-NN adjacency: k must be in 1..%u", VC_MAX_K - 1);
  if (!vc_adj_kk_ok(k, kk)) return fail(e, VC_ERR_INVALID, "k-NN adjacency: kk must be in 1..k");
  if (!vc_adj_flags_ok(flags)) return fail(e, VC_ERR_INVALID, "k-NN adjacency: unknown flags 0x%x", flags);
  if (!vc_adj_items_ok(e->n, kk)) return fail(e, VC_ERR_INVALID, "k-NN adjacency: N * kk must not exceed 2^31 - 1");
  return VC_OK;
}
static int check_knn_mst_args(vc_engine* e, const uint64_t* rows, uint32_t k, uint32_t kk, uint32_t flags, uint32_t weight_kind, uint32_t min_pts,
                              const vc_mst_edge* edges) {
  if (!e || !rows || !edges) return VC_ERR_INVALID;
  if (!vc_kgraph_k_ok(k)) return fail(e, VC_ERR_INVALID, "k-NN spanning forest: k must be in 1..%u", VC_MAX_K - 1);
  if (!vc_mst_kk_ok(k, kk)) return fail(e, VC_ERR_INVALID, "k-NN spanning forest: kk must be in 1..k");
  if (!vc_mst_flags_ok(flags)) return fail(e, VC_ERR_INVALID, "k-NN spanning forest: flags must be VC_KNN_MUTUAL or VC_KNN_EITHER, not 0x%x", flags);
  if (!vc_mst_kind_ok(weight_kind)) return fail(e, VC_ERR_INVALID, "k-NN spanning forest: unknown weight_kind %u", weight_kind);
  if (!vc_mst_min_pts_ok(weight_kind, k, min_pts))
    return fail(e, VC_ERR_INVALID, "k-NN spanning forest: min_pts must be 1 under VC_MST_DISTANCE and in 1..k+1 under VC_MST_REACHABILITY");
  if (!vc_mst_items_ok(e->n, kk)) return fail(e, VC_ERR_INVALID, "k-NN spanning forest: N * kk must not exceed 2^31 - 1");
  return VC_OK;
}
static int check_mst_cut_args(vc_engine* e, const vc_mst_edge* edges, uint64_t n_edges, const uint32_t* labels) {
  if (!e || !labels || (!edges && n_edges)) return VC_ERR_INVALID;
  return VC_OK;
}
static int check_mst_condense_args(vc_engine* e, const vc_mst_edge* edges, uint64_t n_edges, uint32_t mcs, uint32_t root_weight, uint32_t method,
                                   const vc_condensed_node* nodes, const uint32_t* labels) {
  if (!e || !labels || !nodes || (!edges && n_edges)) return VC_ERR_INVALID;
  if (!vc_cond_edges_ok(e->n, n_edges)) return fail(e, VC_ERR_INVALID, "condensed tree: a forest over N records has at most max(N, 1) - 1 edges");
  if (!vc_cond_mcs_ok(mcs)) return fail(e, VC_ERR_INVALID, "condensed tree: min_cluster_size must be in 2..2^31");
  if (!vc_cond_root_weight_ok(root_weight, e->bits)) return fail(e, VC_ERR_INVALID, "condensed tree: root_weight must not exceed bits + 1");
  if (!vc_cond_method_ok(method)) return fail(e, VC_ERR_INVALID, "condensed tree: unknown method %u", method);
  return VC_OK;
}
static int check_knn_vote_args(vc_engine* e, const uint64_t* rows, uint32_t k, uint32_t kk, const uint32_t* labels, uint32_t weight_kind, const uint32_t* out_label) {
  if (!e || !rows || !labels || !out_label) return VC_ERR_INVALID;
  if (!vc_vote_k_ok(k, VC_MAX_K)) return fail(e, VC_ERR_INVALID, "label vote: k must be in 1..%u", VC_MAX_K);
  if (!vc_vote_kk_ok(k, kk)) return fail(e, VC_ERR_INVALID, "label vote: kk must be in 1..k");
  if (!vc_vote_kind_ok(weight_kind)) return fail(e, VC_ERR_INVALID, "label vote: unknown weight_kind %u", weight_kind);
  return VC_OK;
}
static int check_label_propagate_args(vc_engine* e, const uint64_t* offsets, const uint64_t* adj, uint64_t n_entries, const uint32_t* labels_in,
                                      uint32_t weight_kind, uint32_t flags, uint32_t max_iters, const uint32_t* labels_out) {
  if (!e || !offsets || (!adj && n_entries) || !labels_in || !labels_out) return VC_ERR_INVALID;
  if (!vc_vote_kind_ok(weight_kind)) return fail(e, VC_ERR_INVALID, "label propagation: unknown weight_kind %u", weight_kind);
  if (!vc_vote_lp_flags_ok(flags)) return fail(e, VC_ERR_INVALID, "label propagation: unknown flags 0x%x", flags);
  if (!vc_vote_iters_ok(max_iters)) return fail(e, VC_ERR_INVALID, "label propagation: max_iters must be in 1..%u", VC_LP_MAX_ITERS);
  return VC_OK;
}
// a built graph after vc_add_codes (vc_knn_graph_update.hip): vc_knn_graph*'s checks with n_old as the first position
static int check_kgupd_args(vc_engine* e, uint32_t k, uint32_t mode, uint64_t n_old, uint32_t k_first, const uint64_t* rows) {
  uint64_t n_rows = 0;
  if (!e || !rows) return VC_ERR_INVALID;
  if (n_old > e->n)
    return fail(e, VC_ERR_INVALID, "k-NN graph update: n_old %llu exceeds the %llu resident records", (unsigned long long)n_old, (unsigned long long)e->n);
  return check_kgraph_args(e, k, mode, n_old, 0, k_first, rows, &n_rows);
}
static VcKgupdArgs kgupd_args(vc_engine* e, uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first, uint64_t* d_rows, uint32_t* d_counts) {
  return VcKgupdArgs{kgraph_args(e, k, mode, batch, n_old, e->n - n_old, k_first, d_rows ? d_rows + n_old * k : nullptr, d_counts ? d_counts + n_old : nullptr),
                     n_old, d_rows, d_counts, e->knobs.kgraph_scratch, vc_kgupd_old_batch(e->knobs.kgraph_old_batch), vc_kgupd_window(e->knobs.kgraph_window)};
}
// a built graph after vc_retain* (vc_knn_graph_retain.hip): vc_knn_graph*'s checks over the store as it is now
static int check_kgret_args(vc_engine* e, uint32_t k, uint32_t mode, uint64_t n_old, uint32_t k_first, const uint32_t* new_ids, const uint64_t* rows) {
  uint64_t n_rows = 0;
  if (!e || !rows || !new_ids) return VC_ERR_INVALID;
  const int rc = check_kgraph_args(e, k, mode, 0, 0, k_first, rows, &n_rows);
  if (rc) return rc;
  if (n_old < e->n)
    return fail(e, VC_ERR_INVALID, "k-NN graph retain: n_old %llu is below the %llu resident records", (unsigned long long)n_old, (unsigned long long)e->n);
  return VC_OK;
}
static VcKgretArgs kgret_args(vc_engine* e, uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first, const uint32_t* d_new_ids, uint64_t* d_rows,
                              uint32_t* d_counts) {
  return VcKgretArgs{kgraph_args(e, k, mode, batch, 0, e->n, k_first, d_rows, d_counts), n_old, d_new_ids};
}
// the degenerate cases, which write nothing: K == n_old, K == 0 (n_old == 0 is one of the two)
static bool kgret_nothing_to_do(uint64_t K, uint64_t n_old, vc_knn_graph_retain_stats* stats) {
  if (stats) {
    *stats = vc_knn_graph_retain_stats{};
    stats->n_rows_kept = K;
  }
  return K == n_old || K == 0;
}

extern "C" {

int vc_knn_graph_dev(vc_engine* e, uint32_t k, uint32_t mode, uint32_t batch, uint64_t first, uint64_t count, uint32_t k_first, uint64_t* d_rows,
                     uint32_t* d_counts, vc_knn_graph_stats* stats, void* stream) {
  uint64_t n_rows = 0;
  const int rc = check_kgraph_args(e, k, mode, first, count, k_first, d_rows, &n_rows);
  if (rc) return rc;
  if (stats) *stats = vc_knn_graph_stats{};
  if (n_rows == 0) return VC_OK;
  return store_call(e, caller_stream(e, stream), [&](hipStream_t s, std::string* err) {
    return vc_knn_graph_run(store_view(e, mode), store_view(e, VC_MODE_LINEAR).knn, kgraph_args(e, k, mode, batch, first, n_rows, k_first, d_rows, d_counts), stats,
                            s, err);
  });
}

int vc_knn_graph(vc_engine* e, uint32_t k, uint32_t mode, uint32_t batch, uint64_t first, uint64_t count, uint32_t k_first, uint64_t* rows, uint32_t* counts,
                 vc_knn_graph_stats* stats) {
  uint64_t n_rows = 0;
  int rc = check_kgraph_args(e, k, mode, first, count, k_first, rows, &n_rows);
  if (rc) return rc;
  if (stats) *stats = vc_knn_graph_stats{};
  if (n_rows == 0) return VC_OK;
  if ((rc = bind_device(e))) return rc;
  const VcStoreView v = store_view(e, mode);
  hipStream_t s = e->stream;
  std::string err;
  rc = vc_knn_graph_run_host(v, kgraph_args(e, k, mode, batch, first, n_rows, k_first, nullptr, nullptr), rows, counts, stats,
                             [&](uint64_t* d_rows, uint32_t* d_counts, vc_knn_graph_stats* st) {
                               return store_call(e, s, [&](hipStream_t cs, std::string* cerr) {
                                 return vc_knn_graph_run(v, store_view(e, VC_MODE_LINEAR).knn, kgraph_args(e, k, mode, batch, first, n_rows, k_first, d_rows, d_counts),
                                                         st, cs, cerr);
                               });
                             },
                             [&](const uint64_t* codes, uint32_t nq, uint64_t* hrows, uint32_t* rcnt) {
                               return vc_search_knn(e, codes, nq, k + 1, VC_MODE_LINEAR, VC_ORDER_ASCENDING, hrows, rcnt, nullptr);
                             },
                             s, &err);
  return driver_done(e, rc, err);
}

int vc_knn_graph_update_dev(vc_engine* e, uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first, uint64_t* d_rows, uint32_t* d_counts,
                            vc_knn_graph_update_stats* stats, void* stream) {
  const int rc = check_kgupd_args(e, k, mode, n_old, k_first, d_rows);
  if (rc) return rc;
  if (stats) *stats = vc_knn_graph_update_stats{};
  if (n_old == e->n) return VC_OK;
  return store_call(e, caller_stream(e, stream), [&](hipStream_t s, std::string* err) {
    return vc_knn_graph_update_run(store_view(e, mode), store_view(e, VC_MODE_LINEAR).knn, kgupd_args(e, k, mode, batch, n_old, k_first, d_rows, d_counts), stats, s,
                                   err);
  });
}

int vc_knn_graph_update(vc_engine* e, uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first, uint64_t* rows, uint32_t* counts,
                        vc_knn_graph_update_stats* stats) {
  int rc = check_kgupd_args(e, k, mode, n_old, k_first, rows);
  if (rc) return rc;
  if (stats) *stats = vc_knn_graph_update_stats{};
  if (n_old == e->n) return VC_OK;
  if ((rc = bind_device(e))) return rc;
  const VcStoreView v = store_view(e, mode);
  hipStream_t s = e->stream;
  std::string err;
  rc = vc_knn_graph_update_run_host(v, kgupd_args(e, k, mode, batch, n_old, k_first, nullptr, nullptr), rows, counts, stats,
                                    [&](uint64_t* d_rows, uint32_t* d_counts, vc_knn_graph_update_stats* st) {
                                      return store_call(e, s, [&](hipStream_t cs, std::string* cerr) {
                                        return vc_knn_graph_update_run(v, store_view(e, VC_MODE_LINEAR).knn,
                                                                       kgupd_args(e, k, mode, batch, n_old, k_first, d_rows, d_counts), st, cs, cerr);
                                      });
                                    },
                                    [&](const uint64_t* codes, uint32_t nq, uint64_t* hrows, uint32_t* rcnt) {
                                      return vc_search_knn(e, codes, nq, k + 1, VC_MODE_LINEAR, VC_ORDER_ASCENDING, hrows, rcnt, nullptr);
                                    },
                                    s, &err);
  return driver_done(e, rc, err);
}

int vc_knn_graph_retain_dev(vc_engine* e, uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first, const uint32_t* d_new_ids, uint64_t* d_rows,
                            uint32_t* d_counts, vc_knn_graph_retain_stats* stats, void* stream) {
  const int rc = check_kgret_args(e, k, mode, n_old, k_first, d_new_ids, d_rows);
  if (rc) return rc;
  if (kgret_nothing_to_do(e->n, n_old, stats)) return VC_OK;
  return store_call(e, caller_stream(e, stream), [&](hipStream_t s, std::string* err) {
    return vc_knn_graph_retain_run(store_view(e, mode), store_view(e, VC_MODE_LINEAR).knn, kgret_args(e, k, mode, batch, n_old, k_first, d_new_ids, d_rows, d_counts),
                                   stats, s, err);
  });
}

int vc_knn_graph_retain(vc_engine* e, uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first, const uint32_t* new_ids, uint64_t* rows,
                        uint32_t* counts, vc_knn_graph_retain_stats* stats) {
  int rc = check_kgret_args(e, k, mode, n_old, k_first, new_ids, rows);
  if (rc) return rc;
  if (kgret_nothing_to_do(e->n, n_old, stats)) return VC_OK;
  if ((rc = bind_device(e))) return rc;
  const VcStoreView v = store_view(e, mode);
  hipStream_t s = e->stream;
  std::string err;
  rc = vc_knn_graph_retain_run_host(v, kgret_args(e, k, mode, batch, n_old, k_first, nullptr, nullptr, nullptr), new_ids, rows, counts, stats,
                                    [&](const uint32_t* d_new_ids, uint64_t* d_rows, uint32_t* d_counts, vc_knn_graph_retain_stats* st) {
                                      return store_call(e, s, [&](hipStream_t cs, std::string* cerr) {
                                        return vc_knn_graph_retain_run(v, store_view(e, VC_MODE_LINEAR).knn,
                                                                       kgret_args(e, k, mode, batch, n_old, k_first, d_new_ids, d_rows, d_counts), st, cs, cerr);
                                      });
                                    },
                                    [&](const uint64_t* codes, uint32_t nq, uint64_t* hrows, uint32_t* rcnt) {
                                      return vc_search_knn(e, codes, nq, k + 1, VC_MODE_LINEAR, VC_ORDER_ASCENDING, hrows, rcnt, nullptr);
                                    },
                                    s, &err);
  return driver_done(e, rc, err);
}

int vc_cluster_knn_dev(vc_engine* e, const uint64_t* d_rows, const uint32_t* d_counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist,
                       uint32_t* d_labels, uint32_t* d_in_degree, vc_cluster_knn_stats* stats, void* stream) {
  const int rc = check_cluster_knn_args(e, d_rows, k, kk, flags, d_labels);
  if (rc) return rc;
  if (stats) *stats = vc_cluster_knn_stats{};
  if (e->n == 0) return VC_OK;
  return store_call(e, caller_stream(e, stream), [&](hipStream_t s, std::string* err) {
    return vc_cluster_knn_run(store_view(e, VC_MODE_LINEAR), VcKgraphClusterArgs{d_rows, d_counts, k, kk, flags, max_dist, d_labels, d_in_degree}, stats, s, err);
  });
}

int vc_cluster_knn(vc_engine* e, const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist, uint32_t* labels,
                   uint32_t* in_degree, vc_cluster_knn_stats* stats) {
  const int rc = check_cluster_knn_args(e, rows, k, kk, flags, labels);
  if (rc) return rc;
  if (stats) *stats = vc_cluster_knn_stats{};
  if (e->n == 0) return VC_OK;
  return store_call(e, e->stream, [&](hipStream_t s, std::string* err) {
    return vc_cluster_knn_run_host(store_view(e, VC_MODE_LINEAR), VcKgraphClusterArgs{nullptr, nullptr, k, kk, flags, max_dist, nullptr, nullptr}, rows, counts,
                                   labels, in_degree, stats, s, err);
  });
}

int vc_cluster_snn_dev(vc_engine* e, const uint64_t* d_rows, const uint32_t* d_counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist,
                       uint32_t min_shared, uint32_t* d_labels, uint32_t* d_shared, uint64_t* d_hist, vc_cluster_snn_stats* stats, void* stream) {
  const int rc = check_cluster_snn_args(e, d_rows, k, kk, flags, d_labels);
  if (rc) return rc;
  if (stats) *stats = vc_cluster_snn_stats{};
  if (e->n == 0) return VC_OK;
  return store_call(e, caller_stream(e, stream), [&](hipStream_t s, std::string* err) {
    return vc_cluster_snn_run(store_view(e, VC_MODE_LINEAR), VcSnnArgs{d_rows, d_counts, k, kk, flags, max_dist, min_shared, d_labels, d_shared, d_hist}, stats, s,
                              err);
  });
}

int vc_cluster_snn(vc_engine* e, const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist, uint32_t min_shared,
                   uint32_t* labels, uint32_t* shared, uint64_t* hist, vc_cluster_snn_stats* stats) {
  const int rc = check_cluster_snn_args(e, rows, k, kk, flags, labels);
  if (rc) return rc;
  if (stats) *stats = vc_cluster_snn_stats{};
  if (e->n == 0) return VC_OK;
  return store_call(e, e->stream, [&](hipStream_t s, std::string* err) {
    return vc_cluster_snn_run_host(store_view(e, VC_MODE_LINEAR), VcSnnArgs{nullptr, nullptr, k, kk, flags, max_dist, min_shared, nullptr, nullptr, nullptr}, rows,
                                   counts, labels, shared, hist, stats, s, err);
  });
}

int vc_knn_adjacency_dev(vc_engine* e, const uint64_t* d_rows, const uint32_t* d_counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist,
                         uint64_t* d_adj, uint64_t adj_cap, uint64_t* d_offsets, vc_knn_adjacency_stats* stats, void* stream) {
  const int rc = check_knn_adjacency_args(e, d_rows, k, kk, flags, d_adj, adj_cap, d_offsets);
  if (rc) return rc;
  return store_call(e, caller_stream(e, stream), [&](hipStream_t s, std::string* err) {
    return vc_knn_adjacency_run(store_view(e, VC_MODE_LINEAR), VcAdjArgs{d_rows, d_counts, k, kk, flags, max_dist, d_adj, adj_cap, d_offsets}, stats, s, err);
  });
}

int vc_knn_adjacency(vc_engine* e, const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist, uint64_t* adj,
                     uint64_t adj_cap, uint64_t* offsets, vc_knn_adjacency_stats* stats) {
  const int rc = check_knn_adjacency_args(e, rows, k, kk, flags, adj, adj_cap, offsets);
  if (rc) return rc;
  return store_call(e, e->stream, [&](hipStream_t s, std::string* err) {
    return vc_knn_adjacency_run_host(store_view(e, VC_MODE_LINEAR), VcAdjArgs{nullptr, nullptr, k, kk, flags, max_dist, nullptr, adj_cap, nullptr}, rows, counts,
                                     adj, offsets, stats, s, err);
  });
}

int vc_knn_mst_dev(vc_engine* e, const uint64_t* d_rows, const uint32_t* d_counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist,
                   uint32_t weight_kind, uint32_t min_pts, vc_mst_edge* d_edges, uint32_t* d_labels, uint64_t* d_hist, vc_knn_mst_stats* stats, void* stream) {
  const int rc = check_knn_mst_args(e, d_rows, k, kk, flags, weight_kind, min_pts, d_edges);
  if (rc) return rc;
  return store_call(e, caller_stream(e, stream), [&](hipStream_t s, std::string* err) {
    return vc_knn_mst_run(store_view(e, VC_MODE_LINEAR), VcMstArgs{d_rows, d_counts, k, kk, flags, max_dist, weight_kind, min_pts, d_edges, d_labels, d_hist}, stats,
                          s, err);
  });
}

int vc_knn_mst(vc_engine* e, const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist, uint32_t weight_kind,
               uint32_t min_pts, vc_mst_edge* edges, uint32_t* labels, uint64_t* hist, vc_knn_mst_stats* stats) {
  const int rc = check_knn_mst_args(e, rows, k, kk, flags, weight_kind, min_pts, edges);
  if (rc) return rc;
  return store_call(e, e->stream, [&](hipStream_t s, std::string* err) {
    return vc_knn_mst_run_host(store_view(e, VC_MODE_LINEAR), VcMstArgs{nullptr, nullptr, k, kk, flags, max_dist, weight_kind, min_pts, nullptr, nullptr, nullptr},
                               rows, counts, edges, labels, hist, stats, s, err);
  });
}

int vc_mst_cut_dev(vc_engine* e, const vc_mst_edge* d_edges, uint64_t n_edges, uint32_t max_weight, uint32_t* d_labels, uint64_t* n_clusters, void* stream) {
  const int rc = check_mst_cut_args(e, d_edges, n_edges, d_labels);
  if (rc) return rc;
  return store_call(e, caller_stream(e, stream), [&](hipStream_t s, std::string* err) {
    return vc_mst_cut_run(store_view(e, VC_MODE_LINEAR), d_edges, n_edges, max_weight, d_labels, n_clusters, s, err);
  });
}

int vc_mst_cut(vc_engine* e, const vc_mst_edge* edges, uint64_t n_edges, uint32_t max_weight, uint32_t* labels, uint64_t* n_clusters) {
  const int rc = check_mst_cut_args(e, edges, n_edges, labels);
  if (rc) return rc;
  return store_call(e, e->stream, [&](hipStream_t s, std::string* err) {
    return vc_mst_cut_run_host(store_view(e, VC_MODE_LINEAR), edges, n_edges, max_weight, labels, n_clusters, s, err);
  });
}

int vc_mst_condense_dev(vc_engine* e, const vc_mst_edge* d_edges, uint64_t n_edges, uint32_t min_cluster_size, uint32_t root_weight, uint32_t method,
                        vc_condensed_node* d_nodes, uint32_t* d_labels, uint32_t* d_node, uint32_t* d_own, uint32_t* d_leave, vc_mst_condense_stats* stats,
                        void* stream) {
  const int rc = check_mst_condense_args(e, d_edges, n_edges, min_cluster_size, root_weight, method, d_nodes, d_labels);
  if (rc) return rc;
  return store_call(e, caller_stream(e, stream), [&](hipStream_t s, std::string* err) {
    return vc_mst_condense_run(store_view(e, VC_MODE_LINEAR),
                               VcCondenseArgs{d_edges, n_edges, min_cluster_size, root_weight, method, d_nodes, d_labels, d_node, d_own, d_leave}, stats, s, err);
  });
}

int vc_mst_condense(vc_engine* e, const vc_mst_edge* edges, uint64_t n_edges, uint32_t min_cluster_size, uint32_t root_weight, uint32_t method,
                    vc_condensed_node* nodes, uint32_t* labels, uint32_t* node, uint32_t* own, uint32_t* leave, vc_mst_condense_stats* stats) {
  const int rc = check_mst_condense_args(e, edges, n_edges, min_cluster_size, root_weight, method, nodes, labels);
  if (rc) return rc;
  return store_call(e, e->stream, [&](hipStream_t s, std::string* err) {
    return vc_mst_condense_run_host(store_view(e, VC_MODE_LINEAR),
                                    VcCondenseArgs{nullptr, n_edges, min_cluster_size, root_weight, method, nullptr, nullptr, nullptr, nullptr, nullptr}, edges,
                                    nodes, labels, node, own, leave, stats, s, err);
  });
}

int vc_knn_vote_dev(vc_engine* e, const uint64_t* d_rows, const uint32_t* d_counts, uint64_t n_rows, uint32_t k, uint32_t kk, uint32_t max_dist,
                    const uint32_t* d_labels, uint32_t weight_kind, uint32_t* d_out_label, uint32_t* d_out_votes, uint32_t* d_out_total, vc_knn_vote_stats* stats,
                    void* stream) {
  const int rc = check_knn_vote_args(e, d_rows, k, kk, d_labels, weight_kind, d_out_label);
  if (rc) return rc;
  return store_call(e, caller_stream(e, stream), [&](hipStream_t s, std::string* err) {
    return vc_knn_vote_run(store_view(e, VC_MODE_LINEAR), VcVoteArgs{d_rows, d_counts, n_rows, k, kk, max_dist, d_labels, weight_kind, d_out_label, d_out_votes, d_out_total},
                           stats, s, err);
  });
}

int vc_knn_vote(vc_engine* e, const uint64_t* rows, const uint32_t* counts, uint64_t n_rows, uint32_t k, uint32_t kk, uint32_t max_dist, const uint32_t* labels,
                uint32_t weight_kind, uint32_t* out_label, uint32_t* out_votes, uint32_t* out_total, vc_knn_vote_stats* stats) {
  const int rc = check_knn_vote_args(e, rows, k, kk, labels, weight_kind, out_label);
  if (rc) return rc;
  return store_call(e, e->stream, [&](hipStream_t s, std::string* err) {
    return vc_knn_vote_run_host(store_view(e, VC_MODE_LINEAR), VcVoteArgs{nullptr, nullptr, n_rows, k, kk, max_dist, nullptr, weight_kind, nullptr, nullptr, nullptr}, rows,
                                counts, labels, out_label, out_votes, out_total, stats, s, err);
  });
}

int vc_label_propagate_dev(vc_engine* e, const uint64_t* d_offsets, const uint64_t* d_adj, uint64_t n_entries, const uint32_t* d_labels_in, uint32_t weight_kind,
                           uint32_t flags, uint32_t max_iters, uint32_t* d_labels_out, uint32_t* d_votes, uint32_t* d_total, vc_label_propagate_stats* stats,
                           void* stream) {
  const int rc = check_label_propagate_args(e, d_offsets, d_adj, n_entries, d_labels_in, weight_kind, flags, max_iters, d_labels_out);
  if (rc) return rc;
  return store_call(e, caller_stream(e, stream), [&](hipStream_t s, std::string* err) {
    return vc_label_propagate_run(store_view(e, VC_MODE_LINEAR),
                                  VcLabelPropagateArgs{d_offsets, d_adj, n_entries, d_labels_in, weight_kind, flags, max_iters, d_labels_out, d_votes, d_total}, stats, s, err);
  });
}

int vc_label_propagate(vc_engine* e, const uint64_t* offsets, const uint64_t* adj, uint64_t n_entries, const uint32_t* labels_in, uint32_t weight_kind, uint32_t flags,
                       uint32_t max_iters, uint32_t* labels_out, uint32_t* votes, uint32_t* total, vc_label_propagate_stats* stats) {
  const int rc = check_label_propagate_args(e, offsets, adj, n_entries, labels_in, weight_kind, flags, max_iters, labels_out);
  if (rc) return rc;
  return store_call(e, e->stream, [&](hipStream_t s, std::string* err) {
    return vc_label_propagate_run_host(store_view(e, VC_MODE_LINEAR),
                                       VcLabelPropagateArgs{nullptr, nullptr, n_entries, nullptr, weight_kind, flags, max_iters, nullptr, nullptr, nullptr}, offsets, adj,
                                       labels_in, labels_out, votes, total, stats, s, err);
  });
}

}  // extern "C"

extern "C" {

// is `p` page-locked host memory (hipHostMalloc / hipHostRegister / torch pin_memory)?  Then a copy is one DMA, no staging.
static bool host_pinned(const void* p) {
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();   // ordinary malloc'ed memory is "invalid value" to the runtime
    return false;
  }
  return a.type == hipMemoryTypeHost;
}

#define VC_PIPE_CHUNK ((size_t)1 << 20)
// Large results to PAGEABLE host memory: the runtime's own staged copy is serial (DMA a chunk, memcpy it, next chunk); here the
// DMA of chunk i+1 runs while the host copies chunk i out of the other pinned buffer.  Synchronises the stream.
static int d2h_pipelined(vc_engine* e, void* dst, const void* d_src, size_t bytes) {
  if (!e->h_pipe) {
    if (hipHostMalloc((void**)&e->h_pipe, 2 * VC_PIPE_CHUNK, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); e->h_pipe = nullptr; }
    for (hipEvent_t& ev : e->pipe_ev)
      if (e->h_pipe && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); ev = nullptr; }
  }
  if (!e->h_pipe || !e->pipe_ev[0] || !e->pipe_ev[1]) {   // no pinned memory to be had: the runtime's staged copy
    VC_HIP(e, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, e->stream));
    VC_HIP(e, hipStreamSynchronize(e->stream));
    return VC_OK;
  }
  const size_t n_chunks = (bytes + VC_PIPE_CHUNK - 1) / VC_PIPE_CHUNK;
  for (size_t c = 0; c <= n_chunks; ++c) {
    if (c < n_chunks) {
      const size_t off = c * VC_PIPE_CHUNK, len = std::min(VC_PIPE_CHUNK, bytes - off);
      VC_HIP(e, hipMemcpyAsync(e->h_pipe + (c & 1) * VC_PIPE_CHUNK, (const uint8_t*)d_src + off, len, hipMemcpyDeviceToHost, e->stream));
      VC_HIP(e, hipEventRecord(e->pipe_ev[c & 1], e->stream));
    }
    if (c > 0) {
      const size_t off = (c - 1) * VC_PIPE_CHUNK, len = std::min(VC_PIPE_CHUNK, bytes - off);
      VC_HIP(e, hipEventSynchronize(e->pipe_ev[(c - 1) & 1]));
      memcpy((uint8_t*)dst + off, e->h_pipe + ((c - 1) & 1) * VC_PIPE_CHUNK, len);
    }
  }
  return VC_OK;
}

int vc_search_knn(vc_engine* e, const void* queries, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order,
                  uint64_t* out, uint32_t* counts, vc_query_stats* stats) {
  int rc = check_knn_args(e, queries, nq, k, mode);
  if (rc) return rc;
  if (!out || order > VC_ORDER_FARTHEST_FIRST) return VC_ERR_INVALID;
  if ((rc = bind_device(e))) return rc;
  const size_t qbytes = (size_t)nq * (e->bits / 8);
  if ((rc = grow(e, &e->d_q, &e->q_bytes, qbytes))) return rc;
  if ((rc = grow(e, &e->d_out, &e->out_bytes, (size_t)nq * k * 8))) return rc;
  if ((rc = grow(e, &e->d_cnt, &e->cnt_bytes, (size_t)nq * 8))) return rc;
  // Pageable host memory makes every async copy a staged, partly synchronous one (~20 us each at this size: a third of what the
  // host-pointer call costs over the device-pointer call).  Batches of up to 512 KB go through a pinned staging buffer of the
  // engine: one memcpy in, one out, true async copies in between.
  // Larger batches (an MIH call of 16 384 queries returns 13 MB of rows): straight DMA when the caller's buffers are page-locked,
  // else the rows travel through two pinned chunks, DMA and host copy overlapped (d2h_pipelined).
  const size_t rows_bytes = (size_t)nq * k * 8, pin_need = ((qbytes + 63) & ~(size_t)63) + rows_bytes + (size_t)nq * 4;
  uint8_t *pin_q = nullptr, *pin_rows = nullptr, *pin_cnt = nullptr;
  const bool small = pin_need <= ((size_t)512 << 10);     // (one staging buffer, one host copy: 8 queries x top-100 and the like)
  const bool out_direct = !small && host_pinned(out);
  if (small) {
    if (pin_need > e->pin_bytes) {
      if (e->h_pin) (void)hipHostFree(e->h_pin);
      e->h_pin = nullptr;
      e->pin_bytes = 0;
      const size_t want = std::max<size_t>(pin_need, 64 << 10);
      if (hipHostMalloc((void**)&e->h_pin, want, hipHostMallocDefault) == hipSuccess) e->pin_bytes = want;
      else { (void)hipGetLastError(); e->h_pin = nullptr; }
    }
    if (e->h_pin) {
      pin_q = e->h_pin;
      pin_rows = e->h_pin + ((qbytes + 63) & ~(size_t)63);
      pin_cnt = pin_rows + rows_bytes;
      memcpy(pin_q, queries, qbytes);
    }
  }
  VC_HIP(e, hipMemcpyAsync(e->d_q, pin_q ? (const void*)pin_q : queries, qbytes, hipMemcpyHostToDevice, e->stream));
  std::vector<uint32_t> cnt(2 * (size_t)nq, 0);
  std::vector<vc_query_stats> st;
  timing_begin(e);
  if (mode == VC_MODE_LINEAR) {
    LinearSearch ls(e, nq, k);
    ls.stream_ok = true;
    rc = ls.run(e->d_q, nq, e->d_out, e->d_cnt);
  } else {
    if (stats) st.resize(nq);      // (the statistics cost four read-backs and a wait per launch: only when asked for)
    const VcMihScanFallback fb{mih_scan_fallback, e, e->n_cu};
    rc = vc_mih_search(live_index(e), e->d_cols, e->stride, e->n, e->d_q, nq, k, mode == VC_MODE_MIH_APPROX, e->d_out,
                       e->d_cnt, stats ? st.data() : nullptr, e->stream, &e->err, &fb);
  }
  timing_end(e);
  if (rc) return rc;
  VC_HIP(e, hipMemcpyAsync(pin_cnt ? (void*)pin_cnt : (void*)cnt.data(), e->d_cnt, (size_t)nq * 4, hipMemcpyDeviceToHost, e->stream));
  if (small || out_direct) {
    VC_HIP(e, hipMemcpyAsync(pin_rows ? (void*)pin_rows : (void*)out, e->d_out, rows_bytes, hipMemcpyDeviceToHost, e->stream));
    VC_HIP(e, hipStreamSynchronize(e->stream));
  } else if ((rc = d2h_pipelined(e, out, e->d_out, rows_bytes))) {
    return rc;
  }
  if (pin_rows) {
    memcpy(out, pin_rows, rows_bytes);
    memcpy(cnt.data(), pin_cnt, (size_t)nq * 4);
  }
  if (mode == VC_MODE_LINEAR) {
    // a row still flagged here overflowed its ring and was not recomputed on the device (VC_DEVICE_RECOVER=0, or the
    // recovery grid gave up): host-driven fallback
    std::vector<uint32_t> over;
    for (uint32_t i = 0; i < nq; ++i)
      if (cnt[i] == 0xFFFFFFFFu) over.push_back(i);
    if (!over.empty()) {
      // the device recovery gave up (or is switched off): its last block restores the barrier words itself, but should
      // that block never have run (the grid was cut short) they would stay dirty for the life of the engine -- the
      // stream is idle here, so the three lines are simply rewritten
      if (e->d_rec) VC_HIP(e, hipMemsetAsync(e->d_rec + VcRecoverScratch::bar, 0, VcRecoverScratch::bar_words * 4, e->stream));
      if ((rc = linear_recover(e, e->d_q, k, over, out, cnt.data()))) return rc;
    }
  }
  for (uint32_t i = 0; i < nq; ++i) {
    if (order == VC_ORDER_FARTHEST_FIRST) std::reverse(out + (size_t)i * k, out + (size_t)i * k + cnt[i]);
    if (counts) counts[i] = cnt[i];
    if (stats) {
      if (mode == VC_MODE_LINEAR) {
        memset(&stats[i], 0, sizeof stats[i]);
        stats[i].n_candidates = e->n;
      } else {
        stats[i] = st[i];
      }
      stats[i].n_results = cnt[i];
    }
  }
  return VC_OK;
}

int vc_device_status(vc_engine* e, uint32_t* n_gave_up) {
  if (!e || !n_gave_up) return VC_ERR_INVALID;
  *n_gave_up = 0;
  if (!e->d_rec) return VC_OK;
  int rc = bind_device(e);
  if (rc) return rc;
  uint32_t* d_flag = e->d_rec + VcRecoverScratch::gave_up;
  VC_HIP(e, hipMemcpyAsync(n_gave_up, d_flag, 4, hipMemcpyDeviceToHost, e->stream));
  VC_HIP(e, hipMemsetAsync(d_flag, 0, 4, e->stream));
  VC_HIP(e, hipStreamSynchronize(e->stream));
  return VC_OK;
}

int vc_merge_topk_dev(const uint64_t* d_lists, uint32_t n_lists, uint32_t nq, uint32_t k, uint64_t* d_out,
                      uint32_t* d_counts, void* stream) {
  if (!d_lists || !d_out || n_lists == 0 || nq == 0 || k == 0 || k > VC_MAX_K) return VC_ERR_INVALID;
  hipError_t r = vc_launch_select_lists(d_lists, n_lists, nq, k, d_out, d_counts, (hipStream_t)stream);
  if (r != hipSuccess) return fail(nullptr, VC_ERR_HIP, "merge launch: %s", hipGetErrorString(r));
  return VC_OK;
}

// ---- MIH index / bucket views -----------------------------------------------------------------------
int vc_build_index(vc_engine* e) {
  if (!e) return VC_ERR_INVALID;
  if (e->m == 0) return fail(e, VC_ERR_STATE, "engine was created with n_tables = 0 (linear only)");
  int rc = bind_device(e);
  if (rc) return rc;
  drop_index(e);
  rc = vc_mih_build(&e->mih, e->d_cols, e->stride, e->n, e->W, e->m, e->sbits, e->cfg.id_base, e->cfg.flags, e->n_cu,
                    e->cap, e->knobs, e->stream, &e->err);
  if (rc == VC_OK) e->n_indexed = e->n;
  return rc;
}

// build_hash_tables.cc:40-70 (get bucket, append, put): the records added since the index was built, loaded or last updated are
// appended to their buckets -- the stale index is merged with them (vc_mih_update), not rebuilt
int vc_update_index(vc_engine* e) {
  if (!e) return VC_ERR_INVALID;
  if (e->m == 0) return fail(e, VC_ERR_STATE, "engine was created with n_tables = 0 (linear only)");
  if (!e->mih) return vc_build_index(e);
  int rc = bind_device(e);
  if (rc) return rc;
  if (e->knobs.mih_update == 0 && e->n_indexed != e->n) {   // A/B and test route: the full rebuild
    const uint64_t added = e->n - e->n_indexed;
    if ((rc = vc_build_index(e)) == VC_OK) vc_mih_update_trace(e->mih, added, "rebuild", "0");
    return rc;
  }
  rc = vc_mih_update(&e->mih, e->d_cols, e->stride, e->n, e->stream, &e->err);
  e->n_indexed = e->mih ? vc_mih_records(e->mih) : 0;   // (a failed update leaves the old stale index, or none)
  return rc;
}

// ---- the prefix-sorted scan stream (vc_scan_stream.hip) ---------------------------------------------------------------
int vc_build_scan_stream(vc_engine* e) {
  if (!e) return VC_ERR_INVALID;
  if (e->bits != 128) return fail(e, VC_ERR_INVALID, "the scan stream is built for 128-bit codes only (bits = %u)", e->bits);
  int rc = bind_device(e);
  if (rc) return rc;
  VC_HIP(e, hipStreamSynchronize(e->stream));   // no search still reads the stream that is about to go
  // the memory rule sees the memory as it is with the old stream still held: a refused build leaves the engine as it was
  size_t free_b = 0, total_b = 0;
  bool have_free = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
  if (!have_free) (void)hipGetLastError();
  uint64_t free_bytes = (uint64_t)free_b + (e->sstream.built() ? e->sstream.plan.bytes : 0);
  if (e->knobs.stream_free_set) { have_free = true; free_bytes = e->knobs.stream_free; }   // test knob VC_SCAN_STREAM_FREE
  if (!vc_stream_fits(vc_stream_plan(e->n, vc_radix_sort_work_words(e->n)), have_free, free_bytes))
    return fail(e, VC_ERR_NOMEM, "scan stream of %llu records does not fit %u %% of %llu free bytes", (unsigned long long)e->n,
                VC_STREAM_MEM_SHARE, (unsigned long long)free_bytes);
  drop_scan_stream(e);
  const hipError_t r = vc_scan_stream_build(e->d_cols, e->stride, e->n, have_free, free_bytes, &e->sstream, e->stream);
  if (r == hipErrorOutOfMemory) (void)hipGetLastError();
  if (r != hipSuccess)
    return fail(e, r == hipErrorOutOfMemory ? VC_ERR_NOMEM : VC_ERR_HIP, "scan stream build: %s", hipGetErrorString(r));
  return VC_OK;
}

int vc_scan_stream_info(vc_engine* e, vc_scan_stream_state* info) {
  if (!e || !info) return VC_ERR_INVALID;
  memset(info, 0, sizeof *info);
  if (!e->sstream.built()) return VC_OK;
  info->built = 1;
  info->items = e->sstream.plan.n;
  info->granules = e->sstream.plan.granules;
  info->bytes = e->sstream.plan.bytes;
  info->launches = e->sstream.launches;
#if VC_SCAN_STREAM_DIAG
  int rc = bind_device(e);
  if (rc) return rc;
  uint32_t c[2] = {0, 0};
  VC_HIP(e, hipStreamSynchronize(e->stream));
  VC_HIP(e, hipMemcpy(c, e->sstream.d_diag, 8, hipMemcpyDeviceToHost));
  info->bound_passes = c[0];
  info->exact_passes = c[1];
#endif
  return VC_OK;
}

}  // extern "C"

// ---- removal: the store and its index cut down to the surviving records ---------------------------------------------------------
// The reference has no delete (base_proxy.h:18-22: put and get); this stands for running build_hash_tables.cc:40-70 again over the
// code file without the removed records -- ids stay the ordinals of the records in file order.
static bool ranges_overlap(const void* a, const void* b, uint64_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}
static int check_retain_args(vc_engine* e, const uint32_t* sel, uint32_t kind, const uint32_t* new_ids) {
  if (!e) return VC_ERR_INVALID;
  if (kind > VC_RETAIN_FROM || (kind == VC_RETAIN_FROM && sel)) return fail(e, VC_ERR_INVALID, "retain: unknown kind %u", kind);
  if (e->n && !sel && kind != VC_RETAIN_FROM) return fail(e, VC_ERR_INVALID, "retain: null selection");
  if (e->n && new_ids && sel && ranges_overlap(sel, new_ids, e->n * 4)) return fail(e, VC_ERR_INVALID, "retain: new_ids overlaps the selection");
  return VC_OK;
}

// The whole call on e->stream, e->n > 0.  Keep set -> K (the one wait of the column phase) -> map -> columns -> index.  Everything
// the column phase needs is allocated before the first column byte changes; the scratch is call-scoped.
static int retain_run(vc_engine* e, const uint32_t* d_sel, uint32_t kind, uint64_t first_kept, uint32_t* d_new_ids, uint64_t* n_kept) {
  const uint64_t N = e->n, nblocks = vc_keep_blocks(N);
  hipStream_t s = e->stream;
  ScopedDev<uint64_t> bits, scratch;
  ScopedDev<uint32_t> rank, work;
  VC_HIP(e, bits.alloc(nblocks * VC_KEEP_BLOCK_WORDS * 8));
  VC_HIP(e, rank.alloc((nblocks + 1) * 4));
  VC_HIP(e, work.alloc(std::max<size_t>(vc_scan_work_words(nblocks + 1), 1) * 4));
  VC_HIP(e, scratch.alloc(((N + 1) & ~1ull) * 8));
  VC_HIP(e, vc_launch_keep_bits(d_sel, kind, e->cfg.id_base, first_kept, N, bits.p, rank.p, work.p, e->n_cu, s));
  uint32_t k32 = 0;
  VC_HIP(e, hipMemcpyAsync(&k32, rank.p + nblocks, 4, hipMemcpyDeviceToHost, s));
  VC_HIP(e, hipStreamSynchronize(s));
  const uint64_t K = k32;
  const VcKeepSet ks{bits.p, rank.p, N, K};
  if (d_new_ids) VC_HIP(e, vc_launch_keep_map(ks, e->cfg.id_base, d_new_ids, e->n_cu, s));
  if (n_kept) *n_kept = K;
  if (K == N) {   // nothing removed: no column or index byte is written
    if (live_index(e)) vc_mih_retain_trace(e->mih, 0, "none", "0");
    VC_HIP(e, hipStreamSynchronize(s));   // (the keep set is freed on the way out)
    return VC_OK;
  }
  const bool had_live = live_index(e) != nullptr;
  drop_scan_stream(e);
  if (K == 0) {
    for (uint32_t j = 0; j < e->W; ++j) VC_HIP(e, hipMemsetAsync(e->d_cols + j * e->stride, 0, N * 8, s));
  } else {
    for (uint32_t j = 0; j < e->W; ++j) VC_HIP(e, vc_launch_keep_compact_column(ks, e->d_cols + j * e->stride, scratch.p, e->n_cu, s));
  }
  hipError_t r = hipStreamSynchronize(s);
  e->n = K;
  if (r != hipSuccess || !had_live || K == 0) drop_index(e);   // a stale index, or that of a store of nothing, serves no one
  if (r != hipSuccess) return fail(e, VC_ERR_HIP, "retain: %s", hipGetErrorString(r));
  if (!e->mih) return VC_OK;
  // index phase: a failure leaves the compacted records with no index, never a half-filtered one
  int rc;
  if (e->knobs.mih_retain == 0) {   // A/B and test route: the full rebuild
    if ((rc = vc_build_index(e)) == VC_OK) vc_mih_retain_trace(e->mih, N - K, "rebuild", "0");
    return rc;
  }
  rc = vc_mih_retain(&e->mih, ks, e->d_cols, e->stride, s, &e->err);
  e->n_indexed = e->mih ? K : 0;
  return rc;
}

// what the sharded store needs of a shard: the records from local position `first_kept` on survive (a prefix is given away)
int vc_engine_retain_from(vc_engine* e, uint64_t first_kept, hipStream_t s) {
  if (!e || first_kept > e->n) return VC_ERR_INVALID;
  if (e->n == 0 || first_kept == 0) return VC_OK;
  int rc = bind_device(e);
  if (rc) return rc;
  const StreamCall call(e, s);
  return retain_run(e, nullptr, VC_RETAIN_FROM, first_kept, nullptr, nullptr);
}

// ... and `count` records of `src` from its local position `first` on appended to e's columns (device / peer copies, column by column)
int vc_engine_append_from(vc_engine* e, vc_engine* src, uint64_t first, uint64_t count, hipStream_t s) {
  if (!e || !src || e->W != src->W || first + count > src->n) return VC_ERR_INVALID;
  if (e->n + count > e->cfg.capacity) return fail(e, VC_ERR_CAPACITY, "append beyond capacity");
  if (count == 0) return VC_OK;
  int rc = bind_device(e);
  if (rc) return rc;
  drop_scan_stream(e);
  for (uint32_t j = 0; j < e->W; ++j) {
    uint64_t* dst = e->d_cols + j * e->stride + e->n;
    const uint64_t* from = src->d_cols + j * src->stride + first;
    if (e->device == src->device) VC_HIP(e, hipMemcpyAsync(dst, from, count * 8, hipMemcpyDeviceToDevice, s));
    else VC_HIP(e, hipMemcpyPeerAsync(dst, e->device, from, src->device, count * 8, s));
  }
  VC_HIP(e, hipStreamSynchronize(s));
  e->n += count;   // (an index, if any, is stale from here on: live_index)
  return VC_OK;
}

extern "C" {

int vc_retain_dev(vc_engine* e, const uint32_t* d_sel, uint32_t kind, uint32_t* d_new_ids, uint64_t* n_kept, void* stream) {
  int rc = check_retain_args(e, d_sel, kind, d_new_ids);
  if (rc) return rc;
  if (kind > VC_RETAIN_ROOTS) return fail(e, VC_ERR_INVALID, "retain: unknown kind %u", kind);
  if (e->n == 0) {
    if (n_kept) *n_kept = 0;
    return VC_OK;
  }
  if ((rc = bind_device(e))) return rc;
  const StreamCall call(e, caller_stream(e, stream));
  return retain_run(e, d_sel, kind, 0, d_new_ids, n_kept);
}

int vc_retain(vc_engine* e, const uint32_t* sel, uint32_t kind, uint32_t* new_ids, uint64_t* n_kept) {
  int rc = check_retain_args(e, sel, kind, new_ids);
  if (rc) return rc;
  if (kind > VC_RETAIN_ROOTS) return fail(e, VC_ERR_INVALID, "retain: unknown kind %u", kind);
  if (e->n == 0) {
    if (n_kept) *n_kept = 0;
    return VC_OK;
  }
  if ((rc = bind_device(e))) return rc;
  const uint64_t N = e->n;
  ScopedDev<uint32_t> d_sel, d_map;   // staged selection and map: call-scoped, like the rest of the call's scratch
  VC_HIP(e, d_sel.alloc(N * 4));
  if (new_ids) VC_HIP(e, d_map.alloc(N * 4));
  VC_HIP(e, hipMemcpyAsync(d_sel.p, sel, N * 4, hipMemcpyHostToDevice, e->stream));
  uint64_t K = 0;
  {
    const StreamCall call(e, e->stream);
    rc = retain_run(e, d_sel.p, kind, 0, d_map.p, &K);
  }
  if (new_ids && e->n == K) {   // (the map is final once K is known, whatever became of the index)
    VC_HIP(e, hipMemcpyAsync(new_ids, d_map.p, N * 4, hipMemcpyDeviceToHost, e->stream));
    VC_HIP(e, hipStreamSynchronize(e->stream));
  }
  if (n_kept && (rc == VC_OK || e->n == K)) *n_kept = K;
  return rc;
}

}  // extern "C"

extern "C" {

int vc_get_bucket(vc_engine* e, uint32_t table, uint32_t index, uint32_t* ids, void* codes, uint32_t cap, uint32_t* n) {
  if (!e || !n) return VC_ERR_INVALID;
  if (!live_index(e)) return fail(e, VC_ERR_STATE, "no index built");
  if (table >= e->m) return fail(e, VC_ERR_INVALID, "table %u >= n_tables %u", table, e->m);
  int rc = bind_device(e);
  if (rc) return rc;
  std::vector<uint32_t> local;
  rc = vc_mih_bucket(live_index(e), table, index, &local, e->stream, &e->err);
  if (rc < 0) return rc;
  *n = (uint32_t)local.size();
  if (local.empty()) return VC_NOT_FOUND;
  const uint32_t take = std::min<uint32_t>(cap, (uint32_t)local.size());
  if (codes && take) {
    const size_t rec = e->bits / 8;
    if ((rc = grow(e, (uint8_t**)&e->d_stage, &e->stage_bytes, take * (rec + 4)))) return rc;
    uint32_t* d_ids = (uint32_t*)((uint8_t*)e->d_stage + (size_t)take * rec);
    VC_HIP(e, hipMemcpyAsync(d_ids, local.data(), take * 4, hipMemcpyHostToDevice, e->stream));
    VC_HIP(e, vc_launch_gather_rows(e->d_cols, e->stride, e->W, d_ids, take, (uint64_t*)e->d_stage, e->stream));
    VC_HIP(e, hipMemcpyAsync(codes, e->d_stage, take * rec, hipMemcpyDeviceToHost, e->stream));
    VC_HIP(e, hipStreamSynchronize(e->stream));
  }
  if (ids)
    for (uint32_t i = 0; i < take; ++i) ids[i] = e->cfg.id_base + local[i];
  return VC_OK;
}

int vc_bitmap_test(vc_engine* e, uint32_t table, uint32_t index, int* bit) {
  if (!e || !bit) return VC_ERR_INVALID;
  if (!live_index(e)) return fail(e, VC_ERR_STATE, "no index built");
  if (table >= e->m) return VC_ERR_INVALID;
  int rc = bind_device(e);
  if (rc) return rc;
  return vc_mih_bitmap_test(live_index(e), table, index, bit, e->stream, &e->err);
}

int vc_bitmap_read(vc_engine* e, uint32_t table, uint64_t word_off, uint64_t n_words, uint32_t* out) {
  if (!e || !out) return VC_ERR_INVALID;
  if (!live_index(e)) return fail(e, VC_ERR_STATE, "no index built");
  if (table >= e->m) return VC_ERR_INVALID;
  int rc = bind_device(e);
  if (rc) return rc;
  return vc_mih_bitmap_read(live_index(e), table, word_off, n_words, out, e->stream, &e->err);
}

int vc_search_radius(vc_engine* e, const void* queries, uint32_t nq, uint32_t radius, uint32_t mode, uint64_t* out,
                     uint64_t out_cap, uint64_t* out_offsets) {
  if (!e || !queries || !out_offsets || nq == 0) return VC_ERR_INVALID;
  if (mode != VC_MODE_LINEAR && mode != VC_MODE_MIH_EXACT) return fail(e, VC_ERR_INVALID, "radius search: mode must be LINEAR or MIH_EXACT");
  if (mode == VC_MODE_MIH_EXACT && !live_index(e)) return fail(e, VC_ERR_STATE, "MIH search needs vc_build_index() first");
  int rc = bind_device(e);
  if (rc) return rc;
  const size_t qbytes = (size_t)nq * (e->bits / 8);
  if ((rc = grow(e, &e->d_q, &e->q_bytes, qbytes))) return rc;
  VC_HIP(e, hipMemcpyAsync(e->d_q, queries, qbytes, hipMemcpyHostToDevice, e->stream));
  timing_begin(e);
  rc = vc_radius_search(live_index(e), mode == VC_MODE_MIH_EXACT, e->d_cols, e->stride, e->n, e->W, e->cfg.id_base, e->n_cu, &e->knobs,
                        e->d_q, nq, radius, out, out_cap, out_offsets, false, &e->radius_work, e->stream, &e->err);
  timing_end(e);
  return rc;
}

int vc_search_radius_dev(vc_engine* e, const void* d_queries, uint32_t nq, uint32_t radius, uint32_t mode, uint64_t* d_out,
                         uint64_t out_cap, uint64_t* d_offsets, void* stream) {
  if (!e || !d_queries || !d_offsets || (!d_out && out_cap) || nq == 0) return VC_ERR_INVALID;
  if (mode != VC_MODE_LINEAR && mode != VC_MODE_MIH_EXACT) return fail(e, VC_ERR_INVALID, "radius search: mode must be LINEAR or MIH_EXACT");
  if (mode == VC_MODE_MIH_EXACT && !live_index(e)) return fail(e, VC_ERR_STATE, "MIH search needs vc_build_index() first");
  int rc = bind_device(e);
  if (rc) return rc;
  const StreamCall call(e, caller_stream(e, stream));
  return vc_radius_search(live_index(e), mode == VC_MODE_MIH_EXACT, e->d_cols, e->stride, e->n, e->W, e->cfg.id_base, e->n_cu, &e->knobs,
                          (const uint64_t*)d_queries, nq, radius, d_out, out_cap, d_offsets, true, &e->radius_work, e->stream, &e->err);
}

}  // extern "C"
