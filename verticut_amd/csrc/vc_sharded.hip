// ============================================================================
// vc_sharded.hip -- the vc_sharded_* family of include/verticut_gpu.h: ONE process drives the GPUs of a node.
//
// Replaces the reference's distribution layer for this path:
//   src/search_worker.cc:99-101,177,207  per-radius MPI_Gather / Gatherv / Bcast between the ranks
//   src/mpi_coordinator.cc:34-69         gather_vectors (variable-length concat on rank 0)
//   src/search_worker.cc:179-199         master-side dedup map + heap
// by: the database split BY ID RANGE into shards (one vc_engine each, shard g on device_ids[g % n_devices]); every
// shard answers the whole query batch for its ids; the per-shard top-k rows -- nq * k * 8 bytes per shard, the only
// inter-GPU traffic of a batch -- are brought together by ONE exchange and merged by vc_merge_topk_dev:
//   VC_EXCHANGE_RCCL       single-process ncclCommInitAll over the devices + a grouped ncclAllGather on the shards'
//                          own streams (one shard per device); librccl is opened lazily with dlopen, so the library
//                          has no link-time dependency on it and a process that already carries RCCL (PyTorch)
//                          keeps its copy
//   VC_EXCHANGE_PEER_COPY  hipMemcpyPeerAsync of each shard's rows into the root device's gather buffer, ordered
//                          behind the shard's search by an event; also the path when several shards share a device
// No CPU compute anywhere: the host moves pointers, the merge is the device kernel of vc_scan.hip.
// ============================================================================
#include <dlfcn.h>
#include <rccl/rccl.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "vc_internal.hpp"
#include "vc_mih.hpp"

namespace {

struct RcclApi {
  void* lib = nullptr;
  decltype(&ncclCommInitAll) CommInitAll = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  bool load(std::string* why) {
    if (lib) return true;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (lib) break;
    }
    if (!lib) {
      if (why) *why = std::string("librccl not loadable: ") + dlerror();
      return false;
    }
#define VC_SYM(field, sym)                                   \
  field = (decltype(field))dlsym(lib, sym);                  \
  if (!field) {                                              \
    if (why) *why = std::string("librccl lacks ") + sym;     \
    dlclose(lib);                                            \
    lib = nullptr;                                           \
    return false;                                            \
  }
    VC_SYM(CommInitAll, "ncclCommInitAll")
    VC_SYM(CommDestroy, "ncclCommDestroy")
    VC_SYM(AllGather, "ncclAllGather")
    VC_SYM(GroupStart, "ncclGroupStart")
    VC_SYM(GroupEnd, "ncclGroupEnd")
    VC_SYM(GetErrorString, "ncclGetErrorString")
#undef VC_SYM
    return true;
  }
};

// One lane per distinct device: the shards that live there run ONE AFTER THE OTHER on the lane's stream -- at most one
// persistent-grid kernel sequence per GPU (the recovery kernel's grid barrier needs its whole grid resident; a neighbour
// shard's full-chip verify grid on another stream could keep it off the CUs for seconds: ADVICE round 3) -- while the
// lanes, i.e. the devices, run concurrently.  The root device's lane runs on the caller's stream.
struct Lane {
  int dev = 0;
  std::vector<uint32_t> shards;
  hipStream_t stream = nullptr;                   // own stream (the root lane uses the caller's)
  hipEvent_t done = nullptr;                      // behind the lane's last shard of a batch
  void* q = nullptr;        size_t q_bytes = 0;   // the batch's queries on this device (peer copy from the root)
  uint64_t* gath = nullptr; size_t gath_bytes = 0;   // [G][slot]: shard g's rows | counts | statistics at slot g; on the root
                                                     // (and, with RCCL, everywhere) the gathered results of all shards
  uint32_t* aux = nullptr;  size_t aux_bytes = 0;    // union scan of VC_FLAG_GLOBAL_STOP: its per-query inputs and outputs here
};

}  // namespace

struct vc_sharded {
  vc_sharded_config cfg;
  uint32_t G = 0, D = 0, nbytes = 0;
  uint64_t capacity = 0, n = 0;
  std::vector<vc_engine*> eng;
  std::vector<int> dev;                 // device of shard g
  std::vector<uint64_t> lo, hi;         // ids [lo, hi) relative to cfg.engine.id_base
  std::vector<Lane> lanes;
  std::vector<uint32_t> lane_of;        // shard -> lane
  uint32_t root_lane = 0;
  int root = 0;                         // device that merges
  hipStream_t root_stream = nullptr;    // stream of the host-pointer calls / VC_STREAM_OWN
  hipEvent_t ev_q = nullptr;            // "the batch's queries are ready" on the caller's stream
  void* d_hq = nullptr;         size_t hq_bytes = 0;      // host-pointer API: staged queries, merged rows, counts, statistics
  uint64_t* d_out = nullptr;    size_t out_bytes = 0;
  uint32_t* d_ocnt = nullptr;   size_t ocnt_bytes = 0;
  vc_query_stats* d_ostats = nullptr; size_t ostats_bytes = 0;
  // VC_FLAG_GLOBAL_STOP (root device): round lists + counters + floors, gathered queries, merged rows / counts / statistics,
  // the union scan's per-query words and the shards' tie ids
  uint32_t* gs_u32 = nullptr;   size_t gs_u32_bytes = 0;
  uint64_t* gs_q = nullptr;     size_t gs_q_bytes = 0;
  uint64_t* gs_rows = nullptr;  size_t gs_rows_bytes = 0;
  uint32_t* gs_cnt = nullptr;   size_t gs_cnt_bytes = 0;
  vc_query_stats* gs_st = nullptr; size_t gs_st_bytes = 0;
  uint32_t* gs_scan = nullptr;  size_t gs_scan_bytes = 0;
  VcKnobs knobs;                // the handle's own developer knobs: gs_cap (first round's cap), gs_trace
  RcclApi rccl;
  std::vector<ncclComm_t> comms;
  uint32_t exchange = VC_EXCHANGE_PEER_COPY;   // what is in use
  std::string err;
};

static thread_local std::string g_sharded_create_err;

static int sfail(vc_sharded* h, int code, const char* fmt, ...) {
  char b[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(b, sizeof b, fmt, ap);
  va_end(ap);
  if (h) h->err = b; else g_sharded_create_err = b;
  return code;
}

#define VS_HIP(h, call)                                                                                        \
  do {                                                                                                         \
    hipError_t _r = (call);                                                                                    \
    if (_r != hipSuccess)                                                                                      \
      return sfail(h, _r == hipErrorOutOfMemory ? VC_ERR_NOMEM : VC_ERR_HIP, "%s: %s", #call, hipGetErrorString(_r)); \
  } while (0)

template <class T>
static int sgrow(vc_sharded* h, T** p, size_t* have, size_t need) {
  if (need <= *have) return VC_OK;
  if (*p) VS_HIP(h, hipFree(*p));
  *p = nullptr;
  *have = 0;
  need = (need + 255) & ~(size_t)255;
  VS_HIP(h, hipMalloc((void**)p, need));
  *have = need;
  return VC_OK;
}

static uint32_t shard_of(const vc_sharded* h, uint64_t pos) {   // pos relative to id_base, < capacity
  uint32_t g = (uint32_t)std::min<uint64_t>(h->G - 1, pos * h->G / std::max<uint64_t>(h->capacity, 1));
  while (g + 1 < h->G && pos >= h->hi[g]) ++g;
  while (g > 0 && pos < h->lo[g]) --g;
  return g;
}

static uint64_t shard_size(const vc_sharded* h, uint32_t g) {   // records shard g holds (ingest fills the id ranges in order)
  return h->n <= h->lo[g] ? 0 : std::min(h->n, h->hi[g]) - h->lo[g];
}

extern "C" {

const char* vc_sharded_last_error(const vc_sharded* h) { return h ? h->err.c_str() : g_sharded_create_err.c_str(); }

int vc_sharded_destroy(vc_sharded* h) {
  if (!h) return VC_OK;
  for (Lane& l : h->lanes) {
    (void)hipSetDevice(l.dev);
    (void)hipDeviceSynchronize();
  }
  if (!h->comms.empty() && h->rccl.CommDestroy)
    for (ncclComm_t c : h->comms)
      if (c) (void)h->rccl.CommDestroy(c);
  for (Lane& l : h->lanes) {
    (void)hipSetDevice(l.dev);
    (void)hipFree(l.q); (void)hipFree(l.gath); (void)hipFree(l.aux);
    if (l.done) (void)hipEventDestroy(l.done);
    if (l.stream) (void)hipStreamDestroy(l.stream);
  }
  for (vc_engine* e : h->eng) vc_destroy(e);
  (void)hipSetDevice(h->root);
  (void)hipFree(h->d_hq); (void)hipFree(h->d_out); (void)hipFree(h->d_ocnt); (void)hipFree(h->d_ostats);
  (void)hipFree(h->gs_u32); (void)hipFree(h->gs_q); (void)hipFree(h->gs_rows); (void)hipFree(h->gs_cnt); (void)hipFree(h->gs_st);
  (void)hipFree(h->gs_scan);
  if (h->ev_q) (void)hipEventDestroy(h->ev_q);
  if (h->root_stream) (void)hipStreamDestroy(h->root_stream);
  delete h;
  return VC_OK;
}

int vc_sharded_create(const vc_sharded_config* cfg, vc_sharded** out) {
  if (!cfg || !out) return sfail(nullptr, VC_ERR_INVALID, "null argument");
  *out = nullptr;
  if (cfg->abi_version != VC_ABI_VERSION) return sfail(nullptr, VC_ERR_INVALID, "abi_version %u != %u", cfg->abi_version, VC_ABI_VERSION);
  if (cfg->n_shards == 0 || cfg->n_shards > VC_MAX_SHARDS) return sfail(nullptr, VC_ERR_INVALID, "n_shards must be 1..%d", VC_MAX_SHARDS);
  if (cfg->n_devices > VC_MAX_SHARDS) return sfail(nullptr, VC_ERR_INVALID, "n_devices must be <= %d", VC_MAX_SHARDS);
  if (cfg->exchange > VC_EXCHANGE_RCCL) return sfail(nullptr, VC_ERR_INVALID, "unknown exchange %u", cfg->exchange);
  if (cfg->engine.capacity == 0 || cfg->engine.capacity + (uint64_t)cfg->engine.id_base > 0x100000000ull)
    return sfail(nullptr, VC_ERR_INVALID, "capacity must be > 0 and id_base + capacity <= 2^32 (ids are uint32)");
  if (cfg->engine.flags & VC_FLAG_GLOBAL_STOP) {   // the global stop reproduces an exact radius loop whose statistics have a closed form
    const uint32_t f = cfg->engine.flags, m = cfg->engine.n_tables;
    if (m == 0) return sfail(nullptr, VC_ERR_INVALID, "VC_FLAG_GLOBAL_STOP needs an MIH index (n_tables > 0)");
    if (f & VC_FLAG_REF_SIGNEXT_KEYS)
      return sfail(nullptr, VC_ERR_INVALID, "VC_FLAG_GLOBAL_STOP: VC_FLAG_REF_SIGNEXT_KEYS makes the radius loop inexact");
    if ((f & VC_FLAG_REF_STOP_LITERAL4) && m < 4)
      return sfail(nullptr, VC_ERR_INVALID, "VC_FLAG_GLOBAL_STOP: VC_FLAG_REF_STOP_LITERAL4 with fewer than 4 tables makes the radius loop inexact");
    if (f & VC_FLAG_USE_BITMAP)
      return sfail(nullptr, VC_ERR_INVALID, "VC_FLAG_GLOBAL_STOP: the statistics of VC_FLAG_USE_BITMAP would need the union's bitmap");
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return sfail(nullptr, VC_ERR_NO_DEVICE, "no HIP device visible");
  vc_sharded* h = new vc_sharded();
  h->cfg = *cfg;
  h->G = cfg->n_shards;
  h->D = cfg->n_devices ? cfg->n_devices : (uint32_t)std::min<int>(ndev, (int)cfg->n_shards);
  h->capacity = cfg->engine.capacity;
  h->nbytes = cfg->engine.bits / 8;
  read_knobs(&h->knobs);
  h->eng.assign(h->G, nullptr);
  h->dev.resize(h->G);
  h->lo.resize(h->G);
  h->hi.resize(h->G);
  h->lane_of.resize(h->G);
  int rc = VC_OK;
  for (uint32_t g = 0; g < h->G && rc == VC_OK; ++g) {
    h->dev[g] = cfg->n_devices ? cfg->device_ids[g % h->D] : (int)(g % h->D);
    h->lo[g] = h->capacity * g / h->G;
    h->hi[g] = h->capacity * (g + 1) / h->G;
    if (h->dev[g] < 0 || h->dev[g] >= ndev) { rc = sfail(nullptr, VC_ERR_NO_DEVICE, "device %d of shard %u is out of range (%d visible)", h->dev[g], g, ndev); break; }
    vc_config ec = cfg->engine;
    ec.capacity = std::max<uint64_t>(h->hi[g] - h->lo[g], 1);
    ec.id_base = cfg->engine.id_base + (uint32_t)h->lo[g];
    ec.device = h->dev[g];
    ec.flags |= VC_FLAG_LEAN_TIMING;
    rc = vc_create(&ec, &h->eng[g]);
    if (rc != VC_OK) { g_sharded_create_err = std::string("shard ") + std::to_string(g) + ": " + vc_last_error(nullptr); break; }
    uint32_t li = 0;
    while (li < h->lanes.size() && h->lanes[li].dev != h->dev[g]) ++li;
    if (li == h->lanes.size()) {
      h->lanes.emplace_back();
      Lane& l = h->lanes.back();
      l.dev = h->dev[g];
      if (hipSetDevice(l.dev) != hipSuccess || hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking) != hipSuccess ||
          hipEventCreateWithFlags(&l.done, hipEventDisableTiming) != hipSuccess)
        rc = sfail(nullptr, VC_ERR_HIP, "device %d: stream / event creation failed", l.dev);
    }
    h->lanes[li].shards.push_back(g);
    h->lane_of[g] = li;
  }
  if (rc == VC_OK) {
    h->root = h->dev[0];
    h->root_lane = h->lane_of[0];
    if (hipSetDevice(h->root) != hipSuccess || hipStreamCreateWithFlags(&h->root_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_q, hipEventDisableTiming) != hipSuccess)
      rc = sfail(nullptr, VC_ERR_HIP, "root stream / event creation failed");
  }
  // peer access root <- every other device (hipMemcpyPeerAsync works without it through a staged copy; with it the
  // copy is one xGMI transfer)
  if (rc == VC_OK)
    for (uint32_t g = 0; g < h->G; ++g)
      if (h->dev[g] != h->root) {
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, h->root, h->dev[g]) == hipSuccess && can) {
          (void)hipSetDevice(h->root);
          hipError_t r = hipDeviceEnablePeerAccess(h->dev[g], 0);
          if (r != hipSuccess && r != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
        }
      }
  // exchange: RCCL needs one shard per device (a communicator rank is a device)
  if (rc == VC_OK) {
    bool one_per_device = h->G == h->D;
    for (uint32_t g = 0; g < h->G && one_per_device; ++g)
      for (uint32_t g2 = 0; g2 < g; ++g2)
        if (h->dev[g] == h->dev[g2]) one_per_device = false;
    const bool want_rccl = cfg->exchange == VC_EXCHANGE_RCCL || (cfg->exchange == VC_EXCHANGE_AUTO && one_per_device && h->G > 1);
    h->exchange = VC_EXCHANGE_PEER_COPY;
    if (want_rccl) {
      std::string why;
      if (!one_per_device) {
        why = "RCCL exchange needs exactly one shard per device";
      } else if (h->rccl.load(&why)) {
        h->comms.assign(h->G, nullptr);
        ncclResult_t nr = h->rccl.CommInitAll(h->comms.data(), (int)h->G, h->dev.data());
        if (nr == ncclSuccess) h->exchange = VC_EXCHANGE_RCCL;
        else { why = std::string("ncclCommInitAll: ") + h->rccl.GetErrorString(nr); h->comms.clear(); }
      }
      if (h->exchange != VC_EXCHANGE_RCCL && cfg->exchange == VC_EXCHANGE_RCCL) rc = sfail(nullptr, VC_ERR_STATE, "%s", why.c_str());
    }
  }
  if (rc != VC_OK) {
    vc_sharded_destroy(h);
    return rc;
  }
  *out = h;
  return VC_OK;
}

int vc_sharded_exchange(const vc_sharded* h, uint32_t* kind) {
  if (!h || !kind) return VC_ERR_INVALID;
  *kind = h->exchange;
  return VC_OK;
}

int vc_sharded_size(const vc_sharded* h, uint64_t* n) {
  if (!h || !n) return VC_ERR_INVALID;
  *n = h->n;
  return VC_OK;
}

int vc_sharded_shard(vc_sharded* h, uint32_t shard, vc_engine** e, uint64_t* first_id, uint64_t* n_ids) {
  if (!h || shard >= h->G) return VC_ERR_INVALID;
  if (e) *e = h->eng[shard];
  if (first_id) *first_id = (uint64_t)h->cfg.engine.id_base + h->lo[shard];
  if (n_ids) *n_ids = h->hi[shard] - h->lo[shard];
  return VC_OK;
}

// records arrive in global id order (build_hash_tables.cc:40-70: id = ordinal of the record in the file) and fill
// the shards' id ranges one after the other
int vc_sharded_add_codes(vc_sharded* h, const void* codes, uint64_t n) {
  if (!h || (!codes && n)) return VC_ERR_INVALID;
  if (h->n + n > h->capacity) return sfail(h, VC_ERR_CAPACITY, "add %llu codes: beyond capacity %llu", (unsigned long long)n, (unsigned long long)h->capacity);
  const uint8_t* src = (const uint8_t*)codes;
  while (n) {
    const uint32_t g = shard_of(h, h->n);
    const uint64_t take = std::min<uint64_t>(n, h->hi[g] - h->n);
    int rc = vc_add_codes(h->eng[g], src, take);
    if (rc) return sfail(h, rc, "shard %u: %s", g, vc_last_error(h->eng[g]));
    src += take * h->nbytes;
    h->n += take;
    n -= take;
  }
  return VC_OK;
}

int vc_sharded_add_synthetic(vc_sharded* h, uint64_t n, uint64_t seed, uint32_t kind, uint32_t n_centres, uint32_t max_flips) {
  if (!h) return VC_ERR_INVALID;
  if (h->n + n > h->capacity) return sfail(h, VC_ERR_CAPACITY, "add_synthetic beyond capacity");
  while (n) {
    const uint32_t g = shard_of(h, h->n);
    const uint64_t take = std::min<uint64_t>(n, h->hi[g] - h->n);
    int rc = vc_add_synthetic(h->eng[g], take, seed, kind, n_centres, max_flips);
    if (rc) return sfail(h, rc, "shard %u: %s", g, vc_last_error(h->eng[g]));
    h->n += take;
    n -= take;
  }
  return VC_OK;
}

int vc_sharded_build_index(vc_sharded* h) {
  if (!h) return VC_ERR_INVALID;
  for (uint32_t g = 0; g < h->G; ++g) {
    if (shard_size(h, g) == 0) continue;   // a store filled below its capacity leaves the trailing shards empty: nothing to index
    int rc = vc_build_index(h->eng[g]);
    if (rc) return sfail(h, rc, "shard %u: %s", g, vc_last_error(h->eng[g]));
  }
  return VC_OK;
}

int vc_sharded_get_code(vc_sharded* h, uint32_t id, void* out) {
  if (!h || !out) return VC_ERR_INVALID;
  if (id < h->cfg.engine.id_base || (uint64_t)id - h->cfg.engine.id_base >= h->n) return VC_NOT_FOUND;
  return vc_get_code(h->eng[shard_of(h, id - h->cfg.engine.id_base)], id, out);
}

// HashIndex -> Image_List over all shards: a bucket is the concatenation of the shards' buckets in shard (= id) order
int vc_sharded_get_bucket(vc_sharded* h, uint32_t table, uint32_t index, uint32_t* ids, void* codes, uint32_t cap, uint32_t* n) {
  if (!h || !n) return VC_ERR_INVALID;
  uint32_t total = 0;
  for (uint32_t g = 0; g < h->G; ++g) {
    if (shard_size(h, g) == 0) continue;
    uint32_t got = 0;
    const uint32_t room = total < cap ? cap - total : 0;
    int rc = vc_get_bucket(h->eng[g], table, index, ids ? ids + std::min(total, cap) : nullptr,
                           codes ? (uint8_t*)codes + (size_t)std::min(total, cap) * h->nbytes : nullptr, room, &got);
    if (rc < 0) return sfail(h, rc, "shard %u: %s", g, vc_last_error(h->eng[g]));
    total += got;
  }
  *n = total;
  return total ? VC_OK : VC_NOT_FOUND;
}

// ---- a batch -------------------------------------------------------------------------------------------------
// Slot of shard g in a gather buffer: [nq][k] rows | [nq] counts (padded to 8 bytes) | [nq] vc_query_stats (when wanted).
// Rows, counts and statistics travel together: ONE peer copy per remote shard, or ONE all-gather.
struct SlotLayout {
  size_t rows, cnt_off, stats_off, words;
  SlotLayout(uint32_t nq, uint32_t k, bool stats) {
    rows = (size_t)nq * k;
    cnt_off = rows;
    stats_off = rows + ((size_t)nq + 1) / 2;
    words = stats_off + (stats ? (size_t)nq * (sizeof(vc_query_stats) / 8) : 0);
  }
};
static_assert(sizeof(vc_query_stats) == 40, "slot layout assumes 5 words per vc_query_stats");

// SearchWorker::get_stat over the shards: every shard stops by its own rule -- the widest radius, the summed work
__global__ void vc_sharded_stats_kernel(const uint64_t* __restrict__ base, uint64_t slot_words, uint64_t stats_off, uint32_t G, uint32_t nq,
                                        const uint32_t* __restrict__ merged_cnt, vc_query_stats* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  vc_query_stats s{};
  for (uint32_t g = 0; g < G; ++g) {
    const vc_query_stats t = ((const vc_query_stats*)(base + (uint64_t)g * slot_words + stats_off))[i];
    s.radius = max(s.radius, t.radius);
    s.n_sub_reads += t.n_sub_reads;
    s.n_local_reads += t.n_local_reads;
    s.n_candidates += t.n_candidates;
  }
  s.n_results = merged_cnt[i];
  out[i] = s;
}

// Everything of a batch is enqueued, nothing is waited for (LINEAR; the MIH modes make the host wait inside each shard's
// vc_search_knn_dev -- how many queries continue decides what is enqueued next -- which is why lanes of different devices
// then run on host threads): queries, rows, counts and statistics live in HBM on the root device, valid in `S` order.
// r_cap != VC_NO_CAP (VC_MODE_MIH_EXACT only): every shard runs capped at that shell (vc_engine_knn_capped), the round of the
// global stop; the slots stay in the root lane's gather buffer for its settle kernel.
#define VC_NO_CAP 0xFFFFFFFFu
static int sharded_search_dev(vc_sharded* h, const void* d_queries, uint32_t nq, uint32_t k, uint32_t mode, uint64_t* d_out,
                              uint32_t* d_counts, vc_query_stats* d_stats, hipStream_t S, uint32_t r_cap = VC_NO_CAP) {
  const SlotLayout L(nq, k, d_stats != nullptr);
  const size_t qbytes = (size_t)nq * h->nbytes;
  int rc;
  for (uint32_t li = 0; li < h->lanes.size(); ++li) {
    Lane& l = h->lanes[li];
    const bool everything = li == h->root_lane || h->exchange == VC_EXCHANGE_RCCL;   // gathered results of all shards land here
    VS_HIP(h, hipSetDevice(l.dev));
    if ((rc = sgrow(h, &l.gath, &l.gath_bytes, L.words * 8 * (everything ? h->G : l.shards.back() + 1)))) return rc;
    if (li != h->root_lane && (rc = sgrow(h, (uint8_t**)&l.q, &l.q_bytes, qbytes))) return rc;
  }
  Lane& R = h->lanes[h->root_lane];
  if (!d_counts) {
    VS_HIP(h, hipSetDevice(h->root));
    if ((rc = sgrow(h, &h->d_ocnt, &h->ocnt_bytes, (size_t)nq * 4))) return rc;
    d_counts = h->d_ocnt;
  }
  // ---- the queries reach every device once: an event on the caller's stream, a peer copy per remote lane
  if (h->lanes.size() > 1) {
    VS_HIP(h, hipSetDevice(h->root));
    VS_HIP(h, hipEventRecord(h->ev_q, S));
    for (uint32_t li = 0; li < h->lanes.size(); ++li) {
      if (li == h->root_lane) continue;
      Lane& l = h->lanes[li];
      VS_HIP(h, hipSetDevice(l.dev));
      VS_HIP(h, hipStreamWaitEvent(l.stream, h->ev_q, 0));   // also orders the lane behind the previous batch's copies out of its slots
      VS_HIP(h, hipMemcpyPeerAsync(l.q, l.dev, d_queries, h->root, qbytes, l.stream));
    }
  }
  // ---- every shard answers the batch for its id range, the shards of a device one after the other
  std::vector<int> lane_rc(h->lanes.size(), VC_OK);
  std::vector<std::string> lane_err(h->lanes.size());
  auto run_lane = [&](uint32_t li) {
    Lane& l = h->lanes[li];
    const bool is_root = li == h->root_lane;
    hipStream_t ls = is_root ? S : l.stream;
    const void* q = is_root ? d_queries : l.q;
    auto hip = [&](hipError_t r, const char* what) {
      if (r != hipSuccess && lane_rc[li] == VC_OK) { lane_rc[li] = VC_ERR_HIP; lane_err[li] = std::string(what) + ": " + hipGetErrorString(r); }
      return r == hipSuccess;
    };
    if (!hip(hipSetDevice(l.dev), "hipSetDevice")) return;
    for (uint32_t g : l.shards) {
      uint64_t* slot = l.gath + (size_t)g * L.words;
      if (shard_size(h, g) == 0) {
        // an empty shard (a store filled below its capacity) contributes INF rows, zero counts, zero statistics; its engine
        // is never asked -- an exact radius loop over nothing would walk every shell of every table (search_worker.cc:170)
        if (!hip(hipMemsetAsync(slot, 0xFF, L.rows * 8, ls), "hipMemsetAsync") ||
            !hip(hipMemsetAsync(slot + L.cnt_off, 0, (L.words - L.cnt_off) * 8, ls), "hipMemsetAsync")) return;
        continue;
      }
      vc_query_stats* sst = d_stats ? (vc_query_stats*)(slot + L.stats_off) : nullptr;
      const int r = r_cap != VC_NO_CAP ? vc_engine_knn_capped(h->eng[g], q, nq, k, r_cap, slot, (uint32_t*)(slot + L.cnt_off), sst, ls)
                                       : vc_search_knn_dev_stats(h->eng[g], q, nq, k, mode, slot, (uint32_t*)(slot + L.cnt_off), sst, ls);
      if (r != VC_OK) { lane_rc[li] = r; lane_err[li] = std::string("shard ") + std::to_string(g) + ": " + vc_last_error(h->eng[g]); return; }
    }
    if (!is_root) hip(hipEventRecord(l.done, ls), "hipEventRecord");
  };
  if (mode == VC_MODE_LINEAR || h->lanes.size() == 1) {
    for (uint32_t li = 0; li < h->lanes.size(); ++li) run_lane(li);
  } else {
    std::vector<std::thread> th;
    for (uint32_t li = 0; li < h->lanes.size(); ++li) th.emplace_back(run_lane, li);
    for (auto& t : th) t.join();
  }
  for (uint32_t li = 0; li < h->lanes.size(); ++li)
    if (lane_rc[li]) return sfail(h, lane_rc[li], "%s", lane_err[li].c_str());
  // ---- ONE exchange (replaces gather_vectors, mpi_coordinator.cc:34-69): every shard's slot -> the root's gather buffer
  if (h->exchange == VC_EXCHANGE_RCCL) {
    ncclResult_t nr = h->rccl.GroupStart();
    for (uint32_t g = 0; g < h->G && nr == ncclSuccess; ++g) {   // rank g = shard g = its device's lane; in place: the send slot sits in the receive buffer
      Lane& l = h->lanes[h->lane_of[g]];
      nr = h->rccl.AllGather(l.gath + (size_t)g * L.words, l.gath, L.words, ncclUint64, h->comms[g], h->lane_of[g] == h->root_lane ? S : l.stream);
    }
    const ncclResult_t ne = h->rccl.GroupEnd();
    if (nr == ncclSuccess) nr = ne;
    if (nr != ncclSuccess) return sfail(h, VC_ERR_HIP, "ncclAllGather: %s", h->rccl.GetErrorString(nr));
  } else {
    VS_HIP(h, hipSetDevice(h->root));
    for (uint32_t li = 0; li < h->lanes.size(); ++li) {
      if (li == h->root_lane) continue;      // the root's shards wrote their slots in place
      Lane& l = h->lanes[li];
      VS_HIP(h, hipStreamWaitEvent(S, l.done, 0));
      for (uint32_t g : l.shards)
        VS_HIP(h, hipMemcpyPeerAsync(R.gath + (size_t)g * L.words, h->root, l.gath + (size_t)g * L.words, l.dev, L.words * 8, S));
    }
  }
  // ---- merge (replaces the master's heap, search_worker.cc:179-199); a flagged shard row flags the merged row
  VS_HIP(h, hipSetDevice(h->root));
  VS_HIP(h, vc_launch_select_slots(R.gath, L.words, (uint32_t)L.cnt_off, h->G, nq, k, d_out, d_counts, S));
  if (d_stats) {
    hipLaunchKernelGGL(vc_sharded_stats_kernel, dim3((nq + 255) / 256), dim3(256), 0, S, (const uint64_t*)R.gath, (uint64_t)L.words,
                       (uint64_t)L.stats_off, h->G, nq, (const uint32_t*)d_counts, d_stats);
    VS_HIP(h, hipGetLastError());
  }
  return VC_OK;
}

// ---- VC_FLAG_GLOBAL_STOP ------------------------------------------------------------------------------------------------
// Exact MIH over the shards with the stop decision of ONE SearchWorker over the union (the reference's master tests the
// merged heap, qmax.top().dist <= radius * 4, and broadcasts is_stop: search_worker.cc:179-207, mpi_coordinator.cc:26-69).
// The shards run in CAPPED rounds (vc_engine_knn_capped: shells 0..t, the shard's own stop rule active, no scan switch); the
// merged rows of a round are judged on the root by gs_settle_kernel, one thread per query.  What it rests on (D = merged k-th
// distance, e_g = last shell shard g evaluated, mult = the stop multiplier min(m, 4)):
//   * a shard's rows hold every one of its items below m (e_g + 1) (pigeonhole), so D <= m (e_lo + 1) over the non-empty
//     shards makes D the union's exact k-th distance D*; a shard that stopped by its own rule always meets it;
//   * the union loop stops at R = ceil(D* / mult) - 1 (0 for D* = 0) -- when mult == m and D* = m r0 it may already stop at
//     r0 - 1 (then R = r0 - 1 iff shell r0 - 1 holds k items at or below D*: mih_replay_kernel's rule), else at r0;
//   * no shard stops before R (its local k-th distance is never below the union's), so in a round capped at t = R every shard
//     ends at e_g = R: the merged rows are the union loop's rows at R and the shards' candidate counts add up to its count.
// A query is settled when its round ended every shard in the shell R requires; otherwise the kernel files it under the cap
// the next round needs.  Queries that need a shell beyond the shards' in-block reach (far or uniform queries) go to the
// union scan: LINEAR over the shards gives D* and the rows, mih_tie_collect_kernel decides the tie at the threshold and
// vc_launch_minsub_count counts the candidates -- the union-wide counterpart of the single engine's scan + replay.
#define GS_CAPS 17u   // caps 0..16 (inblock_last_shell never goes beyond 16)

__device__ __forceinline__ unsigned long long gs_leaves(uint32_t S, uint32_t R) {   // table 0's gets of shells 0..R: sum of C(S, r)
  unsigned long long c = 1, sum = 0;
  for (uint32_t r = 0; r <= R && r <= S; ++r) {
    sum += c;
    c = c * (S - r) / (r + 1);
  }
  return sum;
}

__global__ void __launch_bounds__(256) gs_iota_kernel(uint32_t* __restrict__ p, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = i;
}

struct GsSettleArgs {
  const uint64_t* base;          // the round's gathered slots (rows | counts | statistics per shard)
  uint64_t slot_words, stats_off;
  uint32_t G, nonempty;          // bit g: shard g holds records
  uint32_t n, t, k, m, S, mult, reach, nq;
  const uint32_t* list;          // [n] query of merged row j
  const uint64_t* rows;          // [n][k] merged rows
  const uint32_t* cnt;           // [n]
  uint32_t* floor_;              // [nq] the union loop cannot stop below this shell
  uint64_t* out;                 // final rows / counts / statistics, by query
  uint32_t* out_cnt;
  vc_query_stats* out_stats;     // may be null
  uint32_t* next;                // [GS_CAPS][nq] lists of the next round, counters next_ctr[cap]
  uint32_t* next_ctr;
  uint32_t* scan;                // union-scan list, counter *scan_ctr
  uint32_t* scan_ctr;
};

__global__ void __launch_bounds__(256) gs_settle_kernel(const GsSettleArgs a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.n) return;
  const uint32_t q = a.list[j];
  const uint32_t c = min(a.cnt[j], a.k);
  const uint64_t* row = a.rows + (uint64_t)j * a.k;
  uint32_t e_lo = 0xFFFFFFFFu, e_hi = 0;
  unsigned long long seen = 0;
  for (uint32_t g = 0; g < a.G; ++g) {
    if (!((a.nonempty >> g) & 1u)) continue;
    const vc_query_stats s = ((const vc_query_stats*)(a.base + (uint64_t)g * a.slot_words + a.stats_off))[j];
    e_lo = min(e_lo, s.radius);
    e_hi = max(e_hi, s.radius);
    seen += s.n_candidates;
  }
  const uint32_t D = c == a.k ? (uint32_t)(row[a.k - 1] >> 32) : 0xFFFFFFFFu;
  uint32_t flo = a.floor_[q];
  // every shard ended exactly in shell t: the rows are the union loop's at t -- if it does not stop there, it stops later
  const bool at_t = e_lo == a.t && e_hi == a.t;
  if (at_t && !(c == a.k && D <= a.mult * (a.t + 1))) flo = max(flo, a.t + 1);
  uint32_t R = 0xFFFFFFFFu, next = 0xFFFFFFFFu;
  if (c < a.k) {
    if (e_lo >= a.S) R = a.S;                        // every shell searched: the union holds fewer than k items
    else next = a.t + 1;
  } else if (D > a.m * (e_lo + 1)) {
    next = (D + a.m - 1) / a.m - 1;                  // pigeonhole not met: D only bounds D* from above
  } else {
    const uint32_t rs = min(a.S, D == 0 ? 0u : (D + a.mult - 1) / a.mult - 1);
    const bool tie = a.mult == a.m && D != 0 && D % a.m == 0;
    const uint32_t want = (tie && flo > rs) ? rs + 1 : rs;
    if (e_lo == want && e_hi == want) R = want;
    else next = want;
  }
  a.floor_[q] = flo;
  if (R != 0xFFFFFFFFu) {
    uint64_t* o = a.out + (uint64_t)q * a.k;
    for (uint32_t i = 0; i < a.k; ++i) o[i] = row[i];
    a.out_cnt[q] = c;
    if (a.out_stats) {
      vc_query_stats s{};
      s.radius = R;
      s.n_results = c;
      s.n_sub_reads = gs_leaves(a.S, R);
      s.n_candidates = seen;
      a.out_stats[q] = s;
    }
  } else if (next <= a.reach) {
    a.next[(uint64_t)next * a.nq + atomicAdd(&a.next_ctr[next], 1u)] = q;
  } else {
    a.scan[atomicAdd(a.scan_ctr, 1u)] = q;
  }
}

// union scan, step 1: the rule applied to the LINEAR rows (sd = [dist | radius | need | R | iota | ones], nq apart)
__global__ void __launch_bounds__(256) gs_scan_plan_kernel(uint32_t n, uint32_t k, uint32_t m, uint32_t S, uint32_t mult,
                                                           const uint32_t* __restrict__ list, const uint32_t* __restrict__ floor_,
                                                           const uint64_t* __restrict__ rows, const uint32_t* __restrict__ cnt,
                                                           uint32_t* __restrict__ sd, uint32_t nq) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t c = min(cnt[j], k);
  const uint64_t* row = rows + (uint64_t)j * k;
  uint32_t dist = 0, rad = 0, need = 0, R = S;       // fewer than k items: the loop runs to its last shell
  if (c == k) {
    const uint32_t D = (uint32_t)(row[k - 1] >> 32);
    const uint32_t rs = min(S, D == 0 ? 0u : (D + mult - 1) / mult - 1);
    R = rs;
    if (mult == m && D != 0 && D % m == 0) {
      if (floor_[list[j]] > rs) {
        R = rs + 1;
      } else {                                       // does shell rs = D/m - 1 already hold k items at or below D?
        uint32_t below = 0;
        while (below < k && (uint32_t)(row[below] >> 32) < D) ++below;
        dist = D;
        rad = rs;
        need = k - below;
      }
    }
  }
  sd[j] = dist;
  sd[nq + j] = rad;
  sd[2 * (size_t)nq + j] = need;
  sd[3 * (size_t)nq + j] = R;
  sd[4 * (size_t)nq + j] = j;
  sd[5 * (size_t)nq + j] = 1;
}

// union scan, step 2: the shards' ties (ids ascending within a shard, shards in id order) decide the tie at the threshold
__global__ void __launch_bounds__(256) gs_scan_tie_kernel(uint32_t n, uint32_t k, uint32_t G, uint32_t* __restrict__ sd, uint32_t nq,
                                                          const uint32_t* __restrict__ tie_ids, const uint32_t* __restrict__ tie_cnt,
                                                          uint64_t* __restrict__ rows) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t need = sd[2 * (size_t)nq + j], rs = sd[nq + j], D = sd[j];
  if (need == 0) return;
  uint32_t total = 0;
  for (uint32_t g = 0; g < G; ++g) total += tie_cnt[(size_t)g * nq + j];
  if (total < need) {
    sd[3 * (size_t)nq + j] = rs + 1;                 // shell rs has too few: the loop stops at D/m with the scan's rows
    return;
  }
  uint32_t w = k - need;                             // the rows below D stay; the ties of shell rs follow, smallest ids first
  for (uint32_t g = 0; g < G && w < k; ++g)
    for (uint32_t i = 0; i < tie_cnt[(size_t)g * nq + j] && w < k; ++i)
      rows[(uint64_t)j * k + w++] = ((uint64_t)D << 32) | tie_ids[((size_t)g * nq + j) * k + i];
  sd[3 * (size_t)nq + j] = rs;
}

// union scan, step 3: rows, counts and the statistics of one SearchWorker stopping at R
__global__ void __launch_bounds__(256) gs_scan_final_kernel(uint32_t n, uint32_t k, uint32_t S, const uint32_t* __restrict__ list,
                                                            const uint32_t* __restrict__ sd, uint32_t nq, const uint64_t* __restrict__ rows,
                                                            const uint32_t* __restrict__ cnt, const unsigned long long* __restrict__ seen,
                                                            uint32_t n_lanes, uint64_t* __restrict__ out, uint32_t* __restrict__ out_cnt,
                                                            vc_query_stats* __restrict__ out_stats) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t q = list[j];
  for (uint32_t i = 0; i < k; ++i) out[(uint64_t)q * k + i] = rows[(uint64_t)j * k + i];
  out_cnt[q] = cnt[j];
  if (out_stats) {
    const uint32_t R = sd[3 * (size_t)nq + j];
    vc_query_stats s{};
    s.radius = R;
    s.n_results = cnt[j];
    s.n_sub_reads = gs_leaves(S, R);
    for (uint32_t l = 0; l < n_lanes; ++l) s.n_candidates += seen[(size_t)l * nq + j];
    out_stats[q] = s;
  }
}

static int sharded_global_stop(vc_sharded* h, const void* d_queries, uint32_t nq, uint32_t k, uint64_t* d_out, uint32_t* d_counts,
                               vc_query_stats* d_stats, hipStream_t S) {
  const uint32_t W = h->nbytes / 8, m = h->cfg.engine.n_tables, Sb = h->cfg.engine.bits / m;
  const uint32_t mult = (h->cfg.engine.flags & VC_FLAG_REF_STOP_LITERAL4) ? 4u : std::min(m, 4u);
  const bool trace = h->knobs.gs_trace;   // dev: per-round wall times on stderr
  uint32_t nonempty = 0, reach = GS_CAPS - 1;
  std::vector<VcEngineView> view(h->G);
  for (uint32_t g = 0; g < h->G; ++g) {
    vc_engine_view(h->eng[g], &view[g]);
    if (shard_size(h, g) == 0) continue;
    nonempty |= 1u << g;
    reach = std::min(reach, view[g].reach);
  }
  int rc;
  VS_HIP(h, hipSetDevice(h->root));
  if (!d_counts) {
    if ((rc = sgrow(h, &h->d_ocnt, &h->ocnt_bytes, (size_t)nq * 4))) return rc;
    d_counts = h->d_ocnt;
  }
  const size_t LW = (size_t)GS_CAPS * nq;   // words of one set of round lists
  if ((rc = sgrow(h, &h->gs_u32, &h->gs_u32_bytes, (2 * LW + 2 * (size_t)nq + 96) * 4))) return rc;
  if ((rc = sgrow(h, &h->gs_q, &h->gs_q_bytes, (size_t)nq * h->nbytes))) return rc;
  if ((rc = sgrow(h, &h->gs_rows, &h->gs_rows_bytes, (size_t)nq * k * 8))) return rc;
  if ((rc = sgrow(h, &h->gs_cnt, &h->gs_cnt_bytes, (size_t)nq * 4))) return rc;
  if ((rc = sgrow(h, &h->gs_st, &h->gs_st_bytes, (size_t)nq * sizeof(vc_query_stats)))) return rc;
  uint32_t* lists[2] = {h->gs_u32, h->gs_u32 + LW};
  uint32_t* ctr[2] = {h->gs_u32 + 2 * LW, h->gs_u32 + 2 * LW + 32};
  uint32_t* scan_ctr = h->gs_u32 + 2 * LW + 64;
  uint32_t* scan = h->gs_u32 + 2 * LW + 96;
  uint32_t* floor_ = scan + nq;
  VS_HIP(h, hipMemsetAsync(floor_, 0, (size_t)nq * 4, S));
  VS_HIP(h, hipMemsetAsync(scan_ctr, 0, 4, S));
  std::vector<uint32_t> n_at(GS_CAPS + 1, 0);   // queries per cap of the coming round | union scan
  uint32_t n_scan = 0;
  if (nonempty == 0) {   // nothing to probe: the union scan reports the empty union (R = last shell, no candidates)
    hipLaunchKernelGGL(gs_iota_kernel, dim3((nq + 255) / 256), dim3(256), 0, S, scan, nq);
    VS_HIP(h, hipGetLastError());
    n_scan = nq;
  } else {
    const uint32_t t0 = std::min(h->knobs.gs_cap, reach);
    hipLaunchKernelGGL(gs_iota_kernel, dim3((nq + 255) / 256), dim3(256), 0, S, lists[0] + (size_t)t0 * nq, nq);
    VS_HIP(h, hipGetLastError());
    n_at[t0] = nq;
  }
  Lane& Rl = h->lanes[h->root_lane];
  int cur = 0;
  for (uint32_t round = 0; round < 8; ++round) {
    bool any = false;
    for (uint32_t t = 0; t < GS_CAPS; ++t) any = any || n_at[t];
    if (!any) break;
    const auto t_round = std::chrono::steady_clock::now();
    VS_HIP(h, hipSetDevice(h->root));
    VS_HIP(h, hipMemsetAsync(ctr[cur ^ 1], 0, GS_CAPS * 4, S));
    for (uint32_t t = 0; t < GS_CAPS; ++t) {
      const uint32_t n = n_at[t];
      if (!n) continue;
      const uint32_t* list = lists[cur] + (size_t)t * nq;
      VS_HIP(h, hipSetDevice(h->root));
      VS_HIP(h, vc_launch_gather_queries((const uint64_t*)d_queries, list, n, W, h->gs_q, S));
      if ((rc = sharded_search_dev(h, h->gs_q, n, k, VC_MODE_MIH_EXACT, h->gs_rows, h->gs_cnt, h->gs_st, S, t))) return rc;
      const SlotLayout L(n, k, true);
      GsSettleArgs a{};
      a.base = Rl.gath; a.slot_words = L.words; a.stats_off = L.stats_off; a.G = h->G; a.nonempty = nonempty;
      a.n = n; a.t = t; a.k = k; a.m = m; a.S = Sb; a.mult = mult; a.reach = reach; a.nq = nq;
      a.list = list; a.rows = h->gs_rows; a.cnt = h->gs_cnt; a.floor_ = floor_;
      a.out = d_out; a.out_cnt = d_counts; a.out_stats = d_stats;
      a.next = lists[cur ^ 1]; a.next_ctr = ctr[cur ^ 1]; a.scan = scan; a.scan_ctr = scan_ctr;
      VS_HIP(h, hipSetDevice(h->root));
      hipLaunchKernelGGL(gs_settle_kernel, dim3((n + 255) / 256), dim3(256), 0, S, a);
      VS_HIP(h, hipGetLastError());
    }
    cur ^= 1;
    std::vector<uint32_t> c(GS_CAPS + 1);
    VS_HIP(h, hipMemcpyAsync(c.data(), ctr[cur], GS_CAPS * 4, hipMemcpyDeviceToHost, S));
    VS_HIP(h, hipMemcpyAsync(c.data() + GS_CAPS, scan_ctr, 4, hipMemcpyDeviceToHost, S));
    VS_HIP(h, hipStreamSynchronize(S));
    if (trace) {
      fprintf(stderr, "[vc_gs] round %u:", round);
      for (uint32_t t = 0; t < GS_CAPS; ++t) if (n_at[t]) fprintf(stderr, " cap %u x %u", t, n_at[t]);
      fprintf(stderr, " -> open");
      for (uint32_t t = 0; t < GS_CAPS; ++t) if (c[t]) fprintf(stderr, " cap %u x %u", t, c[t]);
      fprintf(stderr, ", union scan %u  %.1f us\n", c[GS_CAPS],
              std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_round).count());
    }
    n_at.assign(c.begin(), c.begin() + GS_CAPS);
    n_scan = c[GS_CAPS];
  }
  // (the rounds settle a query in at most four: the first cap, the pigeonhole cap, R, and R + 1 after a tie; 8 is a bound)
  for (uint32_t t = 0; t < GS_CAPS; ++t)
    if (n_at[t]) {
      VS_HIP(h, hipMemcpyAsync(scan + n_scan, lists[cur] + (size_t)t * nq, (size_t)n_at[t] * 4, hipMemcpyDeviceToDevice, S));
      n_scan += n_at[t];
    }
  if (n_scan == 0) return VC_OK;
  // ---- the union scan
  const auto t_scan = std::chrono::steady_clock::now();
  const uint32_t n = n_scan, NL = (uint32_t)h->lanes.size();
  VS_HIP(h, hipSetDevice(h->root));
  // root words: seen [NL][nq] u64 | sd [6][nq] | tie counts [G][nq] | tie ids [G][nq][k]
  const size_t seen_w = 2 * (size_t)NL * nq, sd_w = 6 * (size_t)nq, tc_w = (size_t)h->G * nq;
  if ((rc = sgrow(h, &h->gs_scan, &h->gs_scan_bytes, (seen_w + sd_w + tc_w + (size_t)h->G * nq * k) * 4))) return rc;
  unsigned long long* seen = (unsigned long long*)h->gs_scan;
  uint32_t* sd = h->gs_scan + seen_w;
  uint32_t* tie_cnt = sd + sd_w;
  uint32_t* tie_ids = tie_cnt + tc_w;
  VS_HIP(h, vc_launch_gather_queries((const uint64_t*)d_queries, scan, n, W, h->gs_q, S));
  if ((rc = sharded_search_dev(h, h->gs_q, n, k, VC_MODE_LINEAR, h->gs_rows, h->gs_cnt, nullptr, S))) return rc;
  VS_HIP(h, hipSetDevice(h->root));
  hipLaunchKernelGGL(gs_scan_plan_kernel, dim3((n + 255) / 256), dim3(256), 0, S, n, k, m, Sb, mult, (const uint32_t*)scan,
                     (const uint32_t*)floor_, (const uint64_t*)h->gs_rows, (const uint32_t*)h->gs_cnt, sd, nq);
  VS_HIP(h, hipGetLastError());
  // one pass over the lanes: the per-query words go out, fn runs the lane's shards, results come back
  auto over_lanes = [&](auto&& fn) -> int {
    for (uint32_t li = 0; li < NL; ++li) {
      Lane& l = h->lanes[li];
      const bool is_root = li == h->root_lane;
      hipStream_t ls = is_root ? S : l.stream;
      const size_t LS = l.shards.size();
      VS_HIP(h, hipSetDevice(h->root));
      if (!is_root) VS_HIP(h, hipEventRecord(h->ev_q, S));
      VS_HIP(h, hipSetDevice(l.dev));
      // lane words: seen [nq] u64 | sd [6][nq] | tie counts [LS][nq] | tie ids [LS][nq][k] | tie chunk counts [nq][VC_TIE_CHUNKS]
      if ((rc = sgrow(h, &l.aux, &l.aux_bytes, (2 * (size_t)nq + sd_w + LS * nq + LS * nq * k + (size_t)nq * VC_TIE_CHUNKS) * 4))) return rc;
      if (!is_root) VS_HIP(h, hipStreamWaitEvent(ls, h->ev_q, 0));
      VS_HIP(h, hipMemcpyPeerAsync(l.aux + 2 * (size_t)nq, l.dev, sd, h->root, sd_w * 4, ls));
      const uint64_t* lq = is_root ? h->gs_q : (const uint64_t*)l.q;
      if ((rc = fn(li, l, ls, lq))) return rc;
      if (!is_root) {
        VS_HIP(h, hipEventRecord(l.done, ls));
        VS_HIP(h, hipSetDevice(h->root));
        VS_HIP(h, hipStreamWaitEvent(S, l.done, 0));
      }
    }
    VS_HIP(h, hipSetDevice(h->root));
    return VC_OK;
  };
  // the tie at the threshold: every shard's smallest-id ties whose substrings reach below D/m
  if ((rc = over_lanes([&](uint32_t, Lane& l, hipStream_t ls, const uint64_t* lq) -> int {
         const uint32_t* lsd = l.aux + 2 * (size_t)nq;
         uint32_t* lcnt = l.aux + 2 * (size_t)nq + sd_w;
         uint32_t* lids = lcnt + l.shards.size() * nq;
         for (size_t i = 0; i < l.shards.size(); ++i) {
           const uint32_t g = l.shards[i];
           if (!((nonempty >> g) & 1u)) {
             VS_HIP(h, hipMemsetAsync(lcnt + i * nq, 0, (size_t)n * 4, ls));
           } else {
             const VcEngineView& v = view[g];
             VS_HIP(h, vc_launch_tie_collect(v.cols, v.stride, v.n, W, m, Sb, v.id_base, lq, n, k, lsd, lsd + nq, lsd + 2 * (size_t)nq,
                                             lids + l.shards.size() * nq * k, lids + i * nq * k, lcnt + i * nq, ls));
           }
           VS_HIP(h, hipMemcpyPeerAsync(tie_cnt + (size_t)g * nq, h->root, lcnt + i * nq, l.dev, (size_t)n * 4, ls));
           VS_HIP(h, hipMemcpyPeerAsync(tie_ids + (size_t)g * nq * k, h->root, lids + i * nq * k, l.dev, (size_t)n * k * 4, ls));
         }
         return VC_OK;
       })))
    return rc;
  hipLaunchKernelGGL(gs_scan_tie_kernel, dim3((n + 255) / 256), dim3(256), 0, S, n, k, h->G, sd, nq, (const uint32_t*)tie_ids,
                     (const uint32_t*)tie_cnt, h->gs_rows);
  VS_HIP(h, hipGetLastError());
  // the candidates of the union loop up to R: every item whose minimum substring distance is <= R
  if (d_stats) {
    if ((rc = over_lanes([&](uint32_t li, Lane& l, hipStream_t ls, const uint64_t* lq) -> int {
           const uint32_t* lsd = l.aux + 2 * (size_t)nq;
           unsigned long long* lseen = (unsigned long long*)l.aux;
           VS_HIP(h, hipMemsetAsync(lseen, 0, (size_t)n * 8, ls));
           for (uint32_t g : l.shards) {
             if (!((nonempty >> g) & 1u)) continue;
             const VcEngineView& v = view[g];
             VS_HIP(h, vc_launch_minsub_count(v.cols, v.stride, v.n, W, m, Sb, lq, lsd + 4 * (size_t)nq, lsd + 5 * (size_t)nq, n,
                                              lsd + 3 * (size_t)nq, lseen, v.n_cu, ls));
           }
           VS_HIP(h, hipMemcpyPeerAsync(seen + (size_t)li * nq, h->root, lseen, l.dev, (size_t)n * 8, ls));
           return VC_OK;
         })))
      return rc;
  }
  hipLaunchKernelGGL(gs_scan_final_kernel, dim3((n + 255) / 256), dim3(256), 0, S, n, k, Sb, (const uint32_t*)scan, (const uint32_t*)sd,
                     nq, (const uint64_t*)h->gs_rows, (const uint32_t*)h->gs_cnt, (const unsigned long long*)seen, NL, d_out, d_counts, d_stats);
  VS_HIP(h, hipGetLastError());
  if (trace) {
    VS_HIP(h, hipStreamSynchronize(S));
    fprintf(stderr, "[vc_gs] union scan: %u queries  %.1f us\n", n,
            std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_scan).count());
  }
  return VC_OK;
}

static int sharded_search_any(vc_sharded* h, const void* d_queries, uint32_t nq, uint32_t k, uint32_t mode, uint64_t* d_out,
                              uint32_t* d_counts, vc_query_stats* d_stats, hipStream_t S) {
  if (mode == VC_MODE_MIH_EXACT && (h->cfg.engine.flags & VC_FLAG_GLOBAL_STOP))
    return sharded_global_stop(h, d_queries, nq, k, d_out, d_counts, d_stats, S);
  return sharded_search_dev(h, d_queries, nq, k, mode, d_out, d_counts, d_stats, S);
}

int vc_sharded_root_device(const vc_sharded* h, int* device) {
  if (!h || !device) return VC_ERR_INVALID;
  *device = h->root;
  return VC_OK;
}

int vc_sharded_search_knn_dev(vc_sharded* h, const void* d_queries, uint32_t nq, uint32_t k, uint32_t mode, uint64_t* d_out,
                              uint32_t* d_counts, vc_query_stats* d_stats, void* stream) {
  if (!h || !d_queries || !d_out || nq == 0 || k == 0 || k > VC_MAX_K || mode > VC_MODE_MIH_APPROX) return VC_ERR_INVALID;
  return sharded_search_any(h, d_queries, nq, k, mode, d_out, d_counts, d_stats, stream == VC_STREAM_OWN ? h->root_stream : (hipStream_t)stream);
}

int vc_sharded_search_knn(vc_sharded* h, const void* queries, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order,
                          uint64_t* out, uint32_t* counts, vc_query_stats* stats) {
  if (!h || !queries || !out || nq == 0 || k == 0 || k > VC_MAX_K || mode > VC_MODE_MIH_APPROX || order > VC_ORDER_FARTHEST_FIRST)
    return VC_ERR_INVALID;
  const size_t qbytes = (size_t)nq * h->nbytes, rows = (size_t)nq * k;
  int rc;
  hipStream_t S = h->root_stream;
  VS_HIP(h, hipSetDevice(h->root));
  if ((rc = sgrow(h, (uint8_t**)&h->d_hq, &h->hq_bytes, qbytes))) return rc;
  if ((rc = sgrow(h, &h->d_out, &h->out_bytes, rows * 8))) return rc;
  if ((rc = sgrow(h, &h->d_ocnt, &h->ocnt_bytes, (size_t)nq * 4))) return rc;
  if (stats && (rc = sgrow(h, &h->d_ostats, &h->ostats_bytes, (size_t)nq * sizeof(vc_query_stats)))) return rc;
  VS_HIP(h, hipMemcpyAsync(h->d_hq, queries, qbytes, hipMemcpyHostToDevice, S));
  if ((rc = sharded_search_any(h, h->d_hq, nq, k, mode, h->d_out, h->d_ocnt, stats ? h->d_ostats : nullptr, S))) return rc;
  std::vector<uint32_t> cnt(nq);
  VS_HIP(h, hipSetDevice(h->root));
  VS_HIP(h, hipMemcpyAsync(out, h->d_out, rows * 8, hipMemcpyDeviceToHost, S));
  VS_HIP(h, hipMemcpyAsync(cnt.data(), h->d_ocnt, (size_t)nq * 4, hipMemcpyDeviceToHost, S));
  if (stats) VS_HIP(h, hipMemcpyAsync(stats, h->d_ostats, (size_t)nq * sizeof(vc_query_stats), hipMemcpyDeviceToHost, S));
  VS_HIP(h, hipStreamSynchronize(S));
  bool gave_up = false;
  for (uint32_t i = 0; i < nq; ++i) gave_up = gave_up || cnt[i] == 0xFFFFFFFFu;
  if (gave_up && mode == VC_MODE_LINEAR) {
    // A shard's device-side ring-overflow recovery gave up (its grid never met; never seen outside tests): the batch is
    // answered again through the shards' host API, whose host-driven recovery always ends, one shard after the other;
    // the rows go back into the root's slots and are merged by the same kernel.
    const SlotLayout L(nq, k, false);
    Lane& R = h->lanes[h->root_lane];
    VS_HIP(h, hipSetDevice(h->root));
    if ((rc = sgrow(h, &R.gath, &R.gath_bytes, L.words * 8 * h->G))) return rc;
    std::vector<uint64_t> slot(L.words);
    for (uint32_t g = 0; g < h->G; ++g) {
      uint32_t* c = (uint32_t*)(slot.data() + L.cnt_off);
      std::fill(slot.begin(), slot.begin() + L.rows, VC_PACK_INF);
      std::fill(slot.begin() + L.rows, slot.end(), 0ull);
      if (shard_size(h, g)) {
        rc = vc_search_knn(h->eng[g], queries, nq, k, VC_MODE_LINEAR, VC_ORDER_ASCENDING, slot.data(), c, nullptr);
        if (rc) return sfail(h, rc, "shard %u: %s", g, vc_last_error(h->eng[g]));
        for (uint32_t i = 0; i < nq; ++i)
          for (uint32_t j = c[i]; j < k; ++j) slot[(size_t)i * k + j] = VC_PACK_INF;
      }
      VS_HIP(h, hipSetDevice(h->root));
      VS_HIP(h, hipMemcpyAsync(R.gath + (size_t)g * L.words, slot.data(), L.words * 8, hipMemcpyHostToDevice, S));
      VS_HIP(h, hipStreamSynchronize(S));   // `slot` is reused by the next shard
    }
    VS_HIP(h, vc_launch_select_slots(R.gath, L.words, (uint32_t)L.cnt_off, h->G, nq, k, h->d_out, h->d_ocnt, S));
    VS_HIP(h, hipMemcpyAsync(out, h->d_out, rows * 8, hipMemcpyDeviceToHost, S));
    VS_HIP(h, hipMemcpyAsync(cnt.data(), h->d_ocnt, (size_t)nq * 4, hipMemcpyDeviceToHost, S));
    VS_HIP(h, hipStreamSynchronize(S));
  }
  for (uint32_t i = 0; i < nq; ++i) {
    // the MIH modes have no host-side recovery above: a row flagged by the slot merge (UINT32_MAX) must not be reversed
    // past its k entries nor reported as more than k results
    if (mode != VC_MODE_LINEAR) cnt[i] = std::min(cnt[i], k);
    if (order == VC_ORDER_FARTHEST_FIRST) std::reverse(out + (size_t)i * k, out + (size_t)i * k + cnt[i]);
    if (counts) counts[i] = cnt[i];
    if (stats) stats[i].n_results = cnt[i];
  }
  return VC_OK;
}

// All items within `radius` of every query over all shards (search_R_neighbors per rank + gather_vectors + the master's dedup,
// search_worker.cc:177-199,222-264: every shard searches its id range, the per-query results of the shards are brought together and
// ordered).  Shard by shard through the shards' host API (a shard's radius search waits for its own total anyway); the
// concatenated segments are ordered ON THE DEVICE by the radius search's own segment sort, one block per query.
int vc_sharded_search_radius(vc_sharded* h, const void* queries, uint32_t nq, uint32_t radius, uint32_t mode, uint64_t* out,
                             uint64_t out_cap, uint64_t* out_offsets) {
  if (!h || !queries || !out_offsets || nq == 0 || (mode != VC_MODE_LINEAR && mode != VC_MODE_MIH_EXACT) || (!out && out_cap))
    return VC_ERR_INVALID;
  std::vector<std::vector<uint64_t>> res(h->G), offs(h->G, std::vector<uint64_t>((size_t)nq + 1, 0));
  for (uint32_t g = 0; g < h->G; ++g) {
    if (shard_size(h, g) == 0) continue;
    uint64_t cap = (uint64_t)nq * 64;
    for (int attempt = 0;; ++attempt) {
      res[g].resize(std::max<uint64_t>(cap, 1));
      const int rc = vc_search_radius(h->eng[g], queries, nq, radius, mode, res[g].data(), cap, offs[g].data());
      if (rc == VC_OK) break;
      if (rc != VC_ERR_CAPACITY || attempt) return sfail(h, rc, "shard %u: %s", g, vc_last_error(h->eng[g]));
      cap = offs[g][nq];   // the needed size came back in the offsets
    }
  }
  // per-query totals -> output offsets; the largest query sizes the segment ring (a power of two, as the sort wants it)
  std::vector<uint32_t> count(nq);
  uint64_t total = 0, mx = 0;
  for (uint32_t q = 0; q < nq; ++q) {
    uint64_t c = 0;
    for (uint32_t g = 0; g < h->G; ++g) c += offs[g][q + 1] - offs[g][q];
    out_offsets[q] = total;
    total += c;
    mx = std::max(mx, c);
    if (c > 0xFFFFFFFFull) return sfail(h, VC_ERR_CAPACITY, "radius search: a query has more than 2^32 neighbours");
    count[q] = (uint32_t)c;
  }
  out_offsets[nq] = total;
  if (total > out_cap) return sfail(h, VC_ERR_CAPACITY, "radius search: output buffer too small (needed counts are in out_offsets)");
  if (total == 0) return VC_OK;
  uint64_t cap2 = 2;
  while (cap2 < mx) cap2 <<= 1;
  if (cap2 > 0x80000000ull || (uint64_t)nq * cap2 * 8 > (4ull << 30))   // (the padded segments are assembled in host memory first)
    return sfail(h, VC_ERR_CAPACITY, "radius search: result segments too large (a query with %llu neighbours x %u queries): search fewer queries per call", (unsigned long long)mx, nq);
  std::vector<uint64_t> ring((size_t)nq * cap2);
  for (uint32_t q = 0; q < nq; ++q) {      // shard after shard = ascending id ranges; the distances interleave: ordered below
    uint64_t* dst = ring.data() + (size_t)q * cap2;
    for (uint32_t g = 0; g < h->G; ++g)
      dst = std::copy(res[g].begin() + offs[g][q], res[g].begin() + offs[g][q + 1], dst);
  }
  hipStream_t S = h->root_stream;
  VS_HIP(h, hipSetDevice(h->root));
  uint64_t *d_ring = nullptr, *d_offs = nullptr, *d_out = nullptr;
  uint32_t* d_count = nullptr;
  auto cleanup = [&]() { (void)hipFree(d_ring); (void)hipFree(d_offs); (void)hipFree(d_out); (void)hipFree(d_count); };
#define VR_HIP(call) do { hipError_t _r = (call); if (_r != hipSuccess) { cleanup(); return sfail(h, _r == hipErrorOutOfMemory ? VC_ERR_NOMEM : VC_ERR_HIP, "%s: %s", #call, hipGetErrorString(_r)); } } while (0)
  VR_HIP(hipMalloc((void**)&d_ring, ring.size() * 8));
  VR_HIP(hipMalloc((void**)&d_offs, ((size_t)nq + 1) * 8));
  VR_HIP(hipMalloc((void**)&d_out, total * 8));
  VR_HIP(hipMalloc((void**)&d_count, (size_t)nq * 4));
  VR_HIP(hipMemcpyAsync(d_ring, ring.data(), ring.size() * 8, hipMemcpyHostToDevice, S));
  VR_HIP(hipMemcpyAsync(d_offs, out_offsets, ((size_t)nq + 1) * 8, hipMemcpyHostToDevice, S));
  VR_HIP(hipMemcpyAsync(d_count, count.data(), (size_t)nq * 4, hipMemcpyHostToDevice, S));
  VR_HIP(vc_launch_sort_compact_segments(d_ring, (uint32_t)cap2, d_count, d_offs, d_out, total, nq, S));
  VR_HIP(hipMemcpyAsync(out, d_out, total * 8, hipMemcpyDeviceToHost, S));
  VR_HIP(hipStreamSynchronize(S));
#undef VR_HIP
  cleanup();
  return VC_OK;
}

}  // extern "C"
