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
//
// In this file: Lane, vc_sharded (its grow-only scratch: DevBuf, vc_internal.hpp) | create / ingest / look-up | ShardBatch = one batch through the
// shards (prepare_lanes, send_queries, run_lanes, exchange, merge; sharded_search_dev) | VC_FLAG_GLOBAL_STOP: the stop rule
// (gs_stop_shell), the kernels, the layouts they share with the host (GsRoundLists, GsScanCols, GsScanBlock) and GsSearch,
// the steps of a flagged call (sharded_global_stop, GsSearch::union_scan) | the device-resident radius search: its two kernels
// (union offsets, rank merge) and ShardRadius, the steps of a call (sharded_radius_dev) | the search entry points.
// VC_FLAG_GLOBAL_APPROX (behind the global stop): ga_settle_kernel, GaRoundLists and GaSearch, the steps of a flagged approximate call
// (sharded_global_approx).
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

#include "vc_distinct_plan.hpp"
#include "vc_filter_plan.hpp"
#include "vc_internal.hpp"
#include "vc_knn_graph_plan.hpp"
#include "vc_snn_plan.hpp"
#include "vc_knn_adjacency_plan.hpp"
#include "vc_knn_mst_plan.hpp"
#include "vc_mst_condense_plan.hpp"
#include "vc_vote_plan.hpp"
#include "vc_knn_graph_update_plan.hpp"
#include "vc_mih.hpp"
#include "vc_seed_plan.hpp"
#include "vc_sharded_radius.hpp"

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
enum LaneBuf {
  LANE_Q,      // the batch's queries on this device (peer copy from the root)
  LANE_GATH,   // [G][slot]: shard g's rows | counts | statistics at slot g (SlotLayout); on the root (and, with RCCL, everywhere)
               // the gathered results of all shards
  LANE_AUX,    // union scan of VC_FLAG_GLOBAL_STOP: its per-query inputs and outputs here (GsScanBlock, gs_lane_block)
  LANE_IDS,    // queries named by id: the batch's ids on this device (peer copy from the root)
  LANE_IDGATH, // [G][slot]: the gathered words | found words of shard g at slot g (vc_ids_slot_words); on the root all shards' slots
  LANE_ACENT,  // nearest of K codes: the centres on this device (peer copy from the root)
  LANE_AOUT,   // nearest of K codes: the packed results of this device's shards, one after the other, before they travel to the root
  LANE_SWORK,  // seeding: per shard of this device its slot word, its total and its partials (SeedShard)
  LANE_SCODE,  // seeding: the round's centre code on this device (peer copy from the root)
  LANE_SBEST,  // seeding: best of this device's shards, one after the other, before it travels to the root
  LANE_BUFS
};
struct Lane {
  int dev = 0;
  std::vector<uint32_t> shards;
  hipStream_t stream = nullptr;   // own stream (the root lane uses the caller's)
  hipEvent_t done = nullptr;      // behind the lane's last shard of a batch
  DevBuf buf[LANE_BUFS];
  const void* q() const { return buf[LANE_Q].p; }
  uint64_t* gath() const { return buf[LANE_GATH].as<uint64_t>(); }
  uint64_t* slot(uint32_t g, size_t slot_words) const { return gath() + (size_t)g * slot_words; }
};

// The handle's scratch on the root device.
enum RootBuf {
  ROOT_HQ, ROOT_OUT, ROOT_OCNT, ROOT_OSTATS,   // host-pointer API: staged queries, merged rows, counts, statistics
  // VC_FLAG_GLOBAL_STOP: round lists + counters + floors (GsRoundLists), gathered queries, merged rows / counts / statistics
  // of a round, the union scan's per-query words and the shards' tie ids (GsScanBlock, gs_root_block)
  GS_LISTS, GS_Q, GS_ROWS, GS_CNT, GS_ST, GS_SCAN,
  GA_LISTS,   // VC_FLAG_GLOBAL_APPROX: the open lists and counters of its rounds (GaRoundLists); gathered queries and a round's merged rows in GS_Q .. GS_ST
  // the scratch of the drivers shared with the single engine, on the root device: SCRATCH + a VcScratch (vc_internal.hpp)
  SCRATCH, SCRATCH_LAST = SCRATCH + VC_SCRATCH_BUFS - 1,
  ROOT_BUFS
};

// vc_sharded_search_radius_dev, per shard: its flat results and its nq + 1 offsets on the shard's own device; for a shard of
// another device also the root's copies of both (a shard of the root device is read where it lies).
struct RadiusShardBufs {
  DevBuf res, offs;             // on the shard's device
  DevBuf root_res, root_offs;   // on the root device (remote shards only)
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
  DevBuf buf[ROOT_BUFS];                // see RootBuf
  std::vector<RadiusShardBufs> rad;     // see RadiusShardBufs
  VcKnobs knobs;                // the handle's own developer knobs: gs_cap (first round's cap), gs_trace
  RcclApi rccl;
  std::vector<ncclComm_t> comms;
  uint32_t exchange = VC_EXCHANGE_PEER_COPY;   // what is in use
  std::string err;
  Lane& root_lane_ref() { return lanes[root_lane]; }
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

// b of at least `need` bytes on the current device, the handle keeping the text of a failure
static int grow(vc_sharded* h, DevBuf& b, size_t need) {
  VS_HIP(h, b.regrow(need));
  return VC_OK;
}

// Temporaries of one call on one device, released on every way out (the caller keeps that device current until then).
template <size_t N>
struct ScopedBufs {
  DevBuf b[N];
  ~ScopedBufs() { for (DevBuf& x : b) x.release(); }
};

static uint32_t shard_of(const vc_sharded* h, uint64_t pos) {   // pos relative to id_base, < capacity
  uint32_t g = (uint32_t)std::min<uint64_t>(h->G - 1, pos * h->G / std::max<uint64_t>(h->capacity, 1));
  while (g + 1 < h->G && pos >= h->hi[g]) ++g;
  while (g > 0 && pos < h->lo[g]) --g;
  return g;
}

static uint64_t shard_size(const vc_sharded* h, uint32_t g) {   // records shard g holds (ingest fills the id ranges in order)
  return h->n <= h->lo[g] ? 0 : std::min(h->n, h->hi[g]) - h->lo[g];
}

// the stream of a device-pointer call
static hipStream_t sharded_caller_stream(const vc_sharded* h, void* stream) { return stream == VC_STREAM_OWN ? h->root_stream : (hipStream_t)stream; }

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
    for (DevBuf& b : l.buf) b.release();
    if (l.done) (void)hipEventDestroy(l.done);
    if (l.stream) (void)hipStreamDestroy(l.stream);
  }
  for (uint32_t g = 0; g < h->rad.size(); ++g) {
    if (!h->rad[g].res.p && !h->rad[g].offs.p) continue;   // (a handle whose creation failed may name a device that does not exist)
    (void)hipSetDevice(h->dev[g]);
    h->rad[g].res.release();
    h->rad[g].offs.release();
  }
  for (vc_engine* e : h->eng) vc_destroy(e);
  (void)hipSetDevice(h->root);
  for (DevBuf& b : h->buf) b.release();
  for (RadiusShardBufs& b : h->rad) { b.root_res.release(); b.root_offs.release(); }
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
  if (cfg->engine.flags & VC_FLAG_GLOBAL_APPROX) {   // the union's approximate loop: shards and union must issue the same gets
    if (cfg->engine.n_tables == 0) return sfail(nullptr, VC_ERR_INVALID, "VC_FLAG_GLOBAL_APPROX needs an MIH index (n_tables > 0)");
    if (cfg->engine.flags & VC_FLAG_USE_BITMAP)
      return sfail(nullptr, VC_ERR_INVALID, "VC_FLAG_GLOBAL_APPROX: the statistics of VC_FLAG_USE_BITMAP would need the union's bitmap");
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
  h->rad.resize(h->G);
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

// Appended ids fill the id-range shards in order, so an update touches the shard the store ended in and the ones after it: every
// other shard's index is current and its vc_update_index does nothing.  A shard reached for the first time has no index and builds
// one.  Nothing on the root depends on the store's size between calls (shard_size reads h->n), so there is nothing else to refresh.
int vc_sharded_update_index(vc_sharded* h) {
  if (!h) return VC_ERR_INVALID;
  for (uint32_t g = 0; g < h->G; ++g) {
    if (shard_size(h, g) == 0) continue;
    int rc = vc_update_index(h->eng[g]);
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

}  // extern "C"

// ---- a batch -------------------------------------------------------------------------------------------------
// (C++ from here to the entry points at the end; the kernels keep their C names, which profiles and traces carry)
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
extern "C" __global__ void vc_sharded_stats_kernel(const uint64_t* __restrict__ base, uint64_t slot_words, uint64_t stats_off, uint32_t G, uint32_t nq,
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

// A caller that passes no count buffer gets the handle's own (the root device is current).
static int counts_or_own(vc_sharded* h, uint32_t nq, uint32_t** d_counts) {
  if (*d_counts) return VC_OK;
  if (int rc = grow(h, h->buf[ROOT_OCNT], (size_t)nq * 4)) return rc;
  *d_counts = h->buf[ROOT_OCNT].as<uint32_t>();
  return VC_OK;
}

// The queries of a batch reach every device once: an event on the caller's stream, a peer copy per remote lane into its LANE_Q
// buffer (grown by the caller).
static int send_queries_to_lanes(vc_sharded* h, const void* d_queries, size_t qbytes, hipStream_t S) {
  if (h->lanes.size() <= 1) return VC_OK;
  VS_HIP(h, hipSetDevice(h->root));
  VS_HIP(h, hipEventRecord(h->ev_q, S));
  for (uint32_t li = 0; li < h->lanes.size(); ++li) {
    if (li == h->root_lane) continue;
    Lane& l = h->lanes[li];
    VS_HIP(h, hipSetDevice(l.dev));
    VS_HIP(h, hipStreamWaitEvent(l.stream, h->ev_q, 0));   // also orders the lane behind the previous batch's copies out of its buffers
    VS_HIP(h, hipMemcpyPeerAsync(l.buf[LANE_Q].p, l.dev, d_queries, h->root, qbytes, l.stream));
  }
  return VC_OK;
}

// One batch through the shards, and its steps in the order sharded_search_dev takes them.
// Everything of a batch is enqueued, nothing is waited for (LINEAR; the MIH modes make the host wait inside each shard's
// vc_search_knn_dev -- how many queries continue decides what is enqueued next -- which is why lanes of different devices
// then run on host threads): queries, rows, counts and statistics live in HBM on the root device, valid in `S` order.
// r_cap != VC_NO_CAP (the MIH modes): every shard runs capped at that shell (vc_engine_knn_capped, in `mode`), the round of the
// global stop and of the global approximate stop; the slots stay in the root lane's gather buffer for their settle kernels.
#define VC_NO_CAP 0xFFFFFFFFu
struct ShardBatch {
  vc_sharded* h;
  const void* d_queries;
  uint32_t nq, k, mode;
  uint64_t* d_out;
  uint32_t* d_counts;
  vc_query_stats* d_stats;
  hipStream_t S;
  uint32_t r_cap;
  SlotLayout L;
  size_t qbytes;
  std::vector<int> lane_rc;             // run_lane: the first failure of every lane, reported by run_lanes
  std::vector<std::string> lane_err;

  // every lane's gather buffer and query copy, the count buffer
  int prepare_lanes() {
    int rc;
    for (uint32_t li = 0; li < h->lanes.size(); ++li) {
      Lane& l = h->lanes[li];
      const bool everything = li == h->root_lane || h->exchange == VC_EXCHANGE_RCCL;   // gathered results of all shards land here
      VS_HIP(h, hipSetDevice(l.dev));
      if ((rc = grow(h, l.buf[LANE_GATH], L.words * 8 * (everything ? h->G : l.shards.back() + 1)))) return rc;
      if (li != h->root_lane && (rc = grow(h, l.buf[LANE_Q], qbytes))) return rc;
    }
    if (!d_counts) {
      VS_HIP(h, hipSetDevice(h->root));
      if ((rc = counts_or_own(h, nq, &d_counts))) return rc;
    }
    return VC_OK;
  }

  // the queries reach every device once: an event on the caller's stream, a peer copy per remote lane
  int send_queries() { return send_queries_to_lanes(h, d_queries, qbytes, S); }

  // the shards of one device answer the batch for their id ranges, one after the other (on a host thread of its own in the
  // MIH modes: binds the lane's device for that thread, touches only the lane's lane_rc / lane_err)
  void run_lane(uint32_t li) {
    Lane& l = h->lanes[li];
    const bool is_root = li == h->root_lane;
    hipStream_t ls = is_root ? S : l.stream;
    const void* q = is_root ? d_queries : l.q();
    auto hip = [&](hipError_t r, const char* what) {
      if (r != hipSuccess && lane_rc[li] == VC_OK) { lane_rc[li] = VC_ERR_HIP; lane_err[li] = std::string(what) + ": " + hipGetErrorString(r); }
      return r == hipSuccess;
    };
    if (!hip(hipSetDevice(l.dev), "hipSetDevice")) return;
    for (uint32_t g : l.shards) {
      uint64_t* slot = l.slot(g, L.words);
      if (shard_size(h, g) == 0) {
        // an empty shard (a store filled below its capacity) contributes INF rows, zero counts, zero statistics; its engine
        // is never asked -- an exact radius loop over nothing would walk every shell of every table (search_worker.cc:170)
        if (!hip(hipMemsetAsync(slot, 0xFF, L.rows * 8, ls), "hipMemsetAsync") ||
            !hip(hipMemsetAsync(slot + L.cnt_off, 0, (L.words - L.cnt_off) * 8, ls), "hipMemsetAsync")) return;
        continue;
      }
      vc_query_stats* sst = d_stats ? (vc_query_stats*)(slot + L.stats_off) : nullptr;
      const int r = r_cap != VC_NO_CAP ? vc_engine_knn_capped(h->eng[g], q, nq, k, mode, r_cap, slot, (uint32_t*)(slot + L.cnt_off), sst, ls)
                                       : vc_search_knn_dev_stats(h->eng[g], q, nq, k, mode, slot, (uint32_t*)(slot + L.cnt_off), sst, ls);
      if (r != VC_OK) { lane_rc[li] = r; lane_err[li] = std::string("shard ") + std::to_string(g) + ": " + vc_last_error(h->eng[g]); return; }
    }
    if (!is_root) hip(hipEventRecord(l.done, ls), "hipEventRecord");
  }

  // every lane: in turn where nothing waits (LINEAR) or there is one lane, else concurrently
  int run_lanes() {
    lane_rc.assign(h->lanes.size(), VC_OK);
    lane_err.assign(h->lanes.size(), std::string());
    if (mode == VC_MODE_LINEAR || h->lanes.size() == 1) {
      for (uint32_t li = 0; li < h->lanes.size(); ++li) run_lane(li);
    } else {
      std::vector<std::thread> th;
      for (uint32_t li = 0; li < h->lanes.size(); ++li) th.emplace_back([this, li] { run_lane(li); });
      for (auto& t : th) t.join();
    }
    for (uint32_t li = 0; li < h->lanes.size(); ++li)
      if (lane_rc[li]) return sfail(h, lane_rc[li], "%s", lane_err[li].c_str());
    return VC_OK;
  }

  // ONE exchange (replaces gather_vectors, mpi_coordinator.cc:34-69): every shard's slot -> the root's gather buffer
  int exchange() {
    Lane& R = h->root_lane_ref();
    if (h->exchange == VC_EXCHANGE_RCCL) {
      ncclResult_t nr = h->rccl.GroupStart();
      for (uint32_t g = 0; g < h->G && nr == ncclSuccess; ++g) {   // rank g = shard g = its device's lane; in place: the send slot sits in the receive buffer
        Lane& l = h->lanes[h->lane_of[g]];
        nr = h->rccl.AllGather(l.slot(g, L.words), l.gath(), L.words, ncclUint64, h->comms[g], h->lane_of[g] == h->root_lane ? S : l.stream);
      }
      const ncclResult_t ne = h->rccl.GroupEnd();
      if (nr == ncclSuccess) nr = ne;
      if (nr != ncclSuccess) return sfail(h, VC_ERR_HIP, "ncclAllGather: %s", h->rccl.GetErrorString(nr));
      return VC_OK;
    }
    VS_HIP(h, hipSetDevice(h->root));
    for (uint32_t li = 0; li < h->lanes.size(); ++li) {
      if (li == h->root_lane) continue;      // the root's shards wrote their slots in place
      Lane& l = h->lanes[li];
      VS_HIP(h, hipStreamWaitEvent(S, l.done, 0));
      for (uint32_t g : l.shards)
        VS_HIP(h, hipMemcpyPeerAsync(R.slot(g, L.words), h->root, l.slot(g, L.words), l.dev, L.words * 8, S));
    }
    return VC_OK;
  }

  // merge (replaces the master's heap, search_worker.cc:179-199); a flagged shard row flags the merged row.
  // Returns with the root device current.
  int merge() {
    Lane& R = h->root_lane_ref();
    VS_HIP(h, hipSetDevice(h->root));
    VS_HIP(h, vc_launch_select_slots(R.gath(), L.words, (uint32_t)L.cnt_off, h->G, nq, k, d_out, d_counts, S));
    if (d_stats) {
      hipLaunchKernelGGL(vc_sharded_stats_kernel, dim3((nq + 255) / 256), dim3(256), 0, S, (const uint64_t*)R.gath(), (uint64_t)L.words,
                         (uint64_t)L.stats_off, h->G, nq, (const uint32_t*)d_counts, d_stats);
      VS_HIP(h, hipGetLastError());
    }
    return VC_OK;
  }
};

// Any device may be current on entry; the root device is on a successful return.
static int sharded_search_dev(vc_sharded* h, const void* d_queries, uint32_t nq, uint32_t k, uint32_t mode, uint64_t* d_out,
                              uint32_t* d_counts, vc_query_stats* d_stats, hipStream_t S, uint32_t r_cap = VC_NO_CAP) {
  ShardBatch b{h, d_queries, nq, k, mode, d_out, d_counts, d_stats, S, r_cap, SlotLayout(nq, k, d_stats != nullptr), (size_t)nq * h->nbytes, {}, {}};
  int rc = b.prepare_lanes();
  if (!rc) rc = b.send_queries();
  if (!rc) rc = b.run_lanes();
  if (!rc) rc = b.exchange();
  if (!rc) rc = b.merge();
  return rc;
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
//     r0 - 1 (then R = r0 - 1 iff shell r0 - 1 holds k items at or below D*: mih_replay_kernel's rule), else at r0
//     (gs_stop_shell);
//   * no shard stops before R (its local k-th distance is never below the union's), so in a round capped at t = R every shard
//     ends at e_g = R: the merged rows are the union loop's rows at R and the shards' candidate counts add up to its count.
// A query is settled when its round ended every shard in the shell R requires; otherwise the kernel files it under the cap
// the next round needs.  Queries that need a shell beyond the shards' in-block reach (far or uniform queries) go to the
// union scan: LINEAR over the shards gives D* and the rows, mih_tie_collect_kernel decides the tie at the threshold and
// vc_launch_minsub_count counts the candidates -- the union-wide counterpart of the single engine's scan + replay.
// The host side is GsSearch below: sharded_global_stop() shows the rounds, GsSearch::union_scan() the scan.
#define GS_CAPS 17u   // caps 0..16 (inblock_last_shell never goes beyond 16)

__device__ __forceinline__ unsigned long long gs_leaves(uint32_t S, uint32_t R) {   // table 0's gets of shells 0..R: sum of C(S, r)
  unsigned long long c = 1, sum = 0;
  for (uint32_t r = 0; r <= R && r <= S; ++r) {
    sum += c;
    c = c * (S - r) / (r + 1);
  }
  return sum;
}

// Where the union's radius loop stops once its k-th distance is D (m tables of S-bit substrings, stop multiplier mult): the
// loop leaves shell r when D <= mult (r + 1) (search_worker.cc:201-205), i.e. in shell rs = ceil(D / mult) - 1, its last
// shell at the latest.  `tie`: D sits exactly on the threshold of shell rs + 1 while the pigeonhole bound of shell rs is the
// same D (mult == m), so shell rs stops the loop only if it already holds k items at or below D, else shell rs + 1 does.
// mih_replay_kernel (vc_mih.hip) states the same rule for the single engine's scan; the two must agree.
struct GsStopShell {
  uint32_t rs;
  bool tie;
};
__device__ __forceinline__ GsStopShell gs_stop_shell(uint32_t D, uint32_t m, uint32_t S, uint32_t mult) {
  return {min(S, D == 0 ? 0u : (D + mult - 1) / mult - 1), mult == m && D != 0 && D % m == 0};
}

extern "C" __global__ void __launch_bounds__(256) gs_iota_kernel(uint32_t* __restrict__ p, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = i;
}

// Queries per cap: what gs_settle_kernel counts into the next round's lists, and what the host reads back after a round.
struct GsCapCounters {
  uint32_t at_cap[GS_CAPS];
};
#define GS_CTR_SLOT_WORDS 32u   // words a counter block occupies in the buffer
static_assert(sizeof(GsCapCounters) == GS_CAPS * 4 && sizeof(GsCapCounters) <= GS_CTR_SLOT_WORDS * 4,
              "gs_settle_kernel indexes next_ctr[cap], cap <= reach < GS_CAPS; a block fits its slot");

// vc_sharded::buf[GS_LISTS] of one call: list[0] | list[1] | ctr[0] | ctr[1] | scan_ctr | scan[nq] | floor_[nq].
// list[i] is [GS_CAPS][nq]: under cap t the queries whose next round is capped at shell t, ctr[i]->at_cap[t] of them.  One
// set is the round that runs, the other is filled by its settle kernels; the sets swap after a round.
struct GsRoundLists {
  uint32_t* list[2];
  GsCapCounters* ctr[2];
  uint32_t* scan_ctr;   // entries of scan
  uint32_t* scan;       // the queries for the union scan
  uint32_t* floor_;     // per query: the union loop cannot stop below this shell
  uint32_t nq;
  static size_t words(uint32_t nq) { return 2 * (size_t)GS_CAPS * nq + 3 * (size_t)GS_CTR_SLOT_WORDS + 2 * (size_t)nq; }
  static GsRoundLists carve(uint32_t* base, uint32_t nq) {
    GsRoundLists ls{};
    ls.nq = nq;
    for (uint32_t*& l : ls.list) { l = base; base += (size_t)GS_CAPS * nq; }
    for (GsCapCounters*& c : ls.ctr) { c = (GsCapCounters*)base; base += GS_CTR_SLOT_WORDS; }
    ls.scan_ctr = base; base += GS_CTR_SLOT_WORDS;
    ls.scan = base; base += nq;
    ls.floor_ = base;
    return ls;
  }
  uint32_t* of_cap(int set, uint32_t t) const { return list[set] + (size_t)t * nq; }
};

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

extern "C" __global__ void __launch_bounds__(256) gs_settle_kernel(const GsSettleArgs a) {
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
    const GsStopShell stop = gs_stop_shell(D, a.m, a.S, a.mult);
    const uint32_t want = (stop.tie && flo > stop.rs) ? stop.rs + 1 : stop.rs;
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

// The union scan's per-query words ("sd"): six columns of nq words each, in this order, row j = the j-th query of the scan
// list.  Written by gs_scan_plan_kernel on the root, copied to every lane, read there by the tie collection and the count.
template <class Word>
struct GsScanCols {
  Word* dist;     // D where the tie at the threshold is open (need > 0), else 0: vc_launch_tie_collect's d_dist
  Word* radius;   // the shell rs whose ties decide (vc_launch_tie_collect's d_radius)
  Word* need;     // how many ties of shell rs complete the k rows; 0: nothing to decide
  Word* R;        // the shell the union loop stops in (vc_launch_minsub_count's d_radius; the final statistics)
  Word* iota;     // j: vc_launch_minsub_count's query list
  Word* ones;     // 1: vc_launch_minsub_count's flags
  static __host__ __device__ size_t words(uint32_t nq) { return sizeof(GsScanCols) / sizeof(Word*) * (size_t)nq; }
  static __host__ __device__ GsScanCols carve(Word* base, uint32_t nq) {
    GsScanCols c;
    for (Word** col : {&c.dist, &c.radius, &c.need, &c.R, &c.iota, &c.ones}) { *col = base; base += nq; }
    return c;
  }
};
using GsScanWords = GsScanCols<uint32_t>;
using GsScanWordsIn = GsScanCols<const uint32_t>;

// union scan, step 1: the rule applied to the LINEAR rows
extern "C" __global__ void __launch_bounds__(256) gs_scan_plan_kernel(uint32_t n, uint32_t k, uint32_t m, uint32_t S, uint32_t mult,
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
    const GsStopShell stop = gs_stop_shell(D, m, S, mult);
    R = stop.rs;
    if (stop.tie) {
      if (floor_[list[j]] > stop.rs) {
        R = stop.rs + 1;
      } else {                                       // does shell rs = D/m - 1 already hold k items at or below D?
        uint32_t below = 0;
        while (below < k && (uint32_t)(row[below] >> 32) < D) ++below;
        dist = D;
        rad = stop.rs;
        need = k - below;
      }
    }
  }
  const GsScanWords w = GsScanWords::carve(sd, nq);
  w.dist[j] = dist;
  w.radius[j] = rad;
  w.need[j] = need;
  w.R[j] = R;
  w.iota[j] = j;
  w.ones[j] = 1;
}

// union scan, step 2: the shards' ties (ids ascending within a shard, shards in id order) decide the tie at the threshold
extern "C" __global__ void __launch_bounds__(256) gs_scan_tie_kernel(uint32_t n, uint32_t k, uint32_t G, uint32_t* __restrict__ sd, uint32_t nq,
                                                          const uint32_t* __restrict__ tie_ids, const uint32_t* __restrict__ tie_cnt,
                                                          uint64_t* __restrict__ rows) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const GsScanWords w = GsScanWords::carve(sd, nq);
  const uint32_t need = w.need[j], rs = w.radius[j], D = w.dist[j];
  if (need == 0) return;
  uint32_t total = 0;
  for (uint32_t g = 0; g < G; ++g) total += tie_cnt[(size_t)g * nq + j];
  if (total < need) {
    w.R[j] = rs + 1;                                 // shell rs has too few: the loop stops at D/m with the scan's rows
    return;
  }
  uint32_t wr = k - need;                            // the rows below D stay; the ties of shell rs follow, smallest ids first
  for (uint32_t g = 0; g < G && wr < k; ++g)
    for (uint32_t i = 0; i < tie_cnt[(size_t)g * nq + j] && wr < k; ++i)
      rows[(uint64_t)j * k + wr++] = ((uint64_t)D << 32) | tie_ids[((size_t)g * nq + j) * k + i];
  w.R[j] = rs;
}

// union scan, step 3: rows, counts and the statistics of one SearchWorker stopping at R
extern "C" __global__ void __launch_bounds__(256) gs_scan_final_kernel(uint32_t n, uint32_t k, uint32_t S, const uint32_t* __restrict__ list,
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
    const uint32_t R = GsScanWordsIn::carve(sd, nq).R[j];
    vc_query_stats s{};
    s.radius = R;
    s.n_results = cnt[j];
    s.n_sub_reads = gs_leaves(S, R);
    for (uint32_t l = 0; l < n_lanes; ++l) s.n_candidates += seen[(size_t)l * nq + j];
    out_stats[q] = s;
  }
}

// The union scan's words on one device: seen | sd | tie_cnt | tie_ids | chunk_scratch, everything nq apart per row so that
// what crosses devices is a run of n <= nq words.  Two shapes of the one layout:
//   the root (gs_root_block, vc_sharded::buf[GS_SCAN]): a seen row per LANE, tie counts / ids per shard of the store, no scratch;
//   a lane (gs_lane_block, Lane::buf[LANE_AUX]):        one seen row, tie counts / ids per shard of the LANE, the tie kernel's scratch.
struct GsScanBlock {
  unsigned long long* seen;   // [seen_rows][nq] candidates of the union loop up to R (vc_launch_minsub_count)
  uint32_t* sd;               // GsScanCols
  uint32_t* tie_cnt;          // [shards][nq]
  uint32_t* tie_ids;          // [shards][nq][k]
  uint32_t* chunk_scratch;    // [nq][VC_TIE_CHUNKS] (lanes only, else null)
  uint32_t nq, k;
  unsigned long long* seen_of(uint32_t row) const { return seen + (size_t)row * nq; }
  uint32_t* cnt_of(size_t shard) const { return tie_cnt + shard * nq; }
  uint32_t* ids_of(size_t shard) const { return tie_ids + shard * nq * k; }
  static size_t words(size_t seen_rows, size_t shards, uint32_t nq, uint32_t k, bool scratch) {
    return seen_rows * nq * (sizeof(unsigned long long) / 4) + GsScanWords::words(nq) + shards * nq + shards * nq * k +
           (scratch ? (size_t)nq * VC_TIE_CHUNKS : 0);
  }
  static GsScanBlock carve(uint32_t* base, size_t seen_rows, size_t shards, uint32_t nq, uint32_t k, bool scratch) {
    GsScanBlock b{};
    b.nq = nq;
    b.k = k;
    b.seen = (unsigned long long*)base; base += seen_rows * nq * (sizeof(unsigned long long) / 4);
    b.sd = base;                        base += GsScanWords::words(nq);
    b.tie_cnt = base;                   base += shards * nq;
    b.tie_ids = base;                   base += shards * nq * k;
    b.chunk_scratch = scratch ? base : nullptr;
    return b;
  }
};
// (the owning device is current: the buffer may grow)
static int gs_root_block(vc_sharded* h, uint32_t nq, uint32_t k, GsScanBlock* out) {
  if (int rc = grow(h, h->buf[GS_SCAN], GsScanBlock::words(h->lanes.size(), h->G, nq, k, false) * 4)) return rc;
  *out = GsScanBlock::carve(h->buf[GS_SCAN].as<uint32_t>(), h->lanes.size(), h->G, nq, k, false);
  return VC_OK;
}
static int gs_lane_block(vc_sharded* h, Lane& l, uint32_t nq, uint32_t k, GsScanBlock* out) {
  if (int rc = grow(h, l.buf[LANE_AUX], GsScanBlock::words(1, l.shards.size(), nq, k, true) * 4)) return rc;
  *out = GsScanBlock::carve(l.buf[LANE_AUX].as<uint32_t>(), 1, l.shards.size(), nq, k, true);
  return VC_OK;
}

#define GS_MAX_ROUNDS 8u   // the rounds settle a query in at most four: the first cap, the pigeonhole cap, R, and R + 1 after a tie; 8 is a bound

// One flagged call: what is fixed for it, and its steps in the order sharded_global_stop() and union_scan() take them.
// Current device: every step is entered and left with the ROOT device current (prepare() binds it; sharded_search_dev and
// over_lanes, the two that bind others, return with it).
struct GsSearch {
  vc_sharded* h;
  const void* d_queries;
  uint32_t nq, k;
  uint64_t* d_out;
  uint32_t* d_counts;
  vc_query_stats* d_stats;
  hipStream_t S;
  // ---- fixed by prepare()
  uint32_t W, m, Sb, mult;
  uint32_t nonempty;                 // bit g: shard g holds records
  uint32_t reach;                    // last shell every non-empty shard's query kernel reaches: the largest cap of a round
  bool trace;                        // dev (VC_MIH_GS_TRACE): per-round wall times on stderr
  std::vector<VcEngineView> view;
  GsRoundLists ls;
  uint64_t* gs_q;                    // the gathered queries of a cap group / of the union scan
  uint64_t* rows;                    // their merged rows, counts, statistics
  uint32_t* cnt;
  vc_query_stats* st;
  // ---- the rounds
  int cur;                           // the list set of the round that runs
  GsCapCounters todo;                // queries per cap of the coming round
  uint32_t n_scan;                   // queries of the union scan so far
  GsScanBlock rb;                    // the root's union-scan words (union_scan)

  int prepare() {
    W = h->nbytes / 8; m = h->cfg.engine.n_tables; Sb = h->cfg.engine.bits / m;
    mult = (h->cfg.engine.flags & VC_FLAG_REF_STOP_LITERAL4) ? 4u : std::min(m, 4u);
    trace = h->knobs.gs_trace;
    nonempty = 0; reach = GS_CAPS - 1;
    view.resize(h->G);
    for (uint32_t g = 0; g < h->G; ++g) {
      vc_engine_view(h->eng[g], &view[g]);
      if (shard_size(h, g) == 0) continue;
      nonempty |= 1u << g;
      reach = std::min(reach, view[g].reach);
    }
    int rc;
    VS_HIP(h, hipSetDevice(h->root));
    if ((rc = counts_or_own(h, nq, &d_counts))) return rc;
    if ((rc = grow(h, h->buf[GS_LISTS], GsRoundLists::words(nq) * 4))) return rc;
    if ((rc = grow(h, h->buf[GS_Q], (size_t)nq * h->nbytes))) return rc;
    if ((rc = grow(h, h->buf[GS_ROWS], (size_t)nq * k * 8))) return rc;
    if ((rc = grow(h, h->buf[GS_CNT], (size_t)nq * 4))) return rc;
    if ((rc = grow(h, h->buf[GS_ST], (size_t)nq * sizeof(vc_query_stats)))) return rc;
    ls = GsRoundLists::carve(h->buf[GS_LISTS].as<uint32_t>(), nq);
    gs_q = h->buf[GS_Q].as<uint64_t>();
    rows = h->buf[GS_ROWS].as<uint64_t>();
    cnt = h->buf[GS_CNT].as<uint32_t>();
    st = h->buf[GS_ST].as<vc_query_stats>();
    cur = 0; todo = GsCapCounters{}; n_scan = 0;
    VS_HIP(h, hipMemsetAsync(ls.floor_, 0, (size_t)nq * 4, S));
    VS_HIP(h, hipMemsetAsync(ls.scan_ctr, 0, 4, S));
    return VC_OK;
  }

  // every query starts under the first round's cap (VC_MIH_GS_CAP, within the shards' reach) -- or, with nothing to probe, in
  // the union scan, which reports the empty union (R = last shell, no candidates)
  int seed_first_round() {
    const uint32_t t0 = std::min(h->knobs.gs_cap, reach);
    hipLaunchKernelGGL(gs_iota_kernel, dim3((nq + 255) / 256), dim3(256), 0, S, nonempty == 0 ? ls.scan : ls.of_cap(0, t0), nq);
    VS_HIP(h, hipGetLastError());
    if (nonempty == 0) n_scan = nq;
    else todo.at_cap[t0] = nq;
    return VC_OK;
  }

  bool round_open() const {
    for (uint32_t n : todo.at_cap)
      if (n) return true;
    return false;
  }

  GsSettleArgs settle_args(uint32_t t, uint32_t n, const uint32_t* list) const {   // after the cap group's search: it may grow the slots
    const SlotLayout L(n, k, true);
    GsSettleArgs a{};
    a.base = h->root_lane_ref().gath(); a.slot_words = L.words; a.stats_off = L.stats_off; a.G = h->G; a.nonempty = nonempty;
    a.n = n; a.t = t; a.k = k; a.m = m; a.S = Sb; a.mult = mult; a.reach = reach; a.nq = nq;
    a.list = list; a.rows = rows; a.cnt = cnt; a.floor_ = ls.floor_;
    a.out = d_out; a.out_cnt = d_counts; a.out_stats = d_stats;
    a.next = ls.list[cur ^ 1]; a.next_ctr = ls.ctr[cur ^ 1]->at_cap; a.scan = ls.scan; a.scan_ctr = ls.scan_ctr;
    return a;
  }

  // one round: per cap with queries, gather them, run every shard capped at that shell, merge, and let the settle kernel
  // finish them or file them in the other list set.  (The host waits inside each shard's capped search, not here.)
  int run_round() {
    int rc;
    VS_HIP(h, hipMemsetAsync(ls.ctr[cur ^ 1], 0, sizeof(GsCapCounters), S));
    for (uint32_t t = 0; t < GS_CAPS; ++t) {
      const uint32_t n = todo.at_cap[t];
      if (!n) continue;
      const uint32_t* list = ls.of_cap(cur, t);
      VS_HIP(h, vc_launch_gather_queries((const uint64_t*)d_queries, list, n, W, gs_q, S));
      if ((rc = sharded_search_dev(h, gs_q, n, k, VC_MODE_MIH_EXACT, rows, cnt, st, S, t))) return rc;
      hipLaunchKernelGGL(gs_settle_kernel, dim3((n + 255) / 256), dim3(256), 0, S, settle_args(t, n, list));
      VS_HIP(h, hipGetLastError());
    }
    cur ^= 1;
    return VC_OK;
  }

  // the round ends: the host waits for its counters -- what stays open per cap (the coming round) and the union scan's total
  int read_round_counters(uint32_t round, std::chrono::steady_clock::time_point t_round) {
    GsCapCounters open;
    uint32_t open_scan;
    VS_HIP(h, hipMemcpyAsync(&open, ls.ctr[cur], sizeof(GsCapCounters), hipMemcpyDeviceToHost, S));
    VS_HIP(h, hipMemcpyAsync(&open_scan, ls.scan_ctr, 4, hipMemcpyDeviceToHost, S));
    VS_HIP(h, hipStreamSynchronize(S));
    if (trace) {
      fprintf(stderr, "[vc_gs] round %u:", round);
      for (uint32_t t = 0; t < GS_CAPS; ++t) if (todo.at_cap[t]) fprintf(stderr, " cap %u x %u", t, todo.at_cap[t]);
      fprintf(stderr, " -> open");
      for (uint32_t t = 0; t < GS_CAPS; ++t) if (open.at_cap[t]) fprintf(stderr, " cap %u x %u", t, open.at_cap[t]);
      fprintf(stderr, ", union scan %u  %.1f us\n", open_scan,
              std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_round).count());
    }
    todo = open;
    n_scan = open_scan;
    return VC_OK;
  }

  // what the last round left open joins the union scan's list
  int leftovers_to_scan() {
    for (uint32_t t = 0; t < GS_CAPS; ++t)
      if (todo.at_cap[t]) {
        VS_HIP(h, hipMemcpyAsync(ls.scan + n_scan, ls.of_cap(cur, t), (size_t)todo.at_cap[t] * 4, hipMemcpyDeviceToDevice, S));
        n_scan += todo.at_cap[t];
      }
    return VC_OK;
  }

  // ---- the union scan over the n_scan queries of ls.scan
  // LINEAR over the shards gives the rows and D*; the rule gives R, or leaves the tie at the threshold open
  int scan_plan() {
    int rc;
    const uint32_t n = n_scan;
    if ((rc = gs_root_block(h, nq, k, &rb))) return rc;
    VS_HIP(h, vc_launch_gather_queries((const uint64_t*)d_queries, ls.scan, n, W, gs_q, S));
    if ((rc = sharded_search_dev(h, gs_q, n, k, VC_MODE_LINEAR, rows, cnt, nullptr, S))) return rc;
    hipLaunchKernelGGL(gs_scan_plan_kernel, dim3((n + 255) / 256), dim3(256), 0, S, n, k, m, Sb, mult, (const uint32_t*)ls.scan,
                       (const uint32_t*)ls.floor_, (const uint64_t*)rows, (const uint32_t*)cnt, rb.sd, nq);
    VS_HIP(h, hipGetLastError());
    return VC_OK;
  }

  // One pass over the lanes, in lane order: the per-query words (rb.sd) go out to the lane's block, fn enqueues the lane's
  // shards on the lane's stream and the copies of their results into rb, the root's stream waits for the lane.
  // Entered and left with the root device current (inside, the lane's device is, for fn too).  Order: a remote lane starts
  // behind everything enqueued on S so far (ev_q) and S continues behind the lane's last copy (Lane::done); the root lane
  // runs on S itself.  The queries are where the scan's LINEAR search left them: gs_q on the root, Lane::q() elsewhere.
  template <class Fn>
  int over_lanes(Fn&& fn) {
    int rc;
    for (uint32_t li = 0; li < h->lanes.size(); ++li) {
      Lane& l = h->lanes[li];
      const bool is_root = li == h->root_lane;
      hipStream_t lstream = is_root ? S : l.stream;
      if (!is_root) VS_HIP(h, hipEventRecord(h->ev_q, S));
      VS_HIP(h, hipSetDevice(l.dev));
      GsScanBlock lb;
      if ((rc = gs_lane_block(h, l, nq, k, &lb))) return rc;
      if (!is_root) VS_HIP(h, hipStreamWaitEvent(lstream, h->ev_q, 0));
      VS_HIP(h, hipMemcpyPeerAsync(lb.sd, l.dev, rb.sd, h->root, GsScanWords::words(nq) * 4, lstream));
      const uint64_t* lq = is_root ? gs_q : (const uint64_t*)l.q();
      if ((rc = fn(li, l, lb, lstream, lq))) return rc;
      if (!is_root) {
        VS_HIP(h, hipEventRecord(l.done, lstream));
        VS_HIP(h, hipSetDevice(h->root));
        VS_HIP(h, hipStreamWaitEvent(S, l.done, 0));
      }
    }
    return VC_OK;
  }

  // the tie at the threshold: every shard's smallest-id ties whose substrings reach below D/m, to the root by shard
  int collect_ties() {
    const uint32_t n = n_scan;
    return over_lanes([&](uint32_t, Lane& l, const GsScanBlock& lb, hipStream_t lstream, const uint64_t* lq) -> int {
      const GsScanWordsIn sd = GsScanWordsIn::carve(lb.sd, nq);
      for (size_t i = 0; i < l.shards.size(); ++i) {
        const uint32_t g = l.shards[i];
        if (!((nonempty >> g) & 1u)) {
          VS_HIP(h, hipMemsetAsync(lb.cnt_of(i), 0, (size_t)n * 4, lstream));
        } else {
          const VcEngineView& v = view[g];
          VS_HIP(h, vc_launch_tie_collect(v.cols, v.stride, v.n, W, m, Sb, v.id_base, lq, n, k, sd.dist, sd.radius, sd.need,
                                          lb.chunk_scratch, lb.ids_of(i), lb.cnt_of(i), lstream));
        }
        VS_HIP(h, hipMemcpyPeerAsync(rb.cnt_of(g), h->root, lb.cnt_of(i), l.dev, (size_t)n * 4, lstream));
        VS_HIP(h, hipMemcpyPeerAsync(rb.ids_of(g), h->root, lb.ids_of(i), l.dev, (size_t)n * k * 4, lstream));
      }
      return VC_OK;
    });
  }

  // the ties complete the rows where shell rs holds enough of them; R is final afterwards
  int apply_ties() {
    const uint32_t n = n_scan;
    hipLaunchKernelGGL(gs_scan_tie_kernel, dim3((n + 255) / 256), dim3(256), 0, S, n, k, h->G, rb.sd, nq, (const uint32_t*)rb.tie_ids,
                       (const uint32_t*)rb.tie_cnt, rows);
    VS_HIP(h, hipGetLastError());
    return VC_OK;
  }

  // the candidates of the union loop up to R: every item whose minimum substring distance is <= R, summed per lane
  int count_candidates() {
    const uint32_t n = n_scan;
    return over_lanes([&](uint32_t li, Lane& l, const GsScanBlock& lb, hipStream_t lstream, const uint64_t* lq) -> int {
      const GsScanWordsIn sd = GsScanWordsIn::carve(lb.sd, nq);
      VS_HIP(h, hipMemsetAsync(lb.seen, 0, (size_t)n * 8, lstream));
      for (uint32_t g : l.shards) {
        if (!((nonempty >> g) & 1u)) continue;
        const VcEngineView& v = view[g];
        VS_HIP(h, vc_launch_minsub_count(v.cols, v.stride, v.n, W, m, Sb, lq, sd.iota, sd.ones, n, sd.R, lb.seen, v.n_cu, lstream));
      }
      VS_HIP(h, hipMemcpyPeerAsync(rb.seen_of(li), h->root, lb.seen, l.dev, (size_t)n * 8, lstream));
      return VC_OK;
    });
  }

  // rows, counts and statistics of the scanned queries into the caller's buffers
  int scan_finish(std::chrono::steady_clock::time_point t_scan) {
    const uint32_t n = n_scan;
    hipLaunchKernelGGL(gs_scan_final_kernel, dim3((n + 255) / 256), dim3(256), 0, S, n, k, Sb, (const uint32_t*)ls.scan, (const uint32_t*)rb.sd,
                       nq, (const uint64_t*)rows, (const uint32_t*)cnt, (const unsigned long long*)rb.seen, (uint32_t)h->lanes.size(), d_out,
                       d_counts, d_stats);
    VS_HIP(h, hipGetLastError());
    if (trace) {
      VS_HIP(h, hipStreamSynchronize(S));
      fprintf(stderr, "[vc_gs] union scan: %u queries  %.1f us\n", n,
              std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_scan).count());
    }
    return VC_OK;
  }

  int union_scan() {
    const auto t_scan = std::chrono::steady_clock::now();
    int rc = scan_plan();
    if (!rc) rc = collect_ties();
    if (!rc) rc = apply_ties();
    if (!rc && d_stats) rc = count_candidates();   // (only the statistics need them)
    if (!rc) rc = scan_finish(t_scan);
    return rc;
  }
};

static int sharded_global_stop(vc_sharded* h, const void* d_queries, uint32_t nq, uint32_t k, uint64_t* d_out, uint32_t* d_counts,
                               vc_query_stats* d_stats, hipStream_t S) {
  GsSearch c{h, d_queries, nq, k, d_out, d_counts, d_stats, S};
  int rc = c.prepare();
  if (!rc) rc = c.seed_first_round();
  for (uint32_t round = 0; !rc && round < GS_MAX_ROUNDS && c.round_open(); ++round) {
    const auto t_round = std::chrono::steady_clock::now();
    rc = c.run_round();                                    // enqueued on S: every open cap group searched capped and judged
    if (!rc) rc = c.read_round_counters(round, t_round);   // the round ends here: the host waits for what it left open
  }
  if (!rc) rc = c.leftovers_to_scan();                     // (a query still open after the last round is scanned too)
  if (!rc && c.n_scan) rc = c.union_scan();                // the union scan takes over: everything the rounds could not settle
  return rc;
}

// ---- VC_FLAG_GLOBAL_APPROX ----------------------------------------------------------------------------------------------
// Approximate MIH over the shards with the stop decision of ONE SearchWorker over the union (the reference's master fills ONE
// heap of knn_ * APPROXIMATE_FACTOR distinct candidates from all ranks and broadcasts is_stop: search_worker.cc:104-139).  The
// union's loop stops after the first shell r* in which its distinct candidates of shells 0..r* reach 20 k, else after shell S.
// What the rounds rest on (c_g(r) = shard g's distinct candidates of shells 0..r, c(r) = the union's):
//   * the owner rule counts an item once and the shards hold disjoint ids, so c(r) = sum over g of c_g(r);
//   * shards and union share one key function, so table 0's gets of shells 0..r are the same number everywhere;
//   * c_g(r) <= c(r): a shard whose own rule stops it in a shell r < t proves c(r) >= 20 k.
// INVARIANT: a query is settled in a round capped at t only when c(t - 1) < 20 k is known, or t == 0.  Then no shard stops
// before t, every non-empty shard ends in shell t with the k best of its items of shells 0..t and with c_g(t), and the round's
// merged rows and summed counts are the union loop's at t: it stops there iff the sum reaches 20 k or t == S.  The schedule is
// t = 0, 1, 2, ... with every open query in every round, which keeps the invariant by construction and ends after at most S + 1
// rounds.  A shard that ended elsewhere than in t breaks the argument: ga_settle_kernel counts such shards and the call fails.
// No pigeonhole bound and no stop multiplier enter, so VC_FLAG_REF_SIGNEXT_KEYS and VC_FLAG_REF_STOP_LITERAL4 are allowed.
// The host side is GaSearch below: sharded_global_approx() shows the rounds.

// vc_sharded::buf[GA_LISTS] of one call: list[0] | list[1] | open[0] | open[1] | bad.  list[i] is [nq]: the open queries of a
// round, open[i] of them; one list is the round that runs, the other is filled by its settle kernel; they swap after a round.
struct GaCounters {
  uint32_t open[2];   // entries of list[0], list[1]
  uint32_t bad;       // shards that did not end in their round's shell (never, under the invariant)
};
struct GaRoundLists {
  uint32_t* list[2];
  GaCounters* ctr;
  static size_t words(uint32_t nq) { return 2 * (size_t)nq + GS_CTR_SLOT_WORDS; }
  static GaRoundLists carve(uint32_t* base, uint32_t nq) {
    GaRoundLists ls{};
    for (uint32_t*& l : ls.list) { l = base; base += nq; }
    ls.ctr = (GaCounters*)base;
    return ls;
  }
};
static_assert(sizeof(GaCounters) <= GS_CTR_SLOT_WORDS * 4, "the counters fit their slot");

struct GaSettleArgs {
  const uint64_t* base;          // the round's gathered slots (rows | counts | statistics per shard)
  uint64_t slot_words, stats_off;
  uint32_t G, nonempty;          // bit g: shard g holds records
  uint32_t n, t, k, S;           // n queries in a round capped at shell t; S = the last shell
  const uint32_t* list;          // [n] query of merged row j (< nq)
  const uint64_t* rows;          // [n][k] merged rows
  const uint32_t* cnt;           // [n]
  uint64_t* out;                 // final rows / counts / statistics, by query
  uint32_t* out_cnt;
  vc_query_stats* out_stats;     // may be null
  uint32_t* next;                // [nq] open list of the next round, *next_ctr entries
  uint32_t* next_ctr;
  uint32_t* bad;
};

// One wave per query of the round (GA_SETTLE_BLK / VC_WAVE queries per block): the union's candidate count at shell t is the sum
// of the shards'; at 20 k (or in the last shell) the merged row is the union loop's answer and goes to the query's own place --
// the wave's lanes copy its k entries side by side --, else the query stays open.  Every lane reads the same G statistics
// records, so the decision is uniform over the wave; lane 0 writes the words and takes the counters.
#define GA_SETTLE_BLK 256u
extern "C" __global__ void __launch_bounds__(GA_SETTLE_BLK) ga_settle_kernel(const GaSettleArgs a) {
  const uint32_t j = blockIdx.x * (GA_SETTLE_BLK / VC_WAVE) + threadIdx.x / VC_WAVE;
  if (j >= a.n) return;
  const uint32_t lane = vc_lane();
  const uint32_t q = a.list[j];
  unsigned long long seen = 0, sub = 0;
  uint32_t astray = 0;
  bool first = true;
  for (uint32_t g = 0; g < a.G; ++g) {
    if (!((a.nonempty >> g) & 1u)) continue;
    const vc_query_stats s = ((const vc_query_stats*)(a.base + (uint64_t)g * a.slot_words + a.stats_off))[j];
    seen += s.n_candidates;
    if (s.radius != a.t) ++astray;
    if (first) { sub = s.n_sub_reads; first = false; }   // table 0's gets of shells 0..t: the same on every shard
  }
  if (lane == 0 && astray) atomicAdd(a.bad, astray);
  if (seen >= (unsigned long long)a.k * MIH_APPROX_FACTOR || a.t >= a.S) {   // search_worker.cc:136-137
    const uint32_t c = min(a.cnt[j], a.k);
    const uint64_t* row = a.rows + (uint64_t)j * a.k;
    uint64_t* o = a.out + (uint64_t)q * a.k;
    for (uint32_t i = lane; i < a.k; i += VC_WAVE) o[i] = row[i];
    if (lane != 0) return;
    a.out_cnt[q] = c;
    if (a.out_stats) {
      vc_query_stats s{};
      s.radius = a.t;
      s.n_results = c;
      s.n_sub_reads = sub;
      s.n_candidates = seen;
      a.out_stats[q] = s;
    }
  } else if (lane == 0) {
    a.next[atomicAdd(a.next_ctr, 1u)] = q;
  }
}

// One flagged approximate call: what is fixed for it, and its steps in the order sharded_global_approx() takes them.  Every step
// is entered and left with the ROOT device current (prepare() binds it; sharded_search_dev returns with it).
struct GaSearch {
  vc_sharded* h;
  const void* d_queries;
  uint32_t nq, k;
  uint64_t* d_out;
  uint32_t* d_counts;
  vc_query_stats* d_stats;
  hipStream_t S;
  // ---- fixed by prepare()
  uint32_t W, Sb;
  uint32_t nonempty;                 // bit g: shard g holds records
  bool trace;                        // dev (VC_MIH_GS_TRACE): per-round wall times on stderr
  GaRoundLists ls;
  uint64_t* ga_q;                    // the gathered open queries
  uint64_t* rows;                    // their merged rows, counts, statistics
  uint32_t* cnt;
  vc_query_stats* st;
  // ---- the rounds
  int cur;                           // the list of the round that runs
  uint32_t n_open;                   // its entries

  int prepare() {
    W = h->nbytes / 8; Sb = h->cfg.engine.bits / h->cfg.engine.n_tables;
    trace = h->knobs.gs_trace;
    nonempty = 0;
    for (uint32_t g = 0; g < h->G; ++g)
      if (shard_size(h, g)) nonempty |= 1u << g;
    int rc;
    VS_HIP(h, hipSetDevice(h->root));
    if ((rc = counts_or_own(h, nq, &d_counts))) return rc;
    if ((rc = grow(h, h->buf[GA_LISTS], GaRoundLists::words(nq) * 4))) return rc;
    if ((rc = grow(h, h->buf[GS_Q], (size_t)nq * h->nbytes))) return rc;
    if ((rc = grow(h, h->buf[GS_ROWS], (size_t)nq * k * 8))) return rc;
    if ((rc = grow(h, h->buf[GS_CNT], (size_t)nq * 4))) return rc;
    if ((rc = grow(h, h->buf[GS_ST], (size_t)nq * sizeof(vc_query_stats)))) return rc;
    ls = GaRoundLists::carve(h->buf[GA_LISTS].as<uint32_t>(), nq);
    ga_q = h->buf[GS_Q].as<uint64_t>();
    rows = h->buf[GS_ROWS].as<uint64_t>();
    cnt = h->buf[GS_CNT].as<uint32_t>();
    st = h->buf[GS_ST].as<vc_query_stats>();
    cur = 0; n_open = 0;
    VS_HIP(h, hipMemsetAsync(ls.ctr, 0, sizeof(GaCounters), S));
    return VC_OK;
  }

  // every query is open in the first round
  int open_all() {
    hipLaunchKernelGGL(gs_iota_kernel, dim3((nq + 255) / 256), dim3(256), 0, S, ls.list[0], nq);
    VS_HIP(h, hipGetLastError());
    n_open = nq;
    return VC_OK;
  }

  GaSettleArgs settle_args(uint32_t t) const {   // after the round's search: it may grow the slots
    const SlotLayout L(n_open, k, true);
    GaSettleArgs a{};
    a.base = h->root_lane_ref().gath(); a.slot_words = L.words; a.stats_off = L.stats_off; a.G = h->G; a.nonempty = nonempty;
    a.n = n_open; a.t = t; a.k = k; a.S = Sb;
    a.list = ls.list[cur]; a.rows = rows; a.cnt = cnt;
    a.out = d_out; a.out_cnt = d_counts; a.out_stats = d_stats;
    a.next = ls.list[cur ^ 1]; a.next_ctr = &ls.ctr->open[cur ^ 1]; a.bad = &ls.ctr->bad;
    return a;
  }

  // one round capped at t: gather the open queries, run every shard through shells 0..t in approximate mode, merge, and let the
  // settle kernel finish them or keep them open in the other list.  (The host waits inside each shard's capped search, not here.)
  int run_round(uint32_t t) {
    int rc;
    VS_HIP(h, hipMemsetAsync(&ls.ctr->open[cur ^ 1], 0, 4, S));
    VS_HIP(h, vc_launch_gather_queries((const uint64_t*)d_queries, ls.list[cur], n_open, W, ga_q, S));
    if ((rc = sharded_search_dev(h, ga_q, n_open, k, VC_MODE_MIH_APPROX, rows, cnt, st, S, t))) return rc;
    const uint32_t per_block = GA_SETTLE_BLK / VC_WAVE;
    hipLaunchKernelGGL(ga_settle_kernel, dim3((n_open + per_block - 1) / per_block), dim3(GA_SETTLE_BLK), 0, S, settle_args(t));
    VS_HIP(h, hipGetLastError());
    cur ^= 1;
    return VC_OK;
  }

  // the round ends: the host waits for its counters -- how many queries stay open, and whether a shard went astray
  int read_round_counters(uint32_t t, std::chrono::steady_clock::time_point t_round) {
    GaCounters c;
    VS_HIP(h, hipMemcpyAsync(&c, ls.ctr, sizeof c, hipMemcpyDeviceToHost, S));
    VS_HIP(h, hipStreamSynchronize(S));
    if (trace)
      fprintf(stderr, "[vc_ga] round %u: %u open -> %u open  %.1f us\n", t, n_open, c.open[cur],
              std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_round).count());
    n_open = c.open[cur];
    if (c.bad) return sfail(h, VC_ERR_STATE, "VC_FLAG_GLOBAL_APPROX: %u shard results of the round capped at shell %u ended in another shell", c.bad, t);
    return VC_OK;
  }
};

static int sharded_global_approx(vc_sharded* h, const void* d_queries, uint32_t nq, uint32_t k, uint64_t* d_out, uint32_t* d_counts,
                                 vc_query_stats* d_stats, hipStream_t S) {
  GaSearch c{h, d_queries, nq, k, d_out, d_counts, d_stats, S};
  int rc = c.prepare();
  if (!rc) rc = c.open_all();
  for (uint32_t t = 0; !rc && t <= c.Sb && c.n_open; ++t) {   // the round capped at the last shell settles whatever is open
    const auto t_round = std::chrono::steady_clock::now();
    rc = c.run_round(t);                                  // enqueued on S: the open queries searched capped at t and judged
    if (!rc) rc = c.read_round_counters(t, t_round);      // the round ends here: the host waits for what it left open
  }
  return rc;
}

static int sharded_search_any(vc_sharded* h, const void* d_queries, uint32_t nq, uint32_t k, uint32_t mode, uint64_t* d_out,
                              uint32_t* d_counts, vc_query_stats* d_stats, hipStream_t S) {
  if (mode == VC_MODE_MIH_EXACT && (h->cfg.engine.flags & VC_FLAG_GLOBAL_STOP))
    return sharded_global_stop(h, d_queries, nq, k, d_out, d_counts, d_stats, S);
  if (mode == VC_MODE_MIH_APPROX && (h->cfg.engine.flags & VC_FLAG_GLOBAL_APPROX) && h->n)   // (nothing ingested: what the unflagged store returns)
    return sharded_global_approx(h, d_queries, nq, k, d_out, d_counts, d_stats, S);
  return sharded_search_dev(h, d_queries, nq, k, mode, d_out, d_counts, d_stats, S);
}


// ---- radius search over the shards, device-resident ---------------------------------------------------------------------------
// vc_sharded_search_radius_dev (search_R_neighbors on every rank + gather_vectors + the master's dedup, search_worker.cc:177-199,
// 222-264, for callers that keep the batch in HBM).  Every non-empty shard answers the batch for its id range into its own flat
// result array + nq + 1 offsets; what a query's union looks like follows from two facts: a shard's segment is ascending, and the
// shards hold disjoint id ranges, so no two packed values (dist << 32 | id) of a query are equal.  The union is therefore a
// merge of G sorted lists of DISTINCT values, and the place of value v -- element i of shard g's segment of query q -- is
//     out_offs[q] + i + sum over g' != g of lower_bound(segment of g' for q, v)
// (i values of its own list and lower_bound values of every other list are smaller; no tie rule is needed).  Two kernels on the
// root: the union's offsets (a scan over the queries of the shards' summed segment lengths) and the rank merge, whose grid runs
// over ELEMENTS -- (shard, chunk of that shard's flat array) -- so that a heavy query is spread over many blocks.
// Scratch is what the shards found (no padded ring); the host waits once per shard, inside the shard's own call, for its total:
// the sum of those totals is the union's total, so the capacity decision and the merge grid need no further wait.
static_assert(VC_RMERGE_SHARDS == VC_MAX_SHARDS, "VcRadiusMergeArgs holds one pointer pair per shard");

// d_offsets[q] = sum over q' < q and all shards of len_g(q'), d_offsets[nq] = the total.  One block walks nq in tiles of its
// 1024 threads with a running carry.  A query's length is at most 2^32 (ids are uint32), so its low and high 16-bit halves each
// add up to less than 2^32 over a wave: two 32-bit wave scans make the 64-bit one.
extern "C" __global__ void __launch_bounds__(1024) vc_sharded_radius_offsets_kernel(const VcRadiusMergeArgs a, uint64_t* __restrict__ offsets) {
  __shared__ uint64_t s_w[1024 / VC_WAVE];
  const uint32_t lane = vc_lane(), wave = threadIdx.x / VC_WAVE;
  uint64_t carry = 0;
  for (uint32_t q0 = 0; q0 < a.nq; q0 += 1024) {
    const uint32_t q = q0 + threadIdx.x;
    uint64_t len = 0;
    if (q < a.nq)
      for (uint32_t g = 0; g < a.G; ++g)
        if (a.offs[g]) len += a.offs[g][q + 1] - a.offs[g][q];
    uint32_t tlo, thi;
    const uint32_t elo = vc_wave_excl_scan((uint32_t)(len & 0xFFFFu), tlo);
    const uint32_t ehi = vc_wave_excl_scan((uint32_t)(len >> 16), thi);
    if (lane == 0) s_w[wave] = ((uint64_t)thi << 16) + tlo;
    __syncthreads();
    uint64_t base = carry, tile = 0;
    for (uint32_t w = 0; w < 1024 / VC_WAVE; ++w) {
      if (w < wave) base += s_w[w];
      tile += s_w[w];
    }
    if (q < a.nq) offsets[q] = base + ((uint64_t)ehi << 16) + elo;
    carry += tile;
    __syncthreads();   // the next tile rewrites s_w
  }
  if (threadIdx.x == 0) offsets[a.nq] = carry;
}

// the q in [lo, hi) with offs[q] <= e < offs[q + 1]; needs offs[lo] <= e < offs[hi]
__device__ __forceinline__ uint32_t rmerge_query_of(const uint64_t* __restrict__ offs, uint32_t lo, uint32_t hi, uint64_t e) {
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (offs[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

// One block per (shard g, chunk of VC_RMERGE_CHUNK elements of g's flat result array); a chunk may hold parts of many queries
// and a query may span many chunks.  The block finds the chunk's first and last query, keeps that range of g's offsets in LDS
// (queries beyond the window -- a chunk that crosses more than VC_RMERGE_CHUNK queries, most of them empty -- are read from
// global memory), every thread finds its element's query there, ranks the value in the other shards' segments of that query by
// binary search in global memory and writes it once.  No atomics, no scratch, nothing padded.
extern "C" __global__ void __launch_bounds__(VC_RMERGE_THREADS) vc_sharded_radius_merge_kernel(const VcRadiusMergeArgs a) {
  constexpr uint32_t WIN = VC_RMERGE_CHUNK + 2;
  __shared__ uint64_t s_off[WIN];
  __shared__ uint32_t s_q[2];
  uint32_t g = 0;
  while (g + 1 < VC_RMERGE_SHARDS && blockIdx.x >= a.first_block[g + 1]) ++g;   // first_block[g] <= blockIdx.x < first_block[g + 1]
  const uint64_t* __restrict__ og = a.offs[g];
  const uint64_t* __restrict__ sg = a.seg[g];
  const uint64_t e0 = (uint64_t)(blockIdx.x - a.first_block[g]) * VC_RMERGE_CHUNK;
  const uint64_t e1 = min(e0 + VC_RMERGE_CHUNK, a.total_g[g]);
  if (e0 >= e1) return;                                                         // (never: the grid holds no empty chunk)
  // og[0] = 0 <= e < total_g = og[nq] for every element of the shard; two waves search at the same time
  if (threadIdx.x == 0) s_q[0] = rmerge_query_of(og, 0, a.nq, e0);
  if (threadIdx.x == VC_WAVE) s_q[1] = rmerge_query_of(og, 0, a.nq, e1 - 1);
  __syncthreads();
  const uint32_t q_lo = s_q[0], q_hi = s_q[1];
  const uint32_t nwin = min(q_hi - q_lo + 2, WIN);                              // og[q_lo .. q_hi + 1], as far as the window goes
  for (uint32_t i = threadIdx.x; i < nwin; i += VC_RMERGE_THREADS) s_off[i] = og[q_lo + i];
  __syncthreads();
  auto off = [&](uint32_t q) { return q - q_lo < nwin ? s_off[q - q_lo] : og[q]; };
  for (uint32_t j = 0; j < VC_RMERGE_PER_THREAD; ++j) {
    const uint64_t e = e0 + (uint64_t)j * VC_RMERGE_THREADS + threadIdx.x;
    if (e >= e1) break;
    const uint64_t v = sg[e];
    uint32_t lo = q_lo, hi = q_hi + 1;                                          // off(lo) <= e < off(hi)
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (off(mid) <= e) lo = mid; else hi = mid;
    }
    const uint32_t q = lo;
    uint64_t pos = a.out_offs[q] + (e - off(q));
    for (uint32_t g2 = 0; g2 < a.G; ++g2) {
      if (g2 == g || !a.offs[g2]) continue;
      const uint64_t b = a.offs[g2][q];
      const uint64_t* __restrict__ seg = a.seg[g2] + b;
      uint64_t l = 0, r = a.offs[g2][q + 1] - b;                                // lower_bound: how many of g2's values are below v
      while (l < r) {
        const uint64_t mid = l + (r - l) / 2;
        if (seg[mid] < v) l = mid + 1; else r = mid;
      }
      pos += l;
    }
    if (pos < a.total) a.out[pos] = v;
  }
}

// One radius batch through the shards, and its steps in the order sharded_radius_dev takes them.  Queries, results and offsets
// live in HBM on the root device; the merge may still run on `S` when the call returns (results are valid in `S` order).
struct ShardRadius {
  vc_sharded* h;
  const void* d_queries;
  uint32_t nq, radius, mode;
  uint64_t* d_out;
  uint64_t out_cap;
  uint64_t* d_offsets;
  hipStream_t S;
  size_t qbytes;
  uint64_t total_g[VC_MAX_SHARDS];      // what every shard found (empty shards: 0), known to the host after run_lanes
  VcRadiusMergeArgs A;
  std::vector<int> lane_rc;             // run_lane: the first failure of every lane, reported by run_lanes
  std::vector<std::string> lane_err;

  // every non-empty shard's offsets and (first call: starting size) result buffer on its own device, the remote lanes' query copy
  int prepare_buffers() {
    int rc;
    size_t first_bytes;
    if (!vc_rshard_bytes(vc_rshard_first_cap(nq), &first_bytes)) return sfail(h, VC_ERR_NOMEM, "radius search: batch too large");
    for (uint32_t li = 0; li < h->lanes.size(); ++li) {
      Lane& l = h->lanes[li];
      VS_HIP(h, hipSetDevice(l.dev));
      if (li != h->root_lane && (rc = grow(h, l.buf[LANE_Q], qbytes))) return rc;
      for (uint32_t g : l.shards) {
        if (shard_size(h, g) == 0) continue;
        if ((rc = grow(h, h->rad[g].offs, vc_rshard_offs_bytes(nq)))) return rc;
        if ((rc = grow(h, h->rad[g].res, first_bytes))) return rc;
      }
    }
    return VC_OK;
  }

  int send_queries() { return send_queries_to_lanes(h, d_queries, qbytes, S); }

  // the shards of one device answer the batch for their id ranges, one after the other; every shard's call makes the host wait
  // for its total.  A shard whose result buffer was too small grows it to the reported total and repeats once.  (On a host
  // thread of its own when there are several lanes: binds the lane's device for that thread, touches only the lane's shards'
  // buffers and totals and the lane's lane_rc / lane_err.)
  void run_lane(uint32_t li) {
    Lane& l = h->lanes[li];
    const bool is_root = li == h->root_lane;
    hipStream_t ls = is_root ? S : l.stream;
    const void* q = is_root ? d_queries : l.q();
    auto hip = [&](hipError_t r, const char* what) {
      if (r != hipSuccess && lane_rc[li] == VC_OK) {
        lane_rc[li] = r == hipErrorOutOfMemory ? VC_ERR_NOMEM : VC_ERR_HIP;
        lane_err[li] = std::string(what) + ": " + hipGetErrorString(r);
      }
      return r == hipSuccess;
    };
    if (!hip(hipSetDevice(l.dev), "hipSetDevice")) return;
    for (uint32_t g : l.shards) {
      if (shard_size(h, g) == 0) continue;   // never asked: zero-length segments
      RadiusShardBufs& B = h->rad[g];
      for (int attempt = 0;; ++attempt) {
        const uint64_t cap = B.res.bytes / 8;
        const int r = vc_engine_radius_dev(h->eng[g], q, nq, radius, mode, B.res.as<uint64_t>(), cap, B.offs.as<uint64_t>(), &total_g[g], ls);
        if (r == VC_OK) break;
        size_t need;
        if (r != VC_ERR_CAPACITY || attempt || !vc_rshard_must_repeat(total_g[g], cap) || !vc_rshard_bytes(total_g[g], &need)) {
          lane_rc[li] = r;
          lane_err[li] = std::string("shard ") + std::to_string(g) + ": " + vc_last_error(h->eng[g]);
          return;
        }
        if (!hip(B.res.regrow(need), "result buffer")) return;   // (the first attempt has been waited for: nothing reads the old one)
      }
    }
    if (!is_root) hip(hipEventRecord(l.done, ls), "hipEventRecord");
  }

  // every lane: in turn when there is one, else concurrently (every shard call waits on the host, in both modes)
  int run_lanes() {
    lane_rc.assign(h->lanes.size(), VC_OK);
    lane_err.assign(h->lanes.size(), std::string());
    for (uint64_t& t : total_g) t = 0;
    if (h->lanes.size() == 1) {
      run_lane(0);
    } else {
      std::vector<std::thread> th;
      for (uint32_t li = 0; li < h->lanes.size(); ++li) th.emplace_back([this, li] { run_lane(li); });
      for (auto& t : th) t.join();
    }
    for (uint32_t li = 0; li < h->lanes.size(); ++li)
      if (lane_rc[li]) return sfail(h, lane_rc[li], "%s", lane_err[li].c_str());
    return VC_OK;
  }

  // replaces gather_vectors (mpi_coordinator.cc:34-69): a remote shard's offsets and its total_g results reach the root by one
  // peer copy each, behind its lane's `done` event -- always peer copies, whatever the handle's exchange: the lengths vary and
  // only the root needs the data.  Shards of the root device are read where they lie.  Leaves the pointers in A.
  int exchange() {
    VS_HIP(h, hipSetDevice(h->root));
    int rc;
    for (uint32_t g = 0; g < h->G; ++g) {   // the root's copies first (growing one waits for the device)
      if (h->lane_of[g] == h->root_lane || shard_size(h, g) == 0) continue;
      size_t bytes;
      if (!vc_rshard_bytes(total_g[g], &bytes)) return sfail(h, VC_ERR_NOMEM, "radius search: shard %u found too much", g);
      if ((rc = grow(h, h->rad[g].root_offs, vc_rshard_offs_bytes(nq)))) return rc;
      if ((rc = grow(h, h->rad[g].root_res, bytes))) return rc;
    }
    for (uint32_t li = 0; li < h->lanes.size(); ++li) {
      if (li == h->root_lane) continue;
      Lane& l = h->lanes[li];
      VS_HIP(h, hipStreamWaitEvent(S, l.done, 0));
      for (uint32_t g : l.shards) {
        if (shard_size(h, g) == 0) continue;
        RadiusShardBufs& B = h->rad[g];
        VS_HIP(h, hipMemcpyPeerAsync(B.root_offs.p, h->root, B.offs.p, l.dev, vc_rshard_offs_bytes(nq), S));
        if (total_g[g]) VS_HIP(h, hipMemcpyPeerAsync(B.root_res.p, h->root, B.res.p, l.dev, (size_t)total_g[g] * 8, S));
      }
    }
    for (uint32_t g = 0; g < VC_MAX_SHARDS; ++g) {
      const bool empty = g >= h->G || shard_size(h, g) == 0, local = !empty && h->lane_of[g] == h->root_lane;
      A.offs[g] = empty ? nullptr : (local ? h->rad[g].offs : h->rad[g].root_offs).as<uint64_t>();
      A.seg[g] = empty ? nullptr : (local ? h->rad[g].res : h->rad[g].root_res).as<uint64_t>();
    }
    return VC_OK;
  }

  // the union's offsets (also when the call is going to report VC_ERR_CAPACITY: they are the needed counts)
  int offsets() {
    if (!vc_rmerge_plan(total_g, h->G, &A)) return sfail(h, VC_ERR_CAPACITY, "radius search: more results than one merge launch can place");
    A.nq = nq;
    A.out_offs = d_offsets;
    A.out = d_out;
    hipLaunchKernelGGL(vc_sharded_radius_offsets_kernel, dim3(1), dim3(1024), 0, S, A, d_offsets);
    VS_HIP(h, hipGetLastError());
    return VC_OK;
  }

  // the rank merge straight to the final positions; not launched when the results do not fit or there are none
  int merge() {
    if (A.total > out_cap) return sfail(h, VC_ERR_CAPACITY, "radius search: output buffer too small (needed counts are in d_offsets)");
    if (A.total == 0) return VC_OK;
    hipLaunchKernelGGL(vc_sharded_radius_merge_kernel, dim3(A.first_block[VC_RMERGE_SHARDS]), dim3(VC_RMERGE_THREADS), 0, S, A);
    VS_HIP(h, hipGetLastError());
    return VC_OK;
  }
};

// Any device may be current on entry; the root device is on return from exchange() onwards.
// total (may be null): the union's total once the shards have answered, also when it exceeds out_cap (VC_ERR_CAPACITY).
static int sharded_radius_dev(vc_sharded* h, const void* d_queries, uint32_t nq, uint32_t radius, uint32_t mode, uint64_t* d_out,
                              uint64_t out_cap, uint64_t* d_offsets, hipStream_t S, uint64_t* total = nullptr) {
  ShardRadius b{h, d_queries, nq, radius, mode, d_out, out_cap, d_offsets, S, (size_t)nq * h->nbytes, {}, {}, {}, {}};
  int rc = b.prepare_buffers();
  if (!rc) rc = b.send_queries();
  if (!rc) rc = b.run_lanes();
  if (!rc) rc = b.exchange();
  if (!rc) rc = b.offsets();
  if (!rc && total) *total = b.A.total;
  if (!rc) rc = b.merge();
  return rc;
}

// ---- queries named by id over the shards (search_image_by_id, image_search_client.h:12-27) ------------------------------------------
// d_ids (root device) -> d_q [nq][W] + d_found (nullable) on the root, all enqueued, nothing waited for: the ids reach every other
// device by one peer copy, every non-empty shard gathers the ids it owns into its slot on its own device (vc_ids_gather_kernel with
// the shard's id range: zero rows for the rest), a remote shard's slot travels to the root by one peer copy behind its lane's `done`
// event, the root's shards wrote theirs in place, and vc_ids_merge_kernel ORs the filled slots.  Returns with the root device current.
// fill (the search calls): the first non-empty shard gives an id that is resident NOWHERE in the store its record 0 as a stand-in query.
static int sharded_gather_ids(vc_sharded* h, const uint32_t* d_ids, uint32_t nq, uint64_t* d_q, uint32_t* d_found, bool fill, hipStream_t S) {
  const uint32_t W = h->nbytes / 8;
  const uint64_t slot_words = vc_ids_slot_words(nq, W);
  int rc;
  for (uint32_t li = 0; li < h->lanes.size(); ++li) {
    Lane& l = h->lanes[li];
    VS_HIP(h, hipSetDevice(l.dev));
    if ((rc = grow(h, l.buf[LANE_IDGATH], slot_words * 8 * (li == h->root_lane ? h->G : l.shards.back() + 1)))) return rc;
    if (li != h->root_lane && (rc = grow(h, l.buf[LANE_IDS], (size_t)nq * 4))) return rc;
  }
  if (h->lanes.size() > 1) {
    VS_HIP(h, hipSetDevice(h->root));
    VS_HIP(h, hipEventRecord(h->ev_q, S));
  }
  uint32_t mask = 0;
  for (uint32_t li = 0; li < h->lanes.size(); ++li) {
    Lane& l = h->lanes[li];
    const bool is_root = li == h->root_lane;
    hipStream_t ls = is_root ? S : l.stream;
    VS_HIP(h, hipSetDevice(l.dev));
    if (!is_root) {
      VS_HIP(h, hipStreamWaitEvent(ls, h->ev_q, 0));   // also orders the lane behind the previous batch's copies out of its buffers
      VS_HIP(h, hipMemcpyPeerAsync(l.buf[LANE_IDS].p, l.dev, d_ids, h->root, (size_t)nq * 4, ls));
    }
    for (uint32_t g : l.shards) {
      if (shard_size(h, g) == 0) continue;
      VcEngineView v;
      if ((rc = vc_engine_view(h->eng[g], &v))) return sfail(h, rc, "shard %u: no view", g);
      uint64_t* slot = l.buf[LANE_IDGATH].as<uint64_t>() + (size_t)g * slot_words;
      VS_HIP(h, vc_launch_ids_gather(v.cols, v.stride, v.W, v.id_base, v.n, h->cfg.engine.id_base, fill && g == 0 ? h->n : 0,
                                     is_root ? d_ids : l.buf[LANE_IDS].as<uint32_t>(), nq, slot,
                                     (uint32_t*)(slot + (size_t)nq * W), ls));
      mask |= 1u << g;
    }
    if (!is_root) VS_HIP(h, hipEventRecord(l.done, ls));
  }
  VS_HIP(h, hipSetDevice(h->root));
  uint64_t* root_slots = h->root_lane_ref().buf[LANE_IDGATH].as<uint64_t>();
  for (uint32_t li = 0; li < h->lanes.size(); ++li) {
    if (li == h->root_lane) continue;
    Lane& l = h->lanes[li];
    VS_HIP(h, hipStreamWaitEvent(S, l.done, 0));
    for (uint32_t g : l.shards)
      if (mask >> g & 1)
        VS_HIP(h, hipMemcpyPeerAsync(root_slots + (size_t)g * slot_words, h->root, l.buf[LANE_IDGATH].as<uint64_t>() + (size_t)g * slot_words,
                                     l.dev, slot_words * 8, S));
  }
  VS_HIP(h, vc_launch_ids_merge(root_slots, slot_words, mask, nq, W, d_q, d_found, S));
  return VC_OK;
}

static int check_sharded_ids_args(vc_sharded* h, const uint32_t* ids, uint32_t nq, uint32_t k, uint32_t mode, uint32_t id_flags, const void* out) {
  if (!h || !ids || !out || nq == 0 || k == 0 || k > VC_MAX_K || mode > VC_MODE_MIH_APPROX) return VC_ERR_INVALID;
  if (id_flags & ~VC_IDS_EXCLUDE_SELF) return sfail(h, VC_ERR_INVALID, "unknown id_flags 0x%x", id_flags);
  if ((id_flags & VC_IDS_EXCLUDE_SELF) && k > VC_MAX_K - 1) return sfail(h, VC_ERR_INVALID, "k must be in 1..%u with VC_IDS_EXCLUDE_SELF", VC_MAX_K - 1);
  return VC_OK;
}

extern "C" {

int vc_sharded_root_device(const vc_sharded* h, int* device) {
  if (!h || !device) return VC_ERR_INVALID;
  *device = h->root;
  return VC_OK;
}

int vc_sharded_search_knn_dev(vc_sharded* h, const void* d_queries, uint32_t nq, uint32_t k, uint32_t mode, uint64_t* d_out,
                              uint32_t* d_counts, vc_query_stats* d_stats, void* stream) {
  if (!h || !d_queries || !d_out || nq == 0 || k == 0 || k > VC_MAX_K || mode > VC_MODE_MIH_APPROX) return VC_ERR_INVALID;
  return sharded_search_any(h, d_queries, nq, k, mode, d_out, d_counts, d_stats, sharded_caller_stream(h, stream));
}

// the merged rows and counts (and statistics, when wanted) of the host-pointer call reach the host; waits for them
static int fetch_results(vc_sharded* h, uint32_t nq, uint32_t k, uint64_t* out, uint32_t* cnt, vc_query_stats* stats, hipStream_t S) {
  VS_HIP(h, hipMemcpyAsync(out, h->buf[ROOT_OUT].p, (size_t)nq * k * 8, hipMemcpyDeviceToHost, S));
  VS_HIP(h, hipMemcpyAsync(cnt, h->buf[ROOT_OCNT].p, (size_t)nq * 4, hipMemcpyDeviceToHost, S));
  if (stats) VS_HIP(h, hipMemcpyAsync(stats, h->buf[ROOT_OSTATS].p, (size_t)nq * sizeof(vc_query_stats), hipMemcpyDeviceToHost, S));
  VS_HIP(h, hipStreamSynchronize(S));
  return VC_OK;
}

// A shard's device-side ring-overflow recovery gave up (its grid never met; never seen outside tests): the LINEAR batch is
// answered again through the shards' host API, whose host-driven recovery always ends, one shard after the other;
// the rows go back into the root's slots and are merged by the same kernel into the handle's row / count buffers.
static int reanswer_linear_by_host(vc_sharded* h, const void* queries, uint32_t nq, uint32_t k, hipStream_t S) {
  const SlotLayout L(nq, k, false);
  Lane& R = h->root_lane_ref();
  int rc;
  VS_HIP(h, hipSetDevice(h->root));
  if ((rc = grow(h, R.buf[LANE_GATH], L.words * 8 * h->G))) return rc;
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
    VS_HIP(h, hipMemcpyAsync(R.slot(g, L.words), slot.data(), L.words * 8, hipMemcpyHostToDevice, S));
    VS_HIP(h, hipStreamSynchronize(S));   // `slot` is reused by the next shard
  }
  VS_HIP(h, vc_launch_select_slots(R.gath(), L.words, (uint32_t)L.cnt_off, h->G, nq, k, h->buf[ROOT_OUT].as<uint64_t>(),
                                   h->buf[ROOT_OCNT].as<uint32_t>(), S));
  return VC_OK;
}

int vc_sharded_search_knn(vc_sharded* h, const void* queries, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order,
                          uint64_t* out, uint32_t* counts, vc_query_stats* stats) {
  if (!h || !queries || !out || nq == 0 || k == 0 || k > VC_MAX_K || mode > VC_MODE_MIH_APPROX || order > VC_ORDER_FARTHEST_FIRST)
    return VC_ERR_INVALID;
  const size_t qbytes = (size_t)nq * h->nbytes, rows = (size_t)nq * k;
  int rc;
  hipStream_t S = h->root_stream;
  VS_HIP(h, hipSetDevice(h->root));
  if ((rc = grow(h, h->buf[ROOT_HQ], qbytes))) return rc;
  if ((rc = grow(h, h->buf[ROOT_OUT], rows * 8))) return rc;
  if ((rc = grow(h, h->buf[ROOT_OCNT], (size_t)nq * 4))) return rc;
  if (stats && (rc = grow(h, h->buf[ROOT_OSTATS], (size_t)nq * sizeof(vc_query_stats)))) return rc;
  VS_HIP(h, hipMemcpyAsync(h->buf[ROOT_HQ].p, queries, qbytes, hipMemcpyHostToDevice, S));
  if ((rc = sharded_search_any(h, h->buf[ROOT_HQ].p, nq, k, mode, h->buf[ROOT_OUT].as<uint64_t>(), h->buf[ROOT_OCNT].as<uint32_t>(),
                               stats ? h->buf[ROOT_OSTATS].as<vc_query_stats>() : nullptr, S)))
    return rc;
  std::vector<uint32_t> cnt(nq);
  VS_HIP(h, hipSetDevice(h->root));
  if ((rc = fetch_results(h, nq, k, out, cnt.data(), stats, S))) return rc;
  bool gave_up = false;
  for (uint32_t i = 0; i < nq; ++i) gave_up = gave_up || cnt[i] == 0xFFFFFFFFu;
  if (gave_up && mode == VC_MODE_LINEAR) {
    if ((rc = reanswer_linear_by_host(h, queries, nq, k, S))) return rc;
    if ((rc = fetch_results(h, nq, k, out, cnt.data(), nullptr, S))) return rc;
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

// every shard's neighbours within `radius` through its host API: res[g] holds them query after query, offs[g] where each starts
static int radius_by_shard(vc_sharded* h, const void* queries, uint32_t nq, uint32_t radius, uint32_t mode,
                           std::vector<std::vector<uint64_t>>* res, std::vector<std::vector<uint64_t>>* offs) {
  for (uint32_t g = 0; g < h->G; ++g) {
    if (shard_size(h, g) == 0) continue;
    uint64_t cap = (uint64_t)nq * 64;
    for (int attempt = 0;; ++attempt) {
      (*res)[g].resize(std::max<uint64_t>(cap, 1));
      const int rc = vc_search_radius(h->eng[g], queries, nq, radius, mode, (*res)[g].data(), cap, (*offs)[g].data());
      if (rc == VC_OK) break;
      if (rc != VC_ERR_CAPACITY || attempt) return sfail(h, rc, "shard %u: %s", g, vc_last_error(h->eng[g]));
      cap = (*offs)[g][nq];   // the needed size came back in the offsets
    }
  }
  return VC_OK;
}

// the padded segments ([nq][cap2], count[q] entries each) are ordered and packed on the root device by the radius search's own
// segment sort, one block per query, into out[0 .. total) at out_offsets
static int sort_segments_on_root(vc_sharded* h, const std::vector<uint64_t>& ring, uint64_t cap2, const std::vector<uint32_t>& count,
                                 const uint64_t* out_offsets, uint64_t total, uint32_t nq, uint64_t* out) {
  hipStream_t S = h->root_stream;
  VS_HIP(h, hipSetDevice(h->root));
  enum { RING, OFFS, OUT, COUNT, N_TMP };
  ScopedBufs<N_TMP> tmp;
  int rc;
  if ((rc = grow(h, tmp.b[RING], ring.size() * 8))) return rc;
  if ((rc = grow(h, tmp.b[OFFS], ((size_t)nq + 1) * 8))) return rc;
  if ((rc = grow(h, tmp.b[OUT], total * 8))) return rc;
  if ((rc = grow(h, tmp.b[COUNT], (size_t)nq * 4))) return rc;
  VS_HIP(h, hipMemcpyAsync(tmp.b[RING].p, ring.data(), ring.size() * 8, hipMemcpyHostToDevice, S));
  VS_HIP(h, hipMemcpyAsync(tmp.b[OFFS].p, out_offsets, ((size_t)nq + 1) * 8, hipMemcpyHostToDevice, S));
  VS_HIP(h, hipMemcpyAsync(tmp.b[COUNT].p, count.data(), (size_t)nq * 4, hipMemcpyHostToDevice, S));
  VS_HIP(h, vc_launch_sort_compact_segments(tmp.b[RING].as<uint64_t>(), (uint32_t)cap2, tmp.b[COUNT].as<uint32_t>(), tmp.b[OFFS].as<uint64_t>(),
                                            tmp.b[OUT].as<uint64_t>(), total, nq, S));
  VS_HIP(h, hipMemcpyAsync(out, tmp.b[OUT].p, total * 8, hipMemcpyDeviceToHost, S));
  VS_HIP(h, hipStreamSynchronize(S));
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
  if (int rc = radius_by_shard(h, queries, nq, radius, mode, &res, &offs)) return rc;
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
  return sort_segments_on_root(h, ring, cap2, count, out_offsets, total, nq, out);
}

int vc_sharded_search_radius_dev(vc_sharded* h, const void* d_queries, uint32_t nq, uint32_t radius, uint32_t mode, uint64_t* d_out,
                                 uint64_t out_cap, uint64_t* d_offsets, void* stream) {
  if (!h || !d_queries || !d_offsets || nq == 0 || (mode != VC_MODE_LINEAR && mode != VC_MODE_MIH_EXACT) || (!d_out && out_cap))
    return VC_ERR_INVALID;
  return sharded_radius_dev(h, d_queries, nq, radius, mode, d_out, out_cap, d_offsets, sharded_caller_stream(h, stream));
}

int vc_sharded_get_codes_dev(vc_sharded* h, const uint32_t* d_ids, uint32_t nq, void* d_codes, uint32_t* d_found, void* stream) {
  if (!h || !d_ids || !d_codes || nq == 0) return VC_ERR_INVALID;
  return sharded_gather_ids(h, d_ids, nq, (uint64_t*)d_codes, d_found, false, sharded_caller_stream(h, stream));
}

}  // extern "C"

// ---- the store as the drivers it shares with the single engine see it --------------------------------------------------------
static int check_sharded_index(vc_sharded* h, uint32_t mode) {   // exact MIH needs an index on every non-empty shard
  if (mode == VC_MODE_MIH_EXACT)
    for (uint32_t g = 0; g < h->G; ++g)
      if (shard_size(h, g) && !vc_engine_has_index(h->eng[g])) return sfail(h, VC_ERR_STATE, "shard %u: MIH search needs vc_sharded_build_index() first", g);
  return VC_OK;
}

static VcScratchAlloc sharded_scratch_alloc(vc_sharded* h) {   // buffer `which` of the table (VcScratch) on the root, which it binds
  return [h](int which, size_t bytes) -> void* {
    if (hipSetDevice(h->root) != hipSuccess) return nullptr;
    DevBuf& b = h->buf[SCRATCH + which];
    return grow(h, b, bytes) ? nullptr : b.p;
  };
}

// The view of one call: the buffers are the root's, everything the root does goes to S.  The gather and the searches visit the other
// devices and come back with the root current, so the drivers never bind one.
static VcStoreView sharded_store_view(vc_sharded* h, uint32_t mode, hipStream_t S) {
  VcStoreView v;
  v.n = h->n;
  v.id_base = h->cfg.engine.id_base;
  v.W = h->nbytes / 8;
  v.alloc = sharded_scratch_alloc(h);
  v.held = [h](int which) { return h->buf[SCRATCH + which].bytes; };
  v.gather = [h, S](const uint32_t* d_ids, uint32_t nq, uint64_t* d_q, uint32_t* d_found) { return sharded_gather_ids(h, d_ids, nq, d_q, d_found, true, S); };
  v.search = [h, mode, S](const uint64_t* d_q, uint32_t nq, uint32_t radius, uint64_t* d_raw, uint64_t cap, uint64_t* d_roffs, uint64_t* raw_total) -> int {
    const int rc = sharded_radius_dev(h, d_q, nq, radius, mode, d_raw, cap, d_roffs, S, raw_total);
    if (rc && rc != VC_ERR_CAPACITY) return rc;
    VS_HIP(h, hipSetDevice(h->root));
    return rc;
  };
  v.knn = [h, mode, S](const uint64_t* d_q, uint32_t nq, uint32_t kp, uint64_t* d_rows, uint32_t* d_cnt, vc_query_stats* d_stats) -> int {
    const int rc = sharded_search_any(h, d_q, nq, kp, mode, d_rows, d_cnt, d_stats, S);
    if (rc) return rc;
    VS_HIP(h, hipSetDevice(h->root));
    return VC_OK;
  };
  return v;
}

// An entry point after its checks: the root bound, `run` (a driver's vc_*_run or vc_*_run_host) with the view on stream S.
template <class Run>
static int sharded_store_call(vc_sharded* h, uint32_t mode, hipStream_t S, const Run& run) {
  VS_HIP(h, hipSetDevice(h->root));
  std::string err;
  const int rc = run(sharded_store_view(h, mode, S), S, &err);
  return rc && !err.empty() ? sfail(h, rc, "%s", err.c_str()) : rc;   // (a closure of the view has left its own text)
}

// ---- queries named by id over the shards: the drivers of vc_ids.hip and vc_ids_radius.hip on the root --------------------------------
static int check_sharded_radius_ids_args(vc_sharded* h, const uint32_t* ids, uint32_t nq, uint32_t mode, uint32_t id_flags, const uint64_t* out,
                                         uint64_t out_cap, const uint64_t* offsets) {
  if (!h || !ids || !offsets || nq == 0 || (mode != VC_MODE_LINEAR && mode != VC_MODE_MIH_EXACT) || (!out && out_cap)) return VC_ERR_INVALID;
  if (id_flags & ~(VC_IDS_EXCLUDE_SELF | VC_IDS_ONLY_GREATER)) return sfail(h, VC_ERR_INVALID, "unknown id_flags 0x%x", id_flags);
  return check_sharded_index(h, mode);
}

extern "C" {

int vc_sharded_search_knn_ids_dev(vc_sharded* h, const uint32_t* d_ids, uint32_t nq, uint32_t k, uint32_t mode, uint32_t id_flags,
                                  uint64_t* d_out, uint32_t* d_counts, vc_query_stats* d_stats, void* stream) {
  const int rc = check_sharded_ids_args(h, d_ids, nq, k, mode, id_flags, d_out);
  if (rc) return rc;
  const uint32_t kp = vc_ids_kp(k, id_flags);
  return sharded_store_call(h, mode, sharded_caller_stream(h, stream), [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    VcIdsKnnBufs b;
    const int r = vc_ids_knn_reserve(v, nq, kp, &b);
    return r ? r : vc_ids_knn_run(v, b, d_ids, nq, kp, k, d_out, d_counts, d_stats, S, err);
  });
}

int vc_sharded_search_knn_ids(vc_sharded* h, const uint32_t* ids, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order,
                              uint32_t id_flags, uint64_t* out, uint32_t* counts, vc_query_stats* stats) {
  const int rc = check_sharded_ids_args(h, ids, nq, k, mode, id_flags, out);
  if (rc) return rc;
  if (order > VC_ORDER_FARTHEST_FIRST) return VC_ERR_INVALID;
  const uint32_t kp = vc_ids_kp(k, id_flags);
  return sharded_store_call(h, mode, h->root_stream, [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_ids_knn_run_host(v, VcIdsKnnHostArgs{ids, nq, kp, k, order, mode == VC_MODE_LINEAR, out, counts, stats},
                               [&](const VcIdsKnnBufs& b, const uint32_t* d_ids, uint64_t* d_out, uint32_t* d_counts, vc_query_stats* d_stats) {
                                 return vc_ids_knn_run(v, b, d_ids, nq, kp, k, d_out, d_counts, d_stats, S, err);
                               },
                               [&](const uint64_t* codes, uint64_t* rows, uint32_t* rcnt) {   // (its shards recover on the host)
                                 return vc_sharded_search_knn(h, codes, nq, kp, mode, VC_ORDER_ASCENDING, rows, rcnt, stats);
                               },
                               S, err);
  });
}

int vc_sharded_search_radius_ids_dev(vc_sharded* h, const uint32_t* d_ids, uint32_t nq, uint32_t radius, uint32_t mode, uint32_t id_flags,
                                     uint64_t* d_out, uint64_t out_cap, uint64_t* d_offsets, void* stream) {
  const int rc = check_sharded_radius_ids_args(h, d_ids, nq, mode, id_flags, d_out, out_cap, d_offsets);
  if (rc) return rc;
  return sharded_store_call(h, mode, sharded_caller_stream(h, stream), [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_ids_radius_run(v, d_ids, nq, radius, id_flags, d_out, out_cap, d_offsets, S, err);
  });
}

int vc_sharded_search_radius_ids(vc_sharded* h, const uint32_t* ids, uint32_t nq, uint32_t radius, uint32_t mode, uint32_t id_flags, uint64_t* out,
                                 uint64_t out_cap, uint64_t* out_offsets) {
  const int rc = check_sharded_radius_ids_args(h, ids, nq, mode, id_flags, out, out_cap, out_offsets);
  if (rc) return rc;
  return sharded_store_call(h, mode, h->root_stream, [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_ids_radius_run_host(v, ids, nq, out, out_cap, out_offsets,
                                  [&](const uint32_t* d_ids, uint64_t* d_out, uint64_t* d_offsets) {
                                    return vc_ids_radius_run(v, d_ids, nq, radius, id_flags, d_out, out_cap, d_offsets, S, err);
                                  },
                                  S, err);
  });
}

}  // extern "C"

// ---- the clustering calls over the shards: the drivers of vc_cluster.hip, vc_levels.hip, vc_leaders.hip, vc_dbscan.hip and
// vc_dbscan_levels.hip on the root, their walk (vc_walk.hip) through the sharded gather and the union's radius search ------------------
static int check_sharded_cluster_args(vc_sharded* h, const char* what, uint32_t mode, uint64_t n_labelled, const uint32_t* labels) {   // what: "cluster" or "leaders"
  if (!h || !labels || (mode != VC_MODE_LINEAR && mode != VC_MODE_MIH_EXACT)) return VC_ERR_INVALID;
  if (n_labelled > h->n) return sfail(h, VC_ERR_INVALID, "%s: n_labelled %llu exceeds the %llu resident records", what, (unsigned long long)n_labelled, (unsigned long long)h->n);
  return check_sharded_index(h, mode);
}
static int check_sharded_levels_args(vc_sharded* h, uint32_t max_radius, uint32_t mode, uint64_t n_labelled, const uint32_t* labels) {
  if (!h || !labels || (mode != VC_MODE_LINEAR && mode != VC_MODE_MIH_EXACT)) return VC_ERR_INVALID;
  if (max_radius >= VC_LEVELS_MAX) return sfail(h, VC_ERR_INVALID, "cluster levels: max_radius %u exceeds %u", max_radius, VC_LEVELS_MAX - 1);
  return check_sharded_cluster_args(h, "cluster", mode, n_labelled, labels);
}
static int check_sharded_dbscan_args(vc_sharded* h, uint32_t min_pts, uint32_t mode, const uint32_t* labels) {
  if (!h || !labels || (mode != VC_MODE_LINEAR && mode != VC_MODE_MIH_EXACT)) return VC_ERR_INVALID;
  if (min_pts == 0) return sfail(h, VC_ERR_INVALID, "dbscan: min_pts must be at least 1");
  return check_sharded_index(h, mode);
}
static int check_sharded_dbscan_levels_args(vc_sharded* h, uint32_t max_radius, uint32_t min_pts, uint32_t mode, const uint32_t* labels) {
  if (!h || !labels || (mode != VC_MODE_LINEAR && mode != VC_MODE_MIH_EXACT)) return VC_ERR_INVALID;
  if (max_radius >= VC_LEVELS_MAX) return sfail(h, VC_ERR_INVALID, "dbscan levels: max_radius %u exceeds %u", max_radius, VC_LEVELS_MAX - 1);
  return check_sharded_dbscan_args(h, min_pts, mode, labels);
}

extern "C" {

int vc_sharded_cluster_radius_dev(vc_sharded* h, uint32_t radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* d_labels,
                                  vc_cluster_stats* stats, void* stream) {
  int rc = check_sharded_cluster_args(h, "cluster", mode, n_labelled, d_labels);
  if (rc) return rc;
  if (stats) *stats = vc_cluster_stats{0, 0};
  if (h->n == 0) return VC_OK;
  return sharded_store_call(h, mode, sharded_caller_stream(h, stream), [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_cluster_run(v, radius, batch, n_labelled, d_labels, stats, S, err);
  });
}

int vc_sharded_cluster_radius(vc_sharded* h, uint32_t radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* labels,
                              vc_cluster_stats* stats) {
  int rc = check_sharded_cluster_args(h, "cluster", mode, n_labelled, labels);
  if (rc) return rc;
  if (stats) *stats = vc_cluster_stats{0, 0};
  if (h->n == 0) return VC_OK;
  return sharded_store_call(h, mode, h->root_stream, [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_cluster_run_host(v, radius, batch, n_labelled, labels, stats, S, err);
  });
}

int vc_sharded_cluster_levels_dev(vc_sharded* h, uint32_t max_radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* d_labels,
                                  vc_levels_stats* stats, void* stream) {
  int rc = check_sharded_levels_args(h, max_radius, mode, n_labelled, d_labels);
  if (rc) return rc;
  if (stats) *stats = vc_levels_stats{};
  if (h->n == 0) return VC_OK;
  return sharded_store_call(h, mode, sharded_caller_stream(h, stream), [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_levels_run(v, max_radius, batch, n_labelled, d_labels, stats, S, err);
  });
}

int vc_sharded_cluster_levels(vc_sharded* h, uint32_t max_radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* labels,
                              vc_levels_stats* stats) {
  int rc = check_sharded_levels_args(h, max_radius, mode, n_labelled, labels);
  if (rc) return rc;
  if (stats) *stats = vc_levels_stats{};
  if (h->n == 0) return VC_OK;
  return sharded_store_call(h, mode, h->root_stream, [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_levels_run_host(v, max_radius, batch, n_labelled, labels, stats, S, err);
  });
}

int vc_sharded_leaders_radius_dev(vc_sharded* h, uint32_t radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* d_labels,
                                  vc_leader_stats* stats, void* stream) {
  int rc = check_sharded_cluster_args(h, "leaders", mode, n_labelled, d_labels);
  if (rc) return rc;
  if (stats) *stats = vc_leader_stats{0, 0, 0};
  if (h->n == 0) return VC_OK;
  return sharded_store_call(h, mode, sharded_caller_stream(h, stream), [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_leaders_run(v, radius, batch, n_labelled, d_labels, stats, S, err);
  });
}

int vc_sharded_leaders_radius(vc_sharded* h, uint32_t radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* labels,
                              vc_leader_stats* stats) {
  int rc = check_sharded_cluster_args(h, "leaders", mode, n_labelled, labels);
  if (rc) return rc;
  if (stats) *stats = vc_leader_stats{0, 0, 0};
  if (h->n == 0) return VC_OK;
  return sharded_store_call(h, mode, h->root_stream, [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_leaders_run_host(v, radius, batch, n_labelled, labels, stats, S, err);
  });
}

int vc_sharded_dbscan_radius_dev(vc_sharded* h, uint32_t radius, uint32_t min_pts, uint32_t mode, uint32_t batch, uint32_t* d_labels,
                                 uint32_t* d_degrees, vc_dbscan_stats* stats, void* stream) {
  int rc = check_sharded_dbscan_args(h, min_pts, mode, d_labels);
  if (rc) return rc;
  if (stats) *stats = vc_dbscan_stats{0, 0, 0, 0, 0};
  if (h->n == 0) return VC_OK;
  return sharded_store_call(h, mode, sharded_caller_stream(h, stream), [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_dbscan_run(v, radius, min_pts, batch, d_labels, d_degrees, stats, S, err);
  });
}

int vc_sharded_dbscan_radius(vc_sharded* h, uint32_t radius, uint32_t min_pts, uint32_t mode, uint32_t batch, uint32_t* labels, uint32_t* degrees,
                             vc_dbscan_stats* stats) {
  int rc = check_sharded_dbscan_args(h, min_pts, mode, labels);
  if (rc) return rc;
  if (stats) *stats = vc_dbscan_stats{0, 0, 0, 0, 0};
  if (h->n == 0) return VC_OK;
  return sharded_store_call(h, mode, h->root_stream, [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_dbscan_run_host(v, radius, min_pts, batch, labels, degrees, stats, S, err);
  });
}

int vc_sharded_dbscan_levels_dev(vc_sharded* h, uint32_t max_radius, uint32_t min_pts, uint32_t mode, uint32_t batch, uint32_t* d_labels,
                                 uint32_t* d_core_dist, vc_dbscan_levels_stats* stats, void* stream) {
  int rc = check_sharded_dbscan_levels_args(h, max_radius, min_pts, mode, d_labels);
  if (rc) return rc;
  if (stats) *stats = vc_dbscan_levels_stats{};
  if (h->n == 0) return VC_OK;
  return sharded_store_call(h, mode, sharded_caller_stream(h, stream), [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_dbscan_levels_run(v, max_radius, min_pts, batch, d_labels, d_core_dist, stats, S, err);
  });
}

int vc_sharded_dbscan_levels(vc_sharded* h, uint32_t max_radius, uint32_t min_pts, uint32_t mode, uint32_t batch, uint32_t* labels, uint32_t* core_dist,
                             vc_dbscan_levels_stats* stats) {
  int rc = check_sharded_dbscan_levels_args(h, max_radius, min_pts, mode, labels);
  if (rc) return rc;
  if (stats) *stats = vc_dbscan_levels_stats{};
  if (h->n == 0) return VC_OK;
  return sharded_store_call(h, mode, h->root_stream, [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_dbscan_levels_run_host(v, max_radius, min_pts, batch, labels, core_dist, stats, S, err);
  });
}

}  // extern "C"

// ---- label groups summarised over the shards: the driver of vc_groups.hip on the root, its rows through the sharded gather ------------
static VcGroupsFetch sharded_groups_fetch(vc_sharded* h, hipStream_t S) {
  return [h, S](const uint32_t* d_ids, uint32_t nq, uint64_t* d_rows) { return vc_sharded_get_codes_dev(h, d_ids, nq, d_rows, nullptr, (void*)S); };
}
static VcGroupsArgs sharded_groups_args(vc_sharded* h, const uint32_t* d_labels, uint64_t groups_cap, vc_group* d_groups, void* d_centroids,
                                        uint32_t* d_rep_labels, uint32_t* d_group_index) {
  return VcGroupsArgs{h->n, h->cfg.engine.id_base, h->nbytes / 8, h->knobs.group_window, d_labels, groups_cap, d_groups, (uint64_t*)d_centroids, d_rep_labels,
                      d_group_index, sharded_scratch_alloc(h)};
}

extern "C" {

int vc_sharded_group_summary_dev(vc_sharded* h, const uint32_t* d_labels, uint64_t groups_cap, vc_group* d_groups, void* d_centroids,
                                 uint32_t* d_rep_labels, uint32_t* d_group_index, uint64_t* n_groups, void* stream) {
  if (!h || (!d_labels && h->n) || (!d_groups && groups_cap)) return VC_ERR_INVALID;
  if (n_groups) *n_groups = 0;
  if (h->n == 0) return VC_OK;
  hipStream_t S = sharded_caller_stream(h, stream);
  VS_HIP(h, hipSetDevice(h->root));
  std::string err;
  const int rc = vc_groups_run(sharded_groups_args(h, d_labels, groups_cap, d_groups, d_centroids, d_rep_labels, d_group_index), sharded_groups_fetch(h, S),
                               n_groups, S, &err);
  return rc && !err.empty() ? sfail(h, rc, "%s", err.c_str()) : rc;
}

int vc_sharded_group_summary(vc_sharded* h, const uint32_t* labels, uint64_t groups_cap, vc_group* groups, void* centroids, uint32_t* rep_labels,
                             uint32_t* group_index, uint64_t* n_groups) {
  if (!h || (!labels && h->n) || (!groups && groups_cap)) return VC_ERR_INVALID;
  if (n_groups) *n_groups = 0;
  if (h->n == 0) return VC_OK;
  hipStream_t S = h->root_stream;
  VS_HIP(h, hipSetDevice(h->root));
  std::string err;
  const int rc = vc_groups_run_host(sharded_groups_args(h, nullptr, groups_cap, nullptr, nullptr, nullptr, nullptr), sharded_groups_fetch(h, S), labels, groups,
                                    centroids, rep_labels, group_index, n_groups, S, &err);
  return rc && !err.empty() ? sfail(h, rc, "%s", err.c_str()) : rc;
}

}  // extern "C"

// ---- nearest of K codes and k-majority over the shards: vc_assign.hip's driver on the root, the assign step on every shard's device ----
static int check_sharded_assign_args(vc_sharded* h, const void* centres, uint32_t n_centres, uint64_t first, uint64_t count, const uint64_t* out) {
  if (!h || !centres || n_centres == 0 || first > h->n || count > h->n - first || (!out && count)) return VC_ERR_INVALID;
  return VC_OK;
}
static int check_sharded_kmajority_args(vc_sharded* h, uint32_t n_centres, uint32_t max_iters, const void* centres, const uint64_t* assign) {
  if (!h || !centres || !assign || n_centres == 0 || (h->n && n_centres > h->n) || max_iters > VC_KMAJ_MAX_ITERS) return VC_ERR_INVALID;
  return VC_OK;
}

// d_centres / d_out on the root device, valid on S; count > 0.  All enqueued, nothing waited for: the centres reach every other lane
// by one peer copy behind ev_q, every non-empty shard assigns the part of [first, first + count) it owns on its own device -- a
// root-device shard straight into d_out, a remote one into its lane's buffer, which one peer copy per shard brings to the root behind
// the lane's `done` event.  Returns with the root device current.
static int sharded_assign_range(vc_sharded* h, const uint64_t* d_centres, uint32_t K, uint64_t first, uint64_t count, uint64_t* d_out, hipStream_t S) {
  const size_t cbytes = (size_t)K * h->nbytes;
  const uint64_t last = first + count;
  auto part = [&](uint32_t g, uint64_t* a, uint64_t* b) {   // the store ordinals [a, b) of the range that shard g holds
    *a = std::max(first, h->lo[g]);
    *b = std::min(last, h->lo[g] + shard_size(h, g));
    return *a < *b;
  };
  int rc;
  bool remote = false;
  for (uint32_t li = 0; li < h->lanes.size(); ++li) {
    if (li == h->root_lane) continue;
    Lane& l = h->lanes[li];
    uint64_t words = 0, a, b;
    for (uint32_t g : l.shards)
      if (part(g, &a, &b)) words += b - a;
    if (!words) continue;
    remote = true;
    VS_HIP(h, hipSetDevice(l.dev));
    if ((rc = grow(h, l.buf[LANE_ACENT], cbytes)) || (rc = grow(h, l.buf[LANE_AOUT], (size_t)words * 8))) return rc;
  }
  VS_HIP(h, hipSetDevice(h->root));
  if (remote) VS_HIP(h, hipEventRecord(h->ev_q, S));
  for (uint32_t li = 0; li < h->lanes.size(); ++li) {
    Lane& l = h->lanes[li];
    const bool is_root = li == h->root_lane;
    hipStream_t ls = is_root ? S : l.stream;
    uint64_t at = 0, a, b;
    bool any = false;
    for (uint32_t g : l.shards) {
      if (!part(g, &a, &b)) continue;
      if (!is_root && !any) {
        VS_HIP(h, hipSetDevice(l.dev));
        VS_HIP(h, hipStreamWaitEvent(ls, h->ev_q, 0));   // also orders the lane behind the previous call's copies out of its buffers
        VS_HIP(h, hipMemcpyPeerAsync(l.buf[LANE_ACENT].p, l.dev, d_centres, h->root, cbytes, ls));
      }
      any = true;
      uint64_t* dst = is_root ? d_out + (a - first) : l.buf[LANE_AOUT].as<uint64_t>() + at;
      if ((rc = vc_assign_nearest_dev(h->eng[g], is_root ? (const void*)d_centres : l.buf[LANE_ACENT].p, K, a - h->lo[g], b - a, dst, ls)))
        return sfail(h, rc, "shard %u: %s", g, vc_last_error(h->eng[g]));
      at += b - a;
    }
    if (!is_root && any) {
      VS_HIP(h, hipSetDevice(l.dev));
      VS_HIP(h, hipEventRecord(l.done, ls));
    }
  }
  VS_HIP(h, hipSetDevice(h->root));
  for (uint32_t li = 0; li < h->lanes.size(); ++li) {
    if (li == h->root_lane) continue;
    Lane& l = h->lanes[li];
    uint64_t at = 0, a, b;
    bool any = false;
    for (uint32_t g : l.shards) {
      if (!part(g, &a, &b)) continue;
      if (!any) VS_HIP(h, hipStreamWaitEvent(S, l.done, 0));
      any = true;
      VS_HIP(h, hipMemcpyPeerAsync(d_out + (a - first), h->root, l.buf[LANE_AOUT].as<uint64_t>() + at, l.dev, (size_t)(b - a) * 8, S));
      at += b - a;
    }
  }
  return VC_OK;
}
static VcAssignAll sharded_assign_all(vc_sharded* h, uint32_t K, uint64_t first, uint64_t count, hipStream_t S) {
  return [h, K, first, count, S](const uint64_t* d_centres, uint64_t* d_out) { return sharded_assign_range(h, d_centres, K, first, count, d_out, S); };
}

extern "C" {

int vc_sharded_assign_nearest_dev(vc_sharded* h, const void* d_centres, uint32_t n_centres, uint64_t first, uint64_t count, uint64_t* d_out,
                                  void* stream) {
  const int rc = check_sharded_assign_args(h, d_centres, n_centres, first, count, d_out);
  if (rc || count == 0) return rc;
  return sharded_assign_range(h, (const uint64_t*)d_centres, n_centres, first, count, d_out, sharded_caller_stream(h, stream));
}

int vc_sharded_assign_nearest(vc_sharded* h, const void* centres, uint32_t n_centres, uint64_t first, uint64_t count, uint64_t* out) {
  int rc = check_sharded_assign_args(h, centres, n_centres, first, count, out);
  if (rc || count == 0) return rc;
  hipStream_t S = h->root_stream;
  VS_HIP(h, hipSetDevice(h->root));
  std::string err;
  rc = vc_assign_run_host(sharded_scratch_alloc(h), h->nbytes / 8, centres, n_centres, count, out, sharded_assign_all(h, n_centres, first, count, S), S, &err);
  return rc && !err.empty() ? sfail(h, rc, "%s", err.c_str()) : rc;
}

int vc_sharded_kmajority_dev(vc_sharded* h, uint32_t n_centres, uint32_t max_iters, void* d_centres, uint64_t* d_assign, uint32_t* d_labels,
                             vc_kmajority_stats* stats, void* stream) {
  int rc = check_sharded_kmajority_args(h, n_centres, max_iters, d_centres, d_assign);
  if (rc) return rc;
  if (stats) *stats = vc_kmajority_stats{};
  if (h->n == 0) return VC_OK;
  hipStream_t S = sharded_caller_stream(h, stream);
  VS_HIP(h, hipSetDevice(h->root));
  std::string err;
  rc = vc_kmajority_run(VcKmajArgs{n_centres, max_iters, (uint64_t*)d_centres, d_assign, d_labels, sharded_scratch_alloc(h)},
                        sharded_groups_args(h, nullptr, 0, nullptr, nullptr, nullptr, nullptr), sharded_assign_all(h, n_centres, 0, h->n, S),
                        sharded_groups_fetch(h, S), stats, S, &err);
  return rc && !err.empty() ? sfail(h, rc, "%s", err.c_str()) : rc;
}

int vc_sharded_kmajority(vc_sharded* h, uint32_t n_centres, uint32_t max_iters, void* centres, uint64_t* assign, uint32_t* labels,
                         vc_kmajority_stats* stats) {
  int rc = check_sharded_kmajority_args(h, n_centres, max_iters, centres, assign);
  if (rc) return rc;
  if (stats) *stats = vc_kmajority_stats{};
  if (h->n == 0) return VC_OK;
  hipStream_t S = h->root_stream;
  VS_HIP(h, hipSetDevice(h->root));
  std::string err;
  rc = vc_kmajority_run_host(VcKmajArgs{n_centres, max_iters, nullptr, nullptr, nullptr, sharded_scratch_alloc(h)},
                             sharded_groups_args(h, nullptr, 0, nullptr, nullptr, nullptr, nullptr), sharded_assign_all(h, n_centres, 0, h->n, S),
                             sharded_groups_fetch(h, S), centres, assign, labels, stats, S, &err);
  return rc && !err.empty() ? sfail(h, rc, "%s", err.c_str()) : rc;
}

}  // extern "C"

// ---- device-side seeding over the shards: vc_seed.hip's kernels on every shard's device, the pick decided on the root ---------------------
static int check_sharded_seed_args(vc_sharded* h, uint32_t n_centres, uint32_t method, const void* centres) {
  if (!h || !centres || n_centres == 0 || (h->n && n_centres > h->n) || (method != VC_SEED_FARTHEST && method != VC_SEED_WEIGHTED)) return VC_ERR_INVALID;
  return VC_OK;
}

namespace {
// what a non-empty shard brings to a seeding call; words[0] = its slot word, words[1] = its total, both on its device
struct SeedShard {
  uint32_t g, lane;
  VcEngineView v;
  uint64_t* words;
  uint32_t* partial;
  uint64_t* best;          // a root-device shard: its part of the root's best; else inside its lane's LANE_SBEST
  const uint64_t* code;    // the round's centre code on its device
  hipStream_t ls;
};
}  // namespace

// THE ROUNDS over the shards (the header states the rule and the waits).  All pointers on the root device, valid on S; N > 0.  The
// root keeps the picks on the host: per round it fetches the chosen record's code into centres[t] (sharded_gather_ids), every
// non-empty shard runs the round launch with that code -- on S for a root-device shard, on its lane's stream behind ev_q and a peer
// copy of the code for a remote one -- and sends its slot word and total home; the root waits for them and decides.  Returns with
// the root device current.
static int sharded_seed_run(vc_sharded* h, uint32_t K, uint32_t method, uint64_t seed, uint64_t* d_centres, uint64_t* d_picks, uint64_t* d_assign,
                            vc_seed_stats* stats, hipStream_t S) {
  const uint32_t W = h->nbytes / 8, id_base = h->cfg.engine.id_base;
  const uint64_t N = h->n;
  int rc;
  VS_HIP(h, hipSetDevice(h->root));
  DevBuf& rb = h->buf[SCRATCH + VC_SEED_WORK];   // the id word | the two statistics words | best [N] unless d_assign holds it
  if ((rc = grow(h, rb, 24 + (d_assign ? 0 : (size_t)N * 8)))) return rc;
  uint32_t* d_id = rb.as<uint32_t>();
  uint64_t* d_stat = rb.as<uint64_t>() + 1;
  uint64_t* best = d_assign ? d_assign : rb.as<uint64_t>() + 3;
  std::vector<SeedShard> sh;
  bool remote = false;
  for (uint32_t li = 0; li < h->lanes.size(); ++li) {
    Lane& l = h->lanes[li];
    const bool is_root = li == h->root_lane;
    uint64_t words = 0, recs = 0;
    for (uint32_t g : l.shards) {
      if (shard_size(h, g) == 0) continue;
      words += 2 + (vc_seed_blocks(shard_size(h, g)) + 1) / 2;
      recs += shard_size(h, g);
    }
    if (!words) continue;
    VS_HIP(h, hipSetDevice(l.dev));
    if ((rc = grow(h, l.buf[LANE_SWORK], (size_t)words * 8))) return rc;
    if (!is_root && ((rc = grow(h, l.buf[LANE_SCODE], (size_t)W * 8)) || (rc = grow(h, l.buf[LANE_SBEST], (size_t)recs * 8)))) return rc;
    remote |= !is_root;
    uint64_t at_w = 0, at_r = 0;
    for (uint32_t g : l.shards) {
      if (shard_size(h, g) == 0) continue;
      SeedShard x;
      x.g = g;
      x.lane = li;
      if ((rc = vc_engine_view(h->eng[g], &x.v))) return sfail(h, rc, "shard %u: no view", g);
      x.words = l.buf[LANE_SWORK].as<uint64_t>() + at_w;
      x.partial = (uint32_t*)(x.words + 2);
      x.best = is_root ? best + h->lo[g] : l.buf[LANE_SBEST].as<uint64_t>() + at_r;
      x.code = is_root ? nullptr : l.buf[LANE_SCODE].as<uint64_t>();
      x.ls = is_root ? S : l.stream;
      at_w += 2 + (vc_seed_blocks(x.v.n) + 1) / 2;
      at_r += x.v.n;
      sh.push_back(x);
    }
  }
  std::vector<uint64_t> picks(K), home(2 * (size_t)h->G, 0), totals(h->G, 0);
  std::vector<uint32_t> ids(K);
  uint64_t s = vc_seed_draw(seed, 0) % N;
  uint32_t pick_dist = 0, n_zero = 0;
  auto wait_lanes = [&]() -> hipError_t {   // every stream a shard of this call works on
    hipError_t r = hipSuccess;
    for (size_t j = 0; j < sh.size() && r == hipSuccess; ++j) {
      if (j && sh[j].lane == sh[j - 1].lane) continue;
      if ((r = hipSetDevice(h->lanes[sh[j].lane].dev)) == hipSuccess) r = hipStreamSynchronize(sh[j].ls);
    }
    return r;
  };
  for (uint32_t t = 0; t < K; ++t) {
    const bool last = t + 1 == K;
    ids[t] = id_base + (uint32_t)s;
    picks[t] = vc_pack(pick_dist, ids[t]);
    n_zero += t >= 1 && pick_dist == 0 ? 1u : 0u;
    uint64_t* d_code = d_centres + (uint64_t)t * W;
    VS_HIP(h, hipSetDevice(h->root));
    VS_HIP(h, hipMemcpyAsync(d_id, &ids[t], 4, hipMemcpyHostToDevice, S));
    if ((rc = sharded_gather_ids(h, d_id, 1, d_code, nullptr, false, S))) return rc;
    VS_HIP(h, hipSetDevice(h->root));
    if (remote) VS_HIP(h, hipEventRecord(h->ev_q, S));
    for (size_t j = 0; j < sh.size(); ++j) {
      SeedShard& x = sh[j];
      Lane& l = h->lanes[x.lane];
      VS_HIP(h, hipSetDevice(l.dev));
      if (x.code && (j == 0 || sh[j - 1].lane != x.lane)) {
        VS_HIP(h, hipStreamWaitEvent(x.ls, h->ev_q, 0));
        VS_HIP(h, hipMemcpyPeerAsync(l.buf[LANE_SCODE].p, l.dev, d_code, h->root, (size_t)W * 8, x.ls));
      }
      const bool farthest = method == VC_SEED_FARTHEST;
      if (!last) VS_HIP(h, hipMemsetAsync(x.words, 0, 16, x.ls));
      VcSeedRound r{};   // (a shard's slot is one word: it has few blocks next to the wait that follows)
      r.cols = x.v.cols; r.stride = x.v.stride; r.n = x.v.n; r.W = W; r.t = t; r.method = method;
      r.d_code = x.code ? x.code : d_code;
      r.d_best = x.best;
      r.d_slot_next = !last && farthest ? x.words : nullptr;
      r.n_slot_next = 1;
      r.d_partial = !last && !farthest ? x.partial : nullptr;
      VS_HIP(h, vc_launch_seed_round(r, x.ls));
      if (last) continue;
      if (!farthest) VS_HIP(h, vc_launch_seed_pick(x.partial, x.best, x.v.n, 0, nullptr, x.words + 1, x.ls));
      VS_HIP(h, hipMemcpyAsync(&home[2 * (size_t)x.g], x.words, 16, hipMemcpyDeviceToHost, x.ls));
    }
    if (last) break;
    VS_HIP(h, wait_lanes());   // the round's wait
    if (method == VC_SEED_FARTHEST) {
      uint64_t top = 0;   // the maximum over the shards of the slot word in store ordinals: the rule itself
      for (const SeedShard& x : sh) {
        const uint64_t w = home[2 * (size_t)x.g];
        const uint64_t i = h->lo[x.g] + vc_seed_slot_index(w);
        if (i < N) top = std::max(top, vc_seed_slot(vc_seed_slot_dist(w), (uint32_t)i));
      }
      s = vc_seed_slot_index(top);
      pick_dist = vc_seed_slot_dist(top);
      if (s >= N) return sfail(h, VC_ERR_HIP, "seeding: no shard reported a record in round %u", t);
    } else {
      uint64_t total = 0, before = 0;
      for (const SeedShard& x : sh) total += totals[x.g] = home[2 * (size_t)x.g + 1];
      s = 0;
      pick_dist = 0;
      if (total) {
        const uint64_t target = vc_seed_draw(seed, (uint64_t)t + 1) % total;
        const uint64_t g = vc_seed_find(totals.data(), (uint64_t)h->G, target, &before, VcSeedWeightPlain());
        const SeedShard* own = nullptr;
        for (const SeedShard& x : sh)
          if (x.g == g) own = &x;
        if (!own) return sfail(h, VC_ERR_HIP, "seeding: the shards' totals do not reach the target in round %u", t);
        VS_HIP(h, hipSetDevice(h->lanes[own->lane].dev));
        VS_HIP(h, vc_launch_seed_pick(own->partial, own->best, own->v.n, target - before, own->words, nullptr, own->ls));   // (the rest is below the shard's total)
        VS_HIP(h, hipMemcpyAsync(&home[2 * (size_t)own->g], own->words, 8, hipMemcpyDeviceToHost, own->ls));
        VS_HIP(h, hipStreamSynchronize(own->ls));   // the round's second wait
        const uint64_t w = home[2 * (size_t)own->g];
        s = h->lo[own->g] + vc_seed_slot_index(w);
        pick_dist = vc_seed_slot_dist(w);
        if (s >= N) return sfail(h, VC_ERR_HIP, "seeding: shard %u reported no record in round %u", own->g, t);
      }
    }
  }
  // best of the remote shards comes to the root behind their lanes' events
  for (size_t j = 0; j < sh.size(); ++j) {
    if (!sh[j].code || (j + 1 < sh.size() && sh[j + 1].lane == sh[j].lane)) continue;
    VS_HIP(h, hipSetDevice(h->lanes[sh[j].lane].dev));
    VS_HIP(h, hipEventRecord(h->lanes[sh[j].lane].done, sh[j].ls));
  }
  VS_HIP(h, hipSetDevice(h->root));
  for (size_t j = 0; j < sh.size(); ++j) {
    const SeedShard& x = sh[j];
    if (!x.code) continue;
    Lane& l = h->lanes[x.lane];
    if (j == 0 || sh[j - 1].lane != x.lane) VS_HIP(h, hipStreamWaitEvent(S, l.done, 0));
    VS_HIP(h, hipMemcpyPeerAsync(best + h->lo[x.g], h->root, x.best, l.dev, (size_t)x.v.n * 8, S));
  }
  if (d_picks) VS_HIP(h, hipMemcpyAsync(d_picks, picks.data(), (size_t)K * 8, hipMemcpyHostToDevice, S));
  vc_seed_stats st{};
  if (stats) {
    VS_HIP(h, hipMemsetAsync(d_stat, 0, 16, S));
    VS_HIP(h, vc_launch_seed_finish(best, N, nullptr, K, d_stat, S));
    VS_HIP(h, hipMemcpyAsync(&st, d_stat, sizeof st, hipMemcpyDeviceToHost, S));
  }
  VS_HIP(h, hipStreamSynchronize(S));   // the last wait: the picks leave the host, the statistics arrive
  if (stats) {
    st.n_zero_picks = n_zero;
    *stats = st;
  }
  return VC_OK;
}

extern "C" {

int vc_sharded_seed_centres_dev(vc_sharded* h, uint32_t n_centres, uint32_t method, uint64_t seed, void* d_centres, uint64_t* d_picks,
                                uint64_t* d_assign, vc_seed_stats* stats, void* stream) {
  const int rc = check_sharded_seed_args(h, n_centres, method, d_centres);
  if (rc) return rc;
  if (stats) *stats = vc_seed_stats{};
  if (h->n == 0) return VC_OK;
  return sharded_seed_run(h, n_centres, method, seed, (uint64_t*)d_centres, d_picks, d_assign, stats, sharded_caller_stream(h, stream));
}

int vc_sharded_seed_centres(vc_sharded* h, uint32_t n_centres, uint32_t method, uint64_t seed, void* centres, uint64_t* picks, uint64_t* assign,
                            vc_seed_stats* stats) {
  int rc = check_sharded_seed_args(h, n_centres, method, centres);
  if (rc) return rc;
  if (stats) *stats = vc_seed_stats{};
  if (h->n == 0) return VC_OK;
  hipStream_t S = h->root_stream;
  VS_HIP(h, hipSetDevice(h->root));
  std::string err;
  rc = vc_seed_run_host(VcSeedHostArgs{h->n, h->nbytes / 8, n_centres, centres, picks, assign, stats, sharded_scratch_alloc(h)},
                        [&](uint64_t* d_centres, uint64_t* d_picks, uint64_t* d_assign, vc_seed_stats* st) {
                          return sharded_seed_run(h, n_centres, method, seed, d_centres, d_picks, d_assign, st, S);
                        },
                        S, &err);
  return rc && !err.empty() ? sfail(h, rc, "%s", err.c_str()) : rc;
}

}  // extern "C"

// ---- one result per label group over the shards: vc_distinct.hip's driver on the root over the merged rows of the store's own search --------
static int check_sharded_distinct_args(vc_sharded* h, const void* q, uint32_t nq, uint32_t k, uint32_t mode, const uint32_t* labels, uint32_t k_first,
                                       const uint64_t* out) {
  if (!h || !q || !labels || !out || nq == 0 || k == 0 || k > VC_MAX_K) return VC_ERR_INVALID;
  if (!vc_distinct_k_first_ok(k, k_first)) return sfail(h, VC_ERR_INVALID, "k_first must be 0 or in k..%u", VC_MAX_K);
  if (mode != VC_MODE_LINEAR && mode != VC_MODE_MIH_EXACT) return sfail(h, VC_ERR_INVALID, "distinct search: mode must be LINEAR or MIH_EXACT");
  return check_sharded_index(h, mode);
}
// All pointers on the root device, valid on S: the merged rows of the store's search are collapsed where the caller's labels live
static int sharded_distinct_run(vc_sharded* h, const uint64_t* d_queries, uint32_t nq, uint32_t k, uint32_t mode, const uint32_t* d_labels, uint32_t k_first,
                                uint64_t* d_out, uint32_t* d_row_labels, uint32_t* d_counts, vc_distinct_stats* stats, hipStream_t S) {
  VS_HIP(h, hipSetDevice(h->root));
  std::string err;
  const int rc = vc_distinct_run(VcDistinctArgs{h->n, h->cfg.engine.id_base, h->nbytes / 8, d_queries, nq, k, k_first, d_labels, d_out, d_row_labels, d_counts,
                                                h->knobs.distinct_scratch, mode == VC_MODE_MIH_EXACT, sharded_scratch_alloc(h)},
                                 sharded_store_view(h, mode, S).knn,
                                 stats, S, &err);
  return rc && !err.empty() ? sfail(h, rc, "%s", err.c_str()) : rc;
}

extern "C" {

int vc_sharded_search_knn_distinct_dev(vc_sharded* h, const void* d_queries, uint32_t nq, uint32_t k, uint32_t mode, const uint32_t* d_labels,
                                       uint32_t k_first, uint64_t* d_out, uint32_t* d_row_labels, uint32_t* d_counts, vc_distinct_stats* stats, void* stream) {
  const int rc = check_sharded_distinct_args(h, d_queries, nq, k, mode, d_labels, k_first, d_out);
  if (rc) return rc;
  return sharded_distinct_run(h, (const uint64_t*)d_queries, nq, k, mode, d_labels, k_first, d_out, d_row_labels, d_counts, stats,
                              sharded_caller_stream(h, stream));
}

int vc_sharded_search_knn_distinct(vc_sharded* h, const void* queries, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order, const uint32_t* labels,
                                   uint32_t k_first, uint64_t* out, uint32_t* row_labels, uint32_t* counts, vc_distinct_stats* stats) {
  int rc = check_sharded_distinct_args(h, queries, nq, k, mode, labels, k_first, out);
  if (rc) return rc;
  if (order > VC_ORDER_FARTHEST_FIRST) return VC_ERR_INVALID;
  hipStream_t S = h->root_stream;
  VS_HIP(h, hipSetDevice(h->root));
  std::string err;
  rc = vc_distinct_run_host(VcDistinctHostArgs{h->n, h->nbytes / 8, nq, k, order, queries, labels, out, row_labels, counts, stats, sharded_scratch_alloc(h)},
                            [&](const uint64_t* d_q, const uint32_t* d_labels, uint64_t* d_out, uint32_t* d_rl, uint32_t* d_cnt, vc_distinct_stats* st) {
                              return sharded_distinct_run(h, d_q, nq, k, mode, d_labels, k_first, d_out, d_rl, d_cnt, st, S);
                            },
                            S, &err);
  return rc && !err.empty() ? sfail(h, rc, "%s", err.c_str()) : rc;
}

}  // extern "C"

// ---- k-NN among the allowed records over the shards: vc_filter.hip's driver on the root, the shards behind the view's knn and gather --------
static int check_sharded_filter_args(vc_sharded* h, const void* q, uint32_t nq, uint32_t k, uint32_t mode, const uint32_t* sel, uint32_t kind, uint32_t k_first,
                                     const uint64_t* out) {
  if (!h || !q || !sel || !out || nq == 0 || k == 0 || k > VC_MAX_K) return VC_ERR_INVALID;
  if (!vc_distinct_k_first_ok(k, k_first)) return sfail(h, VC_ERR_INVALID, "k_first must be 0 or in k..%u", VC_MAX_K);
  if (kind >= VC_FILTER_KINDS) return sfail(h, VC_ERR_INVALID, "filtered search: unknown kind %u", kind);
  if (mode != VC_MODE_LINEAR && mode != VC_MODE_MIH_EXACT) return sfail(h, VC_ERR_INVALID, "filtered search: mode must be LINEAR or MIH_EXACT");
  const uint32_t f = h->cfg.engine.flags;
  if (mode == VC_MODE_MIH_EXACT && ((f & VC_FLAG_REF_SIGNEXT_KEYS) || ((f & VC_FLAG_REF_STOP_LITERAL4) && h->cfg.engine.n_tables < 4)))
    return sfail(h, VC_ERR_INVALID, "filtered search: MIH_EXACT rows are not the true nearest records under this store's reference flags");
  return check_sharded_index(h, mode);
}
static VcFilterArgs sharded_filter_args(vc_sharded* h, const uint64_t* d_queries, uint32_t nq, uint32_t k, uint32_t mode, const uint32_t* d_sel, uint32_t kind,
                                        uint32_t value, uint32_t k_first, uint64_t* d_out, uint32_t* d_counts) {
  return VcFilterArgs{d_queries, nq, k, k_first, d_sel, kind, value, h->nbytes * 8u, d_out, d_counts, h->knobs.filter_scratch, h->knobs.filter_window,
                      h->knobs.filter_route, mode == VC_MODE_MIH_EXACT};
}

extern "C" {

int vc_sharded_search_knn_filtered_dev(vc_sharded* h, const void* d_queries, uint32_t nq, uint32_t k, uint32_t mode, const uint32_t* d_sel, uint32_t kind,
                                       uint32_t value, uint32_t k_first, uint64_t* d_out, uint32_t* d_counts, vc_filter_stats* stats, void* stream) {
  const int rc = check_sharded_filter_args(h, d_queries, nq, k, mode, d_sel, kind, k_first, d_out);
  if (rc) return rc;
  return sharded_store_call(h, mode, sharded_caller_stream(h, stream), [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_filter_run(v, sharded_filter_args(h, (const uint64_t*)d_queries, nq, k, mode, d_sel, kind, value, k_first, d_out, d_counts), stats, S, err);
  });
}

int vc_sharded_search_knn_filtered(vc_sharded* h, const void* queries, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order, const uint32_t* sel, uint32_t kind,
                                   uint32_t value, uint32_t k_first, uint64_t* out, uint32_t* counts, vc_filter_stats* stats) {
  const int rc = check_sharded_filter_args(h, queries, nq, k, mode, sel, kind, k_first, out);
  if (rc) return rc;
  if (order > VC_ORDER_FARTHEST_FIRST) return VC_ERR_INVALID;
  return sharded_store_call(h, mode, h->root_stream, [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_filter_run_host(v, VcFilterHostArgs{nq, k, order, kind, queries, sel, out, counts},
                              [&](const uint64_t* d_q, const uint32_t* d_sel, uint64_t* d_out, uint32_t* d_cnt) {
                                return vc_filter_run(v, sharded_filter_args(h, d_q, nq, k, mode, d_sel, kind, value, k_first, d_out, d_cnt), stats, S, err);
                              },
                              S, err);
  });
}

}  // extern "C"

// ---- k-NN inside each query's own scope over the shards: vc_scope.hip's driver on the root, the shards behind the view's gather -------------
static int check_sharded_scope_args(vc_sharded* h, const void* q, uint32_t nq, uint32_t k, const uint32_t* scope, const uint32_t* qscope, uint32_t flags,
                                    const uint64_t* out) {
  if (!h || !q || !scope || !qscope || !out || nq == 0 || k == 0 || k > VC_MAX_K) return VC_ERR_INVALID;
  if (flags) return sfail(h, VC_ERR_INVALID, "scoped search: flags is reserved and must be 0");
  return VC_OK;
}
static VcScopeArgs sharded_scope_args(vc_sharded* h, const uint64_t* d_queries, uint32_t nq, uint32_t k, const uint32_t* d_scope, const uint32_t* d_qscope,
                                      uint64_t* d_out, uint32_t* d_counts) {
  return VcScopeArgs{d_queries, nq, k, d_scope, d_qscope, h->nbytes * 8u, d_out, d_counts, h->knobs.scope_scratch, h->knobs.scope_window};
}

extern "C" {

int vc_sharded_search_knn_scoped_dev(vc_sharded* h, const void* d_queries, uint32_t nq, uint32_t k, const uint32_t* d_scope, const uint32_t* d_qscope,
                                     uint32_t flags, uint64_t* d_out, uint32_t* d_counts, vc_scope_stats* stats, void* stream) {
  const int rc = check_sharded_scope_args(h, d_queries, nq, k, d_scope, d_qscope, flags, d_out);
  if (rc) return rc;
  return sharded_store_call(h, VC_MODE_LINEAR, sharded_caller_stream(h, stream), [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_scope_run(v, sharded_scope_args(h, (const uint64_t*)d_queries, nq, k, d_scope, d_qscope, d_out, d_counts), stats, S, err);
  });
}

int vc_sharded_search_knn_scoped(vc_sharded* h, const void* queries, uint32_t nq, uint32_t k, uint32_t order, const uint32_t* scope, const uint32_t* qscope,
                                 uint32_t flags, uint64_t* out, uint32_t* counts, vc_scope_stats* stats) {
  const int rc = check_sharded_scope_args(h, queries, nq, k, scope, qscope, flags, out);
  if (rc) return rc;
  if (order > VC_ORDER_FARTHEST_FIRST) return VC_ERR_INVALID;
  return sharded_store_call(h, VC_MODE_LINEAR, h->root_stream, [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_scope_run_host(v, VcScopeHostArgs{nq, k, order, queries, scope, qscope, out, counts},
                             [&](const uint64_t* d_q, const uint32_t* d_scope, const uint32_t* d_qscope, uint64_t* d_out, uint32_t* d_cnt) {
                               return vc_scope_run(v, sharded_scope_args(h, d_q, nq, k, d_scope, d_qscope, d_out, d_cnt), stats, S, err);
                             },
                             S, err);
  });
}

}  // extern "C"

// ---- the exact k-NN graph over the shards and its components: vc_knn_graph.hip's drivers on the root, the shards behind the view's knn and gather ----
static int check_sharded_kgraph_args(vc_sharded* h, uint32_t k, uint32_t mode, uint64_t first, uint64_t count, uint32_t k_first, const uint64_t* rows,
                                     uint64_t* n_rows) {
  if (!h || !rows) return VC_ERR_INVALID;
  if (!vc_kgraph_k_ok(k)) return sfail(h, VC_ERR_INVALID, "k-NN graph: k must be in 1..%u", VC_MAX_K - 1);
  if (!vc_kgraph_k_first_ok(k, k_first)) return sfail(h, VC_ERR_INVALID, "k-NN graph: k_first must be 0 or in k+1..%u", VC_MAX_K);
  if (mode != VC_MODE_LINEAR && mode != VC_MODE_MIH_EXACT) return sfail(h, VC_ERR_INVALID, "k-NN graph: mode must be LINEAR or MIH_EXACT");
  if (!vc_kgraph_range(h->n, first, count, n_rows))
    return sfail(h, VC_ERR_INVALID, "k-NN graph: first %llu + count %llu exceeds the %llu resident records", (unsigned long long)first, (unsigned long long)count,
                 (unsigned long long)h->n);
  return check_sharded_index(h, mode);
}
static VcKgraphArgs sharded_kgraph_args(vc_sharded* h, uint32_t k, uint32_t mode, uint32_t batch, uint64_t first, uint64_t n_rows, uint32_t k_first,
                                        uint64_t* d_rows, uint32_t* d_counts) {
  return VcKgraphArgs{k, k_first, batch, mode == VC_MODE_LINEAR, first, n_rows, d_rows, d_counts, h->knobs.kgraph_scratch};
}
static int check_sharded_cluster_knn_args(vc_sharded* h, const uint64_t* rows, uint32_t k, uint32_t kk, uint32_t flags, const uint32_t* labels) {
  if (!h || !rows || !labels) return VC_ERR_INVALID;
  if (!vc_kgraph_k_ok(k)) return sfail(h, VC_ERR_INVALID, "k-NN clusters: k must be in 1..%u", VC_MAX_K - 1);
  if (kk == 0 || kk > k) return sfail(h, VC_ERR_INVALID, "k-NN clusters: kk must be in 1..k");
  if (flags & ~VC_KNN_EITHER) return sfail(h, VC_ERR_INVALID, "k-NN clusters: unknown flags 0x%x", flags);
  return VC_OK;
}
static int check_sharded_cluster_snn_args(vc_sharded* h, const uint64_t* rows, uint32_t k, uint32_t kk, uint32_t flags, const uint32_t* labels) {
  if (!h || !rows || !labels) return VC_ERR_INVALID;
  if (!vc_kgraph_k_ok(k)) return sfail(h, VC_ERR_INVALID, "SNN clusters: k must be in 1..%u", VC_MAX_K - 1);
  if (!vc_snn_kk_ok(k, kk)) return sfail(h, VC_ERR_INVALID, "SNN clusters: kk must be in 1..min(k, %u)", VC_SNN_MAX_KK);
  if (!vc_snn_flags_ok(flags)) return sfail(h, VC_ERR_INVALID, "SNN clusters: unknown flags 0x%x", flags);
  return VC_OK;
}
static int check_sharded_knn_adjacency_args(vc_sharded* h, const uint64_t* rows, uint32_t k, uint32_t kk, uint32_t flags, const uint64_t* adj, uint64_t adj_cap,
                                            const uint64_t* offsets) {
  if (!h || !rows || !offsets || (!adj && adj_cap)) return VC_ERR_INVALID;
  if (!vc_kgraph_k_ok(k)) return sfail(h, VC_ERR_INVALID, "k-NN adjacency: k must be in 1..%u", VC_MAX_K - 1);
  if (!vc_adj_kk_ok(k, kk)) return sfail(h, VC_ERR_INVALID, "k-NN adjacency: kk must be in 1..k");
  if (!vc_adj_flags_ok(flags)) return sfail(h, VC_ERR_INVALID, "k-NN adjacency: unknown flags 0x%x", flags);
  if (!vc_adj_items_ok(h->n, kk)) return sfail(h, VC_ERR_INVALID, "k-NN adjacency: N * kk must not exceed 2^31 - 1");
  return VC_OK;
}
static int check_sharded_knn_mst_args(vc_sharded* h, const uint64_t* rows, uint32_t k, uint32_t kk, uint32_t flags, uint32_t weight_kind, uint32_t min_pts,
                                      const vc_mst_edge* edges) {
  if (!h || !rows || !edges) return VC_ERR_INVALID;
  if (!vc_kgraph_k_ok(k)) return sfail(h, VC_ERR_INVALID, "k-NN spanning forest: k must be in 1..%u", VC_MAX_K - 1);
  if (!vc_mst_kk_ok(k, kk)) return sfail(h, VC_ERR_INVALID, "k-NN spanning forest: kk must be in 1..k");
  if (!vc_mst_flags_ok(flags)) return sfail(h, VC_ERR_INVALID, "k-NN spanning forest: flags must be VC_KNN_MUTUAL or VC_KNN_EITHER, not 0x%x", flags);
  if (!vc_mst_kind_ok(weight_kind)) return sfail(h, VC_ERR_INVALID, "k-NN spanning forest: unknown weight_kind %u", weight_kind);
  if (!vc_mst_min_pts_ok(weight_kind, k, min_pts))
    return sfail(h, VC_ERR_INVALID, "k-NN spanning forest: min_pts must be 1 under VC_MST_DISTANCE and in 1..k+1 under VC_MST_REACHABILITY");
  if (!vc_mst_items_ok(h->n, kk)) return sfail(h, VC_ERR_INVALID, "k-NN spanning forest: N * kk must not exceed 2^31 - 1");
  return VC_OK;
}
static int check_sharded_mst_condense_args(vc_sharded* h, const vc_mst_edge* edges, uint64_t n_edges, uint32_t mcs, uint32_t root_weight, uint32_t method,
                                           const vc_condensed_node* nodes, const uint32_t* labels) {
  if (!h || !labels || !nodes || (!edges && n_edges)) return VC_ERR_INVALID;
  if (!vc_cond_edges_ok(h->n, n_edges)) return sfail(h, VC_ERR_INVALID, "condensed tree: a forest over N records has at most max(N, 1) - 1 edges");
  if (!vc_cond_mcs_ok(mcs)) return sfail(h, VC_ERR_INVALID, "condensed tree: min_cluster_size must be in 2..2^31");
  if (!vc_cond_root_weight_ok(root_weight, (uint32_t)h->nbytes * 8u)) return sfail(h, VC_ERR_INVALID, "condensed tree: root_weight must not exceed bits + 1");
  if (!vc_cond_method_ok(method)) return sfail(h, VC_ERR_INVALID, "condensed tree: unknown method %u", method);
  return VC_OK;
}
static int check_sharded_knn_vote_args(vc_sharded* h, const uint64_t* rows, uint32_t k, uint32_t kk, const uint32_t* labels, uint32_t weight_kind,
                                       const uint32_t* out_label) {
  if (!h || !rows || !labels || !out_label) return VC_ERR_INVALID;
  if (!vc_vote_k_ok(k, VC_MAX_K)) return sfail(h, VC_ERR_INVALID, "label vote: k must be in 1..%u", VC_MAX_K);
  if (!vc_vote_kk_ok(k, kk)) return sfail(h, VC_ERR_INVALID, "label vote: kk must be in 1..k");
  if (!vc_vote_kind_ok(weight_kind)) return sfail(h, VC_ERR_INVALID, "label vote: unknown weight_kind %u", weight_kind);
  return VC_OK;
}
static int check_sharded_label_propagate_args(vc_sharded* h, const uint64_t* offsets, const uint64_t* adj, uint64_t n_entries, const uint32_t* labels_in,
                                              uint32_t weight_kind, uint32_t flags, uint32_t max_iters, const uint32_t* labels_out) {
  if (!h || !offsets || (!adj && n_entries) || !labels_in || !labels_out) return VC_ERR_INVALID;
  if (!vc_vote_kind_ok(weight_kind)) return sfail(h, VC_ERR_INVALID, "label propagation: unknown weight_kind %u", weight_kind);
  if (!vc_vote_lp_flags_ok(flags)) return sfail(h, VC_ERR_INVALID, "label propagation: unknown flags 0x%x", flags);
  if (!vc_vote_iters_ok(max_iters)) return sfail(h, VC_ERR_INVALID, "label propagation: max_iters must be in 1..%u", VC_LP_MAX_ITERS);
  return VC_OK;
}
// a built graph after vc_sharded_add_codes (vc_knn_graph_update.hip): the graph call's checks with n_old as the first position
static int check_sharded_kgupd_args(vc_sharded* h, uint32_t k, uint32_t mode, uint64_t n_old, uint32_t k_first, const uint64_t* rows) {
  uint64_t n_rows = 0;
  if (!h || !rows) return VC_ERR_INVALID;
  if (n_old > h->n)
    return sfail(h, VC_ERR_INVALID, "k-NN graph update: n_old %llu exceeds the %llu resident records", (unsigned long long)n_old, (unsigned long long)h->n);
  return check_sharded_kgraph_args(h, k, mode, n_old, 0, k_first, rows, &n_rows);
}
static VcKgupdArgs sharded_kgupd_args(vc_sharded* h, uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first, uint64_t* d_rows,
                                      uint32_t* d_counts) {
  return VcKgupdArgs{sharded_kgraph_args(h, k, mode, batch, n_old, h->n - n_old, k_first, d_rows ? d_rows + n_old * k : nullptr,
                                         d_counts ? d_counts + n_old : nullptr),
                     n_old, d_rows, d_counts, h->knobs.kgraph_scratch, vc_kgupd_old_batch(h->knobs.kgraph_old_batch), vc_kgupd_window(h->knobs.kgraph_window)};
}
// a built graph after vc_sharded_retain* (vc_knn_graph_retain.hip): the graph call's checks over the store as it is now
static int check_sharded_kgret_args(vc_sharded* h, uint32_t k, uint32_t mode, uint64_t n_old, uint32_t k_first, const uint32_t* new_ids, const uint64_t* rows) {
  uint64_t n_rows = 0;
  if (!h || !rows || !new_ids) return VC_ERR_INVALID;
  const int rc = check_sharded_kgraph_args(h, k, mode, 0, 0, k_first, rows, &n_rows);
  if (rc) return rc;
  if (n_old < h->n)
    return sfail(h, VC_ERR_INVALID, "k-NN graph retain: n_old %llu is below the %llu resident records", (unsigned long long)n_old, (unsigned long long)h->n);
  return VC_OK;
}
static VcKgretArgs sharded_kgret_args(vc_sharded* h, uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first, const uint32_t* d_new_ids,
                                      uint64_t* d_rows, uint32_t* d_counts) {
  return VcKgretArgs{sharded_kgraph_args(h, k, mode, batch, 0, h->n, k_first, d_rows, d_counts), n_old, d_new_ids};
}
static bool sharded_kgret_nothing_to_do(uint64_t K, uint64_t n_old, vc_knn_graph_retain_stats* stats) {
  if (stats) {
    *stats = vc_knn_graph_retain_stats{};
    stats->n_rows_kept = K;
  }
  return K == n_old || K == 0;
}

extern "C" {

int vc_sharded_knn_graph_dev(vc_sharded* h, uint32_t k, uint32_t mode, uint32_t batch, uint64_t first, uint64_t count, uint32_t k_first, uint64_t* d_rows,
                             uint32_t* d_counts, vc_knn_graph_stats* stats, void* stream) {
  uint64_t n_rows = 0;
  const int rc = check_sharded_kgraph_args(h, k, mode, first, count, k_first, d_rows, &n_rows);
  if (rc) return rc;
  if (stats) *stats = vc_knn_graph_stats{};
  if (n_rows == 0) return VC_OK;
  return sharded_store_call(h, mode, sharded_caller_stream(h, stream), [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_knn_graph_run(v, sharded_store_view(h, VC_MODE_LINEAR, S).knn, sharded_kgraph_args(h, k, mode, batch, first, n_rows, k_first, d_rows, d_counts), stats,
                            S, err);
  });
}

int vc_sharded_knn_graph(vc_sharded* h, uint32_t k, uint32_t mode, uint32_t batch, uint64_t first, uint64_t count, uint32_t k_first, uint64_t* rows,
                         uint32_t* counts, vc_knn_graph_stats* stats) {
  uint64_t n_rows = 0;
  const int rc = check_sharded_kgraph_args(h, k, mode, first, count, k_first, rows, &n_rows);
  if (rc) return rc;
  if (stats) *stats = vc_knn_graph_stats{};
  if (n_rows == 0) return VC_OK;
  return sharded_store_call(h, mode, h->root_stream, [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_knn_graph_run_host(v, sharded_kgraph_args(h, k, mode, batch, first, n_rows, k_first, nullptr, nullptr), rows, counts, stats,
                                 [&](uint64_t* d_rows, uint32_t* d_counts, vc_knn_graph_stats* st) {
                                   return vc_knn_graph_run(v, sharded_store_view(h, VC_MODE_LINEAR, S).knn,
                                                           sharded_kgraph_args(h, k, mode, batch, first, n_rows, k_first, d_rows, d_counts), st, S, err);
                                 },
                                 [&](const uint64_t* codes, uint32_t nq, uint64_t* hrows, uint32_t* rcnt) {   // (its shards recover on the host)
                                   const int r = vc_sharded_search_knn(h, codes, nq, k + 1, VC_MODE_LINEAR, VC_ORDER_ASCENDING, hrows, rcnt, nullptr);
                                   if (r) return r;
                                   VS_HIP(h, hipSetDevice(h->root));
                                   return (int)VC_OK;
                                 },
                                 S, err);
  });
}

int vc_sharded_knn_graph_update_dev(vc_sharded* h, uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first, uint64_t* d_rows,
                                    uint32_t* d_counts, vc_knn_graph_update_stats* stats, void* stream) {
  const int rc = check_sharded_kgupd_args(h, k, mode, n_old, k_first, d_rows);
  if (rc) return rc;
  if (stats) *stats = vc_knn_graph_update_stats{};
  if (n_old == h->n) return VC_OK;
  return sharded_store_call(h, mode, sharded_caller_stream(h, stream), [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_knn_graph_update_run(v, sharded_store_view(h, VC_MODE_LINEAR, S).knn, sharded_kgupd_args(h, k, mode, batch, n_old, k_first, d_rows, d_counts), stats, S,
                                   err);
  });
}

int vc_sharded_knn_graph_update(vc_sharded* h, uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first, uint64_t* rows, uint32_t* counts,
                                vc_knn_graph_update_stats* stats) {
  const int rc = check_sharded_kgupd_args(h, k, mode, n_old, k_first, rows);
  if (rc) return rc;
  if (stats) *stats = vc_knn_graph_update_stats{};
  if (n_old == h->n) return VC_OK;
  return sharded_store_call(h, mode, h->root_stream, [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_knn_graph_update_run_host(v, sharded_kgupd_args(h, k, mode, batch, n_old, k_first, nullptr, nullptr), rows, counts, stats,
                                        [&](uint64_t* d_rows, uint32_t* d_counts, vc_knn_graph_update_stats* st) {
                                          return vc_knn_graph_update_run(v, sharded_store_view(h, VC_MODE_LINEAR, S).knn,
                                                                         sharded_kgupd_args(h, k, mode, batch, n_old, k_first, d_rows, d_counts), st, S, err);
                                        },
                                        [&](const uint64_t* codes, uint32_t nq, uint64_t* hrows, uint32_t* rcnt) {   // (its shards recover on the host)
                                          const int r = vc_sharded_search_knn(h, codes, nq, k + 1, VC_MODE_LINEAR, VC_ORDER_ASCENDING, hrows, rcnt, nullptr);
                                          if (r) return r;
                                          VS_HIP(h, hipSetDevice(h->root));
                                          return (int)VC_OK;
                                        },
                                        S, err);
  });
}

int vc_sharded_knn_graph_retain_dev(vc_sharded* h, uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first, const uint32_t* d_new_ids,
                                    uint64_t* d_rows, uint32_t* d_counts, vc_knn_graph_retain_stats* stats, void* stream) {
  const int rc = check_sharded_kgret_args(h, k, mode, n_old, k_first, d_new_ids, d_rows);
  if (rc) return rc;
  if (sharded_kgret_nothing_to_do(h->n, n_old, stats)) return VC_OK;
  return sharded_store_call(h, mode, sharded_caller_stream(h, stream), [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_knn_graph_retain_run(v, sharded_store_view(h, VC_MODE_LINEAR, S).knn, sharded_kgret_args(h, k, mode, batch, n_old, k_first, d_new_ids, d_rows, d_counts),
                                   stats, S, err);
  });
}

int vc_sharded_knn_graph_retain(vc_sharded* h, uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first, const uint32_t* new_ids, uint64_t* rows,
                                uint32_t* counts, vc_knn_graph_retain_stats* stats) {
  const int rc = check_sharded_kgret_args(h, k, mode, n_old, k_first, new_ids, rows);
  if (rc) return rc;
  if (sharded_kgret_nothing_to_do(h->n, n_old, stats)) return VC_OK;
  return sharded_store_call(h, mode, h->root_stream, [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_knn_graph_retain_run_host(v, sharded_kgret_args(h, k, mode, batch, n_old, k_first, nullptr, nullptr, nullptr), new_ids, rows, counts, stats,
                                        [&](const uint32_t* d_new_ids, uint64_t* d_rows, uint32_t* d_counts, vc_knn_graph_retain_stats* st) {
                                          return vc_knn_graph_retain_run(v, sharded_store_view(h, VC_MODE_LINEAR, S).knn,
                                                                         sharded_kgret_args(h, k, mode, batch, n_old, k_first, d_new_ids, d_rows, d_counts), st, S,
                                                                         err);
                                        },
                                        [&](const uint64_t* codes, uint32_t nq, uint64_t* hrows, uint32_t* rcnt) {   // (its shards recover on the host)
                                          const int r = vc_sharded_search_knn(h, codes, nq, k + 1, VC_MODE_LINEAR, VC_ORDER_ASCENDING, hrows, rcnt, nullptr);
                                          if (r) return r;
                                          VS_HIP(h, hipSetDevice(h->root));
                                          return (int)VC_OK;
                                        },
                                        S, err);
  });
}

int vc_sharded_cluster_knn_dev(vc_sharded* h, const uint64_t* d_rows, const uint32_t* d_counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist,
                               uint32_t* d_labels, uint32_t* d_in_degree, vc_cluster_knn_stats* stats, void* stream) {
  const int rc = check_sharded_cluster_knn_args(h, d_rows, k, kk, flags, d_labels);
  if (rc) return rc;
  if (stats) *stats = vc_cluster_knn_stats{};
  if (h->n == 0) return VC_OK;
  return sharded_store_call(h, VC_MODE_LINEAR, sharded_caller_stream(h, stream), [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_cluster_knn_run(v, VcKgraphClusterArgs{d_rows, d_counts, k, kk, flags, max_dist, d_labels, d_in_degree}, stats, S, err);
  });
}

int vc_sharded_cluster_knn(vc_sharded* h, const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist,
                           uint32_t* labels, uint32_t* in_degree, vc_cluster_knn_stats* stats) {
  const int rc = check_sharded_cluster_knn_args(h, rows, k, kk, flags, labels);
  if (rc) return rc;
  if (stats) *stats = vc_cluster_knn_stats{};
  if (h->n == 0) return VC_OK;
  return sharded_store_call(h, VC_MODE_LINEAR, h->root_stream, [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_cluster_knn_run_host(v, VcKgraphClusterArgs{nullptr, nullptr, k, kk, flags, max_dist, nullptr, nullptr}, rows, counts, labels, in_degree, stats, S,
                                   err);
  });
}

int vc_sharded_cluster_snn_dev(vc_sharded* h, const uint64_t* d_rows, const uint32_t* d_counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist,
                               uint32_t min_shared, uint32_t* d_labels, uint32_t* d_shared, uint64_t* d_hist, vc_cluster_snn_stats* stats, void* stream) {
  const int rc = check_sharded_cluster_snn_args(h, d_rows, k, kk, flags, d_labels);
  if (rc) return rc;
  if (stats) *stats = vc_cluster_snn_stats{};
  if (h->n == 0) return VC_OK;
  return sharded_store_call(h, VC_MODE_LINEAR, sharded_caller_stream(h, stream), [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_cluster_snn_run(v, VcSnnArgs{d_rows, d_counts, k, kk, flags, max_dist, min_shared, d_labels, d_shared, d_hist}, stats, S, err);
  });
}

int vc_sharded_cluster_snn(vc_sharded* h, const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist,
                           uint32_t min_shared, uint32_t* labels, uint32_t* shared, uint64_t* hist, vc_cluster_snn_stats* stats) {
  const int rc = check_sharded_cluster_snn_args(h, rows, k, kk, flags, labels);
  if (rc) return rc;
  if (stats) *stats = vc_cluster_snn_stats{};
  if (h->n == 0) return VC_OK;
  return sharded_store_call(h, VC_MODE_LINEAR, h->root_stream, [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_cluster_snn_run_host(v, VcSnnArgs{nullptr, nullptr, k, kk, flags, max_dist, min_shared, nullptr, nullptr, nullptr}, rows, counts, labels, shared, hist,
                                   stats, S, err);
  });
}

int vc_sharded_knn_adjacency_dev(vc_sharded* h, const uint64_t* d_rows, const uint32_t* d_counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist,
                                 uint64_t* d_adj, uint64_t adj_cap, uint64_t* d_offsets, vc_knn_adjacency_stats* stats, void* stream) {
  const int rc = check_sharded_knn_adjacency_args(h, d_rows, k, kk, flags, d_adj, adj_cap, d_offsets);
  if (rc) return rc;
  return sharded_store_call(h, VC_MODE_LINEAR, sharded_caller_stream(h, stream), [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_knn_adjacency_run(v, VcAdjArgs{d_rows, d_counts, k, kk, flags, max_dist, d_adj, adj_cap, d_offsets}, stats, S, err);
  });
}

int vc_sharded_knn_adjacency(vc_sharded* h, const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist,
                             uint64_t* adj, uint64_t adj_cap, uint64_t* offsets, vc_knn_adjacency_stats* stats) {
  const int rc = check_sharded_knn_adjacency_args(h, rows, k, kk, flags, adj, adj_cap, offsets);
  if (rc) return rc;
  return sharded_store_call(h, VC_MODE_LINEAR, h->root_stream, [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_knn_adjacency_run_host(v, VcAdjArgs{nullptr, nullptr, k, kk, flags, max_dist, nullptr, adj_cap, nullptr}, rows, counts, adj, offsets, stats, S, err);
  });
}

int vc_sharded_knn_mst_dev(vc_sharded* h, const uint64_t* d_rows, const uint32_t* d_counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist,
                           uint32_t weight_kind, uint32_t min_pts, vc_mst_edge* d_edges, uint32_t* d_labels, uint64_t* d_hist, vc_knn_mst_stats* stats,
                           void* stream) {
  const int rc = check_sharded_knn_mst_args(h, d_rows, k, kk, flags, weight_kind, min_pts, d_edges);
  if (rc) return rc;
  return sharded_store_call(h, VC_MODE_LINEAR, sharded_caller_stream(h, stream), [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_knn_mst_run(v, VcMstArgs{d_rows, d_counts, k, kk, flags, max_dist, weight_kind, min_pts, d_edges, d_labels, d_hist}, stats, S, err);
  });
}

int vc_sharded_knn_mst(vc_sharded* h, const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist,
                       uint32_t weight_kind, uint32_t min_pts, vc_mst_edge* edges, uint32_t* labels, uint64_t* hist, vc_knn_mst_stats* stats) {
  const int rc = check_sharded_knn_mst_args(h, rows, k, kk, flags, weight_kind, min_pts, edges);
  if (rc) return rc;
  return sharded_store_call(h, VC_MODE_LINEAR, h->root_stream, [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_knn_mst_run_host(v, VcMstArgs{nullptr, nullptr, k, kk, flags, max_dist, weight_kind, min_pts, nullptr, nullptr, nullptr}, rows, counts, edges, labels,
                               hist, stats, S, err);
  });
}

int vc_sharded_mst_cut_dev(vc_sharded* h, const vc_mst_edge* d_edges, uint64_t n_edges, uint32_t max_weight, uint32_t* d_labels, uint64_t* n_clusters,
                           void* stream) {
  if (!h || !d_labels || (!d_edges && n_edges)) return VC_ERR_INVALID;
  return sharded_store_call(h, VC_MODE_LINEAR, sharded_caller_stream(h, stream), [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_mst_cut_run(v, d_edges, n_edges, max_weight, d_labels, n_clusters, S, err);
  });
}

int vc_sharded_mst_cut(vc_sharded* h, const vc_mst_edge* edges, uint64_t n_edges, uint32_t max_weight, uint32_t* labels, uint64_t* n_clusters) {
  if (!h || !labels || (!edges && n_edges)) return VC_ERR_INVALID;
  return sharded_store_call(h, VC_MODE_LINEAR, h->root_stream, [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_mst_cut_run_host(v, edges, n_edges, max_weight, labels, n_clusters, S, err);
  });
}

int vc_sharded_mst_condense_dev(vc_sharded* h, const vc_mst_edge* d_edges, uint64_t n_edges, uint32_t min_cluster_size, uint32_t root_weight, uint32_t method,
                                vc_condensed_node* d_nodes, uint32_t* d_labels, uint32_t* d_node, uint32_t* d_own, uint32_t* d_leave, vc_mst_condense_stats* stats,
                                void* stream) {
  const int rc = check_sharded_mst_condense_args(h, d_edges, n_edges, min_cluster_size, root_weight, method, d_nodes, d_labels);
  if (rc) return rc;
  return sharded_store_call(h, VC_MODE_LINEAR, sharded_caller_stream(h, stream), [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_mst_condense_run(v, VcCondenseArgs{d_edges, n_edges, min_cluster_size, root_weight, method, d_nodes, d_labels, d_node, d_own, d_leave}, stats, S, err);
  });
}

int vc_sharded_mst_condense(vc_sharded* h, const vc_mst_edge* edges, uint64_t n_edges, uint32_t min_cluster_size, uint32_t root_weight, uint32_t method,
                            vc_condensed_node* nodes, uint32_t* labels, uint32_t* node, uint32_t* own, uint32_t* leave, vc_mst_condense_stats* stats) {
  const int rc = check_sharded_mst_condense_args(h, edges, n_edges, min_cluster_size, root_weight, method, nodes, labels);
  if (rc) return rc;
  return sharded_store_call(h, VC_MODE_LINEAR, h->root_stream, [&](const VcStoreView& v, hipStream_t S, std::string* err) {
    return vc_mst_condense_run_host(v, VcCondenseArgs{nullptr, n_edges, min_cluster_size, root_weight, method, nullptr, nullptr, nullptr, nullptr, nullptr}, edges,
                                    nodes, labels, node, own, leave, stats, S, err);
  });
}

int vc_sharded_knn_vote_dev(vc_sharded* h, const uint64_t* d_rows, const uint32_t* d_counts, uint64_t n_rows, uint32_t k, uint32_t kk, uint32_t max_dist,
                            const uint32_t* d_labels, uint32_t weight_kind, uint32_t* d_out_label, uint32_t* d_out_votes, uint32_t* d_out_total,
                            vc_knn_vote_stats* stats, void* stream) {
  const int rc = check_sharded_knn_vote_args(h, d_rows, k, kk, d_labels, weight_kind, d_out_label);
  if (rc) return rc;
  return sharded_store_call(h, VC_MODE_LINEAR, sharded_caller_stream(h, stream), [&](const VcStoreView& v, hipStream_t s, std::string* err) {
    return vc_knn_vote_run(v, VcVoteArgs{d_rows, d_counts, n_rows, k, kk, max_dist, d_labels, weight_kind, d_out_label, d_out_votes, d_out_total},
                           stats, s, err);
  });
}

int vc_sharded_knn_vote(vc_sharded* h, const uint64_t* rows, const uint32_t* counts, uint64_t n_rows, uint32_t k, uint32_t kk, uint32_t max_dist, const uint32_t* labels,
                        uint32_t weight_kind, uint32_t* out_label, uint32_t* out_votes, uint32_t* out_total, vc_knn_vote_stats* stats) {
  const int rc = check_sharded_knn_vote_args(h, rows, k, kk, labels, weight_kind, out_label);
  if (rc) return rc;
  return sharded_store_call(h, VC_MODE_LINEAR, h->root_stream, [&](const VcStoreView& v, hipStream_t s, std::string* err) {
    return vc_knn_vote_run_host(v, VcVoteArgs{nullptr, nullptr, n_rows, k, kk, max_dist, nullptr, weight_kind, nullptr, nullptr, nullptr}, rows,
                                counts, labels, out_label, out_votes, out_total, stats, s, err);
  });
}

int vc_sharded_label_propagate_dev(vc_sharded* h, const uint64_t* d_offsets, const uint64_t* d_adj, uint64_t n_entries, const uint32_t* d_labels_in, uint32_t weight_kind,
                                   uint32_t flags, uint32_t max_iters, uint32_t* d_labels_out, uint32_t* d_votes, uint32_t* d_total,
                                   vc_label_propagate_stats* stats, void* stream) {
  const int rc = check_sharded_label_propagate_args(h, d_offsets, d_adj, n_entries, d_labels_in, weight_kind, flags, max_iters, d_labels_out);
  if (rc) return rc;
  return sharded_store_call(h, VC_MODE_LINEAR, sharded_caller_stream(h, stream), [&](const VcStoreView& v, hipStream_t s, std::string* err) {
    return vc_label_propagate_run(v,
                                  VcLabelPropagateArgs{d_offsets, d_adj, n_entries, d_labels_in, weight_kind, flags, max_iters, d_labels_out, d_votes, d_total}, stats, s, err);
  });
}

int vc_sharded_label_propagate(vc_sharded* h, const uint64_t* offsets, const uint64_t* adj, uint64_t n_entries, const uint32_t* labels_in, uint32_t weight_kind, uint32_t flags,
                               uint32_t max_iters, uint32_t* labels_out, uint32_t* votes, uint32_t* total, vc_label_propagate_stats* stats) {
  const int rc = check_sharded_label_propagate_args(h, offsets, adj, n_entries, labels_in, weight_kind, flags, max_iters, labels_out);
  if (rc) return rc;
  return sharded_store_call(h, VC_MODE_LINEAR, h->root_stream, [&](const VcStoreView& v, hipStream_t s, std::string* err) {
    return vc_label_propagate_run_host(v,
                                       VcLabelPropagateArgs{nullptr, nullptr, n_entries, nullptr, weight_kind, flags, max_iters, nullptr, nullptr, nullptr}, offsets, adj,
                                       labels_in, labels_out, votes, total, stats, s, err);
  });
}

}  // extern "C"

// ---- removal over the shards ----------------------------------------------------------------------------------------------------------
// a shard's map names ids of its own range (shard id_base + j); survivor j of shard g is survivor P_g + j of the store
extern "C" __global__ void __launch_bounds__(256) vc_sharded_retain_shift_kernel(uint32_t* __restrict__ ids, uint64_t n, uint32_t delta) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t v = ids[i];
    if (v != 0xFFFFFFFFu) ids[i] = v + delta;
  }
}

static int check_sharded_retain_args(vc_sharded* h, const uint32_t* sel, uint32_t kind, const uint32_t* new_ids) {
  if (!h) return VC_ERR_INVALID;
  if (kind > VC_RETAIN_ROOTS) return sfail(h, VC_ERR_INVALID, "retain: unknown kind %u", kind);
  if (h->n && !sel) return sfail(h, VC_ERR_INVALID, "retain: null selection");
  if (h->n && new_ids) {
    const uintptr_t x = (uintptr_t)sel, y = (uintptr_t)new_ids, bytes = (uintptr_t)h->n * 4;
    if (x < y + bytes && y < x + bytes) return sfail(h, VC_ERR_INVALID, "retain: new_ids overlaps the selection");
  }
  return VC_OK;
}

// d_sel / d_new_ids on the root device, valid on S; h->n > 0.  Every step is waited for before the next one starts on another
// device.  1. every shard filters its slice; 2. the maps are shifted to store-wide ids; 3. in ascending shard order a shard takes
// what it lacks from the front of the following shards, which drop that prefix; 4. the shards that received bring their index up
// to date.  Nothing on the root depends on the store's size between calls (shard_size reads h->n).
static int sharded_retain_run(vc_sharded* h, const uint32_t* d_sel, uint32_t kind, uint32_t* d_new_ids, uint64_t* n_kept, hipStream_t S) {
  const uint32_t G = h->G, id_base = h->cfg.engine.id_base;
  auto stream_of = [&](uint32_t g) { return h->dev[g] == h->root ? S : h->lanes[h->lane_of[g]].stream; };
  auto shard_fail = [&](uint32_t g, int rc) { return sfail(h, rc, "shard %u: %s", g, vc_last_error(h->eng[g])); };
  bool indexed = true;
  for (uint32_t g = 0; g < G; ++g) indexed = indexed && (shard_size(h, g) == 0 || vc_engine_has_index(h->eng[g]));
  VS_HIP(h, hipSetDevice(h->root));
  VS_HIP(h, hipStreamSynchronize(S));

  // 1. the shards' own removals
  std::vector<uint64_t> had(G, 0), cur(G, 0), arrived(G, 0);
  uint64_t K = 0;
  for (uint32_t g = 0; g < G; ++g) {
    const uint64_t ng = had[g] = shard_size(h, g);
    if (!ng) continue;
    const uint32_t* sel_g = d_sel + h->lo[g];
    uint32_t* map_g = d_new_ids ? d_new_ids + h->lo[g] : nullptr;
    int rc;
    if (h->dev[g] == h->root) {
      rc = vc_retain_dev(h->eng[g], sel_g, kind, map_g, &cur[g], S);
    } else {   // the slice travels to the shard's device and the map back
      VS_HIP(h, hipSetDevice(h->dev[g]));
      ScopedBufs<2> tmp;
      hipStream_t L = stream_of(g);
      if ((rc = grow(h, tmp.b[0], ng * 4)) || (map_g && (rc = grow(h, tmp.b[1], ng * 4)))) return rc;
      VS_HIP(h, hipMemcpyPeerAsync(tmp.b[0].p, h->dev[g], sel_g, h->root, ng * 4, L));
      rc = vc_retain_dev(h->eng[g], tmp.b[0].as<uint32_t>(), kind, map_g ? tmp.b[1].as<uint32_t>() : nullptr, &cur[g], L);
      if (rc == VC_OK && map_g) VS_HIP(h, hipMemcpyPeerAsync(map_g, h->root, tmp.b[1].p, h->dev[g], ng * 4, L));
      VS_HIP(h, hipStreamSynchronize(L));
    }
    if (rc) return shard_fail(g, rc);
    // 2. the shard's ids start at id_base + lo[g], its survivors at id_base + K
    if (map_g && K != h->lo[g]) {
      VS_HIP(h, hipSetDevice(h->root));
      hipLaunchKernelGGL(vc_sharded_retain_shift_kernel, dim3((uint32_t)std::min<uint64_t>((ng + 255) / 256, 4096)), dim3(256), 0, S, map_g, ng,
                         (uint32_t)K - (uint32_t)h->lo[g]);
      VS_HIP(h, hipGetLastError());
    }
    K += cur[g];
  }
  (void)id_base;
  const std::vector<uint64_t> kept = cur;

  // 3. the survivors fill shard 0, then shard 1, ...
  uint32_t src = 0;
  for (uint32_t g = 0; g < G; ++g) {
    const uint64_t target = K <= h->lo[g] ? 0 : std::min(K, h->hi[g]) - h->lo[g];
    src = std::max(src, g + 1);
    while (cur[g] < target) {
      while (src < G && cur[src] == 0) ++src;
      if (src >= G) return sfail(h, VC_ERR_STATE, "retain: the shards hold fewer records than they reported");
      const uint64_t take = std::min(target - cur[g], cur[src]);
      int rc = vc_engine_append_from(h->eng[g], h->eng[src], 0, take, stream_of(g));
      if (rc) return shard_fail(g, rc);
      if ((rc = vc_engine_retain_from(h->eng[src], take, stream_of(src)))) return shard_fail(src, rc);
      cur[g] += take;
      arrived[g] += take;
      cur[src] -= take;
    }
  }
  h->n = K;

  // 4. indexes: filtered where records only left (done above), updated where records arrived, built where none was left
  for (uint32_t g = 0; g < G; ++g) {
    const char* route = had[g] == 0 ? "none" : !indexed ? "columns" : cur[g] == 0 ? "empty" : arrived[g] ? "update" : kept[g] == had[g] && cur[g] == kept[g] ? "none" : "filter";
    if (indexed && cur[g] && !vc_engine_has_index(h->eng[g])) {
      int rc = vc_update_index(h->eng[g]);
      if (rc) return shard_fail(g, rc);
    }
    if (h->knobs.mih_trace)
      fprintf(stderr, "[vc_sharded] retained: shard=%u n=%llu kept=%llu given=%llu arrived=%llu route=%s\n", g, (unsigned long long)cur[g],
              (unsigned long long)kept[g], (unsigned long long)(kept[g] + arrived[g] - cur[g]), (unsigned long long)arrived[g], route);
  }
  VS_HIP(h, hipSetDevice(h->root));
  VS_HIP(h, hipStreamSynchronize(S));
  if (n_kept) *n_kept = K;
  return VC_OK;
}

extern "C" {

int vc_sharded_retain_dev(vc_sharded* h, const uint32_t* d_sel, uint32_t kind, uint32_t* d_new_ids, uint64_t* n_kept, void* stream) {
  int rc = check_sharded_retain_args(h, d_sel, kind, d_new_ids);
  if (rc) return rc;
  if (h->n == 0) {
    if (n_kept) *n_kept = 0;
    return VC_OK;
  }
  return sharded_retain_run(h, d_sel, kind, d_new_ids, n_kept, sharded_caller_stream(h, stream));
}

int vc_sharded_retain(vc_sharded* h, const uint32_t* sel, uint32_t kind, uint32_t* new_ids, uint64_t* n_kept) {
  int rc = check_sharded_retain_args(h, sel, kind, new_ids);
  if (rc) return rc;
  if (h->n == 0) {
    if (n_kept) *n_kept = 0;
    return VC_OK;
  }
  const uint64_t N = h->n;
  hipStream_t S = h->root_stream;
  VS_HIP(h, hipSetDevice(h->root));
  ScopedBufs<2> tmp;   // staged selection and map: call-scoped
  if ((rc = grow(h, tmp.b[0], N * 4)) || (new_ids && (rc = grow(h, tmp.b[1], N * 4)))) return rc;
  VS_HIP(h, hipMemcpyAsync(tmp.b[0].p, sel, N * 4, hipMemcpyHostToDevice, S));
  rc = sharded_retain_run(h, tmp.b[0].as<uint32_t>(), kind, new_ids ? tmp.b[1].as<uint32_t>() : nullptr, n_kept, S);
  (void)hipSetDevice(h->root);   // (the buffers are released on the device they live on)
  if (rc) return rc;
  if (new_ids) {
    VS_HIP(h, hipMemcpyAsync(new_ids, tmp.b[1].p, N * 4, hipMemcpyDeviceToHost, S));
    VS_HIP(h, hipStreamSynchronize(S));
  }
  return VC_OK;
}

}  // extern "C"
