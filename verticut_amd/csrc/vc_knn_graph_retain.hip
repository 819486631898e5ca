// ============================================================================
// vc_knn_graph_retain.hip -- a built k-NN graph brought up to date after vc_retain* (vc_knn_graph_retain*,
// vc_sharded_knn_graph_retain*); the header states the contract.  One driver for both handle kinds over a VcStoreView; the plan
// arithmetic is vc_knn_graph_retain_plan.hpp.  vc_retain* renumbers the survivors monotonically, so the order of (dist << 32 | id)
// among them is the same before and after: the surviving entries of an old row, translated, are the smallest entries of the rebuilt
// row, and the row is wrong only where it became SHORT (vc_kgret_short).  Only the short rows are searched: vc_knn_graph_run over
// their id list.
//   vc_kgraph_live_kernel     the map check, before the scan: a live flag per word of the map
//   vc_kgraph_map_kernel      the map check, after it: every live word is id_base + its rank, and the live words number K
//   vc_kgraph_retain_kernel   a chunk of old rows: a removed record's row is skipped, every entry of a surviving row reads its new id
//                             straight from the map in global memory, the live entries are placed by the popcount of a ballot below
//                             the lane, the tail is padded; the row goes out of place to its new position within the chunk, with its
//                             count, a short flag per old row and two tallies, one atomic per wave each
//   vc_kgraph_back_kernel     the chunk's rows and counts back into the graph, at or before the chunk's own start
//   vc_kgraph_short_kernel    the ascending list of the short rows' new ids, placed by the exclusive scan of the flags (vc_sort.hip)
// None of them uses LDS or scratch memory or waits for another block.  Every address formed from data -- an entry's word of the map,
// a row's place in the chunk -- is bounds-checked, so a graph or a map that is not what the contract asks for raises the error word
// and is passed over.
// ============================================================================
#include <algorithm>
#include <vector>

#include "vc_internal.hpp"
#include "vc_knn_graph_plan.hpp"
#include "vc_knn_graph_retain_plan.hpp"

static_assert(sizeof(vc_knn_graph_retain_stats) == 64, "the header's size");
static_assert(VC_KGRET_WAVE == VC_WAVE, "the plan's wave");

namespace {

#define KR_BLK VC_KGRET_BLOCK
#define KR_DEAD 0xFFFFFFFFu

__device__ __forceinline__ void kr_raise(unsigned long long* stat) { ((uint32_t*)(stat + VC_KGRET_ST_LIST))[1] = 1u; }

__global__ void __launch_bounds__(KR_BLK) vc_kgraph_live_kernel(const uint32_t* __restrict__ new_ids, uint64_t n_old, uint32_t* __restrict__ live) {
  for (uint64_t i = (uint64_t)blockIdx.x * KR_BLK + threadIdx.x; i <= n_old; i += (uint64_t)gridDim.x * KR_BLK)
    live[i] = i < n_old && new_ids[i] != KR_DEAD ? 1u : 0u;
}

__global__ void __launch_bounds__(KR_BLK) vc_kgraph_map_kernel(const uint32_t* __restrict__ new_ids, const uint32_t* __restrict__ rank, uint64_t n_old, uint64_t K,
                                                               uint32_t id_base, unsigned long long* __restrict__ stat) {
  bool bad = blockIdx.x == 0 && threadIdx.x == 0 && rank[n_old] != K;
  for (uint64_t i = (uint64_t)blockIdx.x * KR_BLK + threadIdx.x; i < n_old; i += (uint64_t)gridDim.x * KR_BLK) {
    const uint32_t w = new_ids[i];
    bad |= w != KR_DEAD && w != id_base + rank[i];
  }
  if (bad) kr_raise(stat);
}

// what a translate or copy-back launch works on: the old rows [c0, c0 + nrows)
struct RetainArgs {
  uint64_t* rows;             // [n_old][k]: the graph; the translate kernel only reads it
  uint32_t* counts;           // [n_old], nullable: every old row holds `uniform` entries
  const uint32_t* new_ids;    // [n_old]
  const uint32_t* rank;       // [n_old + 1]: live words of the map before each position
  uint64_t n_old, K, c0, nrows;
  uint32_t k, P, shift, id_base, uniform;   // P = vc_kgret_lanes(k) = 1 << shift
  uint64_t* out;              // [nrows][k]: the chunk's rows at their new positions, counted from rank[c0]
  uint32_t* out_cnt;          // [nrows]
  uint32_t* shrt;             // [n_old]
  unsigned long long* stat;   // VC_KGRET_ST_*
};

// A wave carries 64 / P rows; lane l serves entry j0 + l % P of row l / P of its group.  The bounds of both loops are wave-uniform, so
// every lane votes in every ballot.  The place of a live entry is the row's running base plus the live lanes of its segment below it,
// so the entries stay ascending.
__global__ void __launch_bounds__(KR_BLK) vc_kgraph_retain_kernel(const RetainArgs a) {
  const uint32_t lane = vc_lane(), P = a.P, R = VC_WAVE >> a.shift, seg = lane >> a.shift, jl = lane & (P - 1), k = a.k;
  const uint64_t segmask = vc_kgret_segment_mask(P, seg), below = segmask & ((1ull << lane) - 1);
  const uint64_t waves = (uint64_t)gridDim.x * (KR_BLK / VC_WAVE), wave = (uint64_t)blockIdx.x * (KR_BLK / VC_WAVE) + threadIdx.x / VC_WAVE;
  const uint32_t dest0 = a.rank[a.c0];
  uint32_t dropped = 0, shorts = 0;   // wave-uniform
  bool bad = false;
  for (uint64_t g = wave * R; g < a.nrows; g += waves * R) {
    const uint64_t r = g + seg, i = a.c0 + r;
    const bool on = r < a.nrows;
    bool alive = false;   // the row of a surviving record that can be translated
    uint32_t c = 0, sr = 0;
    if (on) {
      const uint32_t own = a.new_ids[i];
      if (own != KR_DEAD) {
        c = a.counts ? a.counts[i] : a.uniform;
        sr = own - a.id_base - dest0;
        alive = c <= k && (uint64_t)sr < a.nrows;
        bad |= !alive;
      }
    }
    const uint64_t* row = a.rows + i * k;
    uint64_t* out = a.out + (uint64_t)(alive ? sr : 0u) * k;
    uint32_t base = 0;
    for (uint32_t j0 = 0; j0 < k; j0 += P) {
      const uint32_t j = j0 + jl;
      bool live = false, dead = false;
      uint64_t v = 0;
      uint32_t nid = 0;
      if (alive && j < c) {
        v = row[j];
        const uint32_t id = (uint32_t)v - a.id_base;
        if ((uint64_t)id >= a.n_old) {
          bad = true;
        } else {
          nid = a.new_ids[id];
          live = nid != KR_DEAD;
          dead = !live;
        }
      }
      const uint64_t votes = __ballot(live);
      dropped += (uint32_t)__popcll(__ballot(dead));
      if (live) out[base + (uint32_t)__popcll(votes & below)] = (v & 0xFFFFFFFF00000000ull) | nid;   // (below c <= k: inside the row)
      base += (uint32_t)__popcll(votes & segmask);
    }
    if (alive)
      for (uint32_t p = base + jl; p < k; p += P) out[p] = VC_PACK_INF;
    const bool is_short = alive && vc_kgret_short(base, a.K, k);
    if (on && jl == 0) {
      a.shrt[i] = is_short ? 1u : 0u;
      if (alive) a.out_cnt[sr] = base;
    }
    shorts += (uint32_t)__popcll(__ballot(is_short && jl == 0));
  }
  if (bad) kr_raise(a.stat);
  if (lane == 0) {
    if (dropped) atomicAdd(a.stat + VC_KGRET_ST_DROPPED, (unsigned long long)dropped);
    if (shorts) atomicAdd(a.stat + VC_KGRET_ST_SHORT, (unsigned long long)shorts);
  }
}

// thread e serves entry e % k of row e / k of the chunk's rank[c0 + nrows] - rank[c0] new rows.  They go to the rows from rank[c0]
// on, which end at rank[c0 + nrows] <= c0 + nrows: only rows the translate launch has consumed are overwritten, whatever the map says.
__global__ void __launch_bounds__(KR_BLK) vc_kgraph_back_kernel(const RetainArgs a) {
  const uint32_t dest0 = a.rank[a.c0];
  const uint64_t total = (uint64_t)(a.rank[a.c0 + a.nrows] - dest0) * a.k;
  for (uint64_t e = (uint64_t)blockIdx.x * KR_BLK + threadIdx.x; e < total; e += (uint64_t)gridDim.x * KR_BLK) {
    a.rows[(uint64_t)dest0 * a.k + e] = a.out[e];
    if (a.counts && e % a.k == 0) a.counts[dest0 + e / a.k] = a.out_cnt[e / a.k];
  }
}

// old row i with shrt[i] goes to place srank[i] of the list, as its new id: ascending, independent of block order.  The thread of the
// last old row leaves the length.
__global__ void __launch_bounds__(KR_BLK) vc_kgraph_short_kernel(const uint32_t* __restrict__ shrt, const uint32_t* __restrict__ srank,
                                                                 const uint32_t* __restrict__ new_ids, uint64_t n_old, uint64_t K, uint32_t* __restrict__ list,
                                                                 unsigned long long* __restrict__ stat) {
  for (uint64_t i = (uint64_t)blockIdx.x * KR_BLK + threadIdx.x; i < n_old; i += (uint64_t)gridDim.x * KR_BLK) {
    const uint32_t f = shrt[i], at = srank[i];
    if (i == n_old - 1) ((uint32_t*)(stat + VC_KGRET_ST_LIST))[0] = at + f;
    if (f && at < K) list[at] = new_ids[i];
  }
}

uint32_t kr_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + KR_BLK - 1) / KR_BLK, 1), 256 * 8); }

#define KR_HIP(call) VC_HIP_OR_FAIL("k-NN graph retain", call)

}  // namespace

// THE STEPS (the header states the rule).  1. the map check: live flags, their scan, the compare.  2. chunk by chunk in ascending
// order: the translate launch into the out-of-place rows, the copy back.  3. the scan of the short flags and the list.  4. THE WAIT
// of the call, 32 bytes: the tallies, the length of the list and the error word.  5. vc_knn_graph_run over the list, with its own waits.
int vc_knn_graph_retain_run(const VcStoreView& v, const VcKnnSearch& linear_knn, const VcKgretArgs& a, vc_knn_graph_retain_stats* stats, hipStream_t s,
                            std::string* err) {
  if (stats) *stats = vc_knn_graph_retain_stats{};
  const uint64_t K = v.n, n_old = a.n_old;
  const uint32_t k = a.repair.k;
  const uint64_t chunk = vc_kgret_chunk_rows(a.repair.budget, k, n_old);
  const VcKgretWork wp(n_old, K, vc_scan_work_words(n_old + 1));
  uint8_t* work = (uint8_t*)v.alloc(VC_KGRAPH_RET_WORK, wp.total);
  uint8_t* side = (uint8_t*)v.alloc(VC_KGRAPH_RET_ROWS, (size_t)vc_kgret_rows_bytes(chunk, k));
  if (!work || !side) return VC_ERR_NOMEM;
  unsigned long long* stat = (unsigned long long*)(work + wp.stat);
  uint32_t* live = (uint32_t*)(work + wp.live);
  uint32_t* rank = (uint32_t*)(work + wp.rank);
  uint32_t* shrt = (uint32_t*)(work + wp.shrt);
  uint32_t* srank = (uint32_t*)(work + wp.srank);
  uint32_t* list = (uint32_t*)(work + wp.list);
  uint32_t* scan_work = (uint32_t*)(work + wp.scan_work);
  KR_HIP(hipMemsetAsync(stat, 0, VC_KGRET_STAT_BYTES, s));
  hipLaunchKernelGGL(vc_kgraph_live_kernel, dim3(kr_grid(n_old + 1)), dim3(KR_BLK), 0, s, a.d_new_ids, n_old, live);
  KR_HIP(hipGetLastError());
  KR_HIP(vc_exclusive_scan_u32(live, rank, n_old + 1, scan_work, s));
  hipLaunchKernelGGL(vc_kgraph_map_kernel, dim3(kr_grid(n_old)), dim3(KR_BLK), 0, s, a.d_new_ids, (const uint32_t*)rank, n_old, K, v.id_base, stat);
  KR_HIP(hipGetLastError());
  RetainArgs ra{};
  ra.rows = a.repair.d_rows; ra.counts = a.repair.d_counts; ra.new_ids = a.d_new_ids; ra.rank = rank; ra.n_old = n_old; ra.K = K;
  ra.k = k; ra.P = vc_kgret_lanes(k); ra.shift = (uint32_t)__builtin_ctz(ra.P); ra.id_base = v.id_base; ra.uniform = vc_kgraph_row_count(n_old, k);
  ra.out = (uint64_t*)side; ra.out_cnt = (uint32_t*)(side + chunk * k * 8); ra.shrt = shrt; ra.stat = stat;
  for (uint64_t c0 = 0; c0 < n_old; c0 += chunk) {
    ra.c0 = c0;
    ra.nrows = std::min<uint64_t>(chunk, n_old - c0);
    hipLaunchKernelGGL(vc_kgraph_retain_kernel, dim3(vc_kgret_blocks(ra.nrows, k)), dim3(KR_BLK), 0, s, ra);
    KR_HIP(hipGetLastError());
    hipLaunchKernelGGL(vc_kgraph_back_kernel, dim3(kr_grid(ra.nrows * k)), dim3(KR_BLK), 0, s, ra);
    KR_HIP(hipGetLastError());
  }
  KR_HIP(vc_exclusive_scan_u32(shrt, srank, n_old, scan_work, s));
  hipLaunchKernelGGL(vc_kgraph_short_kernel, dim3(kr_grid(n_old)), dim3(KR_BLK), 0, s, (const uint32_t*)shrt, (const uint32_t*)srank, a.d_new_ids, n_old, K, list,
                     stat);
  KR_HIP(hipGetLastError());
  // THE WAIT of the call: the tallies, the length of the short list and the error word, 32 bytes
  struct { uint64_t dropped, n_short; uint32_t S, bad; uint64_t pad; } home{};
  static_assert(sizeof(home) == VC_KGRET_STAT_BYTES, "the counters as they lie");
  KR_HIP(hipMemcpyAsync(&home, stat, VC_KGRET_STAT_BYTES, hipMemcpyDeviceToHost, s));
  KR_HIP(hipStreamSynchronize(s));
  if (home.bad) {
    if (err)
      *err = "k-NN graph retain: an old count above k, an entry outside the old store, or a map vc_retain* did not write for this store -- not the graph and map "
             "the call asks for";
    return VC_ERR_INVALID;
  }
  if (home.S > K || home.S != home.n_short) {
    if (err) *err = "k-NN graph retain: the short list does not fit the short rows";
    return VC_ERR_HIP;
  }
  vc_knn_graph_retain_stats st{};
  st.n_rows_kept = K;
  st.n_rows_short = home.n_short;
  st.n_entries_dropped = home.dropped;
  if (home.S) {
    VcKgraphArgs ga = a.repair;
    ga.first = 0;
    ga.rows = home.S;
    ga.d_id_list = list;
    const int rc = vc_knn_graph_run(v, linear_knn, ga, stats ? &st.repair : nullptr, s, err);
    if (rc) return rc;
  }
  if (stats) *stats = st;
  return VC_OK;
}

// The host form: the old rows, counts and map staged up (rows | counts | map, over all n_old records), `run` on them, the K rows and
// counts home.  Without counts the staged old counts are the uniform min(k, n_old - 1), so that the repaired rows' counts can still
// tell which rows the linear scan passed on; those are answered again as vc_knn_graph_run_host answers them -- over the range [0, K),
// in which only a repaired row can carry the count UINT32_MAX.
int vc_knn_graph_retain_run_host(const VcStoreView& v, const VcKgretArgs& a, const uint32_t* new_ids, uint64_t* rows, uint32_t* counts,
                                 vc_knn_graph_retain_stats* stats,
                                 const std::function<int(const uint32_t* d_new_ids, uint64_t* d_rows, uint32_t* d_counts, vc_knn_graph_retain_stats* stats)>& run,
                                 const std::function<int(const uint64_t* codes, uint32_t nq, uint64_t* rows, uint32_t* counts)>& host_knn, hipStream_t s,
                                 std::string* err) {
  const size_t K = (size_t)v.n, n_old = (size_t)a.n_old, k = a.repair.k, rbytes = n_old * k * 8, cbytes = (n_old * 4 + 7) & ~(size_t)7;
  uint8_t* stage = (uint8_t*)v.alloc(VC_KGRAPH_RET_STAGE, rbytes + 2 * cbytes);
  if (!stage) return VC_ERR_NOMEM;
  uint64_t* d_rows = (uint64_t*)stage;
  uint32_t* d_cnt = (uint32_t*)(stage + rbytes);
  uint32_t* d_map = (uint32_t*)(stage + rbytes + cbytes);
  std::vector<uint32_t> uniform;
  if (!counts) uniform.assign(n_old, vc_kgraph_row_count(n_old, (uint32_t)k));
  KR_HIP(hipMemcpyAsync(d_rows, rows, rbytes, hipMemcpyHostToDevice, s));
  KR_HIP(hipMemcpyAsync(d_cnt, counts ? counts : uniform.data(), n_old * 4, hipMemcpyHostToDevice, s));
  KR_HIP(hipMemcpyAsync(d_map, new_ids, n_old * 4, hipMemcpyHostToDevice, s));
  KR_HIP(hipStreamSynchronize(s));   // (the uniform counts leave this scope)
  vc_knn_graph_retain_stats st{};
  int rc = run(d_map, d_rows, d_cnt, &st);
  if (rc) return rc;
  std::vector<uint32_t> own_cnt;
  uint32_t* cnt = counts;
  if (!cnt && st.repair.n_gave_up) {
    own_cnt.resize(K);
    cnt = own_cnt.data();
  }
  KR_HIP(hipMemcpyAsync(rows, d_rows, K * k * 8, hipMemcpyDeviceToHost, s));
  if (cnt) KR_HIP(hipMemcpyAsync(cnt, d_cnt, K * 4, hipMemcpyDeviceToHost, s));
  KR_HIP(hipStreamSynchronize(s));
  if (st.repair.n_gave_up) {
    VcKgraphArgs ga = a.repair;
    ga.first = 0;
    ga.rows = K;
    if ((rc = vc_knn_graph_answer_again_host(v, ga, rows, cnt, host_knn, s, err))) return rc;
  }
  if (stats) *stats = st;
  return VC_OK;
}
