// ============================================================================
// vc_snn.hip -- shared-nearest-neighbour clustering of a built k-NN graph (vc_cluster_snn*, vc_sharded_cluster_snn*); the header
// states the contract.  One driver for both handle kinds over a VcStoreView; the plan arithmetic is vc_snn_plan.hpp.
//   vc_snn_init_kernel        labels[i] = id_base + i
//   vc_snn_kernel<1>          kk <= VC_SNN_WAVE_KK: one WAVE serves a row; its set is a private LDS slice, four rows share a block
//   vc_snn_kernel<4>          above: one BLOCK serves a row; the four waves share the set and split the listed entries
// A team puts S_i -- the positions row i lists -- into an open-addressing set in LDS (atomicCAS, at most half full), then takes the
// listed entries (d, j) in a team-uniform loop: the lanes stride over row j's first min(kk, count_j) entries with coalesced 8-byte
// loads, test the cap, probe the set; a ballot's popcount is shared(i, j).  Short lists (kk <= 32) take 64 / P entries per pass, P
// lanes each.  The mutual test is vc_cluster_knn*'s one compare.  Around that loop every entry has a lane of its own: it loads the
// entry, row j's count and the word of the one compare beforehand (all entries at once, so the misses overlap), and afterwards
// writes the weight, bumps the block's LDS histogram and unites in the lock-free forest.  The loop itself is then one dependent
// load per entry, issued one entry ahead.  Static LDS only, no scratch memory, no cooperative launch.
// ============================================================================
#include <algorithm>

#include "vc_forest.hpp"
#include "vc_internal.hpp"
#include "vc_knn_graph_plan.hpp"
#include "vc_snn_plan.hpp"

static_assert(VC_SNN_PLAN_MAX_KK == VC_SNN_MAX_KK && VC_SNN_PLAN_NONE == VC_SNN_NONE && VC_SNN_FLAG_EITHER == VC_KNN_EITHER, "the header's constants");
static_assert(sizeof(vc_cluster_snn_stats) == VC_SNN_STAT_BYTES, "the header's size");
static_assert(VC_SNN_WAVE == VC_WAVE && VC_SNN_WAVE_KK <= VC_SNN_PLAN_MAX_KK, "the plan's wave");

namespace {

// what the launches work on
struct SnnArgs {
  const uint64_t* rows;      // [n][k]
  const uint32_t* counts;    // [n], nullable: every row holds `uniform` entries
  uint64_t n;
  uint32_t k, kk, either, max_dist, min_shared, id_base, uniform;
  uint32_t shift;            // vc_snn_table_shift(kk)
  uint32_t lanes;            // vc_snn_entry_lanes(kk)
  uint32_t* labels;          // [n]: the forest of vc_forest.hpp
  uint32_t* shared;          // [n][kk], nullable
  unsigned long long* hist;  // [kk], nullable, zeroed before the launch
  unsigned long long* stat;  // [0] += edges, [1] += mutual pairs, [2] += joined pairs, [3] clusters (the flatten pass)
  uint32_t* stat32;          // = (uint32_t*)(stat + 4): [0] the largest weight, [1] the error word
};

__global__ void __launch_bounds__(VC_SNN_BLOCK) vc_snn_init_kernel(uint32_t* __restrict__ labels, uint64_t n, uint32_t id_base) {
  for (uint64_t i = (uint64_t)blockIdx.x * VC_SNN_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * VC_SNN_BLOCK) labels[i] = id_base + (uint32_t)i;
}

__device__ __forceinline__ uint32_t snn_count(const SnnArgs& a, uint64_t i) { return a.counts ? a.counts[i] : a.uniform; }

// the team's LDS writes so far are seen by its reads from here on.  One wave: its LDS operations complete in program order, the
// fence keeps the compiler from moving them and waits for them.  One block: the barrier.
template <int TEAM_WAVES>
__device__ __forceinline__ void snn_team_sync() {
  if (TEAM_WAVES == 1) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
}

// position x (below n, so never the empty word) into the set; a second copy of x finds the first and stops
__device__ __forceinline__ void snn_insert(uint32_t* tab, uint32_t mask, uint32_t shift, uint32_t x) {
  uint32_t h = vc_snn_slot(x, shift);
  for (;;) {                                                  // at most kk insertions into >= 2 kk slots: an empty slot is always ahead
    const uint32_t old = atomicCAS(tab + h, VC_SNN_PLAN_NONE, x);
    if (old == VC_SNN_PLAN_NONE || old == x) return;
    h = (h + 1) & mask;
  }
}
__device__ __forceinline__ bool snn_holds(const uint32_t* tab, uint32_t mask, uint32_t shift, uint32_t x) {
  uint32_t h = vc_snn_slot(x, shift);
  for (;;) {
    const uint32_t s = tab[h];
    if (s == x) return true;
    if (s == VC_SNN_PLAN_NONE) return false;
    h = (h + 1) & mask;
  }
}

// words t and t + P of row j's first m_j entries (a lane whose word lies beyond them loads nothing)
__device__ __forceinline__ void snn_fetch(const SnnArgs& a, uint32_t j, uint32_t mj, uint32_t t, uint32_t P, uint64_t& w0, uint64_t& w1) {
  const uint64_t* __restrict__ row_j = a.rows + (uint64_t)j * a.k;
  if (t < mj) w0 = row_j[t];
  if (t + P < mj) w1 = row_j[t + P];
}
// entry w of row j is listed and row i lists the same record
__device__ __forceinline__ bool snn_hit(const SnnArgs& a, const uint32_t* tab, uint32_t mask, uint64_t w) {
  const uint32_t x = (uint32_t)w - a.id_base;
  return (uint32_t)(w >> 32) <= a.max_dist && (uint64_t)x < a.n && snn_holds(tab, mask, a.shift, x);
}
// TEAM_WAVES waves serve row i; a block holds VC_SNN_BLOCK / 64 / TEAM_WAVES teams, and its teams walk the rows with the grid's
// stride.  Every loop bound below is uniform over the team, so every lane of it reaches every ballot and every team_sync.
// A count above k, an id outside the store or the row's own id raises the error word and is passed over: nothing is read or
// written out of bounds.  A row that lists an id twice puts it into the set once; its weights are then whatever the loops give.
template <int TEAM_WAVES>
__global__ void __launch_bounds__(VC_SNN_BLOCK) vc_snn_kernel(const SnnArgs a) {
  constexpr uint32_t TEAMS = VC_SNN_BLOCK / VC_SNN_WAVE / TEAM_WAVES;
  constexpr uint32_t SLOTS = TEAM_WAVES == 1 ? VC_SNN_WAVE_SLOTS : VC_SNN_BLOCK_SLOTS;
  constexpr uint32_t HIST = TEAM_WAVES == 1 ? VC_SNN_WAVE_KK : VC_SNN_PLAN_MAX_KK;
  constexpr uint32_t TEAM_LANES = VC_SNN_WAVE * TEAM_WAVES;
  constexpr uint32_t R = (TEAM_WAVES == 1 ? VC_SNN_WAVE_KK : VC_SNN_PLAN_MAX_KK / TEAM_WAVES) / VC_SNN_WAVE;   // entries of a row a lane holds: 2, 4
  static_assert((R == 2 || R == 4) && R * VC_SNN_WAVE * TEAM_WAVES >= (TEAM_WAVES == 1 ? VC_SNN_WAVE_KK : VC_SNN_PLAN_MAX_KK), "a wave's lanes hold its share of the widest row");
  __shared__ uint32_t s_tab[TEAMS * SLOTS];
  __shared__ uint32_t s_hist[HIST];
  static_assert(sizeof(s_tab) + sizeof(s_hist) == (TEAM_WAVES == 1 ? VC_SNN_LDS_BYTES_WAVE : VC_SNN_LDS_BYTES_BLOCK), "the plan's LDS bytes");

  const uint32_t lane = vc_lane();
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / VC_SNN_WAVE));
  const uint32_t team = wave / TEAM_WAVES, team_wave = wave % TEAM_WAVES, team_lane = team_wave * VC_SNN_WAVE + lane;
  uint32_t* tab = s_tab + team * SLOTS;
  const uint32_t slots = 1u << (32 - a.shift), mask = slots - 1;     // vc_snn_table_slots(kk) <= SLOTS
  const uint32_t P = a.lanes, G = VC_SNN_WAVE / P;                    // lanes per entry, entries per pass of a wave
  const uint32_t gshift = (uint32_t)__ffs((int)G) - 1;                  // G is a power of two
  const uint32_t group = lane / P, sub = lane % P;
  const uint64_t gmask = (P == VC_SNN_WAVE ? ~0ull : ((1ull << P) - 1)) << (group * P);
  const bool with_hist = a.hist != nullptr;

  if (with_hist) {
    for (uint32_t s = threadIdx.x; s < a.kk; s += VC_SNN_BLOCK) s_hist[s] = 0u;
    __syncthreads();
  }
  uint32_t edges = 0, mutuals = 0, joins = 0;   // wave-uniform
  uint32_t best = 0;                            // per lane
  bool bad = false;
  for (uint64_t i = (uint64_t)blockIdx.x * TEAMS + team; i < a.n; i += (uint64_t)gridDim.x * TEAMS) {   // (team-uniform)
    const uint32_t ci = snn_count(a, i);
    bad |= ci > a.k;
    const uint32_t mi = ci > a.k ? 0u : vc_kgraph_edge_entries(a.kk, ci);
    const uint64_t* __restrict__ row_i = a.rows + i * a.k;
    const uint32_t own = a.id_base + (uint32_t)i;
    // PHASE A, a lane per entry: wave-local entry e = lane + 64 r is entry g = e % G of the wave's pass q = e / G, entry
    // jj = (q TEAM_WAVES + team_wave) G + g of the row.  Its words -- the entry, row j's count, the last of row j's listed
    // entries for the one compare -- are loaded for all entries at once, so their misses overlap each other and the set's build.
    uint32_t e_jj[R], e_j[R], e_mj[R], e_flag[R], e_hits[R];               // flag: 1 the entry exists, 2 it is listed, 4 j lists i
    for (uint32_t s = team_lane; s < slots; s += TEAM_LANES) tab[s] = VC_SNN_PLAN_NONE;
    auto load_entry = [&](const uint32_t r) __attribute__((always_inline)) {
      const uint32_t e = lane + VC_SNN_WAVE * r, jj = (((e >> gshift) * TEAM_WAVES + team_wave) << gshift) + (e & (G - 1));
      e_jj[r] = jj; e_j[r] = 0; e_mj[r] = 0; e_flag[r] = 0; e_hits[r] = 0;
      if (jj < mi) {
        const uint64_t v = row_i[jj];
        const uint32_t d = (uint32_t)(v >> 32), j = (uint32_t)v - a.id_base;
        e_flag[r] = 1u;
        if ((uint64_t)j >= a.n || (uint64_t)j == i) {
          bad = true;
        } else if (d <= a.max_dist) {
          const uint32_t cj = snn_count(a, j), mj = cj > a.k ? 0u : vc_kgraph_edge_entries(a.kk, cj);
          e_j[r] = j; e_mj[r] = mj; e_flag[r] = 3u;
          if (mj && vc_kgraph_lists(a.rows[(uint64_t)j * a.k + mj - 1], d, own)) e_flag[r] = 7u;
        }
      }
    };
    load_entry(0); load_entry(1);                                          // (spelled out: the registers are never indexed)
    if constexpr (R > 2) { load_entry(2); load_entry(3); }
    snn_team_sync<TEAM_WAVES>();
    // the set of row i
    for (uint32_t jj = team_lane; jj < mi; jj += TEAM_LANES) {
      const uint64_t v = row_i[jj];
      const uint32_t j = (uint32_t)v - a.id_base;
      if ((uint64_t)j < a.n && (uint64_t)j != i && (uint32_t)(v >> 32) <= a.max_dist) snn_insert(tab, mask, a.shift, j);
    }
    snn_team_sync<TEAM_WAVES>();
    // PHASE B, the wave's passes in turn, G entries per pass, P lanes per entry: (j, m_j) come from the entry's lane, two words of
    // row j per lane are loaded at a time, and the first two of the NEXT pass before the set is probed for this one
    const uint32_t npass = mi > team_wave * G ? (mi - team_wave * G + G * TEAM_WAVES - 1) / (G * TEAM_WAVES) : 0u;   // <= 64 R / G
    uint32_t cj = 0, cm = 0;
    uint64_t c0 = 0, c1 = 0;
    if (npass) {
      cj = (uint32_t)__shfl((int)e_j[0], (int)group, VC_WAVE);
      cm = (uint32_t)__shfl((int)e_mj[0], (int)group, VC_WAVE);
      snn_fetch(a, cj, cm, sub, P, c0, c1);
    }
    for (uint32_t q = 0; q < npass; ++q) {                                 // (wave-uniform)
      uint32_t nj = 0, nm = 0;
      uint64_t n0 = 0, n1 = 0;
      if (q + 1 < npass) {
        const uint32_t e0 = (q + 1) << gshift, r = e0 / VC_SNN_WAVE, src = (e0 % VC_SNN_WAVE) + group;
        uint32_t pj = r == 1 ? e_j[1] : e_j[0], pm = r == 1 ? e_mj[1] : e_mj[0];   // (r is wave-uniform; the registers are never indexed)
        if constexpr (R > 2) {
          pj = r == 2 ? e_j[2] : r == 3 ? e_j[3] : pj;
          pm = r == 2 ? e_mj[2] : r == 3 ? e_mj[3] : pm;
        }
        nj = (uint32_t)__shfl((int)pj, (int)src, VC_WAVE);
        nm = (uint32_t)__shfl((int)pm, (int)src, VC_WAVE);
        snn_fetch(a, nj, nm, sub, P, n0, n1);
      }
      uint32_t hits = 0;
      for (uint32_t t0 = 0; t0 < a.kk; t0 += 2 * P) {                      // (wave-uniform: m_j <= kk for every entry)
        if (t0) snn_fetch(a, cj, cm, t0 + sub, P, c0, c1);
        const bool h0 = t0 + sub < cm && snn_hit(a, tab, mask, c0);
        const bool h1 = t0 + sub + P < cm && snn_hit(a, tab, mask, c1);
        hits += (uint32_t)__popcll(__ballot(h0) & gmask) + (uint32_t)__popcll(__ballot(h1) & gmask);
      }
      // the weights go home to the entries' lanes: lane base + g takes group g's sum
      const uint32_t e0 = q << gshift, r = e0 / VC_SNN_WAVE, base = e0 % VC_SNN_WAVE;
      const uint32_t got = (uint32_t)__shfl((int)hits, (int)(((lane - base) & (G - 1)) * P), VC_WAVE);
      const bool mine = lane - base < G;
      e_hits[0] = (mine && r == 0) ? got : e_hits[0];
      e_hits[1] = (mine && r == 1) ? got : e_hits[1];
      if constexpr (R > 2) {
        e_hits[2] = (mine && r == 2) ? got : e_hits[2];
        e_hits[3] = (mine && r == 3) ? got : e_hits[3];
      }
      cj = nj; cm = nm; c0 = n0; c1 = n1;
    }
    // PHASE C, a lane per entry again: the weight, the histogram, the sums, the union
    auto finish_entry = [&](const uint32_t r) __attribute__((always_inline)) {
      const uint32_t hits = e_hits[r], other = a.id_base + e_j[r];
      const bool edge = (e_flag[r] & 2u) != 0u, mutual = (e_flag[r] & 4u) != 0u;
      if ((e_flag[r] & 1u) && a.shared) a.shared[i * a.kk + e_jj[r]] = edge ? hits : VC_SNN_PLAN_NONE;
      if (edge) {
        best = max(best, hits);
        if (with_hist && hits < a.kk) atomicAdd(s_hist + hits, 1u);        // (hits == kk only in a row that is no graph row)
      }
      const bool enough = edge && hits >= a.min_shared;
      edges += (uint32_t)__popcll(__ballot(edge));
      mutuals += (uint32_t)__popcll(__ballot(edge && mutual && own < other));
      joins += (uint32_t)__popcll(__ballot(enough && (mutual ? own < other : a.either != 0u)));
      if (enough && (a.either || mutual)) cl_unite(a.labels, a.id_base, own, other);
    };
    finish_entry(0); finish_entry(1);
    if constexpr (R > 2) { finish_entry(2); finish_entry(3); }
    if (a.shared)
      for (uint32_t jj = mi + team_lane; jj < a.kk; jj += TEAM_LANES) a.shared[i * a.kk + jj] = VC_SNN_PLAN_NONE;
    snn_team_sync<TEAM_WAVES>();                                           // the set is cleared for the next row only after every probe
  }
  if (bad) a.stat32[1] = 1u;
  for (int o = VC_WAVE / 2; o; o >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, o, VC_WAVE));
  if (lane == 0) {
    if (edges) atomicAdd(a.stat, (unsigned long long)edges);
    if (mutuals) atomicAdd(a.stat + 1, (unsigned long long)mutuals);
    if (joins) atomicAdd(a.stat + 2, (unsigned long long)joins);
    if (best) atomicMax(a.stat32, best);
  }
  if (with_hist) {
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < a.kk; s += VC_SNN_BLOCK) {
      const uint32_t c = s_hist[s];
      if (c) atomicAdd(a.hist + s, (unsigned long long)c);
    }
  }
}

uint32_t snn_init_grid(uint64_t n) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n + VC_SNN_BLOCK - 1) / VC_SNN_BLOCK, 1), 256 * 8); }

}  // namespace

#define SNN_HIP(call) VC_HIP_OR_FAIL("SNN clusters", call)

int vc_cluster_snn_run(const VcStoreView& v, const VcSnnArgs& a, vc_cluster_snn_stats* stats, hipStream_t s, std::string* err) {
  uint64_t* d_stat = (uint64_t*)v.alloc(VC_SNN_STAT, VC_SNN_STAT_BYTES);
  if (!d_stat) return VC_ERR_NOMEM;
  SNN_HIP(hipMemsetAsync(d_stat, 0, VC_SNN_STAT_BYTES, s));
  if (a.d_hist) SNN_HIP(hipMemsetAsync(a.d_hist, 0, (size_t)a.kk * 8, s));
  SnnArgs sa{};
  sa.rows = a.d_rows; sa.counts = a.d_counts; sa.n = v.n; sa.k = a.k; sa.kk = a.kk; sa.either = (a.flags & VC_KNN_EITHER) ? 1u : 0u;
  sa.max_dist = a.max_dist; sa.min_shared = a.min_shared; sa.id_base = v.id_base; sa.uniform = vc_kgraph_row_count(v.n, a.k);
  sa.shift = vc_snn_table_shift(a.kk); sa.lanes = vc_snn_entry_lanes(a.kk);
  sa.labels = a.d_labels; sa.shared = a.d_shared; sa.hist = (unsigned long long*)a.d_hist;
  sa.stat = (unsigned long long*)d_stat; sa.stat32 = (uint32_t*)(d_stat + 4);
  hipLaunchKernelGGL(vc_snn_init_kernel, dim3(snn_init_grid(v.n)), dim3(VC_SNN_BLOCK), 0, s, a.d_labels, v.n, v.id_base);
  SNN_HIP(hipGetLastError());
  if (vc_snn_wave_team(a.kk)) hipLaunchKernelGGL(vc_snn_kernel<1>, dim3(vc_snn_grid(v.n, a.kk)), dim3(VC_SNN_BLOCK), 0, s, sa);
  else hipLaunchKernelGGL(vc_snn_kernel<4>, dim3(vc_snn_grid(v.n, a.kk)), dim3(VC_SNN_BLOCK), 0, s, sa);
  SNN_HIP(hipGetLastError());
  SNN_HIP(vc_launch_cluster_flatten(a.d_labels, v.n, v.id_base, d_stat + 3, s));
  // THE WAIT: the statistics and the error word, 40 bytes
  struct { uint64_t n_edges, n_mutual, n_joined, n_clusters; uint32_t max_shared, bad; } home{};
  static_assert(sizeof(home) == VC_SNN_STAT_BYTES, "the statistics block as it lies");
  SNN_HIP(hipMemcpyAsync(&home, d_stat, VC_SNN_STAT_BYTES, hipMemcpyDeviceToHost, s));
  SNN_HIP(hipStreamSynchronize(s));
  if (home.bad) {
    if (err) *err = "SNN clusters: a count above k, an id outside the store or a row's own id -- not a graph vc_knn_graph built for this store";
    return VC_ERR_INVALID;
  }
  if (stats) *stats = vc_cluster_snn_stats{home.n_edges, home.n_mutual, home.n_joined, home.n_clusters, home.max_shared, 0u};
  return VC_OK;
}

int vc_cluster_snn_run_host(const VcStoreView& v, VcSnnArgs a, const uint64_t* rows, const uint32_t* counts, uint32_t* labels, uint32_t* shared, uint64_t* hist,
                            vc_cluster_snn_stats* stats, hipStream_t s, std::string* err) {
  const size_t n = (size_t)v.n;
  const VcSnnStage L(n, a.k, a.kk, counts != nullptr, shared != nullptr, hist != nullptr);
  uint8_t* stage = (uint8_t*)v.alloc(VC_SNN_STAGE, (size_t)L.total);
  uint32_t* d_labels = (uint32_t*)v.alloc(VC_SNN_HLAB, n * 4);
  if (!stage || !d_labels) return VC_ERR_NOMEM;
  uint64_t* d_rows = (uint64_t*)(stage + L.rows);
  uint32_t* d_cnt = (uint32_t*)(stage + L.counts);
  SNN_HIP(hipMemcpyAsync(d_rows, rows, n * a.k * 8, hipMemcpyHostToDevice, s));
  if (counts) SNN_HIP(hipMemcpyAsync(d_cnt, counts, n * 4, hipMemcpyHostToDevice, s));
  a.d_rows = d_rows; a.d_counts = counts ? d_cnt : nullptr; a.d_labels = d_labels;
  a.d_shared = shared ? (uint32_t*)(stage + L.shared) : nullptr;
  a.d_hist = hist ? (uint64_t*)(stage + L.hist) : nullptr;
  const int rc = vc_cluster_snn_run(v, a, stats, s, err);
  if (rc) return rc;
  SNN_HIP(hipMemcpyAsync(labels, d_labels, n * 4, hipMemcpyDeviceToHost, s));
  if (shared) SNN_HIP(hipMemcpyAsync(shared, a.d_shared, n * a.kk * 4, hipMemcpyDeviceToHost, s));
  if (hist) SNN_HIP(hipMemcpyAsync(hist, a.d_hist, (size_t)a.kk * 8, hipMemcpyDeviceToHost, s));
  SNN_HIP(hipStreamSynchronize(s));
  return VC_OK;
}
