// ============================================================================
// vc_knn_mst.hip -- the minimum spanning forest of a built k-NN graph in Kruskal order (vc_knn_mst*, vc_sharded_knn_mst*) and the
// components of an edge list under a weight cut (vc_mst_cut*, vc_sharded_mst_cut*); the header states the contract.  One driver for
// both handle kinds over a VcStoreView; the plan arithmetic -- the key, the home rule, the sizes -- is vc_knn_mst_plan.hpp.
// Boruvka on the device.  The order of the edges is strict (one 64-bit key per edge), so the forest is unique and no round closes a cycle.
//   vc_mst_init_kernel       forest[i] = comp[i] = id_base + i, best[i] = all ones
//   vc_mst_enumerate_kernel  thread e serves entry e % kk of record e / kk (vc_kgraph_edge_kernel's layout, tests and error word): the
//                            one compare, the home rule, the weight; every HOME entry is appended to the live list (key, pos b) by
//                            ballot rank, one cursor bump per wave
//   vc_mst_min_kernel        a round, per live edge: the two component ids of the round's snapshot; an edge inside one component is
//                            dropped, every other is appended to the other live buffer and offered to best[ca] and best[cb] -- a
//                            relaxed load in front of each 64-bit atomicMin, so a hub or a giant component does not serialise on one word
//   vc_mst_hook_kernel       per component with a pick: the key decoded, the edge appended to the picked list exactly once (the pick of
//                            ca is written iff it is not also cb's pick, or ca < cb), the two trees united by vc_forest.hpp's cl_unite
//   vc_mst_flatten_kernel    comp[i] = the root of i with path halving, best[i] = all ones again
//   vc_mst_write_kernel      after vc_sort.hip's stable radix sort of the picked list by (weight, home index): vc_mst_edge t, the
//                            histogram (LDS counters, one global atomic per block and bin), the total and the largest weight
//   vc_mst_cut_kernel        vc_mst_cut*: an end outside the store raises the error word; an edge within the cut is united
// The host reads the 48-byte block once per round (the picked count ends the loop, the error word comes with the first) and once at
// the end.  Static LDS in the write launch only, no scratch memory, no cooperative launch.
// ============================================================================
#include <algorithm>

#include "vc_forest.hpp"
#include "vc_internal.hpp"
#include "vc_knn_graph_plan.hpp"
#include "vc_knn_mst_plan.hpp"

static_assert(VC_MST_MUTUAL == VC_KNN_MUTUAL && VC_MST_EITHER == VC_KNN_EITHER, "the header's flags");
static_assert(VC_MST_KIND_DISTANCE == VC_MST_DISTANCE && VC_MST_KIND_REACHABILITY == VC_MST_REACHABILITY, "the header's weight kinds");
static_assert(sizeof(vc_knn_mst_stats) == VC_MST_HOST_STAT_BYTES && sizeof(vc_mst_edge) == VC_MST_EDGE_BYTES, "the header's sizes");

namespace {

// the device's block; the host reads it as it lies
struct VcMstStat {
  unsigned long long n_edges, n_graph_edges, total_weight;
  uint32_t picked;       // the picked list's cursor: M at the end
  uint32_t live[2];      // the cursors of the two live buffers
  uint32_t max_weight, bad, pad;
};
static_assert(sizeof(VcMstStat) == VC_MST_STAT_BYTES, "the statistics block as it lies");

// what the launches work on
struct MstArgs {
  const uint64_t* rows;      // [n][k]
  const uint32_t* counts;    // [n], nullable: every row holds `uniform` entries
  uint64_t n;
  uint32_t k, kk, flags, max_dist, id_base, uniform, min_pts, bits;
  uint32_t* forest;          // [n]: the forest of vc_forest.hpp, global ids
  uint32_t* comp;            // [n]: the round's snapshot, the root (smallest global id) of every record's component
  unsigned long long* best;  // [n]: the smallest key that leaves the component rooted here
  uint64_t* live_key[2];     // [live_cap] each
  uint32_t* live_b[2];
  uint32_t live_cap;
  uint32_t* pick_w;          // [pick_cap]: the picked edges' weights, the sort's keys
  uint64_t* pick_home;       // [pick_cap]: home index << 32, the sort's values
  uint32_t pick_cap;
  VcMstStat* stat;
};

__device__ __forceinline__ uint32_t mst_count(const MstArgs& a, uint64_t i) { return a.counts ? a.counts[i] : a.uniform; }

// j lists i: vc_cluster_knn*'s one compare against the last of row j's first min(kk, count_j) entries (d <= max_dist holds already)
__device__ __forceinline__ bool mst_listed_back(const MstArgs& a, uint32_t j, uint32_t d, uint32_t own) {
  const uint32_t cj = mst_count(a, j), mj = vc_kgraph_edge_entries(a.kk, cj);
  return cj <= a.k && mj && vc_kgraph_lists(a.rows[(uint64_t)j * a.k + mj - 1], d, own);
}
// the core distance of record i (min_pts >= 2): entry min_pts - 2 of the k columns, whatever kk and max_dist are
__device__ __forceinline__ uint32_t mst_core(const MstArgs& a, uint64_t i) {
  const uint32_t ci = mst_count(a, i);
  return ci <= a.k && vc_mst_core_held(ci, a.min_pts) ? (uint32_t)(a.rows[i * a.k + a.min_pts - 2] >> 32) : a.bits;
}
// The lanes with `take` get consecutive places behind *cursor, in lane order; one atomic per wave.  Every lane of the wave calls.
__device__ __forceinline__ uint32_t mst_place(bool take, uint32_t* cursor) {
  const uint64_t m = __ballot(take);
  if (!m) return 0;
  const uint32_t lane = vc_lane();
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(cursor, (uint32_t)__popcll(m));
  base = (uint32_t)__shfl((int)base, 0, VC_WAVE);
  return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}
__device__ __forceinline__ void mst_offer(unsigned long long* slot, unsigned long long key) {
  if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(slot, key);
}

__global__ void __launch_bounds__(VC_MST_BLOCK) vc_mst_init_kernel(const MstArgs a) {
  for (uint64_t i = (uint64_t)blockIdx.x * VC_MST_BLOCK + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * VC_MST_BLOCK) {
    a.forest[i] = a.comp[i] = a.id_base + (uint32_t)i;
    a.best[i] = VC_MST_NONE;
  }
}

// A count above k, an id outside the store or the row's own id raises the error word and is passed over: nothing is read or written
// out of bounds.  A live list that would outgrow its buffer -- no vc_knn_graph* rows do that -- raises it too.
__global__ void __launch_bounds__(VC_MST_BLOCK) vc_mst_enumerate_kernel(const MstArgs a) {
  const uint64_t total = a.n * a.kk;
  uint32_t edges = 0, homes = 0;   // wave-uniform
  for (uint64_t e0 = (uint64_t)blockIdx.x * VC_MST_BLOCK; e0 < total; e0 += (uint64_t)gridDim.x * VC_MST_BLOCK) {   // (block-uniform bounds: every lane votes)
    const uint64_t e = e0 + threadIdx.x;
    bool edge = false, home = false, bad = false;
    uint64_t key = 0;
    uint32_t pb = 0;
    if (e < total) {
      const uint64_t i = e / a.kk;
      const uint32_t jj = (uint32_t)(e % a.kk), ci = mst_count(a, i);
      bad = ci > a.k;
      if (!bad && jj < vc_kgraph_edge_entries(a.kk, ci)) {
        const uint64_t v = a.rows[i * a.k + jj];
        const uint32_t d = (uint32_t)(v >> 32), j = (uint32_t)v - a.id_base;
        if ((uint64_t)j >= a.n || (uint64_t)j == i) {
          bad = true;
        } else if (d <= a.max_dist) {
          edge = true;
          home = vc_mst_is_home(a.flags, i < (uint64_t)j, mst_listed_back(a, j, d, a.id_base + (uint32_t)i));
          if (home) {
            const uint32_t w = a.min_pts > 1 ? vc_mst_weight(d, mst_core(a, i), mst_core(a, j)) : d;
            key = vc_mst_key(w, i, a.kk, jj);
            pb = j;
          }
        }
      }
    }
    edges += (uint32_t)__popcll(__ballot(edge));
    homes += (uint32_t)__popcll(__ballot(home));
    const uint32_t at = mst_place(home, &a.stat->live[0]);
    if (home) {
      if (at < a.live_cap) {
        a.live_key[0][at] = key;
        a.live_b[0][at] = pb;
      } else {
        bad = true;
      }
    }
    if (bad) a.stat->bad = 1u;
  }
  if (vc_lane() == 0) {
    if (edges) atomicAdd(&a.stat->n_edges, (unsigned long long)edges);
    if (homes) atomicAdd(&a.stat->n_graph_edges, (unsigned long long)homes);
  }
}

// live buffer `src` -> the edges between two components of the snapshot, into buffer src ^ 1 and into best[]
__global__ void __launch_bounds__(VC_MST_BLOCK) vc_mst_min_kernel(const MstArgs a, const uint32_t src) {
  const uint32_t L = min(a.stat->live[src], a.live_cap), dst = src ^ 1u;
  const uint64_t* __restrict__ keys = a.live_key[src];
  const uint32_t* __restrict__ ends = a.live_b[src];
  for (uint32_t e0 = blockIdx.x * VC_MST_BLOCK; e0 < L; e0 += gridDim.x * VC_MST_BLOCK) {   // (block-uniform)
    const uint32_t e = e0 + threadIdx.x;
    bool alive = false;
    uint64_t key = 0;
    uint32_t b = 0;
    if (e < L) {
      key = keys[e];
      b = ends[e];
      const uint32_t ca = a.comp[vc_mst_home_pos(vc_mst_key_home(key), a.kk)], cb = a.comp[b];
      alive = ca != cb;
      if (alive) {
        mst_offer(a.best + (ca - a.id_base), key);
        mst_offer(a.best + (cb - a.id_base), key);
      }
    }
    const uint32_t at = mst_place(alive, &a.stat->live[dst]);   // at most L of them: in bounds
    if (alive) {
      a.live_key[dst][at] = key;
      a.live_b[dst][at] = b;
    }
  }
}

// Thread r serves the component rooted at position r, if a live edge leaves it.  best[] and comp[] are the round's and are only read
// here; the forest is only united.  A chain of any length may hook in one round: cl_unite takes every interleaving.
__global__ void __launch_bounds__(VC_MST_BLOCK) vc_mst_hook_kernel(const MstArgs a) {
  for (uint64_t r0 = (uint64_t)blockIdx.x * VC_MST_BLOCK; r0 < a.n; r0 += (uint64_t)gridDim.x * VC_MST_BLOCK) {   // (block-uniform)
    const uint64_t r = r0 + threadIdx.x;
    bool write = false;
    uint64_t key = VC_MST_NONE;
    uint32_t ca = 0, cb = 0;
    if (r < a.n) key = a.best[r];
    if (key != VC_MST_NONE) {
      const uint32_t home = vc_mst_key_home(key), pa = vc_mst_home_pos(home, a.kk);
      const uint32_t pb = (uint32_t)a.rows[(uint64_t)pa * a.k + vc_mst_home_entry(home, a.kk)] - a.id_base;   // the entry the enumeration accepted
      ca = a.comp[pa];
      cb = a.comp[pb];
      const uint32_t me = a.id_base + (uint32_t)r, other = me == ca ? cb : ca;
      write = a.best[other - a.id_base] != key || me < other;
    }
    const uint32_t at = mst_place(write, &a.stat->picked);
    if (write) {
      if (at < a.pick_cap) {   // a forest of n records has at most n - 1 edges
        a.pick_w[at] = vc_mst_key_weight(key);
        a.pick_home[at] = (uint64_t)vc_mst_key_home(key) << 32;
      } else {
        a.stat->bad = 1u;
      }
      cl_unite(a.forest, a.id_base, ca, cb);
    }
  }
}

__global__ void __launch_bounds__(VC_MST_BLOCK) vc_mst_flatten_kernel(const MstArgs a) {
  for (uint64_t i = (uint64_t)blockIdx.x * VC_MST_BLOCK + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * VC_MST_BLOCK) {
    const uint32_t root = cl_find_halving(a.forest, a.id_base, a.id_base + (uint32_t)i);
    cl_st(a.forest + i, root);   // an ancestor, as path halving stores one
    a.comp[i] = root;
    a.best[i] = VC_MST_NONE;
  }
}

// the sorted picked list -> the caller's edges, histogram and the two sums.  A weight above the code width -- no vc_knn_graph* row
// holds one -- is in no bin.
__global__ void __launch_bounds__(VC_MST_BLOCK) vc_mst_write_kernel(const MstArgs a, const uint32_t* __restrict__ weights, const uint64_t* __restrict__ homes,
                                                                    const uint32_t M, vc_mst_edge* __restrict__ out, unsigned long long* __restrict__ hist) {
  __shared__ uint32_t bins[VC_MST_MAX_BITS + 1];
  for (uint32_t b = threadIdx.x; b <= VC_MST_MAX_BITS; b += VC_MST_BLOCK) bins[b] = 0u;
  __syncthreads();
  unsigned long long sum = 0;
  uint32_t top = 0;
  for (uint32_t t = blockIdx.x * VC_MST_BLOCK + threadIdx.x; t < M; t += gridDim.x * VC_MST_BLOCK) {
    const uint32_t w = weights[t], home = (uint32_t)(homes[t] >> 32), pa = vc_mst_home_pos(home, a.kk);
    const uint64_t v = a.rows[(uint64_t)pa * a.k + vc_mst_home_entry(home, a.kk)];
    out[t].a = a.id_base + pa;
    out[t].b = (uint32_t)v;
    out[t].weight = w;
    out[t].dist = (uint32_t)(v >> 32);
    if (w <= a.bits && w <= VC_MST_MAX_BITS) atomicAdd(bins + w, 1u);
    sum += w;
    top = max(top, w);
  }
  __syncthreads();
  if (hist)
    for (uint32_t b = threadIdx.x; b <= a.bits && b <= VC_MST_MAX_BITS; b += VC_MST_BLOCK)
      if (bins[b]) atomicAdd(hist + b, (unsigned long long)bins[b]);
  for (int o = VC_WAVE / 2; o; o >>= 1) {
    top = max(top, (uint32_t)__shfl_xor((int)top, o, VC_WAVE));
    sum += ((unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)(sum >> 32), o, VC_WAVE) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)sum, o, VC_WAVE);
  }
  if (vc_lane() == 0) {
    if (sum) atomicAdd(&a.stat->total_weight, sum);
    if (top) atomicMax(&a.stat->max_weight, top);
  }
}

// vc_mst_cut*: stat[0] the clusters (the flatten pass), the low word of stat[1] the error word
__global__ void __launch_bounds__(VC_MST_BLOCK) vc_mst_cut_kernel(const vc_mst_edge* __restrict__ edges, uint64_t n_edges, uint32_t max_weight, uint64_t n,
                                                                  uint32_t id_base, uint32_t* labels, uint32_t* __restrict__ bad) {
  for (uint64_t t = (uint64_t)blockIdx.x * VC_MST_BLOCK + threadIdx.x; t < n_edges; t += (uint64_t)gridDim.x * VC_MST_BLOCK) {
    const uint32_t ea = edges[t].a, eb = edges[t].b;
    if ((uint64_t)(uint32_t)(ea - id_base) >= n || (uint64_t)(uint32_t)(eb - id_base) >= n) *bad = 1u;
    else if (edges[t].weight <= max_weight) cl_unite(labels, id_base, ea, eb);
  }
}

uint32_t mst_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + VC_MST_BLOCK - 1) / VC_MST_BLOCK, 1), 256 * 8); }

}  // namespace

#define MST_HIP(call) VC_HIP_OR_FAIL("k-NN spanning forest", call)

int vc_knn_mst_run(const VcStoreView& v, const VcMstArgs& a, vc_knn_mst_stats* stats, hipStream_t s, std::string* err) {
  if (stats) *stats = vc_knn_mst_stats{};
  const uint64_t n = v.n;
  const uint32_t bits = 64 * v.W;
  if (n == 0) {
    if (a.d_hist) MST_HIP(hipMemsetAsync(a.d_hist, 0, ((size_t)bits + 1) * 8, s));
    return VC_OK;
  }
  // every buffer of the call, before the first launch
  const uint64_t live_cap = vc_mst_live_cap(n, a.kk, a.flags), pick_cap = vc_mst_pick_cap(n);
  const size_t word4 = (size_t)vc_mst_words4(n), live4 = (size_t)vc_mst_words4(live_cap), pick4 = (size_t)vc_mst_words4(pick_cap);
  VcMstStat* d_stat = (VcMstStat*)v.alloc(VC_MST_STAT, VC_MST_STAT_BYTES);
  uint8_t* d_forest = (uint8_t*)v.alloc(VC_MST_FOREST, (size_t)vc_mst_forest_bytes(n));
  uint8_t* d_live = (uint8_t*)v.alloc(VC_MST_LIVE, (size_t)vc_mst_live_bytes(n, a.kk, a.flags));
  uint8_t* d_pick = (uint8_t*)v.alloc(VC_MST_PICK, (size_t)vc_mst_pick_bytes(n));
  uint32_t* d_sort_work = (uint32_t*)v.alloc(VC_MST_SORT, vc_radix_sort_work_words(pick_cap) * 4);
  if (!d_stat || !d_forest || !d_live || !d_pick || !d_sort_work) return VC_ERR_NOMEM;
  MstArgs k{};
  k.rows = a.d_rows; k.counts = a.d_counts; k.n = n; k.k = a.k; k.kk = a.kk; k.flags = a.flags; k.max_dist = a.max_dist; k.id_base = v.id_base;
  k.uniform = vc_kgraph_row_count(n, a.k); k.min_pts = a.min_pts; k.bits = bits;
  k.best = (unsigned long long*)d_forest; k.forest = (uint32_t*)(d_forest + n * 8); k.comp = (uint32_t*)(d_forest + n * 8 + word4);
  k.live_key[0] = (uint64_t*)d_live; k.live_key[1] = k.live_key[0] + live_cap;
  k.live_b[0] = (uint32_t*)(d_live + 2 * live_cap * 8); k.live_b[1] = (uint32_t*)(d_live + 2 * live_cap * 8 + live4);
  k.live_cap = (uint32_t)live_cap;
  uint64_t* pick_vals[2] = {(uint64_t*)d_pick, (uint64_t*)d_pick + pick_cap};
  uint32_t* pick_keys[2] = {(uint32_t*)(d_pick + 2 * pick_cap * 8), (uint32_t*)(d_pick + 2 * pick_cap * 8 + pick4)};
  k.pick_w = pick_keys[0]; k.pick_home = pick_vals[0]; k.pick_cap = (uint32_t)vc_mst_pick_items(n);
  k.stat = d_stat;
  MST_HIP(hipMemsetAsync(d_stat, 0, VC_MST_STAT_BYTES, s));
  // 1. the forest of singletons and the live list of the home entries
  hipLaunchKernelGGL(vc_mst_init_kernel, dim3(mst_grid(n)), dim3(VC_MST_BLOCK), 0, s, k);
  MST_HIP(hipGetLastError());
  hipLaunchKernelGGL(vc_mst_enumerate_kernel, dim3(mst_grid(n * a.kk)), dim3(VC_MST_BLOCK), 0, s, k);
  MST_HIP(hipGetLastError());
  // 2. the rounds, one wait each: the picked count ends the loop, the error word comes with the first
  VcMstStat home{};
  uint32_t rounds = 0, picked = 0;
  uint64_t live = live_cap;   // an upper bound of the source buffer's length, exact from the second round on
  for (uint32_t r = 0;; ++r) {
    if (r > vc_mst_round_bound(n)) {
      if (err) *err = "k-NN spanning forest: more rounds than a forest of this size can take";
      return VC_ERR_STATE;
    }
    const uint32_t src = r & 1u;
    MST_HIP(hipMemsetAsync(&d_stat->live[src ^ 1u], 0, 4, s));
    hipLaunchKernelGGL(vc_mst_min_kernel, dim3(mst_grid(live)), dim3(VC_MST_BLOCK), 0, s, k, src);
    MST_HIP(hipGetLastError());
    hipLaunchKernelGGL(vc_mst_hook_kernel, dim3(mst_grid(n)), dim3(VC_MST_BLOCK), 0, s, k);
    MST_HIP(hipGetLastError());
    hipLaunchKernelGGL(vc_mst_flatten_kernel, dim3(mst_grid(n)), dim3(VC_MST_BLOCK), 0, s, k);
    MST_HIP(hipGetLastError());
    MST_HIP(hipMemcpyAsync(&home, d_stat, VC_MST_STAT_BYTES, hipMemcpyDeviceToHost, s));
    MST_HIP(hipStreamSynchronize(s));
    if (home.bad) {
      if (err) *err = "k-NN spanning forest: a count above k, an id outside the store or a row's own id -- not a graph vc_knn_graph built for this store";
      return VC_ERR_INVALID;
    }
    if (home.picked == picked) break;   // nothing hooked: every live edge lies inside a component
    picked = home.picked;
    ++rounds;
    live = home.live[src ^ 1u];
    if ((uint64_t)picked + 1 == n) break;   // one tree: no edge is left to pick
  }
  // 3. Kruskal order: the stable sort by (weight, home index), then the outputs
  const uint32_t M = picked;
  if (a.d_hist) MST_HIP(hipMemsetAsync(a.d_hist, 0, ((size_t)bits + 1) * 8, s));
  if (M) {
    const uint32_t home_bits = vc_mst_home_bits(n, a.kk), weight_bits = vc_mst_weight_bits(bits);
    MST_HIP(vc_radix_sort_items(pick_keys, pick_vals, M, home_bits, weight_bits, d_sort_work, s));
    const uint32_t at = vc_radix_sort_item_passes(home_bits, weight_bits) & 1u;
    hipLaunchKernelGGL(vc_mst_write_kernel, dim3(mst_grid(M)), dim3(VC_MST_BLOCK), 0, s, k, (const uint32_t*)pick_keys[at], (const uint64_t*)pick_vals[at], M, a.d_edges,
                       (unsigned long long*)a.d_hist);
    MST_HIP(hipGetLastError());
  }
  if (a.d_labels) MST_HIP(hipMemcpyAsync(a.d_labels, k.comp, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  // THE LAST WAIT: the two sums
  MST_HIP(hipMemcpyAsync(&home, d_stat, VC_MST_STAT_BYTES, hipMemcpyDeviceToHost, s));
  MST_HIP(hipStreamSynchronize(s));
  if (stats) *stats = vc_knn_mst_stats{home.n_edges, home.n_graph_edges, M, n - M, home.total_weight, home.max_weight, rounds};
  return VC_OK;
}

int vc_knn_mst_run_host(const VcStoreView& v, VcMstArgs a, const uint64_t* rows, const uint32_t* counts, vc_mst_edge* edges, uint32_t* labels, uint64_t* hist,
                        vc_knn_mst_stats* stats, hipStream_t s, std::string* err) {
  const size_t n = (size_t)v.n, bits = 64 * (size_t)v.W;
  if (n == 0) {
    if (stats) *stats = vc_knn_mst_stats{};
    if (hist) std::fill(hist, hist + bits + 1, 0ull);
    return VC_OK;
  }
  const VcMstStage L(n, a.k, (uint32_t)bits, counts != nullptr);
  uint8_t* stage = (uint8_t*)v.alloc(VC_MST_STAGE, (size_t)L.total);
  if (!stage) return VC_ERR_NOMEM;
  uint64_t* d_rows = (uint64_t*)(stage + L.rows);
  uint32_t* d_cnt = (uint32_t*)(stage + L.counts);
  MST_HIP(hipMemcpyAsync(d_rows, rows, n * a.k * 8, hipMemcpyHostToDevice, s));
  if (counts) MST_HIP(hipMemcpyAsync(d_cnt, counts, n * 4, hipMemcpyHostToDevice, s));
  a.d_rows = d_rows; a.d_counts = counts ? d_cnt : nullptr;
  a.d_edges = (vc_mst_edge*)(stage + L.edges);
  a.d_labels = labels ? (uint32_t*)(stage + L.labels) : nullptr;
  a.d_hist = hist ? (uint64_t*)(stage + L.hist) : nullptr;
  vc_knn_mst_stats st{};
  const int rc = vc_knn_mst_run(v, a, &st, s, err);
  if (rc) return rc;
  if (stats) *stats = st;
  if (st.n_tree) MST_HIP(hipMemcpyAsync(edges, a.d_edges, (size_t)st.n_tree * VC_MST_EDGE_BYTES, hipMemcpyDeviceToHost, s));
  if (labels) MST_HIP(hipMemcpyAsync(labels, a.d_labels, n * 4, hipMemcpyDeviceToHost, s));
  if (hist) MST_HIP(hipMemcpyAsync(hist, a.d_hist, (bits + 1) * 8, hipMemcpyDeviceToHost, s));
  MST_HIP(hipStreamSynchronize(s));
  return VC_OK;
}

#undef MST_HIP
#define MST_HIP(call) VC_HIP_OR_FAIL("spanning forest cut", call)

int vc_mst_cut_run(const VcStoreView& v, const vc_mst_edge* d_edges, uint64_t n_edges, uint32_t max_weight, uint32_t* d_labels, uint64_t* n_clusters, hipStream_t s,
                   std::string* err) {
  if (n_clusters) *n_clusters = 0;
  if (v.n == 0) return VC_OK;
  uint64_t* d_stat = (uint64_t*)v.alloc(VC_MST_STAT, VC_MST_STAT_BYTES);
  if (!d_stat) return VC_ERR_NOMEM;
  MST_HIP(hipMemsetAsync(d_stat, 0, 16, s));
  MST_HIP(vc_launch_cluster_init(d_labels, v.n, v.id_base, s));
  if (n_edges) {
    hipLaunchKernelGGL(vc_mst_cut_kernel, dim3(mst_grid(n_edges)), dim3(VC_MST_BLOCK), 0, s, d_edges, n_edges, max_weight, v.n, v.id_base, d_labels, (uint32_t*)(d_stat + 1));
    MST_HIP(hipGetLastError());
  }
  MST_HIP(vc_launch_cluster_flatten(d_labels, v.n, v.id_base, d_stat, s));
  uint64_t home[2] = {0, 0};   // THE WAIT: the clusters and the error word
  MST_HIP(hipMemcpyAsync(home, d_stat, 16, hipMemcpyDeviceToHost, s));
  MST_HIP(hipStreamSynchronize(s));
  if (home[1]) {
    if (err) *err = "spanning forest cut: an edge names a record outside the store";
    return VC_ERR_INVALID;
  }
  if (n_clusters) *n_clusters = home[0];
  return VC_OK;
}

int vc_mst_cut_run_host(const VcStoreView& v, const vc_mst_edge* edges, uint64_t n_edges, uint32_t max_weight, uint32_t* labels, uint64_t* n_clusters, hipStream_t s,
                        std::string* err) {
  if (v.n == 0) {
    if (n_clusters) *n_clusters = 0;
    return VC_OK;
  }
  const size_t n = (size_t)v.n;
  const VcMstCutStage L(n, n_edges);
  uint8_t* stage = (uint8_t*)v.alloc(VC_MST_STAGE, (size_t)std::max<uint64_t>(L.total, 8));
  if (!stage) return VC_ERR_NOMEM;
  vc_mst_edge* d_edges = (vc_mst_edge*)(stage + L.edges);
  uint32_t* d_labels = (uint32_t*)(stage + L.labels);
  if (n_edges) MST_HIP(hipMemcpyAsync(d_edges, edges, (size_t)n_edges * VC_MST_EDGE_BYTES, hipMemcpyHostToDevice, s));
  const int rc = vc_mst_cut_run(v, d_edges, n_edges, max_weight, d_labels, n_clusters, s, err);
  if (rc) return rc;
  MST_HIP(hipMemcpyAsync(labels, d_labels, n * 4, hipMemcpyDeviceToHost, s));
  MST_HIP(hipStreamSynchronize(s));
  return VC_OK;
}
