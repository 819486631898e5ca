// ============================================================================
// vc_knn_adjacency.hip -- the reverse, mutual and symmetrised k-NN graph in CSR form (vc_knn_adjacency*, vc_sharded_knn_adjacency*);
// the header states the contract.  One driver for both handle kinds over a VcStoreView; the plan arithmetic is
// vc_knn_adjacency_plan.hpp.
//   vc_adj_enumerate_kernel<E>  VC_KNN_REVERSE / VC_KNN_EITHER: thread e serves entry e % kk of record e / kk (vc_kgraph_edge_kernel's
//                               layout, tests and error word) and writes sort item e: key = the target position, value =
//                               dist << 32 | id of the source; what is no item gets the sentinel key N; exact integer atomics
//                               bump the target's counter (EITHER: the one-sided in-part, and the whole segment of both ends)
//   vc_adj_mutual_kernel<F>     VC_KNN_MUTUAL: P lanes serve a row, 64 / P rows share a wave; the mutual entries of a row are counted
//                               by ballot (F = 0) and, after the scan, written in row order at the row's offset (F = 1)
//   vc_adj_degree_kernel        the sum, the largest and the zeros of the segment lengths
//   vc_adj_offsets_kernel       the scanned counters widened into d_offsets
//   vc_adj_merge_kernel         VC_KNN_EITHER: a wave per record (the block above VC_ADJ_TEAM_DEGREE) merges the row's listed entries
//                               with the record's run of the sorted in-part by rank counting; the two lists never share a word
// Between them vc_sort.hip's stable radix sort in its 64-bit-payload instantiation: first by the distance (digits of value >> 32),
// then by the key; the enumerate order is source-major, so equal (target, dist) stay in id order.  Nothing but scratch is written
// before the one wait.  No LDS of its own, no scratch memory, no cooperative launch.
// ============================================================================
#include <algorithm>

#include "vc_internal.hpp"
#include "vc_knn_adjacency_plan.hpp"
#include "vc_knn_graph_plan.hpp"

static_assert(VC_ADJ_MUTUAL == VC_KNN_MUTUAL && VC_ADJ_EITHER == VC_KNN_EITHER && VC_ADJ_REVERSE == VC_KNN_REVERSE, "the header's constants");
static_assert(sizeof(vc_knn_adjacency_stats) == VC_ADJ_STAT_BYTES, "the header's size");
static_assert(VC_ADJ_WAVE == VC_WAVE, "the plan's wave");

namespace {

// what the launches work on
struct AdjArgs {
  const uint64_t* rows;      // [n][k]
  const uint32_t* counts;    // [n], nullable: every row holds `uniform` entries
  uint64_t n;
  uint32_t k, kk, max_dist, id_base, uniform;
  uint32_t* cnt_in;          // [n + 1]: REVERSE the in-degrees, EITHER the one-sided in-part; after the scan their offsets
  uint32_t* cnt_seg;         // [n + 1]: the segment lengths (REVERSE: = cnt_in); after the scan the segments' offsets
  uint32_t* keys;            // [n kk], nullable (a sizing call writes no items)
  uint64_t* vals;            // [n kk]
  const uint64_t* sorted;    // [n kk]: the values after the sort (the merge)
  uint64_t* adj;             // the caller's (the mutual fill, the merge)
  unsigned long long* stat;  // [0] += edges, [1] the entries, [2] the empty segments
  uint32_t* stat32;          // = (uint32_t*)(stat + 3): [0] the longest segment, [1] the error word
};

__device__ __forceinline__ uint32_t adj_count(const AdjArgs& a, uint64_t i) { return a.counts ? a.counts[i] : a.uniform; }

// j lists i: vc_cluster_knn*'s one compare against the last of row j's first min(kk, count_j) entries (d <= max_dist holds already)
__device__ __forceinline__ bool adj_listed_back(const AdjArgs& a, uint32_t j, uint32_t d, uint32_t own) {
  const uint32_t cj = adj_count(a, j), mj = vc_kgraph_edge_entries(a.kk, cj);
  return cj <= a.k && mj && vc_kgraph_lists(a.rows[(uint64_t)j * a.k + mj - 1], d, own);
}

// A count above k, an id outside the store or the row's own id raises the error word and is passed over: nothing is read or written
// out of bounds.  The sum of the listed entries is one add per wave.
template <bool EITHER>
__global__ void __launch_bounds__(VC_ADJ_BLOCK) vc_adj_enumerate_kernel(const AdjArgs a) {
  const uint64_t total = a.n * a.kk;
  uint32_t edges = 0;   // wave-uniform
  for (uint64_t e0 = (uint64_t)blockIdx.x * VC_ADJ_BLOCK; e0 < total; e0 += (uint64_t)gridDim.x * VC_ADJ_BLOCK) {   // (block-uniform bounds: every lane votes)
    const uint64_t e = e0 + threadIdx.x;
    bool edge = false, bad = false;
    uint32_t key = (uint32_t)a.n;   // the sentinel: sorts behind every position
    uint64_t val = 0;
    if (e < total) {
      const uint64_t i = e / a.kk;
      const uint32_t jj = (uint32_t)(e % a.kk), ci = adj_count(a, i);
      bad = ci > a.k;
      if (!bad && jj < vc_kgraph_edge_entries(a.kk, ci)) {
        const uint64_t v = a.rows[i * a.k + jj];
        const uint32_t d = (uint32_t)(v >> 32), j = (uint32_t)v - a.id_base;
        if ((uint64_t)j >= a.n || (uint64_t)j == i) {
          bad = true;
        } else if (d <= a.max_dist) {
          const uint32_t own = a.id_base + (uint32_t)i;
          edge = true;
          bool item = true;
          if (EITHER) {
            atomicAdd(a.cnt_seg + i, 1u);                   // the row's own listed entry
            item = !adj_listed_back(a, j, d, own);          // a mutual pair is in row j already
            if (item) atomicAdd(a.cnt_seg + j, 1u);
          }
          if (item) {
            atomicAdd(a.cnt_in + j, 1u);
            key = j;
            val = ((uint64_t)d << 32) | own;
          }
        }
      }
      if (a.keys) {
        a.keys[e] = key;
        a.vals[e] = val;
      }
    }
    if (bad) a.stat32[1] = 1u;
    edges += (uint32_t)__popcll(__ballot(edge));
  }
  if (vc_lane() == 0 && edges) atomicAdd(a.stat, (unsigned long long)edges);
}

// VC_KNN_MUTUAL.  P = vc_adj_row_lanes(kk) lanes serve row i in passes of P entries; every loop bound is wave-uniform, so every lane
// reaches every ballot.  FILL = false counts (cnt_seg[i], the edges); FILL = true writes the mutual entries, which are ascending as
// the row is, at cnt_seg[i] -- by then the row's offset.
template <bool FILL>
__global__ void __launch_bounds__(VC_ADJ_BLOCK) vc_adj_mutual_kernel(const AdjArgs a, const uint32_t P) {
  const uint32_t lane = vc_lane(), wave = threadIdx.x / VC_ADJ_WAVE;
  const uint32_t G = VC_ADJ_WAVE / P, group = lane / P, sub = lane % P;
  const uint64_t gmask = (P == VC_ADJ_WAVE ? ~0ull : ((1ull << P) - 1)) << (group * P);
  const uint64_t below = gmask & ((1ull << lane) - 1ull);
  constexpr uint32_t WAVES = VC_ADJ_BLOCK / VC_ADJ_WAVE;
  uint32_t edges = 0;   // wave-uniform
  bool bad = false;
  for (uint64_t r0 = ((uint64_t)blockIdx.x * WAVES + wave) * G; r0 < a.n; r0 += (uint64_t)gridDim.x * WAVES * G) {   // (wave-uniform)
    const uint64_t i = r0 + group;
    const bool row = i < a.n;
    const uint32_t ci = row ? adj_count(a, i) : 0u;
    bad |= ci > a.k;
    const uint32_t mi = ci > a.k ? 0u : vc_kgraph_edge_entries(a.kk, ci);
    const uint32_t own = a.id_base + (uint32_t)i;
    const uint32_t out0 = FILL && row ? a.cnt_seg[i] : 0u;
    uint32_t seen = 0;   // the row's mutual entries before this pass
    for (uint32_t t0 = 0; t0 < a.kk; t0 += P) {   // (wave-uniform)
      const uint32_t jj = t0 + sub;
      bool edge = false, mutual = false;
      uint64_t v = 0;
      if (jj < mi) {
        v = a.rows[i * a.k + jj];
        const uint32_t d = (uint32_t)(v >> 32), j = (uint32_t)v - a.id_base;
        if ((uint64_t)j >= a.n || (uint64_t)j == i) {
          bad = true;
        } else if (d <= a.max_dist) {
          edge = true;
          mutual = adj_listed_back(a, j, d, own);
        }
      }
      const uint64_t m = __ballot(mutual);
      if (FILL && mutual) a.adj[(uint64_t)out0 + seen + (uint32_t)__popcll(m & below)] = v;
      seen += (uint32_t)__popcll(m & gmask);
      if (!FILL) edges += (uint32_t)__popcll(__ballot(edge));
    }
    if (!FILL && row && sub == 0) a.cnt_seg[i] = seen;
  }
  if (!FILL) {
    if (bad) a.stat32[1] = 1u;
    if (lane == 0 && edges) atomicAdd(a.stat, (unsigned long long)edges);
  }
}

// the segment lengths' sum, largest and zeros (before the scan)
__global__ void __launch_bounds__(VC_ADJ_BLOCK) vc_adj_degree_kernel(const uint32_t* __restrict__ cnt, uint64_t n, unsigned long long* __restrict__ stat,
                                                                     uint32_t* __restrict__ stat32) {
  uint32_t best = 0, empty = 0;
  unsigned long long sum = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * VC_ADJ_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * VC_ADJ_BLOCK) {
    const uint32_t c = cnt[i];
    best = max(best, c);
    empty += c == 0u;
    sum += c;
  }
  for (int o = VC_WAVE / 2; o; o >>= 1) {
    best = max(best, (uint32_t)__shfl_xor((int)best, o, VC_WAVE));
    empty += (uint32_t)__shfl_xor((int)empty, o, VC_WAVE);
    sum += ((unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)(sum >> 32), o, VC_WAVE) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)sum, o, VC_WAVE);
  }
  if (vc_lane() == 0) {
    if (sum) atomicAdd(stat + 1, sum);
    if (empty) atomicAdd(stat + 2, (unsigned long long)empty);
    if (best) atomicMax(stat32, best);
  }
}

__global__ void __launch_bounds__(VC_ADJ_BLOCK) vc_adj_offsets_kernel(const uint32_t* __restrict__ scanned, uint64_t words, uint64_t* __restrict__ offsets) {
  for (uint64_t i = (uint64_t)blockIdx.x * VC_ADJ_BLOCK + threadIdx.x; i < words; i += (uint64_t)gridDim.x * VC_ADJ_BLOCK) offsets[i] = scanned[i];
}

// the first position of `list` [0, len) whose word is not below x
__device__ __forceinline__ uint32_t adj_rank(const uint64_t* __restrict__ list, uint32_t len, uint64_t x) {
  uint32_t lo = 0, hi = len;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) / 2;
    if (list[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// record j's segment: its row's listed entries A (a prefix of the row, since the row ascends: as many as the segment holds beyond the
// in-part) merged with its run B of the sorted in-part.  A word's place is its index plus its rank in the other list; no word is in
// both, so the places are a permutation of [0, |A| + |B|).  Thread t of `team` takes every team-th word.
__device__ __forceinline__ void adj_merge(const AdjArgs& a, uint64_t j, uint32_t t, uint32_t team) {
  const uint32_t in0 = a.cnt_in[j], nb = a.cnt_in[j + 1] - in0, out0 = a.cnt_seg[j], na = a.cnt_seg[j + 1] - out0 - nb;
  const uint64_t* __restrict__ A = a.rows + j * a.k;
  const uint64_t* __restrict__ B = a.sorted + in0;
  uint64_t* __restrict__ out = a.adj + out0;
  for (uint32_t x = t; x < na; x += team) {
    const uint64_t w = A[x];
    out[x + adj_rank(B, nb, w)] = w;
  }
  for (uint32_t x = t; x < nb; x += team) {
    const uint64_t w = B[x];
    out[x + adj_rank(A, na, w)] = w;
  }
}
// four records per block, a wave each; then the block takes those of the four whose segment is above the plan's boundary
__global__ void __launch_bounds__(VC_ADJ_BLOCK) vc_adj_merge_kernel(const AdjArgs a) {
  constexpr uint32_t WAVES = VC_ADJ_BLOCK / VC_ADJ_WAVE;
  const uint32_t lane = vc_lane(), wave = threadIdx.x / VC_ADJ_WAVE;
  for (uint64_t r0 = (uint64_t)blockIdx.x * WAVES; r0 < a.n; r0 += (uint64_t)gridDim.x * WAVES) {
    const uint64_t j = r0 + wave;
    if (j < a.n && !vc_adj_block_team(a.cnt_seg[j + 1] - a.cnt_seg[j])) adj_merge(a, j, lane, VC_ADJ_WAVE);
    for (uint32_t w = 0; w < WAVES; ++w) {
      const uint64_t jw = r0 + w;
      if (jw < a.n && vc_adj_block_team(a.cnt_seg[jw + 1] - a.cnt_seg[jw])) adj_merge(a, jw, threadIdx.x, VC_ADJ_BLOCK);
    }
  }
}

uint32_t adj_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + VC_ADJ_BLOCK - 1) / VC_ADJ_BLOCK, 1), 256 * 8); }

}  // namespace

#define ADJ_HIP(call) VC_HIP_OR_FAIL("k-NN adjacency", call)

int vc_knn_adjacency_run(const VcStoreView& v, const VcAdjArgs& a, vc_knn_adjacency_stats* stats, hipStream_t s, std::string* err) {
  if (stats) *stats = vc_knn_adjacency_stats{};
  if (v.n == 0) {
    ADJ_HIP(hipMemsetAsync(a.d_offsets, 0, 8, s));
    return VC_OK;
  }
  const uint64_t n = v.n, items = n * a.kk;
  const bool either = a.flags == VC_KNN_EITHER, mutual = a.flags == VC_KNN_MUTUAL, with_items = vc_adj_key_bytes(n, a.kk, a.flags, a.adj_cap) != 0;
  // every buffer of the call, before the first launch
  const size_t counter_words = (size_t)vc_adj_counter_words(n, a.flags), scan_words = vc_scan_work_words(n + 1);
  uint64_t* d_stat = (uint64_t*)v.alloc(VC_ADJ_STAT, VC_ADJ_STAT_BYTES);
  uint32_t* d_cnt = (uint32_t*)v.alloc(VC_ADJ_COUNT, (counter_words + scan_words) * 4);
  if (!d_stat || !d_cnt) return VC_ERR_NOMEM;
  uint32_t *d_keys = nullptr, *d_sort_work = nullptr;
  uint64_t* d_vals = nullptr;
  if (with_items) {
    d_keys = (uint32_t*)v.alloc(VC_ADJ_KEYS, (size_t)vc_adj_key_bytes(n, a.kk, a.flags, a.adj_cap));
    d_vals = (uint64_t*)v.alloc(VC_ADJ_VALS, (size_t)vc_adj_val_bytes(n, a.kk, a.flags, a.adj_cap));
    d_sort_work = (uint32_t*)v.alloc(VC_ADJ_SORT, vc_radix_sort_work_words(items) * 4);
    if (!d_keys || !d_vals || !d_sort_work) return VC_ERR_NOMEM;
  }
  uint32_t* d_scan_work = d_cnt + counter_words;
  ADJ_HIP(hipMemsetAsync(d_stat, 0, VC_ADJ_STAT_BYTES, s));
  ADJ_HIP(hipMemsetAsync(d_cnt, 0, counter_words * 4, s));
  AdjArgs k{};
  k.rows = a.d_rows; k.counts = a.d_counts; k.n = n; k.k = a.k; k.kk = a.kk; k.max_dist = a.max_dist; k.id_base = v.id_base;
  k.uniform = vc_kgraph_row_count(n, a.k);
  k.cnt_in = d_cnt; k.cnt_seg = either ? d_cnt + (n + 1) : d_cnt;
  k.keys = d_keys; k.vals = d_vals; k.adj = a.d_adj;
  k.stat = (unsigned long long*)d_stat; k.stat32 = (uint32_t*)(d_stat + 3);
  const uint32_t P = vc_adj_row_lanes(a.kk), mutual_grid = adj_grid((n + VC_ADJ_WAVE / P - 1) / (VC_ADJ_WAVE / P) * VC_ADJ_WAVE);
  // 1. the items and the counters
  if (mutual) hipLaunchKernelGGL(vc_adj_mutual_kernel<false>, dim3(mutual_grid), dim3(VC_ADJ_BLOCK), 0, s, k, P);
  else if (either) hipLaunchKernelGGL(vc_adj_enumerate_kernel<true>, dim3(adj_grid(items)), dim3(VC_ADJ_BLOCK), 0, s, k);
  else hipLaunchKernelGGL(vc_adj_enumerate_kernel<false>, dim3(adj_grid(items)), dim3(VC_ADJ_BLOCK), 0, s, k);
  ADJ_HIP(hipGetLastError());
  // 2. the statistics, the scans, THE WAIT: 32 bytes
  hipLaunchKernelGGL(vc_adj_degree_kernel, dim3(adj_grid(n)), dim3(VC_ADJ_BLOCK), 0, s, (const uint32_t*)k.cnt_seg, n, k.stat, k.stat32);
  ADJ_HIP(hipGetLastError());
  ADJ_HIP(vc_exclusive_scan_u32(k.cnt_seg, k.cnt_seg, n + 1, d_scan_work, s));
  if (either) ADJ_HIP(vc_exclusive_scan_u32(k.cnt_in, k.cnt_in, n + 1, d_scan_work, s));
  struct { uint64_t n_edges, n_entries, n_empty; uint32_t max_degree, bad; } home{};
  static_assert(sizeof(home) == VC_ADJ_STAT_BYTES, "the statistics block as it lies");
  ADJ_HIP(hipMemcpyAsync(&home, d_stat, VC_ADJ_STAT_BYTES, hipMemcpyDeviceToHost, s));
  ADJ_HIP(hipStreamSynchronize(s));
  if (home.bad) {
    if (err) *err = "k-NN adjacency: a count above k, an id outside the store or a row's own id -- not a graph vc_knn_graph built for this store";
    return VC_ERR_INVALID;
  }
  if (stats) *stats = vc_knn_adjacency_stats{home.n_edges, home.n_entries, home.n_empty, home.max_degree, 0u};
  // 4. the offsets
  hipLaunchKernelGGL(vc_adj_offsets_kernel, dim3(adj_grid(n + 1)), dim3(VC_ADJ_BLOCK), 0, s, (const uint32_t*)k.cnt_seg, n + 1, a.d_offsets);
  ADJ_HIP(hipGetLastError());
  const uint64_t T = home.n_entries;
  if (T > a.adj_cap) {
    if (err) *err = "k-NN adjacency: the segments hold " + std::to_string(T) + " words, adj_cap is " + std::to_string(a.adj_cap);
    return VC_ERR_CAPACITY;
  }
  if (T == 0) return VC_OK;
  if (mutual) {   // 5. the row-local fill
    hipLaunchKernelGGL(vc_adj_mutual_kernel<true>, dim3(mutual_grid), dim3(VC_ADJ_BLOCK), 0, s, k, P);
    ADJ_HIP(hipGetLastError());
    return VC_OK;
  }
  // 3. the sort: by the distance, then by the target
  const uint32_t dist_bits = vc_adj_dist_bits(a.max_dist, 64 * v.W), key_bits = vc_adj_key_bits(n);
  uint32_t* keys[2] = {d_keys, d_keys + items};
  uint64_t* vals[2] = {d_vals, d_vals + items};
  ADJ_HIP(vc_radix_sort_items(keys, vals, items, dist_bits, key_bits, d_sort_work, s));
  k.sorted = vals[vc_radix_sort_item_passes(dist_bits, key_bits) & 1];
  // 5. the fill
  if (either) {
    hipLaunchKernelGGL(vc_adj_merge_kernel, dim3(adj_grid(n * VC_ADJ_WAVE)), dim3(VC_ADJ_BLOCK), 0, s, k);
    ADJ_HIP(hipGetLastError());
  } else {
    ADJ_HIP(hipMemcpyAsync(a.d_adj, k.sorted, T * 8, hipMemcpyDeviceToDevice, s));
  }
  return VC_OK;
}

int vc_knn_adjacency_run_host(const VcStoreView& v, VcAdjArgs a, const uint64_t* rows, const uint32_t* counts, uint64_t* adj, uint64_t* offsets,
                              vc_knn_adjacency_stats* stats, hipStream_t s, std::string* err) {
  if (v.n == 0) {
    if (stats) *stats = vc_knn_adjacency_stats{};
    offsets[0] = 0;
    return VC_OK;
  }
  const size_t n = (size_t)v.n;
  const VcAdjStage L(n, a.k, a.kk, a.flags, a.adj_cap, counts != nullptr);
  uint8_t* stage = (uint8_t*)v.alloc(VC_ADJ_STAGE, (size_t)L.total);
  if (!stage) return VC_ERR_NOMEM;
  uint64_t* d_rows = (uint64_t*)(stage + L.rows);
  uint32_t* d_cnt = (uint32_t*)(stage + L.counts);
  ADJ_HIP(hipMemcpyAsync(d_rows, rows, n * a.k * 8, hipMemcpyHostToDevice, s));
  if (counts) ADJ_HIP(hipMemcpyAsync(d_cnt, counts, n * 4, hipMemcpyHostToDevice, s));
  a.d_rows = d_rows; a.d_counts = counts ? d_cnt : nullptr;
  a.d_offsets = (uint64_t*)(stage + L.offsets);
  a.d_adj = L.cap ? (uint64_t*)(stage + L.adj) : nullptr;
  a.adj_cap = L.cap;
  vc_knn_adjacency_stats st{};
  const int rc = vc_knn_adjacency_run(v, a, &st, s, err);
  if (rc != VC_OK && rc != VC_ERR_CAPACITY) return rc;
  if (stats) *stats = st;
  ADJ_HIP(hipMemcpyAsync(offsets, a.d_offsets, (n + 1) * 8, hipMemcpyDeviceToHost, s));
  if (rc == VC_OK && st.n_entries) ADJ_HIP(hipMemcpyAsync(adj, a.d_adj, (size_t)st.n_entries * 8, hipMemcpyDeviceToHost, s));
  ADJ_HIP(hipStreamSynchronize(s));
  return rc;
}
