// ============================================================================
// vc_knn_graph.hip -- the exact k-NN graph of the store (vc_knn_graph*, vc_sharded_knn_graph*) and its components and in-degrees
// (vc_cluster_knn*, vc_sharded_cluster_knn*); the header states both contracts.  One driver each for both handle kinds over a
// VcStoreView; the plan arithmetic is vc_knn_graph_plan.hpp.
//   vc_kgraph_settle_kernel   one thread per output entry: the own record dropped by value, the verdict on the row, a settled row and
//                             its count written through the index map, flag[row] = 1 for a query that goes to the next round; with
//                             an id list in place of the range (vc_knn_graph_retain.hip) the own id and the row's place come from it
//   vc_kgraph_gather_kernel   the retry list of a round: the exclusive scan of the flags (vc_sort.hip) places the flagged rows, so the
//                             list is ascending and nothing depends on block order
//   vc_kgraph_init_kernel     vc_cluster_knn: labels[i] = id_base + i, in_degree[i] = 0
//   vc_kgraph_edge_kernel     one thread per (record, entry < kk): the in-degree atomic, the one-compare mutual test, the union
//   vc_kgraph_degree_kernel   the largest in-degree
// None of them uses LDS or scratch memory.  The searches in between are the handle's unchanged k-NN.
// ============================================================================
#include <algorithm>
#include <vector>

#include "vc_forest.hpp"
#include "vc_internal.hpp"
#include "vc_knn_graph_plan.hpp"

static_assert(VC_KGRAPH_MAX_K == VC_MAX_K, "the plan's widest row is the search's");
static_assert(VC_KGRAPH_BATCH_DEFAULT == VC_CLUSTER_BATCH, "batch = 0 means what it means to the walk calls");
static_assert(sizeof(vc_knn_graph_stats) == 32 && sizeof(vc_cluster_knn_stats) == VC_KGRAPH_STAT_BYTES, "the header's sizes");

namespace {

#define KG_BLK 256u

// what a settle launch works on; rows, cnt, flag and map are those of the sub-batch, out and counts those of the batch
struct SettleArgs {
  const uint64_t* rows;      // [n][kp]
  const uint32_t* cnt;       // [n]
  uint32_t n, kp, k;
  uint32_t tie_cut;          // exact MIH underneath: a full row is sure only below its last distance (vc_kgraph_verdict)
  const uint32_t* map;       // [n] compact row -> the batch's query; null: first + row
  uint32_t first;
  uint32_t first_id;         // the global id of the batch's query 0: query oq is record first_id + oq
  const uint32_t* ids;       // [nb] nullable: the batch comes from an id list; query oq is record ids[oq], and its row and count go
  uint32_t id_base;          //   to place ids[oq] - id_base of out and counts, which are then those of the whole store
  uint64_t* out;             // [nb][k]
  uint32_t* counts;          // [nb], nullable
  uint32_t* flag;            // [n]
  unsigned long long* tally; // += rows passed on
};

// the first entry of row[0 .. m) that is >= x
__device__ __forceinline__ uint32_t kg_lower_bound(const uint64_t* __restrict__ row, uint32_t m, uint64_t x) {
  uint32_t lo = 0, hi = m;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (row[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Thread e serves entry e % k of row e / k.  Every thread of a row reaches the same verdict from the same words (two binary
// searches in a row the cache holds); entry 0's thread writes the row's flag, count and tally.
__global__ void __launch_bounds__(KG_BLK) vc_kgraph_settle_kernel(const SettleArgs a) {
  const uint64_t total = (uint64_t)a.n * a.k;
  for (uint64_t e = (uint64_t)blockIdx.x * KG_BLK + threadIdx.x; e < total; e += (uint64_t)gridDim.x * KG_BLK) {
    const uint32_t r = (uint32_t)(e / a.k), j = (uint32_t)(e % a.k);
    const uint64_t* row = a.rows + (uint64_t)r * a.kp;
    const uint32_t c = a.cnt[r], m = vc_kgraph_row_entries(c, a.kp);
    const uint32_t oq = a.map ? a.map[r] : a.first + r;
    const uint32_t own = a.ids ? a.ids[oq] : a.first_id + oq;
    const uint64_t self = (uint64_t)own, to = a.ids ? (uint64_t)(own - a.id_base) : (uint64_t)oq;
    const uint32_t lo = kg_lower_bound(row, m, self);
    const bool present = lo < m && row[lo] == self;
    uint32_t below = 0;
    if (a.tie_cut && c == a.kp) below = kg_lower_bound(row, m, row[a.kp - 1] & 0xFFFFFFFF00000000ull);   // entries nearer than the last
    const int verdict = vc_kgraph_verdict(a.tie_cut != 0, c, a.kp, a.k, present, below);
    if (verdict == VC_KGRAPH_RETRY) {
      if (j == 0) a.flag[r] = 1u;
      continue;
    }
    const uint32_t left = vc_kgraph_count(m, present, a.k);
    a.out[to * a.k + j] = j < left ? row[j + (present && j >= lo ? 1u : 0u)] : VC_PACK_INF;   // (j < left: the index stays below m)
    if (j == 0) {
      a.flag[r] = 0u;
      if (a.counts) a.counts[to] = verdict == VC_KGRAPH_PASSED ? 0xFFFFFFFFu : left;
      if (verdict == VC_KGRAPH_PASSED) atomicAdd(a.tally, 1ull);
    }
  }
}

// row r with flag[r] goes to place scanned[r]: its query's place in the batch to map_next, its code out of the batch's codes to
// q_next.  The last thread leaves the length of the list in *n_next.
__global__ void __launch_bounds__(KG_BLK) vc_kgraph_gather_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ scanned, uint32_t n,
                                                                  const uint32_t* __restrict__ map, const uint64_t* __restrict__ queries, uint32_t W,
                                                                  uint32_t* __restrict__ map_next, uint64_t* __restrict__ q_next, uint32_t* __restrict__ n_next) {
  const uint32_t r = blockIdx.x * KG_BLK + threadIdx.x;
  if (r >= n) return;
  const uint32_t f = flag[r], at = scanned[r];
  if (r == n - 1) *n_next = at + f;
  if (!f) return;
  const uint32_t oq = map ? map[r] : r;
  map_next[at] = oq;
  for (uint32_t w = 0; w < W; ++w) q_next[(uint64_t)at * W + w] = queries[(uint64_t)oq * W + w];
}

uint32_t kg_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + KG_BLK - 1) / KG_BLK, 1), 256 * 8); }

hipError_t launch_settle(const SettleArgs& a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  if (a.kp == 0 || a.kp > VC_MAX_K || a.k == 0 || a.k >= a.kp) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vc_kgraph_settle_kernel, dim3(kg_grid((uint64_t)a.n * a.k)), dim3(KG_BLK), 0, s, a);
  return hipGetLastError();
}

#define KG_HIP(call) VC_HIP_OR_FAIL("k-NN graph", call)

}  // namespace

// THE ROUNDS of a batch (the header states the rule).  Per round: the search and the settle launch, sub-batch by sub-batch; under
// exact MIH then the scan of the flags, the gather and the one wait, for the length of the retry list.  The list left after the round
// at VC_MAX_K goes through linear_knn at k + 1, whose rows the same kernel settles without the tie cut.
int vc_knn_graph_run(const VcStoreView& v, const VcKnnSearch& linear_knn, const VcKgraphArgs& a, vc_knn_graph_stats* stats, hipStream_t s, std::string* err) {
  if (stats) *stats = vc_knn_graph_stats{};
  const uint32_t batch = vc_kgraph_batch(a.batch), nq_max = (uint32_t)std::min<uint64_t>(batch, a.rows), k = a.k;
  const VcKgraphWork wp(nq_max, v.W, vc_scan_work_words(nq_max));
  uint8_t* work = (uint8_t*)v.alloc(VC_KGRAPH_WORK, wp.total);
  if (!work) return VC_ERR_NOMEM;
  unsigned long long* tally = (unsigned long long*)(work + wp.tally);
  uint32_t* n_next = (uint32_t*)(work + wp.n_next);
  uint32_t* flag = (uint32_t*)(work + wp.flag);
  uint32_t* scanned = (uint32_t*)(work + wp.scanned);
  uint32_t* scan_work = (uint32_t*)(work + wp.scan_work);
  uint32_t* maps[2] = {(uint32_t*)(work + wp.map[0]), (uint32_t*)(work + wp.map[1])};
  uint32_t* cnt = (uint32_t*)(work + wp.cnt);
  uint32_t* d_ids = (uint32_t*)(work + wp.ids);
  uint32_t* d_found = (uint32_t*)(work + wp.found);
  uint64_t* d_q = (uint64_t*)(work + wp.q);
  uint64_t* q_next = (uint64_t*)(work + wp.q_next);
  KG_HIP(hipMemsetAsync(work, 0, 16, s));   // the tally and the length

  vc_knn_graph_stats st{};
  int rc;
  for (uint64_t pos = 0; pos < a.rows; pos += batch) {
    const uint32_t nb = (uint32_t)std::min<uint64_t>(batch, a.rows - pos), first_id = v.id_base + (uint32_t)(a.first + pos);
    if (a.d_id_list) KG_HIP(hipMemcpyAsync(d_ids, a.d_id_list + pos, (size_t)nb * 4, hipMemcpyDeviceToDevice, s));
    else KG_HIP(vc_launch_cluster_init(d_ids, nb, first_id, s));
    if ((rc = v.gather(d_ids, nb, d_q, d_found))) return rc;
    // a range writes the batch's rows in order; an id list writes every row to its record's own place (the settle kernel)
    uint64_t* out = a.d_id_list ? a.d_rows : a.d_rows + pos * k;
    uint32_t* counts = !a.d_counts ? nullptr : a.d_id_list ? a.d_counts : a.d_counts + pos;
    // one round over the list (q, map, n) at kp through `search`
    auto round = [&](const VcKnnSearch& search, const uint64_t* q, const uint32_t* map, uint32_t n, uint32_t kp, bool tie_cut) -> int {
      const uint32_t sub = vc_kgraph_sub_batch(a.budget, kp);
      uint64_t* rows = (uint64_t*)v.alloc(VC_KGRAPH_ROWS, vc_kgraph_rows_bytes(n, a.budget, kp));
      if (!rows) return VC_ERR_NOMEM;
      for (uint32_t first = 0; first < n; first += sub) {
        const uint32_t ns = std::min(sub, n - first);
        const int r = search(q + (uint64_t)first * v.W, ns, kp, rows, cnt, nullptr);
        if (r) return r;
        SettleArgs c{};
        c.rows = rows; c.cnt = cnt; c.n = ns; c.kp = kp; c.k = k; c.tie_cut = tie_cut ? 1u : 0u;
        c.map = map ? map + first : nullptr; c.first = first; c.first_id = first_id;
        c.ids = a.d_id_list ? d_ids : nullptr; c.id_base = v.id_base;
        c.out = out; c.counts = counts; c.flag = flag + first; c.tally = tally;
        KG_HIP(launch_settle(c, s));
      }
      return VC_OK;
    };
    const uint64_t* q = d_q;   // round 0: the batch, identity map
    const uint32_t* map = nullptr;
    uint32_t n = nb, kp = vc_kgraph_first_k(k, a.k_first, a.linear);
    for (uint32_t r = 0;; ++r) {
      if ((rc = round(v.knn, q, map, n, kp, !a.linear))) return rc;
      st.n_searched += n;
      st.k_last = std::max(st.k_last, kp);
      st.n_rounds_max = std::max(st.n_rounds_max, r + 1);
      if (a.linear) break;   // every verdict of the linear scan is final
      KG_HIP(vc_exclusive_scan_u32(flag, scanned, n, scan_work, s));
      hipLaunchKernelGGL(vc_kgraph_gather_kernel, dim3((n + KG_BLK - 1) / KG_BLK), dim3(KG_BLK), 0, s, (const uint32_t*)flag, (const uint32_t*)scanned, n, map,
                         (const uint64_t*)d_q, v.W, maps[r & 1], q_next, n_next);
      KG_HIP(hipGetLastError());
      // THE WAIT of the round: 4 bytes
      uint32_t left = 0;
      KG_HIP(hipMemcpyAsync(&left, n_next, 4, hipMemcpyDeviceToHost, s));
      KG_HIP(hipStreamSynchronize(s));
      if (left > n) {
        if (err) *err = "k-NN graph: the retry list is longer than the round";
        return VC_ERR_HIP;
      }
      if (left == 0) break;
      // the gather read the batch's codes through the old map and wrote q_next and the other map: the next round reads those
      q = q_next;
      map = maps[r & 1];
      n = left;
      if (kp >= VC_MAX_K) {   // no wider row exists: the linear scan's order settles the ties
        if ((rc = round(linear_knn, q, map, n, k + 1, false))) return rc;
        st.n_linear += n;
        st.n_rounds_max = std::max(st.n_rounds_max, r + 2);
        break;
      }
      kp = vc_kgraph_next_k(kp);
    }
  }
  if (stats) {
    unsigned long long gave_up = 0;
    KG_HIP(hipMemcpyAsync(&gave_up, tally, 8, hipMemcpyDeviceToHost, s));
    KG_HIP(hipStreamSynchronize(s));
    st.n_gave_up = gave_up;
    *stats = st;
  }
  return VC_OK;
}

// A ring overflowed and the device-side recovery gave up: the records of the range whose count is UINT32_MAX are answered again by
// the handle's host-form LINEAR k-NN, whose host-driven recovery always ends, on their gathered codes, and stripped by the strip
// kernel's rule.  rows [a.rows][k] and cnt [a.rows] are the range's outputs in host memory.
int vc_knn_graph_answer_again_host(const VcStoreView& v, const VcKgraphArgs& a, uint64_t* rows, uint32_t* cnt,
                                   const std::function<int(const uint64_t* codes, uint32_t nq, uint64_t* rows, uint32_t* counts)>& host_knn, hipStream_t s,
                                   std::string* err) {
  const size_t n = (size_t)a.rows, k = a.k;
  int rc;
  std::vector<uint32_t> ids, where;
  for (size_t i = 0; i < n; ++i)
    if (cnt[i] == 0xFFFFFFFFu) {
      where.push_back((uint32_t)i);
      ids.push_back(v.id_base + (uint32_t)(a.first + i));
    }
  const uint32_t nf = (uint32_t)ids.size(), kp = a.k + 1;
  if (nf) {
    const VcKgraphWork wp(nf, v.W, 0);
    uint8_t* work = (uint8_t*)v.alloc(VC_KGRAPH_WORK, wp.total);   // (the device form is over: its words are free)
    if (!work) return VC_ERR_NOMEM;
    uint32_t* d_ids = (uint32_t*)(work + wp.ids);
    uint32_t* d_found = (uint32_t*)(work + wp.found);
    uint64_t* d_q = (uint64_t*)(work + wp.q);
    std::vector<uint64_t> codes((size_t)nf * v.W), hrows((size_t)nf * kp), hout((size_t)nf * k);
    std::vector<uint32_t> found(nf, 1u), rcnt(nf), hcnt(nf);
    KG_HIP(hipMemcpyAsync(d_ids, ids.data(), (size_t)nf * 4, hipMemcpyHostToDevice, s));
    if ((rc = v.gather(d_ids, nf, d_q, d_found))) return rc;
    KG_HIP(hipMemcpyAsync(codes.data(), d_q, codes.size() * 8, hipMemcpyDeviceToHost, s));
    KG_HIP(hipStreamSynchronize(s));
    if ((rc = host_knn(codes.data(), nf, hrows.data(), rcnt.data()))) return rc;
    vc_ids_strip_host(ids.data(), found.data(), hrows.data(), rcnt.data(), nf, kp, a.k, hout.data(), hcnt.data(), nullptr);
    for (uint32_t f = 0; f < nf; ++f) {
      std::copy(hout.begin() + (size_t)f * k, hout.begin() + (size_t)(f + 1) * k, rows + (size_t)where[f] * k);
      cnt[where[f]] = hcnt[f];
    }
  }
  return VC_OK;
}

int vc_knn_graph_run_host(const VcStoreView& v, const VcKgraphArgs& a, uint64_t* rows, uint32_t* counts, vc_knn_graph_stats* stats,
                          const std::function<int(uint64_t* d_rows, uint32_t* d_counts, vc_knn_graph_stats* stats)>& run,
                          const std::function<int(const uint64_t* codes, uint32_t nq, uint64_t* rows, uint32_t* counts)>& host_knn, hipStream_t s,
                          std::string* err) {
  const size_t n = (size_t)a.rows, k = a.k, rbytes = n * k * 8, cbytes = n * 4;   // staged: rows | counts
  uint8_t* stage = (uint8_t*)v.alloc(VC_KGRAPH_STAGE, rbytes + cbytes);
  if (!stage) return VC_ERR_NOMEM;
  uint64_t* d_rows = (uint64_t*)stage;
  uint32_t* d_cnt = (uint32_t*)(stage + rbytes);
  vc_knn_graph_stats st{};
  int rc = run(d_rows, d_cnt, &st);
  if (rc) return rc;
  std::vector<uint32_t> own_cnt;
  uint32_t* cnt = counts;
  if (!cnt && st.n_gave_up) {
    own_cnt.resize(n);
    cnt = own_cnt.data();
  }
  KG_HIP(hipMemcpyAsync(rows, d_rows, rbytes, hipMemcpyDeviceToHost, s));
  if (cnt) KG_HIP(hipMemcpyAsync(cnt, d_cnt, cbytes, hipMemcpyDeviceToHost, s));
  KG_HIP(hipStreamSynchronize(s));
  if (st.n_gave_up && (rc = vc_knn_graph_answer_again_host(v, a, rows, cnt, host_knn, s, err))) return rc;
  if (stats) *stats = st;
  return VC_OK;
}

// ---- vc_cluster_knn*: components and in-degrees of a built graph -------------------------------------------------------------------------
namespace {

// what the three launches work on
struct EdgeArgs {
  const uint64_t* rows;      // [n][k]
  const uint32_t* counts;    // [n], nullable: every row holds `uniform` entries
  uint64_t n;
  uint32_t k, kk, either, max_dist, id_base, uniform;
  uint32_t* labels;          // [n]: the forest of vc_forest.hpp
  uint32_t* in_degree;       // [n]
  unsigned long long* stat;  // [0] += edges, [1] += mutual pairs, [2] clusters (the flatten pass)
  uint32_t* stat32;          // = (uint32_t*)(stat + 3): [0] the largest in-degree, [1] the error word
};

__global__ void __launch_bounds__(KG_BLK) vc_kgraph_init_kernel(uint32_t* __restrict__ labels, uint32_t* __restrict__ in_degree, uint64_t n, uint32_t id_base) {
  for (uint64_t i = (uint64_t)blockIdx.x * KG_BLK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * KG_BLK) {
    labels[i] = id_base + (uint32_t)i;
    in_degree[i] = 0u;
  }
}

__device__ __forceinline__ uint32_t kg_count(const EdgeArgs& a, uint64_t i) { return a.counts ? a.counts[i] : a.uniform; }

// Thread e serves entry e % kk of record e / kk.  The entry (d, id j) of row i is an edge when it is among the row's first
// min(kk, count_i) and d <= max_dist; then j's in-degree goes up, and j lists i in turn iff (d << 32 | id of i) is no greater than
// the last of row j's first min(kk, count_j) entries (vc_kgraph_lists; the cap holds for both since the distance is the same).  A
// mutual pair is counted from its smaller member.  A count above k, or an id outside the store, raises the error word and is passed
// over: nothing is read or written out of bounds.  The sums are one add per wave.
__global__ void __launch_bounds__(KG_BLK) vc_kgraph_edge_kernel(const EdgeArgs a) {
  const uint64_t total = a.n * a.kk;
  uint32_t edges = 0, mutuals = 0;   // wave-uniform
  for (uint64_t e0 = (uint64_t)blockIdx.x * KG_BLK; e0 < total; e0 += (uint64_t)gridDim.x * KG_BLK) {   // (block-uniform bounds: every lane votes)
    const uint64_t e = e0 + threadIdx.x;
    bool edge = false, mutual = false, bad = false;
    uint32_t own = 0, other = 0;
    if (e < total) {
      const uint64_t i = e / a.kk;
      const uint32_t jj = (uint32_t)(e % a.kk), ci = kg_count(a, i);
      bad = ci > a.k;
      if (!bad && jj < vc_kgraph_edge_entries(a.kk, ci)) {
        const uint64_t v = a.rows[i * a.k + jj];
        const uint32_t d = (uint32_t)(v >> 32), j = (uint32_t)v - a.id_base;
        if ((uint64_t)j >= a.n || (uint64_t)j == i) {
          bad = true;
        } else if (d <= a.max_dist) {
          const uint32_t cj = kg_count(a, j), mj = vc_kgraph_edge_entries(a.kk, cj);
          edge = true;
          own = a.id_base + (uint32_t)i;
          other = (uint32_t)v;
          if (cj <= a.k && mj) mutual = vc_kgraph_lists(a.rows[(uint64_t)j * a.k + mj - 1], d, own);
        }
      }
    }
    if (bad) a.stat32[1] = 1u;
    if (edge) atomicAdd(a.in_degree + (other - a.id_base), 1u);
    edges += (uint32_t)__popcll(__ballot(edge));
    mutuals += (uint32_t)__popcll(__ballot(mutual && own < other));
    if (edge && (a.either || mutual)) cl_unite(a.labels, a.id_base, own, other);
  }
  if (vc_lane() == 0) {
    if (edges) atomicAdd(a.stat, (unsigned long long)edges);
    if (mutuals) atomicAdd(a.stat + 1, (unsigned long long)mutuals);
  }
}

__global__ void __launch_bounds__(KG_BLK) vc_kgraph_degree_kernel(const uint32_t* __restrict__ in_degree, uint64_t n, uint32_t* __restrict__ max_out) {
  uint32_t best = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * KG_BLK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * KG_BLK) best = max(best, in_degree[i]);
  for (int o = VC_WAVE / 2; o; o >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, o, VC_WAVE));
  if (vc_lane() == 0 && best) atomicMax(max_out, best);
}

}  // namespace

#define KGC_HIP(call) VC_HIP_OR_FAIL("k-NN clusters", call)

int vc_cluster_knn_run(const VcStoreView& v, const VcKgraphClusterArgs& a, vc_cluster_knn_stats* stats, hipStream_t s, std::string* err) {
  uint64_t* d_stat = (uint64_t*)v.alloc(VC_KGRAPH_STAT, VC_KGRAPH_STAT_BYTES);
  uint32_t* d_deg = a.d_in_degree ? a.d_in_degree : (uint32_t*)v.alloc(VC_KGRAPH_DEG, (size_t)v.n * 4);
  if (!d_stat || !d_deg) return VC_ERR_NOMEM;
  KGC_HIP(hipMemsetAsync(d_stat, 0, VC_KGRAPH_STAT_BYTES, s));
  EdgeArgs ea{};
  ea.rows = a.d_rows; ea.counts = a.d_counts; ea.n = v.n; ea.k = a.k; ea.kk = a.kk; ea.either = (a.flags & VC_KNN_EITHER) ? 1u : 0u;
  ea.max_dist = a.max_dist; ea.id_base = v.id_base; ea.uniform = vc_kgraph_row_count(v.n, a.k);
  ea.labels = a.d_labels; ea.in_degree = d_deg; ea.stat = (unsigned long long*)d_stat; ea.stat32 = (uint32_t*)(d_stat + 3);
  hipLaunchKernelGGL(vc_kgraph_init_kernel, dim3(kg_grid(v.n)), dim3(KG_BLK), 0, s, a.d_labels, d_deg, v.n, v.id_base);
  KGC_HIP(hipGetLastError());
  hipLaunchKernelGGL(vc_kgraph_edge_kernel, dim3(kg_grid(v.n * a.kk)), dim3(KG_BLK), 0, s, ea);
  KGC_HIP(hipGetLastError());
  KGC_HIP(vc_launch_cluster_flatten(a.d_labels, v.n, v.id_base, d_stat + 2, s));
  hipLaunchKernelGGL(vc_kgraph_degree_kernel, dim3(kg_grid(v.n)), dim3(KG_BLK), 0, s, (const uint32_t*)d_deg, v.n, ea.stat32);
  KGC_HIP(hipGetLastError());
  // THE WAIT: the statistics and the error word, 32 bytes
  struct { uint64_t n_edges, n_mutual, n_clusters; uint32_t max_in_degree, bad; } home{};
  static_assert(sizeof(home) == VC_KGRAPH_STAT_BYTES, "the statistics block as it lies");
  KGC_HIP(hipMemcpyAsync(&home, d_stat, VC_KGRAPH_STAT_BYTES, hipMemcpyDeviceToHost, s));
  KGC_HIP(hipStreamSynchronize(s));
  if (home.bad) {
    if (err) *err = "k-NN clusters: a count above k or an id outside the store -- not a graph vc_knn_graph built for this store";
    return VC_ERR_INVALID;
  }
  if (stats) *stats = vc_cluster_knn_stats{home.n_edges, home.n_mutual, home.n_clusters, home.max_in_degree, 0u};
  return VC_OK;
}

int vc_cluster_knn_run_host(const VcStoreView& v, VcKgraphClusterArgs a, const uint64_t* rows, const uint32_t* counts, uint32_t* labels, uint32_t* in_degree,
                            vc_cluster_knn_stats* stats, hipStream_t s, std::string* err) {
  const size_t n = (size_t)v.n, rbytes = n * a.k * 8, wbytes = (n * 4 + 7) & ~(size_t)7;   // staged: rows | counts | labels | in-degrees
  uint8_t* stage = (uint8_t*)v.alloc(VC_KGRAPH_STAGE, rbytes + 3 * wbytes);
  if (!stage) return VC_ERR_NOMEM;
  uint64_t* d_rows = (uint64_t*)stage;
  uint32_t* d_cnt = (uint32_t*)(stage + rbytes);
  uint32_t* d_labels = (uint32_t*)(stage + rbytes + wbytes);
  uint32_t* d_deg = (uint32_t*)(stage + rbytes + 2 * wbytes);
  KGC_HIP(hipMemcpyAsync(d_rows, rows, rbytes, hipMemcpyHostToDevice, s));
  if (counts) KGC_HIP(hipMemcpyAsync(d_cnt, counts, n * 4, hipMemcpyHostToDevice, s));
  a.d_rows = d_rows; a.d_counts = counts ? d_cnt : nullptr; a.d_labels = d_labels; a.d_in_degree = d_deg;
  const int rc = vc_cluster_knn_run(v, a, stats, s, err);
  if (rc) return rc;
  KGC_HIP(hipMemcpyAsync(labels, d_labels, n * 4, hipMemcpyDeviceToHost, s));
  if (in_degree) KGC_HIP(hipMemcpyAsync(in_degree, d_deg, n * 4, hipMemcpyDeviceToHost, s));
  KGC_HIP(hipStreamSynchronize(s));
  return VC_OK;
}
