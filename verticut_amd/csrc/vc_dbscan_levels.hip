// ============================================================================
// vc_dbscan_levels.hip -- density clustering at every radius 0 .. R in ONE walk (vc_dbscan_levels*, vc_sharded_dbscan_levels*).
// vc_levels.hip's scheme (one forest per level, in place in the level-major label array, a pair united in ONE forest, then the
// cascade) with vc_dbscan.hip's state (a core's slot the forest, a non-core's slot its anchor); the forest is vc_forest.hpp's.
// ============================================================================
#include <algorithm>

#include "vc_forest.hpp"
#include "vc_internal.hpp"

// THE RULE: a record's raw segment at R ascends by distance and holds the record itself, so its entry at position min_pts - 1 is its
// CORE DISTANCE cd: the smallest radius at which min_pts records, itself included, lie within -- VC_CORE_NEVER if the segment is
// shorter.  Record i is a core at level r iff cd[i] <= r.  A pair {a, b} at distance d joins two cores at exactly the levels
// r >= w = max(d, cd[a], cd[b]); it is united in forest w ONLY, and after the last batch the CASCADE carries level r - 1 into level
// r: every core of level r - 1 is united in forest r with its root of forest r - 1, which is final by then.  By induction forest
// r - 1 connects the cores of level r - 1 as the pairs of w <= r - 1 do, so after its step forest r connects what those and the
// pairs of w == r connect; a record with cd == r enters forest r as a singleton and is joined by its pairs of w == r.
// STATE, in labels[] itself and without a sentinel.  The kind of slot (r, i) is decided by cd[i] alone, never by its content:
//   cd[i] <= r   the forest of level r: the global id of the parent, the own id at a root;
//   cd[i] >  r   record i's ANCHOR CANDIDATE OF EXACTLY LEVEL r: its own id = "none", else the smallest record v seen so far with
//                max(d(i, v), cd[v]) == r, that is, the smallest core neighbour that BECOMES one at level r; a CAS minimum.
// The anchor of a non-core record at level r is the minimum of its candidates of the levels t <= r (all of them anchor slots, as
// t <= r < cd[i]).  No union touches a non-core slot of its level: both ends of a pair have cd <= w, a cascade step joins a core of
// level r - 1 to a core of level r - 1, both cores of level r, and a core's chain passes through cores only.
// ONE WALK, as vc_dbscan.hip: the core kernel of a batch makes the core distances of its queries final, the edge kernel then acts
// on the entries (own, v < own) only -- every pair once, from its larger member, both core distances final.
//   vc_dbscan_levels_core_kernel     core distances of a batch's queries from its offsets and raw result
//   vc_dbscan_levels_edge_kernel     one thread per entry: its query by binary search, the union in forest w, the two anchor
//                                    candidates; the histogram of the distances
//   vc_dbscan_levels_cascade_kernel  one level: a core of the level below joins its root of the level below
//   vc_dbscan_levels_finish_kernel   one thread per record, level after level: root, root of the anchor or own id; counts the kinds
// All accesses to the forests and the anchors are relaxed device-scope atomics; no kernel waits for another block.
#define DL_BLK 256u

// cd[q] of the queries first .. first + nq - 1 (cd points at the first).  64-bit index arithmetic: min_pts may be 2^32 - 1.  An
// entry never lies beyond max_radius; a core distance that did would be no level of this call, so it is VC_CORE_NEVER too.
__global__ void __launch_bounds__(DL_BLK) vc_dbscan_levels_core_kernel(const uint64_t* __restrict__ raw, const uint64_t* __restrict__ roffs, uint32_t nq,
                                                                       uint32_t min_pts, uint32_t max_radius, uint32_t* __restrict__ cd) {
  for (uint32_t q = blockIdx.x * DL_BLK + threadIdx.x; q < nq; q += gridDim.x * DL_BLK) {
    const uint64_t lo = roffs[q], len = roffs[q + 1] - lo;
    uint32_t c = VC_CORE_NEVER;
    if (len >= (uint64_t)min_pts) {
      const uint32_t d = (uint32_t)(raw[lo + (uint64_t)min_pts - 1] >> 32);
      if (d <= max_radius) c = d;
    }
    cd[q] = c;
  }
}

// the slot of a non-core record takes `cand` while it still holds the own id `sparse`, else the smaller of the two (vc_dbscan.hip)
__device__ __forceinline__ void dl_lower(uint32_t* slot, uint32_t sparse, uint32_t cand) {
  uint32_t cur = cl_ld(slot);
  while (cur == sparse || cand < cur) {
    const uint32_t seen = atomicCAS(slot, cur, cand);
    if (seen == cur) break;
    cur = seen;
  }
}

// raw / roffs / nq / total / first_id as in vc_dbscan_edge_kernel, whose binary search and rule v < own these are.  cd [records] is
// final for every record up to first_id + nq - 1.  w and t select the level that is written, so each is tested against max_radius
// first.  n_pairs[d] += the acting entries of distance d, through vc_levels_union_kernel's 64 LDS counters.
__global__ void __launch_bounds__(DL_BLK) vc_dbscan_levels_edge_kernel(const uint64_t* __restrict__ raw, const uint64_t* __restrict__ roffs, uint32_t nq,
                                                                       uint64_t total, uint32_t first_id, uint32_t id_base, uint64_t n, uint32_t max_radius,
                                                                       const uint32_t* __restrict__ cd, uint32_t* labels,
                                                                       unsigned long long* __restrict__ n_pairs) {
  __shared__ uint32_t hist[VC_LEVELS_MAX];
  if (threadIdx.x < VC_LEVELS_MAX) hist[threadIdx.x] = 0;
  __syncthreads();
  for (uint64_t p0 = (uint64_t)blockIdx.x * DL_BLK; p0 < total; p0 += (uint64_t)gridDim.x * DL_BLK) {   // (block-uniform bounds: every lane votes)
    const uint64_t p = p0 + threadIdx.x;
    bool act = false;
    uint32_t own = 0, v = 0, d = 0;
    if (p < total) {
      uint32_t lo = 0, hi = nq;   // roffs[lo] <= p < roffs[hi]
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (roffs[mid] <= p) lo = mid; else hi = mid;
      }
      own = first_id + lo;
      const uint64_t entry = raw[p];
      v = (uint32_t)entry;
      d = (uint32_t)(entry >> 32);
      act = v < own && d <= max_radius;
    }
    for (uint64_t open = __ballot(act); open;) {   // (wave-uniform)
      const uint32_t d0 = (uint32_t)__shfl((int)d, __ffsll((long long)open) - 1);
      const uint64_t same = __ballot(act && d == d0);
      if (vc_lane() == 0) atomicAdd(&hist[d0], (uint32_t)__popcll(same));
      open &= ~same;
    }
    if (act) {
      const uint32_t cd_own = cd[own - id_base], cd_v = cd[v - id_base];
      const uint32_t t_own = d > cd_v ? d : cd_v, t_v = d > cd_own ? d : cd_own;   // v a core neighbour of own from level t_own on; own of v from t_v on
      const uint32_t w = t_own > cd_own ? t_own : cd_own;
      if (w <= max_radius) {
        cl_unite(labels + (uint64_t)w * n, id_base, own, v);
      }
      if (t_own < cd_own && t_own <= max_radius) dl_lower(labels + (uint64_t)t_own * n + (own - id_base), own, v);
      if (t_v < cd_v && t_v <= max_radius) dl_lower(labels + (uint64_t)t_v * n + (v - id_base), v, own);
    }
  }
  __syncthreads();
  if (threadIdx.x < VC_LEVELS_MAX && hist[threadIdx.x]) atomicAdd(n_pairs + threadIdx.x, (unsigned long long)hist[threadIdx.x]);
}

// `below` = level r - 1 is final and only read, `level` = level r.  A record that is no core at r - 1 is passed over: its slot
// there is an anchor, not a parent.  A core that is its own root there has nothing to carry up.
__global__ void __launch_bounds__(DL_BLK) vc_dbscan_levels_cascade_kernel(const uint32_t* below, uint32_t* level, const uint32_t* __restrict__ cd, uint64_t n,
                                                                          uint32_t id_base, uint32_t r) {
  for (uint64_t i = (uint64_t)blockIdx.x * DL_BLK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * DL_BLK) {
    if (cd[i] > r - 1) continue;
    const uint32_t own = id_base + (uint32_t)i, x = cl_find(below, id_base, own);
    if (x != own) {
      cl_unite(level, id_base, own, x);
    }
  }
}

// In place, one thread per record, r = 0 .. max_radius in turn.  A core of level r writes its root: a walk through a slot already
// written reads that root, still an ancestor chain with the same end (vc_dbscan_finish_kernel's argument, level by level).  A
// non-core reads ITS OWN slot (r, i) -- its candidate of exactly level r, which nobody else reads or writes here -- BEFORE it writes
// it, keeps the minimum of the candidates so far in a register and writes that anchor's root in forest r (the anchor is a core of
// level r, so the walk passes through core slots only), or leaves the own id.  counts [4][VC_LEVELS_MAX]: [0][r] += the roots
// among the cores of level r, [1][r] the cores, [2][r] the borders, [3][r] the noise: a wave adds into the block's 4 x 64 LDS
// counters, a block flushes its non-zero counters with one global add each.  A block counts fewer than 2^32 records.
__global__ void __launch_bounds__(DL_BLK) vc_dbscan_levels_finish_kernel(uint32_t* labels, const uint32_t* __restrict__ cd, uint64_t n, uint32_t id_base,
                                                                         uint32_t max_radius, unsigned long long* __restrict__ counts) {
  __shared__ uint32_t cnt[4 * VC_LEVELS_MAX];
  cnt[threadIdx.x] = 0;   // (DL_BLK == 4 * VC_LEVELS_MAX)
  __syncthreads();
  for (uint64_t i0 = (uint64_t)blockIdx.x * DL_BLK; i0 < n; i0 += (uint64_t)gridDim.x * DL_BLK) {   // (block-uniform bounds: every lane votes)
    const uint64_t i = i0 + threadIdx.x;
    const bool live = i < n;
    const uint32_t x = id_base + (uint32_t)i, c = live ? cd[i] : 0;
    uint32_t anchor = x;   // the own id: none yet
    for (uint32_t r = 0; r <= max_radius; ++r) {   // (uniform)
      bool is_root = false, is_core = false, is_border = false;
      if (live) {
        uint32_t* slot = labels + (uint64_t)r * n + i;
        if (c <= r) {
          const uint32_t root = cl_find(labels + (uint64_t)r * n, id_base, x);
          cl_st(slot, root);
          is_core = true;
          is_root = root == x;
        } else {
          const uint32_t cand = cl_ld(slot);
          if (cand != x && (anchor == x || cand < anchor)) anchor = cand;
          if (anchor != x) {
            cl_st(slot, cl_find(labels + (uint64_t)r * n, id_base, anchor));
            is_border = true;
          }
        }
      }
      const uint32_t roots = (uint32_t)__popcll(__ballot(is_root)), cores = (uint32_t)__popcll(__ballot(is_core));
      const uint32_t borders = (uint32_t)__popcll(__ballot(is_border)), noise = (uint32_t)__popcll(__ballot(live)) - cores - borders;
      if (vc_lane() == 0) {
        if (roots) atomicAdd(&cnt[0 * VC_LEVELS_MAX + r], roots);
        if (cores) atomicAdd(&cnt[1 * VC_LEVELS_MAX + r], cores);
        if (borders) atomicAdd(&cnt[2 * VC_LEVELS_MAX + r], borders);
        if (noise) atomicAdd(&cnt[3 * VC_LEVELS_MAX + r], noise);
      }
    }
  }
  __syncthreads();
  if (cnt[threadIdx.x]) atomicAdd(counts + threadIdx.x, (unsigned long long)cnt[threadIdx.x]);
}
static_assert(DL_BLK == 4 * VC_LEVELS_MAX, "the finish kernel's counters: one thread each");

static uint32_t dl_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + DL_BLK - 1) / DL_BLK, 1), 256 * 8); }

hipError_t vc_launch_dbscan_levels_edges(const uint64_t* d_raw, const uint64_t* d_roffs, uint32_t nq, uint64_t total, uint32_t first_id, uint32_t id_base,
                                         uint64_t n, uint32_t max_radius, uint32_t min_pts, uint32_t* d_core_dist, uint32_t* d_labels, uint64_t* d_n_pairs,
                                         hipStream_t s) {
  if (nq == 0) return hipSuccess;
  hipLaunchKernelGGL(vc_dbscan_levels_core_kernel, dim3(dl_grid(nq)), dim3(DL_BLK), 0, s, d_raw, d_roffs, nq, min_pts, max_radius,
                     d_core_dist + (first_id - id_base));
  hipError_t err = hipGetLastError();
  if (err != hipSuccess || total == 0) return err;
  hipLaunchKernelGGL(vc_dbscan_levels_edge_kernel, dim3(dl_grid(total)), dim3(DL_BLK), 0, s, d_raw, d_roffs, nq, total, first_id, id_base, n, max_radius,
                     d_core_dist, d_labels, (unsigned long long*)d_n_pairs);
  return hipGetLastError();
}

hipError_t vc_launch_dbscan_levels_cascade(uint32_t* d_labels, const uint32_t* d_core_dist, uint64_t n, uint32_t id_base, uint32_t max_radius, hipStream_t s) {
  if (n == 0) return hipSuccess;
  for (uint32_t r = 1; r <= max_radius; ++r) {   // level r reads level r - 1 as the launch before left it: stream order is the dependence
    hipLaunchKernelGGL(vc_dbscan_levels_cascade_kernel, dim3(dl_grid(n)), dim3(DL_BLK), 0, s, d_labels + (uint64_t)(r - 1) * n, d_labels + (uint64_t)r * n,
                       d_core_dist, n, id_base, r);
    const hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
  }
  return hipSuccess;
}

hipError_t vc_launch_dbscan_levels_finish(uint32_t* d_labels, const uint32_t* d_core_dist, uint64_t n, uint32_t id_base, uint32_t max_radius,
                                          uint64_t* d_counts, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vc_dbscan_levels_finish_kernel, dim3(dl_grid(n)), dim3(DL_BLK), 0, s, d_labels, d_core_dist, n, id_base, max_radius,
                     (unsigned long long*)d_counts);
  return hipGetLastError();
}

int vc_dbscan_levels_run(const VcStoreView& v, uint32_t max_radius, uint32_t min_pts, uint32_t batch, uint32_t* d_labels, uint32_t* d_core_dist,
                         vc_dbscan_levels_stats* stats, hipStream_t s, std::string* err) {
  const uint64_t N = v.n;
  uint64_t* d_stat = (uint64_t*)v.alloc(VC_WALK_STAT, VC_DBSCAN_LEVELS_STAT_BYTES);
  if (!d_stat) return VC_ERR_NOMEM;
  if (!d_core_dist && !(d_core_dist = (uint32_t*)v.alloc(VC_WALK_RECORD, (size_t)N * 4))) return VC_ERR_NOMEM;
  VC_WALK_HIP(hipMemsetAsync(d_stat, 0, VC_DBSCAN_LEVELS_STAT_BYTES, s));
  for (uint32_t r = 0; r <= max_radius; ++r) VC_WALK_HIP(vc_launch_cluster_init(d_labels + (uint64_t)r * N, N, v.id_base, s));
  const int rc = vc_walk_run(v, 0, batch, max_radius, [&](const VcWalkBatch& b) -> int {   // the batch's core distances, then its edges over the raw result
    VC_WALK_HIP(vc_launch_dbscan_levels_edges(b.d_raw, b.d_roffs, b.nq, b.raw_total, b.first_id, v.id_base, N, max_radius, min_pts, d_core_dist, d_labels,
                                              d_stat, s));
    return VC_OK;
  }, s, err);
  if (rc) return rc;
  VC_WALK_HIP(vc_launch_dbscan_levels_cascade(d_labels, d_core_dist, N, v.id_base, max_radius, s));
  VC_WALK_HIP(vc_launch_dbscan_levels_finish(d_labels, d_core_dist, N, v.id_base, max_radius, d_stat + VC_LEVELS_MAX, s));
  vc_dbscan_levels_stats st;
  VC_WALK_HIP(hipMemcpyAsync(&st, d_stat, VC_DBSCAN_LEVELS_STAT_BYTES, hipMemcpyDeviceToHost, s));
  VC_WALK_HIP(hipStreamSynchronize(s));
  if (stats) *stats = st;
  return VC_OK;
}

int vc_dbscan_levels_run_host(const VcStoreView& v, uint32_t max_radius, uint32_t min_pts, uint32_t batch, uint32_t* labels, uint32_t* core_dist,
                              vc_dbscan_levels_stats* stats, hipStream_t s, std::string* err) {
  const size_t N = (size_t)v.n, levels = (size_t)max_radius + 1;
  uint32_t* d_labels = nullptr;
  uint32_t* d_core_dist = (uint32_t*)v.alloc(VC_WALK_RECORD, N * 4);
  if (!d_core_dist) return VC_ERR_NOMEM;
  int rc = vc_walk_stage_labels(v, labels, levels, 0, &d_labels, s, err);
  if (rc || (rc = vc_dbscan_levels_run(v, max_radius, min_pts, batch, d_labels, d_core_dist, stats, s, err))) return rc;
  VC_WALK_HIP(hipMemcpyAsync(labels, d_labels, levels * N * 4, hipMemcpyDeviceToHost, s));
  if (core_dist) VC_WALK_HIP(hipMemcpyAsync(core_dist, d_core_dist, N * 4, hipMemcpyDeviceToHost, s));
  VC_WALK_HIP(hipStreamSynchronize(s));
  return VC_OK;
}
