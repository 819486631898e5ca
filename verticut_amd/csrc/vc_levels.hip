// ============================================================================
// vc_levels.hip -- single-linkage clusters at every radius 0 .. R in ONE walk (vc_cluster_levels*, vc_sharded_cluster_levels*).
// The raw result of the radius search at R holds every pair within every smaller radius, its distance in the high word.  One forest
// per level, in place in the level-major label array (forest r = labels + r * n); the forest and its primitives are vc_forest.hpp's.
// ============================================================================
#include <algorithm>

#include "vc_forest.hpp"
#include "vc_internal.hpp"

// A pair of distance d belongs to the radius graphs of the levels d .. R.  It is united in forest d ONLY (one union per pair, not up
// to R + 1); after the last batch the CASCADE carries every level into the next: for r = 1 .. R record i is united in forest r with
// its root in forest r - 1, which is final by then.  By induction forest r - 1 connects exactly what the pairs of distance <= r - 1
// connect, so after its step forest r connects what those and the pairs of distance r connect: the pairs of distance <= r.  The
// incoming labels of the incremental form are trees of their level like any other.  The label of a record at a level -- the
// smallest id of its component -- depends on the database and the level only.
//   vc_levels_union_kernel    one thread per entry of the flat raw result: its query by binary search, the keep rule, the union in the
//                             forest of the entry's distance; the histogram of the kept distances
//   vc_levels_cascade_kernel  one level: record i, no root below, joins its root of the level below
//   vc_levels_flatten_kernel  labels[r][i] = root of i at level r, in place, all levels in one launch; counts the roots per level
#define LV_BLK 256u

// raw / roffs, the binary search and the KEEP RULE are vc_cluster_union_kernel's (vc_cluster.hip): the entry (dist, v) of the query
// with id `own` is kept when v > own or v < first_new.  dist <= max_radius holds for every entry of the search; it is tested all
// the same, since dist selects the forest that is written.  n_pairs[d] += the kept entries of distance d: a wave adds once per
// distinct distance among its kept entries (a query's entries ascend by distance, so that is one or two) into the block's 64 LDS
// counters, and a block flushes its non-zero counters with one global add each.  A block counts fewer than 2^32 entries.
__global__ void __launch_bounds__(LV_BLK) vc_levels_union_kernel(const uint64_t* __restrict__ raw, const uint64_t* __restrict__ roffs, uint32_t nq,
                                                                 uint64_t total, uint32_t first_id, uint64_t first_new, uint32_t id_base, uint64_t n,
                                                                 uint32_t max_radius, uint32_t* labels, unsigned long long* __restrict__ n_pairs) {
  __shared__ uint32_t hist[VC_LEVELS_MAX];
  if (threadIdx.x < VC_LEVELS_MAX) hist[threadIdx.x] = 0;
  __syncthreads();
  for (uint64_t p0 = (uint64_t)blockIdx.x * LV_BLK; p0 < total; p0 += (uint64_t)gridDim.x * LV_BLK) {   // (block-uniform bounds: every lane votes)
    const uint64_t p = p0 + threadIdx.x;
    bool keep = false;
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
      keep = (v > own || (uint64_t)v < first_new) && d <= max_radius;
    }
    for (uint64_t open = __ballot(keep); open;) {   // (wave-uniform)
      const uint32_t d0 = (uint32_t)__shfl((int)d, __ffsll((long long)open) - 1);
      const uint64_t same = __ballot(keep && d == d0);
      if (vc_lane() == 0) atomicAdd(&hist[d0], (uint32_t)__popcll(same));
      open &= ~same;
    }
    if (keep) {
      cl_unite(labels + (uint64_t)d * n, id_base, own, v);
    }
  }
  __syncthreads();
  if (threadIdx.x < VC_LEVELS_MAX && hist[threadIdx.x]) atomicAdd(n_pairs + threadIdx.x, (unsigned long long)hist[threadIdx.x]);
}

// `below` is final and only read; a record that is its own root there has nothing to carry up.
__global__ void __launch_bounds__(LV_BLK) vc_levels_cascade_kernel(const uint32_t* below, uint32_t* level, uint64_t n, uint32_t id_base) {
  for (uint64_t i = (uint64_t)blockIdx.x * LV_BLK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * LV_BLK) {
    const uint32_t own = id_base + (uint32_t)i, x = cl_find(below, id_base, own);
    if (x != own) {
      cl_unite(level, id_base, own, x);
    }
  }
}

// blockIdx.y is the level.  In place and race-free against itself, as vc_cluster_flatten_kernel: a walk only reads, record i writes
// only its own slot, with its root.  n_clusters[level] += the roots, one add per wave.
__global__ void __launch_bounds__(LV_BLK) vc_levels_flatten_kernel(uint32_t* labels, uint64_t n, uint32_t id_base,
                                                                   unsigned long long* __restrict__ n_clusters) {
  uint32_t* level = labels + (uint64_t)blockIdx.y * n;
  uint32_t roots = 0;   // wave-uniform
  for (uint64_t i0 = (uint64_t)blockIdx.x * LV_BLK; i0 < n; i0 += (uint64_t)gridDim.x * LV_BLK) {
    const uint64_t i = i0 + threadIdx.x;
    bool is_root = false;
    if (i < n) {
      const uint32_t x = id_base + (uint32_t)i, r = cl_find(level, id_base, x);
      cl_st(level + i, r);
      is_root = r == x;
    }
    roots += (uint32_t)__popcll(__ballot(is_root));
  }
  if (vc_lane() == 0 && roots) atomicAdd(n_clusters + blockIdx.y, (unsigned long long)roots);
}

static uint32_t lv_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + LV_BLK - 1) / LV_BLK, 1), 256 * 8); }

hipError_t vc_launch_levels_union(const uint64_t* d_raw, const uint64_t* d_roffs, uint32_t nq, uint64_t total, uint32_t first_id, uint64_t first_new,
                                  uint32_t id_base, uint64_t n, uint32_t max_radius, uint32_t* d_labels, uint64_t* d_n_pairs, hipStream_t s) {
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(vc_levels_union_kernel, dim3(lv_grid(total)), dim3(LV_BLK), 0, s, d_raw, d_roffs, nq, total, first_id, first_new, id_base, n, max_radius,
                     d_labels, (unsigned long long*)d_n_pairs);
  return hipGetLastError();
}

hipError_t vc_launch_levels_cascade(uint32_t* d_labels, uint64_t n, uint32_t id_base, uint32_t max_radius, hipStream_t s) {
  if (n == 0) return hipSuccess;
  for (uint32_t r = 1; r <= max_radius; ++r) {   // level r reads level r - 1 as the launch before left it: stream order is the dependence
    hipLaunchKernelGGL(vc_levels_cascade_kernel, dim3(lv_grid(n)), dim3(LV_BLK), 0, s, d_labels + (uint64_t)(r - 1) * n, d_labels + (uint64_t)r * n, n, id_base);
    const hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
  }
  return hipSuccess;
}

hipError_t vc_launch_levels_flatten(uint32_t* d_labels, uint64_t n, uint32_t id_base, uint32_t max_radius, uint64_t* d_n_clusters, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vc_levels_flatten_kernel, dim3(lv_grid(n), max_radius + 1), dim3(LV_BLK), 0, s, d_labels, n, id_base, (unsigned long long*)d_n_clusters);
  return hipGetLastError();
}

int vc_levels_run(const VcStoreView& v, uint32_t max_radius, uint32_t batch, uint64_t n_labelled, uint32_t* d_labels, vc_levels_stats* stats, hipStream_t s,
                  std::string* err) {
  const uint64_t N = v.n, first_new = (uint64_t)v.id_base + n_labelled;
  uint64_t* d_stat = (uint64_t*)v.alloc(VC_WALK_STAT, VC_LEVELS_STAT_BYTES);
  if (!d_stat) return VC_ERR_NOMEM;
  VC_WALK_HIP(hipMemsetAsync(d_stat, 0, VC_LEVELS_STAT_BYTES, s));
  for (uint32_t r = 0; r <= max_radius; ++r) VC_WALK_HIP(vc_launch_cluster_init(d_labels + (uint64_t)r * N + n_labelled, N - n_labelled, (uint32_t)first_new, s));
  const int rc = vc_walk_run(v, n_labelled, batch, max_radius, [&](const VcWalkBatch& b) -> int {   // every kept entry in the forest of its distance
    VC_WALK_HIP(vc_launch_levels_union(b.d_raw, b.d_roffs, b.nq, b.raw_total, b.first_id, first_new, v.id_base, N, max_radius, d_labels, d_stat, s));
    return VC_OK;
  }, s, err);
  if (rc) return rc;
  VC_WALK_HIP(vc_launch_levels_cascade(d_labels, N, v.id_base, max_radius, s));
  VC_WALK_HIP(vc_launch_levels_flatten(d_labels, N, v.id_base, max_radius, d_stat + VC_LEVELS_MAX, s));
  vc_levels_stats st;
  VC_WALK_HIP(hipMemcpyAsync(&st, d_stat, VC_LEVELS_STAT_BYTES, hipMemcpyDeviceToHost, s));
  VC_WALK_HIP(hipStreamSynchronize(s));
  if (stats) *stats = st;
  return VC_OK;
}

int vc_levels_run_host(const VcStoreView& v, uint32_t max_radius, uint32_t batch, uint64_t n_labelled, uint32_t* labels, vc_levels_stats* stats, hipStream_t s,
                       std::string* err) {
  const size_t levels = (size_t)max_radius + 1;
  uint32_t* d_labels = nullptr;
  int rc = vc_walk_stage_labels(v, labels, levels, n_labelled, &d_labels, s, err);
  if (rc || (rc = vc_levels_run(v, max_radius, batch, n_labelled, d_labels, stats, s, err))) return rc;
  VC_WALK_HIP(hipMemcpyAsync(labels, d_labels, levels * (size_t)v.n * 4, hipMemcpyDeviceToHost, s));
  VC_WALK_HIP(hipStreamSynchronize(s));
  return VC_OK;
}
