// ============================================================================
// vc_cluster.hip -- near-duplicate clustering on the device (vc_cluster_radius*, vc_sharded_cluster_radius*): the connected
// components of the radius graph, by a lock-free union-find over the RAW result of the radius search underneath.  No compaction,
// no plan, no LDS: the union needs neither sorted nor gap-free segments.
// ============================================================================
#include <algorithm>

#include "vc_forest.hpp"
#include "vc_internal.hpp"

// labels[] IS the forest, in place; the forest, its three invariants and its primitives are vc_forest.hpp's.  Once every kept entry
// has been united the trees are the components of the radius graph, so the flattened label of a record -- the smallest id of its
// component -- depends on the database and the radius only, not on the order in which the lanes arrived.
//   vc_cluster_init_kernel     dst[j] = first + j: the labels of the records that come in unlabelled, and a batch's ids
//   vc_cluster_union_kernel    one thread per entry of the flat raw result: its query by binary search, the keep rule, the union
//   vc_cluster_flatten_kernel  labels[i] = root of i, in place; counts the roots
#define CL_BLK 256u

__global__ void __launch_bounds__(CL_BLK) vc_cluster_init_kernel(uint32_t* __restrict__ dst, uint64_t count, uint32_t first) {
  for (uint64_t j = (uint64_t)blockIdx.x * CL_BLK + threadIdx.x; j < count; j += (uint64_t)gridDim.x * CL_BLK) dst[j] = first + (uint32_t)j;
}

// raw / roffs: the flat result of the radius search for the queries first_id + 0 .. first_id + nq - 1 and its nq + 1 offsets; total =
// roffs[nq].  Entry p belongs to the last query q with roffs[q] <= p (queries without entries share their successor's offset and are
// passed over); the 64 consecutive entries of a wave mostly share one query, so the search's loads are broadcasts out of the cache.
// KEEP RULE: the entry (dist, v) of the query with id `own` is united when v > own, or when v < first_new = id_base + n_labelled:
// every pair of new records is seen once, from its smaller member, and every pair with an old member from its new one (old records
// are not queried).  The own entry and the smaller new ids are dropped.  *n_pairs += the kept entries, one add per wave.
__global__ void __launch_bounds__(CL_BLK) vc_cluster_union_kernel(const uint64_t* __restrict__ raw, const uint64_t* __restrict__ roffs, uint32_t nq,
                                                                  uint64_t total, uint32_t first_id, uint64_t first_new, uint32_t id_base,
                                                                  uint32_t* labels, unsigned long long* __restrict__ n_pairs) {
  uint32_t kept = 0;   // wave-uniform
  for (uint64_t p0 = (uint64_t)blockIdx.x * CL_BLK; p0 < total; p0 += (uint64_t)gridDim.x * CL_BLK) {   // (block-uniform bounds: every lane votes)
    const uint64_t p = p0 + threadIdx.x;
    bool keep = false;
    uint32_t own = 0, v = 0;
    if (p < total) {
      uint32_t lo = 0, hi = nq;   // roffs[lo] <= p < roffs[hi]
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (roffs[mid] <= p) lo = mid; else hi = mid;
      }
      own = first_id + lo;
      v = (uint32_t)raw[p];
      keep = v > own || (uint64_t)v < first_new;
    }
    kept += (uint32_t)__popcll(__ballot(keep));
    if (keep) {
      cl_unite(labels, id_base, own, v);
    }
  }
  if (vc_lane() == 0 && kept) atomicAdd(n_pairs, (unsigned long long)kept);
}

// In place, race-free against itself: a walk only reads, and record i writes only its own slot, with its root.  A walk that passes
// through a slot already written reads that root -- still an ancestor chain ending in the same root -- so every record stores the
// same value whatever the order.  A root's slot is rewritten with itself.  *n_clusters += the roots, one add per wave.
__global__ void __launch_bounds__(CL_BLK) vc_cluster_flatten_kernel(uint32_t* labels, uint64_t n, uint32_t id_base,
                                                                    unsigned long long* __restrict__ n_clusters) {
  uint32_t roots = 0;   // wave-uniform
  for (uint64_t i0 = (uint64_t)blockIdx.x * CL_BLK; i0 < n; i0 += (uint64_t)gridDim.x * CL_BLK) {
    const uint64_t i = i0 + threadIdx.x;
    bool is_root = false;
    if (i < n) {
      const uint32_t x = id_base + (uint32_t)i, r = cl_find(labels, id_base, x);
      cl_st(labels + i, r);
      is_root = r == x;
    }
    roots += (uint32_t)__popcll(__ballot(is_root));
  }
  if (vc_lane() == 0 && roots) atomicAdd(n_clusters, (unsigned long long)roots);
}

static uint32_t cl_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + CL_BLK - 1) / CL_BLK, 1), 256 * 8); }

hipError_t vc_launch_cluster_init(uint32_t* d_dst, uint64_t count, uint32_t first, hipStream_t s) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(vc_cluster_init_kernel, dim3(cl_grid(count)), dim3(CL_BLK), 0, s, d_dst, count, first);
  return hipGetLastError();
}

hipError_t vc_launch_cluster_union(const uint64_t* d_raw, const uint64_t* d_roffs, uint32_t nq, uint64_t total, uint32_t first_id, uint64_t first_new,
                                   uint32_t id_base, uint32_t* d_labels, uint64_t* d_n_pairs, hipStream_t s) {
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(vc_cluster_union_kernel, dim3(cl_grid(total)), dim3(CL_BLK), 0, s, d_raw, d_roffs, nq, total, first_id, first_new, id_base, d_labels,
                     (unsigned long long*)d_n_pairs);
  return hipGetLastError();
}

hipError_t vc_launch_cluster_flatten(uint32_t* d_labels, uint64_t n, uint32_t id_base, uint64_t* d_n_clusters, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vc_cluster_flatten_kernel, dim3(cl_grid(n)), dim3(CL_BLK), 0, s, d_labels, n, id_base, (unsigned long long*)d_n_clusters);
  return hipGetLastError();
}

int vc_cluster_run(const VcStoreView& v, uint32_t radius, uint32_t batch, uint64_t n_labelled, uint32_t* d_labels, vc_cluster_stats* stats, hipStream_t s,
                   std::string* err) {
  const uint64_t first_new = (uint64_t)v.id_base + n_labelled;
  uint64_t* d_stat = (uint64_t*)v.alloc(VC_WALK_STAT, 16);
  if (!d_stat) return VC_ERR_NOMEM;
  VC_WALK_HIP(hipMemsetAsync(d_stat, 0, 16, s));
  VC_WALK_HIP(vc_launch_cluster_init(d_labels + n_labelled, v.n - n_labelled, (uint32_t)first_new, s));
  const int rc = vc_walk_run(v, n_labelled, batch, radius, [&](const VcWalkBatch& b) -> int {   // the union over the raw result as it lies; no compaction
    VC_WALK_HIP(vc_launch_cluster_union(b.d_raw, b.d_roffs, b.nq, b.raw_total, b.first_id, first_new, v.id_base, d_labels, d_stat, s));
    return VC_OK;
  }, s, err);
  if (rc) return rc;
  VC_WALK_HIP(vc_launch_cluster_flatten(d_labels, v.n, v.id_base, d_stat + 1, s));
  uint64_t st[2] = {0, 0};
  VC_WALK_HIP(hipMemcpyAsync(st, d_stat, 16, hipMemcpyDeviceToHost, s));
  VC_WALK_HIP(hipStreamSynchronize(s));
  if (stats) *stats = vc_cluster_stats{st[0], st[1]};
  return VC_OK;
}

int vc_cluster_run_host(const VcStoreView& v, uint32_t radius, uint32_t batch, uint64_t n_labelled, uint32_t* labels, vc_cluster_stats* stats, hipStream_t s,
                        std::string* err) {
  uint32_t* d_labels = nullptr;
  int rc = vc_walk_stage_labels(v, labels, 1, n_labelled, &d_labels, s, err);
  if (rc || (rc = vc_cluster_run(v, radius, batch, n_labelled, d_labels, stats, s, err))) return rc;
  VC_WALK_HIP(hipMemcpyAsync(labels, d_labels, (size_t)v.n * 4, hipMemcpyDeviceToHost, s));
  VC_WALK_HIP(hipStreamSynchronize(s));
  return VC_OK;
}
