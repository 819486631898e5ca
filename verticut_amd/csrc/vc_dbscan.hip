// ============================================================================
// vc_dbscan.hip -- density clustering on the device (vc_dbscan_radius*, vc_sharded_dbscan_radius*): DBSCAN over the RAW result of the
// radius search underneath, in ONE walk of the ids.  No compaction, no plan, no LDS.
// ============================================================================
#include <algorithm>

#include "vc_forest.hpp"
#include "vc_internal.hpp"

// THE RULE: degrees[i] = the records within the radius of record i, itself included = the length of its raw segment (the radius
// search returns every such record exactly once).  A record is a CORE iff degrees[i] >= min_pts; the clusters are the components of
// the graph whose vertices are the cores and whose edges join two cores within the radius; a non-core record with a core within the
// radius is a BORDER of the cluster of its SMALLEST-id core neighbour; every other record is NOISE.
// ONE WALK: the batches are taken in ascending id order.  The degree kernel of a batch makes the degrees of its queries final, so
// after it every record up to the batch's end has its final degree.  The edge kernel then acts on the entries (query own, neighbour
// v) with v < own only: every unordered pair is met exactly once, from its larger member, and at that moment both degrees are final
// whether v lies in this batch or below it.
// STATE, in labels[] itself and without a sentinel (every 32-bit value is a legal id):
//   a core's slot      the forest of vc_forest.hpp over the cores: the global id of its parent, its own id at a root;
//   a non-core's slot  its ANCHOR: its own id = "no core neighbour seen", else the smallest core neighbour seen so far (an anchor is
//                      never the record itself, so the two cannot be confused); lowered by a CAS loop, so it ends as the minimum
//                      over all core neighbours whatever the order of the lanes.
// Both kinds start as the own id.  Unions touch only core slots (both ends of a union are cores, and a core's chain passes through
// cores only: a core is hooked under a core), anchors only non-core slots, so no walk ever reads an anchor and no anchor store ever
// lands in the forest.  Which kind a slot is, is decided by degrees[] alone, never by its content.
//   vc_dbscan_degree_kernel   degrees of a batch's queries from its offsets
//   vc_dbscan_edge_kernel     one thread per entry of the flat raw result: its query by binary search, then union or anchor
//   vc_dbscan_finish_kernel   labels[i] = root (core), root of the anchor (border) or own id (noise), in place; counts the kinds
// All accesses to the forest and the anchors are relaxed device-scope atomics; no kernel waits for another block.
#define DB_BLK 256u

__global__ void __launch_bounds__(DB_BLK) vc_dbscan_degree_kernel(const uint64_t* __restrict__ roffs, uint32_t nq, uint32_t* __restrict__ deg) {
  for (uint32_t q = blockIdx.x * DB_BLK + threadIdx.x; q < nq; q += gridDim.x * DB_BLK) deg[q] = (uint32_t)(roffs[q + 1] - roffs[q]);
}

// raw / roffs / nq / total / first_id as in vc_cluster_union_kernel, whose binary search this is.  degrees [records] is final for every
// record up to first_id + nq - 1.  Entries with v >= own (the own entry among them) are passed over.  *n_pairs += the acting entries,
// one add per wave.
__global__ void __launch_bounds__(DB_BLK) vc_dbscan_edge_kernel(const uint64_t* __restrict__ raw, const uint64_t* __restrict__ roffs, uint32_t nq,
                                                                uint64_t total, uint32_t first_id, uint32_t id_base, uint32_t min_pts,
                                                                const uint32_t* __restrict__ degrees, uint32_t* labels,
                                                                unsigned long long* __restrict__ n_pairs) {
  uint32_t acted = 0;   // wave-uniform
  for (uint64_t p0 = (uint64_t)blockIdx.x * DB_BLK; p0 < total; p0 += (uint64_t)gridDim.x * DB_BLK) {   // (block-uniform bounds: every lane votes)
    const uint64_t p = p0 + threadIdx.x;
    bool act = false;
    uint32_t own = 0, v = 0;
    if (p < total) {
      uint32_t lo = 0, hi = nq;   // roffs[lo] <= p < roffs[hi]
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (roffs[mid] <= p) lo = mid; else hi = mid;
      }
      own = first_id + lo;
      v = (uint32_t)raw[p];
      act = v < own;
    }
    acted += (uint32_t)__popcll(__ballot(act));
    if (act) {
      const bool core_own = degrees[own - id_base] >= min_pts, core_v = degrees[v - id_base] >= min_pts;
      if (core_own && core_v) {
        cl_unite(labels, id_base, own, v);
      } else if (core_own != core_v) {
        // the non-core member notes the core: its slot takes the candidate while it still holds the own id, else the smaller of the two
        const uint32_t sparse = core_own ? v : own, cand = core_own ? own : v;
        uint32_t* slot = labels + (sparse - id_base);
        uint32_t cur = cl_ld(slot);
        while (cur == sparse || cand < cur) {
          const uint32_t seen = atomicCAS(slot, cur, cand);
          if (seen == cur) break;
          cur = seen;
        }
      }
    }
  }
  if (vc_lane() == 0 && acted) atomicAdd(n_pairs, (unsigned long long)acted);
}

// In place, race-free against itself: a walk passes through core slots only and only reads; record i writes only its own slot.  A
// core writes its root -- a walk through a slot already written reads that root, still an ancestor chain with the same end (the
// argument of vc_cluster_flatten_kernel).  A non-core record reads its own slot (its anchor, which nobody else reads or writes here)
// and writes the anchor's root or leaves the own id.  counts: [0] += the roots among the cores, [1] cores, [2] borders, [3] noise,
// one add per wave and counter.
__global__ void __launch_bounds__(DB_BLK) vc_dbscan_finish_kernel(uint32_t* labels, const uint32_t* __restrict__ degrees, uint64_t n, uint32_t id_base,
                                                                  uint32_t min_pts, unsigned long long* __restrict__ counts) {
  uint32_t roots = 0, cores = 0, borders = 0, noise = 0;   // wave-uniform
  for (uint64_t i0 = (uint64_t)blockIdx.x * DB_BLK; i0 < n; i0 += (uint64_t)gridDim.x * DB_BLK) {
    const uint64_t i = i0 + threadIdx.x;
    bool is_root = false, is_core = false, is_border = false, is_noise = false;
    if (i < n) {
      const uint32_t x = id_base + (uint32_t)i;
      if (degrees[i] >= min_pts) {
        const uint32_t r = cl_find(labels, id_base, x);
        cl_st(labels + i, r);
        is_core = true;
        is_root = r == x;
      } else {
        const uint32_t anchor = cl_ld(labels + i);
        if (anchor != x) {
          cl_st(labels + i, cl_find(labels, id_base, anchor));
          is_border = true;
        } else {
          is_noise = true;
        }
      }
    }
    roots += (uint32_t)__popcll(__ballot(is_root));
    cores += (uint32_t)__popcll(__ballot(is_core));
    borders += (uint32_t)__popcll(__ballot(is_border));
    noise += (uint32_t)__popcll(__ballot(is_noise));
  }
  if (vc_lane() == 0) {
    if (roots) atomicAdd(counts + 0, (unsigned long long)roots);
    if (cores) atomicAdd(counts + 1, (unsigned long long)cores);
    if (borders) atomicAdd(counts + 2, (unsigned long long)borders);
    if (noise) atomicAdd(counts + 3, (unsigned long long)noise);
  }
}

static uint32_t db_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + DB_BLK - 1) / DB_BLK, 1), 256 * 8); }

hipError_t vc_launch_dbscan_edges(const uint64_t* d_raw, const uint64_t* d_roffs, uint32_t nq, uint64_t total, uint32_t first_id, uint32_t id_base,
                                  uint32_t min_pts, uint32_t* d_degrees, uint32_t* d_labels, uint64_t* d_n_pairs, hipStream_t s) {
  if (nq == 0) return hipSuccess;
  hipLaunchKernelGGL(vc_dbscan_degree_kernel, dim3(db_grid(nq)), dim3(DB_BLK), 0, s, d_roffs, nq, d_degrees + (first_id - id_base));
  hipError_t err = hipGetLastError();
  if (err != hipSuccess || total == 0) return err;
  hipLaunchKernelGGL(vc_dbscan_edge_kernel, dim3(db_grid(total)), dim3(DB_BLK), 0, s, d_raw, d_roffs, nq, total, first_id, id_base, min_pts, d_degrees,
                     d_labels, (unsigned long long*)d_n_pairs);
  return hipGetLastError();
}

hipError_t vc_launch_dbscan_finish(uint32_t* d_labels, const uint32_t* d_degrees, uint64_t n, uint32_t id_base, uint32_t min_pts, uint64_t* d_counts,
                                   hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vc_dbscan_finish_kernel, dim3(db_grid(n)), dim3(DB_BLK), 0, s, d_labels, d_degrees, n, id_base, min_pts,
                     (unsigned long long*)d_counts);
  return hipGetLastError();
}

int vc_dbscan_run(const VcStoreView& v, uint32_t radius, uint32_t min_pts, uint32_t batch, uint32_t* d_labels, uint32_t* d_degrees, vc_dbscan_stats* stats,
                  hipStream_t s, std::string* err) {
  const uint64_t N = v.n;
  uint64_t* d_stat = (uint64_t*)v.alloc(VC_WALK_STAT, VC_DBSCAN_STAT_BYTES);
  if (!d_stat) return VC_ERR_NOMEM;
  if (!d_degrees && !(d_degrees = (uint32_t*)v.alloc(VC_WALK_RECORD, (size_t)N * 4))) return VC_ERR_NOMEM;
  VC_WALK_HIP(hipMemsetAsync(d_stat, 0, VC_DBSCAN_STAT_BYTES, s));
  VC_WALK_HIP(vc_launch_cluster_init(d_labels, N, v.id_base, s));
  const int rc = vc_walk_run(v, 0, batch, radius, [&](const VcWalkBatch& b) -> int {   // the batch's degrees, then its edges over the raw result as it lies
    VC_WALK_HIP(vc_launch_dbscan_edges(b.d_raw, b.d_roffs, b.nq, b.raw_total, b.first_id, v.id_base, min_pts, d_degrees, d_labels, d_stat, s));
    return VC_OK;
  }, s, err);
  if (rc) return rc;
  VC_WALK_HIP(vc_launch_dbscan_finish(d_labels, d_degrees, N, v.id_base, min_pts, d_stat + 1, s));
  uint64_t st[5] = {0, 0, 0, 0, 0};
  VC_WALK_HIP(hipMemcpyAsync(st, d_stat, VC_DBSCAN_STAT_BYTES, hipMemcpyDeviceToHost, s));
  VC_WALK_HIP(hipStreamSynchronize(s));
  if (stats) *stats = vc_dbscan_stats{st[0], st[1], st[2], st[3], st[4]};
  return VC_OK;
}

int vc_dbscan_run_host(const VcStoreView& v, uint32_t radius, uint32_t min_pts, uint32_t batch, uint32_t* labels, uint32_t* degrees, vc_dbscan_stats* stats,
                       hipStream_t s, std::string* err) {
  const size_t bytes = (size_t)v.n * 4;
  uint32_t* d_labels = nullptr;
  uint32_t* d_degrees = (uint32_t*)v.alloc(VC_WALK_RECORD, bytes);
  if (!d_degrees) return VC_ERR_NOMEM;
  int rc = vc_walk_stage_labels(v, labels, 1, 0, &d_labels, s, err);
  if (rc || (rc = vc_dbscan_run(v, radius, min_pts, batch, d_labels, d_degrees, stats, s, err))) return rc;
  VC_WALK_HIP(hipMemcpyAsync(labels, d_labels, bytes, hipMemcpyDeviceToHost, s));
  if (degrees) VC_WALK_HIP(hipMemcpyAsync(degrees, d_degrees, bytes, hipMemcpyDeviceToHost, s));
  VC_WALK_HIP(hipStreamSynchronize(s));
  return VC_OK;
}
