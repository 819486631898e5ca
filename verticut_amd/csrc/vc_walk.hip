// ============================================================================
// vc_walk.hip -- the radius-graph walk under the clustering calls (vc_cluster_radius*, vc_cluster_levels*, vc_leaders_radius*,
// vc_dbscan_radius*, vc_dbscan_levels* and their vc_sharded_* forms), and what every driver over a VcStoreView shares: host code only.
// The handle comes as that view, so nothing here knows an engine from a sharded store, or which device is current.
// ============================================================================
#include <algorithm>

#include "vc_internal.hpp"

int vc_hip_fail(std::string* err, const char* who, hipError_t r, const char* what) {
  if (err) *err = std::string(who) + ": " + what + ": " + hipGetErrorString(r);
  return r == hipErrorOutOfMemory ? VC_ERR_NOMEM : VC_ERR_HIP;
}

int vc_search_raw(const VcStoreView& v, int raw_buf, const uint64_t* d_q, uint32_t nq, uint32_t radius, uint64_t** d_raw, uint64_t* d_roffs, uint64_t* raw_total) {
  *raw_total = 0;
  for (int attempt = 0;; ++attempt) {
    const uint64_t cap = v.held(raw_buf) / 8;
    const int rc = v.search(d_q, nq, radius, *d_raw, cap, d_roffs, raw_total);
    if (rc != VC_ERR_CAPACITY || attempt || *raw_total <= cap) return rc;
    if (!(*d_raw = (uint64_t*)v.alloc(raw_buf, (size_t)*raw_total * 8))) return VC_ERR_NOMEM;   // (search has waited: nothing reads the old one)
  }
}

int vc_walk_run(const VcStoreView& v, uint64_t first_pos, uint32_t batch, uint32_t radius, const std::function<int(const VcWalkBatch&)>& consume, hipStream_t s,
                std::string* err) {
  if (first_pos >= v.n) return VC_OK;
  batch = vc_walk_batch(batch);
  const size_t nq_max = (size_t)std::min<uint64_t>(batch, v.n - first_pos);
  uint32_t* d_ids = (uint32_t*)v.alloc(VC_WALK_IDS, nq_max * 4);
  uint64_t* d_q = (uint64_t*)v.alloc(VC_WALK_Q, nq_max * v.W * 8);
  uint32_t* d_found = (uint32_t*)v.alloc(VC_WALK_FOUND, nq_max * 4);
  uint64_t* d_roffs = (uint64_t*)v.alloc(VC_WALK_ROFFS, (nq_max + 1) * 8);
  uint64_t* d_raw = (uint64_t*)v.alloc(VC_WALK_RAW, VC_RAW_FIRST_BYTES);
  if (!d_ids || !d_q || !d_found || !d_roffs || !d_raw) return VC_ERR_NOMEM;
  int rc;
  for (uint64_t pos = first_pos; pos < v.n; pos += batch) {
    const uint32_t nq = (uint32_t)std::min<uint64_t>(batch, v.n - pos), first_id = v.id_base + (uint32_t)pos;
    VC_WALK_HIP(vc_launch_cluster_init(d_ids, nq, first_id, s));
    if ((rc = v.gather(d_ids, nq, d_q, d_found))) return rc;
    uint64_t raw_total;
    if ((rc = vc_search_raw(v, VC_WALK_RAW, d_q, nq, radius, &d_raw, d_roffs, &raw_total))) return rc;
    if ((rc = consume(VcWalkBatch{d_raw, d_roffs, nq, raw_total, first_id}))) return rc;
  }
  return VC_OK;
}

int vc_walk_stage_labels(const VcStoreView& v, const uint32_t* labels, size_t planes, uint64_t n_labelled, uint32_t** d_labels, hipStream_t s, std::string* err) {
  const size_t N = (size_t)v.n;
  uint32_t* d = (uint32_t*)v.alloc(VC_WALK_HLAB, planes * N * 4);
  if (!d) return VC_ERR_NOMEM;
  if (n_labelled)
    for (size_t r = 0; r < planes; ++r) VC_WALK_HIP(hipMemcpyAsync(d + r * N, labels + r * N, (size_t)n_labelled * 4, hipMemcpyHostToDevice, s));
  *d_labels = d;
  return VC_OK;
}
