// ============================================================================
// vc_ids.hip -- queries named by id (image_search_client::search_image_by_id, image_search_client.h:12-27; the
// ID -> BinaryCode read of linear_search.cc:45-46) for a whole batch, without leaving HBM.
//   vc_ids_gather_kernel  ids -> the [nq][W] query layout + a found word per id, out of the column store
//   vc_ids_strip_kernel   rows of a k' = k + 1 search -> the caller's k rows without the query's own record
//                         (k' = k: pass-through that only applies the found mask)
//   vc_ids_merge_kernel   sharded store: the shards' gathered slots ORed into one query buffer on the root
// None of them uses LDS or scratch; the search in between is the unchanged vc_search_knn_dev_stats.
// The radius search by id (vc_search_radius_ids*) compacts a variable-length result instead: vc_ids_radius.hip.
// ============================================================================
#include <algorithm>

#include "vc_internal.hpp"

// One thread per (query, word): thread e serves word e % W of query e / W, so a wave reads each of the W columns for 64 / W
// ids at once and writes 64 consecutive words.  An id outside [id_base, id_base + n) -- n the RESIDENT count -- gives a zero
// row and found = 0 (the subtraction wraps for id < id_base, which the one unsigned compare then rejects as well).
// fill_n != 0 (the search calls; needs n > 0): an id outside [fill_base, fill_base + fill_n) -- resident nowhere in the store --
// still reports found = 0 but gets the code of local record 0 as its query, so that the search underneath, whose row the strip
// kernel throws away, meets a query that has a neighbour at distance 0 instead of the all-zero code, which may be far from
// every record: the approximate radius loop of such a query walks shells of C(32, r) keys.
__global__ void __launch_bounds__(256) vc_ids_gather_kernel(const uint64_t* __restrict__ cols, uint64_t stride, uint32_t W, uint32_t id_base,
                                                            uint64_t n, uint32_t fill_base, uint64_t fill_n, const uint32_t* __restrict__ ids,
                                                            uint32_t nq, uint64_t* __restrict__ q, uint32_t* __restrict__ found) {
  const uint64_t total = (uint64_t)nq * W;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t i = (uint32_t)(e / W), j = (uint32_t)(e % W);
    const uint32_t id = ids[i], local = id - id_base;
    const bool here = local < n, fill = fill_n && (uint32_t)(id - fill_base) >= fill_n;
    q[e] = (here || fill) ? cols[j * stride + (here ? local : 0u)] : 0ull;
    if (j == 0 && found) found[i] = here ? 1u : 0u;
  }
}

// One thread per (query, output entry j < k).  rows [nq][kp] ascending, VC_PACK_INF padded, cnt[q] of them valid
// (UINT32_MAX == flagged upper-bound row of kp entries, passed on as it is).  kp == k + 1: the entry equal to (uint64)id -- distance
// 0, own id -- is dropped if it is there.  It is matched BY VALUE: duplicates of the record with smaller ids sort before it,
// and with more than k of them it is not in the row at all; the row being ascending, a binary search finds its place.
__global__ void __launch_bounds__(256) vc_ids_strip_kernel(const uint32_t* __restrict__ ids, const uint32_t* __restrict__ found,
                                                           const uint64_t* __restrict__ rows, const uint32_t* __restrict__ cnt, uint32_t nq,
                                                           uint32_t kp, uint32_t k, uint64_t* __restrict__ out, uint32_t* __restrict__ out_cnt,
                                                           vc_query_stats* __restrict__ stats) {
  const uint64_t total = (uint64_t)nq * k;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t i = (uint32_t)(e / k), j = (uint32_t)(e % k);
    if (!found[i]) {
      out[e] = VC_PACK_INF;
      if (j == 0) {
        if (out_cnt) out_cnt[i] = 0;
        if (stats) stats[i] = vc_query_stats{};
      }
      continue;
    }
    const uint64_t* row = rows + (uint64_t)i * kp;
    const uint32_t c = cnt[i], nrow = c < kp ? c : kp;
    const uint64_t self = ids[i];
    uint64_t v = row[j];
    uint32_t present = 0;
    if (kp > k && (v >= self || j == 0)) {
      uint32_t lo = 0, hi = nrow;   // first entry >= self
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (row[mid] < self) lo = mid + 1; else hi = mid;
      }
      present = lo < nrow && row[lo] == self;
      if (present && j >= lo) v = row[j + 1];   // j + 1 <= k < kp
    }
    out[e] = v;
    if (j == 0) {
      const uint32_t left = c == 0xFFFFFFFFu ? c : (c - present < k ? c - present : k);
      if (out_cnt) out_cnt[i] = left;
      if (stats) stats[i].n_results = left;
    }
  }
}

// Sharded store.  Slot g (slot_words apart) holds shard g's [nq][W] gathered words, zero for the ids it does not own, and
// behind them its nq found words.  The id ranges are disjoint, so at most one slot of `mask` is non-zero per row: OR.
__global__ void __launch_bounds__(256) vc_ids_merge_kernel(const uint64_t* __restrict__ slots, uint64_t slot_words, uint32_t mask, uint32_t nq,
                                                           uint32_t W, uint64_t* __restrict__ q, uint32_t* __restrict__ found) {
  const uint64_t total = (uint64_t)nq * W;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t i = (uint32_t)(e / W), j = (uint32_t)(e % W);
    uint64_t w = 0;
    uint32_t f = 0;
    for (uint32_t m = mask; m; m &= m - 1) {
      const uint64_t* slot = slots + (uint64_t)(__builtin_ctz(m)) * slot_words;
      w |= slot[e];
      if (j == 0) f |= ((const uint32_t*)(slot + total))[i];
    }
    q[e] = w;
    if (j == 0 && found) found[i] = f;
  }
}

static uint32_t ids_grid(uint64_t threads) { return (uint32_t)std::min<uint64_t>((threads + 255) / 256, 256 * 8); }

hipError_t vc_launch_ids_gather(const uint64_t* cols, uint64_t stride, uint32_t W, uint32_t id_base, uint64_t n, uint32_t fill_base,
                                uint64_t fill_n, const uint32_t* d_ids, uint32_t nq, uint64_t* d_q, uint32_t* d_found, hipStream_t s) {
  if (nq == 0) return hipSuccess;
  if (n == 0) fill_n = 0;   // nothing to fill with
  hipLaunchKernelGGL(vc_ids_gather_kernel, dim3(ids_grid((uint64_t)nq * W)), dim3(256), 0, s, cols, stride, W, id_base, n, fill_base, fill_n, d_ids,
                     nq, d_q, d_found);
  return hipGetLastError();
}

hipError_t vc_launch_ids_strip(const uint32_t* d_ids, const uint32_t* d_found, const uint64_t* d_rows, const uint32_t* d_cnt, uint32_t nq,
                               uint32_t kp, uint32_t k, uint64_t* d_out, uint32_t* d_out_cnt, vc_query_stats* d_stats, hipStream_t s) {
  if (nq == 0) return hipSuccess;
  hipLaunchKernelGGL(vc_ids_strip_kernel, dim3(ids_grid((uint64_t)nq * k)), dim3(256), 0, s, d_ids, d_found, d_rows, d_cnt, nq, kp, k, d_out,
                     d_out_cnt, d_stats);
  return hipGetLastError();
}

hipError_t vc_launch_ids_merge(const uint64_t* d_slots, uint64_t slot_words, uint32_t mask, uint32_t nq, uint32_t W, uint64_t* d_q,
                               uint32_t* d_found, hipStream_t s) {
  if (nq == 0) return hipSuccess;
  hipLaunchKernelGGL(vc_ids_merge_kernel, dim3(ids_grid((uint64_t)nq * W)), dim3(256), 0, s, d_slots, slot_words, mask, nq, W, d_q, d_found);
  return hipGetLastError();
}

// The strip kernel's rule on the host: the host-pointer calls use it for a LINEAR batch that had to be answered again by the
// host-driven ring-overflow recovery.  rows / cnt / stats: the k' search's; out [nq][k], counts [nq]
void vc_ids_strip_host(const uint32_t* ids, const uint32_t* found, const uint64_t* rows, const uint32_t* cnt, uint32_t nq, uint32_t kp, uint32_t k,
                       uint64_t* out, uint32_t* counts, vc_query_stats* stats) {
  for (uint32_t i = 0; i < nq; ++i) {
    uint64_t* o = out + (size_t)i * k;
    if (!found[i]) {
      std::fill(o, o + k, VC_PACK_INF);
      counts[i] = 0;
      if (stats) stats[i] = vc_query_stats{};
      continue;
    }
    const uint64_t* row = rows + (size_t)i * kp;
    const uint32_t nrow = std::min(cnt[i], kp);
    const uint64_t* self = kp > k ? std::lower_bound(row, row + nrow, (uint64_t)ids[i]) : row + nrow;
    const bool present = self < row + nrow && *self == ids[i];
    uint32_t w = 0;
    for (const uint64_t* p = row; p < row + nrow && w < k; ++p)
      if (!(present && p == self)) o[w++] = *p;
    std::fill(o + w, o + k, VC_PACK_INF);
    counts[i] = w;
    if (stats) stats[i].n_results = w;
  }
}

// ---- k-NN by id over a VcStoreView: the one driver of vc_search_knn_ids* and vc_sharded_search_knn_ids* ----------------------------
#define VC_IDS_HIP(call) VC_HIP_OR_FAIL("k-NN by id", call)

int vc_ids_knn_reserve(const VcStoreView& v, uint32_t nq, uint32_t kp, VcIdsKnnBufs* b) {
  b->d_q = (uint64_t*)v.alloc(VC_KIDS_Q, (size_t)nq * v.W * 8);
  b->d_found = (uint32_t*)v.alloc(VC_KIDS_FOUND, (size_t)nq * 4);
  b->d_rows = (uint64_t*)v.alloc(VC_KIDS_ROWS, (size_t)nq * kp * 8);
  b->d_cnt = (uint32_t*)v.alloc(VC_KIDS_CNT, (size_t)nq * 4);
  return b->d_q && b->d_found && b->d_rows && b->d_cnt ? VC_OK : VC_ERR_NOMEM;
}

int vc_ids_knn_run(const VcStoreView& v, const VcIdsKnnBufs& b, const uint32_t* d_ids, uint32_t nq, uint32_t kp, uint32_t k, uint64_t* d_out, uint32_t* d_counts,
                   vc_query_stats* d_stats, hipStream_t s, std::string* err) {
  int rc;
  if ((rc = v.gather(d_ids, nq, b.d_q, b.d_found))) return rc;
  if ((rc = v.knn(b.d_q, nq, kp, b.d_rows, b.d_cnt, d_stats))) return rc;
  VC_IDS_HIP(vc_launch_ids_strip(d_ids, b.d_found, b.d_rows, b.d_cnt, nq, kp, k, d_out, d_counts, d_stats, s));
  return VC_OK;
}

int vc_ids_knn_run_host(const VcStoreView& v, const VcIdsKnnHostArgs& a,
                        const std::function<int(const VcIdsKnnBufs& b, const uint32_t* d_ids, uint64_t* d_out, uint32_t* d_counts, vc_query_stats* d_stats)>& run,
                        const std::function<int(const uint64_t* codes, uint64_t* rows, uint32_t* counts)>& host_knn, hipStream_t s, std::string* err) {
  const uint32_t nq = a.nq, k = a.k;
  const size_t st_bytes = (size_t)nq * sizeof(vc_query_stats);
  VcIdsKnnBufs b;
  int rc = vc_ids_knn_reserve(v, nq, a.kp, &b);
  if (rc) return rc;
  uint32_t* d_hids = (uint32_t*)v.alloc(VC_KIDS_HIDS, (size_t)nq * 4);
  uint64_t* d_hrows = (uint64_t*)v.alloc(VC_KIDS_HROWS, (size_t)nq * k * 8);
  uint32_t* d_hcnt = (uint32_t*)v.alloc(VC_KIDS_HCNT, (size_t)nq * 4);
  vc_query_stats* d_hstats = a.stats ? (vc_query_stats*)v.alloc(VC_KIDS_HSTATS, st_bytes) : nullptr;
  if (!d_hids || !d_hrows || !d_hcnt || (a.stats && !d_hstats)) return VC_ERR_NOMEM;
  VC_IDS_HIP(hipMemcpyAsync(d_hids, a.ids, (size_t)nq * 4, hipMemcpyHostToDevice, s));
  if ((rc = run(b, d_hids, d_hrows, d_hcnt, d_hstats))) return rc;
  std::vector<uint32_t> cnt(nq);
  VC_IDS_HIP(hipMemcpyAsync(a.out, d_hrows, (size_t)nq * k * 8, hipMemcpyDeviceToHost, s));
  VC_IDS_HIP(hipMemcpyAsync(cnt.data(), d_hcnt, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
  if (a.stats) VC_IDS_HIP(hipMemcpyAsync(a.stats, d_hstats, st_bytes, hipMemcpyDeviceToHost, s));
  VC_IDS_HIP(hipStreamSynchronize(s));
  if (a.linear && std::find(cnt.begin(), cnt.end(), 0xFFFFFFFFu) != cnt.end()) {
    // a ring overflowed and the device-side recovery gave up: the batch is answered again by the handle's host-form k-NN, whose
    // host-driven recovery always ends, on the gathered codes, and stripped here by the kernel's rule
    std::vector<uint64_t> codes((size_t)nq * v.W), rows((size_t)nq * a.kp);
    std::vector<uint32_t> found(nq), rcnt(nq);
    VC_IDS_HIP(hipMemcpyAsync(codes.data(), b.d_q, codes.size() * 8, hipMemcpyDeviceToHost, s));
    VC_IDS_HIP(hipMemcpyAsync(found.data(), b.d_found, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
    VC_IDS_HIP(hipStreamSynchronize(s));
    if ((rc = host_knn(codes.data(), rows.data(), rcnt.data()))) return rc;
    vc_ids_strip_host(a.ids, found.data(), rows.data(), rcnt.data(), nq, a.kp, k, a.out, cnt.data(), a.stats);
  }
  for (uint32_t i = 0; i < nq; ++i) {
    if (!a.linear) cnt[i] = std::min(cnt[i], k);   // (as vc_sharded_search_knn: a flagged MIH row has k entries)
    if (a.order == VC_ORDER_FARTHEST_FIRST) std::reverse(a.out + (size_t)i * k, a.out + (size_t)i * k + cnt[i]);
    if (a.counts) a.counts[i] = cnt[i];
    if (a.stats) a.stats[i].n_results = cnt[i];
  }
  return VC_OK;
}
