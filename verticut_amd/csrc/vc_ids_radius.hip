// ============================================================================
// vc_ids_radius.hip -- radius search for queries named by id (vc_search_radius_ids*, vc_sharded_search_radius_ids*): the stable,
// segment-wise compaction of the variable-length result of the radius search underneath.  A translation unit of its own: unlike
// the kernels of vc_ids.hip these use LDS (the waves' sums of a block-level prefix).
// ============================================================================
#include <algorithm>

#include "vc_internal.hpp"

// The radius search underneath leaves `raw` (ascending packed per query) and its nq + 1 offsets `roffs`.  An entry of query q is KEPT
// when the id is resident (found[q]), and it is not the query's own entry (distance 0, own id: VC_IDS_EXCLUDE_SELF, matched by value),
// and its id exceeds the query's own (VC_IDS_ONLY_GREATER).  The work is cut into (query, chunk) ITEMS of VC_IDS_RCHUNK entries, so a
// long segment spreads over many blocks; item j belongs to the query q with cs[q] <= j < cs[q + 1] (cs: the chunk starts).
//   vc_ids_radius_plan_kernel        cs[0 .. nq]: exclusive sums of the queries' chunk counts (none for an id that is not resident)
//   vc_ids_radius_count_kernel       kept entries of every item -> chunk_cnt[j]
//   vc_ids_radius_chunk_scan_kernel  per query: chunk_base[j] = kept entries of the query's earlier chunks, qsum[q] = its kept entries
//   vc_ids_radius_offsets_kernel     d_offsets[0 .. nq]: exclusive sums of qsum, the compacted total also in *total
//   vc_ids_radius_copy_kernel        item j writes its kept entries, in order, to out[offsets[q] + chunk_base[j] ..)
// LDS holds only the waves' sums of a block-level prefix.
#define IDS_RBLK 256u                                   // threads of the count / copy blocks
#define IDS_RITER (VC_IDS_RCHUNK / IDS_RBLK)            // entries per thread and item
#define IDS_RWAVES (IDS_RBLK / VC_WAVE)
static_assert(VC_IDS_RCHUNK % IDS_RBLK == 0 && IDS_RBLK % VC_WAVE == 0, "a chunk is whole passes of a block of whole waves");

__device__ __forceinline__ bool ids_radius_keep(uint64_t v, uint32_t own, uint32_t flags) {
  return !((flags & VC_IDS_EXCLUDE_SELF) && v == (uint64_t)own) && !((flags & VC_IDS_ONLY_GREATER) && (uint32_t)v <= own);
}

// the query of item j: the last q with cs[q] <= j (queries without chunks share their successor's start and are passed over)
__device__ __forceinline__ uint32_t ids_radius_query_of(const uint32_t* __restrict__ cs, uint32_t nq, uint32_t j) {
  uint32_t lo = 0, hi = nq;   // cs[lo] <= j < cs[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (cs[mid] <= j) lo = mid; else hi = mid;
  }
  return lo;
}

// Exclusive prefix sum of one value per thread over a block of 1024; *total = the block's sum.  The wave scan runs in two 32-bit halves
// (the value's low 24 bits and the 8 above them: the sums of 64 lanes of either stay below 2^32); s_w: one word per wave.
__device__ __forceinline__ uint64_t ids_block_excl_scan(uint32_t v, uint64_t* s_w, uint64_t* total) {
  const uint32_t lane = vc_lane(), wave = threadIdx.x / VC_WAVE;
  uint32_t tlo, thi;
  const uint32_t xlo = vc_wave_excl_scan(v & 0xFFFFFFu, tlo), xhi = vc_wave_excl_scan(v >> 24, thi);
  __syncthreads();   // (s_w of the previous tile has been read)
  if (lane == 0) s_w[wave] = (uint64_t)tlo + ((uint64_t)thi << 24);
  __syncthreads();
  uint64_t base = 0, sum = 0;
  for (uint32_t w = 0; w < 1024 / VC_WAVE; ++w) {
    if (w < wave) base += s_w[w];
    sum += s_w[w];
  }
  *total = sum;
  return base + xlo + ((uint64_t)xhi << 24);
}

__global__ void __launch_bounds__(1024) vc_ids_radius_plan_kernel(const uint64_t* __restrict__ roffs, const uint32_t* __restrict__ found, uint32_t nq,
                                                                  uint32_t* __restrict__ cs) {
  __shared__ uint64_t s_w[1024 / VC_WAVE];
  uint64_t carry = 0;
  for (uint32_t q0 = 0; q0 < nq; q0 += 1024) {   // (block-uniform bounds: every lane scans)
    const uint32_t q = q0 + threadIdx.x;
    uint32_t c = 0;
    if (q < nq && found[q]) c = (uint32_t)((roffs[q + 1] - roffs[q] + VC_IDS_RCHUNK - 1) / VC_IDS_RCHUNK);
    uint64_t tile;
    const uint64_t ex = ids_block_excl_scan(c, s_w, &tile);
    if (q < nq) cs[q] = (uint32_t)(carry + ex);
    carry += tile;
  }
  if (threadIdx.x == 0) cs[nq] = (uint32_t)carry;   // (the host has checked that the items fit 32 bits)
}

__global__ void __launch_bounds__(IDS_RBLK) vc_ids_radius_count_kernel(const uint64_t* __restrict__ raw, const uint64_t* __restrict__ roffs,
                                                                       const uint32_t* __restrict__ ids, const uint32_t* __restrict__ cs, uint32_t nq,
                                                                       uint32_t flags, uint32_t* __restrict__ chunk_cnt) {
  __shared__ uint32_t s_w[IDS_RWAVES];
  const uint32_t lane = vc_lane(), wave = threadIdx.x / VC_WAVE, items = cs[nq];
  for (uint32_t j = blockIdx.x; j < items; j += gridDim.x) {
    const uint32_t q = ids_radius_query_of(cs, nq, j), own = ids[q];
    const uint64_t beg = roffs[q] + (uint64_t)(j - cs[q]) * VC_IDS_RCHUNK, end = roffs[q + 1];
    uint32_t kept = 0;
#pragma unroll
    for (uint32_t it = 0; it < IDS_RITER; ++it) {
      const uint64_t p = beg + it * IDS_RBLK + threadIdx.x;
      kept += (uint32_t)__popcll(__ballot(p < end && ids_radius_keep(raw[p < end ? p : beg], own, flags)));
    }
    if (lane == 0) s_w[wave] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t sum = 0;
      for (uint32_t w = 0; w < IDS_RWAVES; ++w) sum += s_w[w];
      chunk_cnt[j] = sum;
    }
    __syncthreads();
  }
}

// one wave per query walks the query's chunk counts 64 at a time
__global__ void __launch_bounds__(IDS_RBLK) vc_ids_radius_chunk_scan_kernel(const uint32_t* __restrict__ cs, const uint32_t* __restrict__ chunk_cnt,
                                                                            uint32_t nq, uint32_t* __restrict__ chunk_base, uint32_t* __restrict__ qsum) {
  const uint32_t lane = vc_lane();
  for (uint32_t q = blockIdx.x * IDS_RWAVES + threadIdx.x / VC_WAVE; q < nq; q += gridDim.x * IDS_RWAVES) {   // (wave-uniform)
    const uint32_t c0 = cs[q], c1 = cs[q + 1];
    uint32_t carry = 0;   // (a query's entries fit 32 bits: the radius search counts them in a uint32)
    for (uint32_t c = c0; c < c1; c += VC_WAVE) {
      const uint32_t j = c + lane, v = j < c1 ? chunk_cnt[j] : 0u;
      uint32_t tot;
      const uint32_t ex = vc_wave_excl_scan(v, tot);
      if (j < c1) chunk_base[j] = carry + ex;
      carry += tot;
    }
    if (lane == 0) qsum[q] = carry;
  }
}

__global__ void __launch_bounds__(1024) vc_ids_radius_offsets_kernel(const uint32_t* __restrict__ qsum, uint32_t nq, uint64_t* __restrict__ offsets,
                                                                     uint64_t* __restrict__ total) {
  __shared__ uint64_t s_w[1024 / VC_WAVE];
  uint64_t carry = 0;
  for (uint32_t q0 = 0; q0 < nq; q0 += 1024) {
    const uint32_t q = q0 + threadIdx.x;
    uint64_t tile;
    const uint64_t ex = ids_block_excl_scan(q < nq ? qsum[q] : 0u, s_w, &tile);
    if (q < nq) offsets[q] = carry + ex;
    carry += tile;
  }
  if (threadIdx.x == 0) {
    offsets[nq] = carry;
    *total = carry;
  }
}

// Order inside an item: the rank of a kept entry is the kept entries of the earlier passes and of the pass's earlier waves (LDS)
// plus those of the lower lanes of its wave (ballot prefix) -- the entries leave in the order they lie in, the compaction is stable.
__global__ void __launch_bounds__(IDS_RBLK) vc_ids_radius_copy_kernel(const uint64_t* __restrict__ raw, const uint64_t* __restrict__ roffs,
                                                                      const uint32_t* __restrict__ ids, const uint32_t* __restrict__ cs, uint32_t nq,
                                                                      uint32_t flags, const uint32_t* __restrict__ chunk_base,
                                                                      const uint64_t* __restrict__ offsets, uint64_t* __restrict__ out) {
  __shared__ uint32_t s_w[IDS_RITER * IDS_RWAVES];
  const uint32_t lane = vc_lane(), wave = threadIdx.x / VC_WAVE, items = cs[nq];
  for (uint32_t j = blockIdx.x; j < items; j += gridDim.x) {
    const uint32_t q = ids_radius_query_of(cs, nq, j), own = ids[q];
    const uint64_t beg = roffs[q] + (uint64_t)(j - cs[q]) * VC_IDS_RCHUNK, end = roffs[q + 1];
    uint64_t v[IDS_RITER], km[IDS_RITER];
#pragma unroll
    for (uint32_t it = 0; it < IDS_RITER; ++it) {
      const uint64_t p = beg + it * IDS_RBLK + threadIdx.x;
      v[it] = raw[p < end ? p : beg];
      km[it] = __ballot(p < end && ids_radius_keep(v[it], own, flags));
      if (lane == 0) s_w[it * IDS_RWAVES + wave] = (uint32_t)__popcll(km[it]);
    }
    __syncthreads();
    uint64_t* dst = out + offsets[q] + chunk_base[j];
    uint32_t before = 0;   // kept entries of the passes and waves ahead of this wave's pass `it`
#pragma unroll
    for (uint32_t it = 0; it < IDS_RITER; ++it) {
      for (uint32_t w = 0; w < IDS_RWAVES; ++w)
        if (w < wave) before += s_w[it * IDS_RWAVES + w];
      if (km[it] >> lane & 1) dst[before + (uint32_t)__popcll(km[it] & ((1ull << lane) - 1ull))] = v[it];
      for (uint32_t w = 0; w < IDS_RWAVES; ++w)
        if (w >= wave) before += s_w[it * IDS_RWAVES + w];
    }
    __syncthreads();
  }
}

static uint32_t ids_radius_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(items, 1), 256 * 32); }

hipError_t vc_launch_ids_radius_count(const VcIdsRadiusWork& w, const uint64_t* d_raw, const uint64_t* d_roffs, const uint32_t* d_ids,
                                      const uint32_t* d_found, uint32_t nq, uint32_t id_flags, uint64_t* d_offsets, hipStream_t s) {
  hipLaunchKernelGGL(vc_ids_radius_plan_kernel, dim3(1), dim3(1024), 0, s, d_roffs, d_found, nq, w.cs);
  hipLaunchKernelGGL(vc_ids_radius_count_kernel, dim3(ids_radius_grid(w.items)), dim3(IDS_RBLK), 0, s, d_raw, d_roffs, d_ids, w.cs, nq, id_flags,
                     w.chunk_cnt);
  hipLaunchKernelGGL(vc_ids_radius_chunk_scan_kernel, dim3(ids_radius_grid(((uint64_t)nq + IDS_RWAVES - 1) / IDS_RWAVES)), dim3(IDS_RBLK), 0, s, w.cs,
                     w.chunk_cnt, nq, w.chunk_base, w.qsum);
  hipLaunchKernelGGL(vc_ids_radius_offsets_kernel, dim3(1), dim3(1024), 0, s, w.qsum, nq, d_offsets, w.total);
  return hipGetLastError();
}

hipError_t vc_launch_ids_radius_copy(const VcIdsRadiusWork& w, const uint64_t* d_raw, const uint64_t* d_roffs, const uint32_t* d_ids, uint32_t nq,
                                     uint32_t id_flags, const uint64_t* d_offsets, uint64_t* d_out, hipStream_t s) {
  hipLaunchKernelGGL(vc_ids_radius_copy_kernel, dim3(ids_radius_grid(w.items)), dim3(IDS_RBLK), 0, s, d_raw, d_roffs, d_ids, w.cs, nq, id_flags,
                     w.chunk_base, d_offsets, d_out);
  return hipGetLastError();
}

// ---- radius search by id over a VcStoreView: the one driver of vc_search_radius_ids* and vc_sharded_search_radius_ids* ------------
#define VC_RIDS_HIP(call) VC_HIP_OR_FAIL("radius search by id", call)

int vc_ids_radius_run(const VcStoreView& v, const uint32_t* d_ids, uint32_t nq, uint32_t radius, uint32_t id_flags, uint64_t* d_out, uint64_t out_cap,
                      uint64_t* d_offsets, hipStream_t s, std::string* err) {
  uint64_t* d_q = (uint64_t*)v.alloc(VC_RIDS_Q, (size_t)nq * v.W * 8);
  uint32_t* d_found = (uint32_t*)v.alloc(VC_RIDS_FOUND, (size_t)nq * 4);
  uint64_t* d_roffs = (uint64_t*)v.alloc(VC_RIDS_ROFFS, ((size_t)nq + 1) * 8);
  uint64_t* d_raw = (uint64_t*)v.alloc(VC_RIDS_RAW, VC_RAW_FIRST_BYTES);
  if (!d_q || !d_found || !d_roffs || !d_raw) return VC_ERR_NOMEM;
  int rc;
  if ((rc = v.gather(d_ids, nq, d_q, d_found))) return rc;
  uint64_t raw_total;
  if ((rc = vc_search_raw(v, VC_RIDS_RAW, d_q, nq, radius, &d_raw, d_roffs, &raw_total))) return rc;
  const uint64_t items = vc_ids_radius_items(nq, raw_total);
  if (items > 0xFFFFFFFFull) {
    *err = "radius search by id: more results than one compaction can place";
    return VC_ERR_CAPACITY;
  }
  void* d_work = v.alloc(VC_RIDS_WORK, VcIdsRadiusWork::bytes(nq, items));
  if (!d_work) return VC_ERR_NOMEM;
  const VcIdsRadiusWork w(d_work, nq, items);
  VC_RIDS_HIP(vc_launch_ids_radius_count(w, d_raw, d_roffs, d_ids, d_found, nq, id_flags, d_offsets, s));
  if (raw_total > out_cap) {   // T <= raw_total: only then the host has to learn T
    uint64_t T = 0;
    VC_RIDS_HIP(hipMemcpyAsync(&T, w.total, 8, hipMemcpyDeviceToHost, s));
    VC_RIDS_HIP(hipStreamSynchronize(s));
    if (T > out_cap) {
      *err = "radius search: output buffer too small (needed counts are in the offsets)";
      return VC_ERR_CAPACITY;
    }
  }
  if (d_out && raw_total) VC_RIDS_HIP(vc_launch_ids_radius_copy(w, d_raw, d_roffs, d_ids, nq, id_flags, d_offsets, d_out, s));
  return VC_OK;
}

int vc_ids_radius_run_host(const VcStoreView& v, const uint32_t* ids, uint32_t nq, uint64_t* out, uint64_t out_cap, uint64_t* out_offsets,
                           const std::function<int(const uint32_t* d_ids, uint64_t* d_out, uint64_t* d_offsets)>& run, hipStream_t s, std::string* err) {
  uint32_t* d_ids = (uint32_t*)v.alloc(VC_RIDS_HIDS, (size_t)nq * 4);
  uint64_t* d_offsets = (uint64_t*)v.alloc(VC_RIDS_HOFFS, ((size_t)nq + 1) * 8);
  uint64_t* d_out = (uint64_t*)v.alloc(VC_RIDS_HOUT, (size_t)out_cap * 8);
  if (!d_ids || !d_offsets || (out_cap && !d_out)) return VC_ERR_NOMEM;
  VC_RIDS_HIP(hipMemcpyAsync(d_ids, ids, (size_t)nq * 4, hipMemcpyHostToDevice, s));
  const int rc = run(d_ids, out_cap ? d_out : nullptr, d_offsets);
  if (rc != VC_OK && rc != VC_ERR_CAPACITY) return rc;
  // the offsets come home in both cases (VC_ERR_CAPACITY: they are the needed counts); the staged results behind them
  VC_RIDS_HIP(hipMemcpyAsync(out_offsets, d_offsets, ((size_t)nq + 1) * 8, hipMemcpyDeviceToHost, s));
  VC_RIDS_HIP(hipStreamSynchronize(s));
  if (rc == VC_OK && out_offsets[nq]) {
    VC_RIDS_HIP(hipMemcpyAsync(out, d_out, (size_t)out_offsets[nq] * 8, hipMemcpyDeviceToHost, s));
    VC_RIDS_HIP(hipStreamSynchronize(s));
  }
  return rc;
}
