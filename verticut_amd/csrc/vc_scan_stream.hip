// ============================================================================
// vc_scan_stream.hip -- builder of the prefix-sorted 96-bit scan stream of a 128-bit store.   gfx950 only.
//
// One-off per store state (the database is constant between ingest and serving): the records' key words (the low 32 bits of
// code word 0) are radix-sorted with their local ids (vc_sort.hip, stable, as the MIH table build does), the other 96 bits are
// gathered into three uint32 columns in that order, and every granule of 256 sorted records gets the key bits its first and
// last key share.  Layout, header arithmetic and the memory rule: vc_scan_stream_plan.hpp; the reader: vc_scan_kernel_stream
// (vc_scan.hip).
// ============================================================================
#include <algorithm>

#include "vc_internal.hpp"

namespace {

// keys[i] = key word of local record i, ids[i] = i
__global__ void __launch_bounds__(256) vc_stream_keys_kernel(const uint64_t* __restrict__ col0, uint64_t n, uint32_t* __restrict__ keys,
                                                             uint32_t* __restrict__ ids) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    keys[i] = (uint32_t)col0[i];
    ids[i] = (uint32_t)i;
  }
}

// sorted position p < n: the other three words of record perm[p]; n <= p < n_pad: zeros in all four columns and perm
__global__ void __launch_bounds__(256) vc_stream_gather_kernel(const uint64_t* __restrict__ cols, uint64_t stride, uint64_t n, uint64_t n_pad,
                                                               uint32_t* __restrict__ perm, uint32_t* __restrict__ key, uint32_t* __restrict__ t0,
                                                               uint32_t* __restrict__ t1, uint32_t* __restrict__ t2) {
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pad; p += (uint64_t)gridDim.x * blockDim.x) {
    if (p < n) {
      const uint32_t id = perm[p];
      const uint64_t w0 = cols[id], w1 = cols[stride + id];
      t0[p] = (uint32_t)(w0 >> 32);
      t1[p] = (uint32_t)w1;
      t2[p] = (uint32_t)(w1 >> 32);
    } else {
      perm[p] = 0;
      key[p] = 0;
      t0[p] = 0;
      t1[p] = 0;
      t2[p] = 0;
    }
  }
}

// hdr[g] = the shared leading bits of granule g's first and last resident key; a granule of padding only gets {0, 0}
__global__ void __launch_bounds__(256) vc_stream_header_kernel(const uint32_t* __restrict__ key, uint64_t n, uint64_t granules,
                                                               uint32_t* __restrict__ hdr) {
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < granules; g += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t first = g * VC_STREAM_GRANULE;
    VcStreamHeader h{0, 0};
    const uint64_t end = first + VC_STREAM_GRANULE < n ? first + VC_STREAM_GRANULE : n;
    if (first < n) h = vc_stream_header(key[first], key[end - 1]);
    hdr[2 * g] = h.prefix;
    hdr[2 * g + 1] = h.mask;
  }
}

uint32_t grid_for(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + 255) / 256, 1), 256 * 32); }

}  // namespace

void vc_scan_stream_free(VcScanStream* st) {
  if (st->d_base) (void)hipFree(st->d_base);
  if (st->d_diag) (void)hipFree(st->d_diag);
  *st = VcScanStream{};
}

hipError_t vc_scan_stream_build(const uint64_t* cols, uint64_t stride, uint64_t n, bool have_free, uint64_t free_bytes, VcScanStream* out,
                                hipStream_t s) {
  if (!out || out->built() || n > 0xFFFFFFFFull) return hipErrorInvalidValue;
  const size_t work_words = vc_radix_sort_work_words(n);
  const VcStreamPlan plan = vc_stream_plan(n, work_words);
  if (!vc_stream_fits(plan, have_free, free_bytes)) return hipErrorOutOfMemory;
  VcScanStream st;
  st.plan = plan;
  uint32_t *k1 = nullptr, *v1 = nullptr, *work = nullptr;
  hipError_t r = hipMalloc((void**)&st.d_base, std::max<uint64_t>(plan.bytes, 256));
  if (r != hipSuccess) st.d_base = nullptr;
  if (r == hipSuccess) r = hipMalloc((void**)&st.d_diag, 256);
  if (r == hipSuccess) r = hipMemsetAsync(st.d_diag, 0, 256, s);
  if (r == hipSuccess && n) {
    r = hipMalloc((void**)&k1, n * 4);
    if (r == hipSuccess) r = hipMalloc((void**)&v1, n * 4);
    if (r == hipSuccess) r = hipMalloc((void**)&work, std::max<size_t>(work_words, 1) * 4);
  }
  if (r == hipSuccess && n) {
    uint32_t* const key = st.d_base + plan.key;
    uint32_t* const t0 = st.d_base + plan.t0;
    uint32_t* const perm = st.d_base + plan.perm;
    // the sort's first buffer pair IS the stream's key column and perm[]: 32 key bits are four passes, so the result lands there
    uint32_t* keys[2] = {key, k1};
    uint32_t* vals[2] = {perm, v1};
    hipLaunchKernelGGL(vc_stream_keys_kernel, dim3(grid_for(n)), dim3(256), 0, s, cols, n, key, perm);
    r = hipGetLastError();
    if (r == hipSuccess) r = vc_radix_sort_pairs(keys, vals, n, 32, work, s);
    if (r == hipSuccess && (vc_radix_sort_passes(32) & 1) != 0) r = hipErrorInvalidValue;   // (the result must be in pair 0)
    if (r == hipSuccess) {
      hipLaunchKernelGGL(vc_stream_gather_kernel, dim3(grid_for(plan.n_pad)), dim3(256), 0, s, cols, stride, n, plan.n_pad, perm, key, t0,
                         t0 + plan.stride, t0 + 2 * plan.stride);
      hipLaunchKernelGGL(vc_stream_header_kernel, dim3(grid_for(plan.granules)), dim3(256), 0, s, key, n, plan.granules, st.d_base + plan.hdr);
      r = hipGetLastError();
    }
  }
  const hipError_t rs = hipStreamSynchronize(s);   // the temporaries go, and the caller may search on any stream afterwards
  if (r == hipSuccess) r = rs;
  (void)hipFree(k1);
  (void)hipFree(v1);
  (void)hipFree(work);
  if (r != hipSuccess) {
    vc_scan_stream_free(&st);
    return r;
  }
  *out = st;
  return hipSuccess;
}
