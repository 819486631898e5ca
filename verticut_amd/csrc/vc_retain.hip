// ============================================================================
// vc_retain.hip -- removal of records from a built store (vc_retain*): the keep set and the code columns.
//
// Replaces (reference, CPU + KV tier): nothing the reference can do in place -- its store has put and get only
// (base_proxy.h:18-22), and taking records out means running build_hash_tables.cc:40-70 again over a code file without
// them.  Here the survivors are renumbered in order (ids stay ordinals of the records, build_hash_tables.cc:55,61,69):
//   keep set      sel[] -> one bit per record + a rank directory (VcKeepSet, vc_retain.hpp); K = the set bits
//   new_ids       the map old id -> new id, one coalesced pass
//   code columns  a stable compaction of each column through ONE scratch column, positions [K, N) zeroed afterwards
// The index side (a built index filtered to the survivors) is vc_mih_retain in vc_mih.hip.
// ============================================================================
#include <algorithm>

#include "vc_internal.hpp"
#include "vc_retain.hpp"

#define RT_BLK 256u

namespace {

// One ballot per wave of 64 records makes one 64-bit word.  Words [ceil(n / 64), nwords) -- the padding to whole blocks -- and the
// bits behind record n - 1 of the last, partial word come out zero: their lanes vote "no".
__global__ void __launch_bounds__(RT_BLK) retain_bits_kernel(const uint32_t* __restrict__ sel, uint32_t kind, uint32_t id_base, uint64_t first_kept,
                                                             uint64_t n, uint64_t nwords, uint64_t* __restrict__ bits) {
  const uint32_t lane = vc_lane();
  const uint64_t wave = ((uint64_t)blockIdx.x * RT_BLK + threadIdx.x) / VC_WAVE, nwaves = (uint64_t)gridDim.x * (RT_BLK / VC_WAVE);
  for (uint64_t w = wave; w < nwords; w += nwaves) {   // (wave-uniform)
    const uint64_t i = w * VC_WAVE + lane;
    bool keep = false;
    if (i < n) {
      if (kind == VC_RETAIN_MASK) keep = sel[i] != 0u;
      else if (kind == VC_RETAIN_ROOTS) keep = sel[i] == id_base + (uint32_t)i;
      else keep = i >= first_kept;   // VC_RETAIN_FROM (internal): the records from first_kept on, sel unused
    }
    const uint64_t word = __ballot(keep);
    if (lane == 0) bits[w] = word;
  }
}

// set bits per 256-bit block; pop[nblocks] = 0, so that the exclusive scan over nblocks + 1 entries ends in K
__global__ void __launch_bounds__(RT_BLK) retain_blockpop_kernel(const uint64_t* __restrict__ bits, uint64_t nblocks, uint32_t* __restrict__ pop) {
  for (uint64_t b = (uint64_t)blockIdx.x * RT_BLK + threadIdx.x; b <= nblocks; b += (uint64_t)gridDim.x * RT_BLK) {
    uint32_t c = 0;
    if (b < nblocks) {
      const vc_u64x2 lo = reinterpret_cast<const vc_u64x2*>(bits)[2 * b], hi = reinterpret_cast<const vc_u64x2*>(bits)[2 * b + 1];
      c = __popcll(lo.x) + __popcll(lo.y) + __popcll(hi.x) + __popcll(hi.y);
    }
    pop[b] = c;
  }
}

__global__ void __launch_bounds__(RT_BLK) retain_map_kernel(const VcKeepSet ks, uint32_t id_base, uint32_t* __restrict__ new_ids) {
  for (uint64_t i = (uint64_t)blockIdx.x * RT_BLK + threadIdx.x; i < ks.n; i += (uint64_t)gridDim.x * RT_BLK)
    new_ids[i] = vc_keep_test(ks, (uint32_t)i) ? id_base + vc_keep_rank(ks, (uint32_t)i) : 0xFFFFFFFFu;
}

// Stable compaction of one column into the scratch column.  A thread takes the records 2p and 2p + 1: one 16-byte load (column
// bases and even positions are 16-byte aligned; position n of an odd n is zero padding inside the stride), both keep bits from
// one bitmap word, the second survivor right behind the first.  Out of place: a block's output run may overlap input that
// another block has not read yet, so nothing is written to the column before every block is done.
__global__ void __launch_bounds__(RT_BLK) retain_compact_kernel(const VcKeepSet ks, const uint64_t* __restrict__ col, uint64_t* __restrict__ scratch) {
  const uint64_t npairs = (ks.n + 1) / 2;
  for (uint64_t p = (uint64_t)blockIdx.x * RT_BLK + threadIdx.x; p < npairs; p += (uint64_t)gridDim.x * RT_BLK) {
    const uint32_t i = (uint32_t)(2 * p);
    const uint32_t two = (uint32_t)(ks.bits[i >> 6] >> (i & 63u)) & 3u;   // (i & 63 is even: both bits lie in this word)
    if (!two) continue;
    const vc_u64x2 v = *reinterpret_cast<const vc_u64x2*>(col + i);
    const uint32_t r = vc_keep_rank(ks, i);
    if (two & 1u) scratch[r] = v.x;
    if (two & 2u) scratch[r + (two & 1u)] = v.y;
  }
}

// column[0, K) = scratch[0, K), column[K, round_up(n, 2)) = 0: 16-byte stores throughout, 16-byte loads while both words are survivors
__global__ void __launch_bounds__(RT_BLK) retain_writeback_kernel(const uint64_t* __restrict__ scratch, uint64_t k, uint64_t n, uint64_t* __restrict__ col) {
  const uint64_t npairs = (n + 1) / 2;
  for (uint64_t p = (uint64_t)blockIdx.x * RT_BLK + threadIdx.x; p < npairs; p += (uint64_t)gridDim.x * RT_BLK) {
    const uint64_t i = 2 * p;
    vc_u64x2 v = {0ull, 0ull};
    if (i + 1 < k) v = *reinterpret_cast<const vc_u64x2*>(scratch + i);
    else if (i < k) v.x = scratch[i];
    *reinterpret_cast<vc_u64x2*>(col + i) = v;
  }
}

uint32_t rt_grid(uint64_t items, uint32_t n_cu) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + RT_BLK - 1) / RT_BLK, (uint64_t)n_cu * 16)); }

}  // namespace

hipError_t vc_launch_keep_bits(const uint32_t* d_sel, uint32_t kind, uint32_t id_base, uint64_t first_kept, uint64_t n, uint64_t* d_bits, uint32_t* d_rank,
                               uint32_t* d_work, uint32_t n_cu, hipStream_t s) {
  const uint64_t nblocks = vc_keep_blocks(n), nwords = nblocks * VC_KEEP_BLOCK_WORDS;
  hipLaunchKernelGGL(retain_bits_kernel, dim3(rt_grid(nwords * VC_WAVE, n_cu)), dim3(RT_BLK), 0, s, d_sel, kind, id_base, first_kept, n, nwords, d_bits);
  hipError_t r = hipGetLastError();
  if (r != hipSuccess) return r;
  hipLaunchKernelGGL(retain_blockpop_kernel, dim3(rt_grid(nblocks + 1, n_cu)), dim3(RT_BLK), 0, s, (const uint64_t*)d_bits, nblocks, d_rank);
  if ((r = hipGetLastError()) != hipSuccess) return r;
  return vc_exclusive_scan_u32(d_rank, d_rank, nblocks + 1, d_work, s);
}

hipError_t vc_launch_keep_map(const VcKeepSet& ks, uint32_t id_base, uint32_t* d_new_ids, uint32_t n_cu, hipStream_t s) {
  hipLaunchKernelGGL(retain_map_kernel, dim3(rt_grid(ks.n, n_cu)), dim3(RT_BLK), 0, s, ks, id_base, d_new_ids);
  return hipGetLastError();
}

hipError_t vc_launch_keep_compact_column(const VcKeepSet& ks, uint64_t* d_col, uint64_t* d_scratch, uint32_t n_cu, hipStream_t s) {
  const uint32_t grid = rt_grid((ks.n + 1) / 2, n_cu);
  hipLaunchKernelGGL(retain_compact_kernel, dim3(grid), dim3(RT_BLK), 0, s, ks, (const uint64_t*)d_col, d_scratch);
  hipError_t r = hipGetLastError();
  if (r != hipSuccess) return r;
  hipLaunchKernelGGL(retain_writeback_kernel, dim3(grid), dim3(RT_BLK), 0, s, (const uint64_t*)d_scratch, ks.k, ks.n, d_col);
  return hipGetLastError();
}
