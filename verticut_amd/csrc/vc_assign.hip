// ============================================================================
// vc_assign.hip -- nearest of K given codes for a range of resident records (vc_assign_nearest*, vc_sharded_assign_nearest*) and
// Lloyd iterations in Hamming space on top of it (vc_kmajority*, vc_sharded_kmajority*).  One kernel set and one round driver for
// both handle kinds: the handle says how "assign every record" runs (VcAssignAll) and how codes are fetched by id (VcGroupsFetch);
// the update step is vc_groups_run itself, unchanged.  The plan arithmetic is vc_assign_plan.hpp.
// ============================================================================
#include <algorithm>

#include "vc_assign_plan.hpp"
#include "vc_internal.hpp"

// THE RULE of the assign step: out[j] = c | dist << 32 with c the centre of the smallest (Hamming distance, index) for record
// first + j -- the project's packed result with the centre's index in the id field, so the minimum of packed values IS the rule.
// DATA FLOW, the transpose of the verify kernel's: a thread loads R records x W words from the column-major store once (lane l of a
// wave reads word l of 64 consecutive ones: coalesced) and keeps them in VGPRs; the centres stream past in LDS tiles of `tile`
// centres that the block stages together.  In the inner loop every lane reads the SAME LDS address -- a broadcast, no bank
// conflict -- so one ds_read feeds R pair-words per lane, each two XORs and two v_bcnt_u32_b32 with the accumulator operand.
// Centres are visited in ascending index and a strict < keeps the earlier one: the tie rule.  A slice (blockIdx.y) takes a
// contiguous range of the centres; with more than one slice the results meet in a 64-bit atomicMin on `out`, which an init launch
// has set to all ones -- still exact, for the reason above.  One slice: a plain store, no init launch.
// No address is ever formed from data: centre indices are loop counters, record indices come from the grid.
#define KM_BLK 256u
// the counters of a vc_kmajority* call, 64-bit words: [2 t], [2 t + 1] = cost and changed of round t; [128] = cost_final, [129] = n_empty
// (km_block_add2 names two words: one more keeps the second of the n_empty launch, never written, inside the array)
#define KM_STAT_WORDS (2 * VC_KMAJ_MAX_ITERS + 3)

namespace {

template <int W, int R>
__global__ void __launch_bounds__(VC_ASSIGN_BLOCK) vc_assign_kernel(const uint64_t* __restrict__ cols, uint64_t stride, uint64_t first, uint64_t count,
                                                                     const uint64_t* __restrict__ centres, uint32_t K, uint32_t tile, uint32_t per_slice,
                                                                     uint32_t slices, unsigned long long* __restrict__ out) {
  static_assert(R == (int)vc_assign_records(W), "the plan's records per thread");
  __shared__ uint64_t lds[VC_ASSIGN_LDS_WORDS];
  uint64_t rec[R][W];
  uint32_t bd[R], bi[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint64_t i = vc_assign_record_of(W, blockIdx.x, threadIdx.x, r);
#pragma unroll
    for (int w = 0; w < W; ++w) rec[r][w] = i < count ? cols[(uint64_t)w * stride + first + i] : 0ull;
    bd[r] = 0xFFFFFFFFu;
    bi[r] = 0xFFFFFFFFu;
  }
  const uint64_t c_lo = vc_assign_slice_lo(per_slice, blockIdx.y), c_hi = vc_assign_slice_hi(per_slice, K, blockIdx.y);
  for (uint64_t t0 = c_lo; t0 < c_hi; t0 += tile) {
    const uint32_t nt = vc_assign_tile_centres(t0, c_hi, tile);
    __syncthreads();   // (the previous tile has been read by every wave)
    for (uint32_t j = threadIdx.x; j < nt * (uint32_t)W; j += VC_ASSIGN_BLOCK) lds[j] = centres[t0 * W + j];
    __syncthreads();
#pragma unroll 2
    for (uint32_t c = 0; c < nt; ++c) {
      uint64_t cw[W];
#pragma unroll
      for (int w = 0; w < W; ++w) cw[w] = lds[c * W + w];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        uint32_t d = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) d += (uint32_t)__builtin_popcountll(rec[r][w] ^ cw[w]);
        if (d < bd[r]) {
          bd[r] = d;
          bi[r] = (uint32_t)t0 + c;
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint64_t i = vc_assign_record_of(W, blockIdx.x, threadIdx.x, r);
    if (i >= count) continue;
    const unsigned long long v = vc_pack(bd[r], bi[r]);
    if (slices > 1) atomicMin(out + i, v);
    else out[i] = v;
  }
}

// out[0 .. count) = all ones: what the slices' atomicMin starts from
__global__ void __launch_bounds__(KM_BLK) vc_assign_init_kernel(uint64_t* __restrict__ out, uint64_t count) {
  for (uint64_t i = (uint64_t)blockIdx.x * KM_BLK + threadIdx.x; i < count; i += (uint64_t)gridDim.x * KM_BLK) out[i] = VC_PACK_INF;
}

// dst[0] += the block's sum of a, dst[1] += of b: wave sums on the DPP path, the four of a block meet in LDS, one 64-bit atomic per
// counter and block.  Every thread of the block calls it; a and b are small enough that a wave's sum fits 32 bits.
__device__ __forceinline__ void km_block_add2(uint32_t a, uint32_t b, unsigned long long* dst) {
  __shared__ uint32_t part[2][KM_BLK / VC_WAVE];
  const uint32_t sa = vc_wave_incl_scan(a), sb = vc_wave_incl_scan(b);
  if (vc_lane() == VC_WAVE - 1) {
    part[0][threadIdx.x / VC_WAVE] = sa;
    part[1][threadIdx.x / VC_WAVE] = sb;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long ta = 0, tb = 0;
    for (uint32_t w = 0; w < KM_BLK / VC_WAVE; ++w) {
      ta += part[0][w];
      tb += part[1][w];
    }
    if (ta) atomicAdd(dst, ta);
    if (tb) atomicAdd(dst + 1, tb);
  }
}

// One round's bookkeeping over the packed assignment: labels[i] = id_base + index, stat[0] += the distances, stat[1] += the records
// whose index differs from prev[i] (first: every record counts), prev[i] = index, flags[index] = 1.  prev and flags may be null.
// An index is < K by construction (vc_assign_kernel's loop counter); it is range-checked all the same before flags is addressed.
__global__ void __launch_bounds__(KM_BLK) vc_kmaj_round_kernel(const uint64_t* __restrict__ assign, uint64_t n, uint32_t id_base, uint32_t K,
                                                               uint32_t* __restrict__ prev, uint32_t first, uint32_t* __restrict__ labels,
                                                               uint32_t* __restrict__ flags, unsigned long long* __restrict__ stat) {
  uint32_t cost = 0, changed = 0;   // (at most 2^32 / (4096 * 256) records per thread, 512 each)
  for (uint64_t i = (uint64_t)blockIdx.x * KM_BLK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * KM_BLK) {
    const uint64_t a = assign[i];
    const uint32_t idx = (uint32_t)a;
    cost += (uint32_t)(a >> 32);
    labels[i] = id_base + idx;
    if (prev) {
      changed += first || prev[i] != idx ? 1u : 0u;
      prev[i] = idx;
    }
    if (flags && idx < K) flags[idx] = 1u;
  }
  km_block_add2(cost, changed, stat);
}

// centroid row g of the update step's groups becomes centre groups[g].label - id_base; a centre without a member has no group and
// keeps its code.  The labels are id_base + index with index < K; an index outside is skipped, never addressed.
__global__ void __launch_bounds__(KM_BLK) vc_kmaj_scatter_kernel(const vc_group* __restrict__ groups, const uint64_t* __restrict__ centroids, uint64_t G, uint32_t W,
                                                                 uint32_t id_base, uint32_t K, uint64_t* __restrict__ centres) {
  for (uint64_t j = (uint64_t)blockIdx.x * KM_BLK + threadIdx.x; j < G * W; j += (uint64_t)gridDim.x * KM_BLK) {
    const uint64_t g = j / W, w = j % W;
    const uint32_t c = groups[g].label - id_base;
    if (c < K) centres[(uint64_t)c * W + w] = centroids[j];
  }
}

// stat[0] += the centres whose flag is still 0
__global__ void __launch_bounds__(KM_BLK) vc_kmaj_empty_kernel(const uint32_t* __restrict__ flags, uint32_t K, unsigned long long* __restrict__ stat) {
  uint32_t empty = 0;
  for (uint64_t c = (uint64_t)blockIdx.x * KM_BLK + threadIdx.x; c < K; c += (uint64_t)gridDim.x * KM_BLK) empty += flags[c] == 0u;
  km_block_add2(empty, 0u, stat);
}

uint32_t km_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + KM_BLK - 1) / KM_BLK, 1), 4096); }

int km_fail(std::string* err, hipError_t r, const char* what) {
  if (err) *err = std::string("assign: ") + what + ": " + hipGetErrorString(r);
  return r == hipErrorOutOfMemory ? VC_ERR_NOMEM : VC_ERR_HIP;
}
#define KM_HIP(call)                                       \
  do {                                                     \
    hipError_t _r = (call);                                \
    if (_r != hipSuccess) return km_fail(err, _r, #call);  \
  } while (0)

template <int W>
void launch_assign(const VcAssignPlan& p, const uint64_t* cols, uint64_t stride, uint64_t first, uint64_t count, const uint64_t* d_centres, uint32_t K,
                   uint64_t* d_out, hipStream_t s) {
  hipLaunchKernelGGL((vc_assign_kernel<W, (int)vc_assign_records(W)>), dim3((uint32_t)p.blocks, p.slices), dim3(VC_ASSIGN_BLOCK), 0, s, cols, stride, first, count,
                     d_centres, K, p.tile, p.per_slice, p.slices, (unsigned long long*)d_out);
}

// the scratch of a vc_kmajority* call behind the caller's outputs, in bytes; every word is written before it is read
struct KmWork {
  uint64_t prev, labels, groups, cents, flags, stat, total;
  KmWork(uint64_t n, uint32_t K, uint32_t W) {
    const uint64_t words = ((n * 4 + 7) & ~7ull);
    uint64_t o = 0;
    prev = o;    o += words;
    labels = o;  o += words;
    groups = o;  o += (uint64_t)K * sizeof(vc_group);
    cents = o;   o += (uint64_t)K * W * 8;
    flags = o;   o += ((uint64_t)K * 4 + 7) & ~7ull;
    stat = o;    o += KM_STAT_WORDS * 8;
    total = o;
  }
};

}  // namespace

hipError_t vc_launch_assign(const uint64_t* cols, uint64_t stride, uint32_t W, uint64_t first, uint64_t count, const uint64_t* d_centres, uint32_t K,
                            uint64_t* d_out, uint32_t n_cu, const VcKnobs* knobs, hipStream_t s) {
  if (count == 0) return hipSuccess;
  const VcAssignPlan p = vc_assign_plan(count, K, W, n_cu, knobs ? knobs->assign_tile : 0, knobs ? knobs->assign_slices : 0);
  if (K == 0 || p.blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  if (p.slices > 1) hipLaunchKernelGGL(vc_assign_init_kernel, dim3(km_grid(count)), dim3(KM_BLK), 0, s, d_out, count);
  switch (W) {
    case 1: launch_assign<1>(p, cols, stride, first, count, d_centres, K, d_out, s); break;
    case 2: launch_assign<2>(p, cols, stride, first, count, d_centres, K, d_out, s); break;
    case 4: launch_assign<4>(p, cols, stride, first, count, d_centres, K, d_out, s); break;
    case 8: launch_assign<8>(p, cols, stride, first, count, d_centres, K, d_out, s); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

int vc_assign_run_host(const std::function<void*(int which, size_t bytes)>& alloc, uint32_t W, const void* centres, uint32_t K, uint64_t count, uint64_t* out,
                       const VcAssignAll& run, hipStream_t s, std::string* err) {
  const size_t cbytes = (size_t)K * W * 8;
  uint8_t* stage = (uint8_t*)alloc(VC_KMAJ_STAGE, cbytes + (size_t)count * 8);
  if (!stage) return VC_ERR_NOMEM;
  uint64_t* d_out = (uint64_t*)(stage + cbytes);
  KM_HIP(hipMemcpyAsync(stage, centres, cbytes, hipMemcpyHostToDevice, s));
  const int rc = run((const uint64_t*)stage, d_out);
  if (rc) return rc;
  KM_HIP(hipMemcpyAsync(out, d_out, (size_t)count * 8, hipMemcpyDeviceToHost, s));
  KM_HIP(hipStreamSynchronize(s));
  return VC_OK;
}

// THE ROUNDS (the header states the rule).  Per round: the handle's assign over all records, one bookkeeping launch, 16 bytes home
// (cost, changed) -- the round's one wait; unless nothing changed, the update: vc_groups_run on labels = id_base + index with
// groups_cap = K (its one wait), and the scatter of its centroid rows into the centres.  At the end always one more assign, whose
// bookkeeping launch also marks the centres that have a member, and the count of those that have none.
int vc_kmajority_run(const VcKmajArgs& k, VcGroupsArgs g, const VcAssignAll& assign_all, const VcGroupsFetch& fetch, vc_kmajority_stats* stats, hipStream_t s,
                     std::string* err) {
  const uint64_t n = g.n;
  const uint32_t K = k.n_centres;
  vc_kmajority_stats st{};
  if (stats) *stats = st;
  if (n == 0) return VC_OK;
  const KmWork wp(n, K, g.W);
  uint8_t* work = (uint8_t*)k.alloc(VC_KMAJ_WORK, wp.total);
  if (!work) return VC_ERR_NOMEM;
  uint32_t* prev = (uint32_t*)(work + wp.prev);
  uint32_t* labels = k.d_labels ? k.d_labels : (uint32_t*)(work + wp.labels);
  uint32_t* flags = (uint32_t*)(work + wp.flags);
  unsigned long long* stat = (unsigned long long*)(work + wp.stat);
  g.d_labels = labels;
  g.groups_cap = K;
  g.d_groups = (vc_group*)(work + wp.groups);
  g.d_centroids = (uint64_t*)(work + wp.cents);
  g.d_rep_labels = nullptr;
  g.d_group_index = nullptr;
  KM_HIP(hipMemsetAsync(stat, 0, KM_STAT_WORDS * 8, s));
  int rc;
  for (uint32_t t = 0; t < k.max_iters; ++t) {
    if ((rc = assign_all(k.d_centres, k.d_assign))) return rc;
    hipLaunchKernelGGL(vc_kmaj_round_kernel, dim3(km_grid(n)), dim3(KM_BLK), 0, s, (const uint64_t*)k.d_assign, n, g.id_base, K, prev, t == 0 ? 1u : 0u, labels,
                       (uint32_t*)nullptr, stat + 2 * t);
    KM_HIP(hipGetLastError());
    unsigned long long home[2] = {0, 0};
    KM_HIP(hipMemcpyAsync(home, stat + 2 * t, 16, hipMemcpyDeviceToHost, s));
    KM_HIP(hipStreamSynchronize(s));
    st.cost[t] = home[0];
    st.n_changed[t] = home[1];
    st.n_iters = t + 1;
    if (home[1] == 0) {
      st.converged = 1;
      break;
    }
    uint64_t G = 0;
    if ((rc = vc_groups_run(g, fetch, &G, s, err))) return rc;
    hipLaunchKernelGGL(vc_kmaj_scatter_kernel, dim3(km_grid(G * g.W)), dim3(KM_BLK), 0, s, (const vc_group*)g.d_groups, (const uint64_t*)g.d_centroids, G, g.W,
                       g.id_base, K, k.d_centres);
    KM_HIP(hipGetLastError());
  }
  if ((rc = assign_all(k.d_centres, k.d_assign))) return rc;
  unsigned long long* fin = stat + 2 * VC_KMAJ_MAX_ITERS;
  KM_HIP(hipMemsetAsync(flags, 0, (size_t)K * 4, s));
  hipLaunchKernelGGL(vc_kmaj_round_kernel, dim3(km_grid(n)), dim3(KM_BLK), 0, s, (const uint64_t*)k.d_assign, n, g.id_base, K, (uint32_t*)nullptr, 0u, labels, flags,
                     fin);
  hipLaunchKernelGGL(vc_kmaj_empty_kernel, dim3(km_grid(K)), dim3(KM_BLK), 0, s, (const uint32_t*)flags, K, fin + 1);   // (fin[1] is 0: nothing "changed" without prev)
  KM_HIP(hipGetLastError());
  unsigned long long home[2] = {0, 0};
  KM_HIP(hipMemcpyAsync(home, fin, 16, hipMemcpyDeviceToHost, s));
  KM_HIP(hipStreamSynchronize(s));
  st.cost_final = home[0];
  st.n_empty = home[1];
  if (stats) *stats = st;
  return VC_OK;
}

int vc_kmajority_run_host(VcKmajArgs k, const VcGroupsArgs& g, const VcAssignAll& assign_all, const VcGroupsFetch& fetch, void* centres, uint64_t* assign,
                          uint32_t* labels, vc_kmajority_stats* stats, hipStream_t s, std::string* err) {
  const uint64_t n = g.n;
  if (stats) *stats = vc_kmajority_stats{};
  if (n == 0) return VC_OK;
  const size_t cbytes = (size_t)k.n_centres * g.W * 8, abytes = (size_t)n * 8;   // staged: centres | assign | labels
  uint8_t* stage = (uint8_t*)k.alloc(VC_KMAJ_STAGE, cbytes + abytes + (size_t)n * 4);
  if (!stage) return VC_ERR_NOMEM;
  k.d_centres = (uint64_t*)stage;
  k.d_assign = (uint64_t*)(stage + cbytes);
  k.d_labels = (uint32_t*)(stage + cbytes + abytes);
  KM_HIP(hipMemcpyAsync(stage, centres, cbytes, hipMemcpyHostToDevice, s));
  const int rc = vc_kmajority_run(k, g, assign_all, fetch, stats, s, err);
  if (rc) return rc;
  KM_HIP(hipMemcpyAsync(centres, k.d_centres, cbytes, hipMemcpyDeviceToHost, s));
  KM_HIP(hipMemcpyAsync(assign, k.d_assign, abytes, hipMemcpyDeviceToHost, s));
  if (labels) KM_HIP(hipMemcpyAsync(labels, k.d_labels, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  KM_HIP(hipStreamSynchronize(s));
  return VC_OK;
}
