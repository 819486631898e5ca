// ============================================================================
// vc_seed.hip -- device-side seeding for vc_kmajority*: farthest-first traversal and distance-weighted sampling over the resident
// records (vc_seed_centres*, vc_sharded_seed_centres*).  K sequential rounds, one small launch each (two in the weighted mode), no
// byte home.  The single engine's driver is here; the sharded root (vc_sharded.hip) drives the same kernels shard by shard through
// the launchers.  The plan arithmetic -- generator, block ranges, slot word, prefix search -- is vc_seed_plan.hpp.
// ============================================================================
#include <algorithm>

#include "vc_internal.hpp"
#include "vc_seed_plan.hpp"

// HAND-OFF.  A pick travels in a slot word, dist << 32 | (0xFFFFFFFF - i) (vc_seed_slot): round t reads the slot that an EARLIER
// launch has finished writing -- the init launch (t = 0), the block maxima of round t - 1 meeting in 64-bit atomicMax (farthest), or
// the pick launch (weighted) -- and leaves the next slot or partial[block] for a LATER launch.  A thousand blocks queueing on ONE
// address cost 10 us a round, so the farthest mode's slot is VC_SEED_SUBSLOTS words on lines of their own: block b adds to word
// b % VC_SEED_SUBSLOTS and the next launch takes the maximum of them all, which is the same maximum.  Three such slots rotate: round t
// reads one, adds to the next and clears the third, which round t - 1 read and round t + 1 will add to.  No block waits for, polls
// or counts another block.  The only addresses formed from data are the picked record's, range-checked against n first, and a
// block number of the prefix search, which is a loop counter below the number of blocks by construction.
namespace {

#define SEED_KEEP 8u   // trips of the pick kernel whose partials stay in registers

// the four wave results of a block meet here
struct SeedLds {
  uint64_t w[VC_SEED_BLOCK / VC_WAVE];
};

// the sum of a 64-bit value over a wave, in every lane's reach at lane 63: two 32-bit scans of the low 24 bits and the rest
// (x < 2^56: a block's distances sum to < 2^20, a store holds < 2^32 records)
__device__ __forceinline__ uint64_t seed_wave_sum64(uint64_t x) {
  const uint32_t lo = vc_wave_incl_scan((uint32_t)x & 0xFFFFFFu), hi = vc_wave_incl_scan((uint32_t)(x >> 24));
  return (uint64_t)lo + ((uint64_t)hi << 24);
}

// ring[0] = the first pick at distance 0 in its word 0, ring[1] = 0 (what atomicMax starts from; round 0 clears ring[2]), the two
// statistics words = 0.  One block.
__global__ void __launch_bounds__(VC_SEED_BLOCK) vc_seed_init_kernel(unsigned long long* __restrict__ ring, uint32_t s0, unsigned long long* __restrict__ stat) {
  for (uint32_t j = threadIdx.x; j < 2 * VC_SEED_SLOT_WORDS; j += VC_SEED_BLOCK) ring[j] = j == 0 ? vc_seed_slot(0u, s0) : 0ull;
  if (threadIdx.x < 2) stat[threadIdx.x] = 0ull;
}

// ROUND t.  The centre is the record that the maximum of slot_prev's n_prev words names (or, for a shard of a sharded store, the W
// words at `code`, fetched by the root): wave-uniform loads.  Block 0 records it into centre_out / pick_out / slot_rec and clears
// slot_zero.  Every block walks its fixed contiguous range of records (vc_seed_record_of: lane l of a wave reads word l of 64
// consecutive ones of each column), lowers best where the new distance is strictly smaller -- in round 0 best counts as infinity
// and is not read -- and writes only what changed.  Then the reduction for the next pick over the NEW best: the block maximum of
// the slot word into word blockIdx.x % n_next of slot_next by atomicMax (farthest), or the block's sum of distances into
// partial[block] (weighted).  slot_next / partial are null in the last round: nothing follows it.
template <int W>
__global__ void __launch_bounds__(VC_SEED_BLOCK) vc_seed_round_kernel(const uint64_t* __restrict__ cols, uint64_t stride, uint64_t n, uint32_t t, uint32_t method,
                                                                      const unsigned long long* __restrict__ slot_prev, uint32_t n_prev,
                                                                      const uint64_t* __restrict__ code, uint32_t id_base, uint64_t* __restrict__ centre_out,
                                                                      uint64_t* __restrict__ pick_out, unsigned long long* __restrict__ slot_rec,
                                                                      uint64_t* __restrict__ best, unsigned long long* __restrict__ slot_next, uint32_t n_next,
                                                                      unsigned long long* __restrict__ slot_zero, uint32_t* __restrict__ partial) {
  __shared__ SeedLds lds;
  uint64_t cw[W];
  if (code) {
#pragma unroll
    for (int w = 0; w < W; ++w) cw[w] = code[w];
  } else {
    uint64_t slot = 0;
    for (uint32_t q = 0; q < n_prev; ++q) {
      const uint64_t v = slot_prev[q * VC_SEED_SLOT_STRIDE];
      slot = v > slot ? v : slot;
    }
    const uint64_t s = vc_seed_slot_index(slot);
    if (s >= n) return;   // (never: every slot is written from a resident index; the whole grid leaves together)
#pragma unroll
    for (int w = 0; w < W; ++w) cw[w] = cols[(uint64_t)w * stride + s];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
      for (int w = 0; w < W; ++w) centre_out[w] = cw[w];
      if (pick_out) *pick_out = vc_pack(vc_seed_slot_dist(slot), id_base + (uint32_t)s);
      if (slot_rec) *slot_rec = slot;
    }
    if (slot_zero && blockIdx.x == 0 && threadIdx.x < VC_SEED_SUBSLOTS) slot_zero[threadIdx.x * VC_SEED_SLOT_STRIDE] = 0ull;
  }
  uint32_t sum = 0, far_d = 0, far_i = 0xFFFFFFFFu;   // this thread's records: their distances' sum; the farthest, the first of equals
  // (a thread past the end loads the last record instead, so that every load stands ahead of the first use, and uses nothing of it)
  uint32_t dist[VC_SEED_RECORDS], old[VC_SEED_RECORDS];
#pragma unroll
  for (uint32_t r = 0; r < VC_SEED_RECORDS; ++r) {
    const uint64_t i = vc_seed_record_of(blockIdx.x, threadIdx.x, r), at = i < n ? i : n - 1;
    dist[r] = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) dist[r] += (uint32_t)__builtin_popcountll(cols[(uint64_t)w * stride + at] ^ cw[w]);
    old[r] = t == 0 ? 0xFFFFFFFFu : (uint32_t)(best[at] >> 32);
  }
#pragma unroll
  for (uint32_t r = 0; r < VC_SEED_RECORDS; ++r) {
    const uint64_t i = vc_seed_record_of(blockIdx.x, threadIdx.x, r);
    if (i >= n) continue;
    const uint32_t d = dist[r];
    uint32_t now = old[r];
    if (d < now) {
      best[i] = vc_pack(d, t);
      now = d;
    }
    sum += now;
    if (far_i == 0xFFFFFFFFu || now > far_d) {
      far_d = now;
      far_i = (uint32_t)i;
    }
  }
  const uint32_t wave = threadIdx.x / VC_WAVE;
  if (method == VC_SEED_FARTHEST) {
    if (!slot_next) return;
    const uint32_t dmax = ~vc_wave_min(~far_d);   // (a thread without a record holds distance 0 and no index: it loses to every record)
    const uint32_t imin = vc_wave_min(far_d == dmax ? far_i : 0xFFFFFFFFu);
    if (vc_lane() == 0) lds.w[wave] = vc_seed_slot(dmax, imin);
    __syncthreads();
    if (threadIdx.x == 0) {
      uint64_t m = lds.w[0];
      for (uint32_t k = 1; k < VC_SEED_BLOCK / VC_WAVE; ++k) m = lds.w[k] > m ? lds.w[k] : m;
      // The word only grows, so a maximum at or below what one atomic load shows could not change it and the atomic is skipped (an
      // older value only costs the atomic it would have saved).
      unsigned long long* dst = slot_next + (blockIdx.x % n_next) * VC_SEED_SLOT_STRIDE;
      if (m > __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(dst, (unsigned long long)m);
    }
  } else {
    if (!partial) return;
    const uint32_t x = vc_wave_incl_scan(sum);
    if (vc_lane() == VC_WAVE - 1) lds.w[wave] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t tot = 0;
      for (uint32_t k = 0; k < VC_SEED_BLOCK / VC_WAVE; ++k) tot += (uint32_t)lds.w[k];
      partial[blockIdx.x] = tot;
    }
  }
}

// One step of the pick's block-wide prefix search: the 256 weights w (one per thread, in order) behind `base`.  The thread whose
// weight crosses the target (vc_seed_crosses; at most one in the whole search) reports through `found`.  Returns the 256 weights'
// sum; lds is free again on return.
__device__ __forceinline__ uint32_t seed_search_step(SeedLds& lds, uint32_t w, uint64_t base, uint64_t target, bool* found, uint64_t* before) {
  const uint32_t incl = vc_wave_incl_scan(w), wave = threadIdx.x / VC_WAVE;
  if (vc_lane() == VC_WAVE - 1) lds.w[wave] = incl;
  __syncthreads();
  uint32_t ahead = 0, all = 0;
  for (uint32_t k = 0; k < VC_SEED_BLOCK / VC_WAVE; ++k) {
    const uint32_t x = (uint32_t)lds.w[k];
    ahead += k < wave ? x : 0u;
    all += x;
  }
  __syncthreads();
  *before = base + ahead + (incl - w);
  *found = vc_seed_crosses(*before, w, target);
  return all;
}

// THE PICK of the weighted mode, one block: total = the sum of the partials, target = rnd % total (rnd = draw(t + 1), or for a
// shard the rest of the root's target, which is below its total); the block whose running sum crosses the target, 256 partials a
// trip; then that block's best re-read in record order, 256 records a trip, for the record.  total == 0: record 0 at distance 0.
// total_out (nullable) gets the total; slot_out (nullable: a shard asked for its total only) the pick.
__global__ void __launch_bounds__(VC_SEED_BLOCK) vc_seed_pick_kernel(const uint32_t* __restrict__ partial, const uint64_t* __restrict__ best, uint64_t n, uint64_t rnd,
                                                                     unsigned long long* __restrict__ slot_out, unsigned long long* __restrict__ total_out) {
  __shared__ SeedLds lds;
  __shared__ uint64_t hit[2];   // the crossing block and the rest of the target inside it
  const uint64_t nb = vc_seed_blocks(n);
  // the partials of the first SEED_KEEP trips stay in registers from the summing pass (2048 blocks: two million records), so that the
  // search's trips over them wait for no load
  uint32_t keep[SEED_KEEP];
  uint64_t mine = 0;
#pragma unroll
  for (uint32_t c = 0; c < SEED_KEEP; ++c) {
    const uint64_t j = (uint64_t)c * VC_SEED_BLOCK + threadIdx.x;
    keep[c] = j < nb ? partial[j] : 0u;
    mine += keep[c];
  }
  for (uint64_t j = (uint64_t)SEED_KEEP * VC_SEED_BLOCK + threadIdx.x; j < nb; j += VC_SEED_BLOCK) mine += partial[j];
  const uint64_t ws = seed_wave_sum64(mine);
  if (vc_lane() == VC_WAVE - 1) lds.w[threadIdx.x / VC_WAVE] = ws;
  if (threadIdx.x == 0) hit[0] = nb;
  __syncthreads();
  uint64_t total = 0;
  for (uint32_t k = 0; k < VC_SEED_BLOCK / VC_WAVE; ++k) total += lds.w[k];
  __syncthreads();
  if (total_out && threadIdx.x == 0) *total_out = total;
  if (!slot_out) return;
  if (total == 0) {
    if (threadIdx.x == 0) *slot_out = vc_seed_slot(0u, 0u);
    return;
  }
  const uint64_t target = rnd % total;
  uint64_t base = 0;   // (base <= target on entry of every trip)
  bool crossed = false;
  auto trip = [&](uint64_t j0, uint32_t w) {
    bool found;
    uint64_t before;
    const uint32_t all = seed_search_step(lds, w, base, target, &found, &before);
    if (found) {
      hit[0] = j0 + threadIdx.x;
      hit[1] = target - before;
    }
    if (target - base < all) crossed = true;
    else base += all;
  };
#pragma unroll
  for (uint32_t c = 0; c < SEED_KEEP; ++c)
    if (!crossed && (uint64_t)c * VC_SEED_BLOCK < nb) trip((uint64_t)c * VC_SEED_BLOCK, keep[c]);
  for (uint64_t j0 = (uint64_t)SEED_KEEP * VC_SEED_BLOCK; !crossed && j0 < nb; j0 += VC_SEED_BLOCK) trip(j0, j0 + threadIdx.x < nb ? partial[j0 + threadIdx.x] : 0u);
  __syncthreads();
  const uint64_t blk = hit[0], rest = hit[1];
  if (blk >= nb) {   // (never: the partials are the sums of what is searched)
    if (threadIdx.x == 0) *slot_out = vc_seed_slot(0u, 0u);
    return;
  }
  const uint64_t hi = vc_seed_block_hi(blk, n);
  uint32_t w[VC_SEED_RECORDS];   // (all loads ahead of the first trip)
#pragma unroll
  for (uint32_t r = 0; r < VC_SEED_RECORDS; ++r) {
    const uint64_t i = vc_seed_record_of(blk, threadIdx.x, r);
    w[r] = i < hi ? (uint32_t)(best[i] >> 32) : 0u;
  }
  base = 0;
  crossed = false;
#pragma unroll
  for (uint32_t r = 0; r < VC_SEED_RECORDS; ++r) {
    if (crossed) continue;
    bool found;
    uint64_t before;
    const uint32_t all = seed_search_step(lds, w[r], base, rest, &found, &before);
    if (found) *slot_out = vc_seed_slot(w[r], (uint32_t)vc_seed_record_of(blk, threadIdx.x, r));
    if (rest - base < all) crossed = true;
    else base += all;
  }
}

// After the last round: stat[0] += the distances of best, the low half of stat[1] = their maximum (atomics: the blocks' only
// meeting), and block 0 counts the picks t >= 1 at distance 0 from the slots into the high half of stat[1].  The two words are
// vc_seed_stats as it lies in memory.  slots may be null (the sharded root counts on the host).
__global__ void __launch_bounds__(VC_SEED_BLOCK) vc_seed_finish_kernel(const uint64_t* __restrict__ best, uint64_t n, const unsigned long long* __restrict__ slots,
                                                                       uint32_t K, unsigned long long* __restrict__ stat) {
  __shared__ SeedLds lds;
  __shared__ uint32_t far[VC_SEED_BLOCK / VC_WAVE];
  uint64_t sum = 0;
  uint32_t mx = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * VC_SEED_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * VC_SEED_BLOCK) {
    const uint32_t d = (uint32_t)(best[i] >> 32);
    sum += d;
    mx = d > mx ? d : mx;
  }
  const uint64_t ws = seed_wave_sum64(sum);
  const uint32_t wm = ~vc_wave_min(~mx), wave = threadIdx.x / VC_WAVE;
  if (vc_lane() == VC_WAVE - 1) {
    lds.w[wave] = ws;
    far[wave] = wm;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t tot = 0;
    uint32_t m = 0;
    for (uint32_t k = 0; k < VC_SEED_BLOCK / VC_WAVE; ++k) {
      tot += lds.w[k];
      m = far[k] > m ? far[k] : m;
    }
    if (tot) atomicAdd(stat, (unsigned long long)tot);
    if (m) atomicMax((uint32_t*)(stat + 1), m);
  }
  if (blockIdx.x != 0 || !slots) return;
  __syncthreads();
  uint32_t zero = 0;
  for (uint64_t t = 1 + threadIdx.x; t < K; t += VC_SEED_BLOCK) zero += vc_seed_slot_dist(slots[t]) == 0u ? 1u : 0u;
  const uint64_t wz = seed_wave_sum64(zero);
  if (vc_lane() == VC_WAVE - 1) lds.w[wave] = wz;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t z = 0;
    for (uint32_t k = 0; k < VC_SEED_BLOCK / VC_WAVE; ++k) z += (uint32_t)lds.w[k];
    ((uint32_t*)(stat + 1))[1] = z;
  }
}

int seed_fail(std::string* err, hipError_t r, const char* what) {
  if (err) *err = std::string("seed: ") + what + ": " + hipGetErrorString(r);
  return r == hipErrorOutOfMemory ? VC_ERR_NOMEM : VC_ERR_HIP;
}
#define SEED_HIP(call)                                       \
  do {                                                       \
    hipError_t _r = (call);                                  \
    if (_r != hipSuccess) return seed_fail(err, _r, #call);  \
  } while (0)

template <int W>
void launch_round(const VcSeedRound& a, hipStream_t s) {
  hipLaunchKernelGGL(vc_seed_round_kernel<W>, dim3((uint32_t)vc_seed_blocks(a.n)), dim3(VC_SEED_BLOCK), 0, s, a.cols, a.stride, a.n, a.t, a.method,
                     (const unsigned long long*)a.d_slot_prev, a.n_slot_prev, a.d_code, a.id_base, a.d_centre_out, a.d_pick_out, (unsigned long long*)a.d_slot_rec,
                     a.d_best, (unsigned long long*)a.d_slot_next, a.n_slot_next ? a.n_slot_next : 1u, (unsigned long long*)a.d_slot_zero, a.d_partial);
}

// the scratch of a vc_seed_centres* call, in bytes: the three rotating slots | slots [K], the record of every round's pick | the
// two statistics words | partial [blocks] | best [n] unless the caller's d_assign holds it.  Every word is written before it is
// read: two slots of the ring and the statistics by the init launch, the third by round 0, slots[t] by round t, a partial by every
// round that a pick follows, best by round 0.
struct SeedWork {
  uint64_t ring, slots, stat, partial, best, total;
  SeedWork(uint64_t n, uint32_t K, bool own_best) {
    uint64_t o = 0;
    ring = o;     o += 3ull * VC_SEED_SLOT_WORDS * 8;
    slots = o;    o += (uint64_t)K * 8;
    stat = o;     o += 16;
    partial = o;  o += (vc_seed_blocks(n) * 4 + 7) & ~7ull;
    best = o;     o += own_best ? n * 8 : 0;
    total = o;
  }
};

}  // namespace

hipError_t vc_launch_seed_round(const VcSeedRound& a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  if (vc_seed_blocks(a.n) > 0x7FFFFFFFull || (!a.d_code && (!a.d_slot_prev || !a.d_centre_out)) || !a.d_best || a.n_slot_prev > VC_SEED_SUBSLOTS ||
      a.n_slot_next > VC_SEED_SUBSLOTS)
    return hipErrorInvalidValue;
  switch (a.W) {
    case 1: launch_round<1>(a, s); break;
    case 2: launch_round<2>(a, s); break;
    case 4: launch_round<4>(a, s); break;
    case 8: launch_round<8>(a, s); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t vc_launch_seed_pick(const uint32_t* d_partial, const uint64_t* d_best, uint64_t n, uint64_t rnd, uint64_t* d_slot, uint64_t* d_total, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vc_seed_pick_kernel, dim3(1), dim3(VC_SEED_BLOCK), 0, s, d_partial, d_best, n, rnd, (unsigned long long*)d_slot, (unsigned long long*)d_total);
  return hipGetLastError();
}

hipError_t vc_launch_seed_finish(const uint64_t* d_best, uint64_t n, const uint64_t* d_slots, uint32_t K, uint64_t* d_stat, hipStream_t s) {
  const uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n + VC_SEED_BLOCK - 1) / VC_SEED_BLOCK, 1), 1024);
  hipLaunchKernelGGL(vc_seed_finish_kernel, dim3(grid), dim3(VC_SEED_BLOCK), 0, s, d_best, n, (const unsigned long long*)d_slots, K, (unsigned long long*)d_stat);
  return hipGetLastError();
}

// THE ROUNDS of the single engine (the header states the rule): the init launch, then per seed the round launch and, in the weighted
// mode and unless it was the last, the pick launch; the finish launch.  Nothing is waited for but, with stats, the 16 bytes at the end.
int vc_seed_run(const VcSeedArgs& a, vc_seed_stats* stats, hipStream_t s, std::string* err) {
  if (stats) *stats = vc_seed_stats{};
  if (a.n == 0) return VC_OK;
  const uint32_t K = a.n_centres;
  const SeedWork wp(a.n, K, a.d_assign == nullptr);
  uint8_t* work = (uint8_t*)a.alloc(VC_SEED_WORK, wp.total);
  if (!work) return VC_ERR_NOMEM;
  uint64_t* ring = (uint64_t*)(work + wp.ring);
  uint64_t* slots = (uint64_t*)(work + wp.slots);
  uint64_t* stat = (uint64_t*)(work + wp.stat);
  uint32_t* partial = (uint32_t*)(work + wp.partial);
  uint64_t* best = a.d_assign ? a.d_assign : (uint64_t*)(work + wp.best);
  const uint32_t s0 = (uint32_t)(vc_seed_draw(a.seed, 0) % a.n);
  hipLaunchKernelGGL(vc_seed_init_kernel, dim3(1), dim3(VC_SEED_BLOCK), 0, s, (unsigned long long*)ring, s0, (unsigned long long*)stat);
  SEED_HIP(hipGetLastError());
  // farthest: the ring rotates; weighted: the pick launch writes the one word the next round reads, word 0 of ring[0]
  const bool farthest = a.method == VC_SEED_FARTHEST;
  VcSeedRound r{};
  r.cols = a.cols; r.stride = a.stride; r.n = a.n; r.W = a.W; r.id_base = a.id_base; r.method = a.method; r.d_best = best;
  for (uint32_t t = 0; t < K; ++t) {
    const bool last = t + 1 == K;
    r.t = t;
    r.d_slot_prev = farthest ? ring + (uint64_t)(t % 3) * VC_SEED_SLOT_WORDS : ring;
    r.n_slot_prev = farthest ? VC_SEED_SUBSLOTS : 1u;
    r.d_slot_rec = slots + t;
    r.d_centre_out = a.d_centres + (uint64_t)t * a.W;
    r.d_pick_out = a.d_picks ? a.d_picks + t : nullptr;
    r.d_slot_next = !last && farthest ? ring + (uint64_t)((t + 1) % 3) * VC_SEED_SLOT_WORDS : nullptr;
    r.n_slot_next = VC_SEED_SUBSLOTS;
    r.d_slot_zero = !last && farthest ? ring + (uint64_t)((t + 2) % 3) * VC_SEED_SLOT_WORDS : nullptr;
    r.d_partial = !last && !farthest ? partial : nullptr;
    SEED_HIP(vc_launch_seed_round(r, s));
    if (r.d_partial) SEED_HIP(vc_launch_seed_pick(partial, best, a.n, vc_seed_draw(a.seed, (uint64_t)t + 1), ring, nullptr, s));
  }
  SEED_HIP(vc_launch_seed_finish(best, a.n, slots, K, stat, s));
  if (stats) {
    vc_seed_stats st{};
    SEED_HIP(hipMemcpyAsync(&st, stat, sizeof st, hipMemcpyDeviceToHost, s));
    SEED_HIP(hipStreamSynchronize(s));
    *stats = st;
  }
  return VC_OK;
}

int vc_seed_run_host(const VcSeedHostArgs& a, const std::function<int(uint64_t* d_centres, uint64_t* d_picks, uint64_t* d_assign, vc_seed_stats* stats)>& run,
                     hipStream_t s, std::string* err) {
  if (a.stats) *a.stats = vc_seed_stats{};
  if (a.n == 0) return VC_OK;
  const size_t cbytes = (size_t)a.n_centres * a.W * 8, pbytes = (size_t)a.n_centres * 8, abytes = a.assign ? (size_t)a.n * 8 : 0;   // staged: centres | picks | assign
  uint8_t* stage = (uint8_t*)a.alloc(VC_SEED_STAGE, cbytes + pbytes + abytes);
  if (!stage) return VC_ERR_NOMEM;
  uint64_t* d_centres = (uint64_t*)stage;
  uint64_t* d_picks = (uint64_t*)(stage + cbytes);
  uint64_t* d_assign = a.assign ? (uint64_t*)(stage + cbytes + pbytes) : nullptr;
  const int rc = run(d_centres, a.picks ? d_picks : nullptr, d_assign, a.stats);
  if (rc) return rc;
  SEED_HIP(hipMemcpyAsync(a.centres, d_centres, cbytes, hipMemcpyDeviceToHost, s));
  if (a.picks) SEED_HIP(hipMemcpyAsync(a.picks, d_picks, pbytes, hipMemcpyDeviceToHost, s));
  if (a.assign) SEED_HIP(hipMemcpyAsync(a.assign, d_assign, abytes, hipMemcpyDeviceToHost, s));
  SEED_HIP(hipStreamSynchronize(s));
  return VC_OK;
}
