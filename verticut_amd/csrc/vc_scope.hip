// Scoped k-NN: vc_search_knn_scoped* and vc_sharded_search_knn_scoped* (the header states the contract).  Every query searches only
// among the records whose scope word equals its own.  One driver for both handle kinds over the view's gather by id; the plan
// arithmetic is vc_scope_plan.hpp.  Exact brute force over each scope: no index, no search underneath.
//
// 1 QUERY SIDE.  (qscope[q], q) sorted by vc_radix_sort_pairs; head flags and a scan number the U distinct values ascending (slots):
//   uniq [U], the slot of every SORTED query, the run [qrun[u], qrun[u + 1]) of sorted queries of slot u, the query codes in sorted order.
// 2 MATCH.  One pass over scope: a record whose value is one of the U (binary search) sets its bit in a keep set (bits + rank, as
//   vc_filter_bits_kernel).  THE FIRST WAIT fetches U and A.  Records no query names cost nothing from here on.
// 3 ORDER.  The A matched ids ascending, each with its slot, then the stable radix sort by slot on ceil(log2 U) bits: the list L,
//   slots ascending and ids ascending within a slot -- list order within a scope is id order.  seg[u] = the first position of slot u
//   (a binary search per slot).  THE SECOND WAIT fetches seg and qrun, 2 (U + 1) words: the host knows every S_q, hence the
//   statistics, the sub-batches and the windows, and the device never has to be asked again.
// 4 SCAN, per sub-batch of sorted queries and window of L.  The window's codes come through the view's gather as rows [n][W].  A
//   wave owns a slice (vc_filter_plan.hpp): it keeps its positions' codes and slots in registers, reads the slots of its first and
//   last position, and loops over the sorted queries of exactly those slots (vc_scope_slice_queries) -- query words are read at
//   wave-uniform addresses, a pair counts only where the position's slot is the query's.  The three walks of vc_filter.hip:
//     walk 1  distances counted per (query, slice) in the wave's own LDS histogram, added to the query's global one (sums)
//             vc_scope_cut_kernel: tau, below and kk = min(k, positions of the segment in the window) per query
//     walk 2  per (query, slice) the in-scope entries with d < tau and d == tau -> the query's OWN counters: a query owns one pair
//             per slice its segment touches, laid out by an exclusive scan of vc_scope_cost over the sorted queries
//             vc_scope_base_kernel: exclusive bases along a query's slices of the window
//     walk 3  placement by ballot rank: d < tau at base_lt + rank, d == tau at below + base_eq + rank while below kk
//   A query whose part of the window has at most k positions takes them all: no histogram, tau above every distance.
//   vc_launch_select_ring orders the kk entries; a segment that began in an earlier window has its row merged into its running row by
//   vc_launch_select_lists.  Sums and ranks only: no result depends on the order in which blocks finish.  Blocks meet in the next
//   launch only.  Every store into a row or a counter is bounds-tested.
// 5 FINISH.  Rows go from sorted-query order to the caller's, cut at min(k, S_q) and padded; counts; the statistics are the host's.
#include <algorithm>
#include <vector>

#include "vc_internal.hpp"
#include "vc_retain.hpp"
#include "vc_scope_plan.hpp"

static_assert(VC_FILTER_BLOCK == VC_WAVE * VC_FILTER_BLOCK_SLICES, "a wave per slice");

namespace {

#define SC_BLK 256u
#define SC_NO_SLOT 0xFFFFFFFFu   // the slot of a position past the window: no query has it (slots are below nq <= 2^32 - 1)

// the first index of ascending a[0, n) whose value is not below v
__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t* __restrict__ a, uint32_t n, uint32_t v) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- 1. the query side --------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SC_BLK) vc_scope_pairs_kernel(const uint32_t* __restrict__ qscope, uint32_t nq, uint32_t* __restrict__ keys,
                                                                uint32_t* __restrict__ vals) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  keys[q] = qscope[q];
  vals[q] = q;
}

// flag[j] = sorted query j opens a new value (j > 0); flag[nq] = 0
__global__ void __launch_bounds__(SC_BLK) vc_scope_heads_kernel(const uint32_t* __restrict__ skeys, uint32_t nq, uint32_t* __restrict__ flag) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j > nq) return;
  flag[j] = j > 0 && j < nq && skeys[j] != skeys[j - 1] ? 1u : 0u;
}

// scanned = the exclusive scan of flag: slot[j] = scanned[j] + flag[j].  The head of a slot writes its value and where its run of
// sorted queries begins; the last query closes the tables (qrun[U] = nq) and leaves U in *n_slots; every query's code goes to sorted order
__global__ void __launch_bounds__(SC_BLK) vc_scope_slots_kernel(const uint32_t* __restrict__ skeys, const uint32_t* __restrict__ svals,
                                                                const uint32_t* __restrict__ flag, const uint32_t* __restrict__ scanned, uint32_t nq,
                                                                const uint64_t* __restrict__ queries, uint32_t W, uint32_t* __restrict__ qslot,
                                                                uint32_t* __restrict__ uniq, uint32_t* __restrict__ qrun, uint64_t* __restrict__ sq,
                                                                uint32_t* __restrict__ n_slots) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nq) return;
  const uint32_t f = flag[j], u = scanned[j] + f;   // u <= j < nq: inside uniq and qrun
  qslot[j] = u;
  if (j == 0 || f) {
    uniq[u] = skeys[j];
    qrun[u] = j;
  }
  if (j == nq - 1) {
    qrun[u + 1] = nq;
    *n_slots = u + 1;
  }
  const uint32_t q = svals[j];
  if (q < nq)
    for (uint32_t w = 0; w < W; ++w) sq[(uint64_t)j * W + w] = queries[(uint64_t)q * W + w];
}

// ---- 2. the match: one block per 256-bit keep block, one ballot per wave makes one word (vc_filter_bits_kernel's shape) ---------------
__global__ void __launch_bounds__(VC_FILTER_BLOCK) vc_scope_match_kernel(const uint32_t* __restrict__ scope, const uint32_t* __restrict__ uniq,
                                                                         const uint32_t* __restrict__ n_slots, uint32_t nq, uint64_t n, uint64_t nblocks,
                                                                         uint64_t* __restrict__ bits, uint32_t* __restrict__ pop) {
  __shared__ uint32_t wpop[VC_FILTER_BLOCK_SLICES];
  const uint32_t lane = vc_lane(), wave = threadIdx.x / VC_WAVE, U = min(*n_slots, nq);
  for (uint64_t b = blockIdx.x; b <= nblocks; b += gridDim.x) {   // (block-uniform)
    if (b == nblocks) {
      if (threadIdx.x == 0) pop[b] = 0u;
      break;
    }
    const uint64_t i = b * VC_KEEP_BLOCK_BITS + threadIdx.x;
    bool keep = false;
    if (i < n) {
      const uint32_t v = scope[i], at = lower_bound_u32(uniq, U, v);
      keep = at < U && uniq[at] == v;
    }
    const uint64_t word = __ballot(keep);
    if (lane == 0) {
      bits[b * VC_KEEP_BLOCK_WORDS + wave] = word;
      wpop[wave] = (uint32_t)__popcll(word);
    }
    __syncthreads();
    if (threadIdx.x == 0) pop[b] = wpop[0] + wpop[1] + wpop[2] + wpop[3];
    __syncthreads();
  }
}

// ---- 3. the matched ids ascending, each with its slot: one thread per 64-bit word of the keep set --------------------------------------
__global__ void __launch_bounds__(SC_BLK) vc_scope_list_kernel(const VcKeepSet ks, uint64_t nwords, uint32_t id_base, const uint32_t* __restrict__ scope,
                                                               const uint32_t* __restrict__ uniq, uint32_t U, uint32_t A, uint32_t* __restrict__ slots,
                                                               uint32_t* __restrict__ ids) {
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nwords; j += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t word = ks.bits[j];
    if (!word) continue;
    uint32_t r = vc_keep_rank(ks, (uint32_t)(j << 6));   // set bits before this word
    while (word) {
      const uint32_t b = (uint32_t)__ffsll((unsigned long long)word) - 1u;
      word &= word - 1;
      const uint32_t i = (uint32_t)(j << 6) + b;          // a set bit: i < n
      if (r < A) {
        slots[r] = lower_bound_u32(uniq, U, scope[i]);    // (a matched record: its value is among the U)
        ids[r] = id_base + i;
      }
      ++r;
    }
  }
}

// seg[u] = the first position of L whose slot is not below u, u = 0 .. U: seg[U] = A
__global__ void __launch_bounds__(SC_BLK) vc_scope_segs_kernel(const uint32_t* __restrict__ sslots, uint32_t A, uint32_t U, uint32_t* __restrict__ seg) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u > U) return;
  seg[u] = lower_bound_u32(sslots, A, u);
}

// the counters of every sorted query (vc_scope_cost); cost[nq] = 0, so that the exclusive scan over nq + 1 words ends in the total
__global__ void __launch_bounds__(SC_BLK) vc_scope_cost_kernel(const uint32_t* __restrict__ qslot, const uint32_t* __restrict__ seg, uint32_t nq, uint32_t U,
                                                               uint32_t window, uint32_t len, uint32_t* __restrict__ cost) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j > nq) return;
  uint32_t c = 0;
  if (j < nq) {
    const uint32_t u = qslot[j];
    if (u < U) c = vc_scope_cost(seg[u], seg[u + 1], window, len);
  }
  cost[j] = c;
}

// ---- 4. the scan ------------------------------------------------------------------------------------------------------------------------
struct ScopeWalk {
  const uint64_t* codes;     // [n][W] the gathered rows of the window
  const uint32_t* ids;       // [n] their ids (L from w0 on)
  const uint32_t* pslot;     // [n] their slots
  uint32_t n, w0, window;    // positions of the window, where it starts in L, the window knob
  uint32_t U;
  const uint32_t* qrun;      // [U + 1]
  const uint32_t* seg;       // [U + 1]
  const uint32_t* qslot;     // [nq] slot of the sorted queries
  const uint64_t* sq;        // [nq][W] their codes
  const uint32_t* coff;      // [nq + 1] exclusive scan of the queries' counters
  uint32_t b0;               // the sub-batch's first sorted query: row j - b0, counters from coff[j] - coff[b0]
  uint32_t j0, j1;           // the sorted queries whose segment reaches into this window
  uint32_t n_rows;           // rows of the sub-batch's tables
  uint32_t n_counters;       // entries of lt and eq
  uint32_t bits, k;
  uint32_t* hist;            // [n_rows][bits + 1]
  uint32_t* tau;             // [n_rows]
  uint32_t* below;           // [n_rows]
  uint32_t* kk;              // [n_rows] entries the window gives the row: min(k, positions of the segment in the window)
  uint32_t* lt;              // counts, then exclusive bases, of d < tau
  uint32_t* eq;              // the same of d == tau
  uint64_t* cand;            // [n_rows][k]
};

template <int W>
__device__ __forceinline__ uint32_t pair_dist(const uint64_t (&x)[W], const uint64_t (&y)[W]) {
  uint32_t d = 0;
#pragma unroll
  for (int w = 0; w < W; ++w) d += (uint32_t)__builtin_popcountll(x[w] ^ y[w]);
  return d;
}

enum { WALK_HIST = 0, WALK_COUNT = 1, WALK_PLACE = 2 };

// THE WALKS.  No block barrier: a wave's trip count is its own.  WALK_HIST, dynamic LDS: a histogram of bits + 1 words per wave, used by
// that wave alone (its LDS operations execute in program order).
template <int W, int WALK>
__global__ void __launch_bounds__(VC_FILTER_BLOCK) vc_scope_walk_kernel(const ScopeWalk a) {
  constexpr int R = (int)vc_filter_steps(W);
  constexpr uint32_t LEN = vc_filter_slice_len(W);
  extern __shared__ uint32_t hl_all[];
  const uint32_t lane = vc_lane(), wave = threadIdx.x / VC_WAVE, slice = blockIdx.x * VC_FILTER_BLOCK_SLICES + wave, B = a.bits + 1;
  const uint32_t p0 = slice * LEN;   // (slice * LEN < n + 4 LEN: the grid covers the window's slices)
  if (p0 >= a.n) return;             // wave-uniform
  const uint32_t p1 = min(a.n, p0 + LEN);
  uint64_t rec[R][W];
  uint32_t ps[R], id[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t p = p0 + 64u * r + lane;
    const bool in = p < a.n;
    ps[r] = in ? a.pslot[p] : SC_NO_SLOT;
    id[r] = WALK == WALK_PLACE && in ? a.ids[p] : 0u;
#pragma unroll
    for (int w = 0; w < W; ++w) rec[r][w] = in ? a.codes[(uint64_t)p * W + w] : 0ull;
  }
  const uint32_t u_first = a.pslot[p0], u_last = a.pslot[p1 - 1];   // wave-uniform
  if (u_first > u_last || u_last >= a.U) return;
  uint32_t ja, jb, j_lo, j_hi;
  vc_scope_slice_queries(a.qrun, u_first, u_last, a.j0, a.j1, &ja, &jb);
  vc_scope_split(ja, jb, blockIdx.y, gridDim.y, &j_lo, &j_hi);
  const uint32_t off0 = a.coff[a.b0];
  const unsigned long long lower = (1ull << lane) - 1ull;
  uint32_t* hl = hl_all + wave * B;
  for (uint32_t j = j_lo; j < j_hi; ++j) {   // wave-uniform
    const uint32_t u = a.qslot[j], row = j - a.b0;
    if (u >= a.U || row >= a.n_rows) continue;
    const uint32_t lo = a.seg[u], hi = a.seg[u + 1];
    if (max(lo, a.w0 + p0) >= min(hi, a.w0 + p1)) continue;   // an empty scope between its neighbours: no position, no counter
    uint64_t cw[W];
#pragma unroll
    for (int w = 0; w < W; ++w) cw[w] = a.sq[(uint64_t)j * W + w];
    if (WALK == WALK_HIST) {
      if (vc_scope_in_window(lo, hi, a.w0, a.n) <= a.k) continue;   // the row takes every position: the cut needs no histogram
      for (uint32_t b = lane; b < B; b += VC_WAVE) hl[b] = 0u;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint32_t d = pair_dist<W>(rec[r], cw);   // d <= bits
        if (ps[r] == u) atomicAdd(&hl[d], 1u);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      __builtin_amdgcn_wave_barrier();
      for (uint32_t b = lane; b < B; b += VC_WAVE) {
        const uint32_t v = hl[b];
        if (v) atomicAdd(&a.hist[(uint64_t)row * B + b], v);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      __builtin_amdgcn_wave_barrier();
      continue;
    }
    const uint32_t tau = a.tau[row];
    const uint32_t c = a.coff[j] - off0 + vc_scope_counter(lo, hi, a.w0, a.window, LEN, slice);
    if (WALK == WALK_COUNT) {
      uint32_t n_lt = 0, n_eq = 0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint32_t d = pair_dist<W>(rec[r], cw);
        const bool in = ps[r] == u;
        n_lt += (uint32_t)__popcll(__ballot(in && d < tau));
        n_eq += (uint32_t)__popcll(__ballot(in && d == tau));
      }
      if (lane == 0 && c < a.n_counters) {
        a.lt[c] = n_lt;
        a.eq[c] = n_eq;
      }
      continue;
    }
    if (c >= a.n_counters) continue;
    const uint32_t kk = min(a.kk[row], a.k);
    uint32_t at_lt = a.lt[c];          // wave-uniform
    uint32_t at_eq = a.below[row] + a.eq[c];
    uint64_t* out = a.cand + (uint64_t)row * a.k;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint32_t d = pair_dist<W>(rec[r], cw);
      const bool in = ps[r] == u, is_lt = in && d < tau, is_eq = in && d == tau;
      const unsigned long long m_lt = __ballot(is_lt), m_eq = __ballot(is_eq);
      const uint32_t p_lt = at_lt + (uint32_t)__popcll(m_lt & lower), p_eq = at_eq + (uint32_t)__popcll(m_eq & lower);
      if (is_lt && p_lt < kk) out[p_lt] = vc_pack(d, id[r]);   // (below < kk: the test never fails; it keeps the store inside the row)
      if (is_eq && p_eq < kk) out[p_eq] = vc_pack(d, id[r]);
      at_lt += (uint32_t)__popcll(m_lt);
      at_eq += (uint32_t)__popcll(m_eq);
    }
  }
}

// tau, below and kk of the sorted queries [j0, j1) in this window
__global__ void __launch_bounds__(SC_BLK) vc_scope_cut_kernel(const ScopeWalk a) {
  const uint32_t j = a.j0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.j1) return;
  const uint32_t u = a.qslot[j], row = j - a.b0;
  if (row >= a.n_rows) return;
  uint32_t tau = 0xFFFFFFFFu, below = 0, kk = 0;
  if (u < a.U) {
    const uint32_t m = vc_scope_in_window(a.seg[u], a.seg[u + 1], a.w0, a.n);
    kk = min(a.k, m);
    below = m;
    if (m > a.k) vc_filter_cut(a.hist + (uint64_t)row * (a.bits + 1), a.bits, kk, &tau, &below);
  }
  a.tau[row] = tau;
  a.below[row] = below;
  a.kk[row] = kk;
}

// the counts of a query along its slices of this window -> exclusive bases, in place: one wave per query
__global__ void __launch_bounds__(VC_FILTER_BLOCK) vc_scope_base_kernel(const ScopeWalk a, uint32_t len) {
  const uint32_t j = a.j0 + blockIdx.x * VC_FILTER_BLOCK_SLICES + threadIdx.x / VC_WAVE, lane = vc_lane();
  if (j >= a.j1) return;
  const uint32_t u = a.qslot[j];
  if (u >= a.U) return;
  const uint32_t lo = a.seg[u], hi = a.seg[u + 1], n_sl = vc_scope_window_slices(lo, hi, a.w0, a.n, len);
  const uint32_t c0 = a.coff[j] - a.coff[a.b0] + vc_scope_prior(lo, hi, a.w0, a.window, len);
  uint32_t cl = 0, ce = 0;   // wave-uniform carries
  for (uint32_t s0 = 0; s0 < n_sl; s0 += VC_WAVE) {
    const uint32_t s = s0 + lane, c = c0 + s;
    const bool in = s < n_sl && c < a.n_counters;
    const uint32_t vl = in ? a.lt[c] : 0u, ve = in ? a.eq[c] : 0u;
    uint32_t tl, te;
    const uint32_t xl = vc_wave_excl_scan(vl, tl), xe = vc_wave_excl_scan(ve, te);
    if (in) {
      a.lt[c] = cl + xl;
      a.eq[c] = ce + xe;
    }
    cl += tl;
    ce += te;
  }
}

// ---- 5. rows [n][k] of the sorted queries first .. first + n -> the caller's rows, cut at min(k, S_q) and padded; rows null: padded rows
// and count 0 for the caller's queries first .. first + n themselves
__global__ void __launch_bounds__(SC_BLK) vc_scope_emit_kernel(const uint64_t* __restrict__ rows, uint32_t first, uint32_t n, uint32_t k, uint32_t nq,
                                                               const uint32_t* __restrict__ svals, const uint32_t* __restrict__ qslot,
                                                               const uint32_t* __restrict__ seg, uint32_t U, uint64_t* __restrict__ out,
                                                               uint32_t* __restrict__ counts) {
  const uint64_t total = (uint64_t)n * k;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = (uint32_t)(e / k), i = (uint32_t)(e % k), j = first + r;
    uint32_t oq = j, cnt = 0;
    if (rows) {
      oq = svals[j];
      const uint32_t u = qslot[j];
      if (u < U) cnt = min(k, seg[u + 1] - seg[u]);
    }
    if (oq >= nq) continue;
    out[(uint64_t)oq * k + i] = i < cnt ? rows[e] : VC_PACK_INF;
    if (i == 0 && counts) counts[oq] = cnt;
  }
}

int scope_fail(std::string* err, hipError_t r, const char* what) { return vc_hip_fail(err, "scoped search", r, what); }
#define SCOPE_HIP(call)                                       \
  do {                                                        \
    hipError_t _r = (call);                                   \
    if (_r != hipSuccess) return scope_fail(err, _r, #call);  \
  } while (0)

hipError_t launch_walk(int which, const ScopeWalk& a, uint32_t W, hipStream_t s) {
  if (a.n == 0 || a.j1 <= a.j0) return hipSuccess;
  const uint32_t gx = vc_filter_scan_blocks(vc_filter_n_slices(a.n, W)), gy = vc_scope_grid_y(gx, a.j1 - a.j0);
  const dim3 grid(gx, gy), block(VC_FILTER_BLOCK);
  const size_t lds = (size_t)VC_FILTER_BLOCK_SLICES * (a.bits + 1) * 4;
#define SC_LAUNCH(Wc)                                                                                                             \
  case Wc:                                                                                                                        \
    if (which == WALK_HIST) hipLaunchKernelGGL((vc_scope_walk_kernel<Wc, WALK_HIST>), grid, block, lds, s, a);                    \
    else if (which == WALK_COUNT) hipLaunchKernelGGL((vc_scope_walk_kernel<Wc, WALK_COUNT>), grid, block, 0, s, a);               \
    else hipLaunchKernelGGL((vc_scope_walk_kernel<Wc, WALK_PLACE>), grid, block, 0, s, a);                                        \
    break;
  switch (W) {
    SC_LAUNCH(1)
    SC_LAUNCH(2)
    SC_LAUNCH(4)
    SC_LAUNCH(8)
    default: return hipErrorInvalidValue;
  }
#undef SC_LAUNCH
  return hipGetLastError();
}

uint32_t grid_of(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + SC_BLK - 1) / SC_BLK, 1), 4096); }
uint32_t blocks_of(uint64_t items) { return (uint32_t)((items + SC_BLK - 1) / SC_BLK); }   // one thread per item
inline uint64_t up8(uint64_t x) { return (x + 7) & ~7ull; }

// VC_SCOPE_QUERY, in bytes: U | two (key, value) pairs of the query sort [nq] | its work | flag, scanned [nq + 1] | the scan's work |
// qslot [nq] | uniq [nq] | qrun, seg, coff [nq + 1] | the sorted queries' codes [nq][W]
struct QueryWork {
  uint64_t n_slots, keys[2], vals[2], sort_work, flag, scanned, scan_work, qslot, uniq, qrun, seg, coff, sq, total;
  QueryWork(uint32_t nq, uint32_t W) {
    const uint64_t row = up8((uint64_t)nq * 4), row1 = up8(((uint64_t)nq + 1) * 4);
    uint64_t o = 0;
    n_slots = o;    o += 8;
    for (int i = 0; i < 2; ++i) { keys[i] = o; o += row; vals[i] = o; o += row; }
    sort_work = o;  o += up8(vc_radix_sort_work_words(nq) * 4);
    flag = o;       o += row1;
    scanned = o;    o += row1;
    scan_work = o;  o += up8(vc_scan_work_words((uint64_t)nq + 1) * 4);
    qslot = o;      o += row;
    uniq = o;       o += row;
    qrun = o;       o += row1;
    seg = o;        o += row1;
    coff = o;       o += row1;
    sq = o;         o += (uint64_t)nq * W * 8;
    total = o;
  }
};
// VC_SCOPE_LIST: two (slot, id) pairs [A] | the sort's work
struct ListWork {
  uint64_t keys[2], vals[2], sort_work, total;
  explicit ListWork(uint32_t A) {
    const uint64_t row = up8((uint64_t)A * 4);
    uint64_t o = 0;
    for (int i = 0; i < 2; ++i) { keys[i] = o; o += row; vals[i] = o; o += row; }
    sort_work = o;  o += up8(vc_radix_sort_work_words(A) * 4);
    total = o;
  }
};
// VC_SCOPE_WORK for sub-batches of at most nb queries and nc counters: hist [nb][bits + 1] | tau, below, kk [nb] | lt, eq [nc] | found [wcap]
struct BatchWork {
  uint64_t hist, tau, below, kk, lt, eq, found, total;
  BatchWork(uint32_t nb, uint32_t nc, uint32_t wcap, uint32_t bits) {
    const uint64_t row = up8((uint64_t)nb * 4);
    uint64_t o = 0;
    hist = o;   o += up8((uint64_t)nb * (bits + 1) * 4);
    tau = o;    o += row;
    below = o;  o += row;
    kk = o;     o += row;
    lt = o;     o += up8((uint64_t)nc * 4);
    eq = o;     o += up8((uint64_t)nc * 4);
    found = o;  o += up8((uint64_t)wcap * 4);
    total = o;
  }
};

}  // namespace

int vc_scope_run(const VcStoreView& v, const VcScopeArgs& a, vc_scope_stats* stats, hipStream_t s, std::string* err) {
  if (stats) *stats = vc_scope_stats{};
  vc_scope_stats st{};
  const uint32_t W = v.W, nq = a.nq, k = a.k, len = vc_filter_slice_len(W), window = vc_scope_window(a.window);
  const auto pad_all = [&]() {
    hipLaunchKernelGGL(vc_scope_emit_kernel, dim3(grid_of((uint64_t)nq * k)), dim3(SC_BLK), 0, s, (const uint64_t*)nullptr, 0u, nq, k, nq,
                       (const uint32_t*)nullptr, (const uint32_t*)nullptr, (const uint32_t*)nullptr, 0u, a.d_out, a.d_counts);
    return hipGetLastError();
  };
  if (v.n == 0) {
    SCOPE_HIP(pad_all());
    return VC_OK;
  }
  if (v.n > 0xFFFFFFFFull) {
    if (err) *err = "scoped search: more than 2^32 - 1 records";
    return VC_ERR_INVALID;
  }
  int dev = 0, n_cu = 0;
  SCOPE_HIP(hipGetDevice(&dev));
  SCOPE_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
  // ---- 1. the query side
  const QueryWork qw(nq, W);
  uint8_t* qb = (uint8_t*)v.alloc(VC_SCOPE_QUERY, qw.total);
  if (!qb) return VC_ERR_NOMEM;
  uint32_t* n_slots = (uint32_t*)(qb + qw.n_slots);
  uint32_t* qkeys[2] = {(uint32_t*)(qb + qw.keys[0]), (uint32_t*)(qb + qw.keys[1])};
  uint32_t* qvals[2] = {(uint32_t*)(qb + qw.vals[0]), (uint32_t*)(qb + qw.vals[1])};
  uint32_t* flag = (uint32_t*)(qb + qw.flag);
  uint32_t* scanned = (uint32_t*)(qb + qw.scanned);
  uint32_t* qslot = (uint32_t*)(qb + qw.qslot);
  uint32_t* uniq = (uint32_t*)(qb + qw.uniq);
  uint32_t* qrun = (uint32_t*)(qb + qw.qrun);
  uint32_t* seg = (uint32_t*)(qb + qw.seg);
  uint32_t* coff = (uint32_t*)(qb + qw.coff);
  uint64_t* sq = (uint64_t*)(qb + qw.sq);
  hipLaunchKernelGGL(vc_scope_pairs_kernel, dim3(blocks_of(nq)), dim3(SC_BLK), 0, s, a.d_qscope, nq, qkeys[0], qvals[0]);
  SCOPE_HIP(hipGetLastError());
  SCOPE_HIP(vc_radix_sort_pairs(qkeys, qvals, nq, 32, (uint32_t*)(qb + qw.sort_work), s));
  const int qres = (int)(vc_radix_sort_passes(32) & 1);
  const uint32_t* skeys = qkeys[qres];
  const uint32_t* svals = qvals[qres];
  hipLaunchKernelGGL(vc_scope_heads_kernel, dim3(blocks_of((uint64_t)nq + 1)), dim3(SC_BLK), 0, s, skeys, nq, flag);
  SCOPE_HIP(hipGetLastError());
  SCOPE_HIP(vc_exclusive_scan_u32(flag, scanned, (uint64_t)nq + 1, (uint32_t*)(qb + qw.scan_work), s));
  hipLaunchKernelGGL(vc_scope_slots_kernel, dim3(blocks_of(nq)), dim3(SC_BLK), 0, s, skeys, svals, (const uint32_t*)flag, (const uint32_t*)scanned, nq,
                     a.d_queries, W, qslot, uniq, qrun, sq, n_slots);
  SCOPE_HIP(hipGetLastError());
  // ---- 2. the match, and THE FIRST WAIT: U and A
  const uint64_t nblocks = vc_keep_blocks(v.n), nwords = nblocks * VC_KEEP_BLOCK_WORDS;
  const uint64_t o_rank = nwords * 8, o_work = o_rank + up8((nblocks + 1) * 4), keep_bytes = o_work + up8(vc_scan_work_words(nblocks + 1) * 4);
  uint8_t* kb = (uint8_t*)v.alloc(VC_SCOPE_KEEP, keep_bytes);
  if (!kb) return VC_ERR_NOMEM;
  uint64_t* bits = (uint64_t*)kb;
  uint32_t* rank = (uint32_t*)(kb + o_rank);
  hipLaunchKernelGGL(vc_scope_match_kernel, dim3((uint32_t)std::min<uint64_t>(nblocks + 1, (uint64_t)n_cu * 32)), dim3(VC_FILTER_BLOCK), 0, s, a.d_scope,
                     (const uint32_t*)uniq, (const uint32_t*)n_slots, nq, v.n, nblocks, bits, rank);
  SCOPE_HIP(hipGetLastError());
  SCOPE_HIP(vc_exclusive_scan_u32(rank, rank, nblocks + 1, (uint32_t*)(kb + o_work), s));
  uint32_t U = 0, A = 0;
  SCOPE_HIP(hipMemcpyAsync(&U, n_slots, 4, hipMemcpyDeviceToHost, s));
  SCOPE_HIP(hipMemcpyAsync(&A, rank + nblocks, 4, hipMemcpyDeviceToHost, s));
  SCOPE_HIP(hipStreamSynchronize(s));
  if (U == 0 || U > nq || A > v.n) {
    if (err) *err = "scoped search: the query side or the keep set is out of range";
    return VC_ERR_HIP;
  }
  st.n_scopes = U;
  st.n_matched = A;
  if (A == 0) {
    SCOPE_HIP(pad_all());
    st.n_short = st.n_empty = nq;
    if (stats) *stats = st;
    return VC_OK;
  }
  // ---- 3. the order, the segments, and THE SECOND WAIT: seg and qrun
  const ListWork lw(A);
  uint8_t* lb = (uint8_t*)v.alloc(VC_SCOPE_LIST, lw.total);
  if (!lb) return VC_ERR_NOMEM;
  uint32_t* lkeys[2] = {(uint32_t*)(lb + lw.keys[0]), (uint32_t*)(lb + lw.keys[1])};
  uint32_t* lvals[2] = {(uint32_t*)(lb + lw.vals[0]), (uint32_t*)(lb + lw.vals[1])};
  const VcKeepSet ks{bits, rank, v.n, A};
  hipLaunchKernelGGL(vc_scope_list_kernel, dim3(grid_of(nwords)), dim3(SC_BLK), 0, s, ks, nwords, v.id_base, a.d_scope, (const uint32_t*)uniq, U, A, lkeys[0],
                     lvals[0]);
  SCOPE_HIP(hipGetLastError());
  const uint32_t key_bits = vc_scope_key_bits(U);
  int lres = 0;
  if (key_bits) {   // (U == 1: one slot, the list is in id order already)
    SCOPE_HIP(vc_radix_sort_pairs(lkeys, lvals, A, key_bits, (uint32_t*)(lb + lw.sort_work), s));
    lres = (int)(vc_radix_sort_passes(key_bits) & 1);
  }
  const uint32_t* sslots = lkeys[lres];
  const uint32_t* sids = lvals[lres];
  hipLaunchKernelGGL(vc_scope_segs_kernel, dim3(blocks_of((uint64_t)U + 1)), dim3(SC_BLK), 0, s, sslots, A, U, seg);
  SCOPE_HIP(hipGetLastError());
  hipLaunchKernelGGL(vc_scope_cost_kernel, dim3(blocks_of((uint64_t)nq + 1)), dim3(SC_BLK), 0, s, (const uint32_t*)qslot, (const uint32_t*)seg, nq, U, window,
                     len, coff);
  SCOPE_HIP(hipGetLastError());
  SCOPE_HIP(vc_exclusive_scan_u32(coff, coff, (uint64_t)nq + 1, (uint32_t*)(qb + qw.scan_work), s));
  std::vector<uint32_t> h_seg((size_t)U + 1), h_run((size_t)U + 1);
  SCOPE_HIP(hipMemcpyAsync(h_seg.data(), seg, ((size_t)U + 1) * 4, hipMemcpyDeviceToHost, s));
  SCOPE_HIP(hipMemcpyAsync(h_run.data(), qrun, ((size_t)U + 1) * 4, hipMemcpyDeviceToHost, s));
  SCOPE_HIP(hipStreamSynchronize(s));
  bool sane = h_seg[0] == 0 && h_seg[U] == A && h_run[0] == 0 && h_run[U] == nq;
  for (uint32_t u = 0; u < U && sane; ++u) sane = h_seg[u] <= h_seg[u + 1] && h_run[u] < h_run[u + 1];
  if (!sane) {
    if (err) *err = "scoped search: the segment table is not in order";
    return VC_ERR_HIP;
  }
  // the host's copy of the plan: segment and counters of every sorted query, the statistics
  std::vector<uint32_t> q_lo(nq), q_hi(nq), cost(nq);
  for (uint32_t u = 0; u < U; ++u)
    for (uint32_t j = h_run[u]; j < h_run[u + 1]; ++j) {
      q_lo[j] = h_seg[u];
      q_hi[j] = h_seg[u + 1];
      cost[j] = vc_scope_cost(q_lo[j], q_hi[j], window, len);
      const uint32_t S = q_hi[j] - q_lo[j];
      st.n_pairs += S;
      st.n_short += S < k;
      st.n_empty += S == 0;
    }
  // ---- 4. the scan: the sub-batches, their largest sizes first (one allocation each)
  std::vector<uint32_t> ends;
  uint32_t nb_max = 0, nc_max = 0;
  for (uint32_t b0 = 0; b0 < nq;) {
    const uint32_t b1 = vc_scope_batch_end(cost.data(), nq, b0, a.budget);
    uint64_t c = 0;
    for (uint32_t j = b0; j < b1; ++j) c += cost[j];
    if (c > 0xFFFFFFFFull) {
      if (err) *err = "scoped search: a query's counters exceed 2^32";
      return VC_ERR_INVALID;
    }
    nb_max = std::max(nb_max, b1 - b0);
    nc_max = std::max(nc_max, (uint32_t)c);
    ends.push_back(b1);
    b0 = b1;
  }
  const uint32_t wcap = std::min(A, window);
  const BatchWork bw(nb_max, std::max(nc_max, 1u), wcap, a.bits);
  const uint64_t rows_max = (uint64_t)nb_max * k;
  uint8_t* wb = (uint8_t*)v.alloc(VC_SCOPE_WORK, bw.total);
  uint64_t* rowbuf = (uint64_t*)v.alloc(VC_SCOPE_ROWS, 4 * rows_max * 8);   // cand | run | the merge's two lists
  uint64_t* codes = (uint64_t*)v.alloc(VC_SCOPE_CODES, (uint64_t)wcap * W * 8);
  if (!wb || !rowbuf || !codes) return VC_ERR_NOMEM;
  uint64_t* cand = rowbuf;
  uint64_t* run = rowbuf + rows_max;
  uint64_t* pair = rowbuf + 2 * rows_max;
  ScopeWalk wa{};
  wa.codes = codes; wa.window = window; wa.U = U; wa.qrun = qrun; wa.seg = seg; wa.qslot = qslot; wa.sq = sq; wa.coff = coff;
  wa.bits = a.bits; wa.k = k;
  wa.hist = (uint32_t*)(wb + bw.hist); wa.tau = (uint32_t*)(wb + bw.tau); wa.below = (uint32_t*)(wb + bw.below); wa.kk = (uint32_t*)(wb + bw.kk);
  wa.lt = (uint32_t*)(wb + bw.lt); wa.eq = (uint32_t*)(wb + bw.eq); wa.cand = cand;
  uint32_t* found = (uint32_t*)(wb + bw.found);
  uint32_t b0 = 0;
  for (const uint32_t b1 : ends) {
    const uint32_t nb = b1 - b0, plo = q_lo[b0], phi = q_hi[b1 - 1];
    uint64_t nc = 0;
    for (uint32_t j = b0; j < b1; ++j) nc += cost[j];
    wa.b0 = b0; wa.n_rows = nb; wa.n_counters = (uint32_t)nc;
    const uint32_t n_win = vc_scope_n_windows(plo, phi, window), w_first = vc_scope_first_window(plo, window);
    uint32_t j0 = b0;
    for (uint32_t wi = 0; wi < n_win; ++wi) {
      const uint32_t w0 = (w_first + wi) * window, wn = std::min(window, A - w0);
      // the sorted queries whose segment reaches into the window: [j0, j1); those before jm began in an earlier window
      while (j0 < b1 && q_hi[j0] <= w0) ++j0;
      uint32_t jm = j0;
      while (jm < b1 && q_lo[jm] < w0) ++jm;
      uint32_t j1 = jm;
      while (j1 < b1 && q_lo[j1] < w0 + wn) ++j1;
      const int rc = v.gather(sids + w0, wn, codes, found);
      if (rc) return rc;
      wa.ids = sids + w0; wa.pslot = sslots + w0; wa.n = wn; wa.w0 = w0; wa.j0 = j0; wa.j1 = j1;
      const uint32_t na = j1 - j0, r0 = j0 - b0;
      if (na) {
        SCOPE_HIP(hipMemsetAsync(wa.hist + (uint64_t)r0 * (a.bits + 1), 0, (size_t)na * (a.bits + 1) * 4, s));
        SCOPE_HIP(launch_walk(WALK_HIST, wa, W, s));
        hipLaunchKernelGGL(vc_scope_cut_kernel, dim3(blocks_of(na)), dim3(SC_BLK), 0, s, wa);
        SCOPE_HIP(hipGetLastError());
        SCOPE_HIP(launch_walk(WALK_COUNT, wa, W, s));
        hipLaunchKernelGGL(vc_scope_base_kernel, dim3((na + VC_FILTER_BLOCK_SLICES - 1) / VC_FILTER_BLOCK_SLICES), dim3(VC_FILTER_BLOCK), 0, s, wa, len);
        SCOPE_HIP(hipGetLastError());
        SCOPE_HIP(launch_walk(WALK_PLACE, wa, W, s));
        // the order of the kk entries: a segment that begins here gets its running row, one that began earlier is merged into it
        const uint32_t n_cont = jm - j0, n_new = j1 - jm, rm = jm - b0;
        SCOPE_HIP(vc_launch_select_ring(cand + (uint64_t)rm * k, k, wa.kk + rm, nullptr, 1, n_new, k, run + (uint64_t)rm * k, nullptr, s));
        if (n_cont) {
          const uint64_t words = (uint64_t)n_cont * k;
          SCOPE_HIP(hipMemcpyAsync(pair, run + (uint64_t)r0 * k, words * 8, hipMemcpyDeviceToDevice, s));
          SCOPE_HIP(vc_launch_select_ring(cand + (uint64_t)r0 * k, k, wa.kk + r0, nullptr, 1, n_cont, k, pair + words, nullptr, s));
          SCOPE_HIP(vc_launch_select_lists(pair, 2, n_cont, k, run + (uint64_t)r0 * k, nullptr, s));
        }
      }
      ++st.n_windows;
    }
    // ---- 5. the finish
    hipLaunchKernelGGL(vc_scope_emit_kernel, dim3(grid_of((uint64_t)nb * k)), dim3(SC_BLK), 0, s, (const uint64_t*)run, b0, nb, k, nq, svals, (const uint32_t*)qslot,
                       (const uint32_t*)seg, U, a.d_out, a.d_counts);
    SCOPE_HIP(hipGetLastError());
    b0 = b1;
  }
  if (stats) *stats = st;
  return VC_OK;
}

int vc_scope_run_host(const VcStoreView& v, const VcScopeHostArgs& a,
                      const std::function<int(const uint64_t* d_queries, const uint32_t* d_scope, const uint32_t* d_qscope, uint64_t* d_out, uint32_t* d_counts)>& run,
                      hipStream_t s, std::string* err) {
  const size_t qbytes = (size_t)a.nq * v.W * 8, obytes = (size_t)a.nq * a.k * 8, sbytes = up8((size_t)v.n * 4), cbytes = up8((size_t)a.nq * 4);
  uint8_t* stage = (uint8_t*)v.alloc(VC_SCOPE_STAGE, qbytes + obytes + sbytes + 2 * cbytes + 8);   // staged: queries | out | scope | qscope | counts
  if (!stage) return VC_ERR_NOMEM;
  uint64_t* d_q = (uint64_t*)stage;
  uint64_t* d_out = (uint64_t*)(stage + qbytes);
  uint32_t* d_scope = (uint32_t*)(stage + qbytes + obytes);
  uint32_t* d_qscope = (uint32_t*)(stage + qbytes + obytes + sbytes);
  uint32_t* d_cnt = (uint32_t*)(stage + qbytes + obytes + sbytes + cbytes);
  SCOPE_HIP(hipMemcpyAsync(d_q, a.queries, qbytes, hipMemcpyHostToDevice, s));
  if (v.n) SCOPE_HIP(hipMemcpyAsync(d_scope, a.scope, (size_t)v.n * 4, hipMemcpyHostToDevice, s));
  SCOPE_HIP(hipMemcpyAsync(d_qscope, a.qscope, (size_t)a.nq * 4, hipMemcpyHostToDevice, s));
  const int rc = run(d_q, d_scope, d_qscope, d_out, d_cnt);
  if (rc) return rc;
  std::vector<uint32_t> cnt(a.nq);
  SCOPE_HIP(hipMemcpyAsync(a.out, d_out, obytes, hipMemcpyDeviceToHost, s));
  SCOPE_HIP(hipMemcpyAsync(cnt.data(), d_cnt, (size_t)a.nq * 4, hipMemcpyDeviceToHost, s));
  SCOPE_HIP(hipStreamSynchronize(s));
  for (uint32_t i = 0; i < a.nq; ++i) {
    if (a.order == VC_ORDER_FARTHEST_FIRST) {
      uint64_t* row = a.out + (size_t)i * a.k;
      std::reverse(row, row + std::min(cnt[i], a.k));
    }
    if (a.counts) a.counts[i] = cnt[i];
  }
  return VC_OK;
}
