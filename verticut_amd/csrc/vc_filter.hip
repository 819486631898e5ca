// Filtered k-NN: vc_search_knn_filtered* and vc_sharded_search_knn_filtered* (the header states the contract).  One driver for both
// handle kinds over the view's k-NN search and by-id gather; the plan arithmetic is vc_filter_plan.hpp.
//
// THE KEEP SET.  sel becomes one bit per record and a rank directory per 256 bits (VcKeepSet, vc_retain.hpp): MASK and ROOTS through
// vc_launch_keep_bits as vc_retain* does, EQUAL, NOT_EQUAL and BITS through vc_filter_bits_kernel here.  One wait fetches A.
// POST-FILTER ROUTE (dense filters).  The rounds of vc_distinct.hip: the unchanged search at k' for the open queries, then
// vc_filter_strip_kernel -- one wave per query walks the row in steps of 64 and keeps the entries whose bit is set, placed by ballot
// and a running count.  A query is done with k kept entries or a row that was not full; else it is flagged, and the exclusive scan
// of the flags is the next round's list -- or, after k' = VC_MAX_K, the list the pre-filter route answers.
// PRE-FILTER ROUTE (sparse filters, the fallback): an exact brute-force top-k over the allowed records, window by window.  The ids of
// a window are listed ascending from bits + rank, their codes come through the view's gather as rows [n][W], and three walks over
// those rows give the kk = min(k, n) smallest (distance, list position) of every query:
//   walk 1  vc_filter_hist_kernel   distances counted per block in LDS, added to a global [nq][bits + 1] table (sums: order-free).
//                                   First over a prefix of the window, whose cut is an upper bound U of the kk-th distance; the
//                                   rest of the window then skips the LDS atomic above U -- on uniform data nearly every lane.
//           vc_filter_cut_kernel    tau = the smallest d whose cumulative count reaches kk, below = the count under tau
//   walk 2  vc_filter_count_kernel  per (query, wave-slice) the entries with d < tau and with d == tau;
//           vc_filter_base_kernel   turns them into exclusive bases along the slices of a query
//   walk 3  vc_filter_place_kernel  d < tau goes to base_lt + its ballot rank, d == tau to below + base_eq + its ballot rank while
//                                   that is below kk: exactly kk entries per query, ties to the smaller list position = smaller id.
// The data flow of the walks is vc_assign.hip's: a lane holds vc_filter_steps(W) gathered codes in registers, a tile of queries sits
// in LDS and every lane reads the SAME address (a broadcast), so a pair costs XOR + v_bcnt per 64-bit word.  A wave owns a
// contiguous slice of the window, hence lane order within a step is list order.  vc_launch_select_ring orders the kk entries;
// the rows of a further window are merged into the running rows by vc_launch_select_lists.  Blocks meet in the next launch only.
// No address is formed from data but through a bounds test: row entries are range-checked before their bit is read, placement
// positions are tested against kk.
#include <algorithm>

#include "vc_filter_plan.hpp"
#include "vc_internal.hpp"
#include "vc_retain.hpp"

static_assert(VC_FILTER_MAX_K == VC_MAX_K, "the plan's widest row is the search's");
static_assert(VC_FILTER_ROUTE_POST == VC_FILTER_RAN_POST && VC_FILTER_ROUTE_PRE == VC_FILTER_RAN_PRE, "the plan's routes are the header's flags");
static_assert(VC_FILTER_KINDS == VC_FILTER_BITS + 1, "the plan's kinds are the header's");
static_assert(VC_FILTER_BLOCK == VC_WAVE * VC_FILTER_BLOCK_SLICES, "a wave per slice");

namespace {

// ---- the keep set of EQUAL, NOT_EQUAL and BITS: one block per 256-bit keep block, one ballot per wave makes one word, the four
// popcounts meet in LDS.  Block `nblocks` of the rank array gets 0, so that the exclusive scan over nblocks + 1 entries ends in A.
__global__ void __launch_bounds__(VC_FILTER_BLOCK) vc_filter_bits_kernel(const uint32_t* __restrict__ sel, uint32_t kind, uint32_t value, uint64_t n,
                                                                         uint64_t nblocks, uint64_t* __restrict__ bits, uint32_t* __restrict__ pop) {
  __shared__ uint32_t wpop[VC_FILTER_BLOCK_SLICES];
  const uint32_t lane = vc_lane(), wave = threadIdx.x / VC_WAVE;
  for (uint64_t b = blockIdx.x; b <= nblocks; b += gridDim.x) {   // (block-uniform)
    if (b == nblocks) {
      if (threadIdx.x == 0) pop[b] = 0u;
      break;
    }
    const uint64_t i = b * VC_KEEP_BLOCK_BITS + threadIdx.x;
    bool keep = false;
    if (i < n) {
      if (kind == VC_FILTER_EQUAL) keep = sel[i] == value;
      else if (kind == VC_FILTER_NOT_EQUAL) keep = sel[i] != value;
      else keep = (sel[i >> 5] >> (i & 31u)) & 1u;   // VC_FILTER_BITS: word i >> 5 exists for every i < n
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

// ---- the post-filter route ------------------------------------------------------------------------------------------------------------
struct StripArgs {
  const uint64_t* rows;      // [n][kp]
  const uint32_t* cnt;       // [n]
  uint32_t n, kp, k;
  uint32_t tie_cut;          // exact MIH underneath: only the sure prefix of a full row counts (vc_filter_sure_below)
  const uint64_t* bits;      // the keep set
  uint64_t n_records;
  uint32_t id_base;
  const uint32_t* map;       // [n] compact row -> the caller's query; null: first + row
  uint32_t first;
  uint64_t* out;             // [nq][k]
  uint32_t* counts;          // [nq], nullable
  uint32_t* flag;            // [n]
};

__global__ void __launch_bounds__(VC_FILTER_BLOCK) vc_filter_strip_kernel(const StripArgs a) {
  const uint32_t row = blockIdx.x * VC_FILTER_BLOCK_SLICES + threadIdx.x / VC_WAVE;   // wave-uniform
  if (row >= a.n) return;
  const uint32_t lane = vc_lane();
  const uint32_t cnt = a.cnt[row], m = vc_filter_row_entries(cnt, a.kp);
  const uint32_t last = a.tie_cut && cnt == a.kp ? (uint32_t)(a.rows[(uint64_t)row * a.kp + a.kp - 1] >> 32) : 0u;
  const uint32_t below = vc_filter_sure_below(a.tie_cut != 0, cnt, a.kp, last);
  const uint32_t oq = a.map ? a.map[row] : a.first + row;
  uint64_t* out = a.out + (uint64_t)oq * a.k;
  uint32_t kept = 0;   // wave-uniform
  for (uint32_t j0 = 0; j0 < m && kept < a.k; j0 += VC_WAVE) {
    const uint32_t j = j0 + lane;
    uint64_t v = VC_PACK_INF;
    bool ok = false;
    if (j < m) {
      v = a.rows[(uint64_t)row * a.kp + j];
      const uint32_t i = (uint32_t)v - a.id_base;
      ok = (uint32_t)(v >> 32) < below && i < a.n_records && ((a.bits[i >> 6] >> (i & 63u)) & 1ull);   // (an empty entry is at distance 0xFFFFFFFF)
    }
    const unsigned long long mask = __ballot(ok);
    const uint32_t pos = kept + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (ok && pos < a.k) out[pos] = v;   // (a row that is retried is written again by the round that finishes it)
    kept += (uint32_t)__popcll(mask);
  }
  const VcFilterVerdict vd = vc_filter_verdict(kept, cnt, a.kp, a.k);
  const bool open = vd.status == VC_FILTER_RETRY || vd.status == VC_FILTER_FALLBACK;
  if (lane == 0) {
    a.flag[row] = open ? 1u : 0u;
    if (!open && a.counts) a.counts[oq] = vd.count;
  }
  if (open) return;
  for (uint32_t j = vd.written + lane; j < a.k; j += VC_WAVE) out[j] = VC_PACK_INF;
}

// the list of the flagged rows: row r with flag[r] goes to place scanned[r]; its query's code is gathered from the caller's batch.
// The last thread leaves the length of the list in *n_next.
__global__ void __launch_bounds__(256) vc_filter_gather_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ scanned, uint32_t n,
                                                               const uint32_t* __restrict__ map, const uint64_t* __restrict__ queries, uint32_t W,
                                                               uint32_t* __restrict__ map_next, uint64_t* __restrict__ q_next, uint32_t* __restrict__ n_next) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const uint32_t f = flag[r], at = scanned[r];
  if (r == n - 1) *n_next = at + f;
  if (!f) return;
  const uint32_t oq = map ? map[r] : r;
  map_next[at] = oq;
  for (uint32_t w = 0; w < W; ++w) q_next[(uint64_t)at * W + w] = queries[(uint64_t)oq * W + w];
}

// out rows [n][k] through the map: padded rows and count 0 (rows null), or the running rows of the pre-filter route and count kk
__global__ void __launch_bounds__(256) vc_filter_emit_kernel(const uint64_t* __restrict__ rows, uint32_t n, uint32_t k, uint32_t count,
                                                             const uint32_t* __restrict__ map, uint32_t first, uint64_t* __restrict__ out,
                                                             uint32_t* __restrict__ counts) {
  const uint64_t total = (uint64_t)n * k;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = (uint32_t)(e / k), j = (uint32_t)(e % k);
    const uint32_t oq = map ? map[r] : first + r;
    out[(uint64_t)oq * k + j] = rows ? rows[e] : VC_PACK_INF;
    if (j == 0 && counts) counts[oq] = count;
  }
}

// ---- the pre-filter route -------------------------------------------------------------------------------------------------------------
// the allowed ids of list positions [w0, w0 + wn), ascending: one thread per 64-bit word of the keep set
__global__ void __launch_bounds__(256) vc_filter_list_kernel(const VcKeepSet ks, uint64_t nwords, uint32_t id_base, uint64_t w0, uint32_t wn,
                                                             uint32_t* __restrict__ ids) {
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nwords; j += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t word = ks.bits[j];
    if (!word) continue;
    uint64_t r = vc_keep_rank(ks, (uint32_t)(j << 6));   // set bits before this word
    if (r >= w0 + wn || r + (uint64_t)__popcll(word) <= w0) continue;
    while (word) {
      const uint32_t b = (uint32_t)__ffsll((unsigned long long)word) - 1u;
      word &= word - 1;
      if (r >= w0 && r < w0 + wn) ids[r - w0] = id_base + (uint32_t)(j << 6) + b;
      ++r;
    }
  }
}

// what the three walks share: the window, the sub-batch and where a block stands in them
struct WalkArgs {
  const uint64_t* codes;     // [n][W] the gathered rows of the window
  const uint32_t* ids;       // [n] their ids
  uint32_t n;                // positions of the window
  uint32_t n_slices;         // vc_filter_n_slices(n, W)
  uint32_t slice0, slice1;   // the slices [slice0, slice1) this launch walks
  const uint64_t* queries;   // [nq][W] of the sub-batch
  uint32_t nq, bits, k;
  const uint32_t* bound;     // walk 1: [nq] distances above are not counted; null: all are
  uint32_t* hist;            // [nq][bits + 1]
  const uint32_t* tau;       // [nq]
  const uint32_t* below;     // [nq]
  const uint32_t* kk;        // [nq] entries the row gets: min(k, n)
  uint32_t* lt;              // [nq][n_slices] counts, then exclusive bases, of d < tau
  uint32_t* eq;              // the same of d == tau
  uint64_t* cand;            // [nq][k]
};

// the codes (and the mask of the steps that hold one) of this lane in its wave's slice; a wave past the launch's slices holds none
template <int W, int R>
__device__ __forceinline__ uint32_t load_slice(const WalkArgs& a, uint32_t slice, uint32_t lane, uint64_t (&rec)[R][W]) {
  uint32_t valid = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t p = vc_filter_position(W, slice, r, lane);
    const bool in = slice < a.slice1 && p < a.n;
    valid |= (in ? 1u : 0u) << r;
#pragma unroll
    for (int w = 0; w < W; ++w) rec[r][w] = in ? a.codes[(uint64_t)p * W + w] : 0ull;
  }
  return valid;
}
template <int W>
__device__ __forceinline__ uint32_t pair_dist(const uint64_t (&x)[W], const uint64_t (&y)[W]) {
  uint32_t d = 0;
#pragma unroll
  for (int w = 0; w < W; ++w) d += (uint32_t)__builtin_popcountll(x[w] ^ y[w]);
  return d;
}

// WALK 1.  Dynamic LDS: VC_FILTER_QTILE histograms of bits + 1 words.
template <int W>
__global__ void __launch_bounds__(VC_FILTER_BLOCK) vc_filter_hist_kernel(const WalkArgs a) {
  constexpr int R = (int)vc_filter_steps(W);
  extern __shared__ uint32_t hl[];                     // [QTILE][bits + 1]
  __shared__ uint64_t ql[VC_FILTER_QTILE * W];
  __shared__ uint32_t ub[VC_FILTER_QTILE];
  const uint32_t lane = vc_lane(), slice = a.slice0 + blockIdx.x * VC_FILTER_BLOCK_SLICES + threadIdx.x / VC_WAVE, B = a.bits + 1;
  uint64_t rec[R][W];
  const uint32_t valid = load_slice<W, R>(a, slice, lane, rec);
  const uint32_t tiles = (a.nq + VC_FILTER_QTILE - 1) / VC_FILTER_QTILE;
  for (uint32_t t = blockIdx.y; t < tiles; t += gridDim.y) {   // (block-uniform)
    const uint32_t q0 = t * VC_FILTER_QTILE, nt = min(VC_FILTER_QTILE, a.nq - q0);
    __syncthreads();   // (the previous tile has been flushed)
    for (uint32_t j = threadIdx.x; j < nt * (uint32_t)W; j += VC_FILTER_BLOCK) ql[j] = a.queries[(uint64_t)q0 * W + j];
    for (uint32_t j = threadIdx.x; j < nt; j += VC_FILTER_BLOCK) ub[j] = a.bound ? a.bound[q0 + j] : 0xFFFFFFFFu;
    for (uint32_t j = threadIdx.x; j < nt * B; j += VC_FILTER_BLOCK) hl[j] = 0u;
    __syncthreads();
    for (uint32_t c = 0; c < nt; ++c) {
      uint64_t cw[W];
#pragma unroll
      for (int w = 0; w < W; ++w) cw[w] = ql[c * W + w];
      const uint32_t u = ub[c];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint32_t d = pair_dist<W>(rec[r], cw);   // d <= bits
        if (((valid >> r) & 1u) && d <= u) atomicAdd(&hl[c * B + d], 1u);
      }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < nt * B; j += VC_FILTER_BLOCK) {
      const uint32_t v = hl[j];
      if (v) atomicAdd(&a.hist[(uint64_t)q0 * B + j], v);
    }
  }
}

// tau, below and kk of every query from its histogram; dst_tau is the bound of the second hist launch or the final tau
__global__ void __launch_bounds__(256) vc_filter_cut_kernel(const uint32_t* __restrict__ hist, uint32_t nq, uint32_t bits, uint32_t kk,
                                                            uint32_t* __restrict__ dst_tau, uint32_t* __restrict__ dst_below, uint32_t* __restrict__ dst_kk) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  uint32_t tau, below;
  vc_filter_cut(hist + (uint64_t)q * (bits + 1), bits, kk, &tau, &below);
  dst_tau[q] = tau;
  if (dst_below) dst_below[q] = below;
  if (dst_kk) dst_kk[q] = kk;
}

// WALK 2
template <int W>
__global__ void __launch_bounds__(VC_FILTER_BLOCK) vc_filter_count_kernel(const WalkArgs a) {
  constexpr int R = (int)vc_filter_steps(W);
  __shared__ uint64_t ql[VC_FILTER_QTILE * W];
  __shared__ uint32_t tl[VC_FILTER_QTILE];
  const uint32_t lane = vc_lane(), slice = a.slice0 + blockIdx.x * VC_FILTER_BLOCK_SLICES + threadIdx.x / VC_WAVE;
  uint64_t rec[R][W];
  const uint32_t valid = load_slice<W, R>(a, slice, lane, rec);
  const uint32_t tiles = (a.nq + VC_FILTER_QTILE - 1) / VC_FILTER_QTILE;
  for (uint32_t t = blockIdx.y; t < tiles; t += gridDim.y) {
    const uint32_t q0 = t * VC_FILTER_QTILE, nt = min(VC_FILTER_QTILE, a.nq - q0);
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < nt * (uint32_t)W; j += VC_FILTER_BLOCK) ql[j] = a.queries[(uint64_t)q0 * W + j];
    for (uint32_t j = threadIdx.x; j < nt; j += VC_FILTER_BLOCK) tl[j] = a.tau[q0 + j];
    __syncthreads();
    if (slice >= a.slice1) continue;   // (wave-uniform; the barriers above are met by every wave)
    for (uint32_t c = 0; c < nt; ++c) {
      uint64_t cw[W];
#pragma unroll
      for (int w = 0; w < W; ++w) cw[w] = ql[c * W + w];
      const uint32_t tau = tl[c];
      uint32_t n_lt = 0, n_eq = 0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint32_t d = pair_dist<W>(rec[r], cw);
        const bool in = (valid >> r) & 1u;
        n_lt += (uint32_t)__popcll(__ballot(in && d < tau));
        n_eq += (uint32_t)__popcll(__ballot(in && d == tau));
      }
      if (lane == 0) {
        a.lt[(uint64_t)(q0 + c) * a.n_slices + slice] = n_lt;
        a.eq[(uint64_t)(q0 + c) * a.n_slices + slice] = n_eq;
      }
    }
  }
}

// the counts of a query along its slices -> exclusive bases, in place: one wave per query
__global__ void __launch_bounds__(VC_FILTER_BLOCK) vc_filter_base_kernel(uint32_t* __restrict__ lt, uint32_t* __restrict__ eq, uint32_t nq, uint32_t n_slices) {
  const uint32_t q = blockIdx.x * VC_FILTER_BLOCK_SLICES + threadIdx.x / VC_WAVE, lane = vc_lane();
  if (q >= nq) return;
  uint32_t* l = lt + (uint64_t)q * n_slices;
  uint32_t* e = eq + (uint64_t)q * n_slices;
  uint32_t cl = 0, ce = 0;   // wave-uniform carries
  for (uint32_t s0 = 0; s0 < n_slices; s0 += VC_WAVE) {
    const uint32_t s = s0 + lane;
    const uint32_t vl = s < n_slices ? l[s] : 0u, ve = s < n_slices ? e[s] : 0u;
    uint32_t tl, te;
    const uint32_t xl = vc_wave_excl_scan(vl, tl), xe = vc_wave_excl_scan(ve, te);
    if (s < n_slices) {
      l[s] = cl + xl;
      e[s] = ce + xe;
    }
    cl += tl;
    ce += te;
  }
}

// WALK 3
template <int W>
__global__ void __launch_bounds__(VC_FILTER_BLOCK) vc_filter_place_kernel(const WalkArgs a) {
  constexpr int R = (int)vc_filter_steps(W);
  __shared__ uint64_t ql[VC_FILTER_QTILE * W];
  __shared__ uint32_t tl[VC_FILTER_QTILE], bl[VC_FILTER_QTILE], kl[VC_FILTER_QTILE];
  const uint32_t lane = vc_lane(), slice = a.slice0 + blockIdx.x * VC_FILTER_BLOCK_SLICES + threadIdx.x / VC_WAVE;
  uint64_t rec[R][W];
  uint32_t id[R];
  const uint32_t valid = load_slice<W, R>(a, slice, lane, rec);
#pragma unroll
  for (int r = 0; r < R; ++r) id[r] = ((valid >> r) & 1u) ? a.ids[vc_filter_position(W, slice, r, lane)] : 0u;
  const unsigned long long lower = (1ull << lane) - 1ull;
  const uint32_t tiles = (a.nq + VC_FILTER_QTILE - 1) / VC_FILTER_QTILE;
  for (uint32_t t = blockIdx.y; t < tiles; t += gridDim.y) {
    const uint32_t q0 = t * VC_FILTER_QTILE, nt = min(VC_FILTER_QTILE, a.nq - q0);
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < nt * (uint32_t)W; j += VC_FILTER_BLOCK) ql[j] = a.queries[(uint64_t)q0 * W + j];
    for (uint32_t j = threadIdx.x; j < nt; j += VC_FILTER_BLOCK) {
      tl[j] = a.tau[q0 + j];
      bl[j] = a.below[q0 + j];
      kl[j] = a.kk[q0 + j];
    }
    __syncthreads();
    if (slice >= a.slice1) continue;
    for (uint32_t c = 0; c < nt; ++c) {
      uint64_t cw[W];
#pragma unroll
      for (int w = 0; w < W; ++w) cw[w] = ql[c * W + w];
      const uint32_t tau = tl[c], kk = min(kl[c], a.k);
      uint32_t at_lt = a.lt[(uint64_t)(q0 + c) * a.n_slices + slice];          // wave-uniform
      uint32_t at_eq = bl[c] + a.eq[(uint64_t)(q0 + c) * a.n_slices + slice];
      uint64_t* row = a.cand + (uint64_t)(q0 + c) * a.k;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint32_t d = pair_dist<W>(rec[r], cw);
        const bool in = (valid >> r) & 1u, is_lt = in && d < tau, is_eq = in && d == tau;
        const unsigned long long m_lt = __ballot(is_lt), m_eq = __ballot(is_eq);
        const uint32_t p_lt = at_lt + (uint32_t)__popcll(m_lt & lower), p_eq = at_eq + (uint32_t)__popcll(m_eq & lower);
        if (is_lt && p_lt < kk) row[p_lt] = vc_pack(d, id[r]);   // (below < kk: the test never fails; it keeps the store inside the row)
        if (is_eq && p_eq < kk) row[p_eq] = vc_pack(d, id[r]);
        at_lt += (uint32_t)__popcll(m_lt);
        at_eq += (uint32_t)__popcll(m_eq);
      }
    }
  }
}

int filter_fail(std::string* err, hipError_t r, const char* what) { return vc_hip_fail(err, "filtered search", r, what); }
#define FILTER_HIP(call)                                       \
  do {                                                         \
    hipError_t _r = (call);                                    \
    if (_r != hipSuccess) return filter_fail(err, _r, #call);  \
  } while (0)

template <class F>
hipError_t dispatch_words(uint32_t W, F&& f) {
  switch (W) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
  }
  return hipErrorInvalidValue;
}

enum { WALK_HIST = 0, WALK_COUNT = 1, WALK_PLACE = 2 };
hipError_t launch_walk(int which, const WalkArgs& a, uint32_t W, hipStream_t s) {
  if (a.slice1 <= a.slice0 || a.nq == 0) return hipSuccess;
  const uint32_t gx = vc_filter_scan_blocks(a.slice1 - a.slice0), gy = vc_filter_scan_grid_y(gx, a.nq);
  return dispatch_words(W, [&](auto w) {
    constexpr int Wc = decltype(w)::value;
    if (which == WALK_HIST)
      hipLaunchKernelGGL((vc_filter_hist_kernel<Wc>), dim3(gx, gy), dim3(VC_FILTER_BLOCK), (size_t)VC_FILTER_QTILE * (a.bits + 1) * 4, s, a);
    else if (which == WALK_COUNT)
      hipLaunchKernelGGL((vc_filter_count_kernel<Wc>), dim3(gx, gy), dim3(VC_FILTER_BLOCK), 0, s, a);
    else
      hipLaunchKernelGGL((vc_filter_place_kernel<Wc>), dim3(gx, gy), dim3(VC_FILTER_BLOCK), 0, s, a);
    return hipGetLastError();
  });
}

uint32_t small_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + 255) / 256, 1), 4096); }
inline uint64_t up8(uint64_t x) { return (x + 7) & ~7ull; }

// the scratch of the rounds beside the rows (VC_FILTER_WORK), in bytes: the length of the next list | flag [nq] | scanned [nq] | the
// scan's work | two index maps [nq] | counts of a sub-batch [nq] | the listed queries [nq][W].  Every word is written before it is
// read: flag by every strip launch, scanned and the work by the scan, the next map, the listed queries and the length by the gather.
struct RoundWork {
  uint64_t n_next, flag, scanned, scan_work, map[2], cnt, q, total;
  RoundWork(uint32_t nq, uint32_t W) {
    const uint64_t row4 = up8((uint64_t)nq * 4);
    uint64_t o = 0;
    n_next = o;     o += 8;
    flag = o;       o += row4;
    scanned = o;    o += row4;
    scan_work = o;  o += up8(vc_scan_work_words(nq) * 4);
    map[0] = o;     o += row4;
    map[1] = o;     o += row4;
    cnt = o;        o += row4;
    q = o;          o += (uint64_t)nq * W * 8;
    total = o;
  }
};

// the scratch of the pre-filter route (VC_FILTER_PRE) for sub-batches of nb queries and windows of at most wcap positions in at most
// `slices` slices: ids and found words of a window | hist | tau, below, kk, bound [nb] | lt, eq [nb][slices] | cand [nb][k] | the two
// lists [2][nb][k] | merged [nb][k].  hist is zeroed per window; the walks write the rest before the next launch reads it.
struct PreWork {
  uint64_t ids, found, hist, tau, below, kk, bound, lt, eq, cand, lists, merged, total;
  PreWork(uint32_t nb, uint32_t wcap, uint32_t slices, uint32_t bits, uint32_t k) {
    const uint64_t row4 = up8((uint64_t)nb * 4), rows = (uint64_t)nb * k * 8;
    uint64_t o = 0;
    ids = o;     o += up8((uint64_t)wcap * 4);
    found = o;   o += up8((uint64_t)wcap * 4);
    hist = o;    o += up8((uint64_t)nb * (bits + 1) * 4);
    tau = o;     o += row4;
    below = o;   o += row4;
    kk = o;      o += row4;
    bound = o;   o += row4;
    lt = o;      o += up8((uint64_t)nb * slices * 4);
    eq = o;      o += up8((uint64_t)nb * slices * 4);
    cand = o;    o += rows;
    lists = o;   o += 2 * rows;
    merged = o;  o += rows;
    total = o;
  }
};

struct Keep {
  VcKeepSet ks;
  uint64_t nwords;
};

// THE PRE-FILTER ROUTE for n queries q [n][W] whose rows go to out through map (null: query i is row i)
int pre_run(const VcStoreView& v, const VcFilterArgs& a, const Keep& keep, const uint64_t* q, const uint32_t* map, uint32_t n, vc_filter_stats* st, hipStream_t s,
            std::string* err) {
  const uint64_t A = keep.ks.k;
  const uint32_t W = v.W, window = vc_filter_window(a.window), wcap = (uint32_t)std::min<uint64_t>(A, window);
  const uint64_t n_windows = vc_filter_n_windows(A, window);
  const uint32_t max_slices = vc_filter_n_slices(wcap, W), nb_max = vc_filter_pre_batch(a.budget, max_slices, n);
  const PreWork wp(nb_max, wcap, max_slices, a.bits, a.k);
  uint8_t* work = (uint8_t*)v.alloc(VC_FILTER_PRE, wp.total);
  uint64_t* codes = (uint64_t*)v.alloc(VC_FILTER_CODES, (uint64_t)wcap * W * 8);
  if (!work || !codes) return VC_ERR_NOMEM;
  uint32_t* ids = (uint32_t*)(work + wp.ids);
  uint32_t* found = (uint32_t*)(work + wp.found);
  uint32_t* hist = (uint32_t*)(work + wp.hist);
  uint32_t* tau = (uint32_t*)(work + wp.tau);
  uint32_t* below = (uint32_t*)(work + wp.below);
  uint32_t* kkw = (uint32_t*)(work + wp.kk);
  uint32_t* bound = (uint32_t*)(work + wp.bound);
  uint32_t* lt = (uint32_t*)(work + wp.lt);
  uint32_t* eq = (uint32_t*)(work + wp.eq);
  uint64_t* cand = (uint64_t*)(work + wp.cand);
  uint64_t* lists = (uint64_t*)(work + wp.lists);
  uint64_t* merged = (uint64_t*)(work + wp.merged);
  const uint32_t count = (uint32_t)std::min<uint64_t>(a.k, A);
  for (uint32_t first = 0; first < n; first += nb_max) {
    const uint32_t nb = std::min(nb_max, n - first);
    const uint64_t rows = (uint64_t)nb * a.k;
    for (uint64_t w = 0; w < n_windows; ++w) {
      const uint32_t wn = vc_filter_window_len(A, window, w), n_slices = vc_filter_n_slices(wn, W), kk = std::min(a.k, wn);
      hipLaunchKernelGGL(vc_filter_list_kernel, dim3(small_grid(keep.nwords)), dim3(256), 0, s, keep.ks, keep.nwords, v.id_base, w * window, wn, ids);
      FILTER_HIP(hipGetLastError());
      const int rc = v.gather(ids, wn, codes, found);
      if (rc) return rc;
      WalkArgs wa{};
      wa.codes = codes; wa.ids = ids; wa.n = wn; wa.n_slices = n_slices;
      wa.queries = q + (uint64_t)first * W; wa.nq = nb; wa.bits = a.bits; wa.k = a.k;
      wa.hist = hist; wa.tau = tau; wa.below = below; wa.kk = kkw; wa.lt = lt; wa.eq = eq; wa.cand = cand;
      // walk 1: the prefix without a bound, its cut, the rest under that bound, the cut of the whole
      FILTER_HIP(hipMemsetAsync(hist, 0, (size_t)nb * (a.bits + 1) * 4, s));
      const uint32_t s_sample = vc_filter_sample_slices(wn, W, kk);
      wa.slice0 = 0; wa.slice1 = s_sample; wa.bound = nullptr;
      FILTER_HIP(launch_walk(WALK_HIST, wa, W, s));
      if (s_sample < n_slices) {
        hipLaunchKernelGGL(vc_filter_cut_kernel, dim3((nb + 255) / 256), dim3(256), 0, s, (const uint32_t*)hist, nb, a.bits, kk, bound, (uint32_t*)nullptr,
                           (uint32_t*)nullptr);
        FILTER_HIP(hipGetLastError());
        wa.slice0 = s_sample; wa.slice1 = n_slices; wa.bound = bound;
        FILTER_HIP(launch_walk(WALK_HIST, wa, W, s));
      }
      hipLaunchKernelGGL(vc_filter_cut_kernel, dim3((nb + 255) / 256), dim3(256), 0, s, (const uint32_t*)hist, nb, a.bits, kk, tau, below, kkw);
      FILTER_HIP(hipGetLastError());
      // walk 2 and the bases, walk 3, the order of the kk entries
      wa.slice0 = 0; wa.slice1 = n_slices; wa.bound = nullptr;
      FILTER_HIP(launch_walk(WALK_COUNT, wa, W, s));
      hipLaunchKernelGGL(vc_filter_base_kernel, dim3((nb + VC_FILTER_BLOCK_SLICES - 1) / VC_FILTER_BLOCK_SLICES), dim3(VC_FILTER_BLOCK), 0, s, lt, eq, nb, n_slices);
      FILTER_HIP(hipGetLastError());
      FILTER_HIP(launch_walk(WALK_PLACE, wa, W, s));
      uint64_t* dst = w == 0 ? lists : lists + rows;
      FILTER_HIP(vc_launch_select_ring(cand, a.k, kkw, nullptr, 1, nb, a.k, dst, nullptr, s));
      if (w > 0) {   // the window's rows into the running rows
        FILTER_HIP(vc_launch_select_lists(lists, 2, nb, a.k, merged, nullptr, s));
        FILTER_HIP(hipMemcpyAsync(lists, merged, rows * 8, hipMemcpyDeviceToDevice, s));
      }
      ++st->n_windows;
    }
    hipLaunchKernelGGL(vc_filter_emit_kernel, dim3(small_grid(rows)), dim3(256), 0, s, (const uint64_t*)lists, nb, a.k, count, map ? map + first : nullptr, first,
                       a.d_out, a.d_counts);
    FILTER_HIP(hipGetLastError());
  }
  st->routes |= VC_FILTER_RAN_PRE;
  return VC_OK;
}

}  // namespace

int vc_filter_run(const VcStoreView& v, const VcFilterArgs& a, vc_filter_stats* stats, hipStream_t s, std::string* err) {
  if (stats) *stats = vc_filter_stats{};
  vc_filter_stats st{};
  const auto pad_all = [&]() {
    hipLaunchKernelGGL(vc_filter_emit_kernel, dim3(small_grid((uint64_t)a.nq * a.k)), dim3(256), 0, s, (const uint64_t*)nullptr, a.nq, a.k, 0u,
                       (const uint32_t*)nullptr, 0u, a.d_out, a.d_counts);
    return hipGetLastError();
  };
  if (v.n == 0) {
    FILTER_HIP(pad_all());
    return VC_OK;
  }
  // ---- the keep set and A: the one wait before the plan
  int dev = 0, n_cu = 0;
  FILTER_HIP(hipGetDevice(&dev));
  FILTER_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
  const uint64_t nblocks = vc_keep_blocks(v.n), nwords = nblocks * VC_KEEP_BLOCK_WORDS;
  const uint64_t o_rank = nwords * 8, o_work = o_rank + up8((nblocks + 1) * 4), keep_bytes = o_work + up8(vc_scan_work_words(nblocks + 1) * 4);
  uint8_t* kb = (uint8_t*)v.alloc(VC_FILTER_KEEP, keep_bytes);
  if (!kb) return VC_ERR_NOMEM;
  uint64_t* bits = (uint64_t*)kb;
  uint32_t* rank = (uint32_t*)(kb + o_rank);
  uint32_t* scan_w = (uint32_t*)(kb + o_work);
  if (a.kind == VC_FILTER_MASK || a.kind == VC_FILTER_ROOTS) {
    FILTER_HIP(vc_launch_keep_bits(a.d_sel, a.kind == VC_FILTER_MASK ? VC_RETAIN_MASK : VC_RETAIN_ROOTS, v.id_base, 0, v.n, bits, rank, scan_w, (uint32_t)n_cu, s));
  } else {
    hipLaunchKernelGGL(vc_filter_bits_kernel, dim3((uint32_t)std::min<uint64_t>(nblocks + 1, (uint64_t)n_cu * 32)), dim3(VC_FILTER_BLOCK), 0, s, a.d_sel, a.kind,
                       a.value, v.n, nblocks, bits, rank);
    FILTER_HIP(hipGetLastError());
    FILTER_HIP(vc_exclusive_scan_u32(rank, rank, nblocks + 1, scan_w, s));
  }
  uint32_t A32 = 0;
  FILTER_HIP(hipMemcpyAsync(&A32, rank + nblocks, 4, hipMemcpyDeviceToHost, s));
  FILTER_HIP(hipStreamSynchronize(s));
  const uint64_t A = A32;
  if (A > v.n) {
    if (err) *err = "filtered search: the keep set counts more records than the store holds";
    return VC_ERR_HIP;
  }
  st.n_allowed = A;
  st.n_short = A < a.k ? a.nq : 0;
  if (A == 0) {
    FILTER_HIP(pad_all());
    if (stats) *stats = st;
    return VC_OK;
  }
  const Keep keep{VcKeepSet{bits, rank, v.n, A}, nwords};
  if (vc_filter_route(a.k, v.n, A, a.route) == VC_FILTER_ROUTE_PRE) {
    const int rc = pre_run(v, a, keep, a.d_queries, nullptr, a.nq, &st, s, err);
    if (rc) return rc;
    if (stats) *stats = st;
    return VC_OK;
  }
  // ---- THE ROUNDS.  Per round: the search underneath and the strip, sub-batch by sub-batch; the scan of the flags and the gather;
  // then the one wait, for the length of the list.
  const RoundWork wp(a.nq, v.W);
  uint8_t* work = (uint8_t*)v.alloc(VC_FILTER_WORK, wp.total);
  if (!work) return VC_ERR_NOMEM;
  uint32_t* n_next = (uint32_t*)(work + wp.n_next);
  uint32_t* flag = (uint32_t*)(work + wp.flag);
  uint32_t* scanned = (uint32_t*)(work + wp.scanned);
  uint32_t* scan_work = (uint32_t*)(work + wp.scan_work);
  uint32_t* maps[2] = {(uint32_t*)(work + wp.map[0]), (uint32_t*)(work + wp.map[1])};
  uint32_t* cnt = (uint32_t*)(work + wp.cnt);
  uint64_t* q_next = (uint64_t*)(work + wp.q);
  st.routes |= VC_FILTER_RAN_POST;
  const uint64_t* q = a.d_queries;   // round 0: the caller's batch, identity map
  const uint32_t* map = nullptr;
  uint32_t n = a.nq, kp = vc_filter_first_k(a.k, a.k_first, v.n, A);
  for (uint32_t round = 0;; ++round) {
    const uint32_t batch = vc_filter_batch(a.budget, kp);
    uint64_t* rows = (uint64_t*)v.alloc(VC_FILTER_ROWS, vc_filter_rows_bytes(n, a.budget, kp));
    if (!rows) return VC_ERR_NOMEM;
    for (uint32_t first = 0; first < n; first += batch) {
      const uint32_t nb = std::min(batch, n - first);
      const int rc = v.knn(q + (uint64_t)first * v.W, nb, kp, rows, cnt, nullptr);
      if (rc) return rc;
      StripArgs c{};
      c.rows = rows; c.cnt = cnt; c.n = nb; c.kp = kp; c.k = a.k; c.tie_cut = a.tie_cut ? 1u : 0u;
      c.bits = bits; c.n_records = v.n; c.id_base = v.id_base;
      c.map = map ? map + first : nullptr; c.first = first;
      c.out = a.d_out; c.counts = a.d_counts; c.flag = flag + first;
      hipLaunchKernelGGL(vc_filter_strip_kernel, dim3((nb + VC_FILTER_BLOCK_SLICES - 1) / VC_FILTER_BLOCK_SLICES), dim3(VC_FILTER_BLOCK), 0, s, c);
      FILTER_HIP(hipGetLastError());
    }
    st.n_rounds = round + 1;
    st.k_last = kp;
    st.n_searched += n;
    FILTER_HIP(vc_exclusive_scan_u32(flag, scanned, n, scan_work, s));
    hipLaunchKernelGGL(vc_filter_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const uint32_t*)flag, (const uint32_t*)scanned, n, map, a.d_queries, v.W,
                       maps[round & 1], q_next, n_next);
    FILTER_HIP(hipGetLastError());
    uint32_t left = 0;   // THE WAIT of the round: 4 bytes
    FILTER_HIP(hipMemcpyAsync(&left, n_next, 4, hipMemcpyDeviceToHost, s));
    FILTER_HIP(hipStreamSynchronize(s));
    if (left > n) {
      if (err) *err = "filtered search: the list of open queries is longer than the round";
      return VC_ERR_HIP;
    }
    if (left == 0) break;
    // the gather read the caller's queries through the old map and wrote q_next and the other map: the next step reads those
    q = q_next;
    map = maps[round & 1];
    n = left;
    if (kp >= VC_MAX_K) {   // the widest row did not finish them: the exact route does
      st.n_fallback = left;
      const int rc = pre_run(v, a, keep, q, map, n, &st, s, err);
      if (rc) return rc;
      break;
    }
    kp = vc_filter_next_k(kp);
  }
  if (stats) *stats = st;
  return VC_OK;
}

int vc_filter_run_host(const VcStoreView& v, const VcFilterHostArgs& a,
                       const std::function<int(const uint64_t* d_queries, const uint32_t* d_sel, uint64_t* d_out, uint32_t* d_counts)>& run, hipStream_t s,
                       std::string* err) {
  const size_t sel_words = a.kind == VC_FILTER_BITS ? (size_t)((v.n + 31) / 32) : (size_t)v.n;
  const size_t qbytes = (size_t)a.nq * v.W * 8, obytes = (size_t)a.nq * a.k * 8, sbytes = up8(sel_words * 4), cbytes = (size_t)a.nq * 4;
  uint8_t* stage = (uint8_t*)v.alloc(VC_FILTER_STAGE, qbytes + obytes + sbytes + cbytes + 8);   // staged: queries | out | sel | counts
  if (!stage) return VC_ERR_NOMEM;
  uint64_t* d_q = (uint64_t*)stage;
  uint64_t* d_out = (uint64_t*)(stage + qbytes);
  uint32_t* d_sel = (uint32_t*)(stage + qbytes + obytes);
  uint32_t* d_cnt = (uint32_t*)(stage + qbytes + obytes + sbytes);
  FILTER_HIP(hipMemcpyAsync(d_q, a.queries, qbytes, hipMemcpyHostToDevice, s));
  if (sel_words) FILTER_HIP(hipMemcpyAsync(d_sel, a.sel, sel_words * 4, hipMemcpyHostToDevice, s));
  const int rc = run(d_q, d_sel, d_out, d_cnt);
  if (rc) return rc;
  std::vector<uint32_t> cnt(a.nq);
  FILTER_HIP(hipMemcpyAsync(a.out, d_out, obytes, hipMemcpyDeviceToHost, s));
  FILTER_HIP(hipMemcpyAsync(cnt.data(), d_cnt, cbytes, hipMemcpyDeviceToHost, s));
  FILTER_HIP(hipStreamSynchronize(s));
  for (uint32_t i = 0; i < a.nq; ++i) {
    if (a.order == VC_ORDER_FARTHEST_FIRST) {
      uint64_t* row = a.out + (size_t)i * a.k;
      // the valid part: the count; a passed-on row (UINT32_MAX) has what is not padding
      const uint32_t valid = cnt[i] == 0xFFFFFFFFu ? (uint32_t)(std::find(row, row + a.k, VC_PACK_INF) - row) : std::min(cnt[i], a.k);
      std::reverse(row, row + valid);
    }
    if (a.counts) a.counts[i] = cnt[i];
  }
  return VC_OK;
}
