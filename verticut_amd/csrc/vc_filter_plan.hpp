// Plan arithmetic of vc_search_knn_filtered* (vc_filter.hip): the route rule, the k' schedule of the post-filter rounds, the verdict
// on a stripped row, the sub-batches of both routes, the windows and the wave-slice layout of the subset scan, and the cut of a
// distance histogram.  Plain C++ with no HIP in it, so that tests/cpp/filter_plan_test.cc checks it on the CPU; the kernels and the
// driver call exactly these functions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VC_FP_FN __host__ __device__ inline
#else
#define VC_FP_FN inline
#endif

#define VC_FILTER_MAX_K 8192u                       // = VC_MAX_K: the widest row the search underneath returns
// THE ROUTE THRESHOLD: the plan takes the post-filter route while 2 * ceil(k N / A) <= this.  The first guess was 1024, never
// measured.  Measured (tools/bench_filtered.py, profiles/filtered_bench.json, DESIGN.md 5.14: 1e6 64-bit codes, exact MIH, 4096
// queries, k = 100): the pre-filter route was the faster one at EVERY selectivity from A/N = 1 (200 units) down, so the crossover lies
// below the smallest point measured and the threshold sits just under it.  Below 200 units (k < 100 on a dense filter) nothing
// was measured and the rounds keep the automatic route.  The unit does not see N or the batch size, which the pre-filter
// route's cost is proportional to: VC_FILTER_ROUTE=1 is there for stores and batches far from the measured ones.
#define VC_FILTER_POST_MAX_K 199u
#define VC_FILTER_SCRATCH_DEFAULT (64ull << 20)     // bytes of k' rows / of per-slice counters per sub-batch (VC_FILTER_SCRATCH)
#define VC_FILTER_WINDOW_DEFAULT (1u << 20)         // allowed ids per window of the pre-filter route (VC_FILTER_WINDOW)
#define VC_FILTER_WINDOW_MAX (1u << 24)
#define VC_FILTER_KINDS 5u                          // VC_FILTER_MASK .. VC_FILTER_BITS
#define VC_FILTER_ROUTE_AUTO 0u
#define VC_FILTER_ROUTE_POST 1u                     // = VC_FILTER_RAN_POST
#define VC_FILTER_ROUTE_PRE 2u                      // = VC_FILTER_RAN_PRE

// ---- the route -----------------------------------------------------------------------------------------------------------------------
// the k' at which a row of the unfiltered search is expected to hold k allowed records: ceil(k N / A); A >= 1
VC_FP_FN uint64_t vc_filter_expected_k(uint32_t k, uint64_t N, uint64_t A) { return ((uint64_t)k * N + A - 1) / A; }
// knob: VC_FILTER_ROUTE (0 auto, 1 post first, 2 pre only; anything else counts as auto)
VC_FP_FN uint32_t vc_filter_route(uint32_t k, uint64_t N, uint64_t A, uint32_t knob) {
  if (knob == VC_FILTER_ROUTE_POST || knob == VC_FILTER_ROUTE_PRE) return knob;
  return 2 * vc_filter_expected_k(k, N, A) <= VC_FILTER_POST_MAX_K ? VC_FILTER_ROUTE_POST : VC_FILTER_ROUTE_PRE;
}

// ---- the schedule of the post-filter rounds: k'_0 = k_first, or clamp(2 ceil(k N / A), k, VC_MAX_K); k'_{j+1} = min(VC_MAX_K, 2 k'_j) ----
VC_FP_FN uint32_t vc_filter_next_k(uint32_t kp) { return kp >= VC_FILTER_MAX_K / 2 ? VC_FILTER_MAX_K : 2 * kp; }
VC_FP_FN uint32_t vc_filter_first_k(uint32_t k, uint32_t k_first, uint64_t N, uint64_t A) {
  if (k_first) return k_first;
  const uint64_t e = vc_filter_expected_k(k, N, A);
  const uint64_t want = e >= VC_FILTER_MAX_K ? VC_FILTER_MAX_K : 2 * e;
  return want < k ? k : want > VC_FILTER_MAX_K ? VC_FILTER_MAX_K : (uint32_t)want;
}

// ---- the verdict on a stripped row: `kept` allowed entries among the sure part of the `cnt` entries the search at k' returned -----------
enum { VC_FILTER_DONE = 0, VC_FILTER_RETRY = 1, VC_FILTER_FALLBACK = 2, VC_FILTER_PASSED = 3 };
struct VcFilterVerdict {
  uint32_t status;   // VC_FILTER_*
  uint32_t count;    // the word for counts[] (DONE, PASSED)
  uint32_t written;  // entries of the row that are results, the rest is padding
};
VC_FP_FN VcFilterVerdict vc_filter_verdict(uint32_t kept, uint32_t cnt, uint32_t kp, uint32_t k) {
  const uint32_t w = kept < k ? kept : k;
  if (cnt == 0xFFFFFFFFu) return VcFilterVerdict{VC_FILTER_PASSED, 0xFFFFFFFFu, w};   // the recovery underneath gave up: passed on
  if (kept >= k) return VcFilterVerdict{VC_FILTER_DONE, k, k};
  if (cnt < kp) return VcFilterVerdict{VC_FILTER_DONE, kept, kept};                   // the database is exhausted: A < k
  return VcFilterVerdict{kp >= VC_FILTER_MAX_K ? VC_FILTER_FALLBACK : VC_FILTER_RETRY, 0, 0};
}
VC_FP_FN uint32_t vc_filter_row_entries(uint32_t cnt, uint32_t kp) { return cnt == 0xFFFFFFFFu || cnt > kp ? kp : cnt; }
// THE SURE PREFIX, vc_distinct_sure_below's reason: a full row of exact MIH holds every record nearer than its last distance D but
// only some of those at D.  Here the cut holds at k' = VC_MAX_K as well: a query that the sure prefix does not finish there goes to
// the pre-filter route, which is exact, so no row ever rests on the ties.  Returns the distance entries must stay below.
VC_FP_FN uint32_t vc_filter_sure_below(bool tie_cut, uint32_t cnt, uint32_t kp, uint32_t last_dist) {
  return tie_cut && cnt == kp ? last_dist : 0xFFFFFFFFu;
}

// ---- sub-batches of the post-filter rounds: the rows scratch holds at most `budget` bytes, but always one row ---------------------------
VC_FP_FN uint32_t vc_filter_batch(uint64_t budget, uint32_t kp) {
  const uint64_t b = budget / (8ull * kp);
  return b < 1 ? 1u : b > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)b;
}
VC_FP_FN uint64_t vc_filter_rows_bytes(uint32_t n, uint64_t budget, uint32_t kp) {
  const uint32_t b = vc_filter_batch(budget, kp);
  return 8ull * kp * (n < b ? n : b);
}

// ---- the windows of the pre-filter route: the A allowed ids in list order, `window` at a time ------------------------------------------
VC_FP_FN uint32_t vc_filter_window(uint32_t knob) { return knob == 0 || knob > VC_FILTER_WINDOW_MAX ? VC_FILTER_WINDOW_DEFAULT : knob; }
VC_FP_FN uint64_t vc_filter_n_windows(uint64_t A, uint32_t window) { return (A + window - 1) / window; }
VC_FP_FN uint32_t vc_filter_window_len(uint64_t A, uint32_t window, uint64_t w) {
  const uint64_t lo = w * window, left = A > lo ? A - lo : 0;
  return left < window ? (uint32_t)left : window;
}

// ---- the wave-slices of a window of n list positions ----------------------------------------------------------------------------------
// A wave keeps `steps` gathered codes per lane in registers (steps x W = 8 words, 16 VGPRs): its slice is the positions
// [s * len, min(n, (s + 1) * len)), len = 64 * steps, and step r of lane l is position s * len + 64 r + l -- ascending in (r, l), so
// ballot order within a step, steps in order and slices in order IS list order, which is id order.
#define VC_FILTER_BLOCK 256u          // threads per block of the scan kernels: four waves, four consecutive slices
#define VC_FILTER_BLOCK_SLICES 4u
#define VC_FILTER_QTILE 16u           // queries per LDS tile
VC_FP_FN constexpr uint32_t vc_filter_steps(uint32_t W) { return W <= 1 ? 8u : W == 2 ? 4u : W <= 4 ? 2u : 1u; }
VC_FP_FN constexpr uint32_t vc_filter_slice_len(uint32_t W) { return 64u * vc_filter_steps(W); }
VC_FP_FN uint32_t vc_filter_n_slices(uint32_t n, uint32_t W) { return (n + vc_filter_slice_len(W) - 1) / vc_filter_slice_len(W); }
VC_FP_FN uint32_t vc_filter_position(uint32_t W, uint32_t slice, uint32_t step, uint32_t lane) { return slice * vc_filter_slice_len(W) + 64u * step + lane; }
VC_FP_FN uint32_t vc_filter_scan_blocks(uint32_t n_slices) { return (n_slices + VC_FILTER_BLOCK_SLICES - 1) / VC_FILTER_BLOCK_SLICES; }
// grid.y of a scan launch: blocks that share the query tiles of a sub-batch among them, enough to fill the device at small windows
VC_FP_FN uint32_t vc_filter_scan_grid_y(uint32_t blocks_x, uint32_t nq) {
  const uint32_t tiles = (nq + VC_FILTER_QTILE - 1) / VC_FILTER_QTILE;
  const uint32_t want = blocks_x >= 4096u ? 1u : (4096u + blocks_x - 1) / (blocks_x ? blocks_x : 1u);
  return tiles < want ? (tiles ? tiles : 1u) : want;
}
// queries per sub-batch of the pre-filter route: two 32-bit counters per (query, slice) of the largest window stay under `budget`
VC_FP_FN uint32_t vc_filter_pre_batch(uint64_t budget, uint32_t max_slices, uint32_t nq) {
  const uint64_t b = budget / (8ull * (max_slices ? max_slices : 1u));
  return b < 1 ? 1u : b > nq ? nq : (uint32_t)b;
}
// the prefix of a window whose histogram is taken without a bound; its cut bounds the rest (never below the true kk-th distance,
// the prefix being a subset of the window): whole blocks, at least 16 kk and 4096 positions, the whole window when that is no more
VC_FP_FN uint32_t vc_filter_sample_slices(uint32_t n, uint32_t W, uint32_t kk) {
  const uint32_t total = vc_filter_n_slices(n, W);
  const uint64_t want = 16ull * kk > 4096ull ? 16ull * kk : 4096ull;
  uint64_t s = (want + vc_filter_slice_len(W) - 1) / vc_filter_slice_len(W);
  s = (s + VC_FILTER_BLOCK_SLICES - 1) / VC_FILTER_BLOCK_SLICES * VC_FILTER_BLOCK_SLICES;
  return s >= total ? total : (uint32_t)s;
}

// ---- the cut of a histogram of distances 0 .. bits: tau = the smallest d whose cumulative count reaches kk (kk >= 1), below = the
// count of the distances under tau.  A histogram that never reaches kk (the caller's kk exceeds its total) cuts at `bits`.
VC_FP_FN void vc_filter_cut(const uint32_t* hist, uint32_t bits, uint32_t kk, uint32_t* tau, uint32_t* below) {
  uint32_t c = 0;
  for (uint32_t d = 0; d < bits; ++d) {
    const uint32_t h = hist[d];
    if (c + h >= kk) {
      *tau = d;
      *below = c;
      return;
    }
    c += h;
  }
  *tau = bits;
  *below = c;
}
