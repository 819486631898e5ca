// Plan arithmetic of vc_search_knn_scoped* (vc_scope.hip): the key bits of the slot sort, the windows of the scope-sorted list, which
// sorted queries a wave-slice serves, how many (query, slice) counters a segment needs and where they lie, and the sub-batches of
// queries that keep the counters under a budget.  Plain C++ with no HIP in it, so that tests/cpp/scope_plan_test.cc checks it on the
// CPU; the kernels and the driver call exactly these functions.  The wave-slices are vc_filter_plan.hpp's.
//
// THE SORTED LIST L holds the A matched records, slots ascending and ids ascending within a slot; slot u (the u-th distinct query
// scope, ascending) owns the SEGMENT [seg[u], seg[u + 1]) of L and the run [qrun[u], qrun[u + 1]) of the SORTED queries.  L is cut
// into windows [w * window, min(A, (w + 1) * window)); a window of n positions into the slices [s * len, min(n, (s + 1) * len)) of
// WINDOW positions, len = vc_filter_slice_len(W).  All positions are below 2^32 (ids are 32 bits wide).
#pragma once
#include <stdint.h>

#include "vc_filter_plan.hpp"

#define VC_SCOPE_SCRATCH_DEFAULT (64ull << 20)     // bytes of (query, slice) counters per sub-batch (VC_SCOPE_SCRATCH)
#define VC_SCOPE_WINDOW_DEFAULT (1u << 20)         // positions of L per window (VC_SCOPE_WINDOW)
#define VC_SCOPE_WINDOW_MAX (1u << 24)
#define VC_SCOPE_COUNTER_BYTES 8u                  // two 32-bit counters per (query, slice): d < tau and d == tau
#define VC_SCOPE_MAX_COUNTERS (1u << 28)           // per sub-batch, whatever the budget says: offsets stay 32-bit differences

VC_FP_FN uint32_t vc_scope_window(uint32_t knob) { return knob == 0 || knob > VC_SCOPE_WINDOW_MAX ? VC_SCOPE_WINDOW_DEFAULT : knob; }

// key bits of the stable sort of the matched records by slot: the smallest b with 2^b >= U; none at U <= 1 (no sort)
VC_FP_FN uint32_t vc_scope_key_bits(uint32_t U) {
  uint32_t b = 0;
  while (b < 32 && (1ull << b) < U) ++b;
  return b;
}

// ---- a segment [lo, hi) of L against the window that starts at w0 and holds wn positions ------------------------------------------------
VC_FP_FN uint32_t vc_scope_in_window(uint32_t lo, uint32_t hi, uint32_t w0, uint32_t wn) {
  const uint32_t a = lo > w0 ? lo : w0, b = hi < w0 + wn ? hi : w0 + wn;
  return b > a ? b - a : 0u;
}
// slices touched by the window positions [a, b), b > a
VC_FP_FN uint32_t vc_scope_slices_of(uint32_t a, uint32_t b, uint32_t len) { return (b - 1) / len - a / len + 1; }
// the first slice of the window at w0 that the segment touches (the segment reaches into the window)
VC_FP_FN uint32_t vc_scope_first_slice(uint32_t lo, uint32_t w0, uint32_t len) { return lo > w0 ? (lo - w0) / len : 0u; }
// slices the segment touches in that window
VC_FP_FN uint32_t vc_scope_window_slices(uint32_t lo, uint32_t hi, uint32_t w0, uint32_t wn, uint32_t len) {
  if (vc_scope_in_window(lo, hi, w0, wn) == 0) return 0u;
  const uint32_t a = (lo > w0 ? lo : w0) - w0, b = (hi < w0 + wn ? hi : w0 + wn) - w0;
  return vc_scope_slices_of(a, b, len);
}
// THE COUNTERS OF A QUERY: one per slice its segment touches, summed over the windows -- window after window, slices ascending
VC_FP_FN uint32_t vc_scope_cost(uint32_t lo, uint32_t hi, uint32_t window, uint32_t len) {
  if (hi <= lo) return 0u;
  const uint32_t wa = lo / window, wb = (hi - 1) / window;
  if (wa == wb) return vc_scope_slices_of(lo - wa * window, hi - wa * window, len);
  return vc_scope_slices_of(lo - wa * window, window, len) + (wb - wa - 1) * ((window + len - 1) / len) + vc_scope_slices_of(0u, hi - wb * window, len);
}
// the query's counters that belong to the windows before the one at w0
VC_FP_FN uint32_t vc_scope_prior(uint32_t lo, uint32_t hi, uint32_t w0, uint32_t window, uint32_t len) {
  return lo < w0 ? vc_scope_cost(lo, hi < w0 ? hi : w0, window, len) : 0u;
}
// where the counter of (query, slice `s` of the window at w0) lies among the query's own; the caller adds the query's offset
VC_FP_FN uint32_t vc_scope_counter(uint32_t lo, uint32_t hi, uint32_t w0, uint32_t window, uint32_t len, uint32_t s) {
  return vc_scope_prior(lo, hi, w0, window, len) + s - vc_scope_first_slice(lo, w0, len);
}

// ---- THE SLICE -> QUERY-RANGE RULE: a slice whose first and last position carry slots u_first <= u_last serves the sorted queries
// [qrun[u_first], qrun[u_last + 1]), cut to the launch's range [j0, j1); qrun has U + 1 entries and u_last < U
VC_FP_FN void vc_scope_slice_queries(const uint32_t* qrun, uint32_t u_first, uint32_t u_last, uint32_t j0, uint32_t j1, uint32_t* ja, uint32_t* jb) {
  const uint32_t a = qrun[u_first], b = qrun[u_last + 1];
  *ja = a > j0 ? a : j0;
  *jb = b < j1 ? b : j1;
  if (*jb < *ja) *jb = *ja;
}
// part y of gy of the range [ja, jb): contiguous, disjoint, covering
VC_FP_FN void vc_scope_split(uint32_t ja, uint32_t jb, uint32_t y, uint32_t gy, uint32_t* a, uint32_t* b) {
  const uint32_t n = jb - ja, per = (n + gy - 1) / gy;
  const uint64_t lo = (uint64_t)y * per, hi = lo + per;
  *a = ja + (uint32_t)(lo < n ? lo : n);
  *b = ja + (uint32_t)(hi < n ? hi : n);
}
// grid.y of a walk launch over blocks_x blocks of four slices and nq sorted queries: enough blocks to fill the device at small windows
VC_FP_FN uint32_t vc_scope_grid_y(uint32_t blocks_x, uint32_t nq) {
  const uint32_t want = blocks_x >= 2048u ? 1u : (2048u + blocks_x - 1) / (blocks_x ? blocks_x : 1u);
  const uint32_t cap = nq < 64u ? (nq ? nq : 1u) : 64u;
  return want < cap ? want : cap;
}

// ---- sub-batches of the sorted queries: [b0, b1) takes queries while their counters stay under the budget, but always one ---------------
VC_FP_FN uint32_t vc_scope_batch_counters(uint64_t budget) {
  const uint64_t c = budget / VC_SCOPE_COUNTER_BYTES;
  return c > VC_SCOPE_MAX_COUNTERS ? VC_SCOPE_MAX_COUNTERS : (uint32_t)c;
}
// cost[j]: vc_scope_cost of sorted query j
VC_FP_FN uint32_t vc_scope_batch_end(const uint32_t* cost, uint32_t nq, uint32_t b0, uint64_t budget) {
  const uint64_t cap = vc_scope_batch_counters(budget);
  uint64_t sum = cost[b0];
  uint32_t b1 = b0 + 1;
  while (b1 < nq && sum + cost[b1] <= cap) sum += cost[b1++];
  return b1;
}
// the windows a sub-batch scans: those its position range [plo, phi) touches
VC_FP_FN uint32_t vc_scope_first_window(uint32_t plo, uint32_t window) { return plo / window; }
VC_FP_FN uint32_t vc_scope_n_windows(uint32_t plo, uint32_t phi, uint32_t window) { return phi > plo ? (phi - 1) / window - plo / window + 1 : 0u; }
