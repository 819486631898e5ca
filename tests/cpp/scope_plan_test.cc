// The plan arithmetic of vc_search_knn_scoped* (csrc/vc_scope_plan.hpp) against brute-force loops, on the CPU: the key bits of the slot
// sort, the counters of a segment and where each (window, slice) counter lies, the slice -> query-range rule and its split over
// grid.y, the sub-batches and the windows.  Stand-alone: built with -fsanitize=address,undefined by tests/test_scope_cpu.py and run as
// its own process.  Prints the constants and three planned cases that the numpy model of tests/scope_common.py is held against.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "vc_scope_plan.hpp"

#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                      \
    }                                                                    \
  } while (0)

static std::mt19937_64 rng(12345);
static uint32_t rnd(uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % (hi - lo + 1)); }

static void test_knobs_and_key_bits() {
  CHECK(vc_scope_window(0) == VC_SCOPE_WINDOW_DEFAULT && vc_scope_window(VC_SCOPE_WINDOW_MAX + 1) == VC_SCOPE_WINDOW_DEFAULT);
  CHECK(vc_scope_window(1) == 1 && vc_scope_window(256) == 256 && vc_scope_window(VC_SCOPE_WINDOW_MAX) == VC_SCOPE_WINDOW_MAX);
  for (uint32_t U = 0; U < 70000; ++U) {
    uint32_t b = 0;
    while ((1ull << b) < U) ++b;
    CHECK(vc_scope_key_bits(U) == b);
    if (U > 1) CHECK(U - 1 < (1ull << b) && U - 1 >= (1ull << (b - 1)));   // every slot fits, and no bit is spare
  }
  CHECK(vc_scope_key_bits(0xFFFFFFFFu) == 32);
}

// the (window, slice) pairs a segment touches, in order -> the counter index of each
static std::map<std::pair<uint32_t, uint32_t>, uint32_t> brute_counters(uint32_t lo, uint32_t hi, uint32_t window, uint32_t len) {
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> m;
  for (uint32_t p = lo; p < hi; ++p) {
    const uint32_t w = p / window, s = (p - w * window) / len;
    m.emplace(std::make_pair(w, s), 0u);
  }
  uint32_t i = 0;
  for (auto& kv : m) kv.second = i++;
  return m;
}

static void test_counters() {
  const uint32_t lens[4] = {512, 256, 128, 64};
  for (int it = 0; it < 4000; ++it) {
    const uint32_t len = lens[it & 3], window = it % 7 == 0 ? len * rnd(1, 4) : rnd(1, 3000);
    const uint32_t lo = rnd(0, 6000), hi = lo + (it % 11 == 0 ? 0 : rnd(0, 5000)), A = hi + rnd(0, 100);
    const auto m = brute_counters(lo, hi, window, len);
    CHECK(vc_scope_cost(lo, hi, window, len) == m.size());
    uint32_t per_window_total = 0;
    for (uint32_t w0 = 0; w0 < A; w0 += window) {
      const uint32_t wn = A - w0 < window ? A - w0 : window;
      uint32_t in = 0, first = 0xFFFFFFFFu, last = 0;
      for (uint32_t p = w0; p < w0 + wn; ++p)
        if (p >= lo && p < hi) {
          ++in;
          const uint32_t s = (p - w0) / len;
          if (first == 0xFFFFFFFFu) first = s;
          last = s;
          const uint32_t c = vc_scope_counter(lo, hi, w0, window, len, s);
          CHECK(c == m.at(std::make_pair(w0 / window, s)) && c < m.size());
        }
      CHECK(vc_scope_in_window(lo, hi, w0, wn) == in);
      const uint32_t n_sl = vc_scope_window_slices(lo, hi, w0, wn, len);
      CHECK(n_sl == (in ? last - first + 1 : 0u));
      if (in) CHECK(vc_scope_first_slice(lo, w0, len) == first);
      per_window_total += n_sl;
    }
    CHECK(per_window_total == m.size());
  }
}

struct Scene {
  std::vector<uint32_t> seg, qrun;   // U + 1 each
  uint32_t U, nq, A;
};
static Scene scene(const std::vector<uint32_t>& sizes, const std::vector<uint32_t>& queries) {
  Scene sc;
  sc.U = (uint32_t)sizes.size();
  sc.seg.assign(1, 0);
  sc.qrun.assign(1, 0);
  for (uint32_t u = 0; u < sc.U; ++u) {
    sc.seg.push_back(sc.seg.back() + sizes[u]);
    sc.qrun.push_back(sc.qrun.back() + queries[u]);
  }
  sc.A = sc.seg.back();
  sc.nq = sc.qrun.back();
  return sc;
}

static void test_slice_queries() {
  for (int it = 0; it < 300; ++it) {
    const uint32_t U = rnd(1, 90), len = 64u << (it & 3), window = rnd(1, 2000);
    std::vector<uint32_t> sizes(U), queries(U);
    for (uint32_t u = 0; u < U; ++u) {
      sizes[u] = it % 5 == 0 ? rnd(0, 9) : rnd(0, 400);
      queries[u] = rnd(1, 4);   // every slot is named by a query
    }
    const Scene sc = scene(sizes, queries);
    std::vector<uint32_t> pslot(sc.A), slot_of_q(sc.nq);
    for (uint32_t u = 0; u < U; ++u) {
      for (uint32_t p = sc.seg[u]; p < sc.seg[u + 1]; ++p) pslot[p] = u;
      for (uint32_t j = sc.qrun[u]; j < sc.qrun[u + 1]; ++j) slot_of_q[j] = u;
    }
    const uint32_t j0 = rnd(0, sc.nq), j1 = rnd(j0, sc.nq);
    for (uint32_t w0 = 0; w0 < sc.A; w0 += window) {
      const uint32_t wn = sc.A - w0 < window ? sc.A - w0 : window;
      for (uint32_t s = 0; s < vc_filter_n_slices(wn, len / 64 == 8 ? 1 : len / 64 == 4 ? 2 : len / 64 == 2 ? 4 : 8); ++s) {
        const uint32_t p0 = w0 + s * len, p1 = w0 + (wn < (s + 1) * len ? wn : (s + 1) * len);
        uint32_t ja, jb;
        vc_scope_slice_queries(sc.qrun.data(), pslot[p0], pslot[p1 - 1], j0, j1, &ja, &jb);
        CHECK(ja <= jb);
        for (uint32_t j = 0; j < sc.nq; ++j) {   // a query is served iff it is in the launch's range and its slot lies between the ends'
          const bool want = j >= j0 && j < j1 && slot_of_q[j] >= pslot[p0] && slot_of_q[j] <= pslot[p1 - 1];
          CHECK(want == (j >= ja && j < jb));
          bool touches = false;   // every query whose segment has a position in the slice is among them
          for (uint32_t p = p0; p < p1; ++p) touches |= pslot[p] == slot_of_q[j];
          if (touches && j >= j0 && j < j1) CHECK(j >= ja && j < jb);
        }
        const uint32_t gy = rnd(1, 9);
        uint32_t at = ja;
        for (uint32_t y = 0; y < gy; ++y) {   // the parts are contiguous, disjoint and cover the range
          uint32_t a, b;
          vc_scope_split(ja, jb, y, gy, &a, &b);
          CHECK(a == at && b >= a && b <= jb);
          at = b;
        }
        CHECK(at == jb);
      }
    }
  }
  CHECK(vc_scope_grid_y(1, 1) == 1 && vc_scope_grid_y(4096, 4096) == 1 && vc_scope_grid_y(1, 4096) == 64 && vc_scope_grid_y(512, 4096) == 4);
  CHECK(vc_scope_grid_y(0, 0) == 1 && vc_scope_grid_y(100, 3) == 3);
}

// sub-batches and windows of a scene: what vc_scope_run does on the host; returns n_windows and the number of sub-batches
static std::pair<uint32_t, uint32_t> plan_of(const Scene& sc, uint32_t window, uint32_t len, uint64_t budget, bool check) {
  std::vector<uint32_t> lo(sc.nq), hi(sc.nq), cost(sc.nq);
  for (uint32_t u = 0; u < sc.U; ++u)
    for (uint32_t j = sc.qrun[u]; j < sc.qrun[u + 1]; ++j) {
      lo[j] = sc.seg[u];
      hi[j] = sc.seg[u + 1];
      cost[j] = vc_scope_cost(lo[j], hi[j], window, len);
    }
  const uint64_t cap = vc_scope_batch_counters(budget);
  uint32_t n_windows = 0, n_batches = 0;
  for (uint32_t b0 = 0; b0 < sc.nq;) {
    const uint32_t b1 = vc_scope_batch_end(cost.data(), sc.nq, b0, budget);
    CHECK(b1 > b0 && b1 <= sc.nq);
    if (check) {
      uint64_t sum = 0;
      for (uint32_t j = b0; j < b1; ++j) sum += cost[j];
      CHECK(b1 == b0 + 1 || sum <= cap);                   // under the budget, or a single query
      if (b1 < sc.nq) CHECK(sum + cost[b1] > cap);         // and no query more would fit
    }
    const uint32_t nw = vc_scope_n_windows(lo[b0], hi[b1 - 1], window);
    if (check) {
      uint32_t brute = 0;
      for (uint32_t w0 = 0; w0 < sc.A; w0 += window) brute += w0 < hi[b1 - 1] && w0 + window > lo[b0] && hi[b1 - 1] > lo[b0];
      CHECK(nw == brute);
      if (nw) CHECK(vc_scope_first_window(lo[b0], window) * window <= lo[b0] && lo[b0] < (vc_scope_first_window(lo[b0], window) + 1) * (uint64_t)window);
    }
    n_windows += nw;
    ++n_batches;
    b0 = b1;
  }
  return {n_windows, n_batches};
}

static void test_batches_and_windows() {
  for (int it = 0; it < 400; ++it) {
    const uint32_t U = rnd(1, 60), len = 64u << (it & 3), window = rnd(1, 1500);
    std::vector<uint32_t> sizes(U), queries(U);
    for (uint32_t u = 0; u < U; ++u) {
      sizes[u] = rnd(0, 700);
      queries[u] = rnd(1, 5);
    }
    plan_of(scene(sizes, queries), window, len, it % 3 == 0 ? 8 : rnd(0, 2000), true);
  }
  CHECK(vc_scope_batch_counters(0) == 0 && vc_scope_batch_counters(4096) == 512 && vc_scope_batch_counters(~0ull) == VC_SCOPE_MAX_COUNTERS);
}

int main() {
  test_knobs_and_key_bits();
  test_counters();
  test_slice_queries();
  test_batches_and_windows();
  std::printf("scope plan ok:\n");
  std::printf("WINDOW %u\nWINDOWMAX %u\nSCRATCH %llu\nCOUNTERBYTES %u\nMAXCOUNTERS %u\n", VC_SCOPE_WINDOW_DEFAULT, VC_SCOPE_WINDOW_MAX,
              (unsigned long long)VC_SCOPE_SCRATCH_DEFAULT, VC_SCOPE_COUNTER_BYTES, VC_SCOPE_MAX_COUNTERS);
  for (uint32_t W = 1; W <= 8; W *= 2) std::printf("SLICE %u %u\n", W, vc_filter_slice_len(W));
  // the cases of scope_common.PLAN_CASES: slot sizes 37 u mod 1500, queries 1 + u mod 3 per slot, 40 slots
  std::vector<uint32_t> sizes, queries;
  for (uint32_t u = 0; u < 40; ++u) {
    sizes.push_back(37 * u * u % 1500);
    queries.push_back(1 + u % 3);
  }
  const Scene sc = scene(sizes, queries);
  const uint32_t cases[3][3] = {{1u << 20, 1, 64u << 20}, {256, 1, 4096}, {1000, 8, 64}};   // window, W, scratch
  for (const auto& c : cases) {
    const auto r = plan_of(sc, vc_scope_window(c[0]), vc_filter_slice_len(c[1]), c[2], true);
    std::printf("CASE %u %u %u %u %u\n", c[0], c[1], c[2], r.first, r.second);
  }
  return 0;
}
