// Host test of csrc/vc_filter_plan.hpp, the plan arithmetic of vc_search_knn_filtered*: the route rule at its edge, the k' schedule,
// the verdict on a row, the sub-batches, the windows, the wave-slice layout and the cut of a histogram.  Built stand-alone with the
// sanitizers by tests/test_filter_cpu.py; prints the constants the Python model must share.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vc_filter_plan.hpp"

#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

static void test_route() {
  CHECK(vc_filter_expected_k(100, 1000, 1000) == 100);
  CHECK(vc_filter_expected_k(100, 1000, 999) == 101);    // ceil
  CHECK(vc_filter_expected_k(1, 1ull << 32, 1) == 1ull << 32);
  CHECK(vc_filter_expected_k(8192, 0xFFFFFFFFull, 1) == 8192ull * 0xFFFFFFFFull);   // no 64-bit overflow at the limits
  // the edge: 2 ceil(k N / A) == POST_MAX_K is still the post-filter route
  const uint32_t half = VC_FILTER_POST_MAX_K / 2;
  CHECK(vc_filter_route(half, 1000, 1000, 0) == VC_FILTER_ROUTE_POST);
  CHECK(vc_filter_route(half, 1000, 999, 0) == VC_FILTER_ROUTE_PRE);     // ceil lifts it by one
  CHECK(vc_filter_route(half + 1, 1000, 1000, 0) == VC_FILTER_ROUTE_PRE);
  CHECK(vc_filter_route(1, half, 1, 0) == VC_FILTER_ROUTE_POST && vc_filter_route(1, half + 1, 1, 0) == VC_FILTER_ROUTE_PRE);   // k = 1: N / A alone
  for (uint32_t knob = 1; knob <= 2; ++knob) {   // the knob forces either route whatever the selectivity
    CHECK(vc_filter_route(1, 1000, 1000, knob) == knob);
    CHECK(vc_filter_route(8192, 1000, 1, knob) == knob);
  }
  CHECK(vc_filter_route(1, 1000, 1000, 3) == VC_FILTER_ROUTE_POST);     // an unknown knob value counts as auto
}

static void test_schedule() {
  CHECK(vc_filter_first_k(10, 0, 1000, 1000) == 20);
  CHECK(vc_filter_first_k(10, 0, 1000, 500) == 40);
  CHECK(vc_filter_first_k(10, 0, 1000, 1) == VC_FILTER_MAX_K);            // clamped above
  CHECK(vc_filter_first_k(8192, 0, 1000, 1000) == 8192);
  CHECK(vc_filter_first_k(5000, 0, 10, 10) == 8192);
  CHECK(vc_filter_first_k(10, 33, 1000, 1) == 33);                        // the caller's k_first as it is
  CHECK(vc_filter_first_k(1, 0, 0xFFFFFFFFull, 1) == VC_FILTER_MAX_K);
  for (uint32_t k = 1; k <= VC_FILTER_MAX_K; k = k * 3 + 1) CHECK(vc_filter_first_k(k, 0, 77, 77) >= k);
  uint32_t kp = 1, steps = 0;
  while (kp < VC_FILTER_MAX_K) {
    const uint32_t next = vc_filter_next_k(kp);
    CHECK(next == (2 * kp > VC_FILTER_MAX_K ? VC_FILTER_MAX_K : 2 * kp));
    kp = next;
    ++steps;
  }
  CHECK(steps == 13 && vc_filter_next_k(VC_FILTER_MAX_K) == VC_FILTER_MAX_K && vc_filter_next_k(5000) == VC_FILTER_MAX_K);
}

static void test_verdict() {
  VcFilterVerdict v = vc_filter_verdict(10, 40, 40, 10);
  CHECK(v.status == VC_FILTER_DONE && v.count == 10 && v.written == 10);
  v = vc_filter_verdict(12, 40, 40, 10);
  CHECK(v.status == VC_FILTER_DONE && v.count == 10 && v.written == 10);
  v = vc_filter_verdict(3, 39, 40, 10);                                   // the row was not full: the database is exhausted
  CHECK(v.status == VC_FILTER_DONE && v.count == 3 && v.written == 3);
  v = vc_filter_verdict(0, 0, 40, 10);
  CHECK(v.status == VC_FILTER_DONE && v.count == 0 && v.written == 0);
  CHECK(vc_filter_verdict(9, 40, 40, 10).status == VC_FILTER_RETRY);
  CHECK(vc_filter_verdict(9, 8192, 8192, 10).status == VC_FILTER_FALLBACK);
  CHECK(vc_filter_verdict(10, 8192, 8192, 10).status == VC_FILTER_DONE);
  v = vc_filter_verdict(4, 0xFFFFFFFFu, 40, 10);                          // passed on
  CHECK(v.status == VC_FILTER_PASSED && v.count == 0xFFFFFFFFu && v.written == 4);
  CHECK(vc_filter_row_entries(0xFFFFFFFFu, 40) == 40 && vc_filter_row_entries(7, 40) == 7 && vc_filter_row_entries(41, 40) == 40);
  CHECK(vc_filter_sure_below(false, 40, 40, 3) == 0xFFFFFFFFu);
  CHECK(vc_filter_sure_below(true, 39, 40, 3) == 0xFFFFFFFFu);            // not full: the whole database
  CHECK(vc_filter_sure_below(true, 40, 40, 3) == 3);
  CHECK(vc_filter_sure_below(true, 8192, 8192, 3) == 3);                  // at the widest row too: the fallback is exact
}

static void test_batches() {
  CHECK(vc_filter_batch(64ull << 20, 8192) == 1024 && vc_filter_batch(0, 8192) == 1 && vc_filter_batch(20480, 20) == 128);
  CHECK(vc_filter_rows_bytes(4096, 64ull << 20, 8192) == 64ull << 20 && vc_filter_rows_bytes(3, 64ull << 20, 8192) == 3ull * 8192 * 8);
  CHECK(vc_filter_rows_bytes(5, 0, 100) == 800);
  CHECK(vc_filter_pre_batch(64ull << 20, 2048, 4096) == 4096 && vc_filter_pre_batch(64ull << 20, 16384, 4096) == 512);
  CHECK(vc_filter_pre_batch(0, 16384, 4096) == 1 && vc_filter_pre_batch(1ull << 40, 1, 7) == 7 && vc_filter_pre_batch(100, 0, 7) == 7);
}

static void test_windows() {
  CHECK(vc_filter_window(0) == VC_FILTER_WINDOW_DEFAULT && vc_filter_window(256) == 256 && vc_filter_window(VC_FILTER_WINDOW_MAX + 1) == VC_FILTER_WINDOW_DEFAULT);
  CHECK(vc_filter_n_windows(0, 256) == 0 && vc_filter_n_windows(256, 256) == 1 && vc_filter_n_windows(257, 256) == 2);
  const uint64_t A = 2000;
  uint64_t sum = 0;
  for (uint64_t w = 0; w < vc_filter_n_windows(A, 256); ++w) {
    const uint32_t len = vc_filter_window_len(A, 256, w);
    CHECK(len > 0 && len <= 256 && (len == 256 || w + 1 == vc_filter_n_windows(A, 256)));
    sum += len;
  }
  CHECK(sum == A && vc_filter_window_len(A, 256, 8) == 0);
}

// every list position lies in exactly one (slice, step, lane), and those ascend with the position
static void test_slices() {
  const uint32_t sizes[] = {1, 63, 64, 65, 511, 512, 513, VC_FILTER_WINDOW_DEFAULT - 1, VC_FILTER_WINDOW_DEFAULT};
  for (uint32_t W : {1u, 2u, 4u, 8u}) {
    CHECK(vc_filter_steps(W) * W == 8 && vc_filter_slice_len(W) == 64 * vc_filter_steps(W));
    for (uint32_t n : sizes) {
      const uint32_t S = vc_filter_n_slices(n, W);
      CHECK((uint64_t)S * vc_filter_slice_len(W) >= n && (uint64_t)(S - 1) * vc_filter_slice_len(W) < n);
      std::vector<uint8_t> seen(n, 0);
      uint32_t prev = 0;
      bool first = true;
      const uint32_t lo = n > 4096 ? S - 3 : 0;   // a large window: its first slices and its edge
      for (uint32_t s = 0; s < S; ++s) {
        if (s >= 2 && s < lo) continue;
        for (uint32_t r = 0; r < vc_filter_steps(W); ++r)
          for (uint32_t l = 0; l < 64; ++l) {
            const uint32_t p = vc_filter_position(W, s, r, l);
            if (p >= n) continue;
            CHECK(!seen[p]);
            seen[p] = 1;
            CHECK(first || p == prev + 1 || (s == lo && r == 0 && l == 0));
            prev = p;
            first = false;
          }
      }
      for (uint32_t p = 0; p < n; ++p) CHECK(seen[p] || (p >= 2 * vc_filter_slice_len(W) && p < lo * vc_filter_slice_len(W)));
      const uint32_t blocks = vc_filter_scan_blocks(S);
      CHECK(blocks * VC_FILTER_BLOCK_SLICES >= S && (blocks - 1) * VC_FILTER_BLOCK_SLICES < S);
      for (uint32_t nq : {1u, 16u, 17u, 4096u}) {
        const uint32_t gy = vc_filter_scan_grid_y(blocks, nq);
        CHECK(gy >= 1 && gy <= (nq + VC_FILTER_QTILE - 1) / VC_FILTER_QTILE && gy <= 4096);
      }
      for (uint32_t kk : {1u, 100u, 8192u}) {
        const uint32_t ss = vc_filter_sample_slices(n, W, kk);
        CHECK(ss >= 1 && ss <= S && (ss == S || (ss % VC_FILTER_BLOCK_SLICES == 0 && (uint64_t)ss * vc_filter_slice_len(W) >= 16ull * kk &&
                                                 (uint64_t)ss * vc_filter_slice_len(W) >= 4096)));
      }
    }
  }
}

static void test_cut() {
  const uint32_t bits = 64;
  std::vector<uint32_t> h(bits + 1, 0);
  h[3] = 2; h[5] = 4; h[9] = 1; h[64] = 10;
  uint32_t tau = 99, below = 99;
  vc_filter_cut(h.data(), bits, 1, &tau, &below);  CHECK(tau == 3 && below == 0);
  vc_filter_cut(h.data(), bits, 2, &tau, &below);  CHECK(tau == 3 && below == 0);    // kk == cumulative
  vc_filter_cut(h.data(), bits, 3, &tau, &below);  CHECK(tau == 5 && below == 2);    // kk == cumulative + 1
  vc_filter_cut(h.data(), bits, 6, &tau, &below);  CHECK(tau == 5 && below == 2);
  vc_filter_cut(h.data(), bits, 7, &tau, &below);  CHECK(tau == 9 && below == 6);
  vc_filter_cut(h.data(), bits, 8, &tau, &below);  CHECK(tau == 64 && below == 7);   // the last bin
  vc_filter_cut(h.data(), bits, 17, &tau, &below); CHECK(tau == 64 && below == 7);
  vc_filter_cut(h.data(), bits, 18, &tau, &below); CHECK(tau == 64 && below == 7);   // more than there is: the last bin, never past the table
  std::vector<uint32_t> z(bits + 1, 0);
  vc_filter_cut(z.data(), bits, 1, &tau, &below);  CHECK(tau == 64 && below == 0);
  // a bounded histogram (bins above U incomplete) cuts where the complete one does, U being no less than the true cut
  std::vector<uint32_t> full(bits + 1, 0), part(bits + 1, 0);
  uint32_t x = 12345;
  for (int i = 0; i < 5000; ++i) {
    x = x * 1664525u + 1013904223u;
    ++full[20 + (x >> 24) % 30];
  }
  for (uint32_t kk : {1u, 50u, 777u, 5000u}) {
    uint32_t t0, b0;
    vc_filter_cut(full.data(), bits, kk, &t0, &b0);
    for (uint32_t U = t0; U <= bits; U += 7) {
      for (uint32_t d = 0; d <= bits; ++d) part[d] = d <= U ? full[d] : full[d] / 3;
      uint32_t t1, b1;
      vc_filter_cut(part.data(), bits, kk, &t1, &b1);
      CHECK(t1 == t0 && b1 == b0);
    }
  }
}

int main() {
  test_route();
  test_schedule();
  test_verdict();
  test_batches();
  test_windows();
  test_slices();
  test_cut();
  std::printf("filter plan ok:\nMAXK %u\nPOSTMAXK %u\nWINDOW %u\nSCRATCH %llu\nQTILE %u\n", VC_FILTER_MAX_K, VC_FILTER_POST_MAX_K, VC_FILTER_WINDOW_DEFAULT,
              (unsigned long long)VC_FILTER_SCRATCH_DEFAULT, VC_FILTER_QTILE);
  for (uint32_t W : {1u, 2u, 4u, 8u}) std::printf("SLICE %u %u\n", W, vc_filter_slice_len(W));
  return 0;
}
