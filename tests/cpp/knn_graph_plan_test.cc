// csrc/vc_knn_graph_plan.hpp on the CPU, host code only: built with -fsanitize=address,undefined by tests/test_knn_graph_cpu.py.
// The argument rules, the range, the schedule, the verdict on a row against the rule spelled out again over brute-forced rows, the
// sub-batches, the scratch layout and the one-compare test against a search inside the row.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "vc_knn_graph_plan.hpp"

#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
      exit(1);                                                  \
    }                                                           \
  } while (0)

static const uint32_t K = VC_KGRAPH_MAX_K;

static void arguments() {
  CHECK(!vc_kgraph_k_ok(0) && vc_kgraph_k_ok(1) && vc_kgraph_k_ok(K - 1) && !vc_kgraph_k_ok(K) && !vc_kgraph_k_ok(0xFFFFFFFFu));
  for (uint32_t k = 1; k < K; ++k) {
    CHECK(vc_kgraph_k_first_ok(k, 0) && vc_kgraph_k_first_ok(k, k + 1) && vc_kgraph_k_first_ok(k, K));
    CHECK(!vc_kgraph_k_first_ok(k, k) && !vc_kgraph_k_first_ok(k, K + 1) && !vc_kgraph_k_first_ok(k, 0xFFFFFFFFu));
  }
  CHECK(vc_kgraph_batch(0) == 4096 && vc_kgraph_batch(1) == 1 && vc_kgraph_batch(0xFFFFFFFFu) == 0xFFFFFFFFu);
  uint64_t rows = 99;
  CHECK(vc_kgraph_range(0, 0, 0, &rows) && rows == 0);
  CHECK(vc_kgraph_range(10, 0, 0, &rows) && rows == 10);
  CHECK(vc_kgraph_range(10, 3, 0, &rows) && rows == 7);
  CHECK(vc_kgraph_range(10, 3, 7, &rows) && rows == 7);
  CHECK(vc_kgraph_range(10, 10, 0, &rows) && rows == 0);
  CHECK(!vc_kgraph_range(10, 3, 8, &rows) && !vc_kgraph_range(10, 11, 0, &rows) && !vc_kgraph_range(0, 0, 1, &rows));
  CHECK(!vc_kgraph_range(10, 0xFFFFFFFFFFFFFFFFull, 2, &rows) && !vc_kgraph_range(10, 2, 0xFFFFFFFFFFFFFFFFull, &rows));   // (no wrap)
  CHECK(vc_kgraph_row_count(0, 5) == 0 && vc_kgraph_row_count(1, 5) == 0 && vc_kgraph_row_count(5, 5) == 4 && vc_kgraph_row_count(6, 5) == 5);
  CHECK(vc_kgraph_row_count(0xFFFFFFFFull, K - 1) == K - 1);
}

static void schedule() {
  for (uint32_t k = 1; k < K; ++k) {
    CHECK(vc_kgraph_first_k(k, 0, true) == k + 1 && vc_kgraph_first_k(k, K, true) == k + 1);
    const uint32_t want = 2 * (k + 1) < K ? 2 * (k + 1) : K;
    CHECK(vc_kgraph_first_k(k, 0, false) == want && vc_kgraph_first_k(k, k + 1, false) == k + 1 && vc_kgraph_first_k(k, K, false) == K);
    uint32_t kp = vc_kgraph_first_k(k, k + 1, false), rounds = 1;
    while (kp < K) {
      const uint32_t next = vc_kgraph_next_k(kp);
      CHECK(next > kp && next <= K);
      kp = next;
      ++rounds;
    }
    CHECK(kp == K && vc_kgraph_next_k(kp) == K && rounds <= 13);
  }
}

// rows of a tiny store by brute force: the verdict says "settled" exactly when the first k stripped entries are the rule's
static void verdict() {
  uint64_t state = 12345;
  auto rnd = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(state >> 33); };
  for (int scene = 0; scene < 300; ++scene) {
    const uint32_t n = 2 + rnd() % 30, own = rnd() % n;
    std::vector<uint32_t> dist(n);
    for (uint32_t i = 0; i < n; ++i) dist[i] = i == own ? 0 : rnd() % 4;   // few distances: ties everywhere; duplicates of the own record
    std::vector<uint64_t> all;
    for (uint32_t i = 0; i < n; ++i) all.push_back(((uint64_t)dist[i] << 32) | (100 + i));
    std::sort(all.begin(), all.end());
    const uint64_t self = 100 + own;
    for (uint32_t k = 1; k <= 6; ++k)
      for (uint32_t kp = k + 1; kp <= 12; ++kp) {
        // an exact-MIH row: the true k' smallest distances; at the last distance ANY members (here: the largest ids)
        std::vector<uint64_t> row;
        const uint32_t m = std::min(kp, n);
        const uint32_t D = (uint32_t)(all[m - 1] >> 32);
        for (uint64_t v : all)
          if ((uint32_t)(v >> 32) < D) row.push_back(v);
        for (size_t i = all.size(); i-- > 0 && row.size() < m;)
          if ((uint32_t)(all[i] >> 32) == D) row.push_back(all[i]);
        std::sort(row.begin(), row.end());
        const uint32_t cnt = m;
        CHECK(vc_kgraph_row_entries(cnt, kp) == m && vc_kgraph_row_entries(0xFFFFFFFFu, kp) == kp);
        const bool present = std::binary_search(row.begin(), row.end(), self);
        const uint32_t below = (uint32_t)(std::lower_bound(row.begin(), row.end(), (uint64_t)D << 32) - row.begin());
        const int v = vc_kgraph_verdict(true, cnt, kp, k, present, cnt == kp ? below : 0);
        uint32_t others_below = 0;
        for (uint32_t i = 0; i < n; ++i) others_below += i != own && dist[i] < D;
        CHECK(v == (n < kp || others_below >= k ? VC_KGRAPH_SETTLED : VC_KGRAPH_RETRY));
        if (v == VC_KGRAPH_SETTLED) {   // the stripped prefix is the rule's row
          std::vector<uint64_t> want, got;
          for (uint64_t x : all)
            if (x != self && want.size() < k) want.push_back(x);
          for (uint64_t x : row)
            if (x != self && got.size() < k) got.push_back(x);
          CHECK(got == want && vc_kgraph_count(m, present, k) == want.size());
        }
        // the linear scan's row is settled whatever it holds; its given-up count is passed on
        CHECK(vc_kgraph_verdict(false, cnt, kp, k, present, 0) == VC_KGRAPH_SETTLED);
        CHECK(vc_kgraph_verdict(false, 0xFFFFFFFFu, kp, k, present, 0) == VC_KGRAPH_PASSED);
        CHECK(vc_kgraph_verdict(true, 0xFFFFFFFFu, kp, k, present, kp) == VC_KGRAPH_RETRY && vc_kgraph_verdict(true, kp + 1, kp, k, present, kp) == VC_KGRAPH_RETRY);
      }
  }
  CHECK(vc_kgraph_verdict(true, 8, 8, 3, true, 0) == VC_KGRAPH_RETRY);     // eight duplicates: nothing lies below distance 0
  CHECK(vc_kgraph_verdict(true, 8, 8, 3, true, 4) == VC_KGRAPH_SETTLED && vc_kgraph_verdict(true, 8, 8, 3, true, 3) == VC_KGRAPH_RETRY);
  CHECK(vc_kgraph_count(5, true, 9) == 4 && vc_kgraph_count(5, false, 9) == 5 && vc_kgraph_count(5, true, 3) == 3 && vc_kgraph_count(1, true, 3) == 0);
}

static void batches() {
  CHECK(VC_KGRAPH_SCRATCH_DEFAULT == 64ull << 20);
  CHECK(vc_kgraph_sub_batch(VC_KGRAPH_SCRATCH_DEFAULT, K) == 1024 && vc_kgraph_sub_batch(VC_KGRAPH_SCRATCH_DEFAULT, 22) == (64u << 20) / (8 * 22));
  CHECK(vc_kgraph_sub_batch(0, K) == 1 && vc_kgraph_sub_batch(1, 2) == 1 && vc_kgraph_sub_batch(0xFFFFFFFFFFFFFFFFull, 2) == 0xFFFFFFFFu);
  for (uint32_t kp : {2u, 3u, 100u, K})
    for (uint64_t budget : {0ull, 1ull, 4096ull, 1ull << 20, VC_KGRAPH_SCRATCH_DEFAULT})
      for (uint32_t n : {1u, 2u, 63u, 4096u, 100000u}) {
        const uint32_t b = vc_kgraph_sub_batch(budget, kp);
        CHECK(b >= 1 && (b == 1 || 8ull * kp * b <= budget));
        CHECK(vc_kgraph_rows_bytes(n, budget, kp) == 8ull * kp * std::min(n, b));
      }
}

static void layout() {
  for (uint32_t nq : {1u, 2u, 3u, 4096u, 100001u})
    for (uint32_t W : {1u, 2u, 4u, 8u})
      for (uint64_t scan : {0ull, 1ull, 7ull, 1000ull}) {
        const VcKgraphWork w(nq, W, scan);
        const uint64_t offs[] = {w.tally, w.n_next, w.flag, w.scanned, w.scan_work, w.map[0], w.map[1], w.cnt, w.ids, w.found, w.q, w.q_next, w.total};
        const uint64_t need[] = {8, 4, 4ull * nq, 4ull * nq, 4 * scan, 4ull * nq, 4ull * nq, 4ull * nq, 4ull * nq, 4ull * nq, 8ull * nq * W, 8ull * nq * W};
        CHECK(offs[0] == 0 && offs[2] == 16);                        // the memset at the start covers the tally and the length
        for (int i = 0; i < 12; ++i) CHECK(offs[i] % 8 == 0 && offs[i] + need[i] <= offs[i + 1]);
      }
  CHECK(VC_KGRAPH_STAT_BYTES == 32);
}

// "j lists i among its first m" by the one compare == by a search inside row j
static void one_compare() {
  uint64_t state = 99;
  auto rnd = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(state >> 33); };
  for (int scene = 0; scene < 200; ++scene) {
    const uint32_t n = 2 + rnd() % 20, k = 1 + rnd() % 8;
    std::vector<std::vector<uint32_t>> d(n, std::vector<uint32_t>(n, 0));
    for (uint32_t i = 0; i < n; ++i)
      for (uint32_t j = 0; j < i; ++j) d[i][j] = d[j][i] = rnd() % 3;   // symmetric, full of ties
    std::vector<std::vector<uint64_t>> rows(n);
    for (uint32_t j = 0; j < n; ++j) {
      for (uint32_t i = 0; i < n; ++i)
        if (i != j) rows[j].push_back(((uint64_t)d[j][i] << 32) | (7 + i));
      std::sort(rows[j].begin(), rows[j].end());
      rows[j].resize(std::min<size_t>(rows[j].size(), k));
    }
    const uint32_t cnt = vc_kgraph_row_count(n, k);
    for (uint32_t kk = 1; kk <= k; ++kk)
      for (uint32_t j = 0; j < n; ++j) {
        const uint32_t m = vc_kgraph_edge_entries(kk, cnt);
        CHECK(m == std::min(kk, cnt) && m >= 1);
        for (uint32_t i = 0; i < n; ++i) {
          if (i == j) continue;
          const uint64_t mine = ((uint64_t)d[i][j] << 32) | (7 + i);
          const bool listed = std::find(rows[j].begin(), rows[j].begin() + m, mine) != rows[j].begin() + m;
          CHECK(vc_kgraph_lists(rows[j][m - 1], d[i][j], 7 + i) == listed);
        }
      }
  }
}

int main() {
  arguments();
  schedule();
  verdict();
  batches();
  layout();
  one_compare();
  printf("knn graph plan ok: MAXK %u SCRATCH %llu BATCH %u\n", VC_KGRAPH_MAX_K, (unsigned long long)VC_KGRAPH_SCRATCH_DEFAULT, VC_KGRAPH_BATCH_DEFAULT);
  for (uint32_t k : {1u, 10u, 100u, 5u, 4095u, 8191u}) printf("FIRST %u %u\n", k, vc_kgraph_first_k(k, 0, false));
  for (uint32_t nq : {1u, 4096u}) printf("WORK %u %llu\n", nq, (unsigned long long)VcKgraphWork(nq, 2, 33).total);
  return 0;
}
