// csrc/vc_distinct_plan.hpp on the CPU, host code only: built with -fsanitize=address,undefined by tests/test_distinct_cpu.py.
// The schedule, the size classes and their LDS, the hash, the verdict on a row against the rule spelled out again, and the
// sub-batches, over every k' and over the edges of the 32-bit arithmetic.
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <vector>

#include "vc_distinct_plan.hpp"

#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
      exit(1);                                                  \
    }                                                           \
  } while (0)

static void schedule() {
  for (uint32_t k = 1; k <= VC_DISTINCT_MAX_K; ++k) {
    CHECK(vc_distinct_k_first_ok(k, 0) && vc_distinct_k_first_ok(k, k) && vc_distinct_k_first_ok(k, VC_DISTINCT_MAX_K));
    CHECK(k == 1 || !vc_distinct_k_first_ok(k, k - 1));
    CHECK(!vc_distinct_k_first_ok(k, VC_DISTINCT_MAX_K + 1) && !vc_distinct_k_first_ok(k, 0xFFFFFFFFu));
    const uint32_t want = 2 * k < VC_DISTINCT_MAX_K ? 2 * k : VC_DISTINCT_MAX_K;
    CHECK(vc_distinct_first_k(k, 0) == want && vc_distinct_first_k(k, k) == k);
    CHECK(vc_distinct_next_k(k) == want);
    uint32_t kp = vc_distinct_first_k(k, 0), rounds = 1;   // the schedule reaches the widest row and stays there
    while (kp < VC_DISTINCT_MAX_K) {
      const uint32_t next = vc_distinct_next_k(kp);
      CHECK(next > kp && next <= VC_DISTINCT_MAX_K);
      kp = next;
      ++rounds;
    }
    CHECK(kp == VC_DISTINCT_MAX_K && vc_distinct_next_k(kp) == VC_DISTINCT_MAX_K && rounds <= 13);
  }
}

static void classes() {
  for (uint32_t kp = 1; kp <= VC_DISTINCT_MAX_K; ++kp) {
    const int c = vc_distinct_class(kp);
    CHECK(c == (kp <= 64 ? VC_DISTINCT_WAVE : kp <= 1024 ? VC_DISTINCT_BLOCK : VC_DISTINCT_TABLE));
    const uint32_t P = vc_distinct_positions(kp), T = vc_distinct_threads(kp);
    CHECK(P >= kp && P >= 64 && (P & (P - 1)) == 0 && (P == 64 || P / 2 < kp));
    CHECK(vc_distinct_slots(kp) == 2 * P);
    CHECK(T == (c == VC_DISTINCT_TABLE ? 1024u : 256u));
    CHECK((kp + T - 1) / T <= 8);                                  // the tiles of a thread fit the 32 bits of its mask, with room
    CHECK(vc_distinct_lds_bytes(kp) == (c == VC_DISTINCT_WAVE ? 0u : 12u * P));
    CHECK(vc_distinct_lds_bytes(kp) + 64 <= 160u * 1024);           // a CU's LDS
    CHECK(c == VC_DISTINCT_TABLE || vc_distinct_lds_bytes(kp) <= 64u * 1024);
    for (uint32_t n : {1u, 3u, 4u, 5u, 257u, 0xFFFFFFFCu}) CHECK(vc_distinct_grid(kp, n) == (c == VC_DISTINCT_WAVE ? (n + 3) / 4 : n));
  }
  CHECK(vc_distinct_lds_bytes(8192) == 96u * 1024 && vc_distinct_lds_bytes(1024) == 12u * 1024 && vc_distinct_lds_bytes(1025) == 24u * 1024);
}

static void hash() {
  // every value lands inside the table; labels that differ only above bit 16, only in the low 4 bits or only at the top spread out
  for (uint32_t slots : {128u, 2048u, 16384u}) {
    for (uint32_t x : {0u, 1u, 0xFFFFFFFFu, 0xFFFFFFFEu, 0x80000000u}) CHECK(vc_distinct_hash(x, slots) < slots);
    std::vector<std::vector<uint32_t>> sets(3);
    for (uint32_t j = 0; j < slots / 2; ++j) {
      sets[0].push_back((j << 16) | 0xBEEFu);
      sets[1].push_back(0x12345670u + (j & 15u) + ((j >> 4) << 20));
      sets[2].push_back(0xFFFFFFFFu - j);
    }
    for (const auto& s : sets) {
      std::vector<uint32_t> load(slots, 0);
      uint32_t worst = 0;
      for (uint32_t x : s) worst = ++load[vc_distinct_hash(x, slots)] > worst ? load[vc_distinct_hash(x, slots)] : worst;
      CHECK(worst <= 8);                                              // at half load a good hash stays far below this
    }
  }
}

static void verdict() {
  const uint32_t kps[] = {1, 2, 63, 64, 65, 1024, 1025, 4096, 8191, 8192};
  for (uint32_t kp : kps)
    for (uint32_t k : {1u, 2u, 10u, kp})
      for (uint32_t cnt : {0u, 1u, kp - 1, kp, 0xFFFFFFFFu})
        for (uint32_t d : {0u, 1u, k - 1, k, k + 1, kp}) {
          if (k > kp || (cnt != 0xFFFFFFFFu && (cnt > kp || d > cnt)) || d > kp) continue;
          const VcDistinctVerdict v = vc_distinct_verdict(d, cnt, kp, k);
          CHECK(vc_distinct_row_entries(cnt, kp) == (cnt == 0xFFFFFFFFu ? kp : cnt));
          if (cnt == 0xFFFFFFFFu) {
            CHECK(v.status == VC_DISTINCT_PASSED && v.count == 0xFFFFFFFFu && v.written == (d < k ? d : k));
          } else if (d >= k) {
            CHECK(v.status == VC_DISTINCT_FULL && v.count == k && v.written == k);
          } else if (cnt < kp) {
            CHECK(v.status == VC_DISTINCT_SHORT && v.count == d && v.written == d);
          } else if (kp == VC_DISTINCT_MAX_K) {
            CHECK(v.status == VC_DISTINCT_CUT && v.count == (d | 0x80000000u) && v.written == d);
          } else {
            CHECK(v.status == VC_DISTINCT_RETRY);
          }
        }
  CHECK(VC_DISTINCT_TRUNCATED_BIT == 0x80000000u);
  // the sure prefix: cut at the row's last distance only where exact MIH is underneath, the row is full and a wider one exists
  for (uint32_t kp : kps)
    for (uint32_t cnt : {0u, 1u, kp - 1, kp, 0xFFFFFFFFu})
      for (uint32_t last : {0u, 7u, 0xFFFFFFFEu}) {
        CHECK(vc_distinct_sure_below(false, cnt, kp, last) == 0xFFFFFFFFu);
        CHECK(vc_distinct_sure_below(true, cnt, kp, last) == (cnt == kp && kp < VC_DISTINCT_MAX_K ? last : 0xFFFFFFFFu));
      }
}

static void batches() {
  CHECK(VC_DISTINCT_SCRATCH_DEFAULT == 64ull << 20);
  CHECK(vc_distinct_batch(VC_DISTINCT_SCRATCH_DEFAULT, 8192) == 1024 && vc_distinct_batch(VC_DISTINCT_SCRATCH_DEFAULT, 200) == 41943);
  CHECK(vc_distinct_rows_bytes(4096, VC_DISTINCT_SCRATCH_DEFAULT, 8192) == 64ull << 20);   // not 256 MiB
  CHECK(vc_distinct_n_batches(4096, VC_DISTINCT_SCRATCH_DEFAULT, 8192) == 4);
  for (uint64_t budget : {0ull, 1ull, 7ull, 8ull, 4096ull, 65536ull, 1ull << 20, 64ull << 20, 1ull << 40, ~0ull})
    for (uint32_t kp : {1u, 64u, 65u, 1025u, 8192u})
      for (uint32_t n : {1u, 2u, 257u, 4096u, 0xFFFFFFFFu}) {
        const uint32_t b = vc_distinct_batch(budget, kp), nb = vc_distinct_n_batches(n, budget, kp);
        CHECK(b >= 1);
        CHECK(b == 1 || 8ull * kp * b <= budget);                       // within the budget, but always one row
        CHECK(b == 0xFFFFFFFFu || 8ull * kp * ((uint64_t)b + 1) > budget);   // and no smaller than it has to be
        CHECK((uint64_t)nb * b >= n && (uint64_t)(nb - 1) * b < n);       // the sub-batches cover the round, none is empty
        const uint64_t bytes = vc_distinct_rows_bytes(n, budget, kp);
        CHECK(bytes == 8ull * kp * (n < b ? n : b));
        // the driver's walk visits every query once
        if (nb <= 100000) {
          uint64_t seen = 0;
          for (uint64_t first = 0; first < n; first += b) seen += (n - first < b ? n - first : b);
          CHECK(seen == n);
        }
      }
}

int main() {
  schedule();
  classes();
  hash();
  verdict();
  batches();
  printf("distinct plan ok:\nWAVE %u\nBLOCK %u\nMAXK %u\n", VC_DISTINCT_WAVE_MAX, VC_DISTINCT_BLOCK_MAX, VC_DISTINCT_MAX_K);
  return 0;
}
