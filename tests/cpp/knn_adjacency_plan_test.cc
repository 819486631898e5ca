// csrc/vc_knn_adjacency_plan.hpp on the CPU, host code only: built with -fsanitize=address,undefined by
// tests/test_knn_adjacency_cpu.py.  The argument checks and the 2^31 - 1 limit, the passes of the sort, the bound and the scratch
// sizes, the lanes of the mutual compaction, the team boundary of the merge with a replay of its rank counting over rows of every
// kind, and the staging layout.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "vc_knn_adjacency_plan.hpp"

#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
      exit(1);                                                  \
    }                                                           \
  } while (0)

static void arguments() {
  CHECK(!vc_adj_kk_ok(10, 0) && vc_adj_kk_ok(10, 1) && vc_adj_kk_ok(10, 10) && !vc_adj_kk_ok(10, 11) && vc_adj_kk_ok(8191, 8191));
  CHECK(vc_adj_flags_ok(0) && vc_adj_flags_ok(1) && vc_adj_flags_ok(2) && !vc_adj_flags_ok(3) && !vc_adj_flags_ok(0x80000000u));
  // the limit: n kk <= 2^31 - 1, with no overflow on the way
  CHECK(vc_adj_items_ok(0, 8191) && vc_adj_items_ok(1, 1) && vc_adj_items_ok(0x7FFFFFFFull, 1) && !vc_adj_items_ok(0x80000000ull, 1));
  CHECK(vc_adj_items_ok(214748364ull, 10) && !vc_adj_items_ok(214748365ull, 10));                  // 2 147 483 640 / 2 147 483 650
  CHECK(vc_adj_items_ok(262176ull, 8191) && !vc_adj_items_ok(262177ull, 8191));                    // 2 147 483 616 / 2 147 491 807
  CHECK(!vc_adj_items_ok(0xFFFFFFFFFFFFFFFFull, 2) && !vc_adj_items_ok(1ull << 63, 8191) && !vc_adj_items_ok(1ull << 32, 0x80000000u));
  CHECK(!vc_adj_sorts(VC_ADJ_MUTUAL) && vc_adj_sorts(VC_ADJ_EITHER) && vc_adj_sorts(VC_ADJ_REVERSE));
}

static void passes() {
  CHECK(vc_adj_bitlength(0) == 0 && vc_adj_bitlength(1) == 1 && vc_adj_bitlength(255) == 8 && vc_adj_bitlength(256) == 9 &&
        vc_adj_bitlength(0x7FFFFFFFull) == 31 && vc_adj_bitlength(0xFFFFFFFFFFFFFFFFull) == 64);
  // one distance pass up to 128-bit codes, two for 256 and 512 bits; a cap below the width counts
  CHECK(vc_adj_passes(vc_adj_dist_bits(0xFFFFFFFFu, 64)) == 1 && vc_adj_passes(vc_adj_dist_bits(0xFFFFFFFFu, 128)) == 1);
  CHECK(vc_adj_passes(vc_adj_dist_bits(0xFFFFFFFFu, 256)) == 2 && vc_adj_passes(vc_adj_dist_bits(0xFFFFFFFFu, 512)) == 2);
  CHECK(vc_adj_passes(vc_adj_dist_bits(255, 512)) == 1 && vc_adj_passes(vc_adj_dist_bits(256, 512)) == 2 && vc_adj_passes(vc_adj_dist_bits(0, 64)) == 0);
  // the keys are 0 .. n, the sentinel included
  CHECK(vc_adj_passes(vc_adj_key_bits(1)) == 1 && vc_adj_passes(vc_adj_key_bits(255)) == 1 && vc_adj_passes(vc_adj_key_bits(256)) == 2);
  CHECK(vc_adj_passes(vc_adj_key_bits(65535)) == 2 && vc_adj_passes(vc_adj_key_bits(65536)) == 3 && vc_adj_passes(vc_adj_key_bits(66000)) == 3);
  CHECK(vc_adj_passes(vc_adj_key_bits(1000000)) == 3 && vc_adj_passes(vc_adj_key_bits(0x7FFFFFFFull)) == 4);
  for (uint64_t n : {1ull, 2ull, 255ull, 256ull, 65535ull, 65536ull, 16777215ull, 16777216ull})
    CHECK((n >> (8 * vc_adj_passes(vc_adj_key_bits(n)))) == 0);                                    // every bit of the sentinel is sorted on
  CHECK(vc_adj_sort_passes(1000000, 0xFFFFFFFFu, 64) == 4 && vc_adj_sort_passes(66000, 0xFFFFFFFFu, 512) == 5);
}

static void sizes() {
  CHECK(vc_adj_bound(1000, 10, VC_ADJ_REVERSE) == 10000 && vc_adj_bound(1000, 10, VC_ADJ_MUTUAL) == 10000 && vc_adj_bound(1000, 10, VC_ADJ_EITHER) == 20000);
  CHECK(vc_adj_bound(262176ull, 8191, VC_ADJ_EITHER) == 2ull * 2147483616ull);                     // beyond 32 bits of nothing: T stays below 2^32
  CHECK(vc_adj_bound(262176ull, 8191, VC_ADJ_EITHER) < (1ull << 32));
  CHECK(vc_adj_item_bytes(1000, 10, VC_ADJ_REVERSE, 1) == 24ull * 10000 && vc_adj_item_bytes(1000, 10, VC_ADJ_EITHER, 5) == 24ull * 10000);
  CHECK(vc_adj_item_bytes(1000, 10, VC_ADJ_MUTUAL, 10000) == 0 && vc_adj_item_bytes(1000, 10, VC_ADJ_REVERSE, 0) == 0);   // no sort buffers
  CHECK(vc_adj_item_bytes(214748364ull, 10, VC_ADJ_REVERSE, 1) == 24ull * 2147483640ull);
  CHECK(vc_adj_counter_words(1000, VC_ADJ_REVERSE) == 1001 && vc_adj_counter_words(1000, VC_ADJ_MUTUAL) == 1001 && vc_adj_counter_words(1000, VC_ADJ_EITHER) == 2002);
  CHECK(VC_ADJ_SORT_LDS_BYTES == 55316 && VC_ADJ_SORT_LDS_BYTES < VC_ADJ_SORT_LDS_LIMIT && VC_ADJ_SORT_TILE * 12 == 48 * 1024);
  CHECK(vc_adj_row_lanes(1) == 1 && vc_adj_row_lanes(2) == 2 && vc_adj_row_lanes(3) == 4 && vc_adj_row_lanes(10) == 16 && vc_adj_row_lanes(32) == 32 &&
        vc_adj_row_lanes(33) == 64 && vc_adj_row_lanes(64) == 64 && vc_adj_row_lanes(65) == 64 && vc_adj_row_lanes(8191) == 64);
  for (uint32_t kk = 1; kk <= 8191; ++kk) {
    const uint32_t p = vc_adj_row_lanes(kk);
    CHECK((p & (p - 1)) == 0 && p <= VC_ADJ_WAVE && (p >= kk || p == VC_ADJ_WAVE) && VC_ADJ_WAVE % p == 0);
  }
  const VcAdjStage a(700, 12, 10, VC_ADJ_EITHER, 1ull << 40, true), b(700, 12, 10, VC_ADJ_REVERSE, 100, false), c(700, 12, 10, VC_ADJ_MUTUAL, 0, true);
  CHECK(a.cap == 14000 && b.cap == 100 && c.cap == 0);
  CHECK(a.rows == 0 && a.offsets == 700 * 12 * 8 && a.adj == a.offsets + 701 * 8 && a.counts == a.adj + 14000 * 8 && a.total == a.counts + 2800);
  CHECK(b.total == 700 * 12 * 8 + 701 * 8 + 800 && c.total == 700 * 12 * 8 + 701 * 8 + 2800);
  CHECK(VcAdjStage(3, 2, 2, VC_ADJ_REVERSE, 6, true).total == 48 + 32 + 48 + 16);                  // three counts take two 8-byte words
}

// the merge's rank counting, word for word: A (a row's listed entries) and B (the sorted in-part) share no word; every word's
// place is its index plus its rank in the other list.  The output has exactly |A| + |B| words: ASan sees any place outside it.
static uint32_t rank_in(const std::vector<uint64_t>& list, uint64_t x) {
  uint32_t lo = 0, hi = (uint32_t)list.size();
  while (lo < hi) {
    const uint32_t mid = (lo + hi) / 2;
    if (list[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}
static void merge_replay(uint32_t na, uint32_t nb, uint32_t seed) {
  std::vector<uint64_t> all;
  uint64_t x = seed;
  for (uint32_t i = 0; i < na + nb; ++i) {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    all.push_back((((x >> 40) % 7) << 32) | i);            // few distances: many ties, every id once
  }
  std::vector<uint64_t> A, B;
  for (uint32_t i = 0; i < na + nb; ++i) ((i * 2654435761u >> 16) % (na + nb) < na && A.size() < na ? A : B).push_back(all[i]);
  while (A.size() < na) { A.push_back(B.back()); B.pop_back(); }
  std::sort(A.begin(), A.end());
  std::sort(B.begin(), B.end());
  std::sort(all.begin(), all.end());
  std::vector<uint64_t> out(A.size() + B.size(), ~0ull);
  const uint32_t team = vc_adj_block_team((uint32_t)out.size()) ? VC_ADJ_BLOCK : VC_ADJ_WAVE;
  for (uint32_t t = 0; t < team; ++t) {
    for (uint32_t i = t; i < A.size(); i += team) out[i + rank_in(B, A[i])] = A[i];
    for (uint32_t i = t; i < B.size(); i += team) out[i + rank_in(A, B[i])] = B[i];
  }
  CHECK(out == all);
}
static void teams() {
  CHECK(!vc_adj_block_team(0) && !vc_adj_block_team(VC_ADJ_TEAM_DEGREE) && vc_adj_block_team(VC_ADJ_TEAM_DEGREE + 1) && vc_adj_block_team(0xFFFFFFFFu));
  const uint32_t D = VC_ADJ_TEAM_DEGREE;
  const uint32_t shapes[][2] = {{0, 0}, {1, 0}, {0, 1}, {5, 0}, {0, 9000}, {5, 8520}, {10, 3}, {10, D - 10}, {10, D - 9}, {100, 100}, {8191, 40000}};
  for (const auto& s : shapes) merge_replay(s[0], s[1], s[0] * 31 + s[1]);
}

int main() {
  arguments();
  passes();
  sizes();
  teams();
  printf("knn adjacency plan ok: MAX_ITEMS %llu TEAM_DEGREE %u STAT %u LDS %u\n", (unsigned long long)VC_ADJ_MAX_ITEMS, VC_ADJ_TEAM_DEGREE, VC_ADJ_STAT_BYTES,
         VC_ADJ_SORT_LDS_BYTES);
  const uint64_t ns[] = {1, 2, 71, 2000, 9000, 66000, 1000000};
  for (uint64_t n : ns)
    for (uint32_t bits : {64u, 128u, 256u, 512u})
      printf("PASSES %llu %u %u %u %u\n", (unsigned long long)n, bits, vc_adj_passes(vc_adj_dist_bits(0xFFFFFFFFu, bits)), vc_adj_passes(vc_adj_dist_bits(bits / 4, bits)),
             vc_adj_passes(vc_adj_key_bits(n)));
  for (uint32_t flags = 0; flags < 3; ++flags)
    printf("SCRATCH %u %llu %llu %llu %llu\n", flags, (unsigned long long)vc_adj_bound(9000, 5, flags), (unsigned long long)vc_adj_item_bytes(9000, 5, flags, 1),
           (unsigned long long)vc_adj_counter_words(9000, flags), (unsigned long long)VcAdjStage(9000, 5, 5, flags, 50000, true).total);
  for (uint32_t kk : {1u, 5u, 10u, 33u, 100u}) printf("LANES %u %u\n", kk, vc_adj_row_lanes(kk));
  return 0;
}
