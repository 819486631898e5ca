// csrc/vc_knn_mst_plan.hpp on the CPU, host code only: built with -fsanitize=address,undefined by tests/test_knn_mst_cpu.py.  The
// argument checks and the 2^31 - 1 limit, the edge key at its extremes (weight 512, home index 2^31 - 2) and its order, the home rule
// over all cases, the weights, the round bound, the bit counts of the final sort, the scratch sizes and the staging layouts.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <tuple>
#include <vector>

#include "vc_knn_mst_plan.hpp"

#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
      exit(1);                                                  \
    }                                                           \
  } while (0)

static void arguments() {
  CHECK(!vc_mst_kk_ok(10, 0) && vc_mst_kk_ok(10, 1) && vc_mst_kk_ok(10, 10) && !vc_mst_kk_ok(10, 11) && vc_mst_kk_ok(8191, 8191));
  CHECK(vc_mst_flags_ok(0) && vc_mst_flags_ok(1) && !vc_mst_flags_ok(2) && !vc_mst_flags_ok(3) && !vc_mst_flags_ok(0x80000001u));   // VC_KNN_REVERSE is refused
  CHECK(vc_mst_kind_ok(0) && vc_mst_kind_ok(1) && !vc_mst_kind_ok(2) && !vc_mst_kind_ok(0xFFFFFFFFu));
  CHECK(vc_mst_min_pts_ok(VC_MST_KIND_DISTANCE, 10, 1) && !vc_mst_min_pts_ok(VC_MST_KIND_DISTANCE, 10, 0) && !vc_mst_min_pts_ok(VC_MST_KIND_DISTANCE, 10, 2));
  CHECK(vc_mst_min_pts_ok(VC_MST_KIND_REACHABILITY, 10, 1) && vc_mst_min_pts_ok(VC_MST_KIND_REACHABILITY, 10, 11) && !vc_mst_min_pts_ok(VC_MST_KIND_REACHABILITY, 10, 12) &&
        !vc_mst_min_pts_ok(VC_MST_KIND_REACHABILITY, 10, 0) && vc_mst_min_pts_ok(VC_MST_KIND_REACHABILITY, 8191, 8192));
  CHECK(vc_mst_items_ok(0, 8191) && vc_mst_items_ok(1, 1) && vc_mst_items_ok(0x7FFFFFFFull, 1) && !vc_mst_items_ok(0x80000000ull, 1));
  CHECK(vc_mst_items_ok(214748364ull, 10) && !vc_mst_items_ok(214748365ull, 10));
  CHECK(vc_mst_items_ok(262176ull, 8191) && !vc_mst_items_ok(262177ull, 8191));
  CHECK(!vc_mst_items_ok(0xFFFFFFFFFFFFFFFFull, 2) && !vc_mst_items_ok(1ull << 63, 8191));
}

static void keys() {
  // the largest weight (the tenth bit) and the largest home index the limit admits: n kk = 2^31 - 1, the last entry is 2^31 - 2
  const uint64_t n = 0x7FFFFFFFull;
  const uint64_t top = vc_mst_key(512, n - 1, 1, 0);
  CHECK(top == ((512ull << 32) | 0x7FFFFFFEull) && vc_mst_key_weight(top) == 512 && vc_mst_key_home(top) == 0x7FFFFFFEu);
  CHECK(top != VC_MST_NONE && top < VC_MST_NONE);
  const uint64_t wide = vc_mst_key(512, 262175, 8191, 8190);                 // n = 262176, kk = 8191: 2 147 483 616 entries
  CHECK(vc_mst_key_home(wide) == 2147483615u && vc_mst_home_pos(vc_mst_key_home(wide), 8191) == 262175 && vc_mst_home_entry(vc_mst_key_home(wide), 8191) == 8190);
  CHECK(vc_mst_key_weight(wide) == 512);
  for (uint32_t kk : {1u, 2u, 10u, 100u, 8191u})
    for (uint64_t pos : {0ull, 1ull, 70ull, 262175ull})
      for (uint32_t jj : {0u, kk / 2, kk - 1}) {
        const uint64_t key = vc_mst_key(37, pos, kk, jj);
        CHECK(vc_mst_key_weight(key) == 37 && vc_mst_home_pos(vc_mst_key_home(key), kk) == pos && vc_mst_home_entry(vc_mst_key_home(key), kk) == jj);
      }
  // the key's order is (weight, a, dist, b) when rows ascend in (dist, id): rows of kk = 3 with ties in the distance
  const uint32_t kk = 3;
  const uint32_t row_dist[4][3] = {{1, 1, 2}, {1, 2, 2}, {0, 5, 5}, {2, 2, 2}};
  const uint32_t row_id[4][3] = {{5, 9, 4}, {7, 3, 8}, {6, 1, 2}, {4, 5, 6}};   // ids ascend within one distance
  std::vector<std::pair<uint64_t, std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>>> all;
  for (uint32_t a = 0; a < 4; ++a)
    for (uint32_t jj = 0; jj < kk; ++jj)
      for (uint32_t extra : {0u, 3u}) {   // the weight may exceed the distance (reachability)
        const uint32_t w = row_dist[a][jj] + extra;
        all.push_back({vc_mst_key(w, a, kk, jj), std::make_tuple(w, a, row_dist[a][jj], row_id[a][jj])});
      }
  auto by_key = all, by_tuple = all;
  std::sort(by_key.begin(), by_key.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
  std::stable_sort(by_tuple.begin(), by_tuple.end(), [](const auto& x, const auto& y) { return x.second < y.second; });
  for (size_t t = 0; t < all.size(); ++t) CHECK(by_key[t].second == by_tuple[t].second);
}

static void homes_and_weights() {
  // MUTUAL: an edge iff both list; its home entry is the smaller end's
  CHECK(vc_mst_is_home(VC_MST_MUTUAL, true, true) && !vc_mst_is_home(VC_MST_MUTUAL, false, true) && !vc_mst_is_home(VC_MST_MUTUAL, true, false) &&
        !vc_mst_is_home(VC_MST_MUTUAL, false, false));
  // EITHER: the smaller end's entry always; the larger end's only when the smaller does not list back
  CHECK(vc_mst_is_home(VC_MST_EITHER, true, true) && vc_mst_is_home(VC_MST_EITHER, true, false) && !vc_mst_is_home(VC_MST_EITHER, false, true) &&
        vc_mst_is_home(VC_MST_EITHER, false, false));
  // every pair has exactly one home entry among its listed ones
  for (uint32_t flags : {VC_MST_MUTUAL, VC_MST_EITHER})
    for (int lo_lists = 0; lo_lists < 2; ++lo_lists)
      for (int hi_lists = 0; hi_lists < 2; ++hi_lists) {
        const int homes = (lo_lists && vc_mst_is_home(flags, true, hi_lists)) + (hi_lists && vc_mst_is_home(flags, false, lo_lists));
        const bool is_edge = flags == VC_MST_MUTUAL ? (lo_lists && hi_lists) : (lo_lists || hi_lists);
        CHECK(homes == (is_edge ? 1 : 0));
      }
  CHECK(vc_mst_weight(5, 0, 0) == 5 && vc_mst_weight(5, 7, 3) == 7 && vc_mst_weight(5, 3, 9) == 9 && vc_mst_weight(0, 0, 512) == 512);
  CHECK(vc_mst_core_held(4, 5) && !vc_mst_core_held(3, 5) && vc_mst_core_held(1, 2) && !vc_mst_core_held(0, 2) && vc_mst_core_held(8191, 8192));
}

static void rounds_and_bits() {
  CHECK(vc_mst_ceil_log2(0) == 0 && vc_mst_ceil_log2(1) == 0 && vc_mst_ceil_log2(2) == 1 && vc_mst_ceil_log2(3) == 2 && vc_mst_ceil_log2(4) == 2 &&
        vc_mst_ceil_log2(513) == 10 && vc_mst_ceil_log2(4096) == 12 && vc_mst_ceil_log2(4097) == 13 && vc_mst_ceil_log2(0x7FFFFFFFull) == 31);
  CHECK(vc_mst_round_bound(2) == 2 && vc_mst_round_bound(2000) == 12 && vc_mst_round_bound(1000000) == 21);
  CHECK(vc_mst_weight_bits(64) == 7 && vc_mst_weight_bits(128) == 8 && vc_mst_weight_bits(256) == 9 && vc_mst_weight_bits(512) == 10);
  for (uint32_t bits : {64u, 128u, 256u, 512u}) CHECK((bits >> vc_mst_weight_bits(bits)) == 0);             // every bit of the largest weight is sorted on
  CHECK(vc_mst_home_bits(2000, 10) == 15 && vc_mst_home_bits(1, 1) == 1 && vc_mst_home_bits(0x7FFFFFFFull, 1) == 31 && vc_mst_home_bits(262176, 8191) == 31);
  for (uint64_t n : {1ull, 2ull, 71ull, 2000ull, 1000000ull})
    for (uint32_t kk : {1u, 10u, 100u}) CHECK(((n * kk - 1) >> vc_mst_home_bits(n, kk)) == 0);
}

static void sizes() {
  CHECK(vc_mst_live_bound(2000, 10, VC_MST_EITHER) == 20000 && vc_mst_live_bound(2000, 10, VC_MST_MUTUAL) == 10000 && vc_mst_live_bound(3, 1, VC_MST_MUTUAL) == 1);
  CHECK(vc_mst_live_cap(1, 1, VC_MST_MUTUAL) == 1 && vc_mst_live_cap(1, 1, VC_MST_EITHER) == 1 && vc_mst_live_cap(2000, 10, VC_MST_EITHER) == 20000);
  CHECK(vc_mst_words4(0) == 0 && vc_mst_words4(1) == 8 && vc_mst_words4(2) == 8 && vc_mst_words4(3) == 16);
  CHECK(vc_mst_live_bytes(2000, 10, VC_MST_EITHER) == 2 * (20000 * 8 + 80000) && vc_mst_live_bytes(3, 1, VC_MST_EITHER) == 2 * (24 + 16));
  CHECK(vc_mst_live_bytes(214748364ull, 10, VC_MST_EITHER) == 24ull * 2147483640ull);
  CHECK(vc_mst_forest_bytes(2000) == 16 * 2000 && vc_mst_forest_bytes(3) == 24 + 2 * 16);
  CHECK(vc_mst_pick_items(0) == 0 && vc_mst_pick_items(1) == 0 && vc_mst_pick_items(2000) == 1999 && vc_mst_pick_cap(0) == 1 && vc_mst_pick_cap(1) == 1 &&
        vc_mst_pick_cap(2000) == 1999);
  CHECK(vc_mst_pick_bytes(2001) == 2 * (2000 * 8 + 8000) && vc_mst_pick_bytes(1) == 2 * (8 + 8));
  const VcMstStage a(700, 12, 64, true), b(700, 12, 512, false), c(1, 3, 64, true);
  CHECK(a.rows == 0 && a.edges == 700 * 12 * 8 && a.hist == a.edges + 699 * 16 && a.labels == a.hist + 65 * 8 && a.counts == a.labels + 2800 && a.total == a.counts + 2800);
  CHECK(b.total == 700 * 12 * 8 + 699 * 16 + 513 * 8 + 2800);
  CHECK(c.edges == 24 && c.hist == 24 && c.labels == 24 + 520 && c.total == 24 + 520 + 8 + 8);
  const VcMstCutStage d(700, 699), e(3, 0);
  CHECK(d.edges == 0 && d.labels == 699 * 16 && d.total == 699 * 16 + 2800 && e.labels == 0 && e.total == 16);
}

int main() {
  arguments();
  keys();
  homes_and_weights();
  rounds_and_bits();
  sizes();
  printf("knn mst plan ok: MAX_ITEMS %llu STAT %u EDGE %u\n", (unsigned long long)VC_MST_MAX_ITEMS, VC_MST_STAT_BYTES, VC_MST_EDGE_BYTES);
  const uint64_t ns[] = {1, 2, 71, 513, 2000, 4096, 9000, 1000000};
  for (uint64_t n : ns) printf("ROUNDS %llu %u\n", (unsigned long long)n, vc_mst_round_bound(n));
  for (uint32_t flags = 0; flags < 2; ++flags)
    printf("SCRATCH %u %llu %llu %llu %llu\n", flags, (unsigned long long)vc_mst_live_bytes(9000, 5, flags), (unsigned long long)vc_mst_forest_bytes(9000),
           (unsigned long long)vc_mst_pick_bytes(9000), (unsigned long long)VcMstStage(9000, 5, 64, true).total);
  printf("KEY %llu\n", (unsigned long long)vc_mst_key(512, 0x7FFFFFFEull, 1, 0));
  return 0;
}
