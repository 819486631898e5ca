// csrc/vc_mst_condense_plan.hpp on the CPU, host code only: built with -fsanitize=address,undefined by tests/test_mst_condense_cpu.py.
// The argument checks at their limits, the bound on the nodes against the caller's buffer, the level table from a first-edge table
// (every weight of a 512-bit code, one weight, none), the tags of the claims, the stability and the tie rule, the bit counts of the node
// sort, the scratch sizes and the staging layout.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "vc_mst_condense_plan.hpp"

#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
      exit(1);                                                  \
    }                                                           \
  } while (0)

static void arguments() {
  CHECK(!vc_cond_mcs_ok(0) && !vc_cond_mcs_ok(1) && vc_cond_mcs_ok(2) && vc_cond_mcs_ok(5) && vc_cond_mcs_ok(0x80000000u) && !vc_cond_mcs_ok(0x80000001u) &&
        !vc_cond_mcs_ok(0xFFFFFFFFu));
  CHECK(vc_cond_root_weight_ok(0, 64) && vc_cond_root_weight_ok(65, 64) && !vc_cond_root_weight_ok(66, 64) && vc_cond_root_weight_ok(513, 512) &&
        !vc_cond_root_weight_ok(514, 512) && !vc_cond_root_weight_ok(0xFFFFFFFFu, 512));
  CHECK(vc_cond_method_ok(VC_COND_EOM) && vc_cond_method_ok(VC_COND_LEAF) && !vc_cond_method_ok(2) && !vc_cond_method_ok(0x80000000u));
  CHECK(vc_cond_edge_cap(0) == 0 && vc_cond_edge_cap(1) == 0 && vc_cond_edge_cap(2) == 1 && vc_cond_edge_cap(3000) == 2999);
  CHECK(vc_cond_edges_ok(0, 0) && !vc_cond_edges_ok(0, 1) && vc_cond_edges_ok(1, 0) && !vc_cond_edges_ok(1, 1) && vc_cond_edges_ok(3000, 2999) &&
        !vc_cond_edges_ok(3000, 3000) && !vc_cond_edges_ok(3000, 1ull << 40) && !vc_cond_edges_ok(3000, 0xFFFFFFFFFFFFFFFFull));
  CHECK(vc_cond_root_above(0, 64) && vc_cond_root_above(65, 64) && !vc_cond_root_above(64, 64) && !vc_cond_root_above(1, 64) && vc_cond_root_above(1, 0) &&
        vc_cond_root_above(513, 512));
}

static void nodes() {
  CHECK(vc_cond_node_bound(0, 2) == 0 && vc_cond_node_bound(1, 2) == 0 && vc_cond_node_bound(2, 2) == 1 && vc_cond_node_bound(3, 2) == 1 &&
        vc_cond_node_bound(4, 2) == 3 && vc_cond_node_bound(3000, 5) == 1199 && vc_cond_node_bound(2048, 2) == 2047 && vc_cond_node_bound(3000, 0x80000000u) == 0);
  // the caller's buffer of max(n, 1) - 1 records always holds the bound
  for (uint64_t n : {0ull, 1ull, 2ull, 3ull, 4ull, 5ull, 71ull, 2048ull, 3000ull, 1000000ull, 0xFFFFFFFFull})
    for (uint32_t mcs : {2u, 3u, 5u, 25u, 0x80000000u}) CHECK(vc_cond_node_bound(n, mcs) <= vc_cond_node_cap(n));
  CHECK(vc_cond_node_cap(0) == 0 && vc_cond_node_cap(1) == 0 && vc_cond_node_cap(3000) == 2999);
}

static void levels() {
  // no edge: no level
  std::vector<uint32_t> first(513, VC_COND_NONE);
  std::vector<VcCondLevel> rows(513);
  CHECK(vc_cond_levels(first.data(), 512, 0, rows.data()) == 0);
  // one weight, the largest
  first[512] = 0;
  CHECK(vc_cond_levels(first.data(), 512, 7, rows.data()) == 1 && rows[0].weight == 512 && rows[0].first == 0 && rows[0].count == 7);
  // every weight of a 512-bit code, w + 1 edges of weight w
  uint32_t at = 0;
  for (uint32_t w = 0; w <= 512; ++w) {
    first[w] = at;
    at += w + 1;
  }
  CHECK(vc_cond_levels(first.data(), 512, at, rows.data()) == 513);
  for (uint32_t w = 0; w <= 512; ++w) CHECK(rows[w].weight == w && rows[w].count == w + 1 && rows[w].first == w * (w + 1) / 2);
  // gaps: weights 3, 4 and 64 of a 64-bit code
  std::vector<uint32_t> few(65, VC_COND_NONE);
  few[3] = 0; few[4] = 10; few[64] = 11;
  CHECK(vc_cond_levels(few.data(), 64, 2999, rows.data()) == 3);
  CHECK(rows[0].weight == 3 && rows[0].first == 0 && rows[0].count == 10 && rows[1].weight == 4 && rows[1].first == 10 && rows[1].count == 1 && rows[2].weight == 64 &&
        rows[2].first == 11 && rows[2].count == 2988);
  // the tags ascend through a level and from one level to the next, above the zero the arrays start with
  uint32_t before_old = 0, before_new = 0;
  for (uint32_t l = 0; l <= 513; ++l) {
    CHECK(vc_cond_tag_tally(l) > before_old && vc_cond_tag_apply(l) > vc_cond_tag_tally(l) && vc_cond_tag_new(l) > before_new);
    before_old = vc_cond_tag_apply(l);
    before_new = vc_cond_tag_new(l);
  }
}

static void stabilities() {
  // a leaf of 5 records formed at 3 that took 2 more at 7 and ended at 10: 10 * 7 - (3 * 5 + 7 * 2)
  CHECK(vc_cond_stability(10, 7, 3 * 5 + 7 * 2, false, 0) == 41 && vc_cond_stability(10, 7, 29, true, 11) == 41 && vc_cond_stability(0, 7, 29, true, 0) == 0);
  CHECK(vc_cond_stability(3, 5, 15, false, 0) == 0);   // ended where it formed
  // the extremes: 2^32 - 1 records formed at 0, ended at 513
  CHECK(vc_cond_stability(513, 0xFFFFFFFFu, 0, true, 513) == 513ull * 0xFFFFFFFFull);
  CHECK(vc_cond_allowed(false, 0) && vc_cond_allowed(false, 9) && vc_cond_allowed(true, 9) && !vc_cond_allowed(true, 0));
  CHECK(vc_cond_keep(5, 5, true) && vc_cond_keep(6, 5, true) && !vc_cond_keep(4, 5, true) && !vc_cond_keep(9, 0, false) && vc_cond_keep(0, 0, true));   // a tie goes to the parent
}

static void bits_and_sizes() {
  CHECK(vc_cond_form_bits(64) == 7 && vc_cond_form_bits(128) == 8 && vc_cond_form_bits(256) == 9 && vc_cond_form_bits(512) == 10);
  for (uint32_t bits : {64u, 128u, 256u, 512u}) CHECK((bits >> vc_cond_form_bits(bits)) == 0);   // every bit of the largest level is sorted on
  CHECK(vc_cond_rep_bits(0, 0) == 1 && vc_cond_rep_bits(0, 1) == 0 && vc_cond_rep_bits(0, 3000) == 12 && vc_cond_rep_bits(1000, 3000) == 12 &&
        vc_cond_rep_bits(0xFFFFEC78u, 3000) == 32 && vc_cond_rep_bits(0xFFFFFFFFu, 1) == 32);
  for (uint32_t id_base : {0u, 40u, 0xFFFFEC78u})
    for (uint64_t n : {1ull, 2ull, 3000ull}) CHECK((((uint64_t)id_base + n - 1) >> vc_cond_rep_bits(id_base, n)) == 0);
  CHECK(vc_cond_words4(0) == 0 && vc_cond_words4(1) == 8 && vc_cond_words4(2) == 8 && vc_cond_words4(3) == 16);
  CHECK(vc_cond_work_bytes(3000) == 12 * 12000 && vc_cond_work_bytes(3) == 12 * 16);
  CHECK(vc_cond_plan_bytes(64) == 264 && vc_cond_plan_bytes(512) == 2056);
  CHECK(vc_cond_scratch_nodes(0) == 1 && vc_cond_scratch_nodes(1) == 1 && vc_cond_scratch_nodes(2) == 1 && vc_cond_scratch_nodes(3000) == 2999);
  CHECK(vc_cond_tree_bytes(3001) == 3000 * 40 + 4 * 12000 + 3000 * 8 && vc_cond_tree_bytes(1) == 40 + 4 * 8 + 8);
  CHECK(vc_cond_sort_bytes(3001) == 2 * (3000 * 8 + 12000) && vc_cond_sort_bytes(1) == 2 * (8 + 8));
  const VcCondStage a(3000, 2999), b(1, 0), c(3, 1);
  CHECK(a.edges == 0 && a.nodes == 2999 * 16 && a.labels == a.nodes + 2999 * 48 && a.node == a.labels + 12000 && a.own == a.node + 12000 && a.leave == a.own + 12000 &&
        a.total == a.leave + 12000);
  CHECK(b.nodes == 0 && b.labels == 0 && b.node == 8 && b.total == 32);
  CHECK(c.nodes == 16 && c.labels == 16 + 96 && c.total == 16 + 96 + 4 * 16);
}

int main() {
  arguments();
  nodes();
  levels();
  stabilities();
  bits_and_sizes();
  printf("condense plan ok: NODE %u STAT %u WORK_NODE %u RECORD_WORDS %u\n", VC_COND_NODE_BYTES, VC_COND_HOST_STAT_BYTES, VC_COND_WORK_NODE_BYTES, VC_COND_RECORD_WORDS);
  const uint64_t ns[] = {1, 2, 513, 2048, 3000, 9000, 1000000};
  for (uint64_t n : ns)
    printf("SCRATCH %llu %llu %llu %llu %llu\n", (unsigned long long)n, (unsigned long long)vc_cond_work_bytes(n), (unsigned long long)vc_cond_tree_bytes(n),
           (unsigned long long)vc_cond_sort_bytes(n), (unsigned long long)VcCondStage(n, n - 1).total);
  for (uint32_t mcs : {2u, 5u, 25u}) printf("BOUND %u %llu\n", mcs, (unsigned long long)vc_cond_node_bound(3000, mcs));
  return 0;
}
