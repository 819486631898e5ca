// csrc/vc_vote_plan.hpp on the CPU, host code only: built with -fsanitize=address,undefined by tests/test_vote_cpu.py.  The argument
// checks, the weight and the 32-bit tally limit, the winner key at its extremes and its order against the three rules spelled out, the
// team shape and the bin of every length, the table slots and their half-full bound, a table filled to that bound through the slot
// function, the scratch sizes and the staging layouts.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <tuple>
#include <vector>

#include "vc_vote_plan.hpp"

#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
      exit(1);                                                  \
    }                                                           \
  } while (0)

static void arguments() {
  CHECK(!vc_vote_k_ok(0, 8192) && vc_vote_k_ok(1, 8192) && vc_vote_k_ok(8192, 8192) && !vc_vote_k_ok(8193, 8192));
  CHECK(!vc_vote_kk_ok(10, 0) && vc_vote_kk_ok(10, 1) && vc_vote_kk_ok(10, 10) && !vc_vote_kk_ok(10, 11));
  CHECK(vc_vote_kind_ok(0) && vc_vote_kind_ok(1) && !vc_vote_kind_ok(2) && !vc_vote_kind_ok(0xFFFFFFFFu));
  CHECK(vc_vote_lp_flags_ok(0) && vc_vote_lp_flags_ok(1) && !vc_vote_lp_flags_ok(2) && !vc_vote_lp_flags_ok(3) && !vc_vote_lp_flags_ok(0x80000000u));
  CHECK(!vc_vote_iters_ok(0) && vc_vote_iters_ok(1) && vc_vote_iters_ok(64) && !vc_vote_iters_ok(65));
  CHECK(vc_vote_row_count(0, 10) == 0 && vc_vote_row_count(3, 10) == 3 && vc_vote_row_count(10, 10) == 10 && vc_vote_row_count(1ull << 40, 10) == 10);
  CHECK(vc_vote_row_entries(3, 10) == 3 && vc_vote_row_entries(10, 3) == 3 && vc_vote_row_entries(1, 0) == 0);
}

static void weights() {
  for (uint32_t bits : {64u, 128u, 256u, 512u}) {
    CHECK(vc_vote_weight(VC_VOTE_KIND_COUNT, bits, 0) == 1 && vc_vote_weight(VC_VOTE_KIND_COUNT, bits, bits) == 1);
    CHECK(vc_vote_weight(VC_VOTE_KIND_CLOSENESS, bits, 0) == bits + 1 && vc_vote_weight(VC_VOTE_KIND_CLOSENESS, bits, bits) == 1);
    const uint64_t longest = 0xFFFFFFFFull / (bits + 1);
    CHECK(vc_vote_length_ok(longest, bits) && !vc_vote_length_ok(longest + 1, bits) && longest * (bits + 1) <= 0xFFFFFFFFull);
    CHECK(longest < (1ull << 31));   // so a position fits the key's 31 bits
  }
  CHECK(vc_vote_length_ok(0, 64) && !vc_vote_length_ok(0xFFFFFFFFFFFFFFFFull, 64));
}

// the three rules spelled out on (tally, is-current, first position)
static bool before(std::tuple<uint32_t, bool, uint32_t> a, std::tuple<uint32_t, bool, uint32_t> b) {
  if (std::get<0>(a) != std::get<0>(b)) return std::get<0>(a) > std::get<0>(b);
  if (std::get<1>(a) != std::get<1>(b)) return std::get<1>(a);
  return std::get<2>(a) < std::get<2>(b);
}
static void keys() {
  const uint64_t top = vc_vote_key(0xFFFFFFFFu, true, 0);
  CHECK(top == 0xFFFFFFFFFFFFFFFFull && vc_vote_key_tally(top) == 0xFFFFFFFFu && vc_vote_key_current(top) && vc_vote_key_pos(top) == 0);
  const uint64_t low = vc_vote_key(1, false, 0x7FFFFFFFu);
  CHECK(low == (1ull << 32) && low != 0 && vc_vote_key_pos(low) == 0x7FFFFFFFu && !vc_vote_key_current(low));
  std::vector<std::tuple<uint32_t, bool, uint32_t>> all;
  for (uint32_t tally : {1u, 2u, 65u, 513u * 8192u, 0xFFFFFFFFu})
    for (bool cur : {false, true})
      for (uint32_t pos : {0u, 1u, 63u, 8191u, 66076419u, 0x7FFFFFFFu}) all.push_back({tally, cur, pos});
  for (auto a : all)
    for (auto b : all) {
      const uint64_t ka = vc_vote_key(std::get<0>(a), std::get<1>(a), std::get<2>(a)), kb = vc_vote_key(std::get<0>(b), std::get<1>(b), std::get<2>(b));
      CHECK((ka > kb) == before(a, b) && (ka == kb) == (a == b));
      CHECK(vc_vote_key_tally(ka) == std::get<0>(a) && vc_vote_key_current(ka) == std::get<1>(a) && vc_vote_key_pos(ka) == std::get<2>(a));
    }
  CHECK(!vc_vote_is_tie(vc_vote_key(3, false, 0), 1) && vc_vote_is_tie(vc_vote_key(3, false, 0), 2) && !vc_vote_is_tie(vc_vote_key(3, true, 0), 2));
}

static void shapes() {
  CHECK(vc_vote_team_lanes(0) == 8 && vc_vote_team_lanes(8) == 8 && vc_vote_team_lanes(9) == 16 && vc_vote_team_lanes(10) == 16 && vc_vote_team_lanes(33) == 64 &&
        vc_vote_team_lanes(64) == 64);
  uint32_t last = 0;
  for (uint64_t len = 0; len <= 20000; ++len) {
    const uint32_t bin = vc_vote_bin(len);
    CHECK(bin >= last && bin < VC_VOTE_BINS);
    last = bin;
    if (bin < VC_VOTE_BIN_LONG) {
      CHECK(len <= vc_vote_bin_max(bin) && (bin == 0 || len > vc_vote_bin_max(bin - 1)));
      if (bin <= VC_VOTE_BIN_P64) CHECK(vc_vote_team_lanes(vc_vote_bin_max(bin)) == vc_vote_bin_max(bin) && 64 % vc_vote_bin_max(bin) == 0);
      else CHECK(vc_vote_slots(len) * VC_VOTE_SLOT_BYTES <= vc_vote_lds_bytes(vc_vote_bin_max(bin)));
    } else {
      CHECK(len > VC_VOTE_BIG_MAX);
    }
    const uint64_t s = vc_vote_slots(len);
    CHECK((s & (s - 1)) == 0 && s >= VC_VOTE_MIN_SLOTS && s >= 2 * len && (s == VC_VOTE_MIN_SLOTS || s < 4 * len) && (1ull << vc_vote_log2(s)) == s);
  }
  CHECK(vc_vote_bin(64) == VC_VOTE_BIN_P64 && vc_vote_bin(65) == VC_VOTE_BIN_WAVE && vc_vote_bin(256) == VC_VOTE_BIN_WAVE && vc_vote_bin(257) == VC_VOTE_BIN_SMALL);
  CHECK(vc_vote_bin(1024) == VC_VOTE_BIN_SMALL && vc_vote_bin(1025) == VC_VOTE_BIN_BIG && vc_vote_bin(8192) == VC_VOTE_BIN_BIG && vc_vote_bin(8193) == VC_VOTE_BIN_LONG);
  CHECK(vc_vote_bin(1ull << 40) == VC_VOTE_BIN_LONG);
  CHECK(vc_vote_lds_bytes(VC_VOTE_WAVE_MAX) == 4096 && vc_vote_lds_bytes(VC_VOTE_SMALL_MAX) == 16384 && vc_vote_lds_bytes(VC_VOTE_BIG_MAX) == 131072);
  CHECK(vc_vote_lds_bytes(65) == 2048 && vc_vote_lds_bytes(100) == 2048 && vc_vote_lds_bytes(8191) == 131072);
  CHECK(vc_vote_table_threads(65) == 64 && vc_vote_table_threads(256) == 64 && vc_vote_table_threads(257) == 256 && vc_vote_table_threads(8192) == 256);
}

// a table filled to its half-full bound with distinct labels through vc_vote_slot_of and linear probing: every probe ends, every
// label is found again, and one label alone takes every add in one slot
static void tables() {
  for (uint64_t len : {1ull, 65ull, 1024ull, 8192ull, 8193ull}) {
    const uint64_t s = vc_vote_slots(len);
    const uint32_t lg = vc_vote_log2(s), mask = (uint32_t)s - 1;
    std::vector<uint32_t> label(s, VC_VOTE_LABEL_NONE), tally(s, 0);
    uint64_t probes = 0;
    for (uint64_t e = 0; e < len; ++e) {
      const uint32_t lab = (uint32_t)(e * 2654435761ull + 12345);
      uint32_t h = vc_vote_slot_of(lab, lg);
      CHECK(h < s);
      while (label[h] != VC_VOTE_LABEL_NONE && label[h] != lab) { h = (h + 1) & mask; ++probes; CHECK(probes < s * len); }
      label[h] = lab;
      tally[h] += 1;
    }
    uint64_t used = 0;
    for (uint64_t i = 0; i < s; ++i) used += label[i] != VC_VOTE_LABEL_NONE;
    CHECK(used <= len && 2 * used <= s);
    printf("TABLE %llu %llu %u\n", (unsigned long long)len, (unsigned long long)s, lg);
  }
  CHECK(vc_vote_slot_of(0, 6) < 64 && vc_vote_slot_of(0xFFFFFFFEu, 6) < 64 && vc_vote_slot_of(0xFFFFFFFEu, 31) < (1u << 31));
}

static void sizes() {
  CHECK(vc_vote_plan_blocks(0) == 0 && vc_vote_plan_blocks(1) == 1 && vc_vote_plan_blocks(256) == 1 && vc_vote_plan_blocks(257) == 2);
  CHECK(vc_vote_plan_count_words(700) == 8 * 3);
  CHECK(vc_vote_lp_stat_bytes() == 128 + 64 * 64 && VC_VOTE_PLAN_STAT_BYTES >= 8 * (VC_VOTE_BINS + 1) + 8);
  CHECK(vc_vote_long_cap(0) == 1 && vc_vote_long_cap(8192) == 1 && vc_vote_long_cap(8193) == 2 && vc_vote_long_cap(3 * 8193 + 5) == 4);
  for (uint64_t n : {1ull, 2ull, 700ull, 8200ull, 1000000ull})
    printf("SCRATCH %llu %llu %llu\n", (unsigned long long)n, (unsigned long long)vc_vote_lp_bytes(n), (unsigned long long)vc_vote_long_bytes(2, vc_vote_slots(8193) + vc_vote_slots(n)));
  for (bool with_counts : {false, true}) {
    const VcVoteStage L(33, 10, 701, with_counts);
    CHECK(L.rows == 0 && L.labels == 33 * 10 * 8 && L.out_label == L.labels + 2808 && L.out_votes == L.out_label + 136 && L.out_total == L.out_votes + 136);
    CHECK(L.counts == L.out_total + 136 && L.total == L.counts + (with_counts ? 136 : 0));
    CHECK(L.labels % 8 == 0 && L.out_label % 8 == 0 && L.counts % 8 == 0);
    printf("STAGE %d %llu\n", (int)with_counts, (unsigned long long)L.total);
  }
  CHECK(VcVoteStage(0, 10, 0, false).total == 8);
  const VcVoteLpStage P(701, 12345);
  CHECK(P.offsets == 0 && P.adj == 702 * 8 && P.labels_in == P.adj + 12345 * 8 && P.labels_out == P.labels_in + 2808 && P.votes == P.labels_out + 2808 &&
        P.totals == P.votes + 2808 && P.total == P.totals + 2808);
  printf("LPSTAGE %llu\n", (unsigned long long)P.total);
}

int main() {
  arguments();
  weights();
  keys();
  shapes();
  tables();
  sizes();
  printf("vote plan ok: TEAM %u WAVE %u SMALL %u BIG %u MIN_SLOTS %u BINS %u STAT %u\n", VC_VOTE_TEAM_MAX, VC_VOTE_WAVE_MAX, VC_VOTE_SMALL_MAX, VC_VOTE_BIG_MAX,
         VC_VOTE_MIN_SLOTS, (unsigned)VC_VOTE_BINS, VC_VOTE_STAT_BYTES);
  return 0;
}
