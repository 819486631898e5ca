// csrc/vc_snn_plan.hpp on the CPU, host code only: built with -fsanitize=address,undefined by tests/test_snn_cpu.py.
// The argument checks, the set's size and the home slot, a replay of the set's insert and probe loops over rows of every kind, the
// team shapes at their edges, the LDS bytes, the grid and the staging layout.
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <vector>

#include "vc_snn_plan.hpp"

#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
      exit(1);                                                  \
    }                                                           \
  } while (0)

static const uint32_t B = VC_SNN_WAVE_KK, M = VC_SNN_PLAN_MAX_KK;

static void arguments() {
  CHECK(!vc_snn_kk_ok(10, 0) && vc_snn_kk_ok(10, 1) && vc_snn_kk_ok(10, 10) && !vc_snn_kk_ok(10, 11));
  CHECK(vc_snn_kk_ok(M, M) && vc_snn_kk_ok(8191, M) && !vc_snn_kk_ok(8191, M + 1) && !vc_snn_kk_ok(8191, 8191) && !vc_snn_kk_ok(1, 0xFFFFFFFFu));
  CHECK(vc_snn_flags_ok(0) && vc_snn_flags_ok(1) && !vc_snn_flags_ok(2) && !vc_snn_flags_ok(3) && !vc_snn_flags_ok(0x80000000u));
}

// the kernel's loops, word for word, over a table of exactly vc_snn_table_slots(kk) words: ASan sees any step outside it
static void insert(std::vector<uint32_t>& tab, uint32_t shift, uint32_t x, uint32_t* steps) {
  const uint32_t mask = (uint32_t)tab.size() - 1;
  uint32_t h = vc_snn_slot(x, shift);
  for (;;) {
    CHECK(++*steps <= tab.size());
    if (tab[h] == VC_SNN_PLAN_NONE) { tab[h] = x; return; }
    if (tab[h] == x) return;
    h = (h + 1) & mask;
  }
}
static bool holds(const std::vector<uint32_t>& tab, uint32_t shift, uint32_t x) {
  const uint32_t mask = (uint32_t)tab.size() - 1;
  uint32_t h = vc_snn_slot(x, shift), steps = 0;
  for (;;) {
    CHECK(++steps <= tab.size());
    if (tab[h] == x) return true;
    if (tab[h] == VC_SNN_PLAN_NONE) return false;
    h = (h + 1) & mask;
  }
}

static void the_set() {
  uint64_t state = 12345;
  auto rnd = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(state >> 33); };
  const uint32_t kks[] = {1, 2, 3, 10, 31, 32, 33, 63, 64, 65, 100, B - 1, B, B + 1, 511, 512, 513, M - 1, M};
  for (uint32_t kk : kks) {
    const uint32_t slots = vc_snn_table_slots(kk), shift = vc_snn_table_shift(kk);
    CHECK(slots >= 2 * kk && slots < 4 * kk + 2 && (slots & (slots - 1)) == 0 && slots == 1u << (32 - shift) && shift >= 21 && shift <= 31);
    CHECK(slots <= (vc_snn_wave_team(kk) ? VC_SNN_WAVE_SLOTS : VC_SNN_BLOCK_SLOTS));
    for (int kind = 0; kind < 4; ++kind) {
      // 0: random positions; 1: consecutive ones; 2: a regular stride; 3: one id kk times (no graph row: the set holds it once)
      std::vector<uint32_t> row(kk);
      for (uint32_t t = 0; t < kk; ++t) row[t] = kind == 0 ? rnd() % 0xFFFFFFFFu : kind == 1 ? 1000 + t : kind == 2 ? t * slots * 7u : 77u;
      std::vector<uint32_t> tab(slots, VC_SNN_PLAN_NONE);
      std::set<uint32_t> want;
      for (uint32_t x : row) {
        uint32_t steps = 0;
        CHECK(vc_snn_slot(x, shift) < slots);
        insert(tab, shift, x, &steps);
        want.insert(x);
      }
      uint32_t taken = 0;
      for (uint32_t w : tab) taken += w != VC_SNN_PLAN_NONE;
      CHECK(taken == want.size() && 2 * taken <= slots);                                  // at most half full
      for (uint32_t x : row) CHECK(holds(tab, shift, x));
      for (int t = 0; t < 200; ++t) {
        const uint32_t x = rnd() % 0xFFFFFFFFu;
        CHECK(holds(tab, shift, x) == (want.count(x) != 0));
      }
    }
  }
  CHECK(vc_snn_table_slots(1) == 2 && vc_snn_table_slots(64) == 128 && vc_snn_table_slots(65) == 256 && vc_snn_table_slots(M) == 2 * M);
}

static void teams() {
  CHECK(vc_snn_wave_team(1) && vc_snn_wave_team(B) && !vc_snn_wave_team(B + 1) && !vc_snn_wave_team(M));
  CHECK(vc_snn_team_waves(B) == 1 && vc_snn_rows_per_block(B) == 4 && vc_snn_team_waves(B + 1) == 4 && vc_snn_rows_per_block(B + 1) == 1);
  for (uint32_t kk = 1; kk <= M; ++kk) {
    const uint32_t p = vc_snn_entry_lanes(kk);
    CHECK(p >= 1 && p <= 64 && (p & (p - 1)) == 0 && 64 % p == 0 && (p >= kk || p == 64) && (p < 2 * kk));
    CHECK(vc_snn_team_waves(kk) * vc_snn_rows_per_block(kk) * VC_SNN_WAVE == VC_SNN_BLOCK);
  }
  CHECK(vc_snn_entry_lanes(1) == 1 && vc_snn_entry_lanes(10) == 16 && vc_snn_entry_lanes(32) == 32 && vc_snn_entry_lanes(33) == 64 && vc_snn_entry_lanes(M) == 64);
  CHECK(VC_SNN_LDS_BYTES_WAVE == 4608 && VC_SNN_LDS_BYTES_BLOCK == 12288 && VC_SNN_LDS_BYTES_BLOCK <= 65536);
  CHECK(vc_snn_grid(0, 10) == 1 && vc_snn_grid(1, 10) == 1 && vc_snn_grid(4, 10) == 1 && vc_snn_grid(5, 10) == 2 && vc_snn_grid(5, B + 1) == 5);
  CHECK(vc_snn_grid(0xFFFFFFFFull, 10) == 4096 && vc_snn_grid(0xFFFFFFFFull, M) == 4096);
}

static void staging() {
  const VcSnnStage all(5, 7, 3, true, true, true);
  CHECK(all.rows == 0 && all.counts == 280 && all.shared == 304 && all.hist == 368 && all.total == 392);
  const VcSnnStage none(5, 7, 3, false, false, false);
  CHECK(none.counts == 280 && none.shared == 280 && none.hist == 280 && none.total == 280);
  const VcSnnStage big(0xFFFFFFFFull, 8191, M, true, true, true);                       // no wrap at the widest shapes
  CHECK(big.total > big.hist && big.hist > big.shared && big.shared > big.counts && big.counts == 0xFFFFFFFFull * 8191 * 8);
  for (uint64_t n = 1; n < 40; ++n)
    for (uint32_t kk = 1; kk < 9; ++kk) {
      const VcSnnStage s(n, kk + 1, kk, n & 1, n & 2, n & 4);
      CHECK(s.counts % 8 == 0 && s.shared % 8 == 0 && s.hist % 8 == 0 && s.total % 8 == 0);
      CHECK(s.shared - s.counts >= ((n & 1) ? n * 4 : 0) && s.hist - s.shared >= ((n & 2) ? n * kk * 4 : 0) && s.total - s.hist == ((n & 4) ? kk * 8 : 0));
    }
}

int main() {
  arguments();
  the_set();
  teams();
  staging();
  printf("snn plan ok: WAVE_KK %u MAX_KK %u STAT %u\n", VC_SNN_WAVE_KK, VC_SNN_PLAN_MAX_KK, VC_SNN_STAT_BYTES);
  const uint32_t kks[] = {1, 64, 65, B, B + 1, M};
  for (uint32_t kk : kks) printf("TEAM %u %u %u %u\n", kk, vc_snn_table_slots(kk), vc_snn_team_waves(kk), vc_snn_entry_lanes(kk));
  printf("STAGE %llu\n", (unsigned long long)VcSnnStage(700, 70, 64, true, true, true).total);
  return 0;
}
