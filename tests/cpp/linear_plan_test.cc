// Stand-alone check of the linear scan driver's host arithmetic (verticut_amd/csrc/vc_linear_plan.hpp): the plan of a call
// (tile, group, histogram stride, bootstrap sample), the carving of the per-group state, the recovery scratch layout and the
// interval arithmetic of the host-driven ring-overflow recovery, driven here against a simulated scan.  Plain C++ with its own
// main: build it with -fsanitize=address,undefined to have every index it forms checked.  Exit status 0 = all checks hold.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../verticut_amd/csrc/vc_linear_plan.hpp"

static int g_bad = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++g_bad; } \
  } while (0)

static LinearPlan plan(uint64_t n, uint32_t bits, uint32_t nq, uint32_t k, uint32_t tile, uint32_t ring_cap = 65536) {
  LinearPlanIn in{};
  in.n = n; in.bits = bits; in.nq = nq; in.k = k; in.ring_cap = ring_cap; in.explicit_tile = tile;
  return LinearPlan(in);
}

static void check_plan_values() {
  // tile left to the engine: 32 from 256 MB on, doubling per halving below, at most 512
  const struct { uint64_t n; uint32_t bits, tile; } tiles[] = {
      {1ull << 20, 64, 512}, {1ull << 20, 128, 512}, {1ull << 22, 128, 128}, {1ull << 24, 128, 32}, {1000000000ull, 128, 32}};
  for (const auto& t : tiles) CHECK(vc_linear_tile(t.n, t.bits, 0) == t.tile);
  for (uint32_t t : {1u, 4u, 8u, 11u, 32u, 4096u}) {   // an explicit tile is returned unchanged, on any database
    CHECK(vc_linear_tile(1ull << 20, 128, t) == t);
    CHECK(vc_linear_tile(1000000000ull, 64, t) == t);
  }
  // queries per group: whole tiles, at least one, at most the batch
  const struct { uint32_t qt, nq, gq; } groups[] = {{8, 200, 64}, {11, 200, 55}, {32, 200, 64}, {4, 5, 5}, {32, 40, 40}, {4096, 4096, 4096}};
  for (const auto& g : groups) {
    const LinearPlan p = plan(1000000000ull, 128, g.nq, 10, g.qt);
    CHECK(p.GQ == g.gq);
    CHECK(p.QT == std::min(g.qt, g.nq) && !p.tile_auto);
    CHECK(p.shape_n(p.QT) == 0);                       // explicit tiles keep the headline's shape
  }
  {
    const LinearPlan p = plan(1ull << 20, 64, 200, 10, 0);   // auto tile 512, 200 queries: one pass
    CHECK(p.QT == 200 && p.GQ == 200 && p.tile_auto);
    CHECK(p.shape_n(200) == (1ull << 20) && p.shape_n(8) == 0 && p.shape_n(9) == (1ull << 20));
  }
  const struct { uint32_t bits, hs; } strides[] = {{64, 72}, {128, 136}, {256, 264}, {512, 520}};
  for (const auto& s : strides) CHECK(plan(1000, s.bits, 1, 1, 0).hs == s.hs);
  CHECK(plan(1000, 128, 1, 100, 0, 65536).cap == 65536 && plan(1000, 128, 1, 100, 0, 300).cap == 400);
  // bootstrap sample
  const struct { uint64_t n; uint32_t k; uint64_t sample; } samples[] = {{1000000000ull, 100, 1048576}, {1ull << 20, 100, 262144}, {1000, 10, 1000}};
  for (const auto& s : samples) {
    const LinearPlan p = plan(s.n, 128, 8, s.k, 0);
    CHECK(p.sample == s.sample && p.sample2 == 0);
  }
  for (uint32_t k : {100u, 8192u}) {                    // a refining stage and no VC_SAMPLE1: stage 1 only seeds it
    LinearPlanIn in{};
    in.n = 1000000000ull; in.bits = 128; in.nq = 8; in.k = k; in.ring_cap = 65536;
    in.sample2_set = true; in.sample2 = 2000000;
    LinearPlan p(in);
    CHECK(p.sample2 == 2000000 && p.sample == std::max<uint64_t>(65536, 64ull * k));
    in.sample1_set = true; in.sample1 = 5000;           // VC_SAMPLE1 is taken as given
    p = LinearPlan(in);
    CHECK(p.sample == 5000 && p.sample2 == 2000000);
    in.n = 3000;                                        // never more than the database
    p = LinearPlan(in);
    CHECK(p.sample == 3000 && p.sample2 == 3000);
  }
}

static void check_state_layout() {
  const struct { uint32_t gq, hs; } shapes[] = {{5, 136}, {64, 72}, {200, 520}};
  for (const auto& s : shapes) {
    const LinearState st(s.gq, s.hs);
    // ascending, non-overlapping: count lines | hist | shist copies | shist2 copies | tau lines
    CHECK(st.count == 0 && st.hist == st.count + (size_t)s.gq * VC_QUERY_LINE_WORDS);
    CHECK(st.shist == st.hist + (size_t)s.gq * s.hs);
    CHECK(st.shist2 == st.shist + (size_t)VC_SHIST_COPIES * s.gq * s.hs);
    CHECK(st.tau >= st.shist2 + (size_t)VC_SHIST_COPIES * s.gq * s.hs && st.tau % 32 == 0);
    CHECK(st.state_words == st.tau + st.tau_words() && st.tau_words() == (size_t)s.gq * 32);
    // the size the driver has always allocated
    const size_t hist_words = (((size_t)s.gq * (1 + 2 * (size_t)VC_SHIST_COPIES) * s.hs) + 31) & ~(size_t)31;
    CHECK(st.state_words == (size_t)s.gq * 2 * VC_QUERY_LINE_WORDS + hist_words);
    CHECK(st.tau == (size_t)s.gq * VC_QUERY_LINE_WORDS + hist_words);
    // every word a tile / recover chunk touches lies inside its region: walk a real array of the planned size
    std::vector<unsigned char> owner(st.state_words, 0);
    for (uint32_t q = 0; q < s.gq; ++q) {
      const LinearState::At at = st.at(q);
      for (uint32_t w = 0; w < VC_QUERY_LINE_WORDS; ++w) { ++owner[at.count + w]; ++owner[at.tau + w]; }
      for (uint32_t w = 0; w < s.hs; ++w) ++owner[at.hist + w];
      for (uint32_t c = 0; c < VC_SHIST_COPIES; ++c)
        for (uint32_t w = 0; w < s.hs; ++w) {
          ++owner[at.shist + c * st.shist_copy_stride(s.gq) + w];
          ++owner[st.shist2 + (st.at(q).shist - st.shist) + c * st.shist_copy_stride(s.gq) + w];
        }
    }
    size_t twice = 0, unused = 0;
    for (unsigned char o : owner) { twice += o > 1; unused += o == 0; }
    CHECK(twice == 0 && unused < 32);                   // nothing shared; only the padding in front of tau[] is nobody's
    CHECK(st.at(0).count == st.count && st.at(3).tau == st.tau + 3 * 32 && st.at(3).hist == st.hist + 3 * (size_t)s.hs);
  }
  // a smaller last group of the same layout packs its partial histograms closer: still inside the shist region
  const LinearState st(64, 136);
  CHECK(st.shist + (VC_SHIST_COPIES - 1) * st.shist_copy_stride(6) + 6 * 136 <= st.shist2);
  // the clean-state record
  CleanState clean;
  uint32_t buf[2];
  CHECK(!clean.matches(buf, st));
  clean.set(buf, st);
  CHECK(clean.matches(buf, st) && clean.matches(buf, LinearState(64, 136)));
  CHECK(!clean.matches(buf, LinearState(40, 136)) && !clean.matches(buf, LinearState(64, 72)) && !clean.matches(buf + 1, st));
  clean.invalidate();
  CHECK(!clean.matches(buf, st));
}

static void check_scratch_layout() {
  CHECK(VcRecoverScratch::words == (size_t)VC_REC_MAXQ * 3 * VC_REC_BINS + (size_t)VC_REC_MAXQ * 32 + 96 + 32);
  CHECK(VcRecoverScratch::gave_up == VcRecoverScratch::words - 32);                  // the give-up line is the last 32 words
  CHECK(VcRecoverScratch::bar == (size_t)VC_REC_MAXQ * 3 * VC_REC_BINS + (size_t)VC_REC_MAXQ * 32 && VcRecoverScratch::bar_words == 96);
  CHECK(VcRecoverScratch::idhist == 0 && VcRecoverScratch::rcount == (size_t)VC_REC_MAXQ * 3 * VC_REC_BINS);
  CHECK(VcRecoverScratch::bar + VcRecoverScratch::bar_words == VcRecoverScratch::gave_up);
}

// ---- the recovery interval against a simulated scan ------------------------------------------------------------------
// `vals`: the database's packed values, sorted, distinct.  A probing scan counts everything <= probe exactly and its ring keeps
// `cap` of those values: which ones is the arrival order's business.
struct Sim {
  std::vector<uint64_t> vals;
  uint32_t cap;
  bool adversarial;
  uint64_t rng;
  uint64_t next() { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return rng >> 33; }
  // returns the count; *kept: what the ring holds, ascending
  uint64_t scan(uint64_t probe, std::vector<uint64_t>* kept) {
    const size_t c = (size_t)(std::upper_bound(vals.begin(), vals.end(), probe) - vals.begin());
    kept->assign(vals.begin(), vals.begin() + c);
    if (c > cap) {
      if (adversarial) {
        kept->erase(kept->begin(), kept->end() - cap);          // the early waves deliver the values just under the limit
      } else {
        for (size_t i = 0; i < cap; ++i) std::swap((*kept)[i], (*kept)[i + next() % (c - i)]);
        kept->resize(cap);
        std::sort(kept->begin(), kept->end());
      }
    }
    return c;
  }
};

// drives one query the way linear_recover does; returns the number of rounds, *bisected: rounds whose probe was a midpoint
static int recover_one(Sim& sim, uint32_t k, std::vector<uint64_t>* row, int* bisected) {
  const uint64_t want = std::min<uint64_t>(k, sim.vals.size());
  std::vector<uint64_t> kept;
  sim.scan(UINT64_MAX, &kept);                                   // the first pass: an unlimited scan, its ring truncated
  RecoverInterval iv(kept[k - 1]);
  *bisected = 0;
  for (int round = 0; round <= VC_RECOVER_MAX_ROUNDS; ++round) {
    const uint64_t lo = iv.has_lo ? iv.lo : 0, hi = iv.hi;
    const bool had_lo = iv.has_lo;
    *bisected += iv.bisect;
    const uint64_t probe = iv.next_probe();
    CHECK(probe <= hi && (!had_lo || lo < probe));               // lo < probe <= hi
    const uint64_t c = sim.scan(probe, &kept);
    const uint64_t kth = kept.size() >= k ? kept[k - 1] : UINT64_MAX;
    const RecoverInterval::Outcome o = iv.update(c, kth, sim.cap, want);
    CHECK(iv.hi <= hi && (!had_lo || iv.lo >= lo));              // the interval never widens
    CHECK(!iv.has_lo || iv.lo < iv.hi);
    if (o != RecoverInterval::UNDERSHOOT) row->assign(kept.begin(), kept.begin() + want);
    if (o == RecoverInterval::DONE) return round + 1;
  }
  CHECK(!"the recovery did not end within the driver's limit");
  return VC_RECOVER_MAX_ROUNDS + 1;
}

static void check_recovery(size_t n, uint32_t k, uint32_t cap, bool adversarial, bool expect_bisect) {
  Sim sim{{}, cap, adversarial, 88172645463325252ull + n * 31 + k};
  // distinct packed values: distances 20..27 in the high word (thousands of ties per distance), ids in the low word
  for (size_t i = 0; i < n; ++i) sim.vals.push_back(((uint64_t)(20 + i * 8 / n) << 32) | (uint32_t)(7 + 3 * i));
  std::sort(sim.vals.begin(), sim.vals.end());
  std::vector<uint64_t> row;
  int bisected = 0;
  const int rounds = recover_one(sim, k, &row, &bisected);
  const size_t want = std::min<size_t>(k, n);
  CHECK(row.size() == want && std::equal(row.begin(), row.end(), sim.vals.begin()));   // the k smallest values
  CHECK(rounds <= VC_RECOVER_MAX_ROUNDS + 1);
  if (expect_bisect) CHECK(bisected > 0);                        // the adversarial order has teeth: it takes the bisect branch
  printf("recovery n=%zu k=%u cap=%u %s: %d rounds, %d of them bisecting\n", n, k, cap, adversarial ? "adversarial" : "random", rounds, bisected);
}

int main() {
  check_plan_values();
  check_state_layout();
  check_scratch_layout();
  for (int adversarial = 0; adversarial < 2; ++adversarial) {
    check_recovery(5000, 100, 400, adversarial, adversarial);
    check_recovery(5000, 1, 4, adversarial, adversarial);
    check_recovery(300, 100, 400, adversarial, false);           // smaller than the ring: one bounding round ends it
  }
  printf(g_bad ? "%d checks FAILED\n" : "linear plan: all checks hold\n", g_bad);
  return g_bad ? 1 : 0;
}
