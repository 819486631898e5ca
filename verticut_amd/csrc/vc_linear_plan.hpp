// Plan, state layout and recovery arithmetic of the linear scan driver (LinearSearch in vc_engine.hip): what the host driver,
// the launchers of vc_scan.hip and the kernels' parameter fills share.  Plain C++ on purpose -- no HIP type, no HIP call -- so
// that the arithmetic also compiles into a stand-alone host program (tests/cpp/linear_plan_test.cc).
#pragma once
#include <stddef.h>
#include <stdint.h>

#define VC_SHIST_COPIES 16       // partial histograms per bootstrap stage (spreads the flush atomics over L2 channels)
// The linear path gives every query its own 128-byte line for its threshold and for its ring cursor: both are read /
// updated coherently by every wave that enters the rare path, coherent traffic to one line is served by ONE memory
// channel, and eight queries sharing a line overloaded that channel enough to slow the whole (channel-interleaved)
// code stream by 5-14 % depending on where the allocation happened to land (tools/placement_probe.py).
#define VC_QUERY_LINE_WORDS 32u
// Queries whose bootstrap is done by ONE pair of sampling launches: the tiles of a group share them (the stage
// kernels read the sampled prefix once per 32 queries instead of once per tile) and one select launch.
#define VC_GROUP_QUERIES 64u
#define VC_RESIDENT_MB_DEFAULT 240   // of the 256 MB Infinity Cache (profiles/r02_sweeps.md: 224-256 MB best, 320 MB thrashes)
#define VC_REC_BINS 2048u
#define VC_REC_MAXQ 64u              // = VC_GROUP_QUERIES: queries one select / recover launch serves
// The exact-MIH cost-model switch scans 32 queries per pass: a pass of 8 sits on the HBM roofline, but the switch is asked for
// QUERIES, and per query the VALU-bound pass of 32 is the cheaper one (8.2 ms per 32 against 2.5 ms per 8 at 1e9 x 128 bit:
// 3 900 against 3 200 queries/s)
#define VC_FALLBACK_TILE 32u

static inline uint64_t vc_plan_min(uint64_t a, uint64_t b) { return a < b ? a : b; }
static inline uint64_t vc_plan_max(uint64_t a, uint64_t b) { return a > b ? a : b; }

// Queries per database pass.  An explicit tile (vc_config.query_tile, VC_QUERY_TILE, the MIH switch's VC_FALLBACK_TILE) is taken
// as it is; 0 leaves it to the engine.  A pass over a BIG database is priced by its bytes and 32 queries keep it near the
// VALU / HBM balance point; a pass over a small one is priced by its launches (~50 us of bootstrap / verify / select / recover
// whatever it reads), so the tile grows as the database shrinks: 32 from 256 MB on, doubling per halving below, at most 512 --
// configs[0] (8 MB, 200 queries per call) runs in ONE pass instead of seven: 0.42 -> 0.92 M queries/s (1.3 M with the lane tile
// of vc_scan_pick_shape fitted to it as well).
static inline uint32_t vc_linear_tile(uint64_t n, uint32_t bits, uint32_t explicit_tile) {
  if (explicit_tile) return explicit_tile;
  const uint64_t bytes = vc_plan_max(n, 1) * (bits / 8);
  uint32_t t = 32;
  for (uint64_t b = bytes; b < ((uint64_t)256 << 20) && t < 512; b <<= 1) t <<= 1;
  return t;
}

// What one linear search call is run by.  The VC_SAMPLE1 / VC_SAMPLE2 dev knobs come in as values (set == false: not given).
struct LinearPlanIn {
  uint64_t n;              // records in the database
  uint32_t bits, nq, k;
  uint32_t ring_cap;       // the engine's candidate ring (vc_config.cand_cap)
  uint32_t explicit_tile;  // 0 = the tile follows the database size
  bool sample1_set, sample2_set;
  uint64_t sample1, sample2;
};

struct LinearPlan {
  uint64_t n;
  uint32_t QT, GQ;         // queries per tile (one verify launch), per group (one bootstrap, one select)
  uint32_t cap, hs;        // ring entries per query, histogram stride (words)
  bool tile_auto;
  // Threshold bootstrap: exact distance histogram of the first `sample` codes -> tau (k-th best of the sample), so that
  // the verify kernel's first tiles do not flood the ring / histogram atomics from every wave at once (that flood cost
  // ~0.4 ms per launch while eight queries shared one line for their ring cursors and one for their thresholds).
  // Round 1 ran two stages (64 K codes exactly, then 2 M codes counting only distances <= tau1): 4 launches, 26 us.
  // With one line per query the flood is mild and the threshold of ONE exact stage over 1 M codes starts the verify
  // kernel just as well -- 2 launches, 15 us; a 125 M-code shard step 0.397 -> 0.384 ms, 1e9 unchanged
  // (profiles/r02_sweeps.md; below 512 K codes the verify pass pays for the looser threshold, beyond 1 M nothing is
  // gained -- an exact threshold makes a 1e9 pass no faster).  The refining stage stays selectable (VC_SAMPLE2, tests).
  uint64_t sample, sample2;   // sample2 == 0: no refining stage

  explicit LinearPlan(const LinearPlanIn& in) : n(in.n), tile_auto(in.explicit_tile == 0) {
    hs = (in.bits + 1 + 7) & ~7u;
    QT = (uint32_t)vc_plan_min(vc_linear_tile(in.n, in.bits, in.explicit_tile), in.nq);
    GQ = (uint32_t)vc_plan_min(in.nq, vc_plan_max(QT, VC_GROUP_QUERIES / QT * QT));   // whole tiles, >= one tile
    cap = (uint32_t)vc_plan_max(in.ring_cap, 4ull * in.k);
    sample = vc_plan_min(in.n, vc_plan_max(vc_plan_max(262144, 64ull * in.k), vc_plan_min(in.n / 16, 1048576)));
    sample2 = in.sample2_set ? vc_plan_min(in.n, in.sample2) : 0;
    if (in.sample1_set) sample = vc_plan_min(in.n, in.sample1);
    else if (sample2) sample = vc_plan_min(sample, vc_plan_max(65536, 64ull * in.k));   // stage 1 only has to seed stage 2
  }
  // The database size the verify kernel's shape is fitted to: the shape follows a small database only where the TILE does too
  // -- query_tile left to the engine -- and only for tiles beyond the small-tile form: explicit tiles and <= 8 queries keep the
  // headline's kernel, on any database.
  uint64_t shape_n(uint32_t qt) const { return (tile_auto && qt > 8) ? n : 0; }
};

// Per-group state of the linear scan, one allocation: count lines | hist | shist copies | shist2 copies | tau lines (word
// offsets).  count[GQ] and tau[GQ] hold one 128-byte line per query, the histograms are dense: row q of hist at hist + q * hs,
// row q of partial copy c of a group of gq queries at shist + (c * gq + q) * hs.
struct LinearState {
  uint32_t GQ, hs;
  size_t count = 0, hist = 0, shist = 0, shist2 = 0, tau = 0, state_words = 0;

  constexpr LinearState(uint32_t gq_max, uint32_t hist_stride) : GQ(gq_max), hs(hist_stride) {
    count = 0;
    hist = count + (size_t)GQ * VC_QUERY_LINE_WORDS;
    shist = hist + (size_t)GQ * hs;
    shist2 = shist + (size_t)VC_SHIST_COPIES * GQ * hs;
    const size_t hist_end = shist2 + (size_t)VC_SHIST_COPIES * GQ * hs;
    tau = (hist_end + VC_QUERY_LINE_WORDS - 1) & ~(size_t)(VC_QUERY_LINE_WORDS - 1);   // keeps tau[] line-aligned
    state_words = tau + tau_words();
  }
  constexpr size_t tau_words() const { return (size_t)GQ * VC_QUERY_LINE_WORDS; }
  // distance between the partial bootstrap histograms of a group of gq queries
  uint64_t shist_copy_stride(uint32_t gq) const { return (uint64_t)gq * hs; }

  // the state of the queries from q0 of the group on: a tile at t0, a recover chunk at c0
  struct At { size_t count, hist, shist, tau; };
  At at(uint32_t q0) const {
    return At{count + (size_t)q0 * VC_QUERY_LINE_WORDS, hist + (size_t)q0 * hs, shist + (size_t)q0 * hs,
              tau + (size_t)q0 * VC_QUERY_LINE_WORDS};
  }
};
// what the kernels assume of it: they step through count[] and tau[] in whole 128-byte lines
static_assert(VC_QUERY_LINE_WORDS == 32 && (VC_QUERY_LINE_WORDS & (VC_QUERY_LINE_WORDS - 1)) == 0,
              "count[] / tau[] stride: one 128-byte line per query");
static_assert(LinearState(5, 136).tau % VC_QUERY_LINE_WORDS == 0 && LinearState(5, 136).tau >= LinearState(5, 136).shist2 + 16 * 5 * 136 &&
              LinearState(64, 72).tau % VC_QUERY_LINE_WORDS == 0 && LinearState(200, 520).tau % VC_QUERY_LINE_WORDS == 0,
              "tau[] starts on a line of its own behind the histograms, whatever the group and the histogram stride");
static_assert(VC_REC_MAXQ == VC_GROUP_QUERIES, "one recover launch serves the queries of one default group");

// "The state is already clean": the last kernel of a linear step (vc_recover_kernel) hands the group's state back zeroed, with
// the threshold lines at ~0, so the next step needs no memset -- as long as it carves the same buffer the same way.
struct CleanState {
  const uint32_t* ptr = nullptr;
  uint32_t GQ = 0, hs = 0;
  bool matches(const uint32_t* state, const LinearState& s) const { return ptr && ptr == state && GQ == s.GQ && hs == s.hs; }
  void set(const uint32_t* state, const LinearState& s) { ptr = state; GQ = s.GQ; hs = s.hs; }
  void invalidate() { ptr = nullptr; }
};

// Scratch of the device-side ring-overflow recovery (vc_recover_kernel), word offsets: idhist [MAXQ][3][BINS] | rcount, one line
// per query | three barrier lines (arrivals, give-up flag, departures) | the sticky give-up counter's line.
struct VcRecoverScratch {
  static constexpr size_t idhist = 0;
  static constexpr size_t rcount = idhist + (size_t)VC_REC_MAXQ * 3 * VC_REC_BINS;
  static constexpr size_t bar = rcount + (size_t)VC_REC_MAXQ * VC_QUERY_LINE_WORDS;
  static constexpr size_t bar_words = 3 * VC_QUERY_LINE_WORDS;
  static constexpr size_t gave_up = bar + bar_words;
  static constexpr size_t words = gave_up + VC_QUERY_LINE_WORDS;
};

// Ring-overflow recovery (host-driven, rare: more than `cap` items at or below the k-th distance).  The truncated
// ring still yields a valid upper bound on the k-th best packed value (the k-th best of what fitted); the query is
// scanned again appending only packed values <= a probe, and the append counter tells EXACTLY how many items lie at
// or below the probe whether they fitted or not.  Per query an interval (lo, hi] is kept with count(<= lo) < k <=
// count(<= hi):
//   * probe = hi; the k-th best of what fitted becomes the new hi.  With entries arriving in random order that
//     quarters the survivors per round (cap >= 4k); but arrival order is NOT random (the same early waves deliver
//     ids just under the limit round after round: tests/campaign/parity_campaign.py case 259 needed > 64 rounds), so
//   * whenever a round fails to halve the survivors the next probe bisects (lo, hi] instead: fewer than k items
//     below it -> lo = probe; otherwise hi = min(probe, k-th best of what fitted).
// Each bisection halves a 64-bit interval, the other steps never widen it: it ends (the driver gives up beyond
// VC_RECOVER_MAX_ROUNDS all the same).
#define VC_RECOVER_MAX_ROUNDS 200
struct RecoverInterval {
  uint64_t lo = 0, hi;     // count(<= lo) < k (valid only if has_lo), count(<= hi) >= k
  bool has_lo = false;
  uint64_t prev = 0;       // survivors of the previous valid round (0 = none yet)
  bool bisect = false;     // the next probe is a midpoint, not hi
  uint64_t probe = 0;
  enum Outcome { DONE, TRUNCATED, UNDERSHOOT };   // DONE / TRUNCATED: the round's row is valid (TRUNCATED: not yet the final one)

  explicit RecoverInterval(uint64_t kth_of_truncated_row) : hi(kth_of_truncated_row) {}

  uint64_t next_probe() {
    if (!bisect) probe = hi;                                       // bound
    else if (has_lo) probe = lo + (hi - lo + 1) / 2;               // rounds up: lo < probe <= hi, so the interval always shrinks
    else if (hi >> 32) probe = ((hi >> 32) << 32) - 1;             // first: everything strictly nearer than hi's distance
    else probe = hi / 2;
    return probe;
  }
  // count_le_probe: exact number of items <= probe; kth_fitted: the k-th best of what the ring kept of them
  Outcome update(uint64_t count_le_probe, uint64_t kth_fitted, uint32_t cap, uint64_t want) {
    if (count_le_probe < want) {                                   // only a bisection probe can undershoot
      lo = probe;
      has_lo = true;
      bisect = true;
      return UNDERSHOOT;
    }
    // a valid row: everything <= probe was counted, the best min(count, cap) >= k of it was stored
    if (count_le_probe <= cap) return DONE;                        // nothing was dropped: exact
    hi = kth_fitted < probe ? kth_fitted : probe;
    bisect = prev != 0 && count_le_probe * 2 > prev;               // poor progress since the last valid round -> bisect next
    prev = count_le_probe;
    return TRUNCATED;
  }
};
