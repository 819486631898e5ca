// Stand-alone check of the MIH memory policy (verticut_amd/csrc/vc_mih_policy.hpp): which of the optional per-table structures --
// bucket-order code copies (bcodes), {id, code} records (bent), directory lines (lines) -- an index gets for a shape, a free-memory
// figure and the three dev knobs.  The rule is restated below in unsigned __int128 from the policy table of DESIGN.md, and every
// expectation comes from that restatement or is written out; the header is never asked what to expect.  Plain C++ with its own
// main: build it with -fsanitize=address,undefined to have the 64-bit products checked.  Exit status 0 = all checks hold.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../verticut_amd/csrc/vc_mih_policy.hpp"

typedef unsigned __int128 u128;

static int g_bad = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++g_bad; } \
  } while (0)

// ---- the rule, restated.  Byte figures of an index of m tables over n records of W 64-bit words:
static u128 bcodes_bytes(u128 m, u128 n, u128 W) { return m * n * W * 8; }      // m more copies of the codes
static u128 bent_bytes(u128 m, u128 n, u128 W) { return m * n * 16 * W; }       // one 16-byte {id, code word} record per word
static u128 lines_bytes(u128 m) { return m * ((u128)1 << 25) * 64; }            // 2^25 lines of 64 bytes per table
static u128 index_bytes(u128 m, u128 n) { return m * (n * 8 + ((u128)1 << 29) + ((u128)3 << 26)); }   // ids, offsets, bitmap, directories
static const u128 LINES_FROM = 300000000;

struct Want { bool bcodes, bent, lines; };

static Want rule(uint32_t sbits, u128 m, u128 n, u128 W, bool have_free, u128 free_b, int k_bcodes, int k_bent, int k_lines) {
  Want w;
  // copies: <= 16-bit substrings, while they take at most a third of the free memory; the knob has the last word
  w.bcodes = sbits <= 16 && (!have_free || 3 * bcodes_bytes(m, n, W) <= free_b);
  if (k_bcodes >= 0) w.bcodes = k_bcodes != 0;
  // records: 32-bit substrings of codes of at most two words, within 55 hundredths of the free memory -- whole hundredths:
  // the division comes first.  The knob cannot force them onto another shape
  const bool bent_shape = sbits == 32 && W <= 2;
  w.bent = bent_shape && (!have_free || bent_bytes(m, n, W) <= (free_b - free_b % 100) / 100 * 55);
  if (k_bent >= 0) w.bent = bent_shape && k_bent != 0;
  // lines: 32-bit substrings of a non-empty index only; the knob decides; else from 3e8 records on, when the free memory is
  // known and four times the lines fit into what the index (with the records, if it gets them) leaves free
  w.lines = false;
  if (sbits == 32 && n != 0) {
    if (k_lines >= 0) {
      w.lines = k_lines != 0;
    } else if (n >= LINES_FROM && have_free) {
      const u128 ib = index_bytes(m, n) + (w.bent ? bent_bytes(m, n, W) : 0);
      w.lines = free_b > ib && 4 * lines_bytes(m) <= free_b - ib;
    }
  }
  return w;
}

// the thresholds: the least free-memory figure at which a structure is built (no knob)
static u128 bcodes_from(u128 m, u128 n, u128 W) { return 3 * bcodes_bytes(m, n, W); }
static u128 bent_from(u128 m, u128 n, u128 W) { return (bent_bytes(m, n, W) + 54) / 55 * 100; }   // whole hundredths: round up
static u128 lines_from(u128 m, u128 n, u128 W, bool with_bent) {
  return index_bytes(m, n) + (with_bent ? bent_bytes(m, n, W) : 0) + 4 * lines_bytes(m);
}

static MihMemPolicy ask(uint32_t sbits, uint32_t m, uint64_t n, uint32_t W, bool have_free, u128 free_b, int kb = -1, int ke = -1, int kl = -1) {
  CHECK(free_b <= UINT64_MAX);
  return vc_mih_policy(sbits, m, n, W, have_free, (uint64_t)free_b, MihPolicyKnobs{kb, ke, kl});
}

static bool same(const MihMemPolicy& p, const Want& w) { return p.bcodes == w.bcodes && p.bent == w.bent && p.lines == w.lines; }
static bool is(const MihMemPolicy& p, bool bcodes, bool bent, bool lines) { return p.bcodes == bcodes && p.bent == bent && p.lines == lines; }

static const uint64_t N_MAX = 0xFFFFFFFFull;   // the ABI's extremes: 2^32 - 1 records, 64 tables, 512-bit codes

static void check_thresholds() {
  // bcodes: m*n*W*8 <= free/3.  Built at the threshold and one byte above, not one byte below
  const struct { uint32_t sbits, m; uint64_t n; uint32_t W; } small[] = {
      {16, 4, 30000, 1}, {8, 8, 20000, 1}, {16, 8, 30000, 2}, {16, 4, 1000000000ull, 1}, {8, 8, 1000000007ull, 1}, {16, 32, 999999937ull, 8},
      {8, 64, N_MAX, 8}};
  for (const auto& c : small) {
    const u128 t = bcodes_from(c.m, c.n, c.W);
    CHECK(t == (u128)3 * c.m * c.n * c.W * 8 && t <= UINT64_MAX);
    CHECK(is(ask(c.sbits, c.m, c.n, c.W, true, t), true, false, false));
    CHECK(is(ask(c.sbits, c.m, c.n, c.W, true, t + 1), true, false, false));
    CHECK(is(ask(c.sbits, c.m, c.n, c.W, true, t + 2), true, false, false));   // (free / 3 steps every third byte)
    CHECK(is(ask(c.sbits, c.m, c.n, c.W, true, t - 1), false, false, false));
    CHECK(is(ask(c.sbits, c.m, c.n, c.W, true, 0), false, false, false));
    CHECK(is(ask(c.sbits, c.m, c.n, c.W, true, UINT64_MAX), true, false, false));
  }
  // bent: m*n*16*W <= free/100*55, the division first.  n below 3e8: no lines to mix in
  const struct { uint32_t m; uint64_t n; uint32_t W; } rec[] = {{4, 30000, 2}, {2, 30000, 1}, {4, 100000000, 2}, {2, 299999999, 1}, {1, 7, 1}, {64, 11, 2}};
  for (const auto& c : rec) {
    const u128 x = bent_bytes(c.m, c.n, c.W), t = bent_from(c.m, c.n, c.W);
    CHECK(t % 100 == 0 && t / 100 * 55 >= x && (t / 100 - 1) * 55 < x);
    CHECK(is(ask(32, c.m, c.n, c.W, true, t), false, true, false));
    CHECK(is(ask(32, c.m, c.n, c.W, true, t + 1), false, true, false));
    CHECK(is(ask(32, c.m, c.n, c.W, true, t + 99), false, true, false));
    CHECK(is(ask(32, c.m, c.n, c.W, true, t - 1), false, false, false));
    // the order of the operations matters: one byte below the threshold free*55/100 would already be enough
    CHECK((t - 1) * 55 / 100 >= x);
  }
  // lines: n >= 3e8, and 4 x the lines within what the index leaves free.  W = 4: no records in the budget
  const struct { uint32_t m; uint64_t n; uint32_t W; } big[] = {{8, 300000000, 4}, {4, 1000000000, 4}, {16, N_MAX, 8}, {64, N_MAX, 8}, {64, 300000000, 3}};
  for (const auto& c : big) {
    const u128 t = lines_from(c.m, c.n, c.W, false);
    CHECK(t == (u128)c.m * (c.n * 8 + (1ull << 29) + (3ull << 26)) + (u128)c.m * (1ull << 33) && t <= UINT64_MAX);
    CHECK(is(ask(32, c.m, c.n, c.W, true, t), false, false, true));
    CHECK(is(ask(32, c.m, c.n, c.W, true, t + 1), false, false, true));
    CHECK(is(ask(32, c.m, c.n, c.W, true, t - 1), false, false, false));
    CHECK(is(ask(32, c.m, c.n, c.W, true, index_bytes(c.m, c.n)), false, false, false));       // free == index: nothing left
    CHECK(is(ask(32, c.m, c.n, c.W, true, index_bytes(c.m, c.n) - 1), false, false, false));   // (the difference would wrap)
    CHECK(is(ask(32, c.m, c.n, c.W, true, 0), false, false, false));
  }
  // the size from which the lines are built unasked
  const u128 roomy = lines_from(4, 1000000000, 2, true) * 4;
  CHECK(is(ask(32, 4, 299999999, 2, true, roomy), false, true, false));
  CHECK(is(ask(32, 4, 300000000, 2, true, roomy), false, true, true));
  CHECK(is(ask(32, 4, 300000001, 2, true, roomy), false, true, true));
  CHECK(is(ask(32, 4, 299999999, 4, true, roomy), false, false, false));
  CHECK(is(ask(32, 4, 300000000, 4, true, roomy), false, false, true));
  CHECK(is(ask(32, 4, 30000, 2, true, roomy), false, true, false));        // the suite's size: no lines without the knob
}

static void check_lines_budget_counts_the_records() {
  // W <= 2: the lines budget counts the {id, code} records exactly when the index gets them -- decided by the free memory or by
  // the knob -- and the two thresholds differ by exactly the records' bytes
  const struct { uint32_t m; uint64_t n; uint32_t W; } cs[] = {{4, 1000000000, 2}, {2, 1000000000, 1}, {4, 300000000, 2}, {64, N_MAX, 2}};
  for (const auto& c : cs) {
    const u128 with = lines_from(c.m, c.n, c.W, true), without = lines_from(c.m, c.n, c.W, false);
    CHECK(with - without == (u128)c.m * c.n * 16 * c.W && with <= UINT64_MAX);
    // records forced: the budget holds them
    CHECK(is(ask(32, c.m, c.n, c.W, true, with, -1, 1), false, true, true));
    CHECK(is(ask(32, c.m, c.n, c.W, true, with - 1, -1, 1), false, true, false));
    CHECK(is(ask(32, c.m, c.n, c.W, true, without, -1, 1), false, true, false));
    // records forbidden: it does not
    CHECK(is(ask(32, c.m, c.n, c.W, true, without, -1, 0), false, false, true));
    CHECK(is(ask(32, c.m, c.n, c.W, true, without - 1, -1, 0), false, false, false));
    CHECK(is(ask(32, c.m, c.n, c.W, true, with, -1, 0), false, false, true));
  }
  // left to the free memory.  Large 128-bit indexes: the records need 100/55 of their size free, the lines budget only their size
  // next to 8 GB per table, so wherever the records are built the lines fit as well, and below that the lines get their room earlier
  const struct { uint32_t m; uint64_t n; uint32_t W; } roomy[] = {{4, 1000000000, 2}, {64, N_MAX, 2}, {8, 600000000, 2}};
  for (const auto& c : roomy) {
    const u128 bf = bent_from(c.m, c.n, c.W), with = lines_from(c.m, c.n, c.W, true), without = lines_from(c.m, c.n, c.W, false);
    CHECK(without < with && with < bf);
    CHECK(is(ask(32, c.m, c.n, c.W, true, without - 1), false, false, false));
    CHECK(is(ask(32, c.m, c.n, c.W, true, without), false, false, true));
    CHECK(is(ask(32, c.m, c.n, c.W, true, bf - 1), false, false, true));
    CHECK(is(ask(32, c.m, c.n, c.W, true, bf), false, true, true));
  }
  // 64-bit codes, and 128-bit ones near 3e8 records: the lines' 8 GB per table weigh more than the 45 % the records leave over, so
  // there is a band of free memory where getting the records costs the lines
  const struct { uint32_t m; uint64_t n; uint32_t W; } tight[] = {{2, 1000000000, 1}, {1, 1000000000, 1}, {4, 300000000, 2}};
  for (const auto& c : tight) {
    const u128 bf = bent_from(c.m, c.n, c.W), with = lines_from(c.m, c.n, c.W, true), without = lines_from(c.m, c.n, c.W, false);
    CHECK(without < bf && bf < with);
    CHECK(is(ask(32, c.m, c.n, c.W, true, without - 1), false, false, false));
    CHECK(is(ask(32, c.m, c.n, c.W, true, without), false, false, true));
    CHECK(is(ask(32, c.m, c.n, c.W, true, bf - 1), false, false, true));     // no records: the lines fit
    CHECK(is(ask(32, c.m, c.n, c.W, true, bf), false, true, false));         // records: the same memory no longer holds the lines
    CHECK(is(ask(32, c.m, c.n, c.W, true, with - 1), false, true, false));
    CHECK(is(ask(32, c.m, c.n, c.W, true, with), false, true, true));
  }
}

static void check_shapes_and_knobs() {
  const uint64_t roomy = 1ull << 50, none = 0;
  // <= 16-bit substrings: neither records nor lines, whatever the knobs say
  for (uint32_t sbits : {8u, 16u})
    for (int ke = -1; ke <= 1; ++ke)
      for (int kl = -1; kl <= 1; ++kl)
        for (uint64_t n : {(uint64_t)30000, (uint64_t)1000000000}) {
          CHECK(is(ask(sbits, 4, n, 1, true, roomy, -1, ke, kl), true, false, false));
          CHECK(is(ask(sbits, 4, n, 1, true, none, -1, ke, kl), false, false, false));
          CHECK(is(ask(sbits, 4, n, 1, false, none, -1, ke, kl), true, false, false));
        }
  // 32-bit substrings of codes wider than two words: VC_MIH_BENT=1 gives no records
  for (uint32_t W : {3u, 4u, 8u})
    for (int ke = -1; ke <= 1; ++ke) {
      CHECK(is(ask(32, 2 * W, 30000, W, true, roomy, -1, ke), false, false, false));
      CHECK(is(ask(32, 2 * W, 30000, W, false, none, -1, ke), false, false, false));
    }
  // an empty index has no lines, knob or not; the other structures are decided as for any n (and then not allocated)
  for (int kl = -1; kl <= 1; ++kl) {
    CHECK(is(ask(32, 4, 0, 2, true, roomy, -1, -1, kl), false, true, false));
    CHECK(is(ask(32, 8, 0, 4, true, roomy, -1, -1, kl), false, false, false));
    CHECK(is(ask(16, 4, 0, 1, true, roomy, -1, -1, kl), true, false, false));
  }
  // VC_MIH_BCODES at -1 / 0 / 1, with and without room; 1 forces the copies even at 32-bit substrings
  CHECK(is(ask(16, 4, 30000, 1, true, roomy, -1), true, false, false));
  CHECK(is(ask(16, 4, 30000, 1, true, roomy, 0), false, false, false));
  CHECK(is(ask(16, 4, 30000, 1, true, roomy, 1), true, false, false));
  CHECK(is(ask(16, 4, 30000, 1, true, none, -1), false, false, false));
  CHECK(is(ask(16, 4, 30000, 1, true, none, 0), false, false, false));
  CHECK(is(ask(16, 4, 30000, 1, true, none, 1), true, false, false));
  CHECK(is(ask(32, 4, 30000, 2, true, roomy, -1), false, true, false));
  CHECK(is(ask(32, 4, 30000, 2, true, roomy, 0), false, true, false));
  CHECK(is(ask(32, 4, 30000, 2, true, roomy, 1), true, true, false));
  CHECK(is(ask(32, 8, 30000, 4, true, none, 1), true, false, false));
  // VC_MIH_BENT at -1 / 0 / 1
  CHECK(is(ask(32, 4, 30000, 2, true, roomy, -1, -1), false, true, false));
  CHECK(is(ask(32, 4, 30000, 2, true, roomy, -1, 0), false, false, false));
  CHECK(is(ask(32, 4, 30000, 2, true, roomy, -1, 1), false, true, false));
  CHECK(is(ask(32, 4, 30000, 2, true, none, -1, -1), false, false, false));
  CHECK(is(ask(32, 4, 30000, 2, true, none, -1, 0), false, false, false));
  CHECK(is(ask(32, 4, 30000, 2, true, none, -1, 1), false, true, false));
  // VC_MIH_LINES at -1 / 0 / 1, at the suite's size and at one where they are built unasked
  CHECK(is(ask(32, 4, 30000, 2, true, roomy, -1, -1, -1), false, true, false));
  CHECK(is(ask(32, 4, 30000, 2, true, roomy, -1, -1, 0), false, true, false));
  CHECK(is(ask(32, 4, 30000, 2, true, roomy, -1, -1, 1), false, true, true));
  CHECK(is(ask(32, 4, 30000, 2, true, none, -1, -1, 1), false, false, true));
  CHECK(is(ask(32, 8, 30000, 4, true, none, -1, -1, 1), false, false, true));
  CHECK(is(ask(32, 4, 1000000000, 2, true, roomy, -1, -1, -1), false, true, true));
  CHECK(is(ask(32, 4, 1000000000, 2, true, roomy, -1, -1, 0), false, true, false));
  CHECK(is(ask(32, 4, 1000000000, 2, true, none, -1, -1, 1), false, false, true));
  CHECK(is(ask(32, 4, 30000, 2, true, none, -1, 1, 1), false, true, true));        // the bent0_lines1 route's counterpart
  CHECK(is(ask(32, 4, 30000, 2, true, roomy, -1, 0, 1), false, false, true));      // the bent0_lines1 route
  // the free-memory query failed: copies and records stay as the shape wants them, no lines unasked.  Today's behaviour, pinned
  CHECK(is(ask(16, 4, 1000000000, 1, false, none), true, false, false));
  CHECK(is(ask(8, 64, N_MAX, 8, false, none), true, false, false));
  CHECK(is(ask(32, 4, 1000000000, 2, false, none), false, true, false));
  CHECK(is(ask(32, 4, 1000000000, 2, false, roomy), false, true, false));          // (the figure is not looked at)
  CHECK(is(ask(32, 8, 1000000000, 4, false, roomy), false, false, false));
  CHECK(is(ask(32, 4, 1000000000, 2, false, none, -1, 0, -1), false, false, false));
  CHECK(is(ask(32, 4, 1000000000, 2, false, none, -1, -1, 1), false, true, true));  // the knob needs no figure
  CHECK(is(ask(32, 4, 1000000000, 2, false, none, 0, 0, 0), false, false, false));
}

// the sizes the documentation speaks of, in decimal GB (1e9 bytes) of free memory on either side of each threshold
static void check_documented_sizes() {
  const u128 GB = 1000000000;
  // 128 bit / 4 tables, 1e8 records: 12.8 GB of records; they go below 100/55 of that.  No lines at this size, knob apart
  CHECK(bent_bytes(4, 100000000, 2) == 12800 * GB / 1000);
  CHECK(bent_from(4, 100000000, 2) > 23 * GB && bent_from(4, 100000000, 2) < 24 * GB);
  // 128 bit / 4 tables, 1e9 records: 128 GB of records, gone below about 233 GB free; the lines (8 GB, budget 4 x that) need
  // 35 GB of index + 34.4 GB without the records
  CHECK(bent_bytes(4, 1000000000, 2) == 128 * GB);
  CHECK(bent_from(4, 1000000000, 2) > 232 * GB && bent_from(4, 1000000000, 2) < 234 * GB);
  CHECK(lines_from(4, 1000000000, 2, false) > 69 * GB && lines_from(4, 1000000000, 2, false) < 70 * GB);
  CHECK(lines_from(4, 1000000000, 2, true) < bent_from(4, 1000000000, 2));          // with the records in, the lines always fit
  // 64 bit / 4 tables, 1e9 records: 16-bit substrings, 32 GB of copies, gone below 96 GB free
  CHECK(bcodes_bytes(4, 1000000000, 1) == 32 * GB && bcodes_from(4, 1000000000, 1) == 96 * GB);
  const struct { uint32_t bits, m; uint64_t n; uint64_t free_gb; bool bcodes, bent, lines; } rows[] = {
      {128, 4, 100000000, 23, false, false, false},
      {128, 4, 100000000, 24, false, true, false},
      {128, 4, 100000000, 280, false, true, false},
      {128, 4, 1000000000, 69, false, false, false},
      {128, 4, 1000000000, 70, false, false, true},
      {128, 4, 1000000000, 232, false, false, true},
      {128, 4, 1000000000, 234, false, true, true},
      {128, 4, 1000000000, 280, false, true, true},      // an empty 288 GB part with the codes resident
      {64, 4, 1000000000, 95, false, false, false},
      {64, 4, 1000000000, 97, true, false, false},
  };
  for (const auto& r : rows) {
    const uint32_t sbits = r.bits / r.m, W = r.bits / 64;
    CHECK(is(ask(sbits, r.m, r.n, W, true, r.free_gb * GB), r.bcodes, r.bent, r.lines));
    CHECK(same(ask(sbits, r.m, r.n, W, true, r.free_gb * GB), rule(sbits, r.m, r.n, W, true, r.free_gb * GB, -1, -1, -1)));
  }
}

// everything against the restatement: shapes up to the ABI's extremes x the free-memory figures around every threshold of the
// shape x every knob setting.  Under -fsanitize=undefined a product that left 64 bits in the header would not show (unsigned
// arithmetic wraps silently), so the 128-bit figures are also checked to fit
static void check_sweep() {
  long cells = 0;
  for (uint32_t sbits : {8u, 16u, 32u})
    for (uint32_t m : {1u, 2u, 4u, 8u, 64u})
      for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)30000, (uint64_t)299999999, (uint64_t)300000000, (uint64_t)1000000000, N_MAX})
        for (uint32_t W : {1u, 2u, 3u, 4u, 8u}) {
          std::vector<u128> frees = {0, 1, 99, 100, 101, (u128)1 << 40, UINT64_MAX - 1, UINT64_MAX};
          for (u128 t : {bcodes_from(m, n, W), bent_from(m, n, W), lines_from(m, n, W, false), lines_from(m, n, W, true), index_bytes(m, n),
                         index_bytes(m, n) + bent_bytes(m, n, W), bcodes_bytes(m, n, W), bent_bytes(m, n, W)}) {
            CHECK(t < ((u128)1 << 63));
            for (int d = -2; d <= 2; ++d)
              if (d >= 0 || t >= (u128)-d) frees.push_back(t + d);
          }
          for (u128 f : frees)
            for (int have = 0; have <= 1; ++have)
              for (int kb = -1; kb <= 1; ++kb)
                for (int ke = -1; ke <= 1; ++ke)
                  for (int kl = -1; kl <= 1; ++kl) {
                    const MihMemPolicy p = ask(sbits, m, n, W, have != 0, f, kb, ke, kl);
                    const Want w = rule(sbits, m, n, W, have != 0, f, kb, ke, kl);
                    ++cells;
                    if (!same(p, w)) {
                      printf("FAILED sbits=%u m=%u n=%llu W=%u have=%d free=%llu knobs=%d/%d/%d: header %d%d%d, rule %d%d%d\n", sbits, m,
                             (unsigned long long)n, W, have, (unsigned long long)f, kb, ke, kl, p.bcodes, p.bent, p.lines, w.bcodes, w.bent,
                             w.lines);
                      ++g_bad;
                    }
                  }
        }
  CHECK(cells > 500000);
  // the extremes by name: 64 tables x (2^32 - 1) records x 8 words.  The records' bytes take 45 bits; a 32-bit or a size_t-free
  // product would have wrapped long before
  CHECK(bent_bytes(64, N_MAX, 8) == ((u128)(N_MAX) << 13) && bent_bytes(64, N_MAX, 8) > ((u128)1 << 44));
  CHECK(is(ask(32, 64, N_MAX, 8, true, UINT64_MAX), false, false, true));
  CHECK(is(ask(32, 64, N_MAX, 2, true, bent_from(64, N_MAX, 2)), false, true, true));
  CHECK(is(ask(32, 64, N_MAX, 2, true, bent_from(64, N_MAX, 2) - 1), false, false, true));
  CHECK(is(ask(16, 64, N_MAX, 8, true, bcodes_from(64, N_MAX, 8) - 1), false, false, false));
  CHECK(is(ask(16, 64, N_MAX, 8, true, bcodes_from(64, N_MAX, 8)), true, false, false));
}

int main() {
  check_thresholds();
  check_lines_budget_counts_the_records();
  check_shapes_and_knobs();
  check_documented_sizes();
  check_sweep();
  if (g_bad) { printf("%d checks FAILED\n", g_bad); return 1; }
  printf("all checks hold\n");
  return 0;
}
