// Which optional per-table structures an MIH index gets (mem_policy in vc_mih.hip): one decision for a build and a load, from the
// shape of the index, the free device memory and three dev knobs.  Plain C++ on purpose -- no HIP type, no HIP call -- so that the
// arithmetic also compiles into a stand-alone host program (tests/cpp/mih_policy_test.cc), which can hand it any free-memory figure.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define MIH_NLINES (1u << 25)                      // directory lines of a 32-bit table, 64 bytes each: 2 GB per table
#define MIH_LINES_MIN_RECORDS 300000000ull         // records from which the lines are built unasked (see vc_mih_policy)

struct MihPolicyKnobs {
  int bcodes, bent, lines;   // VC_MIH_BCODES, VC_MIH_BENT, VC_MIH_LINES: -1 auto, 0 / 1 forced
};

struct MihMemPolicy {
  bool bcodes;   // VcTableView::bcodes: bucket-order code copies
  bool bent;     // VcTableView::bent: {id, code} records in bucket order
  bool lines;    // VcTableView::lines: directory lines
};

// sbits: substring width (8, 16 or 32); m tables (<= 64); n records (< 2^32); W 64-bit words per code (<= 8): every product below
// stays under 2^52.  have_free == false: the free-memory query failed and free_bytes means nothing.
static inline MihMemPolicy vc_mih_policy(uint32_t sbits, uint32_t m, uint64_t n, uint32_t W, bool have_free, uint64_t free_bytes,
                                         const MihPolicyKnobs& knobs) {
  // bucket-order code copies for the tables whose buckets are big (see VcTableView::bcodes): m more copies of the
  // codes, so only while they fit comfortably (dev knob VC_MIH_BCODES=0/1 overrides)
  bool want_bcodes = sbits <= 16;
  bool want_bent = sbits == 32 && W <= 2;   // (VcTableView::bent; VC_MIH_BENT=0/1 overrides)
  if (have_free) {
    if ((uint64_t)m * n * W * 8 > free_bytes / 3) want_bcodes = false;
    // (55 % of the free memory: 128 GB of records at 1e9 x 128 bit next to 50 GB of codes + index on a 288 GB part)
    if ((uint64_t)m * n * 16 * W > free_bytes / 100 * 55) want_bent = false;
  }
  if (knobs.bcodes >= 0) want_bcodes = knobs.bcodes != 0;
  if (knobs.bent >= 0) want_bent = knobs.bent != 0 && sbits == 32 && W <= 2;

  // directory lines (VcTableView::lines): 2 GB per 32-bit table, built while that is a small part of what is still free once the
  // records of the index itself (ids, offsets, bitmaps, directories, {id, code} records) have their room (VC_MIH_LINES=0/1 overrides)
  bool want_lines = false;
  if (sbits == 32 && n != 0) {
    if (knobs.lines >= 0) {
      want_lines = knobs.lines != 0;
    } else if (n >= MIH_LINES_MIN_RECORDS && have_free) {
      // Where most 256-key blocks hold single-entry buckets only (93 % at 1e8 codes) the block directory answers a hit in one round
      // trip too and the lines gain nothing (r04, same box: 13.7 vs 13.6 M queries/s at 1e8, 9.96 -> 10.25 M at 1e9): build them from
      // the size on where a block's buckets are rarely all single (n / 2^32 = 0.07: a third of the blocks)
      const uint64_t index_bytes = (uint64_t)m * (n * 8 + (1ull << 29) + (3ull << 26)) + (want_bent ? (uint64_t)m * n * 16 * W : 0);
      want_lines = free_bytes > index_bytes && (uint64_t)m * MIH_NLINES * 64 <= (free_bytes - index_bytes) / 4;
    }
  }
  return {want_bcodes, want_bent, want_lines};
}
