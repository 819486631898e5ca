// Stand-alone check of csrc/vc_seed_plan.hpp (built with -fsanitize=address,undefined by tests/test_seed_cpu.py).
//  1. The block ranges: for every N in 0 .. 9000 and a few around 256 B, every record belongs to exactly one block and to exactly one
//     (thread, r) of it; no block is empty.  Records are a real array that every plan item writes: a plan that oversteps is an
//     address error here and not on a device.
//  2. The two-level prefix search (vc_seed_search: which block, which record, total == 0) equals a naive cumulative sum for random
//     and adversarial weights: zeros at the ends, one nonzero record, all zero, targets on block boundaries; and the per-item test
//     the pick kernel's threads make (vc_seed_crosses) holds for exactly that record.
//  3. The generator's first outputs, the slot word's order, and "B <seed_block_records>" for the Python side.
#include <stdio.h>

#include <vector>

#include "vc_seed_plan.hpp"

#define CHECK(c)                                                                                            \
  do {                                                                                                      \
    if (!(c)) {                                                                                             \
      printf("FAILED %s (line %d) n %llu rnd %llu\n", #c, __LINE__, (unsigned long long)n, (unsigned long long)rnd); \
      return 1;                                                                                             \
    }                                                                                                       \
  } while (0)

static int ranges(uint64_t n) {
  const uint64_t rnd = 0;
  const uint64_t nb = vc_seed_blocks(n);
  CHECK(nb == (n + VC_SEED_BLOCK_RECORDS - 1) / VC_SEED_BLOCK_RECORDS);
  std::vector<unsigned char> owner(n, 0), thread(n, 0);
  uint64_t next = 0;
  for (uint64_t b = 0; b < nb; ++b) {
    const uint64_t lo = vc_seed_block_lo(b), hi = vc_seed_block_hi(b, n);
    CHECK(lo == next && hi > lo && hi <= n);
    for (uint64_t i = lo; i < hi; ++i) owner[i] += 1;   // (unchecked on purpose: the sanitizer's business)
    for (uint32_t t = 0; t < VC_SEED_BLOCK; ++t)
      for (uint32_t r = 0; r < VC_SEED_RECORDS; ++r) {
        const uint64_t i = vc_seed_record_of(b, t, r);
        CHECK(i >= lo && i < lo + VC_SEED_BLOCK_RECORDS);
        if (i < n) thread[i] += 1;   // the guard of the kernels
      }
    next = hi;
  }
  CHECK(next == n);
  for (uint64_t i = 0; i < n; ++i) CHECK(owner[i] == 1 && thread[i] == 1);
  return 0;
}

// dist[i] -> best and partial as a round leaves them; every target that matters against the naive running sum
static int search(const std::vector<uint32_t>& dist, const std::vector<uint64_t>& rnds) {
  const uint64_t n = dist.size();
  uint64_t rnd = 0;
  std::vector<uint64_t> best(n), cum(n);
  std::vector<uint32_t> partial(vc_seed_blocks(n), 0);
  uint64_t total = 0;
  for (uint64_t i = 0; i < n; ++i) {
    best[i] = ((uint64_t)dist[i] << 32) | (uint32_t)(i * 2654435761u);   // (the index field must not matter)
    partial[i / VC_SEED_BLOCK_RECORDS] += dist[i];
    total += dist[i];
    cum[i] = total;
  }
  for (uint64_t x : rnds) {
    rnd = x;
    const VcSeedPick p = vc_seed_search(partial.data(), best.data(), n, rnd);
    CHECK(p.total == total);
    if (total == 0) {
      CHECK(p.record == 0);
      continue;
    }
    const uint64_t target = rnd % total;
    uint64_t want = 0;
    while (cum[want] <= target) ++want;   // the smallest i with cum[i] > target
    CHECK(p.target == target && p.record == want && p.block == want / VC_SEED_BLOCK_RECORDS);
    CHECK(dist[want] > 0);
    // the test a thread of the pick kernel makes holds for this record and for no other
    for (uint64_t i = 0; i < n; ++i) CHECK(vc_seed_crosses(cum[i] - dist[i], dist[i], target) == (i == want));
  }
  return 0;
}

static uint64_t g_state = 12345;
static uint64_t rnd64() { return vc_seed_draw(g_state++, 0); }

int main() {
  uint64_t n = 0, rnd = 0;
  long cases = 0;
  const uint64_t B = VC_SEED_BLOCK_RECORDS;
  CHECK(B == (uint64_t)VC_SEED_BLOCK * VC_SEED_RECORDS);
  for (n = 0; n <= 9000; ++n, ++cases)
    if (int rc = ranges(n)) return rc;
  for (uint64_t m : {255ull, 256ull, 257ull})
    for (uint64_t d : {0ull, 1ull, 2ull, 5ull}) {
      for (uint64_t sign : {0ull, 1ull}) {
        n = sign ? m * B - d : m * B + d;
        if (int rc = ranges(n)) return rc;
        ++cases;
      }
    }
  // the search
  for (uint64_t size : std::vector<uint64_t>{1, 2, 255, B - 1, B, B + 1, 3 * B + 1, 5 * B + 7}) {
    for (int shape = 0; shape < 7; ++shape) {
      std::vector<uint32_t> dist(size, 0);
      for (uint64_t i = 0; i < size; ++i) {
        const uint32_t r = (uint32_t)(rnd64() % 513);
        switch (shape) {
          case 0: dist[i] = r; break;                                           // random
          case 1: dist[i] = r % 3 == 0 ? r : 0; break;                          // many zeros
          case 2: dist[i] = i < size / 3 || i >= size - size / 3 ? 0 : r; break;   // zeros at both ends
          case 3: dist[i] = i == size / 2 ? 7 : 0; break;                       // one nonzero record
          case 4: dist[i] = 0; break;                                           // total == 0
          case 5: dist[i] = 512; break;                                         // the maximum everywhere
          case 6: dist[i] = i % B == B - 1 || i % B == 0 ? 1 : 0; break;        // only the ends of the blocks
        }
      }
      std::vector<uint64_t> rnds = {0, 1, 0xFFFFFFFFFFFFFFFFull};
      for (int j = 0; j < 40; ++j) rnds.push_back(rnd64());
      // targets on and beside every block boundary of the running sum, and the last ones
      uint64_t run = 0;
      for (uint64_t i = 0; i < size; ++i) {
        run += dist[i];
        if ((i + 1) % B == 0 || i + 1 == size)
          for (uint64_t d : {0ull, 1ull, 2ull}) {
            if (run >= d) rnds.push_back(run - d);   // (taken mod total by the search: run == total wraps to 0)
            rnds.push_back(run + d);
          }
      }
      n = size;
      if (int rc = search(dist, rnds)) return rc;
      cases += (long)rnds.size();
    }
  }
  // the generator: SplitMix64's published first outputs for the state 0, and draw(t) = the t-th step
  CHECK(vc_seed_draw(0, 0) == 0xE220A8397B1DCDAFull && vc_seed_draw(0, 1) == 0x6E789E6AA1B965F4ull && vc_seed_draw(0, 2) == 0x06C45D188009454Full);
  CHECK(vc_seed_draw(0x9E3779B97F4A7C15ull, 0) == vc_seed_draw(0, 1));
  // the slot word: a larger distance wins, then the smaller index; 0 loses to every record
  CHECK(vc_seed_slot(3, 9) > vc_seed_slot(2, 0) && vc_seed_slot(3, 4) > vc_seed_slot(3, 5) && vc_seed_slot(0, 0xFFFFFFFEu) > 0);
  CHECK(vc_seed_slot_index(vc_seed_slot(77, 123456)) == 123456 && vc_seed_slot_dist(vc_seed_slot(77, 123456)) == 77);
  printf("seed plan ok: %ld cases\nB %u\nTRIP %u\n", cases, VC_SEED_BLOCK_RECORDS, VC_SEED_BLOCK);
  return 0;
}
