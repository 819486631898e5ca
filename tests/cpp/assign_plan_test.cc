// Stand-alone check of csrc/vc_assign_plan.hpp (built with -fsanitize=address,undefined by tests/test_assign_cpu.py): for count
// 0 .. 9000, K 1 .. 2000, every code width and the knob values at and beside their limits -- the grid covers every record exactly
// once, the slices and their tiles cover every centre exactly once in ascending order, no slice is empty, S >= 1 and a tile fits the
// LDS array.  Records and centres are real arrays that every plan item writes: a plan that oversteps is an address error here and not
// on a device.
#include <stdio.h>

#include <vector>

#include "vc_assign_plan.hpp"

#define CHECK(c)                                                                                                                      \
  do {                                                                                                                                \
    if (!(c)) {                                                                                                                       \
      printf("FAILED %s (line %d) count %llu K %u W %u tile %u slices %u\n", #c, __LINE__, (unsigned long long)count, K, W, knob_tile, \
             knob_slices);                                                                                                            \
      return 1;                                                                                                                       \
    }                                                                                                                                 \
  } while (0)

static int one(uint64_t count, uint32_t K, uint32_t W, uint32_t n_cu, uint32_t knob_tile, uint32_t knob_slices) {
  const VcAssignPlan p = vc_assign_plan(count, K, W, n_cu, knob_tile, knob_slices);
  CHECK(p.W == W && p.R == vc_assign_records(W) && p.R * W <= 16);
  CHECK(p.tile >= 1 && (uint64_t)p.tile * W <= VC_ASSIGN_LDS_WORDS);
  CHECK(knob_tile == 0 || knob_tile > vc_assign_tile_max(W) ? p.tile == vc_assign_tile_max(W) : p.tile == knob_tile);
  CHECK(p.slices >= 1 && p.slices <= VC_ASSIGN_SLICES_MAX && p.slices <= K && p.per_slice >= 1);
  CHECK(knob_slices == 0 || p.slices <= knob_slices);
  CHECK(p.blocks == (count + vc_assign_block_records(W) - 1) / vc_assign_block_records(W));
  // records: the guard of the kernel is i < count
  std::vector<unsigned char> rec(count, 0);
  for (uint64_t b = 0; b < p.blocks; ++b)
    for (uint32_t t = 0; t < VC_ASSIGN_BLOCK; ++t)
      for (uint32_t r = 0; r < p.R; ++r) {
        const uint64_t i = vc_assign_record_of(W, b, t, r);
        if (i < count) rec[i] += 1;   // (unchecked on purpose: the sanitizer's business)
      }
  for (unsigned char x : rec) CHECK(x == 1);
  if (p.blocks) CHECK(vc_assign_record_of(W, p.blocks - 1, 0, 0) < count);   // no block without a record
  // centres: the slices in order, the tiles of a slice in order, as the kernel's loops walk them
  std::vector<unsigned char> cen(K, 0);
  uint64_t next = 0;
  for (uint32_t s = 0; s < p.slices; ++s) {
    const uint64_t lo = vc_assign_slice_lo(p.per_slice, s), hi = vc_assign_slice_hi(p.per_slice, K, s);   // the kernel's own calls
    CHECK(lo == next && hi > lo && hi <= K);
    for (uint64_t t0 = lo; t0 < hi; t0 += p.tile) {
      const uint32_t nt = vc_assign_tile_centres(t0, hi, p.tile);
      CHECK(nt >= 1 && (uint64_t)nt * W <= VC_ASSIGN_LDS_WORDS);
      for (uint32_t c = 0; c < nt; ++c) cen[t0 + c] += 1;
    }
    next = hi;
  }
  CHECK(next == K);
  for (unsigned char x : cen) CHECK(x == 1);
  return 0;
}

int main() {
  long cases = 0;
  const uint32_t widths[] = {1, 2, 4, 8};
  std::vector<uint64_t> counts = {0, 1, 2, 63, 64, 65, 255, 256, 257, 4097, 8192, 9000};
  for (uint32_t W : widths)
    for (uint64_t d : {0ull, 1ull})   // a block's size - 1, itself, + 1
      for (uint64_t m : {1ull, 2ull, 3ull}) {
        counts.push_back(m * vc_assign_block_records(W) - 1 + d);
        counts.push_back(m * vc_assign_block_records(W) + d);
      }
  // every count at a few shapes, every K at a few counts, then the corners of both against every knob value
  for (uint32_t W : widths) {
    for (uint64_t count = 0; count <= 9000; ++count)
      for (uint32_t K : {1u, 2000u}) {
        if (int rc = one(count, K, W, 256, 0, 0)) return rc;
        ++cases;
      }
    for (uint32_t K = 1; K <= 2000; ++K)
      for (uint64_t count : {1ull, 4097ull})
        for (uint32_t slices : {0u, 3u}) {
          if (int rc = one(count, K, W, 256, K % 3 ? 0 : 64, slices)) return rc;
          ++cases;
        }
    const uint32_t tmax = vc_assign_tile_max(W);
    for (uint64_t count : counts)
      for (uint32_t K : {1u, 2u, 3u, 64u, 65u, 257u, 2000u, tmax - 1, tmax, tmax + 1, 2 * tmax + 1})
        for (uint32_t tile : {0u, 1u, 64u, tmax - 1, tmax, tmax + 1, 0xFFFFFFFFu})
          for (uint32_t slices : {0u, 1u, 3u, VC_ASSIGN_SLICES_MAX, VC_ASSIGN_SLICES_MAX + 1, 0xFFFFFFFFu})
            for (uint32_t n_cu : {256u, 0u, 1u}) {
              if (slices && n_cu != 256) continue;   // (the CUs only matter to the automatic choice)
              if (int rc = one(count, K, W, n_cu, tile, slices)) return rc;
              ++cases;
            }
  }
  // the automatic slices: a small count against many centres is cut, a large one is not; one centre is never cut
  {
    const uint64_t count = 1000;
    const uint32_t K = 16384, W = 1, knob_tile = 0, knob_slices = 0;
    CHECK(vc_assign_plan(count, K, W, 256, 0, 0).slices > 1);
    CHECK(vc_assign_plan(100000000ull, K, W, 256, 0, 0).slices == 1);
    CHECK(vc_assign_plan(count, 1, W, 256, 0, 0).slices == 1);
    CHECK(vc_assign_plan(count, vc_assign_tile_max(W), W, 256, 0, 0).slices == 1);   // one tile of centres: nothing to cut
  }
  printf("assign plan ok: %ld cases\n", cases);
  return 0;
}
