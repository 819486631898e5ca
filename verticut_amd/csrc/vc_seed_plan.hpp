// Plan arithmetic of vc_seed_centres* (vc_seed.hip): the generator, the block ranges, the slot word a pick travels in and the
// two-level prefix search of the distance-weighted pick.  Plain C++ with no HIP in it, so that tests/cpp/seed_plan_test.cc checks it
// on the CPU; the kernels, their launcher and the sharded root call exactly these functions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VC_SP_FN __host__ __device__ inline
#else
#define VC_SP_FN inline
#endif

#define VC_SEED_BLOCK 256u             // threads per block of every vc_seed kernel
#define VC_SEED_RECORDS 4u             // records per thread of the round kernel
#define VC_SEED_BLOCK_RECORDS 1024u    // B = VC_SEED_BLOCK * VC_SEED_RECORDS: records per block, the unit of `partial`
#define VC_SEED_SUBSLOTS 16u           // words the farthest mode's block maxima spread over (block b: word b % 16); their maximum is the pick
#define VC_SEED_SLOT_STRIDE 16u        // 64-bit words between two of them: 128 bytes, a line each
#define VC_SEED_SLOT_WORDS (VC_SEED_SUBSLOTS * VC_SEED_SLOT_STRIDE)

// draw(t): output number t (from 0) of SplitMix64 started at `seed`.  The state after t + 1 steps is seed + (t + 1) * gamma, so an
// output is a function of (seed, t) alone; all arithmetic mod 2^64.
VC_SP_FN uint64_t vc_seed_draw(uint64_t seed, uint64_t t) {
  uint64_t z = seed + (t + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// Block b owns the records [lo, hi) = [b * B, min(n, (b + 1) * B)); its thread t owns lo + r * VC_SEED_BLOCK + t, r < VC_SEED_RECORDS:
// the 64 lanes of a wave read 64 consecutive words of a column.
VC_SP_FN uint64_t vc_seed_blocks(uint64_t n) { return (n + VC_SEED_BLOCK_RECORDS - 1) / VC_SEED_BLOCK_RECORDS; }
VC_SP_FN uint64_t vc_seed_block_lo(uint64_t b) { return b * VC_SEED_BLOCK_RECORDS; }
VC_SP_FN uint64_t vc_seed_block_hi(uint64_t b, uint64_t n) {
  const uint64_t hi = (b + 1) * VC_SEED_BLOCK_RECORDS;
  return hi < n ? hi : n;
}
VC_SP_FN uint64_t vc_seed_record_of(uint64_t b, uint32_t thread, uint32_t r) {
  return vc_seed_block_lo(b) + (uint64_t)r * VC_SEED_BLOCK + thread;
}

// The slot word of a pick: dist << 32 | (0xFFFFFFFF - i).  The MAXIMUM of slot words is the farthest-first rule -- the largest
// distance, the smallest index on a tie -- and 0 (no record: the index 0xFFFFFFFF is never resident, ids are 32 bits) loses to all.
VC_SP_FN uint64_t vc_seed_slot(uint32_t dist, uint32_t i) { return ((uint64_t)dist << 32) | (0xFFFFFFFFu - i); }
VC_SP_FN uint32_t vc_seed_slot_index(uint64_t slot) { return 0xFFFFFFFFu - (uint32_t)slot; }
VC_SP_FN uint32_t vc_seed_slot_dist(uint64_t slot) { return (uint32_t)(slot >> 32); }

// THE PREFIX SEARCH.  Over weights w[0 .. n) and a target, the answer is the smallest j with w[0] + .. + w[j] > target.  Item j with
// `before` = w[0] + .. + w[j - 1] is that answer exactly when this holds (so a weight of 0 never is):
VC_SP_FN bool vc_seed_crosses(uint64_t before, uint64_t weight, uint64_t target) { return before <= target && target - before < weight; }
// the same search in order: the answer, or n when the sum does not exceed target; *before = the sum ahead of the answer
template <class Wt, class Get>
VC_SP_FN uint64_t vc_seed_find(const Wt* w, uint64_t n, uint64_t target, uint64_t* before, Get weight_of) {
  uint64_t sum = 0;
  for (uint64_t j = 0; j < n; ++j) {
    const uint64_t x = weight_of(w[j]);
    if (vc_seed_crosses(sum, x, target)) {
      *before = sum;
      return j;
    }
    sum += x;
  }
  *before = sum;
  return n;
}
struct VcSeedWeightPlain {
  VC_SP_FN uint64_t operator()(uint64_t x) const { return x; }
};
struct VcSeedWeightPacked {   // the distance field of a packed `best` word
  VC_SP_FN uint64_t operator()(uint64_t x) const { return x >> 32; }
};
// Two levels, as the pick kernel and the sharded root walk them: partial[b] = the sum of the distances of block b's records (of a
// shard's records, for the root); the block whose running sum crosses the target, then the record inside it with the rest of the
// target.  total == 0 gives record 0.  `rnd` is the raw draw: target = rnd % total.
struct VcSeedPick {
  uint64_t total, target, block, record;
};
VC_SP_FN VcSeedPick vc_seed_search(const uint32_t* partial, const uint64_t* best, uint64_t n, uint64_t rnd) {
  VcSeedPick p{0, 0, 0, 0};
  const uint64_t nb = vc_seed_blocks(n);
  for (uint64_t b = 0; b < nb; ++b) p.total += partial[b];
  if (p.total == 0) return p;
  p.target = rnd % p.total;
  uint64_t before = 0;
  p.block = vc_seed_find(partial, nb, p.target, &before, VcSeedWeightPlain());
  if (p.block >= nb) {   // (partial and best disagree: cannot happen with a round kernel's outputs)
    p.block = 0;
    return p;
  }
  const uint64_t lo = vc_seed_block_lo(p.block), hi = vc_seed_block_hi(p.block, n);
  uint64_t inner = 0;
  const uint64_t j = vc_seed_find(best + lo, hi - lo, p.target - before, &inner, VcSeedWeightPacked());
  p.record = j < hi - lo ? lo + j : 0;
  return p;
}
