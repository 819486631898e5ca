// Layout and index arithmetic of the device-resident radius search over shards (vc_sharded_search_radius_dev): what the host
// driver and vc_sharded_radius_merge_kernel share.  Plain C++ on purpose -- no HIP type, no HIP call -- so that the arithmetic
// (grid bases, running totals, buffer sizes of the regrow path) also compiles into a stand-alone host program
// (tests/cpp/sharded_radius_plan_test.cc).
#pragma once
#include <stddef.h>
#include <stdint.h>

#define VC_RMERGE_SHARDS 16u      // == VC_MAX_SHARDS (checked where both are visible)
#define VC_RMERGE_THREADS 256u
#define VC_RMERGE_PER_THREAD 4u
#define VC_RMERGE_CHUNK (VC_RMERGE_THREADS * VC_RMERGE_PER_THREAD)   // elements of one shard's flat result array per block
#define VC_RMERGE_MAX_BLOCKS 0x7FFFFFFFull                           // grid.x limit of a launch

// The merge kernel's argument, passed by value.  Shard g's results of the whole batch lie flat in seg[g], query q's at
// seg[g][offs[g][q] .. offs[g][q + 1]); an empty shard has offs[g] == nullptr (all its segments are empty).  The grid runs over
// (shard, chunk): blocks [first_block[g], first_block[g + 1]) take shard g's elements in chunks of VC_RMERGE_CHUNK.
struct VcRadiusMergeArgs {
  const uint64_t* seg[VC_RMERGE_SHARDS];
  const uint64_t* offs[VC_RMERGE_SHARDS];
  uint64_t total_g[VC_RMERGE_SHARDS];            // elements in seg[g]
  uint32_t first_block[VC_RMERGE_SHARDS + 1];
  uint32_t G, nq;
  const uint64_t* out_offs;                      // [nq + 1] the union's offsets (vc_sharded_radius_offsets_kernel)
  uint64_t* out;
  uint64_t total;                                // sum of total_g: entries of `out` the kernel may write
};

// Grid of the merge: fills total_g, first_block and total from the shards' totals.  Returns false when the grid would exceed a
// launch (more than 2^31 chunks: beyond any memory).
static inline bool vc_rmerge_plan(const uint64_t* totals, uint32_t G, VcRadiusMergeArgs* a) {
  uint64_t blocks = 0, total = 0;
  for (uint32_t g = 0; g < VC_RMERGE_SHARDS; ++g) {
    const uint64_t t = g < G ? totals[g] : 0;
    a->total_g[g] = t;
    a->first_block[g] = (uint32_t)blocks;
    blocks += t / VC_RMERGE_CHUNK + (t % VC_RMERGE_CHUNK ? 1 : 0);
    total += t;
    if (blocks > VC_RMERGE_MAX_BLOCKS) return false;
  }
  a->first_block[VC_RMERGE_SHARDS] = (uint32_t)blocks;
  a->G = G;
  a->total = total;
  return true;
}

// A shard's result buffer: what it starts with (entries) and what a repeat needs after the shard reported `needed`.
static inline uint64_t vc_rshard_first_cap(uint32_t nq) { return (uint64_t)nq * 64; }
static inline bool vc_rshard_must_repeat(uint64_t needed, uint64_t cap) { return needed > cap; }
// bytes behind `entries` packed values / an offsets array of nq + 1 entries; false on overflow of size_t
static inline bool vc_rshard_bytes(uint64_t entries, size_t* bytes) {
  if (entries > (uint64_t)(SIZE_MAX / 8)) return false;
  *bytes = (size_t)entries * 8;
  return true;
}
static inline size_t vc_rshard_offs_bytes(uint32_t nq) { return ((size_t)nq + 1) * 8; }
