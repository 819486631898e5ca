// Keep set of a removal (vc_retain*): which records survive and where they go.  Shared by vc_retain.hip (built there, used on the
// code columns) and vc_mih.hip (used on the index tables).
#pragma once
#include "vc_common.hpp"

// bits: one bit per record (bit i & 63 of word i >> 6), padded with zero words to whole 256-bit blocks; rank[b]: set bits before
// block b, b = 0 .. nblocks (rank[nblocks] = K) -- the bit + rank shape of the 32-bit tables' occupancy bitmap.  The survivors keep
// their order, so an id translates as new_local(i) = rank[i >> 8] + popcount(bits of the block below i).
#define VC_KEEP_BLOCK_BITS 256u
#define VC_KEEP_BLOCK_WORDS 4u
struct VcKeepSet {
  const uint64_t* bits;
  const uint32_t* rank;
  uint64_t n;   // records before the removal
  uint64_t k;   // survivors
};
inline uint64_t vc_keep_blocks(uint64_t n) { return (n + VC_KEEP_BLOCK_BITS - 1) / VC_KEEP_BLOCK_BITS; }

#if defined(__HIPCC__)
__device__ __forceinline__ bool vc_keep_test(const VcKeepSet& ks, uint32_t i) { return (ks.bits[i >> 6] >> (i & 63u)) & 1ull; }
// new local id of record i (meaningful when its bit is set): set bits strictly below i
__device__ __forceinline__ uint32_t vc_keep_rank(const VcKeepSet& ks, uint32_t i) {
  const uint32_t blk = i >> 8, w = (i >> 6) & 3u;
  const uint64_t* b = ks.bits + ((uint64_t)blk << 2);
  uint32_t r = ks.rank[blk];
  const uint64_t w0 = b[0], w1 = b[1], w2 = b[2], w3 = b[3];   // one 32-byte block: the words below by masks, no indexed array
  r += w > 0 ? __popcll(w0) : 0;
  r += w > 1 ? __popcll(w1) : 0;
  r += w > 2 ? __popcll(w2) : 0;
  const uint64_t cur = w == 0 ? w0 : w == 1 ? w1 : w == 2 ? w2 : w3;
  return r + __popcll(cur & ((1ull << (i & 63u)) - 1ull));
}
#endif
