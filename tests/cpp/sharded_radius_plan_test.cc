// Stand-alone check of the index arithmetic behind vc_sharded_search_radius_dev (verticut_amd/csrc/vc_sharded_radius.hpp): the
// merge grid's per-shard block bases and running totals, the block -> (shard, chunk) mapping the kernel derives from them, and
// the buffer sizes of the shard-side regrow path.  Plain C++ with its own main: build it with -fsanitize=address,undefined to
// have every index it forms checked against real arrays of the planned sizes.  Exit status 0 = all checks hold.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../verticut_amd/csrc/vc_sharded_radius.hpp"

static int g_bad = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++g_bad; } \
  } while (0)

// what vc_sharded_radius_merge_kernel does with blockIdx.x: the shard, and the chunk's element range in that shard's array
static void block_to_chunk(const VcRadiusMergeArgs& a, uint32_t b, uint32_t* g, uint64_t* e0, uint64_t* e1) {
  uint32_t s = 0;
  while (s + 1 < VC_RMERGE_SHARDS && b >= a.first_block[s + 1]) ++s;
  *g = s;
  *e0 = (uint64_t)(b - a.first_block[s]) * VC_RMERGE_CHUNK;
  *e1 = *e0 + VC_RMERGE_CHUNK < a.total_g[s] ? *e0 + VC_RMERGE_CHUNK : a.total_g[s];
}

// every element of every shard is covered by exactly one block, no block is empty, no index leaves its array
static void check_plan(const std::vector<uint64_t>& totals) {
  VcRadiusMergeArgs a{};
  const uint32_t G = (uint32_t)totals.size();
  CHECK(vc_rmerge_plan(totals.data(), G, &a));
  uint64_t sum = 0;
  std::vector<std::vector<unsigned char>> seen(G);
  for (uint32_t g = 0; g < G; ++g) {
    sum += totals[g];
    seen[g].assign((size_t)totals[g], 0);
    CHECK(a.total_g[g] == totals[g]);
    CHECK(a.first_block[g] <= a.first_block[g + 1]);
  }
  CHECK(a.total == sum && a.G == G && a.first_block[0] == 0);
  for (uint32_t g = G; g < VC_RMERGE_SHARDS; ++g) CHECK(a.total_g[g] == 0 && a.first_block[g] == a.first_block[VC_RMERGE_SHARDS]);
  for (uint32_t b = 0; b < a.first_block[VC_RMERGE_SHARDS]; ++b) {
    uint32_t g;
    uint64_t e0, e1;
    block_to_chunk(a, b, &g, &e0, &e1);
    CHECK(g < G && e0 < e1 && e1 <= totals[g]);
    if (g >= G) continue;
    for (uint64_t e = e0; e < e1; ++e) ++seen[g][(size_t)e];   // (under AddressSanitizer: an index past the shard's array aborts)
  }
  for (uint32_t g = 0; g < G; ++g)
    for (unsigned char c : seen[g]) CHECK(c == 1);
}

// the regrow path of ShardRadius::run_lane on plain arrays: a shard reports `found`; a buffer that is too small is grown to
// exactly that and the repeat must fit
static void check_regrow(uint32_t nq, uint64_t found) {
  size_t bytes = 0;
  CHECK(vc_rshard_bytes(vc_rshard_first_cap(nq), &bytes));
  std::vector<uint64_t> buf(bytes / 8);
  for (int attempt = 0; attempt < 2; ++attempt) {
    const uint64_t cap = buf.size();
    if (!vc_rshard_must_repeat(found, cap)) {
      for (uint64_t i = 0; i < found; ++i) buf[(size_t)i] = i;   // the shard's writes
      return;
    }
    CHECK(attempt == 0);
    CHECK(vc_rshard_bytes(found, &bytes) && bytes / 8 == found);
    buf.assign(bytes / 8, 0);
  }
  CHECK(!"the repeat did not fit");
}

int main() {
  check_plan({0});
  check_plan({1});
  check_plan({VC_RMERGE_CHUNK});
  check_plan({VC_RMERGE_CHUNK + 1});
  check_plan({0, 0, 5, 0, VC_RMERGE_CHUNK * 3, 0, 1, 0});
  check_plan(std::vector<uint64_t>(VC_RMERGE_SHARDS, 1900 * 7 + 1231));        // 16 shards of a heavy batch
  check_plan({13155, 13144, 13065, 12987, 12926, 13174, 13202, 13190});         // the heavy test shape
  std::vector<uint64_t> mixed;
  for (uint32_t g = 0; g < VC_RMERGE_SHARDS; ++g) mixed.push_back(g % 3 == 1 ? 0 : (uint64_t)g * 1000 + g);
  check_plan(mixed);
  // totals beyond 2^32 (no arrays: the arithmetic alone) and beyond a launch
  {
    VcRadiusMergeArgs a{};
    const uint64_t big[2] = {(1ull << 33) + 5, 7};
    CHECK(vc_rmerge_plan(big, 2, &a));
    CHECK(a.first_block[1] == (1u << 23) + 1 && a.first_block[2] == (1u << 23) + 2 && a.total == (1ull << 33) + 12);
    uint32_t g;
    uint64_t e0, e1;
    block_to_chunk(a, (1u << 23), &g, &e0, &e1);
    CHECK(g == 0 && e0 == (1ull << 33) && e1 == (1ull << 33) + 5);
    block_to_chunk(a, (1u << 23) + 1, &g, &e0, &e1);
    CHECK(g == 1 && e0 == 0 && e1 == 7);
    const uint64_t huge[2] = {VC_RMERGE_MAX_BLOCKS * VC_RMERGE_CHUNK, 1};
    CHECK(!vc_rmerge_plan(huge, 2, &a));
    const uint64_t edge[1] = {VC_RMERGE_MAX_BLOCKS * VC_RMERGE_CHUNK};
    CHECK(vc_rmerge_plan(edge, 1, &a) && a.first_block[VC_RMERGE_SHARDS] == VC_RMERGE_MAX_BLOCKS);
  }
  check_regrow(8, 0);
  check_regrow(8, 8 * 64);
  check_regrow(8, 8 * 64 + 1);
  check_regrow(8, 13155);
  check_regrow(1, 30000);
  check_regrow(4099, 45000);
  {
    size_t bytes;
    CHECK(!vc_rshard_bytes(UINT64_MAX / 4, &bytes));
    CHECK(vc_rshard_offs_bytes(0xFFFFFFFFu) == ((size_t)0xFFFFFFFFu + 1) * 8);
  }
  printf(g_bad ? "%d checks FAILED\n" : "sharded radius plan: all checks hold\n", g_bad);
  return g_bad ? 1 : 0;
}
