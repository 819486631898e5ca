// Stand-alone check of the arithmetic the stream kernel's split threshold test rests on
// (verticut_amd/csrc/vc_scan_stream_plan.hpp): chain base + fire level against the one-piece chain start, exhaustively over
// small key fields, every tau 0..128 and every count of matching streamed bits.  Plain C++ with its own main: build it with
// -fsanitize=address,undefined to have every index it forms checked.  Exit status 0 = all checks hold.
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>

#include "../../verticut_amd/csrc/vc_scan_stream_plan.hpp"

static int g_bad = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++g_bad; } \
  } while (0)

static uint32_t popc(uint32_t x) {
  uint32_t c = 0;
  for (; x; x &= x - 1) ++c;
  return c;
}

// The kernel's test is  chain_base + matching >= fire_level(tau);  the one-piece form is  chain_start + matching >= 128.
// For every header over FIELD-bit key ranges, every key in the range, every query key, every tau and every number of matching
// streamed bits: the two agree, and neither drops a record with dist <= tau.
static void check_split_threshold_exhaustively() {
  const uint32_t FIELD = 4, SHIFT = 32 - FIELD, NK = 1u << FIELD;
  for (uint32_t low : {0u, 0x0FFFFFFFu, 0x05555555u}) {
    for (uint32_t lo = 0; lo < NK; ++lo) {
      for (uint32_t hi = lo; hi < NK; ++hi) {
        const VcStreamHeader h = vc_stream_header((lo << SHIFT) | low, (hi << SHIFT) | low);
        for (uint32_t qf = 0; qf < NK; ++qf) {
          const uint32_t qkey = (qf << SHIFT) | (low ^ 0x00F0F0F0u);
          const uint32_t base = vc_stream_chain_base(h, qkey);
          CHECK(base == 32 - vc_stream_key_bound(h, qkey));
          CHECK(base <= 32);
          for (uint32_t tau = 0; tau <= 128; ++tau) {
            CHECK(vc_stream_chain_start(h, qkey, tau) == tau + base);
            const uint32_t level = vc_stream_fire_level(tau);
            CHECK(level == 128 - tau);
            for (uint32_t match = 0; match <= 96; ++match) {
              const bool fires = base + match >= level;
              CHECK(fires == (vc_stream_chain_start(h, qkey, tau) + match >= 128));
              for (uint32_t kf = lo; kf <= hi; ++kf) {
                const uint32_t key = (kf << SHIFT) | low;
                const uint32_t dist = popc(key ^ qkey) + (96 - match);
                if (dist <= tau) CHECK(fires);
              }
            }
          }
        }
      }
    }
  }
  // a threshold above the code width accepts everything, as 128 does (the level never wraps)
  for (uint32_t tau : {129u, 1000u, 0x7FFFFFFFu, 0xFFFFFFFFu}) CHECK(vc_stream_fire_level(tau) == 0);
  // the largest chain still fits the compare: base <= 32, matching <= 96
  CHECK(vc_stream_chain_base(vc_stream_header(0u, 0xFFFFFFFFu), 0x12345678u) == 32);
}

int main() {
  check_split_threshold_exhaustively();
  if (g_bad) {
    printf("%d checks FAILED\n", g_bad);
    return 1;
  }
  printf("all checks hold\n");
  return 0;
}
