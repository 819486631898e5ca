// Stand-alone check of the scan stream's host arithmetic (verticut_amd/csrc/vc_scan_stream_plan.hpp): the common-prefix header
// of a granule, the chain start as a true lower bound of the distance for every key a header covers (exhaustively over small
// key fields), the layout of the one allocation, padding, the bytes a launch streams and the memory rule.  Plain C++ with its
// own main: build it with -fsanitize=address,undefined to have every index it forms checked.  Exit status 0 = all checks hold.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

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

static void check_headers() {
  // equal keys: every bit is known
  for (uint32_t k : {0u, 1u, 0x80000000u, 0xFFFFFFFFu, 0x12345678u}) {
    const VcStreamHeader h = vc_stream_header(k, k);
    CHECK(h.mask == 0xFFFFFFFFu && h.prefix == k);
  }
  // adjacent keys share everything above the lowest bit that flips
  for (uint32_t k : {0u, 1u, 2u, 0x7FFFFFFFu, 0xFFFFFFFEu, 0x0000FFFFu}) {
    const VcStreamHeader h = vc_stream_header(k, k + 1);
    const uint32_t x = k ^ (k + 1);
    uint32_t known = 0;
    while (known < 32 && !((x >> (31 - known)) & 1u)) ++known;
    CHECK(popc(h.mask) == known);
    CHECK((k & h.mask) == h.prefix && ((k + 1) & h.mask) == h.prefix);
  }
  // the whole key range in one granule: nothing is known
  {
    const VcStreamHeader h = vc_stream_header(0x00000000u, 0xFFFFFFFFu);
    CHECK(h.mask == 0 && h.prefix == 0);
  }
  // straddles of every power of two: 2^b - 1 and 2^b differ in bit b, so only the 31 - b bits above it are shared
  for (uint32_t b = 0; b < 32; ++b) {
    const uint32_t hi = 1u << b, lo = hi - 1;
    const VcStreamHeader h = vc_stream_header(lo, hi);
    CHECK(popc(h.mask) == 31 - b);
    CHECK(h.prefix == 0);
    CHECK(h.mask == (b == 31 ? 0u : 0xFFFFFFFFu << (b + 1)));
    // and a granule that ends just below the power of two keeps bit b among the known ones when it starts in the same half
    if (b >= 1) {
      const VcStreamHeader g = vc_stream_header(hi, hi | (hi - 1));
      CHECK(popc(g.mask) == 32 - b && g.prefix == hi);
    }
  }
  // the mask is always a run of leading ones and the prefix lies inside it
  uint64_t s = 88172645463325252ull;
  for (int i = 0; i < 100000; ++i) {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    uint32_t a = (uint32_t)s, b = (uint32_t)(s >> 32);
    if (a > b) { const uint32_t t = a; a = b; b = t; }
    const VcStreamHeader h = vc_stream_header(a, b);
    CHECK(((~h.mask) & ((~h.mask) + 1)) == 0);          // ~mask = 2^j - 1
    CHECK((h.prefix & ~h.mask) == 0);
    CHECK((a & h.mask) == h.prefix && (b & h.mask) == h.prefix);
    const uint32_t mid = a + (b - a) / 2;                 // any key between them shares the prefix
    CHECK((mid & h.mask) == h.prefix);
  }
}

// Exhaustive over FIELD-bit keys placed at the top of the word (the low 32 - FIELD bits equal in all keys of a range): for every
// range [lo, hi], every key in it, every query key and a few thresholds the chain start bounds tau + matching key bits from
// above, the key bound bounds the key's distance from below, and the pass rule (chain >= 128) never drops a record with
// dist <= tau.  `rest` plays the matching bits of the 96 streamed bits.
static void check_lower_bound_exhaustively() {
  const uint32_t FIELD = 5, SHIFT = 32 - FIELD, NK = 1u << FIELD;
  for (uint32_t low : {0u, 0x07FFFFFFu, 0x02AAAAAAu}) {
    for (uint32_t lo = 0; lo < NK; ++lo) {
      for (uint32_t hi = lo; hi < NK; ++hi) {
        const VcStreamHeader h = vc_stream_header((lo << SHIFT) | low, (hi << SHIFT) | low);
        for (uint32_t qf = 0; qf < NK; ++qf) {
          const uint32_t qkey = (qf << SHIFT) | (low ^ 0x00F0F0F0u);
          const uint32_t lb = vc_stream_key_bound(h, qkey);
          for (uint32_t kf = lo; kf <= hi; ++kf) {
            const uint32_t key = (kf << SHIFT) | low;
            const uint32_t dkey = popc(key ^ qkey);
            CHECK(lb <= dkey);
            for (uint32_t tau : {0u, 1u, 35u, 128u}) {
              const uint32_t start = vc_stream_chain_start(h, qkey, tau);
              CHECK(start >= tau + (32 - dkey));                 // an upper bound of tau + matching key bits
              CHECK(start == tau + 32 - lb);                     // the two forms agree
              for (uint32_t rest_match : {0u, 61u, 96u}) {       // matching bits among the 96 streamed ones
                const uint32_t dist = dkey + (96 - rest_match);
                if (dist <= tau) CHECK(start + rest_match >= 128);
              }
            }
          }
        }
      }
    }
  }
  // a full mask makes the bound exact
  for (uint32_t key : {0u, 0xDEADBEEFu})
    for (uint32_t q : {0u, 0xFFFFFFFFu, 0x13579BDFu}) {
      const VcStreamHeader h = vc_stream_header(key, key);
      CHECK(vc_stream_key_bound(h, q) == popc(key ^ q));
      CHECK(vc_stream_chain_start(h, q, 7) == 7 + 32 - popc(key ^ q));
    }
}

static void check_plan() {
  const uint64_t sizes[] = {0, 1, 255, 256, 257, 2047, 2048, 2049, 8191, 8192, 8193, 100003, 1ull << 20, 125000000ull, 1000000000ull, 0xFFFFFFFFull};
  for (uint64_t n : sizes) {
    const uint64_t work = 1000 + n / 16;
    const VcStreamPlan p = vc_stream_plan(n, work);
    CHECK(p.n == n);
    CHECK(p.n_pad >= n && p.n_pad % VC_STREAM_CHUNK == 0 && p.n_pad < n + VC_STREAM_CHUNK);
    CHECK(p.chunks * VC_STREAM_CHUNK == p.n_pad);
    CHECK(p.granules * VC_STREAM_GRANULE == p.n_pad);
    CHECK(p.stride >= p.n_pad && p.stride % VC_STREAM_PAD_ITEMS == 0 && p.stride < p.n_pad + VC_STREAM_PAD_ITEMS);
    // the four columns, perm and the headers do not overlap, in this order, and every 16-byte load of a column is aligned
    CHECK(p.key == 0 && p.t0 == p.stride && p.perm == 4 * p.stride && p.hdr == p.perm + p.n_pad);
    CHECK(p.words == p.hdr + 2 * p.granules && p.bytes == p.words * 4);
    CHECK(p.t0 % 4 == 0 && p.perm % 4 == 0 && p.hdr % 2 == 0);
    // the last load of the last chunk stays inside its column, the last exact-check load inside key / perm
    if (p.chunks) {
      CHECK((p.chunks - 1) * VC_STREAM_CHUNK + VC_STREAM_CHUNK <= p.stride);
      CHECK(p.perm + p.n_pad <= p.hdr);
    }
    CHECK(p.temp_bytes == (2 * n + work) * 4);
    CHECK(vc_stream_scan_bytes(p) == p.n_pad * 12 + p.granules * 8);
    // the memory rule: stream + temporaries within 55 % of the free memory; an unknown figure refuses nothing
    const uint64_t need = p.bytes + p.temp_bytes;
    CHECK(vc_stream_fits(p, false, 0));
    CHECK(vc_stream_fits(p, true, need / 55 * 100 + 200));
    if (need > 100) CHECK(!vc_stream_fits(p, true, need));
    if (need > 100) CHECK(!vc_stream_fits(p, true, need / 55 * 100 - 100));
  }
  // the headline: 1e9 records hold about 20.03 bytes each and a launch streams about 12.03 bytes per record
  const VcStreamPlan p = vc_stream_plan(1000000000ull, 0);
  CHECK(p.bytes > 20000000000ull && p.bytes < 20100000000ull);
  CHECK(vc_stream_scan_bytes(p) > 12000000000ull && vc_stream_scan_bytes(p) < 12050000000ull);
  CHECK(VC_STREAM_MEM_SHARE == 55);
}

int main() {
  check_headers();
  check_lower_bound_exhaustively();
  check_plan();
  if (g_bad) {
    printf("%d checks FAILED\n", g_bad);
    return 1;
  }
  printf("all checks hold\n");
  return 0;
}
