// csrc/vc_knn_graph_retain_plan.hpp on the CPU, host code only: built with -fsanitize=address,undefined by
// tests/test_knn_graph_retain_cpu.py.  The lane map for every k in 1 .. 65 and at the widest row (every entry of every row of a wave's
// group served exactly once, the segment masks a partition of the wave), a host replay of the kernel's placement by ballot ranks
// against a plain stable partition, the chunks for budgets down to one row (they cover the old rows exactly once, in order), the
// short rule at K - 1 < k, and the scratch layout.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "vc_knn_graph_retain_plan.hpp"

#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
      exit(1);                                                  \
    }                                                           \
  } while (0)

static void lanes() {
  const uint32_t ks[] = {1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 100, 129, 500, 8191};
  for (uint32_t k = 1; k <= 65; ++k) {
    const uint32_t P = vc_kgret_lanes(k), R = vc_kgret_rows_per_wave(k);
    CHECK((P & (P - 1)) == 0 && P <= VC_KGRET_WAVE && P * R == VC_KGRET_WAVE);
    CHECK(k > VC_KGRET_WAVE ? P == VC_KGRET_WAVE : (P >= k && (P == 1 || P / 2 < k)));
    CHECK(k <= 32 ? R >= 2 && vc_kgret_steps(k) == 1 : R == 1);
    printf("LANES %u %u %u %u\n", k, P, R, vc_kgret_steps(k));
  }
  for (uint32_t k : ks) {
    const uint32_t P = vc_kgret_lanes(k), R = vc_kgret_rows_per_wave(k);
    CHECK(vc_kgret_steps(k) == (k + P - 1) / P && (uint64_t)vc_kgret_steps(k) * P >= k);
    // the segment masks partition the wave, and lane l lies in segment l / P
    uint64_t all = 0;
    for (uint32_t r = 0; r < R; ++r) {
      const uint64_t m = vc_kgret_segment_mask(P, r);
      CHECK((all & m) == 0 && (uint32_t)__builtin_popcountll(m) == P);
      all |= m;
    }
    CHECK(all == ~0ull);
    for (uint32_t l = 0; l < VC_KGRET_WAVE; ++l) CHECK((vc_kgret_segment_mask(P, l / P) >> l) & 1);
    // every (row of the group, entry) has exactly one (step, lane)
    std::vector<uint8_t> seen((size_t)R * k, 0);
    for (uint32_t j0 = 0; j0 < k; j0 += P)
      for (uint32_t l = 0; l < VC_KGRET_WAVE; ++l) {
        const uint32_t j = j0 + l % P;
        if (j < k) CHECK(seen[(size_t)(l / P) * k + j]++ == 0);
      }
    for (uint8_t s : seen) CHECK(s == 1);
  }
  CHECK(vc_kgret_blocks(0, 10) == 1 && vc_kgret_blocks(1, 10) == 1 && vc_kgret_blocks(17, 10) == 2 && vc_kgret_blocks(1000000, 100) == 2048);
  CHECK(vc_kgret_blocks(4, 100) == 1 && vc_kgret_blocks(5, 100) == 2);
}

// the kernel's placement replayed on the host: per step the ballot of the live lanes, a live entry at the row's running base plus
// the live lanes of its segment below it, the tail padded -- against a stable partition of each row
static void placement() {
  uint64_t seed = 12345;
  auto rnd = [&]() { return (seed = seed * 6364136223846793005ull + 1442695040888963407ull) >> 33; };
  const uint32_t ks[] = {1, 2, 3, 5, 16, 17, 32, 33, 63, 64, 65, 129, 200};
  for (uint32_t k : ks) {
    const uint32_t P = vc_kgret_lanes(k), R = vc_kgret_rows_per_wave(k);
    for (int round = 0; round < 20; ++round) {
      std::vector<uint32_t> cnt(R);
      std::vector<uint8_t> alive((size_t)R * k);
      for (uint32_t r = 0; r < R; ++r) cnt[r] = (uint32_t)(rnd() % (k + 1));
      for (auto& a : alive) a = round == 0 ? 1 : round == 1 ? 0 : (uint8_t)(rnd() % 4 != 0);
      std::vector<uint64_t> out((size_t)R * k, 7), want((size_t)R * k, ~0ull);
      std::vector<uint32_t> base(R, 0);
      for (uint32_t j0 = 0; j0 < k; j0 += P) {
        uint64_t votes = 0;
        for (uint32_t l = 0; l < VC_KGRET_WAVE; ++l) {
          const uint32_t r = l / P, j = j0 + l % P;
          if (j < cnt[r] && alive[(size_t)r * k + j]) votes |= 1ull << l;
        }
        for (uint32_t l = 0; l < VC_KGRET_WAVE; ++l) {
          const uint32_t r = l / P, j = j0 + l % P;
          const uint64_t below = vc_kgret_segment_mask(P, r) & ((1ull << l) - 1);
          if ((votes >> l) & 1) {
            const uint32_t at = base[r] + (uint32_t)__builtin_popcountll(votes & below);
            CHECK(at < k);
            out[(size_t)r * k + at] = (uint64_t)r << 32 | j;
          }
        }
        for (uint32_t r = 0; r < R; ++r) base[r] += (uint32_t)__builtin_popcountll(votes & vc_kgret_segment_mask(P, r));
      }
      for (uint32_t r = 0; r < R; ++r) {
        for (uint32_t l = 0; l < P; ++l)
          for (uint32_t p = base[r] + l; p < k; p += P) out[(size_t)r * k + p] = ~0ull;
        uint32_t m = 0;
        for (uint32_t j = 0; j < cnt[r]; ++j)
          if (alive[(size_t)r * k + j]) want[(size_t)r * k + m++] = (uint64_t)r << 32 | j;
        CHECK(m == base[r]);
      }
      CHECK(out == want);
    }
  }
}

static void chunks() {
  const uint64_t budgets[] = {0, 1, 7, 8, 79, 80, 81, 800, 4096, 64ull << 20, ~0ull};
  const uint32_t ks[] = {1, 10, 100, 8191};
  const uint64_t ns[] = {1, 2, 9, 10, 11, 2000};
  for (uint64_t b : budgets)
    for (uint32_t k : ks)
      for (uint64_t n : ns) {
        const uint64_t c = vc_kgret_chunk_rows(b, k, n);
        CHECK(c >= 1 && c <= n);
        CHECK(c == n || (c * 8 * k <= b && (c + 1) * 8 * k > b) || (c == 1 && b < 8ull * k));
        uint64_t covered = 0, launches = 0;
        for (uint64_t c0 = 0; c0 < n; c0 += c) {
          CHECK(c0 == covered);
          covered += n - c0 < c ? n - c0 : c;
          ++launches;
        }
        CHECK(covered == n && launches == (n + c - 1) / c);
        CHECK(vc_kgret_rows_bytes(c, k) >= c * k * 8 + c * 4 && vc_kgret_rows_bytes(c, k) % 8 == 0);
      }
  CHECK(vc_kgret_chunk_rows(79, 10, 2000) == 1 && vc_kgret_chunk_rows(80, 10, 2000) == 1 && vc_kgret_chunk_rows(160, 10, 2000) == 2);
  CHECK(vc_kgret_chunk_rows(64ull << 20, 10, 1000000) == 838860 && vc_kgret_chunk_rows(64ull << 20, 100, 1000000) == 83886);
  printf("CHUNK %llu %llu %llu\n", (unsigned long long)vc_kgret_chunk_rows(4096, 100, 2000), (unsigned long long)vc_kgret_chunk_rows(1, 5, 70),
         (unsigned long long)vc_kgret_chunk_rows(64ull << 20, 10, 2000));
}

static void short_rule() {
  // a full store: a row is short as soon as it lost one entry
  CHECK(vc_kgret_full(1000, 10) == 10 && !vc_kgret_short(10, 1000, 10) && vc_kgret_short(9, 1000, 10) && vc_kgret_short(0, 1000, 10));
  // K - 1 < k: a row that holds the whole new store is not short, whatever it lost
  CHECK(vc_kgret_full(5, 10) == 4 && !vc_kgret_short(4, 5, 10) && vc_kgret_short(3, 5, 10));
  CHECK(vc_kgret_full(11, 10) == 10 && vc_kgret_full(10, 10) == 9 && !vc_kgret_short(9, 10, 10) && vc_kgret_short(9, 11, 10));
  CHECK(vc_kgret_full(1, 10) == 0 && !vc_kgret_short(0, 1, 10) && vc_kgret_full(0, 10) == 0 && !vc_kgret_short(0, 0, 10));
  CHECK(vc_kgret_full(2, 1) == 1 && vc_kgret_short(0, 2, 1) && !vc_kgret_short(1, 2, 1));
  CHECK(vc_kgret_full(1ull << 40, 8191) == 8191);
  for (uint32_t k = 1; k <= 65; ++k)
    for (uint64_t K = 0; K <= 70; ++K)
      for (uint32_t m = 0; m <= k; ++m) CHECK(vc_kgret_short(m, K, k) == (K > 0 && m < k && (uint64_t)m < K - 1));
}

static void work() {
  const uint64_t ns[] = {1, 2, 70, 2000, 1000000};
  for (uint64_t n : ns) {
    const VcKgretWork w(n, n - n / 10, 33);
    const uint64_t row4 = ((n + 1) * 4 + 7) & ~7ull;
    CHECK(w.stat == 0 && w.live == VC_KGRET_STAT_BYTES && w.rank == w.live + row4 && w.shrt == w.rank + row4 && w.srank == w.shrt + row4);
    CHECK(w.list == w.srank + row4 && w.scan_work >= w.list + (n - n / 10) * 4 && w.total == w.scan_work + 136 && w.total % 8 == 0);
    printf("WORK %llu %llu\n", (unsigned long long)n, (unsigned long long)w.total);
  }
  CHECK(VcKgretWork(5, 0, 0).list + 8 == VcKgretWork(5, 0, 0).scan_work);
}

int main() {
  lanes();
  placement();
  chunks();
  short_rule();
  work();
  printf("knn graph retain plan ok: WAVE %u BLOCK %u\n", VC_KGRET_WAVE, VC_KGRET_BLOCK);
  return 0;
}
