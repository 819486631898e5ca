// csrc/vc_knn_graph_update_plan.hpp on the CPU, host code only: built with -fsanitize=address,undefined by
// tests/test_knn_graph_update_cpu.py.  The knobs at and beside their limits, the join kernel's map (every old record of every batch
// size 0 .. 9000 covered exactly once at every width), the tiles (every new record of a window staged exactly once, and a tile fits
// the LDS), the window rule (the windows of a batch cover the new records exactly once whatever is refused, and the halving ends at
// one record), the merge's sub-batches and the scratch layout.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "vc_knn_graph_update_plan.hpp"

#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
      exit(1);                                                  \
    }                                                           \
  } while (0)

static const uint32_t WIDTHS[4] = {1, 2, 4, 8};

static void knobs() {
  CHECK(vc_kgupd_old_batch(0) == VC_KGUPD_OLD_BATCH_DEFAULT && vc_kgupd_old_batch(1) == 1 && vc_kgupd_old_batch(100) == 100);
  CHECK(vc_kgupd_old_batch(VC_KGUPD_OLD_BATCH_MAX) == VC_KGUPD_OLD_BATCH_MAX && vc_kgupd_old_batch(VC_KGUPD_OLD_BATCH_MAX - 1) == VC_KGUPD_OLD_BATCH_MAX - 1);
  CHECK(vc_kgupd_old_batch((uint64_t)VC_KGUPD_OLD_BATCH_MAX + 1) == VC_KGUPD_OLD_BATCH_DEFAULT && vc_kgupd_old_batch(~0ull) == VC_KGUPD_OLD_BATCH_DEFAULT);
  CHECK(vc_kgupd_window(0) == VC_KGUPD_WINDOW_DEFAULT && vc_kgupd_window(1) == 1 && vc_kgupd_window(3) == 3);
  CHECK(vc_kgupd_window(VC_KGUPD_WINDOW_MAX) == VC_KGUPD_WINDOW_MAX && vc_kgupd_window(VC_KGUPD_WINDOW_MAX - 1) == VC_KGUPD_WINDOW_MAX - 1);
  CHECK(vc_kgupd_window((uint64_t)VC_KGUPD_WINDOW_MAX + 1) == VC_KGUPD_WINDOW_DEFAULT && vc_kgupd_window(~0ull) == VC_KGUPD_WINDOW_DEFAULT);
  CHECK(vc_kgupd_threshold(5, 5, 77) == 77 && vc_kgupd_threshold(4, 5, 77) == ~0ull && vc_kgupd_threshold(0, 1, 77) == ~0ull);
  CHECK(vc_kgupd_count(0, 0, 5) == 0 && vc_kgupd_count(3, 1, 5) == 4 && vc_kgupd_count(3, 2, 5) == 5 && vc_kgupd_count(5, 1ull << 40, 5) == 5);
  CHECK(vc_kgupd_count(8191, 0xFFFFFFFFull, 8191) == 8191 && vc_kgupd_count(0, 0xFFFFFFFFull, 8191) == 8191);
}

// every record of a batch of nb has exactly one (block, thread, r), and no slot of the grid names a record twice
static void map() {
  for (uint32_t W : WIDTHS) {
    const uint32_t R = vc_kgupd_records(W), br = vc_kgupd_block_records(W);
    CHECK(R * W <= 16 && br == VC_KGUPD_BLOCK * R);
    std::vector<uint8_t> seen;
    for (uint32_t nb = 0; nb <= 9000; ++nb) {
      const uint32_t blocks = vc_kgupd_blocks(nb, W);
      CHECK((uint64_t)blocks * br >= nb && (blocks == 0 || (uint64_t)(blocks - 1) * br < nb));
      seen.assign(nb, 0);
      for (uint32_t b = 0; b < blocks; ++b)
        for (uint32_t t = 0; t < VC_KGUPD_BLOCK; ++t)
          for (uint32_t r = 0; r < R; ++r) {
            const uint64_t i = vc_kgupd_record_of(W, b, t, r);
            CHECK(i < (uint64_t)blocks * br);
            if (i < nb) CHECK(seen[i]++ == 0);
          }
      for (uint32_t i = 0; i < nb; ++i) CHECK(seen[i] == 1);
    }
  }
}

// the tiles of a window stage each of its records once, and a tile fits the LDS
static void tiles() {
  for (uint32_t W : WIDTHS) {
    const uint32_t tile = vc_kgupd_tile(W);
    CHECK(tile >= 1 && (uint64_t)tile * W * 8 <= 16384 && VC_KGUPD_LDS_WORDS * 8 == 16384);
    for (uint32_t nw = 1; nw <= 9000; ++nw) {
      uint32_t covered = 0;
      for (uint32_t t0 = 0; t0 < nw; t0 += tile) {
        const uint32_t nt = vc_kgupd_tile_records(t0, nw, W);
        CHECK(nt >= 1 && nt <= tile && (uint64_t)nt * W <= VC_KGUPD_LDS_WORDS && t0 == covered);
        covered += nt;
      }
      CHECK(covered == nw);
    }
  }
}

// the driver's loop over the windows of one old batch, with `refuse(j0, nw)` standing in for the count pass
template <class Refuse>
static void walk(uint64_t n_new, uint32_t window, const Refuse& refuse, uint32_t* n_windows, uint32_t* n_halvings) {
  std::vector<uint8_t> seen(n_new, 0);
  uint32_t size = window, last = window;
  *n_windows = *n_halvings = 0;
  for (uint64_t j0 = 0; j0 < n_new;) {
    uint32_t nw = vc_kgupd_window_records(j0, n_new, size);
    CHECK(nw >= 1 && nw <= size && j0 + nw <= n_new);
    for (;;) {
      ++*n_windows;
      const uint64_t H = refuse(j0, nw);
      if (vc_kgupd_accept(H, 4096, nw)) break;
      CHECK(nw > 1);                                  // a window of one record is never refused
      size = nw = vc_kgupd_halve(nw);
      ++*n_halvings;
    }
    CHECK(size <= last);                              // the size only shrinks inside a batch
    last = size;
    for (uint32_t j = 0; j < nw; ++j) CHECK(seen[j0 + j]++ == 0);
    j0 += nw;
  }
  for (uint64_t j = 0; j < n_new; ++j) CHECK(seen[j] == 1);
}

static void windows() {
  CHECK(vc_kgupd_accept(0, 0, 7) && vc_kgupd_accept(512, 4096, 7) && !vc_kgupd_accept(513, 4096, 7) && vc_kgupd_accept(513, 4096, 1));
  CHECK(vc_kgupd_accept(~0ull, 0, 1) && vc_kgupd_accept(~0ull, 0, 0) && !vc_kgupd_accept(1, 0, 2));
  CHECK(!vc_kgupd_accept(0x100000000ull, ~0ull, 2) && vc_kgupd_accept(0xFFFFFFFFull, ~0ull, 2));   // the offsets are 32-bit words
  CHECK(!vc_kgupd_accept(1ull << 61, ~0ull, 2));                                                     // (8 H wraps: H is refused before)
  CHECK(vc_kgupd_halve(1) == 1 && vc_kgupd_halve(2) == 1 && vc_kgupd_halve(3) == 1 && vc_kgupd_halve(1024) == 512 && vc_kgupd_halve(0) == 1);
  for (uint32_t nw = 1; nw <= VC_KGUPD_WINDOW_MAX; nw = nw * 2 + 1) {   // the halving ends at one record, within log2 steps
    uint32_t x = nw, steps = 0;
    while (x > 1) {
      x = vc_kgupd_halve(x);
      ++steps;
    }
    CHECK(x == 1 && steps <= 20);
  }
  uint32_t nwin = 0, nhalf = 0;
  for (uint32_t window : {1u, 3u, 64u, 1024u, 4096u})
    for (uint64_t n_new : {1ull, 2ull, 63ull, 64ull, 65ull, 200ull, 1025ull, 9000ull}) {
      walk(n_new, window, [](uint64_t, uint32_t) { return 0ull; }, &nwin, &nhalf);                  // nothing refused
      CHECK(nhalf == 0 && nwin == (n_new + window - 1) / window);
      walk(n_new, window, [](uint64_t, uint32_t) { return 1ull << 40; }, &nwin, &nhalf);            // everything refused: down to one record
      uint32_t first = (uint32_t)std::min<uint64_t>(window, n_new), steps = 0;
      while (first > 1) {
        first = vc_kgupd_halve(first);
        ++steps;
      }
      CHECK(nhalf == steps && nwin == steps + n_new);
      walk(n_new, window, [](uint64_t j0, uint32_t nw) { return (j0 % 7 == 0 ? 300ull : 20ull) * nw; }, &nwin, &nhalf);   // a dense spot now and then
      CHECK(nwin >= nhalf + 1);
    }
}

static void sub_batches() {
  CHECK(vc_kgupd_merge_sub(0, 1) == 1 && vc_kgupd_merge_sub(7, 1) == 1 && vc_kgupd_merge_sub(8, 1) == 1 && vc_kgupd_merge_sub(16, 1) == 2);
  CHECK(vc_kgupd_merge_sub(64ull << 20, 8191) == (64ull << 20) / (8ull * 8191) && vc_kgupd_merge_sub(~0ull, 1) == 0xFFFFFFFFu);
  for (uint32_t k : {1u, 10u, 100u, 8191u})
    for (uint64_t budget : {0ull, 4096ull, 64ull << 20})
      for (uint64_t affected : {0ull, 1ull, 5ull, 100000ull}) {
        const uint32_t sub = vc_kgupd_merge_sub(budget, k);
        uint64_t covered = 0, most = 0;
        for (uint64_t a0 = 0; a0 < affected; a0 += sub) {
          const uint64_t na = std::min<uint64_t>(sub, affected - a0);
          covered += na;
          most = std::max(most, na);
        }
        CHECK(covered == affected && 8ull * k * most == vc_kgupd_merge_bytes(affected, budget, k));
        CHECK(vc_kgupd_merge_bytes(affected, budget, k) <= std::max<uint64_t>(budget, 8ull * k));
      }
  CHECK(vc_kgupd_hits_bytes(0) == 8 && vc_kgupd_hits_bytes(1) == 8 && vc_kgupd_hits_bytes(512) == 4096);
}

static void layout() {
  for (uint32_t W : WIDTHS)
    for (uint32_t nb : {1u, 2u, 100u, 2047u, 2048u, 2049u, 9000u, 1u << 18})
      for (uint32_t ng : {1u, 200u, 1u << 18}) {
        const VcKgupdWork w(nb, ng, W, 33);
        const uint64_t at[] = {w.stat, w.cnt, w.flag, w.offs, w.rank, w.list, w.newcnt, w.blk, w.mark, w.scan_work, w.ids, w.found, w.q, w.total};
        const uint64_t big = std::max(nb, ng);
        const uint64_t need[] = {VC_KGUPD_STAT_BYTES, 4ull * nb, 4ull * nb, 4ull * nb, 4ull * nb, 4ull * nb, 4ull * nb, 4ull * vc_kgupd_blocks(nb, W), nb, 4ull * 33,
                                 4 * big, 4 * big, 8ull * nb * W};
        for (int i = 0; i < 13; ++i) CHECK(at[i] % 8 == 0 && at[i] + need[i] <= at[i + 1]);   // in order, aligned, none overlaps the next
        CHECK(w.stat == 0 && (VC_KGUPD_ST_BAD + 1) * 8 <= VC_KGUPD_STAT_BYTES);
      }
}

int main() {
  knobs();
  map();
  tiles();
  windows();
  sub_batches();
  layout();
  printf("knn graph update plan ok: OLD_BATCH %u WINDOW %u LDS %u BLOCK %u\n", VC_KGUPD_OLD_BATCH_DEFAULT, VC_KGUPD_WINDOW_DEFAULT, VC_KGUPD_LDS_WORDS,
         VC_KGUPD_BLOCK);
  for (uint32_t W : WIDTHS) printf("MAP %u %u %u %u\n", W, vc_kgupd_records(W), vc_kgupd_blocks(9000, W), vc_kgupd_tile(W));
  for (uint32_t nb : {1u, 2000u, 1u << 18}) printf("WORK %u %llu\n", nb, (unsigned long long)VcKgupdWork(nb, 200, 2, 33).total);
  printf("SUB %u %llu\n", vc_kgupd_merge_sub(4096, 100), (unsigned long long)vc_kgupd_merge_bytes(1000, 4096, 100));
  return 0;
}
