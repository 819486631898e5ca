// Stand-alone check of csrc/vc_groups_plan.hpp (built with -fsanitize=address,undefined by tests/test_groups_cpu.py): for every group
// size 0 .. 4097, a set of start positions around the window boundaries and the windows 1024 and 2048 -- the tier of the size, the
// items tile the group exactly, every item (and every small group) lies inside the buffer of the window it starts in, the first item of
// a window is what a count gives, and the scratch arrays do not overlap.  The buffer is a real array that every item writes: a plan
// that oversteps it is an address error here and not on a device.
#include <stdio.h>

#include <vector>

#include "vc_groups_plan.hpp"

#define CHECK(c)                                                                 \
  do {                                                                           \
    if (!(c)) {                                                                  \
      printf("FAILED %s (line %d) window %llu start %llu size %llu\n", #c, __LINE__, (unsigned long long)window, (unsigned long long)start, \
             (unsigned long long)size);                                          \
      return 1;                                                                  \
    }                                                                            \
  } while (0)

static int one(uint64_t window, uint64_t start, uint64_t size, uint64_t tail) {
  const uint64_t n = start + size + tail;
  const uint32_t tier = vc_group_tier(size);
  CHECK(tier == (size == 0 ? VC_GROUP_NONE : size <= 2 ? VC_GROUP_SMALL : size <= 1024 ? VC_GROUP_WAVE : VC_GROUP_BIG));
  const uint64_t items = vc_group_items(size);
  CHECK(items == (tier == VC_GROUP_WAVE ? 1 : tier == VC_GROUP_BIG ? (size + 1023) / 1024 : 0));
  if (size == 0) return 0;
  std::vector<std::vector<unsigned char>> buf(vc_group_windows(n, window));
  for (uint64_t w = 0; w < buf.size(); ++w) {
    CHECK(vc_group_window_rows(n, window, w) <= vc_group_buffer_rows(n, window));
    CHECK(w * window + vc_group_window_rows(n, window, w) <= n);
    buf[w].assign(vc_group_window_rows(n, window, w), 0);
  }
  if (tier == VC_GROUP_SMALL) {   // taken whole by the window it starts in
    const uint64_t w = vc_group_window_of(start, window);
    for (uint64_t p = start; p < start + size; ++p) buf[w].at(p - w * window) = 1;
  }
  uint64_t next = start;
  for (uint64_t c = 0; c < items; ++c) {
    const uint64_t first = vc_group_item_first(start, c), cnt = vc_group_item_count(size, c);
    CHECK(first == next && cnt >= 1 && cnt <= VC_GROUP_CHUNK);   // the items tile the group in order
    next = first + cnt;
    const uint64_t w = vc_group_window_of(first, window);
    CHECK(w < buf.size() && first >= w * window && first < (w + 1) * window);
    CHECK(first - w * window + cnt <= buf[w].size());
    for (uint64_t p = first; p < first + cnt; ++p) buf[w][p - w * window] += 1;   // (unchecked on purpose: the sanitizer's business)
  }
  CHECK(items == 0 || next == start + size);
  uint64_t covered = 0;
  for (uint64_t w = 0; w < buf.size(); ++w)
    for (unsigned char x : buf[w]) { CHECK(x <= 1); covered += x; }
  CHECK(covered == size);   // every member exactly once
  for (uint64_t w = 0; w <= buf.size(); ++w) {   // the first item at or behind a boundary inside (or around) the group
    const uint64_t pos = w * window < n ? w * window : n;
    if (pos < start || pos >= start + size) continue;
    uint64_t before = 0;
    for (uint64_t c = 0; c < items; ++c) before += vc_group_item_first(start, c) < pos;
    CHECK(vc_group_first_item_from(pos, start, size, 77) == 77 + before);
  }
  return 0;
}

int main() {
  uint64_t window = 0, start = 0, size = 0;
  CHECK(!vc_group_window_valid(0) && !vc_group_window_valid(1000) && !vc_group_window_valid(1536) && vc_group_window_valid(1024));
  CHECK(vc_group_window_valid(2048) && vc_group_window_valid(VC_GROUP_WINDOW_DEFAULT) && !vc_group_window_valid(1ull << 31));
  long cases = 0;
  for (uint64_t win : {1024ull, 2048ull}) {
    const uint64_t starts[] = {0, 1, 2, 1023, 1024, 1025, win - 2, win - 1, win, win + 1, 2 * win - 1, 3 * win - 1, 3 * win, 5 * win - 1023};
    for (uint64_t st : starts)
      for (uint64_t sz = 0; sz <= 4097; ++sz)
        for (uint64_t tail : {0ull, 5ull}) {
          if (int rc = one(win, st, sz, tail)) return rc;
          ++cases;
        }
  }
  for (uint64_t n : {1ull, 2ull, 1000ull, 1ull << 20, (1ull << 20) + 7}) {   // the scratch arrays lie side by side
    const VcGroupsScratchPlan sp(n, 1001, 33);
    const uint64_t offs[] = {sp.off_meta(), sp.off_pair(0, 0), sp.off_pair(0, 1), sp.off_pair(1, 0), sp.off_pair(1, 1), sp.off_gnum(), sp.off_starts(),
                             sp.off_sort_work(), sp.off_scan_work(), sp.total};
    window = n;
    CHECK(offs[1] - offs[0] >= 8);
    for (int i = 1; i < 7; ++i) CHECK(offs[i + 1] - offs[i] >= n + 2);
    CHECK(offs[8] - offs[7] >= 1001 && offs[9] - offs[8] >= 33);
    const VcGroupsScratchPlan sw(n, 1001, 33, vc_group_windows(n, 1024));
    CHECK(sw.off_win_big() - sw.off_scan_work() >= 33 && sw.total - sw.off_win_big() >= vc_group_windows(n, 1024) && sw.off_win_big() == sp.total);
    const VcGroupsWorkPlan wp(n, 2048, 8, 3);
    CHECK(wp.best - wp.rows == vc_group_buffer_rows(n, 2048) * 64 && wp.cents - wp.best == 24 && wp.counters - wp.cents == 3 * 64);
    CHECK(wp.maxd - wp.counters == 3 * 512 * 4 && wp.big_group - wp.maxd == 12 && wp.win_items - wp.big_group == 12);
    CHECK(wp.total >= wp.win_items + (vc_group_windows(n, 2048) + 1) * 4);
  }
  printf("groups plan ok: %ld cases\n", cases);
  return 0;
}
