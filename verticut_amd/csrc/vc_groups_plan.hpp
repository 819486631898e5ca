// Plan arithmetic of vc_group_summary* (vc_groups.hip): the tier of a group size, the work items of a group, the window of an item and
// the buffer sizes.  Plain C++ with no HIP in it, so that tests/cpp/groups_plan_test.cc checks it on the CPU; the kernels and the
// host driver call exactly these functions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VC_GP_FN __host__ __device__ inline
#else
#define VC_GP_FN inline
#endif

#define VC_GROUP_CHUNK 1024u                   // sorted positions per work item, and the overlap a window's buffer carries
#define VC_GROUP_WINDOW_DEFAULT (1u << 20)     // VC_GROUP_WINDOW: sorted positions whose items one gather serves
#define VC_GROUP_WINDOW_MAX (1u << 30)

// Groups lie contiguous in the sorted order: group g holds the sorted positions [start, start + size).
enum VcGroupTier : uint32_t {
  VC_GROUP_NONE = 0,    // size 0 (no such group)
  VC_GROUP_SMALL = 1,   // 1 .. 2 members: one thread, closed form, no work item
  VC_GROUP_WAVE = 2,    // 3 .. 1024: one work item, the whole group in one wave
  VC_GROUP_BIG = 3      // above 1024: one work item per chunk of 1024, partial results meet in atomics
};
VC_GP_FN uint32_t vc_group_tier(uint64_t size) {
  return size == 0 ? VC_GROUP_NONE : size <= 2 ? VC_GROUP_SMALL : size <= VC_GROUP_CHUNK ? VC_GROUP_WAVE : VC_GROUP_BIG;
}
// work items of a group: none for the small tier, else its chunks of 1024
VC_GP_FN uint64_t vc_group_items(uint64_t size) { return size <= 2 ? 0 : (size + VC_GROUP_CHUNK - 1) / VC_GROUP_CHUNK; }
// item c of a group: its first sorted position and its length (1 .. 1024)
VC_GP_FN uint64_t vc_group_item_first(uint64_t start, uint64_t c) { return start + c * VC_GROUP_CHUNK; }
VC_GP_FN uint32_t vc_group_item_count(uint64_t size, uint64_t c) {
  const uint64_t left = size - c * VC_GROUP_CHUNK;
  return (uint32_t)(left < VC_GROUP_CHUNK ? left : VC_GROUP_CHUNK);
}

VC_GP_FN bool vc_group_window_valid(uint64_t window) {
  return window >= VC_GROUP_CHUNK && window <= VC_GROUP_WINDOW_MAX && window % VC_GROUP_CHUNK == 0;
}
// Window w serves the items and small groups whose FIRST position lies in [w * window, (w + 1) * window); its buffer holds the rows
// of the positions [w * window, w * window + rows).  An item is at most 1024 positions long and a small group at most 2, so with
// 1024 positions of overlap whatever starts in a window lies wholly inside its buffer (or ends at n).
VC_GP_FN uint64_t vc_group_windows(uint64_t n, uint64_t window) { return (n + window - 1) / window; }
VC_GP_FN uint64_t vc_group_window_of(uint64_t pos, uint64_t window) { return pos / window; }
VC_GP_FN uint64_t vc_group_window_rows(uint64_t n, uint64_t window, uint64_t w) {
  const uint64_t left = n - w * window;
  return left < window + VC_GROUP_CHUNK ? left : window + VC_GROUP_CHUNK;
}
VC_GP_FN uint64_t vc_group_buffer_rows(uint64_t n, uint64_t window) { return n < window + VC_GROUP_CHUNK ? n : window + VC_GROUP_CHUNK; }
// The items are numbered group after group, chunk after chunk, so by ascending first position: those of a window are a range.  The
// number of the first item whose first position is >= pos, where the group that CONTAINS pos starts at `start`, has `size` members
// and its item 0 has number item_base.
VC_GP_FN uint64_t vc_group_first_item_from(uint64_t pos, uint64_t start, uint64_t size, uint64_t item_base) {
  if (pos <= start) return item_base;
  const uint64_t items = vc_group_items(size), skip = (pos - start + VC_GROUP_CHUNK - 1) / VC_GROUP_CHUNK;
  return item_base + (skip < items ? skip : items);
}

// The first scratch buffer, in 32-bit words (the sort's and the scan's work sizes come from vc_sort.hip).  Four arrays of n + 2 words for
// the radix sort's ping-pong (after the sort the pair that does not hold the result carries the item and big-group prefix sums), the
// group numbers per position, the group starts: 24 n bytes and change; 8 counter words lead.
struct VcGroupsScratchPlan {
  uint64_t arr;          // words of each of the six arrays: n + 2, rounded to even
  uint64_t sort_work, scan_work, win_big, total;
  // n_win: the windows of the call -- one word each says whether a chunk of a big group starts in the window (read back with G, so
  // that the second walk skips the windows that hold none)
  VcGroupsScratchPlan(uint64_t n, uint64_t sort_work_words, uint64_t scan_work_words, uint64_t n_win = 0)
      : arr((n + 3) & ~1ull), sort_work((sort_work_words + 1) & ~1ull), scan_work((scan_work_words + 1) & ~1ull), win_big((n_win + 1) & ~1ull),
        total(8 + 6 * arr + sort_work + scan_work + win_big) {}
  uint64_t off_meta() const { return 0; }
  uint64_t off_pair(int which, int vals) const { return 8 + (uint64_t)(2 * which + vals) * arr; }
  uint64_t off_gnum() const { return 8 + 4 * arr; }
  uint64_t off_starts() const { return 8 + 5 * arr; }
  uint64_t off_sort_work() const { return 8 + 6 * arr; }
  uint64_t off_scan_work() const { return 8 + 6 * arr + sort_work; }
  uint64_t off_win_big() const { return 8 + 6 * arr + sort_work + scan_work; }
};
// The second buffer, sized once G and the number of big groups are known, in bytes: the row buffer, the windows' first items and,
// per big group, bits vote counters, the centroid, the packed best (distance, id), the largest distance and the group's number.
struct VcGroupsWorkPlan {
  uint64_t rows, win_items, counters, cents, best, maxd, big_group, total;   // byte offsets, then the total
  VcGroupsWorkPlan(uint64_t n, uint64_t window, uint32_t W, uint64_t n_big) {
    uint64_t o = 0;
    rows = o;      o += vc_group_buffer_rows(n, window) * W * 8;
    best = o;      o += n_big * 8;
    cents = o;     o += n_big * W * 8;
    counters = o;  o += n_big * W * 64 * 4;
    maxd = o;      o += n_big * 4;
    big_group = o; o += n_big * 4;
    win_items = o; o += (vc_group_windows(n, window) + 1) * 4;
    total = (o + 255) & ~255ull;
  }
};
