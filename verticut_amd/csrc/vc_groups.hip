// ============================================================================
// vc_groups.hip -- label groups summarised on the device (vc_group_summary*, vc_sharded_group_summary*): per group its size, the
// per-bit majority code (the centroid), the member nearest to it (the representative) and the largest distance of a member to it.
// One driver and one set of kernels for both handle kinds: the codes are read through a fetch callback (vc_get_codes_dev or
// vc_sharded_get_codes_dev, both unchanged) into contiguous rows.
// ============================================================================
#include <algorithm>

#include "vc_groups_plan.hpp"
#include "vc_internal.hpp"

// THE RULE: two records are in one group iff their labels are equal; the groups are numbered by ascending label.  Bit b of a group's
// centroid is 1 iff STRICTLY more than half of the members have it set (a tie in an even group gives 0); this code minimises the sum
// of Hamming distances to the members.  The representative is the member with the smallest (distance to the centroid, id).
// SORT AND NUMBER: keys label - id_base (range-checked, clamped to 0 and flagged when outside) with the global ids as values go
// through the stable radix sort, so a group's members lie contiguous and in ascending id order.  Head flags, scanned, number the
// positions' groups (gnum[p] = heads before p, gnum[n] = G); the heads scatter the group starts; the groups' item counts and big
// flags, scanned, number the work items and the big groups.  One read-back: the error flag, G, the items, the big groups, and per
// window whether a chunk of a big group starts in it.
// WINDOWS: the rows of the sorted ids are fetched window by window (vc_groups_plan.hpp) and a window's launches take what STARTS in it.
// TIERS by group size: 1 .. 2 one thread per group in closed form; 3 .. 1024 one wave per group, vote and distances out of the same
// rows; above 1024 one wave per chunk of 1024, whose vote counts meet in a counter table by atomicAdd -- the centroid of such a group
// exists only after its last chunk, which may lie windows later, so its distances are taken in a SECOND walk of the windows (only
// when a big group exists), meeting in 64-bit atomicMin / atomicMax.  All of it integer arithmetic: no order of lanes changes a bit.
// THE VOTE in a wave: 64 members per round, for word j and bit b the ballot of (w >> b) & 1, whose popcount lane b adds to its
// counter of word j; centroid word j is the ballot of 2 * count > size.  W counters per lane, no LDS, no scratch.
#define GR_BLK 256u
#define GR_WAVES (GR_BLK / VC_WAVE)

namespace {

struct GrMeta { uint32_t bad, n_groups, n_items, n_big, pad[4]; };   // the 8 words at the head of the scratch

__global__ void __launch_bounds__(GR_BLK) vc_groups_prep_kernel(const uint32_t* __restrict__ labels, uint64_t n, uint32_t id_base,
                                                                 uint32_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t* meta) {
  for (uint64_t i0 = (uint64_t)blockIdx.x * GR_BLK; i0 < n; i0 += (uint64_t)gridDim.x * GR_BLK) {
    const uint64_t i = i0 + threadIdx.x;
    bool bad = false;
    if (i < n) {
      uint32_t k = labels[i] - id_base;   // (mod 2^32: a label below id_base wraps to a large key)
      bad = k >= n;
      keys[i] = bad ? 0u : k;             // clamped: nothing downstream ever forms an address from a label outside the range
      vals[i] = id_base + (uint32_t)i;
    }
    if (__ballot(bad) && vc_lane() == 0) atomicOr(meta, 1u);
  }
}

// flags[p] = 1 at the first position of a group, flags[n] = 0: their exclusive scan is gnum
__global__ void __launch_bounds__(GR_BLK) vc_groups_heads_kernel(const uint32_t* __restrict__ keys, uint64_t n, uint32_t* __restrict__ flags) {
  for (uint64_t p = (uint64_t)blockIdx.x * GR_BLK + threadIdx.x; p <= n; p += (uint64_t)gridDim.x * GR_BLK)
    flags[p] = p < n && (p == 0 || keys[p] != keys[p - 1]) ? 1u : 0u;
}

__global__ void __launch_bounds__(GR_BLK) vc_groups_starts_kernel(const uint32_t* __restrict__ gnum, uint64_t n, uint32_t* __restrict__ starts) {
  for (uint64_t p = (uint64_t)blockIdx.x * GR_BLK + threadIdx.x; p <= n; p += (uint64_t)gridDim.x * GR_BLK)
    if (p == n || gnum[p + 1] != gnum[p]) starts[gnum[p]] = (uint32_t)p;   // starts[G] = n
}

// per group its work items and whether it is big, zero behind the last group: both arrays are scanned over n + 1 entries.  A big
// group also marks the windows in which one of its chunks starts (win_big, zeroed before; every writer stores the same 1).
__global__ void __launch_bounds__(GR_BLK) vc_groups_sizes_kernel(const uint32_t* __restrict__ gnum, const uint32_t* __restrict__ starts, uint64_t n,
                                                                  uint64_t window, uint32_t* __restrict__ items, uint32_t* __restrict__ bigs,
                                                                  uint32_t* __restrict__ win_big) {
  const uint32_t G = gnum[n];
  for (uint64_t g = (uint64_t)blockIdx.x * GR_BLK + threadIdx.x; g <= n; g += (uint64_t)gridDim.x * GR_BLK) {
    const uint32_t start = g < G ? starts[g] : 0u, size = g < G ? starts[g + 1] - start : 0u;
    const bool big = vc_group_tier(size) == VC_GROUP_BIG;
    items[g] = (uint32_t)vc_group_items(size);
    bigs[g] = big ? 1u : 0u;
    if (big)
      for (uint64_t c = 0; c < vc_group_items(size); ++c) win_big[vc_group_window_of(vc_group_item_first(start, c), window)] = 1u;
  }
}

__global__ void vc_groups_meta_kernel(const uint32_t* __restrict__ gnum, const uint32_t* __restrict__ item_start, const uint32_t* __restrict__ big_start,
                                      uint64_t n, uint32_t* meta) {
  meta[1] = gnum[n];
  meta[2] = item_start[n];   // (index n >= G: the entries behind the last group repeat the total)
  meta[3] = big_start[n];
}

// win_items[w] = the first work item whose first position is >= w * window (w = number of windows: the item total)
__global__ void __launch_bounds__(GR_BLK) vc_groups_windows_kernel(const uint32_t* __restrict__ gnum, const uint32_t* __restrict__ starts,
                                                                    const uint32_t* __restrict__ item_start, uint64_t n, uint64_t window, uint32_t n_win,
                                                                    uint32_t* __restrict__ win_items) {
  for (uint32_t w = blockIdx.x * GR_BLK + threadIdx.x; w <= n_win; w += gridDim.x * GR_BLK) {
    const uint64_t pos = (uint64_t)w * window < n ? (uint64_t)w * window : n;
    const uint32_t G = gnum[n];
    if (pos >= n) { win_items[w] = item_start[G]; continue; }
    const uint32_t g = gnum[pos + 1] - 1;   // the group that contains pos
    win_items[w] = (uint32_t)vc_group_first_item_from(pos, starts[g], starts[g + 1] - starts[g], item_start[g]);
  }
}

__device__ __forceinline__ void gr_store_group(vc_group* dst, uint32_t label, uint32_t size, uint32_t rep, uint32_t rep_dist, uint32_t max_dist) {
  vc_group v;
  v.label = label; v.size = size; v.rep = rep; v.rep_dist = rep_dist; v.max_dist = max_dist; v.reserved = 0;
  *dst = v;
}

// Small tier of one window: one thread per group that starts in [pos_lo, pos_hi).  rows = the window's buffer, row 0 = position pos_lo.
template <int W>
__global__ void __launch_bounds__(GR_BLK) vc_groups_small_kernel(const uint32_t* __restrict__ gnum, const uint32_t* __restrict__ starts,
                                                                  const uint32_t* __restrict__ keys, const uint32_t* __restrict__ ids,
                                                                  const uint64_t* __restrict__ rows, uint64_t pos_lo, uint64_t pos_hi, uint32_t id_base,
                                                                  vc_group* __restrict__ groups, uint64_t* __restrict__ cents) {
  const uint32_t g_lo = gnum[pos_lo], g_hi = gnum[pos_hi];   // heads before a position = the first group starting at or behind it
  for (uint32_t g = g_lo + blockIdx.x * GR_BLK + threadIdx.x; g < g_hi; g += gridDim.x * GR_BLK) {
    const uint32_t start = starts[g], size = starts[g + 1] - start;
    if (size > 2) continue;
    const uint64_t* a = rows + (uint64_t)(start - pos_lo) * W;
    uint32_t d0 = 0, d1 = 0;
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const uint64_t x = a[j], y = size == 2 ? a[W + j] : x, c = x & y;   // two members: a bit needs both to be a majority
      d0 += (uint32_t)__popcll(x ^ c);
      d1 += (uint32_t)__popcll(y ^ c);
      if (cents) cents[(uint64_t)g * W + j] = c;
    }
    const bool second = size == 2 && d1 < d0;   // ascending ids: the first member wins a tie
    gr_store_group(groups + g, keys[start] + id_base, size, ids[start + (second ? 1 : 0)], second ? d1 : d0, d0 > d1 ? d0 : d1);
  }
}

__device__ __forceinline__ uint64_t gr_wave_min64(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t o = __shfl_xor(v, off);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ uint32_t gr_wave_max32(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t o = __shfl_xor(v, off);
    v = o > v ? o : v;
  }
  return v;
}

// the vote of `cnt` rows: lane b's counter j = the rows whose word j has bit b set
template <int W>
__device__ __forceinline__ void gr_vote(const uint64_t* __restrict__ rows, uint32_t cnt, uint32_t lane, uint32_t (&votes)[W]) {
#pragma unroll
  for (int j = 0; j < W; ++j) votes[j] = 0;
  for (uint32_t r0 = 0; r0 < cnt; r0 += VC_WAVE) {   // wave-uniform bounds: every lane takes part in every ballot
    const uint32_t m = r0 + lane;
    uint64_t w[W];
#pragma unroll
    for (int j = 0; j < W; ++j) w[j] = m < cnt ? rows[(uint64_t)m * W + j] : 0ull;
#pragma unroll
    for (int j = 0; j < W; ++j) {
#pragma unroll 8
      for (uint32_t b = 0; b < 64; ++b) {
        const uint32_t ones = (uint32_t)__popcll(__ballot((w[j] >> b) & 1ull));
        votes[j] += lane == b ? ones : 0u;
      }
    }
  }
}

// smallest packed (distance, id) and largest distance of `cnt` rows to the centroid c (wave-uniform results)
template <int W>
__device__ __forceinline__ void gr_distances(const uint64_t* __restrict__ rows, const uint32_t* __restrict__ ids, uint32_t cnt, uint32_t lane,
                                             const uint64_t (&c)[W], uint64_t* best, uint32_t* maxd) {
  uint64_t b = VC_PACK_INF;
  uint32_t mx = 0;
  for (uint32_t m = lane; m < cnt; m += VC_WAVE) {
    uint32_t d = 0;
#pragma unroll
    for (int j = 0; j < W; ++j) d += (uint32_t)__popcll(rows[(uint64_t)m * W + j] ^ c[j]);
    const uint64_t p = vc_pack(d, ids[m]);
    b = p < b ? p : b;
    mx = d > mx ? d : mx;
  }
  *best = gr_wave_min64(b);
  *maxd = gr_wave_max32(mx);
}

struct GrBig {   // per big group b (numbered by the scan of the big flags)
  unsigned long long* best;   // packed (distance, id) minimum, starts as VC_PACK_INF
  uint64_t* cents;            // [W]
  uint32_t* counters;         // [W * 64] votes
  uint32_t* maxd;             // starts as 0
  uint32_t* group;            // the group's number
};

// Work items [win_items[w], win_items[w + 1]) of window w, one wave per item.  pass 0: the vote; a group of the wave tier is finished
// here, a big group's chunk adds its votes to the counter table.  pass 1 (big groups only): the chunk's distances to the finished centroid.
template <int W>
__global__ void __launch_bounds__(GR_BLK) vc_groups_items_kernel(const uint32_t* __restrict__ starts, const uint32_t* __restrict__ item_start,
                                                                  const uint32_t* __restrict__ big_start, const uint32_t* __restrict__ keys,
                                                                  const uint32_t* __restrict__ ids, const uint64_t* __restrict__ rows,
                                                                  const uint32_t* __restrict__ win_items, uint32_t w, uint64_t pos_lo, uint32_t G,
                                                                  uint32_t id_base, int pass, GrBig big, vc_group* __restrict__ groups,
                                                                  uint64_t* __restrict__ cents) {
  const uint32_t lane = vc_lane();
  const uint32_t it_lo = win_items[w], it_hi = win_items[w + 1];
  for (uint32_t it = it_lo + blockIdx.x * GR_WAVES + threadIdx.x / VC_WAVE; it < it_hi; it += gridDim.x * GR_WAVES) {   // wave-uniform
    uint32_t lo = 0, hi = G;   // item_start[lo] <= it < item_start[hi]: the last group whose first item is <= it owns it
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (item_start[mid] <= it) lo = mid; else hi = mid;
    }
    const uint32_t g = lo, start = starts[g], size = starts[g + 1] - start, c = it - item_start[g];
    const bool is_big = vc_group_tier(size) == VC_GROUP_BIG;
    if (pass == 1 && !is_big) continue;
    const uint64_t first = vc_group_item_first(start, c);
    const uint32_t cnt = vc_group_item_count(size, c);
    const uint64_t* r = rows + (first - pos_lo) * W;
    const uint32_t* rid = ids + first;
    uint64_t cw[W];
    if (pass == 0) {
      uint32_t votes[W];
      gr_vote<W>(r, cnt, lane, votes);
      if (is_big) {
        const uint32_t b = big_start[g];
#pragma unroll
        for (int j = 0; j < W; ++j) atomicAdd(big.counters + ((uint64_t)b * W + j) * 64 + lane, votes[j]);
        if (c == 0 && lane == 0) big.group[b] = g;
        continue;
      }
#pragma unroll
      for (int j = 0; j < W; ++j) cw[j] = __ballot(2u * votes[j] > size);
    } else {
#pragma unroll
      for (int j = 0; j < W; ++j) cw[j] = big.cents[(uint64_t)big_start[g] * W + j];
    }
    uint64_t best;
    uint32_t maxd;
    gr_distances<W>(r, rid, cnt, lane, cw, &best, &maxd);
    if (lane == 0) {
      if (is_big) {
        atomicMin(big.best + big_start[g], (unsigned long long)best);
        atomicMax(big.maxd + big_start[g], maxd);
      } else {
        gr_store_group(groups + g, keys[start] + id_base, size, (uint32_t)best, (uint32_t)(best >> 32), maxd);
        if (cents)
#pragma unroll
          for (int j = 0; j < W; ++j) cents[(uint64_t)g * W + j] = cw[j];
      }
    }
  }
}

// between the walks: one wave per big group turns its counters into the centroid
__global__ void __launch_bounds__(GR_BLK) vc_groups_big_centroid_kernel(const uint32_t* __restrict__ starts, uint32_t n_big, uint32_t W, GrBig big,
                                                                         uint64_t* __restrict__ cents) {
  const uint32_t lane = vc_lane();
  for (uint32_t b = blockIdx.x * GR_WAVES + threadIdx.x / VC_WAVE; b < n_big; b += gridDim.x * GR_WAVES) {
    const uint32_t g = big.group[b], size = starts[g + 1] - starts[g];
    for (uint32_t j = 0; j < W; ++j) {
      const uint64_t c = __ballot(2ull * big.counters[((uint64_t)b * W + j) * 64 + lane] > size);
      if (lane == 0) {
        big.cents[(uint64_t)b * W + j] = c;
        if (cents) cents[(uint64_t)g * W + j] = c;
      }
    }
  }
}

// after the second walk: the big groups' records
__global__ void __launch_bounds__(GR_BLK) vc_groups_big_finish_kernel(const uint32_t* __restrict__ starts, const uint32_t* __restrict__ keys,
                                                                       uint32_t n_big, uint32_t id_base, GrBig big, vc_group* __restrict__ groups) {
  for (uint32_t b = blockIdx.x * GR_BLK + threadIdx.x; b < n_big; b += gridDim.x * GR_BLK) {
    const uint32_t g = big.group[b], start = starts[g];
    const uint64_t best = big.best[b];
    gr_store_group(groups + g, keys[start] + id_base, starts[g + 1] - start, (uint32_t)best, (uint32_t)(best >> 32), big.maxd[b]);
  }
}

__global__ void __launch_bounds__(GR_BLK) vc_groups_big_init_kernel(uint32_t n_big, uint32_t W, GrBig big) {
  for (uint64_t i = (uint64_t)blockIdx.x * GR_BLK + threadIdx.x; i < (uint64_t)n_big * W * 64; i += (uint64_t)gridDim.x * GR_BLK) {
    big.counters[i] = 0;
    if (i < n_big) {
      big.best[i] = VC_PACK_INF;
      big.maxd[i] = 0;
    }
  }
}

// per sorted position: its record's group number and its group's representative
__global__ void __launch_bounds__(GR_BLK) vc_groups_scatter_kernel(const uint32_t* __restrict__ gnum, const uint32_t* __restrict__ ids, uint64_t n,
                                                                    uint32_t id_base, const vc_group* __restrict__ groups,
                                                                    uint32_t* __restrict__ rep_labels, uint32_t* __restrict__ group_index) {
  for (uint64_t p = (uint64_t)blockIdx.x * GR_BLK + threadIdx.x; p < n; p += (uint64_t)gridDim.x * GR_BLK) {
    const uint32_t g = gnum[p + 1] - 1, i = ids[p] - id_base;
    if (rep_labels) rep_labels[i] = groups[g].rep;
    if (group_index) group_index[i] = g;
  }
}

uint32_t gr_grid(uint64_t items, uint32_t per_block) {
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + per_block - 1) / per_block, 1), 256 * 8);
}

int gr_fail(std::string* err, hipError_t r, const char* what) {
  if (err) *err = std::string("group summary: ") + what + ": " + hipGetErrorString(r);
  return r == hipErrorOutOfMemory ? VC_ERR_NOMEM : VC_ERR_HIP;
}
#define GR_HIP(call)                                       \
  do {                                                     \
    hipError_t _r = (call);                                \
    if (_r != hipSuccess) return gr_fail(err, _r, #call);  \
  } while (0)

template <int W>
hipError_t gr_launch_window(const VcGroupsArgs& a, const uint32_t* gnum, const uint32_t* starts, const uint32_t* item_start, const uint32_t* big_start,
                            const uint32_t* keys, const uint32_t* ids, const uint64_t* rows, const uint32_t* win_items, uint32_t w, uint32_t G,
                            uint32_t n_items, int pass, const GrBig& big, hipStream_t s) {
  const uint64_t pos_lo = (uint64_t)w * a.window, pos_hi = std::min<uint64_t>(pos_lo + a.window, a.n);
  if (pass == 0)
    hipLaunchKernelGGL(vc_groups_small_kernel<W>, dim3(gr_grid(std::min<uint64_t>(G, pos_hi - pos_lo), GR_BLK)), dim3(GR_BLK), 0, s, gnum, starts, keys, ids,
                       rows, pos_lo, pos_hi, a.id_base, a.d_groups, a.d_centroids);
  if (n_items)
    hipLaunchKernelGGL(vc_groups_items_kernel<W>, dim3(gr_grid(std::min<uint64_t>(n_items, (pos_hi - pos_lo) / 3 + 1), GR_WAVES)), dim3(GR_BLK), 0, s, starts,
                       item_start, big_start, keys, ids, rows, win_items, w, pos_lo, G, a.id_base, pass, big, a.d_groups, a.d_centroids);
  return hipGetLastError();
}

}  // namespace

int vc_groups_run(const VcGroupsArgs& a, const VcGroupsFetch& fetch, uint64_t* n_groups, hipStream_t s, std::string* err) {
  const uint64_t n = a.n;
  if (n_groups) *n_groups = 0;
  if (n == 0) return VC_OK;
  if (n + 2 > 0xFFFFFFFFull) {   // (the prefix sums are 32-bit words over n + 1 entries)
    if (err) *err = "group summary: more than 2^32 - 3 records";
    return VC_ERR_INVALID;
  }
  uint32_t key_bits = 0;
  while (key_bits < 32 && (1ull << key_bits) < n) ++key_bits;
  const uint32_t n_win = (uint32_t)vc_group_windows(n, a.window);
  const VcGroupsScratchPlan sp(n, vc_radix_sort_work_words(n), vc_scan_work_words(n + 1), n_win);
  uint32_t* base = (uint32_t*)a.alloc(VC_GROUPS_SCRATCH, sp.total * 4);
  if (!base) return VC_ERR_NOMEM;
  uint32_t* meta = base + sp.off_meta();
  uint32_t* keys[2] = {base + sp.off_pair(0, 0), base + sp.off_pair(1, 0)};
  uint32_t* vals[2] = {base + sp.off_pair(0, 1), base + sp.off_pair(1, 1)};
  uint32_t* gnum = base + sp.off_gnum();
  uint32_t* starts = base + sp.off_starts();
  uint32_t* scan_work = base + sp.off_scan_work();
  uint32_t* win_big = base + sp.off_win_big();
  const int res = (int)(vc_radix_sort_passes(key_bits) & 1);
  const uint32_t* skeys = keys[res];
  const uint32_t* sids = vals[res];
  uint32_t* item_start = keys[res ^ 1];   // the pair the sort has left
  uint32_t* big_start = vals[res ^ 1];
  const uint32_t grid_n = gr_grid(n + 1, GR_BLK);

  GR_HIP(hipMemsetAsync(meta, 0, 32, s));
  GR_HIP(hipMemsetAsync(win_big, 0, (size_t)n_win * 4, s));
  hipLaunchKernelGGL(vc_groups_prep_kernel, dim3(grid_n), dim3(GR_BLK), 0, s, a.d_labels, n, a.id_base, keys[0], vals[0], meta);
  GR_HIP(hipGetLastError());
  GR_HIP(vc_radix_sort_pairs(keys, vals, n, key_bits, base + sp.off_sort_work(), s));
  hipLaunchKernelGGL(vc_groups_heads_kernel, dim3(grid_n), dim3(GR_BLK), 0, s, skeys, n, gnum);
  GR_HIP(hipGetLastError());
  GR_HIP(vc_exclusive_scan_u32(gnum, gnum, n + 1, scan_work, s));
  hipLaunchKernelGGL(vc_groups_starts_kernel, dim3(grid_n), dim3(GR_BLK), 0, s, gnum, n, starts);
  hipLaunchKernelGGL(vc_groups_sizes_kernel, dim3(grid_n), dim3(GR_BLK), 0, s, gnum, starts, n, (uint64_t)a.window, item_start, big_start, win_big);
  GR_HIP(hipGetLastError());
  GR_HIP(vc_exclusive_scan_u32(item_start, item_start, n + 1, scan_work, s));
  GR_HIP(vc_exclusive_scan_u32(big_start, big_start, n + 1, scan_work, s));
  hipLaunchKernelGGL(vc_groups_meta_kernel, dim3(1), dim3(1), 0, s, gnum, item_start, big_start, n, meta);
  GR_HIP(hipGetLastError());
  GrMeta m{};
  GR_HIP(hipMemcpyAsync(&m, meta, sizeof m, hipMemcpyDeviceToHost, s));
  std::vector<uint32_t> has_big(n_win);
  GR_HIP(hipMemcpyAsync(has_big.data(), win_big, (size_t)n_win * 4, hipMemcpyDeviceToHost, s));
  GR_HIP(hipStreamSynchronize(s));   // the one wait: everything below is sized by what came home
  if (m.bad) {
    if (err) *err = "group summary: a label lies outside the resident id range";
    return VC_ERR_INVALID;
  }
  const uint32_t G = m.n_groups;
  if (n_groups) *n_groups = G;
  if (G > a.groups_cap) {
    if (err) *err = "group summary: more groups than groups_cap (the count is in *n_groups)";
    return VC_ERR_CAPACITY;
  }

  const VcGroupsWorkPlan wp(n, a.window, a.W, m.n_big);
  uint8_t* work = (uint8_t*)a.alloc(VC_GROUPS_WORK, wp.total);
  if (!work) return VC_ERR_NOMEM;
  uint64_t* rows = (uint64_t*)(work + wp.rows);
  uint32_t* win_items = (uint32_t*)(work + wp.win_items);
  GrBig big;
  big.best = (unsigned long long*)(work + wp.best);
  big.cents = (uint64_t*)(work + wp.cents);
  big.counters = (uint32_t*)(work + wp.counters);
  big.maxd = (uint32_t*)(work + wp.maxd);
  big.group = (uint32_t*)(work + wp.big_group);
  hipLaunchKernelGGL(vc_groups_windows_kernel, dim3(gr_grid(n_win + 1, GR_BLK)), dim3(GR_BLK), 0, s, gnum, starts, item_start, n, (uint64_t)a.window, n_win,
                     win_items);
  if (m.n_big) hipLaunchKernelGGL(vc_groups_big_init_kernel, dim3(gr_grid((uint64_t)m.n_big * a.W * 64, GR_BLK)), dim3(GR_BLK), 0, s, m.n_big, a.W, big);
  GR_HIP(hipGetLastError());
  for (int pass = 0; pass < (m.n_big ? 2 : 1); ++pass) {
    if (pass == 1) {
      hipLaunchKernelGGL(vc_groups_big_centroid_kernel, dim3(gr_grid(m.n_big, GR_WAVES)), dim3(GR_BLK), 0, s, starts, m.n_big, a.W, big, a.d_centroids);
      GR_HIP(hipGetLastError());
    }
    for (uint32_t w = 0; w < n_win; ++w) {
      if (pass == 1 && !has_big[w]) continue;   // no chunk of a big group starts here: neither a gather nor a launch
      if (pass == 0 || n_win > 1) {   // (a single window's rows are still in the buffer for the second walk)
        const int rc = fetch(sids + (uint64_t)w * a.window, (uint32_t)vc_group_window_rows(n, a.window, w), rows);
        if (rc) return rc;
      }
      hipError_t r = hipSuccess;
      switch (a.W) {
        case 1: r = gr_launch_window<1>(a, gnum, starts, item_start, big_start, skeys, sids, rows, win_items, w, G, m.n_items, pass, big, s); break;
        case 2: r = gr_launch_window<2>(a, gnum, starts, item_start, big_start, skeys, sids, rows, win_items, w, G, m.n_items, pass, big, s); break;
        case 4: r = gr_launch_window<4>(a, gnum, starts, item_start, big_start, skeys, sids, rows, win_items, w, G, m.n_items, pass, big, s); break;
        case 8: r = gr_launch_window<8>(a, gnum, starts, item_start, big_start, skeys, sids, rows, win_items, w, G, m.n_items, pass, big, s); break;
        default: r = hipErrorInvalidValue;
      }
      GR_HIP(r);
    }
  }
  if (m.n_big) hipLaunchKernelGGL(vc_groups_big_finish_kernel, dim3(gr_grid(m.n_big, GR_BLK)), dim3(GR_BLK), 0, s, starts, skeys, m.n_big, a.id_base, big, a.d_groups);
  if (a.d_rep_labels || a.d_group_index)
    hipLaunchKernelGGL(vc_groups_scatter_kernel, dim3(grid_n), dim3(GR_BLK), 0, s, gnum, sids, n, a.id_base, a.d_groups, a.d_rep_labels, a.d_group_index);
  GR_HIP(hipGetLastError());
  return VC_OK;
}

int vc_groups_run_host(VcGroupsArgs a, const VcGroupsFetch& fetch, const uint32_t* labels, vc_group* groups, void* centroids, uint32_t* rep_labels,
                       uint32_t* group_index, uint64_t* n_groups, hipStream_t s, std::string* err) {
  const uint64_t n = a.n, cap = std::min<uint64_t>(a.groups_cap, n);   // (there are never more than n groups)
  if (n_groups) *n_groups = 0;
  if (n == 0) return VC_OK;
  const size_t row = (size_t)a.W * 8, words = (((size_t)n * 4 + 7) & ~(size_t)7);   // staged: labels | groups | centroids | rep_labels | group_index
  const size_t off_groups = words, off_cents = off_groups + (size_t)cap * sizeof(vc_group), off_rep = off_cents + (centroids ? (size_t)cap * row : 0),
               off_gi = off_rep + (rep_labels ? words : 0), total = off_gi + (group_index ? words : 0);
  uint8_t* stage = (uint8_t*)a.alloc(VC_GROUPS_STAGE, total);
  if (!stage) return VC_ERR_NOMEM;
  GR_HIP(hipMemcpyAsync(stage, labels, (size_t)n * 4, hipMemcpyHostToDevice, s));
  a.d_labels = (const uint32_t*)stage;
  a.groups_cap = cap;
  a.d_groups = (vc_group*)(stage + off_groups);
  a.d_centroids = centroids ? (uint64_t*)(stage + off_cents) : nullptr;
  a.d_rep_labels = rep_labels ? (uint32_t*)(stage + off_rep) : nullptr;
  a.d_group_index = group_index ? (uint32_t*)(stage + off_gi) : nullptr;
  uint64_t G = 0;
  const int rc = vc_groups_run(a, fetch, &G, s, err);
  if (n_groups) *n_groups = G;
  if (rc) return rc;
  if (G) GR_HIP(hipMemcpyAsync(groups, a.d_groups, (size_t)G * sizeof(vc_group), hipMemcpyDeviceToHost, s));
  if (centroids && G) GR_HIP(hipMemcpyAsync(centroids, a.d_centroids, (size_t)G * row, hipMemcpyDeviceToHost, s));
  if (rep_labels) GR_HIP(hipMemcpyAsync(rep_labels, a.d_rep_labels, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  if (group_index) GR_HIP(hipMemcpyAsync(group_index, a.d_group_index, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  GR_HIP(hipStreamSynchronize(s));
  return VC_OK;
}
