// ============================================================================
// vc_knn_graph_update.hip -- a built k-NN graph brought up to date after vc_add_codes (vc_knn_graph_update*,
// vc_sharded_knn_graph_update*); the header states the contract.  One driver for both handle kinds over a VcStoreView; the plan
// arithmetic is vc_knn_graph_update_plan.hpp.  The rows of the new records are vc_knn_graph_run over [n_old, N), unchanged.  The rows
// of the old records need no search: old row i changes only where a new record j has (dist(i, j) << 32 | id_j) < row_i[k - 1], a
// threshold join of the old records against the new ones.
//   vc_kgraph_join_kernel     vc_assign_kernel's data flow with a per-record threshold in place of the running minimum: a thread keeps
//                             R old records and their thresholds in registers, a window of new codes streams past in LDS tiles read as
//                             broadcasts.  FILL = false counts a record's hits, FILL = true writes them at the record's offset, in
//                             ascending new id, without atomics; a block without a hit leaves the fill pass before it stages a tile
//   vc_kgraph_list_kernel     the ascending list of the affected records, placed by the exclusive scan of their flags (vc_sort.hip)
//   vc_kgraph_merge_kernel    one wave per affected record: the k smallest of its row and its hits by rank counting, out of place
//   vc_kgraph_copy_kernel     the merged rows and their counts back into the graph
//   vc_kgraph_marks_kernel    the records of a batch that any window changed
//   vc_kgraph_inserted_kernel the entries of the old rows that name a new record
// None of them uses scratch memory or waits for another block.  The only address formed from data is that of row_i through the
// affected list, and of a record's hits through its offset; both are bounds-checked.
// ============================================================================
#include <algorithm>
#include <vector>

#include "vc_internal.hpp"
#include "vc_knn_graph_plan.hpp"
#include "vc_knn_graph_update_plan.hpp"

static_assert(sizeof(vc_knn_graph_update_stats) == 64, "the header's size");

namespace {

#define KU_BLK 256u

// what a join launch works on; q, rows, counts and the per-record arrays are those of the old batch, codes those of the window
struct JoinArgs {
  const uint64_t* q;          // [nb][W]
  const uint64_t* rows;       // [nb][k]
  const uint32_t* counts;     // [nb], nullable: a row's last word says whether it is full
  uint32_t nb, k;
  const uint64_t* codes;      // [nw][W]
  uint32_t nw, first_id;      // the global id of the window's record 0
  uint32_t* cnt;              // [nb]: count pass out, fill pass unused
  uint32_t* flag;             // [nb]: cnt > 0
  uint32_t* blk;              // [blocks]: the block has a hit
  const uint32_t* offs;       // [nb]: the exclusive scan of cnt (fill pass)
  uint64_t* hits;             // [n_hits] (fill pass)
  uint64_t n_hits;
  unsigned long long* stat;   // VC_KGUPD_ST_*
};

template <int W, int R, bool FILL>
__global__ void __launch_bounds__(VC_KGUPD_BLOCK) vc_kgraph_join_kernel(const JoinArgs a) {
  static_assert(R == (int)vc_kgupd_records(W), "the plan's records per thread");
  __shared__ uint64_t lds[VC_KGUPD_LDS_WORDS];
  if (FILL && a.blk[blockIdx.x] == 0u) return;   // block-uniform, before any barrier: nothing of this block passed a threshold
  uint64_t rec[R][W], T[R];
  uint32_t c[R];   // count pass: the hits so far; fill pass: the place of the next hit
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint64_t i = vc_kgupd_record_of(W, blockIdx.x, threadIdx.x, r);
    const bool valid = i < a.nb;
#pragma unroll
    for (int w = 0; w < W; ++w) rec[r][w] = valid ? a.q[i * W + w] : 0ull;
    T[r] = 0ull;   // nothing is below it
    c[r] = 0u;
    if (valid) {
      const uint64_t last = a.rows[i * a.k + a.k - 1];
      if (a.counts) {
        const uint32_t ci = a.counts[i];
        if (ci > a.k) a.stat[VC_KGUPD_ST_BAD] = 1ull;   // not a count vc_knn_graph* wrote: the record takes no hit
        else T[r] = vc_kgupd_threshold(ci, a.k, last);
      } else {
        T[r] = last;   // the padding of a row that is not full is UINT64_MAX
      }
      if (FILL) c[r] = a.offs[i];
    }
  }
  constexpr uint32_t tile = vc_kgupd_tile(W);
  for (uint32_t t0 = 0; t0 < a.nw; t0 += tile) {
    const uint32_t nt = vc_kgupd_tile_records(t0, a.nw, W);
    __syncthreads();   // (the previous tile has been read by every wave)
    for (uint32_t j = threadIdx.x; j < nt * (uint32_t)W; j += VC_KGUPD_BLOCK) lds[j] = a.codes[(uint64_t)t0 * W + j];
    __syncthreads();
#pragma unroll 2
    for (uint32_t n = 0; n < nt; ++n) {
      uint64_t cw[W];
#pragma unroll
      for (int w = 0; w < W; ++w) cw[w] = lds[n * W + w];
      const uint32_t id = a.first_id + t0 + n;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        uint32_t d = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) d += (uint32_t)__builtin_popcountll(rec[r][w] ^ cw[w]);
        const uint64_t p = vc_pack(d, id);
        if (FILL) {
          if (p < T[r]) {
            if (c[r] < a.n_hits) a.hits[c[r]] = p;
            ++c[r];
          }
        } else {
          c[r] += p < T[r] ? 1u : 0u;
        }
      }
    }
  }
  if (FILL) return;
  uint32_t h = 0, affected = 0;   // (at most R * 2^20 hits a thread: a wave's sum fits 32 bits)
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint64_t i = vc_kgupd_record_of(W, blockIdx.x, threadIdx.x, r);
    if (i < a.nb) {
      a.cnt[i] = c[r];
      a.flag[i] = c[r] ? 1u : 0u;
    }
    h += c[r];
    affected += c[r] ? 1u : 0u;
  }
  const uint32_t sh = vc_wave_incl_scan(h), sa = vc_wave_incl_scan(affected), wave = threadIdx.x / VC_WAVE;
  __syncthreads();   // (the last tile has been read by every wave: its words are free)
  if (vc_lane() == VC_WAVE - 1) {
    lds[2 * wave] = sh;
    lds[2 * wave + 1] = sa;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long th = 0, ta = 0;
    for (uint32_t w = 0; w < VC_KGUPD_BLOCK / VC_WAVE; ++w) {
      th += lds[2 * w];
      ta += lds[2 * w + 1];
    }
    a.blk[blockIdx.x] = th ? 1u : 0u;
    if (th) {
      atomicAdd(a.stat + VC_KGUPD_ST_HITS, th);
      atomicAdd(a.stat + VC_KGUPD_ST_AFFECTED, ta);
    }
  }
}

// record i with flag[i] goes to place rank[i] of the list: ascending, independent of block order
__global__ void __launch_bounds__(KU_BLK) vc_kgraph_list_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ rank, uint32_t nb,
                                                                uint32_t* __restrict__ list) {
  const uint32_t i = blockIdx.x * KU_BLK + threadIdx.x;
  if (i >= nb || !flag[i]) return;
  const uint32_t at = rank[i];
  if (at < nb) list[at] = i;
}

// the first entry of row[0 .. m) that is >= x
__device__ __forceinline__ uint32_t ku_lower_bound(const uint64_t* __restrict__ row, uint32_t m, uint64_t x) {
  uint32_t lo = 0, hi = m;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (row[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// what a merge or copy launch works on: the affected records list[a0 .. a0 + na) of the batch
struct MergeArgs {
  uint64_t* rows;             // [nb][k]
  uint32_t* counts;           // [nb], nullable
  uint32_t nb, k;
  const uint32_t* list;
  uint32_t a0, na;
  const uint32_t* offs;       // [nb]
  const uint32_t* cnt;        // [nb]
  const uint64_t* hits;       // [n_hits]
  uint64_t n_hits;
  uint64_t* out;              // [na][k]
  uint32_t* newcnt;           // [affected]
  uint8_t* mark;              // [nb]
};

// One wave per affected record.  The packed values of a row and of its hits are distinct (a hit names a new record, an entry an
// older one, and a hit enters a row only once), so the rank of a value in the union is its place: an old entry at p goes to
// p + #{hits < it}, a hit to #{hits < it} + #{old entries < it}.  Places >= k are dropped, places from the new count on are padding;
// every word of the output row has one writer.  The row itself is only read here.
__global__ void __launch_bounds__(KU_BLK) vc_kgraph_merge_kernel(const MergeArgs a) {
  const uint32_t lane = vc_lane(), at = blockIdx.x * (KU_BLK / VC_WAVE) + threadIdx.x / VC_WAVE;
  if (at >= a.na) return;
  const uint32_t i = a.list[a.a0 + at];
  if (i >= a.nb) return;
  const uint32_t h = a.cnt[i], off = a.offs[i], k = a.k;
  if ((uint64_t)off + h > a.n_hits) return;
  const uint64_t* row = a.rows + (uint64_t)i * k;
  const uint64_t* hit = a.hits + off;
  uint64_t* out = a.out + (uint64_t)at * k;
  const uint32_t c = a.counts ? min(a.counts[i], k) : ku_lower_bound(row, k, VC_PACK_INF);
  const uint32_t nc = vc_kgupd_count(c, h, k);
  for (uint32_t p = lane; p < c; p += VC_WAVE) {
    const uint64_t v = row[p];
    uint32_t below = 0;
    for (uint32_t q = 0; q < h; ++q) below += hit[q] < v ? 1u : 0u;
    if (p + below < k) out[p + below] = v;
  }
  for (uint32_t q0 = lane; q0 < h; q0 += VC_WAVE) {
    const uint64_t v = hit[q0];
    uint32_t below = ku_lower_bound(row, c, v);
    for (uint32_t q = 0; q < h && below < k; ++q) below += hit[q] < v ? 1u : 0u;
    if (below < k) out[below] = v;
  }
  for (uint32_t p = nc + lane; p < k; p += VC_WAVE) out[p] = VC_PACK_INF;
  if (lane == 0) {
    a.newcnt[a.a0 + at] = nc;
    a.mark[i] = 1;
  }
}

// thread e serves entry e % k of affected record a0 + e / k
__global__ void __launch_bounds__(KU_BLK) vc_kgraph_copy_kernel(const MergeArgs a) {
  const uint64_t total = (uint64_t)a.na * a.k;
  for (uint64_t e = (uint64_t)blockIdx.x * KU_BLK + threadIdx.x; e < total; e += (uint64_t)gridDim.x * KU_BLK) {
    const uint32_t at = (uint32_t)(e / a.k), j = (uint32_t)(e % a.k), i = a.list[a.a0 + at];
    if (i >= a.nb) continue;
    a.rows[(uint64_t)i * a.k + j] = a.out[e];
    if (j == 0 && a.counts) a.counts[i] = a.newcnt[a.a0 + at];
  }
}

// *dst += the sum of x over the block's waves: one atomic per wave that has something
__device__ __forceinline__ void ku_wave_add(uint32_t x, unsigned long long* dst) {
  const uint32_t s = vc_wave_incl_scan(x);
  if (vc_lane() == VC_WAVE - 1 && s) atomicAdd(dst, (unsigned long long)s);
}

__global__ void __launch_bounds__(KU_BLK) vc_kgraph_marks_kernel(const uint8_t* __restrict__ mark, uint32_t nb, unsigned long long* __restrict__ dst) {
  uint32_t n = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * KU_BLK + threadIdx.x; i < nb; i += (uint64_t)gridDim.x * KU_BLK) n += mark[i] ? 1u : 0u;
  ku_wave_add(n, dst);
}

// entries of rows [0, total / k) that are no padding and whose id lies in [id_lo, id_lo + n_new)
__global__ void __launch_bounds__(KU_BLK) vc_kgraph_inserted_kernel(const uint64_t* __restrict__ rows, uint64_t total, uint32_t id_lo, uint64_t n_new,
                                                                    unsigned long long* __restrict__ dst) {
  uint32_t n = 0;   // (at most 2^45 / (2048 * 256) entries a thread)
  for (uint64_t e = (uint64_t)blockIdx.x * KU_BLK + threadIdx.x; e < total; e += (uint64_t)gridDim.x * KU_BLK) {
    const uint64_t v = rows[e];
    n += v != VC_PACK_INF && (uint64_t)((uint32_t)v - id_lo) < n_new ? 1u : 0u;
  }
  ku_wave_add(n, dst);
}

uint32_t ku_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + KU_BLK - 1) / KU_BLK, 1), 256 * 8); }

template <int W, bool FILL>
void launch_join_w(const JoinArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((vc_kgraph_join_kernel<W, (int)vc_kgupd_records(W), FILL>), dim3(vc_kgupd_blocks(a.nb, W)), dim3(VC_KGUPD_BLOCK), 0, s, a);
}
template <bool FILL>
hipError_t launch_join(const JoinArgs& a, uint32_t W, hipStream_t s) {
  if (a.nb == 0 || a.nw == 0 || a.k == 0) return hipErrorInvalidValue;
  switch (W) {
    case 1: launch_join_w<1, FILL>(a, s); break;
    case 2: launch_join_w<2, FILL>(a, s); break;
    case 4: launch_join_w<4, FILL>(a, s); break;
    case 8: launch_join_w<8, FILL>(a, s); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

#define KU_HIP(call) VC_HIP_OR_FAIL("k-NN graph update", call)

}  // namespace

// THE STEPS (the header states the rule).  1. the new records' rows: vc_knn_graph_run over [n_old, N).  2. the new records' codes
// gathered once; per old batch its codes gathered once, and per window of new records: the count pass and THE WAIT of the window
// (16 bytes: the hits and the affected records), which the window rule of the plan header judges; the two scans, the list, the fill
// pass, and the merge and copy launches sub-batch by sub-batch.  3. the statistics and the error word come home in one wait.
int vc_knn_graph_update_run(const VcStoreView& v, const VcKnnSearch& linear_knn, const VcKgupdArgs& a, vc_knn_graph_update_stats* stats, hipStream_t s,
                            std::string* err) {
  if (stats) *stats = vc_knn_graph_update_stats{};
  const uint64_t N = v.n, n_old = a.n_old, n_new = N - n_old;
  const uint32_t k = a.build.k, W = v.W;
  vc_knn_graph_update_stats st{};
  int rc;
  if ((rc = vc_knn_graph_run(v, linear_knn, a.build, stats ? &st.build : nullptr, s, err))) return rc;
  if (n_old == 0) {   // a plain build
    if (stats) *stats = st;
    return VC_OK;
  }
  const uint32_t nb_max = (uint32_t)std::min<uint64_t>(a.old_batch, n_old), ng = (uint32_t)std::min<uint64_t>(VC_KGUPD_GATHER_CHUNK, n_new);
  const VcKgupdWork wp(nb_max, ng, W, vc_scan_work_words(nb_max));
  uint8_t* work = (uint8_t*)v.alloc(VC_KGRAPH_UPD_WORK, wp.total);
  uint64_t* d_new = (uint64_t*)v.alloc(VC_KGRAPH_UPD_NEW, (size_t)n_new * W * 8);
  if (!work || !d_new) return VC_ERR_NOMEM;
  unsigned long long* stat = (unsigned long long*)(work + wp.stat);
  uint32_t* cnt = (uint32_t*)(work + wp.cnt);
  uint32_t* flag = (uint32_t*)(work + wp.flag);
  uint32_t* offs = (uint32_t*)(work + wp.offs);
  uint32_t* rank = (uint32_t*)(work + wp.rank);
  uint32_t* list = (uint32_t*)(work + wp.list);
  uint32_t* newcnt = (uint32_t*)(work + wp.newcnt);
  uint32_t* blk = (uint32_t*)(work + wp.blk);
  uint8_t* mark = work + wp.mark;
  uint32_t* scan_work = (uint32_t*)(work + wp.scan_work);
  uint32_t* d_ids = (uint32_t*)(work + wp.ids);
  uint32_t* d_found = (uint32_t*)(work + wp.found);
  uint64_t* d_q = (uint64_t*)(work + wp.q);
  KU_HIP(hipMemsetAsync(stat, 0, VC_KGUPD_STAT_BYTES, s));
  const uint32_t new_id = v.id_base + (uint32_t)n_old;   // the global id of new record 0
  for (uint64_t j0 = 0; j0 < n_new; j0 += ng) {
    const uint32_t n = (uint32_t)std::min<uint64_t>(ng, n_new - j0);
    KU_HIP(vc_launch_cluster_init(d_ids, n, new_id + (uint32_t)j0, s));
    if ((rc = v.gather(d_ids, n, d_new + j0 * W, d_found))) return rc;
  }
  for (uint64_t pos = 0; pos < n_old; pos += a.old_batch) {
    const uint32_t nb = (uint32_t)std::min<uint64_t>(a.old_batch, n_old - pos);
    KU_HIP(vc_launch_cluster_init(d_ids, nb, v.id_base + (uint32_t)pos, s));
    if ((rc = v.gather(d_ids, nb, d_q, d_found))) return rc;
    KU_HIP(hipMemsetAsync(mark, 0, nb, s));
    uint64_t* rows = a.d_rows + pos * k;
    uint32_t* counts = a.d_counts ? a.d_counts + pos : nullptr;
    uint32_t size = a.window;
    for (uint64_t j0 = 0; j0 < n_new;) {
      uint32_t nw = vc_kgupd_window_records(j0, n_new, size);
      JoinArgs ja{};
      ja.q = d_q; ja.rows = rows; ja.counts = counts; ja.nb = nb; ja.k = k; ja.codes = d_new + j0 * W; ja.first_id = new_id + (uint32_t)j0;
      ja.cnt = cnt; ja.flag = flag; ja.blk = blk; ja.offs = offs; ja.stat = stat;
      unsigned long long home[2] = {0, 0};
      for (;;) {
        ja.nw = nw;
        KU_HIP(hipMemsetAsync(stat, 0, 16, s));
        KU_HIP(launch_join<false>(ja, W, s));
        // THE WAIT of the window: 16 bytes
        KU_HIP(hipMemcpyAsync(home, stat, 16, hipMemcpyDeviceToHost, s));
        KU_HIP(hipStreamSynchronize(s));
        ++st.n_windows;
        if (vc_kgupd_accept(home[0], a.budget, nw)) break;
        size = nw = vc_kgupd_halve(nw);
        ++st.n_halvings;
      }
      const uint64_t H = home[0], affected = home[1];
      if (affected > nb || H < affected || H > (uint64_t)nb * nw) {
        if (err) *err = "k-NN graph update: the counters of a window do not fit it";
        return VC_ERR_HIP;
      }
      st.n_hits += H;
      if (H) {
        KU_HIP(vc_exclusive_scan_u32(cnt, offs, nb, scan_work, s));
        KU_HIP(vc_exclusive_scan_u32(flag, rank, nb, scan_work, s));
        hipLaunchKernelGGL(vc_kgraph_list_kernel, dim3((nb + KU_BLK - 1) / KU_BLK), dim3(KU_BLK), 0, s, (const uint32_t*)flag, (const uint32_t*)rank, nb, list);
        KU_HIP(hipGetLastError());
        uint64_t* hits = (uint64_t*)v.alloc(VC_KGRAPH_UPD_HITS, (size_t)vc_kgupd_hits_bytes(H));
        uint64_t* out = (uint64_t*)v.alloc(VC_KGRAPH_UPD_ROWS, (size_t)vc_kgupd_merge_bytes(affected, a.budget, k));
        if (!hits || !out) return VC_ERR_NOMEM;
        ja.hits = hits;
        ja.n_hits = H;
        KU_HIP(launch_join<true>(ja, W, s));
        MergeArgs ma{};
        ma.rows = rows; ma.counts = counts; ma.nb = nb; ma.k = k; ma.list = list; ma.offs = offs; ma.cnt = cnt; ma.hits = hits; ma.n_hits = H;
        ma.out = out; ma.newcnt = newcnt; ma.mark = mark;
        const uint32_t sub = vc_kgupd_merge_sub(a.budget, k);
        for (uint64_t a0 = 0; a0 < affected; a0 += sub) {
          ma.a0 = (uint32_t)a0;
          ma.na = (uint32_t)std::min<uint64_t>(sub, affected - a0);
          hipLaunchKernelGGL(vc_kgraph_merge_kernel, dim3((ma.na + KU_BLK / VC_WAVE - 1) / (KU_BLK / VC_WAVE)), dim3(KU_BLK), 0, s, ma);
          KU_HIP(hipGetLastError());
          hipLaunchKernelGGL(vc_kgraph_copy_kernel, dim3(ku_grid((uint64_t)ma.na * k)), dim3(KU_BLK), 0, s, ma);
          KU_HIP(hipGetLastError());
        }
      }
      j0 += nw;
    }
    hipLaunchKernelGGL(vc_kgraph_marks_kernel, dim3(ku_grid(nb)), dim3(KU_BLK), 0, s, (const uint8_t*)mark, nb, stat + VC_KGUPD_ST_CHANGED);
    KU_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(vc_kgraph_inserted_kernel, dim3(ku_grid(n_old * k)), dim3(KU_BLK), 0, s, (const uint64_t*)a.d_rows, n_old * k, new_id, n_new,
                     stat + VC_KGUPD_ST_INSERTED);
  KU_HIP(hipGetLastError());
  // THE WAIT of the call: the statistics and the error word, 64 bytes
  unsigned long long home[VC_KGUPD_STAT_BYTES / 8] = {};
  KU_HIP(hipMemcpyAsync(home, stat, VC_KGUPD_STAT_BYTES, hipMemcpyDeviceToHost, s));
  KU_HIP(hipStreamSynchronize(s));
  if (home[VC_KGUPD_ST_BAD]) {
    if (err) *err = "k-NN graph update: an old count above k -- not a graph vc_knn_graph built for the first n_old records";
    return VC_ERR_INVALID;
  }
  st.n_rows_changed = home[VC_KGUPD_ST_CHANGED];
  st.n_inserted = home[VC_KGUPD_ST_INSERTED];
  if (stats) *stats = st;
  return VC_OK;
}

// The host form: the old rows and counts staged up (rows | counts, over all N records), `run` on them, all N rows and counts home; a
// new row the linear scan passed on is answered again as vc_knn_graph_run_host answers it.  Without counts the staged old counts are
// the uniform min(k, n_old - 1), so that the new rows' counts can still tell which rows were passed on.
int vc_knn_graph_update_run_host(const VcStoreView& v, const VcKgupdArgs& a, uint64_t* rows, uint32_t* counts, vc_knn_graph_update_stats* stats,
                                 const std::function<int(uint64_t* d_rows, uint32_t* d_counts, vc_knn_graph_update_stats* stats)>& run,
                                 const std::function<int(const uint64_t* codes, uint32_t nq, uint64_t* rows, uint32_t* counts)>& host_knn, hipStream_t s,
                                 std::string* err) {
  const size_t N = (size_t)v.n, n_old = (size_t)a.n_old, k = a.build.k, rbytes = N * k * 8, cbytes = N * 4;
  uint8_t* stage = (uint8_t*)v.alloc(VC_KGRAPH_UPD_STAGE, rbytes + cbytes);
  if (!stage) return VC_ERR_NOMEM;
  uint64_t* d_rows = (uint64_t*)stage;
  uint32_t* d_cnt = (uint32_t*)(stage + rbytes);
  std::vector<uint32_t> uniform;
  if (n_old) {
    if (!counts) uniform.assign(n_old, vc_kgraph_row_count(n_old, (uint32_t)k));
    KU_HIP(hipMemcpyAsync(d_rows, rows, n_old * k * 8, hipMemcpyHostToDevice, s));
    KU_HIP(hipMemcpyAsync(d_cnt, counts ? counts : uniform.data(), n_old * 4, hipMemcpyHostToDevice, s));
    KU_HIP(hipStreamSynchronize(s));   // (the uniform counts leave this scope)
  }
  vc_knn_graph_update_stats st{};
  int rc = run(d_rows, d_cnt, &st);
  if (rc) return rc;
  std::vector<uint32_t> own_cnt;
  uint32_t* cnt = counts;
  if (!cnt && st.build.n_gave_up) {
    own_cnt.resize(N);
    cnt = own_cnt.data();
  }
  KU_HIP(hipMemcpyAsync(rows, d_rows, rbytes, hipMemcpyDeviceToHost, s));
  if (cnt) KU_HIP(hipMemcpyAsync(cnt, d_cnt, cbytes, hipMemcpyDeviceToHost, s));
  KU_HIP(hipStreamSynchronize(s));
  if (st.build.n_gave_up && (rc = vc_knn_graph_answer_again_host(v, a.build, rows + n_old * k, cnt + n_old, host_knn, s, err))) return rc;
  if (stats) *stats = st;
  return VC_OK;
}
