// One result per label group in k-NN search: vc_search_knn_distinct* and vc_sharded_search_knn_distinct* (the header states the contract).
//
// THE COLLAPSE.  A row of k' ascending entries of the search underneath keeps an entry iff no earlier entry of the row has its label.
//   k' <= 64    vc_distinct_wave_kernel: one wave per query, entry j in lane j, the earlier lanes' labels come by readlane; the kept
//               entries are placed by a ballot.  No LDS.
//   k' <= 8192  vc_distinct_table_kernel<T>: one block per query (T = 256 threads up to k' = 1024, 1024 above), the labels of the row
//               in LDS next to a first-occurrence table of 2 P slots (P = the power of two >= k').  A slot holds a ROW POSITION, never a
//               label, so no label value is reserved: an entry claims the first free slot of its label's probe chain (atomicCAS on
//               the empty marker, a position no row has) or, where the slot's position carries its own label, lowers it (atomicMin).
//               A slot's label never changes once claimed, so every entry of a label ends at the same slot and that slot ends up
//               with the label's smallest position, whatever the order the lanes ran in.  An entry is kept iff its slot names it.
//               The kept entries are placed tile by tile by ballot + the block's wave sums.  12 P bytes of dynamic LDS: 96 KiB at
//               k' = 8192, hence the attribute in launch_collapse.
// Under exact MIH a full row is sure only below its last distance (vc_distinct_sure_below): the entries at that distance do not count.
// Both write the row, its labels and its count through the index map (compact row -> the caller's query) when the verdict of
// vc_distinct_plan.hpp is final, and flag[row] = 1 when the query goes to the next round.  The two statistics counters are sums, so
// the order of the atomics does not matter; the retry list is the exclusive scan of the flags (vc_sort.hip), so it is ascending.
#include <algorithm>

#include "vc_distinct_plan.hpp"
#include "vc_internal.hpp"

static_assert(VC_DISTINCT_MAX_K == VC_MAX_K, "the plan's widest row is the search's");
static_assert(VC_DISTINCT_TRUNCATED_BIT == VC_DISTINCT_TRUNCATED, "the plan's flag is the header's");

namespace {

constexpr uint32_t kEmpty = 0xFFFFFFFFu;   // a slot nobody claimed: positions are < 8192

// what a collapse launch works on; flag, map and the row pointers are those of the sub-batch
struct CollapseArgs {
  const uint64_t* rows;      // [n][kp]
  const uint32_t* cnt;       // [n]
  uint32_t n, kp, k;
  uint32_t tie_cut;          // exact MIH underneath: only the sure prefix of a full row counts (vc_distinct_sure_below)
  const uint32_t* labels;    // [n_labels], indexed by id - id_base
  uint64_t n_labels;
  uint32_t id_base;
  const uint32_t* map;       // [n] compact row -> the caller's query; null: first + row
  uint32_t first;
  uint64_t* out;             // [nq][k]
  uint32_t* row_labels;      // [nq][k], nullable
  uint32_t* counts;          // [nq], nullable
  uint32_t* flag;            // [n]
  unsigned long long* tally; // [0] += truncated, [1] += short
};

// the distance the entries of a row must stay below to count (0xFFFFFFFF: all of them do)
__device__ __forceinline__ uint32_t sure_below(const CollapseArgs& a, uint64_t row, uint32_t cnt) {
  const uint32_t last = a.tie_cut && cnt == a.kp ? (uint32_t)(a.rows[row * a.kp + a.kp - 1] >> 32) : 0u;
  return vc_distinct_sure_below(a.tie_cut != 0, cnt, a.kp, last);
}

// entry j of a row: its packed value, whether it is a result whose label can be read, and the label
struct Entry {
  uint64_t v;
  uint32_t label;
  bool valid;
};
__device__ __forceinline__ Entry load_entry(const CollapseArgs& a, uint64_t row, uint32_t j, uint32_t m, uint32_t below) {
  Entry e{VC_PACK_INF, 0u, false};
  if (j < m) {
    e.v = a.rows[row * a.kp + j];
    const uint32_t i = (uint32_t)e.v - a.id_base;
    e.valid = (uint32_t)(e.v >> 32) < below && i < a.n_labels;   // (an empty entry is at distance 0xFFFFFFFF)
    if (e.valid) e.label = a.labels[i];
  }
  return e;
}

// the verdict's words, by one thread of the query
__device__ __forceinline__ void write_verdict(const CollapseArgs& a, uint32_t row, uint32_t oq, const VcDistinctVerdict& vd) {
  a.flag[row] = vd.status == VC_DISTINCT_RETRY ? 1u : 0u;
  if (vd.status == VC_DISTINCT_RETRY) return;
  if (a.counts) a.counts[oq] = vd.count;
  if (vd.status == VC_DISTINCT_CUT) atomicAdd(a.tally, 1ull);
  if (vd.status == VC_DISTINCT_SHORT) atomicAdd(a.tally + 1, 1ull);
}

__global__ void __launch_bounds__(64 * VC_DISTINCT_WAVES_PER_BLOCK) vc_distinct_wave_kernel(const CollapseArgs a) {
  const uint32_t row = blockIdx.x * VC_DISTINCT_WAVES_PER_BLOCK + threadIdx.x / VC_WAVE;   // wave-uniform
  if (row >= a.n) return;
  const uint32_t lane = vc_lane();
  const uint32_t cnt = a.cnt[row], m = vc_distinct_row_entries(cnt, a.kp);
  const Entry e = load_entry(a, row, lane, m, sure_below(a, row, cnt));
  bool dup = false;
  for (uint32_t i = 0; i + 1 < m; ++i) {   // (m <= 64; the last entry is nobody's predecessor)
    const uint32_t li = (uint32_t)__builtin_amdgcn_readlane((int)e.label, (int)i);
    const uint32_t vi = (uint32_t)__builtin_amdgcn_readlane((int)e.valid, (int)i);
    dup = dup || (i < lane && vi && li == e.label);
  }
  const bool kept = e.valid && !dup;
  const unsigned long long mask = __ballot(kept);
  const uint32_t pos = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)), d = (uint32_t)__popcll(mask);
  const uint32_t oq = a.map ? a.map[row] : a.first + row;
  const VcDistinctVerdict vd = vc_distinct_verdict(d, cnt, a.kp, a.k);
  if (lane == 0) write_verdict(a, row, oq, vd);
  if (vd.status == VC_DISTINCT_RETRY) return;
  uint64_t* out = a.out + (uint64_t)oq * a.k;
  uint32_t* rl = a.row_labels ? a.row_labels + (uint64_t)oq * a.k : nullptr;
  if (kept && pos < vd.written) {
    out[pos] = e.v;
    if (rl) rl[pos] = e.label;
  }
  for (uint32_t j = vd.written + lane; j < a.k; j += VC_WAVE) {
    out[j] = VC_PACK_INF;
    if (rl) rl[j] = 0u;
  }
}

template <int T>
__global__ void __launch_bounds__(T) vc_distinct_table_kernel(const CollapseArgs a, const uint32_t P) {
  extern __shared__ uint32_t lds[];          // labels [P] | slots [2 P]
  __shared__ uint32_t wsum[T / VC_WAVE];
  uint32_t* lab = lds;
  uint32_t* slot = lds + P;
  const uint32_t S = 2 * P, t = threadIdx.x, lane = vc_lane(), wave = t / VC_WAVE;
  const uint32_t row = blockIdx.x;
  const uint32_t cnt = a.cnt[row], m = vc_distinct_row_entries(cnt, a.kp);
  const uint32_t tiles = (m + T - 1) / T;    // <= 8: entry tile * T + t is this thread's in tile `tile`
  const uint32_t below = sure_below(a, row, cnt);
  for (uint32_t i = t; i < S; i += T) slot[i] = kEmpty;
  uint32_t vmask = 0;                        // bit `tile`: this thread's entry of the tile is valid
  for (uint32_t tile = 0; tile < tiles; ++tile) {
    const uint32_t j = tile * T + t;
    const Entry e = load_entry(a, row, j, m, below);
    if (j < m) lab[j] = e.label;
    vmask |= (e.valid ? 1u : 0u) << tile;
  }
  __syncthreads();
  // claim or lower: afterwards the slot of a label holds the smallest position that carries it
  for (uint32_t tile = 0; tile < tiles; ++tile) {
    if (!((vmask >> tile) & 1u)) continue;
    const uint32_t j = tile * T + t, mine = lab[j];
    for (uint32_t h = vc_distinct_hash(mine, S);; h = (h + 1) & (S - 1)) {
      const uint32_t old = atomicCAS(&slot[h], kEmpty, j);
      if (old == kEmpty) break;
      if (lab[old] == mine) {
        atomicMin(&slot[h], j);
        break;
      }
    }
  }
  __syncthreads();
  // place the kept entries in order, a tile at a time
  const uint32_t oq = a.map ? a.map[row] : a.first + row;
  uint64_t* out = a.out + (uint64_t)oq * a.k;
  uint32_t* rl = a.row_labels ? a.row_labels + (uint64_t)oq * a.k : nullptr;
  uint32_t base = 0;                         // block-uniform
  for (uint32_t tile = 0; tile < tiles && base < a.k; ++tile) {
    const uint32_t j = tile * T + t;
    bool kept = false;
    uint32_t mine = 0;
    if ((vmask >> tile) & 1u) {
      mine = lab[j];
      uint32_t h = vc_distinct_hash(mine, S), p = slot[h];
      while (p != kEmpty && lab[p] != mine) {   // (the chain up to the label's slot is all claimed: kEmpty never shows)
        h = (h + 1) & (S - 1);
        p = slot[h];
      }
      kept = p == j;
    }
    const unsigned long long mask = __ballot(kept);
    if (lane == 0) wsum[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t w = 0; w < T / VC_WAVE; ++w) {
      const uint32_t c = wsum[w];
      before += w < wave ? c : 0u;
      total += c;
    }
    const uint32_t pos = base + before + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (kept && pos < a.k) {
      out[pos] = a.rows[(uint64_t)row * a.kp + j];
      if (rl) rl[pos] = mine;
    }
    base += total;
    __syncthreads();
  }
  const VcDistinctVerdict vd = vc_distinct_verdict(base, cnt, a.kp, a.k);   // (base >= k wherever the loop ended early)
  if (t == 0) write_verdict(a, row, oq, vd);
  if (vd.status == VC_DISTINCT_RETRY) return;   // (what the tiles wrote is overwritten by the round that finishes the query)
  for (uint32_t j = vd.written + t; j < a.k; j += T) {
    out[j] = VC_PACK_INF;
    if (rl) rl[j] = 0u;
  }
}

// the retry list of a round: row r with flag[r] goes to place scanned[r]; its query's code is gathered from the caller's batch.
// The last thread leaves the length of the list in *n_next.
__global__ void __launch_bounds__(256) vc_distinct_gather_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ scanned, uint32_t n,
                                                                 const uint32_t* __restrict__ map, const uint64_t* __restrict__ queries, uint32_t W,
                                                                 uint32_t* __restrict__ map_next, uint64_t* __restrict__ q_next, uint32_t* __restrict__ n_next) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const uint32_t f = flag[r], at = scanned[r];
  if (r == n - 1) *n_next = at + f;
  if (!f) return;
  const uint32_t oq = map ? map[r] : r;
  map_next[at] = oq;
  for (uint32_t w = 0; w < W; ++w) q_next[(uint64_t)at * W + w] = queries[(uint64_t)oq * W + w];
}

// N == 0: padded rows, zero labels and counts
__global__ void __launch_bounds__(256) vc_distinct_empty_kernel(uint64_t* __restrict__ out, uint32_t* __restrict__ row_labels, uint32_t* __restrict__ counts,
                                                                uint32_t nq, uint32_t k) {
  const uint64_t total = (uint64_t)nq * k;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
    out[i] = VC_PACK_INF;
    if (row_labels) row_labels[i] = 0u;
    if (counts && i < nq) counts[i] = 0u;
  }
}

int distinct_fail(std::string* err, hipError_t r, const char* what) {
  if (err) *err = std::string("distinct: ") + what + ": " + hipGetErrorString(r);
  return r == hipErrorOutOfMemory ? VC_ERR_NOMEM : VC_ERR_HIP;
}
#define DISTINCT_HIP(call)                                       \
  do {                                                           \
    hipError_t _r = (call);                                      \
    if (_r != hipSuccess) return distinct_fail(err, _r, #call);  \
  } while (0)

hipError_t launch_collapse(const CollapseArgs& a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  if (a.kp == 0 || a.kp > VC_MAX_K || a.k == 0 || a.k > a.kp) return hipErrorInvalidValue;
  const uint32_t grid = vc_distinct_grid(a.kp, a.n), lds = vc_distinct_lds_bytes(a.kp), P = vc_distinct_positions(a.kp);
  switch (vc_distinct_class(a.kp)) {
    case VC_DISTINCT_WAVE:
      hipLaunchKernelGGL(vc_distinct_wave_kernel, dim3(grid), dim3(VC_WAVE * VC_DISTINCT_WAVES_PER_BLOCK), 0, s, a);
      break;
    case VC_DISTINCT_BLOCK:
      hipLaunchKernelGGL(vc_distinct_table_kernel<256>, dim3(grid), dim3(256), lds, s, a, P);
      break;
    default: {
      if (lds > (64u << 10)) {   // above 64 KiB the dynamic LDS of a kernel has to be granted first
        const hipError_t r = hipFuncSetAttribute((const void*)vc_distinct_table_kernel<1024>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (r != hipSuccess) return r;
      }
      hipLaunchKernelGGL(vc_distinct_table_kernel<1024>, dim3(grid), dim3(1024), lds, s, a, P);
    }
  }
  return hipGetLastError();
}

// the scratch of a call beside the rows, in bytes: the two tally words | the length of the retry list | flag [nq] | scanned [nq] |
// the scan's work | two index maps [nq] | counts of a sub-batch [nq] | the retry queries [nq][W].  Every word is written before it
// is read: the tally by the memset at the start, flag by every collapse launch, scanned and the work by the scan, the next map, the
// retry queries and the length by the gather.
struct DistinctWork {
  uint64_t tally, n_next, flag, scanned, scan_work, map[2], cnt, q, total;
  DistinctWork(uint32_t nq, uint32_t W) {
    const uint64_t row4 = ((uint64_t)nq * 4 + 7) & ~7ull;
    uint64_t o = 0;
    tally = o;      o += 16;
    n_next = o;     o += 8;
    flag = o;       o += row4;
    scanned = o;    o += row4;
    scan_work = o;  o += (vc_scan_work_words(nq) * 4 + 7) & ~7ull;
    map[0] = o;     o += row4;
    map[1] = o;     o += row4;
    cnt = o;        o += row4;
    q = o;          o += (uint64_t)nq * W * 8;
    total = o;
  }
};

}  // namespace

// THE ROUNDS (the header states the rule).  Per round: the search underneath and the collapse, sub-batch by sub-batch; then, unless
// no query can be left, the scan of the flags and the gather; then the one wait, for the length of the retry list and the tally.
int vc_distinct_run(const VcDistinctArgs& a, const VcKnnSearch& search, vc_distinct_stats* stats, hipStream_t s, std::string* err) {
  if (stats) *stats = vc_distinct_stats{};
  if (a.n_labels == 0) {
    const uint64_t total = (uint64_t)a.nq * a.k;
    hipLaunchKernelGGL(vc_distinct_empty_kernel, dim3((uint32_t)std::min<uint64_t>((total + 255) / 256, 4096)), dim3(256), 0, s, a.d_out, a.d_row_labels,
                       a.d_counts, a.nq, a.k);
    DISTINCT_HIP(hipGetLastError());
    return VC_OK;
  }
  const DistinctWork wp(a.nq, a.W);
  uint8_t* work = (uint8_t*)a.alloc(VC_DISTINCT_WORK, wp.total);
  if (!work) return VC_ERR_NOMEM;
  unsigned long long* tally = (unsigned long long*)(work + wp.tally);
  uint32_t* n_next = (uint32_t*)(work + wp.n_next);
  uint32_t* flag = (uint32_t*)(work + wp.flag);
  uint32_t* scanned = (uint32_t*)(work + wp.scanned);
  uint32_t* scan_work = (uint32_t*)(work + wp.scan_work);
  uint32_t* maps[2] = {(uint32_t*)(work + wp.map[0]), (uint32_t*)(work + wp.map[1])};
  uint32_t* cnt = (uint32_t*)(work + wp.cnt);
  uint64_t* q_next = (uint64_t*)(work + wp.q);
  DISTINCT_HIP(hipMemsetAsync(work, 0, 24, s));   // the tally and the length

  vc_distinct_stats st{};
  const uint64_t* q = a.d_queries;   // round 0: the caller's batch, identity map
  const uint32_t* map = nullptr;
  uint32_t n = a.nq, kp = vc_distinct_first_k(a.k, a.k_first);
  struct { uint32_t n_next, pad; unsigned long long tally[2]; } home{};
  for (uint32_t round = 0;; ++round) {
    const uint32_t batch = vc_distinct_batch(a.budget, kp);
    uint64_t* rows = (uint64_t*)a.alloc(VC_DISTINCT_ROWS, vc_distinct_rows_bytes(n, a.budget, kp));
    if (!rows) return VC_ERR_NOMEM;
    for (uint32_t first = 0; first < n; first += batch) {
      const uint32_t nb = std::min(batch, n - first);
      const int rc = search(q + (uint64_t)first * a.W, nb, kp, rows, cnt, nullptr);
      if (rc) return rc;
      CollapseArgs c{};
      c.rows = rows; c.cnt = cnt; c.n = nb; c.kp = kp; c.k = a.k; c.tie_cut = a.tie_cut ? 1u : 0u;
      c.labels = a.d_labels; c.n_labels = a.n_labels; c.id_base = a.id_base;
      c.map = map ? map + first : nullptr; c.first = first;
      c.out = a.d_out; c.row_labels = a.d_row_labels; c.counts = a.d_counts;
      c.flag = flag + first; c.tally = tally;
      DISTINCT_HIP(launch_collapse(c, s));
    }
    st.n_rounds = round + 1;
    st.k_last = kp;
    st.n_searched += n;
    const bool may_retry = kp < VC_MAX_K;   // at the widest row every verdict is final
    if (may_retry) {
      DISTINCT_HIP(vc_exclusive_scan_u32(flag, scanned, n, scan_work, s));
      hipLaunchKernelGGL(vc_distinct_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const uint32_t*)flag, (const uint32_t*)scanned, n, map, a.d_queries,
                         a.W, maps[round & 1], q_next, n_next);
      DISTINCT_HIP(hipGetLastError());
    }
    // THE WAIT of the round: 24 bytes
    DISTINCT_HIP(hipMemcpyAsync(&home.tally[0], tally, 16, hipMemcpyDeviceToHost, s));
    if (may_retry) DISTINCT_HIP(hipMemcpyAsync(&home.n_next, n_next, 4, hipMemcpyDeviceToHost, s));
    DISTINCT_HIP(hipStreamSynchronize(s));
    const uint32_t left = may_retry ? home.n_next : 0u;
    if (left > n) {
      if (err) *err = "distinct: the retry list is longer than the round";
      return VC_ERR_HIP;
    }
    if (left == 0) break;
    // the gather read the caller's queries through the old map and wrote q_next and the other map: the next round reads those
    q = q_next;
    map = maps[round & 1];
    n = left;
    kp = vc_distinct_next_k(kp);
  }
  st.n_truncated = home.tally[0];
  st.n_short = home.tally[1];
  if (stats) *stats = st;
  return VC_OK;
}

int vc_distinct_run_host(const VcDistinctHostArgs& a, const std::function<int(const uint64_t* d_queries, const uint32_t* d_labels, uint64_t* d_out,
                                                                            uint32_t* d_row_labels, uint32_t* d_counts, vc_distinct_stats* stats)>& run,
                         hipStream_t s, std::string* err) {
  const size_t qbytes = (size_t)a.nq * a.W * 8, lbytes = ((size_t)a.n_labels * 4 + 7) & ~(size_t)7, obytes = (size_t)a.nq * a.k * 8;
  const size_t rbytes = (size_t)a.nq * a.k * 4, cbytes = (size_t)a.nq * 4;   // staged: queries | out | labels | row labels | counts
  uint8_t* stage = (uint8_t*)a.alloc(VC_DISTINCT_STAGE, qbytes + obytes + lbytes + rbytes + cbytes);
  if (!stage) return VC_ERR_NOMEM;
  uint64_t* d_q = (uint64_t*)stage;
  uint64_t* d_out = (uint64_t*)(stage + qbytes);
  uint32_t* d_labels = (uint32_t*)(stage + qbytes + obytes);
  uint32_t* d_rl = (uint32_t*)(stage + qbytes + obytes + lbytes);
  uint32_t* d_cnt = (uint32_t*)(stage + qbytes + obytes + lbytes + rbytes);
  DISTINCT_HIP(hipMemcpyAsync(d_q, a.queries, qbytes, hipMemcpyHostToDevice, s));
  if (a.n_labels) DISTINCT_HIP(hipMemcpyAsync(d_labels, a.labels, (size_t)a.n_labels * 4, hipMemcpyHostToDevice, s));
  const int rc = run(d_q, d_labels, d_out, d_rl, d_cnt, a.stats);
  if (rc) return rc;
  std::vector<uint32_t> cnt(a.nq), rl;
  DISTINCT_HIP(hipMemcpyAsync(a.out, d_out, obytes, hipMemcpyDeviceToHost, s));
  DISTINCT_HIP(hipMemcpyAsync(cnt.data(), d_cnt, cbytes, hipMemcpyDeviceToHost, s));
  if (a.row_labels) DISTINCT_HIP(hipMemcpyAsync(a.row_labels, d_rl, rbytes, hipMemcpyDeviceToHost, s));
  DISTINCT_HIP(hipStreamSynchronize(s));
  for (uint32_t i = 0; i < a.nq; ++i) {
    if (a.order == VC_ORDER_FARTHEST_FIRST) {
      uint64_t* row = a.out + (size_t)i * a.k;
      // the valid part: the count without its flag; a passed-on row (UINT32_MAX) has what is not padding
      uint32_t valid = cnt[i] == 0xFFFFFFFFu ? (uint32_t)(std::find(row, row + a.k, VC_PACK_INF) - row) : std::min(cnt[i] & ~VC_DISTINCT_TRUNCATED, a.k);
      std::reverse(row, row + valid);
      if (a.row_labels) std::reverse(a.row_labels + (size_t)i * a.k, a.row_labels + (size_t)i * a.k + valid);
    }
    if (a.counts) a.counts[i] = cnt[i];
  }
  return VC_OK;
}
