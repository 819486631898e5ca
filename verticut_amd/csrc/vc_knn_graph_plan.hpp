// Plan arithmetic of vc_knn_graph* and vc_cluster_knn* (vc_knn_graph.hip): the range of a call, the k' schedule of the rounds, the
// verdict on a row, the cut of a round into sub-batches, the scratch layout and the buffer bytes.  Plain C++ with no HIP in it, so
// that tests/cpp/knn_graph_plan_test.cc checks it on the CPU; the kernels and the driver call exactly these functions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VC_KG_FN __host__ __device__ inline
#else
#define VC_KG_FN inline
#endif

#define VC_KGRAPH_MAX_K 8192u                       // = VC_MAX_K: the widest row the search underneath returns
#define VC_KGRAPH_SCRATCH_DEFAULT (64ull << 20)     // bytes of k' rows per sub-batch (VC_KGRAPH_SCRATCH)
#define VC_KGRAPH_BATCH_DEFAULT 4096u               // = VC_CLUSTER_BATCH: ids per batch when the caller passes batch = 0

// ---- the arguments ------------------------------------------------------------------------------------------------------------------
VC_KG_FN bool vc_kgraph_k_ok(uint32_t k) { return k >= 1 && k <= VC_KGRAPH_MAX_K - 1; }   // k + 1 entries must fit a row
VC_KG_FN bool vc_kgraph_k_first_ok(uint32_t k, uint32_t k_first) {                       // k already checked
  return k_first == 0 || (k_first >= k + 1 && k_first <= VC_KGRAPH_MAX_K);
}
VC_KG_FN uint32_t vc_kgraph_batch(uint32_t batch) { return batch ? batch : VC_KGRAPH_BATCH_DEFAULT; }
// the positions of a call: [first, first + count), count == 0 meaning "to the end".  false: the range leaves the store
VC_KG_FN bool vc_kgraph_range(uint64_t n, uint64_t first, uint64_t count, uint64_t* rows) {
  if (first > n || count > n - first) return false;
  *rows = count ? count : n - first;
  return true;
}
// what every row of a store of n records holds
VC_KG_FN uint32_t vc_kgraph_row_count(uint64_t n, uint32_t k) { return n == 0 ? 0u : (n - 1 < k ? (uint32_t)(n - 1) : k); }

// ---- the schedule: LINEAR one round at k + 1; exact MIH k'_0 = k_first, or min(VC_MAX_K, 2 (k + 1)); k'_{j+1} = min(VC_MAX_K, 2 k'_j) ----
VC_KG_FN uint32_t vc_kgraph_next_k(uint32_t kp) { return kp >= VC_KGRAPH_MAX_K / 2 ? VC_KGRAPH_MAX_K : 2 * kp; }
VC_KG_FN uint32_t vc_kgraph_first_k(uint32_t k, uint32_t k_first, bool linear) {
  return linear ? k + 1 : k_first ? k_first : vc_kgraph_next_k(k + 1);
}

// ---- the verdict on a row of the search at k': cnt its count word, and of its entries (the first min(cnt, k'), ascending)
// `present` says whether the own record (0, own id) is among them and `below` how many lie below the distance of the last one -------
enum { VC_KGRAPH_SETTLED = 0, VC_KGRAPH_RETRY = 1, VC_KGRAPH_PASSED = 2 };
// entries of a row that are there to be read
VC_KG_FN uint32_t vc_kgraph_row_entries(uint32_t cnt, uint32_t kp) { return cnt < kp ? cnt : kp; }
// THE SURE PREFIX (tie_cut: the rows are exact MIH's).  A row that is not full holds the whole store.  A full row of exact MIH holds
// every record nearer than its last distance D, but of the records that tie at D only some: it is settled iff k entries other than
// the own record lie below D.  A count above k' or of UINT32_MAX is a full row nobody vouches for.  Without tie_cut (the linear scan)
// a full row is the k' smallest (dist, id) and settled; its UINT32_MAX count -- the ring-overflow recovery gave up -- is passed on.
VC_KG_FN int vc_kgraph_verdict(bool tie_cut, uint32_t cnt, uint32_t kp, uint32_t k, bool present, uint32_t below) {
  if (!tie_cut) return cnt == 0xFFFFFFFFu ? VC_KGRAPH_PASSED : VC_KGRAPH_SETTLED;
  if (cnt < kp) return VC_KGRAPH_SETTLED;
  if (cnt > kp) return VC_KGRAPH_RETRY;
  const uint32_t others = below - (present && below ? 1u : 0u);   // (the own record is at distance 0: below D whenever anything is)
  return others >= k ? VC_KGRAPH_SETTLED : VC_KGRAPH_RETRY;
}
// the count word of a settled row with m entries of which `present` is the own record
VC_KG_FN uint32_t vc_kgraph_count(uint32_t m, bool present, uint32_t k) {
  const uint32_t left = m - (present ? 1u : 0u);
  return left < k ? left : k;
}

// ---- sub-batches: the k' rows of a round hold at most `budget` bytes, but always one row ---------------------------------------------
VC_KG_FN uint32_t vc_kgraph_sub_batch(uint64_t budget, uint32_t kp) {
  const uint64_t b = budget / (8ull * kp);
  return b < 1 ? 1u : b > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)b;
}
VC_KG_FN uint64_t vc_kgraph_rows_bytes(uint32_t n, uint64_t budget, uint32_t kp) {
  const uint32_t b = vc_kgraph_sub_batch(budget, kp);
  return 8ull * kp * (n < b ? n : b);
}

// ---- the scratch of a call beside the rows, for batches of at most nq ids of W words, in bytes: the tally (rows passed on) | the
// length of the retry list | flag [nq] | scanned [nq] | the scan's work (scan_words words) | two index maps [nq] | counts of a
// sub-batch [nq] | the batch's ids [nq] | found [nq] | the batch's codes [nq][W] | the retry codes [nq][W].  Every word is written
// before it is read: the tally by the memset at the start, flag by every settle launch, scanned and the work by the scan, a map, the
// retry codes and the length by the gather of the round before, the ids by the init launch, found and the codes by the store's gather.
struct VcKgraphWork {
  uint64_t tally, n_next, flag, scanned, scan_work, map[2], cnt, ids, found, q, q_next, total;
  VcKgraphWork(uint32_t nq, uint32_t W, uint64_t scan_words) {
    const uint64_t row4 = ((uint64_t)nq * 4 + 7) & ~7ull;
    uint64_t o = 0;
    tally = o;      o += 8;
    n_next = o;     o += 8;
    flag = o;       o += row4;
    scanned = o;    o += row4;
    scan_work = o;  o += (scan_words * 4 + 7) & ~7ull;
    map[0] = o;     o += row4;
    map[1] = o;     o += row4;
    cnt = o;        o += row4;
    ids = o;        o += row4;
    found = o;      o += row4;
    q = o;          o += (uint64_t)nq * W * 8;
    q_next = o;     o += (uint64_t)nq * W * 8;
    total = o;
  }
};

// ---- vc_cluster_knn*: the device's statistics block, 32 bytes: edges | mutual pairs | clusters | the largest in-degree, the error word ----
#define VC_KGRAPH_STAT_BYTES 32u
// entries of row j that are edges before the cap: the first min(kk, count_j)
VC_KG_FN uint32_t vc_kgraph_edge_entries(uint32_t kk, uint32_t cnt) { return cnt < kk ? cnt : kk; }
// THE ONE COMPARE.  Row j is the min(k, N - 1) smallest packed (dist << 32 | id) over the records other than j, and the distance is
// symmetric: record i at distance d is among row j's first m entries iff (d << 32 | i) <= row_j[m - 1].
VC_KG_FN bool vc_kgraph_lists(uint64_t last_of_j, uint32_t d, uint32_t id_i) { return (((uint64_t)d << 32) | id_i) <= last_of_j; }
