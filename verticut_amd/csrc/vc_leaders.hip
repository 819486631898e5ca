// ============================================================================
// vc_leaders.hip -- greedy leader dedup on the device (vc_leaders_radius*, vc_sharded_leaders_radius*): the lexicographically first
// maximal independent set of the radius graph, decided batch by batch over the RAW result of the radius search underneath.  No
// compaction, no plan: one wave walks one query's segment between its two offsets; LDS holds only a block's two counter sums.
// ============================================================================
#include <algorithm>
#include <cstdio>

#include "vc_internal.hpp"

// THE RULE: record i is a LEADER iff no leader with a smaller id lies within the radius of it; a record that is none is DROPPED and
// labelled with its smallest leader neighbour.  Whether i leads depends on the records below i only, so the batches are taken in
// ascending id order and every record below a batch's first id is final when the batch starts: it leads iff labels[v] == v.
// A batch [first_id, first_id + nq) is decided in synchronous ROUNDS, numbered from 1, over one state word per query:
//   0                               undecided
//   round | LD_LEADER               decided in that round: a leader
//   round                           decided in that round: dropped by a leader of this batch
//   round | LD_PAST                 decided in round 1: dropped by a leader below the batch, labels[] already final
// A round R takes a neighbour's word as decided only when its round is below R, so a word stored during round R reads as
// "undecided" to the other waves of that round whether they see the old or the new value: every round works on the state the
// previous one left, whatever the order of the waves, and the number of rounds is a function of the data and the batch alone.
// Only entries with an id v below the query's own matter.  Round 1 (FIRST) also settles against the past -- an entry v below the
// batch whose record leads drops the query, the minimum of such v IS its label, every id below the batch being smaller than any
// inside -- counts the pairs and writes every state word, so no word of the scratch is read before it is written.
// THE EAGER RULE of a round, for an undecided query:
//   dropped  as soon as ONE neighbour v < own of the batch is a decided leader (sound: that leader is final, and greedy drops the
//            query on it whatever the still undecided neighbours turn out to be);
//   leader   when every neighbour v < own of the batch is decided and dropped, or there is none (and the past did not drop it);
//   else it stays undecided and is counted.
// By induction over the rounds every decision is the one the sequential pass makes, so the fixed point is unique.  The smallest
// undecided id has only decided smaller neighbours: every round decides it, and a batch ends after at most nq rounds.
// The label of a query dropped inside the batch is the minimum over ALL its leader neighbours, which the round that dropped it did
// not know (a smaller neighbour may have become a leader later): vc_leaders_assign_kernel takes it once, after the last round.
//   vc_leaders_round_kernel<FIRST>   one wave per query, the rule above; counts the undecided
//   vc_leaders_assign_kernel         one wave per query: the labels of the batch's leaders and of the queries dropped inside it
//   vc_leaders_count_kernel          the records with labels[i] == id_base + i
// Three counters und[round % 3] carry the undecided from round to round: round R adds to und[R % 3], has read und[(R - 1) % 3]
// and zeroes und[(R + 1) % 3].  A round that finds zero there returns before it touches an entry and leaves und[R % 3] at zero, so
// every round launched behind the fixed point is a no-op.  No thread waits for another block; rounds are separate launches.
// The round kernel runs blocks of 16 waves whose sums meet in LDS first: one global atomic per block and counter.  With one per
// wave, round 1's 2 x 4 096 adds to two addresses were most of its 48 us on a batch of 4 096 ids.
#define LD_BLK 256u                      // the assign and count kernels
#define LD_WAVES (LD_BLK / VC_WAVE)
#define LD_RBLK 1024u                    // the round kernel
#define LD_RWAVES (LD_RBLK / VC_WAVE)
#define LD_NONE 0xFFFFFFFFu     // "no leader seen", in POSITIONS (id - id_base, id - first_id): a neighbour's position is below the
                                // query's own, so it never reaches 2^32 - 1 -- ids themselves use all 32 bits
#define LD_LEADER 0x80000000u
#define LD_PAST 0x40000000u
#define LD_ROUND 0x3FFFFFFFu
static_assert(VC_LEADER_BATCH_MAX <= LD_ROUND, "a batch needs at most as many rounds as it has queries, and the round must fit the state word");

__device__ __forceinline__ void ld_st(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// stat: [0] pairs, [1] leaders, [2] rounds that had work.  labels is read below the batch and written inside it (round 1 only).
template <bool FIRST>
__global__ void __launch_bounds__(LD_RBLK) vc_leaders_round_kernel(const uint64_t* __restrict__ raw, const uint64_t* __restrict__ roffs, uint32_t nq,
                                                                  uint32_t first_id, uint32_t id_base, uint32_t* labels, uint32_t* state,
                                                                  unsigned long long* stat, uint32_t* und, uint32_t round) {
  const uint32_t lane = vc_lane();
  const bool head = blockIdx.x == 0 && threadIdx.x == 0;
  if (head) ld_st(und + (round + 1) % 3, 0u);
  if (!FIRST && vc_ld_relaxed(und + (round + 2) % 3) == 0) return;   // the fixed point has been reached: no pass over the entries
  if (head) atomicAdd(stat + 2, 1ull);
  __shared__ unsigned long long s_pairs;
  __shared__ uint32_t s_open;
  if (threadIdx.x == 0) {
    s_pairs = 0;
    s_open = 0;
  }
  __syncthreads();
  uint32_t open = 0;             // wave-uniform
  unsigned long long pairs = 0;  // wave-uniform
  for (uint32_t q = blockIdx.x * LD_RWAVES + threadIdx.x / VC_WAVE; q < nq; q += gridDim.x * LD_RWAVES) {   // (wave-uniform)
    if (!FIRST && vc_ld_relaxed(state + q) != 0) continue;
    const uint32_t own = first_id + q;
    const uint64_t beg = roffs[q], end = roffs[q + 1];
    uint32_t past = LD_NONE;
    bool blocked = false, dropped = false;
    for (uint64_t p0 = beg; p0 < end; p0 += VC_WAVE) {   // (wave-uniform bounds: every lane votes)
      const uint64_t p = p0 + lane;
      bool smaller = false;
      if (p < end) {
        const uint32_t v = (uint32_t)raw[p];
        smaller = v < own;
        if (smaller) {
          if (v < first_id) {
            if (FIRST && labels[v - id_base] == v) past = min(past, v - id_base);
          } else if (FIRST) {
            blocked = true;      // nothing in the batch is decided before round 1
          } else {
            const uint32_t s = vc_ld_relaxed(state + (v - first_id));
            if (s == 0 || (s & LD_ROUND) >= round) blocked = true;
            else if (s & LD_LEADER) dropped = true;
          }
        }
      }
      if (FIRST) pairs += (unsigned long long)__popcll(__ballot(smaller));
    }
    const bool any_dropped = __ballot(dropped) != 0, any_blocked = __ballot(blocked) != 0;
    uint32_t word = 0;
    if (FIRST) {
      past = vc_wave_min(past);
      if (past != LD_NONE) {
        word = round | LD_PAST;
        if (lane == 0) labels[own - id_base] = id_base + past;
      } else if (!any_blocked) {
        word = round | LD_LEADER;
      }
    } else if (any_dropped) {
      word = round;
    } else if (!any_blocked) {
      word = round | LD_LEADER;
    }
    if (word == 0) ++open;
    if (lane == 0 && (FIRST || word)) ld_st(state + q, word);
  }
  if (lane == 0) {
    if (open) atomicAdd(&s_open, open);
    if (FIRST && pairs) atomicAdd(&s_pairs, pairs);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_open) atomicAdd(und + round % 3, s_open);
    if (FIRST && s_pairs) atomicAdd(stat, s_pairs);
  }
}

// After the last round every word of the batch is decided.  A leader is labelled with itself, a query dropped inside the batch with
// the smallest leader among its neighbours v < own of the batch; the queries that the past dropped hold their label since round 1.
__global__ void __launch_bounds__(LD_BLK) vc_leaders_assign_kernel(const uint64_t* __restrict__ raw, const uint64_t* __restrict__ roffs, uint32_t nq,
                                                                   uint32_t first_id, uint32_t id_base, uint32_t* __restrict__ labels,
                                                                   const uint32_t* __restrict__ state) {
  const uint32_t lane = vc_lane();
  for (uint32_t q = blockIdx.x * LD_WAVES + threadIdx.x / VC_WAVE; q < nq; q += gridDim.x * LD_WAVES) {   // (wave-uniform)
    const uint32_t s = state[q], own = first_id + q;
    if (s == 0 || (s & LD_PAST)) continue;
    uint32_t best = LD_NONE;
    if (s & LD_LEADER) {
      best = q;
    } else {
      const uint64_t beg = roffs[q], end = roffs[q + 1];
      for (uint64_t p = beg + lane; p < end; p += VC_WAVE) {
        const uint32_t v = (uint32_t)raw[p];
        if (v < own && v >= first_id && (state[v - first_id] & LD_LEADER)) best = min(best, v - first_id);
      }
      best = vc_wave_min(best);
    }
    if (lane == 0 && best != LD_NONE) labels[own - id_base] = first_id + best;
  }
}

__global__ void __launch_bounds__(LD_BLK) vc_leaders_count_kernel(const uint32_t* __restrict__ labels, uint64_t n, uint32_t id_base,
                                                                  unsigned long long* __restrict__ n_leaders) {
  uint32_t leaders = 0;   // wave-uniform
  for (uint64_t i0 = (uint64_t)blockIdx.x * LD_BLK; i0 < n; i0 += (uint64_t)gridDim.x * LD_BLK) {   // (block-uniform bounds: every lane votes)
    const uint64_t i = i0 + threadIdx.x;
    leaders += (uint32_t)__popcll(__ballot(i < n && labels[i] == id_base + (uint32_t)i));
  }
  if (vc_lane() == 0 && leaders) atomicAdd(n_leaders, (unsigned long long)leaders);
}

static uint32_t ld_grid(uint64_t items, uint32_t per_block) {
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + per_block - 1) / per_block, 1), 256 * 8);
}

hipError_t vc_launch_leaders_count(const uint32_t* d_labels, uint64_t n, uint32_t id_base, uint64_t* d_n_leaders, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vc_leaders_count_kernel, dim3(ld_grid(n, LD_BLK)), dim3(LD_BLK), 0, s, d_labels, n, id_base, (unsigned long long*)d_n_leaders);
  return hipGetLastError();
}

hipError_t vc_leaders_decide_batch(const uint64_t* d_raw, const uint64_t* d_roffs, uint32_t nq, uint32_t first_id, uint32_t id_base, uint32_t* d_labels,
                                   uint32_t* d_state, uint64_t* d_stat, hipStream_t s, bool* stuck) {
  *stuck = false;
  if (nq == 0) return hipSuccess;
  hipError_t err;
  unsigned long long* stat = (unsigned long long*)d_stat;
  uint32_t* und = (uint32_t*)(d_stat + 3);
  const dim3 grid(ld_grid(nq, LD_RWAVES)), block(LD_RBLK), agrid(ld_grid(nq, LD_WAVES)), ablock(LD_BLK);
  if ((err = hipMemsetAsync(und, 0, 16, s)) != hipSuccess) return err;
  uint32_t round = 1;
  hipLaunchKernelGGL(vc_leaders_round_kernel<true>, grid, block, 0, s, d_raw, d_roffs, nq, first_id, id_base, d_labels, d_state, stat, und, round);
  if ((err = hipGetLastError()) != hipSuccess) return err;
  const auto launch_round = [&]() {
    ++round;
    hipLaunchKernelGGL(vc_leaders_round_kernel<false>, grid, block, 0, s, d_raw, d_roffs, nq, first_id, id_base, d_labels, d_state, stat, und, round);
    return hipGetLastError();
  };
  for (;;) {
    while (round % VC_LEADER_ROUND_GROUP && round < nq)   // (a batch needs at most nq rounds)
      if ((err = launch_round()) != hipSuccess) return err;
    uint32_t open = 0;
    if ((err = hipMemcpyAsync(&open, und + round % 3, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return err;
    if ((err = hipStreamSynchronize(s)) != hipSuccess) return err;
    if (open == 0) break;
    if (round >= nq) {
      *stuck = true;
      return hipSuccess;
    }
    if ((err = launch_round()) != hipSuccess) return err;
  }
  hipLaunchKernelGGL(vc_leaders_assign_kernel, agrid, ablock, 0, s, d_raw, d_roffs, nq, first_id, id_base, d_labels, d_state);
  return hipGetLastError();
}

int vc_leaders_run(const VcStoreView& v, uint32_t radius, uint32_t batch, uint64_t n_labelled, uint32_t* d_labels, vc_leader_stats* stats, hipStream_t s,
                   std::string* err) {
  const uint64_t N = v.n;
  batch = std::min(vc_walk_batch(batch), VC_LEADER_BATCH_MAX);
  uint64_t* d_stat = (uint64_t*)v.alloc(VC_WALK_STAT, VC_LEADER_STAT_BYTES);
  uint32_t* d_state = n_labelled < N ? (uint32_t*)v.alloc(VC_WALK_STATE, (size_t)std::min<uint64_t>(batch, N - n_labelled) * 4) : nullptr;
  if (!d_stat || (n_labelled < N && !d_state)) return VC_ERR_NOMEM;
  VC_WALK_HIP(hipMemsetAsync(d_stat, 0, VC_LEADER_STAT_BYTES, s));
  const int rc = vc_walk_run(v, n_labelled, batch, radius, [&](const VcWalkBatch& b) -> int {   // the decision over the raw result as it lies
    bool stuck = false;
    VC_WALK_HIP(vc_leaders_decide_batch(b.d_raw, b.d_roffs, b.nq, b.first_id, v.id_base, d_labels, d_state, d_stat, s, &stuck));
    if (!stuck) return VC_OK;
    char text[96];
    snprintf(text, sizeof text, "leaders: the batch at id %u is undecided after %u rounds", b.first_id, b.nq);
    if (err) *err = text;
    return VC_ERR_HIP;
  }, s, err);
  if (rc) return rc;
  VC_WALK_HIP(vc_launch_leaders_count(d_labels, N, v.id_base, d_stat + 1, s));
  uint64_t st[3] = {0, 0, 0};
  VC_WALK_HIP(hipMemcpyAsync(st, d_stat, 24, hipMemcpyDeviceToHost, s));
  VC_WALK_HIP(hipStreamSynchronize(s));
  if (stats) *stats = vc_leader_stats{st[0], st[1], st[2]};
  return VC_OK;
}

int vc_leaders_run_host(const VcStoreView& v, uint32_t radius, uint32_t batch, uint64_t n_labelled, uint32_t* labels, vc_leader_stats* stats, hipStream_t s,
                        std::string* err) {
  uint32_t* d_labels = nullptr;
  int rc = vc_walk_stage_labels(v, labels, 1, n_labelled, &d_labels, s, err);
  if (rc || (rc = vc_leaders_run(v, radius, batch, n_labelled, d_labels, stats, s, err))) return rc;
  if (n_labelled < v.n)   // the incoming entries are read only: they do not travel back
    VC_WALK_HIP(hipMemcpyAsync(labels + n_labelled, d_labels + n_labelled, (size_t)(v.n - n_labelled) * 4, hipMemcpyDeviceToHost, s));
  VC_WALK_HIP(hipStreamSynchronize(s));
  return VC_OK;
}
