// ============================================================================
// vc_vote.hip -- the weighted label tally of a segment with a strict tie rule, and the two calls built on it: the k-NN classifier over
// any rows (vc_knn_vote*, vc_sharded_knn_vote*) and synchronous label propagation over a CSR graph (vc_label_propagate*,
// vc_sharded_label_propagate*); the header states the contract.  One driver per call for both handle kinds over a VcStoreView; the
// plan arithmetic -- the weight, the winner key, the team shapes, the table sizes, the bins -- is vc_vote_plan.hpp.
// ONE tally routine (vote_open, vote_entry, vote_finish) serves two views: rows of stride k with a count and a cap, and CSR offsets
// with a list of the records of one degree bin.  Three shapes by the segment's length:
//   vc_vote_team_kernel<P>     up to 64 entries: P lanes a segment, 64 / P segments a wave, no LDS and no atomics.  A lane holds its
//                              entry's label and weight; `length` broadcast steps give it the tally of its label and whether an earlier
//                              lane carries it; first-occurrence lanes form the key and a butterfly max within the team picks the winner
//   vc_vote_table_kernel<T>    65 .. 8192 entries: a wave (up to 256 entries) or a block a segment, an open-addressing table of
//                              (label, tally) slots in dynamic LDS, pow2 >= 2 length slots (atomicCAS on the label, integer atomicAdd
//                              on the tally); a second walk in order looks every entry's tally up and max-reduces the key, which picks
//                              the earliest entry of the best label by itself; a walk over the slots counts the labels at the top tally
//   vc_vote_long_*_kernel      above 8192 entries (CSR hubs): the same three walks by VC_VOTE_LONG_BLOCKS blocks a segment over a table
//                              in the handle's scratch, a 64-bit atomicMax and an atomicAdd per wave and segment, and a finish launch;
//                              no limit but the 32-bit tally
// The propagate plan (vc_vote_plan_*_kernel): offsets and entries validated, a block's records counted per bin, ONE exclusive scan of
// counts[bin][block] places every (bin, block) in the list of records -- no atomic cursor --, the long segments' tables laid out, one
// wait.  Then a round is one launch per non-empty bin and one 64-byte read-back.  Statistics are ballot sums kept in registers over a
// grid-stride loop: one atomic per counter and wave (block) at the end.
// ============================================================================
#include <algorithm>

#include "vc_internal.hpp"
#include "vc_vote_plan.hpp"

static_assert(VC_VOTE_LABEL_NONE == VC_VOTE_NONE && VC_VOTE_KIND_COUNT == VC_VOTE_COUNT && VC_VOTE_KIND_CLOSENESS == VC_VOTE_CLOSENESS, "the header's constants");
static_assert(VC_VOTE_CLAMP == VC_LP_CLAMP_SEEDS && VC_VOTE_MAX_ITERS == VC_LP_MAX_ITERS, "the header's constants");
static_assert(sizeof(vc_knn_vote_stats) == VC_VOTE_HOST_STAT_BYTES && sizeof(vc_label_propagate_stats) == VC_VOTE_LP_HOST_STAT_BYTES, "the header's sizes");
static_assert(VC_VOTE_WAVE == VC_WAVE && VC_VOTE_BIG_MAX == VC_MAX_K, "the row view never leaves the LDS table");

namespace {

// the counters of one launch set (a vote call, a propagate round); the host reads the block as it lies
struct VcVoteStat {
  unsigned long long n_voted, n_unlabelled, n_ties, n_entries, n_changed, n_labelled;
  uint32_t bad, pad[3];
};
static_assert(sizeof(VcVoteStat) == VC_VOTE_STAT_BYTES, "the statistics block as it lies");
// the propagate plan's block
struct VcVotePlanStat {
  unsigned long long bin_start[VC_VOTE_BINS];   // the first place of every bin in the list
  unsigned long long long_slots;                // the slots of all long segments' tables
  uint32_t bad, pad;
};
static_assert(sizeof(VcVotePlanStat) <= VC_VOTE_PLAN_STAT_BYTES, "the plan's block");

struct VoteLongAux {   // per long segment
  unsigned long long best;
  uint32_t total, at_top;
};
static_assert(sizeof(VoteLongAux) == VC_VOTE_LONG_AUX_BYTES, "the long segments' block");

// what the tally launches work on
struct VoteArgs {
  const uint64_t* entries;   // rows [n_segs][k] or adj
  const uint64_t* offsets;   // CSR view: [n + 1]; null in the row view
  const uint32_t* counts;    // row view: [n_segs], nullable: every row holds `uniform` entries
  const uint32_t* list;      // CSR view: the records of this launch's bin
  uint64_t n_segs, n;
  uint32_t k, kk, uniform, max_dist, id_base, bits, kind;
  const uint32_t* labels;    // [n]: the labels that vote (L_{t-1})
  const uint32_t* current;   // CSR view: = labels; null in the row view (rule 2 has nothing to prefer)
  const uint32_t* seeds;     // CSR view under VC_LP_CLAMP_SEEDS: labels_in; else null
  uint32_t* out_label;       // [n_segs] / [n]
  uint32_t* out_votes;       // nullable
  uint32_t* out_total;       // nullable
  VcVoteStat* stat;
  // the long shape only
  const uint64_t* long_off;  // [n_segs]: the first slot of segment j's table
  uint32_t* long_label;      // [slots]
  uint32_t* long_tally;      // [slots]
  VoteLongAux* long_aux;     // [n_segs]
};

struct VoteAcc { uint32_t voted, unlabelled, ties, entries, changed, labelled; };

// segment s of the launch -> the record (row) it belongs to, its first entry and its length; false: a count above k (nothing is read)
__device__ __forceinline__ bool vote_open(const VoteArgs& a, uint64_t s, uint64_t* rec, uint64_t* base, uint32_t* len) {
  if (a.offsets) {
    const uint64_t r = a.list[s], b = a.offsets[r];
    *rec = r; *base = b; *len = (uint32_t)(a.offsets[r + 1] - b);   // the plan has checked the offsets
    return true;
  }
  const uint32_t c = a.counts ? a.counts[s] : a.uniform;
  *rec = s; *base = s * a.k;
  *len = c <= a.k ? vc_vote_row_entries(a.kk, c) : 0u;
  return c <= a.k;
}
// an entry of a segment -> its weight (0: it does not vote) and its label.  An id outside the store, or a voting entry beyond the
// code width under CLOSENESS, raises *bad and does not vote: nothing is read out of bounds
__device__ __forceinline__ uint32_t vote_entry(const VoteArgs& a, uint64_t word, uint32_t* lab, bool* bad) {
  const uint32_t d = (uint32_t)(word >> 32), id = (uint32_t)word - a.id_base;
  *lab = VC_VOTE_LABEL_NONE;
  if ((uint64_t)id >= a.n) { *bad = true; return 0u; }
  if (d > a.max_dist) return 0u;
  const uint32_t l = a.labels[id];
  if (l == VC_VOTE_LABEL_NONE) return 0u;
  if (a.kind == VC_VOTE_KIND_CLOSENESS && d > a.bits) { *bad = true; return 0u; }
  *lab = l;
  return vc_vote_weight(a.kind, a.bits, d);
}
__device__ __forceinline__ uint32_t vote_current(const VoteArgs& a, uint64_t rec) { return a.current ? a.current[rec] : VC_VOTE_LABEL_NONE; }
// one lane per segment: the outputs and the counters.  key 0: no voting entry
__device__ __forceinline__ void vote_finish(const VoteArgs& a, uint64_t s, uint64_t rec, uint32_t total, uint64_t key, uint32_t winner, uint32_t at_top, VoteAcc& acc) {
  const bool has = key != 0;
  uint32_t lab = has ? winner : VC_VOTE_LABEL_NONE;
  acc.voted += has;
  acc.unlabelled += !has;
  acc.ties += has && vc_vote_is_tie(key, at_top);
  uint64_t o = s;
  if (a.offsets) {
    o = rec;
    const uint32_t cur = a.current[rec];
    if (!has) lab = cur;
    if (a.seeds) {
      const uint32_t seed = a.seeds[rec];
      if (seed != VC_VOTE_LABEL_NONE) lab = seed;
    }
    acc.changed += lab != cur;
    acc.labelled += lab != VC_VOTE_LABEL_NONE;
  }
  a.out_label[o] = lab;
  if (a.out_votes) a.out_votes[o] = vc_vote_key_tally(key);
  if (a.out_total) a.out_total[o] = total;
}

__device__ __forceinline__ uint32_t vote_shfl(uint32_t v, uint32_t lane) { return (uint32_t)__shfl((int)v, (int)lane, VC_WAVE); }
__device__ __forceinline__ uint32_t vote_xor(uint32_t v, uint32_t o) { return (uint32_t)__shfl_xor((int)v, (int)o, VC_WAVE); }
__device__ __forceinline__ uint64_t vote_xor64(uint64_t v, uint32_t o) { return ((uint64_t)vote_xor((uint32_t)(v >> 32), o) << 32) | vote_xor((uint32_t)v, o); }
__device__ __forceinline__ uint64_t vote_max64(uint64_t a, uint64_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t vote_wave_sum(uint32_t v) {
  for (uint32_t o = VC_WAVE / 2; o; o >>= 1) v += vote_xor(v, o);
  return v;
}
// the wave's counters to the block: every lane calls; one atomic per counter that is not zero
__device__ __forceinline__ void vote_flush_wave(const VoteArgs& a, const VoteAcc& acc, bool bad) {
  const uint32_t voted = vote_wave_sum(acc.voted), unl = vote_wave_sum(acc.unlabelled), ties = vote_wave_sum(acc.ties), ent = vote_wave_sum(acc.entries),
                 chg = vote_wave_sum(acc.changed), labd = vote_wave_sum(acc.labelled);
  const bool any_bad = __ballot(bad) != 0;
  if (vc_lane() == 0) {
    if (voted) atomicAdd(&a.stat->n_voted, (unsigned long long)voted);
    if (unl) atomicAdd(&a.stat->n_unlabelled, (unsigned long long)unl);
    if (ties) atomicAdd(&a.stat->n_ties, (unsigned long long)ties);
    if (ent) atomicAdd(&a.stat->n_entries, (unsigned long long)ent);
    if (chg) atomicAdd(&a.stat->n_changed, (unsigned long long)chg);
    if (labd) atomicAdd(&a.stat->n_labelled, (unsigned long long)labd);
    if (any_bad) a.stat->bad = 1u;
  }
}

// ---- up to 64 entries: P lanes a segment ----------------------------------------------------------------------------------------------------
template <uint32_t P>
__global__ void __launch_bounds__(VC_VOTE_BLOCK) vc_vote_team_kernel(const VoteArgs a) {
  constexpr uint32_t TEAMS = VC_WAVE / P;
  const uint32_t lane = vc_lane(), sub = lane % P, tbase = lane - sub;
  const uint64_t team_mask = (P == VC_WAVE ? ~0ull : ((1ull << (P % VC_WAVE)) - 1ull)) << tbase;
  const uint64_t waves = (uint64_t)gridDim.x * (VC_VOTE_BLOCK / VC_WAVE), groups = (a.n_segs + TEAMS - 1) / TEAMS;
  VoteAcc acc{};
  bool bad = false;
  for (uint64_t g = (uint64_t)blockIdx.x * (VC_VOTE_BLOCK / VC_WAVE) + threadIdx.x / VC_WAVE; g < groups; g += waves) {   // (wave-uniform: every lane shuffles)
    const uint64_t s = g * TEAMS + lane / P;
    const bool live = s < a.n_segs;
    uint64_t rec = 0, base = 0;
    uint32_t len = 0, lab = VC_VOTE_LABEL_NONE, w = 0, cur = VC_VOTE_LABEL_NONE;
    if (live) {
      if (!vote_open(a, s, &rec, &base, &len)) bad = true;
      len = min(len, P);   // the launch's shape holds every segment given to it
      cur = vote_current(a, rec);
      if (sub < len) w = vote_entry(a, a.entries[base + sub], &lab, &bad);
    }
    uint32_t steps = len;
    for (uint32_t o = P; o < VC_WAVE; o <<= 1) steps = max(steps, vote_xor(steps, o));
    uint32_t tally = 0;
    bool earlier = false;
    for (uint32_t t = 0; t < steps; ++t) {
      const uint32_t ol = vote_shfl(lab, tbase + t), ow = vote_shfl(w, tbase + t);
      if (ol == lab) {
        tally += ow;
        earlier |= t < sub;
      }
    }
    const bool first = w != 0 && !earlier;
    uint64_t best = first ? vc_vote_key(tally, lab == cur, sub) : 0ull;
    uint32_t total = w;
    for (uint32_t o = P / 2; o; o >>= 1) {
      best = vote_max64(best, vote_xor64(best, o));
      total += vote_xor(total, o);
    }
    const uint32_t at_top = (uint32_t)__popcll(__ballot(first && tally == vc_vote_key_tally(best)) & team_mask);
    const uint32_t winner = vote_shfl(lab, tbase + (best ? vc_vote_key_pos(best) : 0u));
    acc.entries += w != 0;
    if (live && sub == 0) vote_finish(a, s, rec, total, best, winner, at_top, acc);
  }
  vote_flush_wave(a, acc, bad);
}

// ---- 65 .. 8192 entries: a wave or a block a segment, the table in LDS ------------------------------------------------------------------------
__device__ __forceinline__ void vote_insert(uint32_t* tab_label, uint32_t* tab_tally, uint32_t log2_slots, uint32_t lab, uint32_t w) {
  const uint32_t mask = (1u << log2_slots) - 1u;
  for (uint32_t h = vc_vote_slot_of(lab, log2_slots);; h = (h + 1u) & mask) {   // at most half full: an empty slot ends every probe
    const uint32_t prev = atomicCAS(tab_label + h, VC_VOTE_LABEL_NONE, lab);
    if (prev == VC_VOTE_LABEL_NONE || prev == lab) {
      atomicAdd(tab_tally + h, w);
      return;
    }
  }
}
__device__ __forceinline__ uint32_t vote_lookup(const uint32_t* tab_label, const uint32_t* tab_tally, uint32_t log2_slots, uint32_t lab) {
  const uint32_t mask = (1u << log2_slots) - 1u;
  uint32_t h = vc_vote_slot_of(lab, log2_slots);
  while (tab_label[h] != lab) h = (h + 1u) & mask;   // the label was inserted
  return tab_tally[h];
}

template <uint32_t T>
__global__ void __launch_bounds__(T) vc_vote_table_kernel(const VoteArgs a, const uint32_t max_slots) {
  extern __shared__ uint32_t vote_lds[];   // labels [max_slots] | tallies [max_slots]
  constexpr uint32_t WAVES = T / VC_WAVE;
  __shared__ unsigned long long red_best[WAVES];
  __shared__ uint32_t red_total[WAVES], red_votes[WAVES], red_top[WAVES];
  uint32_t* tab_label = vote_lds;
  uint32_t* tab_tally = vote_lds + max_slots;
  const uint32_t wave = threadIdx.x / VC_WAVE;
  VoteAcc acc{};
  bool bad = false;
  for (uint64_t s = blockIdx.x; s < a.n_segs; s += gridDim.x) {   // (block-uniform)
    uint64_t rec = 0, base = 0;
    uint32_t len = 0;
    if (!vote_open(a, s, &rec, &base, &len)) bad = true;
    const uint32_t slots = min((uint32_t)vc_vote_slots(len), max_slots), log2_slots = 31u - (uint32_t)__clz(slots);
    len = min(len, slots / 2);   // the launch's shape holds every segment given to it
    const uint32_t cur = vote_current(a, rec);
    for (uint32_t i = threadIdx.x; i < slots; i += T) {
      tab_label[i] = VC_VOTE_LABEL_NONE;
      tab_tally[i] = 0u;
    }
    __syncthreads();
    uint32_t total = 0, votes = 0;
    for (uint32_t e = threadIdx.x; e < len; e += T) {
      uint32_t lab;
      const uint32_t w = vote_entry(a, a.entries[base + e], &lab, &bad);
      if (w) {
        vote_insert(tab_label, tab_tally, log2_slots, lab, w);
        total += w;
        ++votes;
      }
    }
    __syncthreads();
    uint64_t best = 0;
    for (uint32_t e = threadIdx.x; e < len; e += T) {
      uint32_t lab;
      bool again = false;
      const uint32_t w = vote_entry(a, a.entries[base + e], &lab, &again);
      if (w) best = vote_max64(best, vc_vote_key(vote_lookup(tab_label, tab_tally, log2_slots, lab), lab == cur, e));
    }
    for (uint32_t o = VC_WAVE / 2; o; o >>= 1) {
      best = vote_max64(best, vote_xor64(best, o));
      total += vote_xor(total, o);
      votes += vote_xor(votes, o);
    }
    if (WAVES > 1) {
      if (vc_lane() == 0) {
        red_best[wave] = best;
        red_total[wave] = total;
        red_votes[wave] = votes;
      }
      __syncthreads();
      best = 0; total = 0; votes = 0;
      for (uint32_t v = 0; v < WAVES; ++v) {
        best = vote_max64(best, red_best[v]);
        total += red_total[v];
        votes += red_votes[v];
      }
    }
    const uint32_t top = vc_vote_key_tally(best);
    uint32_t at_top = 0;
    if (best)
      for (uint32_t i = threadIdx.x; i < slots; i += T) at_top += tab_label[i] != VC_VOTE_LABEL_NONE && tab_tally[i] == top;
    at_top = vote_wave_sum(at_top);
    if (WAVES > 1) {
      if (vc_lane() == 0) red_top[wave] = at_top;
      __syncthreads();
      at_top = 0;
      for (uint32_t v = 0; v < WAVES; ++v) at_top += red_top[v];
    }
    if (threadIdx.x == 0) {
      uint32_t winner = VC_VOTE_LABEL_NONE;
      if (best) winner = a.labels[(uint32_t)a.entries[base + vc_vote_key_pos(best)] - a.id_base];   // an entry that voted: its id is in the store
      acc.entries += votes;
      vote_finish(a, s, rec, total, best, winner, at_top, acc);
    }
    __syncthreads();   // the table and the reduction words are the next segment's
  }
  if (threadIdx.x == 0) {
    if (acc.voted) atomicAdd(&a.stat->n_voted, (unsigned long long)acc.voted);
    if (acc.unlabelled) atomicAdd(&a.stat->n_unlabelled, (unsigned long long)acc.unlabelled);
    if (acc.ties) atomicAdd(&a.stat->n_ties, (unsigned long long)acc.ties);
    if (acc.entries) atomicAdd(&a.stat->n_entries, (unsigned long long)acc.entries);
    if (acc.changed) atomicAdd(&a.stat->n_changed, (unsigned long long)acc.changed);
    if (acc.labelled) atomicAdd(&a.stat->n_labelled, (unsigned long long)acc.labelled);
  }
  if (bad) a.stat->bad = 1u;
}

// ---- above 8192 entries: blockIdx.y names the segment, VC_VOTE_LONG_BLOCKS blocks stride over it, the table lies in scratch ------------------
struct VoteLongSeg {
  uint64_t rec, base;
  uint32_t len, log2_slots;
  uint32_t* tab_label;
  uint32_t* tab_tally;
};
__device__ __forceinline__ VoteLongSeg vote_long_open(const VoteArgs& a, uint64_t j) {
  VoteLongSeg g;
  vote_open(a, j, &g.rec, &g.base, &g.len);
  g.log2_slots = vc_vote_log2(vc_vote_slots(g.len));
  g.tab_label = a.long_label + a.long_off[j];
  g.tab_tally = a.long_tally + a.long_off[j];
  return g;
}
__global__ void __launch_bounds__(VC_VOTE_BLOCK) vc_vote_long_insert_kernel(const VoteArgs a) {
  bool bad = false;
  for (uint64_t j = blockIdx.y; j < a.n_segs; j += gridDim.y) {   // (block-uniform)
  const VoteLongSeg g = vote_long_open(a, j);
  uint32_t total = 0;
  for (uint32_t e = blockIdx.x * VC_VOTE_BLOCK + threadIdx.x; e < g.len; e += gridDim.x * VC_VOTE_BLOCK) {
    uint32_t lab;
    const uint32_t w = vote_entry(a, a.entries[g.base + e], &lab, &bad);
    if (w) {
      vote_insert(g.tab_label, g.tab_tally, g.log2_slots, lab, w);
      total += w;
    }
  }
  total = vote_wave_sum(total);
  if (vc_lane() == 0 && total) atomicAdd(&a.long_aux[j].total, total);
  }
  if (bad) a.stat->bad = 1u;
}
__global__ void __launch_bounds__(VC_VOTE_BLOCK) vc_vote_long_key_kernel(const VoteArgs a) {
  for (uint64_t j = blockIdx.y; j < a.n_segs; j += gridDim.y) {   // (block-uniform)
  const VoteLongSeg g = vote_long_open(a, j);
  const uint32_t cur = vote_current(a, g.rec);
  uint64_t best = 0;
  for (uint32_t e = blockIdx.x * VC_VOTE_BLOCK + threadIdx.x; e < g.len; e += gridDim.x * VC_VOTE_BLOCK) {
    uint32_t lab;
    bool again = false;
    const uint32_t w = vote_entry(a, a.entries[g.base + e], &lab, &again);
    if (w) best = vote_max64(best, vc_vote_key(vote_lookup(g.tab_label, g.tab_tally, g.log2_slots, lab), lab == cur, e));
  }
  for (uint32_t o = VC_WAVE / 2; o; o >>= 1) best = vote_max64(best, vote_xor64(best, o));
  if (vc_lane() == 0 && best) atomicMax(&a.long_aux[j].best, (unsigned long long)best);
  }
}
__global__ void __launch_bounds__(VC_VOTE_BLOCK) vc_vote_long_top_kernel(const VoteArgs a) {
  for (uint64_t j = blockIdx.y; j < a.n_segs; j += gridDim.y) {   // (block-uniform)
  const VoteLongSeg g = vote_long_open(a, j);
  const uint64_t best = a.long_aux[j].best;
  const uint32_t top = vc_vote_key_tally(best), slots = 1u << g.log2_slots;
  uint32_t at_top = 0;
  if (best)
    for (uint32_t i = blockIdx.x * VC_VOTE_BLOCK + threadIdx.x; i < slots; i += gridDim.x * VC_VOTE_BLOCK)
      at_top += g.tab_label[i] != VC_VOTE_LABEL_NONE && g.tab_tally[i] == top;
  at_top = vote_wave_sum(at_top);
  if (vc_lane() == 0 && at_top) atomicAdd(&a.long_aux[j].at_top, at_top);
  }
}
__global__ void __launch_bounds__(VC_VOTE_BLOCK) vc_vote_long_finish_kernel(const VoteArgs a) {
  VoteAcc acc{};
  for (uint64_t j0 = (uint64_t)blockIdx.x * VC_VOTE_BLOCK; j0 < a.n_segs; j0 += (uint64_t)gridDim.x * VC_VOTE_BLOCK) {   // (block-uniform)
    const uint64_t j = j0 + threadIdx.x;
    if (j < a.n_segs) {
      uint64_t rec, base;
      uint32_t len;
      vote_open(a, j, &rec, &base, &len);
      const VoteLongAux x = a.long_aux[j];
      uint32_t winner = VC_VOTE_LABEL_NONE;
      if (x.best) winner = a.labels[(uint32_t)a.entries[base + vc_vote_key_pos(x.best)] - a.id_base];
      vote_finish(a, j, rec, x.total, x.best, winner, x.at_top, acc);
    }
  }
  vote_flush_wave(a, acc, false);
}

// ---- the propagate plan -----------------------------------------------------------------------------------------------------------------------
struct VotePlanArgs {
  const uint64_t* offsets;   // [n + 1]
  const uint64_t* adj;       // [n_entries]
  uint64_t n, n_entries;
  uint32_t id_base, bits, kind;
  uint32_t* counts;          // [VC_VOTE_BINS][blocks], scanned in place
  uint32_t* list;            // [n]
  uint64_t* long_off;        // [long_cap]
  uint64_t long_cap;
  uint64_t blocks;
  VcVotePlanStat* plan;
};
// the length of record i's segment; *bad for offsets that do not start at 0, decrease, do not end at n_entries, or a tally that would
// not fit 32 bits (the length is then 0)
__device__ __forceinline__ uint64_t vote_plan_length(const VotePlanArgs& p, uint64_t i, bool* bad) {
  const uint64_t o0 = p.offsets[i], o1 = p.offsets[i + 1];
  const bool wrong = o1 < o0 || (i == 0 && o0 != 0) || (i + 1 == p.n && o1 != p.n_entries) || o1 > p.n_entries || !vc_vote_length_ok(o1 - o0, p.bits);
  if (wrong) *bad = true;
  return wrong ? 0ull : o1 - o0;
}
__global__ void __launch_bounds__(VC_VOTE_BLOCK) vc_vote_plan_count_kernel(const VotePlanArgs p) {
  __shared__ uint32_t cnt[VC_VOTE_BINS];
  if (threadIdx.x < VC_VOTE_BINS) cnt[threadIdx.x] = 0u;
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * VC_VOTE_BLOCK + threadIdx.x;
  bool bad = false;
  uint32_t bin = VC_VOTE_BINS;
  if (i < p.n) {
    const uint64_t len = vote_plan_length(p, i, &bad);
    bin = vc_vote_bin(len);
    if (bin == VC_VOTE_BIN_LONG) atomicAdd(&p.plan->long_slots, (unsigned long long)vc_vote_slots(len));
  }
  for (uint32_t b = 0; b < VC_VOTE_BINS; ++b) {
    const uint64_t m = __ballot(bin == b);
    if (vc_lane() == 0 && m) atomicAdd(cnt + b, (uint32_t)__popcll(m));
  }
  __syncthreads();
  if (threadIdx.x < VC_VOTE_BINS) p.counts[threadIdx.x * p.blocks + blockIdx.x] = cnt[threadIdx.x];
  if (bad) p.plan->bad = 1u;
}
// every entry names a record of the store, and under CLOSENESS lies within the code width
__global__ void __launch_bounds__(VC_VOTE_BLOCK) vc_vote_plan_entries_kernel(const VotePlanArgs p) {
  bool bad = false;
  for (uint64_t t = (uint64_t)blockIdx.x * VC_VOTE_BLOCK + threadIdx.x; t < p.n_entries; t += (uint64_t)gridDim.x * VC_VOTE_BLOCK) {
    const uint64_t word = p.adj[t];
    bad |= (uint64_t)((uint32_t)word - p.id_base) >= p.n || (p.kind == VC_VOTE_KIND_CLOSENESS && (uint32_t)(word >> 32) > p.bits);
  }
  if (bad) p.plan->bad = 1u;
}
// counts scanned: record i goes to place scan[bin][block] + its rank among the block's records of that bin, in record order
__global__ void __launch_bounds__(VC_VOTE_BLOCK) vc_vote_plan_fill_kernel(const VotePlanArgs p) {
  constexpr uint32_t WAVES = VC_VOTE_BLOCK / VC_WAVE;
  __shared__ uint32_t wcnt[WAVES][VC_VOTE_BINS];
  const uint64_t i = (uint64_t)blockIdx.x * VC_VOTE_BLOCK + threadIdx.x;
  const uint32_t lane = vc_lane(), wave = threadIdx.x / VC_WAVE;
  bool bad = false;
  uint32_t bin = VC_VOTE_BINS, rank = 0;
  if (i < p.n) bin = vc_vote_bin(vote_plan_length(p, i, &bad));
  for (uint32_t b = 0; b < VC_VOTE_BINS; ++b) {
    const uint64_t m = __ballot(bin == b);
    if (bin == b) rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wcnt[wave][b] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  if (i < p.n) {
    uint32_t before = 0;
    for (uint32_t v = 0; v < wave; ++v) before += wcnt[v][bin];
    p.list[(uint64_t)p.counts[bin * p.blocks + blockIdx.x] + before + rank] = (uint32_t)i;   // a place below n: the counts sum to n
  }
}
// one thread: the bins' first places and the layout of the long segments' tables, in list order
__global__ void vc_vote_plan_finish_kernel(const VotePlanArgs p) {
  if (blockIdx.x || threadIdx.x) return;
  for (uint32_t b = 0; b < VC_VOTE_BINS; ++b) p.plan->bin_start[b] = p.counts[b * p.blocks];
  const uint64_t first = p.counts[VC_VOTE_BIN_LONG * p.blocks];
  uint64_t off = 0;
  for (uint64_t j = 0; first + j < p.n && j < p.long_cap; ++j) {
    const uint64_t r = p.list[first + j];
    bool bad = false;
    p.long_off[j] = off;
    off += vc_vote_slots(vote_plan_length(p, r, &bad));
  }
}

uint32_t vote_grid(uint64_t items, uint32_t per_block) {
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + per_block - 1) / per_block, 1), 256 * 8);
}

#define VOTE_HIP(call) VC_HIP_OR_FAIL("label vote", call)

// one tally launch over a.n_segs segments of at most `bound` entries each (bound <= VC_VOTE_BIG_MAX)
hipError_t vote_launch(const VoteArgs& a, uint32_t bound, hipStream_t s) {
  if (bound <= VC_VOTE_TEAM_MAX) {
    const uint32_t P = vc_vote_team_lanes(bound), waves_per_block = VC_VOTE_BLOCK / VC_WAVE;
    const uint32_t grid = vote_grid(a.n_segs, (VC_WAVE / P) * waves_per_block);
    switch (P) {
      case 8: hipLaunchKernelGGL(vc_vote_team_kernel<8>, dim3(grid), dim3(VC_VOTE_BLOCK), 0, s, a); break;
      case 16: hipLaunchKernelGGL(vc_vote_team_kernel<16>, dim3(grid), dim3(VC_VOTE_BLOCK), 0, s, a); break;
      case 32: hipLaunchKernelGGL(vc_vote_team_kernel<32>, dim3(grid), dim3(VC_VOTE_BLOCK), 0, s, a); break;
      default: hipLaunchKernelGGL(vc_vote_team_kernel<64>, dim3(grid), dim3(VC_VOTE_BLOCK), 0, s, a);
    }
    return hipGetLastError();
  }
  const uint32_t lds = vc_vote_lds_bytes(bound), max_slots = lds / VC_VOTE_SLOT_BYTES;
  if (vc_vote_table_threads(bound) == VC_WAVE) {
    const uint32_t grid = (uint32_t)std::min<uint64_t>(a.n_segs, 256 * 32);
    hipLaunchKernelGGL(vc_vote_table_kernel<VC_WAVE>, dim3(grid), dim3(VC_WAVE), lds, s, a, max_slots);
  } else {
    if (lds > (64u << 10)) {   // above 64 KiB the dynamic LDS of a kernel has to be granted first
      const hipError_t r = hipFuncSetAttribute((const void*)vc_vote_table_kernel<VC_VOTE_BLOCK>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (r != hipSuccess) return r;
    }
    const uint32_t grid = (uint32_t)std::min<uint64_t>(a.n_segs, lds > (64u << 10) ? 256 : 256 * 8);
    hipLaunchKernelGGL(vc_vote_table_kernel<VC_VOTE_BLOCK>, dim3(grid), dim3(VC_VOTE_BLOCK), lds, s, a, max_slots);
  }
  return hipGetLastError();
}

}  // namespace

int vc_knn_vote_run(const VcStoreView& v, const VcVoteArgs& a, vc_knn_vote_stats* stats, hipStream_t s, std::string* err) {
  if (stats) *stats = vc_knn_vote_stats{};
  if (a.n_rows == 0) return VC_OK;
  VcVoteStat* d_stat = (VcVoteStat*)v.alloc(VC_VOTE_STAT, (size_t)vc_vote_lp_stat_bytes());
  if (!d_stat) return VC_ERR_NOMEM;
  VoteArgs k{};
  k.entries = a.d_rows; k.counts = a.d_counts; k.n_segs = a.n_rows; k.n = v.n; k.k = a.k; k.kk = a.kk; k.uniform = vc_vote_row_count(v.n, a.k);
  k.max_dist = a.max_dist; k.id_base = v.id_base; k.bits = 64 * v.W; k.kind = a.weight_kind; k.labels = a.d_labels;
  k.out_label = a.d_out_label; k.out_votes = a.d_out_votes; k.out_total = a.d_out_total; k.stat = d_stat;
  VOTE_HIP(hipMemsetAsync(d_stat, 0, VC_VOTE_STAT_BYTES, s));
  VOTE_HIP(vote_launch(k, a.kk, s));
  VcVoteStat home{};   // THE WAIT: the counters and the error word
  VOTE_HIP(hipMemcpyAsync(&home, d_stat, VC_VOTE_STAT_BYTES, hipMemcpyDeviceToHost, s));
  VOTE_HIP(hipStreamSynchronize(s));
  if (home.bad) {
    if (err) *err = "label vote: a count above k, an id outside the store or a distance above the code width under VC_VOTE_CLOSENESS";
    return VC_ERR_INVALID;
  }
  if (stats) *stats = vc_knn_vote_stats{home.n_voted, home.n_unlabelled, home.n_ties, home.n_entries};
  return VC_OK;
}

int vc_knn_vote_run_host(const VcStoreView& v, VcVoteArgs a, const uint64_t* rows, const uint32_t* counts, const uint32_t* labels, uint32_t* out_label,
                         uint32_t* out_votes, uint32_t* out_total, vc_knn_vote_stats* stats, hipStream_t s, std::string* err) {
  if (a.n_rows == 0) {
    if (stats) *stats = vc_knn_vote_stats{};
    return VC_OK;
  }
  const size_t n = (size_t)v.n, nr = (size_t)a.n_rows;
  const VcVoteStage L(nr, a.k, n, counts != nullptr);
  uint8_t* stage = (uint8_t*)v.alloc(VC_VOTE_STAGE, (size_t)L.total);
  if (!stage) return VC_ERR_NOMEM;
  VOTE_HIP(hipMemcpyAsync(stage + L.rows, rows, nr * a.k * 8, hipMemcpyHostToDevice, s));
  if (n) VOTE_HIP(hipMemcpyAsync(stage + L.labels, labels, n * 4, hipMemcpyHostToDevice, s));
  if (counts) VOTE_HIP(hipMemcpyAsync(stage + L.counts, counts, nr * 4, hipMemcpyHostToDevice, s));
  a.d_rows = (const uint64_t*)(stage + L.rows);
  a.d_counts = counts ? (const uint32_t*)(stage + L.counts) : nullptr;
  a.d_labels = (const uint32_t*)(stage + L.labels);
  a.d_out_label = (uint32_t*)(stage + L.out_label);
  a.d_out_votes = out_votes ? (uint32_t*)(stage + L.out_votes) : nullptr;
  a.d_out_total = out_total ? (uint32_t*)(stage + L.out_total) : nullptr;
  const int rc = vc_knn_vote_run(v, a, stats, s, err);
  if (rc) return rc;
  VOTE_HIP(hipMemcpyAsync(out_label, a.d_out_label, nr * 4, hipMemcpyDeviceToHost, s));
  if (out_votes) VOTE_HIP(hipMemcpyAsync(out_votes, a.d_out_votes, nr * 4, hipMemcpyDeviceToHost, s));
  if (out_total) VOTE_HIP(hipMemcpyAsync(out_total, a.d_out_total, nr * 4, hipMemcpyDeviceToHost, s));
  VOTE_HIP(hipStreamSynchronize(s));
  return VC_OK;
}

#undef VOTE_HIP
#define VOTE_HIP(call) VC_HIP_OR_FAIL("label propagation", call)

int vc_label_propagate_run(const VcStoreView& v, const VcLabelPropagateArgs& a, vc_label_propagate_stats* stats, hipStream_t s, std::string* err) {
  if (stats) *stats = vc_label_propagate_stats{};
  const uint64_t n = v.n;
  if (n == 0) return VC_OK;
  // every buffer of the plan and the rounds but the long tables, before the first launch
  const uint64_t blocks = vc_vote_plan_blocks(n), count_words = vc_vote_plan_count_words(n), word4 = vc_vote_words4(n);
  const uint64_t long_cap = vc_vote_long_cap(a.n_entries);
  uint8_t* d_stat = (uint8_t*)v.alloc(VC_VOTE_STAT, (size_t)vc_vote_lp_stat_bytes());
  uint8_t* d_plan = (uint8_t*)v.alloc(VC_VOTE_PLAN, (size_t)vc_vote_lp_bytes(n));
  uint32_t* d_scan = (uint32_t*)v.alloc(VC_VOTE_SCAN, std::max<size_t>(vc_scan_work_words(count_words), 1) * 4);
  uint64_t* d_long_off = (uint64_t*)v.alloc(VC_VOTE_LONG_OFF, (size_t)long_cap * 8);
  if (!d_stat || !d_plan || !d_scan || !d_long_off) return VC_ERR_NOMEM;
  VotePlanArgs p{};
  p.offsets = a.d_offsets; p.adj = a.d_adj; p.n = n; p.n_entries = a.n_entries; p.id_base = v.id_base; p.bits = 64 * v.W; p.kind = a.weight_kind;
  p.list = (uint32_t*)d_plan;
  uint32_t* buf[2] = {(uint32_t*)(d_plan + word4), (uint32_t*)(d_plan + 2 * word4)};
  p.counts = (uint32_t*)(d_plan + 3 * word4);
  p.long_off = d_long_off; p.long_cap = long_cap; p.blocks = blocks;
  p.plan = (VcVotePlanStat*)d_stat;
  VcVoteStat* d_round = (VcVoteStat*)(d_stat + VC_VOTE_PLAN_STAT_BYTES);   // [VC_VOTE_MAX_ITERS]
  VOTE_HIP(hipMemsetAsync(d_stat, 0, (size_t)vc_vote_lp_stat_bytes(), s));
  // 1. the plan: the checks, the bins' lists by ONE scan, the long tables' layout
  hipLaunchKernelGGL(vc_vote_plan_count_kernel, dim3((uint32_t)blocks), dim3(VC_VOTE_BLOCK), 0, s, p);
  VOTE_HIP(hipGetLastError());
  if (a.n_entries) {
    hipLaunchKernelGGL(vc_vote_plan_entries_kernel, dim3(vote_grid(a.n_entries, VC_VOTE_BLOCK)), dim3(VC_VOTE_BLOCK), 0, s, p);
    VOTE_HIP(hipGetLastError());
  }
  VOTE_HIP(vc_exclusive_scan_u32(p.counts, p.counts, count_words, d_scan, s));
  hipLaunchKernelGGL(vc_vote_plan_fill_kernel, dim3((uint32_t)blocks), dim3(VC_VOTE_BLOCK), 0, s, p);
  VOTE_HIP(hipGetLastError());
  hipLaunchKernelGGL(vc_vote_plan_finish_kernel, dim3(1), dim3(VC_WAVE), 0, s, p);
  VOTE_HIP(hipGetLastError());
  VcVotePlanStat plan{};   // THE PLAN'S WAIT: the bins, the long tables' slots, the error word
  VOTE_HIP(hipMemcpyAsync(&plan, d_stat, sizeof(plan), hipMemcpyDeviceToHost, s));
  VOTE_HIP(hipStreamSynchronize(s));
  if (plan.bad) {
    if (err)
      *err = "label propagation: offsets that do not start at 0, decrease or do not end at n_entries, an id outside the store, a distance above the code "
             "width under VC_VOTE_CLOSENESS, or a segment whose tally does not fit 32 bits";
    return VC_ERR_INVALID;
  }
  uint64_t bin_size[VC_VOTE_BINS];
  for (uint32_t b = 0; b < VC_VOTE_BINS; ++b) bin_size[b] = (b + 1 < VC_VOTE_BINS ? plan.bin_start[b + 1] : n) - plan.bin_start[b];
  const uint64_t n_long = bin_size[VC_VOTE_BIN_LONG], long_slots = plan.long_slots;
  uint8_t* d_long = nullptr;
  if (n_long) {
    d_long = (uint8_t*)v.alloc(VC_VOTE_LONG, (size_t)vc_vote_long_bytes(n_long, long_slots));
    if (!d_long) return VC_ERR_NOMEM;
  }
  // 2. the rounds: one launch per non-empty bin (four for the long one), one read-back each
  VoteArgs k{};
  k.entries = a.d_adj; k.offsets = a.d_offsets; k.n = n; k.max_dist = 0xFFFFFFFFu; k.id_base = v.id_base; k.bits = 64 * v.W; k.kind = a.weight_kind;
  k.seeds = (a.flags & VC_VOTE_CLAMP) ? a.d_labels_in : nullptr;
  k.out_votes = a.d_votes; k.out_total = a.d_total;
  k.long_off = d_long_off;
  k.long_aux = (VoteLongAux*)d_long;
  k.long_label = (uint32_t*)(d_long + n_long * VC_VOTE_LONG_AUX_BYTES);
  k.long_tally = k.long_label + long_slots;
  VcVoteStat home{};
  uint32_t iters = 0, converged = 0;
  const uint32_t* src = a.d_labels_in;
  for (uint32_t t = 0; t < a.max_iters; ++t) {
    uint32_t* dst = buf[t & 1u];
    k.labels = k.current = src; k.out_label = dst; k.stat = d_round + t;
    for (uint32_t b = 0; b < VC_VOTE_BIN_LONG; ++b) {
      if (!bin_size[b]) continue;
      k.list = p.list + plan.bin_start[b]; k.n_segs = bin_size[b];
      VOTE_HIP(vote_launch(k, vc_vote_bin_max(b), s));
    }
    if (n_long) {
      k.list = p.list + plan.bin_start[VC_VOTE_BIN_LONG]; k.n_segs = n_long;
      VOTE_HIP(hipMemsetAsync(k.long_aux, 0, (size_t)n_long * VC_VOTE_LONG_AUX_BYTES, s));
      VOTE_HIP(hipMemsetAsync(k.long_label, 0xFF, (size_t)long_slots * 4, s));
      VOTE_HIP(hipMemsetAsync(k.long_tally, 0, (size_t)long_slots * 4, s));
      const dim3 grid(VC_VOTE_LONG_BLOCKS, (uint32_t)std::min<uint64_t>(n_long, 65535));
      hipLaunchKernelGGL(vc_vote_long_insert_kernel, grid, dim3(VC_VOTE_BLOCK), 0, s, k);
      VOTE_HIP(hipGetLastError());
      hipLaunchKernelGGL(vc_vote_long_key_kernel, grid, dim3(VC_VOTE_BLOCK), 0, s, k);
      VOTE_HIP(hipGetLastError());
      hipLaunchKernelGGL(vc_vote_long_top_kernel, grid, dim3(VC_VOTE_BLOCK), 0, s, k);
      VOTE_HIP(hipGetLastError());
      hipLaunchKernelGGL(vc_vote_long_finish_kernel, dim3(vote_grid(n_long, VC_VOTE_BLOCK)), dim3(VC_VOTE_BLOCK), 0, s, k);
      VOTE_HIP(hipGetLastError());
    }
    VOTE_HIP(hipMemcpyAsync(&home, d_round + t, VC_VOTE_STAT_BYTES, hipMemcpyDeviceToHost, s));
    VOTE_HIP(hipStreamSynchronize(s));
    ++iters;
    src = dst;
    if (home.n_changed == 0) {
      converged = 1;
      break;
    }
  }
  VOTE_HIP(hipMemcpyAsync(a.d_labels_out, src, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  if (stats) *stats = vc_label_propagate_stats{iters, converged, home.n_changed, home.n_labelled, home.n_ties};
  return VC_OK;
}

int vc_label_propagate_run_host(const VcStoreView& v, VcLabelPropagateArgs a, const uint64_t* offsets, const uint64_t* adj, const uint32_t* labels_in,
                                uint32_t* labels_out, uint32_t* votes, uint32_t* totals, vc_label_propagate_stats* stats, hipStream_t s, std::string* err) {
  if (v.n == 0) {
    if (stats) *stats = vc_label_propagate_stats{};
    return VC_OK;
  }
  const size_t n = (size_t)v.n, ne = (size_t)a.n_entries;
  const VcVoteLpStage L(n, ne);
  uint8_t* stage = (uint8_t*)v.alloc(VC_VOTE_STAGE, (size_t)L.total);
  if (!stage) return VC_ERR_NOMEM;
  VOTE_HIP(hipMemcpyAsync(stage + L.offsets, offsets, (n + 1) * 8, hipMemcpyHostToDevice, s));
  if (ne) VOTE_HIP(hipMemcpyAsync(stage + L.adj, adj, ne * 8, hipMemcpyHostToDevice, s));
  VOTE_HIP(hipMemcpyAsync(stage + L.labels_in, labels_in, n * 4, hipMemcpyHostToDevice, s));
  a.d_offsets = (const uint64_t*)(stage + L.offsets);
  a.d_adj = (const uint64_t*)(stage + L.adj);
  a.d_labels_in = (const uint32_t*)(stage + L.labels_in);
  a.d_labels_out = (uint32_t*)(stage + L.labels_out);
  a.d_votes = votes ? (uint32_t*)(stage + L.votes) : nullptr;
  a.d_total = totals ? (uint32_t*)(stage + L.totals) : nullptr;
  const int rc = vc_label_propagate_run(v, a, stats, s, err);
  if (rc) return rc;
  VOTE_HIP(hipMemcpyAsync(labels_out, a.d_labels_out, n * 4, hipMemcpyDeviceToHost, s));
  if (votes) VOTE_HIP(hipMemcpyAsync(votes, a.d_votes, n * 4, hipMemcpyDeviceToHost, s));
  if (totals) VOTE_HIP(hipMemcpyAsync(totals, a.d_total, n * 4, hipMemcpyDeviceToHost, s));
  VOTE_HIP(hipStreamSynchronize(s));
  return VC_OK;
}
