// ============================================================================
// vc_mst_condense.hip -- the condensed tree of a spanning forest, its stabilities, the excess-of-mass or leaf selection and the flat
// labels (vc_mst_condense*, vc_sharded_mst_condense*); the header states the contract.  One driver for both handle kinds over a
// VcStoreView; the plan arithmetic -- the checks, the level table, the tags, the stability, the sizes -- is vc_mst_condense_plan.hpp.
// Weights are Hamming distances, so the dendrogram has at most bits + 1 levels, and a level is one parallel union pass.
//   vc_cond_init_kernel      forest[i] = comp[i] = id_base + i, size 1, no node, the sums and the claims zero, own = leave = NONE
//   vc_cond_plan_kernel      per edge: an end outside the store, a == b, a weight above bits, a weight below its predecessor's or a
//                            root weight not above the last raise the error word; the first edge of a weight writes first[weight]
//   per level (tags from the level's number, grids from the level table, no wait):
//   vc_cond_unite_kernel     the level's edges united in the working forest by vc_forest.hpp's cl_unite
//   vc_cond_tally_kernel     per edge end: the old root from the snapshot, claimed once (atomicMax of the tag); its size goes to the new
//                            root's total and to its small sum or big count -- integer atomics, any order
//   vc_cond_decide_kernel    per edge end: the new root, claimed once, applies the table of cases: two or more big children or none with
//                            the total at mcs make a node (a cursor bump, any order), one big child is marked as going on
//   vc_cond_apply_kernel     per edge end: the old root, claimed a second time; a big one ends its node under the new one (parent, end,
//                            rep) or, the only big one, grows it by the small sum and hands it to the new root
//   vc_cond_settle_kernel    per record: the root with path halving into the next snapshot; a record without a node whose new root now
//                            carries one takes own and leave; the new root's own thread takes size and node and zeroes the sums
//   vc_cond_roots_kernel     per record that is a root: counted (a cycle shows in the count); its live node ends at root_weight
//   vc_cond_keys_kernel      node j -> the sort's item (form, rep << 32 | j)
//   vc_cond_rank_kernel      after vc_sort.hip's radix sort by (form, rep): rank[scratch index] = the node's number
//   vc_cond_write_kernel     node t of the output: the parent renumbered, the stability; the reduction's counters armed
//   vc_cond_fold_kernel      one thread per leaf walks upwards: keep and best of the node, best added to the parent's sum, and only the
//                            child that arrives last goes on with the parent -- integer adds, so the order is nothing
//   vc_cond_select_kernel    per node: the topmost candidate (keep, or a leaf under LEAF) on the way up is its selected ancestor
//   vc_cond_label_kernel     per record: label, node, own, leave
// Three small read-backs: the plan, the node count with the component count, the statistics.  No LDS, no scratch memory, no
// cooperative launch.
// ============================================================================
#include <algorithm>
#include <vector>

#include "vc_forest.hpp"
#include "vc_internal.hpp"
#include "vc_mst_condense_plan.hpp"

static_assert(VC_CONDENSE_EOM == VC_COND_EOM && VC_CONDENSE_LEAF == VC_COND_LEAF && VC_CONDENSE_NONE == VC_COND_NONE, "the header's constants");
static_assert(VC_CONDENSE_SELECTED == VC_COND_SELECTED && VC_CONDENSE_KEEP == VC_COND_KEEP && VC_CONDENSE_ROOT == VC_COND_ROOT, "the header's flags");
static_assert(sizeof(vc_condensed_node) == VC_COND_NODE_BYTES && sizeof(vc_mst_condense_stats) == VC_COND_HOST_STAT_BYTES, "the header's sizes");
static_assert(sizeof(vc_mst_edge) == VC_COND_EDGE_BYTES, "the header's edge");

namespace {

// the device's block; the host reads it as it lies
struct VcCondStat {
  unsigned long long n_leaves, n_roots, n_selected, n_clustered, total_stability, n_comp;
  uint32_t n_nodes;   // the cursor of the working nodes
  uint32_t bad;
};
static_assert(sizeof(VcCondStat) == VC_COND_STAT_BYTES, "the statistics block as it lies");

// a node while the levels run, numbered by the cursor
struct CdNode {
  uint32_t parent, rep, form, end, size, n_children, root, pad;
  unsigned long long sum_leave;
};
static_assert(sizeof(CdNode) == VC_COND_WORK_NODE_BYTES, "the working node as it lies");

#define CD_GOES_ON 0xFFFFFFFEu   // decision of a new root with exactly one big child, until that child hands over its node

// what the launches work on
struct CondArgs {
  const vc_mst_edge* edges;
  uint64_t n_edges, n;
  uint32_t id_base, bits, mcs, root_weight, method, node_cap;
  uint32_t* forest;     // [n]: the working forest of vc_forest.hpp, global ids
  uint32_t* comp;       // [n]: the snapshot before the level, the root (smallest global id) of every record's component
  uint32_t* csize;      // [n]: at a root of the snapshot, the records of its component
  uint32_t* cnode;      // [n]: at a root of the snapshot, the working node its component carries, or NONE
  uint32_t* tot;        // [n]: at a new root, the sizes of the old components under it
  uint32_t* big;        // [n]: ... how many of them have mcs records
  uint32_t* small_sum;  // [n]: ... the records of the others
  uint32_t* decided;    // [n]: ... the node the new component carries, NONE, or CD_GOES_ON
  uint32_t* claim_old;  // [n]: vc_cond_tag_tally / vc_cond_tag_apply of the last level that touched this old root
  uint32_t* claim_new;  // [n]: vc_cond_tag_new of the last level that made this a new root
  uint32_t* own;        // [n]: working node index
  uint32_t* leave;      // [n]
  uint32_t* first;      // [bits + 1]: the plan's table
  CdNode* work;         // [node_cap]
  uint32_t* rank;       // [node_cap]: working index -> number
  uint32_t* sel_anc;    // [node_cap]: number -> the selected node at or above it, or NONE
  uint32_t* cand;       // [node_cap]: number -> may be selected when no ancestor is
  uint32_t* pending;    // [node_cap]: children that have not arrived
  unsigned long long* sub;       // [node_cap]: the sum of best over the children that have
  VcCondStat* stat;
};

// every lane of the wave calls; one atomic per wave
__device__ __forceinline__ void cd_count(bool take, unsigned long long* counter) {
  const uint64_t m = __ballot(take);
  if (m && vc_lane() == (uint32_t)__ffsll((long long)m) - 1u) atomicAdd(counter, (unsigned long long)__popcll(m));
}
__device__ __forceinline__ bool cd_claim(uint32_t* slot, uint32_t tag) { return atomicMax(slot, tag) < tag; }
// the position of end t & 1 of edge t >> 1 of the level
__device__ __forceinline__ uint32_t cd_end_pos(const CondArgs& a, uint32_t first, uint64_t t) {
  const vc_mst_edge& e = a.edges[(uint64_t)first + (t >> 1)];
  return ((t & 1u) ? e.b : e.a) - a.id_base;
}

__global__ void __launch_bounds__(VC_COND_BLOCK) vc_cond_init_kernel(const CondArgs a) {
  for (uint64_t i = (uint64_t)blockIdx.x * VC_COND_BLOCK + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * VC_COND_BLOCK) {
    a.forest[i] = a.comp[i] = a.id_base + (uint32_t)i;
    a.csize[i] = 1u;
    a.cnode[i] = a.decided[i] = a.own[i] = a.leave[i] = VC_COND_NONE;
    a.tot[i] = a.big[i] = a.small_sum[i] = a.claim_old[i] = a.claim_new[i] = 0u;
  }
}

// Nothing but the error word and first[] is written.  first[weight] is written only for a weight within the code width; in a list that
// ascends exactly one edge per weight writes it.
__global__ void __launch_bounds__(VC_COND_BLOCK) vc_cond_plan_kernel(const CondArgs a) {
  for (uint64_t t = (uint64_t)blockIdx.x * VC_COND_BLOCK + threadIdx.x; t < a.n_edges; t += (uint64_t)gridDim.x * VC_COND_BLOCK) {
    const uint32_t ea = a.edges[t].a, eb = a.edges[t].b, w = a.edges[t].weight;
    bool bad = (uint64_t)(uint32_t)(ea - a.id_base) >= a.n || (uint64_t)(uint32_t)(eb - a.id_base) >= a.n || ea == eb || w > a.bits;
    if (!bad) {
      const uint32_t before = t ? a.edges[t - 1].weight : VC_COND_NONE;
      if (t && before > w) bad = true;
      else if (!t || before != w) a.first[w] = (uint32_t)t;
      if (t + 1 == a.n_edges && !vc_cond_root_above(a.root_weight, w)) bad = true;
    }
    if (bad) a.stat->bad = 1u;
  }
}

__global__ void __launch_bounds__(VC_COND_BLOCK) vc_cond_unite_kernel(const CondArgs a, const uint32_t first, const uint32_t count) {
  for (uint32_t t = blockIdx.x * VC_COND_BLOCK + threadIdx.x; t < count; t += gridDim.x * VC_COND_BLOCK) {
    const vc_mst_edge& e = a.edges[(uint64_t)first + t];
    cl_unite(a.forest, a.id_base, e.a, e.b);
  }
}

// The forest stands still from here to the settle launch: a root found now is the level's new root.
__global__ void __launch_bounds__(VC_COND_BLOCK) vc_cond_tally_kernel(const CondArgs a, const uint32_t first, const uint32_t count, const uint32_t level) {
  for (uint64_t t = (uint64_t)blockIdx.x * VC_COND_BLOCK + threadIdx.x; t < 2ull * count; t += (uint64_t)gridDim.x * VC_COND_BLOCK) {
    const uint32_t old_root = a.comp[cd_end_pos(a, first, t)], o = old_root - a.id_base;
    if (!cd_claim(a.claim_old + o, vc_cond_tag_tally(level))) continue;
    const uint32_t r = cl_find_halving(a.forest, a.id_base, old_root) - a.id_base, size = a.csize[o];
    atomicAdd(a.tot + r, size);
    if (size >= a.mcs) atomicAdd(a.big + r, 1u);
    else atomicAdd(a.small_sum + r, size);
  }
}

// the node of a new component; NONE (and the error word) when the cursor has left the buffer, which no forest brings about
__device__ __forceinline__ uint32_t cd_new_node(const CondArgs& a, uint32_t weight, uint32_t size, uint32_t n_children) {
  const uint32_t at = atomicAdd(&a.stat->n_nodes, 1u);
  if (at >= a.node_cap) {
    a.stat->bad = 1u;
    return VC_COND_NONE;
  }
  a.work[at] = CdNode{VC_COND_NONE, 0u, weight, 0u, size, n_children, 0u, 0u, (unsigned long long)weight * size};
  return at;
}

__global__ void __launch_bounds__(VC_COND_BLOCK) vc_cond_decide_kernel(const CondArgs a, const uint32_t first, const uint32_t count, const uint32_t level,
                                                                      const uint32_t weight) {
  for (uint64_t t = (uint64_t)blockIdx.x * VC_COND_BLOCK + threadIdx.x; t < 2ull * count; t += (uint64_t)gridDim.x * VC_COND_BLOCK) {
    const uint32_t r = cl_find_halving(a.forest, a.id_base, a.comp[cd_end_pos(a, first, t)]) - a.id_base;
    if (!cd_claim(a.claim_new + r, vc_cond_tag_new(level))) continue;
    const uint32_t n_big = a.big[r], total = a.tot[r];
    uint32_t d = VC_COND_NONE;
    if (n_big >= 2) d = cd_new_node(a, weight, total, n_big);
    else if (n_big == 1) d = CD_GOES_ON;
    else if (total >= a.mcs) d = cd_new_node(a, weight, total, 0u);
    a.decided[r] = d;
  }
}

__global__ void __launch_bounds__(VC_COND_BLOCK) vc_cond_apply_kernel(const CondArgs a, const uint32_t first, const uint32_t count, const uint32_t level,
                                                                     const uint32_t weight) {
  for (uint64_t t = (uint64_t)blockIdx.x * VC_COND_BLOCK + threadIdx.x; t < 2ull * count; t += (uint64_t)gridDim.x * VC_COND_BLOCK) {
    const uint32_t old_root = a.comp[cd_end_pos(a, first, t)], o = old_root - a.id_base;
    if (atomicMax(a.claim_old + o, vc_cond_tag_apply(level)) != vc_cond_tag_tally(level)) continue;   // once, and only after this level's tally
    if (a.csize[o] < a.mcs) continue;
    const uint32_t c = a.cnode[o];
    if (c >= a.node_cap) continue;   // (a big component always carries a node)
    const uint32_t r = cl_find_halving(a.forest, a.id_base, old_root) - a.id_base;
    if (a.big[r] >= 2) {
      a.work[c].parent = a.decided[r];
      a.work[c].end = weight;
      a.work[c].rep = old_root;
    } else {   // the only big one: the same node goes on, grown by the small components
      const uint32_t grown = a.small_sum[r];
      a.work[c].size += grown;
      a.work[c].sum_leave += (unsigned long long)weight * grown;
      a.decided[r] = c;
    }
  }
}

__global__ void __launch_bounds__(VC_COND_BLOCK) vc_cond_settle_kernel(const CondArgs a, const uint32_t level, const uint32_t weight) {
  const uint32_t tag = vc_cond_tag_new(level);
  for (uint64_t i = (uint64_t)blockIdx.x * VC_COND_BLOCK + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * VC_COND_BLOCK) {
    const uint32_t me = a.id_base + (uint32_t)i, root = cl_find_halving(a.forest, a.id_base, me), r = root - a.id_base;
    cl_st(a.forest + i, root);   // an ancestor, as path halving stores one
    a.comp[i] = root;
    if (a.claim_new[r] != tag) continue;
    const uint32_t d = a.decided[r];
    if (d < a.node_cap && a.own[i] == VC_COND_NONE) {
      a.own[i] = d;
      a.leave[i] = weight;
    }
    if (root == me) {   // nobody else reads or writes these words of mine in this launch
      a.csize[i] = a.tot[i];
      a.cnode[i] = d < a.node_cap ? d : VC_COND_NONE;
      a.tot[i] = a.big[i] = a.small_sum[i] = 0u;
    }
  }
}

__global__ void __launch_bounds__(VC_COND_BLOCK) vc_cond_roots_kernel(const CondArgs a) {
  for (uint64_t i0 = (uint64_t)blockIdx.x * VC_COND_BLOCK; i0 < a.n; i0 += (uint64_t)gridDim.x * VC_COND_BLOCK) {   // (block-uniform bounds: every lane votes)
    const uint64_t i = i0 + threadIdx.x;
    const bool is_root = i < a.n && a.comp[i] == a.id_base + (uint32_t)i;
    bool live = false;
    if (is_root) {
      const uint32_t c = a.cnode[i];
      live = c < a.node_cap;
      if (live) {
        a.work[c].end = a.root_weight;
        a.work[c].rep = a.id_base + (uint32_t)i;
        a.work[c].root = 1u;
      }
    }
    cd_count(is_root, &a.stat->n_comp);
    cd_count(live, &a.stat->n_roots);
  }
}

__global__ void __launch_bounds__(VC_COND_BLOCK) vc_cond_keys_kernel(const CondArgs a, const uint32_t M, uint32_t* __restrict__ keys, uint64_t* __restrict__ vals) {
  for (uint32_t j = blockIdx.x * VC_COND_BLOCK + threadIdx.x; j < M; j += gridDim.x * VC_COND_BLOCK) {
    keys[j] = a.work[j].form;
    vals[j] = ((uint64_t)a.work[j].rep << 32) | j;
  }
}

__global__ void __launch_bounds__(VC_COND_BLOCK) vc_cond_rank_kernel(const CondArgs a, const uint32_t M, const uint64_t* __restrict__ vals) {
  for (uint32_t t = blockIdx.x * VC_COND_BLOCK + threadIdx.x; t < M; t += gridDim.x * VC_COND_BLOCK) {
    const uint32_t j = (uint32_t)vals[t];
    if (j < M) a.rank[j] = t;
  }
}

__global__ void __launch_bounds__(VC_COND_BLOCK) vc_cond_write_kernel(const CondArgs a, const uint32_t M, const uint64_t* __restrict__ vals,
                                                                     vc_condensed_node* __restrict__ out) {
  for (uint32_t t0 = blockIdx.x * VC_COND_BLOCK; t0 < M; t0 += gridDim.x * VC_COND_BLOCK) {   // (block-uniform)
    const uint32_t t = t0 + threadIdx.x;
    bool leaf = false;
    if (t < M) {
      const uint32_t j = min((uint32_t)vals[t], M - 1u);
      const CdNode w = a.work[j];
      const bool root = w.root != 0u;
      leaf = w.n_children == 0u;
      vc_condensed_node o;
      o.parent = w.parent < M ? a.rank[w.parent] : VC_COND_NONE;
      o.rep = w.rep; o.form = w.form; o.end = w.end; o.size = w.size; o.n_children = w.n_children;
      o.flags = root ? VC_COND_ROOT : 0u;
      o.pad = 0u;
      o.stability = vc_cond_stability(w.end, w.size, w.sum_leave, root, a.root_weight);
      o.best = 0ull;
      out[t] = o;
      a.pending[t] = w.n_children;
      a.sub[t] = 0ull;
      a.cand[t] = a.method == VC_COND_LEAF && leaf && vc_cond_allowed(root, a.root_weight) ? 1u : 0u;
    }
    cd_count(leaf, &a.stat->n_leaves);
  }
}

// A parent is served by the child whose decrement finds 1: every other child's add to sub[] came before its own decrement, and the
// fences order the two, so the sum read there is complete.  A node is visited once; the walk ends at a root or where a sibling is out.
__global__ void __launch_bounds__(VC_COND_BLOCK) vc_cond_fold_kernel(const CondArgs a, const uint32_t M, vc_condensed_node* out) {
  for (uint32_t t = blockIdx.x * VC_COND_BLOCK + threadIdx.x; t < M; t += gridDim.x * VC_COND_BLOCK) {
    if (out[t].n_children) continue;
    uint32_t c = t;
    unsigned long long below = 0ull;   // a leaf has nothing below
    for (uint32_t steps = 0; steps < M; ++steps) {
      const uint32_t flags = out[c].flags;
      const unsigned long long stability = out[c].stability;
      const bool keep = vc_cond_keep(stability, below, vc_cond_allowed((flags & VC_COND_ROOT) != 0u, a.root_weight));
      const unsigned long long best = keep ? stability : below;
      out[c].best = best;
      if (keep) {
        out[c].flags = flags | VC_COND_KEEP;
        if (a.method == VC_COND_EOM) a.cand[c] = 1u;
      }
      const uint32_t p = out[c].parent;
      if (p >= M) break;
      atomicAdd(a.sub + p, best);
      __threadfence();
      if (atomicSub(a.pending + p, 1u) != 1u) break;
      __threadfence();
      below = __hip_atomic_load(a.sub + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      c = p;
    }
  }
}

__global__ void __launch_bounds__(VC_COND_BLOCK) vc_cond_select_kernel(const CondArgs a, const uint32_t M, vc_condensed_node* out) {
  for (uint32_t t0 = blockIdx.x * VC_COND_BLOCK; t0 < M; t0 += gridDim.x * VC_COND_BLOCK) {   // (block-uniform)
    const uint32_t t = t0 + threadIdx.x;
    bool selected = false;
    if (t < M) {
      uint32_t top = VC_COND_NONE, c = t;
      for (uint32_t steps = 0; steps < M && c < M; ++steps) {   // (a parent's number is above its child's: the walk ends)
        if (a.cand[c]) top = c;
        c = out[c].parent;
      }
      a.sel_anc[t] = top;
      selected = top == t;
      if (selected) {
        out[t].flags |= VC_COND_SELECTED;   // the flags word is mine: the walks of the others read cand[] and the parents only
        atomicAdd(&a.stat->total_stability, (unsigned long long)out[t].stability);
      }
    }
    cd_count(selected, &a.stat->n_selected);
  }
}

__global__ void __launch_bounds__(VC_COND_BLOCK) vc_cond_label_kernel(const CondArgs a, const uint32_t M, const vc_condensed_node* __restrict__ nodes,
                                                                     uint32_t* __restrict__ labels, uint32_t* __restrict__ node, uint32_t* __restrict__ own,
                                                                     uint32_t* __restrict__ leave) {
  for (uint64_t i0 = (uint64_t)blockIdx.x * VC_COND_BLOCK; i0 < a.n; i0 += (uint64_t)gridDim.x * VC_COND_BLOCK) {   // (block-uniform)
    const uint64_t i = i0 + threadIdx.x;
    bool clustered = false;
    if (i < a.n) {
      const uint32_t j = a.own[i], mine = j < M ? a.rank[j] : VC_COND_NONE;
      const uint32_t sel = mine < M ? a.sel_anc[mine] : VC_COND_NONE;
      clustered = sel < M;
      labels[i] = clustered ? nodes[sel].rep : a.id_base + (uint32_t)i;
      if (node) node[i] = clustered ? sel : VC_COND_NONE;
      if (own) own[i] = mine;
      if (leave) leave[i] = mine < M ? a.leave[i] : VC_COND_NONE;
    }
    cd_count(clustered, &a.stat->n_clustered);
  }
}

uint32_t cond_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + VC_COND_BLOCK - 1) / VC_COND_BLOCK, 1), 256 * 8); }

}  // namespace

#define COND_HIP(call) VC_HIP_OR_FAIL("condensed tree", call)
#define COND_LAUNCH(kernel, items, ...)                                                                         \
  do {                                                                                                          \
    hipLaunchKernelGGL(kernel, dim3(cond_grid(items)), dim3(VC_COND_BLOCK), 0, s, __VA_ARGS__);                 \
    COND_HIP(hipGetLastError());                                                                                \
  } while (0)

int vc_mst_condense_run(const VcStoreView& v, const VcCondenseArgs& a, vc_mst_condense_stats* stats, hipStream_t s, std::string* err) {
  const uint64_t n = v.n;
  const uint32_t bits = 64 * v.W;
  if (n == 0) {
    if (stats) *stats = vc_mst_condense_stats{};
    return VC_OK;
  }
  // every buffer of the call, before the first launch
  const uint64_t cap = vc_cond_scratch_nodes(n);
  const size_t word4 = (size_t)vc_cond_words4(n), node4 = (size_t)vc_cond_words4(cap);
  VcCondStat* d_stat = (VcCondStat*)v.alloc(VC_COND_STAT, VC_COND_STAT_BYTES);
  uint32_t* d_first = (uint32_t*)v.alloc(VC_COND_PLAN, (size_t)vc_cond_plan_bytes(bits));
  uint8_t* d_work = (uint8_t*)v.alloc(VC_COND_WORK, (size_t)vc_cond_work_bytes(n));
  uint8_t* d_tree = (uint8_t*)v.alloc(VC_COND_TREE, (size_t)vc_cond_tree_bytes(n));
  uint8_t* d_sort = (uint8_t*)v.alloc(VC_COND_SORT, (size_t)vc_cond_sort_bytes(n));
  uint32_t* d_sort_work = (uint32_t*)v.alloc(VC_COND_SORT_WORK, vc_radix_sort_work_words(cap) * 4);
  if (!d_stat || !d_first || !d_work || !d_tree || !d_sort || !d_sort_work) return VC_ERR_NOMEM;
  CondArgs k{};
  k.edges = a.d_edges; k.n_edges = a.n_edges; k.n = n; k.id_base = v.id_base; k.bits = bits; k.mcs = a.min_cluster_size; k.root_weight = a.root_weight;
  k.method = a.method; k.node_cap = (uint32_t)vc_cond_node_cap(n);
  uint32_t** const per_record[VC_COND_RECORD_WORDS] = {&k.forest, &k.comp, &k.csize, &k.cnode, &k.tot, &k.big, &k.small_sum, &k.decided, &k.claim_old, &k.claim_new,
                                                      &k.own, &k.leave};
  for (uint32_t i = 0; i < VC_COND_RECORD_WORDS; ++i) *per_record[i] = (uint32_t*)(d_work + i * word4);
  k.first = d_first;
  k.sub = (unsigned long long*)d_tree; k.work = (CdNode*)(d_tree + cap * 8);
  uint8_t* const after_nodes = d_tree + cap * 8 + cap * VC_COND_WORK_NODE_BYTES;
  k.rank = (uint32_t*)after_nodes; k.sel_anc = (uint32_t*)(after_nodes + node4); k.cand = (uint32_t*)(after_nodes + 2 * node4);
  k.pending = (uint32_t*)(after_nodes + 3 * node4);
  k.stat = d_stat;
  uint64_t* sort_vals[2] = {(uint64_t*)d_sort, (uint64_t*)d_sort + cap};
  uint32_t* sort_keys[2] = {(uint32_t*)(d_sort + 2 * cap * 8), (uint32_t*)(d_sort + 2 * cap * 8 + node4)};
  // 1. the plan: every edge validated, the first edge of every weight.  THE FIRST WAIT: the table and the error word
  COND_HIP(hipMemsetAsync(d_stat, 0, VC_COND_STAT_BYTES, s));
  COND_HIP(hipMemsetAsync(d_first, 0xFF, ((size_t)bits + 1) * 4, s));
  std::vector<uint32_t> first((size_t)bits + 1, VC_COND_NONE);
  VcCondStat home{};
  if (a.n_edges) {
    COND_LAUNCH(vc_cond_plan_kernel, a.n_edges, k);
    COND_HIP(hipMemcpyAsync(first.data(), d_first, ((size_t)bits + 1) * 4, hipMemcpyDeviceToHost, s));
    COND_HIP(hipMemcpyAsync(&home, d_stat, VC_COND_STAT_BYTES, hipMemcpyDeviceToHost, s));
    COND_HIP(hipStreamSynchronize(s));
    if (home.bad) {
      if (err)
        *err = "condensed tree: an end outside the store, a == b, a weight above the code width, descending weights, or a root_weight that is not above the "
               "last weight";
      return VC_ERR_INVALID;
    }
  }
  std::vector<VcCondLevel> levels((size_t)bits + 1);
  const uint32_t n_levels = vc_cond_levels(first.data(), bits, a.n_edges, levels.data());
  // 2. the levels, no wait
  COND_LAUNCH(vc_cond_init_kernel, n, k);
  for (uint32_t l = 0; l < n_levels; ++l) {
    const VcCondLevel& L = levels[l];
    COND_LAUNCH(vc_cond_unite_kernel, L.count, k, L.first, L.count);
    COND_LAUNCH(vc_cond_tally_kernel, 2ull * L.count, k, L.first, L.count, l);
    COND_LAUNCH(vc_cond_decide_kernel, 2ull * L.count, k, L.first, L.count, l, L.weight);
    COND_LAUNCH(vc_cond_apply_kernel, 2ull * L.count, k, L.first, L.count, l, L.weight);
    COND_LAUNCH(vc_cond_settle_kernel, n, k, l, L.weight);
  }
  // 3. the roots.  THE SECOND WAIT: the number of nodes for the sort, the components for the cycle check
  COND_LAUNCH(vc_cond_roots_kernel, n, k);
  COND_HIP(hipMemcpyAsync(&home, d_stat, VC_COND_STAT_BYTES, hipMemcpyDeviceToHost, s));
  COND_HIP(hipStreamSynchronize(s));
  if (home.n_comp != n - a.n_edges) {
    if (err) *err = "condensed tree: the edges close a cycle -- not a forest over this store";
    return VC_ERR_INVALID;
  }
  if (home.bad || home.n_nodes > k.node_cap) {   // (no forest brings this about: the bound on the nodes is below the buffer's size)
    if (err) *err = "condensed tree: more nodes than a forest over this store can have";
    return VC_ERR_INVALID;
  }
  // 4. the order (form, rep), the tree in that order, the fold upwards, the selection, the labels
  const uint32_t M = home.n_nodes;
  if (M) {
    COND_LAUNCH(vc_cond_keys_kernel, M, k, M, sort_keys[0], sort_vals[0]);
    const uint32_t rep_bits = vc_cond_rep_bits(v.id_base, n), form_bits = vc_cond_form_bits(bits);
    COND_HIP(vc_radix_sort_items(sort_keys, sort_vals, M, rep_bits, form_bits, d_sort_work, s));
    const uint64_t* sorted = sort_vals[vc_radix_sort_item_passes(rep_bits, form_bits) & 1u];
    COND_LAUNCH(vc_cond_rank_kernel, M, k, M, sorted);
    COND_LAUNCH(vc_cond_write_kernel, M, k, M, sorted, a.d_nodes);
    COND_LAUNCH(vc_cond_fold_kernel, M, k, M, a.d_nodes);
    COND_LAUNCH(vc_cond_select_kernel, M, k, M, a.d_nodes);
  }
  COND_LAUNCH(vc_cond_label_kernel, n, k, M, (const vc_condensed_node*)a.d_nodes, a.d_labels, a.d_node, a.d_own, a.d_leave);
  // THE LAST WAIT: the statistics
  COND_HIP(hipMemcpyAsync(&home, d_stat, VC_COND_STAT_BYTES, hipMemcpyDeviceToHost, s));
  COND_HIP(hipStreamSynchronize(s));
  if (stats) *stats = vc_mst_condense_stats{M, home.n_leaves, home.n_roots, home.n_selected, home.n_clustered, n - home.n_clustered, home.total_stability, n_levels, 0u};
  return VC_OK;
}

int vc_mst_condense_run_host(const VcStoreView& v, VcCondenseArgs a, const vc_mst_edge* edges, vc_condensed_node* nodes, uint32_t* labels, uint32_t* node, uint32_t* own,
                             uint32_t* leave, vc_mst_condense_stats* stats, hipStream_t s, std::string* err) {
  const size_t n = (size_t)v.n;
  if (n == 0) {
    if (stats) *stats = vc_mst_condense_stats{};
    return VC_OK;
  }
  const VcCondStage L(n, a.n_edges);
  uint8_t* stage = (uint8_t*)v.alloc(VC_COND_STAGE, (size_t)L.total);
  if (!stage) return VC_ERR_NOMEM;
  vc_mst_edge* d_edges = (vc_mst_edge*)(stage + L.edges);
  if (a.n_edges) COND_HIP(hipMemcpyAsync(d_edges, edges, (size_t)a.n_edges * VC_COND_EDGE_BYTES, hipMemcpyHostToDevice, s));
  a.d_edges = d_edges;
  a.d_nodes = (vc_condensed_node*)(stage + L.nodes);
  a.d_labels = (uint32_t*)(stage + L.labels);
  a.d_node = node ? (uint32_t*)(stage + L.node) : nullptr;
  a.d_own = own ? (uint32_t*)(stage + L.own) : nullptr;
  a.d_leave = leave ? (uint32_t*)(stage + L.leave) : nullptr;
  vc_mst_condense_stats st{};
  const int rc = vc_mst_condense_run(v, a, &st, s, err);
  if (rc) return rc;
  if (stats) *stats = st;
  if (st.n_nodes) COND_HIP(hipMemcpyAsync(nodes, a.d_nodes, (size_t)st.n_nodes * VC_COND_NODE_BYTES, hipMemcpyDeviceToHost, s));
  COND_HIP(hipMemcpyAsync(labels, a.d_labels, n * 4, hipMemcpyDeviceToHost, s));
  if (node) COND_HIP(hipMemcpyAsync(node, a.d_node, n * 4, hipMemcpyDeviceToHost, s));
  if (own) COND_HIP(hipMemcpyAsync(own, a.d_own, n * 4, hipMemcpyDeviceToHost, s));
  if (leave) COND_HIP(hipMemcpyAsync(leave, a.d_leave, n * 4, hipMemcpyDeviceToHost, s));
  COND_HIP(hipStreamSynchronize(s));
  return VC_OK;
}
