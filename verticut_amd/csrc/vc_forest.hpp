// The lock-free union-find forest over a label array, shared by vc_cluster.hip (every record a vertex) and vc_dbscan.hip (the cores).
// labels[] IS the forest, in place: slot i (record id_base + i) holds the GLOBAL id of the record's parent, a root holds its own id.
// Ids stay below 2^32, so unsigned compares on global ids are the order.  Three invariants hold after every single store:
//   (1) a parent never exceeds its child: parent(x) <= x, with equality exactly at a root;
//   (2) only a root's slot is CAS-ed, from "itself" to a smaller id -- a record that stopped being a root never becomes one again;
//   (3) path halving stores an ancestor of the same tree (the grandparent read a moment ago) into a slot that is no root.
// From (1): every chain strictly descends, so every walk ends and the forest is acyclic under any interleaving.  From (2) and (3):
// a store moves a subtree below a smaller record of a tree it is, or becomes, part of -- trees merge and never split, and two records
// are in one tree exactly when the unions made so far connect them.  From (1) again: the root of a tree is its smallest id.
// Slots are read and written with relaxed device-scope atomics (no stale line of a CU's L1 is ever walked), hooked with atomicCAS.
#pragma once
#include "vc_common.hpp"

__device__ __forceinline__ uint32_t cl_ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cl_st(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of global id x, halving the path on the way: x's slot gets its grandparent, the walk goes on from there
__device__ __forceinline__ uint32_t cl_find_halving(uint32_t* labels, uint32_t id_base, uint32_t x) {
  uint32_t p = cl_ld(labels + (x - id_base));
  while (p != x) {
    const uint32_t gp = cl_ld(labels + (p - id_base));
    if (gp == p) return p;
    cl_st(labels + (x - id_base), gp);   // (3): x is no root (p < x), gp <= p is an ancestor of x
    x = gp;
    p = cl_ld(labels + (x - id_base));
  }
  return x;
}

// the root of x by reads alone
__device__ __forceinline__ uint32_t cl_find(const uint32_t* labels, uint32_t id_base, uint32_t x) {
  for (;;) {
    const uint32_t p = cl_ld(labels + (x - id_base));
    if (p == x) return x;
    x = p;
  }
}

// the trees of the global ids a and b made one
__device__ __forceinline__ void cl_unite(uint32_t* labels, uint32_t id_base, uint32_t a, uint32_t b) {
  for (;;) {
    a = cl_find_halving(labels, id_base, a);
    b = cl_find_halving(labels, id_base, b);
    if (a == b) break;
    const uint32_t big = a > b ? a : b, small = a > b ? b : a;
    // (2): hook the LARGER root under the smaller, on the larger root's own slot, expecting it to be a root still.  `small`
    // may have stopped being a root meanwhile: it is smaller all the same, (1) holds, and the trees are merged.
    if (atomicCAS(labels + (big - id_base), big, small) == big) break;
    // somebody else hooked `big`: that is progress of the whole; find again from the two records reached
  }
}
