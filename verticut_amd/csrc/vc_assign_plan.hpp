// Plan arithmetic of vc_assign_nearest* / vc_kmajority* (vc_assign.hip): records per thread, the grid, the centre tile, the centre
// slices and their bounds.  Plain C++ with no HIP in it, so that tests/cpp/assign_plan_test.cc checks it on the CPU; the kernel and
// its launcher call exactly these functions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VC_AP_FN __host__ __device__ inline
#else
#define VC_AP_FN inline
#endif

#define VC_ASSIGN_BLOCK 256u          // threads per block of vc_assign_kernel
#define VC_ASSIGN_LDS_WORDS 2048u     // 64-bit words of the staged centre tile: 16 KiB, so four blocks share a CU's LDS with room to spare
#define VC_ASSIGN_SLICES_MAX 1024u    // grid.y at most (VC_ASSIGN_SLICES above it is cut to it)
#define VC_ASSIGN_WAVES_PER_CU 8u     // the grid the plan wants before it stops cutting the centres: blocks * 4 waves >= CUs * this

// Records a thread keeps in registers for the whole launch: R x W 64-bit words = 16 VGPRs at every width but 512 bits (32), so even
// W = 8 with its 16 registers of centre words stays far from a spill.
VC_AP_FN constexpr uint32_t vc_assign_records(uint32_t W) { return W <= 1 ? 8u : W == 2 ? 4u : 2u; }
VC_AP_FN constexpr uint32_t vc_assign_block_records(uint32_t W) { return VC_ASSIGN_BLOCK * vc_assign_records(W); }
// Block b owns the records [b * block_records, ...); its thread t owns b * block_records + r * VC_ASSIGN_BLOCK + t, r < R: the 64
// lanes of a wave read 64 consecutive words of a column.
VC_AP_FN uint64_t vc_assign_record_of(uint32_t W, uint64_t block, uint32_t thread, uint32_t r) {
  return block * vc_assign_block_records(W) + (uint64_t)r * VC_ASSIGN_BLOCK + thread;
}
// Centres per LDS tile: all that fit by default; VC_ASSIGN_TILE (knob_tile != 0) lowers it, a value above the capacity is cut to it.
VC_AP_FN uint32_t vc_assign_tile_max(uint32_t W) { return VC_ASSIGN_LDS_WORDS / W; }
VC_AP_FN uint32_t vc_assign_tile(uint32_t W, uint32_t knob_tile) {
  const uint32_t cap = vc_assign_tile_max(W);
  return knob_tile == 0 || knob_tile > cap ? cap : knob_tile;
}

struct VcAssignPlan {
  uint32_t W, R, tile;
  uint64_t blocks;      // grid.x: ceil(count / block_records); 0 for count == 0 (nothing is launched)
  uint32_t slices;      // grid.y = S >= 1: S > 1 means an init launch and a 64-bit atomicMin per record and slice
  uint32_t per_slice;   // centres per slice; slice s holds [s * per_slice, min(K, (s + 1) * per_slice)), never empty
};
// slice s of per_slice centres each holds the centres [lo, hi); tile t0 of a slice holds min(tile, hi - t0) centres from t0 on
VC_AP_FN uint64_t vc_assign_slice_lo(uint32_t per_slice, uint32_t s) { return (uint64_t)s * per_slice; }
VC_AP_FN uint64_t vc_assign_slice_hi(uint32_t per_slice, uint32_t K, uint32_t s) {
  const uint64_t hi = ((uint64_t)s + 1) * per_slice;
  return hi < K ? hi : K;
}
VC_AP_FN uint32_t vc_assign_tile_centres(uint64_t t0, uint64_t hi, uint32_t tile) { return hi - t0 < tile ? (uint32_t)(hi - t0) : tile; }
// count records against K >= 1 centres of W words on a device of n_cu CUs.  Slices: as many as it takes to give the device
// VC_ASSIGN_WAVES_PER_CU waves per CU, but no slice below one full tile (a smaller one stages as often as it computes);
// VC_ASSIGN_SLICES (knob_slices != 0) forces the number.  In either case S <= K and S <= VC_ASSIGN_SLICES_MAX, and the slices are
// then made equal, so none is empty.
VC_AP_FN VcAssignPlan vc_assign_plan(uint64_t count, uint32_t K, uint32_t W, uint32_t n_cu, uint32_t knob_tile, uint32_t knob_slices) {
  VcAssignPlan p;
  p.W = W;
  p.R = vc_assign_records(W);
  p.tile = vc_assign_tile(W, knob_tile);
  const uint64_t br = vc_assign_block_records(W);
  p.blocks = (count + br - 1) / br;
  uint64_t S = 1;
  if (knob_slices) {
    S = knob_slices;
  } else if (p.blocks) {
    const uint64_t want_blocks = ((uint64_t)(n_cu ? n_cu : 1) * VC_ASSIGN_WAVES_PER_CU + 3) / 4;   // (a block is four waves)
    const uint64_t by_grid = (want_blocks + p.blocks - 1) / p.blocks, by_tiles = K / p.tile;
    S = by_grid < by_tiles ? by_grid : by_tiles;
  }
  if (S > VC_ASSIGN_SLICES_MAX) S = VC_ASSIGN_SLICES_MAX;
  if (S > K) S = K;
  if (S < 1) S = 1;
  p.per_slice = K ? (uint32_t)((K + S - 1) / S) : 1u;
  p.slices = K ? (uint32_t)(((uint64_t)K + p.per_slice - 1) / p.per_slice) : 1u;   // (K = 5, S = 4: per_slice 2 -> 3 slices, none empty)
  return p;
}
