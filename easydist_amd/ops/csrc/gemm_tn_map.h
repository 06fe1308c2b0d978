// Workgroup-id -> (output tile, R slice) map of the split-R TN GEMMs,
// shared by the host and the kernels the way attn_block_map.h is.
//
// Plain C++: a host compiler builds this header without HIP (the CPU test
// tests/csrc/gemm_tn_map_check.cpp does), hipcc builds it for both sides.
// Placement is a SPEED property only (see attn_block_map.h): both modes are
// bijections, so results never depend on it.
#pragma once

#include "attn_block_map.h"   // ED_MAP_HD, N_XCD, xcd_swizzle

#define TN_MAP_TILE_MAJOR 0   // tile = w / splitr, slice = w % splitr (old)
#define TN_MAP_SLICE_MAJOR 1  // slice = w / ntile, tile = w % ntile

struct TnBlock {
  unsigned tile;    // p-major output tile: p-row = tile / nwg_q
  unsigned slice;   // R slice, 0..splitr-1
};

// Map linear workgroup id L of a 1-D grid of ntile * splitr workgroups.
//
// Two workgroups read the same operand bytes only when they work on the
// same slice AND share a p-row (the A strip) or a q-column (the B strip);
// different slices of one tile share nothing.  xcd_swizzle hands each XCD
// one contiguous run of w.  Tile-major decoding fills that run with a few
// tiles and ALL of their slices: mostly disjoint streams through one L2.
// Slice-major decoding fills it with (nearly) all tiles of one or a few
// slices, which are co-resident and walk r in step, so each strip is
// fetched from beyond the L2 about once per XCD and served from it to the
// other tiles of its row / column.
//
// Within a slice the tiles keep their p-major order, so where a run cuts a
// slice it cuts it into whole p-rows as far as possible: the neighbours of
// a tile in the run share its A strip, and the run still touches every
// q-column it would touch anyway.  With splitr == 1 both modes are w -> w.
ED_MAP_HD TnBlock gemm_tn_map(unsigned L, unsigned ntile, unsigned splitr,
                              int mode) {
  unsigned w = xcd_swizzle(L, ntile * splitr);
  TnBlock r;
  if (mode == TN_MAP_TILE_MAJOR) {
    r.tile = w / splitr;
    r.slice = w % splitr;
  } else {
    r.slice = w / ntile;
    r.tile = w % ntile;
  }
  return r;
}
