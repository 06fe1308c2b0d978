// Workgroup-id -> (block, head) maps shared by the host and the kernels.
//
// Plain C++: a host compiler builds this header without HIP (the CPU test
// tests/csrc/attn_block_map_check.cpp does), hipcc builds it for both sides.
//
// Workgroups are observed to be dealt round-robin over the 8 XCDs by their
// linear id, so ids that agree in `L % 8` share an XCD (and its L2).  That
// is a SPEED property only: HIP promises no dispatch order or placement,
// and every map here is a bijection, so results never depend on it.
#pragma once

#ifdef __HIPCC__
#define ED_MAP_HD __host__ __device__ __forceinline__
#else
#define ED_MAP_HD inline
#endif

#define N_XCD 8

// bijective XCD-aware workgroup remap (cdna_hip_programming.md T1): the
// ids with `wg % 8 == x` receive one contiguous run of the result
ED_MAP_HD unsigned xcd_swizzle(unsigned wg, unsigned nwg) {
  unsigned q = nwg / N_XCD, r = nwg % N_XCD;
  unsigned xcd = wg % N_XCD, idx = wg / N_XCD;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

#define ATTN_MAP_LEGACY 0    // (L % nblk, L / nblk): the old 2-D grid
#define ATTN_MAP_BALANCED 1  // whole heads per XCD group, heavy block first

struct AttnBlock {
  int blk;   // q block (fwd, dq) or kv block (dkv) within the head
  int bh;    // batch * H + head
};

// Map linear workgroup id L of a 1-D grid of nblk * nbh workgroups.
//
// Causal work per block grows with the block index in fwd and dq (block x
// walks x+1 kv steps) and shrinks with it in dkv.  With the legacy map and
// nblk == 8 every block of one index lands on the same XCD, so one XCD
// gets all the longest blocks and the rest idle behind it.  The balanced
// map hands each `L % 8` group a contiguous run of whole heads: equal
// causal work per group whenever nbh % 8 == 0, and all blocks of a head
// share one L2 for the operands they all stream.  Within a head the heavy
// block goes first so the kernel's tail is made of short blocks;
// heavy_last_index says the heavy block is nblk-1 (fwd/dq under a causal
// mask) rather than 0 (dkv, or no mask: order is then irrelevant).
ED_MAP_HD AttnBlock attn_block_map(unsigned L, unsigned nblk, unsigned nbh,
                                   bool heavy_last_index, int mode) {
  AttnBlock r;
  if (mode == ATTN_MAP_LEGACY) {
    r.blk = (int)(L % nblk);
    r.bh = (int)(L / nblk);
    return r;
  }
  unsigned w = xcd_swizzle(L, nblk * nbh);
  unsigned o = w % nblk;
  r.bh = (int)(w / nblk);
  r.blk = (int)(heavy_last_index ? nblk - 1 - o : o);
  return r;
}
