// attn_block_map at the block counts of the 64-key dkv geometry, built by
// tests/test_attn_block_map_geom.py with the system C++ compiler.  Reuses
// the predicates of attn_block_map_check.cpp (its main is renamed away) on
// (nblk, nbh) pairs from the command line: nblk nbh nblk nbh ...
//
// For every pair, both modes and both heavy_last_index settings: bijection.
// In balanced mode with heavy_last_index = false (dkv) also: ids of one
// L % 8 group that follow each other walk a head's blocks in ascending
// order (block 0, the causal-heavy one, first); and, when nbh % 8 == 0,
// equal causal weight per group and all blocks of a head in one group.
#define main attn_block_map_check_main
#include "attn_block_map_check.cpp"
#undef main

#include <cstdlib>

int main(int argc, char** argv) {
  if (argc < 3 || argc % 2 != 1) {
    std::printf("usage: %s nblk nbh [nblk nbh ...]\n", argv[0]);
    return 2;
  }
  const int modes[2] = {ATTN_MAP_LEGACY, ATTN_MAP_BALANCED};
  int pairs = 0;
  for (int a = 1; a + 1 < argc; a += 2, ++pairs) {
    const unsigned nblk = (unsigned)std::atoi(argv[a]);
    const unsigned nbh = (unsigned)std::atoi(argv[a + 1]);
    if (nblk == 0 || nbh == 0) return fail("arguments", nblk, nbh, -1, -1);
    for (int mi = 0; mi < 2; ++mi)
      for (int hl = 0; hl < 2; ++hl)
        if (!bijective(nblk, nbh, modes[mi], hl))
          return fail("bijection", nblk, nbh, modes[mi], hl);
    const int mode = ATTN_MAP_BALANCED;
    for (unsigned L = 0; L + N_XCD < nblk * nbh; ++L) {
      AttnBlock m0 = attn_block_map(L, nblk, nbh, false, mode);
      AttnBlock m1 = attn_block_map(L + N_XCD, nblk, nbh, false, mode);
      const bool next_blk = m1.bh == m0.bh && m1.blk == m0.blk + 1;
      const bool next_head = m1.bh == m0.bh + 1 && m1.blk == 0 &&
                             (unsigned)m0.blk == nblk - 1;
      if (!next_blk && !next_head)
        return fail("heavy-first order", nblk, nbh, mode, 0);
    }
    if (nbh % N_XCD == 0) {
      unsigned long w[N_XCD];
      group_weights(nblk, nbh, mode, false, w);
      for (int g = 1; g < N_XCD; ++g)
        if (w[g] != w[0]) return fail("balance", nblk, nbh, mode, 0);
      if (!head_local(nblk, nbh, mode, false))
        return fail("locality", nblk, nbh, mode, 0);
    }
  }
  std::printf("OK %d pairs\n", pairs);
  return 0;
}
