// Host-side check of easydist_amd/ops/csrc/attn_block_map.h, built with the
// system C++ compiler by tests/test_attn_block_map.py (no HIP needed).
// Exits 0 when every property holds, 1 with a message on the first miss.
#include "attn_block_map.h"

#include <cstdio>
#include <vector>

static int fail(const char* what, unsigned nblk, unsigned nbh, int mode,
                int heavy_last) {
  std::printf("FAIL %s: nblk=%u nbh=%u mode=%d heavy_last_index=%d\n", what,
              nblk, nbh, mode, heavy_last);
  return 1;
}

// ids 0..nblk*nbh-1 hit every (blk, bh) pair exactly once
static bool bijective(unsigned nblk, unsigned nbh, int mode, bool heavy_last) {
  std::vector<char> seen(nblk * nbh, 0);
  for (unsigned L = 0; L < nblk * nbh; ++L) {
    AttnBlock m = attn_block_map(L, nblk, nbh, heavy_last, mode);
    if (m.blk < 0 || m.bh < 0 || (unsigned)m.blk >= nblk ||
        (unsigned)m.bh >= nbh)
      return false;
    char& s = seen[(unsigned)m.bh * nblk + (unsigned)m.blk];
    if (s) return false;
    s = 1;
  }
  return true;
}

// summed causal weight (blk + 1) of each L % 8 group
static void group_weights(unsigned nblk, unsigned nbh, int mode,
                          bool heavy_last, unsigned long w[N_XCD]) {
  for (int g = 0; g < N_XCD; ++g) w[g] = 0;
  for (unsigned L = 0; L < nblk * nbh; ++L)
    w[L % N_XCD] += attn_block_map(L, nblk, nbh, heavy_last, mode).blk + 1;
}

// every block of a head sits in one L % 8 group
static bool head_local(unsigned nblk, unsigned nbh, int mode, bool heavy_last) {
  std::vector<int> grp(nbh, -1);
  for (unsigned L = 0; L < nblk * nbh; ++L) {
    AttnBlock m = attn_block_map(L, nblk, nbh, heavy_last, mode);
    int g = (int)(L % N_XCD);
    if (grp[m.bh] < 0) grp[m.bh] = g;
    else if (grp[m.bh] != g) return false;
  }
  return true;
}

int main() {
  const int modes[2] = {ATTN_MAP_LEGACY, ATTN_MAP_BALANCED};
  long checked = 0;
  for (int mi = 0; mi < 2; ++mi)
    for (int hl = 0; hl < 2; ++hl) {
      const int mode = modes[mi];
      // bijection, exhaustively over the small sizes
      for (unsigned nblk = 1; nblk <= 40; ++nblk)
        for (unsigned nbh = 1; nbh <= 70; ++nbh) {
          if (!bijective(nblk, nbh, mode, hl))
            return fail("bijection", nblk, nbh, mode, hl);
          ++checked;
        }
      // legacy is exactly the old 2-D grid, whatever the flag
      if (mode == ATTN_MAP_LEGACY)
        for (unsigned nblk = 1; nblk <= 40; ++nblk)
          for (unsigned nbh = 1; nbh <= 70; ++nbh)
            for (unsigned L = 0; L < nblk * nbh; ++L) {
              AttnBlock m = attn_block_map(L, nblk, nbh, hl, mode);
              if ((unsigned)m.blk != L % nblk || (unsigned)m.bh != L / nblk)
                return fail("legacy identity", nblk, nbh, mode, hl);
            }
      // balance and locality at the sizes the kernels run at
      const unsigned nblks[3] = {8, 16, 24};
      const unsigned nbhs[4] = {8, 96, 256, 768};
      for (unsigned nblk : nblks)
        for (unsigned nbh : nbhs) {
          if (!bijective(nblk, nbh, mode, hl))
            return fail("bijection (large)", nblk, nbh, mode, hl);
          if (mode != ATTN_MAP_BALANCED) continue;
          unsigned long w[N_XCD];
          group_weights(nblk, nbh, mode, hl, w);
          for (int g = 1; g < N_XCD; ++g)
            if (w[g] != w[0]) return fail("balance", nblk, nbh, mode, hl);
          if (!head_local(nblk, nbh, mode, hl))
            return fail("locality", nblk, nbh, mode, hl);
        }
    }
  // the case the balanced map exists for: legacy at (8, 768) loads the
  // heaviest group with 16/9 of the mean.  max/mean == 16/9 exactly:
  // 9 * max * 8 == 16 * total.
  {
    unsigned long w[N_XCD], tot = 0, mx = 0;
    group_weights(8, 768, ATTN_MAP_LEGACY, true, w);
    for (int g = 0; g < N_XCD; ++g) {
      tot += w[g];
      if (w[g] > mx) mx = w[g];
    }
    if (9 * mx * N_XCD != 16 * tot) {
      std::printf("FAIL legacy imbalance at (8,768): max=%lu total=%lu\n", mx,
                  tot);
      return 1;
    }
  }
  // xcd_swizzle keeps each L % 8 group on one contiguous run of results
  for (unsigned n = 1; n <= 300; ++n)
    for (unsigned L = 0; L + N_XCD < n; ++L)
      if (xcd_swizzle(L + N_XCD, n) != xcd_swizzle(L, n) + 1) {
        std::printf("FAIL swizzle contiguity: n=%u L=%u\n", n, L);
        return 1;
      }
  std::printf("OK %ld bijection cases\n", checked);
  return 0;
}
