// Host-side check of easydist_amd/ops/csrc/gemm_tn_map.h, built with the
// system C++ compiler by tests/test_gemm_tn_map.py (no HIP needed).
// Exits 0 when every property holds, 1 with a message on the first miss.
#include "gemm_tn_map.h"

#include <cstdio>
#include <set>
#include <utility>
#include <vector>

static int fail(const char* what, unsigned ntile, unsigned splitr, int mode) {
  std::printf("FAIL %s: ntile=%u splitr=%u mode=%d\n", what, ntile, splitr,
              mode);
  return 1;
}

// ids 0..ntile*splitr-1 hit every (tile, slice) pair exactly once
static bool bijective(unsigned ntile, unsigned splitr, int mode) {
  std::vector<char> seen(ntile * splitr, 0);
  for (unsigned L = 0; L < ntile * splitr; ++L) {
    TnBlock m = gemm_tn_map(L, ntile, splitr, mode);
    if (m.tile >= ntile || m.slice >= splitr) return false;
    char& s = seen[m.tile * splitr + m.slice];
    if (s) return false;
    s = 1;
  }
  return true;
}

// Distinct (A strip, slice) plus (B strip, slice) pairs, summed over the
// L % 8 groups: the strips each XCD has to fetch from beyond its L2 when
// its workgroups walk their slices in step.
static unsigned distinct_strips(unsigned nwg_p, unsigned nwg_q,
                                unsigned splitr, int mode) {
  const unsigned ntile = nwg_p * nwg_q;
  std::set<std::pair<unsigned, unsigned>> a[N_XCD], b[N_XCD];
  for (unsigned L = 0; L < ntile * splitr; ++L) {
    TnBlock m = gemm_tn_map(L, ntile, splitr, mode);
    a[L % N_XCD].insert({m.tile / nwg_q, m.slice});
    b[L % N_XCD].insert({m.tile % nwg_q, m.slice});
  }
  unsigned n = 0;
  for (int g = 0; g < N_XCD; ++g) n += (unsigned)(a[g].size() + b[g].size());
  return n;
}

int main() {
  long checked = 0;
  for (unsigned ntile = 1; ntile <= 40; ++ntile)
    for (unsigned splitr = 1; splitr <= 64; ++splitr) {
      for (int mode = 0; mode < 2; ++mode) {
        if (!bijective(ntile, splitr, mode))
          return fail("bijection", ntile, splitr, mode);
        ++checked;
      }
      for (unsigned L = 0; L < ntile * splitr; ++L) {
        // mode 0 is the arithmetic the kernels carried before the header
        unsigned wg = xcd_swizzle(L, ntile * splitr);
        TnBlock m0 = gemm_tn_map(L, ntile, splitr, TN_MAP_TILE_MAJOR);
        if (m0.tile != wg / splitr || m0.slice != wg % splitr)
          return fail("tile-major identity", ntile, splitr, 0);
        if (splitr != 1) continue;
        TnBlock m1 = gemm_tn_map(L, ntile, splitr, TN_MAP_SLICE_MAJOR);
        if (m1.tile != m0.tile || m1.slice != m0.slice)
          return fail("modes differ at splitr 1", ntile, splitr, 1);
      }
    }
  // the four per-layer dW shapes of the flagship step (R = 65536, 256x256
  // tiles, splitr = 256 / ntile): {nwg_p, nwg_q, splitr, tile-major count,
  // slice-major count}
  const unsigned shapes[4][5] = {
      {9, 3, 9, 345, 131},    // qkv  2304 x 768
      {3, 3, 28, 483, 189},   // proj  768 x 768
      {12, 3, 7, 284, 131},   // fc1  3072 x 768
      {3, 12, 7, 322, 174},   // fc2   768 x 3072
  };
  for (const unsigned* s : shapes) {
    unsigned d0 = distinct_strips(s[0], s[1], s[2], TN_MAP_TILE_MAJOR);
    unsigned d1 = distinct_strips(s[0], s[1], s[2], TN_MAP_SLICE_MAJOR);
    if (d0 != s[3] || d1 != s[4] || d1 > d0) {
      std::printf("FAIL strips at %ux%u tiles, splitr %u: tile-major %u "
                  "(want %u), slice-major %u (want %u)\n",
                  s[0], s[1], s[2], d0, s[3], d1, s[4]);
      return 1;
    }
  }
  std::printf("OK %ld bijection cases\n", checked);
  return 0;
}
