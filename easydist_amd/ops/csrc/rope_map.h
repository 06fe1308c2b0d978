// Work-item -> (row, head, vector pair) map of the RoPE kernel, shared by
// the host and the kernel.
//
// Plain C++: a host compiler builds this header without HIP (the CPU test
// tests/csrc/rope_map_check.cpp does), hipcc builds it for both sides.
//
// The packed qkv row [q | k | v] of W = (H + 2*Hkv)*D columns is cut into
// units of two 8-element vectors: for head h and j < D/16 the `lo` vector
// at column h*D + 8*j and the `hi` vector D/2 further on.  A q or k unit is
// one rotation (the two vectors are exactly the pairs the rotate-half
// convention mixes); a v unit is a copy of the same two vectors.  A row has
// U = (H + 2*Hkv) * (D/16) units, and the flat item index is row * U + unit.
#pragma once

#ifdef __HIPCC__
#define ED_ROPE_HD __host__ __device__ __forceinline__
#else
#define ED_ROPE_HD inline
#endif

#define ROPE_BLOCK 256   // threads per block = items per block pass

struct RopeShape {
  long n_rows;     // B * S
  long stride_b;   // input strides in elements; the output is contiguous
  long stride_s;
  int S;
  int D;
  int W;           // (H + 2*Hkv) * D
  int U;           // units per row: W / 16
  int VH;          // units per head: D / 16
  int rot_units;   // units of the q and k heads: (H + Hkv) * VH
};

struct RopeItem {
  long in_lo;      // element offset of the lo vector in the input
  long out_lo;     // ... and in the output; hi is D/2 elements further on
  long tab;        // element offset of the 8 cos / sin values
  bool valid;      // false past the last row
  bool rotate;     // false on the v columns: copy
};

// Item `base + tid` of a block pass that starts at item `base`
// (base = pass * ROPE_BLOCK, the same for the whole block, tid < ROPE_BLOCK).
// The two 64-bit divisions depend on `base` alone, so they are uniform over
// the block; what depends on the thread stays in 32 bits: rem + tid
// < U + ROPE_BLOCK and s0 + dr < S + ROPE_BLOCK + 1.
ED_ROPE_HD RopeItem rope_item(unsigned long base, unsigned tid,
                              const RopeShape& p) {
  const unsigned long row0 = base / (unsigned)p.U;
  const unsigned rem0 = (unsigned)(base - row0 * (unsigned)p.U);
  const unsigned long b0 = row0 / (unsigned)p.S;
  const unsigned s0 = (unsigned)(row0 - b0 * (unsigned)p.S);

  const unsigned r = rem0 + tid;
  const unsigned dr = r / (unsigned)p.U;
  const unsigned u = r - dr * (unsigned)p.U;
  const unsigned sq = s0 + dr;
  const unsigned db = sq / (unsigned)p.S;
  const unsigned s = sq - db * (unsigned)p.S;
  const unsigned head = u / (unsigned)p.VH;
  const unsigned j = u - head * (unsigned)p.VH;
  const unsigned col = head * (unsigned)p.D + j * 8u;

  const long row = (long)row0 + dr;
  RopeItem it;
  it.valid = row < p.n_rows;
  it.rotate = u < (unsigned)p.rot_units;
  it.in_lo = ((long)b0 + db) * p.stride_b + (long)s * p.stride_s + col;
  it.out_lo = row * p.W + col;
  it.tab = (long)s * (p.D / 2) + j * 8u;
  return it;
}
