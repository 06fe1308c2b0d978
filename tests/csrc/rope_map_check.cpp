// Host-side check of easydist_amd/ops/csrc/rope_map.h, built with the
// system C++ compiler by tests/test_rope_map.py (no HIP needed).
// Exits 0 when every property holds, 1 with a message on the first miss.
//
// For each shape every item of every block pass is decoded and compared with
// the plain 64-bit decode of its flat index; the two 16-byte vectors of an
// item must lie inside the input's span and the output, the 8 table values
// inside the table, and (small shapes) the valid items must write every
// output vector exactly once.  The large shapes have more than 2^31 elements
// and are sampled: the first, last and some middle passes.
#include "rope_map.h"

#include <cstdio>
#include <vector>

struct Case {
  long B, S, H, Hkv, D;
  long pad_s;   // extra elements per row of the input buffer
  long mul_b;   // batch stride multiplier (2 = every other batch entry)
};

static RopeShape shape_of(const Case& c) {
  RopeShape p;
  p.n_rows = c.B * c.S;
  p.S = (int)c.S;
  p.D = (int)c.D;
  p.W = (int)((c.H + 2 * c.Hkv) * c.D);
  p.U = p.W / 16;
  p.VH = p.D / 16;
  p.rot_units = (int)((c.H + c.Hkv) * (c.D / 16));
  p.stride_s = p.W + c.pad_s;
  p.stride_b = c.S * p.stride_s * c.mul_b;
  return p;
}

static int fail(const char* what, const Case& c, unsigned long item) {
  std::printf("FAIL %s: B=%ld S=%ld H=%ld Hkv=%ld D=%ld pad=%ld mul=%ld "
              "item=%lu\n", what, c.B, c.S, c.H, c.Hkv, c.D, c.pad_s, c.mul_b,
              item);
  return 1;
}

// one block pass; returns nonzero on the first miss
static int check_pass(const Case& c, const RopeShape& p, unsigned long base,
                      std::vector<char>* seen, long* n_valid) {
  const unsigned long n_items = (unsigned long)p.n_rows * (unsigned long)p.U;
  const long in_span = (c.B - 1) * p.stride_b + (c.S - 1) * p.stride_s + p.W;
  const long out_span = p.n_rows * p.W;
  const long tab_span = c.S * (c.D / 2);
  for (unsigned tid = 0; tid < ROPE_BLOCK; ++tid) {
    const unsigned long item = base + tid;
    const RopeItem it = rope_item(base, tid, p);
    if (it.valid != (item < n_items)) return fail("valid", c, item);
    if (!it.valid) continue;
    ++*n_valid;
    // reference decode in 64 bits
    const long row = (long)(item / (unsigned long)p.U);
    const long u = (long)(item % (unsigned long)p.U);
    const long b = row / c.S, s = row % c.S;
    const long head = u / p.VH, j = u % p.VH;
    const long col = head * c.D + j * 8;
    if (it.rotate != (head < c.H + c.Hkv)) return fail("rotate", c, item);
    if (it.in_lo != b * p.stride_b + s * p.stride_s + col)
      return fail("in_lo", c, item);
    if (it.out_lo != row * p.W + col) return fail("out_lo", c, item);
    if (it.tab != s * (c.D / 2) + j * 8) return fail("tab", c, item);
    // bounds of what the kernel touches: [lo, lo+8) and [lo+D/2, lo+D/2+8)
    if (it.in_lo < 0 || it.in_lo + c.D / 2 + 8 > in_span)
      return fail("input bounds", c, item);
    if (it.out_lo < 0 || it.out_lo + c.D / 2 + 8 > out_span)
      return fail("output bounds", c, item);
    if (it.tab < 0 || it.tab + 8 > tab_span)
      return fail("table bounds", c, item);
    if (it.in_lo % 8 || it.out_lo % 8 || it.tab % 8 || (c.D / 2) % 8)
      return fail("alignment", c, item);
    // lo and hi stay inside one head, and on the same side of it
    if (col % c.D + 8 > c.D / 2) return fail("half", c, item);
    if (seen) {
      char& a = (*seen)[it.out_lo / 8];
      char& h = (*seen)[(it.out_lo + c.D / 2) / 8];
      if (a || h) return fail("written twice", c, item);
      a = h = 1;
    }
  }
  return 0;
}

int main() {
  const Case small[] = {
      {1, 1, 1, 1, 64, 0, 1},    {2, 5, 4, 2, 64, 0, 1},
      {1, 130, 3, 1, 128, 0, 1}, {2, 7, 2, 2, 48, 0, 1},
      {1, 5000, 2, 1, 64, 0, 1}, {1, 3, 1, 1, 256, 0, 1},
      {2, 5, 4, 2, 64, 64, 1},   {2, 5, 4, 2, 64, 0, 2},
      {3, 2, 1, 1, 16, 8, 3},    {5, 1, 7, 7, 16, 0, 1},
      {300, 1, 1, 1, 16, 0, 1},  {2, 300, 1, 1, 16, 0, 1},
      {4, 33, 12, 12, 64, 0, 1}, {2, 17, 32, 8, 128, 0, 1},
  };
  long checked = 0;
  for (const Case& c : small) {
    const RopeShape p = shape_of(c);
    const unsigned long n_items = (unsigned long)p.n_rows * (unsigned long)p.U;
    std::vector<char> seen((size_t)(p.n_rows * p.W / 8), 0);
    long n_valid = 0;
    for (unsigned long base = 0; base < n_items; base += ROPE_BLOCK)
      if (check_pass(c, p, base, &seen, &n_valid)) return 1;
    if ((unsigned long)n_valid != n_items) return fail("item count", c, 0);
    for (char s : seen)
      if (!s) return fail("vector not written", c, 0);
    checked += n_valid;
  }
  // more than 2^31 elements: offsets must not wrap
  const Case large[] = {
      {128, 4096, 32, 8, 128, 0, 1},   // 3.2e9 elements
      {64, 1024, 12, 12, 64, 0, 1},    // GPT-2 small at batch 64
      {1, 3000000, 4, 4, 128, 64, 1},  // long sequence, padded rows
      {40000, 1, 255, 1, 256, 0, 2},   // U = 4112 and S = 1
  };
  for (const Case& c : large) {
    const RopeShape p = shape_of(c);
    const unsigned long n_items = (unsigned long)p.n_rows * (unsigned long)p.U;
    const unsigned long n_pass = (n_items + ROPE_BLOCK - 1) / ROPE_BLOCK;
    long n_valid = 0;
    for (unsigned long k = 0; k < 4096; ++k) {
      unsigned long pass = k < 1024 ? k
          : k < 2048 ? n_pass - 1 - (k - 1024)
                     : (n_pass / 2048) * (k - 2048) + (k * 2654435761UL) % 97;
      if (pass >= n_pass) continue;
      if (check_pass(c, p, pass * ROPE_BLOCK, nullptr, &n_valid)) return 1;
    }
    checked += n_valid;
  }
  std::printf("OK %ld items checked\n", checked);
  return 0;
}
