// Rotary position embeddings on the packed qkv projection output (gfx950).
//
// qkv is bf16 [B, S, W], W = (H + 2*Hkv)*D, columns [q | k | v]: the layout
// the attention kernels read through the split/view/transpose views and the
// packed attention backward writes.  Rotate-half convention: for every q and
// k head h and j < D/2, with lo = x[h*D + j], hi = x[h*D + D/2 + j],
// c = cos[s, j], t = sin[s, j]
//
//     out_lo = lo*c - hi*t        out_hi = hi*c + lo*t
//
// in fp32, rounded to bf16 once.  inverse uses -t: the transpose of the
// rotation, which is its backward.  The v columns are copied bit for bit.
//
// One memory-bound pass, no LDS, no atomics.  A thread owns one unit of
// rope_map.h: it loads the lo and hi vectors (16 B each), the matching 8 cos
// and 8 sin values (fp32, 2 x 16 B each) and stores two 16 B vectors; v
// units skip the tables.  The tables are S*D/2*4 bytes (128 KB at S = 1024,
// D = 64) re-read by every head and batch entry, so they stay in cache and
// HBM sees a copy's traffic.  The input is read through its batch and row
// strides (a slice of a wider buffer costs no copy); the output is a new
// contiguous tensor.  Blocks grid-stride over the B*S*W/16 items with 64-bit
// offsets.
#include "common.h"
#include "rope_map.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

__global__ void __launch_bounds__(ROPE_BLOCK)
rope_qkv_kernel(const bf16* __restrict__ X, const float* __restrict__ Cos,
                const float* __restrict__ Sin, bf16* __restrict__ Y,
                RopeShape p, float sgn) {
  const unsigned long n_items = (unsigned long)p.n_rows * (unsigned)p.U;
  const unsigned long step = (unsigned long)gridDim.x * ROPE_BLOCK;
  const int half = p.D / 2;
  for (unsigned long base = (unsigned long)blockIdx.x * ROPE_BLOCK;
       base < n_items; base += step) {
    const RopeItem it = rope_item(base, threadIdx.x, p);
    if (!it.valid) continue;
    const bf16x8 lo = *reinterpret_cast<const bf16x8*>(X + it.in_lo);
    const bf16x8 hi = *reinterpret_cast<const bf16x8*>(X + it.in_lo + half);
    bf16x8 olo = lo, ohi = hi;
    if (it.rotate) {
      const f32x4v* cp = reinterpret_cast<const f32x4v*>(Cos + it.tab);
      const f32x4v* sp = reinterpret_cast<const f32x4v*>(Sin + it.tab);
      const f32x4v c0 = cp[0], c1 = cp[1], s0 = sp[0], s1 = sp[1];
      const float c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
      const float t[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
      #pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float l = bf2f(lo.v[e]), h = bf2f(hi.v[e]), te = sgn * t[e];
        olo.v[e] = f2bf(l * c[e] - h * te);
        ohi.v[e] = f2bf(h * c[e] + l * te);
      }
    }
    *reinterpret_cast<bf16x8*>(Y + it.out_lo) = olo;
    *reinterpret_cast<bf16x8*>(Y + it.out_lo + half) = ohi;
  }
}

// Blocks of the grid: enough to hold 8 of them on each of the 256 CUs, the
// rest of the items by the grid-stride loop.  EASYDIST_ROPE_BLOCKS overrides
// the cap for sweeps (and lets a small shape take the loop more than once);
// read at every launch like the other knobs.
static unsigned rope_blocks(unsigned long n_items) {
  long cap = 2048;
  if (const char* e = getenv("EASYDIST_ROPE_BLOCKS")) {
    const long v = atol(e);
    if (v >= 1 && v <= 65536) cap = v;
  }
  const unsigned long need = (n_items + ROPE_BLOCK - 1) / ROPE_BLOCK;
  return (unsigned)std::max(1UL, std::min((unsigned long)cap, need));
}

at::Tensor rope_qkv(const at::Tensor& qkv, const at::Tensor& cos,
                    const at::Tensor& sin, int64_t H, int64_t Hkv,
                    bool inverse) {
  TORCH_CHECK(qkv.dtype() == at::kBFloat16 && qkv.dim() == 3,
              "rope_qkv: qkv must be bf16 [B, S, W]");
  TORCH_CHECK(cos.dtype() == at::kFloat && sin.dtype() == at::kFloat &&
              cos.dim() == 2 && cos.sizes() == sin.sizes() &&
              cos.is_contiguous() && sin.is_contiguous(),
              "rope_qkv: cos, sin must be contiguous fp32 [S, D/2]");
  const long B = qkv.size(0), S = qkv.size(1), W = qkv.size(2);
  const long D = 2 * cos.size(1);
  TORCH_CHECK(B >= 1 && S >= 1 && H >= 1 && Hkv >= 1);
  TORCH_CHECK(D % 16 == 0 && D <= 256,
              "rope_qkv: head dim must be a multiple of 16, at most 256");
  TORCH_CHECK(cos.size(0) == S && W == (H + 2 * Hkv) * D,
              "rope_qkv: shapes do not match");
  TORCH_CHECK(W < (1L << 31) && S < (1L << 31) - ROPE_BLOCK - 1);
  // 16-byte vectors: every row and both tables start on one
  TORCH_CHECK(qkv.stride(2) == 1 && qkv.stride(0) % 8 == 0 &&
              qkv.stride(1) % 8 == 0 && qkv.stride(0) >= 0 &&
              qkv.stride(1) >= 0 &&
              (uintptr_t)qkv.data_ptr() % 16 == 0 &&
              (uintptr_t)cos.data_ptr() % 16 == 0 &&
              (uintptr_t)sin.data_ptr() % 16 == 0,
              "rope_qkv: qkv needs a contiguous last dim and 16-byte "
              "aligned rows");
  auto out = at::empty({B, S, W}, qkv.options());
  RopeShape p;
  p.n_rows = B * S;
  p.stride_b = qkv.stride(0);
  p.stride_s = qkv.stride(1);
  p.S = (int)S;
  p.D = (int)D;
  p.W = (int)W;
  p.U = (int)(W / 16);
  p.VH = (int)(D / 16);
  p.rot_units = (int)((H + Hkv) * (D / 16));
  const unsigned long n_items = (unsigned long)p.n_rows * (unsigned)p.U;
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(rope_qkv_kernel, dim3(rope_blocks(n_items)),
                     dim3(ROPE_BLOCK), 0, stream,
                     (const bf16*)qkv.data_ptr(), cos.data_ptr<float>(),
                     sin.data_ptr<float>(), (bf16*)out.data_ptr(), p,
                     inverse ? -1.f : 1.f);
  return out;
}
