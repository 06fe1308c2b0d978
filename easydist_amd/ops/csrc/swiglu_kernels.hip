// Fused SwiGLU activation, forward and backward (gfx950).
//
//     s      = 1 / (1 + exp(-g))
//     out    = g * s * u
//     dgate  = dy * u * s * (1 + g * (1 - s))
//     dup    = dy * g * s
//
// in fp32, each result rounded to bf16 once.  The backward recomputes s, so
// nothing but gate and up is kept from the forward.  A gate so negative that
// exp(-g) overflows gives 1/inf = 0 = s and zero outputs, never NaN.
//
// Two memory-bound passes, no LDS, no atomics.  Every operand is [R, F] rows
// with its own row stride and a contiguous last dim (the two halves of one
// [R, 2F] projection output, or two separate bmm results, cost no copy); the
// outputs are new contiguous tensors.  A thread owns 8 columns of one row:
// 16-byte loads and stores, 3 of them forward and 5 backward.  Blocks
// grid-stride over the R*F/8 items with 64-bit offsets.
#include "common.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#define SWIGLU_BLOCK 256   // threads per block = items per block pass

struct SwigluShape {
  unsigned long n_items;   // R * V
  unsigned V;              // 16-byte vectors per row, F / 8
  long stride_g, stride_u, stride_dy;   // row strides in elements
};

DEVINL float swiglu_sigmoid(float g) {
  return __builtin_amdgcn_rcpf(1.f + __expf(-g));
}

__global__ void __launch_bounds__(SWIGLU_BLOCK)
swiglu_fwd_kernel(const bf16* __restrict__ G, const bf16* __restrict__ U,
                  bf16* __restrict__ Y, SwigluShape p) {
  const unsigned long step = (unsigned long)gridDim.x * SWIGLU_BLOCK;
  for (unsigned long it = (unsigned long)blockIdx.x * SWIGLU_BLOCK
           + threadIdx.x; it < p.n_items; it += step) {
    const unsigned long row = it / p.V;
    const long col = (long)(it - row * p.V) * 8;
    const bf16x8 g = *reinterpret_cast<const bf16x8*>(
        G + (long)row * p.stride_g + col);
    const bf16x8 u = *reinterpret_cast<const bf16x8*>(
        U + (long)row * p.stride_u + col);
    bf16x8 y;
    #pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float ge = bf2f(g.v[e]);
      y.v[e] = f2bf(ge * swiglu_sigmoid(ge) * bf2f(u.v[e]));
    }
    *reinterpret_cast<bf16x8*>(Y + it * 8) = y;
  }
}

__global__ void __launch_bounds__(SWIGLU_BLOCK)
swiglu_bwd_kernel(const bf16* __restrict__ DY, const bf16* __restrict__ G,
                  const bf16* __restrict__ U, bf16* __restrict__ DG,
                  bf16* __restrict__ DU, SwigluShape p) {
  const unsigned long step = (unsigned long)gridDim.x * SWIGLU_BLOCK;
  for (unsigned long it = (unsigned long)blockIdx.x * SWIGLU_BLOCK
           + threadIdx.x; it < p.n_items; it += step) {
    const unsigned long row = it / p.V;
    const long col = (long)(it - row * p.V) * 8;
    const bf16x8 dy = *reinterpret_cast<const bf16x8*>(
        DY + (long)row * p.stride_dy + col);
    const bf16x8 g = *reinterpret_cast<const bf16x8*>(
        G + (long)row * p.stride_g + col);
    const bf16x8 u = *reinterpret_cast<const bf16x8*>(
        U + (long)row * p.stride_u + col);
    bf16x8 dg, du;
    #pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float d = bf2f(dy.v[e]), ge = bf2f(g.v[e]), ue = bf2f(u.v[e]);
      const float s = swiglu_sigmoid(ge);
      dg.v[e] = f2bf(d * ue * s * (1.f + ge * (1.f - s)));
      du.v[e] = f2bf(d * ge * s);
    }
    *reinterpret_cast<bf16x8*>(DG + it * 8) = dg;
    *reinterpret_cast<bf16x8*>(DU + it * 8) = du;
  }
}

// Blocks of the grid: enough to hold 8 of them on each of the 256 CUs, the
// rest of the items by the grid-stride loop.  EASYDIST_SWIGLU_BLOCKS
// overrides the cap for sweeps (and lets a small shape take the loop more
// than once); read at every launch like the other knobs.
static unsigned swiglu_blocks(unsigned long n_items) {
  long cap = 2048;
  if (const char* e = getenv("EASYDIST_SWIGLU_BLOCKS")) {
    const long v = atol(e);
    if (v >= 1 && v <= 65536) cap = v;
  }
  const unsigned long need = (n_items + SWIGLU_BLOCK - 1) / SWIGLU_BLOCK;
  return (unsigned)std::max(1UL, std::min((unsigned long)cap, need));
}

// The row stride of t seen as [R, F] rows: its leading dims must collapse to
// one stride.  Dims of size 1 carry no stride; a single row takes F.
static bool swiglu_row_stride(const at::Tensor& t, long* out) {
  long stride = -1, inner = 1;   // inner: rows spanned by the dims so far
  for (int64_t d = t.dim() - 2; d >= 0; --d) {
    if (t.size(d) == 1) continue;
    if (stride < 0) stride = t.stride(d);
    else if (t.stride(d) != stride * inner) return false;
    inner *= t.size(d);
  }
  *out = stride < 0 ? t.size(-1) : stride;
  return true;
}

static long swiglu_check(const at::Tensor& t, const at::Tensor& like,
                         const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dtype() == at::kBFloat16, "swiglu: ", name,
              " must be a bf16 device tensor");
  TORCH_CHECK(t.dim() >= 1 && t.sizes() == like.sizes() && t.numel() > 0,
              "swiglu: all operands must have one non-empty shape");
  TORCH_CHECK(t.stride(-1) == 1 && t.size(-1) % 8 == 0, "swiglu: ", name,
              " needs a contiguous last dim that is a multiple of 8");
  long stride = 0;
  TORCH_CHECK(swiglu_row_stride(t, &stride) && stride >= 0 && stride % 8 == 0,
              "swiglu: the leading dims of ", name, " must collapse to one "
              "row stride, a non-negative multiple of 8");
  TORCH_CHECK((uintptr_t)t.data_ptr() % 16 == 0, "swiglu: ", name,
              " must be 16-byte aligned");
  return stride;
}

static SwigluShape swiglu_shape(const at::Tensor& gate) {
  const long F = gate.size(-1);
  TORCH_CHECK(F / 8 < (1L << 32));
  SwigluShape p;
  p.V = (unsigned)(F / 8);
  p.n_items = (unsigned long)(gate.numel() / F) * p.V;
  p.stride_g = p.stride_u = p.stride_dy = 0;
  return p;
}

at::Tensor swiglu_fwd(const at::Tensor& gate, const at::Tensor& up) {
  SwigluShape p = swiglu_shape(gate);
  p.stride_g = swiglu_check(gate, gate, "gate");
  p.stride_u = swiglu_check(up, gate, "up");
  auto out = at::empty(gate.sizes(), gate.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(swiglu_fwd_kernel, dim3(swiglu_blocks(p.n_items)),
                     dim3(SWIGLU_BLOCK), 0, stream,
                     (const bf16*)gate.data_ptr(), (const bf16*)up.data_ptr(),
                     (bf16*)out.data_ptr(), p);
  return out;
}

std::tuple<at::Tensor, at::Tensor>
swiglu_bwd(const at::Tensor& grad, const at::Tensor& gate,
           const at::Tensor& up) {
  SwigluShape p = swiglu_shape(gate);
  p.stride_dy = swiglu_check(grad, gate, "grad");
  p.stride_g = swiglu_check(gate, gate, "gate");
  p.stride_u = swiglu_check(up, gate, "up");
  auto dgate = at::empty(gate.sizes(), gate.options());
  auto dup = at::empty(gate.sizes(), gate.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(swiglu_bwd_kernel, dim3(swiglu_blocks(p.n_items)),
                     dim3(SWIGLU_BLOCK), 0, stream,
                     (const bf16*)grad.data_ptr(),
                     (const bf16*)gate.data_ptr(), (const bf16*)up.data_ptr(),
                     (bf16*)dgate.data_ptr(), (bf16*)dup.data_ptr(), p);
  return {dgate, dup};
}
