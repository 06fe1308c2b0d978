// LayerNorm / RMSNorm forward+backward for gfx950.
//
// Memory-bound ops: the design target is the HBM3E roofline (~6.3 TB/s
// achievable). One WAVE per row, bf16x8 / float4 vectorized loads
// (16 B/lane), fp32 accumulation, wave shuffle reductions. The LayerNorm
// backward keeps dweight/dbias in registers across a row loop and sums
// per-block partials in a fixed order; the older two-kernel form
// (EASYDIST_NORM_FUSE=0, and RMSNorm) accumulates them into fp32 global
// scratch with device-scope atomics.
// Replaces aten.native_layer_norm(+backward) via the lower_hip pass.
#include "common.h"
#include <string>
#include <cstdlib>

// ---------------------------------------------------------------- fwd -------
template <typename T, bool RMS>
__global__ void norm_fwd_kernel(const T* __restrict__ x,
                                const T* __restrict__ w,
                                const T* __restrict__ b,
                                T* __restrict__ out,
                                float* __restrict__ mean_out,
                                float* __restrict__ rstd_out,
                                int rows, int D, float eps) {
  const int wave_id = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (wave_id >= rows) return;
  const T* xrow = x + (long)wave_id * D;
  T* orow = out + (long)wave_id * D;

  const int VEC = 8;
  float s1 = 0.f, s2 = 0.f;
  for (int i = lane * VEC; i < D; i += WAVE * VEC) {
    bf16x8 xv = *reinterpret_cast<const bf16x8*>(&xrow[i]);
    #pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float f = bf2f(xv.v[j]);
      s1 += f;
      s2 += f * f;
    }
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  float mean, rstd;
  if (RMS) {
    mean = 0.f;
    rstd = rsqrtf(s2 / D + eps);
  } else {
    mean = s1 / D;
    rstd = rsqrtf(fmaxf(s2 / D - mean * mean, 0.f) + eps);
  }
  if (lane == 0) {
    if (!RMS) mean_out[wave_id] = mean;
    rstd_out[wave_id] = rstd;
  }
  for (int i = lane * VEC; i < D; i += WAVE * VEC) {
    bf16x8 xv = *reinterpret_cast<const bf16x8*>(&xrow[i]);
    bf16x8 ov;
    bf16x8 wv, bv;
    if (w) wv = *reinterpret_cast<const bf16x8*>(&w[i]);
    if (b) bv = *reinterpret_cast<const bf16x8*>(&b[i]);
    #pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float f = (bf2f(xv.v[j]) - mean) * rstd;
      if (w) f *= bf2f(wv.v[j]);
      if (b) f += bf2f(bv.v[j]);
      ov.v[j] = f2bf(f);
    }
    *reinterpret_cast<bf16x8*>(&orow[i]) = ov;
  }
}

// fp32 variant
template <bool RMS>
__global__ void norm_fwd_kernel_f32(const float* __restrict__ x,
                                    const float* __restrict__ w,
                                    const float* __restrict__ b,
                                    float* __restrict__ out,
                                    float* __restrict__ mean_out,
                                    float* __restrict__ rstd_out,
                                    int rows, int D, float eps) {
  const int wave_id = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (wave_id >= rows) return;
  const float* xrow = x + (long)wave_id * D;
  float* orow = out + (long)wave_id * D;
  const int VEC = 4;
  float s1 = 0.f, s2 = 0.f;
  for (int i = lane * VEC; i < D; i += WAVE * VEC) {
    float4 xv = *reinterpret_cast<const float4*>(&xrow[i]);
    s1 += xv.x + xv.y + xv.z + xv.w;
    s2 += xv.x * xv.x + xv.y * xv.y + xv.z * xv.z + xv.w * xv.w;
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  float mean, rstd;
  if (RMS) {
    mean = 0.f;
    rstd = rsqrtf(s2 / D + eps);
  } else {
    mean = s1 / D;
    rstd = rsqrtf(fmaxf(s2 / D - mean * mean, 0.f) + eps);
  }
  if (lane == 0) {
    if (!RMS) mean_out[wave_id] = mean;
    rstd_out[wave_id] = rstd;
  }
  for (int i = lane * VEC; i < D; i += WAVE * VEC) {
    float4 xv = *reinterpret_cast<const float4*>(&xrow[i]);
    float4 ov;
    float* xp = &xv.x;
    float* op = &ov.x;
    #pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float f = (xp[j] - mean) * rstd;
      if (w) f *= w[i + j];
      if (b) f += b[i + j];
      op[j] = f;
    }
    *reinterpret_cast<float4*>(&orow[i]) = ov;
  }
}

// ---------------------------------------------------------------- bwd -------
// dx_j = rstd * ( gw_j - mean(gw) - xhat_j * mean(gw * xhat) )   [LN]
// where gw = grad * w. dw_j = sum_rows grad_j * xhat_j ; db_j = sum_rows grad.
template <typename T, bool RMS>
__global__ void norm_bwd_kernel(const T* __restrict__ grad,
                                const T* __restrict__ x,
                                const float* __restrict__ mean,
                                const float* __restrict__ rstd,
                                const T* __restrict__ w,
                                T* __restrict__ dx,
                                float* __restrict__ dw,   // fp32 scratch [D]
                                float* __restrict__ db,   // fp32 scratch [D]
                                int rows, int D) {
  const int wave_id = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (wave_id >= rows) return;
  const T* grow = grad + (long)wave_id * D;
  const T* xrow = x + (long)wave_id * D;
  T* dxrow = dx + (long)wave_id * D;
  const float m = RMS ? 0.f : mean[wave_id];
  const float r = rstd[wave_id];

  const int VEC = 8;
  float sum_gw = 0.f, sum_gwx = 0.f;
  for (int i = lane * VEC; i < D; i += WAVE * VEC) {
    bf16x8 gv = *reinterpret_cast<const bf16x8*>(&grow[i]);
    bf16x8 xv = *reinterpret_cast<const bf16x8*>(&xrow[i]);
    bf16x8 wv;
    if (w) wv = *reinterpret_cast<const bf16x8*>(&w[i]);
    #pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float g = bf2f(gv.v[j]);
      float xh = (bf2f(xv.v[j]) - m) * r;
      float gw = w ? g * bf2f(wv.v[j]) : g;
      sum_gw += gw;
      sum_gwx += gw * xh;
    }
  }
  sum_gw = wave_sum(sum_gw) / D;
  sum_gwx = wave_sum(sum_gwx) / D;
  for (int i = lane * VEC; i < D; i += WAVE * VEC) {
    bf16x8 gv = *reinterpret_cast<const bf16x8*>(&grow[i]);
    bf16x8 xv = *reinterpret_cast<const bf16x8*>(&xrow[i]);
    bf16x8 wv;
    if (w) wv = *reinterpret_cast<const bf16x8*>(&w[i]);
    bf16x8 dxv;
    #pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float g = bf2f(gv.v[j]);
      float xh = (bf2f(xv.v[j]) - m) * r;
      float gw = w ? g * bf2f(wv.v[j]) : g;
      float v = RMS ? r * (gw - xh * sum_gwx)
                    : r * (gw - sum_gw - xh * sum_gwx);
      dxv.v[j] = f2bf(v);
    }
    *reinterpret_cast<bf16x8*>(&dxrow[i]) = dxv;
  }
}

// Column reduction for dweight/dbias: each block owns 256 columns x a chunk
// of rows, accumulates in registers, ONE atomic per (block, column).
template <typename T, bool RMS>
__global__ void norm_param_grads_kernel(const T* __restrict__ grad,
                                        const T* __restrict__ x,
                                        const float* __restrict__ mean,
                                        const float* __restrict__ rstd,
                                        float* __restrict__ dw,
                                        float* __restrict__ db,
                                        int rows, int D, int rows_per_blk) {
  // 8 columns per thread with 16-B vector loads: the scalar-bf16 form
  // streamed at half rate (guide common-mistake 2)
  const int col0 = (blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (col0 >= D) return;
  const int r0 = blockIdx.y * rows_per_blk;
  const int r1 = min(r0 + rows_per_blk, rows);
  float sw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float sb[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int r = r0; r < r1; ++r) {
    const bf16x8 g8 = *reinterpret_cast<const bf16x8*>(
        &grad[(long)r * D + col0]);
    const bf16x8 x8 = *reinterpret_cast<const bf16x8*>(
        &x[(long)r * D + col0]);
    const float m = RMS ? 0.f : mean[r];
    const float rs = rstd[r];
    #pragma unroll
    for (int u = 0; u < 8; ++u) {
      float g = bf2f(g8.v[u]);
      sw[u] += g * (bf2f(x8.v[u]) - m) * rs;
      sb[u] += g;
    }
  }
  #pragma unroll
  for (int u = 0; u < 8; ++u) {
    atomicAdd(&dw[col0 + u], sw[u]);
    atomicAdd(&db[col0 + u], sb[u]);
  }
}

template <typename T, bool RMS>
__global__ void norm_param_grads_scalar_kernel(const T* __restrict__ grad,
                                               const T* __restrict__ x,
                                               const float* __restrict__ mean,
                                               const float* __restrict__ rstd,
                                               float* __restrict__ dw,
                                               float* __restrict__ db,
                                               int rows, int D,
                                               int rows_per_blk) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= D) return;
  const int r0 = blockIdx.y * rows_per_blk;
  const int r1 = min(r0 + rows_per_blk, rows);
  float sw = 0.f, sb = 0.f;
  // unroll keeps ~8 independent load pairs in flight per lane — the
  // rolled form was latency-bound at half of HBM bandwidth
  #pragma unroll 8
  for (int r = r0; r < r1; ++r) {
    float g = bf2f(grad[(long)r * D + col]);
    float m = RMS ? 0.f : mean[r];
    float xh = (bf2f(x[(long)r * D + col]) - m) * rstd[r];
    sw += g * xh;
    sb += g;
  }
  atomicAdd(&dw[col], sw);
  atomicAdd(&db[col], sb);
}

static bool lnpg_scalar() {
  // measured on MI355X (65536x768): scalar-column form 0.166 ms/call vs
  // 0.221 for the vectorized+fewer-atomics form — per-address atomic
  // count and full-block occupancy beat wider loads here
  static int v = [] {
    const char* e = getenv("EASYDIST_LNPG");
    return (e && std::string(e) == "vector") ? 0 : 1;
  }();
  return v;
}

// ------------------------------------------- residual-fused fwd / bwd -------
// The residual stream wraps every LayerNorm in an add: s = a + b feeds the
// norm in the forward, and dx + g leaves it in the backward. These kernels
// do the add on the registers the norm already holds, and the backward also
// keeps the dweight/dbias column sums, so each tensor is streamed once.
//
// Both are bit-exact against the kernels they replace. hipcc contracts only
// some of the mul+add pairs of norm_fwd_kernel / norm_bwd_kernel into FMAs
// (the row-sum accumulations become packed adds and stay unfused), so the
// new kernels switch contraction off and spell out the FMAs that the old
// ones execute. Only the LayerNorm forms (RMS = false) are instantiated and
// held to that by tests/test_gpu_norm_fuse.py; rms_norm_bwd still runs the
// two-kernel form.
#define NORM_WPB 4            // waves per block
#define NORM_MAX_FUSED_D 2048 // NV <= 4 vectors of 8 columns per lane

// s = bf16(a + b) (aten's bf16 add rounding), stored and normalised from
// registers. One wave per row; lane owns columns lane*8 + k*512, k < NV.
template <typename T, bool RMS, int NV>
__global__ void __launch_bounds__(WAVE * NORM_WPB)
add_norm_fwd_kernel(const T* __restrict__ a, const T* __restrict__ b,
                    const T* __restrict__ w, const T* __restrict__ bias,
                    T* __restrict__ sum, T* __restrict__ out,
                    float* __restrict__ mean_out,
                    float* __restrict__ rstd_out,
                    int rows, int D, float eps) {
  #pragma clang fp contract(off)
  const int wave_id = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (wave_id >= rows) return;
  const long base = (long)wave_id * D;
  const int VEC = 8;

  bf16x8 av[NV], bv[NV], sv[NV];
  #pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i = lane * VEC + k * WAVE * VEC;
    if (i < D) {
      av[k] = *reinterpret_cast<const bf16x8*>(&a[base + i]);
      bv[k] = *reinterpret_cast<const bf16x8*>(&b[base + i]);
    }
  }
  float s1 = 0.f, s2 = 0.f;
  #pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i = lane * VEC + k * WAVE * VEC;
    if (i < D) {
      #pragma unroll
      for (int j = 0; j < VEC; ++j) {
        sv[k].v[j] = f2bf(bf2f(av[k].v[j]) + bf2f(bv[k].v[j]));
        float f = bf2f(sv[k].v[j]);
        s1 += f;
        s2 += f * f;
      }
      *reinterpret_cast<bf16x8*>(&sum[base + i]) = sv[k];
    }
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  float mean, rstd;
  if (RMS) {
    mean = 0.f;
    rstd = rsqrtf(s2 / D + eps);
  } else {
    mean = s1 / D;
    rstd = rsqrtf(fmaxf(__builtin_fmaf(-mean, mean, s2 / D), 0.f) + eps);
  }
  if (lane == 0) {
    if (!RMS) mean_out[wave_id] = mean;
    rstd_out[wave_id] = rstd;
  }
  #pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i = lane * VEC + k * WAVE * VEC;
    if (i < D) {
      bf16x8 ov, wv, bsv;
      if (w) wv = *reinterpret_cast<const bf16x8*>(&w[i]);
      if (bias) bsv = *reinterpret_cast<const bf16x8*>(&bias[i]);
      #pragma unroll
      for (int j = 0; j < VEC; ++j) {
        float f = (bf2f(sv[k].v[j]) - mean) * rstd;
        if (w) f *= bf2f(wv.v[j]);
        if (bias) f += bf2f(bsv.v[j]);
        ov.v[j] = f2bf(f);
      }
      *reinterpret_cast<bf16x8*>(&out[base + i]) = ov;
    }
  }
}

// dx (+ residual gradient) and the dweight/dbias column sums in one pass.
// A fixed grid of 4-wave blocks; each wave walks rows wave, wave + nwaves,
// ... with the next row's grad and x loads issued before the current row's
// math, and a lane owns the same columns in every row, so the column sums
// stay in registers. Lanes past D hold zeros and add zeros: the math has no
// branches, only the stores are guarded. Each block then folds its waves
// through LDS and stores one [2][D] fp32 partial; norm_partials_sum_kernel
// adds the partials in a fixed order (no atomics, no zero fill, run-to-run
// identical dw/db).
template <typename T, bool RMS, int NV>
__global__ void __launch_bounds__(WAVE * NORM_WPB)
norm_bwd_fused_kernel(const T* __restrict__ grad, const T* __restrict__ x,
                      const float* __restrict__ mean,
                      const float* __restrict__ rstd,
                      const T* __restrict__ w,
                      const T* __restrict__ res,     // may be null
                      T* __restrict__ dx,
                      float* __restrict__ partial,   // [gridDim.x][2][D]
                      int rows, int D) {
  #pragma clang fp contract(off)
  const int VEC = 8;
  const int lane = threadIdx.x % WAVE;
  const int wave = threadIdx.x / WAVE;
  const int nwaves = gridDim.x * NORM_WPB;
  __shared__ float red[NORM_WPB - 1][2][NV][WAVE * VEC];

  bf16x8 wv[NV], gn[NV], xn[NV];
  float aw[NV][VEC], ab[NV][VEC];
  #pragma unroll
  for (int k = 0; k < NV; ++k) {
    #pragma unroll
    for (int j = 0; j < VEC; ++j) {
      wv[k].v[j] = gn[k].v[j] = xn[k].v[j] = f2bf(0.f);
      aw[k][j] = 0.f;
      ab[k][j] = 0.f;
    }
    const int i = lane * VEC + k * WAVE * VEC;
    if (w && i < D) wv[k] = *reinterpret_cast<const bf16x8*>(&w[i]);
  }

  float mn = 0.f, rsn = 0.f;
  int row = blockIdx.x * NORM_WPB + wave;
  if (row < rows) {
    const long base = (long)row * D;
    #pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int i = lane * VEC + k * WAVE * VEC;
      if (i < D) {
        gn[k] = *reinterpret_cast<const bf16x8*>(&grad[base + i]);
        xn[k] = *reinterpret_cast<const bf16x8*>(&x[base + i]);
      }
    }
    if (!RMS) mn = mean[row];
    rsn = rstd[row];
  }
  for (; row < rows; row += nwaves) {
    bf16x8 gc[NV], xc[NV], rc[NV];
    #pragma unroll
    for (int k = 0; k < NV; ++k) { gc[k] = gn[k]; xc[k] = xn[k]; }
    const float m = RMS ? 0.f : mn;
    const float r = rsn;
    const long base = (long)row * D;
    // needed last, after both wave reductions: no look-ahead registers
    if (res) {
      #pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int i = lane * VEC + k * WAVE * VEC;
        if (i < D) rc[k] = *reinterpret_cast<const bf16x8*>(&res[base + i]);
      }
    }
    // rows and nwaves are both below 2^30 here, so the sum cannot wrap
    const int nrow = row + nwaves;
    if (nrow < rows) {
      const long nbase = (long)nrow * D;
      #pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int i = lane * VEC + k * WAVE * VEC;
        if (i < D) {
          gn[k] = *reinterpret_cast<const bf16x8*>(&grad[nbase + i]);
          xn[k] = *reinterpret_cast<const bf16x8*>(&x[nbase + i]);
        }
      }
      if (!RMS) mn = mean[nrow];
      rsn = rstd[nrow];
    }

    float sum_gw = 0.f, sum_gwx = 0.f;
    #pragma unroll
    for (int k = 0; k < NV; ++k) {
      #pragma unroll
      for (int j = 0; j < VEC; ++j) {
        float g = bf2f(gc[k].v[j]);
        float xh = (bf2f(xc[k].v[j]) - m) * r;
        float gw = w ? g * bf2f(wv[k].v[j]) : g;
        sum_gw += gw;
        sum_gwx += gw * xh;
      }
    }
    sum_gw = wave_sum(sum_gw) / D;
    sum_gwx = wave_sum(sum_gwx) / D;
    #pragma unroll
    for (int k = 0; k < NV; ++k) {
      bf16x8 dxv;
      #pragma unroll
      for (int j = 0; j < VEC; ++j) {
        float g = bf2f(gc[k].v[j]);
        float xh = (bf2f(xc[k].v[j]) - m) * r;
        float gw = w ? g * bf2f(wv[k].v[j]) : g;
        float v = RMS ? r * __builtin_fmaf(-sum_gwx, xh, gw)
                      : r * __builtin_fmaf(-sum_gwx, xh, gw - sum_gw);
        bf16 d = f2bf(v);
        // rounded twice on purpose: dx to bf16, then aten's bf16 add
        if (res) d = f2bf(bf2f(d) + bf2f(rc[k].v[j]));
        dxv.v[j] = d;
        // the same rounded term norm_param_grads_scalar_kernel adds
        aw[k][j] += g * xh;
        ab[k][j] += g;
      }
      const int i = lane * VEC + k * WAVE * VEC;
      if (i < D) *reinterpret_cast<bf16x8*>(&dx[base + i]) = dxv;
    }
  }

  // waves 1..3 park their sums in LDS; wave 0 adds them in wave order
  if (wave > 0) {
    #pragma unroll
    for (int k = 0; k < NV; ++k)
      #pragma unroll
      for (int j = 0; j < VEC; ++j) {
        red[wave - 1][0][k][lane * VEC + j] = aw[k][j];
        red[wave - 1][1][k][lane * VEC + j] = ab[k][j];
      }
  }
  __syncthreads();
  if (wave == 0) {
    float* pw = partial + (long)blockIdx.x * 2 * D;
    float* pb = pw + D;
    #pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int i = lane * VEC + k * WAVE * VEC;
      if (i < D) {
        #pragma unroll
        for (int j = 0; j < VEC; ++j)
          #pragma unroll
          for (int v = 0; v < NORM_WPB - 1; ++v) {
            aw[k][j] += red[v][0][k][lane * VEC + j];
            ab[k][j] += red[v][1][k][lane * VEC + j];
          }
        #pragma unroll
        for (int h = 0; h < VEC; h += 4) {
          *reinterpret_cast<f32x4v*>(&pw[i + h]) =
              f32x4v{aw[k][h], aw[k][h + 1], aw[k][h + 2], aw[k][h + 3]};
          *reinterpret_cast<f32x4v*>(&pb[i + h]) =
              f32x4v{ab[k][h], ab[k][h + 1], ab[k][h + 2], ab[k][h + 3]};
        }
      }
    }
  }
}

// out[c] = sum over g of partial[g][c], c < 2*D, always in the same order:
// slice s of NORM_PS_SLICES adds g = s, s + SLICES, ..., then slice 0 adds
// the slices in order. Columns below D go to dw, the rest to db.
#define NORM_PS_SLICES 16
__global__ void __launch_bounds__(WAVE * NORM_PS_SLICES)
norm_partials_sum_kernel(const float* __restrict__ partial, int G, int D,
                         float* __restrict__ dw, float* __restrict__ db) {
  __shared__ float red[NORM_PS_SLICES][WAVE];
  const int c = blockIdx.x * WAVE + threadIdx.x;
  const int s = threadIdx.y;
  float acc = 0.f;
  if (c < 2 * D) {
    #pragma unroll 8
    for (int g = s; g < G; g += NORM_PS_SLICES)
      acc += partial[(long)g * 2 * D + c];
  }
  red[s][threadIdx.x] = acc;
  __syncthreads();
  if (s == 0 && c < 2 * D) {
    #pragma unroll
    for (int v = 1; v < NORM_PS_SLICES; ++v) acc += red[v][threadIdx.x];
    if (c < D) dw[c] = acc; else db[c - D] = acc;
  }
}

// ---------------------------------------------------------- host wrappers ---
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

static void check_lastdim(const at::Tensor& x) {
  TORCH_CHECK(x.is_contiguous(), "norm kernels need contiguous input");
  TORCH_CHECK(x.size(-1) % 8 == 0, "feature dim must be a multiple of 8");
}

static void check_affine(const at::Tensor& x,
                         const std::optional<at::Tensor>& w,
                         const std::optional<at::Tensor>& b) {
  if (w) TORCH_CHECK(w->numel() == x.size(-1), "weight/feature mismatch");
  if (b) TORCH_CHECK(b->numel() == x.size(-1), "bias/feature mismatch");
}

std::tuple<at::Tensor, at::Tensor, at::Tensor>
layer_norm_fwd(const at::Tensor& x, const std::optional<at::Tensor>& w,
               const std::optional<at::Tensor>& b, double eps) {
  check_lastdim(x);
  check_affine(x, w, b);
  const int D = x.size(-1);
  const long rows = x.numel() / D;
  auto out = at::empty_like(x);
  auto stat_shape = x.sizes().vec();
  stat_shape.back() = 1;
  auto mean = at::empty(stat_shape, x.options().dtype(at::kFloat));
  auto rstd = at::empty(stat_shape, x.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream();
  const int WPB = 4;   // waves per block
  dim3 block(WAVE * WPB), grid((rows + WPB - 1) / WPB);
  if (x.scalar_type() == at::kBFloat16) {
    hipLaunchKernelGGL((norm_fwd_kernel<bf16, false>), grid, block, 0, stream,
        (const bf16*)x.data_ptr(), w ? (const bf16*)w->data_ptr() : nullptr,
        b ? (const bf16*)b->data_ptr() : nullptr, (bf16*)out.data_ptr(),
        mean.data_ptr<float>(), rstd.data_ptr<float>(), rows, D, (float)eps);
  } else {
    hipLaunchKernelGGL((norm_fwd_kernel_f32<false>), grid, block, 0, stream,
        x.data_ptr<float>(), w ? w->data_ptr<float>() : nullptr,
        b ? b->data_ptr<float>() : nullptr, out.data_ptr<float>(),
        mean.data_ptr<float>(), rstd.data_ptr<float>(), rows, D, (float)eps);
  }
  return {out, mean, rstd};
}

// EASYDIST_NORM_FUSE=0 brings back norm_bwd + param_grads (+ aten add) for
// A/B; read at every launch like the other knobs.
static bool norm_fuse_enabled() {
  const char* e = getenv("EASYDIST_NORM_FUSE");
  return !(e && std::string(e) == "0");
}

// Blocks of the fused backward's fixed grid: what the 256 CUs hold at once,
// so no block waits for a slot. The kernel fits 3 waves per SIMD for D in
// 513..1024 (768 blocks; swept on MI355X at 65536x768, profiles/README.md
// Round 7), 4 for D <= 512 (1024 blocks beat 768 at 98304x512) and 1 above
// (256 blocks, by the same rule, not measured). EASYDIST_NORM_BWD_BLOCKS
// overrides it for such sweeps.
static int norm_bwd_blocks(long rows, int D) {
  long g = D <= 512 ? 1024 : D <= 1024 ? 768 : 256;
  if (const char* e = getenv("EASYDIST_NORM_BWD_BLOCKS")) {
    const long v = atol(e);
    if (v >= 1 && v <= 65536) g = v;
  }
  const long need = (rows + NORM_WPB - 1) / NORM_WPB;
  return (int)std::max(1L, std::min(g, need));
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
add_layer_norm_fwd(const at::Tensor& a, const at::Tensor& b,
                   const std::optional<at::Tensor>& w,
                   const std::optional<at::Tensor>& bias, double eps) {
  check_lastdim(a);
  check_affine(a, w, bias);
  TORCH_CHECK(a.sizes() == b.sizes() && b.is_contiguous() &&
              a.scalar_type() == b.scalar_type(),
              "add_layer_norm_fwd: operands must match, no broadcasting");
  const int D = a.size(-1);
  const long rows = a.numel() / D;
  if (a.scalar_type() != at::kBFloat16 || D > NORM_MAX_FUSED_D) {
    auto sum = at::add(a, b);
    auto [out, mean, rstd] = layer_norm_fwd(sum, w, bias, eps);
    return {sum, out, mean, rstd};
  }
  TORCH_CHECK(rows < (1L << 30));
  auto sum = at::empty_like(a);
  auto out = at::empty_like(a);
  auto stat_shape = a.sizes().vec();
  stat_shape.back() = 1;
  auto mean = at::empty(stat_shape, a.options().dtype(at::kFloat));
  auto rstd = at::empty(stat_shape, a.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream();
  dim3 block(WAVE * NORM_WPB), grid((rows + NORM_WPB - 1) / NORM_WPB);
#define LAUNCH_ADD_NORM_FWD(NV)                                              \
  hipLaunchKernelGGL((add_norm_fwd_kernel<bf16, false, NV>), grid, block, 0, \
      stream, (const bf16*)a.data_ptr(), (const bf16*)b.data_ptr(),          \
      w ? (const bf16*)w->data_ptr() : nullptr,                              \
      bias ? (const bf16*)bias->data_ptr() : nullptr,                        \
      (bf16*)sum.data_ptr(), (bf16*)out.data_ptr(), mean.data_ptr<float>(),  \
      rstd.data_ptr<float>(), (int)rows, D, (float)eps)
  if (rows == 0) {}
  else if (D <= 512) LAUNCH_ADD_NORM_FWD(1);
  else if (D <= 1024) LAUNCH_ADD_NORM_FWD(2);
  else LAUNCH_ADD_NORM_FWD(4);
#undef LAUNCH_ADD_NORM_FWD
  return {sum, out, mean, rstd};
}

static std::tuple<at::Tensor, at::Tensor, at::Tensor>
layer_norm_bwd_unfused(const at::Tensor& grad, const at::Tensor& x,
                       const at::Tensor& mean, const at::Tensor& rstd,
                       const std::optional<at::Tensor>& w);

std::tuple<at::Tensor, at::Tensor, at::Tensor>
layer_norm_bwd_res(const at::Tensor& grad, const at::Tensor& x,
                   const at::Tensor& mean, const at::Tensor& rstd,
                   const std::optional<at::Tensor>& w,
                   const std::optional<at::Tensor>& res,
                   std::vector<bool> mask) {
  check_lastdim(x);
  check_affine(x, w, std::nullopt);
  TORCH_CHECK(grad.sizes() == x.sizes() && grad.is_contiguous());
  TORCH_CHECK(mean.numel() == x.numel() / x.size(-1));
  TORCH_CHECK(rstd.numel() == mean.numel());
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 &&
              grad.scalar_type() == at::kBFloat16,
              "layer_norm_bwd kernel: bf16 only (fp32 falls back to aten)");
  if (res)
    TORCH_CHECK(res->sizes() == x.sizes() && res->is_contiguous() &&
                res->scalar_type() == at::kBFloat16,
                "layer_norm_bwd_res: residual must match x, no broadcasting");
  const int D = x.size(-1);
  const long rows = x.numel() / D;
  if (!norm_fuse_enabled() || D > NORM_MAX_FUSED_D) {
    auto [dx, dw, db] = layer_norm_bwd_unfused(grad, x, mean, rstd, w);
    if (res) dx.add_(*res);
    return {dx, dw, db};
  }
  TORCH_CHECK(rows < (1L << 30));
  const int G = norm_bwd_blocks(rows, D);
  auto fopt = x.options().dtype(at::kFloat);
  auto dx = at::empty_like(x);
  auto partial = at::empty({G, 2, D}, fopt);
  auto dwf = at::empty({D}, fopt);
  auto dbf = at::empty({D}, fopt);
  auto stream = at::cuda::getCurrentCUDAStream();
  dim3 block(WAVE * NORM_WPB), grid(G);
#define LAUNCH_NORM_BWD_FUSED(NV)                                            \
  hipLaunchKernelGGL((norm_bwd_fused_kernel<bf16, false, NV>), grid, block,  \
      0, stream, (const bf16*)grad.data_ptr(), (const bf16*)x.data_ptr(),    \
      mean.data_ptr<float>(), rstd.data_ptr<float>(),                        \
      w ? (const bf16*)w->data_ptr() : nullptr,                              \
      res ? (const bf16*)res->data_ptr() : nullptr, (bf16*)dx.data_ptr(),    \
      partial.data_ptr<float>(), (int)rows, D)
  if (D <= 512) LAUNCH_NORM_BWD_FUSED(1);
  else if (D <= 1024) LAUNCH_NORM_BWD_FUSED(2);
  else LAUNCH_NORM_BWD_FUSED(4);
#undef LAUNCH_NORM_BWD_FUSED
  dim3 sblock(WAVE, NORM_PS_SLICES), sgrid((2 * D + WAVE - 1) / WAVE);
  hipLaunchKernelGGL(norm_partials_sum_kernel, sgrid, sblock, 0, stream,
      partial.data_ptr<float>(), G, D, dwf.data_ptr<float>(),
      dbf.data_ptr<float>());
  return {dx, dwf, dbf};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor>
layer_norm_bwd(const at::Tensor& grad, const at::Tensor& x,
               const at::Tensor& mean, const at::Tensor& rstd,
               const std::optional<at::Tensor>& w,
               std::vector<bool> mask) {
  return layer_norm_bwd_res(grad, x, mean, rstd, w, std::nullopt, mask);
}

static std::tuple<at::Tensor, at::Tensor, at::Tensor>
layer_norm_bwd_unfused(const at::Tensor& grad, const at::Tensor& x,
                       const at::Tensor& mean, const at::Tensor& rstd,
                       const std::optional<at::Tensor>& w) {
  const int D = x.size(-1);
  const long rows = x.numel() / D;
  auto dx = at::empty_like(x);
  auto dwf = at::zeros({D}, x.options().dtype(at::kFloat));
  auto dbf = at::zeros({D}, x.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream();
  const int WPB = 4;
  dim3 block(WAVE * WPB), grid((rows + WPB - 1) / WPB);
  hipLaunchKernelGGL((norm_bwd_kernel<bf16, false>), grid, block, 0, stream,
      (const bf16*)grad.data_ptr(), (const bf16*)x.data_ptr(),
      mean.data_ptr<float>(), rstd.data_ptr<float>(),
      w ? (const bf16*)w->data_ptr() : nullptr, (bf16*)dx.data_ptr(),
      dwf.data_ptr<float>(), dbf.data_ptr<float>(), rows, D);
  // one-wave blocks, 512 columns each (64 lanes x 8 cols of 16-B
  // loads); y splits rows so x*y fills the 256 CUs
  const int gx = (D + 511) / 512;
  // few row-chunks: every block atomicAdds the whole 2*D output, so
  // block count IS the atomic contention per address
  int rows_per_blk = 256;
  while ((long)gx * ((rows + rows_per_blk - 1) / rows_per_blk) > 1024)
    rows_per_blk *= 2;
  dim3 gblock(64), ggrid(gx, (rows + rows_per_blk - 1) / rows_per_blk);
  if (lnpg_scalar()) {
    const int rpb2 = 256;
    dim3 sb2(256), sg2((D + 255) / 256, (rows + rpb2 - 1) / rpb2);
    hipLaunchKernelGGL((norm_param_grads_scalar_kernel<bf16, false>), sg2,
        sb2, 0, stream, (const bf16*)grad.data_ptr(),
        (const bf16*)x.data_ptr(), mean.data_ptr<float>(),
        rstd.data_ptr<float>(), dwf.data_ptr<float>(),
        dbf.data_ptr<float>(), rows, D, rpb2);
    auto dtype0 = at::kFloat;
    return {dx, dwf.to(dtype0), dbf.to(dtype0)};
  }
  hipLaunchKernelGGL((norm_param_grads_kernel<bf16, false>), ggrid, gblock, 0,
      stream, (const bf16*)grad.data_ptr(), (const bf16*)x.data_ptr(),
      mean.data_ptr<float>(), rstd.data_ptr<float>(), dwf.data_ptr<float>(),
      dbf.data_ptr<float>(), rows, D, rows_per_blk);
  auto dtype = at::kFloat;   // grads feed fp32 Adam: never truncate
  return {dx, dwf.to(dtype), dbf.to(dtype)};
}

std::tuple<at::Tensor, at::Tensor>
rms_norm_fwd(const at::Tensor& x, const std::optional<at::Tensor>& w,
             double eps) {
  check_lastdim(x);
  check_affine(x, w, std::nullopt);
  const int D = x.size(-1);
  const long rows = x.numel() / D;
  auto out = at::empty_like(x);
  auto stat_shape = x.sizes().vec();
  stat_shape.back() = 1;
  auto rstd = at::empty(stat_shape, x.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream();
  const int WPB = 4;
  dim3 block(WAVE * WPB), grid((rows + WPB - 1) / WPB);
  if (x.scalar_type() == at::kBFloat16) {
    hipLaunchKernelGGL((norm_fwd_kernel<bf16, true>), grid, block, 0, stream,
        (const bf16*)x.data_ptr(), w ? (const bf16*)w->data_ptr() : nullptr,
        nullptr, (bf16*)out.data_ptr(), nullptr, rstd.data_ptr<float>(),
        rows, D, (float)eps);
  } else {
    hipLaunchKernelGGL((norm_fwd_kernel_f32<true>), grid, block, 0, stream,
        x.data_ptr<float>(), w ? w->data_ptr<float>() : nullptr, nullptr,
        out.data_ptr<float>(), nullptr, rstd.data_ptr<float>(), rows, D,
        (float)eps);
  }
  return {out, rstd};
}

std::tuple<at::Tensor, at::Tensor>
rms_norm_bwd(const at::Tensor& grad, const at::Tensor& x,
             const at::Tensor& rstd, const std::optional<at::Tensor>& w) {
  check_lastdim(x);
  check_affine(x, w, std::nullopt);
  TORCH_CHECK(grad.sizes() == x.sizes() && grad.is_contiguous());
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "rms_norm_bwd: bf16 only");
  const int D = x.size(-1);
  const long rows = x.numel() / D;
  auto dx = at::empty_like(x);
  auto dwf = at::zeros({D}, x.options().dtype(at::kFloat));
  auto dbf = at::zeros({D}, x.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream();
  const int WPB = 4;
  dim3 block(WAVE * WPB), grid((rows + WPB - 1) / WPB);
  hipLaunchKernelGGL((norm_bwd_kernel<bf16, true>), grid, block, 0, stream,
      (const bf16*)grad.data_ptr(), (const bf16*)x.data_ptr(), nullptr,
      rstd.data_ptr<float>(), w ? (const bf16*)w->data_ptr() : nullptr,
      (bf16*)dx.data_ptr(), dwf.data_ptr<float>(), dbf.data_ptr<float>(),
      rows, D);
  // one-wave blocks, 512 columns each (64 lanes x 8 cols of 16-B
  // loads); y splits rows so x*y fills the 256 CUs
  const int gx = (D + 511) / 512;
  // few row-chunks: every block atomicAdds the whole 2*D output, so
  // block count IS the atomic contention per address
  int rows_per_blk = 256;
  while ((long)gx * ((rows + rows_per_blk - 1) / rows_per_blk) > 1024)
    rows_per_blk *= 2;
  dim3 gblock(64), ggrid(gx, (rows + rows_per_blk - 1) / rows_per_blk);
  hipLaunchKernelGGL((norm_param_grads_kernel<bf16, true>), ggrid, gblock, 0,
      stream, (const bf16*)grad.data_ptr(), (const bf16*)x.data_ptr(),
      nullptr, rstd.data_ptr<float>(), dwf.data_ptr<float>(),
      dbf.data_ptr<float>(), rows, D, rows_per_blk);
  auto dtype = at::kFloat;   // grads feed fp32 Adam: never truncate
  return {dx, dwf.to(dtype)};
}
