// Hand-written MFMA bf16 GEMM family for gfx950.
//
// Three dense layouts cover the linear-layer training shapes the
// compiler's lowering pass (compiler/passes/lower_hip.py) emits -- NT the
// forward, NN the dX backward, TN the dW backward -- and the grouped moe_nn /
// moe_nt / moe_tn kernels (described at their definitions) the MoE expert
// FFN:
//
//   gemm_nt_256  C[M,N] = A[M,K] @ Bt[N,K]^T (+bias)  -- fwd linears.
//       256x256x64 tile, 8 waves, 8-phase software-pipelined
//       schedule (cdna_hip_programming.md "256-sq 8-phase template"):
//       global_load_lds staging with the st_16x32 XOR swizzle applied on
//       the SOURCE address, counted s_waitcnt vmcnt(6) once per K-tile,
//       raw s_barrier (never __syncthreads: with an LDS-DMA in flight its
//       fence drains vmcnt and serializes the pipeline), s_setprio(1)
//       around each 16-MFMA cluster, LDS-bounced coalesced epilogue.
//   gemm_nt_128  same contract, 128x128x32 tile (the ladder step-3
//       structure) for edge/small shapes; row-clamped staging so M,N need
//       not be tile multiples.
//   gemm_nn_256  C[M,N] = A[M,K] @ B[K,N] (+bias)  -- the dX backward
//       (dX = dY @ W) on the weight as it lies: gemm_nt_256's tile, A half
//       and schedule, with B staged k-major (coalesced: global rows ARE
//       k-rows) into two 32-row tr-read images per tile and read with
//       ds_read_b64_tr_b16.  No transposed copy of B, in HBM or in LDS.
//   gemm_nn_128  same contract for edge/small shapes: moe_nn's plain body
//       with one expert, plus the bias.
//   gemm_tn      C[P,Q] = sum_r A[r,P] * B[r,Q]  -- the dW backward
//       (both operands reduce-dim-strided activations; transposing them
//       globally would cost ~the GEMM itself).  Tiles stage k-major
//       directly (coalesced) and fragments are read with the gfx950
//       ds_read_b64_tr_b16 hardware transpose-read; split-R over a fp32
//       atomic workspace fills all 256 CUs even for small [P,Q].  One
//       kernel template at two output tile sizes: 256x256 (8 waves,
//       three-buffer ring staging) when R >= 2048 and P, Q >= 256, and
//       128x128 (4 waves, double-buffered) for everything else.
//
// MFMA contract used throughout (v_mfma_f32_16x16x32_bf16):
//   D[m][n] += sum_k A[m][k]*B[n][k]; A/B: lane holds row (l&15),
//   k = (l>>4)*8..+8; C/D: lane holds col (l&15), rows (l>>4)*4+r.
#include "common.h"
#include "attn_block_map.h"   // xcd_swizzle, N_XCD
#include "gemm_tn_map.h"      // gemm_tn_map: wg id -> (tile, slice)
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

using f32x4 = __attribute__((ext_vector_type(4))) float;
using bf16x8v = __attribute__((ext_vector_type(8))) __bf16;
using v4s = __attribute__((ext_vector_type(4))) short;
using v8s = __attribute__((ext_vector_type(8))) short;

// global_load_lds: LDS dest is wave-uniform base + lane*16
DEVINL void glds16(const void* gsrc, void* lds_dst) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) unsigned int*)gsrc,
      (__attribute__((address_space(3))) unsigned int*)lds_dst, 16, 0, 0);
}

DEVINL void raw_barrier() { __builtin_amdgcn_s_barrier(); }

// epilogue activation modes (fused into the C store pass):
//   0 none | 1 gelu(tanh) | 2 gelu(tanh) backward: out = acc*dgelu(aux)
//   3 gelu(erf) | 4 gelu(erf) backward
//   5/6 = 1/3 writing the PRE-activation to aux (an OUTPUT here): the
//   fused forward keeps the value gelu_backward needs without a separate
//   activation kernel re-reading the GEMM result from HBM
#define GELU_C 0.7978845608028654f      // sqrt(2/pi)
#define GELU_A 0.044715f

// branch-free tanh: 1 - 2/(e^2u + 1). exp overflow/underflow saturates to
// +-1 naturally, so no range branches. libm tanhf/erff expand to ~60
// divergent exec-masked instructions PER ELEMENT here and measured +0.5 ms
// on the 65536x3072 epilogue; this is ~8 VALU with a single v_exp.
DEVINL float fast_tanh(float u) {
  return 1.f - 2.f / (__expf(2.f * u) + 1.f);
}

// The erf modes (3/4/6) use the SAME tanh approximation: gelu-tanh vs
// gelu-erf differ by <3.2e-3 absolute, under the bf16 output resolution.
DEVINL float act_apply(int act, float x, float aux) {
  if (act == 1 || act == 3) {
    float u = GELU_C * (x + GELU_A * x * x * x);
    return 0.5f * x * (1.f + fast_tanh(u));
  }
  if (act == 2 || act == 4) {
    float u = GELU_C * (aux + GELU_A * aux * aux * aux);
    float t = fast_tanh(u);
    float d = 0.5f * (1.f + t)
              + 0.5f * aux * (1.f - t * t) * GELU_C
                    * (1.f + 3.f * GELU_A * aux * aux);
    return x * d;
  }
  if (act >= 5) {   // fused fwd modes: same activation, aux is an output
    float u = GELU_C * (x + GELU_A * x * x * x);
    return 0.5f * x * (1.f + fast_tanh(u));
  }
  return x;
}

// ===========================================================================
// standalone fast gelu fwd/bwd: aten's GeluCUDAKernel measures 4.6 TB/s
// on the MLP activation (erf libcall latency chains); this bf16x8
// grid-stride form with the branch-free tanh runs at bandwidth. Used as
// the ATEN-ROUTE fallback inside gemm_nt_gelu / gemm_nt_act when the
// profiled dispatcher keeps the GEMM on hipBLASLt.
// ===========================================================================
__global__ void __launch_bounds__(256)
gelu_fwd_kernel(const bf16* __restrict__ X, bf16* __restrict__ Y, long n) {
  long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  for (; i + 7 < n; i += (long)gridDim.x * blockDim.x * 8) {
    bf16x8v x = *reinterpret_cast<const bf16x8v*>(&X[i]);
    bf16x8v y;
    #pragma unroll
    for (int e = 0; e < 8; ++e)
      y[e] = (__bf16)act_apply(1, bf2f((bf16)x[e]), 0.f);
    *reinterpret_cast<bf16x8v*>(&Y[i]) = y;
  }
}

__global__ void __launch_bounds__(256)
gelu_bwd_kernel(const bf16* __restrict__ G, const bf16* __restrict__ X,
                bf16* __restrict__ Y, long n) {
  long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  for (; i + 7 < n; i += (long)gridDim.x * blockDim.x * 8) {
    bf16x8v g = *reinterpret_cast<const bf16x8v*>(&G[i]);
    bf16x8v x = *reinterpret_cast<const bf16x8v*>(&X[i]);
    bf16x8v y;
    #pragma unroll
    for (int e = 0; e < 8; ++e)
      y[e] = (__bf16)act_apply(2, bf2f((bf16)g[e]), bf2f((bf16)x[e]));
    *reinterpret_cast<bf16x8v*>(&Y[i]) = y;
  }
}

// ===========================================================================
// gemm_nt_128: 128x128 tile, BK=32, 4 waves, double-buffered glds staging.
// Row-clamped staging + guarded epilogue: any M,N (N%1), K%32.
// ===========================================================================
#define BM 128
#define BN 128
#define BK 32

extern "C" __global__ void __launch_bounds__(256)
gemm_nt_128(const bf16* __restrict__ A, const bf16* __restrict__ Bt,
            bf16* __restrict__ C, const bf16* __restrict__ bias,
            int M, int N, int K) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const unsigned ATILE = BM * BK * 2;          // bytes per A tile (8 KiB)
  const unsigned BUF = 2 * ATILE;              // A+B per buffer (16 KiB)

  unsigned nwg_m = (M + BM - 1) / BM, nwg_n = (N + BN - 1) / BN;
  unsigned wg = xcd_swizzle(blockIdx.x, nwg_m * nwg_n);
  const unsigned m0 = (wg / nwg_n) * BM;
  const unsigned n0 = (wg % nwg_n) * BN;

  const int t = threadIdx.x;
  const int lane = t % WAVE;
  const int wave = t / WAVE;
  const int wm = (wave / 2) * 64;   // wave row offset in tile
  const int wn = (wave % 2) * 64;   // wave col offset

  // stage: 256 threads x 16 B = 4 KiB per pass; 2 passes per tile.
  // Source rows are CLAMPED so edge blocks read valid (duplicated) data;
  // the epilogue guard masks the stores.
  auto stage = [&](int buf, int k0) {
    #pragma unroll
    for (int p = 0; p < 2; ++p) {
      int e = (t + p * 256) * 8;              // element offset in tile
      int row = e / BK, col = e % BK;
      int grow = min((int)m0 + row, M - 1);
      const bf16* src = A + (long)grow * K + k0 + col;
      glds16(src, smem + buf * BUF + (p * 256 + wave * 64) * 16);
    }
    #pragma unroll
    for (int p = 0; p < 2; ++p) {
      int e = (t + p * 256) * 8;
      int row = e / BK, col = e % BK;
      int grow = min((int)n0 + row, N - 1);
      const bf16* src = Bt + (long)grow * K + k0 + col;
      glds16(src, smem + buf * BUF + ATILE + (p * 256 + wave * 64) * 16);
    }
  };

  f32x4 acc[4][4];
  #pragma unroll
  for (int i = 0; i < 4; ++i)
    #pragma unroll
    for (int j = 0; j < 4; ++j)
      acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  stage(0, 0);
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();

  const int frag_row = lane & 15;        // row inside 16-row fragment
  const int frag_k = (lane >> 4) * 8;    // k offset (8 contiguous bf16)

  int nk = K / BK;
  for (int kt = 0; kt < nk; ++kt) {
    int buf = kt & 1;
    if (kt + 1 < nk) stage(buf ^ 1, (kt + 1) * BK);
    bf16x8v a_frag[4], b_frag[4];
    const char* base = smem;
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned off = buf * BUF + ((wm + i * 16 + frag_row) * BK + frag_k) * 2;
      a_frag[i] = *reinterpret_cast<const bf16x8v*>(base + off);
    }
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned off = buf * BUF + ATILE +
                     ((wn + j * 16 + frag_row) * BK + frag_k) * 2;
      b_frag[j] = *reinterpret_cast<const bf16x8v*>(base + off);
    }
    #pragma unroll
    for (int i = 0; i < 4; ++i)
      #pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a_frag[i], b_frag[j], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
  }

  const int c_col = lane & 15;
  const int c_row0 = (lane >> 4) * 4;
  // hoisted bias loads: a per-element `if (bias) load` makes hipcc emit a
  // branch + vmcnt(0) per element (64 dependent L2 round trips)
  float bias_v[4] = {0.f, 0.f, 0.f, 0.f};
  if (bias) {
    #pragma unroll
    for (int j = 0; j < 4; ++j)
      bias_v[j] = bf2f(bias[min((int)(n0 + wn + j * 16 + c_col), N - 1)]);
  }
  #pragma unroll
  for (int i = 0; i < 4; ++i) {
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
      #pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        int gm = m0 + wm + i * 16 + c_row0 + reg;
        int gn = n0 + wn + j * 16 + c_col;
        if (gm < M && gn < N)
          C[(long)gm * N + gn] = f2bf(acc[i][j][reg] + bias_v[j]);
      }
    }
  }
}

// ===========================================================================
// gemm_nt_256: the 8-phase 256x256x64 template.
//
// LDS map (128 KiB, ONE extern __shared__ object -- a second one makes
// hipcc drain vmcnt before every ds_read, cdna_hip_programming.md §5
// ".s-level traps" (a)):
//   buf b (0/1) at b*65536:
//     A half h at h*16384:   rows r of the 256-row block with
//         ((r>>6)&1)==h, as [stripe s=r>>7][r&63][64 k] bf16
//     B half h at 32768 + h*16384: cols c with ((c>>5)&1)==h, as
//         [stripe s=c>>6][c&31][64 k]
// The halves interleave 64-row / 32-col stripes so that one compute
// QUADRANT (mh,nh) of every wave touches exactly one A half and one B
// half -- that makes half-granular staging safe with barriers only.
//
// Phase schedule per K-tile T (quadrants (mh,nh) in order
// (0,0),(0,1),(1,1),(1,0) so consecutive phases share one operand half):
//   q0: read A-h0+B-h0 (12x ds_read_b128)   stage B-h0(T+1)
//   q1: read B-h1 (4)    [A-h0 kept in reg] stage A-h0(T+2)
//   q2: read A-h1 (8)    [B-h1 kept]        stage B-h1(T+2)
//   q3: read B-h0 (4)    [A-h1 kept]        stage A-h1(T+2), vmcnt(6)
// Each phase: reads; one half staged (2 glds/thread); barrier;
// (compiler-inserted lgkmcnt) setprio(1); 16 MFMA; setprio(0); barrier.
// vmcnt(6) before q3's closing barrier leaves exactly the 3 newest
// staged halves (6 loads) in flight -- everything the next tile's q0/q1
// reads has landed.  Prologue stages 7 halves (tile0 + A0,B1,A1 of
// tile1); B0(1) is staged by q0 of tile 0.
// ===========================================================================
#define BM2 256
#define BN2 256
#define BK2 64
#define HALF_B 16384u
#define BUF_B 65536u

// XOR swizzle on a within-half byte offset (T2, rule 21).  The row bits
// (>=7: 128-B rows) are folded into the 16-B-slot bits so that the 16
// lanes of one ds_read_b128 service group land on distinct banks: row
// bits 8-10 go to slot bits 4-6, conflict-free for contiguous groups
// {16g..16g+15}.  The 1-bit st_16x32 form and a 2-bit form for strided
// groups were A/B'd on hardware and lost.
DEVINL unsigned sw32(unsigned x) { return x ^ (((x >> 8) & 7u) << 4); }

// gemm_nt_256's A half (staging, fragment reads) and epilogue as functions,
// for gemm_nn_256, which takes the same A [M,K] and ends with the same
// accumulator layout.  gemm_nt_256 keeps its own inline copies: built on
// these functions its ISA changed and it measured 1.5-2% slower at two of
// five shapes (profiles/README.md Round 17).
//
// One A half = 16 KiB = 2 glds/thread to smem + dst0.  The LDS image is
// lane-linear; the inverse st_16x32 swizzle is applied to the per-lane
// SOURCE address, source rows clamped to M-1.
DEVINL void g256_stage_a(const bf16* __restrict__ A, int M, int K, unsigned m0,
                         int k0, int h, char* smem, unsigned dst0, int t,
                         int wave) {
  #pragma unroll
  for (int i = 0; i < 2; ++i) {
    unsigned p = (i * 512 + t) * 16;          // linear byte pos in half
    unsigned L = sw32(p);                     // logical (image) byte
    int s = L >> 13;                          // stripe (8 KiB each)
    int row = (L >> 7) & 63;
    int k = (L & 127) >> 1;
    int grow = min((int)m0 + s * 128 + h * 64 + row, M - 1);
    glds16(A + (long)grow * K + k0 + k,
           smem + dst0 + (i * 512 + wave * 64) * 16);
  }
}

// wave row wr's 64 rows x 64 k of the A half at smem + base as MFMA fragments
// (swizzled ds_read_b128)
DEVINL void g256_read_a(bf16x8v (&a)[4][2], const char* smem, unsigned base,
                        int wr, int fr, int fg) {
  #pragma unroll
  for (int i = 0; i < 4; ++i)
    #pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      unsigned L = wr * 8192u + (i * 16 + fr) * 128u + (kk * 32 + fg * 8) * 2u;
      a[i][kk] = *reinterpret_cast<const bf16x8v*>(smem + base + sw32(L));
    }
}

// LDS-bounced coalesced stores of a wave's 128x64 accumulators (rows
// wr*128.., cols wc*64.. of the tile at (m0, n0); a lane holds col l&15,
// rows (l>>4)*4+r of each 16x16 block), bias and activation applied.  The
// caller has drained the LDS-DMA queue and passed a barrier.
DEVINL void g256_epilogue(f32x4 (&acc)[8][4], char* smem,
                          bf16* __restrict__ C, const bf16* __restrict__ bias,
                          bf16* __restrict__ aux, int act, int M, int N,
                          unsigned m0, unsigned n0, int wave, int lane) {
  const int fr = lane & 15, fg = lane >> 4;
  // Repurpose the wave's 16 KiB share as a [128][64] bf16 bounce so
  // global stores are 16-B wide and row-contiguous.
  bf16* share = reinterpret_cast<bf16*>(smem) + wave * 8192;
  const unsigned wm = (wave >> 2) * 128, wn = (wave & 3) * 64;
  // hoisted bias loads (4 per lane) -- see gemm_nt_128 epilogue note
  float bias_v[4] = {0.f, 0.f, 0.f, 0.f};
  if (bias) {
    #pragma unroll
    for (int j = 0; j < 4; ++j)
      bias_v[j] = bf2f(bias[min((int)(n0 + wn + j * 16 + fr), N - 1)]);
  }
  #pragma unroll
  for (int i = 0; i < 8; ++i)
    #pragma unroll
    for (int j = 0; j < 4; ++j)
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = i * 16 + fg * 4 + r;
        int col = j * 16 + fr;
        share[row * 64 + col] = f2bf(acc[i][j][r] + bias_v[j]);
      }
  lds_fence();   // own-wave LDS writes -> reads; no cross-wave traffic
  #pragma unroll
  for (int tt = 0; tt < 16; ++tt) {
    int row = tt * 8 + (lane >> 3);
    int colc = (lane & 7) * 8;
    int gm = m0 + wm + row;
    int gn = n0 + wn + colc;
    if (gm < (int)M && gn + 8 <= (int)N) {
      bf16x8v val = *reinterpret_cast<const bf16x8v*>(&share[row * 64 + colc]);
      if (act) {
        bf16x8v av{};
        if (act == 2 || act == 4)
          av = *reinterpret_cast<const bf16x8v*>(&aux[(long)gm * N + gn]);
        else if (act >= 5)   // fused fwd: keep pre-act for gelu_backward
          *reinterpret_cast<bf16x8v*>(&aux[(long)gm * N + gn]) = val;
        #pragma unroll
        for (int e = 0; e < 8; ++e)
          val[e] = (__bf16)act_apply(act, bf2f((bf16)val[e]),
                                     bf2f((bf16)av[e]));
      }
      *reinterpret_cast<bf16x8v*>(&C[(long)gm * N + gn]) = val;
    } else if (gm < (int)M) {
      for (int e = 0; e < 8 && gn + e < (int)N; ++e) {
        float xv = bf2f(share[row * 64 + colc + e]);
        float axv = (act == 2 || act == 4)
                        ? bf2f(aux[(long)gm * N + gn + e]) : 0.f;
        if (act >= 5) aux[(long)gm * N + gn + e] = f2bf(xv);
        C[(long)gm * N + gn + e] = f2bf(act_apply(act, xv, axv));
      }
    }
  }
}

extern "C" __global__ void __launch_bounds__(512)
gemm_nt_256(const bf16* __restrict__ A, const bf16* __restrict__ Bt,
            bf16* __restrict__ C, const bf16* __restrict__ bias,
            bf16* __restrict__ aux, int act, int M, int N, int K) {
  // aux: INPUT for bwd modes 2/4 (saved pre-act), OUTPUT for fwd 5/6
  extern __shared__ __attribute__((aligned(16))) char smem[];

  unsigned nwg_m = (M + BM2 - 1) / BM2, nwg_n = (N + BN2 - 1) / BN2;
  unsigned wg = xcd_swizzle(blockIdx.x, nwg_m * nwg_n);
  const unsigned m0 = (wg / nwg_n) * BM2;
  const unsigned n0 = (wg % nwg_n) * BN2;

  const int t = threadIdx.x;
  const int lane = t % WAVE;
  const int wave = t / WAVE;
  const int wr = wave >> 2;           // wave row (0/1): rows wr*128..+128
  const int wc = wave & 3;            // wave col (0..3): cols wc*64..+64

  // ---- staging ------------------------------------------------------------
  // One A half = 16 KiB = 2 glds/thread.  LDS image is lane-linear; the
  // inverse st_16x32 swizzle is applied to the per-lane SOURCE address.
  // (parity, k0) are passed separately: near the K-tail the schedule
  // issues DUMMY stages (k0 = 0) into just-freed slots so the glds count
  // per phase stays constant -- s_waitcnt vmcnt(6) counts outstanding
  // loads, and a skipped stage would silently weaken the guarantee for
  // the loads that remain (wrong results at NT <= 2 and on the last two
  // tiles).
  auto stage_a = [&](int parity, int k0, int h) {
    unsigned dst0 = parity * BUF_B + h * HALF_B;
    #pragma unroll
    for (int i = 0; i < 2; ++i) {
      unsigned p = (i * 512 + t) * 16;          // linear byte pos in half
      unsigned L = sw32(p);                     // logical (image) byte
      int s = L >> 13;                          // stripe (8 KiB each)
      int row = (L >> 7) & 63;
      int k = (L & 127) >> 1;
      int grow = min((int)m0 + s * 128 + h * 64 + row, M - 1);
      glds16(A + (long)grow * K + k0 + k,
             smem + dst0 + (i * 512 + wave * 64) * 16);
    }
  };
  auto stage_b = [&](int parity, int k0, int h) {
    unsigned dst0 = parity * BUF_B + 32768u + h * HALF_B;
    #pragma unroll
    for (int i = 0; i < 2; ++i) {
      unsigned p = (i * 512 + t) * 16;
      unsigned L = sw32(p);
      int s = (L >> 12) & 3;                    // stripe (4 KiB each)
      int col = (L >> 7) & 31;
      int k = (L & 127) >> 1;
      int gcol = min((int)n0 + s * 64 + h * 32 + col, N - 1);
      glds16(Bt + (long)gcol * K + k0 + k,
             smem + dst0 + (i * 512 + wave * 64) * 16);
    }
  };

  // ---- fragment reads (swizzled ds_read_b128) -----------------------------
  const int fr = lane & 15;
  const int fg = lane >> 4;
  auto read_a = [&](bf16x8v (&a)[4][2], int tile, int mh) {
    unsigned base = (tile & 1) * BUF_B + mh * HALF_B;
    #pragma unroll
    for (int i = 0; i < 4; ++i)
      #pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        unsigned L = wr * 8192u + (i * 16 + fr) * 128u +
                     (kk * 32 + fg * 8) * 2u;
        a[i][kk] = *reinterpret_cast<const bf16x8v*>(smem + base + sw32(L));
      }
  };
  auto read_b = [&](bf16x8v (&b)[2][2], int tile, int nh) {
    unsigned base = (tile & 1) * BUF_B + 32768u + nh * HALF_B;
    #pragma unroll
    for (int j = 0; j < 2; ++j)
      #pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        unsigned L = wc * 4096u + (j * 16 + fr) * 128u +
                     (kk * 32 + fg * 8) * 2u;
        b[j][kk] = *reinterpret_cast<const bf16x8v*>(smem + base + sw32(L));
      }
  };

  f32x4 acc[8][4];
  #pragma unroll
  for (int i = 0; i < 8; ++i)
    #pragma unroll
    for (int j = 0; j < 4; ++j)
      acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  bf16x8v a_frag[4][2], b_frag[2][2], b0_frag[2][2];
  const int NT = K / BK2;

  // k0 of tile t, clamped to a dummy (t >= NT: data never read)
  auto k_of = [&](int t) { return t < NT ? t * BK2 : 0; };

  // prologue: tile0 fully + A0,B1,A1 of tile1 (B0(1) staged in q0 of T=0);
  // always 7 halves = 14 loads so vmcnt(6) drains exactly tile 0
  stage_a(0, 0, 0); stage_a(0, 0, 1); stage_b(0, 0, 0); stage_b(0, 0, 1);
  stage_a(1, k_of(1), 0); stage_b(1, k_of(1), 1); stage_a(1, k_of(1), 1);
  asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  raw_barrier();

  auto mfma_quad = [&](int mh, int nh, bf16x8v (&bf)[2][2]) {
    __builtin_amdgcn_s_setprio(1);
    #pragma unroll
    for (int i = 0; i < 4; ++i)
      #pragma unroll
      for (int j = 0; j < 2; ++j)
        #pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          acc[mh * 4 + i][nh * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_frag[i][kk], bf[j][kk], acc[mh * 4 + i][nh * 2 + j],
              0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };

  // ONE barrier per phase (the closing one).  Correctness argument: a
  // phase's ds_reads are consumed by its MFMAs, so they complete before
  // the closing barrier in program order; a glds staged in phase p+1
  // overwrites data whose last read was in a phase <= p, separated by at
  // least that closing barrier.  The pre-MFMA barrier of the textbook
  // template only phase-locks the waves -- dropping it lets a wave start
  // its MFMAs as soon as ITS reads land (measured: the two-barrier form
  // spent 8x hipBLASLt's cycles waiting on LDS).
  for (int T = 0; T < NT; ++T) {
    // q0: (mh0, nh0); BOTH B halves read here (B-h1(T) was staged a full
    // tile before B-h0(T), so the vmcnt that covers B-h0 covers it too) —
    // q1/q3 then have no LDS reads at all.
    read_a(a_frag, T, 0);
    read_b(b0_frag, T, 0);
    read_b(b_frag, T, 1);
    stage_b((T + 1) & 1, k_of(T + 1), 0);
    mfma_quad(0, 0, b0_frag);
    raw_barrier();
    // q1: (mh0, nh1) -- A and B-h1 kept
    stage_a(T & 1, k_of(T + 2), 0);
    mfma_quad(0, 1, b_frag);
    raw_barrier();
    // q2: (mh1, nh1) -- B kept
    read_a(a_frag, T, 1);
    stage_b(T & 1, k_of(T + 2), 1);
    mfma_quad(1, 1, b_frag);
    raw_barrier();
    // q3: (mh1, nh0) -- A kept, B-h0 kept from q0
    stage_a(T & 1, k_of(T + 2), 1);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    mfma_quad(1, 0, b0_frag);
    raw_barrier();
  }

  // ---- epilogue: LDS-bounced coalesced stores -----------------------------
  // DRAIN the LDS-DMA queue first: the tail iterations issued dummy
  // stages whose glds may still be in flight — without this they land on
  // top of the bounce data below (timing-dependent corruption, seen as
  // err~100 on the 50k-wide vocab GEMM).
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  raw_barrier();
  // Repurpose the wave's 16 KiB share as a [128][64] bf16 bounce so
  // global stores are 16-B wide and row-contiguous.
  bf16* share = reinterpret_cast<bf16*>(smem) + wave * 8192;
  const unsigned wm = wr * 128, wn = wc * 64;
  // hoisted bias loads (4 per lane) -- see gemm_nt_128 epilogue note
  float bias_v[4] = {0.f, 0.f, 0.f, 0.f};
  if (bias) {
    #pragma unroll
    for (int j = 0; j < 4; ++j)
      bias_v[j] = bf2f(bias[min((int)(n0 + wn + j * 16 + fr), N - 1)]);
  }
  #pragma unroll
  for (int i = 0; i < 8; ++i)
    #pragma unroll
    for (int j = 0; j < 4; ++j)
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = i * 16 + fg * 4 + r;
        int col = j * 16 + fr;
        share[row * 64 + col] = f2bf(acc[i][j][r] + bias_v[j]);
      }
  lds_fence();   // own-wave LDS writes -> reads; no cross-wave traffic
  #pragma unroll
  for (int tt = 0; tt < 16; ++tt) {
    int row = tt * 8 + (lane >> 3);
    int colc = (lane & 7) * 8;
    int gm = m0 + wm + row;
    int gn = n0 + wn + colc;
    if (gm < (int)M && gn + 8 <= (int)N) {
      bf16x8v val = *reinterpret_cast<const bf16x8v*>(&share[row * 64 + colc]);
      if (act) {
        bf16x8v av{};
        if (act == 2 || act == 4)
          av = *reinterpret_cast<const bf16x8v*>(&aux[(long)gm * N + gn]);
        else if (act >= 5)   // fused fwd: keep pre-act for gelu_backward
          *reinterpret_cast<bf16x8v*>(&aux[(long)gm * N + gn]) = val;
        #pragma unroll
        for (int e = 0; e < 8; ++e)
          val[e] = (__bf16)act_apply(act, bf2f((bf16)val[e]),
                                     bf2f((bf16)av[e]));
      }
      *reinterpret_cast<bf16x8v*>(&C[(long)gm * N + gn]) = val;
    } else if (gm < (int)M) {
      for (int e = 0; e < 8 && gn + e < (int)N; ++e) {
        float xv = bf2f(share[row * 64 + colc + e]);
        float axv = (act == 2 || act == 4)
                        ? bf2f(aux[(long)gm * N + gn + e]) : 0.f;
        if (act >= 5) aux[(long)gm * N + gn + e] = f2bf(xv);
        C[(long)gm * N + gn + e] = f2bf(act_apply(act, xv, axv));
      }
    }
  }
}

// ===========================================================================
// gemm_tn: C[P,Q] = sum_r A[r,P]*B[r,Q], fp32 atomic accumulation into a
// workspace (split-R fills the 256 CUs when P*Q is small -- dW shapes).
// ONE kernel template over the output tile edge TILE:
//   128: 4 waves of 64x64   -- edge + small shapes
//   256: 8 waves of 64x128  -- operand re-read traffic scales with
//        1/tile_edge (A is re-read Q/tile times, B P/tile times).
//        Occupancy is VGPR-bound at 2 waves/SIMD (acc[4][8] = 128 VGPRs),
//        one workgroup per CU.
// Tiles: BR=32 x TILE; both operands stage k(r)-major via glds (coalesced:
// global rows ARE r-rows) into tr-read images:
//   image = [pchunk p/16][rblock swz(r/4)][4 r][16 p] bf16, where the
//   r-blocks are stored in order 0-3,8-11,16-19,24-27,4-7,... so that one
//   ds_read_b64_tr_b16 serves each 16-lane group the k-range its MFMA
//   fragment needs (fragment k = 8*(l>>4)+0..7 -> read1 blocks {0,2,4,6},
//   read2 at +512 B blocks {1,3,5,7}).
//
// What bounds the r-loop (measured on the 256 tile, profiles/README.md
// Round 4): NOT HBM.  At the 65536-row dW shapes the issue-then-drain loop
// pulled 3-4 TB/s from beyond the L2 with the MFMA pipe ~40% busy; it sat
// on the loaded latency of the ONE stage it kept in flight and drained
// before every barrier.  Moving the operand re-reads into the L2
// (slice-major map, gemm_tn_map.h: beyond-L2 bytes -54..-62%) bought only
// 1-6%; keeping two stages in flight (the ring below) bought 7-24%.
// ===========================================================================
#define TBR 32
#define TBP 128      // the two output tile edges
#define TBP2 256

// bytes of one operand's tr-image, and of a kernel's whole LDS footprint
// (A+B images per buffer; 3 buffers for the ring, 2 for the drain loop)
constexpr unsigned tn_img_bytes(int tile) { return TBR * tile * 2; }
constexpr unsigned tn_lds_bytes(int tile, int ring) {
  return (ring ? 3 : 2) * 2 * tn_img_bytes(tile);
}

// r-block storage order: even blocks first (see header comment)
DEVINL int tn_unswz(int pos) { return ((pos >> 2) & 1) | ((pos & 3) << 1); }

// one tr-image stage with NTHR threads: tile [32 r][NTHR/2 p] from src rows
// r0.., cols p0.. (16 B per thread per pass, two passes)
template <int NTHR>
DEVINL void tn_stage(const bf16* src, long ld, int r0, int p0, int pmax,
                     char* dst_base, int t, int wave) {
  #pragma unroll
  for (int i = 0; i < 2; ++i) {
    unsigned p = (i * NTHR + t) * 16;         // linear byte pos in the image
    int chunk16 = p >> 10;                    // 1 KiB per 16-p chunk
    unsigned w = p & 1023u;
    int bpos = w >> 7;                        // 128 B per [4r][16p] block
    int blk = tn_unswz(bpos);
    int rr = blk * 4 + ((w & 127) >> 5);
    int pp = chunk16 * 16 + ((w & 31) >> 1);
    // clamp keeps the full 16-B read inside the operand (the last
    // partial tile's rows would otherwise read past the buffer end)
    int gp = min(p0 + pp, pmax - 8);
    glds16(src + (long)(r0 + rr) * ld + gp,
           dst_base + (i * NTHR + wave * 64) * 16);
  }
}

DEVINL bf16x8v tn_frag(const char* img, int chunk, int lane) {
  const char* base = img + chunk * 1024 + (lane >> 4) * 128 + (lane & 15) * 8;
  v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) v4s*)base);
  v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) v4s*)(base + 512));
  v8s out = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8v, out);
}

// TILE in {128, 256}: 2*TILE threads, waves of 64 x TILE/2 outputs.
// RING selects the r-loop's staging:
//   1  three 32-row buffers, two stages in flight: counted vmcnt(4) (a
//      stage is 4 glds per thread) and a raw barrier -- never
//      __syncthreads, whose fence would drain the stage in flight.  Shipped
//      for the 256 tile (96 KiB); not instantiated (nor measured) for 128.
//   0  two buffers: stage rt+1, compute rt, drain, barrier.  The 128 tile's
//      loop (32 KiB), and the 256 tile's older one, kept for A/B (64 KiB).
template <int TILE, int RING>
DEVINL void tn_body(const bf16* __restrict__ Ag, const bf16* __restrict__ Bg,
                    float* __restrict__ Cw, float* __restrict__ Asum, int R,
                    int P, int Q, int splitr, int map_mode) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NTHR = 2 * TILE;               // 256 / 512
  constexpr int NJ = TILE / 32;                // 16-col fragments per wave
  const unsigned IMG = tn_img_bytes(TILE);     // 8 / 16 KiB per operand image
  const unsigned BUF = 2 * IMG;                // A+B per buffer

  // ceil-div: partial edge tiles are safe — staging clamps the source
  // row to pmax-1 (duplicate loads) and the store loop guards gp/gq
  unsigned nwg_p = (P + TILE - 1) / TILE, nwg_q = (Q + TILE - 1) / TILE;
  unsigned ntile = nwg_p * nwg_q;
  const TnBlock blk = gemm_tn_map(blockIdx.x, ntile, splitr, map_mode);
  const unsigned tile = blk.tile, slice = blk.slice;
  const unsigned p0 = (tile / nwg_q) * TILE;
  const unsigned q0 = (tile % nwg_q) * TILE;

  // this slice's r-range (R % 32 == 0 enforced by host)
  int nrt_all = R / TBR;
  int per = (nrt_all + splitr - 1) / splitr;
  int rt0 = slice * per;
  int rt1 = min(nrt_all, rt0 + per);
  if (rt0 >= rt1) return;

  const int t = threadIdx.x;
  const int lane = t % WAVE;
  const int wave = t / WAVE;
  const int wp = (wave >> 1) * 64;             // TILE/64 p-rows of waves
  const int wq = (wave & 1) * (TILE / 2);      // 2 q-cols of waves

  // r-tile rt into buffer buf (past rt1: skipped, uniformly over the
  // workgroup)
  auto stage = [&](int buf, int rt) {
    if (rt < rt1) {
      tn_stage<NTHR>(Ag, P, rt * TBR, p0, P, smem + buf * BUF, t, wave);
      tn_stage<NTHR>(Bg, Q, rt * TBR, q0, Q, smem + buf * BUF + IMG, t, wave);
    }
  };

  f32x4 acc[4][NJ];
  float asum_acc[4] = {0.f, 0.f, 0.f, 0.f};
  #pragma unroll
  for (int i = 0; i < 4; ++i)
    #pragma unroll
    for (int j = 0; j < NJ; ++j)
      acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  // one 32-row k-step from the images at img
  auto compute = [&](const char* img) {
    bf16x8v a_frag[4], b_frag[NJ];
    #pragma unroll
    for (int i = 0; i < 4; ++i)
      a_frag[i] = tn_frag(img, (wp >> 4) + i, lane);
    if (Asum && q0 == 0 && (wave & 1) == 0) {
      // dBias fused into dW (only the q0==0 block column: A tiles repeat
      // across q tiles): the A operand (dY) is already on chip —
      // column-sum it here instead of a separate full re-read
      #pragma unroll
      for (int i = 0; i < 4; ++i) {
        float acc_s = 0.f;
        #pragma unroll
        for (int u = 0; u < 8; ++u) acc_s += bf2f((bf16)a_frag[i][u]);
        asum_acc[i] += acc_s;
      }
    }
    #pragma unroll
    for (int j = 0; j < NJ; ++j)
      b_frag[j] = tn_frag(img + IMG, (wq >> 4) + j, lane);
    #pragma unroll
    for (int i = 0; i < 4; ++i)
      #pragma unroll
      for (int j = 0; j < NJ; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a_frag[i], b_frag[j], acc[i][j], 0, 0, 0);
  };

  if constexpr (RING) {
    stage(0, rt0);
    stage(1, rt0 + 1);
    int buf = 0;
    for (int rt = rt0; rt < rt1; ++rt) {
      // stage rt has landed once at most stage rt+1 is still in flight
      if (rt + 1 < rt1)
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      // every wave's share of rt is in LDS, and every wave is done reading
      // rt-1 (its MFMAs consumed those reads), whose buffer stage rt+2
      // overwrites
      raw_barrier();
      stage(buf == 0 ? 2 : buf - 1, rt + 2);
      compute(smem + buf * BUF);
      buf = buf == 2 ? 0 : buf + 1;
    }
  } else {
    stage(0, rt0);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    for (int rt = rt0; rt < rt1; ++rt) {
      int buf = (rt - rt0) & 1;
      stage(buf ^ 1, rt + 1);
      compute(smem + buf * BUF);
      __builtin_amdgcn_s_waitcnt(0);
      __syncthreads();
    }
  }

  if (Asum && q0 == 0 && (wave & 1) == 0) {
    // fold the r-slice partials (lanes l and l+16/32/48 share a column)
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v = asum_acc[i];
      v += __shfl_down(v, 32, WAVE);
      v += __shfl_down(v, 16, WAVE);
      if (lane < 16) {
        int gp = p0 + wp + i * 16 + lane;
        if (gp < P) atomicAdd(&Asum[gp], v);
      }
    }
  }
  const int c_col = lane & 15;
  const int c_row0 = (lane >> 4) * 4;
  #pragma unroll
  for (int i = 0; i < 4; ++i)
    #pragma unroll
    for (int j = 0; j < NJ; ++j)
      #pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        int gp = p0 + wp + i * 16 + c_row0 + reg;
        int gq = q0 + wq + j * 16 + c_col;
        if (gp < P && gq < Q) {
          if (splitr == 1)
            Cw[(long)gp * Q + gq] = acc[i][j][reg];
          else
            atomicAdd(&Cw[(long)gp * Q + gq], acc[i][j][reg]);
        }
      }
}

// the entry names are what traces, profiles/*.csv and bench_gemm.py match
#define TN_KERNEL(name, tile, ring)                                         \
  extern "C" __global__ void __launch_bounds__(2 * tile)                    \
  name(const bf16* __restrict__ Ag, const bf16* __restrict__ Bg,            \
       float* __restrict__ Cw, float* __restrict__ Asum, int R, int P,      \
       int Q, int splitr, int map_mode) {                                   \
    tn_body<tile, ring>(Ag, Bg, Cw, Asum, R, P, Q, splitr, map_mode);       \
  }
TN_KERNEL(gemm_tn_kernel, TBP, 0)
TN_KERNEL(gemm_tn_256_kernel, TBP2, 1)
TN_KERNEL(gemm_tn_256_drain_kernel, TBP2, 0)

// ===========================================================================
// gemm_nn_256: C[M,N] = A[M,K] @ B[K,N] (+bias[N]), act_apply epilogue -- the
// dX backward (dX = dY @ W) on the weight as it lies in memory.  No
// transposed copy of B exists anywhere, in HBM or in LDS.
// Takes M >= 256, N >= 256, K % 64 == 0, N % 8 == 0; everything else in the
// op's envelope goes to gemm_nn_128 (moe_nn_body).
//
// 256x256 output tile, 8 waves (wave (wr, wc): rows wr*128..+128, cols
// wc*64..+64, acc[8][4]), 64 k per tile: gemm_nt_256's frame with a B side
// of its own.
//
// LDS map (128 KiB, one extern __shared__ object), buf b (0/1) at b*65536:
//   A half h at h*16384: gemm_nt_256's image (g256_stage_a / g256_read_a:
//       glds with the swizzle on the source address, rows clamped to M-1)
//   B image h at 32768 + h*16384: k-rows h*32..+32 of the tile, all 256
//       columns, as tn_stage<512>'s tr-read image.  Global rows ARE k-rows,
//       so the stage is coalesced along N; tn_stage's pmax - 8 clamp keeps
//       the N edge tile's reads inside the row (duplicate columns, masked
//       by the epilogue).  tn_frag (2 ds_read_b64_tr_b16) gives "n = l&15,
//       k = 8*(l>>4)+0..7" -- the operand form the A fragment has for its
//       rows, so image h pairs with the A fragments' kk = h.
//
// MFMA operand order: mfma(a_frag, b_frag), D[m][n] as in gemm_nt_256 (a lane
// ends with col l&15, rows (l>>4)*4+r), NOT moe_nn's transposed product: the
// epilogue is then gemm_nt_256's, as a function (g256_epilogue), and its
// per-wave bounce needs no cross-wave barrier.
//
// Phase schedule per K-tile T.  gemm_nt_256 splits B by column halves and a
// phase is a (row half, column half) quadrant; here B splits by k, so a
// phase is (row half mh, k half kh): 4 i x 4 j x 1 kk = the same 16 MFMAs,
// order (0,0),(0,1),(1,1),(1,0) so consecutive phases share one operand:
//   q0: read A-h0 (8x ds_read_b128), B-img0 + B-img1 (16x tr_b64)
//                                          stage B-img0(T+1)
//   q1: [A-h0, B-img1 kept in registers]   stage A-h0(T+2)
//   q2: read A-h1 (8)   [B-img1 kept]      stage B-img1(T+2)
//   q3: [A-h1, B-img0 kept]                stage A-h1(T+2), vmcnt(6)
// Every half is read in the same phase as its gemm_nt_256 counterpart and
// every stage is 2 glds per thread, so that kernel's arguments carry over
// unchanged: one closing raw barrier per phase, vmcnt(6) leaving the 3
// newest halves in flight, 7 halves in the prologue, dummy stages (k0 = 0,
// valid memory, never read) at the K tail so the count stays constant.
// Never __syncthreads: its fence would drain the LDS-DMA in flight.
//
// Workgroup order: xcd_swizzle with the column tile fastest, as gemm_nt_256.
// For dX, M is the token count and N the layer width: the N/256 (3 to 12)
// consecutive workgroups of one XCD stream one A row panel from HBM once and
// cycle through the few B column panels, each re-used every N/256-th
// workgroup and L2-resident (the whole weight is a few MiB).
//
// The body is an inlined function under a thin kernel, as tn_body is: written
// straight into the kernel, hipcc put an s_waitcnt vmcnt(0) in front of q0's
// tr reads (it was in the ISA), which drains the stages in flight once per
// tile.  Check the loop's ISA after touching this: one vmcnt(6), no vmcnt(0).
// ===========================================================================
DEVINL void nn256_body(const bf16* __restrict__ A, const bf16* __restrict__ B,
                       bf16* __restrict__ C, const bf16* __restrict__ bias,
                       bf16* __restrict__ aux, int act, int M, int N, int K) {
  // aux: INPUT for bwd modes 2/4 (saved pre-act), OUTPUT for fwd 5/6
  extern __shared__ __attribute__((aligned(16))) char smem[];

  unsigned nwg_m = (M + BM2 - 1) / BM2, nwg_n = (N + BN2 - 1) / BN2;
  unsigned wg = xcd_swizzle(blockIdx.x, nwg_m * nwg_n);
  const unsigned m0 = (wg / nwg_n) * BM2;
  const unsigned n0 = (wg % nwg_n) * BN2;

  const int t = threadIdx.x;
  const int lane = t % WAVE;
  const int wave = t / WAVE;
  const int wr = wave >> 2;           // wave row (0/1): rows wr*128..+128
  const int wc = wave & 3;            // wave col (0..3): cols wc*64..+64
  const int fr = lane & 15;
  const int fg = lane >> 4;

  auto stage_a = [&](int parity, int k0, int h) {
    g256_stage_a(A, M, K, m0, k0, h, smem, parity * BUF_B + h * HALF_B, t,
                 wave);
  };
  auto stage_b = [&](int parity, int k0, int h) {
    tn_stage<512>(B, N, k0 + h * 32, (int)n0, N,
                  smem + parity * BUF_B + 32768u + h * HALF_B, t, wave);
  };
  auto read_a = [&](bf16x8v (&a)[4][2], int tile, int mh) {
    g256_read_a(a, smem, (tile & 1) * BUF_B + mh * HALF_B, wr, fr, fg);
  };
  // the wave's 4 column chunks of k image kh
  auto read_b = [&](bf16x8v (&b)[4], int tile, int kh) {
    const char* img = smem + (tile & 1) * BUF_B + 32768u + kh * HALF_B;
    #pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = tn_frag(img, wc * 4 + j, lane);
  };

  f32x4 acc[8][4];
  #pragma unroll
  for (int i = 0; i < 8; ++i)
    #pragma unroll
    for (int j = 0; j < 4; ++j)
      acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  bf16x8v a_frag[4][2], b0_frag[4], b1_frag[4];
  const int NT = K / BK2;

  // k0 of tile t, clamped to a dummy (t >= NT: data never read)
  auto k_of = [&](int t) { return t < NT ? t * BK2 : 0; };

  // prologue: tile0 fully + A0,B1,A1 of tile1 (B0(1) staged in q0 of T=0);
  // always 7 halves = 14 loads so vmcnt(6) drains exactly tile 0
  stage_a(0, 0, 0); stage_a(0, 0, 1); stage_b(0, 0, 0); stage_b(0, 0, 1);
  stage_a(1, k_of(1), 0); stage_b(1, k_of(1), 1); stage_a(1, k_of(1), 1);
  asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  raw_barrier();

  auto mfma_phase = [&](int mh, int kh, bf16x8v (&bf)[4]) {
    __builtin_amdgcn_s_setprio(1);
    #pragma unroll
    for (int i = 0; i < 4; ++i)
      #pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[mh * 4 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a_frag[i][kh], bf[j], acc[mh * 4 + i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };

  for (int T = 0; T < NT; ++T) {
    // q0: (mh0, k0); both B images read here (B-img1(T) was staged a full
    // tile before B-img0(T)), so q1/q3 have no LDS reads at all
    read_a(a_frag, T, 0);
    read_b(b0_frag, T, 0);
    read_b(b1_frag, T, 1);
    stage_b((T + 1) & 1, k_of(T + 1), 0);
    mfma_phase(0, 0, b0_frag);
    raw_barrier();
    // q1: (mh0, k1) -- A and B-img1 kept
    stage_a(T & 1, k_of(T + 2), 0);
    mfma_phase(0, 1, b1_frag);
    raw_barrier();
    // q2: (mh1, k1) -- B-img1 kept
    read_a(a_frag, T, 1);
    stage_b(T & 1, k_of(T + 2), 1);
    mfma_phase(1, 1, b1_frag);
    raw_barrier();
    // q3: (mh1, k0) -- A kept, B-img0 kept from q0
    stage_a(T & 1, k_of(T + 2), 1);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    mfma_phase(1, 0, b0_frag);
    raw_barrier();
  }

  // drain the dummy stages of the tail before the bounce reuses their LDS
  // (see gemm_nt_256)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  raw_barrier();
  g256_epilogue(acc, smem, C, bias, aux, act, M, N, m0, n0, wave, lane);
}

extern "C" __global__ void __launch_bounds__(512)
gemm_nn_256(const bf16* __restrict__ A, const bf16* __restrict__ B,
            bf16* __restrict__ C, const bf16* __restrict__ bias,
            bf16* __restrict__ aux, int act, int M, int N, int K) {
  nn256_body(A, B, C, bias, aux, act, M, N, K);
}

// ===========================================================================
// moe_nn: the MoE expert FFN forward, one grouped NN GEMM template.
//   plain :  C[e] = X[e] @ W[e]           X [E,R,K], W [E,K,N] -> C [E,R,N]
//   swiglu:  A[e] = X[e] @ W1[e], B[e] = X[e] @ W3[e],
//            H[e] = silu(A[e]) * B[e]     -> H, A, B [E,R,N]
// Expert weights are [K,N] with the reduce dim strided, so neither NT
// kernel serves them without a weight-sized transpose per call.  This kernel
// joins the two stagings the file already has: X rows are K-contiguous and
// stage like gemm_nt_128's A tile (128 rows x 32 k, source rows clamped to
// R-1); W rows ARE k-rows and stage k-major through tn_stage into the
// tr-read image, whose tn_frag gives the MFMA operand "n = l&15,
// k = 8*(l>>4)+0..7" that the linear X tile gives for its rows.
//
// One workgroup (4 waves) owns (expert, 128-row tile, column tile):
//   plain   128 columns, waves of 64x64, acc[4][4]
//   swiglu   64 columns of W1 and the same 64 of W3 (waves 0-1 stage the W1
//            image, waves 2-3 the W3 image), waves of 64x32 against both:
//            two acc[4][2] sets, the X tile staged ONCE for both products.
// Both keep 32 KiB of LDS, double-buffered: stage k+1, compute k, wait,
// barrier (the gemm_nt_128 / tn_body<128,0> loop).
//
// The MFMAs run transposed (W fragment as the A operand), so a lane ends
// with 4 CONSECUTIVE columns of one output row: 8-byte LDS writes into an
// XOR-swizzled [128][columns] bf16 tile (16-byte chunk c of row r sits at
// c ^ (r & (chunks-1))), read back as 16-byte vectors and stored as whole
// rows.  N % 8 == 0, so a vector is inside or outside the edge, never
// across it.  H comes from the fp32 accumulators and is rounded once.
//
// valid [E,R] (optional): a workgroup whose (at most 128) row flags are all
// clear writes zeros to its tile(s) and returns without touching X or W.
// Rows of X with a clear flag are zero by contract (moe_bins writes them),
// so skipping changes no output bit.  The zeros are plain stores: no
// memset node enters a captured graph (moe_kernels.hip's header).
//
// Block ids run row tile fastest, then column tile, then expert:
// consecutive workgroups share one [K, columns] weight panel.
// ===========================================================================
#define NN_BM 128
#define NN_BK 32
using bf16x4v = __attribute__((ext_vector_type(4))) __bf16;

template <bool SWIGLU, bool BIAS = false>
DEVINL void moe_nn_body(const bf16* __restrict__ X,
                        const bf16* __restrict__ W1,
                        const bf16* __restrict__ W3, bf16* __restrict__ Out,
                        bf16* __restrict__ Aout, bf16* __restrict__ Bout,
                        const unsigned char* __restrict__ valid, int R, int K,
                        int N, const bf16* __restrict__ bias = nullptr) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NP = SWIGLU ? 2 : 1;           // products per workgroup
  constexpr int TN = SWIGLU ? 64 : 128;        // output columns per product
  constexpr int NJ = TN / 32;                  // 16-col fragments per wave
  constexpr int CV = TN / 8;                   // 16-byte chunks per tile row
  constexpr unsigned ATILE = NN_BM * NN_BK * 2;   // X tile, 8 KiB
  constexpr unsigned WIMG = NN_BK * TN * 2;       // one W image, 8 / 4 KiB
  constexpr unsigned BUF = ATILE + NP * WIMG;     // 16 KiB per buffer
  constexpr unsigned OTILE = NN_BM * TN * 2;      // epilogue tile, 32 / 16 KiB

  const unsigned nrt = (R + NN_BM - 1) / NN_BM, nct = (N + TN - 1) / TN;
  const int m0 = (blockIdx.x % nrt) * NN_BM;
  const int n0 = ((blockIdx.x / nrt) % nct) * TN;
  const long e = blockIdx.x / (nrt * nct);
  const long row0 = e * R;                     // expert e's first row

  const int t = threadIdx.x;
  const int lane = t % WAVE;
  const int wave = t / WAVE;
  const int wm = (wave / 2) * 64;              // wave row offset in the tile
  const int wn = (wave % 2) * (TN / 2);        // wave column offset

  // one output tile as whole rows of 16-byte vectors, vec(row, chunk) each
  auto store_tile = [&](bf16* __restrict__ dst, auto vec) {
    #pragma unroll
    for (int it = 0; it < NN_BM * CV / 256; ++it) {
      const int idx = it * 256 + t;
      const int row = idx / CV, c = idx % CV;
      const int gm = m0 + row, gn = n0 + c * 8;
      if (gm < R && gn < N)
        *reinterpret_cast<bf16x8v*>(dst + (row0 + gm) * N + gn) = vec(row, c);
    }
  };
  auto zeros = [](int, int) { return bf16x8v{}; };
  // ... from the swizzled epilogue tile in LDS
  auto from = [](const char* tile) {
    return [tile](int row, int c) {
      return *reinterpret_cast<const bf16x8v*>(
          tile + row * (TN * 2) + ((c ^ (row & (CV - 1))) * 16));
    };
  };

  if (valid) {
    // every wave reads all 128 flags, two per lane, and ballots: the same
    // answer in all four waves with no LDS object beside smem (a second one
    // makes hipcc drain vmcnt before every ds_read, see gemm_nt_256)
    const int r = m0 + lane;
    const int any = (r < R ? (int)valid[row0 + r] : 0)
                  | (r + 64 < R ? (int)valid[row0 + r + 64] : 0);
    if (__ballot(any) == 0) {
      store_tile(Out, zeros);
      if constexpr (SWIGLU) {
        store_tile(Aout, zeros);
        store_tile(Bout, zeros);
      }
      return;
    }
  }

  const bf16* Xe = X + row0 * K;
  const bf16* W1e = W1 + e * K * N;
  const bf16* W3e = SWIGLU ? W3 + e * K * N : nullptr;

  auto stage = [&](int buf, int k0) {
    char* dst = smem + buf * BUF;
    #pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int el = (t + p * 256) * 8;        // element offset in the tile
      const int row = el / NN_BK, col = el % NN_BK;
      const int grow = min(m0 + row, R - 1);
      glds16(Xe + (long)grow * K + k0 + col,
             dst + (p * 256 + wave * 64) * 16);
    }
    if constexpr (SWIGLU)
      tn_stage<128>(wave < 2 ? W1e : W3e, N, k0, n0, N,
                    dst + ATILE + (wave >> 1) * WIMG, t & 127, wave & 1);
    else
      tn_stage<256>(W1e, N, k0, n0, N, dst + ATILE, t, wave);
  };

  f32x4 acc[NP][4][NJ];
  #pragma unroll
  for (int p = 0; p < NP; ++p)
    #pragma unroll
    for (int i = 0; i < 4; ++i)
      #pragma unroll
      for (int j = 0; j < NJ; ++j)
        acc[p][i][j] = {0.f, 0.f, 0.f, 0.f};

  stage(0, 0);
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();

  const int frag_row = lane & 15;
  const int frag_k = (lane >> 4) * 8;
  const int nk = K / NN_BK;
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) stage(buf ^ 1, (kt + 1) * NN_BK);
    const char* base = smem + buf * BUF;
    bf16x8v x_frag[4], w_frag[NP][NJ];
    #pragma unroll
    for (int i = 0; i < 4; ++i)
      x_frag[i] = *reinterpret_cast<const bf16x8v*>(
          base + ((wm + i * 16 + frag_row) * NN_BK + frag_k) * 2);
    #pragma unroll
    for (int p = 0; p < NP; ++p)
      #pragma unroll
      for (int j = 0; j < NJ; ++j)
        w_frag[p][j] = tn_frag(base + ATILE + p * WIMG, (wn >> 4) + j, lane);
    // transposed product: D[n][row], a lane holds row (l&15) and columns
    // (l>>4)*4 + 0..3 of each 16x16 block
    #pragma unroll
    for (int p = 0; p < NP; ++p)
      #pragma unroll
      for (int i = 0; i < 4; ++i)
        #pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[p][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              w_frag[p][j], x_frag[i], acc[p][i][j], 0, 0, 0);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
  }

  // 4 columns of one row, rounded, into the swizzled epilogue tile
  auto put = [&](char* tile, int i, int j, f32x4 v) {
    const int row = wm + i * 16 + (lane & 15);
    const int col = wn + j * 16 + (lane >> 4) * 4;
    bf16x4v o;
    #pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = (__bf16)v[r];
    *reinterpret_cast<bf16x4v*>(
        tile + row * (TN * 2) + (((col >> 3) ^ (row & (CV - 1))) * 16)
        + (col & 4) * 2) = o;
  };

  if constexpr (SWIGLU) {
    #pragma unroll
    for (int i = 0; i < 4; ++i)
      #pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const f32x4 a = acc[0][i][j], b = acc[1][i][j];
        f32x4 h;
        #pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = a[r] * swiglu_sigmoid(a[r]) * b[r];
        put(smem, i, j, h);
        put(smem + OTILE, i, j, a);
      }
    __syncthreads();
    store_tile(Out, from(smem));
    store_tile(Aout, from(smem + OTILE));
    __syncthreads();
    #pragma unroll
    for (int i = 0; i < 4; ++i)
      #pragma unroll
      for (int j = 0; j < NJ; ++j)
        put(smem, i, j, acc[1][i][j]);
    __syncthreads();
    store_tile(Bout, from(smem));
  } else {
    if constexpr (BIAS) {
      // bias[N] (optional; the dense gemm_nn_128 only, the MoE entries are
      // built without): added in fp32 to the lane's 4 columns, so the output
      // is still rounded once
      if (bias) {
        #pragma unroll
        for (int j = 0; j < NJ; ++j) {
          f32x4 bv;
          #pragma unroll
          for (int r = 0; r < 4; ++r)
            bv[r] = bf2f(
                bias[min(n0 + wn + j * 16 + (lane >> 4) * 4 + r, N - 1)]);
          #pragma unroll
          for (int i = 0; i < 4; ++i) acc[0][i][j] += bv;
        }
      }
    }
    #pragma unroll
    for (int i = 0; i < 4; ++i)
      #pragma unroll
      for (int j = 0; j < NJ; ++j)
        put(smem, i, j, acc[0][i][j]);
    __syncthreads();
    store_tile(Out, from(smem));
  }
}

extern "C" __global__ void __launch_bounds__(256)
moe_nn_gemm_kernel(const bf16* __restrict__ X, const bf16* __restrict__ W,
                   bf16* __restrict__ C,
                   const unsigned char* __restrict__ valid, int R, int K,
                   int N) {
  moe_nn_body<false>(X, W, nullptr, C, nullptr, nullptr, valid, R, K, N);
}

extern "C" __global__ void __launch_bounds__(256)
moe_nn_swiglu_kernel(const bf16* __restrict__ X, const bf16* __restrict__ W1,
                     const bf16* __restrict__ W3, bf16* __restrict__ H,
                     bf16* __restrict__ A, bf16* __restrict__ B,
                     const unsigned char* __restrict__ valid, int R, int K,
                     int N) {
  moe_nn_body<true>(X, W1, W3, H, A, B, valid, R, K, N);
}

// gemm_nn_128: the dense NN GEMM for the shapes gemm_nn_256 does not take
// (M < 256, N < 256 or K % 64 != 0): moe_nn's plain form with one expert and
// no valid flags -- any M, N % 8 == 0, K % 32 == 0 -- plus the bias.
extern "C" __global__ void __launch_bounds__(256)
gemm_nn_128(const bf16* __restrict__ A, const bf16* __restrict__ B,
            bf16* __restrict__ C, const bf16* __restrict__ bias, int M, int N,
            int K) {
  moe_nn_body<false, true>(A, B, nullptr, C, nullptr, nullptr, nullptr, M, K,
                           N, bias);
}

// ===========================================================================
// moe_nt / moe_tn: the MoE expert FFN backward, grouped like moe_nn.
//   moe_nt (dX):  DX[e] = G1[e] @ W1[e]^T (+ G2[e] @ W2[e]^T)
//                 G [E,R,N], W [E,K,N] -> DX [E,R,K]
//   moe_tn (dW):  DW[e] = X[e]^T @ G[e]       X [E,R,K], G [E,R,N] -> [E,K,N]
//                 pair: DW1 = X^T @ G1 and DW3 = X^T @ G2 from one X image
// Both write bf16 from fp32 accumulators, each output rounded once, through
// moe_nn's XOR-swizzled epilogue tile (the MFMAs run transposed, so a lane
// ends with 4 consecutive columns of one output row) to whole-row 16-byte
// stores.  No atomics, no workspace: one workgroup owns one output tile.
//
// moe_nt: both operands are contiguous along the reduce dim N and stage like
// gemm_nt_128's tiles (128 rows x 32 n, source rows clamped to the operand's
// last row); 32 KiB double-buffered.  The two-product form runs ONE k-loop of
// 2 N/32 steps, the first half reading (G1, W1), the second (G2, W2), into the
// same accumulators: da @ w1^T + db @ w3^T leaves fp32 once.  A tile none of
// whose rows is valid is written as zeros (moe_nn's ballot test).  Block ids
// run row tile fastest, then column tile, then expert.
//
// moe_tn: both operands are R-strided and stage k(r)-major through tn_stage
// into tr-read images, as tn_body does.  One workgroup per (expert, 128 x 128
// output tile); the pair form stages the 128-wide X image ONCE per r-step
// against 64 columns of G1 and the same 64 of G2 (waves 0-1 stage G1, waves
// 2-3 G2), two acc[4][2] sets -- the mirror image of moe_nn's SwiGLU form.
// R need not be a multiple of 32: the partial last step goes through
// predicated register loads with zero fill (tn_stage_tail), so rows at or
// beyond R contribute nothing and nothing past the expert is read.
// With valid, every wave reads the expert's R flags (16-byte loads where the
// address allows), ballots per 32-row step and writes the same compact list
// of live steps, one uint16 each, behind the staging buffers in the dynamic
// LDS region (ceil(R/32) <= 4096: at most 8 KiB); the r-loop walks that list.
// Rows of X and G with a clear flag are zero by contract, so a skipped step
// changes no output bit; with no live step the tile is written as zeros.
// Block ids run K tile fastest, then N tile, then expert.
// ===========================================================================
// 4 columns (col % 4 == 0) of one row, rounded, into a swizzled [128][TN] tile
template <int TN>
DEVINL void moe_tile_put(char* tile, int row, int col, f32x4 v) {
  bf16x4v o;
  #pragma unroll
  for (int r = 0; r < 4; ++r) o[r] = (__bf16)v[r];
  *reinterpret_cast<bf16x4v*>(
      tile + row * (TN * 2) + (((col >> 3) ^ (row & (TN / 8 - 1))) * 16)
      + (col & 4) * 2) = o;
}

// a [128][TN] tile as whole rows of 16-byte vectors to dst[rows][ld] at
// (m0, n0); from the swizzled LDS tile, or zeros when tile is null
template <int TN>
DEVINL void moe_tile_store(bf16* __restrict__ dst, long ld, int m0, int n0,
                           int rows, const char* tile, int t) {
  constexpr int CV = TN / 8;
  #pragma unroll
  for (int it = 0; it < NN_BM * CV / 256; ++it) {
    const int idx = it * 256 + t;
    const int row = idx / CV, c = idx % CV;
    const int gm = m0 + row, gn = n0 + c * 8;
    if (gm < rows && gn < ld)
      *reinterpret_cast<bf16x8v*>(dst + (long)gm * ld + gn) = tile
          ? *reinterpret_cast<const bf16x8v*>(
                tile + row * (TN * 2) + ((c ^ (row & (CV - 1))) * 16))
          : bf16x8v{};
  }
}

template <bool TWO>
DEVINL void moe_nt_body(const bf16* __restrict__ G1,
                        const bf16* __restrict__ W1,
                        const bf16* __restrict__ G2,
                        const bf16* __restrict__ W2, bf16* __restrict__ DX,
                        const unsigned char* __restrict__ valid, int R, int K,
                        int N) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr unsigned ATILE = NN_BM * NN_BK * 2;   // one operand tile, 8 KiB
  constexpr unsigned BUF = 2 * ATILE;             // G + W per buffer

  const unsigned nrt = (R + NN_BM - 1) / NN_BM, nct = (K + 127) / 128;
  const int m0 = (blockIdx.x % nrt) * NN_BM;      // first row of the tile
  const int c0 = ((blockIdx.x / nrt) % nct) * 128;   // first column (k index)
  const long e = blockIdx.x / (nrt * nct);
  const long row0 = e * R;

  const int t = threadIdx.x;
  const int lane = t % WAVE;
  const int wave = t / WAVE;
  const int wm = (wave / 2) * 64;
  const int wn = (wave % 2) * 64;
  bf16* DXe = DX + row0 * K;

  if (valid) {
    const int r = m0 + lane;
    const int any = (r < R ? (int)valid[row0 + r] : 0)
                  | (r + 64 < R ? (int)valid[row0 + r + 64] : 0);
    if (__ballot(any) == 0) {
      moe_tile_store<128>(DXe, K, m0, c0, R, nullptr, t);
      return;
    }
  }

  const int nk = N / NN_BK;
  const int nsteps = TWO ? 2 * nk : nk;
  auto stage = [&](int buf, int kt) {
    const bool second = TWO && kt >= nk;
    const bf16* Ge = (second ? G2 : G1) + row0 * N;
    const bf16* We = (second ? W2 : W1) + e * K * N;
    const int k0 = (second ? kt - nk : kt) * NN_BK;
    char* dst = smem + buf * BUF;
    #pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int el = (t + p * 256) * 8;        // element offset in the tile
      const int row = el / NN_BK, col = el % NN_BK;
      glds16(Ge + (long)min(m0 + row, R - 1) * N + k0 + col,
             dst + (p * 256 + wave * 64) * 16);
      glds16(We + (long)min(c0 + row, K - 1) * N + k0 + col,
             dst + ATILE + (p * 256 + wave * 64) * 16);
    }
  };

  f32x4 acc[4][4];
  #pragma unroll
  for (int i = 0; i < 4; ++i)
    #pragma unroll
    for (int j = 0; j < 4; ++j)
      acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  stage(0, 0);
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();

  const int frag_row = lane & 15;
  const int frag_k = (lane >> 4) * 8;
  for (int kt = 0; kt < nsteps; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nsteps) stage(buf ^ 1, kt + 1);
    const char* base = smem + buf * BUF;
    bf16x8v g_frag[4], w_frag[4];
    #pragma unroll
    for (int i = 0; i < 4; ++i)
      g_frag[i] = *reinterpret_cast<const bf16x8v*>(
          base + ((wm + i * 16 + frag_row) * NN_BK + frag_k) * 2);
    #pragma unroll
    for (int j = 0; j < 4; ++j)
      w_frag[j] = *reinterpret_cast<const bf16x8v*>(
          base + ATILE + ((wn + j * 16 + frag_row) * NN_BK + frag_k) * 2);
    // transposed product D[k][row]: a lane holds row (l&15) and columns
    // (l>>4)*4 + 0..3 of each 16x16 block
    #pragma unroll
    for (int i = 0; i < 4; ++i)
      #pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            w_frag[j], g_frag[i], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
  }

  #pragma unroll
  for (int i = 0; i < 4; ++i)
    #pragma unroll
    for (int j = 0; j < 4; ++j)
      moe_tile_put<128>(smem, wm + i * 16 + (lane & 15),
                        wn + j * 16 + (lane >> 4) * 4, acc[i][j]);
  __syncthreads();
  moe_tile_store<128>(DXe, K, m0, c0, R, smem, t);
}

extern "C" __global__ void __launch_bounds__(256)
moe_nt_kernel(const bf16* __restrict__ G, const bf16* __restrict__ W,
              bf16* __restrict__ DX, const unsigned char* __restrict__ valid,
              int R, int K, int N) {
  moe_nt_body<false>(G, W, nullptr, nullptr, DX, valid, R, K, N);
}

extern "C" __global__ void __launch_bounds__(256)
moe_nt2_kernel(const bf16* __restrict__ G1, const bf16* __restrict__ W1,
               const bf16* __restrict__ G2, const bf16* __restrict__ W2,
               bf16* __restrict__ DX, const unsigned char* __restrict__ valid,
               int R, int K, int N) {
  moe_nt_body<true>(G1, W1, G2, W2, DX, valid, R, K, N);
}

// tn_stage's image for a step that crosses the operand's last row: the same
// positions, through registers, rows at or beyond rmax filled with zeros
template <int NTHR>
DEVINL void tn_stage_tail(const bf16* src, long ld, int r0, int rmax, int p0,
                          int pmax, char* dst_base, int t) {
  #pragma unroll
  for (int i = 0; i < 2; ++i) {
    unsigned p = (i * NTHR + t) * 16;
    int chunk16 = p >> 10;
    unsigned w = p & 1023u;
    int rr = tn_unswz(w >> 7) * 4 + ((w & 127) >> 5);
    int pp = chunk16 * 16 + ((w & 31) >> 1);
    int gp = min(p0 + pp, pmax - 8);
    bf16x8v v{};
    if (r0 + rr < rmax)
      v = *reinterpret_cast<const bf16x8v*>(src + (long)(r0 + rr) * ld + gp);
    *reinterpret_cast<bf16x8v*>(dst_base + p) = v;
  }
}

#define MOE_TN_LIST 32768u     // the live-step list sits behind the buffers

template <bool PAIR>
DEVINL void moe_tn_body(const bf16* __restrict__ X, const bf16* __restrict__ G1,
                        const bf16* __restrict__ G2, bf16* __restrict__ DW1,
                        bf16* __restrict__ DW3,
                        const unsigned char* __restrict__ valid, int R, int K,
                        int N) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NP = PAIR ? 2 : 1;             // products per workgroup
  constexpr int TN = PAIR ? 64 : 128;          // output columns per product
  constexpr int NJ = TN / 32;                  // 16-col fragments per wave
  constexpr unsigned XIMG = TBR * 128 * 2;     // X image, 8 KiB
  constexpr unsigned GIMG = TBR * TN * 2;      // one G image, 8 / 4 KiB
  constexpr unsigned BUF = XIMG + NP * GIMG;   // 16 KiB per buffer
  constexpr unsigned OTILE = 128 * TN * 2;     // epilogue tile, 32 / 16 KiB

  const unsigned nkt = (K + 127) / 128, nnt = (N + TN - 1) / TN;
  const int k0 = (blockIdx.x % nkt) * 128;     // first row of the dw tile
  const int n0 = ((blockIdx.x / nkt) % nnt) * TN;
  const long e = blockIdx.x / (nkt * nnt);

  const int t = threadIdx.x;
  const int lane = t % WAVE;
  const int wave = t / WAVE;
  const int wp = (wave >> 1) * 64;             // wave's dw rows (k index)
  const int wq = (wave & 1) * (TN / 2);        // wave's dw columns
  bf16* DW1e = DW1 + e * K * N;
  bf16* DW3e = PAIR ? DW3 + e * K * N : nullptr;

  const int nsteps = (R + TBR - 1) / TBR;
  int nlive = nsteps;
  const unsigned short* live =
      reinterpret_cast<const unsigned short*>(smem + MOE_TN_LIST);
  if (valid) {
    // every wave builds the whole list (the same values to the same
    // addresses), so each has the count in registers.  A lane takes 16 rows,
    // two lanes make a step, a pass of the wave covers 32 steps.
    const unsigned char* ve = valid + e * R;
    const bool aligned = ((uintptr_t)ve & 15) == 0;
    unsigned short* list = reinterpret_cast<unsigned short*>(smem + MOE_TN_LIST);
    nlive = 0;
    for (int s0 = 0; s0 < nsteps; s0 += 32) {
      const int r = s0 * TBR + lane * 16;
      unsigned any = 0;
      if (aligned && r + 16 <= R) {
        const uint4 f = *reinterpret_cast<const uint4*>(ve + r);
        any = f.x | f.y | f.z | f.w;
      } else {
        for (int u = 0; u < 16; ++u)
          if (r + u < R) any |= ve[r + u];
      }
      unsigned long long m = __ballot(any != 0);
      m = (m | (m >> 1)) & 0x5555555555555555ull;   // bit 2s: step s0+s live
      if ((lane & 1) == 0 && ((m >> lane) & 1))
        list[nlive + __popcll(m & ((1ull << lane) - 1))] =
            (unsigned short)(s0 + (lane >> 1));
      nlive += __popcll(m);
    }
    if (nlive == 0) {
      moe_tile_store<TN>(DW1e, N, k0, n0, K, nullptr, t);
      if constexpr (PAIR) moe_tile_store<TN>(DW3e, N, k0, n0, K, nullptr, t);
      return;
    }
    __syncthreads();
  }

  const bf16* Xe = X + e * R * K;
  const bf16* G1e = G1 + e * R * N;
  const bf16* G2e = PAIR ? G2 + e * R * N : nullptr;

  // live step i into buffer buf
  auto stage = [&](int buf, int i) {
    const int r0 = (valid ? (int)live[i] : i) * TBR;
    char* dst = smem + buf * BUF;
    if (r0 + TBR <= R) {
      tn_stage<256>(Xe, K, r0, k0, K, dst, t, wave);
      if constexpr (PAIR)
        tn_stage<128>(wave < 2 ? G1e : G2e, N, r0, n0, N,
                      dst + XIMG + (wave >> 1) * GIMG, t & 127, wave & 1);
      else
        tn_stage<256>(G1e, N, r0, n0, N, dst + XIMG, t, wave);
    } else {
      tn_stage_tail<256>(Xe, K, r0, R, k0, K, dst, t);
      if constexpr (PAIR)
        tn_stage_tail<128>(wave < 2 ? G1e : G2e, N, r0, R, n0, N,
                           dst + XIMG + (wave >> 1) * GIMG, t & 127);
      else
        tn_stage_tail<256>(G1e, N, r0, R, n0, N, dst + XIMG, t);
    }
  };

  f32x4 acc[NP][4][NJ];
  #pragma unroll
  for (int p = 0; p < NP; ++p)
    #pragma unroll
    for (int i = 0; i < 4; ++i)
      #pragma unroll
      for (int j = 0; j < NJ; ++j)
        acc[p][i][j] = {0.f, 0.f, 0.f, 0.f};

  stage(0, 0);
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();

  for (int it = 0; it < nlive; ++it) {
    const int buf = it & 1;
    if (it + 1 < nlive) stage(buf ^ 1, it + 1);
    const char* img = smem + buf * BUF;
    bf16x8v x_frag[4], g_frag[NP][NJ];
    #pragma unroll
    for (int i = 0; i < 4; ++i)
      x_frag[i] = tn_frag(img, (wp >> 4) + i, lane);
    #pragma unroll
    for (int p = 0; p < NP; ++p)
      #pragma unroll
      for (int j = 0; j < NJ; ++j)
        g_frag[p][j] = tn_frag(img + XIMG + p * GIMG, (wq >> 4) + j, lane);
    // transposed product D[n][k]: a lane holds dw row (l&15) and columns
    // (l>>4)*4 + 0..3 of each 16x16 block
    #pragma unroll
    for (int p = 0; p < NP; ++p)
      #pragma unroll
      for (int i = 0; i < 4; ++i)
        #pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[p][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              g_frag[p][j], x_frag[i], acc[p][i][j], 0, 0, 0);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
  }

  #pragma unroll
  for (int p = 0; p < NP; ++p)
    #pragma unroll
    for (int i = 0; i < 4; ++i)
      #pragma unroll
      for (int j = 0; j < NJ; ++j)
        moe_tile_put<TN>(smem + p * OTILE, wp + i * 16 + (lane & 15),
                         wq + j * 16 + (lane >> 4) * 4, acc[p][i][j]);
  __syncthreads();
  moe_tile_store<TN>(DW1e, N, k0, n0, K, smem, t);
  if constexpr (PAIR) moe_tile_store<TN>(DW3e, N, k0, n0, K, smem + OTILE, t);
}

extern "C" __global__ void __launch_bounds__(256)
moe_tn_kernel(const bf16* __restrict__ X, const bf16* __restrict__ G,
              bf16* __restrict__ DW, const unsigned char* __restrict__ valid,
              int R, int K, int N) {
  moe_tn_body<false>(X, G, nullptr, DW, nullptr, valid, R, K, N);
}

extern "C" __global__ void __launch_bounds__(256)
moe_tn2_kernel(const bf16* __restrict__ X, const bf16* __restrict__ G1,
               const bf16* __restrict__ G2, bf16* __restrict__ DW1,
               bf16* __restrict__ DW3, const unsigned char* __restrict__ valid,
               int R, int K, int N) {
  moe_tn_body<true>(X, G1, G2, DW1, DW3, valid, R, K, N);
}


// ===========================================================================
// host wrappers
// ===========================================================================
// edge-shape paths (gemm_nt_128, gemm_nn_128): the activation as a separate
// aten pass over the GEMM's (bias included) result
static at::Tensor act_pass(at::Tensor c, int64_t act,
                           const std::optional<at::Tensor>& aux) {
  if (act == 1) c = at::gelu(c, "tanh");
  else if (act == 3) c = at::gelu(c);
  else if (act == 2) c = at::gelu_backward(c, aux.value(), "tanh");
  else if (act == 4) c = at::gelu_backward(c, aux.value(), "none");
  else if (act >= 5) {           // fused fwd: keep pre-act in aux
    aux.value().copy_(c);
    c = at::gelu(c, "tanh");
  }
  return c;
}

at::Tensor gemm_nt_act(const at::Tensor& a, const at::Tensor& bt,
                       const std::optional<at::Tensor>& bias, int64_t act,
                       const std::optional<at::Tensor>& aux) {
  TORCH_CHECK(a.dtype() == at::kBFloat16 && bt.dtype() == at::kBFloat16);
  TORCH_CHECK(a.is_contiguous() && bt.is_contiguous(),
              "gemm_nt wants K-contiguous operands");
  const long M = a.size(0), K = a.size(1), N = bt.size(0);
  TORCH_CHECK(bt.size(1) == K);
  TORCH_CHECK(K % BK == 0, "gemm_nt: K must be a multiple of 32");
  TORCH_CHECK(N % 8 == 0, "gemm_nt: N must be a multiple of 8");
  auto c = at::empty({M, N}, a.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  const bf16* bias_p = bias ? (const bf16*)bias->data_ptr() : nullptr;
  // modes 1 and 3 are plain forward activations: no aux
  TORCH_CHECK(!(act == 2 || act >= 4) || aux,
              "gemm_nt: activation modes 2/4/5/6 need aux");
  if (K % BK2 == 0 && M >= BM2 && N >= 128) {
    unsigned nwg = ((M + BM2 - 1) / BM2) * ((N + BN2 - 1) / BN2);
    bf16* aux_p = aux ? (bf16*)aux->data_ptr() : nullptr;
    hipLaunchKernelGGL(gemm_nt_256, dim3(nwg), dim3(512), 2 * BUF_B, stream,
        (const bf16*)a.data_ptr(), (const bf16*)bt.data_ptr(),
        (bf16*)c.data_ptr(), bias_p, aux_p, (int)act, (int)M, (int)N,
        (int)K);
  } else {
    unsigned nwg = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
    size_t lds = 2 * 2 * BM * BK * 2;   // 32 KiB
    hipLaunchKernelGGL(gemm_nt_128, dim3(nwg), dim3(256), lds, stream,
        (const bf16*)a.data_ptr(), (const bf16*)bt.data_ptr(),
        (bf16*)c.data_ptr(), bias_p, (int)M, (int)N, (int)K);
    c = act_pass(c, act, aux);
  }
  return c;
}

at::Tensor gemm_nt(const at::Tensor& a, const at::Tensor& bt,
                   const std::optional<at::Tensor>& bias) {
  return gemm_nt_act(a, bt, bias, 0, std::nullopt);
}

// C = a @ b (+bias), activation epilogue: a [M,K] and b [K,N] row-major, the
// dX backward with the weight as it lies.  No host synchronisation, nothing
// allocated but the output (and the aten activation's on the edge path).
at::Tensor gemm_nn_act(const at::Tensor& a, const at::Tensor& b,
                       const std::optional<at::Tensor>& bias, int64_t act,
                       const std::optional<at::Tensor>& aux) {
  TORCH_CHECK(a.is_cuda() && b.is_cuda() && a.dtype() == at::kBFloat16 &&
              b.dtype() == at::kBFloat16, "gemm_nn: bf16 device tensors");
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && a.is_contiguous() &&
              b.is_contiguous(), "gemm_nn wants row-major a [M,K], b [K,N]");
  const long M = a.size(0), K = a.size(1), N = b.size(1);
  TORCH_CHECK(b.size(0) == K, "gemm_nn: reduce dims must match");
  TORCH_CHECK(M >= 1 && K >= NN_BK && K % NN_BK == 0 && N >= 8 && N % 8 == 0,
              "gemm_nn: M >= 1, K % 32 == 0, N % 8 == 0");
  TORCH_CHECK(M < (1L << 31) && K < (1L << 31) && N < (1L << 31));
  TORCH_CHECK((uintptr_t)a.data_ptr() % 16 == 0 &&
              (uintptr_t)b.data_ptr() % 16 == 0,
              "gemm_nn: a and b must be 16-byte aligned");
  TORCH_CHECK(act >= 0 && act <= 6, "gemm_nn: activation modes 0 to 6");
  const bool use_aux = act == 2 || act >= 4;   // 1 and 3 are plain forward
  TORCH_CHECK(!use_aux || aux, "gemm_nn: activation modes 2/4/5/6 need aux");
  if (use_aux)
    TORCH_CHECK(aux->is_cuda() && aux->dtype() == at::kBFloat16 &&
                aux->is_contiguous() && aux->dim() == 2 &&
                aux->size(0) == M && aux->size(1) == N &&
                (uintptr_t)aux->data_ptr() % 16 == 0,
                "gemm_nn: aux must be a contiguous, aligned bf16 [M,N]");
  if (bias)
    TORCH_CHECK(bias->is_cuda() && bias->dtype() == at::kBFloat16 &&
                bias->is_contiguous() && bias->numel() == N,
                "gemm_nn: bias must be a contiguous bf16 [N]");
  auto c = at::empty({M, N}, a.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  const bf16* bias_p = bias ? (const bf16*)bias->data_ptr() : nullptr;
  if (K % BK2 == 0 && M >= BM2 && N >= BN2) {
    const long nwg = ((M + BM2 - 1) / BM2) * ((N + BN2 - 1) / BN2);
    TORCH_CHECK(nwg < (1L << 31), "gemm_nn: too many tiles for one launch");
    bf16* aux_p = use_aux ? (bf16*)aux->data_ptr() : nullptr;
    hipLaunchKernelGGL(gemm_nn_256, dim3((unsigned)nwg), dim3(512), 2 * BUF_B,
        stream, (const bf16*)a.data_ptr(), (const bf16*)b.data_ptr(),
        (bf16*)c.data_ptr(), bias_p, aux_p, (int)act, (int)M, (int)N, (int)K);
  } else {
    const long nwg = ((M + NN_BM - 1) / NN_BM) * ((N + 127) / 128);
    TORCH_CHECK(nwg < (1L << 31), "gemm_nn: too many tiles for one launch");
    hipLaunchKernelGGL(gemm_nn_128, dim3((unsigned)nwg), dim3(256), 32768,
        stream, (const bf16*)a.data_ptr(), (const bf16*)b.data_ptr(),
        (bf16*)c.data_ptr(), bias_p, (int)M, (int)N, (int)K);
    c = act_pass(c, act, aux);
  }
  return c;
}

at::Tensor gemm_nn(const at::Tensor& a, const at::Tensor& b,
                   const std::optional<at::Tensor>& bias) {
  return gemm_nn_act(a, b, bias, 0, std::nullopt);
}

at::Tensor gelu_fast(const at::Tensor& x) {
  TORCH_CHECK(x.dtype() == at::kBFloat16 && x.is_contiguous());
  const long n = x.numel();
  TORCH_CHECK(n % 8 == 0, "gelu_fast: numel multiple of 8");
  auto y = at::empty_like(x);
  long thr = n / 8;
  unsigned grid = (unsigned)std::min<long>((thr + 255) / 256, 8192);
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(gelu_fwd_kernel, dim3(grid), dim3(256), 0, stream,
                     (const bf16*)x.data_ptr(), (bf16*)y.data_ptr(), n);
  return y;
}

at::Tensor gelu_bwd_fast(const at::Tensor& g, const at::Tensor& x) {
  TORCH_CHECK(g.dtype() == at::kBFloat16 && g.is_contiguous());
  TORCH_CHECK(x.dtype() == at::kBFloat16 && x.is_contiguous());
  const long n = x.numel();
  TORCH_CHECK(g.numel() == n && n % 8 == 0);
  auto y = at::empty_like(x);
  long thr = n / 8;
  unsigned grid = (unsigned)std::min<long>((thr + 255) / 256, 8192);
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(gelu_bwd_kernel, dim3(grid), dim3(256), 0, stream,
                     (const bf16*)g.data_ptr(), (const bf16*)x.data_ptr(),
                     (bf16*)y.data_ptr(), n);
  return y;
}

// fused forward linear+gelu: returns (gelu(a@bt^T+bias), pre-activation).
// One kernel writes both, saving the standalone activation kernel's
// HBM re-read of the GEMM result (~0.8 ms/step on GPT-2 small @ b64).
std::tuple<at::Tensor, at::Tensor>
gemm_nt_gelu(const at::Tensor& a, const at::Tensor& bt,
             const std::optional<at::Tensor>& bias, bool tanh_approx) {
  const long M = a.size(0), K = a.size(1), N = bt.size(0);
  if (K % BK2 == 0 && M >= BM2 && N >= 128) {
    auto pre = at::empty({M, N}, a.options());
    auto act = gemm_nt_act(a, bt, bias, tanh_approx ? 5 : 6, pre);
    return {act, pre};
  }
  // edge shapes: 128-tile GEMM then a separate aten activation
  auto pre = gemm_nt_act(a, bt, bias, 0, std::nullopt);
  auto act = at::gelu(pre, tanh_approx ? "tanh" : "none");
  return {act, pre};
}

std::tuple<at::Tensor, at::Tensor> gemm_tn_asum(const at::Tensor& a,
                                                const at::Tensor& b);

// EASYDIST_TN_MAP: 1 = slice-major (default), 0 = tile-major placement,
// kept for A/B timing.  Read at every launch, not cached in a static, so
// one process can run both maps.
static inline int ed_tn_map_mode() {
  const char* e = getenv("EASYDIST_TN_MAP");
  return (e && atoi(e) == 0) ? TN_MAP_TILE_MAJOR : TN_MAP_SLICE_MAJOR;
}

// shared TN launch: picks the 256x256 tile (half the operand re-read
// traffic) when P and Q allow it AND the grid still covers the chip;
// falls back to the 128x128 kernel otherwise (edge + small shapes).
static at::Tensor tn_launch(const at::Tensor& a, const at::Tensor& b,
                            float* asum_p) {
  const int map_mode = ed_tn_map_mode();
  TORCH_CHECK(a.dtype() == at::kBFloat16 && b.dtype() == at::kBFloat16);
  TORCH_CHECK(a.is_contiguous() && b.is_contiguous());
  const long R = a.size(0), P = a.size(1), Q = b.size(0) == R ? b.size(1) : -1;
  TORCH_CHECK(Q > 0, "gemm_tn: reduce dims must match");
  TORCH_CHECK(R % TBR == 0, "gemm_tn: R must be a multiple of 32");
  TORCH_CHECK(P % TBP == 0 && Q % TBP == 0,
              "gemm_tn: P, Q must be multiples of 128");
  // P/Q only need the 128 alignment the op already requires — the 256
  // kernel ceil-divs its grid and guards edge tiles (lm_head dW has
  // P = vocab = 50304 = 128*393)
  bool big = R / TBR >= 64 && P >= TBP2 && Q >= TBP2;
  unsigned ntile;
  int splitr = 1;
  if (big) {
    ntile = ((P + TBP2 - 1) / TBP2) * ((Q + TBP2 - 1) / TBP2);
    // 8-wave WGs are VGPR-bound at ONE resident WG per CU, so the grid
    // should fill the 256 CUs in (near-)whole rounds: a ragged 1.1-round
    // grid serializes a mostly-idle second round. Flat division (not
    // powers of two) lands just under the target; slices ceil-div R.
    const int target = 256;
    splitr = std::max(1, target / (int)ntile);
    // EASYDIST_TN256_SPLITR forces the split (tuning sweeps); read at
    // every launch like the map mode
    if (const char* e = getenv("EASYDIST_TN256_SPLITR"))
      if (atoi(e) > 0) splitr = atoi(e);
    splitr = std::min((long)splitr, R / TBR / 8);   // >=8 k-steps per slice
    splitr = std::max(1, std::min(splitr, 64));
  } else {
    ntile = (P / TBP) * (Q / TBP);
    // split the reduction so the grid covers the chip's 256 CUs
    while (ntile * splitr < 512 && splitr < 16 &&
           (R / TBR) % (splitr * 2) == 0 && (R / TBR) / (splitr * 2) >= 1)
      splitr *= 2;
  }
  auto cw = splitr == 1
      ? at::empty({P, Q}, a.options().dtype(at::kFloat))
      : at::zeros({P, Q}, a.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream();
  if (big) {
    // EASYDIST_TN256_STAGING: 1 = three-buffer ring (default), 0 = the
    // issue-then-drain loop (tn_body's RING), kept for A/B; read at every
    // launch
    const char* se = getenv("EASYDIST_TN256_STAGING");
    const bool ring = !(se && atoi(se) == 0);
    auto kern = ring ? gemm_tn_256_kernel : gemm_tn_256_drain_kernel;
    size_t lds = tn_lds_bytes(TBP2, ring);   // 96 / 64 KiB
    hipLaunchKernelGGL(kern, dim3(ntile * splitr), dim3(2 * TBP2),
        lds, stream,
        (const bf16*)a.data_ptr(), (const bf16*)b.data_ptr(),
        cw.data_ptr<float>(), asum_p, (int)R, (int)P, (int)Q, splitr,
        map_mode);
  } else {
    size_t lds = tn_lds_bytes(TBP, 0);   // 32 KiB
    hipLaunchKernelGGL(gemm_tn_kernel, dim3(ntile * splitr), dim3(2 * TBP),
        lds, stream,
        (const bf16*)a.data_ptr(), (const bf16*)b.data_ptr(),
        cw.data_ptr<float>(), asum_p, (int)R, (int)P, (int)Q, splitr,
        map_mode);
  }
  return cw;
}

at::Tensor gemm_tn(const at::Tensor& a, const at::Tensor& b) {
  // C[P,Q] = a^T @ b with a:[R,P], b:[R,Q]
  return tn_launch(a, b, nullptr).to(at::kBFloat16);
}

std::tuple<at::Tensor, at::Tensor> gemm_tn_asum(const at::Tensor& a,
                                                const at::Tensor& b) {
  // like gemm_tn, additionally returning colsum(a) (dBias) in ONE pass
  auto asum = at::zeros({a.size(1)}, a.options().dtype(at::kFloat));
  auto cw = tn_launch(a, b, asum.data_ptr<float>());
  return {cw.to(at::kBFloat16), asum};
}

// ---------------------------------------------------------------------------
// MoE expert FFN forward (moe_nn kernels)
// ---------------------------------------------------------------------------
struct MoeNnShape { long E, R, K, N; unsigned grid; };

static void moe_nn_operand(const at::Tensor& t, at::IntArrayRef shape,
                           const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dtype() == at::kBFloat16 && t.is_contiguous(),
              "moe_expert: ", name, " must be a contiguous bf16 device tensor");
  TORCH_CHECK(t.sizes() == shape, "moe_expert: ", name, " has the wrong shape");
  TORCH_CHECK((uintptr_t)t.data_ptr() % 16 == 0, "moe_expert: ", name,
              " must be 16-byte aligned");
}

static MoeNnShape moe_nn_shape(const at::Tensor& x, const at::Tensor& w,
                               const std::optional<at::Tensor>& valid,
                               int tile_n) {
  TORCH_CHECK(x.dim() == 3 && w.dim() == 3, "moe_expert: x [E,R,K], w [E,K,N]");
  MoeNnShape s{x.size(0), x.size(1), x.size(2), w.size(2), 0};
  TORCH_CHECK(s.E >= 1 && s.R >= 1 && s.K >= NN_BK && s.K % NN_BK == 0 &&
              s.N >= 8 && s.N % 8 == 0,
              "moe_expert: E, R >= 1, K % 32 == 0, N % 8 == 0");
  TORCH_CHECK(s.R < (1L << 31) && s.K < (1L << 31) && s.N < (1L << 31));
  moe_nn_operand(x, {s.E, s.R, s.K}, "x");
  moe_nn_operand(w, {s.E, s.K, s.N}, "w");
  if (valid)
    TORCH_CHECK(valid->is_cuda() && valid->dtype() == at::kBool &&
                valid->is_contiguous() && valid->dim() == 2 &&
                valid->size(0) == s.E && valid->size(1) == s.R,
                "moe_expert: valid must be a contiguous bool [E,R]");
  const long nwg = s.E * ((s.R + NN_BM - 1) / NN_BM)
                   * ((s.N + tile_n - 1) / tile_n);
  TORCH_CHECK(nwg < (1L << 31), "moe_expert: too many tiles for one launch");
  s.grid = (unsigned)nwg;
  return s;
}

static const unsigned char* moe_nn_valid(const std::optional<at::Tensor>& v) {
  return v ? (const unsigned char*)v->data_ptr() : nullptr;
}

at::Tensor moe_expert_gemm(const at::Tensor& x, const at::Tensor& w,
                           const std::optional<at::Tensor>& valid) {
  const MoeNnShape s = moe_nn_shape(x, w, valid, 128);
  auto c = at::empty({s.E, s.R, s.N}, x.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(moe_nn_gemm_kernel, dim3(s.grid), dim3(256), 32768,
      stream, (const bf16*)x.data_ptr(), (const bf16*)w.data_ptr(),
      (bf16*)c.data_ptr(), moe_nn_valid(valid), (int)s.R, (int)s.K, (int)s.N);
  return c;
}

// (h, a, b) = (silu(a) * b, x @ w1, x @ w3)
std::tuple<at::Tensor, at::Tensor, at::Tensor>
moe_expert_up(const at::Tensor& x, const at::Tensor& w1, const at::Tensor& w3,
              const std::optional<at::Tensor>& valid) {
  const MoeNnShape s = moe_nn_shape(x, w1, valid, 64);
  moe_nn_operand(w3, {s.E, s.K, s.N}, "w3");
  auto h = at::empty({s.E, s.R, s.N}, x.options());
  auto a = at::empty_like(h);
  auto b = at::empty_like(h);
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(moe_nn_swiglu_kernel, dim3(s.grid), dim3(256), 32768,
      stream, (const bf16*)x.data_ptr(), (const bf16*)w1.data_ptr(),
      (const bf16*)w3.data_ptr(), (bf16*)h.data_ptr(), (bf16*)a.data_ptr(),
      (bf16*)b.data_ptr(), moe_nn_valid(valid), (int)s.R, (int)s.K, (int)s.N);
  return {h, a, b};
}

// ---------------------------------------------------------------------------
// MoE expert FFN backward (moe_nt / moe_tn kernels)
// ---------------------------------------------------------------------------
static void moe_bwd_valid(const std::optional<at::Tensor>& valid, long E,
                          long R) {
  if (valid)
    TORCH_CHECK(valid->is_cuda() && valid->dtype() == at::kBool &&
                valid->is_contiguous() && valid->dim() == 2 &&
                valid->size(0) == E && valid->size(1) == R,
                "moe_expert: valid must be a contiguous bool [E,R]");
}

static unsigned moe_bwd_grid(long e, long tiles_a, long tiles_b) {
  const long nwg = e * tiles_a * tiles_b;
  TORCH_CHECK(nwg < (1L << 31), "moe_expert: too many tiles for one launch");
  return (unsigned)nwg;
}

// dx = g1 @ w1^T (+ g2 @ w2^T): g [E,R,N], w [E,K,N] -> [E,R,K]
at::Tensor moe_expert_dx(const at::Tensor& g1, const at::Tensor& w1,
                         const std::optional<at::Tensor>& g2,
                         const std::optional<at::Tensor>& w2,
                         const std::optional<at::Tensor>& valid) {
  TORCH_CHECK(g1.dim() == 3 && w1.dim() == 3,
              "moe_expert_dx: g [E,R,N], w [E,K,N]");
  TORCH_CHECK(g2.has_value() == w2.has_value(),
              "moe_expert_dx: g2 and w2 come together");
  const long E = g1.size(0), R = g1.size(1), N = g1.size(2), K = w1.size(1);
  TORCH_CHECK(E >= 1 && R >= 1 && N >= NN_BK && N % NN_BK == 0 && K >= 8 &&
              K % 8 == 0, "moe_expert_dx: E, R >= 1, N % 32 == 0, K % 8 == 0");
  TORCH_CHECK(R < (1L << 31) && K < (1L << 31) && N < (1L << 31));
  moe_nn_operand(g1, {E, R, N}, "g1");
  moe_nn_operand(w1, {E, K, N}, "w1");
  if (g2) {
    moe_nn_operand(*g2, {E, R, N}, "g2");
    moe_nn_operand(*w2, {E, K, N}, "w2");
  }
  moe_bwd_valid(valid, E, R);
  const unsigned grid =
      moe_bwd_grid(E, (R + NN_BM - 1) / NN_BM, (K + 127) / 128);
  auto dx = at::empty({E, R, K}, g1.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  if (g2)
    hipLaunchKernelGGL(moe_nt2_kernel, dim3(grid), dim3(256), 32768, stream,
        (const bf16*)g1.data_ptr(), (const bf16*)w1.data_ptr(),
        (const bf16*)g2->data_ptr(), (const bf16*)w2->data_ptr(),
        (bf16*)dx.data_ptr(), moe_nn_valid(valid), (int)R, (int)K, (int)N);
  else
    hipLaunchKernelGGL(moe_nt_kernel, dim3(grid), dim3(256), 32768, stream,
        (const bf16*)g1.data_ptr(), (const bf16*)w1.data_ptr(),
        (bf16*)dx.data_ptr(), moe_nn_valid(valid), (int)R, (int)K, (int)N);
  return dx;
}

struct MoeTnShape { long E, R, K, N; unsigned lds; };

static MoeTnShape moe_tn_shape(const at::Tensor& x, const at::Tensor& g,
                               const std::optional<at::Tensor>& valid) {
  TORCH_CHECK(x.dim() == 3 && g.dim() == 3,
              "moe_expert_dw: x [E,R,K], g [E,R,N]");
  MoeTnShape s{x.size(0), x.size(1), x.size(2), g.size(2), MOE_TN_LIST};
  const long nsteps = (s.R + TBR - 1) / TBR;
  TORCH_CHECK(s.E >= 1 && s.R >= 1 && s.K >= 8 && s.K % 8 == 0 && s.N >= 8 &&
              s.N % 8 == 0 && nsteps <= 4096,
              "moe_expert_dw: E, R >= 1, K % 8 == 0, N % 8 == 0, "
              "R <= 131072");
  TORCH_CHECK(s.K < (1L << 31) && s.N < (1L << 31));
  moe_nn_operand(x, {s.E, s.R, s.K}, "x");
  moe_nn_operand(g, {s.E, s.R, s.N}, "g");
  moe_bwd_valid(valid, s.E, s.R);
  if (valid)     // the live-step list, one uint16 per 32-row step
    s.lds += (unsigned)((2 * nsteps + 15) / 16 * 16);
  return s;
}

// dw = x^T @ g: x [E,R,K], g [E,R,N] -> [E,K,N]
at::Tensor moe_expert_dw(const at::Tensor& x, const at::Tensor& g,
                         const std::optional<at::Tensor>& valid) {
  const MoeTnShape s = moe_tn_shape(x, g, valid);
  const unsigned grid = moe_bwd_grid(s.E, (s.K + 127) / 128, (s.N + 127) / 128);
  auto dw = at::empty({s.E, s.K, s.N}, x.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(moe_tn_kernel, dim3(grid), dim3(256), s.lds, stream,
      (const bf16*)x.data_ptr(), (const bf16*)g.data_ptr(),
      (bf16*)dw.data_ptr(), moe_nn_valid(valid), (int)s.R, (int)s.K, (int)s.N);
  return dw;
}

// (dw1, dw3) = (x^T @ g1, x^T @ g2), the x image staged once for both
std::tuple<at::Tensor, at::Tensor>
moe_expert_dw2(const at::Tensor& x, const at::Tensor& g1, const at::Tensor& g2,
               const std::optional<at::Tensor>& valid) {
  const MoeTnShape s = moe_tn_shape(x, g1, valid);
  moe_nn_operand(g2, {s.E, s.R, s.N}, "g2");
  const unsigned grid = moe_bwd_grid(s.E, (s.K + 127) / 128, (s.N + 63) / 64);
  auto dw1 = at::empty({s.E, s.K, s.N}, x.options());
  auto dw3 = at::empty_like(dw1);
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(moe_tn2_kernel, dim3(grid), dim3(256), s.lds, stream,
      (const bf16*)x.data_ptr(), (const bf16*)g1.data_ptr(),
      (const bf16*)g2.data_ptr(), (bf16*)dw1.data_ptr(), (bf16*)dw3.data_ptr(),
      moe_nn_valid(valid), (int)s.R, (int)s.K, (int)s.N);
  return {dw1, dw3};
}
