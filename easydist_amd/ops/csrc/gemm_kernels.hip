// Hand-written MFMA bf16 GEMM family for gfx950.
//
// Three kernel families cover the linear-layer training shapes the
// compiler's lowering pass (compiler/passes/lower_hip.py) emits:
//
//   gemm_nt_256  C[M,N] = A[M,K] @ Bt[N,K]^T (+bias)  -- fwd linears and,
//       with a (cheap, weight-only) transpose in the graph, the dX
//       backward.  256x256x64 tile, 8 waves, 8-phase software-pipelined
//       schedule (cdna_hip_programming.md "256-sq 8-phase template"):
//       global_load_lds staging with the st_16x32 XOR swizzle applied on
//       the SOURCE address, counted s_waitcnt vmcnt(6) once per K-tile,
//       raw s_barrier (never __syncthreads: with an LDS-DMA in flight its
//       fence drains vmcnt and serializes the pipeline), s_setprio(1)
//       around each 16-MFMA cluster, LDS-bounced coalesced epilogue.
//   gemm_nt_128  same contract, 128x128x32 tile (the ladder step-3
//       structure) for edge/small shapes; row-clamped staging so M,N need
//       not be tile multiples.
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
// host wrappers
// ===========================================================================
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
    if (act) {
      // edge-shape path: apply the activation as a separate aten pass
      if (act == 1) c = at::gelu(c, "tanh");
      else if (act == 3) c = at::gelu(c);
      else if (act == 2) c = at::gelu_backward(c, aux.value(), "tanh");
      else if (act == 4) c = at::gelu_backward(c, aux.value(), "none");
      else if (act >= 5) {           // fused fwd: keep pre-act in aux
        aux.value().copy_(c);
        c = at::gelu(c, "tanh");
      }
    }
  }
  return c;
}

at::Tensor gemm_nt(const at::Tensor& a, const at::Tensor& bt,
                   const std::optional<at::Tensor>& bias) {
  return gemm_nt_act(a, bt, bias, 0, std::nullopt);
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
