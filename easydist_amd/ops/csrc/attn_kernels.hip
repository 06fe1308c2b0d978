// Flash attention forward for gfx950 (bf16, causal, D in {64, 128}).
//
// v1 structure (correctness-first; the tuned ladder of
// cdna_hip_programming.md §B comes in later rounds): one workgroup = 4
// waves = one 64-row Q block of one (batch, head). Each wave owns 16 Q
// rows. K/V tiles (64 keys x D) are staged in LDS per workgroup; QK^T and
// P·V run on v_mfma_f32_16x16x32_bf16; the online-softmax state (m, l)
// lives in registers, row-reductions via 16-lane shuffles inside each
// fragment group. P round-trips through a wave-private LDS strip to
// re-fragment from the S layout to the PV A-operand layout.
#include "common.h"
#include "attn_block_map.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <climits>

using f32x4 = __attribute__((ext_vector_type(4))) float;
using bf16x8v = __attribute__((ext_vector_type(8))) __bf16;

#define QB 64     // q rows per workgroup (16 per wave)
#define KB 64     // kv tile
#define KBP (KB + 8)  // padded stride for transposed tiles: row stride
                      // 144 B spreads the 64 LDS banks (unpadded 128 B
                      // collapses onto 2 banks -> 8-way conflicts)
#define QBP (QB + 8)

// Bank-conflict XOR swizzle for LINEAR [rows][64 or 128] bf16 LDS tiles
// (element-index form): a ds_read_b128 fragment read walks 16 rows at a
// 128/256-B stride, collapsing onto 2 (or 1) 16-B bank slots — 8/16-way
// conflicts (guide T2).  Folding row bits into the slot bits
// (e ^= ((e>>7)&15)<<3) is an involution, keeps 8-element chunks whole,
// and is injective across the 16 rows of a fragment for both row widths.
DEVINL int lsw(int e) { return e ^ (((e >> 7) & 15) << 3); }


// ---- shared pieces of the swapped-operand (S^T) form ----------------------
// pack a C-layout f32 fragment row-pair into bf16x2 words
DEVINL void swp_pack(const f32x4* sacc, int nj, unsigned pk[][2]) {
  for (int j = 0; j < nj; ++j)
    #pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
      asm("v_cvt_pk_bf16_f32 %0, %1, %2"
          : "=v"(pk[j][t2])
          : "v"(sacc[j][2 * t2]), "v"(sacc[j][2 * t2 + 1]));
}

// in-register butterfly: C-layout (lane col = row m, regs = 16 k's) ->
// A-operand bf16x8 fragment for mfma #ks.  Key K = 16j + 4g_src + r =
// 32ks + 8g_tgt + u maps g_src=(K>>2)&3 to g_tgt=(K>>3)&3; each target
// half-fragment is one source lane's consecutive regs, so three
// selected-send exchanges (xor 16/32/48) deliver every piece.
DEVINL bf16x8v swp_butterfly(const unsigned pk[][2], int ks, int fg) {
  unsigned o0 = pk[2 * ks][0], o1 = pk[2 * ks][1];
  unsigned p0 = pk[2 * ks + 1][0], p1 = pk[2 * ks + 1][1];
  const bool g_odd = (fg & 1), g_hi = (fg >= 2);
  unsigned r16a = __shfl_xor((int)(g_odd ? o0 : p0), 16, WAVE);
  unsigned r16b = __shfl_xor((int)(g_odd ? o1 : p1), 16, WAVE);
  unsigned r32a = __shfl_xor((int)(g_hi ? o0 : p0), 32, WAVE);
  unsigned r32b = __shfl_xor((int)(g_hi ? o1 : p1), 32, WAVE);
  unsigned r48a = __shfl_xor((int)(fg == 2 ? o0 : p0), 48, WAVE);
  unsigned r48b = __shfl_xor((int)(fg == 2 ? o1 : p1), 48, WAVE);
  union { unsigned u[4]; bf16x8v v; } cv;
  if (fg == 0) {
    cv.u[0] = o0;  cv.u[1] = o1;  cv.u[2] = r16a; cv.u[3] = r16b;
  } else if (fg == 1) {
    cv.u[0] = r48a; cv.u[1] = r48b; cv.u[2] = r32a; cv.u[3] = r32b;
  } else if (fg == 2) {
    cv.u[0] = r32a; cv.u[1] = r32b; cv.u[2] = r48a; cv.u[3] = r48b;
  } else {
    cv.u[0] = r16a; cv.u[1] = r16b; cv.u[2] = p0;  cv.u[3] = p1;
  }
  return cv.v;
}

// SW=1 (swapped-operand form): QK^T runs as K*Q^T so the C-layout puts
// ONE q row per lane (col = l&15 = qrow, regs = 16 keys). The online
// softmax then reduces over REGISTERS (15 VALU max/add) plus TWO
// shuffles (xor 16/32 across the fg groups) instead of four dependent
// 4-level shuffle trees, and P reaches the PV A-operand layout through
// a 12-shuffle in-register butterfly (v_cvt_pk_bf16_f32 pairs exchanged
// at xor distances 16/32/48) instead of an LDS strip round-trip.
// Derivation: key K = 16j + 4g_src + r = 32ks + 8g_tgt + u maps source
// group g_src = (K>>2)&3 to target group g_tgt = (K>>3)&3; each target
// half-fragment (4 keys) is one source lane's consecutive regs, so per
// ks three selected-send exchanges (xor16: g0<-g1/g3<-g2, xor32:
// g1<-g3/g2<-g0, xor48: g1<-g2/g2<-g1) deliver every piece.
template <int D, int RF = 1, int KD = 0, int SW = 0>
__global__ void
__launch_bounds__(512, (D == 64 ? (RF == 1 ? 4 : 3) : 1))  // waves/SIMD floor
flash_fwd_kernel(const bf16* __restrict__ Q, const bf16* __restrict__ K,
                 const bf16* __restrict__ V, bf16* __restrict__ O,
                 float* __restrict__ LSE, int B, int H, int S, bool causal,
                 float scale,
                 long qsb, long qsh, long qss, long ksb, long ksh, long kss,
                 long vsb, long vsh, long vss, int map_mode) {
  // grid: 1-D, ceil(S/QBLK) * B*H workgroups placed by attn_block_map
  // (attn_block_map.h); QBLK = 128*RF q rows per workgroup, 8
  // waves of RF 16-row fragments each.  The round-1 4-wave/256-thread
  // form ran ONE wave per SIMD (110 KB LDS) — every softmax/LDS stall
  // fully exposed, ~100 TF effective.  8 waves + the smaller strip pool
  // give 4 waves/SIMD at D=64/RF=1.  RF=2 doubles the q rows sharing
  // each staged K/V tile (half the staging + barrier cost per flop) at
  // one wave/SIMD lower occupancy — A/B'd on hardware.
  constexpr int QBLK = 8 * 16 * RF;
  const AttnBlock wgm = attn_block_map(blockIdx.x, (S + QBLK - 1) / QBLK,
                                       B * H, causal, map_mode);
  const int qb0 = wgm.blk * QBLK;
  const int bh = wgm.bh;
  const int b_ = bh / H, h_ = bh % H;
  // inputs may be [B,S,H,D]-layout views (the qkv split) — per-tensor
  // batch/head/row strides avoid the activation-sized .contiguous()
  // copies the round-1 wrapper made every step
  const bf16* q = Q + b_ * qsb + h_ * qsh;
  const bf16* k = K + b_ * ksb + h_ * ksh;
  const bf16* v = V + b_ * vsb + h_ * vsh;
  bf16* o = O + (long)bh * S * D;
  float* lse = LSE + (long)bh * S;

  const int lane = threadIdx.x % WAVE;
  const int wave = threadIdx.x / WAVE;

  // LDS: DOUBLE-BUFFERED K [KB][D] + V^T [D][KB] (lsw) pairs + P strips.
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TILE_K = KB * D;
  constexpr int TILE_VT = KB * D;   // [D][KB] linear + lsw swizzle
  bf16* smem_b = reinterpret_cast<bf16*>(smem);
  bf16* p_lds = smem_b + 2 * (TILE_K + TILE_VT) + wave * 16 * KB;
  constexpr int NTHR = 8 * WAVE;   // 512

  const int fr = lane & 15;        // fragment row/col index
  const int fg = lane >> 4;        // fragment k-group (8 contiguous)

  // per-fragment first q row (two contiguous 16-row fragments per wave)
  int qr0[RF];
  #pragma unroll
  for (int rf = 0; rf < RF; ++rf) qr0[rf] = qb0 + wave * 16 * RF + rf * 16;

  // Q fragments (A operand), PRE-SCALED by scale*log2(e): the softmax
  // runs in exp2 domain (v_exp2 without the fused multiply) and the hot
  // loop loses its per-element scale multiply
  const float qscale = scale * 1.44269504088896340736f;
  bf16x8v qf[RF][D / 32];
  #pragma unroll
  for (int rf = 0; rf < RF; ++rf) {
    const int row = qr0[rf] + fr;
    #pragma unroll
    for (int ks = 0; ks < D / 32; ++ks) {
      if (row < S) {
        bf16x8v raw = *reinterpret_cast<const bf16x8v*>(
            &q[(long)row * qss + ks * 32 + fg * 8]);
        #pragma unroll
        for (int u = 0; u < 8; ++u)
          qf[rf][ks][u] = (__bf16)(bf2f((bf16)raw[u]) * qscale);
      } else {
        #pragma unroll
        for (int u = 0; u < 8; ++u) qf[rf][ks][u] = (__bf16)0.f;
      }
    }
  }

  float m_run[RF][4], l_run[RF][4];
  f32x4 o_acc[RF][D / 16];
  #pragma unroll
  for (int rf = 0; rf < RF; ++rf) {
    #pragma unroll
    for (int r = 0; r < 4; ++r) { m_run[rf][r] = -1e30f; l_run[rf][r] = 0.f; }
    #pragma unroll
    for (int j = 0; j < D / 16; ++j) o_acc[rf][j] = {0.f, 0.f, 0.f, 0.f};
  }

  const int kv_end = causal ? min(S, qb0 + QBLK) : S;
  const int n_tiles = (kv_end + KB - 1) / KB;
  constexpr int PF = TILE_K / (NTHR * 8);    // 16B vectors per thread
  bf16x8 kreg[PF], vreg[PF];

  // KD=1: K fragments are read straight from global memory (the per-
  // (b,h) K slab is L2-resident at these shapes) — no K staging, no
  // K-tile LDS reads, and the tile barrier only covers the V transpose
  auto load_tile = [&](int t) {
    #pragma unroll
    for (int pi = 0; pi < PF; ++pi) {
      const int e = threadIdx.x * 8 + pi * (NTHR * 8);
      const int row = t * KB + e / D, col = e % D;
      if (!KD)
        kreg[pi] = *reinterpret_cast<const bf16x8*>(
            &k[(long)row * kss + col]);
      vreg[pi] = *reinterpret_cast<const bf16x8*>(&v[(long)row * vss + col]);
    }
  };
  auto store_tile = [&](int t) {
    bf16* kb = smem_b + (t & 1) * (TILE_K + TILE_VT);
    bf16* vb = kb + TILE_K;
    #pragma unroll
    for (int pi = 0; pi < PF; ++pi) {
      const int e = threadIdx.x * 8 + pi * (NTHR * 8);
      if (!KD)
        *reinterpret_cast<bf16x8*>(&kb[lsw(e)]) = kreg[pi];
      const int row = e / D, col = e % D;
      #pragma unroll
      for (int i = 0; i < 8; ++i)
        vb[lsw((col + i) * KB + row)] = vreg[pi].v[i];
    }
  };

  load_tile(0);
  store_tile(0);
  __syncthreads();

  for (int t = 0; t < n_tiles; ++t) {
    const int kv0 = t * KB;
    const bf16* k_lds = smem_b + (t & 1) * (TILE_K + TILE_VT);
    const bf16* vt_lds = k_lds + TILE_K;
    if (t + 1 < n_tiles)
      load_tile(t + 1);          // global loads overlap the MFMA loop

    // a 128*RF-row block spans 8 waves: tiles strictly above this wave's
    // causal diagonal are all-masked — skip the compute (NOT the
    // barriers: every wave still arrives at __syncthreads)
    const bool wave_active = !(causal && kv0 > qr0[RF - 1] + 15);
    if (wave_active) {
    #pragma unroll
    for (int rf = 0; rf < RF; ++rf) {
      if (RF > 1 && causal && kv0 > qr0[rf] + 15)
        continue;                  // this fragment's rows are all-masked
      if (SW) {
        // ---- S^T = K Q^T: lane col = qrow, regs = 16 keys -------------
        f32x4 s_acc[KB / 16];
        __builtin_amdgcn_s_setprio(1);
        #pragma unroll
        for (int j = 0; j < KB / 16; ++j) {
          s_acc[j] = {0.f, 0.f, 0.f, 0.f};
          #pragma unroll
          for (int ks = 0; ks < D / 32; ++ks) {
            bf16x8v kf = *reinterpret_cast<const bf16x8v*>(
                &k_lds[lsw((j * 16 + fr) * D + ks * 32 + fg * 8)]);
            s_acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                kf, qf[rf][ks], s_acc[j], 0, 0, 0);
          }
        }
        __builtin_amdgcn_s_setprio(0);
        const int qrow = qr0[rf] + fr;
        const bool need_mask = (causal && kv0 + KB - 1 > qrow)
                               || (kv0 + KB > S);
        float mx = -1e30f;
        if (need_mask) {
          #pragma unroll
          for (int j = 0; j < KB / 16; ++j)
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
              int kcol = kv0 + j * 16 + 4 * fg + r;
              float sv = s_acc[j][r];
              if ((causal && kcol > qrow) || kcol >= S) sv = -1e30f;
              s_acc[j][r] = sv;
              mx = fmaxf(mx, sv);
            }
        } else {
          #pragma unroll
          for (int j = 0; j < KB / 16; ++j)
            #pragma unroll
            for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s_acc[j][r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, WAVE));
        mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE));
        float m_new = fmaxf(m_run[rf][0], mx);
        float psum = 0.f;
        #pragma unroll
        for (int j = 0; j < KB / 16; ++j)
          #pragma unroll
          for (int r = 0; r < 4; ++r) {
            float pp = __builtin_amdgcn_exp2f(s_acc[j][r] - m_new);
            s_acc[j][r] = pp;
            psum += pp;
          }
        psum += __shfl_xor(psum, 16, WAVE);
        psum += __shfl_xor(psum, 32, WAVE);
        float alpha = __builtin_amdgcn_exp2f(m_run[rf][0] - m_new);
        l_run[rf][0] = l_run[rf][0] * alpha + psum;
        m_run[rf][0] = m_new;
        // o_acc rows are qrows 4*fg+r: fetch those rows' alpha
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          float ar = __shfl(alpha, 4 * fg + r, WAVE);
          #pragma unroll
          for (int j = 0; j < D / 16; ++j) o_acc[rf][j][r] *= ar;
        }
        // pack to bf16 pairs and run the butterfly (swp_* helpers)
        unsigned pk[KB / 16][2];
        swp_pack(s_acc, KB / 16, pk);
        __builtin_amdgcn_s_setprio(1);
        #pragma unroll
        for (int ks = 0; ks < KB / 32; ++ks) {
          bf16x8v pv = swp_butterfly(pk, ks, fg);
          #pragma unroll
          for (int j = 0; j < D / 16; ++j) {
            bf16x8v vf = *reinterpret_cast<const bf16x8v*>(
                &vt_lds[lsw((j * 16 + fr) * KB + ks * 32 + fg * 8)]);
            o_acc[rf][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                pv, vf, o_acc[rf][j], 0, 0, 0);
          }
        }
        __builtin_amdgcn_s_setprio(0);
        continue;                  // SW path done for this fragment
      }
      // ---- S = Q K^T ----------------------------------------------------
      f32x4 s_acc[KB / 16];
      __builtin_amdgcn_s_setprio(1);
      #pragma unroll
      for (int j = 0; j < KB / 16; ++j) {
        s_acc[j] = {0.f, 0.f, 0.f, 0.f};
        #pragma unroll
        for (int ks = 0; ks < D / 32; ++ks) {
          bf16x8v kf;
          if (KD)
            kf = *reinterpret_cast<const bf16x8v*>(
                &k[(long)(kv0 + j * 16 + fr) * kss + ks * 32 + fg * 8]);
          else
            kf = *reinterpret_cast<const bf16x8v*>(
                &k_lds[lsw((j * 16 + fr) * D + ks * 32 + fg * 8)]);
          s_acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[rf][ks], kf,
                                                             s_acc[j], 0, 0,
                                                             0);
        }
      }
      __builtin_amdgcn_s_setprio(0);

      // ---- online softmax ----------------------------------------------
      // interior tiles (fully below the causal diagonal, fully in-range)
      // skip the per-element mask compares — most tiles at long S
      const bool need_mask = (causal && kv0 + KB - 1 > qr0[rf] + 4 * fg)
                             || (kv0 + KB > S);
      float m_new[4];
      if (need_mask) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          float mx = -1e30f;
          #pragma unroll
          for (int j = 0; j < KB / 16; ++j) {
            float sv = s_acc[j][r];        // already scale*log2e scaled
            int kcol = kv0 + j * 16 + fr;
            int qrow = qr0[rf] + 4 * fg + r;
            if (causal && kcol > qrow) sv = -1e30f;
            else if (kcol >= S) sv = -1e30f;
            s_acc[j][r] = sv;
            mx = fmaxf(mx, sv);
          }
          #pragma unroll
          for (int off = 8; off > 0; off >>= 1)
            mx = fmaxf(mx, __shfl_xor(mx, off, WAVE));
          m_new[r] = fmaxf(m_run[rf][r], mx);
        }
      } else {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          float mx = fmaxf(fmaxf(s_acc[0][r], s_acc[1][r]),
                           fmaxf(s_acc[2][r], s_acc[3][r]));
          #pragma unroll
          for (int off = 8; off > 0; off >>= 1)
            mx = fmaxf(mx, __shfl_xor(mx, off, WAVE));
          m_new[r] = fmaxf(m_run[rf][r], mx);
        }
      }
      float p_sum[4] = {0.f, 0.f, 0.f, 0.f};
      #pragma unroll
      for (int j = 0; j < KB / 16; ++j) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          float pp = __builtin_amdgcn_exp2f(s_acc[j][r] - m_new[r]);
          s_acc[j][r] = pp;
          p_sum[r] += pp;
        }
      }
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        #pragma unroll
        for (int off = 8; off > 0; off >>= 1)
          p_sum[r] += __shfl_xor(p_sum[r], off, WAVE);
        float alpha = __builtin_amdgcn_exp2f(m_run[rf][r] - m_new[r]);
        l_run[rf][r] = l_run[rf][r] * alpha + p_sum[r];
        m_run[rf][r] = m_new[r];
        #pragma unroll
        for (int j = 0; j < D / 16; ++j) o_acc[rf][j][r] *= alpha;
      }

      // ---- P through the wave strip, then P @ V -------------------------
      #pragma unroll
      for (int j = 0; j < KB / 16; ++j)
        #pragma unroll
        for (int r = 0; r < 4; ++r)
          p_lds[lsw((4 * fg + r) * KB + j * 16 + fr)] = f2bf(s_acc[j][r]);
      lds_fence();
      bf16x8v pf[KB / 32];
      #pragma unroll
      for (int ks = 0; ks < KB / 32; ++ks)
        pf[ks] = *reinterpret_cast<const bf16x8v*>(
            &p_lds[lsw(fr * KB + ks * 32 + fg * 8)]);
      lds_fence();   // strip is reused by the next fragment
      __builtin_amdgcn_s_setprio(1);
      #pragma unroll
      for (int j = 0; j < D / 16; ++j) {
        #pragma unroll
        for (int ks = 0; ks < KB / 32; ++ks) {
          bf16x8v vf = *reinterpret_cast<const bf16x8v*>(
              &vt_lds[lsw((j * 16 + fr) * KB + ks * 32 + fg * 8)]);
          o_acc[rf][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              pf[ks], vf, o_acc[rf][j], 0, 0, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);
    }
    }

    if (t + 1 < n_tiles)
      store_tile(t + 1);         // write the prefetched tile
    __syncthreads();
  }

  // ---- epilogue --------------------------------------------------------
  #pragma unroll
  for (int rf = 0; rf < RF; ++rf) {
    if (SW) {
      // softmax state lives per lane (col = qrow); o_acc rows need the
      // row-owners' 1/l via shuffle
      float invl = 1.f / l_run[rf][0];
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        int qrow = qr0[rf] + 4 * fg + r;
        if (qrow >= S) continue;
        float ir = __shfl(invl, 4 * fg + r, WAVE);
        #pragma unroll
        for (int j = 0; j < D / 16; ++j)
          o[(long)qrow * D + j * 16 + fr] = f2bf(o_acc[rf][j][r] * ir);
      }
      int myrow = qr0[rf] + fr;
      if (fg == 0 && myrow < S)
        lse[myrow] = 0.69314718055994530942f
                     * (m_run[rf][0] + __log2f(l_run[rf][0]));
      continue;
    }
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      int qrow = qr0[rf] + 4 * fg + r;
      if (qrow >= S) continue;
      float inv_l = 1.f / l_run[rf][r];
      #pragma unroll
      for (int j = 0; j < D / 16; ++j)
        o[(long)qrow * D + j * 16 + fr] = f2bf(o_acc[rf][j][r] * inv_l);
      if (fr == 0)   // m_run is log2-domain: lse = ln(sum exp) = ln2*(m2 + log2 l)
        lse[qrow] = 0.69314718055994530942f
                    * (m_run[rf][r] + __log2f(l_run[rf][r]));
    }
  }
}

// accept any 4-D view with a contiguous last dim (e.g. the [B,S,H,D]
// layout the qkv split produces) without materializing a copy
static inline at::Tensor ed_attn_arg(const at::Tensor& t) {
  return t.stride(3) == 1 ? t : t.contiguous();
}

// EASYDIST_ATTN_MAP: 1 = balanced (default), 0 = legacy placement, kept
// for A/B timing.  Read at every launch, not cached in a static, so one
// process can run both maps; a getenv is nothing next to these kernels.
static inline int ed_attn_map_mode() {
  const char* e = getenv("EASYDIST_ATTN_MAP");
  return (e && atoi(e) == 0) ? ATTN_MAP_LEGACY : ATTN_MAP_BALANCED;
}

// 1-D grid of nblk * nbh workgroups: the linear id the map consumes
static inline dim3 ed_attn_grid(long nblk, long nbh, const char* who) {
  TORCH_CHECK(nblk * nbh <= (long)INT_MAX, who,
              ": workgroup count ", nblk * nbh, " does not fit in an int");
  return dim3((unsigned)(nblk * nbh));
}

std::tuple<at::Tensor, at::Tensor> flash_attn_fwd(const at::Tensor& q_,
                                                  const at::Tensor& k_,
                                                  const at::Tensor& v_,
                                                  bool causal) {
  auto q = ed_attn_arg(q_), k = ed_attn_arg(k_), v = ed_attn_arg(v_);
  TORCH_CHECK(q.dtype() == at::kBFloat16 && q.dim() == 4);
  TORCH_CHECK(q.sizes() == k.sizes() && q.sizes() == v.sizes(),
              "flash_attn_fwd: q/k/v shapes must match");
  const int B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3);
  TORCH_CHECK(D == 64 || D == 128, "flash_attn_fwd: D in {64,128}");
  TORCH_CHECK(S % QB == 0, "flash_attn_fwd: S multiple of 64");
  auto out = at::empty({B, H, S, D}, q.options());
  auto lse = at::empty({B, H, S}, q.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream();
  static int rf = []() {
    const char* e = getenv("EASYDIST_FWD_RF");
    return e ? atoi(e) : 1;
  }();
  static int kd = []() {
    const char* e = getenv("EASYDIST_FWD_KDIRECT");
    return e ? atoi(e) : 0;
  }();
  static int sw = []() {   // default ON: -17% (D=64) / -12% (D=128) A/B'd
    const char* e = getenv("EASYDIST_FWD_SWAP");
    return e ? atoi(e) : 1;
  }();
  const int use_rf = (rf == 2 && S % 256 == 0) ? 2 : 1;
  dim3 grid = ed_attn_grid((S + 128 * use_rf - 1) / (128 * use_rf),
                           (long)B * H, "flash_attn_fwd"), block(512);
  const int map_mode = ed_attn_map_mode();
  size_t lds = (2 * ((size_t)KB * D + (size_t)KB * D) + 8 * 16 * KB) * 2;
  float scale = 1.f / sqrtf((float)D);
  auto kern = (D == 64)
      ? (use_rf == 2 ? flash_fwd_kernel<64, 2>
         : sw ? flash_fwd_kernel<64, 1, 0, 1>
         : kd ? flash_fwd_kernel<64, 1, 1> : flash_fwd_kernel<64, 1>)
      : (use_rf == 2 ? flash_fwd_kernel<128, 2>
         : sw ? flash_fwd_kernel<128, 1, 0, 1>
         : kd ? flash_fwd_kernel<128, 1, 1> : flash_fwd_kernel<128, 1>);
  hipLaunchKernelGGL(kern, grid, block, lds, stream,
      (const bf16*)q.data_ptr(), (const bf16*)k.data_ptr(),
      (const bf16*)v.data_ptr(), (bf16*)out.data_ptr(),
      lse.data_ptr<float>(), B, H, S, causal, scale,
      q.stride(0), q.stride(1), q.stride(2),
      k.stride(0), k.stride(1), k.stride(2),
      v.stride(0), v.stride(1), v.stride(2), map_mode);
  return {out, lse};
}

// ---------------------------------------------------------------------------
// Flash attention backward: two kernels, no atomics.
//   dq kernel: one workgroup per 64-row Q block; recomputes P from lse,
//     dP = dO V^T, dS = P (dP - delta) scale, dq += dS K.
//   dkv kernel: one workgroup per 64-key KV block; recomputes P^T,
//     dV += P^T dO, dP^T = V dO^T, dS^T = P^T (dP^T - delta) scale,
//     dK += dS^T Q.
// delta = rowsum(dO * O) comes precomputed from the host (one fused
// elementwise+reduce).
// mfma contract (as in fwd): D[m][n] += sum_k A[m][k] B[n][k]; A/B lanes
// hold row fr, k-slice fg; C/D lanes hold row 4*fg+r, col fr.
// ---------------------------------------------------------------------------

template <int D, int SW = 0>
__global__ void __launch_bounds__(512)
flash_bwd_dq_kernel(const bf16* __restrict__ dO, const bf16* __restrict__ Q,
                    const bf16* __restrict__ K, const bf16* __restrict__ V,
                    const float* __restrict__ LSE,
                    const float* __restrict__ DELTA, bf16* __restrict__ DQ,
                    int B, int H, int S, bool causal, float scale,
                    long dsb, long dsh, long dss, long qsb, long qsh,
                    long qss, long ksb, long ksh, long kss, long vsb,
                    long vsh, long vss, long osb, long osh, long oss,
                    int map_mode) {
  // 8 waves x 16 q rows: two 64-row halves share each staged K/V tile
  // (2x arithmetic intensity vs the 4-wave form) at 6+ waves/SIMD.
  // grid: 1-D, S/128 * B*H workgroups placed by attn_block_map
  const AttnBlock wgm = attn_block_map(blockIdx.x, S / (2 * QB), B * H,
                                       causal, map_mode);
  const int qb0 = wgm.blk * (2 * QB);
  const int bh = wgm.bh;
  const int b_ = bh / H, h_ = bh % H;
  const bf16* dO_ = dO + b_ * dsb + h_ * dsh;
  const bf16* q = Q + b_ * qsb + h_ * qsh;
  const bf16* k = K + b_ * ksb + h_ * ksh;
  const bf16* v = V + b_ * vsb + h_ * vsh;
  // output strides (elements): the packed-dqkv variant writes straight
  // into a [B,S,3,H,D] buffer, eliminating the transpose-clone-cat chain
  bf16* dq = DQ + b_ * osb + h_ * osh;
  const float* lse = LSE + (long)bh * S;
  const float* delta = DELTA + (long)bh * S;

  const int lane = threadIdx.x % WAVE;
  const int wave = threadIdx.x / WAVE;
  const int qr0 = qb0 + wave * 16;
  const int fr = lane & 15;
  const int fg = lane >> 4;

  // DOUBLE-BUFFERED K/V/K^T tiles (3 tiles per buffer): the single-
  // buffered store->barrier->compute form serialized the full staging
  // latency into every tile (bwd ran at ~127 TF vs the double-buffered
  // forward's 158+)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int DQBUF = 3 * KB * D;                // elements per buffer
  bf16* k_lds = reinterpret_cast<bf16*>(smem);     // + buf * DQBUF
  bf16* v_lds = k_lds + KB * D;
  bf16* kt_lds = v_lds + KB * D;                   // K^T [D][KB] + lsw
  bf16* s_lds = reinterpret_cast<bf16*>(smem) + 2 * DQBUF
                + wave * 16 * KB;                   // wave-private strip

  // A-operand fragments for this wave's 16 q rows
  bf16x8v qf[D / 32], dof[D / 32];
  #pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) {
    qf[ks] = *reinterpret_cast<const bf16x8v*>(
        &q[(long)(qr0 + fr) * qss + ks * 32 + fg * 8]);
    dof[ks] = *reinterpret_cast<const bf16x8v*>(
        &dO_[(long)(qr0 + fr) * dss + ks * 32 + fg * 8]);
  }
  // per C-row lse/delta (rows 4*fg+r; SW: one row per lane = fr)
  float lse_r[4], dlt_r[4];
  if (!SW) {
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      int qrow = qr0 + 4 * fg + r;
      lse_r[r] = lse[qrow];
      dlt_r[r] = delta[qrow];
    }
  } else {
    lse_r[0] = lse[qr0 + fr];
    dlt_r[0] = delta[qr0 + fr];
  }

  f32x4 dq_acc[D / 16];
  #pragma unroll
  for (int j = 0; j < D / 16; ++j) dq_acc[j] = {0.f, 0.f, 0.f, 0.f};

  const int kv_end = causal ? min(S, qb0 + 2 * QB) : S;
  // register-staged K/V prefetch: tile kv0+KB streams from HBM while the
  // MFMA/softmax work on kv0 runs (the unprefetched form exposed the
  // full HBM latency behind two barriers every tile)
  constexpr int NV = KB * D / (512 * 8);
  bf16x8 kreg[NV], vreg[NV];
  auto kv_load = [&](int t0) {
    #pragma unroll
    for (int pi = 0; pi < NV; ++pi) {
      const int e = threadIdx.x * 8 + pi * 4096;
      // row strides: the inputs may be [B,S,H,D]-layout views
      const long row = t0 + e / D;
      const int col = e % D;
      kreg[pi] = *reinterpret_cast<const bf16x8*>(&k[row * kss + col]);
      vreg[pi] = *reinterpret_cast<const bf16x8*>(&v[row * vss + col]);
    }
  };
  auto kv_store = [&](int buf) {
    #pragma unroll
    for (int pi = 0; pi < NV; ++pi) {
      const int e = threadIdx.x * 8 + pi * 4096;
      *reinterpret_cast<bf16x8*>(&k_lds[buf * DQBUF + lsw(e)]) = kreg[pi];
      *reinterpret_cast<bf16x8*>(&v_lds[buf * DQBUF + lsw(e)]) = vreg[pi];
      const int row = e / D, col = e % D;
      #pragma unroll
      for (int i = 0; i < 8; ++i)
        kt_lds[buf * DQBUF + lsw((col + i) * KB + row)] = kreg[pi].v[i];
    }
  };
  kv_load(0);
  kv_store(0);
  __syncthreads();
  const int n_kt = (kv_end + KB - 1) / KB;
  for (int tt = 0; tt < n_kt; ++tt) {
    const int kv0 = tt * KB;
    const int bofs = (tt & 1) * DQBUF;
    if (tt + 1 < n_kt) kv_load(kv0 + KB);
    if (causal && kv0 > qr0 + 15) {
      if (tt + 1 < n_kt) kv_store((tt + 1) & 1);
      __syncthreads();
      continue;
    }

    // S(^T) = Q K^T and dP(^T) = dO V^T: SW=1 swaps operands so the
    // C-layout holds ONE q row per lane (col = fr) with 16 keys in regs
    f32x4 s_acc[KB / 16], dp_acc[KB / 16];
    #pragma unroll
    for (int j = 0; j < KB / 16; ++j) {
      s_acc[j] = {0.f, 0.f, 0.f, 0.f};
      dp_acc[j] = {0.f, 0.f, 0.f, 0.f};
      #pragma unroll
      for (int ks = 0; ks < D / 32; ++ks) {
        bf16x8v kf = *reinterpret_cast<const bf16x8v*>(
            &k_lds[bofs + lsw((j * 16 + fr) * D + ks * 32 + fg * 8)]);
        bf16x8v vf = *reinterpret_cast<const bf16x8v*>(
            &v_lds[bofs + lsw((j * 16 + fr) * D + ks * 32 + fg * 8)]);
        if (SW) {
          s_acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              kf, qf[ks], s_acc[j], 0, 0, 0);
          dp_acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              vf, dof[ks], dp_acc[j], 0, 0, 0);
        } else {
          s_acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              qf[ks], kf, s_acc[j], 0, 0, 0);
          dp_acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              dof[ks], vf, dp_acc[j], 0, 0, 0);
        }
      }
    }
    // dS = P * (dP - delta) * scale, P = exp(S*scale - lse)
    bf16x8v dsf[KB / 32];
    if (SW) {
      const int qrow = qr0 + fr;
      const bool need_mask = (causal && kv0 + KB - 1 > qrow)
                             || (kv0 + KB > S);
      #pragma unroll
      for (int j = 0; j < KB / 16; ++j)
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          float p = 0.f;
          int kcol = kv0 + j * 16 + 4 * fg + r;
          if (!need_mask || (!(causal && kcol > qrow) && kcol < S))
            p = __expf(s_acc[j][r] * scale - lse_r[0]);
          s_acc[j][r] = p * (dp_acc[j][r] - dlt_r[0]) * scale;
        }
      unsigned pk[KB / 16][2];
      swp_pack(s_acc, KB / 16, pk);
      #pragma unroll
      for (int ks = 0; ks < KB / 32; ++ks)
        dsf[ks] = swp_butterfly(pk, ks, fg);
    } else {
    const bool need_mask = (causal && kv0 + KB - 1 > qr0 + 4 * fg)
                           || (kv0 + KB > S);
    if (need_mask) {
      #pragma unroll
      for (int j = 0; j < KB / 16; ++j) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          int kcol = kv0 + j * 16 + fr;
          int qrow = qr0 + 4 * fg + r;
          float p = 0.f;
          if (!(causal && kcol > qrow) && kcol < S)
            p = __expf(s_acc[j][r] * scale - lse_r[r]);
          s_acc[j][r] = p * (dp_acc[j][r] - dlt_r[r]) * scale;
        }
      }
    } else {
      #pragma unroll
      for (int j = 0; j < KB / 16; ++j) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          float p = __expf(s_acc[j][r] * scale - lse_r[r]);
          s_acc[j][r] = p * (dp_acc[j][r] - dlt_r[r]) * scale;
        }
      }
    }
    // re-fragment dS through the wave strip
    #pragma unroll
    for (int j = 0; j < KB / 16; ++j)
      #pragma unroll
      for (int r = 0; r < 4; ++r)
        s_lds[lsw((4 * fg + r) * KB + j * 16 + fr)] = f2bf(s_acc[j][r]);
    lds_fence();
    #pragma unroll
    for (int ks = 0; ks < KB / 32; ++ks)
      dsf[ks] = *reinterpret_cast<const bf16x8v*>(
          &s_lds[lsw(fr * KB + ks * 32 + fg * 8)]);
    }
    // dq += dS @ K: B-operand from K^T — contiguous vector loads
    #pragma unroll
    for (int j = 0; j < D / 16; ++j) {
      #pragma unroll
      for (int ks = 0; ks < KB / 32; ++ks) {
        bf16x8v kcol = *reinterpret_cast<const bf16x8v*>(
            &kt_lds[bofs + lsw((j * 16 + fr) * KB + ks * 32 + fg * 8)]);
        dq_acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsf[ks], kcol,
                                                            dq_acc[j], 0, 0,
                                                            0);
      }
    }
    if (tt + 1 < n_kt) kv_store((tt + 1) & 1);  // other buffer: no hazard
    __syncthreads();
  }
  #pragma unroll
  for (int r = 0; r < 4; ++r) {
    int qrow = qr0 + 4 * fg + r;
    if (qrow >= S) continue;
    #pragma unroll
    for (int j = 0; j < D / 16; ++j)
      dq[(long)qrow * oss + j * 16 + fr] = f2bf(dq_acc[j][r]);
  }
}

template <int D, int SW = 0>
__global__ void __launch_bounds__(512)
flash_bwd_dkv_kernel(const bf16* __restrict__ dO, const bf16* __restrict__ Q,
                     const bf16* __restrict__ K, const bf16* __restrict__ V,
                     const float* __restrict__ LSE,
                     const float* __restrict__ DELTA, bf16* __restrict__ DK,
                     bf16* __restrict__ DV, int B, int H, int S, bool causal,
                     float scale,
                     long dsb, long dsh, long dss, long qsb, long qsh,
                     long qss, long ksb, long ksh, long kss, long vsb,
                     long vsh, long vss, long osb, long osh, long oss,
                     int map_mode) {
  // 8 waves x 16 key rows share each staged Q/dO tile (see dq note)
  // grid: 1-D as in dq; kv block 0 is the causal-heavy one here, so the
  // map keeps the index order (heavy_last_index = false)
  const AttnBlock wgm = attn_block_map(blockIdx.x, S / (2 * KB), B * H,
                                       false, map_mode);
  const int kb0 = wgm.blk * (2 * KB);
  const int bh = wgm.bh;
  const int b_ = bh / H, h_ = bh % H;
  const bf16* dO_ = dO + b_ * dsb + h_ * dsh;
  const bf16* q = Q + b_ * qsb + h_ * qsh;
  const bf16* k = K + b_ * ksb + h_ * ksh;
  const bf16* v = V + b_ * vsb + h_ * vsh;
  bf16* dk = DK + b_ * osb + h_ * osh;
  bf16* dv = DV + b_ * osb + h_ * osh;
  const float* lse = LSE + (long)bh * S;
  const float* delta = DELTA + (long)bh * S;

  const int lane = threadIdx.x % WAVE;
  const int wave = threadIdx.x / WAVE;
  const int kr0 = kb0 + wave * 16;          // this wave's first key row
  const int fr = lane & 15;
  const int fg = lane >> 4;

  // DOUBLE-BUFFERED Q/dO/Q^T/dO^T tiles (see dq note)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int KVBUF = 4 * QB * D;                // elements per buffer
  bf16* q_lds = reinterpret_cast<bf16*>(smem);     // + buf * KVBUF
  bf16* do_lds = q_lds + QB * D;
  bf16* qt_lds = do_lds + QB * D;                  // Q^T [D][QB] + lsw
  bf16* dot_lds = qt_lds + QB * D;                 // dO^T [D][QB] + lsw
  bf16* s_lds = reinterpret_cast<bf16*>(smem) + 2 * KVBUF + wave * 16 * QB;

  bf16x8v kf[D / 32], vf[D / 32];
  #pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) {
    kf[ks] = *reinterpret_cast<const bf16x8v*>(
        &k[(long)(kr0 + fr) * kss + ks * 32 + fg * 8]);
    vf[ks] = *reinterpret_cast<const bf16x8v*>(
        &v[(long)(kr0 + fr) * vss + ks * 32 + fg * 8]);
  }

  f32x4 dk_acc[D / 16], dv_acc[D / 16];
  #pragma unroll
  for (int j = 0; j < D / 16; ++j) {
    dk_acc[j] = {0.f, 0.f, 0.f, 0.f};
    dv_acc[j] = {0.f, 0.f, 0.f, 0.f};
  }

  const int q_start = causal ? kb0 : 0;
  // register-staged Q/dO prefetch (see dq kernel note)
  constexpr int NV = QB * D / (512 * 8);
  bf16x8 qreg[NV], dreg[NV];
  auto q_load = [&](int t0) {
    #pragma unroll
    for (int pi = 0; pi < NV; ++pi) {
      const int e = threadIdx.x * 8 + pi * 4096;
      // row strides: the inputs may be [B,S,H,D]-layout views
      const long row = t0 + e / D;
      const int col = e % D;
      qreg[pi] = *reinterpret_cast<const bf16x8*>(&q[row * qss + col]);
      dreg[pi] = *reinterpret_cast<const bf16x8*>(&dO_[row * dss + col]);
    }
  };
  auto q_store = [&](int buf) {
    #pragma unroll
    for (int pi = 0; pi < NV; ++pi) {
      const int e = threadIdx.x * 8 + pi * 4096;
      *reinterpret_cast<bf16x8*>(&q_lds[buf * KVBUF + lsw(e)]) = qreg[pi];
      *reinterpret_cast<bf16x8*>(&do_lds[buf * KVBUF + lsw(e)]) = dreg[pi];
      const int row = e / D, col = e % D;
      #pragma unroll
      for (int i = 0; i < 8; ++i) {
        qt_lds[buf * KVBUF + lsw((col + i) * QB + row)] = qreg[pi].v[i];
        dot_lds[buf * KVBUF + lsw((col + i) * QB + row)] = dreg[pi].v[i];
      }
    }
  };
  q_load(q_start);
  q_store(0);
  __syncthreads();
  const int n_qt = (S - q_start + QB - 1) / QB;
  for (int tt = 0; tt < n_qt; ++tt) {
    const int q0 = q_start + tt * QB;
    const int bofs = (tt & 1) * KVBUF;
    if (tt + 1 < n_qt) q_load(q0 + QB);
    if (causal && q0 + QB - 1 < kr0) {
      if (tt + 1 < n_qt) q_store((tt + 1) & 1);
      __syncthreads();
      continue;
    }

    // S^T = K Q^T and dP^T = V dO^T.  SW=1 swaps the operand order so
    // the C-layout holds the wave's 16 KEYS on the lane column and 16
    // q cols in regs — the swp_butterfly then builds the P^T/dS^T
    // A-operands in-register (no strip, no fences).
    f32x4 st_acc[QB / 16], dpt_acc[QB / 16];
    #pragma unroll
    for (int j = 0; j < QB / 16; ++j) {
      st_acc[j] = {0.f, 0.f, 0.f, 0.f};
      dpt_acc[j] = {0.f, 0.f, 0.f, 0.f};
      #pragma unroll
      for (int ks = 0; ks < D / 32; ++ks) {
        bf16x8v qfb = *reinterpret_cast<const bf16x8v*>(
            &q_lds[bofs + lsw((j * 16 + fr) * D + ks * 32 + fg * 8)]);
        bf16x8v dob = *reinterpret_cast<const bf16x8v*>(
            &do_lds[bofs + lsw((j * 16 + fr) * D + ks * 32 + fg * 8)]);
        if (SW) {
          st_acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              qfb, kf[ks], st_acc[j], 0, 0, 0);
          dpt_acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              dob, vf[ks], dpt_acc[j], 0, 0, 0);
        } else {
          st_acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              kf[ks], qfb, st_acc[j], 0, 0, 0);
          dpt_acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              vf[ks], dob, dpt_acc[j], 0, 0, 0);
        }
      }
    }
    // P^T = exp(S^T*scale - lse[qcol]); dS^T = P^T (dP^T - delta[qcol]) scale
    bf16x8v ptf[QB / 32];
    const bool need_mask = (causal && kr0 + 15 > q0) || (q0 + QB > S);
    if (SW) {
      const int krow = kr0 + fr;             // this lane's key row
      // the 4 lse values a lane needs per j are CONSECUTIVE (4*fg+r):
      // one aligned 16-B vector load per j (scattered scalar loads and
      // ds_bpermute broadcasts both measured slower — the latter fight
      // the tile staging for the LDS port)
      #pragma unroll
      for (int j = 0; j < QB / 16; ++j) {
        f32x4 l4 = *reinterpret_cast<const f32x4*>(
            &lse[q0 + j * 16 + 4 * fg]);
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          int qcol = q0 + j * 16 + 4 * fg + r;
          float p = 0.f;
          if (!need_mask || (!(causal && krow > qcol) && qcol < S))
            p = __expf(st_acc[j][r] * scale - l4[r]);
          st_acc[j][r] = p;
        }
      }
      unsigned pk[QB / 16][2];
      swp_pack(st_acc, QB / 16, pk);
      #pragma unroll
      for (int ks = 0; ks < QB / 32; ++ks)
        ptf[ks] = swp_butterfly(pk, ks, fg);
    } else {
    // first pass: P^T into the strip for the dV mfma
    // no-mask fast path: whole wave's keys are <= every q col in tile
    if (need_mask) {
      #pragma unroll
      for (int j = 0; j < QB / 16; ++j) {
        int qcol = q0 + j * 16 + fr;
        float l = lse[qcol];
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          int krow = kr0 + 4 * fg + r;
          float p = 0.f;
          if (!(causal && krow > qcol) && qcol < S)
            p = __expf(st_acc[j][r] * scale - l);
          st_acc[j][r] = p;
          s_lds[lsw((4 * fg + r) * QB + j * 16 + fr)] = f2bf(p);
        }
      }
    } else {
      #pragma unroll
      for (int j = 0; j < QB / 16; ++j) {
        float l = lse[q0 + j * 16 + fr];
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          float p = __expf(st_acc[j][r] * scale - l);
          st_acc[j][r] = p;
          s_lds[lsw((4 * fg + r) * QB + j * 16 + fr)] = f2bf(p);
        }
      }
    }
    lds_fence();
    #pragma unroll
    for (int ks = 0; ks < QB / 32; ++ks)
      ptf[ks] = *reinterpret_cast<const bf16x8v*>(
          &s_lds[lsw(fr * QB + ks * 32 + fg * 8)]);
    }
    // dV += P^T @ dO: B-operand from dO^T — contiguous vector loads
    #pragma unroll
    for (int j = 0; j < D / 16; ++j) {
      #pragma unroll
      for (int ks = 0; ks < QB / 32; ++ks) {
        bf16x8v docol = *reinterpret_cast<const bf16x8v*>(
            &dot_lds[bofs + lsw((j * 16 + fr) * QB + ks * 32 + fg * 8)]);
        dv_acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ptf[ks], docol,
                                                            dv_acc[j], 0, 0,
                                                            0);
      }
    }
    // dS^T for the dK mfma: SW builds it in-register via the butterfly
    bf16x8v dstf[QB / 32];
    if (SW) {
      #pragma unroll
      for (int j = 0; j < QB / 16; ++j) {
        f32x4 d4 = *reinterpret_cast<const f32x4*>(
            &delta[q0 + j * 16 + 4 * fg]);
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          float ds = st_acc[j][r] * (dpt_acc[j][r] - d4[r]) * scale;
          st_acc[j][r] = ds;
        }
      }
      unsigned pk2[QB / 16][2];
      swp_pack(st_acc, QB / 16, pk2);
      #pragma unroll
      for (int ks = 0; ks < QB / 32; ++ks)
        dstf[ks] = swp_butterfly(pk2, ks, fg);
    } else {
    lds_fence();
    #pragma unroll
    for (int j = 0; j < QB / 16; ++j) {
      int qcol = q0 + j * 16 + fr;
      float dlt = delta[qcol];
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        float ds = st_acc[j][r] * (dpt_acc[j][r] - dlt) * scale;
        s_lds[lsw((4 * fg + r) * QB + j * 16 + fr)] = f2bf(ds);
      }
    }
    lds_fence();
    #pragma unroll
    for (int ks = 0; ks < QB / 32; ++ks)
      dstf[ks] = *reinterpret_cast<const bf16x8v*>(
          &s_lds[lsw(fr * QB + ks * 32 + fg * 8)]);
    }
    // dK += dS^T @ Q: B-operand from Q^T — contiguous vector loads
    #pragma unroll
    for (int j = 0; j < D / 16; ++j) {
      #pragma unroll
      for (int ks = 0; ks < QB / 32; ++ks) {
        bf16x8v qcolf = *reinterpret_cast<const bf16x8v*>(
            &qt_lds[bofs + lsw((j * 16 + fr) * QB + ks * 32 + fg * 8)]);
        dk_acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dstf[ks], qcolf,
                                                            dk_acc[j], 0, 0,
                                                            0);
      }
    }
    if (tt + 1 < n_qt) q_store((tt + 1) & 1);   // other buffer: no hazard
    __syncthreads();
  }
  #pragma unroll
  for (int r = 0; r < 4; ++r) {
    int krow = kr0 + 4 * fg + r;
    if (krow >= S) continue;
    #pragma unroll
    for (int j = 0; j < D / 16; ++j) {
      dk[(long)krow * oss + j * 16 + fr] = f2bf(dk_acc[j][r]);
      dv[(long)krow * oss + j * 16 + fr] = f2bf(dv_acc[j][r]);
    }
  }
}

// delta = rowsum(dO * O) in ONE bf16 pass (the aten composite spelled
// dO.float() * O.float() then sum(-1): three full fp32 materializations
// of activation-sized tensors per backward).
template <int D>
__global__ void __launch_bounds__(256)
attn_delta_kernel(const bf16* __restrict__ dO, const bf16* __restrict__ O,
                  float* __restrict__ delta, long rows, int H, int S,
                  long dsb, long dsh, long dss) {
  constexpr int LPR = D / 8;            // lanes per row (16B each)
  const int lane = threadIdx.x % WAVE;
  const int wave = threadIdx.x / WAVE;
  constexpr int RPW = WAVE / LPR;       // rows per wave
  long row = (long)blockIdx.x * (4 * RPW) + wave * RPW + lane / LPR;
  if (row >= rows) return;
  const int c0 = (lane % LPR) * 8;
  const long b_ = row / ((long)H * S), hs = row % ((long)H * S);
  const long h_ = hs / S, s_ = hs % S;
  const bf16x8 d8 = *reinterpret_cast<const bf16x8*>(
      &dO[b_ * dsb + h_ * dsh + s_ * dss + c0]);
  const bf16x8 o8 = *reinterpret_cast<const bf16x8*>(&O[row * D + c0]);
  float acc = 0.f;
  #pragma unroll
  for (int i = 0; i < 8; ++i) acc += bf2f(d8.v[i]) * bf2f(o8.v[i]);
  #pragma unroll
  for (int off = LPR / 2; off > 0; off >>= 1)
    acc += __shfl_down(acc, off, WAVE);
  if (lane % LPR == 0) delta[row] = acc;
}

static void
flash_attn_bwd_launch(const at::Tensor& grad_, const at::Tensor& q_,
                      const at::Tensor& k_, const at::Tensor& v_,
                      const at::Tensor& out, const at::Tensor& lse,
                      bool causal, bf16* dq_p, bf16* dk_p, bf16* dv_p,
                      long osb, long osh, long oss) {
  auto grad = ed_attn_arg(grad_);
  auto q = ed_attn_arg(q_), k = ed_attn_arg(k_), v = ed_attn_arg(v_);
  TORCH_CHECK(q.dtype() == at::kBFloat16 && q.dim() == 4);
  TORCH_CHECK(q.sizes() == k.sizes() && q.sizes() == v.sizes());
  TORCH_CHECK(out.is_contiguous(), "flash_attn_bwd: out must be contiguous");
  const int B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3);
  TORCH_CHECK(D == 64 || D == 128, "flash_attn_bwd: D in {64,128}");
  TORCH_CHECK(S % (2 * QB) == 0, "flash_attn_bwd: S multiple of 128");
  // delta = rowsum(dO * O), fp32 — one fused bf16 pass
  auto delta = at::empty({B, H, S}, q.options().dtype(at::kFloat));
  {
    long rows = (long)B * H * S;
    int rpw = (D == 64) ? 8 : 4;
    long nblk = (rows + 4 * rpw - 1) / (4 * rpw);
    auto stream0 = at::cuda::getCurrentCUDAStream();
    auto dkern = (D == 64) ? attn_delta_kernel<64> : attn_delta_kernel<128>;
    hipLaunchKernelGGL(dkern, dim3(nblk), dim3(256), 0,
        stream0, (const bf16*)grad.data_ptr(), (const bf16*)out.data_ptr(),
        delta.data_ptr<float>(), rows, H, S,
        grad.stride(0), grad.stride(1), grad.stride(2));
  }
  auto stream = at::cuda::getCurrentCUDAStream();
  dim3 grid = ed_attn_grid(S / (2 * QB), (long)B * H, "flash_attn_bwd"),
       block(512);
  const int map_mode = ed_attn_map_mode();
  // dq: DOUBLE-buffered (K+V+K^T) tiles + wave strips
  size_t lds = (2 * (3 * (size_t)KB * D) + 8 * 16 * KB) * 2;
  // dkv: DOUBLE-buffered (Q+dO+Q^T+dO^T) tiles + wave strips
  size_t lds_kv = (2 * (4 * (size_t)QB * D) + 8 * 16 * QB) * 2;
  float scale = 1.f / sqrtf((float)D);
  static int swb = []() {   // swapped-operand dq (butterfly dS transport)
    const char* e = getenv("EASYDIST_BWD_SWAP");
    return e ? atoi(e) : 1;
  }();
  auto qkern = (D == 64)
      ? (swb ? flash_bwd_dq_kernel<64, 1> : flash_bwd_dq_kernel<64>)
      : (swb ? flash_bwd_dq_kernel<128, 1> : flash_bwd_dq_kernel<128>);
  static int swkv = []() {  // dkv butterfly measured SLOWER than the
    const char* e = getenv("EASYDIST_DKV_SWAP");   // strip (2.11 vs 1.74
    return e ? atoi(e) : 0;                        // ms) — default off
  }();
  auto kkern = (D == 64)
      ? (swkv ? flash_bwd_dkv_kernel<64, 1> : flash_bwd_dkv_kernel<64>)
      : (swkv ? flash_bwd_dkv_kernel<128, 1> : flash_bwd_dkv_kernel<128>);
  hipLaunchKernelGGL(qkern, grid, block, lds, stream,
      (const bf16*)grad.data_ptr(), (const bf16*)q.data_ptr(),
      (const bf16*)k.data_ptr(), (const bf16*)v.data_ptr(),
      lse.data_ptr<float>(), delta.data_ptr<float>(),
      dq_p, B, H, S, causal, scale,
      grad.stride(0), grad.stride(1), grad.stride(2),
      q.stride(0), q.stride(1), q.stride(2),
      k.stride(0), k.stride(1), k.stride(2),
      v.stride(0), v.stride(1), v.stride(2), osb, osh, oss, map_mode);
  hipLaunchKernelGGL(kkern, grid, block, lds_kv, stream,
      (const bf16*)grad.data_ptr(), (const bf16*)q.data_ptr(),
      (const bf16*)k.data_ptr(), (const bf16*)v.data_ptr(),
      lse.data_ptr<float>(), delta.data_ptr<float>(),
      dk_p, dv_p, B, H, S, causal, scale,
      grad.stride(0), grad.stride(1), grad.stride(2),
      q.stride(0), q.stride(1), q.stride(2),
      k.stride(0), k.stride(1), k.stride(2),
      v.stride(0), v.stride(1), v.stride(2), osb, osh, oss, map_mode);
}

std::tuple<at::Tensor, at::Tensor, at::Tensor>
flash_attn_bwd(const at::Tensor& grad_, const at::Tensor& q_,
               const at::Tensor& k_, const at::Tensor& v_,
               const at::Tensor& out, const at::Tensor& lse, bool causal) {
  const int B = q_.size(0), H = q_.size(1), S = q_.size(2), D = q_.size(3);
  auto opts = q_.options();
  auto dq = at::empty({B, H, S, D}, opts);
  auto dk = at::empty({B, H, S, D}, opts);
  auto dv = at::empty({B, H, S, D}, opts);
  flash_attn_bwd_launch(grad_, q_, k_, v_, out, lse, causal,
                        (bf16*)dq.data_ptr(), (bf16*)dk.data_ptr(),
                        (bf16*)dv.data_ptr(),
                        (long)H * S * D, (long)S * D, D);
  return {dq, dk, dv};
}

// dq/dk/dv written straight into one [B, S, 3*H*D] buffer (the layout the
// qkv-projection backward consumes) — replaces the reference-model
// transpose+clone+cat chain (three strided gathers plus a cat copy,
// ~1.2 GB of pure layout traffic per GPT layer at batch 64).
at::Tensor
flash_attn_bwd_pack(const at::Tensor& grad_, const at::Tensor& q_,
                    const at::Tensor& k_, const at::Tensor& v_,
                    const at::Tensor& out, const at::Tensor& lse,
                    bool causal) {
  const long B = q_.size(0), H = q_.size(1), S = q_.size(2), D = q_.size(3);
  auto dqkv = at::empty({B, S, 3 * H * D}, q_.options());
  bf16* base = (bf16*)dqkv.data_ptr();
  // dq/dk/dv sections at column offsets 0, H*D, 2*H*D of the packed rows;
  // per-(b,h,s,d) element strides: osb=S*3HD, osh=D, oss=3HD
  flash_attn_bwd_launch(grad_, q_, k_, v_, out, lse, causal,
                        base, base + H * D, base + 2 * H * D,
                        S * 3 * H * D, D, 3 * H * D);
  return dqkv;
}