// Flash attention forward and backward for gfx950 (bf16, causal or full,
// D in {64, 128}, any S >= 1; S % 128 == 0 keeps its own instantiation;
// K/V may have fewer heads than Q, see GQA below).
//
// All four kernels share one structure: one workgroup = 8 waves = one
// 128-row block (q rows in fwd/dq, keys in dkv) of one (batch, head),
// placed on the chip by attn_block_map; each wave owns 16 rows (dkv also
// runs as 4 waves on a 64-key block, see flash_bwd_dkv_kernel).  The
// 64-row tiles of the other operand pair are register-prefetched from
// global memory and double-buffered in LDS, one swizzled row-major image
// per tile that is read by rows (ds_read_b128) and by columns
// (ds_read_b64_tr_b16); every product runs on v_mfma_f32_16x16x32_bf16.
//
// fwd and dq compute the SWAPPED-operand S^T = K Q^T, so each lane holds
// one q row: the online-softmax state (m, l) is one register pair per
// lane, row reductions are in-register plus two cross-group shuffles, and
// P / dS reach the next MFMA's A-operand layout through an in-register
// butterfly (swp_pack + swp_butterfly) with no LDS round-trip.  dkv ships
// un-swapped, re-fragmenting through a wave-private LDS strip.
#include "common.h"
#include "attn_block_map.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <climits>
#include <type_traits>

using f32x4 = __attribute__((ext_vector_type(4))) float;
using bf16x8v = __attribute__((ext_vector_type(8))) __bf16;

#define QB 64     // q tile (dkv); fwd/dq workgroups own 2*QB q rows
#define KB 64     // kv tile (fwd/dq); dkv workgroups own 2*KB keys

// Bank-conflict XOR swizzle for LINEAR [rows][64 or 128] bf16 LDS tiles
// (element-index form): a ds_read_b128 fragment read walks 16 rows at a
// 128/256-B stride, collapsing onto 2 (or 1) 16-B bank slots — 8/16-way
// conflicts (guide T2).  Folding row bits into the slot bits
// (e ^= ((e>>7)&15)<<3) is an involution, keeps 8-element chunks whole,
// and is injective across the 16 rows of a fragment for both row widths.
DEVINL int lsw(int e) { return e ^ (((e >> 7) & 15) << 3); }

// TR = 1: ONE row-major [rows][D] image per tile.  The products that sum
// over the image's ROWS (PV, dS K, P^T dO, dS^T Q) take their B operand
// from it with the gfx950 transposed read (tr_frag) instead of from a
// second, transposed copy built with 2-byte scalar stores.  lsw leaves
// that read 2-way conflicted at both row widths: a 32-lane half takes
// rows r..r+3 and r+8..r+11 in the two 16-B chunks {2j, 2j+1}, and lsw
// sends (row, chunk 2j+1) and (row+1, chunk 2j) to one slot.  tsw XORs
// only row bits 0, 1 and 3 into chunk bits 3, 1 and 2 (row bit 0 is
// already bit 3 of the 256-B slot index at D = 64, hence the mask) and
// leaves chunk bit 0 alone: by the bank rule ((byte/4) % 64, groups as in
// the LDS table) the ds_read_b128 row read, the transposed read and the
// 16-B store are all conflict-free at D = 64 and D = 128.  Element-index
// form like lsw; 8-element chunks stay whole.  Stores and both kinds of
// read go through isw.
template <int D>
DEVINL int tsw(int e) {
  const int r = e / D;
  const int g = (((r & 1) << 3) | (((r >> 3) & 1) << 2) | (((r >> 1) & 1) << 1))
                & (D / 8 - 1);
  return e ^ (g << 3);
}
template <int D, bool TR>
DEVINL int isw(int e) {
  if constexpr (TR) return tsw<D>(e);
  else return lsw(e);
}

// B-operand fragment of v_mfma_f32_16x16x32_bf16 from a row-major tsw
// image: n = image column c0 + fr, k = image rows r0 + 8*fg + 0..7, with
// r0 a multiple of 32 and c0 of 16.  Two ds_read_b64_tr_b16, rows +0..3
// and +4..7: lane 4q+p of a 16-lane group supplies the address of row q,
// columns 4p..4p+3, and lane i receives column i.  A lane's row is
// r0 + 8*fg + 4h + q, so the row bits tsw uses (0, 1, 3) are the lane's
// own for every fragment: tr_lane() gives the lane's element offset and
// XOR once, and a fragment costs one xor-add per c0 with r0 and h in the
// instruction's immediate offset.  Needs EXEC all ones: call it under
// wave-uniform control flow only.
using v4s = __attribute__((ext_vector_type(4))) short;
using v8s = __attribute__((ext_vector_type(8))) short;
struct TrLane { int off, x; };
template <int D, bool TR>
DEVINL TrLane tr_lane(int fr, int fg) {
  if constexpr (!TR) return {0, 0};
  const int e = (fg * 8 + (fr >> 2)) * D + (fr & 3) * 4;
  return {e, tsw<D>(e) ^ e};
}
template <int D>
DEVINL bf16x8v tr_frag(const bf16* img, TrLane tl, int r0, int c0) {
  // tl.x has bits 4..6 only (tsw leaves chunk bit 0 alone) and c0 bits
  // 4..6 only, so the XOR stays clear of the lane's (fr & 3) * 4
  const bf16* a = img + ((c0 ^ tl.x) + tl.off) + r0 * D;
  v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) v4s*)a);
  v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) v4s*)(a + 4 * D));
  v8s out = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8v, out);
}

// Register type of one staged 16-byte vector.  The struct (element access
// for the 2-byte transposed stores) reaches LDS through a stack slot; TR
// never takes a vector apart, and the plain vector type keeps the
// prefetch in registers (no scratch in any TR = 1 kernel).
template <bool TR>
using stage_t = std::conditional_t<TR, bf16x8v, bf16x8>;

// LDS elements (bf16) each kernel asks for; the launch code sizes the
// dynamic LDS from these.  TR = 0 keeps the parent's sizes, including the
// 8 * 16 * KB strip elements fwd and dq no longer touch (LDS size sets
// workgroups per CU, so TR = 0 stays what was measured before).
template <int D, bool TR> constexpr int fwd_lds_elems() {
  return 2 * (2 * KB * D) + (TR ? 0 : 8 * 16 * KB);
}
template <int D, bool TR> constexpr int dq_lds_elems() {
  return 2 * ((TR ? 2 : 3) * KB * D) + (TR ? 0 : 8 * 16 * KB);
}
template <int D, bool TR, int NW = 8> constexpr int dkv_lds_elems() {
  return 2 * ((TR ? 2 : 4) * QB * D) + NW * 16 * QB;  // + P^T/dS^T strips
}


// ---- RAGGED: any S >= 1 ----------------------------------------------------
// RAGGED = false is the S % 128 == 0 code, exactly as it was measured:
// rag_row is the identity there and nblk keeps its spelling, so the
// compiler emits the same instructions as before the parameter existed.
// RAGGED = true is picked by the launch code for every other S and differs
// in the ROW INDEX of its global loads only: rag_row clamps it to S - 1,
// so no lane forms an address past the last row, the loads stay branch-free
// (one v_min each; no tile-uniform test is needed, and the schedule stays
// that of the aligned kernels), and a row >= S arrives as a copy of row
// S - 1: finite, never uninitialised.  The forward's own q rows >= S are
// zeros, as they always were.  Tile order and per-element arithmetic are
// those of RAGGED = false on the same tensors padded to a multiple of 128.
// A key or q column >= S is masked wherever it could contribute, masked
// probabilities are exact zeros and 0 * (a copied row) is 0; a q or key
// row >= S that a wave owns computes what row S - 1 computes, an MFMA
// keeps rows apart, and such accumulator rows are never stored.  No q row
// < S can be fully masked (under the causal mask row i always sees key
// i), so the -1e30 sentinel and 1 / l_run need no special case here
// either: do not add one.  Every wave, including one whose 16 rows are all
// >= S, walks the same block-uniform tile loop and so reaches every
// __syncthreads(), with EXEC all ones at every transposed read.
template <bool RAGGED>
DEVINL int rag_row(int row, int S) {
  if constexpr (RAGGED) return min(row, S - 1);
  else return row;
}

// ---- GQA: fewer K/V heads than query heads ----------------------------------
// K and V are [B, Hkv, S, D] with H = G * Hkv, and query head h attends K/V
// head h / G (torch's repeat_interleave convention).  GQA = false is the
// Hkv == H code as it was measured: the G argument is never read there.
// fwd and dq differ in the head of their K/V base pointer only.  dkv runs
// one workgroup per key block of a K/V head and walks the Q/dO tiles of
// its G query heads in one loop, summing into the same fp32 accumulators:
// dk and dv are rounded to bf16 once, with no atomics and no second pass.
// GQA exists in the default forms only (fwd and dq TR = 1, dkv SW = 0 and
// TR = ATTN_TR_DKV(D, NW)), like RAGGED.

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

// Swapped-operand form: QK^T runs as K*Q^T so the C-layout puts ONE q row
// per lane (col = l&15 = qrow, regs = 16 keys). The online softmax then
// reduces over REGISTERS (15 VALU max/add) plus TWO shuffles (xor 16/32
// across the fg groups) instead of four dependent 4-level shuffle trees,
// and P reaches the PV A-operand layout through the 12-shuffle in-register
// butterfly above instead of an LDS strip round-trip.  The un-swapped
// strip form, a 256-row (two fragments per wave) block and direct-from-L2
// K reads were all A/B'd on hardware and lost (profiles/README.md).
template <int D, bool TR, bool RAGGED = false, bool GQA = false>
__global__ void
// waves/SIMD floor.  The aligned D = 64 kernel fits 5 (96 VGPRs); the
// clamped row index costs the ragged one 4 more, so it runs at 4: a floor
// of 5 there made the allocator spill 3 VGPRs to scratch.
__launch_bounds__(512, (D == 64 ? 4 : 1))
flash_fwd_kernel(const bf16* __restrict__ Q, const bf16* __restrict__ K,
                 const bf16* __restrict__ V, bf16* __restrict__ O,
                 float* __restrict__ LSE, int B, int H, int S, bool causal,
                 float scale,
                 long qsb, long qsh, long qss, long ksb, long ksh, long kss,
                 long vsb, long vsh, long vss, int map_mode, int G) {
  // grid: 1-D, ceil(S/QBLK) * B*H workgroups placed by attn_block_map
  // (attn_block_map.h); 8 waves of one 16-row fragment each.  The round-1
  // 4-wave/256-thread form ran ONE wave per SIMD (110 KB LDS) — every
  // softmax/LDS stall fully exposed, ~100 TF effective.  8 waves + the
  // smaller LDS footprint give 4 waves/SIMD at D=64.
  constexpr int QBLK = 2 * QB;
  const AttnBlock wgm = attn_block_map(blockIdx.x, (S + QBLK - 1) / QBLK,
                                       B * H, causal, map_mode);
  const int qb0 = wgm.blk * QBLK;
  const int bh = wgm.bh;
  const int b_ = bh / H, h_ = bh % H;
  // inputs may be [B,S,H,D]-layout views (the qkv split) — per-tensor
  // batch/head/row strides avoid the activation-sized .contiguous()
  // copies the round-1 wrapper made every step
  const int hk = GQA ? h_ / G : h_;    // this head's K/V head
  const bf16* q = Q + b_ * qsb + h_ * qsh;
  const bf16* k = K + b_ * ksb + hk * ksh;
  const bf16* v = V + b_ * vsb + hk * vsh;
  bf16* o = O + (long)bh * S * D;
  float* lse = LSE + (long)bh * S;

  const int lane = threadIdx.x % WAVE;
  const int wave = threadIdx.x / WAVE;

  // LDS: DOUBLE-BUFFERED K [KB][D] + V^T [D][KB] (lsw) pairs; under TR
  // the second tile is V [KB][D] and both are tsw images.
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TILE_K = KB * D;
  constexpr int TILE_VT = KB * D;   // [D][KB] linear + lsw swizzle
  static_assert(2 * (TILE_K + TILE_VT) <= fwd_lds_elems<D, TR>());
  bf16* smem_b = reinterpret_cast<bf16*>(smem);
  constexpr int NTHR = 8 * WAVE;   // 512

  const int fr = lane & 15;        // fragment row/col index
  const int fg = lane >> 4;        // fragment k-group (8 contiguous)
  const TrLane trl = tr_lane<D, TR>(fr, fg);   // transposed reads (TR only)

  const int qr0 = qb0 + wave * 16; // this wave's first q row
  const int qrow = qr0 + fr;       // this lane's q row

  // Q fragments (B operand of S^T), PRE-SCALED by scale*log2(e): the
  // softmax runs in exp2 domain (v_exp2 without the fused multiply) and
  // the hot loop loses its per-element scale multiply
  const float qscale = scale * 1.44269504088896340736f;
  bf16x8v qf[D / 32];
  #pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) {
    if (qrow < S) {
      bf16x8v raw = *reinterpret_cast<const bf16x8v*>(
          &q[(long)qrow * qss + ks * 32 + fg * 8]);
      #pragma unroll
      for (int u = 0; u < 8; ++u)
        qf[ks][u] = (__bf16)(bf2f((bf16)raw[u]) * qscale);
    } else {
      #pragma unroll
      for (int u = 0; u < 8; ++u) qf[ks][u] = (__bf16)0.f;
    }
  }

  // softmax state of THIS LANE's q row; o_acc rows are qrows 4*fg+r
  float m_run = -1e30f, l_run = 0.f;
  f32x4 o_acc[D / 16];
  #pragma unroll
  for (int j = 0; j < D / 16; ++j) o_acc[j] = {0.f, 0.f, 0.f, 0.f};

  const int kv_end = causal ? min(S, qb0 + QBLK) : S;
  const int n_tiles = (kv_end + KB - 1) / KB;
  constexpr int PF = TILE_K / (NTHR * 8);    // 16B vectors per thread
  stage_t<TR> kreg[PF], vreg[PF];

  auto load_tile = [&](int t) {
    #pragma unroll
    for (int pi = 0; pi < PF; ++pi) {
      const int e = threadIdx.x * 8 + pi * (NTHR * 8);
      const int row = rag_row<RAGGED>(t * KB + e / D, S), col = e % D;
      kreg[pi] = *reinterpret_cast<const stage_t<TR>*>(
          &k[(long)row * kss + col]);
      vreg[pi] = *reinterpret_cast<const stage_t<TR>*>(
          &v[(long)row * vss + col]);
    }
  };
  auto store_tile = [&](int t) {
    bf16* kb = smem_b + (t & 1) * (TILE_K + TILE_VT);
    bf16* vb = kb + TILE_K;
    #pragma unroll
    for (int pi = 0; pi < PF; ++pi) {
      const int e = threadIdx.x * 8 + pi * (NTHR * 8);
      *reinterpret_cast<stage_t<TR>*>(&kb[isw<D, TR>(e)]) = kreg[pi];
      if constexpr (TR) {
        *reinterpret_cast<bf16x8v*>(&vb[tsw<D>(e)]) = vreg[pi];
      } else {
        const int row = e / D, col = e % D;
        #pragma unroll
        for (int i = 0; i < 8; ++i)
          vb[lsw((col + i) * KB + row)] = vreg[pi].v[i];
      }
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

    // a 128-row block spans 8 waves: tiles strictly above this wave's
    // causal diagonal are all-masked — skip the compute (NOT the
    // barriers: every wave still arrives at __syncthreads)
    const bool wave_active = !(causal && kv0 > qr0 + 15);
    if (wave_active) {
      // ---- S^T = K Q^T: lane col = qrow, regs = 16 keys ---------------
      f32x4 s_acc[KB / 16];
      __builtin_amdgcn_s_setprio(1);
      #pragma unroll
      for (int j = 0; j < KB / 16; ++j) {
        s_acc[j] = {0.f, 0.f, 0.f, 0.f};
        #pragma unroll
        for (int ks = 0; ks < D / 32; ++ks) {
          bf16x8v kf = *reinterpret_cast<const bf16x8v*>(
              &k_lds[isw<D, TR>((j * 16 + fr) * D + ks * 32 + fg * 8)]);
          s_acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              kf, qf[ks], s_acc[j], 0, 0, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);
      // ---- online softmax ---------------------------------------------
      // interior tiles (fully below the causal diagonal, fully in-range)
      // skip the per-element mask compares — most tiles at long S
      const bool need_mask = (causal && kv0 + KB - 1 > qrow)
                             || (kv0 + KB > S);
      float mx = -1e30f;
      if (need_mask) {
        #pragma unroll
        for (int j = 0; j < KB / 16; ++j)
          #pragma unroll
          for (int r = 0; r < 4; ++r) {
            int kcol = kv0 + j * 16 + 4 * fg + r;
            float sv = s_acc[j][r];        // already scale*log2e scaled
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
      float m_new = fmaxf(m_run, mx);
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
      float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      l_run = l_run * alpha + psum;
      m_run = m_new;
      // o_acc rows are qrows 4*fg+r: fetch those rows' alpha
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        float ar = __shfl(alpha, 4 * fg + r, WAVE);
        #pragma unroll
        for (int j = 0; j < D / 16; ++j) o_acc[j][r] *= ar;
      }
      // ---- P through the butterfly, then P @ V ------------------------
      unsigned pk[KB / 16][2];
      swp_pack(s_acc, KB / 16, pk);
      __builtin_amdgcn_s_setprio(1);
      #pragma unroll
      for (int ks = 0; ks < KB / 32; ++ks) {
        bf16x8v pv = swp_butterfly(pk, ks, fg);
        #pragma unroll
        for (int j = 0; j < D / 16; ++j) {
          bf16x8v vf;
          if constexpr (TR)
            vf = tr_frag<D>(vt_lds, trl, ks * 32, j * 16);
          else
            vf = *reinterpret_cast<const bf16x8v*>(
                &vt_lds[lsw((j * 16 + fr) * KB + ks * 32 + fg * 8)]);
          o_acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              pv, vf, o_acc[j], 0, 0, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);
    }

    if (t + 1 < n_tiles)
      store_tile(t + 1);         // write the prefetched tile
    __syncthreads();
  }

  // ---- epilogue --------------------------------------------------------
  // o_acc rows need the row-owners' 1/l via shuffle
  float invl = 1.f / l_run;
  #pragma unroll
  for (int r = 0; r < 4; ++r) {
    int orow = qr0 + 4 * fg + r;
    if (orow >= S) continue;
    float ir = __shfl(invl, 4 * fg + r, WAVE);
    #pragma unroll
    for (int j = 0; j < D / 16; ++j)
      o[(long)orow * D + j * 16 + fr] = f2bf(o_acc[j][r] * ir);
  }
  // m_run is log2-domain: lse = ln(sum exp) = ln2*(m2 + log2 l)
  if (fg == 0 && qrow < S)
    lse[qrow] = 0.69314718055994530942f * (m_run + __log2f(l_run));
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

// EASYDIST_ATTN_TR: 1 = one LDS image per tile, read transposed by the
// hardware; 0 = the second, transposed copy, kept for A/B timing and the
// bit-equality test.  Unset, each kernel runs the form that measured
// faster (profiles/README.md Round 6): TR = 1 everywhere but the D = 64
// dkv kernel, which stays VGPR-bound at one workgroup per CU under either
// form and ran 0.3% (causal) to 6.8% (full) slower with the transposed
// reads.  Read at every launch like the map.
// This knob and EASYDIST_DKV_SWAP are A/B timing knobs for the measured
// S % 128 == 0 shapes.  Any other S ignores both: the ragged kernels exist
// in the default form only (fwd and dq TR = 1, dkv TR = ATTN_TR_DKV(D, NW) and
// SW = 0).  EASYDIST_ATTN_MAP is a kernel argument and holds for every S.
// Hkv != H ignores the two knobs in the same way: the GQA kernels exist in
// the default form only, and EASYDIST_ATTN_MAP holds.
#define ATTN_TR_FWD 1
#define ATTN_TR_DQ 1
// The dkv default is per geometry (NW waves, see EASYDIST_DKV_GEOM): the
// 4-wave form needs the 40-KiB TR = 1 request to fit its workgroups.
#define ATTN_TR_DKV(D, NW) ((D) == 128 || (NW) == 4)
static inline bool ed_attn_tr(bool dflt) {
  const char* e = getenv("EASYDIST_ATTN_TR");
  return e ? atoi(e) != 0 : dflt;
}

// EASYDIST_DKV_GEOM: 0 = 8 waves per dkv workgroup on a 128-key block,
// full-tile loop (the kernel as it was); 1 = 4 waves on a 64-key block
// with the half-tile loop, three workgroups per CU at D = 64.  Unset,
// each head size runs what measured faster (profiles/README.md Round 10).
// Read at every launch; it holds for every S and for GQA, each geometry
// running its ragged and GQA kernels in that geometry's default TR form.
// D = 128 stays on geometry 0 (two workgroups per CU at best, 5 to 34%
// slower).  D = 64 runs geometry 1, except for a launch without the mask
// that is only a few rounds of workgroups long: there every workgroup
// does equal work and the time is rounds x time per workgroup.  A 64-key
// workgroup beside two others takes 4/3 of what a 128-key workgroup takes
// alone on its CU (64.4 against 48.9 us at B64 H12 S1024), so geometry 1
// needs 3/4 of the rounds or fewer; 1024 workgroups on 768 slots are two
// rounds like 512 on 256, and measured 17% slower.  Under the causal mask
// the heavy-first order fills the tail and geometry 1 won at every size.
#define ATTN_DKV_GEOM(D) ((D) == 64)
static inline bool ed_dkv_geom(int D, bool causal, long S, long nbh) {
  const char* e = getenv("EASYDIST_DKV_GEOM");
  if (e) return atoi(e) != 0;
  if (!ATTN_DKV_GEOM(D)) return false;
  if (causal) return true;
  const long cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const long r0 = ((S + 127) / 128 * nbh + cus - 1) / cus;
  const long r1 = ((S + 63) / 64 * nbh + 3 * cus - 1) / (3 * cus);
  return 4 * r1 <= 3 * r0;
}

// Shape contract of the three host entries: bf16 q [B, H, S, D] and
// k, v [B, Hkv, S, D] with H % Hkv == 0.  Returns G = H / Hkv.
static inline int ed_attn_group(const at::Tensor& q, const at::Tensor& k,
                                const at::Tensor& v, const char* who) {
  TORCH_CHECK(q.dtype() == at::kBFloat16 && q.dim() == 4, who,
              ": q must be a 4-D bf16 tensor");
  TORCH_CHECK(k.dtype() == at::kBFloat16 && v.dtype() == at::kBFloat16, who,
              ": k and v must be bf16");
  TORCH_CHECK(k.dim() == 4 && k.sizes() == v.sizes(), who,
              ": k and v must be 4-D and of one shape");
  TORCH_CHECK(k.size(0) == q.size(0) && k.size(2) == q.size(2) &&
              k.size(3) == q.size(3), who,
              ": k/v must agree with q in batch, sequence and head dim");
  TORCH_CHECK(k.size(1) >= 1 && q.size(1) % k.size(1) == 0, who, ": ",
              q.size(1), " query heads are no multiple of ", k.size(1),
              " K/V heads");
  return (int)(q.size(1) / k.size(1));
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
  const int G = ed_attn_group(q, k, v, "flash_attn_fwd");
  const int B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3);
  TORCH_CHECK(D == 64 || D == 128, "flash_attn_fwd: D in {64,128}");
  TORCH_CHECK(S >= 1, "flash_attn_fwd: S >= 1");
  const bool ragged = S % (2 * QB) != 0;
  auto out = at::empty({B, H, S, D}, q.options());
  auto lse = at::empty({B, H, S}, q.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream();
  dim3 grid = ed_attn_grid((S + 2 * QB - 1) / (2 * QB), (long)B * H,
                           "flash_attn_fwd"), block(512);
  const int map_mode = ed_attn_map_mode();
  // LDS bytes -> workgroups per 160-KiB CU, D = 64 / 128:
  //   TR = 0: 48 / 80 KiB -> 3 / 2;  TR = 1: 32 / 64 KiB -> 5 / 2
  const bool tr = (ragged || G > 1) ? ATTN_TR_FWD : ed_attn_tr(ATTN_TR_FWD);
  static_assert(ATTN_TR_FWD == 1 && ATTN_TR_DQ == 1,
                "the ragged and GQA fwd and dq kernels are instantiated "
                "for TR = 1");
  size_t lds = sizeof(bf16) *
      (D == 64 ? (tr ? fwd_lds_elems<64, true>() : fwd_lds_elems<64, false>())
               : (tr ? fwd_lds_elems<128, true>()
                     : fwd_lds_elems<128, false>()));
  float scale = 1.f / sqrtf((float)D);
  auto kern = (D == 64)
      ? (tr ? flash_fwd_kernel<64, true> : flash_fwd_kernel<64, false>)
      : (tr ? flash_fwd_kernel<128, true> : flash_fwd_kernel<128, false>);
  if (ragged)
    kern = (D == 64) ? flash_fwd_kernel<64, true, true>
                     : flash_fwd_kernel<128, true, true>;
  if (G > 1)
    kern = (D == 64)
        ? (ragged ? flash_fwd_kernel<64, true, true, true>
                  : flash_fwd_kernel<64, true, false, true>)
        : (ragged ? flash_fwd_kernel<128, true, true, true>
                  : flash_fwd_kernel<128, true, false, true>);
  hipLaunchKernelGGL(kern, grid, block, lds, stream,
      (const bf16*)q.data_ptr(), (const bf16*)k.data_ptr(),
      (const bf16*)v.data_ptr(), (bf16*)out.data_ptr(),
      lse.data_ptr<float>(), B, H, S, causal, scale,
      q.stride(0), q.stride(1), q.stride(2),
      k.stride(0), k.stride(1), k.stride(2),
      v.stride(0), v.stride(1), v.stride(2), map_mode, G);
  return {out, lse};
}

// ---------------------------------------------------------------------------
// Flash attention backward: two kernels, no atomics.
//   dq kernel: one workgroup per 128-row Q block; recomputes P from lse,
//     dP = dO V^T, dS = P (dP - delta) scale, dq += dS K.
//   dkv kernel: one workgroup per 128-key KV block; recomputes P^T,
//     dV += P^T dO, dP^T = V dO^T, dS^T = P^T (dP^T - delta) scale,
//     dK += dS^T Q.
// delta = rowsum(dO * O) comes precomputed from the host (one fused
// elementwise+reduce).
// mfma contract (as in fwd): D[m][n] += sum_k A[m][k] B[n][k]; A/B lanes
// hold row fr, k-slice fg; C/D lanes hold row 4*fg+r, col fr.
// ---------------------------------------------------------------------------

template <int D, bool TR, bool RAGGED = false, bool GQA = false>
__global__ void __launch_bounds__(512)
flash_bwd_dq_kernel(const bf16* __restrict__ dO, const bf16* __restrict__ Q,
                    const bf16* __restrict__ K, const bf16* __restrict__ V,
                    const float* __restrict__ LSE,
                    const float* __restrict__ DELTA, bf16* __restrict__ DQ,
                    int B, int H, int S, bool causal, float scale,
                    long dsb, long dsh, long dss, long qsb, long qsh,
                    long qss, long ksb, long ksh, long kss, long vsb,
                    long vsh, long vss, long osb, long osh, long oss,
                    int map_mode, int G) {
  // 8 waves x 16 q rows: two 64-row halves share each staged K/V tile
  // (2x arithmetic intensity vs the 4-wave form) at 6+ waves/SIMD.
  // grid: 1-D, ceil(S/128) * B*H workgroups placed by attn_block_map
  // (S / 128 spelled as before where it is exact: same code as measured)
  const int nblk = RAGGED ? (S + 2 * QB - 1) / (2 * QB) : S / (2 * QB);
  const AttnBlock wgm = attn_block_map(blockIdx.x, nblk, B * H,
                                       causal, map_mode);
  const int qb0 = wgm.blk * (2 * QB);
  const int bh = wgm.bh;
  const int b_ = bh / H, h_ = bh % H;
  const int hk = GQA ? h_ / G : h_;    // this head's K/V head
  const bf16* dO_ = dO + b_ * dsb + h_ * dsh;
  const bf16* q = Q + b_ * qsb + h_ * qsh;
  const bf16* k = K + b_ * ksb + hk * ksh;
  const bf16* v = V + b_ * vsb + hk * vsh;
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
  const TrLane trl = tr_lane<D, TR>(fr, fg);   // transposed reads (TR only)

  // DOUBLE-BUFFERED K/V/K^T tiles (3 tiles per buffer; under TR K and V
  // only, dS K reads the K image transposed): the single-
  // buffered store->barrier->compute form serialized the full staging
  // latency into every tile (bwd ran at ~127 TF vs the double-buffered
  // forward's 158+)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int DQBUF = (TR ? 2 : 3) * KB * D;     // elements per buffer
  static_assert(2 * DQBUF <= dq_lds_elems<D, TR>());
  bf16* k_lds = reinterpret_cast<bf16*>(smem);     // + buf * DQBUF
  bf16* v_lds = k_lds + KB * D;
  bf16* kt_lds = v_lds + KB * D;       // K^T [D][KB] + lsw (TR = 0 only)

  // A-operand fragments for this wave's 16 q rows
  bf16x8v qf[D / 32], dof[D / 32];
  #pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) {
    qf[ks] = *reinterpret_cast<const bf16x8v*>(
        &q[(long)rag_row<RAGGED>(qr0 + fr, S) * qss + ks * 32 + fg * 8]);
    dof[ks] = *reinterpret_cast<const bf16x8v*>(
        &dO_[(long)rag_row<RAGGED>(qr0 + fr, S) * dss + ks * 32 + fg * 8]);
  }
  // swapped operands below: one q row per lane, so one lse/delta each
  // (scalar loads: the [B,H,S] slabs start at bh * S floats, any alignment)
  const int qrow = qr0 + fr;
  const float lse_r = lse[rag_row<RAGGED>(qrow, S)];
  const float dlt_r = delta[rag_row<RAGGED>(qrow, S)];

  f32x4 dq_acc[D / 16];
  #pragma unroll
  for (int j = 0; j < D / 16; ++j) dq_acc[j] = {0.f, 0.f, 0.f, 0.f};

  const int kv_end = causal ? min(S, qb0 + 2 * QB) : S;
  // register-staged K/V prefetch: tile kv0+KB streams from HBM while the
  // MFMA/softmax work on kv0 runs (the unprefetched form exposed the
  // full HBM latency behind two barriers every tile)
  constexpr int NV = KB * D / (512 * 8);
  stage_t<TR> kreg[NV], vreg[NV];
  auto kv_load = [&](int t0) {
    #pragma unroll
    for (int pi = 0; pi < NV; ++pi) {
      const int e = threadIdx.x * 8 + pi * 4096;
      // row strides: the inputs may be [B,S,H,D]-layout views
      const long row = rag_row<RAGGED>(t0 + e / D, S);
      const int col = e % D;
      kreg[pi] = *reinterpret_cast<const stage_t<TR>*>(&k[row * kss + col]);
      vreg[pi] = *reinterpret_cast<const stage_t<TR>*>(&v[row * vss + col]);
    }
  };
  auto kv_store = [&](int buf) {
    #pragma unroll
    for (int pi = 0; pi < NV; ++pi) {
      const int e = threadIdx.x * 8 + pi * 4096;
      *reinterpret_cast<stage_t<TR>*>(
          &k_lds[buf * DQBUF + isw<D, TR>(e)]) = kreg[pi];
      *reinterpret_cast<stage_t<TR>*>(
          &v_lds[buf * DQBUF + isw<D, TR>(e)]) = vreg[pi];
      if constexpr (!TR) {
        const int row = e / D, col = e % D;
        #pragma unroll
        for (int i = 0; i < 8; ++i)
          kt_lds[buf * DQBUF + lsw((col + i) * KB + row)] = kreg[pi].v[i];
      }
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

    // S^T = K Q^T and dP^T = V dO^T: the swapped operands make the
    // C-layout hold ONE q row per lane (col = fr) with 16 keys in regs
    f32x4 s_acc[KB / 16], dp_acc[KB / 16];
    #pragma unroll
    for (int j = 0; j < KB / 16; ++j) {
      s_acc[j] = {0.f, 0.f, 0.f, 0.f};
      dp_acc[j] = {0.f, 0.f, 0.f, 0.f};
      #pragma unroll
      for (int ks = 0; ks < D / 32; ++ks) {
        bf16x8v kf = *reinterpret_cast<const bf16x8v*>(
            &k_lds[bofs + isw<D, TR>((j * 16 + fr) * D + ks * 32 + fg * 8)]);
        bf16x8v vf = *reinterpret_cast<const bf16x8v*>(
            &v_lds[bofs + isw<D, TR>((j * 16 + fr) * D + ks * 32 + fg * 8)]);
        s_acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            kf, qf[ks], s_acc[j], 0, 0, 0);
        dp_acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            vf, dof[ks], dp_acc[j], 0, 0, 0);
      }
    }
    // dS = P * (dP - delta) * scale, P = exp(S*scale - lse)
    const bool need_mask = (causal && kv0 + KB - 1 > qrow)
                           || (kv0 + KB > S);
    #pragma unroll
    for (int j = 0; j < KB / 16; ++j)
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        float p = 0.f;
        int kcol = kv0 + j * 16 + 4 * fg + r;
        if (!need_mask || (!(causal && kcol > qrow) && kcol < S))
          p = __expf(s_acc[j][r] * scale - lse_r);
        s_acc[j][r] = p * (dp_acc[j][r] - dlt_r) * scale;
      }
    // dS to the A-operand layout in-register (no strip, no fences)
    bf16x8v dsf[KB / 32];
    unsigned pk[KB / 16][2];
    swp_pack(s_acc, KB / 16, pk);
    #pragma unroll
    for (int ks = 0; ks < KB / 32; ++ks)
      dsf[ks] = swp_butterfly(pk, ks, fg);
    // dq += dS @ K: B-operand from K^T — contiguous vector loads — or,
    // under TR, from the K image by transposed reads
    #pragma unroll
    for (int j = 0; j < D / 16; ++j) {
      #pragma unroll
      for (int ks = 0; ks < KB / 32; ++ks) {
        bf16x8v kcol;
        if constexpr (TR)
          kcol = tr_frag<D>(k_lds + bofs, trl, ks * 32, j * 16);
        else
          kcol = *reinterpret_cast<const bf16x8v*>(
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
    int orow = qr0 + 4 * fg + r;
    if (orow >= S) continue;
    #pragma unroll
    for (int j = 0; j < D / 16; ++j)
      dq[(long)orow * oss + j * 16 + fr] = f2bf(dq_acc[j][r]);
  }
}

// NW waves of 16 key rows each make the workgroup's key block: 8 (128 keys,
// 512 threads, two waves per SIMD in one barrier domain) or 4 (64 keys, 256
// threads, one wave per SIMD, so that a third and fourth workgroup fit a CU
// where the registers allow an odd wave per SIMD).  The q tiles stay QB
// columns wide and start at multiples of QB in both, and a 4-wave block at
// key 128 b + 64 starts at the tile the parent's waves 4..7 start at after
// their skipped one: every wave meets the same tiles in the same order.
// HT walks each staged tile as two 32-column halves (S^T and dP^T, P^T and
// the dV MFMAs, dS^T and the dK MFMAs per half) so that only half of the
// S^T/dP^T accumulators are live at once; each dv_acc[j] and dk_acc[j]
// still takes ks = 0 then ks = 1.  dk and dv are bit-identical across NW
// and HT.
template <int D, int NW> constexpr int dkv_waves_per_simd() {
  return NW == 8 ? 2 : (D == 64 ? 3 : 2);
}
template <int D, int SW, bool TR, bool RAGGED = false, bool GQA = false,
          int NW = 8, bool HT = false>
__global__ void __launch_bounds__(NW * WAVE, (dkv_waves_per_simd<D, NW>()))
flash_bwd_dkv_kernel(const bf16* __restrict__ dO, const bf16* __restrict__ Q,
                     const bf16* __restrict__ K, const bf16* __restrict__ V,
                     const float* __restrict__ LSE,
                     const float* __restrict__ DELTA, bf16* __restrict__ DK,
                     bf16* __restrict__ DV, int B, int H, int S, bool causal,
                     float scale,
                     long dsb, long dsh, long dss, long qsb, long qsh,
                     long qss, long ksb, long ksh, long kss, long vsb,
                     long vsh, long vss, long osb, long osh, long oss,
                     int map_mode, int G) {
  // NW waves x 16 key rows share each staged Q/dO tile (see dq note)
  // grid: 1-D as in dq; kv block 0 is the causal-heavy one here, so the
  // map keeps the index order (heavy_last_index = false)
  static_assert(!(RAGGED && SW), "ragged S runs the strip form only");
  static_assert(!(GQA && SW), "GQA runs the strip form only");
  static_assert(NW == 8 || NW == 4, "8 or 4 waves per workgroup");
  static_assert(!(HT && SW), "the half-tile loop is the strip form's");
  constexpr int KBLK = NW * 16;          // keys per workgroup
  constexpr int NT = NW * WAVE;          // threads per workgroup
  // ceil(S/KBLK) key blocks (S / KBLK spelled as before where it is exact)
  const int nblk = RAGGED ? (S + KBLK - 1) / KBLK : S / KBLK;
  // GQA: H is the QUERY head count, the grid and the map count K/V heads,
  // bh = b * Hkv + hkv, and osb/osh are the strides of the [.., Hkv, ..]
  // dk/dv.  The group's first query head is hkv * G, so its lse/delta
  // slab starts at (b * H + hkv * G) * S = bh * G * S; head g of the group
  // lies g * qsh (dsh, S) further on.
  const int nkh = GQA ? H / G : H;
  const AttnBlock wgm = attn_block_map(blockIdx.x, nblk, B * nkh,
                                       false, map_mode);
  const int kb0 = wgm.blk * KBLK;
  const int bh = wgm.bh;
  const int b_ = bh / nkh, h_ = bh % nkh;
  const int hq = GQA ? h_ * G : h_;
  // GQA moves these four on at a head switch: dO_ and q with the prefetch,
  // lse_h and delta_h with the tile being computed
  const bf16* dO_ = dO + b_ * dsb + hq * dsh;
  const bf16* q = Q + b_ * qsb + hq * qsh;
  const bf16* k = K + b_ * ksb + h_ * ksh;
  const bf16* v = V + b_ * vsb + h_ * vsh;
  bf16* dk = DK + b_ * osb + h_ * osh;
  bf16* dv = DV + b_ * osb + h_ * osh;
  const float* lse_h = LSE + (long)bh * (GQA ? G : 1) * S;
  const float* delta_h = DELTA + (long)bh * (GQA ? G : 1) * S;

  const int lane = threadIdx.x % WAVE;
  const int wave = threadIdx.x / WAVE;
  const int kr0 = kb0 + wave * 16;          // this wave's first key row
  const int fr = lane & 15;
  const int fg = lane >> 4;
  const TrLane trl = tr_lane<D, TR>(fr, fg);   // transposed reads (TR only)

  // DOUBLE-BUFFERED Q/dO/Q^T/dO^T tiles (see dq note); under TR Q and dO
  // only, P^T dO and dS^T Q read those images transposed
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int KVBUF = (TR ? 2 : 4) * QB * D;     // elements per buffer
  static_assert(2 * KVBUF + NW * 16 * QB == dkv_lds_elems<D, TR, NW>());
  bf16* q_lds = reinterpret_cast<bf16*>(smem);     // + buf * KVBUF
  bf16* do_lds = q_lds + QB * D;
  bf16* qt_lds = do_lds + QB * D;      // Q^T [D][QB] + lsw (TR = 0 only)
  bf16* dot_lds = qt_lds + QB * D;     // dO^T [D][QB] + lsw (TR = 0 only)
  bf16* s_lds = reinterpret_cast<bf16*>(smem) + 2 * KVBUF + wave * 16 * QB;

  bf16x8v kf[D / 32], vf[D / 32];
  #pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) {
    kf[ks] = *reinterpret_cast<const bf16x8v*>(
        &k[(long)rag_row<RAGGED>(kr0 + fr, S) * kss + ks * 32 + fg * 8]);
    vf[ks] = *reinterpret_cast<const bf16x8v*>(
        &v[(long)rag_row<RAGGED>(kr0 + fr, S) * vss + ks * 32 + fg * 8]);
  }

  f32x4 dk_acc[D / 16], dv_acc[D / 16];
  #pragma unroll
  for (int j = 0; j < D / 16; ++j) {
    dk_acc[j] = {0.f, 0.f, 0.f, 0.f};
    dv_acc[j] = {0.f, 0.f, 0.f, 0.f};
  }

  const int q_start = causal ? kb0 : 0;
  // register-staged Q/dO prefetch (see dq kernel note)
  constexpr int NV = QB * D / (NT * 8);
  stage_t<TR> qreg[NV], dreg[NV];
  auto q_load = [&](int t0) {
    #pragma unroll
    for (int pi = 0; pi < NV; ++pi) {
      const int e = threadIdx.x * 8 + pi * (NT * 8);
      // row strides: the inputs may be [B,S,H,D]-layout views
      const long row = rag_row<RAGGED>(t0 + e / D, S);
      const int col = e % D;
      qreg[pi] = *reinterpret_cast<const stage_t<TR>*>(&q[row * qss + col]);
      dreg[pi] = *reinterpret_cast<const stage_t<TR>*>(
          &dO_[row * dss + col]);
    }
  };
  auto q_store = [&](int buf) {
    #pragma unroll
    for (int pi = 0; pi < NV; ++pi) {
      const int e = threadIdx.x * 8 + pi * (NT * 8);
      *reinterpret_cast<stage_t<TR>*>(
          &q_lds[buf * KVBUF + isw<D, TR>(e)]) = qreg[pi];
      *reinterpret_cast<stage_t<TR>*>(
          &do_lds[buf * KVBUF + isw<D, TR>(e)]) = dreg[pi];
      if constexpr (!TR) {
        const int row = e / D, col = e % D;
        #pragma unroll
        for (int i = 0; i < 8; ++i) {
          qt_lds[buf * KVBUF + lsw((col + i) * QB + row)] = qreg[pi].v[i];
          dot_lds[buf * KVBUF + lsw((col + i) * QB + row)] = dreg[pi].v[i];
        }
      }
    }
  };
  q_load(q_start);
  q_store(0);
  __syncthreads();
  // GQA: one flat loop of G * n_qh iterations, head g = tt / n_qh, tile
  // th = tt % n_qh of that head (kept as a counter, no division).  The
  // buffer parity is that of tt, so it runs on across a head switch, and
  // the trip count is block-uniform: every wave reaches every barrier.
  const int n_qh = (S - q_start + QB - 1) / QB;    // tiles per query head
  const int n_qt = GQA ? G * n_qh : n_qh;
  int th = 0;
  for (int tt = 0; tt < n_qt; ++tt) {
    const int q0 = q_start + (GQA ? th : tt) * QB;
    const int bofs = (tt & 1) * KVBUF;
    // this tile's lse/delta slab; the prefetch below may belong to the
    // next head already
    const float* lse = lse_h;
    const float* delta = delta_h;
    if constexpr (GQA) {
      if (th + 1 == n_qh) {      // last tile of head g
        th = 0;
        lse_h += S;
        delta_h += S;
        q += qsh;
        dO_ += dsh;
        if (tt + 1 < n_qt) q_load(q_start);
      } else {
        ++th;
        q_load(q0 + QB);         // th + 1 < n_qh implies tt + 1 < n_qt
      }
    } else {
      if (tt + 1 < n_qt) q_load(q0 + QB);
    }
    // a wave whose keys all lie past the tile (waves 4..7 on a causal
    // block's first tile; a 4-wave block has none: q0 + QB > kr0 there)
    if (NW == 8 && causal && q0 + QB - 1 < kr0) {
      if (tt + 1 < n_qt) q_store((tt + 1) & 1);
      __syncthreads();
      continue;
    }

    if constexpr (HT) {
    // half-tile walk (strip form): per 32-column half hh the chain is
    // 2 x D/32 x 2 MFMA, exp, strip round-trip, D/16 MFMA, strip
    // round-trip, D/16 MFMA, with half the S^T/dP^T registers of the
    // full-tile walk below.  The strip keeps its 16 x QB layout; half hh
    // owns its columns 32 hh .. 32 hh + 31, so the halves never share an
    // element and no fence separates them.
    const bool need_mask = (causal && kr0 + 15 > q0) || (q0 + QB > S);
    #pragma unroll
    for (int hh = 0; hh < QB / 32; ++hh) {
      f32x4 st_acc[2], dpt_acc[2];
      #pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int j = 2 * hh + jj;
        st_acc[jj] = {0.f, 0.f, 0.f, 0.f};
        dpt_acc[jj] = {0.f, 0.f, 0.f, 0.f};
        #pragma unroll
        for (int ks = 0; ks < D / 32; ++ks) {
          bf16x8v qfb = *reinterpret_cast<const bf16x8v*>(
              &q_lds[bofs + isw<D, TR>((j * 16 + fr) * D + ks * 32 + fg * 8)]);
          bf16x8v dob = *reinterpret_cast<const bf16x8v*>(
              &do_lds[bofs + isw<D, TR>((j * 16 + fr) * D + ks * 32 + fg * 8)]);
          st_acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              kf[ks], qfb, st_acc[jj], 0, 0, 0);
          dpt_acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              vf[ks], dob, dpt_acc[jj], 0, 0, 0);
        }
      }
      // P^T into the strip for the dV mfma
      #pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int j = 2 * hh + jj;
        int qcol = q0 + j * 16 + fr;
        float l = lse[rag_row<RAGGED>(qcol, S)];
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          int krow = kr0 + 4 * fg + r;
          float p = 0.f;
          if (!need_mask || (!(causal && krow > qcol) && qcol < S))
            p = __expf(st_acc[jj][r] * scale - l);
          st_acc[jj][r] = p;
          s_lds[lsw((4 * fg + r) * QB + j * 16 + fr)] = f2bf(p);
        }
      }
      lds_fence();
      bf16x8v ptf = *reinterpret_cast<const bf16x8v*>(
          &s_lds[lsw(fr * QB + hh * 32 + fg * 8)]);
      #pragma unroll
      for (int j = 0; j < D / 16; ++j) {
        bf16x8v docol;
        if constexpr (TR)
          docol = tr_frag<D>(do_lds + bofs, trl, hh * 32, j * 16);
        else
          docol = *reinterpret_cast<const bf16x8v*>(
              &dot_lds[bofs + lsw((j * 16 + fr) * QB + hh * 32 + fg * 8)]);
        dv_acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ptf, docol,
                                                            dv_acc[j], 0, 0,
                                                            0);
      }
      // dS^T through the same strip columns for the dK mfma
      lds_fence();
      #pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int j = 2 * hh + jj;
        int qcol = q0 + j * 16 + fr;
        float dlt = delta[rag_row<RAGGED>(qcol, S)];
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          float ds = st_acc[jj][r] * (dpt_acc[jj][r] - dlt) * scale;
          s_lds[lsw((4 * fg + r) * QB + j * 16 + fr)] = f2bf(ds);
        }
      }
      lds_fence();
      bf16x8v dstf = *reinterpret_cast<const bf16x8v*>(
          &s_lds[lsw(fr * QB + hh * 32 + fg * 8)]);
      #pragma unroll
      for (int j = 0; j < D / 16; ++j) {
        bf16x8v qcolf;
        if constexpr (TR)
          qcolf = tr_frag<D>(q_lds + bofs, trl, hh * 32, j * 16);
        else
          qcolf = *reinterpret_cast<const bf16x8v*>(
              &qt_lds[bofs + lsw((j * 16 + fr) * QB + hh * 32 + fg * 8)]);
        dk_acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dstf, qcolf,
                                                            dk_acc[j], 0, 0,
                                                            0);
      }
    }
    } else {
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
            &q_lds[bofs + isw<D, TR>((j * 16 + fr) * D + ks * 32 + fg * 8)]);
        bf16x8v dob = *reinterpret_cast<const bf16x8v*>(
            &do_lds[bofs + isw<D, TR>((j * 16 + fr) * D + ks * 32 + fg * 8)]);
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
        float l = lse[rag_row<RAGGED>(qcol, S)];
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
    // dV += P^T @ dO: B-operand from dO^T — contiguous vector loads — or,
    // under TR, from the dO image by transposed reads
    #pragma unroll
    for (int j = 0; j < D / 16; ++j) {
      #pragma unroll
      for (int ks = 0; ks < QB / 32; ++ks) {
        bf16x8v docol;
        if constexpr (TR)
          docol = tr_frag<D>(do_lds + bofs, trl, ks * 32, j * 16);
        else
          docol = *reinterpret_cast<const bf16x8v*>(
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
      float dlt = delta[rag_row<RAGGED>(qcol, S)];
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
    // dK += dS^T @ Q: B-operand from Q^T — contiguous vector loads — or,
    // under TR, from the Q image by transposed reads
    #pragma unroll
    for (int j = 0; j < D / 16; ++j) {
      #pragma unroll
      for (int ks = 0; ks < QB / 32; ++ks) {
        bf16x8v qcolf;
        if constexpr (TR)
          qcolf = tr_frag<D>(q_lds + bofs, trl, ks * 32, j * 16);
        else
          qcolf = *reinterpret_cast<const bf16x8v*>(
              &qt_lds[bofs + lsw((j * 16 + fr) * QB + ks * 32 + fg * 8)]);
        dk_acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dstf[ks], qcolf,
                                                            dk_acc[j], 0, 0,
                                                            0);
      }
    }
    }   // !HT
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

// The dkv instantiation and its LDS bytes for one launch.  sw and tr are
// the A/B knobs and apply to the aligned MHA shapes only; ragged S and GQA
// run the strip form in the geometry's default TR.  The half-tile loop is
// the 4-wave geometry's strip form.
using dkv_kern_t = decltype(&flash_bwd_dkv_kernel<64, 0, false>);
struct DkvLaunch { dkv_kern_t kern; size_t lds; };
template <int D, int NW>
static DkvLaunch ed_dkv_pick(bool sw, bool tr, bool ragged, bool gqa) {
  constexpr bool HT = NW == 4;
  constexpr bool TRD = ATTN_TR_DKV(D, NW);
  constexpr size_t L0 = sizeof(bf16) * dkv_lds_elems<D, false, NW>();
  constexpr size_t L1 = sizeof(bf16) * dkv_lds_elems<D, true, NW>();
  if (gqa)
    return {ragged ? flash_bwd_dkv_kernel<D, 0, TRD, true, true, NW, HT>
                   : flash_bwd_dkv_kernel<D, 0, TRD, false, true, NW, HT>,
            TRD ? L1 : L0};
  if (ragged)
    return {flash_bwd_dkv_kernel<D, 0, TRD, true, false, NW, HT>,
            TRD ? L1 : L0};
  if (sw)
    return {tr ? flash_bwd_dkv_kernel<D, 1, true, false, false, NW, false>
               : flash_bwd_dkv_kernel<D, 1, false, false, false, NW, false>,
            tr ? L1 : L0};
  return {tr ? flash_bwd_dkv_kernel<D, 0, true, false, false, NW, HT>
             : flash_bwd_dkv_kernel<D, 0, false, false, false, NW, HT>,
          tr ? L1 : L0};
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
                      long osb, long kosb, long osh, long oss) {
  // osb: batch stride of dq ([.., H, ..]); kosb: that of dk and dv
  // ([.., Hkv, ..]); head and row strides are common to the three
  auto grad = ed_attn_arg(grad_);
  auto q = ed_attn_arg(q_), k = ed_attn_arg(k_), v = ed_attn_arg(v_);
  const int G = ed_attn_group(q, k, v, "flash_attn_bwd");
  TORCH_CHECK(grad.sizes() == q.sizes() && out.sizes() == q.sizes(),
              "flash_attn_bwd: grad and out must have q's shape");
  TORCH_CHECK(out.is_contiguous(), "flash_attn_bwd: out must be contiguous");
  const int B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3);
  TORCH_CHECK(lse.is_contiguous() && lse.numel() == (long)B * H * S,
              "flash_attn_bwd: lse must be a contiguous [B, H, S]");
  TORCH_CHECK(D == 64 || D == 128, "flash_attn_bwd: D in {64,128}");
  TORCH_CHECK(S >= 1, "flash_attn_bwd: S >= 1");
  const bool ragged = S % (2 * QB) != 0;
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
  dim3 grid = ed_attn_grid((S + 2 * QB - 1) / (2 * QB), (long)B * H,
                           "flash_attn_bwd"), block(512);
  const int map_mode = ed_attn_map_mode();
  // LDS bytes -> workgroups per 160-KiB CU, D = 64 / 128:
  //   dq  (K+V+K^T, or K+V under TR), double-buffered:
  //     TR = 0: 64 / 112 KiB -> 2 / 1;  TR = 1: 32 / 64 KiB -> 5 / 2
  //   dkv (Q+dO+Q^T+dO^T, or Q+dO under TR), double-buffered, + strips:
  //     8 waves: TR = 0: 80 / 144 KiB -> 2 / 1;  TR = 1: 48 / 80 KiB -> 3 / 2
  //     4 waves: TR = 0: 72 / 136 KiB -> 2 / 1;  TR = 1: 40 / 72 KiB -> 4 / 2
  const bool dflt = ragged || G > 1;   // default forms only
  const bool tr_q = dflt ? ATTN_TR_DQ : ed_attn_tr(ATTN_TR_DQ);
  size_t lds = sizeof(bf16) *
      (D == 64 ? (tr_q ? dq_lds_elems<64, true>() : dq_lds_elems<64, false>())
               : (tr_q ? dq_lds_elems<128, true>()
                       : dq_lds_elems<128, false>()));
  float scale = 1.f / sqrtf((float)D);
  auto qkern = (D == 64)
      ? (tr_q ? flash_bwd_dq_kernel<64, true> : flash_bwd_dq_kernel<64, false>)
      : (tr_q ? flash_bwd_dq_kernel<128, true>
              : flash_bwd_dq_kernel<128, false>);
  if (ragged)     // default forms only: see the EASYDIST_ATTN_TR note
    qkern = (D == 64) ? flash_bwd_dq_kernel<64, true, true>
                      : flash_bwd_dq_kernel<128, true, true>;
  if (G > 1)      // default forms only, as for ragged S
    qkern = (D == 64)
        ? (ragged ? flash_bwd_dq_kernel<64, true, true, true>
                  : flash_bwd_dq_kernel<64, true, false, true>)
        : (ragged ? flash_bwd_dq_kernel<128, true, true, true>
                  : flash_bwd_dq_kernel<128, true, false, true>);
  // dkv: one workgroup of nw waves per block of nw * 16 keys of a K/V head
  // (the same grid as dq when nw == 8 and Hkv == H)
  static int swkv = []() {  // dkv butterfly measured SLOWER than the
    const char* e = getenv("EASYDIST_DKV_SWAP");   // strip (2.11 vs 1.74
    return e ? atoi(e) : 0;                        // ms) — default off
  }();
  const int nw = ed_dkv_geom(D, causal, S, (long)B * (H / G)) ? 4 : 8;
  const bool tr_d = nw == 4 ? ATTN_TR_DKV(D, 4) : ATTN_TR_DKV(D, 8);
  const bool tr_kv = dflt ? tr_d : ed_attn_tr(tr_d);
  const DkvLaunch kv = (D == 64)
      ? (nw == 4 ? ed_dkv_pick<64, 4>(swkv, tr_kv, ragged, G > 1)
                 : ed_dkv_pick<64, 8>(swkv, tr_kv, ragged, G > 1))
      : (nw == 4 ? ed_dkv_pick<128, 4>(swkv, tr_kv, ragged, G > 1)
                 : ed_dkv_pick<128, 8>(swkv, tr_kv, ragged, G > 1));
  dim3 grid_kv = ed_attn_grid((S + nw * 16 - 1) / (nw * 16),
                              (long)B * (H / G), "flash_attn_bwd");
  dim3 block_kv(nw * WAVE);
  hipLaunchKernelGGL(qkern, grid, block, lds, stream,
      (const bf16*)grad.data_ptr(), (const bf16*)q.data_ptr(),
      (const bf16*)k.data_ptr(), (const bf16*)v.data_ptr(),
      lse.data_ptr<float>(), delta.data_ptr<float>(),
      dq_p, B, H, S, causal, scale,
      grad.stride(0), grad.stride(1), grad.stride(2),
      q.stride(0), q.stride(1), q.stride(2),
      k.stride(0), k.stride(1), k.stride(2),
      v.stride(0), v.stride(1), v.stride(2), osb, osh, oss, map_mode, G);
  hipLaunchKernelGGL(kv.kern, grid_kv, block_kv, kv.lds, stream,
      (const bf16*)grad.data_ptr(), (const bf16*)q.data_ptr(),
      (const bf16*)k.data_ptr(), (const bf16*)v.data_ptr(),
      lse.data_ptr<float>(), delta.data_ptr<float>(),
      dk_p, dv_p, B, H, S, causal, scale,
      grad.stride(0), grad.stride(1), grad.stride(2),
      q.stride(0), q.stride(1), q.stride(2),
      k.stride(0), k.stride(1), k.stride(2),
      v.stride(0), v.stride(1), v.stride(2), kosb, osh, oss, map_mode, G);
}

std::tuple<at::Tensor, at::Tensor, at::Tensor>
flash_attn_bwd(const at::Tensor& grad_, const at::Tensor& q_,
               const at::Tensor& k_, const at::Tensor& v_,
               const at::Tensor& out, const at::Tensor& lse, bool causal) {
  const int B = q_.size(0), H = q_.size(1), S = q_.size(2), D = q_.size(3);
  auto opts = q_.options();
  auto dq = at::empty({B, H, S, D}, opts);
  TORCH_CHECK(k_.dim() == 4, "flash_attn_bwd: k must be 4-D");
  const int Hkv = k_.size(1);          // validated by the launch code
  auto dk = at::empty({B, Hkv, S, D}, opts);
  auto dv = at::empty({B, Hkv, S, D}, opts);
  flash_attn_bwd_launch(grad_, q_, k_, v_, out, lse, causal,
                        (bf16*)dq.data_ptr(), (bf16*)dk.data_ptr(),
                        (bf16*)dv.data_ptr(),
                        (long)H * S * D, (long)Hkv * S * D, (long)S * D, D);
  return {dq, dk, dv};
}

// dq/dk/dv written straight into one [B, S, (H + 2*Hkv)*D] buffer (the
// layout the qkv-projection backward consumes; 3*H*D when Hkv == H) —
// replaces the reference-model
// transpose+clone+cat chain (three strided gathers plus a cat copy,
// ~1.2 GB of pure layout traffic per GPT layer at batch 64).
at::Tensor
flash_attn_bwd_pack(const at::Tensor& grad_, const at::Tensor& q_,
                    const at::Tensor& k_, const at::Tensor& v_,
                    const at::Tensor& out, const at::Tensor& lse,
                    bool causal) {
  const long B = q_.size(0), H = q_.size(1), S = q_.size(2), D = q_.size(3);
  TORCH_CHECK(k_.dim() == 4 && k_.size(1) >= 1,
              "flash_attn_bwd_pack: k must be 4-D");
  const long Hkv = k_.size(1);         // validated by the launch code
  const long W = (H + 2 * Hkv) * D;    // packed row width
  auto dqkv = at::empty({B, S, W}, q_.options());
  bf16* base = (bf16*)dqkv.data_ptr();
  // dq/dk/dv sections at column offsets 0, H*D, (H+Hkv)*D of the packed
  // rows; per-(b,h,s,d) element strides: osb=S*W, osh=D, oss=W
  flash_attn_bwd_launch(grad_, q_, k_, v_, out, lse, causal,
                        base, base + H * D, base + (H + Hkv) * D,
                        S * W, S * W, D, W);
  return dqkv;
}