// MoE capacity routing (gfx950): dispatch, combine and both backwards.
//
//   moe_bins         tokens [N,C], topi/topv [N,K] -> bins [E,cap,C],
//                    gates/src/valid [E,cap]
//   moe_combine      out[t]    = sum_k gates[p(t,k)] * bins[p(t,k)]
//   moe_bins_bwd     gtokens[t] = sum_k gbins[p(t,k)], gtopv[t,k] = ggates[p]
//   moe_combine_bwd  gbins[e,s] = gout[t] * gate, ggates[e,s] = <gout[t], bins>
//
// where entry f = t*K + k of expert topi[f] sits in slot p(t,k) = e*cap + s,
// s being the number of earlier entries of the same expert (the order of a
// stable sort by expert), or in no slot when s >= cap.
//
// Memory-bound row kernels, no MFMA, no atomics, no zero-fill passes: every
// output element is written exactly once, by plain vector stores, in an
// order that does not depend on timing, so all four ops are reproducible.
//
// * Row kernels (fill, gather-reduce, combine backward) give a row of C
//   elements to one wave, four rows per 256-thread workgroup; rows are at
//   most 64 16-byte vectors (C <= 512), one per lane: 16-byte loads and
//   stores, fp32 accumulation, one rounding.  The row dot of the combine
//   backward is reduced in registers, then across the lanes by shuffles.
// * moe_bins is a stable counting sort of the N*K entries by expert in
//   chunks of 1024 entries, one entry per thread of a 16-wave workgroup:
//   count per chunk, scan over chunks, rank.  The rank inside a wave is the
//   popcount of (lanes with the same expert) & (lower lanes), the
//   same-expert mask built from ceil(log2 E) ballots; the last lane of each
//   expert posts the wave's count to LDS, where one thread per expert scans
//   the 16 waves in order.  One chunk needs one launch.  The rank kernel
//   writes src, valid and gates of the occupied slots; the fill kernel
//   copies their token rows and writes the unoccupied slots whole.
// * combine and the bins backward go through the inverse map pos[N*K]
//   (slot of each entry, -1 for none), written from (src, valid) by two
//   small kernels: valid slots hold distinct src, so no two threads write
//   one element.  A fill kernel sets the -1s where hipMemsetAsync(0xFF)
//   would do: a memset on a capturing stream becomes a memset node, and
//   graphs with memset nodes have replayed wrongly under the ROCm runtime
//   this project runs on, while kernel nodes replay reliably.  The fill
//   writes N*K ints, a fraction of a microsecond of traffic.
//
// Indices read from memory (topi, src) are checked before they address
// anything: an expert outside [0, E) is dropped, a src outside [0, N*K)
// makes its slot count as invalid.
#include "common.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

// Packed fp32 arithmetic (v_pk_*_f32) is kept out of these kernels: their
// equality with the aten formula was established for scalar fp32 code, and
// nothing here is bound by arithmetic, so the packed forms would buy nothing.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

#define MOE_BLOCK 256       // threads of a row-kernel workgroup
#define MOE_CHUNK 1024      // entries, and threads, of a sort workgroup
#define MOE_CHUNK_WAVES (MOE_CHUNK / WAVE)
#define MOE_MAX_E 256
#define MOE_MAX_K 8

DEVINL bf16x8 ld8(const bf16* p) {
  return *reinterpret_cast<const bf16x8*>(p);
}
DEVINL void st8(bf16* p, const bf16x8& v) {
  *reinterpret_cast<bf16x8*>(p) = v;
}
DEVINL bf16x8 zero8() {
  bf16x8 z;
  #pragma unroll
  for (int e = 0; e < 8; ++e) z.v[e] = f2bf(0.f);
  return z;
}

// ---------------------------------------------------------------------------
// moe_bins: counting sort by expert
// ---------------------------------------------------------------------------

// The number of earlier entries of expert e in this chunk, plus base[e] when
// base is given; -1 for a thread with no entry (ok == false).  The running
// totals after the chunk go to chunk_tot[E] when it is given.  All MOE_CHUNK
// threads must call it.
DEVINL int chunk_rank(int e, bool ok, int E, int nbits, const int* base,
                      int* chunk_tot, int* lds /* [MOE_CHUNK_WAVES * E] */) {
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  for (int i = tid; i < MOE_CHUNK_WAVES * E; i += MOE_CHUNK) lds[i] = 0;
  unsigned long long same = __builtin_amdgcn_ballot_w64(ok);
  for (int b = 0; b < nbits; ++b) {
    const bool bit = (e >> b) & 1;
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(bit);
    same &= bit ? bal : ~bal;
  }
  const int in_wave = __popcll(same & ((1ull << lane) - 1ull));
  __syncthreads();
  if (ok && in_wave == __popcll(same) - 1)   // last lane of this expert
    lds[wave * E + e] = in_wave + 1;
  __syncthreads();
  if (tid < E) {
    int run = base ? base[tid] : 0;
    #pragma unroll
    for (int w = 0; w < MOE_CHUNK_WAVES; ++w) {
      const int c = lds[w * E + tid];
      lds[w * E + tid] = run;
      run += c;
    }
    if (chunk_tot) chunk_tot[tid] = run;
  }
  __syncthreads();
  return ok ? lds[wave * E + e] + in_wave : -1;
}

// This thread's entry of chunk blockIdx.x: its expert, or ok = false for the
// tail past n and for an expert outside [0, E).
DEVINL long chunk_entry(const long* __restrict__ topi, long n, int E, int* e,
                        bool* ok) {
  const long f = (long)blockIdx.x * MOE_CHUNK + threadIdx.x;
  long ex = f < n ? topi[f] : -1;
  *ok = ex >= 0 && ex < E;
  *e = *ok ? (int)ex : 0;
  return f;
}

// (a) cnt[chunk][E]: entries of each expert in each chunk
__global__ void __launch_bounds__(MOE_CHUNK)
moe_count_kernel(const long* __restrict__ topi, long n, int E, int nbits,
                 int* __restrict__ cnt) {
  __shared__ int lds[MOE_CHUNK_WAVES * MOE_MAX_E];
  int e; bool ok;
  chunk_entry(topi, n, E, &e, &ok);
  chunk_rank(e, ok, E, nbits, nullptr, cnt + (long)blockIdx.x * E, lds);
}

// (b) base[chunk][E]: exclusive scan of cnt over the chunks; tot[E].  One
// thread per expert walks the chunks in order: one coalesced load and store
// per 1024 entries, microseconds at training sizes and about two million
// steps at the 2^31 entry limit.
__global__ void __launch_bounds__(MOE_MAX_E)
moe_scan_kernel(const int* __restrict__ cnt, int* __restrict__ base,
                int* __restrict__ tot, long chunks, int E) {
  const int e = threadIdx.x;
  if (e >= E) return;
  int run = 0;
  for (long c = 0; c < chunks; ++c) {
    base[c * E + e] = run;
    run += cnt[c * E + e];
  }
  tot[e] = run;
}

// (c) rank every entry and write src, valid, gates of the slot it takes.
// ONE: the only chunk; its totals are tot.
template <bool ONE>
__global__ void __launch_bounds__(MOE_CHUNK)
moe_rank_kernel(const long* __restrict__ topi, const bf16* __restrict__ topv,
                long n, int E, int nbits, int cap,
                const int* __restrict__ base, int* __restrict__ tot,
                long* __restrict__ src, unsigned char* __restrict__ valid,
                bf16* __restrict__ gates) {
  __shared__ int lds[MOE_CHUNK_WAVES * MOE_MAX_E];
  int e; bool ok;
  const long f = chunk_entry(topi, n, E, &e, &ok);
  const int rank = chunk_rank(e, ok, E, nbits,
                              ONE ? nullptr : base + (long)blockIdx.x * E,
                              ONE ? tot : nullptr, lds);
  if (ok && rank < cap) {
    const long r = (long)e * cap + rank;
    src[r] = f;
    valid[r] = 1;
    gates[r] = topv[f];
  }
}

// (d) one slot row per ROW_LANES threads: the token row of an occupied slot,
// zeros and the empty metadata for the others.
template <int ROW_LANES>
__global__ void __launch_bounds__(MOE_BLOCK)
moe_fill_kernel(const bf16* __restrict__ tokens, const int* __restrict__ tot,
                bf16* __restrict__ bins, long* __restrict__ src,
                unsigned char* __restrict__ valid, bf16* __restrict__ gates,
                long rows, int cap, int K, int V) {
  const long r = (long)blockIdx.x * (MOE_BLOCK / ROW_LANES)
      + threadIdx.x / ROW_LANES;
  const int lane = threadIdx.x % ROW_LANES;
  if (r >= rows) return;
  const int e = (int)(r / cap), s = (int)(r - (long)e * cap);
  bf16* out = bins + r * V * 8;
  if (s < min(tot[e], cap)) {
    const bf16* in = tokens + (src[r] / K) * V * 8;
    for (int v = lane; v < V; v += ROW_LANES) st8(out + v * 8, ld8(in + v * 8));
  } else {
    const bf16x8 z = zero8();
    for (int v = lane; v < V; v += ROW_LANES) st8(out + v * 8, z);
    if (lane == 0) {
      src[r] = 0;
      valid[r] = 0;
      gates[r] = f2bf(0.f);
    }
  }
}

// ---------------------------------------------------------------------------
// inverse map: pos[f] = the slot of entry f, -1 for none
// ---------------------------------------------------------------------------

__global__ void __launch_bounds__(MOE_BLOCK)
moe_pos_clear_kernel(int* __restrict__ pos, long n) {
  const long f = (long)blockIdx.x * MOE_BLOCK + threadIdx.x;
  if (f < n) pos[f] = -1;
}

__global__ void __launch_bounds__(MOE_BLOCK)
moe_pos_kernel(const long* __restrict__ src,
               const unsigned char* __restrict__ valid, int* __restrict__ pos,
               long rows, long n) {
  const long r = (long)blockIdx.x * MOE_BLOCK + threadIdx.x;
  if (r >= rows || !valid[r]) return;
  const long f = src[r];
  if (f >= 0 && f < n) pos[f] = (int)r;
}

// ---------------------------------------------------------------------------
// gather-reduce: one token row per ROW_LANES threads, its K slots in order
// ---------------------------------------------------------------------------

// COMBINE:  Y[t] = sum_k gates[p] * X[p]
// !COMBINE: Y[t] = sum_k X[p], and gtopv[t,k] = ggates[p] or 0
template <int ROW_LANES, bool COMBINE>
__global__ void __launch_bounds__(MOE_BLOCK)
moe_gather_kernel(const bf16* __restrict__ X, const bf16* __restrict__ gates,
                  const int* __restrict__ pos, bf16* __restrict__ Y,
                  bf16* __restrict__ gtopv, long N, int K, int V) {
  const long t = (long)blockIdx.x * (MOE_BLOCK / ROW_LANES)
      + threadIdx.x / ROW_LANES;
  const int lane = threadIdx.x % ROW_LANES;
  if (t >= N) return;
  int p[MOE_MAX_K];
  float g[MOE_MAX_K];
  #pragma unroll
  for (int k = 0; k < MOE_MAX_K; ++k) {
    p[k] = k < K ? pos[t * K + k] : -1;
    g[k] = (COMBINE && p[k] >= 0) ? bf2f(gates[p[k]]) : 1.f;
  }
  if (!COMBINE && lane < K) {
    // + 0: the sum of a zero-initialised accumulator and one term
    const int pl = pos[t * K + lane];
    gtopv[t * K + lane] = f2bf(pl >= 0 ? bf2f(gates[pl]) + 0.f : 0.f);
  }
  bf16* out = Y + t * V * 8;
  for (int v = lane; v < V; v += ROW_LANES) {
    float acc[8];
    #pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    #pragma unroll
    for (int k = 0; k < MOE_MAX_K; ++k) {
      if (p[k] < 0) continue;
      const bf16x8 x = ld8(X + ((long)p[k] * V + v) * 8);
      #pragma unroll
      for (int e = 0; e < 8; ++e)
        acc[e] += COMBINE ? g[k] * bf2f(x.v[e]) : bf2f(x.v[e]);
    }
    bf16x8 y;
    #pragma unroll
    for (int e = 0; e < 8; ++e) y.v[e] = f2bf(acc[e]);
    st8(out + v * 8, y);
  }
}

// ---------------------------------------------------------------------------
// combine backward: one slot row per ROW_LANES threads
// ---------------------------------------------------------------------------

template <int ROW_LANES>
__global__ void __launch_bounds__(MOE_BLOCK)
moe_combine_bwd_kernel(const bf16* __restrict__ gout,
                       const bf16* __restrict__ bins,
                       const bf16* __restrict__ gates,
                       const long* __restrict__ src,
                       const unsigned char* __restrict__ valid,
                       bf16* __restrict__ gbins, bf16* __restrict__ ggates,
                       long rows, long N, int K, int V) {
  const long r = (long)blockIdx.x * (MOE_BLOCK / ROW_LANES)
      + threadIdx.x / ROW_LANES;
  const int lane = threadIdx.x % ROW_LANES;
  const bool live = r < rows;   // uniform over a wave
  long t = -1;
  if (live && valid[r]) {
    t = src[r] / K;
    if (t < 0 || t >= N) t = -1;
  }
  float dot = 0.f;
  if (live) {
    bf16* out = gbins + r * V * 8;
    if (t >= 0) {
      const float gate = bf2f(gates[r]);
      const bf16* gin = gout + t * V * 8;
      const bf16* bin = bins + r * V * 8;
      for (int v = lane; v < V; v += ROW_LANES) {
        const bf16x8 g = ld8(gin + v * 8), b = ld8(bin + v * 8);
        bf16x8 y;
        #pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float ge = bf2f(g.v[e]);
          y.v[e] = f2bf(ge * gate);
          dot += ge * bf2f(b.v[e]);
        }
        st8(out + v * 8, y);
      }
    } else {
      const bf16x8 z = zero8();
      for (int v = lane; v < V; v += ROW_LANES) st8(out + v * 8, z);
    }
  }
  dot = wave_sum(dot);
  if (live && lane == 0) ggates[r] = f2bf(dot);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

static void moe_check_rows(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dtype() == at::kBFloat16 && t.is_contiguous(),
              "moe: ", name, " must be a contiguous bf16 device tensor");
  TORCH_CHECK(t.size(-1) % 8 == 0 && t.size(-1) <= 8 * WAVE
              && (uintptr_t)t.data_ptr() % 16 == 0, "moe: ", name,
              " needs C % 8 == 0, C <= 512 and 16-byte aligned data");
}

static void moe_check(const at::Tensor& t, at::ScalarType dtype,
                      at::IntArrayRef shape, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dtype() == dtype && t.is_contiguous()
              && t.sizes() == shape, "moe: ", name,
              " has the wrong device, dtype, layout or shape");
}

static void moe_check_sizes(long N, long K, long E, long cap) {
  TORCH_CHECK(E >= 1 && E <= MOE_MAX_E && K >= 1 && K <= MOE_MAX_K && N >= 1
              && cap >= 1 && N * K < (1L << 31) && E * cap < (1L << 31),
              "moe: sizes outside the kernels' envelope");
}

// a row kernel's launch: a wave per row, four rows per workgroup
#define MOE_LAUNCH_ROWS(KERNEL, TARGS, rows, V, stream, ...)                 \
  KERNEL<WAVE TARGS><<<dim3((unsigned)(((rows) + 3) / 4)), dim3(MOE_BLOCK),  \
                       0, stream>>>(__VA_ARGS__)
#define MOE_COMMA ,

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
moe_bins_fwd(const at::Tensor& tokens, const at::Tensor& topi,
             const at::Tensor& topv, int64_t n_experts, int64_t cap) {
  TORCH_CHECK(tokens.dim() == 2 && topi.dim() == 2, "moe_bins: bad ranks");
  const long N = tokens.size(0), C = tokens.size(1), K = topi.size(1);
  const long E = n_experts;
  moe_check_sizes(N, K, E, cap);
  moe_check_rows(tokens, "tokens");
  moe_check(topi, at::kLong, {N, K}, "topi");
  moe_check(topv, at::kBFloat16, {N, K}, "topv");
  const long n = N * K, rows = E * cap, chunks = (n + MOE_CHUNK - 1) / MOE_CHUNK;
  const int V = (int)(C / 8);
  int nbits = 0;
  while ((1L << nbits) < E) ++nbits;

  auto bins = at::empty({E, cap, C}, tokens.options());
  auto gates = at::empty({E, cap}, tokens.options());
  auto src = at::empty({E, cap}, tokens.options().dtype(at::kLong));
  auto valid = at::empty({E, cap}, tokens.options().dtype(at::kBool));
  // tot[E], then cnt[chunks][E] and base[chunks][E] when there are chunks
  // to scan over
  auto scratch = at::empty({E + (chunks > 1 ? 2 * chunks * E : 0)},
                           tokens.options().dtype(at::kInt));
  int* tot = scratch.data_ptr<int>();
  int* cnt = tot + E;
  int* base = cnt + chunks * E;
  const long* topi_p = (const long*)topi.data_ptr();
  const bf16* topv_p = (const bf16*)topv.data_ptr();
  long* src_p = (long*)src.data_ptr();
  unsigned char* valid_p = (unsigned char*)valid.data_ptr();
  bf16* gates_p = (bf16*)gates.data_ptr();
  auto stream = at::cuda::getCurrentCUDAStream();

  if (chunks == 1) {
    hipLaunchKernelGGL(moe_rank_kernel<true>, dim3(1), dim3(MOE_CHUNK), 0,
                       stream, topi_p, topv_p, n, (int)E, nbits, (int)cap,
                       (const int*)nullptr, tot, src_p, valid_p, gates_p);
    C10_CUDA_KERNEL_LAUNCH_CHECK();
  } else {
    hipLaunchKernelGGL(moe_count_kernel, dim3((unsigned)chunks),
                       dim3(MOE_CHUNK), 0, stream, topi_p, n, (int)E, nbits,
                       cnt);
    C10_CUDA_KERNEL_LAUNCH_CHECK();
    hipLaunchKernelGGL(moe_scan_kernel, dim3(1), dim3(MOE_MAX_E), 0, stream,
                       (const int*)cnt, base, tot, chunks, (int)E);
    C10_CUDA_KERNEL_LAUNCH_CHECK();
    hipLaunchKernelGGL(moe_rank_kernel<false>, dim3((unsigned)chunks),
                       dim3(MOE_CHUNK), 0, stream, topi_p, topv_p, n, (int)E,
                       nbits, (int)cap, (const int*)base, tot, src_p, valid_p,
                       gates_p);
    C10_CUDA_KERNEL_LAUNCH_CHECK();
  }
  MOE_LAUNCH_ROWS(moe_fill_kernel, , rows, V, stream,
                  (const bf16*)tokens.data_ptr(), (const int*)tot,
                  (bf16*)bins.data_ptr(), src_p, valid_p, gates_p, rows,
                  (int)cap, (int)K, V);
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return {bins, gates, src, valid};
}

// pos[N*K] from (src, valid)
static at::Tensor moe_inverse_map(const at::Tensor& src,
                                  const at::Tensor& valid, long n,
                                  hipStream_t stream) {
  const long rows = src.numel();
  auto pos = at::empty({n}, src.options().dtype(at::kInt));
  hipLaunchKernelGGL(moe_pos_clear_kernel,
                     dim3((unsigned)((n + MOE_BLOCK - 1) / MOE_BLOCK)),
                     dim3(MOE_BLOCK), 0, stream, pos.data_ptr<int>(), n);
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  hipLaunchKernelGGL(moe_pos_kernel,
                     dim3((unsigned)((rows + MOE_BLOCK - 1) / MOE_BLOCK)),
                     dim3(MOE_BLOCK), 0, stream,
                     (const long*)src.data_ptr(),
                     (const unsigned char*)valid.data_ptr(),
                     pos.data_ptr<int>(), rows, n);
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return pos;
}

// the [E, cap, C] rows, their [E, cap] gates and routing metadata
static void moe_check_slots(const at::Tensor& rows_t, const at::Tensor& gates,
                            const at::Tensor& src, const at::Tensor& valid,
                            const char* name) {
  TORCH_CHECK(rows_t.dim() == 3, "moe: ", name, " must be [E, cap, C]");
  moe_check_rows(rows_t, name);
  const long E = rows_t.size(0), cap = rows_t.size(1);
  moe_check(gates, at::kBFloat16, {E, cap}, "gates");
  moe_check(src, at::kLong, {E, cap}, "src");
  moe_check(valid, at::kBool, {E, cap}, "valid");
}

at::Tensor moe_combine_fwd(const at::Tensor& bins, const at::Tensor& gates,
                           const at::Tensor& src, const at::Tensor& valid,
                           int64_t n_tokens, int64_t top_k) {
  moe_check_slots(bins, gates, src, valid, "bins");
  const long N = n_tokens, K = top_k, C = bins.size(2);
  moe_check_sizes(N, K, bins.size(0), bins.size(1));
  const int V = (int)(C / 8);
  auto stream = at::cuda::getCurrentCUDAStream();
  auto pos = moe_inverse_map(src, valid, N * K, stream);
  auto out = at::empty({N, C}, bins.options());
  MOE_LAUNCH_ROWS(moe_gather_kernel, MOE_COMMA true, N, V, stream,
                  (const bf16*)bins.data_ptr(), (const bf16*)gates.data_ptr(),
                  (const int*)pos.data_ptr<int>(), (bf16*)out.data_ptr(),
                  (bf16*)nullptr, N, (int)K, V);
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return out;
}

std::tuple<at::Tensor, at::Tensor>
moe_bins_bwd(const at::Tensor& gbins, const at::Tensor& ggates,
             const at::Tensor& src, const at::Tensor& valid,
             int64_t n_tokens, int64_t top_k) {
  moe_check_slots(gbins, ggates, src, valid, "gbins");
  const long N = n_tokens, K = top_k, C = gbins.size(2);
  moe_check_sizes(N, K, gbins.size(0), gbins.size(1));
  const int V = (int)(C / 8);
  auto stream = at::cuda::getCurrentCUDAStream();
  auto pos = moe_inverse_map(src, valid, N * K, stream);
  auto gtokens = at::empty({N, C}, gbins.options());
  auto gtopv = at::empty({N, K}, gbins.options());
  MOE_LAUNCH_ROWS(moe_gather_kernel, MOE_COMMA false, N, V, stream,
                  (const bf16*)gbins.data_ptr(),
                  (const bf16*)ggates.data_ptr(),
                  (const int*)pos.data_ptr<int>(), (bf16*)gtokens.data_ptr(),
                  (bf16*)gtopv.data_ptr(), N, (int)K, V);
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return {gtokens, gtopv};
}

std::tuple<at::Tensor, at::Tensor>
moe_combine_bwd(const at::Tensor& gout, const at::Tensor& bins,
                const at::Tensor& gates, const at::Tensor& src,
                const at::Tensor& valid, int64_t top_k) {
  moe_check_slots(bins, gates, src, valid, "bins");
  TORCH_CHECK(gout.dim() == 2 && gout.size(1) == bins.size(2),
              "moe_combine_bwd: gout must be [N, C]");
  moe_check_rows(gout, "gout");
  const long N = gout.size(0), K = top_k, C = bins.size(2);
  const long rows = bins.size(0) * bins.size(1);
  moe_check_sizes(N, K, bins.size(0), bins.size(1));
  const int V = (int)(C / 8);
  auto gbins = at::empty_like(bins);
  auto ggates = at::empty_like(gates);
  auto stream = at::cuda::getCurrentCUDAStream();
  MOE_LAUNCH_ROWS(moe_combine_bwd_kernel, , rows, V, stream,
                  (const bf16*)gout.data_ptr(), (const bf16*)bins.data_ptr(),
                  (const bf16*)gates.data_ptr(), (const long*)src.data_ptr(),
                  (const unsigned char*)valid.data_ptr(),
                  (bf16*)gbins.data_ptr(), (bf16*)ggates.data_ptr(), rows, N,
                  (int)K, V);
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return {gbins, ggates};
}
