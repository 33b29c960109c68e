// Split-K partial reductions fused with the op that follows them in a decode
// layer (SURVEY §3.F hot loop, K2/K3 fused into K6/K7/K9's epilogue).
//
// The decode GEMMs (decode_gemm.hip, DG_PARTIAL) leave fp32 partials
// ws[S, M, N]; instead of a reduce kernel followed by a separate elementwise
// kernel (each ~5 us at decode sizes, almost all of it launch + dependent-load
// latency, profiles/r1_bench_llama3_8b_v3_trace.md), ONE kernel sums the slices
// and applies the next op:
//   * splitk_add_rmsnorm: o_proj / down_proj -> residual add -> RMSNorm
//     (the next layer's input_layernorm, or the final norm);
//   * splitk_rope_cache:  qkv_proj -> RoPE on q, k -> q back into the qkv buffer,
//     k / v into the paged cache.
// Both round exactly where the unfused chain rounds (bf16 after the sum, bf16
// residual), so the fused and unfused decode paths are bit-identical.
#include "hipserve/kernels.h"
#include "hipserve/rope_kv.h"
#include "hipserve/row_norm.h"

namespace hipserve {

// x = bf16(x + b) for 8 bf16 bias values (torch's bf16 add of the bias vector)
HS_DEVICE void add_bias8(float (&x)[8], const unsigned short* __restrict__ b) {
  const u16x8 v = *reinterpret_cast<const u16x8*>(b);
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = bf16_to_f32(f32_to_bf16(x[j] + bf16_to_f32(v[j])));
}

template <int NT, int VPT, bool kWF32>
__global__ __launch_bounds__(NT) void splitk_add_rmsnorm_kernel(unsigned short* __restrict__ out,
                                                                 unsigned short* __restrict__ residual,
                                                                 const float* __restrict__ ws, int S,
                                                                 const void* __restrict__ weight, int M, int N,
                                                                 float eps, unsigned short* __restrict__ out16,
                                                                 unsigned char* __restrict__ out8,
                                                                 float* __restrict__ xs8) {
  __shared__ float scratch[16];
  const int row = blockIdx.x;
  const int nvec = N >> 3;
  const long slice = (long)M * N;
  // the norm weight and the residual do not depend on the reduction: issue their
  // loads first and keep them raw, so no s_waitcnt sits in front of the partials
  NormW8Raw<kWF32> wraw[VPT];
  u16x8 res[VPT];
  u16x8* rr = reinterpret_cast<u16x8*>(residual + (long)row * N);
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int idx = threadIdx.x + i * NT;
    if (idx < nvec) {
      wraw[i] = norm_w8_load<kWF32>(weight, idx);
      res[i] = rr[idx];
    }
  }
  float v[VPT][8];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int idx = threadIdx.x + i * NT;
    if (idx < nvec) {
      float h[8];
      sum8_bf16(h, ws + (long)row * N + idx * 8, slice, S);
      u16x8 r;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        r[j] = f32_to_bf16(h[j] + bf16_to_f32(res[i][j]));
        v[i][j] = bf16_to_f32(r[j]);
        ss += v[i][j] * v[i][j];
      }
      rr[idx] = r;
    }
  }
  row_norm_finish<NT, VPT>(
      v, ss, [&](float (&w)[8], int i, int) { norm_w8<kWF32>(w, wraw[i]); }, out, N, row, N, eps, out16, out8, xs8,
      scratch);
}

void launch_splitk_add_rmsnorm(void* out, void* residual, const float* ws, int S, const void* w, bool weight_f32,
                               int M, int N, float eps, hipStream_t s, void* out16, void* out8, float* xs8) {
  if (M <= 0) return;
  auto* o16 = static_cast<unsigned short*>(out16);
  auto* o8 = static_cast<unsigned char*>(out8);
  row_norm_dispatch(N, weight_f32, [&](auto nt, auto vpt, auto wf) {
    splitk_add_rmsnorm_kernel<nt(), vpt(), wf()><<<M, nt(), 0, s>>>(
        static_cast<unsigned short*>(out), static_cast<unsigned short*>(residual), ws, S, w, M, N, eps, o16, o8, xs8);
  });
}

// Sandwich-norm epilogue (Gemma-3: post-attention / post-feedforward RMSNorm on the
// projection output BEFORE the residual add): h = bf16(sum_s ws); p = bf16(RMSNorm(h)
// * w_post); residual = bf16(p + residual); out = RMSNorm(residual) * w_next — the
// unfused chain splitk_reduce -> rmsnorm -> fused_add_rmsnorm in one kernel, with each
// norm reduced in the row-norm kernels' order (same thread -> element map), so the
// result is bit-identical.
template <int NT, int VPT, bool kWF32>
__global__ __launch_bounds__(NT) void splitk_post_add_rmsnorm_kernel(unsigned short* __restrict__ out,
                                                                      unsigned short* __restrict__ residual,
                                                                      const float* __restrict__ ws, int S,
                                                                      const void* __restrict__ w_post,
                                                                      const void* __restrict__ w_next, int M, int N,
                                                                      float eps, unsigned short* __restrict__ out16,
                                                                      unsigned char* __restrict__ out8,
                                                                      float* __restrict__ xs8) {
  __shared__ float scratch[16];
  const int row = blockIdx.x;
  const int nvec = N >> 3;
  const long slice = (long)M * N;
  u16x8 res[VPT];
  u16x8* rr = reinterpret_cast<u16x8*>(residual + (long)row * N);
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int idx = threadIdx.x + i * NT;
    if (idx < nvec) res[i] = rr[idx];
  }
  float v[VPT][8];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int idx = threadIdx.x + i * NT;
    if (idx < nvec) {
      sum8_bf16(v[i], ws + (long)row * N + idx * 8, slice, S);
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += v[i][j] * v[i][j];
    }
  }
  ss = block_sum(ss, scratch);
  const float inv1 = rsqrtf(ss / N + eps);
  float ss2 = 0.f;
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int idx = threadIdx.x + i * NT;
    if (idx < nvec) {
      float w[8];
      norm_w8<kWF32>(w, w_post, idx);
      u16x8 r;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float p = bf16_to_f32(f32_to_bf16(v[i][j] * inv1 * w[j]));
        r[j] = f32_to_bf16(p + bf16_to_f32(res[i][j]));
        v[i][j] = bf16_to_f32(r[j]);
        ss2 += v[i][j] * v[i][j];
      }
      rr[idx] = r;
    }
  }
  row_norm_finish<NT, VPT>(
      v, ss2, [&](float (&w)[8], int, int idx) { norm_w8<kWF32>(w, w_next, idx); }, out, N, row, N, eps, out16, out8,
      xs8, scratch);
}

void launch_splitk_post_add_rmsnorm(void* out, void* residual, const float* ws, int S, const void* w_post,
                                    const void* w_next, bool weight_f32, int M, int N, float eps, hipStream_t s,
                                    void* out16, void* out8, float* xs8) {
  if (M <= 0) return;
  auto* o16 = static_cast<unsigned short*>(out16);
  auto* o8 = static_cast<unsigned char*>(out8);
  row_norm_dispatch(N, weight_f32, [&](auto nt, auto vpt, auto wf) {
    splitk_post_add_rmsnorm_kernel<nt(), vpt(), wf()>
        <<<M, nt(), 0, s>>>(static_cast<unsigned short*>(out), static_cast<unsigned short*>(residual), ws, S, w_post,
                            w_next, M, N, eps, o16, o8, xs8);
  });
}

// The rope_cache kernel (rope_cache.hip) reading its input from the split-K
// partials instead of a bf16 qkv row. Work item = one 8-wide chunk: (q/k head,
// chunk) pairs first, then the v chunks; 64-thread workgroups over
// (token, item block) so a 64-token decode batch spreads over ~450 workgroups
// instead of 64 (the partial reads are per-CU-bandwidth bound at one WG per token).
//
// Family extras, bit-identical to the unfused chain (GEMM -> bias add -> qk_rmsnorm ->
// rope_cache): bias (Qwen2: bf16 [N], added to the bf16-rounded sum and rounded
// again) and per-head q/k RMSNorm (Qwen3: fp32 weights [D]; a head's lanes are
// consecutive, its sum of squares is reduced in the one order rope_kv.h states).
template <int kMode, bool kNorm, typename KV>
__global__ __launch_bounds__(64) void splitk_rope_cache_kernel(
    unsigned short* __restrict__ qkv, long qkv_stride, const float* __restrict__ ws, int S,
    const long* __restrict__ positions, const long* __restrict__ slots, const float* __restrict__ cos_sin,
    KV* __restrict__ k_cache, KV* __restrict__ v_cache, int T, int nq, int nkv, int D,
    int block_size, const unsigned short* __restrict__ bias, const float* __restrict__ qw,
    const float* __restrict__ kw, float eps) {
  const int t = blockIdx.x;
  const int it = blockIdx.y * 64 + threadIdx.x;
  const int half = D / 2;
  const int qk_chunks = kMode == 0 ? half / 8 : D / 8;  // work items per q/k head
  const int n_qk = (nq + nkv) * qk_chunks;
  const int n_v = nkv * (D / 8);
  if (it >= n_qk + n_v) return;
  const long pos = positions[t];
  const long slot = slots[t];
  const int N = (nq + 2 * nkv) * D;
  const long slice = (long)T * N;
  const float* wrow = ws + (long)t * N;
  const float* cs = cos_sin + pos * D;
  unsigned short* row = qkv + t * qkv_stride;
  const KvSlot sl = kv_slot(slot, block_size);

  if (it >= n_qk) {  // V: transposed cache block (tokens contiguous per d)
    if (slot < 0) return;
    const int iv = it - n_qk, kh = iv / (D / 8), c = iv % (D / 8);
    float x[8];
    sum8_bf16(x, wrow + (nq + nkv) * D + kh * D + c * 8, slice, S);
    if (bias != nullptr) add_bias8(x, bias + (nq + nkv) * D + kh * D + c * 8);
    sl.store_v8(v_cache, nkv, kh, D, c * 8, x);
    return;
  }
  const int h = it / qk_chunks, c = it % qk_chunks;
  if (h >= nq && slot < 0) return;
  if constexpr (kMode == 0) {
    float x[8], y[8];
    sum8_bf16(x, wrow + h * D + c * 8, slice, S);
    sum8_bf16(y, wrow + h * D + half + c * 8, slice, S);
    if (bias != nullptr) {
      add_bias8(x, bias + h * D + c * 8);
      add_bias8(y, bias + h * D + half + c * 8);
    }
    if constexpr (kNorm) {
      float ss = sumsq16(x, y);
      for (int o = qk_chunks / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
      qk_norm_apply(x, y, ss, h < nq ? qw : kw, c * 8, D, eps);
    }
    u16x8 va, vb;
    rope_half8_bf16(va, vb, x, y, cs, c * 8, half);
    if (h < nq) {
      *reinterpret_cast<u16x8*>(row + h * D + c * 8) = va;
      *reinterpret_cast<u16x8*>(row + h * D + half + c * 8) = vb;
    } else {
      KV* dst = sl.k_row(k_cache, nkv, h - nq, D);
      kv_store8(dst + c * 8, va);
      kv_store8(dst + half + c * 8, vb);
    }
  } else {
    float x[8];
    sum8_bf16(x, wrow + h * D + c * 8, slice, S);
    if (bias != nullptr) add_bias8(x, bias + h * D + c * 8);
    u16x8 v;
    rope_pairs8_bf16(v, x, cs, c * 4, half);
    if (h < nq) *reinterpret_cast<u16x8*>(row + h * D + c * 8) = v;
    else kv_store8(sl.k_row(k_cache, nkv, h - nq, D) + c * 8, v);
  }
}

void launch_splitk_rope_cache(void* qkv, long qkv_stride, const float* ws, int S, const long* positions,
                              const long* slots, const float* cos_sin, void* k_cache, void* v_cache, int T, int nq,
                              int nkv, int D, int block_size, int mode, hipStream_t s, const void* bias,
                              const float* qw, const float* kw, float eps, bool kv_f8) {
  if (T <= 0) return;
  const int qk_chunks = mode == 0 ? D / 16 : D / 8;
  const int items = (nq + nkv) * qk_chunks + nkv * (D / 8);
  const dim3 grid(T, (items + 63) / 64);
  kv_dispatch(kv_f8, [&](auto* kv) {
    using KV = std::remove_pointer_t<decltype(kv)>;
    rope_mode_dispatch(mode, [&](auto m) {
      bool_dispatch(m() == 0 && qw != nullptr, [&](auto norm) {
        constexpr bool kNorm = m() == 0 && norm();  // the q/k norm is rotate-half only
        splitk_rope_cache_kernel<m(), kNorm, KV><<<grid, 64, 0, s>>>(
            static_cast<unsigned short*>(qkv), qkv_stride, ws, S, positions, slots, cos_sin,
            static_cast<KV*>(k_cache), static_cast<KV*>(v_cache), T, nq, nkv, D, block_size,
            static_cast<const unsigned short*>(bias), kNorm ? qw : nullptr, kNorm ? kw : nullptr, eps);
      });
    });
  });
}

// GLU over the split-K partials of a merged [gate | up] projection in the plain
// (non-interleaved) layout — the GGUF decode GEMM's output (gguf_mfma.hip):
// act[m, j] = act(bf16(sum_s gate)) * bf16(sum_s up), bit-identical to the reduce
// followed by silu_and_mul / gelu_and_mul. grid (M, ceil(I / 2048)), 8 per thread.
template <bool kGelu>
__global__ __launch_bounds__(256) void splitk_glu_kernel(unsigned short* __restrict__ act, long act_stride,
                                                         const float* __restrict__ ws, int S, int M, int I,
                                                         unsigned short* __restrict__ act16) {
  const int m = blockIdx.x;
  const int c = blockIdx.y * 256 + threadIdx.x;
  if (c * 8 >= I) return;
  const long N = 2L * I, slice = (long)M * N;
  float g[8], u[8];
  sum8_bf16(g, ws + m * N + c * 8, slice, S);
  sum8_bf16(u, ws + m * N + I + c * 8, slice, S);
  u16x8 gb, ub;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    gb[j] = f32_to_bf16(g[j]);
    ub[j] = f32_to_bf16(u[j]);
  }
  const u16x8 o = kGelu ? gelu_mul8(gb, ub) : silu_mul8(gb, ub);
  *reinterpret_cast<u16x8*>(act + m * act_stride + c * 8) = o;
  if (act16 != nullptr) *reinterpret_cast<u16x8*>(act16 + m * act_stride + c * 8) = f16_pairs8(o);
}

void launch_splitk_glu(void* act, long act_stride, const float* ws, int S, int M, int I, bool gelu, hipStream_t s,
                       void* act16) {
  if (M <= 0) return;
  const dim3 grid(M, (I / 8 + 255) / 256);
  auto* a = static_cast<unsigned short*>(act);
  auto* a16 = static_cast<unsigned short*>(act16);
  if (gelu) splitk_glu_kernel<true><<<grid, 256, 0, s>>>(a, act_stride, ws, S, M, I, a16);
  else splitk_glu_kernel<false><<<grid, 256, 0, s>>>(a, act_stride, ws, S, M, I, a16);
}

}  // namespace hipserve
