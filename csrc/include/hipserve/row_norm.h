// The row-norm family: rmsnorm_kernel (norm.hip), splitk_add_rmsnorm_kernel and
// splitk_post_add_rmsnorm_kernel (decode_fused.hip), moe_combine_add_rmsnorm_kernel
// (moe.hip). One NT-thread workgroup per row, lane t owns the 16-byte vectors
// t + i * NT (i < VPT) of it in registers. The fused decode layer equals the unfused
// one bit for bit because all four take their thread -> element map (the ladder) and
// everything after their own first pass (row_norm_finish) from here.
#pragma once

#include <type_traits>

#include "hipserve/common.h"

namespace hipserve {

// 512 threads from 4096 columns up (more loads in flight on the 1-row-per-CU
// decode shapes), 256 below.
HS_HOST_DEVICE int norm_threads(int hidden) { return hidden >= 4096 ? 512 : 256; }

// f(std::bool_constant<b>{}): a runtime flag as a template argument.
template <typename F>
void bool_dispatch(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

// The (NT, VPT) ladder: f(nt, vpt, wf) with integral constants for the block size, the
// vectors per lane that cover N columns, and the weight dtype, so a launcher is
//   row_norm_dispatch(N, wf32, [&](auto nt, auto vpt, auto wf) {
//     kernel<nt(), vpt(), wf()><<<rows, nt(), 0, s>>>(...); });
template <typename F>
void row_norm_dispatch(int N, bool weight_f32, F&& f) {
  const int nvec = N / 8;
  bool_dispatch(weight_f32, [&](auto wf) {
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I4 = std::integral_constant<int, 4>;
    using T256 = std::integral_constant<int, 256>;
    using T512 = std::integral_constant<int, 512>;
    if (norm_threads(N) == 256) {  // N < 4096: nvec < 512
      if (nvec <= 256) f(T256{}, I1{}, wf);
      else f(T256{}, I2{}, wf);
    } else {
      if (nvec <= 512) f(T512{}, I1{}, wf);
      else if (nvec <= 1024) f(T512{}, I2{}, wf);
      else f(T512{}, I4{}, wf);
    }
  });
}

// 8 norm weights as loaded (bf16: HF checkpoints, fp32: GGUF), and their fp32 values.
// A kernel that wants the load in flight early keeps the raw form (splitk_add_rmsnorm).
template <bool kWF32> struct NormW8Raw;
template <> struct NormW8Raw<true> { f32x4 lo, hi; };
template <> struct NormW8Raw<false> { u16x8 v; };

template <bool kWF32>
HS_DEVICE NormW8Raw<kWF32> norm_w8_load(const void* __restrict__ weight, int idx) {
  if constexpr (kWF32) {
    const f32x4* wp = reinterpret_cast<const f32x4*>(weight) + idx * 2;
    return {wp[0], wp[1]};
  } else {
    return {reinterpret_cast<const u16x8*>(weight)[idx]};
  }
}
template <bool kWF32>
HS_DEVICE void norm_w8(float (&w)[8], const NormW8Raw<kWF32>& r) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if constexpr (kWF32) w[j] = j < 4 ? r.lo[j & 3] : r.hi[j & 3];
    else w[j] = bf16_to_f32(r.v[j]);
  }
}
template <bool kWF32>
HS_DEVICE void norm_w8(float (&w)[8], const void* __restrict__ weight, int idx) {
  norm_w8<kWF32>(w, norm_w8_load<kWF32>(weight, idx));
}

// 8 bf16 values -> f16 in the quantised decode GEMM's staging pair order
// {0, 2, 1, 3, 4, 6, 5, 7} (gguf_mfma.hip kX16): bf16 -> fp32 exact, -> f16 round to
// nearest — the conversion the GEMM would otherwise run in every workgroup
HS_DEVICE u16x8 f16_pairs8(const u16x8 v) {
  constexpr int ord[8] = {0, 2, 1, 3, 4, 6, 5, 7};
  u16x8 h;
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = __builtin_bit_cast(unsigned short, static_cast<_Float16>(bf16_to_f32(v[ord[j]])));
  return h;
}

// per-token dynamic e4m3 copy of a bf16 row (e4m3_8, common.h), = act_quant_fp8 of it
template <int VPT, int NT>
HS_DEVICE void row_e4m3(const u16x8 (&ov)[VPT], int nvec, int row, int N, unsigned char* __restrict__ out8,
                        float* __restrict__ xs8, float* scratch) {
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < VPT; ++i)
    if (threadIdx.x + i * NT < nvec)
#pragma unroll
      for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(bf16_to_f32(ov[i][j])));
  __syncthreads();  // scratch was the norm's reduction buffer
  amax = block_max(amax, scratch);
  const float inv = amax > 0.f ? 448.f / amax : 1.f;
  if (threadIdx.x == 0) xs8[row] = amax > 0.f ? amax / 448.f : 1.f;
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int idx = threadIdx.x + i * NT;
    if (idx < nvec) *reinterpret_cast<uint2*>(out8 + (long)row * N + idx * 8) = e4m3_8(ov[i], inv);
  }
}

// Everything after a kernel's own first pass: v holds the row's values, ss this lane's
// sum of their squares. out[row] = bf16(v * rsqrt(mean(v^2) + eps) * w), w from
// wsrc(w, i, idx) for the lane's vector i at row position idx; then the optional copies
// of that bf16 row: out16 (f16, pair order) and out8 / xs8 (per-token e4m3).
template <int NT, int VPT, typename WSrc>
HS_DEVICE void row_norm_finish(const float (&v)[VPT][8], float ss, WSrc&& wsrc, unsigned short* __restrict__ out,
                               long out_stride, int row, int N, float eps, unsigned short* __restrict__ out16,
                               unsigned char* __restrict__ out8, float* __restrict__ xs8, float* scratch) {
  const int nvec = N >> 3;
  ss = block_sum(ss, scratch);
  const float inv = rsqrtf(ss / N + eps);
  u16x8* orow = reinterpret_cast<u16x8*>(out + row * out_stride);
  u16x8 ov[VPT];
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int idx = threadIdx.x + i * NT;
    if (idx < nvec) {
      float w[8];
      wsrc(w, i, idx);
      u16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = f32_to_bf16(v[i][j] * inv * w[j]);
      orow[idx] = o;
      ov[i] = o;
      if (out16 != nullptr) reinterpret_cast<u16x8*>(out16 + (long)row * N)[idx] = f16_pairs8(o);
    }
  }
  if (out8 != nullptr) row_e4m3<VPT, NT>(ov, nvec, row, N, out8, xs8, scratch);
}

}  // namespace hipserve
