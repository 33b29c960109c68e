// The RoPE + KV-write family: rope_cache_kernel, rope_cache_tile_kernel (rope_cache.hip),
// splitk_rope_cache_kernel (decode_fused.hip), the kQKV prologue of paged_decode_kernel
// (attention_decode.hip). Prefill, the unfused and the fused decode agree bit for bit: all
// four take the cache addresses from here, the three decode kernels the q/k norm, the cache
// writers the chunk rotation. The attention prologue writes its rope_rot loops out itself
// (profiles/rope_kv_refactor.md), so a change to rope_*8_bf16 must be repeated there.
#pragma once

#include <type_traits>

#include "hipserve/common.h"

namespace hipserve {

// ---- rotation of one 8-wide chunk for the cache writers: fp32 in, one bf16 rounding ----
// cs: a row [cos | sin], the sines `half` entries after the cosines: a position's cos_sin
// row (half = D/2), or the chunk's own values kept in registers across heads (i0 = 0).
// rotate-half (mode 0): x = elements [i0, i0 + 8) of the head's first half, y = of its second
template <typename C>
HS_DEVICE void rope_half8_bf16(u16x8& va, u16x8& vb, const float (&x)[8], const float (&y)[8], const C cs, int i0,
                               int half) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float c = cs[i0 + j], s = cs[half + i0 + j];
    float ra, rb;
    rope_rot(x[j], y[j], c, s, ra, rb);
    va[j] = f32_to_bf16(ra);
    vb[j] = f32_to_bf16(rb);
  }
}
// interleaved (mode 1): x = the pairs [p0, p0 + 4) as (2p, 2p + 1)
template <typename C>
HS_DEVICE void rope_pairs8_bf16(u16x8& v, const float (&x)[8], const C cs, int p0, int half) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float c = cs[p0 + p], s = cs[half + p0 + p];
    float ra, rb;
    rope_rot(x[2 * p], x[2 * p + 1], c, s, ra, rb);
    v[2 * p] = f32_to_bf16(ra);
    v[2 * p + 1] = f32_to_bf16(rb);
  }
}
HS_DEVICE void bf16_unpack8(float (&x)[8], const u16x8 v) {
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = bf16_to_f32(v[j]);
}

// ---- a token's place in the paged cache (layouts: rope_cache.hip) ----
struct KvSlot {
  long blk;
  int off, block_size;
  template <typename KV>  // the token's K row of kv head kh: D contiguous elements
  HS_DEVICE KV* k_row(KV* k_cache, int nkv, int kh, int D) const {
    return k_cache + ((blk * nkv + kh) * block_size + off) * (long)D;
  }
  template <typename KV>  // element d of its V^T column: the next one is block_size on
  HS_DEVICE KV* v_col(KV* v_cache, int nkv, int kh, int D, int d = 0) const {
    return v_cache + (blk * nkv + kh) * (long)D * block_size + (long)d * block_size + off;
  }
  // elements [d0, d0 + 8) of that column, from bf16 or from fp32 rounded here
  template <typename KV>
  HS_DEVICE void store_v8(KV* v_cache, int nkv, int kh, int D, int d0, const u16x8 v) const {
    KV* vc = v_col(v_cache, nkv, kh, D);
#pragma unroll
    for (int j = 0; j < 8; ++j) kv_store1(vc + (d0 + j) * block_size, v[j]);
  }
  template <typename KV>
  HS_DEVICE void store_v8(KV* v_cache, int nkv, int kh, int D, int d0, const float (&x)[8]) const {
    KV* vc = v_col(v_cache, nkv, kh, D);
#pragma unroll
    for (int j = 0; j < 8; ++j) kv_store1(vc + (d0 + j) * block_size, f32_to_bf16(x[j]));
  }
};
// slot < 0 (padding token) decodes to block 0, offset 0 and must not be stored through
HS_DEVICE KvSlot kv_slot(long slot, int block_size) {
  return {slot >= 0 ? slot / block_size : 0, slot >= 0 ? (int)(slot % block_size) : 0, block_size};
}

// ---- per-head q/k RMSNorm in front of RoPE (Qwen3; rotate-half only) ----
// A head's sum of squares is taken in ONE order: per rotate-half chunk c (elements c * 8 + j
// and D/2 + c * 8 + j) the 8 x terms, then the 8 y terms, then x + y (sumsq16); then the
// chunks by an xor tree over c, D/32 first, 1 last. qk_rmsnorm_vec_kernel (norm.hip) fixes
// it with one chunk of 8 per lane (x + y is its first xor step). The cross-lane part stays
// with each kernel: splitk_rope_cache_kernel and the new k of paged_decode_kernel xor over
// D/16 consecutive lanes, its q prologue in-lane (c xor 4 at D = 128), then lanes 32 and 16.
HS_DEVICE float sumsq16(const float (&x)[8], const float (&y)[8]) {
  float ss = 0.f, s2 = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) ss += x[j] * x[j];
#pragma unroll
  for (int j = 0; j < 8; ++j) s2 += y[j] * y[j];
  return ss + s2;
}
// ss: the head's sum; nw: its fp32 weights [D]; d0 = c * 8. bf16 rounding after the weight
HS_DEVICE void qk_norm_apply(float (&x)[8], float (&y)[8], float ss, const float* nw, int d0, int D, float eps) {
  const float inv = rsqrtf(ss / D + eps);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    x[j] = bf16_to_f32(f32_to_bf16(x[j] * inv * nw[d0 + j]));
    y[j] = bf16_to_f32(f32_to_bf16(y[j] * inv * nw[D / 2 + d0 + j]));
  }
}

// ---- launch dispatch (as row_norm_dispatch, row_norm.h) ----
// f(KV*): a typed null of the cache element, unsigned char (e4m3) or unsigned short (bf16)
template <typename F>
void kv_dispatch(bool kv_f8, F&& f) {
  if (kv_f8) f(static_cast<unsigned char*>(nullptr));
  else f(static_cast<unsigned short*>(nullptr));
}
// f(std::integral_constant<int, m>{}): m = 0 rotate-half, 1 interleaved (any other mode)
template <typename F>
void rope_mode_dispatch(int mode, F&& f) {
  if (mode == 0) f(std::integral_constant<int, 0>{});
  else f(std::integral_constant<int, 1>{});
}

}  // namespace hipserve
