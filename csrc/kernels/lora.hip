// Multi-LoRA: every row of a batch multiplies by the low-rank pair of its own adapter.
//
//   shrink   t[m, :]  = A[idx[m]] @ x[m]                     A [slots, R, K]
//   expand   out[m, n] += scale[idx[m]] * t[m, off_j : off_j + r] . B[idx[m], n, :]   B [slots, N, r]
//
// Both kernels work on 16-row tiles with the adapter weights as the MFMA's row operand and
// the activations as its column operand, so a lane's accumulators all belong to ONE batch
// row (column = lane & 15). The adapter of a tile is wave-uniform: the wave takes the
// distinct adapters among its 16 rows one by one (ballot + readlane), addresses A / B from a
// scalar base, and a lane keeps a product only if the adapter is its row's own. A row
// without an adapter (idx < 0) keeps nothing and is never written by the expand.
//
// The shrink splits K over the grid (a decode step has at most 4 tiles) and over the 4
// waves of a workgroup; the waves' sums meet in LDS in wave order, the K slices' fp32
// partials in a second stage in slice order, and t is rounded to bf16 once: no float
// atomics, the same bits every run.
#include "hipserve/common.h"
#include "hipserve/kernels.h"

namespace hipserve {

namespace {

typedef short i16x4 __attribute__((ext_vector_type(4)));
constexpr int kShrinkWaves = 4;

// The adapter of this lane's row: idx[m] if the row exists and names a resident slot, else -1.
HS_DEVICE int row_adapter(const int* __restrict__ idx, int m, int M, int slots) {
  const int a = m < M ? idx[m] : -1;
  return (unsigned)a < (unsigned)slots ? a : -1;
}

// Pops the adapter of the first row still in `todo` (wave-uniform, in an SGPR) and clears
// all of its rows.
HS_DEVICE int next_adapter(unsigned long long& todo, int mine) {
  const int lead = __builtin_ctzll(todo);
  const int a = __builtin_amdgcn_readlane(mine, lead);
  todo &= ~__ballot(mine == a);
  return a;
}

// ---- shrink
// grid (splits, tiles), 4 waves. The workgroup owns K slice blockIdx.x in 64-column units,
// wave w the w-th quarter of it. Per 256-column chunk the wave loads its x fragment once
// (8 x 16 bytes a lane: lane group g holds columns 64g + 8s of the chunk, the same
// permutation of k on both MFMA operands), then for every distinct adapter and every
// 16-row tile of R streams the A fragment from a scalar base and adds the product into the
// lanes whose row owns that adapter.
template <int RT>
__global__ __launch_bounds__(64 * kShrinkWaves) void lora_shrink_kernel(
    float* __restrict__ ws, unsigned short* __restrict__ t, const unsigned short* __restrict__ x, long x_stride,
    const unsigned short* __restrict__ A, const int* __restrict__ idx, int M, int K, int R, int slots, int splits) {
  extern __shared__ __attribute__((aligned(16))) float red[];  // [waves - 1][rtiles][64][4]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int m0 = blockIdx.y * 16;
  const int mine = row_adapter(idx, m0 + c, M, slots);
  const unsigned long long rows = __ballot(mine >= 0);
  if (rows == 0) return;  // no adapter in the tile: nothing of A is read (the second stage / expand skip these rows)
  const int rtiles = R / 16;
  const int units = K / 64;
  const int per = (units + splits - 1) / splits;
  const int u0 = blockIdx.x * per, u1 = min(units, u0 + per);
  const int wper = (max(u1 - u0, 0) + kShrinkWaves - 1) / kShrinkWaves;
  const int k0 = (u0 + wave * wper) * 64, k1 = min(u1, u0 + (wave + 1) * wper) * 64;

  f32x4 sel[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) sel[r] = f32x4{0.f, 0.f, 0.f, 0.f};
  const unsigned short* xr = x + (long)min(m0 + c, M - 1) * x_stride;
  const long lane_a = (long)c * K;  // row c of an R tile

  int kk = k0;
  for (; kk + 256 <= k1; kk += 256) {
    u16x8 xf[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) xf[s] = *reinterpret_cast<const u16x8*>(xr + kk + 64 * g + 8 * s);
    unsigned long long todo = rows;
    while (todo) {
      const int a = next_adapter(todo, mine);
      const unsigned short* Aa = A + (long)a * R * K + kk + 64 * g;
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        if (r < rtiles) {
          u16x8 af[8];
#pragma unroll
          for (int s = 0; s < 8; ++s) af[s] = *reinterpret_cast<const u16x8*>(Aa + (long)r * 16 * K + lane_a + 8 * s);
          f32x4 acc{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < 8; ++s)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[s]),
                                                          __builtin_bit_cast(bf16x8, xf[s]), acc, 0, 0, 0);
          if (mine == a) sel[r] += acc;
        }
      }
    }
  }
  for (; kk < k1; kk += 64) {  // the slice's ragged end, 64 columns at a time (lane group g: columns 16g + 8s)
    u16x8 xf[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) xf[s] = *reinterpret_cast<const u16x8*>(xr + kk + 16 * g + 8 * s);
    unsigned long long todo = rows;
    while (todo) {
      const int a = next_adapter(todo, mine);
      const unsigned short* Aa = A + (long)a * R * K + kk + 16 * g;
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        if (r < rtiles) {
          u16x8 af[2];
#pragma unroll
          for (int s = 0; s < 2; ++s) af[s] = *reinterpret_cast<const u16x8*>(Aa + (long)r * 16 * K + lane_a + 8 * s);
          f32x4 acc{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < 2; ++s)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[s]),
                                                          __builtin_bit_cast(bf16x8, xf[s]), acc, 0, 0, 0);
          if (mine == a) sel[r] += acc;
        }
      }
    }
  }

  // waves 1..3 -> LDS; wave 0 adds them in wave order
  if (wave != 0) {
#pragma unroll
    for (int r = 0; r < RT; ++r)
      if (r < rtiles) *reinterpret_cast<f32x4*>(red + (((wave - 1) * rtiles + r) * 64 + lane) * 4) = sel[r];
  }
  __syncthreads();
  if (wave != 0) return;
  const int m = m0 + c;
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    if (r < rtiles) {
      f32x4 v = sel[r];
      for (int w = 0; w < kShrinkWaves - 1; ++w) v += *reinterpret_cast<const f32x4*>(red + ((w * rtiles + r) * 64 + lane) * 4);
      if (m >= M) continue;
      // C: column = row m of the batch (lane & 15), rows = t columns 16r + 4g + j
      const long o = (long)m * R + 16 * r + 4 * g;
      if (splits > 1) {
        *reinterpret_cast<f32x4*>(ws + (long)blockIdx.x * M * R + o) = v;
      } else {
        const u32x2 p{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
        *reinterpret_cast<u32x2*>(t + o) = p;
      }
    }
  }
}

// Second stage of a split shrink: t = bf16(sum of the K slices' partials in slice order).
// A row without an adapter reads nothing (its tile may have written nothing) and gets zeros.
__global__ __launch_bounds__(256) void lora_shrink_reduce_kernel(unsigned short* __restrict__ t,
                                                                 const float* __restrict__ ws,
                                                                 const int* __restrict__ idx, int M, int R,
                                                                 int slots, int splits) {
  const int i = blockIdx.x * 256 + threadIdx.x;  // 8 columns of one row
  const int per_row = R / 8;
  if (i >= M * per_row) return;
  const int m = i / per_row, r = (i % per_row) * 8;
  u32x4 o{0u, 0u, 0u, 0u};
  if (row_adapter(idx, m, M, slots) >= 0) {
    f32x4 lo, hi;
    sum_slices8(lo, hi, ws + (long)m * R + r, (long)M * R, splits);
    o = u32x4{pack_bf16x2(lo[0], lo[1]), pack_bf16x2(lo[2], lo[3]), pack_bf16x2(hi[0], hi[1]), pack_bf16x2(hi[2], hi[3])};
  }
  *reinterpret_cast<u32x4*>(t + (long)m * R + r) = o;
}

// ---- expand
// grid (N / 16 / (4 * nt), tiles), 4 waves; a wave takes `nt` 16-column tiles of the output.
// The t fragments of all (up to 3) slices are loaded once per wave: lane (c, g) holds
// columns g * r/4 .. of row c, the same split of the rank on the B side. Per output tile
// and distinct adapter: one B fragment from a scalar base, r / 32 MFMAs (r = 16: one
// 16x16x16), scaled by the adapter's scalar scale into the lanes whose row owns the
// adapter. The accumulator holds out[m, n0 + 4g .. + 4]: one 8- / 16-byte read-modify-write
// per lane, issued only by rows that have an adapter.
template <int r>
struct RankFrag {  // r / 4 bf16 of a row: one lane's share of the rank
  u16x4 v[r / 16];
};
template <int r>
HS_DEVICE RankFrag<r> load_frag(const unsigned short* p) {
  RankFrag<r> f;
#pragma unroll
  for (int s = 0; s < r / 16; ++s) f.v[s] = *reinterpret_cast<const u16x4*>(p + 4 * s);
  return f;
}
template <int r>
HS_DEVICE f32x4 frag_mfma(const RankFrag<r>& b, const RankFrag<r>& tf) {
  f32x4 acc{0.f, 0.f, 0.f, 0.f};
  if constexpr (r == 16) {
    acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(i16x4, b.v[0]),
                                                     __builtin_bit_cast(i16x4, tf.v[0]), acc, 0, 0, 0);
  } else {
#pragma unroll
    for (int s = 0; s < r / 32; ++s) {
      const u16x8 bb{b.v[2 * s][0], b.v[2 * s][1], b.v[2 * s][2], b.v[2 * s][3],
                     b.v[2 * s + 1][0], b.v[2 * s + 1][1], b.v[2 * s + 1][2], b.v[2 * s + 1][3]};
      const u16x8 tt{tf.v[2 * s][0], tf.v[2 * s][1], tf.v[2 * s][2], tf.v[2 * s][3],
                     tf.v[2 * s + 1][0], tf.v[2 * s + 1][1], tf.v[2 * s + 1][2], tf.v[2 * s + 1][3]};
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, bb), __builtin_bit_cast(bf16x8, tt),
                                                    acc, 0, 0, 0);
    }
  }
  return acc;
}

template <int r, bool F32>
__global__ __launch_bounds__(256) void lora_expand_kernel(void* __restrict__ out, long out_stride,
                                                          const unsigned short* __restrict__ t, int R,
                                                          const unsigned short* __restrict__ B,
                                                          const float* __restrict__ scale,
                                                          const int* __restrict__ idx, LoraSlices sl, int M, int N,
                                                          int slots, int nt) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int m0 = blockIdx.y * 16, m = m0 + c;
  const int mine = row_adapter(idx, m, M, slots);
  const unsigned long long rows = __ballot(mine >= 0);
  if (rows == 0) return;  // no adapter in the tile: neither B nor out is touched
  const unsigned short* tr = t + (long)min(m, M - 1) * R + g * (r / 4);
  RankFrag<r> tf[kLoraSlices];
#pragma unroll
  for (int j = 0; j < kLoraSlices; ++j)
    if (j < sl.n) tf[j] = load_frag<r>(tr + sl.t_offset[j]);
  const int ntiles = N / 16;
  const int first = (blockIdx.x * 4 + wave) * nt;
  for (int tile = first; tile < min(ntiles, first + nt); ++tile) {
    const int n0 = tile * 16;
    RankFrag<r> cur = tf[0];
#pragma unroll
    for (int j = 1; j < kLoraSlices; ++j)
      if (j < sl.n && n0 >= sl.n_begin[j]) cur = tf[j];  // slices ascend; uniform
    const long lane_b = (long)(n0 + c) * r + g * (r / 4);
    f32x4 sel{0.f, 0.f, 0.f, 0.f};
    unsigned long long todo = rows;
    while (todo) {
      const int a = next_adapter(todo, mine);
      const RankFrag<r> bf = load_frag<r>(B + (long)a * N * r + lane_b);
      const f32x4 acc = frag_mfma<r>(bf, cur);
      const float sc = scale[a];
      if (mine == a) sel = acc * sc;
    }
    if (mine < 0) continue;
    // C: column = row m (lane & 15), rows = output columns n0 + 4g + j
    if constexpr (F32) {
      f32x4* p = reinterpret_cast<f32x4*>(static_cast<float*>(out) + (long)m * out_stride + n0 + 4 * g);
      *p = *p + sel;
    } else {
      u32x2* p = reinterpret_cast<u32x2*>(static_cast<unsigned short*>(out) + (long)m * out_stride + n0 + 4 * g);
      const u16x4 o = __builtin_bit_cast(u16x4, *p);
      *p = u32x2{pack_bf16x2(bf16_to_f32(o[0]) + sel[0], bf16_to_f32(o[1]) + sel[1]),
                 pack_bf16x2(bf16_to_f32(o[2]) + sel[2], bf16_to_f32(o[3]) + sel[3])};
    }
  }
}

template <int RT>
void shrink_launch(float* ws, void* t, const void* x, long x_stride, const void* A, const int* idx, int M, int K, int R,
                   int slots, int splits, hipStream_t stream) {
  const size_t lds = (size_t)(kShrinkWaves - 1) * (R / 16) * 64 * 4 * sizeof(float);
  lora_shrink_kernel<RT><<<dim3(splits, cdiv(M, 16)), 64 * kShrinkWaves, lds, stream>>>(
      ws, static_cast<unsigned short*>(t), static_cast<const unsigned short*>(x), x_stride,
      static_cast<const unsigned short*>(A), idx, M, K, R, slots, splits);
}

template <int r>
void expand_launch(void* out, bool f32, long out_stride, const void* t, int R, const void* B, const float* scale,
                   const int* idx, const LoraSlices& sl, int M, int N, int slots, hipStream_t stream) {
  // a few tiles: one output tile a wave so a decode step spreads over the chip; a prefill
  // chunk amortises its t fragments and adapter scan over 4
  const int tiles = cdiv(M, 16), nt = tiles > 16 ? 4 : 1;
  const dim3 grid(cdiv(N / 16, 4 * nt), tiles);
  const unsigned short* tp = static_cast<const unsigned short*>(t);
  const unsigned short* Bp = static_cast<const unsigned short*>(B);
  if (f32) lora_expand_kernel<r, true><<<grid, 256, 0, stream>>>(out, out_stride, tp, R, Bp, scale, idx, sl, M, N, slots, nt);
  else lora_expand_kernel<r, false><<<grid, 256, 0, stream>>>(out, out_stride, tp, R, Bp, scale, idx, sl, M, N, slots, nt);
}

}  // namespace

int lora_shrink_splits(int M, int K) {
  // one workgroup a CU at most, 256 columns (64 a wave) a workgroup at least, and no more
  // slices than the second stage sums cheaply. A choice, not a tuned value: at decode (K 4096
  // -> 16 slices, 14336 -> 32) a wave owns 64-128 columns and runs only the 64-column steps;
  // fewer, fatter slices that reach the 256-column loop have not been timed against it
  const int tiles = cdiv(M, 16);
  return max(1, min(min(256 / tiles, K / 256), 32));
}

void launch_lora_shrink(void* t, float* ws, const void* x, long x_stride, const void* A, const int* idx, int M, int K,
                        int R, int slots, int splits, hipStream_t stream) {
  if (M <= 0) return;
  const int rt = R / 16;
  if (rt <= 1) shrink_launch<1>(ws, t, x, x_stride, A, idx, M, K, R, slots, splits, stream);
  else if (rt <= 2) shrink_launch<2>(ws, t, x, x_stride, A, idx, M, K, R, slots, splits, stream);
  else if (rt <= 4) shrink_launch<4>(ws, t, x, x_stride, A, idx, M, K, R, slots, splits, stream);
  else if (rt <= 8) shrink_launch<8>(ws, t, x, x_stride, A, idx, M, K, R, slots, splits, stream);
  else shrink_launch<12>(ws, t, x, x_stride, A, idx, M, K, R, slots, splits, stream);
  if (splits > 1)
    lora_shrink_reduce_kernel<<<cdiv(M * (R / 8), 256), 256, 0, stream>>>(static_cast<unsigned short*>(t), ws, idx, M, R,
                                                                         slots, splits);
}

void launch_lora_expand(void* out, bool out_f32, long out_stride, const void* t, int R, const void* B, int r,
                        const float* scale, const int* idx, const LoraSlices& slices, int M, int N, int slots,
                        hipStream_t stream) {
  if (M <= 0) return;
  if (r == 16) expand_launch<16>(out, out_f32, out_stride, t, R, B, scale, idx, slices, M, N, slots, stream);
  else if (r == 32) expand_launch<32>(out, out_f32, out_stride, t, R, B, scale, idx, slices, M, N, slots, stream);
  else expand_launch<64>(out, out_f32, out_stride, t, R, B, scale, idx, slices, M, N, slots, stream);
}

}  // namespace hipserve
