// MXFP4 W4A8 GEMM for 1-256 rows and the MXFP4 -> bf16 dequantiser.
//   ws[s, m, n] = (sum over K slice s of xq[m, k] . w[n, k]) * xs[m]
// w: OCP MXFP4 — e2m1 elements (sign, 2 exponent bits, 1 mantissa bit: +-{0, .5, 1, 1.5,
// 2, 3, 4, 6}) with one E8M0 byte e per 32 consecutive k of a row, w = e2m1 * 2^(e - 127);
// xq / xs: the per-token dynamic e4m3 activations of act_quant_fp8 (prefill_gemm.hip).
// The fp32 partials feed the fused decode epilogues or splitk_reduce, as fp8_decode.hip's.
//
// Tiled layout (ops/quant.py QuantPart.from_mxfp4): one 2,176-byte chunk per 16 rows x
// 256 k at [(n >> 4) nsb + k / 256] 2176:
//   bytes 0..2047: 16-byte piece (row c = n & 15, 32-block b = 4 h + g of the chunk) at
//     h 1024 + (16 g + c) 16 — the piece is the checkpoint's 16 bytes of that block as
//     they are: byte j holds k 2 j in the low nibble and k 2 j + 1 in the high one;
//   bytes 2048..2175: the E8M0 byte of (row c, block 4 h + g) at 2048 + (16 g + c) 2 + h.
// So lane 16 g + c of a wave reads piece h with one 16-byte load (each load instruction
// covers 1 KiB contiguous) and both of its scales with one 2-byte load (128 B contiguous).
//
// v_mfma_scale_f32_16x16x128_f8f6f4, A = fp4 (cbsz 4), B = e4m3, as measured with one-hot
// weights on an MI355X (the two operand formats do NOT share a lane -> k map):
//   A (fp4): lane 16 g + c holds row c, k = 32 g + i in nibble i (low nibble first) of the
//     first four of the eight operand VGPRs — one aligned 32-block, covered by ONE
//     hardware scale (the byte of the scale VGPR that opsel names);
//   B (e4m3): lane 16 g + c holds row c, byte j = k 16 g + j (j < 16) and k 64 + 16 g +
//     (j - 16): 16-byte chunks g and g + 4 of the tile, fp8_decode.hip's x fragment.
// So the weight side is laid out by 32-blocks while the x fragment stays two 16-byte LDS
// reads 64 bytes apart; B's scale is the unit 127.
//
// Structure (fp8_decode.hip's, re-sized for half the bytes):
//  * a workgroup = 8 waves x 16 weight rows and one K slice of NSTEPS 256-k steps, fully
//    unrolled (every vmcnt is exact);
//  * weights: per step a wave loads one chunk (2 KiB + 128 B: 2 x 16 B + 2 B per lane),
//    non-temporal, FOUR steps ahead in a 5-deep VGPR ring. One step is half of the FP8
//    kernel's bytes, so its distance of two steps would keep only 4 KiB per wave in
//    flight; four steps restore its 8 KiB at fewer registers (5 x 9 against 3 x 16
//    VGPRs; at 16 m-tiles, where 5 slots spilled, 3 slots and two steps). The K step stays 256 (one chunk, two MFMAs per m-tile per barrier, as FP8):
//    a 512-k step would double the x ring in LDS, which at 256 rows is already 136 KiB;
//  * x: the step's [16 MT, 256] e4m3 slice is staged through registers into a 2-slot LDS
//    ring shared by the 8 waves. Rows are 256 + 16 B: the 16 lanes of one read phase
//    (same g, c = 0..15) read 16 B at c * 272 + const, i.e. 16-byte slot (17 c + const)
//    mod 16 — 16 distinct slots, all 64 banks once; the fragment is two such reads.
//    (A 32-byte pad would put lanes c and c + 8 on the same banks.)
//  * the result lane holds 4 consecutive n of one m (f32x4 partial stores).
// Up to 4 parts stacked along N (q | k | v, gate | up); a wave's 16 rows lie in one part.
#include "hipserve/common.h"
#include "hipserve/kernels.h"

namespace hipserve {

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int MX_LDS_ROW = 272;   // 256 e4m3 + 16 B pad
constexpr int MX_CHUNK = 2176;    // 2048 nibble bytes + 128 scale bytes

template <int MT, int NSTEPS>
__global__ __launch_bounds__(512) void mxfp4_gemm_kernel(float* __restrict__ ws, const unsigned char* __restrict__ xq,
                                                         PgMx W, int M, int N, int K, int tiles) {
  constexpr int XR = 16 * MT;                          // staged x rows (padded M)
  constexpr int XPASS = (XR * 16 + 511) / 512;         // 16-byte x loads per thread per step
  // weight ring slots; loads run MX_RING - 1 steps ahead. 16 m-tiles (64 accumulator and 32
  // x staging VGPRs, one workgroup per CU) leave room for 3 slots only: 5 spilled
  constexpr int MX_RING = MT == 16 ? 3 : 5;
  constexpr int AHEAD = MX_RING - 1;
  __shared__ __attribute__((aligned(16))) unsigned char xs_lds[2][XR * MX_LDS_ROW];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int split = blockIdx.x / tiles, tile = blockIdx.x - split * tiles;
  const int nsb = K >> 8;
  const int sb0 = split * NSTEPS;
  const int n0 = tile * 128 + wave * 16;  // this wave's first output row
  const bool active = n0 < N;

  // the wave's part and its chunk row (idle waves of a last tile read the last 16 rows)
  const unsigned char* wb = W.p[0].q;
  int nl = min(n0, N - 16);
  {
    int col = 0;
#pragma unroll
    for (int i = 0; i < kPgMxParts; ++i) {
      if (i < W.n && nl >= col && nl < col + W.p[i].rows) {
        wb = W.p[i].q;
        nl -= col;
        col = 1 << 30;  // found: later parts do not match
      } else if (i < W.n) {
        col += W.p[i].rows;
      }
    }
  }
  const unsigned char* wrow = wb + ((long)(nl >> 4) * nsb + sb0) * MX_CHUNK;

  // x staging: thread -> (row, 16-byte piece of the 256-byte step slice)
  u32x4 xv[XPASS];
  auto load_x = [&](int st) {
#pragma unroll
    for (int p = 0; p < XPASS; ++p) {
      const int idx = p * 512 + tid;
      if (XR * 16 % 512 == 0 || idx < XR * 16) {
        const int row = idx >> 4, ch = idx & 15;
        // rows >= M are clamped (they only feed output columns that are never stored)
        xv[p] = *reinterpret_cast<const u32x4*>(xq + (long)min(row, M - 1) * K + (long)(sb0 + st) * 256 + ch * 16);
      }
    }
  };
  auto store_x = [&](int buf) {
#pragma unroll
    for (int p = 0; p < XPASS; ++p) {
      const int idx = p * 512 + tid;
      if (XR * 16 % 512 == 0 || idx < XR * 16) {
        const int row = idx >> 4, ch = idx & 15;
        *reinterpret_cast<u32x4*>(&xs_lds[buf][row * MX_LDS_ROW + ch * 16]) = xv[p];
      }
    }
  };

  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // weight ring: [slot][h] the lane's block of 128-k tile h; sring: its two E8M0 bytes
  // (byte h = tile h), the MFMA's scale VGPR with opsel = h
  u32x4 ring[MX_RING][2];
  int sring[MX_RING];
  auto load_w = [&](int slot, int st) {
    const unsigned char* ck = wrow + (long)st * MX_CHUNK;
#pragma unroll
    for (int h = 0; h < 2; ++h)
      ring[slot][h] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(ck + h * 1024 + lane * 16));
    sring[slot] = __builtin_nontemporal_load(reinterpret_cast<const unsigned short*>(ck + 2048 + lane * 2));
  };

  // prologue: x(0) -> LDS[0]; x(1) in registers; W(0) .. W(AHEAD - 1) in flight
  load_x(0);
  store_x(0);
  if (NSTEPS > 1) load_x(1);
#pragma unroll
  for (int st = 0; st < AHEAD; ++st)
    if (st < NSTEPS) load_w(st, st);
  __syncthreads();
#pragma unroll
  for (int st = 0; st < NSTEPS; ++st) {
    if (st + 1 < NSTEPS) store_x((st + 1) % 2);  // x(st+1), loaded during step st-1
    if (st + 2 < NSTEPS) load_x(st + 2);
    if (st + AHEAD < NSTEPS) load_w((st + AHEAD) % MX_RING, st + AHEAD);
    const unsigned char* xb = &xs_lds[st % 2][c * MX_LDS_ROW + g * 16];
    const int sc = sring[st % MX_RING];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const u32x4 w0 = ring[st % MX_RING][h];
      // fp4: the first four operand VGPRs hold the 32 elements, the rest are not read
      const i32x8 a = i32x8{(int)w0[0], (int)w0[1], (int)w0[2], (int)w0[3], 0, 0, 0, 0};
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const u32x4 b0 = *reinterpret_cast<const u32x4*>(xb + 16 * t * MX_LDS_ROW + h * 128);
        const u32x4 b1 = *reinterpret_cast<const u32x4*>(xb + 16 * t * MX_LDS_ROW + h * 128 + 64);
        const i32x8 b = i32x8{(int)b0[0], (int)b0[1], (int)b0[2], (int)b0[3], (int)b1[0], (int)b1[1], (int)b1[2], (int)b1[3]};
        // (a, b, c, cbsz = 4: A is fp4, blgp = 0: B is e4m3, opsel_a, scale_a, opsel_b, scale_b = 2^0)
        if (h == 0)
          acc[t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc[t], 4, 0, 0, sc, 0, 127);
        else
          acc[t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc[t], 4, 0, 1, sc, 0, 127);
      }
    }
    // pin this step's MFMAs before the barrier (see fp8_decode.hip: left free, the
    // compiler sinks them to the end of the unrolled loop and keeps every fragment live)
#pragma unroll
    for (int t = 0; t < MT; ++t) asm volatile("" : "+v"(acc[t]));
    if (st + 1 < NSTEPS) __syncthreads();
  }

  if (!active) return;
  // lane: rows n = n0 + 4 g + j (j = 0..3), column m = 16 t + c
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = 16 * t + c;
    if (m >= M) continue;
    const float sx = W.xs[m];
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = acc[t][j] * sx;
    *reinterpret_cast<f32x4*>(ws + ((long)split * M + m) * N + n0 + 4 * g) = o;
  }
}

template <int MT>
static bool mx_launch(float* ws, const unsigned char* xq, const PgMx& W, int M, int N, int K, int S, hipStream_t s) {
  const int tiles = (N + 127) / 128, steps = (K >> 8) / S;
  const dim3 grid(tiles * S);
#define MX_CASE(n)                                                                                   \
  case n:                                                                                            \
    mxfp4_gemm_kernel<MT, n><<<grid, 512, 0, s>>>(ws, xq, W, M, N, K, tiles);                        \
    return true;
  switch (steps) {
    MX_CASE(1) MX_CASE(2) MX_CASE(3) MX_CASE(4) MX_CASE(6) MX_CASE(7) MX_CASE(8) MX_CASE(12) MX_CASE(14)
    MX_CASE(16) MX_CASE(21)
    default: return false;
  }
#undef MX_CASE
}

// (K / 256) / S must be a built step count (fp8_decode.hip's set: the split tables and
// their search are shared); N and every part's rows % 16 == 0
bool launch_mxfp4_gemm(float* ws, const void* xq, const PgMx& W, int M, int N, int K, int S, hipStream_t s) {
  if (M < 1 || M > 256 || K < 256 || K % 256 || S < 1 || (K >> 8) % S || N < 16 || N % 16) return false;
  if (W.n < 1 || W.n > kPgMxParts) return false;
  int rows = 0;
  for (int i = 0; i < W.n; ++i) {
    if (W.p[i].rows < 16 || W.p[i].rows % 16) return false;
    rows += W.p[i].rows;
  }
  if (rows != N) return false;
  auto* x = static_cast<const unsigned char*>(xq);
  if (M <= 16) return mx_launch<1>(ws, x, W, M, N, K, S, s);
  if (M <= 32) return mx_launch<2>(ws, x, W, M, N, K, S, s);
  if (M <= 64) return mx_launch<4>(ws, x, W, M, N, K, S, s);
  if (M <= 128) return mx_launch<8>(ws, x, W, M, N, K, S, s);
  return mx_launch<16>(ws, x, W, M, N, K, S, s);
}

// ---- MoE experts: the same W4A8 step loop over moe_align's expert-sorted slot table.
//   glu == 0: out[split, slot, n] = (sum over K slice of xq[row(slot), k] . w_e[n, k]) * xs[row]
//   glu != 0: act[slot, i] = silu / gelu_tanh(gate * xs) * (up * xs), bf16, rows [gate_e; up_e]
// q: E experts of N x K, each the tiled chunks above ([N/16][K/256][2176], per_e bytes apart).
// Grid (128-column tiles, K slices, expert tiles of 16 MT slots): a workgroup reads its
// tile's expert once (wave-uniform; a negative id is an unused tile of the padded table) and
// streams that expert's chunks only. The x slice in LDS holds GATHERED rows: slot s of the
// tile stages row slots[s] / gather_k of xq (the token of that (token, expert) pair), or row
// s itself when gather_k == 0 (w2: its input is in slot order already). The row is resolved
// once per thread before the K loop; a padded slot (slots[s] < 0) stages row 0 and its
// output row is never stored.
// GLU form: a wave owns 16 gate rows and the 16 up rows N / 2 below them — two weight
// streams against the one x fragment, 2 MT accumulators — so the lane that holds gate
// (m, n .. n + 3) holds up (m, n .. n + 3) too and writes four bf16 with one 8-byte store.
// Its ring is 3 slots (two steps ahead on two streams: the 4 chunks per wave in flight of
// the 5-slot single stream).
template <int MT, int NSTEPS, bool GLU>
__global__ __launch_bounds__(512) void mxfp4_moe_gemm_kernel(void* __restrict__ outp, const unsigned char* __restrict__ xq,
                                                             const float* __restrict__ xs,
                                                             const unsigned char* __restrict__ q, long per_e,
                                                             const int* __restrict__ slots,
                                                             const int* __restrict__ tile_expert, int E, int gather_k,
                                                             int M, int N, int K, int cap, int gelu) {
  constexpr int XR = 16 * MT;
  constexpr int XPASS = (XR * 16 + 511) / 512;
  constexpr int NS = GLU ? 2 : 1;                      // weight streams per wave
  constexpr int MX_RING = GLU ? 3 : 5;
  constexpr int AHEAD = MX_RING - 1;
  __shared__ __attribute__((aligned(16))) unsigned char xs_lds[2][XR * MX_LDS_ROW];

  const int e = tile_expert[blockIdx.z];
  if (e < 0 || e >= E) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int split = blockIdx.y, slot0 = blockIdx.z * XR;
  const int nsb = K >> 8;
  const int sb0 = split * NSTEPS;
  const int NO = GLU ? N >> 1 : N;                     // output columns the waves divide
  const int n0 = blockIdx.x * 128 + wave * 16;
  const bool active = n0 < NO;
  // (idle waves of a last tile read the last 16 rows); stream 1 = the up rows, NO below
  const unsigned char* wrow = q + (long)e * per_e + ((long)(min(n0, NO - 16) >> 4) * nsb + sb0) * MX_CHUNK;
  const long wup = (long)(NO >> 4) * nsb * MX_CHUNK;

  // the xq row of a slot; padded slots read row 0
  auto x_row = [&](int s, int sl) { return min(gather_k > 0 ? max(sl, 0) / gather_k : s, M - 1); };

  const unsigned char* xp[XPASS];
#pragma unroll
  for (int p = 0; p < XPASS; ++p) {
    const int idx = p * 512 + tid;
    xp[p] = xq;
    if (XR * 16 % 512 == 0 || idx < XR * 16) {
      const int s = slot0 + (idx >> 4);
      xp[p] = xq + (long)x_row(s, slots[s]) * K + (long)sb0 * 256 + (idx & 15) * 16;
    }
  }
  u32x4 xv[XPASS];
  auto load_x = [&](int st) {
#pragma unroll
    for (int p = 0; p < XPASS; ++p)
      if (XR * 16 % 512 == 0 || p * 512 + tid < XR * 16) xv[p] = *reinterpret_cast<const u32x4*>(xp[p] + st * 256);
  };
  auto store_x = [&](int buf) {
#pragma unroll
    for (int p = 0; p < XPASS; ++p) {
      const int idx = p * 512 + tid;
      if (XR * 16 % 512 == 0 || idx < XR * 16)
        *reinterpret_cast<u32x4*>(&xs_lds[buf][(idx >> 4) * MX_LDS_ROW + (idx & 15) * 16]) = xv[p];
    }
  };

  f32x4 acc[NS][MT];
#pragma unroll
  for (int w = 0; w < NS; ++w)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[w][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 ring[MX_RING][NS][2];
  int sring[MX_RING][NS];
  auto load_w = [&](int slot, int st) {
#pragma unroll
    for (int w = 0; w < NS; ++w) {
      const unsigned char* ck = wrow + w * wup + (long)st * MX_CHUNK;
#pragma unroll
      for (int h = 0; h < 2; ++h)
        ring[slot][w][h] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(ck + h * 1024 + lane * 16));
      sring[slot][w] = __builtin_nontemporal_load(reinterpret_cast<const unsigned short*>(ck + 2048 + lane * 2));
    }
  };

  load_x(0);
  store_x(0);
  if (NSTEPS > 1) load_x(1);
#pragma unroll
  for (int st = 0; st < AHEAD; ++st)
    if (st < NSTEPS) load_w(st, st);
  __syncthreads();
#pragma unroll
  for (int st = 0; st < NSTEPS; ++st) {
    if (st + 1 < NSTEPS) store_x((st + 1) % 2);
    if (st + 2 < NSTEPS) load_x(st + 2);
    if (st + AHEAD < NSTEPS) load_w((st + AHEAD) % MX_RING, st + AHEAD);
    const unsigned char* xb = &xs_lds[st % 2][c * MX_LDS_ROW + g * 16];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      i32x8 a[NS];
#pragma unroll
      for (int w = 0; w < NS; ++w) {
        const u32x4 w0 = ring[st % MX_RING][w][h];
        a[w] = i32x8{(int)w0[0], (int)w0[1], (int)w0[2], (int)w0[3], 0, 0, 0, 0};
      }
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const u32x4 b0 = *reinterpret_cast<const u32x4*>(xb + 16 * t * MX_LDS_ROW + h * 128);
        const u32x4 b1 = *reinterpret_cast<const u32x4*>(xb + 16 * t * MX_LDS_ROW + h * 128 + 64);
        const i32x8 b = i32x8{(int)b0[0], (int)b0[1], (int)b0[2], (int)b0[3], (int)b1[0], (int)b1[1], (int)b1[2], (int)b1[3]};
#pragma unroll
        for (int w = 0; w < NS; ++w) {
          const int sc = sring[st % MX_RING][w];
          if (h == 0)
            acc[w][t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[w], b, acc[w][t], 4, 0, 0, sc, 0, 127);
          else
            acc[w][t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[w], b, acc[w][t], 4, 0, 1, sc, 0, 127);
        }
      }
    }
#pragma unroll
    for (int w = 0; w < NS; ++w)
#pragma unroll
      for (int t = 0; t < MT; ++t) asm volatile("" : "+v"(acc[w][t]));
    if (st + 1 < NSTEPS) __syncthreads();
  }

  if (!active) return;
  // lane: columns n = n0 + 4 g + j (j = 0..3) of slot slot0 + 16 t + c
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int s = slot0 + 16 * t + c;
    const int sl = slots[s];
    if (sl < 0) continue;
    const float sx = xs[x_row(s, sl)];
    if constexpr (GLU) {
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float gt = acc[0][t][j] * sx, up = acc[1][t][j] * sx;
        const float y = gelu ? 1.5957691216057308f * (gt + 0.044715f * gt * gt * gt) : gt;  // common.h gelu_mul1
        v[j] = gt / (1.f + __expf(-y)) * up;
      }
      *reinterpret_cast<u32x2*>(static_cast<unsigned short*>(outp) + (long)s * NO + n0 + 4 * g) =
          u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
    } else {
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = acc[0][t][j] * sx;
      *reinterpret_cast<f32x4*>(static_cast<float*>(outp) + ((long)split * cap + s) * N + n0 + 4 * g) = o;
    }
  }
}

template <int MT, bool GLU>
static bool mx_moe_launch(void* out, const unsigned char* xq, const float* xs, const unsigned char* q, long per_e,
                          const int* slots, const int* tile_expert, int tiles_cap, int E, int gather_k, int M, int N,
                          int K, int S, bool gelu, hipStream_t s) {
  const int NO = GLU ? N / 2 : N;
  const dim3 grid((NO + 127) / 128, S, tiles_cap);
#define MX_CASE(n)                                                                                               \
  case n:                                                                                                        \
    mxfp4_moe_gemm_kernel<MT, n, GLU><<<grid, 512, 0, s>>>(out, xq, xs, q, per_e, slots, tile_expert, E, gather_k, \
                                                           M, N, K, tiles_cap * 16 * MT, gelu);               \
    return true;
  switch ((K >> 8) / S) {
    MX_CASE(1) MX_CASE(2) MX_CASE(3) MX_CASE(4) MX_CASE(6) MX_CASE(7) MX_CASE(8) MX_CASE(14) MX_CASE(16)
    default: return false;
  }
#undef MX_CASE
}

// tile 16 / 32 / 64 slots; (K / 256) / S in {1, 2, 3, 4, 6, 7, 8, 14, 16}; glu 0: fp32 partials
// out [S, tiles_cap * tile, N]; 1 (SiLU) / 2 (GELU-tanh): S == 1, bf16 act [tiles_cap * tile,
// N / 2]. xq has M rows; with gather_k == 0 at least tiles_cap * tile of them.
bool launch_mxfp4_moe_gemm(void* out, const void* xq, const float* xs, int M, const void* q, int E, long per_e,
                           const int* slots, const int* tile_expert, int tiles_cap, int tile, int gather_k, int N,
                           int K, int S, int glu, hipStream_t s) {
  if (M < 1 || E < 1 || N < 16 || N % 16 || K < 256 || K % 256 || S < 1 || (K >> 8) % S || gather_k < 0) return false;
  if (tiles_cap < 1 || tiles_cap > 65535 || S > 65535 || (tile != 16 && tile != 32 && tile != 64)) return false;
  if (gather_k == 0 && M < tiles_cap * tile) return false;
  if (glu < 0 || glu > 2 || (glu && (S != 1 || (N / 2) % 16))) return false;
  if (per_e < (long)(N >> 4) * (K >> 8) * MX_CHUNK) return false;
  auto* x = static_cast<const unsigned char*>(xq);
  auto* w = static_cast<const unsigned char*>(q);
#define MX_TILE(mt)                                                                                               \
  return glu ? mx_moe_launch<mt, true>(out, x, xs, w, per_e, slots, tile_expert, tiles_cap, E, gather_k, M, N, K, S, \
                                       glu == 2, s)                                                               \
             : mx_moe_launch<mt, false>(out, x, xs, w, per_e, slots, tile_expert, tiles_cap, E, gather_k, M, N, K, S, \
                                        false, s);
  if (tile == 16) { MX_TILE(1) }
  if (tile == 32) { MX_TILE(2) }
  MX_TILE(4)
#undef MX_TILE
}

// ---- tiled chunks -> bf16 [N, K] (row stride ldo elements). Exact: an e2m1 value has one
// mantissa bit and the scale is a power of two, so the fp32 product's low 16 bits are zero.
// One thread per 16-byte piece (32 k of one row): 4 x 16-byte stores.
__global__ __launch_bounds__(256) void mxfp4_dequant_kernel(unsigned short* __restrict__ out, long ldo,
                                                            const unsigned char* __restrict__ q, int N, int K) {
  const int nsb = K >> 8;
  const long piece = (long)blockIdx.x * 256 + threadIdx.x;  // [N/16][nsb][2 h][4 g][16 c]
  if (piece >= (long)(N >> 4) * nsb * 128) return;
  const long chunk = piece >> 7;
  const int r = (int)(piece & 127), h = r >> 6, lane = r & 63, c = lane & 15, g = lane >> 4;
  const unsigned char* ck = q + chunk * MX_CHUNK;
  const u32x4 v = *reinterpret_cast<const u32x4*>(ck + h * 1024 + lane * 16);
  const unsigned e = ck[2048 + lane * 2 + h];
  // 2^(e - 127): e = 0 is the fp32 subnormal 2^-127 (255, E8M0's NaN, gives +inf * v)
  const float sc = __uint_as_float(e ? e << 23 : 0x00400000u);
  const long row = (chunk / nsb) * 16 + c;
  const long k0 = (chunk % nsb) * 256 + h * 128 + g * 32;
  unsigned short* o = out + row * ldo + k0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    u32x4 pk;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned two = 0;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const unsigned nib = (v[w] >> (8 * j + 4 * i)) & 15u, mag = nib & 7u;
        // e2m1 magnitude: 0, .5 (the one subnormal), then 2^(E - 1) (1 + m / 2) for E = mag >> 1
        const float f = mag == 0 ? 0.f : mag == 1 ? 0.5f : __uint_as_float(((mag >> 1) + 126u) << 23 | (mag & 1u) << 22);
        const unsigned bits = __float_as_uint(f * sc) | (nib & 8u) << 28;
        two |= (bits >> 16) << (16 * i);
      }
      pk[j] = two;
    }
    *reinterpret_cast<u32x4*>(o + 8 * w) = pk;
  }
}

bool launch_mxfp4_dequant(void* out, long ldo, const void* q, int N, int K, hipStream_t s) {
  if (N < 16 || N % 16 || K < 256 || K % 256 || ldo < K || ldo % 8) return false;
  const long pieces = (long)(N >> 4) * (K >> 8) * 128;
  mxfp4_dequant_kernel<<<dim3((unsigned)((pieces + 255) / 256)), 256, 0, s>>>(
      static_cast<unsigned short*>(out), ldo, static_cast<const unsigned char*>(q), N, K);
  return true;
}

}  // namespace hipserve
