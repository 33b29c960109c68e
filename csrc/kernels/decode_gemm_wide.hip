// Wide bf16 decode GEMM for 65-256 rows (the decode buckets above 64 sequences):
//   out[M, N] = x[M, K] . W[N, K]^T      (bf16 in/out, fp32 accumulate)
// on the packed weights of pack_decode_weight (decode_gemm.hip),
// [N/128][K/256][8 row groups][8 k-slots][64 lanes][8]: no second weight copy.
//
// The weight-stationary attempt (profiles/r6_decode_gemm_wide_negative.log) lost to
// hipBLASLt because one 128 KiB workgroup per CU left half the wave cycles waiting and
// every 128-row workgroup re-read the whole 256-row x slice (2x its weight bytes). Here
// the weights stream HBM -> VGPR exactly as in decode_gemm_kernel and only x lives in LDS:
//  * a workgroup is 8 waves and owns NW = 128 * RT weight rows, XR = 16 * MT x rows
//    (MT 8 / 16) and one K slice of NH 128-k half-steps (4 of a packed piece's 8
//    k-slots), fully unrolled. The (NW, MH) family keeps x bytes <= weight bytes per
//    workgroup: M <= 128 runs (128, 1) or (256, 1) at MT 8; M > 128 runs (256, 1) at
//    MT 16, or MH = 2 M-halves of 128 rows at MT 8 with NW 128 or 256. (128, 1) above
//    128 rows would read 2x its weight bytes of x and is refused;
//  * x: the [XR, 128] slice of a half-step goes global -> LDS by LDS-DMA
//    (buffer_load_dwordx4 ... lds, 1 KiB per wave instruction), never through VGPRs, into
//    a two-slot ring of XR * 256 B: 64 KiB at MT 8 (two workgroups per CU), 128 KiB at
//    MT 16 (one). Layout as qpg_kernel (gguf_mfma.hip): 4 lane-group planes of
//    [XR rows][4 k-slots of 16 B], slot (s ^ (row >> 2)) & 3, so the 16 lanes of a
//    B-fragment ds_read_b128 hit 16 distinct bank quads. Rows >= M lie past the buffer
//    range of the x descriptor: they read as zero and are never stored;
//  * the DMA is inline asm and is waited for by an explicit s_waitcnt vmcnt(n) before the
//    barrier that opens its slot (n = the weight loads issued after it). hipcc's own
//    tracking of the builtin waits for EVERY pending LDS-DMA at the next ds_read, which
//    would drain x(h + 1) before half-step h computes. hipcc does not see these loads in
//    vmcnt, so its waits for the weight ring are only ever stricter than needed. The asm
//    writes M0 itself (declared clobbered) and holds the wait state the ISA asks for
//    between that write and the DMA;
//  * weights: RT * 4 non-temporal 1 KiB loads per wave and half-step, in a VGPR ring two
//    half-steps ahead of the MFMAs (one at RT * MT = 32, where the 128 accumulators leave
//    room for two ring slots), issued after the x request of the same half-step;
//  * out^T = W . x^T on v_mfma_f32_16x16x32_bf16: a weight fragment feeds MT MFMAs, an x
//    fragment RT. At RT = 2 a wave holds row groups rg and rg + 4 of one packed tile: with
//    the glu packing those are gate rows and their up rows, so the SiLU-GLU epilogue stays
//    in registers (RT = 1 exchanges the up half through LDS like decode_gemm_kernel);
//  * MH = 2: the two workgroups sharing a weight tile get block indices 8 apart, so the
//    round-robin dispatch over 8 XCDs should put both on one XCD and serve the second read
//    of the tile from that XCD's L2. This placement is a supposition until a bench or a
//    counter run shows it (see profiles/decode_gemm_wide_bench.log).
// Output forms and memory contracts are those of launch_decode_gemm: bf16 out (S = 1
// direct, S > 1 through splitk_reduce), fp32 partials ws[S, M, N] (DG_PARTIAL; slice s =
// the sum over K slice s only), GLU (S = 1 epilogue, S > 1 splitk_reduce_glu; gate and up
// are rounded to bf16 before the SiLU in both).
#include "hipserve/common.h"
#include "hipserve/kernels.h"

namespace hipserve {

typedef int i32x4 __attribute__((ext_vector_type(4)));

template <int RT, int MT, int NH, bool kGlu>
__global__ __launch_bounds__(512) void decode_gemm_wide_kernel(
    unsigned short* __restrict__ out, long out_stride, float* __restrict__ ws,
    const unsigned short* __restrict__ x, int x_stride, const unsigned short* __restrict__ w, int M, int N, int K,
    int tiles, int units, int mh) {
  constexpr int XR = 16 * MT;        // x rows of this workgroup
  constexpr int PLANE = XR * 64;     // bytes of one lane-group plane of a ring slot
  constexpr int SLOT = 4 * PLANE;    // one half-step of x: XR rows x 256 B
  constexpr int NDMA = XR / 32;      // 1 KiB DMA instructions per wave and half-step
  constexpr int WD = RT * MT >= 32 ? 2 : 3;  // weight ring slots (WD - 1 half-steps ahead)
  constexpr int WL = RT * 4;         // weight loads per wave and half-step
  __shared__ __attribute__((aligned(1024))) unsigned char xs[2 * SLOT];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  // MH = 2: blocks b and b + 8 are the two M-halves of one (slice, tile) unit
  int unit = blockIdx.x, half = 0;
  if (mh == 2) {
    half = (unit >> 3) & 1;
    unit = ((unit >> 4) << 3) | (unit & 7);
  }
  if (unit >= units) return;  // padding of the last group of 8 (whole workgroup, before any barrier)
  const int split = unit / tiles, tile = unit - split * tiles;  // slice-major, as decode_gemm_kernel
  const int mrow0 = half * XR;
  const int hs0 = split * NH;  // first 128-k half-step of the K slice

  // weights: packed tile, row groups and the lane's 16 bytes of every 1 KiB piece
  const int ptiles = (N + 127) >> 7;
  const int ptile = RT == 1 ? tile : 2 * tile + (wave >> 2);
  int rg[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) rg[r] = RT == 1 ? wave : (wave & 3) + 4 * r;
  // an odd tile count leaves the second packed tile of the last NW = 256 workgroup past
  // the weight: it re-reads the last tile and stores nothing (n >= N)
  const unsigned short* wt = w + (long)min(ptile, ptiles - 1) * (K >> 8) * 32768 + lane * 8;
  u16x8 ring[WD][RT][4];
  auto load_w = [&](int slot, int h) {
    const int H = hs0 + h;  // k-step H >> 1, k-slots 4 (H & 1) .. + 3
    const unsigned short* wp = wt + (long)(H >> 1) * 32768 + (H & 1) * 2048;
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
      for (int s = 0; s < 4; ++s)
        ring[slot][r][s] =
            __builtin_nontemporal_load(reinterpret_cast<const u16x8*>(wp + rg[r] * 4096 + 512 * s));
  };

  // x: raw buffer over rows [0, M) so that a row >= M in the (range-checked) lane offset
  // reads as zero; wave -> plane wave & 3, rows 16 j .. 16 j + 15 per instruction
  const unsigned long xa = reinterpret_cast<unsigned long>(x);
  const i32x4 xrs = i32x4{(int)(unsigned)xa, (int)((xa >> 32) & 0xffff),
                          (int)((((long)M - 1) * x_stride + K) * 2), 0x00020000};
  const int xf = (lane & 3) ^ ((lane >> 4) & 3);  // k-slot held by this lane's 16 bytes
  const int j0 = (wave >> 2) * NDMA;
  const int xvo = ((mrow0 + 16 * j0 + (lane >> 2)) * x_stride + 32 * xf + 8 * (wave & 3)) * 2;
  const int xvstep = 16 * x_stride * 2;
  const unsigned xl0 = (unsigned)(unsigned long)(__attribute__((address_space(3))) unsigned char*)xs +
                       (wave & 3) * PLANE + j0 * 1024;
  auto dma_x = [&](int h) {
    const unsigned dst = xl0 + (h & 1) * SLOT;
    const int so = (hs0 + h) * 256;
#pragma unroll
    for (int j = 0; j < NDMA; ++j) {
      // M0 (the DMA's LDS base) is reserved, so the asm leaves it as it found it. s_nop: an
      // SALU write of M0 needs one wait state before an LDS-DMA reads it, and the hazard
      // recogniser does not look inside inline asm
      unsigned m0_saved;
      asm volatile(
          "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\t"
          "buffer_load_dwordx4 %2, %3, %4 offen lds\n\ts_mov_b32 m0, %0"
          : "=&s"(m0_saved)
          : "s"(dst + j * 1024), "v"(xvo + j * xvstep), "s"(xrs), "s"(so)
          : "memory");
    }
  };

  f32x4 acc[RT][MT];
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[r][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // prologue: x(0), then W(0) .. W(WD - 2)
  dma_x(0);
#pragma unroll
  for (int i = 0; i < WD - 1; ++i)
    if (i < NH) load_w(i, i);
  // Invariant of every explicit wait below: in program order exactly the counted weight
  // loads, and no other VMEM instruction, sit between the x DMA and the wait, so vmcnt(n)
  // retires the DMA (vmcnt completes loads in order). Fewer loads there would leave the DMA
  // pending into the barrier. The asm statements are volatile with a memory clobber and each
  // half-step's issue block ends in sched_barrier(0); neither binds hipcc by contract for
  // loads of a const __restrict__ weight, so the order is checked in the disassembly of all
  // 54 instantiations after any change here (profiles/decode_gemm_wide_resources.md).
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WL * (WD - 1 < NH ? WD - 1 : NH)) : "memory");
  __syncthreads();
  // B fragment (k-slot s, x tile t): plane g, row 16 t + c, slot s ^ ((c >> 2) & 3)
  const int xrd = g * PLANE + c * 64;
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    // slot (h + 1) & 1 was last read in half-step h - 1, which the barrier below ended
    if (h + 1 < NH) dma_x(h + 1);
    if (h + WD - 1 < NH) load_w((h + WD - 1) % WD, h + WD - 1);
    __builtin_amdgcn_sched_barrier(0);  // left free, hipcc sinks the weight loads to the end of the half-step
    const unsigned char* xb = xs + (h & 1) * SLOT + xrd;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const u16x8 b = *reinterpret_cast<const u16x8*>(xb + t * 1024 + ((s ^ ((c >> 2) & 3)) << 4));
#pragma unroll
        for (int r = 0; r < RT; ++r)
          acc[r][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ring[h % WD][r][s]),
                                                               __builtin_bit_cast(bf16x8, b), acc[r][t], 0, 0, 0);
      }
    }
    if (h + 1 < NH) {
      // x(h + 1) has landed once at most the WL weight loads issued after it are pending
      // (none when this half-step issued no weight load): the invariant stated at the prologue
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(h + WD - 1 < NH ? WL : 0) : "memory");
      __syncthreads();
    }
  }

  // C: column m = mrow0 + 16 t + c, rows n = 128 ptile + 16 rg + 4 g + j
  if constexpr (kGlu) {
    if (ws == nullptr) {
      const int I = N >> 1;
      if constexpr (RT == 2) {  // acc[0] = gate rows, acc[1] = their up rows
        const int col = ptile * 64 + (wave & 3) * 16 + 4 * g;
        if (col >= I) return;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          const int m = mrow0 + 16 * t + c;
          if (m >= M) continue;
          unsigned short o[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = silu_mul1(f32_to_bf16(acc[0][t][j]), f32_to_bf16(acc[1][t][j]));
          *reinterpret_cast<uint2*>(out + (long)m * out_stride + col) =
              uint2{(unsigned)o[0] | ((unsigned)o[1] << 16), (unsigned)o[2] | ((unsigned)o[3] << 16)};
        }
      } else {  // waves 0-3 hold gate row groups, 4-7 the matching up row groups
        float* ex = reinterpret_cast<float*>(xs);  // [4][16][XR] fp32 <= the x ring
        __syncthreads();                           // every wave is done reading the x ring
        if (wave >= 4) {
#pragma unroll
          for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              ex[((wave - 4) * 16 + 4 * g + j) * XR + 16 * t + c] = bf16_to_f32(f32_to_bf16(acc[0][t][j]));
        }
        __syncthreads();
        const int col = tile * 64 + wave * 16 + 4 * g;
        if (wave >= 4 || col >= I) return;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          const int m = mrow0 + 16 * t + c;
          if (m >= M) continue;
          unsigned short o[4];
#pragma unroll
          for (int j = 0; j < 4; ++j)
            o[j] = silu_mul1(f32_to_bf16(acc[0][t][j]), f32_to_bf16(ex[(wave * 16 + 4 * g + j) * XR + 16 * t + c]));
          *reinterpret_cast<uint2*>(out + (long)m * out_stride + col) =
              uint2{(unsigned)o[0] | ((unsigned)o[1] << 16), (unsigned)o[2] | ((unsigned)o[3] << 16)};
        }
      }
      return;
    }
  }
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    const int n = ptile * 128 + rg[r] * 16 + 4 * g;
    if (n >= N) continue;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const int m = mrow0 + 16 * t + c;
      if (m >= M) continue;
      if (ws == nullptr) {
        *reinterpret_cast<uint2*>(out + (long)m * out_stride + n) =
            uint2{pack_bf16x2(acc[r][t][0], acc[r][t][1]), pack_bf16x2(acc[r][t][2], acc[r][t][3])};
      } else {
        *reinterpret_cast<f32x4*>(ws + ((long)split * M + m) * N + n) = acc[r][t];
      }
    }
  }
}

template <int RT, int MT, int NH, bool kGlu>
static void dgw_launch(void* out, long out_stride, float* ws, const void* x, long x_stride, const void* w, int M,
                       int N, int K, int mh, int S, int flags, hipStream_t s) {
  const int tiles = (N + 128 * RT - 1) / (128 * RT), units = tiles * S;
  const int grid = mh == 2 ? (units + 7) / 8 * 16 : units;
  decode_gemm_wide_kernel<RT, MT, NH, kGlu><<<grid, 512, 0, s>>>(
      static_cast<unsigned short*>(out), out_stride, ws, static_cast<const unsigned short*>(x), (int)x_stride,
      static_cast<const unsigned short*>(w), M, N, K, tiles, units, mh);
  if (ws != nullptr && !(flags & DG_PARTIAL)) {
    if (kGlu) launch_splitk_reduce_glu(out, out_stride, ws, M, N, S, s);
    else launch_splitk_reduce(out, out_stride, ws, M, N, S, s);
  }
}

// the compiled half-step counts NH (K / S / 128): the one list behind the dispatch switch and
// decode_gemm_wide_steps_ok (WIDE_STEPS in ops/gemm.py builds the tuner's candidates from the same)
#define DGW_STEPS(X) X(1) X(2) X(4) X(7) X(8) X(14) X(16) X(28) X(32)

template <int RT, int MT, bool kGlu>
static bool dgw_steps(void* out, long out_stride, float* ws, const void* x, long x_stride, const void* w, int M, int N,
                      int K, int mh, int S, int flags, hipStream_t s) {
#define DGW_CASE(NH)                                                                              \
  case NH:                                                                                        \
    dgw_launch<RT, MT, NH, kGlu>(out, out_stride, ws, x, x_stride, w, M, N, K, mh, S, flags, s);  \
    return true;
  switch (K / S / 128) {
    DGW_STEPS(DGW_CASE)
    default: return false;
  }
#undef DGW_CASE
}

bool decode_gemm_wide_steps_ok(int half_steps) {
#define DGW_CASE(NH) case NH:
  switch (half_steps) {
    DGW_STEPS(DGW_CASE) return true;
    default: return false;
  }
#undef DGW_CASE
}

template <bool kGlu>
static bool dgw_dispatch(void* out, long out_stride, float* ws, const void* x, long x_stride, const void* w, int M,
                         int N, int K, int nw, int mh, int S, int flags, hipStream_t s) {
  // x rows per workgroup: all of M <= 128 or one 128-row half at MT 8, 256 rows at MT 16
  if (M <= 128 || mh == 2) {
    if (nw == 128) return dgw_steps<1, 8, kGlu>(out, out_stride, ws, x, x_stride, w, M, N, K, mh, S, flags, s);
    return dgw_steps<2, 8, kGlu>(out, out_stride, ws, x, x_stride, w, M, N, K, mh, S, flags, s);
  }
  return dgw_steps<2, 16, kGlu>(out, out_stride, ws, x, x_stride, w, M, N, K, mh, S, flags, s);
}

bool decode_gemm_wide_config_ok(int M, int nw, int mh) {
  if (M <= 64 || M > 256 || (nw != 128 && nw != 256) || (mh != 1 && mh != 2)) return false;
  if (M <= 128) return mh == 1;    // one 128-row x block: nothing to halve
  return !(nw == 128 && mh == 1);  // 256 x rows against 128 weight rows: 2x the weight bytes
}

// K / S must be 128 * one of DGW_STEPS; false for anything it cannot run.
bool launch_decode_gemm_wide(void* out, long out_stride, float* ws, const void* x, long x_stride, const void* w, int M,
                             int N, int K, int nw, int mh, int S, int flags, hipStream_t s) {
  if (!decode_gemm_wide_config_ok(M, nw, mh) || S < 1 || K % 256 || K % (128 * S) ||
      !decode_gemm_wide_steps_ok(K / S / 128))
    return false;
  // the x descriptor's byte offsets are 32-bit
  if (x_stride < K || x_stride % 8 || 256L * x_stride * 2 >= (1L << 31)) return false;
  if (ws == nullptr && S != 1) return false;
  if (flags & DG_GLU)
    return N % 128 == 0 && dgw_dispatch<true>(out, out_stride, ws, x, x_stride, w, M, N, K, nw, mh, S, flags, s);
  return dgw_dispatch<false>(out, out_stride, ws, x, x_stride, w, M, N, K, nw, mh, S, flags, s);
}

}  // namespace hipserve
