// Prompt log-probabilities (OpenAI `echo` + `logprobs`, vLLM `prompt_logprobs`, perplexity):
// for every scored prefill row r with target token t (the NEXT prompt token)
//   out_lp[r]   = l[t] - logsumexp(l)
//   out_rank[r] = 1 + #{v : l[v] > l[t]} + #{v < t : l[v] == l[t]}   on the exact input values,
//                 so rank <= n exactly when t stands in the row's top-n at index rank - 1
//                 (not vLLM's count of >=, which gives every member of a tie run the run's end)
//   out_ids / out_top [r][0 .. nreq[r])  the n largest log-softmax entries, ordered by exact
//                 value descending then id ascending, as top_logprobs (penalties.hip) orders
//                 them; unused slots hold -1 / -inf
// A target outside [0, V) gives out_lp = -inf and out_rank = 0 and is never used as an index.
// -inf logits are legal, the target's included (out_lp = -inf, never NaN).
//
// One workgroup of 1024 threads per row. A row with nreq <= 1 is read from memory exactly
// once: l[t] comes first from one uniform load, then one pass of 16-byte non-temporal loads
// (scalar head and tail where the row is not 16-byte aligned or V is ragged) keeps per thread
//   an online (max, sum-exp) pair  — the max is the argmax's value, so it is kept once,
//   the two rank counts             — one integer: before t ties count, after t they do not,
//   the argmax with the lowest id   — which is top-1.
// Threads merge through (m, s) -> (M, sum s * exp(m - M)); the sums are kept in the log2
// domain (exp2 of an FMA on v_exp_f32). A thread that has seen only -inf holds s = 0 and never
// forms exp(-inf - -inf).
// Rows with nreq >= 2 read the row again for top_logprobs' select (radix select on the
// order-preserving 16-bit key of the bf16-rounded value, then every candidate of the selected
// bin is ordered by its exact value), so its one documented bound on exactness comes along: with
// more than 64 logits in the bf16 bin of the n-th largest, the lowest-index 64 of that bin
// are the candidates (hipserve/ops/reference.py). Their first pass uses plain loads, so the
// row stays in cache for the select. Rows with nreq == 0 and no valid target return at once.
#include "hipserve/common.h"
#include "hipserve/kernels.h"

namespace hipserve {
namespace {

constexpr int kPlpT = 1024;    // threads per row
constexpr int kPlpUnroll = 4;  // 16-byte loads in flight per thread
constexpr int kPlpCand = 64;   // candidates of the select (top_logprobs' bound)
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

HS_DEVICE float plp_ld(const unsigned short* p, long i) { return bf16_to_f32(p[i]); }
HS_DEVICE float plp_ld(const float* p, long i) { return p[i]; }

// 16 bytes of a row
template <typename T> struct Row16;
template <> struct Row16<unsigned short> {
  using V = u16x8;
  static constexpr int N = 8;
};
template <> struct Row16<float> {
  using V = f32x4;
  static constexpr int N = 4;
};
HS_DEVICE void plp_unpack(const u16x8 v, float (&x)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = bf16_to_f32(v[e]);
}
HS_DEVICE void plp_unpack(const f32x4 v, float (&x)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) x[e] = v[e];
}
template <bool kNT, typename VT>
HS_DEVICE VT plp_load16(const VT* p) {
  if constexpr (kNT) return __builtin_nontemporal_load(p);
  else return *p;
}

// per-thread state of the single pass
struct RowAcc {
  float m = -INFINITY;  // running maximum: the argmax's value and the reference of s
  float s = 0.f;        // sum of exp2((x - m) log2e) over the elements seen
  int cnt = 0;          // elements that stand before the target in the top order
  int bi = 0x7fffffff;  // lowest id that holds m
};

// N consecutive elements x of ids v0 .. v0 + N - 1 (a thread sees its ids in ascending order,
// so a strict > keeps the lowest id of equal maxima)
template <int N>
HS_DEVICE void plp_acc(RowAcc& a, const float (&x)[N], int v0, float lt, int t) {
  if (v0 + N <= t) {  // all before the target: a tie stands before it
#pragma unroll
    for (int e = 0; e < N; ++e) a.cnt += x[e] >= lt;
  } else if (v0 > t) {
#pragma unroll
    for (int e = 0; e < N; ++e) a.cnt += x[e] > lt;
  } else {  // the one group that holds the target
#pragma unroll
    for (int e = 0; e < N; ++e) a.cnt += x[e] > lt || (x[e] == lt && v0 + e < t);
  }
  float m = a.m;
#pragma unroll
  for (int e = 0; e < N; ++e) {
    if (x[e] > m) {
      m = x[e];
      a.bi = v0 + e;
    }
  }
  if (m == -INFINITY) return;  // only -inf so far: s stays 0, no exp(-inf - -inf)
  const float m2 = m * kLog2e;
  float s = a.s * __builtin_amdgcn_exp2f(__builtin_fmaf(a.m, kLog2e, -m2));  // a.m == -inf: 0 * 0
#pragma unroll
  for (int e = 0; e < N; ++e) s += __builtin_amdgcn_exp2f(__builtin_fmaf(x[e], kLog2e, -m2));
  a.m = m;
  a.s = s;
}

// the 16-byte groups of a row: kPlpUnroll loads in flight per thread, ids ascending
template <bool kNT, typename VT, int N>
HS_DEVICE void plp_body(RowAcc& a, const VT* __restrict__ body, int nvec, int head, float lt, int t) {
  const int tid = threadIdx.x;
  for (int i0 = tid; i0 < nvec; i0 += kPlpT * kPlpUnroll) {
    VT v[kPlpUnroll];
#pragma unroll
    for (int u = 0; u < kPlpUnroll; ++u) {
      const int i = i0 + u * kPlpT;
      v[u] = plp_load16<kNT>(body + (i < nvec ? i : i0));
    }
#pragma unroll
    for (int u = 0; u < kPlpUnroll; ++u) {
      const int i = i0 + u * kPlpT;
      if (i < nvec) {
        float x[N];
        plp_unpack(v[u], x);
        plp_acc<N>(a, x, head + i * N, lt, t);
      }
    }
  }
}

HS_DEVICE unsigned int plp_key16(float f) {  // order-preserving key of the bf16-rounded value
  const unsigned short b = f32_to_bf16(f);
  return (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u);
}

// integer reductions over the workgroup (once per row); `scratch` holds 16 ints
template <bool kMin>
HS_DEVICE int plp_block_int(int v, int* scratch) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int y = __shfl_xor(v, o, 64);
    v = kMin ? min(v, y) : v + y;
  }
  if (lane == 0) scratch[wid] = v;
  __syncthreads();
  int r = scratch[0];
#pragma unroll
  for (int w = 1; w < kPlpT / 64; ++w) r = kMin ? min(r, scratch[w]) : r + scratch[w];
  __syncthreads();
  return r;
}

template <typename T>
__global__ __launch_bounds__(kPlpT) void prompt_logprobs_kernel(const T* __restrict__ logits, long stride, int V,
                                                                const int* __restrict__ targets,
                                                                const int* __restrict__ nreq,
                                                                float* __restrict__ out_lp, int* __restrict__ out_rank,
                                                                int* __restrict__ out_ids, float* __restrict__ out_top,
                                                                int K) {
  __shared__ float red[16];
  __shared__ int ired[16];
  __shared__ unsigned int hist[256];
  __shared__ unsigned int s_sel[2];  // threshold key, count strictly above
  __shared__ int s_tie_scan[kPlpT];
  __shared__ float c_val[kPlpCand];
  __shared__ int c_idx[kPlpCand];
  __shared__ unsigned int c_n;
  using R16 = Row16<T>;
  using VT = typename R16::V;
  constexpr int N = R16::N;
  const int r = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(nreq[r], 0), K);
  const int t = targets[r];
  const bool valid = t >= 0 && t < V;
  if (!valid && tid == 0) {
    out_lp[r] = -INFINITY;
    out_rank[r] = 0;
  }
  if (n <= 1 && tid >= n && tid < K) {  // slots this row leaves unused (the select writes its own)
    out_ids[(long)r * K + tid] = -1;
    out_top[(long)r * K + tid] = -INFINITY;
  }
  if (!valid && n == 0) return;
  const T* row = logits + (long)r * stride;
  const float lt = valid ? plp_ld(row, t) : 0.f;  // one uniform load

  // ---- the single pass: scalar head up to the first 16-byte boundary, 16-byte body, scalar tail
  const int head = min((long)V, (long)((16 - (reinterpret_cast<uintptr_t>(row) & 15)) & 15) / (long)sizeof(T));
  const int nvec = (V - head) / N;
  const int tail0 = head + nvec * N;
  RowAcc a;
  if (tid < head) {
    const float x[1] = {plp_ld(row, tid)};
    plp_acc<1>(a, x, tid, lt, t);
  }
  const VT* body = reinterpret_cast<const VT*>(row + head);
  if (n <= 1) plp_body<true, VT, N>(a, body, nvec, head, lt, t);  // streamed: nothing reads the row again
  else plp_body<false, VT, N>(a, body, nvec, head, lt, t);
  if (tail0 + tid < V) {
    const float x[1] = {plp_ld(row, tail0 + tid)};
    plp_acc<1>(a, x, tail0 + tid, lt, t);
  }

  // ---- merge: (m, s) pairs, the rank count, the lowest id among the threads that hold M
  const float M = block_max(a.m, red);
  const float M2 = M * kLog2e;
  const float sc = a.m == -INFINITY ? 0.f : a.s * __builtin_amdgcn_exp2f(__builtin_fmaf(a.m, kLog2e, -M2));
  const float S = block_sum(sc, red);
  const float lse = M == -INFINITY ? -INFINITY : (M2 + __builtin_amdgcn_logf(S)) * kLn2;
  const int before = plp_block_int<false>(a.cnt, ired);
  if (valid && tid == 0) {
    out_lp[r] = lt == -INFINITY ? -INFINITY : lt - lse;
    out_rank[r] = 1 + before;
  }
  if (n == 0) return;
  if (n == 1) {
    int best = plp_block_int<true>(a.m == M ? a.bi : 0x7fffffff, ired);
    if (M == -INFINITY) best = 0;  // a row of -inf: every id ties, the lowest leads
    if (tid == 0) {
      out_ids[(long)r * K] = best;
      out_top[(long)r * K] = M == -INFINITY ? -INFINITY : M - lse;
    }
    return;
  }

  // ---- n >= 2: top_logprobs' select (penalties.hip), on a row the pass above left in cache
  // radix select of the n-th largest 16-bit key: high byte, then low byte
  unsigned int prefix = 0, above = 0;  // keys with the selected high byte; count of keys above the bin
  for (int round = 0; round < 2; ++round) {
    for (int i = tid; i < 256; i += kPlpT) hist[i] = 0;
    __syncthreads();
    for (int v = tid; v < V; v += kPlpT) {
      const unsigned int k = plp_key16(plp_ld(row, v));
      if (round == 0) atomicAdd(&hist[k >> 8], 1u);
      else if ((k >> 8) == prefix) atomicAdd(&hist[k & 255], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned int acc = above;
      int b = 255;
      for (; b > 0; --b) {
        if (acc + hist[b] >= (unsigned)n) break;
        acc += hist[b];
      }
      s_sel[0] = round == 0 ? (unsigned)b : (prefix << 8) | (unsigned)b;
      s_sel[1] = acc;  // strictly above the selected bin
    }
    __syncthreads();
    if (round == 0) {
      prefix = s_sel[0];
      above = s_sel[1];
    }
    __syncthreads();
  }
  const unsigned int kth = s_sel[0];
  const unsigned int n_above = s_sel[1];
  // every key in the selected bin is a candidate while they fit the 64 slots, past that
  // the lowest-index ones: the one documented bound on exactness (header)
  const int take_ties = kPlpCand - (int)n_above;
  // collect: every key > kth, then the lowest-index ties (contiguous chunks per thread +
  // a block scan give each tie its global index rank)
  if (tid == 0) c_n = 0;
  const int chunk = (V + kPlpT - 1) / kPlpT;
  const int lo = min((long)V, (long)tid * chunk), hi = min((long)V, (long)lo + chunk);
  int ntie = 0;
  for (int v = lo; v < hi; ++v) ntie += plp_key16(plp_ld(row, v)) == kth;
  s_tie_scan[tid] = ntie;
  __syncthreads();
  for (int d = 1; d < kPlpT; d <<= 1) {  // inclusive scan
    const int x = tid >= d ? s_tie_scan[tid - d] : 0;
    __syncthreads();
    s_tie_scan[tid] += x;
    __syncthreads();
  }
  int tie_rank = s_tie_scan[tid] - ntie;
  for (int v = lo; v < hi; ++v) {
    const float l = plp_ld(row, v);
    const unsigned int k = plp_key16(l);
    bool take = k > kth;
    if (k == kth) take = tie_rank++ < take_ties;
    if (take) {
      const unsigned int p = atomicAdd(&c_n, 1u);
      if (p < (unsigned)kPlpCand) {
        c_val[p] = l;
        c_idx[p] = v;
      }
    }
  }
  __syncthreads();
  // order (exact value desc, id asc) and write the first n
  if (tid == 0) {
    const int cn = min((int)c_n, kPlpCand);
    for (int i = 1; i < cn; ++i) {
      const float k = c_val[i];
      const int x = c_idx[i];
      int j = i - 1;
      while (j >= 0 && (c_val[j] < k || (c_val[j] == k && c_idx[j] > x))) {
        c_val[j + 1] = c_val[j];
        c_idx[j + 1] = c_idx[j];
        --j;
      }
      c_val[j + 1] = k;
      c_idx[j + 1] = x;
    }
    for (int i = 0; i < K; ++i) {
      const bool ok = i < n && i < cn;
      out_ids[(long)r * K + i] = ok ? c_idx[i] : -1;
      out_top[(long)r * K + i] = ok && c_val[i] != -INFINITY ? c_val[i] - lse : -INFINITY;
    }
  }
}

}  // namespace

void launch_prompt_logprobs(const void* logits, bool is_bf16, long stride, int rows, int V, const int* targets,
                            const int* nreq, float* out_lp, int* out_rank, int* out_ids, float* out_top, int K,
                            hipStream_t s) {
  if (rows <= 0 || V <= 0) return;
  if (is_bf16)
    prompt_logprobs_kernel<unsigned short><<<rows, kPlpT, 0, s>>>(static_cast<const unsigned short*>(logits), stride,
                                                                  V, targets, nreq, out_lp, out_rank, out_ids, out_top,
                                                                  K);
  else
    prompt_logprobs_kernel<float><<<rows, kPlpT, 0, s>>>(static_cast<const float*>(logits), stride, V, targets, nreq,
                                                         out_lp, out_rank, out_ids, out_top, K);
}

}  // namespace hipserve
