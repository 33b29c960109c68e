// torch.ops.hipserve.* — operator registration for the gfx950 kernel library.
//
// All ops write into caller-provided outputs (no allocation, no host sync), so
// the decode step can be captured into a hipGraph by torch.cuda.CUDAGraph.
//
// Every op reads "validate, launch": it builds an Args checker from its anchor tensor,
// and a tensor becomes a pointer only through that checker (same device, dtype, layout,
// extent), directly or through one of the shared validators below.
#include <torch/library.h>
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <initializer_list>
#include <sstream>
#include <type_traits>

#include "hipserve/kernels.h"
#include "hipserve/quant_formats.h"

namespace {

hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}

// ---- the per-call argument checker

// element types as a bit set, so an argument can allow several (BF16 | F32)
enum : unsigned { BF16 = 1, F32 = 2, F16 = 4, U8 = 8, I8 = 16, I16 = 32, I32 = 64, I64 = 128, F8 = 256, OTHER = 512 };
constexpr unsigned BYTES = U8 | I8 | F8, ANYTYPE = ~0u;
struct DtypeName { unsigned bit; at::ScalarType type; const char* name; };
const DtypeName kDtypes[] = {{BF16, at::kBFloat16, "bf16"}, {F32, at::kFloat, "fp32"},  {F16, at::kHalf, "f16"},
                             {U8, at::kByte, "uint8"},      {I8, at::kChar, "int8"},    {I16, at::kShort, "int16"},
                             {I32, at::kInt, "int32"},      {I64, at::kLong, "int64"},  {F8, at::kFloat8_e4m3fn, "float8_e4m3fn"}};

unsigned dtype_bit(at::ScalarType t) {
  for (const DtypeName& d : kDtypes)
    if (d.type == t) return d.bit;
  return OTHER;
}
std::string dtype_names(unsigned set) {  // failure path only
  std::string s;
  for (const DtypeName& d : kDtypes)
    if (set & d.bit) s += (s.empty() ? "" : " or ") + std::string(d.name);
  return s;
}
template <class T>
constexpr unsigned dtype_of() {
  if constexpr (std::is_same_v<T, float>) return F32;
  else if constexpr (std::is_same_v<T, int>) return I32;
  else if constexpr (std::is_same_v<T, int64_t>) return I64;
  else {
    static_assert(std::is_same_v<T, uint8_t>, "typed pointers: float, int, int64_t, uint8_t");
    return U8;
  }
}

// contiguous; or unit inner stride (a view of row-major rows), ROWS4 / ROWS8: at a row stride of a multiple of
// 4 / 8 elements too (8- / 16-byte aligned bf16 rows)
enum Layout { CONTIG = 0, ROWS = 1, ROWS4 = 4, ROWS8 = 8 };

// What an argument must hold: at least n elements (an integer), exactly(n) elements, or a
// shape {d0, d1, ...} whose entries are exact sizes, at_least(n) or ANY.
constexpr int64_t at_least(int64_t n) { return ~n; }
constexpr int64_t ANY = at_least(0);
struct Extent {
  enum { MIN_NUMEL, NUMEL, SHAPE } kind = MIN_NUMEL;
  int64_t n = 0;
  std::initializer_list<int64_t> shape;
  Extent() {}
  Extent(int64_t min_numel) : n(min_numel) {}
  Extent(std::initializer_list<int64_t> s) : kind(SHAPE), shape(s) {}
  bool holds(const at::Tensor& t) const {
    if (kind == MIN_NUMEL) return t.numel() >= n;
    if (kind == NUMEL) return t.numel() == n;
    if (t.dim() != (int64_t)shape.size()) return false;
    int i = 0;
    for (int64_t want : shape) {
      const int64_t have = t.size(i++);
      if (want >= 0 ? have != want : have < ~want) return false;
    }
    return true;
  }
  std::string str() const {  // failure path only
    std::ostringstream o;
    if (kind != SHAPE) {
      o << (kind == NUMEL ? "exactly " : "at least ") << n << " elements";
      return o.str();
    }
    o << "shape [";
    const char* sep = "";
    for (int64_t want : shape) {
      o << sep;
      if (want >= 0) o << want;
      else if (want == ANY) o << '*';
      else o << ">=" << ~want;
      sep = ", ";
    }
    o << ']';
    return o.str();
  }
};
Extent exactly(int64_t numel) {
  Extent e(numel);
  e.kind = Extent::NUMEL;
  return e;
}

// an absent optional as an undefined tensor (which ptr_if / as_if turn into nullptr)
const at::Tensor& maybe(const c10::optional<at::Tensor>& t) {
  static const at::Tensor none;
  return t.has_value() ? *t : none;
}

// One per op call, built first from the op's name and its anchor tensor: refuses an anchor off
// the GPU, makes the anchor's device current for the call, and is the only way a tensor
// (input or output alike) becomes a pointer. Messages: "<op>: <argument> must ...".
struct Args {
  const char* op;
  c10::Device dev;
  c10::hip::HIPGuardMasqueradingAsCUDA guard;

  static c10::Device gpu_of(const char* op, const at::Tensor& t, const char* name) {
    TORCH_CHECK(t.defined() && t.is_cuda(), op, ": ", name, " must be a GPU tensor");
    return t.device();
  }
  Args(const char* op, const at::Tensor& anchor, const char* name)
      : op(op), dev(gpu_of(op, anchor, name)), guard(dev) {}

  // same device as the anchor, dtype in `dtypes` (returns which), layout, extent
  unsigned check(const at::Tensor& t, const char* name, unsigned dtypes, Layout lay, const Extent& e = {}) const {
    TORCH_CHECK(t.defined() && t.device() == dev, op, ": ", name, " must be a tensor on ", dev, ", the device of the call");
    const unsigned bit = dtype_bit(t.scalar_type());
    TORCH_CHECK(bit & dtypes, op, ": ", name, " must be ", dtype_names(dtypes), ", got ", t.scalar_type());
    if (lay == CONTIG) {
      TORCH_CHECK(t.is_contiguous(), op, ": ", name, " must be contiguous");
    } else {
      TORCH_CHECK(t.dim() >= 1 && t.stride(-1) == 1, op, ": ", name, " must have unit inner stride");
      TORCH_CHECK(t.dim() < 2 || t.stride(0) % lay == 0, op, ": ", name, " must have rows ", 2 * lay, "-byte aligned");
    }
    TORCH_CHECK(e.holds(t), op, ": ", name, " must have ", e.str(), ", got ", t.sizes());
    return bit;
  }
  void* ptr(const at::Tensor& t, const char* name, unsigned dtypes, Layout lay, const Extent& e = {},
            unsigned* which = nullptr) const {
    const unsigned bit = check(t, name, dtypes, lay, e);
    if (which) *which = bit;
    return t.data_ptr();
  }
  template <class T>
  T* as(const at::Tensor& t, const char* name, Layout lay, const Extent& e = {}) const {
    return static_cast<T*>(ptr(t, name, dtype_of<T>(), lay, e));
  }
  // "absent" arguments: an undefined tensor (see maybe()) or one of zero elements gives
  // nullptr, with no device / dtype demand on it; the extent must still allow that
  void* ptr_if(const at::Tensor& t, const char* name, unsigned dtypes, Layout lay, const Extent& e = {}) const {
    if (!t.defined()) return nullptr;
    if (t.numel() > 0) return ptr(t, name, dtypes, lay, e);
    TORCH_CHECK(e.holds(t), op, ": ", name, " must have ", e.str(), ", got ", t.sizes());
    return nullptr;
  }
  template <class T>
  T* as_if(const at::Tensor& t, const char* name, Layout lay, const Extent& e = {}) const {
    return static_cast<T*>(ptr_if(t, name, dtype_of<T>(), lay, e));
  }
};

// ---- validators shared by the ops

// fp32 split-K partials [S, M, N] (one slab per K slice)
float* splitk_ws(const Args& a, const at::Tensor& ws, int64_t S, int64_t M, int64_t N, const char* name = "ws") {
  return a.as<float>(ws, name, CONTIG, S * M * N);
}

// norm weight [N], bf16 or fp32
struct NormWeight { const void* p; bool f32; };
NormWeight norm_weight(const Args& a, const at::Tensor& w, const char* name, int64_t N) {
  unsigned which;
  const void* p = a.ptr(w, name, BF16 | F32, CONTIG, exactly(N), &which);
  return {p, which == F32};
}

// logits rows [rows, V], bf16 or fp32, unit inner stride
struct Logits { void* p; bool bf16; int rows, V; long stride; };
Logits logits_rows(const Args& a, const at::Tensor& logits) {
  unsigned which;
  void* p = a.ptr(logits, "logits", BF16 | F32, ROWS, {ANY, ANY}, &which);
  return {p, which == BF16, (int)logits.size(0), (int)logits.size(1), (long)logits.stride(0)};
}

// paged KV cache pair: K [blocks, nkv, bs, D] and V [blocks, nkv, D, bs], contiguous, bf16 or
// float8_e4m3fn (--kv-cache-dtype fp8: e4m3 with a per-tensor scale of 1, written rounded /
// read widened by the kernels), K and V alike. head_dim < 0: taken from K.
struct KvCache { void *k, *v; bool f8; int bs, D; };
KvCache kv_cache(const Args& a, const at::Tensor& k, const at::Tensor& v, int64_t nkv, int64_t head_dim = -1) {
  unsigned which;
  void* kp = a.ptr(k, "k_cache", BF16 | F8, CONTIG, {ANY, nkv, ANY, head_dim < 0 ? ANY : head_dim}, &which);
  const int64_t bs = k.size(2), D = k.size(3);
  void* vp = a.ptr(v, "v_cache", which, CONTIG, {k.size(0), nkv, D, bs});
  return {kp, vp, which == F8, (int)bs, (int)D};
}

// RoPE inputs of T rows: int64 positions / cache slots [>= T], fp32 cos_sin table [*, D]
struct RopeArgs { const int64_t *positions, *slots; const float* cos_sin; };
RopeArgs rope_args(const Args& a, const at::Tensor& positions, const at::Tensor& slots, const at::Tensor& cos_sin,
                   int64_t T, int64_t D) {
  return {a.as<int64_t>(positions, "positions", CONTIG, T), a.as<int64_t>(slots, "slots", CONTIG, T),
          a.as<float>(cos_sin, "cos_sin", CONTIG, {ANY, D})};
}

// decode attention over B sequences: GQA / block / partition geometry, block tables
// [>= B, blocks], context lengths [>= B] and the partition workspace tmp_out [>= B, nq,
// max_parts, D] / tmp_ml [>= B, nq, max_parts, 2]
struct DecodeAttn {
  const int* block_tables;
  int bt_stride;
  const int* context_lens;
  float *tmp_out, *tmp_ml;
  int max_parts;
};
DecodeAttn decode_attn_args(const Args& a, const at::Tensor& block_tables, const at::Tensor& context_lens,
                            const at::Tensor& tmp_out, const at::Tensor& tmp_ml, int64_t B, int64_t nq, int64_t nkv,
                            int64_t D, int64_t bs, int64_t part_size, int64_t window) {
  TORCH_CHECK(window >= 0, a.op, ": window >= 0");
  TORCH_CHECK(nkv > 0 && nq % nkv == 0 && nq / nkv <= 16, a.op, ": GQA group <= 16");
  TORCH_CHECK(bs > 0 && bs % 16 == 0 && (bs & (bs - 1)) == 0, a.op, ": block_size a power of two >= 16");
  TORCH_CHECK(part_size > 0 && part_size % 128 == 0 && part_size / bs < 255, a.op, ": part_size % 128 == 0, < 255 blocks");
  DecodeAttn g;
  g.block_tables = a.as<int>(block_tables, "block_tables", ROWS, {at_least(B), ANY});
  g.bt_stride = block_tables.stride(0);
  g.context_lens = a.as<int>(context_lens, "context_lens", CONTIG, B);
  g.tmp_ml = a.as<float>(tmp_ml, "tmp_ml", CONTIG, {at_least(B), nq, ANY, 2});
  g.max_parts = tmp_ml.size(2);
  g.tmp_out = a.as<float>(tmp_out, "tmp_out", CONTIG, {at_least(B), nq, g.max_parts, D});
  TORCH_CHECK((long)g.max_parts * part_size >= (long)block_tables.size(1) * bs, a.op,
              ": workspace partitions must cover block_tables capacity");
  return g;
}

// optional per-head q / k RMSNorm weights (fp32 [head_dim], Qwen3): both or neither
bool qk_norm_weights(const Args& a, const c10::optional<at::Tensor>& q_w, const c10::optional<at::Tensor>& k_w,
                     int64_t D, const float** qw, const float** kw) {
  TORCH_CHECK(maybe(q_w).defined() == maybe(k_w).defined(), a.op, ": q and k norm weights come together");
  *qw = *kw = nullptr;
  if (!maybe(q_w).defined()) return false;
  *qw = a.as<float>(*q_w, "q norm weight", CONTIG, exactly(D));
  *kw = a.as<float>(*k_w, "k norm weight", CONTIG, exactly(D));
  return true;
}

// optional f16 pair-order copy of a bf16 2-D tensor `of` (out16 of out, act16 of act, x16 of
// x): its rows and row stride, `cols` columns (a size or at_least(n)); or nullptr
void* f16_twin(const Args& a, const c10::optional<at::Tensor>& t, const char* name, const at::Tensor& of, int64_t cols) {
  void* p = a.ptr_if(maybe(t), name, F16, ROWS, {of.size(0), cols});
  TORCH_CHECK(!p || t->stride(0) == of.stride(0), a.op, ": ", name, " must have the row stride of the tensor it copies");
  return p;
}
void* out16_arg(const Args& a, const c10::optional<at::Tensor>& out16, const at::Tensor& out) {
  return f16_twin(a, out16, "out16", out, out.size(1));
}

// optional per-token e4m3 copy (out8 uint8 like out, xs8 fp32 [M]) of a norm epilogue's output
struct E4m3Out { void* q = nullptr; float* xs = nullptr; };
E4m3Out e4m3_out_args(const Args& a, const c10::optional<at::Tensor>& out8, const c10::optional<at::Tensor>& xs8,
                      const at::Tensor& out) {
  E4m3Out o;
  if (!maybe(out8).defined()) return o;
  TORCH_CHECK(maybe(xs8).defined(), a.op, ": out8 needs xs8");
  o.q = a.ptr(*out8, "out8", U8, CONTIG, {out.size(0), out.size(1)});
  o.xs = a.as<float>(*xs8, "xs8", CONTIG, exactly(out.size(0)));
  return o;
}

// tiled FP8 weight parts (q [N/16, K/256, 4096] uint8, rs [N] fp32) stacked along N, with the
// activations' row scales xs, into W; returns the total rows. tile0: number the parts'
// 256-column tiles (the prefill GEMM's store epilogues)
int fp8_parts(const Args& a, const float* xs, const std::vector<at::Tensor>& q, const std::vector<at::Tensor>& rs,
              int64_t K, bool tile0, hipserve::PgF8& W) {
  TORCH_CHECK(!q.empty() && q.size() <= (size_t)hipserve::kPgF8Parts && rs.size() == q.size(), a.op, ": 1-",
              hipserve::kPgF8Parts, " parts of q and rs");
  W.n = (int)q.size();
  W.xs = xs;
  int rows = 0;
  for (size_t i = 0; i < q.size(); ++i) {
    const int n = rs[i].numel();
    W.p[i] = hipserve::PgF8Part{a.as<uint8_t>(q[i], "q[i] (tiled FP8 [N/16, K/256, 4096] with rs [N])", CONTIG,
                                              exactly((int64_t)n * K)),
                                a.as<float>(rs[i], "rs[i]", CONTIG), n, tile0 ? rows / 256 : 0};
    rows += n;
  }
  return rows;
}

using hipserve::gq::QuantFormat;

// quant_formats.h as text, "NAME id chunk_bytes sub_shift gguf row_scaled prefill moe" per line:
// for the error messages, and as an op for the cross-check against hipserve/ops/quant.py
std::string quant_formats() {
  std::ostringstream o;
  for (int id : hipserve::gq::kQuantFormatIds) {
    const QuantFormat f = hipserve::gq::quant_format(id);
    o << f.name << ' ' << f.id << ' ' << f.chunk_bytes << ' ' << f.sub_shift << ' ' << f.gguf << ' ' << f.row_scaled
      << ' ' << f.prefill << ' ' << f.moe << '\n';
  }
  return o.str();
}
// the table row of a tiled op's kernel qtype (moe: of a format with an expert body)
QuantFormat tiled_format(int64_t qtype, const char* op, bool moe = false) {
  const QuantFormat f = hipserve::gq::quant_format(qtype == (int)qtype ? (int)qtype : -1);
  TORCH_CHECK(f.id >= 0 && (f.moe || !moe), op, ": kernel qtype ", qtype, moe ? " has no expert body" : " is unknown",
              "; name id chunk sub_shift gguf row_scaled prefill moe:\n", quant_formats());
  return f;
}

// 1-4 parts in the tiled layout (one uint8 tensor [rows/16, K/256, chunk] each) with their
// formats / rows / output columns into P (rss: fp32 row scales of the row-scaled formats, or
// null where the op takes none); returns the parts' column span
long tiled_parts(const Args& a, const std::vector<at::Tensor>& qs, const std::vector<at::Tensor>* rss,
                 const std::vector<int64_t>& qtypes, const std::vector<int64_t>& rows, const std::vector<int64_t>& cols,
                 int64_t K, hipserve::GgufPart* P) {
  const size_t np = qs.size();
  TORCH_CHECK(np >= 1 && np <= 4 && qtypes.size() == np && (!rss || rss->size() == np) && rows.size() == np &&
              cols.size() == np, a.op, ": 1-4 parts");
  long span = 0;
  for (size_t i = 0; i < np; ++i) {
    const QuantFormat f = tiled_format(qtypes[i], a.op);
    TORCH_CHECK(cols[i] >= 0 && cols[i] % 4 == 0 && rows[i] % 16 == 0 && rows[i] > 0, a.op,
                ": parts are 16-row multiples at 4-aligned columns");
    const void* q = a.ptr(qs[i], "qs[i] (a tiled [N/16, K/256, chunk] tensor of its format)", U8, CONTIG,
                          exactly(rows[i] / 16 * (K / 256) * f.chunk_bytes));
    const float* rs = rss && f.row_scaled ? a.as<float>((*rss)[i], "rss[i] (FP8 / INT8C: an fp32 scale per row)",
                                                         CONTIG, exactly(rows[i]))
                                          : nullptr;
    P[i] = hipserve::GgufPart{q, rs, (int)qtypes[i], (int)rows[i], (int)cols[i]};
    span = std::max(span, (long)(cols[i] + rows[i]));
  }
  return span;
}

// the output of a split-K capable GEMM: fp32 partials ws [S, rows, N] where ws has elements,
// else (S == 1) bf16 out [rows, >= out_cols]
struct GemmOut { void* out = nullptr; long stride = 0; float* ws = nullptr; };
GemmOut partials_or_out(const Args& a, const at::Tensor& out, const at::Tensor& ws, int64_t S, int64_t rows, int64_t N,
                        int64_t out_cols) {
  GemmOut o;
  o.ws = a.as_if<float>(ws, "ws", CONTIG, ws.numel() > 0 ? S * rows * N : 0);
  if (o.ws) return o;
  TORCH_CHECK(S == 1, a.op, ": split-K needs a partial workspace");
  o.out = a.ptr(out, "out", BF16, ROWS4, {rows, at_least(out_cols)});
  o.stride = out.stride(0);
  return o;
}

// the activations of a decode GEMM: x bf16 [1..64, K], K % (256 * splits) == 0, 16-byte rows
struct DecodeX { const void* p; int M, K; long stride; };
DecodeX decode_gemm_x(const Args& a, const at::Tensor& x, int64_t splits) {
  const void* p = a.ptr(x, "x", BF16, ROWS8, {ANY, ANY});
  const int M = x.size(0), K = x.size(1);
  TORCH_CHECK(M >= 1 && M <= 64, a.op, ": 1 <= M <= 64");
  TORCH_CHECK(splits >= 1 && K % (256 * splits) == 0, a.op, ": K must be a multiple of 256*splits");
  return {p, M, K, (long)x.stride(0)};
}

// moe_align's tables: int32 slots [nslots] and tile_expert covering them in tiles of `tile`
struct MoeTiles { int *slots, *tile_expert; long nslots; int tiles_cap; };
MoeTiles moe_tiles(const Args& a, const at::Tensor& slots, const at::Tensor& tile_expert, int64_t tile) {
  TORCH_CHECK(tile > 0, a.op, ": tile > 0");
  int* sp = a.as<int>(slots, "slots", CONTIG);
  const long nslots = slots.numel();
  return {sp, a.as<int>(tile_expert, "tile_expert", CONTIG, (nslots + tile - 1) / tile), nslots, (int)tile_expert.numel()};
}

// the routing of a combine: fp32 weights w and int32 pair_slot, [>= T * k] each
struct Combine { const float* w; const int* pair_slot; };
Combine combine_args(const Args& a, const at::Tensor& w, const at::Tensor& pair_slot, int64_t pairs) {
  return {a.as<float>(w, "w", CONTIG, pairs), a.as<int>(pair_slot, "pair_slot", CONTIG, pairs)};
}

// penalty state of V tokens: int32 counts [slots, V], seen bits int32 [slots, ceil(V/32)]
struct PenState { int* counts; unsigned int* seen; int V; };
PenState pen_state(const Args& a, const at::Tensor& counts, const at::Tensor& seen) {
  int* c = a.as<int>(counts, "counts", CONTIG, {ANY, ANY});
  const int V = counts.size(1);
  return {c, reinterpret_cast<unsigned int*>(a.as<int>(seen, "seen", CONTIG, {counts.size(0), (V + 31) / 32})), V};
}

// ---- the ops

// out = RMSNorm(x) * weight; with a residual: residual += x first, and out is its norm
void rmsnorm_op(const char* name, at::Tensor& out, const at::Tensor& x, at::Tensor* residual, const at::Tensor& weight,
                double eps, const c10::optional<at::Tensor>& out8, const c10::optional<at::Tensor>& xs8) {
  Args a(name, x, "x");
  const void* xp = a.ptr(x, "x", BF16, ROWS, {ANY, ANY});
  const int rows = x.size(0), hidden = x.size(1);
  TORCH_CHECK(hidden % 8 == 0 && hidden <= 16384, name, ": hidden must be a multiple of 8, <= 16384");
  void* op = a.ptr(out, "out", BF16, ROWS, {at_least(rows), at_least(hidden)});
  void* rp = residual ? a.ptr(*residual, "residual", BF16, CONTIG, {rows, hidden}) : nullptr;
  const NormWeight w = norm_weight(a, weight, "weight", hidden);
  const E4m3Out o8 = e4m3_out_args(a, out8, xs8, out);
  hipserve::launch_rmsnorm(op, rp, xp, w.p, w.f32, rows, hidden, x.stride(0), out.stride(0), (float)eps,
                           cur_stream(), o8.q, o8.xs);
}
void rmsnorm(at::Tensor& out, const at::Tensor& x, const at::Tensor& weight, double eps,
             const c10::optional<at::Tensor>& out8, const c10::optional<at::Tensor>& xs8) {
  rmsnorm_op("rmsnorm", out, x, nullptr, weight, eps, out8, xs8);
}
void fused_add_rmsnorm(at::Tensor& out, const at::Tensor& x, at::Tensor& residual, const at::Tensor& weight, double eps,
                       const c10::optional<at::Tensor>& out8, const c10::optional<at::Tensor>& xs8) {
  rmsnorm_op("fused_add_rmsnorm", out, x, &residual, weight, eps, out8, xs8);
}

// residual = bf16(table[id] * scale), out = RMSNorm(residual) * weight per row; id =
// ids[row], or tok[src[row]] where src[row] >= 0 (device-side decode lookahead ids);
// out8 / xs8 (optional): out also as per-token e4m3 + row scale (= act_quant_fp8 of out)
void embed_rmsnorm(at::Tensor& out, at::Tensor& residual, const at::Tensor& table, const at::Tensor& ids,
                   const c10::optional<at::Tensor>& src, const c10::optional<at::Tensor>& tok,
                   const at::Tensor& weight, double eps, double scale, const c10::optional<at::Tensor>& out8,
                   const c10::optional<at::Tensor>& xs8) {
  Args a("embed_rmsnorm", table, "table");
  const void* tp = a.ptr(table, "table", BF16, CONTIG, {ANY, ANY});
  const int64_t* idp = a.as<int64_t>(ids, "ids", CONTIG);
  const int hidden = table.size(1), rows = ids.numel();
  TORCH_CHECK(hidden % 8 == 0 && hidden <= 16384, "embed_rmsnorm: hidden must be a multiple of 8, <= 16384");
  void* op = a.ptr(out, "out", BF16, CONTIG, {rows, hidden});
  void* rp = a.ptr(residual, "residual", BF16, CONTIG, {rows, hidden});
  TORCH_CHECK(src.has_value() == tok.has_value(), "embed_rmsnorm: src and tok come together");
  const int64_t *sp = nullptr, *kp = nullptr;
  if (src.has_value()) {
    sp = a.as<int64_t>(*src, "src", CONTIG, exactly(rows));
    kp = a.as<int64_t>(*tok, "tok", CONTIG);
  }
  const NormWeight w = norm_weight(a, weight, "weight", hidden);
  const E4m3Out o8 = e4m3_out_args(a, out8, xs8, out);
  hipserve::launch_embed_rmsnorm(op, rp, tp, idp, sp, kp, w.p, w.f32, rows, hidden, (float)eps, cur_stream(),
                                 (float)scale, o8.q, o8.xs);
}

// out [rows, I] = act(x[:, :I]) * x[:, I:] of x [rows, 2 I]
using GluLauncher = void (*)(void*, const void*, long, int, long, long, hipStream_t);
void glu_and_mul(const char* name, GluLauncher launch, at::Tensor& out, const at::Tensor& x) {
  Args a(name, x, "x");
  const void* xp = a.ptr(x, "x", BF16, ROWS, {ANY, ANY});
  TORCH_CHECK(x.size(1) % 16 == 0, name, ": x [rows, 2 I], I % 8 == 0");
  void* op = a.ptr(out, "out", BF16, ROWS, {x.size(0), x.size(1) / 2});
  launch(op, xp, x.size(0), out.size(1), x.stride(0), out.stride(0), cur_stream());
}
void silu_and_mul(at::Tensor& out, const at::Tensor& x) {
  glu_and_mul("silu_and_mul", &hipserve::launch_silu_and_mul, out, x);
}
void gelu_and_mul(at::Tensor& out, const at::Tensor& x) {
  glu_and_mul("gelu_and_mul", &hipserve::launch_gelu_and_mul, out, x);
}

void rope_cache(at::Tensor& qkv, const at::Tensor& positions, const at::Tensor& slots,
                const at::Tensor& cos_sin, at::Tensor& k_cache, at::Tensor& v_cache,
                int64_t nq, int64_t nkv, int64_t head_dim, int64_t mode) {
  Args a("rope_cache", qkv, "qkv");
  TORCH_CHECK(head_dim > 0 && head_dim % 16 == 0 && (mode == 0 || mode == 1), "rope_cache: head_dim % 16 == 0, mode 0 / 1");
  void* qp = a.ptr(qkv, "qkv", BF16, ROWS, {ANY, at_least((nq + 2 * nkv) * head_dim)});
  const int T = qkv.size(0);
  const RopeArgs r = rope_args(a, positions, slots, cos_sin, T, head_dim);
  const KvCache kv = kv_cache(a, k_cache, v_cache, nkv, head_dim);
  hipserve::launch_rope_cache(qp, qkv.stride(0), r.positions, r.slots, r.cos_sin, kv.k, kv.v, T, nq, nkv, head_dim,
                              kv.bs, mode, cur_stream(), kv.f8);
}

void paged_decode(at::Tensor& out, const at::Tensor& q, const at::Tensor& k_cache,
                  const at::Tensor& v_cache, const at::Tensor& block_tables,
                  const at::Tensor& context_lens, at::Tensor& tmp_out, at::Tensor& tmp_ml,
                  int64_t nq, int64_t nkv, int64_t part_size, double scale, int64_t window,
                  const c10::optional<at::Tensor>& out16, double softcap) {
  Args a("paged_decode", q, "q");
  const KvCache kv = kv_cache(a, k_cache, v_cache, nkv);
  const int D = kv.D;
  TORCH_CHECK(D == 64 || D == 96 || D == 128 || D == 256, "paged_decode: head_dim 64/96/128/256");
  TORCH_CHECK(softcap >= 0, "paged_decode: softcap >= 0 (0 = off)");
  const void* qp = a.ptr(q, "q", BF16, ROWS, {ANY, at_least(nq * D)});
  const int B = q.size(0);
  void* op = a.ptr(out, "out", BF16, ROWS, {at_least(B), at_least(nq * D)});
  const DecodeAttn g = decode_attn_args(a, block_tables, context_lens, tmp_out, tmp_ml, B, nq, nkv, D, kv.bs,
                                        part_size, window);
  hipserve::launch_paged_decode(op, out.stride(0), qp, q.stride(0), kv.k, kv.v, g.block_tables, g.bt_stride,
                                g.context_lens, g.tmp_out, g.tmp_ml, B, nq, nkv, D, kv.bs, part_size, g.max_parts,
                                (float)scale, (int)window, cur_stream(), out16_arg(a, out16, out), kv.f8,
                                (float)softcap);
}

void paged_decode_qkv(at::Tensor& out, const at::Tensor& ws, int64_t splits, const at::Tensor& positions,
                      const at::Tensor& slots, const at::Tensor& cos_sin, at::Tensor& k_cache, at::Tensor& v_cache,
                      const at::Tensor& block_tables, const at::Tensor& context_lens, at::Tensor& tmp_out,
                      at::Tensor& tmp_ml, int64_t nq, int64_t nkv, int64_t part_size, double scale, int64_t window,
                      int64_t mode, const c10::optional<at::Tensor>& out16, const c10::optional<at::Tensor>& q_w,
                      const c10::optional<at::Tensor>& k_w, double eps, double softcap) {
  Args a("paged_decode_qkv", ws, "ws");
  const KvCache kv = kv_cache(a, k_cache, v_cache, nkv);
  const int D = kv.D;
  TORCH_CHECK(!kv.f8, "paged_decode_qkv: bf16 KV cache only");
  TORCH_CHECK(D == 64 || D == 128, "paged_decode_qkv: head_dim 64/128");
  TORCH_CHECK(mode == 0 || mode == 1, "paged_decode_qkv: mode 0 / 1");
  TORCH_CHECK(softcap >= 0, "paged_decode_qkv: softcap >= 0 (0 = off)");
  const float *qwp, *kwp;  // per-head q / k RMSNorm before RoPE (Qwen3)
  if (qk_norm_weights(a, q_w, k_w, D, &qwp, &kwp))
    TORCH_CHECK(mode == 0, "paged_decode_qkv: q/k norm needs rotate-half RoPE (mode 0)");
  void* op = a.ptr(out, "out", BF16, ROWS, {ANY, at_least(nq * D)});
  const int B = out.size(0);
  const long N = (nq + 2 * nkv) * D;
  const float* wsp = splitk_ws(a, ws, splits, B, N);
  const RopeArgs r = rope_args(a, positions, slots, cos_sin, B, D);
  const DecodeAttn g = decode_attn_args(a, block_tables, context_lens, tmp_out, tmp_ml, B, nq, nkv, D, kv.bs,
                                        part_size, window);
  hipserve::launch_paged_decode_qkv(op, out.stride(0), wsp, splits, N, r.positions, r.slots, r.cos_sin, mode, kv.k,
                                    kv.v, g.block_tables, g.bt_stride, g.context_lens, g.tmp_out, g.tmp_ml, B, nq,
                                    nkv, D, kv.bs, part_size, g.max_parts, (float)scale, (int)window, cur_stream(),
                                    out16_arg(a, out16, out), qwp, kwp, (float)eps, (float)softcap);
}

void prefill_attention(at::Tensor& out, const at::Tensor& q, const at::Tensor& k_cache,
                       const at::Tensor& v_cache, const at::Tensor& block_tables,
                       const at::Tensor& cu_q, const at::Tensor& ctx_lens,
                       const at::Tensor& tiles, int64_t nq, int64_t nkv, double scale, int64_t window,
                       double softcap, const c10::optional<at::Tensor>& limits) {
  Args a("prefill_attention", q, "q");
  const KvCache kv = kv_cache(a, k_cache, v_cache, nkv);
  const int D = kv.D;
  TORCH_CHECK(D == 64 || D == 96 || D == 128 || D == 256, "prefill_attention: head_dim 64/96/128/256");
  TORCH_CHECK(window >= 0, "prefill_attention: window >= 0");
  TORCH_CHECK(softcap >= 0, "prefill_attention: softcap >= 0 (0 = off)");
  TORCH_CHECK(kv.bs % 16 == 0 && nq % nkv == 0, "prefill_attention: block_size % 16 == 0, nq % nkv == 0");
  const void* qp = a.ptr(q, "q", BF16, ROWS, {ANY, at_least(nq * D)});
  void* op = a.ptr(out, "out", BF16, ROWS, {ANY, at_least(nq * D)});
  const int* bt = a.as<int>(block_tables, "block_tables", ROWS, {ANY, ANY});
  const int* cu = a.as<int>(cu_q, "cu_q", ROWS);
  const int* cl = a.as<int>(ctx_lens, "ctx_lens", ROWS);
  const int* tp = a.as<int>(tiles, "tiles", CONTIG, {ANY, 2});
  // per-row key limits (Gemma-3 image blocks): one absolute key position per row of q
  const int* lp = nullptr;
  if (limits.has_value()) {
    TORCH_CHECK(softcap == 0, "prefill_attention: limits with softcap > 0 has no kernel");
    TORCH_CHECK(D == 128 || D == 256, "prefill_attention: limits need head_dim 128 or 256, got ", D);
    lp = a.as<int>(*limits, "limits", CONTIG, exactly(q.size(0)));
  }
  hipserve::launch_prefill_attention(op, out.stride(0), qp, q.stride(0), kv.k, kv.v, bt, block_tables.stride(0), cu, cl,
                                     tp, tiles.size(0), nq, nkv, D, kv.bs, (float)scale, (int)window, cur_stream(),
                                     kv.f8, (float)softcap, lp);
}

// Per-head RMSNorm of q and k inside the merged qkv rows, in place (Qwen3 / Gemma-3).
void qk_rmsnorm(at::Tensor& qkv, const at::Tensor& q_w, const at::Tensor& k_w, int64_t nq, int64_t nkv,
                int64_t head_dim, double eps) {
  Args a("qk_rmsnorm", qkv, "qkv");
  TORCH_CHECK(head_dim > 0 && head_dim <= 256, "qk_rmsnorm: head_dim <= 256");
  void* qp = a.ptr(qkv, "qkv", BF16, ROWS, {ANY, at_least((nq + nkv) * head_dim)});
  const float* qw = a.as<float>(q_w, "q_w", CONTIG, exactly(head_dim));
  const float* kw = a.as<float>(k_w, "k_w", CONTIG, exactly(head_dim));
  hipserve::launch_qk_rmsnorm(qp, qkv.stride(0), qw, kw, qkv.size(0), nq, nkv, head_dim, (float)eps, cur_stream());
}

void sample(at::Tensor& out_tok, at::Tensor& out_lp, const at::Tensor& logits,
            const at::Tensor& temperature, const at::Tensor& top_k, const at::Tensor& top_p,
            const at::Tensor& seeds, const at::Tensor& steps, bool two_rounds,
            const c10::optional<at::Tensor>& min_p) {
  Args a("sample", logits, "logits");
  const Logits L = logits_rows(a, logits);
  const int rows = L.rows;
  int64_t* tok = a.as<int64_t>(out_tok, "out_tok", CONTIG, rows);
  float* lp = a.as_if<float>(out_lp, "out_lp", CONTIG, out_lp.numel() > 0 ? rows : 0);
  const float* temp = a.as<float>(temperature, "temperature", CONTIG, rows);
  const int* tk = a.as<int>(top_k, "top_k", CONTIG, rows);
  const float* tpp = a.as<float>(top_p, "top_p", CONTIG, rows);
  const int64_t* sd = a.as<int64_t>(seeds, "seeds", CONTIG, rows);
  const int64_t* st = a.as<int64_t>(steps, "steps", CONTIG, rows);
  const float* minp = maybe(min_p).defined() ? a.as<float>(*min_p, "min_p", CONTIG, rows) : nullptr;
  // multi-CU sampler workspace (caching allocator: graph-capturable)
  const size_t wsn = hipserve::sample_workspace_floats(rows, L.V);
  at::Tensor ws;
  if (wsn) ws = at::empty({(long)wsn}, logits.options().dtype(at::kFloat));
  hipserve::launch_sample(tok, lp, L.p, L.bf16, L.stride, rows, L.V, temp, tk, tpp, sd, st,
                          wsn ? a.as<float>(ws, "workspace", CONTIG) : nullptr, cur_stream(), two_rounds, minp);
}

void gguf_gemm(at::Tensor& out, const at::Tensor& x, const at::Tensor& q, const at::Tensor& d,
               const at::Tensor& mn, int64_t qtype, int64_t row_bytes, int64_t N, int64_t K,
               at::Tensor& ws, int64_t splits) {
  Args a("gguf_gemm", x, "x");
  TORCH_CHECK(K > 0 && K % 256 == 0, "gguf_gemm: K must be a multiple of 256");
  TORCH_CHECK(qtype >= 0 && qtype <= 6, "gguf_gemm: qtype 0..6");
  const void* xp = a.ptr(x, "x", BF16, ROWS8, {ANY, at_least(K)});
  const int M = x.size(0);
  TORCH_CHECK(M <= 64, "gguf_gemm handles M <= 64 (use gguf_dequant + GEMM above)");
  void* op = a.ptr(out, "out", BF16, ROWS, {M, at_least(N)});
  const void* qp = a.ptr(q, "q", U8, CONTIG);
  // SoA f16 scales / mins (as int16 bits) of the Q4_0 / Q4_1 / Q8_0 layouts
  const void* dp = a.ptr_if(d, "d (SoA scales)", I16 | F16, CONTIG, qtype <= 2 ? N * (K / 32) : 0);
  const void* mp = a.ptr_if(mn, "m (SoA mins)", I16 | F16, CONTIG, qtype == 1 ? N * (K / 32) : 0);
  // split-K: one fp32 slab per K slice
  float* wp = splits > 1 ? splitk_ws(a, ws, splits, M, N) : nullptr;
  hipserve::launch_gguf_gemm(op, wp, xp, x.stride(0), out.stride(0), qp, dp, mp, qtype, row_bytes, M, N, K, splits,
                             cur_stream());
}

// parts in the tiled layout (one uint8 tensor [N/16, K/256, chunk] each), their
// formats / rows / output columns. ws.numel() > 0: fp32 partials [S_actual, M, Ntot]
// (returned S_actual = ceil(nsb / ceil(nsb / S))); else bf16 out [M, >= Ntot], S == 1.
int64_t gguf_gemm_parts(at::Tensor& out, at::Tensor& ws, const at::Tensor& x, const std::vector<at::Tensor>& qs,
                        const std::vector<at::Tensor>& rss, const std::vector<int64_t>& qtypes, const std::vector<int64_t>& rows,
                        const std::vector<int64_t>& cols, int64_t Ntot, int64_t K, int64_t splits,
                        const c10::optional<at::Tensor>& x16) {
  Args a("gguf_gemm_parts", x, "x");
  TORCH_CHECK(K > 0 && K % 256 == 0 && splits >= 1, "gguf_gemm_parts: K % 256 == 0, splits >= 1");
  const void* xp = a.ptr(x, "x", BF16, ROWS8, {ANY, at_least(K)});
  const int M = x.size(0);
  TORCH_CHECK(M >= 1, "gguf_gemm_parts: M >= 1 (M > 64 sweeps 64-row tiles)");
  const int nsb = K / 256;
  const int per = (nsb + splits - 1) / splits;
  const int S = (nsb + per - 1) / per;
  hipserve::GgufPart P[4];
  TORCH_CHECK(tiled_parts(a, qs, &rss, qtypes, rows, cols, K, P) <= Ntot, "gguf_gemm_parts: parts must lie inside Ntot");
  const GemmOut o = partials_or_out(a, out, ws, S, M, Ntot, Ntot);
  // f16 pair-order copy of x from the producer (M <= 64)
  const void* x16p = f16_twin(a, x16, "x16", x, at_least(K));
  hipserve::launch_gguf_gemm_parts(o.out, o.stride, o.ws, xp, x.stride(0), P, (int)qs.size(), M, Ntot, K, splits,
                                   cur_stream(), x16p);
  return S;
}

// x [M, >= K] bf16 -> x16 [M, K] f16 in the GGUF kernels' pair order, each row scaled by
// 1 / rsc[m] (a power of two keeping it in the f16 range): the prefill GEMM's operand
void x_f16_pairs(at::Tensor& x16, at::Tensor& rsc, const at::Tensor& x) {
  Args a("x_f16_pairs", x, "x");
  const void* xp = a.ptr(x, "x", BF16, ROWS8, {ANY, ANY});
  const int M = x.size(0);
  void* x16p = a.ptr(x16, "x16", F16, CONTIG, {M, ANY});
  const int K = x16.size(1);
  TORCH_CHECK(K % 8 == 0 && x.size(1) >= K, "x_f16_pairs: x16 [M, K], K % 8, x rows of >= K");
  float* rp = a.as<float>(rsc, "rsc", CONTIG, M);
  if (M == 0) return;
  hipserve::launch_x_f16_pairs(x16p, rp, xp, x.stride(0), M, K, cur_stream());
}

// prefill GEMM on the tiled GGUF parts (gguf_mfma.hip qpg_kernel) over x16 / rsc from
// x_f16_pairs: epi 0 store at each part's column, 1 residual add (out += x . W^T, in
// place), 2 / 3 SiLU / GELU GLU of parts 0 (gate) and 1 (up) into out[M, rows]. Returns
// false when the kernel does not take it.
bool gguf_prefill(at::Tensor& out, const at::Tensor& x16, const at::Tensor& rsc, const std::vector<at::Tensor>& qs,
                  const std::vector<int64_t>& qtypes, const std::vector<int64_t>& rows, const std::vector<int64_t>& cols,
                  int64_t K, int64_t epi) {
  Args a("gguf_prefill", x16, "x16");
  TORCH_CHECK(K > 0 && K % 256 == 0, "gguf_prefill: K % 256 == 0");
  const void* xp = a.ptr(x16, "x16 (x_f16_pairs)", F16, CONTIG, {ANY, K});
  const int M = x16.size(0);
  const float* rp = a.as<float>(rsc, "rsc", CONTIG, M);
  // (a format without a prefill body is no error: the launcher returns false)
  hipserve::GgufPart P[4];
  const long ncols = tiled_parts(a, qs, nullptr, qtypes, rows, cols, K, P);
  const bool glu = epi == 2 || epi == 3;
  void* op = a.ptr(out, "out", BF16, ROWS4, {M, at_least(glu ? rows[0] : ncols)});
  if (M == 0) return true;
  return hipserve::launch_gguf_prefill((int)epi, op, out.stride(0), xp, rp, P, (int)qs.size(), M, (int)K, cur_stream());
}

int64_t qmoe_gemm(at::Tensor& out, at::Tensor& ws, const at::Tensor& x, const at::Tensor& q, const at::Tensor& rs,
                  int64_t qtype, int64_t N, int64_t K, const at::Tensor& slots, const at::Tensor& tile_expert,
                  int64_t tile, int64_t gather_k, int64_t splits, bool kmajor, int64_t glu) {
  Args a("qmoe_gemm", x, "x");
  const QuantFormat f = tiled_format(qtype, "qmoe_gemm", true);
  TORCH_CHECK(tile == 16 || tile == 32 || tile == 64, "qmoe_gemm: tile 16/32/64");
  TORCH_CHECK(N > 0 && N % 16 == 0 && K > 0 && K % 256 == 0 && splits >= 1, "qmoe_gemm: N % 16, K % 256, splits >= 1");
  const void* xp = a.ptr(x, "x", BF16, ROWS8, {ANY, at_least(K)});
  const MoeTiles t = moe_tiles(a, slots, tile_expert, tile);
  TORCH_CHECK(t.nslots == (long)t.tiles_cap * tile, "qmoe_gemm: int32 slots [tiles * tile] and tile_expert [tiles]");
  const long per_e = N / 16 * (K / 256) * f.chunk_bytes;
  const void* qp = a.ptr(q, "q (uint8 [E, tiled [N/16, K/256, chunk] expert])", U8, CONTIG, {ANY, per_e});
  const bool fp8 = f.row_scaled;  // FP8, INT8C: the other expert formats carry their scales in the chunks
  const float* rsp = fp8 ? a.as<float>(rs, "rs (FP8 / INT8C experts)", CONTIG, {q.size(0), N}) : nullptr;
  TORCH_CHECK(gather_k > 0 || x.size(0) >= t.nslots, "qmoe_gemm: slot-indexed x needs a row per slot");
  const int nsb = K / 256;
  const int per = (nsb + splits - 1) / splits;
  const int S = (nsb + per - 1) / per;
  const GemmOut o = partials_or_out(a, out, ws, S, t.nslots, N, glu ? N / 2 : N);
  TORCH_CHECK(hipserve::launch_qmoe_gemm(o.out, o.stride, o.ws, xp, x.stride(0), qp, rsp, qtype, per_e, fp8 ? N : 0,
                                         t.slots, t.tile_expert, t.tiles_cap, tile, gather_k, N, K, splits,
                                         cur_stream(), kmajor, (int)glu),
              "qmoe_gemm: unsupported configuration");
  return S;
}

// pack 0: out row-major [N, K]; 1 / 2: the stacked matrices of `nrows` rows each (N = E nrows)
// in the pack_decode_weight layout (2: gate/up-interleaved), E copies back to back
void gguf_dequant_tiled(at::Tensor& out, const at::Tensor& q, const at::Tensor& rs, int64_t qtype, int64_t N,
                        int64_t K, int64_t pack, int64_t nrows, bool kmajor) {
  Args a("gguf_dequant_tiled", q, "q");
  TORCH_CHECK(N > 0 && N % 16 == 0 && K > 0 && K % 256 == 0, "gguf_dequant_tiled: N % 16, K % 256");
  TORCH_CHECK(pack >= 0 && pack <= 2, "gguf_dequant_tiled: pack 0, 1 or 2");
  int64_t out_numel = N * K;
  if (pack != 0) {
    TORCH_CHECK(nrows > 0 && nrows % 16 == 0 && N % nrows == 0 && (pack == 1 || nrows % 128 == 0),
                "gguf_dequant_tiled: packed matrices of nrows rows (glu: nrows % 128 == 0)");
    out_numel = N / nrows * ((nrows + 127) / 128 * 128) * K;
  }
  void* op = a.ptr(out, "out", BF16, CONTIG, out_numel);
  const QuantFormat f = tiled_format(qtype, "gguf_dequant_tiled");
  const void* qp = a.ptr(q, "q (a tiled tensor of its format)", U8, CONTIG, exactly(N / 16 * (K / 256) * f.chunk_bytes));
  TORCH_CHECK(!kmajor || nrows <= 0 || (nrows % 16 == 0 && N % nrows == 0), "gguf_dequant_tiled: k-major matrices of nrows rows");
  const float* rsp = f.row_scaled ? a.as<float>(rs, "rs (FP8 / INT8C row scale)", CONTIG, exactly(N)) : nullptr;
  hipserve::launch_gguf_dequant_tiled(op, qp, rsp, qtype, N, K, cur_stream(), (int)pack, (int)nrows, kmajor);
}

// per-channel FP8 tiled part q [N/16, K/256, 4096] -> out: row-major [N, K] e4m3 bytes
void fp8_untile(at::Tensor& out, const at::Tensor& q, int64_t N, int64_t K) {
  Args a("fp8_untile", q, "q");
  TORCH_CHECK(N % 16 == 0 && K % 256 == 0, "fp8_untile: N % 16, K % 256");
  const void* qp = a.ptr(q, "q (a tiled FP8 part of N x K)", U8, CONTIG, exactly(N * K));
  void* op = a.ptr(out, "out ([N, K] bytes)", BYTES, CONTIG, exactly(N * K));
  TORCH_CHECK(reinterpret_cast<uintptr_t>(op) % 16 == 0, "fp8_untile: 16-byte aligned out");
  hipserve::launch_fp8_untile(op, qp, (int)N, (int)K, cur_stream());
}

void gguf_dequant(at::Tensor& out, const at::Tensor& q, const at::Tensor& d, const at::Tensor& mn,
                  int64_t qtype, int64_t row_bytes, int64_t N, int64_t K) {
  Args a("gguf_dequant", q, "q");
  TORCH_CHECK(K % 256 == 0 && qtype >= 0 && qtype <= 5, "gguf_dequant: K % 256 == 0, qtype 0..5");
  void* op = a.ptr(out, "out", BF16, CONTIG, N * K);
  const void* qp = a.ptr(q, "q", U8, CONTIG);
  const void* dp = a.ptr_if(d, "d (SoA scales)", I16 | F16, CONTIG);
  const void* mp = a.ptr_if(mn, "m (SoA mins)", I16 | F16, CONTIG);
  hipserve::launch_gguf_dequant(op, qp, dp, mp, qtype, row_bytes, N, K, cur_stream());
}

void skinny_gemm(at::Tensor& out, const at::Tensor& x, const at::Tensor& w, int64_t rt, int64_t kw) {
  Args a("skinny_gemm", x, "x");
  const void* xp = a.ptr(x, "x", BF16, ROWS8, {ANY, ANY});
  const int M = x.size(0), K = x.size(1);
  const void* wp = a.ptr(w, "w", BF16, CONTIG, {ANY, K});
  const int N = w.size(0);
  void* op = a.ptr(out, "out", BF16, ROWS, {M, at_least(N)});
  TORCH_CHECK(M >= 1 && M <= 64, "skinny_gemm: 1 <= M <= 64");
  TORCH_CHECK(kw >= 1 && K % (256 * kw) == 0, "skinny_gemm: K must be a multiple of 256*kw");
  TORCH_CHECK(hipserve::launch_skinny_gemm(op, xp, x.stride(0), wp, out.stride(0), M, N, K, rt, kw, cur_stream()),
              "skinny_gemm: unsupported (rt, kw)");
}

// splits > 0: logits = the router decode GEMM's fp32 split-K partials, flat [splits, T, E]
// with T = w.size(0) (summed in order and rounded to bf16 in the kernel: no reduce launch)
void moe_topk_softmax(at::Tensor& w, at::Tensor& ids, const at::Tensor& logits, int64_t k, bool renorm,
                      int64_t splits) {
  Args a("moe_topk_softmax", logits, "logits");
  unsigned which;
  const void* lp = a.ptr(logits, "logits", splits > 0 ? F32 : F32 | BF16, CONTIG, {}, &which);
  int T, E;
  if (splits > 0) {
    TORCH_CHECK(w.dim() == 2, "moe_topk_softmax: fp32 partials, w [T, k]");
    T = w.size(0);
    TORCH_CHECK(T > 0 && logits.numel() % (splits * T) == 0, "moe_topk_softmax: partials [splits, T, E]");
    E = logits.numel() / (splits * T);
  } else {
    TORCH_CHECK(logits.dim() == 2, "moe_topk_softmax: logits [T, E]");
    T = logits.size(0);
    E = logits.size(1);
  }
  TORCH_CHECK(E <= 128, "moe_topk_softmax: <= 128 experts");
  TORCH_CHECK(k >= 1 && k <= E, "moe_topk_softmax: 1 <= k <= E");
  float* wp = a.as<float>(w, "w", CONTIG, T * k);
  int* ip = a.as<int>(ids, "ids", CONTIG, T * k);
  hipserve::launch_moe_topk_softmax(lp, which == F32, wp, ip, T, E, k, renorm, cur_stream(), (int)splits);
}

// custom all-reduce control ops carry an opaque state handle: catch-all kernels
int64_t car_create(int64_t rank, int64_t world, int64_t max_bytes, int64_t nb_large) {
  return reinterpret_cast<int64_t>(hipserve::car_create((int)rank, (int)world, (size_t)max_bytes, (int)nb_large));
}

at::Tensor car_handle(int64_t state) {
  auto t = at::empty({64}, at::TensorOptions().dtype(at::kByte));
  hipserve::car_get_handle(reinterpret_cast<void*>(state), t.data_ptr());
  return t;
}

void car_open(int64_t state, int64_t peer, const at::Tensor& handle) {
  TORCH_CHECK(handle.device().is_cpu() && handle.numel() == 64 && handle.scalar_type() == at::kByte);
  auto h = handle.contiguous();
  hipserve::car_open(reinterpret_cast<void*>(state), (int)peer, h.data_ptr());
}

bool car_norm_fits(int64_t state, int64_t M, int64_t N, bool exch_f32) {
  return hipserve::car_norm_fits(reinterpret_cast<void*>(state), (int)M, (int)N, exch_f32);
}

bool car_error(int64_t state) { return hipserve::car_error(reinterpret_cast<void*>(state)); }

void car_destroy(int64_t state) { hipserve::car_destroy(reinterpret_cast<void*>(state)); }

void car_all_reduce(int64_t state, const at::Tensor& inp, at::Tensor& out, bool two_shot) {
  Args a("car_all_reduce", inp, "inp");
  const void* ip = a.ptr(inp, "inp", BF16, CONTIG);
  void* op = a.ptr(out, "out", BF16, CONTIG, exactly(inp.numel()));
  const size_t bytes = inp.numel() * 2;
  TORCH_CHECK(bytes % 16 == 0 && bytes <= hipserve::car_max_bytes(reinterpret_cast<void*>(state)),
              "car_all_reduce: size must be a multiple of 16 B and fit the registered buffer");
  hipserve::launch_car(reinterpret_cast<void*>(state), ip, op, bytes, two_shot, 0, cur_stream());
}

// [rows, cols] -> [rows, world * cols]
void car_all_gather(int64_t state, const at::Tensor& inp, at::Tensor& out) {
  Args a("car_all_gather", inp, "inp");
  unsigned which;  // out has inp's dtype
  const void* ip = a.ptr(inp, "inp", ANYTYPE & ~OTHER, CONTIG, {ANY, ANY}, &which);
  void* op = a.ptr(out, "out", which, CONTIG, {inp.size(0), ANY});
  TORCH_CHECK(inp.size(1) > 0 ? out.size(1) % inp.size(1) == 0 : out.size(1) == 0,
              "car_all_gather: out columns must be world * in columns");
  const size_t row = inp.size(1) * inp.element_size();
  const size_t bytes = row * inp.size(0);
  TORCH_CHECK(bytes <= hipserve::car_max_bytes(reinterpret_cast<void*>(state)), "car_all_gather: shard too large");
  if (bytes == 0) return;
  hipserve::launch_car_all_gather(reinterpret_cast<void*>(state), ip, op, bytes, row, cur_stream());
}

void car_add_rmsnorm(int64_t state, at::Tensor& out, at::Tensor& residual, const at::Tensor& x, int64_t splits,
                     const at::Tensor& weight, double eps, bool exch_f32) {
  Args a("car_add_rmsnorm", x, "x");
  void* rp = a.ptr(residual, "residual", BF16, CONTIG, {ANY, ANY});
  const int M = residual.size(0), N = residual.size(1);
  void* op = a.ptr(out, "out", BF16, CONTIG, {M, N});
  TORCH_CHECK(splits >= 1, "car_add_rmsnorm: splits >= 1");
  unsigned which;  // fp32 partials [splits, M, N], or bf16 [M, N]
  const void* xp = a.ptr(x, "x", F32 | BF16, CONTIG, exactly(splits * (int64_t)M * N), &which);
  TORCH_CHECK(which == F32 || splits == 1, "car_add_rmsnorm: bf16 input has one slice");
  const NormWeight w = norm_weight(a, weight, "weight", N);
  TORCH_CHECK(hipserve::car_norm_fits(reinterpret_cast<void*>(state), M, N, exch_f32),
              "car_add_rmsnorm: N must divide into 8-wide chunks per rank and the message fit the buffer");
  if (M == 0) return;
  hipserve::launch_car_add_rmsnorm(reinterpret_cast<void*>(state), op, rp, xp, which == F32, (int)splits, w.p, w.f32, M,
                                   N, (float)eps, exch_f32, cur_stream());
}

void penalty_apply(at::Tensor& logits, const at::Tensor& slot, const at::Tensor& pres, const at::Tensor& freq,
                   const at::Tensor& rep, const at::Tensor& counts, const at::Tensor& seen) {
  Args a("penalty_apply", logits, "logits");
  const Logits L = logits_rows(a, logits);
  const PenState p = pen_state(a, counts, seen);
  TORCH_CHECK(p.V == L.V, "penalty_apply: counts must be int32 [slots, V] of the logits' V");
  hipserve::launch_penalty_apply(L.p, L.bf16, L.stride, L.rows, L.V, a.as<int>(slot, "slot", CONTIG, L.rows),
                                 a.as<float>(pres, "pres", CONTIG, L.rows), a.as<float>(freq, "freq", CONTIG, L.rows),
                                 a.as<float>(rep, "rep", CONTIG, L.rows), p.counts, p.seen, cur_stream());
}

// logits[:, :V] = cap * tanh(logits / cap) in place (Gemma-2 final logit soft-capping)
void logit_softcap_(at::Tensor& logits, double cap) {
  Args a("logit_softcap_", logits, "logits");
  const Logits L = logits_rows(a, logits);
  TORCH_CHECK(cap > 0, "logit_softcap_: cap > 0");
  hipserve::launch_logit_softcap(L.p, L.bf16, L.stride, L.rows, L.V, (float)cap, cur_stream());
}

void logit_bias_apply(at::Tensor& logits, const at::Tensor& slot, const at::Tensor& ids, const at::Tensor& vals,
                      const at::Tensor& n) {
  Args a("logit_bias_apply", logits, "logits");
  const Logits L = logits_rows(a, logits);
  const int* sp = a.as<int>(slot, "slot", CONTIG, L.rows);
  const int* ip = a.as<int>(ids, "ids", CONTIG, {ANY, ANY});  // [slots, width]
  const float* vp = a.as<float>(vals, "vals", CONTIG, {ids.size(0), ids.size(1)});
  const int* np = a.as<int>(n, "n", CONTIG, exactly(ids.size(0)));
  hipserve::launch_logit_bias_apply(L.p, L.bf16, L.stride, L.rows, L.V, sp, ip, vp, np, ids.size(0), ids.size(1),
                                    cur_stream());
}

void penalty_update(const at::Tensor& tok, const at::Tensor& slot, at::Tensor& counts, at::Tensor& seen) {
  Args a("penalty_update", tok, "tok");
  const int64_t* tp = a.as<int64_t>(tok, "tok", CONTIG);
  const int* sp = a.as<int>(slot, "slot", CONTIG, tok.numel());
  const PenState p = pen_state(a, counts, seen);
  hipserve::launch_penalty_update(tp, sp, tok.numel(), p.counts, p.seen, p.V, cur_stream());
}

void penalty_init(at::Tensor& counts, at::Tensor& seen, const at::Tensor& slots, const at::Tensor& off,
                  const at::Tensor& n_prompt, const at::Tensor& toks) {
  Args a("penalty_init", counts, "counts");
  const PenState p = pen_state(a, counts, seen);
  const int* sp = a.as<int>(slots, "slots", CONTIG);
  const int n = slots.numel();
  hipserve::launch_penalty_init(p.counts, p.seen, p.V, sp, a.as<int>(off, "off", CONTIG, exactly(n + 1)),
                                a.as<int>(n_prompt, "n_prompt", CONTIG, exactly(n)), a.as<int>(toks, "toks", CONTIG), n,
                                cur_stream());
}

void top_logprobs(const at::Tensor& logits, const at::Tensor& nreq, at::Tensor& out_ids, at::Tensor& out_lp) {
  Args a("top_logprobs", logits, "logits");
  const Logits L = logits_rows(a, logits);
  const int* np = a.as<int>(nreq, "nreq", CONTIG, L.rows);
  int* ip = a.as<int>(out_ids, "out_ids", CONTIG, {at_least(L.rows), ANY});
  TORCH_CHECK(out_ids.size(1) <= 64, "top_logprobs: at most 64 per row");
  float* lp = a.as<float>(out_lp, "out_lp", CONTIG, {out_ids.size(0), out_ids.size(1)});
  hipserve::launch_top_logprobs(L.p, L.bf16, L.stride, L.rows, L.V, np, ip, lp, out_ids.size(1), cur_stream());
}

// per logits row: log-prob and rank of targets[row], and the nreq[row] largest log-probs
void prompt_logprobs(const at::Tensor& logits, const at::Tensor& targets, const at::Tensor& nreq, at::Tensor& out_lp,
                     at::Tensor& out_rank, at::Tensor& out_ids, at::Tensor& out_top) {
  Args a("prompt_logprobs", logits, "logits");
  const Logits L = logits_rows(a, logits);
  const int* tp = a.as<int>(targets, "targets", CONTIG, exactly(L.rows));
  const int* np = a.as<int>(nreq, "nreq", CONTIG, exactly(L.rows));
  float* lp = a.as<float>(out_lp, "out_lp", CONTIG, exactly(L.rows));
  int* rp = a.as<int>(out_rank, "out_rank", CONTIG, exactly(L.rows));
  int* ip = a.as<int>(out_ids, "out_ids", CONTIG, {L.rows, ANY});
  TORCH_CHECK(out_ids.size(1) <= 20, "prompt_logprobs: out_ids must have at most 20 per row, got ", out_ids.size(1));
  float* vp = a.as<float>(out_top, "out_top", CONTIG, {L.rows, out_ids.size(1)});
  hipserve::launch_prompt_logprobs(L.p, L.bf16, L.stride, L.rows, L.V, tp, np, lp, rp, ip, vp, out_ids.size(1),
                                   cur_stream());
}

void fill_uniform(at::Tensor& out, int64_t row0, int64_t col0, int64_t gcols, int64_t key, double scale) {
  Args a("fill_uniform", out, "out");
  void* op = a.ptr(out, "out", BF16, ROWS, {ANY, ANY});
  hipserve::launch_fill_uniform(op, out.stride(0), out.size(0), out.size(1), row0, col0, gcols,
                                (unsigned int)(key & 0xffffffffu), (float)scale, cur_stream());
}

// Pinned host tensors are addressed through their device mapping; every pair must
// match in byte size (a multiple of 4) and be contiguous. Runs on `device`'s
// current stream.
void stage_copy(const std::vector<at::Tensor>& dst, const std::vector<at::Tensor>& src, int64_t device) {
  TORCH_CHECK(dst.size() == src.size() && dst.size() <= (size_t)hipserve::kMaxStageCopies,
              "stage_copy: matching lists of at most 8 tensors");
  hipserve::StageCopyArgs a{};
  a.n = (int)dst.size();
  auto addr = [](const at::Tensor& t, bool& host) -> void* {
    TORCH_CHECK(t.is_contiguous(), "stage_copy: tensors must be contiguous");
    if (t.is_cuda()) { host = false; return t.data_ptr(); }
    TORCH_CHECK(t.is_pinned(), "stage_copy: host tensors must be pinned");
    host = true;
    void* d = nullptr;
    TORCH_CHECK(hipHostGetDevicePointer(&d, t.data_ptr(), 0) == hipSuccess && d,
                "stage_copy: pinned tensor has no device mapping");
    return d;
  };
  for (int i = 0; i < a.n; ++i) {
    const size_t nb = dst[i].nbytes();
    TORCH_CHECK(nb == src[i].nbytes() && nb % 4 == 0, "stage_copy: pair ", i, " byte sizes differ or not 4-aligned");
    bool hd = false, hs = false;
    a.dst[i] = addr(dst[i], hd);
    a.src[i] = addr(src[i], hs);
    a.words[i] = (long)(nb / 4);
    a.host_mask |= (hs ? 1u : 0u) << (2 * i);
    a.host_mask |= (hd ? 1u : 0u) << (2 * i + 1);
  }
  c10::hip::HIPGuardMasqueradingAsCUDA g((c10::DeviceIndex)device);
  hipserve::launch_stage_copy(a, cur_stream());
}

// out [M, N] = x . w^T; w row-major [N, K] (N < 0: taken from it), or packed =
// pack_decode_weight(w[N, K]) (flat, ceil(N/128)*128*K bf16)
void decode_gemm_op(const char* name, at::Tensor& out, const at::Tensor& x, const at::Tensor& w, at::Tensor& ws,
                    int64_t N, int64_t rt, int64_t splits, bool packed) {
  Args a(name, x, "x");
  const DecodeX X = decode_gemm_x(a, x, splits);
  const void* wp = packed ? a.ptr(w, "wp (pack_decode_weight)", BF16, CONTIG, exactly((N + 127) / 128 * 128 * X.K))
                          : a.ptr(w, "w", BF16, CONTIG, {ANY, X.K});
  if (!packed) N = w.size(0);
  void* op = a.ptr(out, "out", BF16, ROWS4, {X.M, N});
  TORCH_CHECK(N % 4 == 0 && (splits == 1 || N % 8 == 0), name, ": N % 4 == 0 (split-K: N % 8 == 0)");
  float* wsp = splits > 1 ? splitk_ws(a, ws, splits, X.M, N) : nullptr;
  TORCH_CHECK(hipserve::launch_decode_gemm(op, out.stride(0), wsp, X.p, X.stride, wp, X.M, N, X.K, rt, splits, packed,
                                           0, cur_stream()),
              name, ": unsupported (rt, K/splits): rt in {1,2}, K/splits = 256*{1,2,4,7,8,12,16,21}");
}
void decode_gemm(at::Tensor& out, const at::Tensor& x, const at::Tensor& w, at::Tensor& ws, int64_t rt,
                 int64_t splits) {
  decode_gemm_op("decode_gemm", out, x, w, ws, -1, rt, splits, false);
}
void decode_gemm_packed(at::Tensor& out, const at::Tensor& x, const at::Tensor& wp, at::Tensor& ws, int64_t N,
                        int64_t rt, int64_t splits) {
  decode_gemm_op("decode_gemm_packed", out, x, wp, ws, N, rt, splits, true);
}

// Decode GEMM writing fp32 split-K partials ws[S, M, N] for a fused epilogue
// (splitk_add_rmsnorm / splitk_rope_cache).
void decode_gemm_partial(at::Tensor& ws, const at::Tensor& x, const at::Tensor& w, int64_t N, int64_t rt,
                         int64_t splits, bool packed) {
  Args a("decode_gemm_partial", x, "x");
  const DecodeX X = decode_gemm_x(a, x, splits);
  TORCH_CHECK(N % 8 == 0, "decode_gemm_partial: N % 8 == 0");
  const void* wp = packed ? a.ptr(w, "w (pack_decode_weight)", BF16, CONTIG, exactly((N + 127) / 128 * 128 * X.K))
                          : a.ptr(w, "w", BF16, CONTIG, {N, X.K});
  float* wsp = splitk_ws(a, ws, splits, X.M, N);
  TORCH_CHECK(hipserve::launch_decode_gemm(nullptr, N, wsp, X.p, X.stride, wp, X.M, N, X.K, rt, splits, packed,
                                           hipserve::DG_PARTIAL, cur_stream()),
              "decode_gemm_partial: unsupported (rt, K/splits)");
}

// Merged gate|up decode GEMM with the SiLU-GLU fused: act[M, N/2] = silu(x Wg^T) * (x Wu^T),
// wp = pack_decode_weight(w, glu=true). splits > 1 needs ws of S*M*N fp32.
void decode_gemm_glu(at::Tensor& act, const at::Tensor& x, const at::Tensor& wp, at::Tensor& ws, int64_t N,
                     int64_t rt, int64_t splits) {
  Args a("decode_gemm_glu", x, "x");
  const DecodeX X = decode_gemm_x(a, x, splits);
  TORCH_CHECK(N % 128 == 0, "decode_gemm_glu: N % 128 == 0");
  const void* wpp = a.ptr(wp, "wp (pack_decode_weight, glu)", BF16, CONTIG, exactly(N * X.K));
  void* ap = a.ptr(act, "act", BF16, ROWS8, {X.M, N / 2});
  float* wsp = splits > 1 ? splitk_ws(a, ws, splits, X.M, N) : nullptr;
  TORCH_CHECK(hipserve::launch_decode_gemm(ap, act.stride(0), wsp, X.p, X.stride, wpp, X.M, N, X.K, rt, splits, true,
                                           hipserve::DG_GLU, cur_stream()),
              "decode_gemm_glu: unsupported (rt, K/splits)");
}

// Prefill GEMM over the packed decode layout (prefill_gemm_packed.hip): wp =
// pack_decode_weight(w[N, K], glu) (flat, ceil(N/128)*128*K bf16). epi as the FP8 prefill GEMM (PG_EPI_*)
// (2 / 3 need the glu packing); bias (epi 0 only) bf16 [N] or None; wm 1 or 2.
void prefill_gemm_packed(at::Tensor& out, const at::Tensor& x, const at::Tensor& wp, int64_t N, int64_t epi,
                         const c10::optional<at::Tensor>& bias, int64_t wm, int64_t grid, int64_t rw) {
  Args a("prefill_gemm_packed", x, "x");
  const void* xp = a.ptr(x, "x", BF16, ROWS8, {ANY, ANY});
  const int M = x.size(0), K = x.size(1);
  TORCH_CHECK(K % 256 == 0, "prefill_gemm_packed: K % 256 == 0");
  const void* wpp = a.ptr(wp, "wp (pack_decode_weight)", BF16, CONTIG, exactly((N + 127) / 128 * 128 * K));
  const bool glu = epi == 2 || epi == 3;
  void* op = a.ptr(out, "out", BF16, ROWS4, {M, glu ? N / 2 : N});
  const void* bp = a.ptr_if(maybe(bias), "bias", BF16, CONTIG, exactly(N));
  TORCH_CHECK(hipserve::launch_prefill_gemm_packed((int)epi, op, out.stride(0), xp, x.stride(0), wpp, M, (int)N, K, bp,
                                                   (int)wm, (int)grid, cur_stream(), nullptr, (int)rw),
              "prefill_gemm_packed: unsupported (glu needs N % 128, bias only with epi 0, 32-bit offsets)");
}

// Grouped (MoE prefill experts) form: x = expert-sorted slot rows [cap, K] (moe_align
// with tile 128 * wm + moe_gather), wp = [E, packed expert] (pack_decode_weight per
// expert, glu for w13), tile_expert / num_tiles from moe_align. epi 0 or 2 / 3.
void prefill_gemm_packed_grouped(at::Tensor& out, const at::Tensor& x, const at::Tensor& wp, int64_t N, int64_t epi,
                                 const at::Tensor& tile_expert, const at::Tensor& num_tiles, int64_t wm, int64_t rw,
                                 const c10::optional<at::Tensor>& gather_slots, int64_t gather_k) {
  Args a("prefill_gemm_packed_grouped", x, "x");
  // gather: x holds the token rows and slot row s reads x[gather_slots[s] / gather_k] (moe_align's slots)
  const bool gather = maybe(gather_slots).defined() && gather_slots->numel() > 0;
  const void* xp = a.ptr(x, "x", BF16, gather ? ROWS8 : ROWS, {ANY, ANY});
  const int K = x.size(1);
  TORCH_CHECK(K % 256 == 0 && wm >= 1, "prefill_gemm_packed_grouped: K % 256 == 0, wm >= 1");
  const bool glu = epi == 2 || epi == 3;
  TORCH_CHECK(epi == 0 || glu, "prefill_gemm_packed_grouped: store or glu epilogue");
  const void* wpp = a.ptr(wp, "wp ([E, packed expert])", BF16, CONTIG, {ANY, (N + 127) / 128 * 128 * K});
  void* op = a.ptr(out, "out", BF16, ROWS, {ANY, glu ? N / 2 : N});
  const int* gp = gather ? a.as<int>(*gather_slots, "gather_slots", CONTIG, exactly(out.size(0))) : nullptr;
  TORCH_CHECK(!gather || gather_k >= 1, "prefill_gemm_packed_grouped: gather_k >= 1");
  const int M = gp ? out.size(0) : x.size(0);
  TORCH_CHECK(out.size(0) == M && M % (128 * wm) == 0, "prefill_gemm_packed_grouped: out rows in 128 * wm tiles");
  hipserve::PwGroup grp{a.as<int>(tile_expert, "tile_expert", CONTIG, M / (128 * wm)),
                        a.as<int>(num_tiles, "num_tiles", CONTIG, 1), (long)wp.size(1)};
  if (gp) {
    grp.gather_slots = gp;
    grp.gather_k = (int)gather_k;
    grp.x_rows = (int)x.size(0);
  }
  TORCH_CHECK(hipserve::launch_prefill_gemm_packed((int)epi, op, out.stride(0), xp, x.stride(0), wpp, M, (int)N, K,
                                                   nullptr, (int)wm, 0, cur_stream(), &grp, (int)rw),
              "prefill_gemm_packed_grouped: unsupported");
}

// FP8 W8A8 form: xq [M, K] uint8 e4m3 + xs [M] fp32 (act_quant_fp8), the weight as
// tiled FP8 parts (ops/quant.py QuantPart.from_fp8: q [N/16, K/256, 4096] uint8 and
// rs [N] fp32) stacked along N. epi 0 / 1 = store / residual add; 2 / 3: parts = (gate, up),
// out = act [M, I] = silu / gelu_tanh(gate) * up.
void prefill_gemm_f8(at::Tensor& out, const at::Tensor& xq, const at::Tensor& xs, const std::vector<at::Tensor>& q,
                     const std::vector<at::Tensor>& rs, int64_t epi) {
  Args a("prefill_gemm_f8", xq, "xq");
  const void* xp = a.ptr(xq, "xq", U8, CONTIG, {ANY, ANY});
  const int M = xq.size(0), K = xq.size(1);
  TORCH_CHECK(K % 256 == 0, "prefill_gemm_f8: K % 256 == 0");
  hipserve::PgF8 W{};
  const int rows = fp8_parts(a, a.as<float>(xs, "xs", CONTIG, exactly(M)), q, rs, K, true, W);
  const bool glu = epi == 2 || epi == 3;
  void* op = a.ptr(out, "out", BF16, ROWS4, {M, glu ? rows / 2 : rows});
  TORCH_CHECK(hipserve::launch_prefill_gemm_f8((int)epi, op, out.stride(0), xp, K, W, M, rows, K, cur_stream()),
              "prefill_gemm_f8: unsupported part shapes (rows % 256; GLU: two equal parts, rows % 128)");
}

// FP8 W8A8 decode form (fp8_decode.hip): fp32 split-K partials ws [S, M, N] of the
// per-token e4m3 activations xq / xs against the tiled FP8 parts, for the fused decode
// epilogues or splitk_reduce.
void fp8_decode_gemm(at::Tensor& ws, const at::Tensor& xq, const at::Tensor& xs, const std::vector<at::Tensor>& q,
                     const std::vector<at::Tensor>& rs, int64_t splits) {
  Args a("fp8_decode_gemm", xq, "xq");
  const void* xp = a.ptr(xq, "xq", U8, CONTIG, {ANY, ANY});
  const int M = xq.size(0), K = xq.size(1);
  TORCH_CHECK(K % 256 == 0 && splits >= 1, "fp8_decode_gemm: K % 256 == 0, splits >= 1");
  hipserve::PgF8 W{};
  const int rows = fp8_parts(a, a.as<float>(xs, "xs", CONTIG, exactly(M)), q, rs, K, false, W);
  float* wsp = splitk_ws(a, ws, splits, M, rows);
  TORCH_CHECK(hipserve::launch_fp8_decode_gemm(wsp, xp, W, M, rows, K, (int)splits, cur_stream()),
              "fp8_decode_gemm: unsupported (M <= 256, part rows % 16, (K / 256) / splits in the kernel's step set)");
}

// [gate | up] rows -> per-token e4m3 act (q8 [rows, I] uint8, xs [rows] fp32), optionally
// the bf16 act too: glu_and_mul -> act_quant_fp8 in one pass
void glu_quant(const c10::optional<at::Tensor>& out, at::Tensor& q8, at::Tensor& xs, const at::Tensor& x, bool gelu) {
  Args a("glu_quant", x, "x");
  const void* xp = a.ptr(x, "x", BF16, ROWS8, {ANY, ANY});
  const long rows = x.size(0);
  const int inter = x.size(1) / 2;
  void* qp = a.ptr(q8, "q8", U8, CONTIG, {rows, inter});
  float* sp = a.as<float>(xs, "xs", CONTIG, exactly(rows));
  void* op = a.ptr_if(maybe(out), "out", BF16, CONTIG, {rows, inter});
  TORCH_CHECK(hipserve::launch_glu_quant(gelu, op, qp, sp, xp, rows, inter, x.stride(0), cur_stream()),
              "glu_quant: I % 8 == 0 and I <= 32768");
}

void act_quant_fp8(at::Tensor& xq, at::Tensor& xs, const at::Tensor& x) {
  Args a("act_quant_fp8", x, "x");
  const void* xp = a.ptr(x, "x", BF16, ROWS8, {ANY, ANY});
  const int M = x.size(0), K = x.size(1);
  TORCH_CHECK(K % 8 == 0, "act_quant_fp8: K % 8 == 0");
  void* qp = a.ptr(xq, "xq", U8, CONTIG, {M, K});
  float* sp = a.as<float>(xs, "xs", CONTIG, exactly(M));
  hipserve::launch_act_quant_fp8(qp, sp, xp, x.stride(0), M, K, cur_stream());
}

void splitk_add_rmsnorm(at::Tensor& out, at::Tensor& residual, const at::Tensor& ws, int64_t splits,
                        const at::Tensor& weight, double eps, const c10::optional<at::Tensor>& out16,
                        const c10::optional<at::Tensor>& out8, const c10::optional<at::Tensor>& xs8) {
  Args a("splitk_add_rmsnorm", ws, "ws");
  void* rp = a.ptr(residual, "residual", BF16, CONTIG, {ANY, ANY});
  const int M = residual.size(0), N = residual.size(1);
  TORCH_CHECK(N % 8 == 0 && N <= 16384, "splitk_add_rmsnorm: N must be a multiple of 8, <= 16384");
  void* op = a.ptr(out, "out", BF16, CONTIG, {M, N});
  const float* wsp = splitk_ws(a, ws, splits, M, N);
  const NormWeight w = norm_weight(a, weight, "weight", N);
  const E4m3Out o8 = e4m3_out_args(a, out8, xs8, out);
  hipserve::launch_splitk_add_rmsnorm(op, rp, wsp, splits, w.p, w.f32, M, N, (float)eps, cur_stream(),
                                      out16_arg(a, out16, out), o8.q, o8.xs);
}

void splitk_post_add_rmsnorm(at::Tensor& out, at::Tensor& residual, const at::Tensor& ws, int64_t splits,
                             const at::Tensor& w_post, const at::Tensor& w_next, double eps,
                             const c10::optional<at::Tensor>& out16, const c10::optional<at::Tensor>& out8,
                             const c10::optional<at::Tensor>& xs8) {
  Args a("splitk_post_add_rmsnorm", ws, "ws");
  void* rp = a.ptr(residual, "residual", BF16, CONTIG, {ANY, ANY});
  const int M = residual.size(0), N = residual.size(1);
  TORCH_CHECK(N % 8 == 0 && N <= 16384, "splitk_post_add_rmsnorm: N must be a multiple of 8, <= 16384");
  void* op = a.ptr(out, "out", BF16, CONTIG, {M, N});
  const float* wsp = splitk_ws(a, ws, splits, M, N);
  const NormWeight wp = norm_weight(a, w_post, "w_post", N), wn = norm_weight(a, w_next, "w_next", N);
  TORCH_CHECK(wp.f32 == wn.f32, "splitk_post_add_rmsnorm: both norm weights bf16 or both fp32 [N]");
  const E4m3Out o8 = e4m3_out_args(a, out8, xs8, out);
  hipserve::launch_splitk_post_add_rmsnorm(op, rp, wsp, splits, wp.p, wn.p, wp.f32, M, N, (float)eps, cur_stream(),
                                           out16_arg(a, out16, out), o8.q, o8.xs);
}

void splitk_rope_cache(at::Tensor& qkv, const at::Tensor& ws, int64_t splits, const at::Tensor& positions,
                       const at::Tensor& slots, const at::Tensor& cos_sin, at::Tensor& k_cache, at::Tensor& v_cache,
                       int64_t nq, int64_t nkv, int64_t head_dim, int64_t mode,
                       const c10::optional<at::Tensor>& bias, const c10::optional<at::Tensor>& q_w,
                       const c10::optional<at::Tensor>& k_w, double eps) {
  Args a("splitk_rope_cache", qkv, "qkv");
  TORCH_CHECK(head_dim > 0 && head_dim % 16 == 0 && (mode == 0 || mode == 1),
              "splitk_rope_cache: head_dim % 16 == 0, mode 0 / 1");
  const long N = (nq + 2 * nkv) * head_dim;
  void* qp = a.ptr(qkv, "qkv", BF16, ROWS, {ANY, at_least(N)});
  const int T = qkv.size(0);
  const void* bp = a.ptr_if(maybe(bias), "bias", BF16, CONTIG, exactly(N));
  const float *qwp, *kwp;
  if (qk_norm_weights(a, q_w, k_w, head_dim, &qwp, &kwp)) {
    const int lanes = (int)head_dim / 16;
    TORCH_CHECK(mode == 0 && (lanes == 4 || lanes == 8 || lanes == 16),
                "splitk_rope_cache: q/k norm needs mode 0, head_dim 64/128/256");
  }
  const float* wsp = splitk_ws(a, ws, splits, T, N);
  const RopeArgs r = rope_args(a, positions, slots, cos_sin, T, head_dim);
  const KvCache kv = kv_cache(a, k_cache, v_cache, nkv, head_dim);
  hipserve::launch_splitk_rope_cache(qp, qkv.stride(0), wsp, splits, r.positions, r.slots, r.cos_sin, kv.k, kv.v, T, nq,
                                     nkv, head_dim, kv.bs, mode, cur_stream(), bp, qwp, kwp, (float)eps, kv.f8);
}

void splitk_reduce(at::Tensor& out, const at::Tensor& ws, int64_t splits) {
  Args a("splitk_reduce", out, "out");
  void* op = a.ptr(out, "out", BF16, ROWS8, {ANY, ANY});
  const int M = out.size(0), N = out.size(1);
  TORCH_CHECK(N % 8 == 0, "splitk_reduce: N % 8 == 0");
  hipserve::launch_splitk_reduce(op, out.stride(0), splitk_ws(a, ws, splits, M, N), M, N, splits, cur_stream());
}

void splitk_glu(at::Tensor& act, const at::Tensor& ws, int64_t splits, bool gelu,
                const c10::optional<at::Tensor>& act16) {
  Args a("splitk_glu", act, "act");
  void* ap = a.ptr(act, "act", BF16, ROWS8, {ANY, ANY});
  const int M = act.size(0), I = act.size(1);
  TORCH_CHECK(I % 8 == 0, "splitk_glu: I % 8 == 0");
  const float* wsp = splitk_ws(a, ws, splits, M, 2L * I);
  hipserve::launch_splitk_glu(ap, act.stride(0), wsp, splits, M, I, gelu, cur_stream(),
                              f16_twin(a, act16, "act16", act, I));
}

// w [N, K], or a stack [E, N, K] (MoE experts: one launch, out = E packed copies back to back)
void pack_decode_weight(at::Tensor& out, const at::Tensor& w, bool glu) {
  Args a("pack_decode_weight", w, "w");
  const void* wp = a.ptr(w, "w", BF16, CONTIG);
  TORCH_CHECK((w.dim() == 2 || w.dim() == 3) && w.size(-1) % 256 == 0,
              "pack_decode_weight: w [N, K] or [E, N, K], K % 256 == 0");
  const long E = w.dim() == 3 ? w.size(0) : 1, N = w.size(-2), K = w.size(-1);
  void* op = a.ptr(out, "out (E*ceil(N/128)*128*K)", BF16, CONTIG, exactly(E * ((N + 127) / 128 * 128 * K)));
  TORCH_CHECK(!glu || N % 128 == 0, "pack_decode_weight: glu packing needs N % 128 == 0");
  TORCH_CHECK(E <= 65535, "pack_decode_weight: at most 65535 stacked matrices");
  hipserve::launch_pack_decode_weight(op, wp, N, K, glu, cur_stream(), (int)E);
}

void moe_align(const at::Tensor& ids, int64_t E, int64_t tile, at::Tensor& slots, at::Tensor& tile_expert,
               at::Tensor& num_tiles, at::Tensor& pair_slot, const c10::optional<at::Tensor>& group_end,
               int64_t expert_lo) {
  Args a("moe_align", ids, "ids");
  TORCH_CHECK(E >= 1 && E <= 128 && expert_lo >= 0 && expert_lo <= (1 << 20) &&
              (tile == 16 || tile == 32 || tile == 64 || tile == 128 || tile == 256), "moe_align: E <= 128, tile 16..256");
  const int* ip = a.as<int>(ids, "ids", CONTIG);
  const int npairs = ids.numel();
  const MoeTiles t = moe_tiles(a, slots, tile_expert, tile);
  TORCH_CHECK(t.nslots >= npairs + E * (tile - 1) && t.nslots % tile == 0,
              "moe_align: slots capacity must cover padding and be a multiple of the tile");
  int* ntp = a.as<int>(num_tiles, "num_tiles", CONTIG, 1);
  int* psp = a.as<int>(pair_slot, "pair_slot", CONTIG, npairs);
  int* ge = a.as_if<int>(maybe(group_end), "group_end", CONTIG,
                         maybe(group_end).defined() && group_end->numel() > 0 ? E : 0);
  const int nb = hipserve::moe_align_blocks(npairs);
  at::Tensor hist;  // multi-workgroup form (prefill): per-block expert histograms
  if (nb > 1) hist = at::empty({(long)nb * 128}, ids.options().dtype(at::kInt));
  hipserve::launch_moe_align(ip, npairs, E, tile, t.slots, t.nslots, t.tile_expert,
                             t.tiles_cap, ntp, psp, ge, cur_stream(), nb > 1 ? a.as<int>(hist, "histogram", CONTIG) : nullptr,
                             (int)expert_lo);
}

void moe_gather(at::Tensor& out, const at::Tensor& x, const at::Tensor& slots, int64_t k) {
  Args a("moe_gather", x, "x");
  const int* sp = a.as<int>(slots, "slots", CONTIG);
  void* op = a.ptr(out, "out", BF16, CONTIG, {at_least(slots.numel()), ANY});
  const int H = out.size(1);
  const void* xp = a.ptr(x, "x", BF16, ROWS8, {ANY, H});
  TORCH_CHECK(H % 8 == 0, "moe_gather: H % 8 == 0");
  hipserve::launch_moe_gather(op, xp, x.stride(0), sp, slots.numel(), k, H, cur_stream());
}

void moe_gemm(at::Tensor& out, const at::Tensor& x, const at::Tensor& w, const at::Tensor& slots,
              const at::Tensor& tile_expert, int64_t tile, int64_t gather_k) {
  Args a("moe_gemm", x, "x");
  const void* wp = a.ptr(w, "w", BF16, CONTIG, {ANY, ANY, ANY});  // [E, N, K]
  const int N = w.size(1), K = w.size(2);
  TORCH_CHECK(K % 256 == 0, "moe_gemm: K % 256 == 0");
  const MoeTiles t = moe_tiles(a, slots, tile_expert, tile);
  const void* xp = a.ptr(x, "x", BF16, ROWS8, {ANY, at_least(K)});
  void* op = a.ptr(out, "out", BF16, ROWS, {at_least(t.nslots), at_least(N)});
  TORCH_CHECK(gather_k > 0 || x.size(0) >= t.nslots, "moe_gemm: ungathered x needs one row per slot");
  hipserve::launch_moe_gemm(op, out.stride(0), xp, x.stride(0), wp, t.slots, t.tile_expert, t.nslots / tile, tile,
                            gather_k, N, K, cur_stream());
}

void moe_combine(at::Tensor& out, const at::Tensor& y, const at::Tensor& w, const at::Tensor& pair_slot,
                 int64_t k) {
  Args a("moe_combine", y, "y");
  void* op = a.ptr(out, "out", BF16, CONTIG, {ANY, ANY});
  const int T = out.size(0), H = out.size(1);
  TORCH_CHECK(H % 8 == 0, "moe_combine: H % 8 == 0");
  const void* yp = a.ptr(y, "y", BF16, CONTIG, {ANY, H});
  const Combine c = combine_args(a, w, pair_slot, T * k);
  hipserve::launch_moe_combine(op, yp, c.w, c.pair_slot, T, k, H, cur_stream());
}

// Expert GEMM over moe_align tiles on the decode GEMM (decode_gemm.hip, kMoe).
// w: [E, ceil(N/128)*128*K] packed (pack_decode_weight per expert; glu = gate/up
// interleaved) or row-major [E, N, K]. out bf16: [slots, N] (glu: act [slots, N/2],
// splits must be 1); out fp32: partials [splits, slots, N] for moe_combine_partial.
void moe_decode_gemm(at::Tensor& out, const at::Tensor& x, const at::Tensor& w, const at::Tensor& slots,
                     const at::Tensor& tile_expert, int64_t tile, int64_t gather_k, int64_t N, int64_t splits,
                     bool packed, bool glu) {
  Args a("moe_decode_gemm", x, "x");
  TORCH_CHECK(tile == 16 || tile == 32 || tile == 64, "moe_decode_gemm: tile in {16, 32, 64}");
  const void* xp = a.ptr(x, "x", BF16, ROWS8, {ANY, ANY});
  const long K = x.size(1);
  TORCH_CHECK(K % 256 == 0 && splits >= 1 && K % (256 * splits) == 0, "moe_decode_gemm: K must be a multiple of 256 * splits");
  const MoeTiles t = moe_tiles(a, slots, tile_expert, tile);
  TORCH_CHECK(t.nslots % tile == 0, "moe_decode_gemm: slots in whole tiles");
  const void* wp = a.ptr(w, "w", BF16, CONTIG);
  TORCH_CHECK(w.dim() >= 2, "moe_decode_gemm: w [E, ...]");
  const long estride = packed ? (N + 127) / 128 * 128 * K : N * K;
  TORCH_CHECK(w.numel() == w.size(0) * estride, "moe_decode_gemm: weight size != E * (packed) N * K");
  TORCH_CHECK(gather_k > 0 || x.size(0) >= t.nslots, "moe_decode_gemm: ungathered x needs one row per slot");
  void* op;
  float* ws = nullptr;
  long out_stride = N;
  if (a.check(out, "out", F32 | BF16, ROWS) == F32) {
    TORCH_CHECK(!glu && N % 4 == 0, "moe_decode_gemm: fp32 partials [splits, slots, N] take no glu, N % 4 == 0");
    op = ws = a.as<float>(out, "out (fp32 partials [splits, slots, N])", CONTIG, splits * t.nslots * N);
    if (out.dim() == 2) out_stride = out.stride(0);
  } else {
    TORCH_CHECK(splits == 1, "moe_decode_gemm: bf16 out [slots, N] (glu: [slots, N/2]) needs splits == 1");
    TORCH_CHECK(!glu || N % 128 == 0, "moe_decode_gemm: glu needs N % 128 == 0");
    op = a.ptr(out, "out", BF16, ROWS4, {at_least(t.nslots), at_least(glu ? N / 2 : N)});
    out_stride = out.stride(0);
  }
  TORCH_CHECK(hipserve::launch_moe_decode_gemm(op, out_stride, ws, xp, x.stride(0), wp, estride, t.slots, t.tile_expert,
                                               t.nslots / tile, tile, gather_k, N, K, splits, packed, glu, cur_stream()),
              "moe_decode_gemm: unsupported K / splits (K / splits / 256 in {1,2,3,4,6,7,8,16}) or glu without packing");
}

void moe_combine_partial(at::Tensor& out, const at::Tensor& ws, const at::Tensor& w, const at::Tensor& pair_slot,
                         int64_t k) {
  Args a("moe_combine_partial", ws, "ws");
  void* op = a.ptr(out, "out", BF16, CONTIG, {ANY, ANY});
  const int T = out.size(0), H = out.size(1);
  TORCH_CHECK(H % 8 == 0, "moe_combine_partial: H % 8 == 0");
  const float* wsp = a.as<float>(ws, "ws", CONTIG, {ANY, ANY, H});  // [S, slots, H]
  const Combine c = combine_args(a, w, pair_slot, T * k);
  hipserve::launch_moe_combine_partial(op, wsp, ws.stride(0), ws.size(0), c.w, c.pair_slot, T, k, H, cur_stream());
}

// moe_combine(_partial) + fused_add_rmsnorm in one launch (decode MoE tail, TP = 1):
// y bf16 [slots, H] (splits 0) or fp32 partials [splits, slots, H]; out = RMSNorm(residual
// += combine) * norm_w
void moe_combine_add_rmsnorm(at::Tensor& out, at::Tensor& residual, const at::Tensor& y, int64_t splits,
                             const at::Tensor& w, const at::Tensor& pair_slot, int64_t k, const at::Tensor& norm_w,
                             double eps) {
  Args a("moe_combine_add_rmsnorm", y, "y");
  void* op = a.ptr(out, "out", BF16, CONTIG, {ANY, ANY});
  const int T = out.size(0), H = out.size(1);
  TORCH_CHECK(H % 8 == 0 && H <= 16384, "moe_combine_add_rmsnorm: H must be a multiple of 8, <= 16384");
  void* rp = a.ptr(residual, "residual", BF16, CONTIG, {T, H});
  const Combine c = combine_args(a, w, pair_slot, T * k);
  const NormWeight nw = norm_weight(a, norm_w, "norm_w", H);
  const void* yp = splits > 0 ? a.ptr(y, "y (fp32 partials [S, slots, H])", F32, CONTIG, {at_least(splits), ANY, H})
                              : a.ptr(y, "y", BF16, CONTIG, {ANY, H});
  const long slab = splits > 0 ? y.stride(0) : 0;
  hipserve::launch_moe_combine_add_rmsnorm(op, rp, yp, slab, (int)splits, c.w, c.pair_slot, T, k, H, nw.p, nw.f32,
                                           (float)eps, cur_stream());
}

// ---- vision tower (vision.hip)
void layernorm(at::Tensor& out, const at::Tensor& x, const at::Tensor& w, const at::Tensor& b,
               const c10::optional<at::Tensor>& residual, double eps) {
  Args a("layernorm", x, "x");
  const void* xp = a.ptr(x, "x", BF16, CONTIG, {ANY, ANY});
  const int rows = x.size(0), C = x.size(1);
  TORCH_CHECK(C % 8 == 0 && C <= 8192, "layernorm: C must be a multiple of 8, <= 8192");
  void* op = a.ptr(out, "out", BF16, CONTIG, {rows, C});
  const void* wp = a.ptr(w, "w", BF16, CONTIG, exactly(C));
  const void* bp = a.ptr(b, "b", BF16, CONTIG, exactly(C));
  void* rp = maybe(residual).defined() ? a.ptr(*residual, "residual", BF16, CONTIG, {rows, C}) : nullptr;
  hipserve::launch_layernorm(op, rp, xp, wp, bp, rows, C, (float)eps, cur_stream());
}

void gelu_(at::Tensor& x, bool tanh_approx) {
  Args a("gelu_", x, "x");
  void* xp = a.ptr(x, "x", BF16, CONTIG);
  TORCH_CHECK(x.numel() % 8 == 0, "gelu_: numel must be a multiple of 8");
  hipserve::launch_gelu(xp, x.numel(), tanh_approx, cur_stream());
}

void vision_attention(at::Tensor& out, at::Tensor& qkv, const c10::optional<at::Tensor>& cos_sin, const at::Tensor& cu,
                      const at::Tensor& tiles, int64_t nh, int64_t D, double scale) {
  Args a("vision_attention", qkv, "qkv");
  TORCH_CHECK(D == 16 || D == 64 || D == 72 || D == 80 || D == 96 || D == 128,
              "vision_attention: head_dim must be one of 16, 64, 72, 80, 96, 128");
  void* qp = a.ptr(qkv, "qkv", BF16, CONTIG, {ANY, 3 * nh * D});
  const int T = qkv.size(0);
  void* op = a.ptr(out, "out", BF16, CONTIG, {T, nh * D});
  // no table: no RoPE (SigLIP)
  const float* cs = cos_sin.has_value() ? a.as<float>(*cos_sin, "cos_sin", CONTIG, {at_least(T), D}) : nullptr;
  const int* cup = a.as<int>(cu, "cu", CONTIG);
  const int* tp = a.as<int>(tiles, "tiles", CONTIG, {ANY, 2});
  hipserve::launch_vision_attention(op, qp, cs, cup, tp, tiles.size(0), T, nh, D, (float)scale, cur_stream());
}

// Gemma-3 projector front: k x k average pool of each image's g x g patch rows + RMSNorm (1 + w)
void vision_pool_rmsnorm(at::Tensor& out, const at::Tensor& x, const at::Tensor& w, int64_t g, int64_t k, double eps) {
  Args a("vision_pool_rmsnorm", x, "x");
  TORCH_CHECK(g > 0 && k > 0 && g % k == 0, "vision_pool_rmsnorm: the pool size k must divide the grid side g");
  const void* xp = a.ptr(x, "x", BF16, CONTIG, {ANY, ANY});
  const int64_t C = x.size(1);
  TORCH_CHECK(C % 8 == 0 && C <= 4096, "vision_pool_rmsnorm: C must be a multiple of 8, <= 4096");
  TORCH_CHECK(x.size(0) % (g * g) == 0, "vision_pool_rmsnorm: x must hold whole images of g * g rows");
  const int64_t images = x.size(0) / (g * g);
  TORCH_CHECK(x.size(0) < (1L << 31), "vision_pool_rmsnorm: too many rows");
  void* op = a.ptr(out, "out", BF16, CONTIG, {images * (g / k) * (g / k), C});
  const void* wp = a.ptr(w, "w", BF16, CONTIG, exactly(C));
  hipserve::launch_vision_pool_rmsnorm(op, xp, wp, (int)images, (int)g, (int)k, (int)C, (float)eps, cur_stream());
}

}  // namespace

// The ops dispatched on the CUDA key: one (name, schema) list for both the definition and
// the implementation.
#define GPU_KEY_OPS(X) \
  X(moe_topk_softmax, "(Tensor(a!) w, Tensor(b!) ids, Tensor logits, int k, bool renorm=True, int splits=0) -> ()") \
  X(moe_combine_add_rmsnorm, "(Tensor(a!) out, Tensor(b!) residual, Tensor y, int splits, Tensor w, Tensor pair_slot, int k, Tensor norm_w, float eps) -> ()") \
  X(moe_align, "(Tensor ids, int E, int tile, Tensor(a!) slots, Tensor(b!) tile_expert, Tensor(c!) num_tiles, Tensor(d!) pair_slot, Tensor(e!)? group_end=None, int expert_lo=0) -> ()") \
  X(moe_gather, "(Tensor(a!) out, Tensor x, Tensor slots, int k) -> ()") \
  X(moe_gemm, "(Tensor(a!) out, Tensor x, Tensor w, Tensor slots, Tensor tile_expert, int tile, int gather_k) -> ()") \
  X(moe_combine, "(Tensor(a!) out, Tensor y, Tensor w, Tensor pair_slot, int k) -> ()") \
  X(moe_decode_gemm, "(Tensor(a!) out, Tensor x, Tensor w, Tensor slots, Tensor tile_expert, int tile, int gather_k, int N, int splits, bool packed, bool glu) -> ()") \
  X(moe_combine_partial, "(Tensor(a!) out, Tensor ws, Tensor w, Tensor pair_slot, int k) -> ()") \
  X(rmsnorm, "(Tensor(a!) out, Tensor x, Tensor weight, float eps, Tensor(b!)? out8=None, Tensor(c!)? xs8=None) -> ()") \
  X(embed_rmsnorm, "(Tensor(a!) out, Tensor(b!) residual, Tensor table, Tensor ids, Tensor? src, Tensor? tok, " \
                   "Tensor weight, float eps, float scale=1.0, Tensor(c!)? out8=None, Tensor(d!)? xs8=None) -> ()") \
  X(fused_add_rmsnorm, "(Tensor(a!) out, Tensor x, Tensor(b!) residual, Tensor weight, float eps, Tensor(c!)? out8=None, Tensor(d!)? xs8=None) -> ()") \
  X(silu_and_mul, "(Tensor(a!) out, Tensor x) -> ()") \
  X(rope_cache, "(Tensor(a!) qkv, Tensor positions, Tensor slots, Tensor cos_sin, Tensor(b!) k_cache, Tensor(c!) v_cache, int nq, int nkv, int head_dim, int mode) -> ()") \
  X(paged_decode, "(Tensor(a!) out, Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_tables, Tensor context_lens, Tensor(b!) tmp_out, Tensor(c!) tmp_ml, int nq, int nkv, int part_size, float scale, int window=0, Tensor(d!)? out16=None, float softcap=0.0) -> ()") \
  X(prefill_attention, "(Tensor(a!) out, Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_tables, Tensor cu_q, Tensor ctx_lens, Tensor tiles, int nq, int nkv, float scale, int window=0, float softcap=0.0, Tensor? limits=None) -> ()") \
  X(qk_rmsnorm, "(Tensor(a!) qkv, Tensor q_w, Tensor k_w, int nq, int nkv, int head_dim, float eps) -> ()") \
  X(gelu_and_mul, "(Tensor(a!) out, Tensor x) -> ()") \
  X(gguf_gemm, "(Tensor(a!) out, Tensor x, Tensor q, Tensor d, Tensor m, int qtype, int row_bytes, int N, int K, Tensor(b!) ws, int splits) -> ()") \
  X(gguf_dequant, "(Tensor(a!) out, Tensor q, Tensor d, Tensor m, int qtype, int row_bytes, int N, int K) -> ()") \
  X(fill_uniform, "(Tensor(a!) out, int row0, int col0, int gcols, int key, float scale) -> ()") \
  X(decode_gemm, "(Tensor(a!) out, Tensor x, Tensor w, Tensor(b!) ws, int rt, int splits) -> ()") \
  X(decode_gemm_packed, "(Tensor(a!) out, Tensor x, Tensor wp, Tensor(b!) ws, int N, int rt, int splits) -> ()") \
  X(pack_decode_weight, "(Tensor(a!) out, Tensor w, bool glu=False) -> ()") \
  X(decode_gemm_partial, "(Tensor(a!) ws, Tensor x, Tensor w, int N, int rt, int splits, bool packed) -> ()") \
  X(decode_gemm_glu, "(Tensor(a!) act, Tensor x, Tensor wp, Tensor(b!) ws, int N, int rt, int splits) -> ()") \
  X(prefill_gemm_packed, "(Tensor(a!) out, Tensor x, Tensor wp, int N, int epi, Tensor? bias=None, int wm=1, int grid=0, int rw=4) -> ()") \
  X(prefill_gemm_packed_grouped, "(Tensor(a!) out, Tensor x, Tensor wp, int N, int epi, Tensor tile_expert, Tensor num_tiles, int wm=1, int rw=4, Tensor? gather_slots=None, int gather_k=1) -> ()") \
  X(prefill_gemm_f8, "(Tensor(a!) out, Tensor xq, Tensor xs, Tensor[] q, Tensor[] rs, int epi) -> ()") \
  X(fp8_decode_gemm, "(Tensor(a!) ws, Tensor xq, Tensor xs, Tensor[] q, Tensor[] rs, int splits) -> ()") \
  X(glu_quant, "(Tensor(a!)? out, Tensor(b!) q8, Tensor(c!) xs, Tensor x, bool gelu) -> ()") \
  X(act_quant_fp8, "(Tensor(a!) xq, Tensor(b!) xs, Tensor x) -> ()") \
  X(splitk_add_rmsnorm, "(Tensor(a!) out, Tensor(b!) residual, Tensor ws, int splits, Tensor weight, float eps, Tensor(c!)? out16=None, Tensor(d!)? out8=None, Tensor(e!)? xs8=None) -> ()") \
  X(splitk_post_add_rmsnorm, "(Tensor(a!) out, Tensor(b!) residual, Tensor ws, int splits, Tensor w_post, Tensor w_next, float eps, Tensor(c!)? out16=None, Tensor(d!)? out8=None, Tensor(e!)? xs8=None) -> ()") \
  X(splitk_glu, "(Tensor(a!) act, Tensor ws, int splits, bool gelu, Tensor(b!)? act16=None) -> ()") \
  X(paged_decode_qkv, "(Tensor(a!) out, Tensor ws, int splits, Tensor positions, Tensor slots, Tensor cos_sin, Tensor(b!) k_cache, Tensor(c!) v_cache, Tensor block_tables, Tensor context_lens, Tensor(d!) tmp_out, Tensor(e!) tmp_ml, int nq, int nkv, int part_size, float scale, int window, int mode, Tensor(f!)? out16=None, Tensor? q_norm=None, Tensor? k_norm=None, float eps=1e-6, float softcap=0.0) -> ()") \
  X(splitk_reduce, "(Tensor(a!) out, Tensor ws, int splits) -> ()") \
  X(splitk_rope_cache, "(Tensor(a!) qkv, Tensor ws, int splits, Tensor positions, Tensor slots, Tensor cos_sin, Tensor(b!) k_cache, Tensor(c!) v_cache, int nq, int nkv, int head_dim, int mode, Tensor? bias=None, Tensor? q_w=None, Tensor? k_w=None, float eps=1e-6) -> ()") \
  X(skinny_gemm, "(Tensor(a!) out, Tensor x, Tensor w, int rt, int kw) -> ()") \
  X(penalty_apply, "(Tensor(a!) logits, Tensor slot, Tensor pres, Tensor freq, Tensor rep, Tensor counts, Tensor seen) -> ()") \
  X(logit_bias_apply, "(Tensor(a!) logits, Tensor slot, Tensor ids, Tensor vals, Tensor n) -> ()") \
  X(logit_softcap_, "(Tensor(a!) logits, float cap) -> ()") \
  X(penalty_update, "(Tensor tok, Tensor slot, Tensor(a!) counts, Tensor(b!) seen) -> ()") \
  X(penalty_init, "(Tensor(a!) counts, Tensor(b!) seen, Tensor slots, Tensor off, Tensor n_prompt, Tensor toks) -> ()") \
  X(top_logprobs, "(Tensor logits, Tensor nreq, Tensor(a!) out_ids, Tensor(b!) out_lp) -> ()") \
  X(prompt_logprobs, "(Tensor logits, Tensor targets, Tensor nreq, Tensor(a!) out_lp, Tensor(b!) out_rank, Tensor(c!) out_ids, Tensor(d!) out_top) -> ()") \
  X(layernorm, "(Tensor(a!) out, Tensor x, Tensor w, Tensor b, Tensor(b!)? residual, float eps) -> ()") \
  X(gelu_, "(Tensor(a!) x, bool tanh_approx) -> ()") \
  X(vision_pool_rmsnorm, "(Tensor(a!) out, Tensor x, Tensor w, int g, int k, float eps) -> ()") \
  X(vision_attention, "(Tensor(a!) out, Tensor(b!) qkv, Tensor? cos_sin, Tensor cu, Tensor tiles, int nh, int D, float scale) -> ()") \
  X(sample, "(Tensor(a!) out_tok, Tensor(b!) out_lp, Tensor logits, Tensor temperature, Tensor top_k, Tensor top_p, Tensor seeds, Tensor steps, bool two_rounds=True, Tensor? min_p=None) -> ()")

TORCH_LIBRARY(hipserve, m) {
#define DEF_OP(name, schema) m.def(#name schema);
  GPU_KEY_OPS(DEF_OP)
#undef DEF_OP
  // catch-all kernels: ops over tensor lists or without a tensor to dispatch on, and the
  // custom all-reduce ops (car_*), which carry an opaque state handle
  m.def("gguf_gemm_parts(Tensor(a!) out, Tensor(b!) ws, Tensor x, Tensor[] qs, Tensor[] rss, int[] qtypes, int[] rows, int[] cols, int Ntot, int K, int splits, Tensor? x16=None) -> int", &gguf_gemm_parts);
  m.def("gguf_prefill(Tensor(a!) out, Tensor x16, Tensor rsc, Tensor[] qs, int[] qtypes, int[] rows, int[] cols, int K, int epi) -> bool", &gguf_prefill);
  m.def("x_f16_pairs(Tensor(a!) x16, Tensor(b!) rsc, Tensor x) -> ()", &x_f16_pairs);
  m.def("gguf_dequant_tiled(Tensor(a!) out, Tensor q, Tensor rs, int qtype, int N, int K, int pack=0, int nrows=0, bool kmajor=False) -> ()",
        &gguf_dequant_tiled);
  m.def("fp8_untile(Tensor(a!) out, Tensor q, int N, int K) -> ()", &fp8_untile);
  m.def("quant_formats() -> str", &quant_formats);
  m.def("qmoe_gemm(Tensor(a!) out, Tensor(b!) ws, Tensor x, Tensor q, Tensor rs, int qtype, int N, int K, Tensor slots, Tensor tile_expert, int tile, int gather_k, int splits, bool kmajor=False, int glu=0) -> int", &qmoe_gemm);
  m.def("stage_copy(Tensor(a!)[] dst, Tensor[] src, int device) -> ()", &stage_copy);
  m.def("car_create(int rank, int world, int max_bytes, int nb_large=512) -> int", &car_create);
  m.def("car_handle(int state) -> Tensor", &car_handle);
  m.def("car_open(int state, int peer, Tensor handle) -> ()", &car_open);
  m.def("car_all_reduce(int state, Tensor inp, Tensor(a!) out, bool two_shot) -> ()", &car_all_reduce);
  m.def("car_all_gather(int state, Tensor inp, Tensor(a!) out) -> ()", &car_all_gather);
  m.def("car_norm_fits(int state, int M, int N, bool exch_f32) -> bool", &car_norm_fits);
  m.def("car_add_rmsnorm(int state, Tensor(a!) out, Tensor(b!) residual, Tensor x, int splits, Tensor weight, float eps, bool exch_f32) -> ()", &car_add_rmsnorm);
  m.def("car_error(int state) -> bool", &car_error);
  m.def("car_destroy(int state) -> ()", &car_destroy);
}

TORCH_LIBRARY_IMPL(hipserve, CUDA, m) {
#define IMPL_OP(name, schema) m.impl(#name, &name);
  GPU_KEY_OPS(IMPL_OP)
#undef IMPL_OP
}
