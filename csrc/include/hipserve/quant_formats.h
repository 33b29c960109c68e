// The formats of the tiled quantised-weight kernels (gguf_mfma.hip), one row each: the one
// place on the C++ side that says what is true of a format. Plain C++, read by the kernels
// (gguf_tiles.h) and by the host-compiled torch_bindings.cpp; hipserve/ops/quant.py FORMATS
// is the Python copy, held equal by tests/test_native_lib_cpu.py (quant_formats op).
#pragma once

#include <type_traits>

namespace hipserve {
namespace gq {

// X(name, id, chunk bytes, sub shift, gguf, row_scaled, prefill, moe). id: the kernel qtype (in
// the tune cache keys: never renumbered); chunk bytes: one tiled chunk of 16 rows x 256 k
// (gguf_tiles.h); sub shift: the bit at which the subnormal-integer dequant places the integers,
// -1 where it is not used; gguf: a GGUF block format (scales inside the chunk); row_scaled: a
// per-row fp32 scale (Part::rs) multiplies the accumulators in the epilogue; prefill / moe: the
// block prefill GEMM (qpg_kernel) / the expert GEMM (qmoe_kernel) has a body for it
#define HS_QUANT_FORMATS(X)                        \
  X(Q4_0, 0, 2304, 6, true, false, true, true)     \
  X(Q4_1, 1, 2560, 6, true, false, true, true)     \
  X(Q8_0, 2, 4352, 2, true, false, true, true)     \
  X(Q4_K, 3, 2304, 6, true, false, true, true)     \
  X(Q5_K, 4, 2816, 5, true, false, true, true)     \
  X(Q6_K, 5, 3360, 4, true, false, true, true)     \
  X(FP8, 6, 4096, -1, false, true, false, true)    \
  X(FP8B, 7, 4224, -1, false, true, false, false)  \
  X(INT8, 8, 4608, -1, false, false, false, true)  \
  X(INT8C, 9, 4096, -1, false, true, false, true)  \
  X(INT4, 10, 2560, -1, false, false, false, true) \
  X(Q2_K, 11, 1344, 8, true, false, false, true)   \
  X(Q3_K, 12, 1824, 7, true, false, false, true)

struct QuantFormat {
  const char* name;
  int id, chunk_bytes, sub_shift;
  bool gguf, row_scaled, prefill, moe;
};
#define X(name, id, ...) name = id,
enum { HS_QUANT_FORMATS(X) };
#undef X
#define X(name, ...) name,
constexpr int kQuantFormatIds[] = {HS_QUANT_FORMATS(X)};
#undef X

// the row of kernel qtype qt; id -1 and every flag false for an unknown one
constexpr QuantFormat quant_format(int qt) {
  switch (qt) {
#define X(name, ...) \
  case name: return QuantFormat{#name, __VA_ARGS__};
    HS_QUANT_FORMATS(X)
#undef X
  }
  return QuantFormat{"", -1, 0, -1, false, false, false, false};
}
constexpr bool gguf_block_format(int qt) { return quant_format(qt).gguf; }
constexpr bool qpg_format(int qt) { return quant_format(qt).prefill; }
constexpr bool moe_format(int qt) { return quant_format(qt).moe; }

// f(std::integral_constant<int, QT>{}) for a known qt; false (f not called) otherwise
template <class F>
bool dispatch_format(int qt, F&& f) {
  switch (qt) {
#define X(name, ...) \
  case name: f(std::integral_constant<int, name>{}); return true;
    HS_QUANT_FORMATS(X)
#undef X
  }
  return false;
}

}  // namespace gq
}  // namespace hipserve
