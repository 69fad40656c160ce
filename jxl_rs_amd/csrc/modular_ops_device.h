// Per-sample pieces of the Modular inverse transforms that the whole-plane kernels (k_modular.hip) and the group-local
// kernel (k_modular_local.hip) share: the RCT ops and output permutation, the palette look-up with its implicit and
// delta entries.  All arithmetic is wrapping 32-bit, as in the reference's SIMD paths.
// Reference: rct.rs:14-157; palette.rs:24-199.
#pragma once
#include "jxlh_internal.h"
#include "modular_local_host.h"  // rct_permute

namespace jxlh {
namespace {

__device__ __forceinline__ int32_t wadd(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
__device__ __forceinline__ int32_t wsub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }

template <int OP>
__device__ __forceinline__ void rct_op(int32_t v0, int32_t v1, int32_t v2, int32_t& w0, int32_t& w1, int32_t& w2) {
  w0 = v0;
  w1 = v1;
  w2 = v2;
  if constexpr (OP == 1) {
    w2 = wadd(v2, v0);
  } else if constexpr (OP == 2) {
    w1 = wadd(v1, v0);
  } else if constexpr (OP == 3) {
    w1 = wadd(v1, v0);
    w2 = wadd(v2, v0);
  } else if constexpr (OP == 4) {
    w1 = wadd(v1, wadd(v0, v2) >> 1);
  } else if constexpr (OP == 5) {
    const int32_t t2 = wadd(v0, v2);
    w1 = wadd(v1, wadd(v0, t2) >> 1);
    w2 = t2;
  } else if constexpr (OP == 6) {
    int32_t y = wsub(v0, v2 >> 1);
    const int32_t g = wadd(v2, y);
    y = wsub(y, v1 >> 1);
    w0 = wadd(y, v1);
    w1 = g;
    w2 = y;
  }
}

__constant__ int16_t kDeltaPalette[72][3] = {
#include "delta_palette.inc"
};

// get_palette_value (palette.rs:39-163)
__device__ __forceinline__ int32_t palette_value(const int32_t* __restrict__ palette, size_t pstride, int32_t index,
                                                 int c, int palette_size, int bit_depth) {
  if (index < 0) {
    if (c >= 3) return 0;
    uint32_t i = (uint32_t)(-(index + 1));
    i %= 1 + 2 * (72 - 1);
    int32_t r = kDeltaPalette[(i + 1) >> 1][c];
    if ((i & 1) == 0) r = -r;
    if (bit_depth > 8) r *= 1 << (bit_depth - 8);
    return r;
  }
  uint32_t i = (uint32_t)index;
  const uint32_t ps = (uint32_t)palette_size;
  if (i >= ps && i < ps + 64) {
    if (c >= 3) return 0;
    i -= ps;
    i >>= c * 2;
    const int sh = bit_depth > 3 ? bit_depth - 3 : 0;
    return (int32_t)(((uint64_t)(i % 4) * (uint64_t)((1u << bit_depth) - 1)) >> 2) + (1 << sh);
  } else if (i >= ps + 64) {
    if (c >= 3) return 0;
    i -= ps + 64;
    if (c == 1) i /= 5;
    if (c == 2) i /= 25;
    return (int32_t)(((uint64_t)(i % 5) * (uint64_t)((1u << bit_depth) - 1)) >> 2);
  }
  return palette[(size_t)c * pstride + i];
}

}  // namespace
}  // namespace jxlh
