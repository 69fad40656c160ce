// Device pieces of the save tail that k_save.hip and k_lf_preview.hip share: the colour stage on register arrays, the
// conversions of jxl/src/render/stages/convert.rs with the dither table, f16::from_f32 of jxl/src/util/float16.rs, and
// the packing of samples into the dwords of their byte stream.
#pragma once
#include "color_device.h"
#include "jxlh_internal.h"

namespace jxlh {
namespace {

__constant__ float kSaveDitherDev[32 * 32] = {
#include "dither_table.inc"
};

template <int FMT>
constexpr int sample_bytes() {
  return FMT == kSaveU8 ? 1 : FMT == kSaveF32 ? 4 : 2;
}

// f16::from_f32 (util/float16.rs:82-141), branch for branch
__device__ __forceinline__ uint32_t f32_to_f16_bits(float f) {
  const uint32_t bits = __float_as_uint(f);
  const uint32_t sign = (bits >> 16) & 0x8000u;
  const int exp = (int)((bits >> 23) & 0xffu);
  const uint32_t mant = bits & 0x007fffffu;
  if (exp == 0) return sign;  // zero or f32 denormal
  if (exp == 255) return sign | 0x7c00u | (mant != 0 ? 0x0200u : 0u);
  const int unbiased = exp - 127;
  if (unbiased < -24) return sign;
  if (unbiased < -14) return sign | ((mant | 0x00800000u) >> (uint32_t)(-unbiased));  // shift + 14, truncating
  if (unbiased > 15) return sign | 0x7c00u;
  const uint32_t h_exp = (uint32_t)(unbiased + 15);
  uint32_t h_mant = mant >> 13;
  const uint32_t round_bit = (mant >> 12) & 1u, sticky = mant & 0x0fffu;
  if (round_bit == 1 && (sticky != 0 || (h_mant & 1u) == 1)) h_mant += 1;
  if (h_mant > 0x3ffu) return h_exp >= 30 ? (sign | 0x7c00u) : (sign | ((h_exp + 1) << 10));
  return sign | (h_exp << 10) | h_mant;
}

template <int MODE, int NPX>
__device__ __forceinline__ void colour_px(const XybParamsDev& p, const TfParamsDev& t, float (&c)[3][NPX]) {
#pragma unroll
  for (int i = 0; i < NPX; i++) {
    float r, g, b;
    to_display_rgb<MODE>(p, t, c[0][i], c[1][i], c[2][i], r, g, b);
    c[0][i] = r;
    c[1][i] = g;
    c[2][i] = b;
  }
}

// one sample of pipeline channel ch at frame position (fx, fy) in the output's format and byte order
// (A: a launch structure with maxv and big_endian, and with clamp, clamp_min, clamp_max where A::kF16Clamp)
template <int FMT, class A>
__device__ __forceinline__ uint32_t convert_sample(const A& a, const float* __restrict__ dither, float v, int fx,
                                                   int fy, int ch) {
  uint32_t q;
  if constexpr (FMT == kSaveU8) {  // f32_to_u8_simd (convert.rs:570-606)
    const float d = dither[((fy + ch * 13) & 31) * 32 + ((fx + ch * 23) & 31)];
    const float dithered = v * a.maxv + d;
    float clamped = dithered > 0.0f ? dithered : 0.0f;
    clamped = clamped < a.maxv ? clamped : a.maxv;
    return (uint32_t)__builtin_rintf(clamped);
  } else if constexpr (FMT == kSaveU16) {  // f32_to_u16_simd (convert.rs:743-761)
    float clamped = v > 0.0f ? v : 0.0f;
    clamped = clamped < 1.0f ? clamped : 1.0f;
    q = (uint32_t)__builtin_rintf(clamped * a.maxv);
  } else if constexpr (FMT == kSaveF16) {  // f32::clamp keeps a NaN and -0.0, then f16::from_f32
    if constexpr (A::kF16Clamp) {
      if (a.clamp) {
        if (v < a.clamp_min) v = a.clamp_min;
        if (v > a.clamp_max) v = a.clamp_max;
      }
    }
    q = f32_to_f16_bits(v);
  } else {
    q = __float_as_uint(v);
  }
  if (a.big_endian) {
    if constexpr (FMT == kSaveF32)
      q = __builtin_bswap32(q);
    else
      q = ((q >> 8) | (q << 8)) & 0xffffu;
  }
  return q;
}

template <int BPS>
__device__ __forceinline__ void store_sample(uint8_t* o, uint32_t q) {
  if constexpr (BPS == 1)
    *o = (uint8_t)q;
  else if constexpr (BPS == 2)
    *reinterpret_cast<uint16_t*>(o) = (uint16_t)q;
  else
    *reinterpret_cast<uint32_t*>(o) = q;
}

// the samples of NPX pixels as the dwords of their byte stream: NPX * SPP * BPS / 4 words
template <int BPS, int SPP, int NPX>
__device__ __forceinline__ void pack_words(const uint32_t (&q)[NPX][SPP], uint32_t (&wd)[NPX * SPP * BPS / 4]) {
  constexpr int PER = 4 / BPS;  // samples per dword
#pragma unroll
  for (int n = 0; n < NPX * SPP * BPS / 4; n++) {
    uint32_t v = 0;
#pragma unroll
    for (int s = 0; s < PER; s++) {
      const int j = n * PER + s;
      v |= q[j / SPP][j % SPP] << (8 * BPS * s);
    }
    wd[n] = v;
  }
}

// N dwords to a dword-aligned address, in the widest stores its alignment allows
template <int N>
__device__ __forceinline__ void store_words(uint8_t* o, const uint32_t (&wd)[N]) {
  const uintptr_t at = reinterpret_cast<uintptr_t>(o);
  if constexpr (N % 4 == 0) {
    if ((at & 15) == 0) {
#pragma unroll
      for (int n = 0; n < N / 4; n++)
        reinterpret_cast<uint4*>(o)[n] = make_uint4(wd[4 * n], wd[4 * n + 1], wd[4 * n + 2], wd[4 * n + 3]);
      return;
    }
  }
  if constexpr (N % 2 == 0) {
    if ((at & 7) == 0) {
#pragma unroll
      for (int n = 0; n < N / 2; n++) reinterpret_cast<uint2*>(o)[n] = make_uint2(wd[2 * n], wd[2 * n + 1]);
      return;
    }
  }
#pragma unroll
  for (int n = 0; n < N; n++) reinterpret_cast<uint32_t*>(o)[n] = wd[n];
}

}  // namespace
}  // namespace jxlh
