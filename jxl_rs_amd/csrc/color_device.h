// The colour stage of a frame on ONE pixel, shared by the read-outs (k_output.hip), the save tail and frame blending
// (k_blend.hip): XybStage (render/stages/xyb.rs:208-240), FromLinearStage with each of the reference's transfer functions
// (render/stages/from_linear.rs:57-112; curves of color/tf.rs and util/fast_math.rs, operation for operation) and
// YcbcrToRgbStage (render/stages/ycbcr.rs:35-78).  FMAs are explicit: the library builds with -ffp-contract=off.
#pragma once
#include "jxlh_internal.h"

namespace jxlh {
namespace {

__device__ __forceinline__ float linear_to_srgb(float x) {
  constexpr float P0 = -5.135152395e-4f, P1 = 5.287254571e-3f, P2 = 3.903842876e-1f, P3 = 1.474205315f,
                  P4 = 7.352629620e-1f;
  constexpr float Q0 = 1.004519624e-2f, Q1 = 3.036675394e-1f, Q2 = 1.340816930f, Q3 = 9.258482155e-1f,
                  Q4 = 2.424867759e-2f;
  const float a = __builtin_fabsf(x);
  const float t = __builtin_sqrtf(a);
  float yp = __builtin_fmaf(P4, t, P3);
  yp = __builtin_fmaf(yp, t, P2);
  yp = __builtin_fmaf(yp, t, P1);
  yp = __builtin_fmaf(yp, t, P0);
  float yq = __builtin_fmaf(Q4, t, Q3);
  yq = __builtin_fmaf(yq, t, Q2);
  yq = __builtin_fmaf(yq, t, Q1);
  yq = __builtin_fmaf(yq, t, Q0);
  const float r = (0.0031308f > a) ? a * 12.92f : yp / yq;
  return __builtin_copysignf(r, x);
}

#include "tf_constants.inc"

// util/rational_poly.rs:20-35 (FMA Horner, the SIMD form) and :13-17 (plain mul + add, the scalar form)
template <int NP, int NQ>
__device__ __forceinline__ float ratpoly_fma(float x, const float (&p)[NP], const float (&q)[NQ]) {
  float yp = p[NP - 1], yq = q[NQ - 1];
#pragma unroll
  for (int i = NP - 2; i >= 0; i--) yp = __builtin_fmaf(yp, x, p[i]);
#pragma unroll
  for (int i = NQ - 2; i >= 0; i--) yq = __builtin_fmaf(yq, x, q[i]);
  return yp / yq;
}
template <int NP, int NQ>
__device__ __forceinline__ float ratpoly_plain(float x, const float (&p)[NP], const float (&q)[NQ]) {
  float yp = p[NP - 1], yq = q[NQ - 1];
#pragma unroll
  for (int i = NP - 2; i >= 0; i--) yp = yp * x + p[i];
#pragma unroll
  for (int i = NQ - 2; i >= 0; i--) yq = yq * x + q[i];
  return yp / yq;
}

template <bool SIMD>
__device__ __forceinline__ float fast_log2f_dev(float x) {  // util/fast_math.rs:127-149
  const int32_t x_bits = __float_as_int(x);
  const int32_t exp_bits = (int32_t)((uint32_t)x_bits - 0x3f2aaaabu);
  const int32_t exp_shifted = exp_bits >> 23;
  const float mantissa = __int_as_float((int32_t)((uint32_t)x_bits - ((uint32_t)exp_shifted << 23)));
  const float m1 = mantissa - 1.0f;
  const float poly = SIMD ? ratpoly_fma(m1, kTf_LOG2F_P, kTf_LOG2F_Q) : ratpoly_plain(m1, kTf_LOG2F_P, kTf_LOG2F_Q);
  return poly + (float)exp_shifted;
}
template <bool SIMD>
__device__ __forceinline__ float fast_pow2f_dev(float x) {  // util/fast_math.rs:79-114
  const float x_floor = __builtin_floorf(x);
  const float e = __int_as_float((int32_t)(((uint32_t)((int32_t)x_floor + 127)) << 23));
  const float frac = x - x_floor;
  float num = frac + kTf_POW2F_NUMER[0], den;
  if constexpr (SIMD) {
    num = __builtin_fmaf(num, frac, kTf_POW2F_NUMER[1]);
    num = __builtin_fmaf(num, frac, kTf_POW2F_NUMER[2]);
    num = num * e;
    den = __builtin_fmaf(kTf_POW2F_DENOM[0], frac, kTf_POW2F_DENOM[1]);
    den = __builtin_fmaf(den, frac, kTf_POW2F_DENOM[2]);
    den = __builtin_fmaf(den, frac, kTf_POW2F_DENOM[3]);
  } else {
    num = num * frac + kTf_POW2F_NUMER[1];
    num = num * frac + kTf_POW2F_NUMER[2];
    num = num * e;
    den = kTf_POW2F_DENOM[0] * frac + kTf_POW2F_DENOM[1];
    den = den * frac + kTf_POW2F_DENOM[2];
    den = den * frac + kTf_POW2F_DENOM[3];
  }
  return num / den;
}
template <bool SIMD>
__device__ __forceinline__ float fast_powf_dev(float base, float e) {
  return fast_pow2f_dev<SIMD>(fast_log2f_dev<SIMD>(base) * e);
}

__device__ __forceinline__ float linear_to_bt709(float x) {  // color/tf.rs:115-148
  const float a = __builtin_fabsf(x);
  const float r = (0.018f > a) ? a * 4.5f : ratpoly_fma(__builtin_sqrtf(a), kTf_BT709_P, kTf_BT709_Q);
  return __builtin_copysignf(r, x);
}
__device__ __forceinline__ float linear_to_pq(float y_mult, float x) {  // color/tf.rs:288-314
  const float a = __builtin_fabsf(x);
  const float a_1_4 = __builtin_sqrtf(__builtin_sqrtf(a * y_mult));
  const float y_small = ratpoly_fma(a_1_4, kTf_PQ_INV_EOTF_P_SMALL, kTf_PQ_INV_EOTF_Q_SMALL);
  const float y_large = ratpoly_fma(a_1_4, kTf_PQ_INV_EOTF_P, kTf_PQ_INV_EOTF_Q);
  return __builtin_copysignf((1e-4f > a) ? y_small : y_large, x);
}
__device__ __forceinline__ float scene_to_hlg(float x) {  // color/tf.rs:482-497
  constexpr double kA = 0.17883277, kB = 1.0 - 4.0 * kA, kC = 0.5599107295;
  constexpr float k = (float)(kA * 0.693147180559945309417232121458176568), hb = (float)kB, hc = (float)kC;
  const float a = __builtin_fabsf(x);
  const float y = (a <= 1.0f / 12.0f) ? __builtin_sqrtf(3.0f * a) : k * fast_log2f_dev<false>(12.0f * a - hb) + hc;
  return __builtin_copysignf(y, x);
}

// FromLinearStage (render/stages/from_linear.rs:57-112) on one pixel
template <int TF>
__device__ __forceinline__ void from_linear(const TfParamsDev& t, float& r, float& g, float& b) {
  if constexpr (TF == kTfSrgb) {
    r = linear_to_srgb(r);
    g = linear_to_srgb(g);
    b = linear_to_srgb(b);
  } else if constexpr (TF == kTfBt709) {
    r = linear_to_bt709(r);
    g = linear_to_bt709(g);
    b = linear_to_bt709(b);
  } else if constexpr (TF == kTfPq) {
    const float y_mult = t.param * (1.0f / 10000.0f);
    r = linear_to_pq(y_mult, r);
    g = linear_to_pq(y_mult, g);
    b = linear_to_pq(y_mult, b);
  } else if constexpr (TF == kTfHlg) {
    if (!(__builtin_fabsf(t.param) < 0.1f)) {  // hlg_ootf_inner (color/tf.rs:379-393), exponent from the host
      const float mixed = __builtin_fmaf(r, t.lum[0], __builtin_fmaf(g, t.lum[1], b * t.lum[2]));
      const float mult = fast_powf_dev<false>(mixed, t.param);
      r *= mult;
      g *= mult;
      b *= mult;
    }
    r = scene_to_hlg(r);
    g = scene_to_hlg(g);
    b = scene_to_hlg(b);
  } else if constexpr (TF == kTfGamma) {
    r = __builtin_copysignf(fast_powf_dev<true>(__builtin_fabsf(r), t.param), r);
    g = __builtin_copysignf(fast_powf_dev<true>(__builtin_fabsf(g), t.param), g);
    b = __builtin_copysignf(fast_powf_dev<true>(__builtin_fabsf(b), t.param), b);
  }
}

// fma(a, b, c) of the opsin matrix; with NAN_BITS_SHOW, with the NaN an x86 FMA hands on.  Where the product alone is
// invalid (a zero matrix entry times a channel that overflowed to inf) and the addend is a NaN, x86 returns the addend;
// v_fma_f32 makes a fresh default NaN.  Gamma and HLG build a NUMBER from a NaN's bits (fast_log2f_dev reads the pattern,
// copysign the sign), so which NaN comes out is visible behind them, and only behind them: the other curves keep a NaN a
// NaN and pay nothing (the selects measured 5-10 % on the 8 and 16-bit sRGB read-outs of an 8192 x 8192 frame).  A NaN
// in b is left to the hardware, which picks as x86 does.
template <bool NAN_BITS_SHOW>
__device__ __forceinline__ float opsin_fma(float a, float b, float c) {
  const float r = __builtin_fmaf(a, b, c);
  if constexpr (NAN_BITS_SHOW) return (c != c && b == b) ? c : r;
  return r;
}

// Samples of one pixel -> display-referred R, G, B in [0, 1] nominal.
//   YCBCR = false: XybStage (xyb.rs:220-240) + the sRGB transfer function (frame/render.rs:757-762)
//   YCBCR = true : YcbcrToRgbStage on planes ordered Cb, Y, Cr (render/stages/ycbcr.rs:35-78); such frames
//                  are not XYB-encoded, so no transfer-function stage follows (frame/render.rs:755-763)
//   MODE = kTfLinear .. kTfGamma: XybStage, then that transfer function;  kModeYcbcr;  kModeNone: planes are RGB already
template <int MODE>
__device__ __forceinline__ void to_display_rgb(const XybParamsDev& p, const TfParamsDev& t, float c0, float c1, float c2,
                                               float& r, float& g, float& b) {
  if constexpr (MODE == kModeNone) {
    r = c0;
    g = c1;
    b = c2;
  } else if constexpr (MODE == kModeYcbcr) {
    constexpr float k128 = 128.0f / 255.0f, kCrToR = 1.402f, kCrToG = -0.299f * 1.402f / 0.587f,
                    kCbToG = -0.114f * 1.772f / 0.587f, kCbToB = 1.772f;
    const float y = c1 + k128;
    r = __builtin_fmaf(c2, kCrToR, y);
    g = __builtin_fmaf(c2, kCrToG, __builtin_fmaf(c0, kCbToG, y));
    b = __builtin_fmaf(c0, kCbToB, y);
  } else {
    float l = c1 + c0 - p.bias_cbrt[0];
    float m = c1 - c0 - p.bias_cbrt[1];
    float s = c2 - p.bias_cbrt[2];
    const float l2 = l * l, m2 = m * m, s2 = s * s;
    const float sl = l * p.intensity_scale, sm = m * p.intensity_scale, ss = s * p.intensity_scale;
    l = __builtin_fmaf(l2, sl, p.scaled_bias[0]);
    m = __builtin_fmaf(m2, sm, p.scaled_bias[1]);
    s = __builtin_fmaf(s2, ss, p.scaled_bias[2]);
    constexpr bool kShow = MODE == kTfHlg || MODE == kTfGamma;
    r = opsin_fma<kShow>(p.mat[0], l, opsin_fma<kShow>(p.mat[1], m, p.mat[2] * s));
    g = opsin_fma<kShow>(p.mat[3], l, opsin_fma<kShow>(p.mat[4], m, p.mat[5] * s));
    b = opsin_fma<kShow>(p.mat[6], l, opsin_fma<kShow>(p.mat[7], m, p.mat[8] * s));
    from_linear<MODE>(t, r, g, b);
  }
}

}  // namespace
}  // namespace jxlh
