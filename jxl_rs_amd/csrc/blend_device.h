// perform_blending (jxl/src/features/blending.rs:199-474) restated for ONE pixel: the reference's row functions are
// pointwise, and its "old alpha" scratch is a per-pixel copy of the extra channels taken before the blend.  Shared by
// the patches stage (k_patches.hip) and frame blending (BlendingStage, frame/render.rs:765-771: k_blend.hip).
//
// Every expression keeps the reference's association (the library builds with -ffp-contract=off, so nothing fuses),
// and 1 / new_a is the IEEE division: new_a is unbounded when clamp is off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace jxlh {

// PatchBlendMode (features/patches.rs:41-74)
enum : uint32_t {
  kBlendNone = 0,
  kBlendReplace = 1,
  kBlendAdd = 2,
  kBlendMul = 3,
  kBlendAbove = 4,
  kBlendBelow = 5,
  kBlendAddAbove = 6,  // AlphaWeightedAddAbove
  kBlendAddBelow = 7,  // AlphaWeightedAddBelow
};

// one PatchBlending packed into a word: mode | alpha_channel << 8 | clamp << 16
__host__ __device__ constexpr uint32_t pack_blending(uint32_t mode, uint32_t alpha, uint32_t clamp) {
  return mode | alpha << 8 | (clamp ? 1u : 0u) << 16;
}

__device__ __forceinline__ float blend_clamp(float v, bool clamp) {  // v.max(zero).min(one) / f32::clamp(0, 1)
  return clamp ? fminf(fmaxf(v, 0.0f), 1.0f) : v;
}

// v[k] with k a runtime index, without indexing a register array dynamically (that would spill it to scratch)
template <int N>
__device__ __forceinline__ float pick(const float (&v)[N], uint32_t k) {
  float r = 0.0f;
#pragma unroll
  for (int i = 0; i < N; i++)
    if ((uint32_t)i == k) r = v[i];
  return r;
}

// bg: 3 colour + NEC extra channel values of the pixel, blended in place; fg: the same of the foreground;
// blend[0] colour blending, blend[1 + i] extra channel i (pack_blending); ec_alpha / ec_assoc: bit k set when extra
// channel k is of alpha type / has associated alpha (ExtraChannelInfo::ec_type, alpha_associated()).
template <int NEC>
__device__ __forceinline__ void blend_pixel(float (&bg)[3 + NEC], const float (&fg)[3 + NEC], const uint32_t* blend,
                                            uint32_t ec_alpha, uint32_t ec_assoc) {
  constexpr int kEc = NEC > 0 ? NEC : 1;
  float old[kEc];  // tmp: the extra channels before this blend
  float fga[kEc];  // fg's extra channels
#pragma unroll
  for (int i = 0; i < kEc; i++) {
    old[i] = i < NEC ? bg[3 + (i < NEC ? i : 0)] : 0.0f;
    fga[i] = i < NEC ? fg[3 + (i < NEC ? i : 0)] : 0.0f;
  }
  const float one = 1.0f;
#pragma unroll
  for (int i = 0; i < NEC; i++) {
    const uint32_t b = blend[1 + i];
    const uint32_t mode = b & 0xffu, alpha = (b >> 8) & 0xffu;
    const bool clamp = (b >> 16) & 1u;
    const bool assoc = (ec_assoc >> alpha) & 1u;
    float& o = bg[3 + i];
    const float f = fg[3 + i];
    switch (mode) {
      case kBlendAdd:
        o = o + f;
        break;
      case kBlendAbove:
        if ((uint32_t)i == alpha) {  // blend_alpha, fg on top
          const float top_a = blend_clamp(f, clamp);
          o = one - (one - top_a) * (one - o);
        } else if (assoc) {
          const float fa = blend_clamp(pick(fga, alpha), clamp);
          o = f + o * (one - fa);
        } else {
          const float fa = blend_clamp(pick(fga, alpha), clamp);
          const float oa = pick(old, alpha);
          const float new_a = one - (one - fa) * (one - oa);
          const float rnew_a = new_a > 0.0f ? one / new_a : 0.0f;
          o = (f * fa + o * oa * (one - fa)) * rnew_a;
        }
        break;
      case kBlendBelow:
        if ((uint32_t)i == alpha) {  // blend_alpha, bg on top
          const float top_a = blend_clamp(o, clamp);
          o = one - (one - top_a) * (one - f);
        } else if (assoc) {
          const float ba = blend_clamp(pick(old, alpha), clamp);
          o = o + f * (one - ba);
        } else {
          const float ba = blend_clamp(pick(old, alpha), clamp);
          const float fa = pick(fga, alpha);
          const float new_a = one - (one - ba) * (one - fa);
          const float rnew_a = new_a > 0.0f ? one / new_a : 0.0f;
          o = (o * ba + f * fa * (one - ba)) * rnew_a;
        }
        break;
      case kBlendAddAbove:
        if ((uint32_t)i != alpha) o = o + f * blend_clamp(pick(fga, alpha), clamp);
        break;
      case kBlendAddBelow:
        if ((uint32_t)i == alpha) o = f;
        else o = f + o * blend_clamp(pick(old, alpha), clamp);
        break;
      case kBlendMul:
        o = o * blend_clamp(f, clamp);
        break;
      case kBlendReplace:
        o = f;
        break;
      default:  // kBlendNone
        break;
    }
  }
  const uint32_t b = blend[0];
  const uint32_t mode = b & 0xffu, alpha = (b >> 8) & 0xffu;
  const bool clamp = (b >> 16) & 1u;
  const bool has_alpha = ec_alpha != 0u;
  switch (mode) {
    case kBlendAdd:
#pragma unroll
      for (int c = 0; c < 3; c++) bg[c] = bg[c] + fg[c];
      break;
    case kBlendAddAbove:
      if (!has_alpha) {
#pragma unroll
        for (int c = 0; c < 3; c++) bg[c] = bg[c] + fg[c];
      } else {
        const float w = blend_clamp(pick(fga, alpha), clamp);
#pragma unroll
        for (int c = 0; c < 3; c++) bg[c] = bg[c] + fg[c] * w;
      }
      break;
    case kBlendAddBelow:
      if (!has_alpha) {
#pragma unroll
        for (int c = 0; c < 3; c++) bg[c] = bg[c] + fg[c];
      } else {
        const float w = blend_clamp(pick(old, alpha), clamp);
#pragma unroll
        for (int c = 0; c < 3; c++) bg[c] = fg[c] + bg[c] * w;
      }
      break;
    case kBlendAbove:
    case kBlendBelow:
      if (!has_alpha) {
        if (mode == kBlendAbove) {
#pragma unroll
          for (int c = 0; c < 3; c++) bg[c] = fg[c];
        }
      } else {  // blend(): the top layer's alpha is clamped; new_a replaces the alpha channel
        const bool above = mode == kBlendAbove;
        const bool assoc = (ec_assoc >> alpha) & 1u;
        const float fa = pick(fga, alpha), oa = pick(old, alpha);
        const float top_a = blend_clamp(above ? fa : oa, clamp);
        const float bottom_a = above ? oa : fa;
        const float one_minus_top_a = one - top_a;
        const float new_a = one - one_minus_top_a * (one - bottom_a);
        const float reciprocal_a = new_a > 0.0f ? one / new_a : 0.0f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const float top_c = above ? fg[c] : bg[c];
          const float bottom_c = above ? bg[c] : fg[c];
          bg[c] = assoc ? top_c + bottom_c * one_minus_top_a
                        : (top_c * top_a + bottom_c * bottom_a * one_minus_top_a) * reciprocal_a;
        }
#pragma unroll
        for (int i = 0; i < NEC; i++)
          if ((uint32_t)i == alpha) bg[3 + i] = new_a;
      }
      break;
    case kBlendMul:
#pragma unroll
      for (int c = 0; c < 3; c++) bg[c] = bg[c] * blend_clamp(fg[c], clamp);
      break;
    case kBlendReplace:
#pragma unroll
      for (int c = 0; c < 3; c++) bg[c] = fg[c];
      break;
    default:  // kBlendNone
      break;
  }
}

}  // namespace jxlh
