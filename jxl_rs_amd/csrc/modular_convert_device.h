// ConvertModularToF32Stage, floating-point samples (convert.rs:416-486 int_to_float / int_to_float_generic), shared by
// the whole-plane conversion (k_modular.hip) and the Modular frame's intake (k_modular_frame.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace jxlh {
// a `bits`-bit float with `exp_bits` exponent bits stored in an integer -> binary32
__device__ __forceinline__ float float_sample_to_f32(uint32_t f, uint32_t bits, uint32_t exp_bits) {
  const int exp_bias = (1 << (exp_bits - 1)) - 1;
  const uint32_t sign_shift = bits - 1, mant_bits = bits - exp_bits - 1, mant_shift = 23 - mant_bits;
  const bool signbit = (f >> sign_shift) != 0;
  f &= (sign_shift >= 32 ? 0xffffffffu : (1u << sign_shift) - 1u);
  uint32_t r;
  if (f == 0) {
    r = signbit ? 0x80000000u : 0u;
  } else {
    int exp = (int)(f >> mant_bits);
    uint32_t mantissa = f & ((1u << mant_bits) - 1u);
    if (exp == (1 << exp_bits) - 1) {  // NaN or infinity
      r = (signbit ? 0x80000000u : 0u) | 0xffu << 23 | mantissa << mant_shift;
    } else {
      mantissa <<= mant_shift;
      if (exp == 0 && exp_bits < 8) {  // subnormal: normalise
        while ((mantissa & 0x800000u) == 0) {
          mantissa <<= 1;
          exp -= 1;
        }
        exp += 1;
        mantissa &= 0x7fffffu;  // the leading 1 is implicit now
      }
      exp -= exp_bias;
      exp += 127;
      r = (signbit ? 0x80000000u : 0u) | (uint32_t)exp << 23 | mantissa;
    }
  }
  return __uint_as_float(r);
}
}  // namespace jxlh
