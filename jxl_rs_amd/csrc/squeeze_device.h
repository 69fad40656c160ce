// The inverse squeeze's arithmetic on the device: what the whole-plane kernels (k_squeeze.hip) and the group-local ones
// (k_modular_local_squeeze.hip) share.
#pragma once
#include "jxlh_internal.h"
#include "modular_ops_device.h"  // wadd / wsub

namespace jxlh {
namespace {

// smooth_tendency_impl (squeeze.rs:107-141), a = prev, b = avg, c = next_avg.
// The reference clamps with two parity tricks:
//     if (x > 2|a-b| + (x & 1)) x = 2|a-b| + 1;      if (x + (x & 1) > 2|b-c|) x = 2|b-c|;
// Both bounds are even, so whatever the parity of x they reduce to x = min(x, 2|a-b| + 1) and
// x = min(x, 2|b-c|) (x even: x > t <=> x >= t + 2; x odd: x > t + 1 <=> x >= t + 3; x == t + 1 is a
// fixed point) -- also for wrapped operands, since t + 1 and x + 1 cannot overflow (t is even, x is a
// quarter of a 31-bit sum).  That turns eight dependent compare/select operations of the serial chain
// into one v_min3_i32; the sign is applied as (x ^ s) - s.
__device__ __forceinline__ int32_t smooth_tendency(int32_t a, int32_t b, int32_t c) {
  const int32_t a_b = wsub(a, b), b_c = wsub(b, c), a_c = wsub(a, c);
  const int32_t abs_a_b = max(a_b, wsub(0, a_b));
  const int32_t abs_b_c = max(b_c, wsub(0, b_c));
  const int32_t abs_a_c = max(a_c, wsub(0, a_c));
  const bool skip = (b_c != 0) && (a_b != 0) && ((a_b ^ b_c) < 0);
  const int32_t abs_a_b_3 = __mulhi(abs_a_b, 0x55555556);
  int32_t x = wadd(wadd(2, abs_a_c), abs_a_b_3) >> 2;
  const int32_t t1 = (int32_t)(((uint32_t)abs_a_b << 1) + 1u);
  const int32_t u = (int32_t)((uint32_t)abs_b_c << 1);
  x = min(min(x, t1), u);
  if (skip) x = 0;
  const int32_t sgn = a_c >> 31;
  return wsub(x ^ sgn, sgn);
}

// unsqueeze_impl (squeeze.rs:171-185) around smooth_tendency, restated for the serial chain.  One wave owns a line, so
// a step costs (instructions on the dependent path) x 8 cycles (tools/valu_latency.hip: 8 cycles between dependent
// VALU instructions of a lone wave, 5 between independent ones); the step is therefore written on the state
//     d = prev_b - avg                      (a_b of smooth_tendency_impl)
// with everything that does not depend on it moved off the path:
//     b_c = avg - next, sm = sign mask of b_c, bc = |b_c|        (per step constants)
//     e   = d with the sign of b_c applied: the tendency is non-zero only for e >= 0 (prev, avg, next monotone:
//           a_b and b_c of one sign -- `skip` of the reference), and then |a_b| = e, |a_c| = e + bc
//     x   = max(0, min3((e + e/3 + bc + 2) >> 2, 2e + 1, 2bc))   (e < 0 makes 2e + 1 negative: the max is the skip)
//     diff = res + sign(b_c) * x
//     h   = diff - trunc(diff / 2) = (diff + 1 + (diff >> 31)) >> 1
//     b = avg - h, a = b + diff (off the path), and the next state d' = b - next = b_c - h.
// Eleven dependent instructions instead of about twenty-four; bit-equal to the form above wherever the reference's
// i32 SIMD arithmetic does not wrap (test_unsqueeze_large_magnitudes: +-2^28).
__device__ __forceinline__ uint32_t xad(uint32_t a, uint32_t b, uint32_t c) { return (a ^ b) + c; }  // v_xad_u32
__device__ __forceinline__ void unsqueeze_step(int32_t avg, int32_t res, int32_t next_avg, int32_t& d, int32_t& a,
                                               int32_t& b) {
  // off the dependent path
  const int32_t b_c = wsub(avg, next_avg);
  const uint32_t sm = (uint32_t)(b_c >> 31), nsm = (uint32_t)b_c >> 31;
  const uint32_t bc = xad((uint32_t)b_c, sm, nsm);
  const uint32_t k2 = bc + 2u, u = bc << 1, rs = (uint32_t)res + nsm;
  // the chain
  const int32_t e = (int32_t)xad((uint32_t)d, sm, nsm);
  const int32_t e3 = __mulhi(e, 0x55555556);
  const int32_t s = (int32_t)((uint32_t)e + (uint32_t)e3 + k2) >> 2;
  const int32_t t1 = (int32_t)(((uint32_t)e << 1) + 1u);
  const int32_t x = max(min(min(s, t1), (int32_t)u), 0);
  const int32_t diff = (int32_t)xad((uint32_t)x, sm, rs);
  const int32_t h = (int32_t)((uint32_t)diff + (uint32_t)(diff >> 31) + 1u) >> 1;
  d = wsub(b_c, h);
  b = wsub(avg, h);
  a = wadd(b, diff);
}

}  // namespace
}  // namespace jxlh
