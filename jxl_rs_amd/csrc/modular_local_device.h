// The point-wise group-local ops on channel SLOTS kept in registers, four samples of a row per lane: what
// k_modular_local (k_modular_local.hip) and the point-wise phases of groups with general palettes
// (k_modular_local_phase, k_modular_local_palette.hip) share.
#pragma once
#include "jxlh_internal.h"
#include "modular_ops_device.h"

namespace jxlh {
namespace {

// four named registers, not an array: a select chain over array elements is folded back into a dynamically indexed
// load, which puts the array in scratch
struct Slots {
  int4 r0, r1, r2, r3;
};

__device__ __forceinline__ int32_t pick(uint32_t i, int32_t a, int32_t b, int32_t c, int32_t d) {
  return i == 0 ? a : i == 1 ? b : i == 2 ? c : d;
}
__device__ __forceinline__ int4 slot_get(const Slots& s, uint32_t i) {
  return make_int4(pick(i, s.r0.x, s.r1.x, s.r2.x, s.r3.x), pick(i, s.r0.y, s.r1.y, s.r2.y, s.r3.y),
                   pick(i, s.r0.z, s.r1.z, s.r2.z, s.r3.z), pick(i, s.r0.w, s.r1.w, s.r2.w, s.r3.w));
}
__device__ __forceinline__ int4 keep_or(bool take, int4 v, int4 old) {
  return make_int4(take ? v.x : old.x, take ? v.y : old.y, take ? v.z : old.z, take ? v.w : old.w);
}
__device__ __forceinline__ void slot_put(Slots& s, uint32_t i, int4 v) {
  s.r0 = keep_or(i == 0, v, s.r0);
  s.r1 = keep_or(i == 1, v, s.r1);
  s.r2 = keep_or(i == 2, v, s.r2);
  s.r3 = keep_or(i == 3, v, s.r3);
}

template <int OP>
__device__ __forceinline__ void rct4(const int4 a, const int4 b, const int4 c, int4& x, int4& y, int4& z) {
  rct_op<OP>(a.x, b.x, c.x, x.x, y.x, z.x);
  rct_op<OP>(a.y, b.y, c.y, x.y, y.y, z.y);
  rct_op<OP>(a.z, b.z, c.z, x.z, y.z, z.z);
  rct_op<OP>(a.w, b.w, c.w, x.w, y.w, z.w);
}

__device__ __forceinline__ void apply_rct(Slots& s, const LocalOpDev& op) {
  const int4 a = slot_get(s, op.in_slot[0]), b = slot_get(s, op.in_slot[1]), c = slot_get(s, op.in_slot[2]);
  int4 x, y, z;
  switch (op.rct_op) {
    default:
    case 0: rct4<0>(a, b, c, x, y, z); break;
    case 1: rct4<1>(a, b, c, x, y, z); break;
    case 2: rct4<2>(a, b, c, x, y, z); break;
    case 3: rct4<3>(a, b, c, x, y, z); break;
    case 4: rct4<4>(a, b, c, x, y, z); break;
    case 5: rct4<5>(a, b, c, x, y, z); break;
    case 6: rct4<6>(a, b, c, x, y, z); break;
  }
  slot_put(s, op.out_slot[0], x);
  slot_put(s, op.out_slot[1], y);
  slot_put(s, op.out_slot[2], z);
}

// `palette`: LDS or global memory (the caller's branch decides: the address space is known at each call site)
__device__ __forceinline__ void apply_palette(Slots& s, const LocalOpDev& op, const int32_t* __restrict__ palette,
                                              int bit_depth) {
  const int4 idx = slot_get(s, op.in_slot[0]);
  const int nc = (int)op.num_colors;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    if (c < (int)op.n_slots) {
      int4 v;
      v.x = palette_value(palette, (size_t)nc, idx.x, c, nc, bit_depth);
      v.y = palette_value(palette, (size_t)nc, idx.y, c, nc, bit_depth);
      v.z = palette_value(palette, (size_t)nc, idx.z, c, nc, bit_depth);
      v.w = palette_value(palette, (size_t)nc, idx.w, c, nc, bit_depth);
      slot_put(s, op.out_slot[c], v);
    }
  }
}

// the first cnt (1..3) samples of a ragged row end, or all four of an unaligned group
__device__ __forceinline__ int4 load_some(const int32_t* __restrict__ p, uint32_t cnt) {
  int4 v = make_int4(0, 0, 0, 0);
  v.x = p[0];
  if (cnt > 1) v.y = p[1];
  if (cnt > 2) v.z = p[2];
  if (cnt > 3) v.w = p[3];
  return v;
}
__device__ __forceinline__ void store_some(int32_t* __restrict__ p, int4 v, uint32_t cnt) {
  p[0] = v.x;
  if (cnt > 1) p[1] = v.y;
  if (cnt > 2) p[2] = v.z;
  if (cnt > 3) p[3] = v.w;
}

}  // namespace
}  // namespace jxlh
