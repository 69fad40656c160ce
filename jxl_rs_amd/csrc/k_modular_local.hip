// Group-local Modular transforms (frame/modular/transforms/apply_local.rs): the inverse RCTs and non-delta palettes a
// lossless encoder chose PER GROUP, for every group of a batch in one launch.  One streaming pass: the group's coded
// channels come out of the arena (<= 12 B/px, 4 B/px for a three-channel palette), up to four finished channels go to
// raster planes at the group's rect (12 B/px for a colour frame).
//
//  * Work list: blockIdx.x -> LocalItem (group, first row), built on the host.  The group's lowered program
//    (LocalGroupDev) is the same for the whole workgroup: its address derives from blockIdx alone, so its fields arrive
//    through scalar loads and the step dispatch is a uniform branch.
//  * Each lane owns four consecutive samples of a row: 16-byte non-temporal loads and stores when every row of the group
//    starts 16-byte aligned on both sides (LocalGroupDev::vec, decided on the host), four 4-byte accesses otherwise; the
//    last lane of a ragged row handles w % 4 samples one by one.  Nothing outside the rect is read or written.
//  * The <= 4 channel values of a sample stay in registers (slots) across all steps; a step names its slots with uniform
//    indices that are resolved by unrolled compares, never by indexing an array dynamically: no scratch.
//  * Palettes are staged in LDS once per workgroup while the group's palettes together hold <= kLocalLdsEntries values
//    (16 KiB: eight workgroups of 256 threads, the CU's full 32 waves, need 128 of its 160 KiB); a larger palette is read
//    from global memory.  Implicit and negative indices never touch the table (palette_value).
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

__global__ __launch_bounds__(256) void k_modular_local(const LocalLaunch a) {
  __shared__ int32_t s_pal[kLocalLdsEntries];
  const LocalItem item = a.items[blockIdx.x];
  const LocalGroupDev& g = a.groups[item.group];
  const int32_t* __restrict__ arena = a.arena;
  const uint32_t tid = threadIdx.x;
  if (g.lds_entries > 0) {
    for (uint32_t k = 0; k < g.n_ops; k++) {
      const LocalOpDev& op = g.ops[k];
      if (op.kind == JXLH_LOCAL_PALETTE && op.lds_off != kLocalNoLds) {
        const uint32_t cnt = op.n_slots * op.num_colors;  // the meta channel's rows are contiguous
        for (uint32_t i = tid; i < cnt; i += 256) s_pal[op.lds_off + i] = arena[op.pal_off + i];
      }
    }
    __syncthreads();
  }
  const uint32_t w = g.w, lx = g.lanes_x_log2;
  const uint32_t lanes_x = 1u << lx, rows_pass = 256u >> lx;
  const uint32_t tx = tid & (lanes_x - 1), ty = tid >> lx;
  const uint32_t row_end = item.row0 + min(g.rows_per_item, g.h - item.row0);  // (planes are shorter than 2^31 rows)
  const uint32_t nvx = (w + 3) >> 2;
  const bool vec = g.vec != 0;
  const uint32_t n_store = (a.fan_grey && g.n_channels == 1) ? 3u : g.n_channels;
  const bool fan = a.fan_grey && g.n_channels == 1;
  for (uint32_t y = item.row0 + ty; y < row_end; y += rows_pass) {
    const size_t src_row = (size_t)y * g.coded_stride;
    const size_t dst_row = (size_t)(g.y0 + y) * a.out_stride + g.x0;
    for (uint32_t xv = tx; xv < nvx; xv += lanes_x) {
      const uint32_t x = xv * 4;
      const uint32_t cnt = min(4u, w - x);
      const bool full = vec && cnt == 4;
      const int4 zero = make_int4(0, 0, 0, 0);
      auto fetch = [&](int t) {
        if (!(g.slot_mask >> t & 1)) return zero;
        const int32_t* p = arena + g.slot_off[t] + src_row + x;
        return full ? gload_i4<true>(p) : load_some(p, cnt);
      };
      Slots s;
      s.r0 = fetch(0);
      s.r1 = fetch(1);
      s.r2 = fetch(2);
      s.r3 = fetch(3);
      for (uint32_t k = 0; k < g.n_ops; k++) {
        const LocalOpDev& op = g.ops[k];
        if (op.kind == JXLH_LOCAL_RCT) {
          apply_rct(s, op);
        } else if (op.lds_off != kLocalNoLds) {
          apply_palette(s, op, s_pal + op.lds_off, a.bit_depth);
        } else {
          apply_palette(s, op, arena + op.pal_off, a.bit_depth);
        }
      }
      auto put = [&](uint32_t c, int4 v) {
        if (c >= n_store) return;
        int32_t* p = a.out[c] + dst_row + x;
        if (full) gstore_i4<true>(p, fan ? s.r0 : v);
        else store_some(p, fan ? s.r0 : v, cnt);
      };
      put(0, s.r0);
      put(1, s.r1);
      put(2, s.r2);
      put(3, s.r3);
    }
  }
}

}  // namespace

void launch_modular_local(hipStream_t s, const LocalLaunch& a) {
  if (a.n_items == 0) return;
  hipLaunchKernelGGL(k_modular_local, dim3(a.n_items), dim3(256), 0, s, a);
}

}  // namespace jxlh
