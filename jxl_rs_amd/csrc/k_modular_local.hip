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
#include "modular_local_desc.h"
#include "modular_local_device.h"  // Slots, apply_rct, apply_palette, load_some / store_some
#include "modular_ops_device.h"

namespace jxlh {
namespace {

//  * kMixed (jxl_hip_local_extra.h): the slots' planes have strides of their own -- a frame's colour planes beside extra
//    channels' sample stores -- and a grey slot 0 fans out to a.fan, not to the planes of slots 1 and 2.  An
//    instantiation of its own: the other keeps one row offset for all planes.
template <bool kMixed>
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
      if constexpr (kMixed) {
        const size_t gy = (size_t)g.y0 + y, gx = (size_t)g.x0 + x;
        auto put_at = [&](int32_t* plane, size_t stride, int4 v) {
          int32_t* p = plane + gy * stride + gx;
          if (full) gstore_i4<true>(p, v);
          else store_some(p, v, cnt);
        };
        if (g.n_channels > 0) put_at(a.out[0], a.slot_stride[0], s.r0);
        if (g.n_channels > 1) put_at(a.out[1], a.slot_stride[1], s.r1);
        if (g.n_channels > 2) put_at(a.out[2], a.slot_stride[2], s.r2);
        if (g.n_channels > 3) put_at(a.out[3], a.slot_stride[3], s.r3);
        if (a.fan_grey) {
          put_at(a.fan[0], a.slot_stride[0], s.r0);
          put_at(a.fan[1], a.slot_stride[0], s.r0);
        }
        continue;
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
  if (a.mixed) hipLaunchKernelGGL(k_modular_local<true>, dim3(a.n_items), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_modular_local<false>, dim3(a.n_items), dim3(256), 0, s, a);
}

}  // namespace jxlh
