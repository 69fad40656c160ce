// Group-local Modular transforms: the descriptors a batch uploads, as the kernels of k_modular_local*.hip read them and
// as the batch plan (modular_local_plan.h) fills them.  Plain C++ (no device, no context): the layouts are the contract
// between the two, so nothing here may depend on who includes it.
#pragma once
#include <stdint.h>

#include "../../include/jxl_hip.h"

namespace jxlh {

// k_modular_local.hip: the group-local transforms of a batch of groups in one launch.  A group's lowered program
// (modular_local_host.h) as the kernel reads it -- workgroup-uniform, fetched through scalar loads --, and the flat work
// list of (group, first row) items; an item covers rows_per_item rows of its group.
constexpr uint32_t kLocalLdsEntries = 4096;    // palette entries staged in LDS per workgroup (16 KiB)
constexpr uint32_t kLocalNoLds = 0xffffffffu;  // LocalOpDev::lds_off of a palette read from global memory
constexpr uint32_t kLocalItemSamples = 8192;   // samples of one channel a work item covers (32 rows of a 256-wide group)
struct LocalOpDev {
  uint32_t kind, rct_op, n_slots;
  uint32_t in_slot[3], out_slot[4];
  uint32_t num_colors, lds_off;
  uint64_t pal_off;  // samples into the arena
};
struct LocalGroupDev {
  uint32_t x0, y0, w, h;
  uint32_t n_channels, n_ops, coded_stride;
  uint32_t vec;            // 1: every row of the group starts 16-byte aligned on both sides (16-byte accesses)
  uint32_t rows_per_item;  // rows per work item
  uint32_t lanes_x_log2;   // threads of the workgroup along x: 1 << lanes_x_log2 (four samples each), the rest along y
  uint32_t slot_mask;      // bit s: slot s is loaded from slot_off[s]
  uint32_t lds_entries;    // palette entries this group stages
  uint64_t slot_off[4];    // samples into the arena
  LocalOpDev ops[4];
};
struct LocalItem {
  uint32_t group, row0;
};
// k_modular_local_palette.hip: groups with GENERAL palettes (delta entries under a predictor != 0: jxl_hip_local_palette.h)
// run phase by phase.  A channel slot of such a group lives, between phases, in one of these places:
enum : uint32_t { kLpNone = 0, kLpArena = 1, kLpOut = 2, kLpScratch = 3 };
struct LpPlane {
  uint64_t off;     // kLpArena / kLpScratch: samples into the arena / the scratch block, of the group's first sample
  uint32_t stride;  // kLpArena / kLpScratch: samples between rows
  uint32_t space;   // kLp*; kLpOut: plane `slot` of the launch at the group's rect
};
// the weighted predictor's header as the kernels take it (WpHeader, modular/predict.rs)
struct WpParams {
  uint32_t w[4];
  int32_t p1c, p2c, p3c[5];
};
constexpr int kLpRows = 64;                // rows of a group one workgroup (ONE wavefront: a row per lane) walks at a time
constexpr int kLpChunk = 32;               // wavefront steps between two visits to global memory
constexpr uint32_t kLpLdsEntries = 2048;   // entries of ONE channel's palette row staged in LDS (8 KiB)
constexpr uint32_t kLpMaxPhases = 2 * JXLH_LOCAL_MAX_STEPS + 1;  // point-wise phases are even, palette phases odd
// one general palette of one group; the workgroup of output channel c reads row c of the palette
struct LpJobDev {
  uint32_t x0, y0, w, h;
  LpPlane index;           // kLpArena or kLpScratch: never a plane this job writes
  uint64_t pal_off;        // samples into the arena; n_slots rows of palette_size values
  uint32_t palette_size;   // num_colors + num_deltas
  uint32_t num_deltas, predictor, n_slots;
  uint32_t out_slot[4];
  uint32_t lds;            // 1: the palette row is staged in LDS (palette_size <= kLpLdsEntries)
  uint32_t pad;
  uint64_t wp_rows_off;    // predictor 6, h > kLpRows: samples into scratch; per channel 2 x 5 rows of w (TE, E0..E3)
  WpParams wp;
};
// one point-wise phase of one such group: k_modular_local's pass with a place per slot on either side
struct LpPhaseDev {
  uint32_t x0, y0, w, h;
  uint32_t n_ops;
  uint32_t fan;            // 1: slot 0 also goes to planes 1 and 2 (a grey group of a frame)
  uint32_t rows_per_item, pad;
  LpPlane src[4];          // kLpNone: the slot holds nothing yet (zero)
  LpPlane dst[4];          // kLpNone: not stored; kLpOut or kLpScratch
  LocalOpDev ops[4];       // lds_off unused: palettes are read from global memory
};
// k_modular_local_squeeze.hip: the inverse squeeze of a batch of groups (jxl_hip_local_squeeze.h).  A CHAIN is one image
// channel of one group: its base plane and, level by level, a residual plane, all in the arena.  Levels [0, n_lds) run in
// the LDS launch (one workgroup per chain), level n_lds + k in streamed launch k (64 lines per workgroup).  Level i's
// output is the destination rect when it is the chain's last, else the chain's scratch plane i & 1, rows out_w apart.
constexpr int kLsTile = 128;    // the LDS launch: largest plane side (= JXLH_SQL_MAX: squeeze_levels_fit decides)
constexpr int kLsLevels = 16;   // = JXLH_LOCAL_SQUEEZE_MAX_LEVELS
constexpr int kLsLines = 64;    // streamed launches: lines per workgroup, a lane each
struct LsLevelDev {
  uint32_t horizontal, out_w, out_h;
  uint32_t res_stride;
  uint64_t res_off;  // samples into the arena; never read when the level has no residuals
};
struct LsChainDev {
  uint32_t x0, y0;   // the group's rect in the destination planes
  uint32_t slot;     // the destination plane
  uint32_t n_levels, n_lds;
  uint32_t base_w, base_h, base_stride;
  uint64_t base_off;        // samples into the arena
  uint64_t scratch_off[2];  // samples into the scratch block
  LsLevelDev lv[kLsLevels];
};

}  // namespace jxlh
