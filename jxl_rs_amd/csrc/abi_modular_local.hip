// C ABI, group-local Modular transforms (jxlh_modular_local_lower, jxlh_modular_local_transforms,
// jxlh_frame_set_modular_groups* and their _general forms of jxl_hip_local_palette.h): every group's transform list is
// lowered on the host (modular_local_host.h), the lowered programs and a flat (group, row chunk) work list go up in one
// copy from a pinned block, a host arena in one more, and the whole batch is one launch of k_modular_local.  Groups with
// GENERAL palettes (the _general calls only) follow phase by phase -- one launch per phase for all of them, their
// descriptors in the same block and the same copy.  Groups with a squeeze of their own (the _squeeze calls of
// jxl_hip_local_squeeze.h, lowered by modular_local_squeeze_host.h) run their chains first -- one LDS launch and one
// launch per streamed level index for the whole batch -- and then the same phases on their rects.  Everything that can
// refuse a call is checked before the first copy is enqueued.
#include <algorithm>

#include "jxlh_ctx.h"
#include "modular_local_host.h"
#include "modular_local_squeeze_host.h"
#include "squeeze_plan.h"

namespace jxlh_host {
namespace {

constexpr uint32_t kLocalItemSamples = 8192;  // samples of one channel a work item covers (32 rows of a 256-wide group)
constexpr uint32_t kLpMaxPhases = 2 * JXLH_LOCAL_MAX_STEPS + 1;

jxlh_status refuse_group(jxlh_ctx* ctx, jxlh_status st, size_t g, const char* why, size_t* first_bad) {
  if (first_bad) *first_bad = g;
  if (ctx) ctx->last_error = "group " + std::to_string(g) + ": " + why;
  return st;
}

struct LocalDest {
  int32_t* out[4] = {nullptr, nullptr, nullptr, nullptr};
  uint32_t n_out = 0, w = 0, h = 0;
  size_t stride = 0;
  bool frame = false;  // the frame's sample planes: 3 or 1 (fanned out) channels per group
};

// what the phases of the groups with general palettes launch: phase p's descriptors (LpPhaseDev for even p, LpJobDev for
// odd p) and work items, and the scratch the batch needs
struct GeneralBatch {
  std::vector<LpPhaseDev> pointwise[kLpMaxPhases];
  std::vector<LpJobDev> jobs[kLpMaxPhases];
  std::vector<LocalItem> items[kLpMaxPhases];
  bool weighted[kLpMaxPhases] = {}, lds_palette[kLpMaxPhases] = {};
  uint64_t scratch = 0;  // samples
  bool any() const {
    for (const auto& v : items)
      if (!v.empty()) return true;
    return false;
  }
};

// One group with general palettes, cut into phases (jxl_hip_local_palette.h).  Between phases a slot is in the arena
// (a coded channel nothing has touched yet), in the destination rect, or -- the index channel of the next general
// palette, which shares its slot with that palette's output channel 0 while the other channels' workgroups still read
// it -- in scratch.  A point-wise phase loads every slot that is somewhere and stores what it changed (what the next
// palette overwrites excepted); the last one leaves every channel in the destination rect.
// init (a group of the squeeze calls): where each slot is when the phases start -- a coded channel of its own stride, or
// the destination rect, where the slot's squeeze chain ends.  Such a group may have no general palette at all: its one
// point-wise phase is phase 0.
void plan_general_group(const jxlh_local_group& g, const jxlh_local_general_program& prog, const jxlh_wp_header* wp,
                        bool fan, GeneralBatch& b, const LpPlane* init = nullptr) {
  LpPlane loc[4] = {};
  for (uint32_t k = 0; k < prog.n_coded; k++)
    loc[prog.coded_slot[k]] = init ? init[prog.coded_slot[k]] : LpPlane{g.coded_offset[k], g.coded_stride, kLpArena};
  const uint32_t nvx = (g.w + 3) / 4, rows_per_item = std::max(1u, kLocalItemSamples / (4 * nvx));
  bool have_copy = false;
  uint64_t copy_off = 0;
  auto index_copy = [&]() {  // one per group: a copy is dead once its palette has run
    if (!have_copy) {
      copy_off = b.scratch;
      b.scratch += (uint64_t)g.w * g.h;
      have_copy = true;
    }
    return LpPlane{copy_off, g.w, kLpScratch};
  };
  auto pointwise = [&](uint32_t phase, uint32_t op0, uint32_t op1, const jxlh_local_general_op* next) {
    LpPhaseDev d{};
    d.x0 = g.x0, d.y0 = g.y0, d.w = g.w, d.h = g.h;
    d.rows_per_item = rows_per_item;
    bool changed[4] = {};
    for (uint32_t i = op0; i < op1; i++) {
      const jxlh_local_general_op& p = prog.ops[i];
      LocalOpDev& q = d.ops[d.n_ops++];
      q.kind = p.kind, q.rct_op = p.rct_op, q.n_slots = p.n_slots, q.num_colors = p.num_colors, q.pal_off = p.palette_offset;
      q.lds_off = kLocalNoLds;
      for (int k = 0; k < 3; k++) q.in_slot[k] = p.in_slot[k];
      for (int k = 0; k < 4; k++) q.out_slot[k] = p.out_slot[k];
      for (uint32_t k = 0; k < p.n_slots; k++) changed[p.out_slot[k]] = true;
    }
    for (int t = 0; t < 4; t++) d.src[t] = loc[t];
    bool any = false;
    for (uint32_t t = 0; t < g.n_channels; t++) {
      LpPlane to{0, 0, kLpNone};
      if (!next) {
        if (changed[t] || loc[t].space != kLpOut) to.space = kLpOut;
      } else if (t == next->in_slot[0]) {
        if (changed[t] || loc[t].space == kLpOut) to = index_copy();
      } else if (changed[t]) {
        bool overwritten = false;
        for (uint32_t k = 0; k < next->n_slots; k++) overwritten = overwritten || next->out_slot[k] == t;
        if (overwritten) loc[t] = LpPlane{0, 0, kLpNone};
        else to.space = kLpOut;
      }
      if (to.space != kLpNone) {
        d.dst[t] = loc[t] = to;
        any = true;
      }
    }
    if (!next && fan) d.fan = 1, any = true;
    if (!any) return;
    const uint32_t id = (uint32_t)b.pointwise[phase].size();
    b.pointwise[phase].push_back(d);
    for (uint64_t r = 0; r < g.h; r += rows_per_item) b.items[phase].push_back(LocalItem{id, (uint32_t)r});
  };
  uint32_t i = 0, phase = 0;
  bool seen = false;
  while (i < prog.n_ops) {
    uint32_t e = i;
    while (e < prog.n_ops && prog.ops[e].kind != JXLH_LOCAL_GENERAL_PALETTE) e++;
    if (e == prog.n_ops) break;
    const jxlh_local_general_op& p = prog.ops[e];
    pointwise(p.phase - 1, i, e, &p);
    LpJobDev j{};
    j.x0 = g.x0, j.y0 = g.y0, j.w = g.w, j.h = g.h;
    j.index = loc[p.in_slot[0]];  // the arena or scratch: pointwise() moved it out of the destination rect
    j.pal_off = p.palette_offset;
    j.palette_size = p.num_colors, j.num_deltas = p.num_deltas, j.predictor = p.predictor, j.n_slots = p.n_slots;
    for (int k = 0; k < 4; k++) j.out_slot[k] = p.out_slot[k];
    j.lds = p.num_colors <= kLpLdsEntries;
    if (p.predictor == 6) {
      j.wp.p1c = (int32_t)wp->p1c, j.wp.p2c = (int32_t)wp->p2c;
      const uint32_t p3[5] = {wp->p3ca, wp->p3cb, wp->p3cc, wp->p3cd, wp->p3ce}, ww[4] = {wp->w0, wp->w1, wp->w2, wp->w3};
      for (int k = 0; k < 5; k++) j.wp.p3c[k] = (int32_t)p3[k];
      for (int k = 0; k < 4; k++) j.wp.w[k] = ww[k];
      b.weighted[p.phase] = true;
      if (g.h > (uint32_t)kLpRows) {  // state rows between the bands of a channel's workgroup: two sets of five
        j.wp_rows_off = b.scratch;
        b.scratch += (uint64_t)p.n_slots * 10 * g.w;
      }
    }
    b.lds_palette[p.phase] = b.lds_palette[p.phase] || j.lds;
    const uint32_t id = (uint32_t)b.jobs[p.phase].size();
    b.jobs[p.phase].push_back(j);
    for (uint32_t c = 0; c < p.n_slots; c++) b.items[p.phase].push_back(LocalItem{id, c});
    for (uint32_t k = 0; k < p.n_slots; k++) loc[p.out_slot[k]] = LpPlane{0, 0, kLpOut};
    phase = p.phase;
    seen = true;
    i = e + 1;
  }
  pointwise(seen ? phase + 1 : 0, i, prog.n_ops, nullptr);
}

// the groups, coded channels and squeeze parameters of the squeeze calls (jxl_hip_local_squeeze.h)
struct SqueezeIn {
  const jxlh_local_squeeze_group* groups;
  const jxlh_local_coded_channel* coded;
  size_t n_coded;
  const jxlh_squeeze_params* params;
  size_t n_params;
};
// what the squeeze chains of a batch launch: the LDS launch's items (chain, 0) and streamed launch k's (chain, first line)
struct SqueezeBatch {
  std::vector<LsChainDev> chains;
  std::vector<LocalItem> lds_items;
  std::vector<LocalItem> level_items[kLsLevels];
  bool any() const { return !chains.empty(); }
};

// One group of the squeeze calls that does not run as a plain / general group: every squeezed channel becomes a chain
// that ends in the destination rect, every other one stays in the arena; the steps in front follow as phases.
void plan_squeeze_group(const jxlh_local_group& g, const jxlh_local_squeeze_group& sg, const jxlh_local_squeeze_program& prog,
                        const jxlh_local_coded_channel* coded, const jxlh_wp_header* wp, bool fan, GeneralBatch& gb,
                        SqueezeBatch& sb) {
  LpPlane init[4] = {};
  for (uint32_t k = 0; k < prog.general.n_coded; k++) {
    const uint32_t slot = prog.general.coded_slot[k];
    const jxlh_local_squeeze_chain& ch = prog.chains[k];
    const jxlh_local_coded_channel& bc = coded[sg.coded_first + ch.base];
    if (ch.n_levels == 0) {
      init[slot] = LpPlane{bc.offset, bc.stride, kLpArena};
      continue;
    }
    LsChainDev c{};
    c.x0 = g.x0, c.y0 = g.y0, c.slot = slot;
    c.n_levels = ch.n_levels;
    c.base_w = ch.base_w, c.base_h = ch.base_h, c.base_stride = bc.stride, c.base_off = bc.offset;
    jxlh_squeeze_level fit[kLsLevels] = {};
    for (uint32_t i = 0; i < ch.n_levels; i++) {
      const jxlh_local_squeeze_level& lv = ch.levels[i];
      const jxlh_local_coded_channel& rc = coded[sg.coded_first + lv.res];
      const bool has_res = rc.w > 0 && rc.h > 0;
      c.lv[i] = LsLevelDev{lv.horizontal, lv.out_w, lv.out_h, has_res ? rc.stride : 0u, has_res ? rc.offset : 0u};
      fit[i].horizontal = lv.horizontal, fit[i].out_w = lv.out_w, fit[i].out_h = lv.out_h;
    }
    // the LDS launch takes the first levels while every plane fits its tiles (squeeze_plan.h)
    uint32_t n_lds = 0;
    while (n_lds < ch.n_levels && ch.levels[n_lds].out_w <= (uint32_t)kLsTile && ch.levels[n_lds].out_h <= (uint32_t)kLsTile) n_lds++;
    while (n_lds >= 1 && !jxlh::squeeze_levels_fit((int)n_lds, fit, ch.base_w, ch.base_h)) n_lds--;
    c.n_lds = n_lds;
    // level i's output, unless it is the last, goes to the chain's scratch plane i & 1: each as large as the largest it holds
    uint64_t need[2] = {0, 0};
    for (uint32_t i = n_lds > 0 ? n_lds - 1 : 0; i + 1 < ch.n_levels; i++)
      need[i & 1] = std::max(need[i & 1], (uint64_t)ch.levels[i].out_w * ch.levels[i].out_h);
    for (int q = 0; q < 2; q++) {
      c.scratch_off[q] = gb.scratch;
      gb.scratch += need[q];
    }
    const uint32_t id = (uint32_t)sb.chains.size();
    sb.chains.push_back(c);
    if (n_lds > 0) sb.lds_items.push_back(LocalItem{id, 0});
    for (uint32_t k2 = 0; n_lds + k2 < ch.n_levels; k2++) {
      const jxlh_local_squeeze_level& lv = ch.levels[n_lds + k2];
      const uint32_t n_lines = lv.horizontal ? lv.out_h : lv.out_w;
      for (uint32_t l = 0; l < n_lines; l += (uint32_t)kLsLines) sb.level_items[k2].push_back(LocalItem{id, l});
    }
    init[slot] = LpPlane{0, 0, kLpOut};
  }
  plan_general_group(g, prog.general, wp, fan, gb, init);
}

// checks, lowering, upload, launch; nothing is enqueued unless every group passed.  general: the _general calls (wp: one
// header per group, or null)
jxlh_status local_enqueue(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples, const jxlh_local_group* groups,
                          size_t n, uint32_t bit_depth, const LocalDest& d, size_t* first_bad, bool general = false,
                          const jxlh_wp_header* wp = nullptr, const SqueezeIn* sq = nullptr) {
  if (n > 0x7fffffffu || d.w > 0x7fffffffu || d.h > 0x7fffffffu) return JXLH_ERR_INVALID_ARGUMENT;
  std::vector<LocalGroupDev> dev(n);
  std::vector<LocalItem> items;
  GeneralBatch gb;
  SqueezeBatch sb;
  bool dst_aligned = (d.stride & 3) == 0 && (reinterpret_cast<uintptr_t>(arena) & 15) == 0;
  for (uint32_t c = 0; c < d.n_out; c++) dst_aligned = dst_aligned && (reinterpret_cast<uintptr_t>(d.out[c]) & 15) == 0;
  for (size_t gi = 0; gi < n; gi++) {
    jxlh_local_program prog;
    jxlh_local_general_program gprog;
    const char* why = "";
    // a group of the squeeze calls: one without squeeze levels whose coded channels share a stride runs as a group of
    // the _general calls does (gtmp says it in their terms); any other one as chains and phases
    jxlh_local_group gtmp{};
    jxlh_local_squeeze_program sprog;
    bool chains = false;
    if (sq) {
      const jxlh_local_squeeze_group& sg = sq->groups[gi];
      if (jxlh_status st = local_lower_squeeze_group(sg, sq->coded, sq->n_coded, sq->params, sq->n_params, wp ? &wp[gi] : nullptr,
                                                     bit_depth, arena_samples, &sprog, &why))
        return refuse_group(ctx, st, gi, why, first_bad);
      gtmp.x0 = sg.x0, gtmp.y0 = sg.y0, gtmp.w = sg.w, gtmp.h = sg.h;
      gtmp.n_channels = sg.n_channels, gtmp.n_steps = sg.n_steps;
      for (uint32_t k = 0; k < sg.n_steps; k++) gtmp.steps[k] = sg.steps[k];
      for (uint32_t k = 0; k < sprog.general.n_coded; k++) chains = chains || sprog.chains[k].n_levels > 0;
      if (!chains) {  // the coded channels are the channels that reach the squeeze, full size
        gtmp.n_coded = sprog.n_coded;
        gtmp.coded_stride = sg.w;
        for (uint32_t k = 0; k < sprog.n_coded && sg.w > 0 && sg.h > 0; k++) {
          const jxlh_local_coded_channel& c = sq->coded[sg.coded_first + k];
          gtmp.coded_offset[k] = c.offset;
          if (k == 0) gtmp.coded_stride = c.stride;
          chains = chains || c.stride != gtmp.coded_stride;
        }
      }
      gprog = sprog.general;
    }
    const jxlh_local_group& g = sq ? gtmp : groups[gi];
    if (!chains)
      if (jxlh_status st = local_lower_core(g, bit_depth, arena_samples, general, wp ? &wp[gi] : nullptr, &prog, &gprog, &why))
        return refuse_group(ctx, st, gi, why, first_bad);
    if (d.frame ? (g.n_channels != 3 && g.n_channels != 1) : g.n_channels > d.n_out)
      return refuse_group(ctx, JXLH_ERR_INVALID_ARGUMENT, gi, d.frame ? "a frame's groups hold 3 channels, or 1 (grey)" : "more channels than out planes", first_bad);
    if ((uint64_t)g.x0 + g.w > d.w || (uint64_t)g.y0 + g.h > d.h)
      return refuse_group(ctx, JXLH_ERR_INVALID_ARGUMENT, gi, "the rect leaves the planes", first_bad);
    LocalGroupDev& o = dev[gi];
    o = LocalGroupDev{};
    if (chains) {
      if (g.w == 0 || g.h == 0) continue;
      plan_squeeze_group(g, sq->groups[gi], sprog, sq->coded, wp ? &wp[gi] : nullptr, d.frame && g.n_channels == 1, gb, sb);
      size_t most = std::max(sb.chains.size(), sb.lds_items.size());
      for (const auto& v : sb.level_items) most = std::max(most, v.size());
      for (const auto& v : gb.items) most = std::max(most, v.size());
      if (most > 0x7fffffffu) return refuse_group(ctx, JXLH_ERR_INVALID_ARGUMENT, gi, "the batch holds more than 2^31 - 1 work items", first_bad);
      continue;
    }
    if (gprog.n_phases > 1) {  // general palettes: this group runs phase by phase, behind the launch of the others
      if (g.w > (1u << 30)) return refuse_group(ctx, JXLH_ERR_INVALID_ARGUMENT, gi, "a predicted palette on a group wider than 2^30", first_bad);
      if (g.w == 0 || g.h == 0) continue;
      plan_general_group(g, gprog, wp ? &wp[gi] : nullptr, d.frame && g.n_channels == 1, gb);
      for (const auto& v : gb.items)
        if (v.size() > 0x7fffffffu) return refuse_group(ctx, JXLH_ERR_INVALID_ARGUMENT, gi, "the batch holds more than 2^31 - 1 work items", first_bad);
      continue;
    }
    o.x0 = g.x0, o.y0 = g.y0, o.w = g.w, o.h = g.h;
    o.n_channels = g.n_channels;
    o.n_ops = prog.n_ops;
    o.coded_stride = g.coded_stride;
    bool vec = dst_aligned && (g.coded_stride & 3) == 0 && (g.x0 & 3) == 0;
    for (uint32_t k = 0; k < prog.n_coded; k++) {
      o.slot_mask |= 1u << prog.coded_slot[k];
      o.slot_off[prog.coded_slot[k]] = g.coded_offset[k];
      vec = vec && (g.coded_offset[k] & 3) == 0;
    }
    o.vec = vec;
    // palettes share the workgroup's LDS block while they fit, in the order they run
    for (uint32_t k = 0; k < prog.n_ops; k++) {
      const jxlh_local_op& p = prog.ops[k];
      LocalOpDev& q = o.ops[k];
      q.kind = p.kind, q.rct_op = p.rct_op, q.n_slots = p.n_slots, q.num_colors = p.num_colors, q.pal_off = p.palette_offset;
      for (int i = 0; i < 3; i++) q.in_slot[i] = p.in_slot[i];
      for (int i = 0; i < 4; i++) q.out_slot[i] = p.out_slot[i];
      q.lds_off = kLocalNoLds;
      if (p.kind == JXLH_LOCAL_PALETTE) {
        const uint64_t entries = (uint64_t)p.n_slots * p.num_colors;
        if (entries <= kLocalLdsEntries - o.lds_entries) {
          q.lds_off = o.lds_entries;
          o.lds_entries += (uint32_t)entries;
        }
      }
    }
    if (g.w == 0 || g.h == 0) continue;
    // threads along x: the smallest power of two that covers the row's 4-sample vectors, at most the workgroup
    const uint32_t nvx = (g.w + 3) / 4;
    uint32_t lx = 0;
    while (lx < 8 && (1u << lx) < nvx) lx++;
    o.lanes_x_log2 = lx;
    o.rows_per_item = std::max(256u >> lx, kLocalItemSamples / (4 * nvx));
    for (uint64_t r = 0; r < g.h; r += o.rows_per_item) items.push_back(LocalItem{(uint32_t)gi, (uint32_t)r});
    if (items.size() > 0x7fffffffu) return refuse_group(ctx, JXLH_ERR_INVALID_ARGUMENT, gi, "the batch holds more than 2^31 - 1 work items", first_bad);
  }
  const bool have_general = gb.any();
  if (items.empty() && !have_general && !sb.any()) return JXLH_OK;
  // ---- from here on the call cannot be refused for its arguments
  // the block: the plain groups' descriptors and items, then per phase its descriptors and items, each 16-byte aligned
  const size_t desc_bytes = round_up(n * sizeof(LocalGroupDev), 16);
  size_t bytes = desc_bytes + round_up(items.size() * sizeof(LocalItem), 16);
  size_t phase_desc[kLpMaxPhases] = {}, phase_items[kLpMaxPhases] = {};
  for (uint32_t p = 0; p < kLpMaxPhases && have_general; p++) {
    phase_desc[p] = bytes;
    bytes += round_up((p & 1) ? gb.jobs[p].size() * sizeof(LpJobDev) : gb.pointwise[p].size() * sizeof(LpPhaseDev), 16);
    phase_items[p] = bytes;
    bytes += round_up(gb.items[p].size() * sizeof(LocalItem), 16);
  }
  // ... then the squeeze chains, the LDS launch's items and each streamed launch's
  size_t chain_desc = 0, lds_items_at = 0, level_items_at[kLsLevels] = {};
  if (sb.any()) {
    chain_desc = bytes;
    bytes += round_up(sb.chains.size() * sizeof(LsChainDev), 16);
    lds_items_at = bytes;
    bytes += round_up(sb.lds_items.size() * sizeof(LocalItem), 16);
    for (int k = 0; k < kLsLevels; k++) {
      level_items_at[k] = bytes;
      bytes += round_up(sb.level_items[k].size() * sizeof(LocalItem), 16);
    }
  }
  HIPCHK(ctx, ctx->local_copied.sync());  // the pinned block's previous content is on its way
  ctx->local_copied.clear();
  if (ctx->local_desc_host.n < bytes) {
    HIPCHK(ctx, ctx->local_desc_host.reset());
    HIPCHK(ctx, ctx->local_desc_host.alloc(bytes + bytes / 2));
  }
  if (jxlh_status st = ensure(ctx, ctx->local_desc, bytes)) return st;
  if (gb.scratch > 0)
    if (jxlh_status st = ensure(ctx, ctx->local_scratch, (size_t)gb.scratch)) return st;
  std::memcpy(ctx->local_desc_host.p, dev.data(), n * sizeof(LocalGroupDev));
  std::memcpy(ctx->local_desc_host.p + desc_bytes, items.data(), items.size() * sizeof(LocalItem));
  for (uint32_t p = 0; p < kLpMaxPhases && have_general; p++) {
    if (p & 1) std::memcpy(ctx->local_desc_host.p + phase_desc[p], gb.jobs[p].data(), gb.jobs[p].size() * sizeof(LpJobDev));
    else std::memcpy(ctx->local_desc_host.p + phase_desc[p], gb.pointwise[p].data(), gb.pointwise[p].size() * sizeof(LpPhaseDev));
    std::memcpy(ctx->local_desc_host.p + phase_items[p], gb.items[p].data(), gb.items[p].size() * sizeof(LocalItem));
  }
  if (sb.any()) {
    std::memcpy(ctx->local_desc_host.p + chain_desc, sb.chains.data(), sb.chains.size() * sizeof(LsChainDev));
    std::memcpy(ctx->local_desc_host.p + lds_items_at, sb.lds_items.data(), sb.lds_items.size() * sizeof(LocalItem));
    for (int k = 0; k < kLsLevels; k++)
      std::memcpy(ctx->local_desc_host.p + level_items_at[k], sb.level_items[k].data(), sb.level_items[k].size() * sizeof(LocalItem));
  }
  const int32_t* arena_dev = arena;
  if (!is_device_ptr(arena)) {
    // one copy; 16-byte alignment of the samples is kept (hipMalloc's and the caller's bases are both taken as they
    // are: the vector path was decided on the caller's base, so an unaligned host arena already runs the scalar path)
    if (jxlh_status st = stage_in(ctx, ctx->local_arena, arena, (size_t)arena_samples)) return st;
    arena_dev = ctx->local_arena.p;
  }
  HIPCHK(ctx, hipMemcpyAsync(ctx->local_desc.p, ctx->local_desc_host.p, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, ctx->local_copied.record(ctx->stream));
  const int depth = (int)std::min(bit_depth, 24u);  // do_palette_step_general: bits_per_sample().min(24), palette.rs:177
  if (!items.empty()) {
    LocalLaunch a{};
    a.arena = arena_dev;
    a.groups = reinterpret_cast<const LocalGroupDev*>(ctx->local_desc.p);
    a.items = reinterpret_cast<const LocalItem*>(ctx->local_desc.p + desc_bytes);
    a.n_items = (uint32_t)items.size();
    for (int c = 0; c < 4; c++) a.out[c] = d.out[c];
    a.n_out = d.n_out;
    a.fan_grey = d.frame ? 1 : 0;
    a.out_stride = d.stride;
    a.bit_depth = depth;
    {
      ScopedKernelTimer t(ctx, "k_modular_local");
      launch_modular_local(ctx->stream, a);
    }
    HIPCHK(ctx, hipGetLastError());
  }
  if (sb.any()) {  // every chain up to its destination rect, ahead of the phases that read it there
    LsLaunch a{};
    a.arena = arena_dev;
    a.scratch = ctx->local_scratch.p;
    for (int c = 0; c < 4; c++) a.out[c] = d.out[c];
    a.out_stride = d.stride;
    a.chains = reinterpret_cast<const LsChainDev*>(ctx->local_desc.p + chain_desc);
    if (!sb.lds_items.empty()) {
      a.items = reinterpret_cast<const LocalItem*>(ctx->local_desc.p + lds_items_at);
      a.n_items = (uint32_t)sb.lds_items.size();
      ScopedKernelTimer t(ctx, "k_modular_local_squeeze_lds");
      launch_modular_local_squeeze_lds(ctx->stream, a);
    }
    for (int k = 0; k < kLsLevels; k++) {
      if (sb.level_items[k].empty()) continue;
      a.items = reinterpret_cast<const LocalItem*>(ctx->local_desc.p + level_items_at[k]);
      a.n_items = (uint32_t)sb.level_items[k].size();
      a.step = (uint32_t)k;
      ScopedKernelTimer t(ctx, "k_modular_local_squeeze_level");
      launch_modular_local_squeeze_level(ctx->stream, a);
    }
    HIPCHK(ctx, hipGetLastError());
  }
  for (uint32_t p = 0; p < kLpMaxPhases && have_general; p++) {
    if (gb.items[p].empty()) continue;
    LpLaunch a{};
    a.arena = arena_dev;
    a.scratch = ctx->local_scratch.p;
    for (int c = 0; c < 4; c++) a.out[c] = d.out[c];
    a.out_stride = d.stride;
    a.bit_depth = depth;
    a.items = reinterpret_cast<const LocalItem*>(ctx->local_desc.p + phase_items[p]);
    a.n_items = (uint32_t)gb.items[p].size();
    if (p & 1) {
      a.jobs = reinterpret_cast<const LpJobDev*>(ctx->local_desc.p + phase_desc[p]);
      a.weighted = gb.weighted[p], a.lds_palette = gb.lds_palette[p];
      ScopedKernelTimer t(ctx, "k_modular_local_palette");
      launch_modular_local_palette(ctx->stream, a);
    } else {
      a.phases = reinterpret_cast<const LpPhaseDev*>(ctx->local_desc.p + phase_desc[p]);
      ScopedKernelTimer t(ctx, "k_modular_local_phase");
      launch_modular_local_phase(ctx->stream, a);
    }
    HIPCHK(ctx, hipGetLastError());
  }
  return JXLH_OK;
}

jxlh_status frame_set_groups(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples, const jxlh_local_group* groups,
                             size_t n, uint32_t sample_format, size_t* first_bad, bool wait, bool general = false,
                             const jxlh_wp_header* wp = nullptr, const SqueezeIn* sq = nullptr) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !arena || (!(sq ? (const void*)sq->groups : (const void*)groups) && n > 0)) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->in_frame || !ctx->modular) return JXLH_ERR_BAD_STATE;
  const FrameDev& f = ctx->fd;
  if (f.subsampled) {
    ctx->last_error = "group-local transforms on a chroma-subsampled frame";
    return JXLH_ERR_UNSUPPORTED;
  }
  if (ctx->comm) {
    ctx->last_error = "group-local transforms on a sharded context";
    return JXLH_ERR_UNSUPPORTED;
  }
  const bool xyb = (sample_format & JXLH_MODULAR_XYB) != 0;
  const uint32_t depth = sample_format & ~(uint32_t)JXLH_MODULAR_XYB;
  if (!(xyb && depth == 0) && !bit_depth_ok(depth, 31)) return JXLH_ERR_INVALID_ARGUMENT;
  if (ctx->frame.mod_format && ctx->frame.mod_format != sample_format) return JXLH_ERR_INVALID_ARGUMENT;
  LocalDest d;
  for (int c = 0; c < 3; c++) d.out[c] = ctx->mod_src[c].p;
  d.n_out = 3;
  d.w = (uint32_t)f.xsize, d.h = (uint32_t)f.ysize;
  d.stride = f.plane_stride;
  d.frame = true;
  // the palettes' bit depth is the samples' (a palette on 32-bit float samples is refused: no bit depth of 1..31)
  if (jxlh_status st = local_enqueue(ctx, arena, arena_samples, groups, n, depth & 0xffu, d, first_bad, general, wp, sq)) return st;
  ctx->frame.mod_format = sample_format;
  if (wait) JXLH_SYNC(ctx);
  return JXLH_OK;
}

jxlh_status stage_transforms(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples, const jxlh_local_group* groups,
                             size_t n, uint32_t bit_depth, int32_t* const out[], uint32_t n_out, uint32_t out_w,
                             uint32_t out_h, size_t out_stride, size_t* first_bad, bool general, const jxlh_wp_header* wp,
                             const SqueezeIn* sq = nullptr) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !arena || (!(sq ? (const void*)sq->groups : (const void*)groups) && n > 0) || !out || n_out < 1 || n_out > JXLH_LOCAL_MAX_CHANNELS || out_stride < out_w)
    return JXLH_ERR_INVALID_ARGUMENT;
  LocalDest d;
  for (uint32_t c = 0; c < n_out; c++) {
    if (!out[c] || !is_device_ptr(out[c])) return JXLH_ERR_INVALID_ARGUMENT;
    d.out[c] = out[c];
  }
  if (ctx->comm) {
    ctx->last_error = "group-local transforms on a sharded context";
    return JXLH_ERR_UNSUPPORTED;
  }
  d.n_out = n_out;
  d.w = out_w, d.h = out_h;
  d.stride = out_stride;
  if (jxlh_status st = local_enqueue(ctx, arena, arena_samples, groups, n, bit_depth, d, first_bad, general, wp, sq)) return st;
  JXLH_SYNC(ctx);
  return JXLH_OK;
}

}  // namespace

}  // namespace jxlh_host

extern "C" {

jxlh_status jxlh_modular_local_lower(const jxlh_local_group* groups, size_t n, uint32_t bit_depth, uint64_t arena_samples,
                                     jxlh_local_program* programs, size_t* first_bad) {
  if (!groups && n > 0) return JXLH_ERR_INVALID_ARGUMENT;
  // two passes, so that a refused call leaves `programs` as it was
  for (int pass = 0; pass < (programs ? 2 : 1); pass++) {
    for (size_t g = 0; g < n; g++) {
      if (jxlh_status st = local_lower_group(groups[g], bit_depth, arena_samples, pass ? &programs[g] : nullptr, nullptr)) {
        if (first_bad) *first_bad = g;
        return st;
      }
    }
  }
  return JXLH_OK;
}

jxlh_status jxlh_modular_local_lower_general(const jxlh_local_group* groups, const jxlh_wp_header* wp, size_t n,
                                             uint32_t bit_depth, uint64_t arena_samples,
                                             jxlh_local_general_program* programs, size_t* first_bad) {
  if (!groups && n > 0) return JXLH_ERR_INVALID_ARGUMENT;
  for (int pass = 0; pass < (programs ? 2 : 1); pass++) {
    for (size_t g = 0; g < n; g++) {
      if (jxlh_status st = local_lower_core(groups[g], bit_depth, arena_samples, true, wp ? &wp[g] : nullptr, nullptr,
                                            pass ? &programs[g] : nullptr, nullptr)) {
        if (first_bad) *first_bad = g;
        return st;
      }
    }
  }
  return JXLH_OK;
}

jxlh_status jxlh_modular_local_transforms(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                          const jxlh_local_group* groups, size_t n, uint32_t bit_depth, int32_t* const out[],
                                          uint32_t n_out, uint32_t out_w, uint32_t out_h, size_t out_stride,
                                          size_t* first_bad) {
  return stage_transforms(ctx, arena, arena_samples, groups, n, bit_depth, out, n_out, out_w, out_h, out_stride, first_bad,
                          false, nullptr);
}

jxlh_status jxlh_modular_local_transforms_general(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                  const jxlh_local_group* groups, const jxlh_wp_header* wp, size_t n,
                                                  uint32_t bit_depth, int32_t* const out[], uint32_t n_out, uint32_t out_w,
                                                  uint32_t out_h, size_t out_stride, size_t* first_bad) {
  return stage_transforms(ctx, arena, arena_samples, groups, n, bit_depth, out, n_out, out_w, out_h, out_stride, first_bad,
                          true, wp);
}

jxlh_status jxlh_frame_set_modular_groups(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                          const jxlh_local_group* groups, size_t n, uint32_t sample_format,
                                          size_t* first_bad) {
  return frame_set_groups(ctx, arena, arena_samples, groups, n, sample_format, first_bad, true);
}

jxlh_status jxlh_frame_set_modular_groups_async(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                const jxlh_local_group* groups, size_t n, uint32_t sample_format,
                                                size_t* first_bad) {
  return frame_set_groups(ctx, arena, arena_samples, groups, n, sample_format, first_bad, false);
}

jxlh_status jxlh_frame_set_modular_groups_general(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                  const jxlh_local_group* groups, const jxlh_wp_header* wp, size_t n,
                                                  uint32_t sample_format, size_t* first_bad) {
  return frame_set_groups(ctx, arena, arena_samples, groups, n, sample_format, first_bad, true, true, wp);
}

jxlh_status jxlh_frame_set_modular_groups_general_async(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                        const jxlh_local_group* groups, const jxlh_wp_header* wp, size_t n,
                                                        uint32_t sample_format, size_t* first_bad) {
  return frame_set_groups(ctx, arena, arena_samples, groups, n, sample_format, first_bad, false, true, wp);
}

jxlh_status jxlh_modular_local_default_squeeze(const uint32_t* w, const uint32_t* h, uint32_t n, uint32_t n_meta,
                                               jxlh_squeeze_params* params, uint32_t cap, uint32_t* n_params) {
  if (!w || !h || !n_params || n < 1 || n > JXLH_LOCAL_MAX_CHANNELS || (!params && cap > 0)) return JXLH_ERR_INVALID_ARGUMENT;
  *n_params = jxlh::default_squeeze_list(w, h, n, n_meta, params, cap);
  return *n_params > cap ? JXLH_ERR_INVALID_ARGUMENT : JXLH_OK;
}

jxlh_status jxlh_modular_local_lower_squeeze(const jxlh_local_squeeze_group* groups, size_t n,
                                             const jxlh_local_coded_channel* coded, size_t n_coded,
                                             const jxlh_squeeze_params* params, size_t n_params, const jxlh_wp_header* wp,
                                             uint32_t bit_depth, uint64_t arena_samples,
                                             jxlh_local_squeeze_program* programs, size_t* first_bad) {
  if (!groups && n > 0) return JXLH_ERR_INVALID_ARGUMENT;
  // two passes, so that a refused call leaves `programs` as it was
  for (int pass = 0; pass < (programs ? 2 : 1); pass++) {
    for (size_t g = 0; g < n; g++) {
      if (jxlh_status st = jxlh::local_lower_squeeze_group(groups[g], coded, n_coded, params, n_params, wp ? &wp[g] : nullptr,
                                                           bit_depth, arena_samples, pass ? &programs[g] : nullptr, nullptr)) {
        if (first_bad) *first_bad = g;
        return st;
      }
    }
  }
  return JXLH_OK;
}

jxlh_status jxlh_modular_local_transforms_squeeze(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                  const jxlh_local_squeeze_group* groups, size_t n,
                                                  const jxlh_local_coded_channel* coded, size_t n_coded,
                                                  const jxlh_squeeze_params* params, size_t n_params,
                                                  const jxlh_wp_header* wp, uint32_t bit_depth, int32_t* const out[],
                                                  uint32_t n_out, uint32_t out_w, uint32_t out_h, size_t out_stride,
                                                  size_t* first_bad) {
  const jxlh_host::SqueezeIn sq{groups, coded, n_coded, params, n_params};
  return jxlh_host::stage_transforms(ctx, arena, arena_samples, nullptr, n, bit_depth, out, n_out, out_w, out_h, out_stride,
                                     first_bad, true, wp, &sq);
}

jxlh_status jxlh_frame_set_modular_groups_squeeze(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                  const jxlh_local_squeeze_group* groups, size_t n,
                                                  const jxlh_local_coded_channel* coded, size_t n_coded,
                                                  const jxlh_squeeze_params* params, size_t n_params,
                                                  const jxlh_wp_header* wp, uint32_t sample_format, size_t* first_bad) {
  const jxlh_host::SqueezeIn sq{groups, coded, n_coded, params, n_params};
  return jxlh_host::frame_set_groups(ctx, arena, arena_samples, nullptr, n, sample_format, first_bad, true, true, wp, &sq);
}

jxlh_status jxlh_frame_set_modular_groups_squeeze_async(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                        const jxlh_local_squeeze_group* groups, size_t n,
                                                        const jxlh_local_coded_channel* coded, size_t n_coded,
                                                        const jxlh_squeeze_params* params, size_t n_params,
                                                        const jxlh_wp_header* wp, uint32_t sample_format,
                                                        size_t* first_bad) {
  const jxlh_host::SqueezeIn sq{groups, coded, n_coded, params, n_params};
  return jxlh_host::frame_set_groups(ctx, arena, arena_samples, nullptr, n, sample_format, first_bad, false, true, wp, &sq);
}

}  // extern "C"
