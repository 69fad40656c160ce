// Group-local Modular transforms (jxl_hip.h, jxl_hip_local_palette.h, jxl_hip_local_squeeze.h), decided here and issued
// by abi_modular_local.hip: one call's batch of groups as ONE plan -- which route every group takes, the device
// descriptors and work lists (modular_local_desc.h), where every slot lives between phases, how many levels of a chain
// run in LDS and which scratch plane the others write, the scratch the batch needs, the byte layout of the one block
// that goes up, and the launches in their order.  Everything that can refuse the call is checked before the plan holds
// a single launch.  Plain C++: host logic, tested without a device (tests/cpp/modular_local_plan.cc).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "modular_local_desc.h"
#include "modular_local_host.h"
#include "modular_local_squeeze_host.h"
#include "squeeze_plan.h"

namespace jxlh {

// ---- a mixed destination (jxl_hip_local_extra.h): the frame's colour planes followed by extra channels' sample stores,
// or extra channels only.  The plan sees no pointer: a plane is named by what it is, and whoever issues the plan maps
// the names to addresses.
enum : uint32_t { kLocalPlaneColour = 0 /* + c, c in 0..2 */, kLocalPlaneExtra = 3 /* + the extra channel's index */ };
// what such a call meets: the frame and its extra channels
struct LocalDestState {
  bool in_frame = false, modular = false, subsampled = false, sharded = false;
  uint32_t w = 0, h = 0;       // a Modular frame's coded size ...
  uint32_t plane_stride = 0;   // ... and its sample planes' row stride
  uint32_t mod_format = 0;     // the sample_format of the frame's earlier group calls; 0: none yet
  struct Ec {
    bool set = false;
    uint32_t w = 0, h = 0;
  } ec[JXLH_MAX_EXTRA_CHANNELS];
};
// The destination as a table: per channel slot of a group, which plane it is and that plane's row stride.  A grey slot
// 0 (fan) keeps its two further planes, colour planes 1 and 2 of the frame's stride.
struct LocalDestTable {
  jxlh_status status = JXLH_OK;
  const char* why = nullptr;  // a refusal's rule (a literal)
  uint32_t n_slots = 0;
  struct Slot {
    uint32_t plane, stride;
  } slot[4] = {};
  bool fan = false;
  uint32_t w = 0, h = 0;      // the planes' size: rects are checked against it
  uint32_t bit_depth = 0;     // the palettes'
  uint32_t n_colour = 0, n_ec = 0;
  bool mixed() const { return n_colour > 0 && n_ec > 0; }  // planes of two kinds: strides may differ, the fan is apart
};
namespace local_plan_detail {
inline LocalDestTable dest_refused(jxlh_status st, const char* why) {
  LocalDestTable t;
  t.status = st, t.why = why;
  return t;
}
}  // namespace local_plan_detail
// The rules of jxl_hip_local_extra.h that do not depend on a group, in the header's order (checks 2 to 7).
inline LocalDestTable plan_local_dest(const jxlh_local_dest& d, uint32_t sample_format, const LocalDestState& s) {
  using local_plan_detail::dest_refused;
  const jxlh_status INV = JXLH_ERR_INVALID_ARGUMENT, BAD = JXLH_ERR_BAD_STATE, UNS = JXLH_ERR_UNSUPPORTED;
  if (d.n_colour != 0 && d.n_colour != 1 && d.n_colour != 3) return dest_refused(INV, "n_colour is 0, 1 or 3");
  if (d.n_ec > JXLH_LOCAL_MAX_CHANNELS || d.n_colour + d.n_ec < 1 || d.n_colour + d.n_ec > JXLH_LOCAL_MAX_CHANNELS)
    return dest_refused(INV, "n_colour + n_ec is 1..4");
  for (uint32_t k = 0; k < d.n_ec; k++) {
    if (d.ec[k] >= JXLH_MAX_EXTRA_CHANNELS) return dest_refused(INV, "an extra channel index out of range");
    for (uint32_t j = 0; j < k; j++)
      if (d.ec[j] == d.ec[k]) return dest_refused(INV, "an extra channel named twice");
  }
  if (d.n_colour > 0 && d.bit_depth != 0) return dest_refused(INV, "bit_depth with colour channels: the depth is sample_format's");
  if (d.bit_depth > 31) return dest_refused(INV, "a bit depth above 31");
  if (d.n_colour == 0 && sample_format != 0) return dest_refused(INV, "a sample_format without colour channels");
  const bool xyb = (sample_format & JXLH_MODULAR_XYB) != 0;
  const uint32_t depth = sample_format & ~(uint32_t)JXLH_MODULAR_XYB;
  if (d.n_colour > 0) {  // the rule of the other frame calls (bit_depth_ok(depth, 31), jxlh_internal.h)
    const uint32_t bits = depth & 0xffu, eb = depth >> 8;
    const bool ok = eb == 0 ? bits >= 1 && bits <= 31
                            : (depth >> 16) == 0 && bits <= 32 && eb >= 2 && eb <= 8 && bits >= eb + 2 && bits - eb - 1 <= 23;
    if (!(xyb && depth == 0) && !ok) return dest_refused(INV, "a sample_format that names no sample type");
  }
  if (!s.in_frame) return dest_refused(BAD, "outside a frame");
  if (d.n_colour > 0 && !s.modular) return dest_refused(BAD, "colour channels on a VarDCT frame");
  if (s.sharded) return dest_refused(UNS, "group-local transforms on a sharded context");
  if (d.n_colour > 0 && s.subsampled) return dest_refused(UNS, "group-local transforms on a chroma-subsampled frame");
  for (uint32_t k = 0; k < d.n_ec; k++)
    if (!s.ec[d.ec[k]].set) return dest_refused(BAD, "a named extra channel is not set");
  LocalDestTable t;
  t.n_colour = d.n_colour, t.n_ec = d.n_ec;
  t.w = d.n_colour > 0 ? s.w : s.ec[d.ec[0]].w;
  t.h = d.n_colour > 0 ? s.h : s.ec[d.ec[0]].h;
  for (uint32_t k = 0; k < d.n_ec; k++)
    if (s.ec[d.ec[k]].w != t.w || s.ec[d.ec[k]].h != t.h)
      return dest_refused(UNS, "a named extra channel of another size than the call's planes");
  if (d.n_colour > 0 && s.mod_format && s.mod_format != sample_format)
    return dest_refused(INV, "another sample_format than the frame's earlier groups");
  t.n_slots = d.n_colour + d.n_ec;
  for (uint32_t c = 0; c < d.n_colour; c++) t.slot[c] = {kLocalPlaneColour + c, s.plane_stride};
  for (uint32_t k = 0; k < d.n_ec; k++) t.slot[d.n_colour + k] = {kLocalPlaneExtra + d.ec[k], t.w};  // a store's rows are w apart
  t.fan = d.n_colour == 1;
  // the palettes' bit depth is the samples' (a palette on 32-bit float samples is refused: no bit depth of 1..31)
  t.bit_depth = d.n_colour > 0 ? (depth & 0xffu) : d.bit_depth;
  return t;
}

// ---- what a call brings: "group gi of this call" in one form.  The plain and _general calls bring `groups`; the
// _squeeze calls bring `sgroups` and the call-wide tables `coded` / `params`.  No sample pointer: what the vector path
// needs of them is plan_local_batch's `aligned`.
struct LocalBatchIn {
  enum Form { kPlain, kGeneral, kSqueeze } form = kPlain;
  const jxlh_local_group* groups = nullptr;
  const jxlh_local_squeeze_group* sgroups = nullptr;
  const jxlh_local_coded_channel* coded = nullptr;
  size_t n_coded = 0;
  const jxlh_squeeze_params* params = nullptr;
  size_t n_params = 0;
  size_t n = 0;                      // groups
  const jxlh_wp_header* wp = nullptr;  // one header per group, or null
  uint32_t bit_depth = 0;
  uint64_t arena_samples = 0;
  // the destination: n_out planes of w x h; frame: the frame's sample planes, 3 or 1 (fanned out) channels per group
  uint32_t n_out = 0, w = 0, h = 0;
  bool frame = false;
  // ... or a table (jxl_hip_local_extra.h): slot c of every group is dest->slot[c]; n_out, w, h and frame are unused.
  // plane_aligned[c]: slot c's plane starts 16-byte aligned, fan_aligned: so do the two planes a grey slot 0 fans out to
  const LocalDestTable* dest = nullptr;
  bool plane_aligned[4] = {false, false, false, false}, fan_aligned = false;
  bool has_groups() const { return form == kSqueeze ? sgroups != nullptr : groups != nullptr; }
};

// what the phases of the groups with general palettes launch: phase p's descriptors (LpPhaseDev for even p, LpJobDev for
// odd p) and work items
struct GeneralBatch {
  std::vector<LpPhaseDev> pointwise[kLpMaxPhases];
  std::vector<LpJobDev> jobs[kLpMaxPhases];
  std::vector<LocalItem> items[kLpMaxPhases];
  bool weighted[kLpMaxPhases] = {}, lds_palette[kLpMaxPhases] = {};
  uint64_t scratch = 0;  // samples: the index copies, the weighted predictor's row state and the chains' planes
};
// what the squeeze chains of a batch launch: the LDS launch's items (chain, 0) and streamed launch k's (chain, first line)
struct SqueezeBatch {
  std::vector<LsChainDev> chains;
  std::vector<LocalItem> lds_items;
  std::vector<LocalItem> level_items[kLsLevels];
};

// One group with general palettes, cut into phases (jxl_hip_local_palette.h).  Between phases a slot is in the arena
// (a coded channel nothing has touched yet), in the destination rect, or -- the index channel of the next general
// palette, which shares its slot with that palette's output channel 0 while the other channels' workgroups still read
// it -- in scratch.  A point-wise phase loads every slot that is somewhere and stores what it changed (what the next
// palette overwrites excepted); the last one leaves every channel in the destination rect.
// init (a group of the squeeze calls): where each slot is when the phases start -- a coded channel of its own stride, or
// the destination rect, where the slot's squeeze chain ends.  Such a group may have no general palette at all: its one
// point-wise phase is phase 0.
inline void plan_general_group(const jxlh_local_group& g, const jxlh_local_general_program& prog, const jxlh_wp_header* wp,
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

// One group of the squeeze calls that does not run as a plain / general group: every squeezed channel becomes a chain
// that ends in the destination rect, every other one stays in the arena; the steps in front follow as phases.
inline void plan_squeeze_group(const jxlh_local_group& g, const jxlh_local_squeeze_group& sg,
                               const jxlh_local_squeeze_program& prog, const jxlh_local_coded_channel* coded,
                               const jxlh_wp_header* wp, bool fan, GeneralBatch& gb, SqueezeBatch& sb) {
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
    while (n_lds >= 1 && !squeeze_levels_fit((int)n_lds, fit, ch.base_w, ch.base_h)) n_lds--;
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

// ---- the route of one lowered group
enum class LocalRoute {
  kPlain,   // one work list entry per row chunk in the batch's single launch of k_modular_local
  kPhases,  // general palettes: phase by phase, behind that launch
  kChains,  // squeeze chains into the destination rect first, then the phases on it
};
// The rule.  A group of the squeeze calls (sg, sprog non-null) without any squeeze level whose coded channels share a
// stride is exactly a group of the _general calls and runs as one; any other group of those calls runs as chains (a
// zero-area group has no rows for strides to differ on).  Among the groups of the plain and _general calls, and those,
// the phased route is taken when the lowering found a general palette (n_phases > 1); the rest is plain.
inline LocalRoute local_route(const jxlh_local_squeeze_group* sg, const jxlh_local_squeeze_program* sprog,
                              const jxlh_local_coded_channel* coded, uint32_t n_phases) {
  if (sg) {
    for (uint32_t k = 0; k < sprog->general.n_coded; k++)
      if (sprog->chains[k].n_levels > 0) return LocalRoute::kChains;
    for (uint32_t k = 1; k < sprog->n_coded && sg->w > 0 && sg->h > 0; k++)
      if (coded[sg->coded_first + k].stride != coded[sg->coded_first].stride) return LocalRoute::kChains;
  }
  return n_phases > 1 ? LocalRoute::kPhases : LocalRoute::kPlain;
}

// A group of the squeeze calls in the terms of the plain / _general calls: its rect, channels and steps, and -- with_coded,
// off the chain route -- its coded channels, which are then the channels that reach the (absent) squeeze, full size.  An
// empty group's channels are not looked at.
inline jxlh_local_group squeeze_group_as_general(const jxlh_local_squeeze_group& sg, const jxlh_local_squeeze_program& sprog,
                                                 const jxlh_local_coded_channel* coded, bool with_coded) {
  jxlh_local_group g{};
  g.x0 = sg.x0, g.y0 = sg.y0, g.w = sg.w, g.h = sg.h;
  g.n_channels = sg.n_channels, g.n_steps = sg.n_steps;
  for (uint32_t k = 0; k < sg.n_steps; k++) g.steps[k] = sg.steps[k];
  if (with_coded) {
    const bool read = sprog.n_coded > 0 && sg.w > 0 && sg.h > 0;
    g.n_coded = sprog.n_coded;
    g.coded_stride = read ? coded[sg.coded_first].stride : sg.w;
    for (uint32_t k = 0; read && k < sprog.n_coded; k++) g.coded_offset[k] = coded[sg.coded_first + k].offset;
  }
  return g;
}

// no launch takes more than 2^31 - 1 work items (nor a descriptor index beyond that)
inline bool local_item_count_ok(uint64_t count) { return count <= 0x7fffffffu; }

// ---- the plan
struct LocalSection {
  size_t off = 0, bytes = 0;  // in the upload block; off is 16-byte aligned, bytes is what the section holds
};
// The upload block, in this order: the plain route's group descriptors (one per group of the call, zero for the groups
// of the other routes) and items, then per phase its descriptors and items, then the chains, the LDS launch's items and
// streamed launch k's.  Every section starts 16-byte aligned; an empty one takes no room.
struct LocalLayout {
  LocalSection groups, items;
  LocalSection phase_desc[kLpMaxPhases], phase_items[kLpMaxPhases];
  LocalSection chains, lds_items, level_items[kLsLevels];
  size_t total = 0;
};
enum class LocalKernel { kLocal, kSqueezeLds, kSqueezeLevel, kPalette, kPhase };
struct LocalStep {
  LocalKernel kernel;
  LocalSection desc, items;
  uint32_t n_items;
  uint32_t step;                   // kSqueezeLevel: the streamed launch's index
  uint32_t weighted, lds_palette;  // kPalette
  uint32_t fan_grey;               // kLocal: the destination is a frame
};
// the launch list: at most one plain launch, one LDS launch, kLsLevels streamed ones and kLpMaxPhases phases; held in
// place, so that laying out a plan allocates nothing behind the batch's large lists
struct LocalSteps {
  LocalStep at[2 + kLsLevels + kLpMaxPhases];
  uint32_t n = 0;
  LocalStep& push_back(const LocalStep& s) { return at[n++] = s; }
  const LocalStep* begin() const { return at; }
  const LocalStep* end() const { return at + n; }
  const LocalStep& operator[](size_t i) const { return at[i]; }
  size_t size() const { return n; }
  bool empty() const { return n == 0; }
};

struct LocalPlan {
  // a refusal: `why` names the rule (a literal) and first_bad the group; why == nullptr: the call as a whole
  jxlh_status status = JXLH_OK;
  size_t first_bad = 0;
  const char* why = nullptr;
  std::vector<LocalGroupDev> groups;
  std::vector<LocalItem> items;
  GeneralBatch general;
  SqueezeBatch squeeze;
  uint64_t scratch = 0;  // samples
  LocalLayout layout;
  // the plain launch, the LDS launch, the streamed levels ascending, the phases ascending; empty ones are absent
  LocalSteps steps;

  // the longest list a launch indexes
  uint64_t most_items() const {
    uint64_t most = std::max({items.size(), squeeze.chains.size(), squeeze.lds_items.size()});
    for (const auto& v : squeeze.level_items) most = std::max<uint64_t>(most, v.size());
    for (const auto& v : general.items) most = std::max<uint64_t>(most, v.size());
    return most;
  }
  // The block's bytes: the single place the layout becomes memory.  Writes layout.total bytes, padding zeroed.
  void serialize(uint8_t* dst) const {
    size_t at = 0;
    auto put = [&](const LocalSection& s, const void* src) {
      std::memset(dst + at, 0, s.off - at);
      if (s.bytes) std::memcpy(dst + s.off, src, s.bytes);
      at = s.off + s.bytes;
    };
    put(layout.groups, groups.data());
    put(layout.items, items.data());
    for (uint32_t p = 0; p < kLpMaxPhases; p++) {
      if (p & 1) put(layout.phase_desc[p], general.jobs[p].data());
      else put(layout.phase_desc[p], general.pointwise[p].data());
      put(layout.phase_items[p], general.items[p].data());
    }
    put(layout.chains, squeeze.chains.data());
    put(layout.lds_items, squeeze.lds_items.data());
    for (int k = 0; k < kLsLevels; k++) put(layout.level_items[k], squeeze.level_items[k].data());
    std::memset(dst + at, 0, layout.total - at);
  }
};

namespace local_plan_detail {

inline LocalPlan refused(jxlh_status st, size_t g, const char* why) {
  LocalPlan p;
  p.status = st, p.first_bad = g, p.why = why;
  return p;
}

// a group of the plain route: its descriptor, and (unless it is empty) its items
inline void plan_plain_group(const jxlh_local_group& g, const jxlh_local_program& prog, bool aligned, size_t gi, LocalPlan& plan) {
  LocalGroupDev& o = plan.groups[gi];
  o.x0 = g.x0, o.y0 = g.y0, o.w = g.w, o.h = g.h;
  o.n_channels = g.n_channels;
  o.n_ops = prog.n_ops;
  o.coded_stride = g.coded_stride;
  bool vec = aligned && (g.coded_stride & 3) == 0 && (g.x0 & 3) == 0;
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
  if (g.w == 0 || g.h == 0) return;
  // threads along x: the smallest power of two that covers the row's 4-sample vectors, at most the workgroup
  const uint32_t nvx = (g.w + 3) / 4;
  uint32_t lx = 0;
  while (lx < 8 && (1u << lx) < nvx) lx++;
  o.lanes_x_log2 = lx;
  o.rows_per_item = std::max(256u >> lx, kLocalItemSamples / (4 * nvx));
  for (uint64_t r = 0; r < g.h; r += o.rows_per_item) plan.items.push_back(LocalItem{(uint32_t)gi, (uint32_t)r});
}

// the sections in the documented order, and the launches that read them
inline void lay_out(const LocalBatchIn& in, LocalPlan& plan) {
  LocalLayout& L = plan.layout;
  size_t at = 0;
  auto section = [&](size_t count, size_t size) {
    LocalSection s{at, count * size};
    at += (s.bytes + 15) / 16 * 16;
    return s;
  };
  auto step = [&](LocalKernel k, const LocalSection& desc, const LocalSection& items, size_t n_items) {
    LocalStep s{};
    s.kernel = k, s.desc = desc, s.items = items, s.n_items = (uint32_t)n_items;
    return &plan.steps.push_back(s);
  };
  const GeneralBatch& gb = plan.general;
  const SqueezeBatch& sb = plan.squeeze;
  L.groups = section(plan.groups.size(), sizeof(LocalGroupDev));
  L.items = section(plan.items.size(), sizeof(LocalItem));
  for (uint32_t p = 0; p < kLpMaxPhases; p++) {
    L.phase_desc[p] = (p & 1) ? section(gb.jobs[p].size(), sizeof(LpJobDev)) : section(gb.pointwise[p].size(), sizeof(LpPhaseDev));
    L.phase_items[p] = section(gb.items[p].size(), sizeof(LocalItem));
  }
  L.chains = section(sb.chains.size(), sizeof(LsChainDev));
  L.lds_items = section(sb.lds_items.size(), sizeof(LocalItem));
  for (int k = 0; k < kLsLevels; k++) L.level_items[k] = section(sb.level_items[k].size(), sizeof(LocalItem));
  L.total = at;
  if (!plan.items.empty())
    step(LocalKernel::kLocal, L.groups, L.items, plan.items.size())->fan_grey = in.dest ? (in.dest->fan ? 1 : 0) : in.frame ? 1 : 0;
  // every chain up to its destination rect, ahead of the phases that read it there
  if (!sb.lds_items.empty()) step(LocalKernel::kSqueezeLds, L.chains, L.lds_items, sb.lds_items.size());
  for (int k = 0; k < kLsLevels; k++)
    if (!sb.level_items[k].empty()) step(LocalKernel::kSqueezeLevel, L.chains, L.level_items[k], sb.level_items[k].size())->step = (uint32_t)k;
  for (uint32_t p = 0; p < kLpMaxPhases; p++) {
    if (gb.items[p].empty()) continue;
    LocalStep* s = step((p & 1) ? LocalKernel::kPalette : LocalKernel::kPhase, L.phase_desc[p], L.phase_items[p], gb.items[p].size());
    if (p & 1) s->weighted = gb.weighted[p], s->lds_palette = gb.lds_palette[p];
  }
}

}  // namespace local_plan_detail

// The batch.  aligned: the destination's stride is a multiple of 4 samples and the arena and every destination plane
// start 16-byte aligned (the caller's pointers: the plan sees none).  A refused plan (status != JXLH_OK) holds nothing to
// launch; so does an accepted one whose groups are all empty (steps.empty()).
// Per group, in this order: the lowering's refusals; the channel count against the destination; the rect against the
// planes; the width cap of predicted palettes; the item cap.
// A table destination (in.dest, accepted by plan_local_dest): `aligned` speaks of the arena alone, and alignment is a
// per-plane fact -- a plane allows the 16-byte path when it starts 16-byte aligned and its stride is a multiple of 4
// samples; a group takes that path when every plane it writes allows it (a group writes all of the table's planes).
inline LocalPlan plan_local_batch(const LocalBatchIn& in, bool aligned) {
  using namespace local_plan_detail;
  const uint32_t dest_w = in.dest ? in.dest->w : in.w, dest_h = in.dest ? in.dest->h : in.h;
  if (in.n > 0x7fffffffu || dest_w > 0x7fffffffu || dest_h > 0x7fffffffu) return refused(JXLH_ERR_INVALID_ARGUMENT, 0, nullptr);
  if (in.dest) {
    for (uint32_t c = 0; c < in.dest->n_slots; c++) aligned = aligned && in.plane_aligned[c] && (in.dest->slot[c].stride & 3) == 0;
    if (in.dest->fan) aligned = aligned && in.fan_aligned;
  }
  LocalPlan plan;
  plan.groups.assign(in.n, LocalGroupDev{});
  for (size_t gi = 0; gi < in.n; gi++) {
    const jxlh_wp_header* wp = in.wp ? &in.wp[gi] : nullptr;
    const char* why = "";
    jxlh_local_program prog;
    jxlh_local_general_program gprog;
    jxlh_local_squeeze_program sprog;
    const jxlh_local_squeeze_group* sg = in.form == LocalBatchIn::kSqueeze ? &in.sgroups[gi] : nullptr;
    // the lowering of the call's own form, then the route, decided once
    if (sg) {
      if (jxlh_status st = local_lower_squeeze_group(*sg, in.coded, in.n_coded, in.params, in.n_params, wp, in.bit_depth,
                                                     in.arena_samples, &sprog, &why))
        return refused(st, gi, why);
      gprog = sprog.general;
    } else if (jxlh_status st = local_lower_core(in.groups[gi], in.bit_depth, in.arena_samples, in.form != LocalBatchIn::kPlain,
                                                 wp, &prog, &gprog, &why)) {
      return refused(st, gi, why);
    }
    const LocalRoute route = local_route(sg, &sprog, in.coded, gprog.n_phases);
    jxlh_local_group as_general;
    if (sg) {
      as_general = squeeze_group_as_general(*sg, sprog, in.coded, route != LocalRoute::kChains);
      if (route != LocalRoute::kChains)  // ... which the _general lowering checks and lowers as its own
        if (jxlh_status st = local_lower_core(as_general, in.bit_depth, in.arena_samples, true, wp, &prog, &gprog, &why))
          return refused(st, gi, why);
    }
    const jxlh_local_group& g = sg ? as_general : in.groups[gi];
    if (in.dest) {
      if (g.n_channels != in.dest->n_slots)
        return refused(JXLH_ERR_INVALID_ARGUMENT, gi, "the group's channels are not the destination's n_colour + n_ec");
    } else if (in.frame ? (g.n_channels != 3 && g.n_channels != 1) : g.n_channels > in.n_out) {
      return refused(JXLH_ERR_INVALID_ARGUMENT, gi, in.frame ? "a frame's groups hold 3 channels, or 1 (grey)" : "more channels than out planes");
    }
    if ((uint64_t)g.x0 + g.w > dest_w || (uint64_t)g.y0 + g.h > dest_h)
      return refused(JXLH_ERR_INVALID_ARGUMENT, gi, "the rect leaves the planes");
    if (route == LocalRoute::kPhases && g.w > (1u << 30))
      return refused(JXLH_ERR_INVALID_ARGUMENT, gi, "a predicted palette on a group wider than 2^30");
    const bool fan = in.dest ? in.dest->fan : in.frame && g.n_channels == 1, empty = g.w == 0 || g.h == 0;
    // an empty group is checked, never planned (the plain route still writes its descriptor: no item names it)
    if (route == LocalRoute::kPlain) plan_plain_group(g, prog, aligned, gi, plan);
    else if (empty) continue;
    else if (route == LocalRoute::kPhases) plan_general_group(g, gprog, wp, fan, plan.general);
    else plan_squeeze_group(g, *sg, sprog, in.coded, wp, fan, plan.general, plan.squeeze);
    // (the plain route grows one list only: 1024 such groups should not walk the other 26 each)
    if (!local_item_count_ok(route == LocalRoute::kPlain ? plan.items.size() : plan.most_items()))
      return refused(JXLH_ERR_INVALID_ARGUMENT, gi, "the batch holds more than 2^31 - 1 work items");
  }
  plan.scratch = plan.general.scratch;
  lay_out(in, plan);
  return plan;
}

}  // namespace jxlh
