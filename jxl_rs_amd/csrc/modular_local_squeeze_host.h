// Group-local squeeze, host side: default_squeeze (squeeze.rs:39-105) and the squeeze branch of
// meta_apply_single_transform (meta_apply.rs:90-180) on one group's channel list, behind the general lowering of the
// steps in front of it (modular_local_host.h).  Plain C++ (no device, no context, no heap):
// jxlh_modular_local_lower_squeeze, the library's own launches and the stand-alone checks all go through
// local_lower_squeeze_group.
//
// The reference gives every squeezed channel two fresh buffers -- the averages, which take the channel's place in the
// list, and the residuals, which go behind the range (in place) or to the end -- and records one H/VSqueeze step whose
// output is the buffer the channel had.  The averages of one step are the output of the next step on that channel, so
// the steps of one image channel form a CHAIN from the last averages (the base) up to the channel itself; local_apply
// runs the steps last to first, which is each chain from its base upwards.  Chains never meet: a group's squeezes are
// closed inside the group (apply_local.rs:295-348).
#pragma once
#include "modular_local_host.h"
#include "../../include/jxl_hip_local_squeeze.h"

namespace jxlh {

constexpr uint32_t kLsMaxDim = 1u << 20;  // the kernels take `int` line counts / lengths
// default_squeeze never returns more: 2 preview steps and at most 32 halvings per axis
constexpr uint32_t kLsMaxDefaultParams = 2 + 2 * 32;

// default_squeeze for n_meta meta channels and nc image channels of cw[i] x ch[i]; -> the list's length, entries beyond
// cap are counted and not written
inline uint32_t default_squeeze_list(const uint32_t* cw, const uint32_t* ch, uint32_t nc, uint32_t n_meta,
                                     jxlh_squeeze_params* out, uint32_t cap) {
  uint32_t n = 0;
  auto push = [&](uint32_t horizontal, uint32_t in_place, uint32_t begin_c, uint32_t num_c) {
    if (out && n < cap) out[n] = jxlh_squeeze_params{horizontal, in_place, begin_c, num_c};
    n++;
  };
  uint32_t w = cw[0], h = ch[0];
  if (nc > 2 && cw[1] == w && ch[1] == h) {  // 420 previews, squeeze.rs:51-68
    if (w > 1) push(1, 0, n_meta + 1, 2);
    if (h > 1) push(0, 0, n_meta + 1, 2);
  }
  constexpr uint32_t kMaxFirstPreviewSize = 8;
  if (w <= h && h > kMaxFirstPreviewSize) {  // vertical first on tall images
    push(0, 1, n_meta, nc);
    h = (h + 1) / 2;
  }
  while (w > kMaxFirstPreviewSize || h > kMaxFirstPreviewSize) {
    if (w > kMaxFirstPreviewSize) {
      push(1, 1, n_meta, nc);
      w = (w + 1) / 2;
    }
    if (h > kMaxFirstPreviewSize) {
      push(0, 1, n_meta, nc);
      h = (h + 1) / 2;
    }
  }
  return n;
}

// One group.  coded / params: the call-wide arrays.  *why names the rule that refused it (a literal).  prog may be null.
inline jxlh_status local_lower_squeeze_group(const jxlh_local_squeeze_group& g, const jxlh_local_coded_channel* coded,
                                             uint64_t n_coded_all, const jxlh_squeeze_params* params, uint64_t n_params_all,
                                             const jxlh_wp_header* wp, uint32_t bit_depth, uint64_t arena_samples,
                                             jxlh_local_squeeze_program* prog, const char** why) {
  const char* dummy;
  if (!why) why = &dummy;
  auto refuse = [&](jxlh_status st, const char* w) {
    *why = w;
    return st;
  };
  // the steps in front: the general lowering, which leaves the coded channels to this function
  jxlh_local_group lg{};
  lg.x0 = g.x0, lg.y0 = g.y0, lg.w = g.w, lg.h = g.h;
  lg.n_channels = g.n_channels;
  lg.n_steps = g.n_steps;
  for (uint32_t i = 0; i < g.n_steps && i < JXLH_LOCAL_MAX_STEPS; i++) lg.steps[i] = g.steps[i];
  jxlh_local_general_program gp;
  if (jxlh_status st = local_lower_core(lg, bit_depth, arena_samples, true, wp, nullptr, &gp, why, false)) return st;
  if (g.has_squeeze > 1) return refuse(JXLH_ERR_INVALID_ARGUMENT, "has_squeeze above 1");
  if (!g.has_squeeze && g.n_params != 0) return refuse(JXLH_ERR_INVALID_ARGUMENT, "squeeze parameters without a squeeze");
  if (g.has_squeeze && g.squeeze_pos > g.n_steps) return refuse(JXLH_ERR_INVALID_ARGUMENT, "squeeze_pos above n_steps");
  if (g.has_squeeze && g.squeeze_pos < g.n_steps) return refuse(JXLH_ERR_UNSUPPORTED, "a transform behind a local squeeze");
  if ((uint64_t)g.params_first + g.n_params > n_params_all || (g.n_params > 0 && !params))
    return refuse(JXLH_ERR_INVALID_ARGUMENT, "the squeeze parameter range leaves the array");
  if ((uint64_t)g.coded_first + g.n_coded > n_coded_all || (g.n_coded > 0 && !coded))
    return refuse(JXLH_ERR_INVALID_ARGUMENT, "the coded channel range leaves the array");
  if (g.has_squeeze && (g.w > kLsMaxDim || g.h > kLsMaxDim)) return refuse(JXLH_ERR_UNSUPPORTED, "a local squeeze on a group beyond 2^20 on a side");

  // the channel list: meta channels, the running averages of the chains, residuals
  enum : int { kMeta = -1, kResidual = -2 };
  struct Entry {
    int chain;            // >= 0: the head of that chain; kMeta; kResidual
    uint32_t of, level;   // kResidual: of chain `of`, recorded as its level `level` (forward order)
    uint32_t w, h;
  };
  constexpr uint32_t kMaxList = JXLH_LOCAL_MAX_STEPS + JXLH_LOCAL_SQUEEZE_MAX_CODED;
  Entry list[kMaxList];
  uint32_t len = 0, n_meta = 0;
  for (uint32_t i = 0; i < g.n_steps; i++) n_meta += g.steps[i].kind == JXLH_LOCAL_PALETTE;
  for (uint32_t i = 0; i < n_meta; i++) list[len++] = Entry{kMeta, 0, 0, 0, 0};
  for (uint32_t k = 0; k < gp.n_coded; k++) list[len++] = Entry{(int)k, 0, 0, g.w, g.h};
  jxlh_local_squeeze_level fwd[JXLH_LOCAL_MAX_CHANNELS][JXLH_LOCAL_SQUEEZE_MAX_LEVELS] = {};
  uint32_t n_levels[JXLH_LOCAL_MAX_CHANNELS] = {};
  if (g.has_squeeze) {
    jxlh_squeeze_params dflt[kLsMaxDefaultParams];
    const jxlh_squeeze_params* sp = params + g.params_first;
    uint64_t n_sp = g.n_params;
    if (n_sp == 0) {  // default_squeeze(channels), meta_apply.rs:91-92
      uint32_t cw[JXLH_LOCAL_MAX_CHANNELS], ch[JXLH_LOCAL_MAX_CHANNELS];
      for (uint32_t k = 0; k < gp.n_coded; k++) cw[k] = g.w, ch[k] = g.h;
      n_sp = default_squeeze_list(cw, ch, gp.n_coded, n_meta, dflt, kLsMaxDefaultParams);
      sp = dflt;
    }
    for (uint64_t i = 0; i < n_sp; i++) {
      const jxlh_squeeze_params& p = sp[i];
      // check_squeeze_params, squeeze.rs:17-37
      const uint64_t end = (uint64_t)p.begin_c + p.num_c;
      if (end > len) return refuse(JXLH_ERR_INVALID_ARGUMENT, "squeeze channel range leaves the channel list");
      if (p.num_c == 0) return refuse(JXLH_ERR_INVALID_ARGUMENT, "squeeze of no channel");
      for (uint64_t c = p.begin_c; c < end; c++) {
        if (list[c].chain == kMeta) return refuse(JXLH_ERR_UNSUPPORTED, "squeeze of a palette meta channel");
        if (list[c].chain == kResidual) return refuse(JXLH_ERR_UNSUPPORTED, "squeeze of a residual channel");
      }
      const uint32_t new_chan_offset = p.in_place ? (uint32_t)end : len;
      for (uint32_t ic = 0; ic < p.num_c; ic++) {
        Entry& e = list[p.begin_c + ic];
        const uint32_t k = (uint32_t)e.chain;
        if (n_levels[k] == JXLH_LOCAL_SQUEEZE_MAX_LEVELS) return refuse(JXLH_ERR_UNSUPPORTED, "more than 16 squeeze levels on a channel");
        const uint32_t w = e.w, h = e.h;
        fwd[k][n_levels[k]] = jxlh_local_squeeze_level{p.horizontal ? 1u : 0u, w, h, 0};
        Entry res{kResidual, k, n_levels[k], w, h};
        n_levels[k]++;
        if (p.horizontal) e.w = (w + 1) / 2, res.w = w - e.w;
        else e.h = (h + 1) / 2, res.h = h - e.h;
        // channels.insert(new_chan_offset + ic, residual), meta_apply.rs:176 (len < kMaxList: every insertion is a level)
        const uint32_t at = new_chan_offset + ic;
        for (uint32_t q = len; q > at; q--) list[q] = list[q - 1];
        list[at] = res;
        len++;
      }
    }
  }
  // what is left of the list is what the group's section decoded
  const uint32_t want = len - n_meta;
  if (g.n_coded < want) return refuse(JXLH_ERR_UNSUPPORTED, "a coded channel is missing (previews of local squeezes stay on the host)");
  if (g.n_coded > want) return refuse(JXLH_ERR_INVALID_ARGUMENT, "n_coded above what the transforms leave");
  uint32_t base[JXLH_LOCAL_MAX_CHANNELS] = {}, base_w[JXLH_LOCAL_MAX_CHANNELS] = {}, base_h[JXLH_LOCAL_MAX_CHANNELS] = {};
  for (uint32_t j = 0; j < want; j++) {
    const Entry& e = list[n_meta + j];
    if (e.chain == kMeta) return refuse(JXLH_ERR_UNSUPPORTED, "squeeze of a palette meta channel");  // (not reached)
    const jxlh_local_coded_channel& c = coded[g.coded_first + j];
    if (c.w != e.w || c.h != e.h) return refuse(JXLH_ERR_INVALID_ARGUMENT, "a coded channel's size is not what the transforms leave");
    if (e.w > 0 && e.h > 0) {
      if (c.stride < c.w) return refuse(JXLH_ERR_INVALID_ARGUMENT, "coded stride below w");
      if (!local_fits(c.offset, (uint64_t)(e.h - 1) * c.stride + e.w, arena_samples))
        return refuse(JXLH_ERR_INVALID_ARGUMENT, "coded channel beyond the arena");
    }
    if (e.chain >= 0) base[e.chain] = j, base_w[e.chain] = e.w, base_h[e.chain] = e.h;
    else fwd[e.of][e.level].res = j;
  }
  if (prog) {
    *prog = jxlh_local_squeeze_program{};
    prog->general = gp;
    prog->n_coded = want;
    for (uint32_t k = 0; k < gp.n_coded; k++) {
      jxlh_local_squeeze_chain& c = prog->chains[k];
      c.base = base[k], c.base_w = base_w[k], c.base_h = base_h[k];
      c.n_levels = n_levels[k];
      for (uint32_t i = 0; i < n_levels[k]; i++) c.levels[i] = fwd[k][n_levels[k] - 1 - i];  // local_apply: last step first
    }
  }
  return JXLH_OK;
}

}  // namespace jxlh
