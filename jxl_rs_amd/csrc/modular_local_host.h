// Group-local Modular transforms, host side: the lowering of one group's transform list (GroupHeader::transforms) onto
// the channel slots the kernel keeps in registers.  Plain C++ (no device, no context): jxlh_modular_local_lower, the
// library's own launches and the stand-alone checks all go through local_lower_group.
//
// The reference keeps a list of (buffer id, ChannelInfo) and lets every transform rewrite it
// (meta_apply_single_transform, modular/transforms/meta_apply.rs:49-230); the steps it records run last-to-first
// (TransformStep::local_apply, apply_local.rs:233-355).  Here a buffer is a SLOT 0..3: slot s is where image channel s
// ends up.  An RCT renames its three channels' buffers (meta_apply.rs:63-81) and its inverse writes the old ones back
// (apply_local.rs:247-258): on slots it works in place.  A palette keeps the first channel's position for the index
// channel, drops the others and puts the meta channel in front (meta_apply.rs:226-228): its inverse reads the index
// from the first slot and writes every slot of the range.  The list only ever shrinks, so no slot is taken twice.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/jxl_hip.h"
#include "../../include/jxl_hip_local_palette.h"

#if defined(__HIPCC__)
#define JXLH_HOST_DEVICE __host__ __device__
#else
#define JXLH_HOST_DEVICE
#endif

namespace jxlh {

// perm: which output plane receives w0/w1/w2 (rct.rs:132-156)
template <class T>
JXLH_HOST_DEVICE inline void rct_permute(int perm, T p0, T p1, T p2, T (&o)[3]) {
  switch (perm) {
    default:
    case 0: o[0] = p0; o[1] = p1; o[2] = p2; break;
    case 1: o[0] = p1; o[1] = p2; o[2] = p0; break;  // Gbr: out[1,2,0] = in[0,1,2]
    case 2: o[0] = p2; o[1] = p0; o[2] = p1; break;  // Brg
    case 3: o[0] = p0; o[1] = p2; o[2] = p1; break;  // Rbg
    case 4: o[0] = p1; o[1] = p0; o[2] = p2; break;  // Grb
    case 5: o[0] = p2; o[1] = p1; o[2] = p0; break;  // Bgr
  }
}

// offset + extent inside the arena, without wrapping
inline bool local_fits(uint64_t offset, uint64_t extent, uint64_t arena_samples) {
  return offset <= arena_samples && extent <= arena_samples - offset;
}

// Bits(5) / Bits(4) fields of a weighted-predictor header (the rule of jxlh_palette_delta_wp)
inline bool wp_header_ok(const jxlh_wp_header& h) {
  const uint32_t f[11] = {h.p1c, h.p2c, h.p3ca, h.p3cb, h.p3cc, h.p3cd, h.p3ce, h.w0, h.w1, h.w2, h.w3};
  for (int i = 0; i < 11; i++)
    if (f[i] >= (i < 7 ? 32u : 16u)) return false;
  return true;
}

// One group.  *why names the rule that refused it (a literal).  `prog` / `gprog` may be null (checks only).
// general == false: the lowering of jxlh_modular_local_lower, which refuses delta / predicted palettes.
// general == true: the lowering of jxlh_modular_local_lower_general (jxl_hip_local_palette.h); `wp` is the group's own
// header, or null.  gprog receives what prog cannot say: per op num_deltas, predictor and the phase.
// check_coded == false (a squeeze stands behind the steps, modular_local_squeeze_host.h): what is left of the list is not
// what the group brings, so n_coded, coded_offset and coded_stride are not read.
inline jxlh_status local_lower_core(const jxlh_local_group& g, uint32_t bit_depth, uint64_t arena_samples, bool general,
                                    const jxlh_wp_header* wp, jxlh_local_program* prog,
                                    jxlh_local_general_program* gprog, const char** why, bool check_coded = true) {
  const char* dummy;
  if (!why) why = &dummy;
  auto refuse = [&](jxlh_status st, const char* w) {
    *why = w;
    return st;
  };
  if (g.n_channels < 1 || g.n_channels > JXLH_LOCAL_MAX_CHANNELS) return refuse(JXLH_ERR_INVALID_ARGUMENT, "n_channels outside 1..4");
  if (g.n_steps > JXLH_LOCAL_MAX_STEPS) return refuse(JXLH_ERR_INVALID_ARGUMENT, "n_steps above 4");
  if (check_coded && (g.n_coded < 1 || g.n_coded > JXLH_LOCAL_MAX_CHANNELS)) return refuse(JXLH_ERR_INVALID_ARGUMENT, "n_coded outside 1..4");
  if (check_coded && g.coded_stride < g.w) return refuse(JXLH_ERR_INVALID_ARGUMENT, "coded_stride below w");
  // the channel list: slot of an image channel, -1 for a palette's meta channel
  int list[JXLH_LOCAL_MAX_CHANNELS + JXLH_LOCAL_MAX_STEPS];
  uint32_t len = g.n_channels;
  for (uint32_t i = 0; i < len; i++) list[i] = (int)i;
  jxlh_local_op fwd[JXLH_LOCAL_MAX_STEPS] = {};
  uint32_t fwd_deltas[JXLH_LOCAL_MAX_STEPS] = {}, fwd_pred[JXLH_LOCAL_MAX_STEPS] = {};  // general palettes only
  for (uint32_t i = 0; i < g.n_steps; i++) {
    const jxlh_local_step& s = g.steps[i];
    jxlh_local_op& op = fwd[i];
    op.kind = s.kind;
    if (s.kind == JXLH_LOCAL_RCT) {
      if (s.rct_type >= 42) return refuse(JXLH_ERR_INVALID_ARGUMENT, "rct_type above 41");
      // check_equal_channels(channels, begin_channel, 3), meta_apply.rs:31-37
      if ((uint64_t)s.begin_c + 3 > len) return refuse(JXLH_ERR_INVALID_ARGUMENT, "RCT channel range leaves the channel list");
      int in[3];
      for (int k = 0; k < 3; k++) {
        in[k] = list[s.begin_c + k];
        if (in[k] < 0) return refuse(JXLH_ERR_UNSUPPORTED, "RCT on a palette meta channel");
      }
      int out[3];
      rct_permute((int)(s.rct_type / 7), in[0], in[1], in[2], out);  // meta_apply.rs:59-61
      op.rct_op = s.rct_type % 7;
      op.n_slots = 3;
      for (int k = 0; k < 3; k++) {
        op.in_slot[k] = (uint32_t)in[k];
        op.out_slot[k] = (uint32_t)out[k];
      }
    } else if (s.kind == JXLH_LOCAL_PALETTE) {
      if (s.num_c == 0) return refuse(JXLH_ERR_INVALID_ARGUMENT, "palette of no channel");
      // check_equal_channels(channels, begin_channel, num_channels), meta_apply.rs:188
      if ((uint64_t)s.begin_c + s.num_c > len) return refuse(JXLH_ERR_INVALID_ARGUMENT, "palette channel range leaves the channel list");
      if ((uint64_t)s.num_colors + s.num_deltas == 0) return refuse(JXLH_ERR_INVALID_ARGUMENT, "palette without entries");
      for (uint32_t k = 0; k < s.num_c; k++)
        if (list[s.begin_c + k] < 0) return refuse(JXLH_ERR_UNSUPPORTED, "palette of a palette meta channel");
      if (!general && (s.num_deltas > 0 || s.predictor != 0))
        return refuse(JXLH_ERR_UNSUPPORTED, "delta / predicted local palette");
      if (s.predictor > 13) return refuse(JXLH_ERR_INVALID_ARGUMENT, "predictor above 13");
      if (s.predictor == 6 && !wp) return refuse(JXLH_ERR_INVALID_ARGUMENT, "weighted predictor without a wp header");
      if (s.predictor == 6 && !wp_header_ok(*wp)) return refuse(JXLH_ERR_INVALID_ARGUMENT, "wp header field outside its width");
      if (bit_depth < 1 || bit_depth > 31) return refuse(JXLH_ERR_INVALID_ARGUMENT, "a palette needs a bit depth of 1..31");
      const uint64_t palette_size = (uint64_t)s.num_colors + s.num_deltas;
      if (palette_size > 0x7fffffffu) return refuse(JXLH_ERR_INVALID_ARGUMENT, "num_colors + num_deltas above 2^31 - 1");
      // the meta channel: num_c rows of num_colors + num_deltas values (meta_apply.rs:192-197)
      if (!local_fits(s.palette_offset, (uint64_t)s.num_c * palette_size, arena_samples))
        return refuse(JXLH_ERR_INVALID_ARGUMENT, "palette beyond the arena");
      if (s.predictor != 0) {  // a negative index is predicted even without delta entries (palette.rs:239)
        fwd_deltas[i] = s.num_deltas;
        fwd_pred[i] = s.predictor;
      }
      op.n_slots = s.num_c;  // <= 4: the range holds image channels only
      op.in_slot[0] = (uint32_t)list[s.begin_c];
      for (uint32_t k = 0; k < s.num_c; k++) op.out_slot[k] = (uint32_t)list[s.begin_c + k];
      op.num_colors = (uint32_t)palette_size;  // predictor 0: get_palette_value(.., num_colors + num_deltas) per pixel
      op.palette_offset = s.palette_offset;
      // channels.drain(begin + 1..begin + num); channels[begin] = index channel; channels.insert(0, meta) (:226-228)
      for (uint32_t k = s.begin_c + s.num_c; k < len; k++) list[k - (s.num_c - 1)] = list[k];
      len -= s.num_c - 1;
      for (uint32_t k = len; k > 0; k--) list[k] = list[k - 1];
      list[0] = -1;
      len++;
    } else {
      return refuse(JXLH_ERR_UNSUPPORTED, "a transform other than RCT and palette (local squeeze)");
    }
  }
  // what is left of the list is what the group's section decoded: the image-sized channels, in list order
  uint32_t coded_slot[JXLH_LOCAL_MAX_CHANNELS] = {}, n_coded = 0;
  for (uint32_t k = 0; k < len; k++)
    if (list[k] >= 0) coded_slot[n_coded++] = (uint32_t)list[k];
  if (check_coded && n_coded != g.n_coded) return refuse(JXLH_ERR_INVALID_ARGUMENT, "n_coded is not what the steps leave");
  if (check_coded && g.w > 0 && g.h > 0) {
    const uint64_t extent = (uint64_t)(g.h - 1) * g.coded_stride + g.w;
    for (uint32_t k = 0; k < n_coded; k++)
      if (!local_fits(g.coded_offset[k], extent, arena_samples)) return refuse(JXLH_ERR_INVALID_ARGUMENT, "coded channel beyond the arena");
  }
  if (prog) {
    *prog = jxlh_local_program{};
    prog->n_coded = n_coded;
    for (uint32_t k = 0; k < n_coded; k++) prog->coded_slot[k] = coded_slot[k];
    prog->n_ops = g.n_steps;
    for (uint32_t i = 0; i < g.n_steps; i++) prog->ops[i] = fwd[g.n_steps - 1 - i];  // local_apply: last step first
  }
  if (gprog) {
    *gprog = jxlh_local_general_program{};
    gprog->n_coded = n_coded;
    for (uint32_t k = 0; k < n_coded; k++) gprog->coded_slot[k] = coded_slot[k];
    gprog->n_ops = g.n_steps;
    uint32_t phase = 0;
    for (uint32_t i = 0; i < g.n_steps; i++) {
      const uint32_t f = g.n_steps - 1 - i;
      const jxlh_local_op& p = fwd[f];
      jxlh_local_general_op& q = gprog->ops[i];
      q.kind = p.kind, q.rct_op = p.rct_op, q.n_slots = p.n_slots, q.num_colors = p.num_colors, q.palette_offset = p.palette_offset;
      for (int k = 0; k < 3; k++) q.in_slot[k] = p.in_slot[k];
      for (int k = 0; k < 4; k++) q.out_slot[k] = p.out_slot[k];
      if (fwd_pred[f] != 0) {
        q.kind = JXLH_LOCAL_GENERAL_PALETTE;
        q.num_deltas = fwd_deltas[f], q.predictor = fwd_pred[f];
        phase += (phase & 1) ? 2 : 1;  // the next odd phase
        q.phase = phase;
      } else {
        phase += phase & 1;  // point-wise ops behind a general palette: the even phase after it
        q.phase = phase;
      }
    }
    uint32_t generals = 0;
    for (uint32_t i = 0; i < g.n_steps; i++) generals += fwd_pred[i] != 0;
    gprog->n_phases = 1 + 2 * generals;
  }
  return JXLH_OK;
}

inline jxlh_status local_lower_group(const jxlh_local_group& g, uint32_t bit_depth, uint64_t arena_samples,
                                     jxlh_local_program* prog, const char** why) {
  return local_lower_core(g, bit_depth, arena_samples, false, nullptr, prog, nullptr, why);
}

}  // namespace jxlh
