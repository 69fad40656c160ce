/*
 * jxl_hip_local_squeeze.h -- group-local squeeze on the device: the inverse squeeze of many groups per call.  Part of
 * the C ABI of jxl_hip.h; this header includes jxl_hip_local_palette.h (and through it jxl_hip.h).  The declarations live
 * in a header of their own for the reason jxl_hip_save_rects.h gives: the set of entry points and structs jxl_hip.h
 * itself declares is recorded per ABI version, and these were added without a new version -- no existing symbol or
 * struct changed, and the group-local calls of jxl_hip.h and jxl_hip_local_palette.h refuse a squeeze exactly as they
 * did.  tools/gen_py_binding.py and tools/gen_rust_binding.py read this header as they read jxl_hip.h
 * (LOCAL_SQUEEZE_SYMBOLS in jxl_rs_amd/_abi.py, bindings/rust/jxl_hip_sys/src/local_squeeze.rs).
 */
/* (in front of the guard, for the reason jxl_hip_local_palette.h gives) */
#include "jxl_hip_local_palette.h"

#ifndef JXL_HIP_LOCAL_SQUEEZE_H_
#define JXL_HIP_LOCAL_SQUEEZE_H_

#ifdef __cplusplus
extern "C" {
#endif

/* A group whose GroupHeader carries TransformId::Squeeze (an encoder that works group by group has no global transform to
 * put its squeeze in).  In TransformStep::local_apply a group's squeeze steps are closed inside the group (in_next_avg and
 * out_prev are None, apply_local.rs:295-348), so groups are independent and a batch of them is inverted in launches
 * whose number does not depend on the number of groups.
 *
 *   group    self-contained: the rect, n_channels, the RCT / palette steps IN FRONT of the squeeze in bitstream order
 *            (jxlh_local_step, everything jxl_hip_local_palette.h says about them), whether it has a squeeze at all
 *            (groups without one are accepted in the same batch), the squeeze's SqueezeParams as a range of the
 *            call-wide `params` array, and its coded channels as a range of the call-wide `coded` array.
 *   params   headers::modular::SqueezeParams.  n_params == 0 with has_squeeze: default_squeeze (squeeze.rs:39-105,
 *            with its 4:2:0-preview branch for more than 2 equal channels) of the channel list as it stands.
 *            begin_c indexes that list: palette meta channels first.
 *   coded    the image channels of the list after ALL transforms, in list order (meta_apply.rs:90-180: an in-place
 *            squeeze puts the residuals behind its range, any other at the end); palette meta channels are not counted,
 *            their samples stay at palette_offset.  w and h are checked against what the lowering derives.  A channel
 *            with a zero side (the residual of a 1-sample axis) has no samples: offset and stride are ignored.
 *   wp       as for the _general calls: n entries or null.
 *
 * Accepted: one squeeze per group, as the LAST transform of its list (its inverse runs first), on image channels only,
 * at most JXLH_LOCAL_SQUEEZE_MAX_LEVELS levels per image channel (a default squeeze of a 1024 x 1024 group: 14 levels
 * plus the 2 preview levels).  Samples as for jxlh_unsqueeze_chain: bit-exact within +-2^28.
 *
 * Launches.  jxlh_modular_local_lower_squeeze derives, per image channel that reaches the squeeze, its CHAIN: the coded
 * channel that is its base and, level by level in the order the inverse runs, the axis, the output size and the coded
 * channel that holds the residuals.  One launch (k_modular_local_squeeze_lds) walks, for every chain of the batch, the
 * levels whose planes fit its LDS tile (sides <= 128); the levels beyond run as ONE launch per level index for the whole
 * batch (k_modular_local_squeeze_level), intermediates in context scratch.  A chain's last level writes the group's
 * destination rect; the RCT / palette phases of jxl_hip_local_palette.h then run on the rect.  The number of launches
 * is bounded by the deepest chain plus its phases.  Groups without a squeeze whose coded channels share one stride run
 * exactly as in the _general calls: a batch without a squeeze group issues exactly those launches.  No workgroup waits
 * on another; nothing outside a group's rect is written.
 *
 * Statuses: as for the _general calls (a refused call enqueues nothing, changes nothing and names the group in
 * *first_bad and jxlh_last_error), and
 *   JXLH_ERR_UNSUPPORTED       (the group stays on the host) a transform behind the squeeze (squeeze_pos < n_steps); a
 *                              second squeeze (a step of a kind other than RCT / palette in `steps`); a squeeze range
 *                              that touches a palette meta channel; a squeeze of a residual channel; more than 16 levels
 *                              on a channel; a coded channel that is missing (n_coded below what the transforms leave:
 *                              smooth previews of local squeezes are out of scope); a group wider or taller than 2^20
 *                              with a squeeze; a chroma-subsampled frame; a sharded context.
 *   JXLH_ERR_INVALID_ARGUMENT  a squeeze range that leaves the list (the reference's InvalidChannelRange) or is empty; a
 *                              params or coded range that leaves its array; has_squeeze above 1; has_squeeze == 0 with
 *                              n_params != 0; squeeze_pos > n_steps; n_coded above what the transforms leave; a coded w
 *                              or h that is not what they leave; stride < w; an offset + extent beyond the arena;
 *                              everything the general lowering rejects. */
#define JXLH_LOCAL_SQUEEZE_MAX_LEVELS 16
#define JXLH_LOCAL_SQUEEZE_MAX_CODED 68 /* 4 bases + 4 * 16 residuals */

typedef struct jxlh_squeeze_params {
  uint32_t horizontal, in_place, begin_c, num_c;
} jxlh_squeeze_params;
typedef struct jxlh_local_coded_channel {
  uint64_t offset;  /* samples into the arena */
  uint32_t stride;  /* >= w */
  uint32_t w, h;
} jxlh_local_coded_channel;
typedef struct jxlh_local_squeeze_group {
  uint32_t x0, y0, w, h;     /* the rect; w or h 0: checked, then skipped */
  uint32_t n_channels;       /* 1..JXLH_LOCAL_MAX_CHANNELS */
  uint32_t n_steps;          /* RCT / palette steps in front of the squeeze, 0..JXLH_LOCAL_MAX_STEPS */
  jxlh_local_step steps[4];
  uint32_t has_squeeze;      /* 0 or 1 */
  uint32_t squeeze_pos;      /* has_squeeze: where the squeeze stands in the group's transform list, `steps` being the
                                others in their order; accepted: n_steps (the last transform) */
  uint32_t params_first, n_params;
  uint32_t coded_first, n_coded;
} jxlh_local_squeeze_group;

/* What a group lowers to.  chain k belongs to general.coded_slot[k]: its finished plane is what the general program
 * loads into that slot.  n_levels == 0: the channel is not squeezed, `base` is it.  base / res index the group's coded
 * range. */
typedef struct jxlh_local_squeeze_level {
  uint32_t horizontal, out_w, out_h;
  uint32_t res;              /* the coded channel of the residuals: (out_w / 2) x out_h or out_w x (out_h / 2) */
} jxlh_local_squeeze_level;
typedef struct jxlh_local_squeeze_chain {
  uint32_t base, base_w, base_h;
  uint32_t n_levels;
  jxlh_local_squeeze_level levels[16]; /* [JXLH_LOCAL_SQUEEZE_MAX_LEVELS] in the order the inverse runs */
} jxlh_local_squeeze_chain;
typedef struct jxlh_local_squeeze_program {
  jxlh_local_general_program general; /* the steps' program; n_coded = the channels that reach the squeeze */
  uint32_t n_coded;                   /* coded channels the group must bring */
  jxlh_local_squeeze_chain chains[4];
} jxlh_local_squeeze_program;

/* Pure host code: default_squeeze for a channel list of n_meta palette meta channels followed by n image channels of
 * w[i] x h[i].  params: room for `cap` entries (may be null with cap 0); *n_params: how many the list has.  Returns
 * JXLH_ERR_INVALID_ARGUMENT when n is 0 or above 4, or the list is longer than cap (then *n_params is still set). */
jxlh_status jxlh_modular_local_default_squeeze(const uint32_t* w, const uint32_t* h, uint32_t n, uint32_t n_meta,
                                               jxlh_squeeze_params* params, uint32_t cap, uint32_t* n_params);
/* Pure host code (no context, no device): mirrors the squeeze branch of meta_apply_single_transform on each group's
 * channel list behind the general lowering of its steps, and checks everything listed above that does not need a frame.
 * programs: n entries, or null for the checks alone; a refused call leaves them as they were. */
jxlh_status jxlh_modular_local_lower_squeeze(const jxlh_local_squeeze_group* groups, size_t n,
                                             const jxlh_local_coded_channel* coded, size_t n_coded,
                                             const jxlh_squeeze_params* params, size_t n_params, const jxlh_wp_header* wp,
                                             uint32_t bit_depth, uint64_t arena_samples,
                                             jxlh_local_squeeze_program* programs, size_t* first_bad);
/* jxlh_modular_local_transforms_general with local squeezes: the same destination rules, returns when the result is in
 * `out`. */
jxlh_status jxlh_modular_local_transforms_squeeze(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                  const jxlh_local_squeeze_group* groups, size_t n,
                                                  const jxlh_local_coded_channel* coded, size_t n_coded,
                                                  const jxlh_squeeze_params* params, size_t n_params,
                                                  const jxlh_wp_header* wp, uint32_t bit_depth, int32_t* const out[],
                                                  uint32_t n_out, uint32_t out_w, uint32_t out_h, size_t out_stride,
                                                  size_t* first_bad);
/* jxlh_frame_set_modular_groups_general[_async] with local squeezes: the same rules (grey fan-out, one sample_format per
 * frame, replaceable after a run, freely mixed with the other setters on other rects; the _async form's arena stays valid
 * until the next jxlh_ctx_sync / waited mark; groups, coded, params and wp are read before the call returns). */
jxlh_status jxlh_frame_set_modular_groups_squeeze(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                  const jxlh_local_squeeze_group* groups, size_t n,
                                                  const jxlh_local_coded_channel* coded, size_t n_coded,
                                                  const jxlh_squeeze_params* params, size_t n_params,
                                                  const jxlh_wp_header* wp, uint32_t sample_format, size_t* first_bad);
jxlh_status jxlh_frame_set_modular_groups_squeeze_async(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                        const jxlh_local_squeeze_group* groups, size_t n,
                                                        const jxlh_local_coded_channel* coded, size_t n_coded,
                                                        const jxlh_squeeze_params* params, size_t n_params,
                                                        const jxlh_wp_header* wp, uint32_t sample_format,
                                                        size_t* first_bad);

#ifdef __cplusplus
}
#endif
#endif /* JXL_HIP_LOCAL_SQUEEZE_H_ */
