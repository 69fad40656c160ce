/*
 * jxl_hip_local_extra.h -- group-local transforms with extra channels: the groups of an RGBA (grey + alpha, colour +
 * depth + spot ...) image go straight into the frame's colour planes AND its extra channels' sample stores.  Part of the
 * C ABI of jxl_hip.h, which includes this header at its end; this header includes jxl_hip_local_squeeze.h (and through
 * it jxl_hip_local_palette.h and jxl_hip.h), so including any of the four, in any order, gives the whole interface (the
 * two older headers include what they need in front of their guards, so that their declarations exist by the time
 * jxl_hip.h reaches this header).  They live
 * in a header of their own for the reason jxl_hip_save_rects.h gives: the set of entry points and structs jxl_hip.h
 * itself declares is recorded per ABI version, and these were added without a new version -- no existing symbol or
 * struct changed.  tools/gen_py_binding.py and tools/gen_rust_binding.py read this header as they read the others
 * (LOCAL_EXTRA_SYMBOLS in jxl_rs_amd/_abi.py, bindings/rust/jxl_hip_sys/src/local_extra.rs).
 */
#ifndef JXL_HIP_LOCAL_EXTRA_H_
#define JXL_HIP_LOCAL_EXTRA_H_

#include "jxl_hip_local_squeeze.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A lossless RGBA picture decodes to Modular groups that hold R, G, B and A side by side: one palette over all four, an
 * RCT on 0..2, a palette or a squeeze on the alpha alone.  A lossy VarDCT photo carries its alpha, depth and spot
 * channels the same way.  jxlh_frame_set_modular_groups_extra is jxlh_frame_set_modular_groups_squeeze for such groups:
 * the inverses run exactly as there (the group form is that of jxl_hip_local_squeeze.h, the superset: groups without a
 * squeeze, with plain or general palettes and with RCTs are accepted in one batch), and every finished channel is stored
 * where the frame keeps it -- the leading n_colour channels in the frame's sample planes, channel n_colour + k in the i32
 * sample store of extra channel ec[k] (jxl_hip_extra_rects.h).  No intermediate plane, no scatter launch, no wait.
 *
 *   n_colour > 0   a Modular frame; everything jxlh_frame_set_modular_groups_squeeze demands of the frame and of
 *                  sample_format holds (grey, n_colour == 1, is fanned out to the three planes).  Rects are in the
 *                  frame's coded coordinates.  Every named extra channel must be set (begun by
 *                  jxlh_frame_begin_extra_channel or handed over whole) and have exactly the frame's coded size,
 *                  whatever its ec_upsampling.
 *   n_colour == 0  accepted on VarDCT and Modular frames alike.  sample_format must be 0.  All named extra channels
 *                  share one size w x h, and rects are in that channel resolution (as jxlh_ec_rect).  This is also how
 *                  channels with a dim_shift of their own arrive on a Modular frame: a second call.
 *
 * State afterwards.  For the colour, what jxlh_frame_set_modular_groups_squeeze leaves.  For each named extra channel,
 * exactly what ONE jxlh_frame_set_extra_channel_rects call with the non-empty group rects would leave: a whole-plane
 * channel takes rect state, the rects' tiles are dirty, the channel is not rendered (the read-out, a save or a blend that
 * names it answers JXLH_ERR_BAD_STATE) until the next jxlh_frame_run, jxlh_frame_rerender_groups or
 * jxlh_frame_repaint_groups, and a patched copy is rebuilt by the next patches launch.
 * jxlh_extra_channel_changed_rects keeps naming what to repaint.
 *
 * Launches: exactly those jxlh_frame_set_modular_groups_squeeze issues for the same groups (at most one plain launch,
 * the squeeze launches, the phases); no k_ec_scatter, no copy between planes.  The blocking form returns when the arena
 * may be reused; _async returns after enqueueing, and the arena stays valid until the next jxlh_ctx_sync or waited mark.
 * groups, coded, params, wp and dest are read before the call returns.
 *
 * Every refusal is decided before anything is enqueued and changes nothing; *first_bad (may be NULL) and jxlh_last_error
 * name the group (refusals of the call as a whole leave *first_bad alone).  The checks, in this order:
 *   1. JXLH_ERR_INVALID_ARGUMENT  ctx, arena or dest == NULL; groups == NULL with n > 0
 *   2. JXLH_ERR_INVALID_ARGUMENT  n_colour not 0, 1 or 3; n_colour + n_ec outside 1..JXLH_LOCAL_MAX_CHANNELS; an ec[k]
 *                                 >= JXLH_MAX_EXTRA_CHANNELS or named twice; bit_depth != 0 with n_colour > 0, or above 31;
 *                                 sample_format != 0 with n_colour == 0; with n_colour > 0, a sample_format
 *                                 jxlh_frame_set_modular_groups_squeeze rejects
 *   3. JXLH_ERR_BAD_STATE         outside a frame; n_colour > 0 on a VarDCT frame
 *   4. JXLH_ERR_UNSUPPORTED       a sharded context; n_colour > 0 on a chroma-subsampled Modular frame
 *   5. JXLH_ERR_BAD_STATE         a named channel that is not set
 *   6. JXLH_ERR_UNSUPPORTED       a named channel of another size than the call's planes (the frame's coded size, or
 *                                 the first named channel's)
 *   7. JXLH_ERR_INVALID_ARGUMENT  a sample_format other than the one the frame's earlier group calls used
 *   8. per group: everything the squeeze-form lowering rejects, with its status; JXLH_ERR_INVALID_ARGUMENT for
 *      n_channels != n_colour + n_ec; for a rect that leaves the planes; then the caps of the other group-local calls.
 *
 * Out of scope (today's routes -- jxlh_modular_local_transforms_squeeze into caller planes, then
 * jxlh_frame_set_modular_channels and jxlh_frame_set_extra_channel_rects -- stay): more than four channels in a group;
 * groups of one call with different channel layouts (issue one call per layout); extra channels of another size in a
 * call that has colour; sharded contexts; chroma-subsampled Modular frames; previews of local squeezes. */
typedef struct jxlh_local_dest {
  uint32_t n_colour;  /* 0, 1 or 3: the leading channels of EVERY group of the call that are the frame's colour channels */
  uint32_t n_ec;      /* the channels behind them: n_colour + n_ec in 1..JXLH_LOCAL_MAX_CHANNELS */
  uint32_t ec[4];     /* group channel n_colour + k is extra channel ec[k]; distinct, each < JXLH_MAX_EXTRA_CHANNELS */
  uint32_t bit_depth; /* n_colour == 0: the palettes' bit depth (0 allowed when no group has a palette); otherwise 0 --
                         the depth is sample_format's, as for the other frame calls */
} jxlh_local_dest;

jxlh_status jxlh_frame_set_modular_groups_extra(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                const jxlh_local_squeeze_group* groups, size_t n,
                                                const jxlh_local_coded_channel* coded, size_t n_coded,
                                                const jxlh_squeeze_params* params, size_t n_params,
                                                const jxlh_wp_header* wp, uint32_t sample_format,
                                                const jxlh_local_dest* dest, size_t* first_bad);
jxlh_status jxlh_frame_set_modular_groups_extra_async(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                      const jxlh_local_squeeze_group* groups, size_t n,
                                                      const jxlh_local_coded_channel* coded, size_t n_coded,
                                                      const jxlh_squeeze_params* params, size_t n_params,
                                                      const jxlh_wp_header* wp, uint32_t sample_format,
                                                      const jxlh_local_dest* dest, size_t* first_bad);

#ifdef __cplusplus
}
#endif
#endif /* JXL_HIP_LOCAL_EXTRA_H_ */
