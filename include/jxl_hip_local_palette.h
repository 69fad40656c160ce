/*
 * jxl_hip_local_palette.h -- group-local palettes with delta entries and all 14 predictors on the device.  Part of the C
 * ABI of jxl_hip.h; this header includes it.  The declarations live in a header of their own for the reason
 * jxl_hip_save_rects.h gives: the set of entry points and structs jxl_hip.h itself declares is recorded per ABI version,
 * and these were added without a new version -- no existing symbol or struct changed, and the four group-local calls of
 * jxl_hip.h refuse exactly what they refused.  tools/gen_py_binding.py and tools/gen_rust_binding.py read this header as
 * they read jxl_hip.h (LOCAL_PALETTE_SYMBOLS in jxl_rs_amd/_abi.py, bindings/rust/jxl_hip_sys/src/local_palette.rs).
 */
/* (in front of the guard: jxl_hip.h ends by including jxl_hip_local_extra.h, which needs this header's declarations --
 * when this header is the first one a translation unit names, they are made on that way in, and skipped below) */
#include "jxl_hip.h"

#ifndef JXL_HIP_LOCAL_PALETTE_H_
#define JXL_HIP_LOCAL_PALETTE_H_

#ifdef __cplusplus
extern "C" {
#endif

/* The `_general` calls take the jxlh_local_group / jxlh_local_step of jxl_hip.h and everything said there about them,
 * and run EVERY local palette (TransformStep::Palette::local_apply -> do_palette_step_general, apply_local.rs:260-294,
 * palette.rs:165-262), not only the pure look-ups:
 *   predictor 0, num_deltas > 0   the prediction is 0, so every pixel is get_palette_value(.., num_colors + num_deltas):
 *                                 lowered to the look-up op with num_colors := num_colors + num_deltas.
 *   predictors 1..5, 7..13        a GENERAL palette, also with num_deltas == 0 (a negative index is < num_deltas and is
 *                                 predicted, palette.rs:239): the entry plus Predictor::predict_one of the group's own
 *                                 finished samples, wrapping to i32.
 *   predictor 6                   a GENERAL palette of the weighted kind: every pixel runs the self-correcting predictor
 *                                 (palette.rs:200-227) under the group's own header.
 *   wp   n entries, one per group (GroupHeader::wp_header); read only for groups with a predictor-6 step; may be null
 *        when no step of the call has predictor 6.
 * The bit depth is taken as min(bit_depth, 24) (palette.rs:177).
 *
 * Composition.  A group's inverse op list (last step first) is cut at its general palettes into PHASES: phase 0 holds
 * the point-wise ops (RCT, look-up palette) in front of the first general palette, phase 2k + 1 is the k-th general
 * palette, phase 2k + 2 the point-wise ops behind it; a phase may be empty.  A batch runs phase by phase: groups
 * without a general palette finish in the one k_modular_local launch a call of jxlh_modular_local_transforms issues; then
 * per non-empty phase ONE launch for all groups that have it (k_modular_local_phase for point-wise phases,
 * k_modular_local_palette for general palettes: one workgroup per (group, output channel), no workgroup waits on
 * another).  The number of launches is bounded by the deepest group's phase count (<= 2 * JXLH_LOCAL_MAX_STEPS + 1) and
 * never depends on the number of groups; a call without general palettes issues exactly the launch of the plain call.
 * Between phases a group's channels stay in its destination rect; an index channel that a general palette would
 * overwrite while other workgroups still read it is kept in context scratch.  Nothing outside a group's rect is read
 * or written.
 *
 * Statuses: as for the calls of jxl_hip.h (a refused call enqueues nothing, changes nothing and names the group in
 * *first_bad and jxlh_last_error), except
 *   JXLH_ERR_UNSUPPORTED       no longer: a palette with num_deltas > 0 or predictor != 0.  Still: a step whose range
 *                              touches a palette meta channel; any other transform kind (local squeeze: the _squeeze
 *                              calls of jxl_hip_local_squeeze.h); a chroma-subsampled frame; a sharded context.
 *   JXLH_ERR_INVALID_ARGUMENT  also: predictor > 13; predictor 6 with wp == NULL; a wp field outside its width (p1c, p2c,
 *                              p3ca..p3ce >= 32, w0..w3 >= 16: the rule of jxlh_palette_delta_wp) in a group that has a
 *                              predictor-6 step; a palette whose num_c * (num_colors + num_deltas) values leave the arena
 *                              (the meta channel's rows are num_colors + num_deltas wide, meta_apply.rs:192-197);
 *                              num_colors + num_deltas > 2^31 - 1; a group with a predicted palette wider than 2^30
 *                              samples. */
#define JXLH_LOCAL_GENERAL_PALETTE 2 /* jxlh_local_general_op::kind; never a jxlh_local_step::kind */

typedef struct jxlh_local_general_op {
  uint32_t kind;         /* JXLH_LOCAL_RCT, JXLH_LOCAL_PALETTE (look-up) or JXLH_LOCAL_GENERAL_PALETTE */
  uint32_t rct_op;       /* RCT: 0..6 */
  uint32_t n_slots;      /* RCT: 3; palettes: num_c */
  uint32_t in_slot[3];   /* RCT: the slots read as v0, v1, v2; palettes: in_slot[0] holds the index */
  uint32_t out_slot[4];  /* RCT: the slots w0, w1, w2 go to; palettes: the slot of channel c */
  uint32_t num_colors;   /* palettes: the palette_size of get_palette_value = the step's num_colors + num_deltas */
  uint32_t num_deltas;   /* general palette: entries below this index are added to the prediction; else 0 */
  uint32_t predictor;    /* general palette: 1..13; else 0 */
  uint32_t phase;        /* point-wise: even; the k-th general palette of the group: 2k + 1 */
  uint64_t palette_offset;
} jxlh_local_general_op;
typedef struct jxlh_local_general_program {
  uint32_t n_coded;
  uint32_t coded_slot[4];
  uint32_t n_ops;
  uint32_t n_phases;     /* 1 + 2 * (general palettes of the group): phases 0 .. n_phases - 1, some possibly empty */
  jxlh_local_general_op ops[4]; /* the inverse steps, last step first; phase never decreases */
} jxlh_local_general_program;

/* Pure host code (no context, no device): jxlh_modular_local_lower for the general calls.  programs: n entries, or null
 * for the checks alone; a refused call leaves them as they were. */
jxlh_status jxlh_modular_local_lower_general(const jxlh_local_group* groups, const jxlh_wp_header* wp, size_t n,
                                             uint32_t bit_depth, uint64_t arena_samples,
                                             jxlh_local_general_program* programs, size_t* first_bad);
/* jxlh_modular_local_transforms with every local palette: the same destination rules, returns when the result is in
 * `out`. */
jxlh_status jxlh_modular_local_transforms_general(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                  const jxlh_local_group* groups, const jxlh_wp_header* wp, size_t n,
                                                  uint32_t bit_depth, int32_t* const out[], uint32_t n_out, uint32_t out_w,
                                                  uint32_t out_h, size_t out_stride, size_t* first_bad);
/* jxlh_frame_set_modular_groups[_async] with every local palette: the same rules (grey fan-out, one sample_format per
 * frame, replaceable after a run, freely mixed with the other setters on other rects; the _async form's arena stays valid
 * until the next jxlh_ctx_sync / waited mark, wp is read before the call returns). */
jxlh_status jxlh_frame_set_modular_groups_general(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                  const jxlh_local_group* groups, const jxlh_wp_header* wp, size_t n,
                                                  uint32_t sample_format, size_t* first_bad);
jxlh_status jxlh_frame_set_modular_groups_general_async(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                        const jxlh_local_group* groups, const jxlh_wp_header* wp, size_t n,
                                                        uint32_t sample_format, size_t* first_bad);

#ifdef __cplusplus
}
#endif
#endif /* JXL_HIP_LOCAL_PALETTE_H_ */
