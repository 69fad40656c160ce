/*
 * jxl_hip_blend_rects.h -- blend rectangles: recompose only what a group re-render changed.  Part of the C ABI of
 * jxl_hip.h, which includes this header; including either one gives the whole interface.  The declarations live in a
 * header of their own for the reason jxl_hip_save_rects.h gives: the set of entry points and structs jxl_hip.h itself
 * declares is recorded per ABI version, and these were added without a new version -- no existing symbol or struct
 * changed.  tools/gen_py_binding.py and tools/gen_rust_binding.py read this header as they read jxl_hip.h
 * (BLEND_RECTS_SYMBOLS in jxl_rs_amd/_abi.py, bindings/rust/jxl_hip_sys/src/blend_rects.rs).
 */
#ifndef JXL_HIP_BLEND_RECTS_H_
#define JXL_HIP_BLEND_RECTS_H_

#include "jxl_hip.h"
#include "jxl_hip_save_rects.h" /* jxlh_rect, JXLH_MAX_SAVE_RECTS */

#ifdef __cplusplus
extern "C" {
#endif

/* Pure host code: no context, no device, any thread.  Rects of a frame's result -- what jxlh_changed_rects,
 * jxlh_repaint_changed_rects and jxlh_extra_channel_changed_rects return, in the coordinates of the frame_w x frame_h
 * result -- as rects of the image `desc` composes the frame onto.  Each rect is cut at frame_w x frame_h, shifted by
 * (desc->x0, desc->y0) -- the origin may be negative and is clamped to +-2^30 as jxlh_frame_blend clamps it; the
 * arithmetic is 64-bit -- and intersected with image_w x image_h.  Rects that become empty are dropped, the order of
 * the others is kept; only x0, y0, image_w and image_h of the descriptor are read.  The list serves both
 * jxlh_frame_blend_rects and, after it, jxlh_frame_save_rects.  *n_out is always the number of rects needed.
 * JXLH_ERR_INVALID_ARGUMENT: a null pointer (frame_rects may be NULL while n == 0, image_rects while cap == 0); cap
 * smaller than needed (*n_out is set, nothing is written). */
jxlh_status jxlh_blend_image_rects(const jxlh_blend_desc* desc, uint32_t frame_w, uint32_t frame_h,
                                   const jxlh_rect* frame_rects, uint32_t n, jxlh_rect* image_rects, uint32_t cap,
                                   uint32_t* n_out);

/* jxlh_frame_blend_rects recomposes the listed rectangles of a KEPT COMPOSITION: the canvas an earlier successful
 * jxlh_frame_blend or jxlh_frame_blend_rects has written since jxlh_frame_begin, with the same descriptor in the fields
 * the blend reads (x0, y0, image_w, image_h, num_ec; mode, clamp and source of the colour and of every extra channel,
 * alpha_channel where the mode reads it; the alpha bits of ec_flags) and with the same colour stage.  A render
 * (jxlh_frame_run, jxlh_frame_rerender_groups, jxlh_frame_repaint_groups, the extra-channel rect calls) points the
 * frame's result back at the frame's own planes, as documented there, but the canvas is a buffer of its own that
 * nothing else writes: the composition stays in memory, stale where the render changed pixels.
 * `rects` are IMAGE coordinates (jxlh_blend_image_rects maps a frame's changed rects); the rules for the list are
 * those of jxlh_frame_save_rects against image_w x image_h: at most JXLH_MAX_SAVE_RECTS rects, a rect is cut at the
 * image's right and bottom edge, a rect with w == 0 or h == 0 is skipped wherever it starts, rects may overlap.
 * The call rewrites exactly the canvas samples of the pixels that lie in at least one rect, each with the value
 * jxlh_frame_blend would give it now, bit for bit: colour stage and blend inside the frame, the source slot's value
 * (or zero) outside it.  No other sample of the canvas is written.  The canvas then IS THE FRAME'S RESULT again,
 * exactly as after jxlh_frame_blend: every read, jxlh_frame_save[_rects] and jxlh_frame_save_reference serve it.
 * n == 0, or a list of only empty rects, launches nothing and still makes the canvas the result.  All rects go in ONE
 * kernel launch on the context's stream; the call never waits for the device, like jxlh_frame_blend.
 * THE CALLER'S CONTRACT: every image pixel one of whose inputs has changed since the canvas was last written -- the
 * frame's sample there, an extra channel's, or a source slot's (jxlh_frame_save_reference into a slot the descriptor
 * names) -- must lie in a rect.  The library cannot check this and does not try: a pixel left out keeps its old value.
 * Statuses, all decided before anything is enqueued; a refused call changes nothing: everything jxlh_frame_blend
 * checks, in its order and with its status (sharded contexts: JXLH_ERR_UNSUPPORTED); then JXLH_ERR_BAD_STATE without a
 * kept composition; JXLH_ERR_INVALID_ARGUMENT for a descriptor or colour stage that differs from the kept one; the
 * list's errors as in jxlh_frame_save_rects (JXLH_ERR_INVALID_ARGUMENT: rects == NULL with n > 0, n >
 * JXLH_MAX_SAVE_RECTS, a non-empty rect with x0 >= image_w or y0 >= image_h, x0 + w or y0 + h beyond 32 bits);
 * JXLH_ERR_UNSUPPORTED for a list that would take 2^31 workgroups or more. */
jxlh_status jxlh_frame_blend_rects(jxlh_ctx* ctx, const jxlh_blend_desc* desc, const jxlh_output_desc* colour,
                                   const jxlh_rect* rects, uint32_t n);

/* jxlh_stage_blend with a rect list in front of out[]: the same kernel as jxlh_frame_blend_rects on caller planes.
 * out[] must already hold a composition; only the samples of the pixels in the rects (image coordinates, the list
 * rules above) are rewritten.  Device planes whose rows are 16-byte aligned (16-byte-aligned pointers, out_stride a
 * multiple of 4) are written in place; host planes -- and device planes at another alignment -- are staged whole:
 * copied in, the rects rewritten, copied out.  The frame planes are staged as in jxlh_stage_blend.  The statuses of
 * jxlh_stage_blend, then the list's.  The Modular seam and tests. */
jxlh_status jxlh_stage_blend_rects(jxlh_ctx* ctx, const jxlh_blend_desc* desc, const float* const frame[],
                                   uint32_t n_channels, uint32_t w, uint32_t h, size_t stride, const jxlh_rect* rects,
                                   uint32_t n, float* const out[], size_t out_stride);

#ifdef __cplusplus
}
#endif
#endif /* JXL_HIP_BLEND_RECTS_H_ */
