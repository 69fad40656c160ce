/*
 * jxl_hip_save_rects.h -- save rectangles: repaint only what a group re-render changed.  Part of the C ABI of
 * jxl_hip.h, which includes this header; including either one gives the whole interface.  The declarations live in a
 * header of their own for the reason jxl_hip_preview.h gives: the set of entry points and structs jxl_hip.h itself
 * declares is recorded per ABI version, and these were added without a new version -- no existing symbol or struct
 * changed.  tools/gen_py_binding.py and tools/gen_rust_binding.py read this header as they read jxl_hip.h
 * (SAVE_RECTS_SYMBOLS in jxl_rs_amd/_abi.py, bindings/rust/jxl_hip_sys/src/save_rects.rs).
 */
#ifndef JXL_HIP_SAVE_RECTS_H_
#define JXL_HIP_SAVE_RECTS_H_

#include "jxl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* jxlh_frame_save_rects / _async / jxlh_stage_save_rects are jxlh_frame_save / _async / jxlh_stage_save ("the save tail"
 * in jxl_hip.h) with the row band replaced by a list of rectangles of the SOURCE: the result's coordinates, the (x, y)
 * of that section -- image coordinates after jxlh_frame_blend.  `out` and bytes_per_row describe the WHOLE oriented
 * image, as there.  Every source pixel that lies in at least one rect (a rect is cut at the result's right and bottom
 * edge, as y1 is) is written at display_pixel((x, y), (w, h)) with exactly the samples jxlh_frame_save writes for it:
 * the same colour stage, spot colours, premultiplication and conversion, the dither phase of its absolute (x, y) and
 * pipeline channel (plus frame_x0 / frame_y0 in the stage form), the same fill and byte order.  No byte of a pixel
 * outside the union of the rects is written and row padding never is, for 1-, 2-, 3- and 6-byte pixels too: the edges
 * of a rect inside a dword are stored bytewise.  Rects may overlap (the same bytes land twice); a rect with w == 0 or
 * h == 0 is skipped, wherever it starts; n == 0 is JXLH_OK with nothing enqueued.  Results of any kind are served, as
 * by jxlh_frame_save; the extra channels resolve as there.
 * Device destination: all rects are written in ONE kernel launch, in place, never waited for.  Host destination: the
 * rects are staged one after another in the context's staging buffer, each at its own dword-rounded pitch, and leave
 * it with one 2-D copy of exactly its pixel bytes per rect -- the bytes that cross the bus are the rects' bytes.  The
 * blocking forms wait once at the end; _async follows jxlh_frame_save_async.
 * Statuses: everything jxlh_frame_save (jxlh_stage_save) checks, in its order and with its status, the list standing
 * where y0 / y1 stand.  JXLH_ERR_INVALID_ARGUMENT also for rects == NULL with n > 0, n > JXLH_MAX_SAVE_RECTS, a rect
 * with x0 >= width or y0 >= height whose w and h are non-zero, and x0 + w or y0 + h beyond 32 bits.
 * JXLH_ERR_UNSUPPORTED also for a list that would take 2^31 workgroups or more (thousands of image-sized rects).
 * All of it is decided before anything is enqueued or written. */
typedef struct jxlh_rect {
  uint32_t x0, y0, w, h; /* pixels of a frame's RESULT (source coordinates) */
} jxlh_rect;
#define JXLH_MAX_SAVE_RECTS 4096
jxlh_status jxlh_frame_save_rects(jxlh_ctx* ctx, const jxlh_output_desc* colour, const jxlh_save_desc* save,
                                  const jxlh_rect* rects, uint32_t n, void* out, size_t bytes_per_row);
jxlh_status jxlh_frame_save_rects_async(jxlh_ctx* ctx, const jxlh_output_desc* colour, const jxlh_save_desc* save,
                                        const jxlh_rect* rects, uint32_t n, void* out, size_t bytes_per_row);
jxlh_status jxlh_stage_save_rects(jxlh_ctx* ctx, const jxlh_output_desc* colour, const jxlh_save_desc* save,
                                  const float* const planes[], uint32_t n_planes, uint32_t w, uint32_t h, size_t stride,
                                  uint32_t frame_x0, uint32_t frame_y0, const jxlh_rect* rects, uint32_t n, void* out,
                                  size_t bytes_per_row);

/* Pure host code: no context, no device, any thread.  The rectangles of the frame's result, in result coordinates,
 * outside which jxlh_frame_rerender_groups(group_ids, count) leaves every pixel bit-identical -- and so does a later
 * whole jxlh_frame_run after only those groups' coefficients or LF-only marks changed.  A group's 256 x 256 pixels are
 * widened on all four sides by the reach of the frame's stage list (Gaborish 1, EPF0 3, EPF1 2, EPF2 1 pixels: 0 to
 * 7), plus one pixel on an axis on which a channel is sub-sampled (the chroma upsampling in front of the filters reads
 * one sub-sampled neighbour), and clipped to xsize x ysize: never more than 8 pixels beyond the groups.  Patches,
 * splines and noise do not widen it.  (Held to the oracle by tests/test_changed_rects_cpu.py.)
 * One rect per maximal run of listed groups that are horizontal neighbours in one group row, in ascending group
 * order; duplicate ids count once; rects of neighbouring group rows may overlap (jxlh_frame_save_rects takes them as
 * they are).  *n is always the number of rects needed.
 * After jxlh_frame_blend the result is the canvas in image coordinates: shift the rects by the frame's (x0, y0) and
 * clip them to the image before saving them.
 * JXLH_ERR_INVALID_ARGUMENT: a null pointer (rects may be NULL while cap == 0); parameters jxlh_frame_begin refuses
 * (abi_version, sizes, epf_iters, shifts); an id beyond the frame's group count; cap smaller than needed (*n is set).
 * JXLH_ERR_UNSUPPORTED: exactly where jxlh_frame_rerender_groups says so from the parameters alone: upsampling > 1,
 * JXLH_FRAME_MODULAR. */
jxlh_status jxlh_changed_rects(const jxlh_frame_params* p, const uint32_t* group_ids, uint32_t count, jxlh_rect* rects,
                               uint32_t cap, uint32_t* n);

#ifdef __cplusplus
}
#endif
#endif /* JXL_HIP_SAVE_RECTS_H_ */
