/*
 * jxl_hip_repaint.h -- repaint groups of upsampled and Modular frames in one call.  Part of the C ABI of jxl_hip.h,
 * which includes this header; including either one gives the whole interface.  The declarations live in a header of
 * their own for the reason jxl_hip_save_rects.h gives: the set of entry points and structs jxl_hip.h itself declares is
 * recorded per ABI version, and these were added without a new version -- no existing symbol or struct changed.
 * tools/gen_py_binding.py and tools/gen_rust_binding.py read this header as they read jxl_hip.h (REPAINT_SYMBOLS in
 * jxl_rs_amd/_abi.py, bindings/rust/jxl_hip_sys/src/repaint.rs).
 */
#ifndef JXL_HIP_REPAINT_H_
#define JXL_HIP_REPAINT_H_

#include "jxl_hip.h"
#include "jxl_hip_save_rects.h" /* jxlh_rect */

#ifdef __cplusplus
extern "C" {
#endif

/* jxlh_frame_repaint_groups re-renders the listed groups of the current frame after a whole jxlh_frame_run, on every
 * kind of unsharded frame: it is jxlh_frame_rerender_groups without the two refusals that call keeps (upsampling > 1,
 * JXLH_FRAME_MODULAR).  Group ids are cells of the 256 x 256 grid over the CODED size, row-major, ceil(xsize / 256) per
 * row: a VarDCT frame's groups; for a Modular frame the same grid, whatever the codestream's group size (its group rows
 * are the 256-row bands of jxlh_frame_run).  Afterwards the result planes are bit for bit what a fresh context gives for
 * the same final inputs.
 *   VarDCT, upsampling 1        exactly what jxlh_frame_rerender_groups enqueues and returns.
 *   VarDCT, upsampling 2, 4, 8  at the coded size what jxlh_frame_rerender_groups does for the same frame without
 *                               upsampling: transforms or LF fill of the listed groups, the filters on the row bands they
 *                               reach, patches and splines on those rows -- or the whole run where that call runs the
 *                               frame again (never rendered, a stage list that ends in the planes the transforms write,
 *                               the strip kernel, chroma subsampling, patches / splines / noise without a filter stage).
 *                               Then, for every rewritten band [y_lo, y_hi), Upsample<N> of the three colour planes on
 *                               centre rows [max(0, y_lo - 2), min(ysize, y_hi + 2)) (ranges that overlap or touch are
 *                               merged; one launch per range for all three planes), and the noise on exactly the result
 *                               rows that were written again: no row receives it twice.
 *   Modular, any upsampling     the caller has replaced samples beforehand (jxlh_frame_set_modular_channels /
 *                               _set_modular_groups).  For every maximal run of listed group rows [gy0, gy1) the intake
 *                               jxlh_frame_run(ctx, gy0, gy1) does, and the stage list on the run's rows widened by the
 *                               stage list's reach (a replaced sample changes filtered rows of the neighbouring band
 *                               too); the whole run where jxlh_frame_run renders such a band whole, and on
 *                               chroma-subsampled frames.  On an upsampled frame the row-range upsampling and noise follow
 *                               as above.
 *   never rendered whole        if no whole run has happened since jxlh_frame_begin, the call is a whole run.
 * Extra channels behave as in jxlh_frame_rerender_groups.
 * Statuses, in this order: JXLH_ERR_INVALID_ARGUMENT ctx == NULL, group_ids == NULL with count > 0;
 * JXLH_ERR_BAD_STATE outside a frame; JXLH_ERR_UNSUPPORTED a sharded context; JXLH_ERR_BAD_STATE a VarDCT frame
 * without its dequantisation tables; JXLH_ERR_INVALID_ARGUMENT an id beyond the grid; count == 0 is JXLH_OK with
 * nothing enqueued.  A refused call enqueues nothing and changes no state.
 * Out of scope: band runs and sharded runs of upsampled frames (jxlh_frame_run keeps JXLH_ERR_UNSUPPORTED there: they
 * need rows no earlier run has produced); repaint on sharded contexts; any change to what jxlh_frame_rerender_groups,
 * jxlh_changed_rects or jxlh_frame_run return; chroma-subsampled frames repainted by band (they keep the whole run);
 * rect-granular rather than row-granular upsampling (the filters rewrite whole rows already). */
jxlh_status jxlh_frame_repaint_groups(jxlh_ctx* ctx, const uint32_t* group_ids, uint32_t count);

/* Pure host code: no context, no device, any thread.  The rectangles of the frame's RESULT (upsampled size) outside
 * which jxlh_frame_repaint_groups(group_ids, count) leaves every pixel bit-identical; the cap protocol and the argument
 * checks of jxlh_changed_rects (a factor that is not 0, 1, 2, 4 or 8 is JXLH_ERR_INVALID_ARGUMENT as well).
 * A VarDCT frame with upsampling <= 1: exactly jxlh_changed_rects' list.  Otherwise every listed cell, clipped to the
 * frame, is widened by the reach of the stage list (gab, epf_iters; for a Modular frame the same stages under the
 * constant sigma) plus one pixel on a sub-sampled axis; for upsampling n > 1 by 2 more coded pixels per side (the 5 x 5
 * window), scaled by n and clipped to xsize_upsampled x ysize_upsampled (n * xsize x n * ysize where those are 0).
 * These rects are DISJOINT and cover exactly the union: cells that are horizontal neighbours give one rect, and where
 * rects of neighbouring group rows overlap the overlap is kept once.  (Held to the oracle by tests/test_repaint_cpu.py.)
 * No parameters are known for which nothing can be said: JXLH_ERR_UNSUPPORTED is never returned. */
jxlh_status jxlh_repaint_changed_rects(const jxlh_frame_params* p, const uint32_t* group_ids, uint32_t count,
                                       jxlh_rect* rects, uint32_t cap, uint32_t* n);

#ifdef __cplusplus
}
#endif
#endif /* JXL_HIP_REPAINT_H_ */
