/*
 * jxl_hip_extra_rects.h -- extra channels by rect: set, convert and upsample only what arrived.  Part of the C ABI of
 * jxl_hip.h, which includes this header; including either one gives the whole interface.  The declarations live in a
 * header of their own for the reason jxl_hip_save_rects.h gives: the set of entry points and structs jxl_hip.h itself
 * declares is recorded per ABI version, and these were added without a new version -- no existing symbol or struct
 * changed.  tools/gen_py_binding.py and tools/gen_rust_binding.py read this header as they read jxl_hip.h
 * (EXTRA_RECTS_SYMBOLS in jxl_rs_amd/_abi.py, bindings/rust/jxl_hip_sys/src/extra_rects.rs).
 */
#ifndef JXL_HIP_EXTRA_RECTS_H_
#define JXL_HIP_EXTRA_RECTS_H_

#include "jxl_hip.h"
#include "jxl_hip_save_rects.h" /* jxlh_rect */

#ifdef __cplusplus
extern "C" {
#endif

/* The reference decodes an extra channel's samples group by group, in the pass-group section that carries the group's
 * HF coefficients.  These calls are jxlh_frame_set_extra_channel for that arrival: a channel is declared once
 * (jxlh_frame_begin_extra_channel), its samples arrive as rects (jxlh_frame_set_extra_channel_rects), and the next
 * jxlh_frame_run or jxlh_frame_rerender_groups converts and upsamples only the tiles a rect can have changed
 * (k_ec_finish: ConvertModularToF32Stage, and for a factor above 1 Upsample<N> read straight from the i32 samples).
 * The finished channel is what the whole-plane route gives, bit for bit, in the same buffers: the read-out, the save
 * tail, jxlh_frame_blend and the patches read it unchanged.
 *
 * jxlh_frame_begin_extra_channel declares channel `ec` of w x h samples with no samples yet: every sample reads as
 * zero until a rect sets it (the plane is zero-filled on the stream), and the whole channel is converted by the next
 * run.  bits_per_sample (bits | exponent_bits << 8) and ec_upsampling as for jxlh_frame_set_extra_channel, with its
 * argument checks and statuses.  Once per channel and frame: JXLH_ERR_BAD_STATE for a channel that was begun or handed
 * over whole in this frame already.  JXLH_ERR_UNSUPPORTED also on a sharded context.
 *
 * jxlh_frame_set_extra_channel_rects writes the rects of one call into the sample planes of channels that are set: by
 * the begin above, or by a whole-plane jxlh_frame_set_extra_channel (a whole hand-over can be followed by rect
 * updates).  `samples` is one block of n_samples i32 in host or device memory; rect i is h rows of w samples, `stride`
 * samples apart, the first at samples[offset].  A host block goes up in one asynchronous copy (of the span of the block
 * the rects name) and one kernel scatters all rects; a device block is read in place -- the plane
 * jxlh_modular_local_transforms wrote, for one.  The touched channels are not rendered afterwards: the read-out, a save
 * or a blend that names one answers JXLH_ERR_BAD_STATE until the next jxlh_frame_run / jxlh_frame_rerender_groups, as
 * after a whole hand-over.  Rects of one call may overlap; which one lands last is unspecified.  A rect with w == 0 or
 * h == 0 is skipped; n == 0 is JXLH_OK with nothing enqueued.
 * The blocking form returns when the caller's block may be reused; _async returns after enqueueing, and the block
 * stays valid until the next jxlh_ctx_sync or waited mark (as for jxlh_frame_set_modular_groups_async).
 * Every refusal is decided before anything is enqueued and changes nothing; *first_bad (may be NULL) and
 * jxlh_last_error name the rect.  JXLH_ERR_INVALID_ARGUMENT: ctx == NULL; samples or rects == NULL with n > 0;
 * n > JXLH_MAX_EC_RECTS; ec >= JXLH_MAX_EXTRA_CHANNELS; stride < w; a rect that leaves its channel (x0 + w and y0 + h
 * are computed without wrapping); offset + stride * (h - 1) + w beyond n_samples (likewise).  JXLH_ERR_BAD_STATE:
 * outside a frame; a channel that is not set.  JXLH_ERR_UNSUPPORTED: a sharded context. */
typedef struct jxlh_ec_rect {
  uint32_t ec;           /* extra channel 0 .. JXLH_MAX_EXTRA_CHANNELS - 1 */
  uint32_t x0, y0, w, h; /* samples of the channel at ITS OWN resolution; w or h 0: skipped */
  uint64_t offset;       /* first sample of the rect, in samples from `samples` */
  uint32_t stride;       /* samples between the rect's rows, >= w */
} jxlh_ec_rect;
#define JXLH_MAX_EC_RECTS 4096
jxlh_status jxlh_frame_begin_extra_channel(jxlh_ctx* ctx, uint32_t ec, uint32_t w, uint32_t h, uint32_t bits_per_sample,
                                           uint32_t ec_upsampling);
jxlh_status jxlh_frame_set_extra_channel_rects(jxlh_ctx* ctx, const int32_t* samples, uint64_t n_samples,
                                               const jxlh_ec_rect* rects, uint32_t n, uint32_t* first_bad);
jxlh_status jxlh_frame_set_extra_channel_rects_async(jxlh_ctx* ctx, const int32_t* samples, uint64_t n_samples,
                                                     const jxlh_ec_rect* rects, uint32_t n, uint32_t* first_bad);

/* Pure host code: no context, no device, any thread.  Maps rects of a w x h channel with factor ec_upsampling, in
 * source samples, to the rects of the finished channel -- min(w * ec_upsampling, res_w) x min(h * ec_upsampling, res_h)
 * -- outside which every sample is bit-identical after the rects' samples changed.  Factor 1: the rect itself, cut at
 * the finished channel.  Factor > 1: the rect widened by 2 source samples on every side (the 5 x 5 window of Upsample<N>,
 * BORDER 2, mirrored), clipped to the channel, multiplied by the factor and clipped to the finished channel.  (Held
 * to the oracle by tests/test_extra_rects_cpu.py.)  One output rect per input rect, in input order; an input rect with
 * w == 0 or h == 0 gives {0, 0, 0, 0}.  *n is always the number of rects needed (n_src).
 * JXLH_ERR_INVALID_ARGUMENT: a null pointer (out may be NULL while cap == 0, src while n_src == 0); a zero size; a
 * factor not in 1, 2, 4, 8; a non-empty rect that leaves the channel; cap smaller than needed (*n is set). */
jxlh_status jxlh_extra_channel_changed_rects(uint32_t w, uint32_t h, uint32_t ec_upsampling, uint32_t res_w,
                                             uint32_t res_h, const jxlh_rect* src, uint32_t n_src, jxlh_rect* out,
                                             uint32_t cap, uint32_t* n);

#ifdef __cplusplus
}
#endif
#endif /* JXL_HIP_EXTRA_RECTS_H_ */
