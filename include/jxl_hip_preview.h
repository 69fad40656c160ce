/*
 * jxl_hip_preview.h -- progressive previews of a squeezed Modular image: part of the C ABI of jxl_hip.h, which
 * includes this header; including either one gives the whole interface.  The entry points live in a header of their
 * own because the set of entry points jxl_hip.h itself declares is recorded per ABI version
 * (tests/golden/lib_public_abi.json) and these were added without a new version: no existing symbol or struct changed.
 * tools/gen_py_binding.py and tools/gen_rust_binding.py read this header as they read jxl_hip.h (PREVIEW_SYMBOLS in
 * jxl_rs_amd/_abi.py, bindings/rust/jxl_hip_sys/src/preview.rs).
 */
#ifndef JXL_HIP_PREVIEW_H_
#define JXL_HIP_PREVIEW_H_

#include "jxl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A progressive preview of a WHOLE squeeze transform in one call: jxlh_unsqueeze_chain for an image whose finest
 * residual channels have not arrived.  A level is MISSING when it has residual samples and res[p] == NULL for every
 * plane p < n_planes (some but not all NULL: JXLH_ERR_INVALID_ARGUMENT; a level without residual samples is regular
 * whatever its pointers are); any pattern of missing levels is accepted, a present level behind a missing one included.
 * What level L runs is the reference's choice for whole channels (meta_apply.rs:150-161, step.rs:138-150):
 *   JXLH_PREVIEW_REGULAR    its residual is present: the regular step;
 *   JXLH_PREVIEW_SMOOTH_2D  it is missing, level L - 1 squeezes the other axis and is missing too: smooth_2d_unsqueeze
 *                           of the average level L - 1 reads (the output of level L - 2, or the base);
 *   JXLH_PREVIEW_SMOOTH_1D  it is missing otherwise: smooth_h / smooth_v_unsqueeze of its own average.
 * Levels the last level's planes do not depend on (the level in front of a 2-D one, unless something else reads it)
 * are not computed: live[L] == 0.  jxlh_squeeze_preview_kinds is that rule on the host, without a context: geometry is
 * checked as in the launch call (pointers are only tested for NULL), `kinds` and `live` (may be NULL) take n_levels
 * entries.
 * jxlh_unsqueeze_chain_preview: levels, base, out, rct_op and rct_perm as in jxlh_unsqueeze_chain; device pointers only;
 * asynchronous on the context's stream, no host round trip; the RCT is fused into the last level, smooth or regular.
 * flags: 0, or JXLH_SMOOTH_CVT_NEAREST_EVEN for the float-to-int conversion of an x86 reference build (see
 * jxlh_smooth_unsqueeze).  With no missing level the result and the launches are jxlh_unsqueeze_chain's.  Channels
 * whose residual GROUPS have partly arrived (per-tile mixtures): jxlh_unsqueeze_chain_preview_tiles, jxl_hip_preview_tiles.h. */
enum { JXLH_PREVIEW_REGULAR = 0, JXLH_PREVIEW_SMOOTH_1D = 1, JXLH_PREVIEW_SMOOTH_2D = 2 };
jxlh_status jxlh_squeeze_preview_kinds(int32_t n_planes, int32_t n_levels, const jxlh_squeeze_level* levels,
                                       uint32_t base_w, uint32_t base_h, uint8_t* kinds, uint8_t* live);
jxlh_status jxlh_unsqueeze_chain_preview(jxlh_ctx* ctx, int32_t n_planes, int32_t n_levels,
                                         const jxlh_squeeze_level* levels, const int32_t* const base[], size_t base_stride,
                                         uint32_t base_w, uint32_t base_h, int32_t* const out[], size_t out_stride,
                                         int32_t rct_op, int32_t rct_perm, uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* JXL_HIP_PREVIEW_H_ */
