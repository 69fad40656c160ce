/*
 * jxl_hip_preview_tiles.h -- progressive previews of a squeezed Modular image whose residual GROUPS have partly
 * arrived: part of the C ABI of jxl_hip.h, which includes this header; including either one gives the whole interface.
 * The entry points live in a header of their own for the reason jxl_hip_preview.h and jxl_hip_save_rects.h give: the
 * sets of entry points jxl_hip.h and jxl_hip_preview.h declare are recorded (tests/golden/lib_public_abi.json,
 * PREVIEW_SYMBOLS) and these were added without a new ABI version: no existing symbol or struct changed.
 * tools/gen_py_binding.py and tools/gen_rust_binding.py read this header as they read the others (PREVIEW_TILES_SYMBOLS
 * in jxl_rs_amd/_abi.py, bindings/rust/jxl_hip_sys/src/preview_tiles.rs).
 */
#ifndef JXL_HIP_PREVIEW_TILES_H_
#define JXL_HIP_PREVIEW_TILES_H_

#include "jxl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* jxlh_unsqueeze_chain_preview per grid cell.  The small channels of a squeezed image sit in the global section; the
 * large ones are split over the groups, which arrive one after another, so for most of a download a level is neither
 * present nor missing: some of its grid cells have their residuals and the rest do not.  The reference decides per cell
 * (SqueezeInfo::new, transforms/step.rs:123-198, from the DataStatus of the residual buffer at that grid position) and
 * so does this call.
 *
 * tiles[L] describes level L's grid; one mask serves all planes of a level (a group carries all channels):
 *   tile_w, tile_h  one cell in samples of the level's OUTPUT (0 / 0: one cell, the whole channel).  Cell (tx, ty)
 *                   covers [tx tile_w, min(out_w, (tx + 1) tile_w)) x [ty tile_h, min(out_h, (ty + 1) tile_h)).
 *   present         HOST memory, tiles_y rows of tiles_x bytes, copied by the call; non-zero: the residual samples of
 *                   that cell have arrived.  NULL: every cell follows the level's res[] pointers.
 * A cell is MISSING when the level has residual samples and its res[] are all NULL or its byte of `present` is 0 (a
 * level with res[] == NULL is wholly missing whatever `present` says; a level without residual samples is regular).
 * The res[] planes of a partly arrived level are whole planes; samples that belong to missing cells are never read.
 *
 * The kind of a cell (JXLH_PREVIEW_*) is the reference's rule moved from grid indices to positions (get_grid_idx,
 * frame/modular/mod.rs:133-148: the same group index for equal grid kinds, / 8 for a group cell over an LF-group buffer,
 * cell 0 for a whole channel -- all of them "the cell that contains the position"):
 *   REGULAR    the cell is not missing;
 *   SMOOTH_2D  it is missing, L > 0, level L - 1 squeezes the other axis, and the cell of level L - 1 that contains the
 *              cell's top-left sample mapped into L's average (x0 >> 1 for a horizontal L, y0 >> 1 for a vertical one)
 *              is missing too;
 *   SMOOTH_1D  it is missing otherwise.
 * The samples of a cell are whole-plane equivalents (the reference hands every output's borders to its neighbours
 * whatever kind produced it, step.rs:903-905):
 *   smooth   what jxlh_smooth_unsqueeze writes for the cell's rect (2-D: from the average level L - 1 reads).  A cell
 *            without one complete pair on a doubled axis (the 1-wide last cell of out_w = k tile_w + 1) is left
 *            untouched there; the reference's output buffer is freshly allocated, so the cell is ZERO.  (A rect's origin
 *            is halved on every axis the step doubles, as in jxlh_smooth_unsqueeze: a 2-D cell wants an even origin on
 *            BOTH axes, which the reference's grids -- group dimensions shifted per channel -- always give.)
 *   regular  the regular step's recurrence over the cell's pairs: `prev` is the output sample just in front of the cell
 *            on the squeezed axis, whatever kind produced it (avg[0] at the channel's start); next_avg is avg[x + 1]
 *            across the cell edge (avg[x] at the channel's end); the odd tail is copied.
 * Levels nothing depends on are not computed.
 *
 * jxlh_squeeze_tile_kinds is the rule on the host, without a context: `kinds` takes tiles_x * tiles_y entries of
 * `level`, row by row.  jxlh_unsqueeze_chain_preview_tiles: levels, base, out, rct_op, rct_perm and flags as in
 * jxlh_unsqueeze_chain_preview; device pointers only; asynchronous on the context's stream, no host round trip; launches
 * are ordered by the stream alone.  A level whose cells are of more than one kind takes at most two launches whatever
 * the number of cells (its smooth cells, then its regular runs), and the RCT behind such a last level is a launch of its
 * own.  When no level is mixed the result and the launches are jxlh_unsqueeze_chain_preview's (with no missing level:
 * jxlh_unsqueeze_chain's) -- unless a missing level's grid has a cell without a complete pair: that cell is zero, which
 * the whole-channel step is not, so such a level goes cell by cell like a mixed one.
 * Everything jxlh_unsqueeze_chain_preview checks is checked here, in its order; JXLH_ERR_INVALID_ARGUMENT also for
 * tiles == NULL, one of tile_w / tile_h zero and the other not, an odd tile_w on a horizontal level with more than one
 * cell column (an odd tile_h on a vertical one with more than one cell row: a cell starts on a pair), and more than 2^20
 * cells in a level.  All of it is decided before anything is enqueued. */
typedef struct jxlh_squeeze_tiles {
  uint32_t tile_w, tile_h;
  const uint8_t* present;
} jxlh_squeeze_tiles;

jxlh_status jxlh_squeeze_tile_kinds(int32_t n_planes, int32_t n_levels, const jxlh_squeeze_level* levels,
                                    const jxlh_squeeze_tiles* tiles, uint32_t base_w, uint32_t base_h, int32_t level,
                                    uint8_t* kinds);
jxlh_status jxlh_unsqueeze_chain_preview_tiles(jxlh_ctx* ctx, int32_t n_planes, int32_t n_levels,
                                               const jxlh_squeeze_level* levels, const jxlh_squeeze_tiles* tiles,
                                               const int32_t* const base[], size_t base_stride, uint32_t base_w,
                                               uint32_t base_h, int32_t* const out[], size_t out_stride, int32_t rct_op,
                                               int32_t rct_perm, uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* JXL_HIP_PREVIEW_TILES_H_ */
