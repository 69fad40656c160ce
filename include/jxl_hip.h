/*
 * jxl_hip.h -- C ABI of the MI355X-native JPEG XL reconstruction hot path.
 *
 * This is the drop-in boundary for libjxl/jxl-rs (v0.6.0).  jxl-rs has no FFI of
 * its own (`#![deny(unsafe_code)]`, jxl/src/lib.rs:6): the path sits behind Rust
 * traits, so each entry point below names the reference call site it replaces;
 * INTEGRATION.md shows the Rust `extern "C"` block and the
 * `HipRenderPipeline: RenderPipeline` shim that binds them.
 *
 * Conventions
 *   - every function returns jxlh_status (0 = OK, <0 = error class); nothing
 *     throws or aborts across the ABI (reference: Result<T, Error>, error.rs:15-276)
 *   - all pointers are caller-owned; a pointer argument may be a host pointer or a
 *     device (HIP) pointer -- uploads/downloads use hipMemcpyDefault
 *   - plane descriptor == RawImageBuffer / JxlOutputBuffer::new_from_ptr
 *     (jxl/src/image/internal.rs:15-31, image/output_buffer.rs:32-52)
 *   - frame-level calls are single-threaded (any ONE thread at a time, not necessarily the
 *     same one); the jxlh_submit_group* calls are re-entrant per `slot` (one HIP stream + one
 *     pinned staging slab per slot, mirroring PerThreadStorage,
 *     jxl/src/util/per_thread_storage.rs:13-60).  Every entry point makes the context's device
 *     the calling thread's current HIP device, so pool threads need no device set-up
 *   - channel order is X, Y, B everywhere (pipeline channels 0, 1, 2)
 */
#ifndef JXL_HIP_H_
#define JXL_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JXLH_ABI_VERSION 6  /* additions only since 6: round 6 added the jxlh_host_*, jxlh_slot_writer_* and
                               jxlh_ctx_wait_* / _record_event entry points; then the reference-frame slots and the
                               patch dictionary (jxlh_ctx_*_reference, jxlh_frame_save_reference,
                               jxlh_frame_set_patches, jxlh_stage_patches); frame blending and the save tail; splines
                               (jxlh_frame_set_splines, jxlh_stage_splines, jxlh_splines_build_segments) */
#define JXLH_NUM_TRANSFORMS 27   /* HfTransformType::CARDINALITY, transform_map.rs:59-61 */
#define JXLH_NUM_QUANT_TABLES 17 /* NUM_QUANT_TABLES, quantizer.rs:11 */
#define JXLH_GROUP_DIM 256       /* GROUP_DIM, jxl/src/lib.rs:24-26 */

typedef int32_t jxlh_status;
enum {
  JXLH_OK = 0,
  JXLH_ERR_INVALID_ARGUMENT = -1, /* -> Error::Gpu(InvalidArgument) */
  JXLH_ERR_OUT_OF_MEMORY = -2,    /* hipMalloc failed (reference: try_reserve, group.rs:47-55) */
  JXLH_ERR_DEVICE = -3,           /* any other HIP runtime error; see jxlh_last_error */
  JXLH_ERR_BAD_STATE = -4,        /* call order violated (e.g. submit before frame_begin) */
  JXLH_ERR_INVALID_TRANSFORM = -5,/* transform_map holds an id >= 27 (Error::InvalidVarDCTTransform) */
  JXLH_ERR_UNSUPPORTED = -6,      /* valid stream feature outside the device path (caller falls back): band or sharded
                                     runs and group re-renders of upsampled frames, frames beyond 2^31 coefficients,
                                     predictor 6 in jxlh_palette_delta (use jxlh_palette_delta_wp) */
  JXLH_ERR_INVALID_BLOCK_SIZE = -7, /* a varblock larger than 8x8 in a chroma-subsampled frame
                                      (Error::InvalidBlockSizeForChromaSubsampling, frame/modular/mod.rs:1058-1060) */
  JXLH_ERR_BLOCK_OUT_OF_BOUNDS = -8 /* a varblock crosses its group's or the frame's edge, or the first-block flags of
                                       a group cover more than its 1024 blocks (Error::HFBlockOutOfBounds,
                                       frame/modular/mod.rs:1061-1064); the offending varblocks are not reconstructed */
};

typedef struct jxlh_ctx jxlh_ctx;

/* RawImageBuffer (image/internal.rs:15-31). */
typedef struct {
  void* ptr;
  size_t bytes_per_row;
  size_t num_rows;
  size_t bytes_between_rows;
} jxlh_plane;

/* Everything the device needs that the reference keeps in FrameHeader /
 * LfGlobalState / HfGlobalState.  Field by field:
 *   xsize, ysize .......... frame_header.size_upsampled() == pipeline image size
 *                           (frame/render.rs:541-545)
 *   global_scale, quant_lf . QuantizerParams (frame/quantizer.rs:56-85)
 *   lf_quant_factors ....... LfQuantFactors::quant_factors (quantizer.rs:14-51)
 *   quant_biases ........... OpsinInverseMatrix::quant_biases (headers/transform_data.rs:30-31)
 *   x_qm_scale, b_qm_scale . FrameHeader (headers/frame_header.rs:308-315); the device computes
 *                           0.8^(scale-2) exactly like group.rs:395-396
 *   color_factor .. ytob_lf  ColorCorrelationParams (frame/color_correlation_map.rs:21-94)
 *   gab .. epf_border_sad_mul RestorationFilter (headers/frame_header.rs:146-233)
 *   do_lf_smoothing ........ FrameHeader::should_do_adaptive_lf_smoothing (:496-500)
 *   hshift, vshift ......... FrameHeader::hshift(c) / vshift(c) (headers/frame_header.rs:501-512), channel order
 *                           X/Cb, Y, B/Cr, each 0 or 1: channel c holds (size >> shift) samples (4:2:0, 4:2:2,
 *                           4:4:0 JPEG recompressions).  Such frames are limited to 8x8 transforms
 *                           (frame/modular/mod.rs:1058-1060; JXLH_ERR_INVALID_BLOCK_SIZE otherwise), their size
 *                           in blocks is rounded up to whole blocks of the coarsest channel
 *                           (FrameHeader::size_blocks, :564-569), the LF samples of a sub-sampled channel
 *                           sit in the top-left (w >> hshift) x (h >> vshift) corner of each LF group's rectangle
 *                           (frame/group.rs:485-504, modular/mod.rs:877-893) and the LF dequantisation skips
 *                           chroma-from-luma.  The setters store the whole rectangle of every channel.  What a
 *                           caller passes outside that corner is never read by the transforms; adaptive LF
 *                           smoothing (do_lf_smoothing) does read it, as the reference's does, whose LF image is
 *                           zero there (dequant_lf writes the corner only): pass zeros outside the corner to get
 *                           the reference's smoothed LF, anything at all when smoothing is off.
 *                           The transforms reconstruct every channel at its own resolution
 *                           (frame/group.rs:223-250) and the chroma upsampling stages
 *                           (render/stages/chroma_upsample.rs, frame/render.rs:569-576) run before Gaborish /
 *                           EPF, so everything downstream sees full-resolution planes.
 *   upsampling ............. FrameHeader::upsampling (1, 2, 4 or 8; 0 means 1).  xsize / ysize are then the CODED
 *                           size FrameHeader::size() = ceil(size_upsampled / upsampling) (:555-561) and
 *                           xsize_upsampled / ysize_upsampled the image size after the Upsample2x/4x/8x stages
 *                           (0 = xsize * upsampling); the stages run on the three colour channels after the
 *                           filters (frame/render.rs:655-671) and every jxlh_frame_read_* call then returns the
 *                           upsampled image.  Such a frame is run whole (JXLH_ERR_UNSUPPORTED for a band).
 *   noise, noise_lut ....... FrameHeader::has_noise() (:486-488) and Noise::lut (features/noise.rs:9-20).  The frame then
 *                           ends with the reference's noise synthesis at the result's resolution: random planes
 *                           from Xorshift128Plus seeded per 256x256 tile with (visible_frame_index,
 *                           nonvisible_frame_index, x0, y0) (frame/decode.rs:578-668), ConvolveNoiseStage on
 *                           each, AddNoiseStage with ColorCorrelationParams::y_to_x_lf / y_to_b_lf
 *                           (render/stages/noise.rs, frame/render.rs:673-683)
 *   epf_sigma_for_modular .. RestorationFilter field used when EPF runs on a Modular frame
 *                           (features/epf.rs:81-84): jxlh_modular_frame_filters; VarDCT frames ignore it
 */
typedef struct {
  uint32_t abi_version; /* JXLH_ABI_VERSION */
  uint32_t xsize, ysize;
  uint32_t global_scale, quant_lf;
  float lf_quant_factors[3];
  float quant_biases[4];
  uint32_t x_qm_scale, b_qm_scale;
  uint32_t color_factor;
  float base_correlation_x, base_correlation_b;
  int32_t ytox_lf, ytob_lf;
  uint32_t gab;
  float gab_w1[3], gab_w2[3];
  uint32_t epf_iters;
  float epf_sharp_lut[8];
  float epf_channel_scale[3];
  float epf_quant_mul, epf_pass0_sigma_scale, epf_pass2_sigma_scale, epf_border_sad_mul;
  uint32_t do_lf_smoothing;
  uint32_t flags; /* JXLH_FRAME_* */
  uint32_t hshift[3], vshift[3];
  float epf_sigma_for_modular;
  uint32_t upsampling;
  uint32_t xsize_upsampled, ysize_upsampled;
  uint32_t noise;
  float noise_lut[8];
  uint32_t visible_frame_index, nonvisible_frame_index;
} jxlh_frame_params;

enum {
  JXLH_FRAME_UNFUSED_FILTERS = 1u << 0, /* run Gaborish/EPF as one kernel per stage (debug/parity) */
  JXLH_FRAME_EXPAND_SPARSE = 1u << 1,   /* always expand sparse submissions into dense slabs before the
                                           transforms instead of letting them read the pairs (debug/parity) */
  JXLH_FRAME_STRIP = 1u << 2,           /* whole-frame runs go through the single strip kernel (dequantisation, IDCT and
                                           the filter stages in one persistent launch, no intermediate planes in HBM:
                                           2.35 GB of traffic per 8K frame instead of 3.58) instead of transforms ->
                                           planes -> fused filters.  Bit-identical output; slower on MI355X today
                                           (both forms are bound by instruction issue), hence
                                           opt-in */
  JXLH_FRAME_DENSE_DEQUANT = 1u << 3,   /* a frame resident in the slot-bucketed form (jxlh_submit_groups_slots): the
                                           transforms always dequantise every coefficient position instead of only the
                                           positions that have an entry (debug/parity: both give the same bits) */
  JXLH_FRAME_MODULAR = 1u << 4,         /* a Modular frame (lossless, lossy Modular): xsize x ysize coded samples handed
                                           over with jxlh_frame_set_modular_channels instead of LF, HF metadata and
                                           coefficients; see "Modular frames" below */
};

/* Header defaults of the reference (RestorationFilter / ColorCorrelationParams /
 * quant_biases defaults), for callers that only override a few fields. */
jxlh_status jxlh_default_frame_params(jxlh_frame_params* p, uint32_t xsize, uint32_t ysize);

/* ---------------------------------------------------------------- context */
/* n_slots = number of host threads that will call jxlh_submit_group concurrently
 * (the JxlParallelRunner's thread count, jxl/src/api/mod.rs:77-81). */
jxlh_status jxlh_ctx_create(int32_t device_ordinal, int32_t n_slots, jxlh_ctx** out);
void jxlh_ctx_destroy(jxlh_ctx* ctx);
const char* jxlh_status_string(jxlh_status s);
/* human-readable detail of the last JXLH_ERR_DEVICE on this context (thread-unsafe, debugging) */
const char* jxlh_last_error(const jxlh_ctx* ctx);
/* pinned host memory for coefficient slabs (replaces VarDctBuffers::coeffs_storage,
 * frame/group.rs:27-67) */
jxlh_status jxlh_alloc_pinned(jxlh_ctx* ctx, size_t bytes, void** out);
jxlh_status jxlh_free_pinned(jxlh_ctx* ctx, void* p);

/* ---------------------------------------------------------------- VarDCT frame */
/* Replaces Frame::from_header_and_toc's LF / HfMetadata allocation
 * (frame/decode.rs:172-204) + prepare_render_pipeline (frame/render.rs:907).
 * SIZES.  xsize and ysize may each be up to 2^20 (JXLH_ERR_INVALID_ARGUMENT beyond), subject to two totals
 * (JXLH_ERR_UNSUPPORTED beyond): fewer than 2^30 samples in one plane -- whole 8x8 blocks, rows rounded up to 64
 * samples -- and fewer than 2^31 coefficients (3 * 65536 per 256x256 group).  Inside these bounds every entry point
 * serves either axis at its full length, and so do the stage and Modular entry points, whose w and h are bounded by
 * 2^20 where they are bounded at all: a frame 8 pixels wide and 65 544 tall is as good as a square one.  Several
 * kernels take one image row (or 2 to 8) per workgroup row, so such a frame launches grids of more than 65 535
 * workgroup rows; gfx950 runs them, and tests/test_gpu_long_axis.py holds frames and planes of more than 65 536 rows
 * or columns to the oracle through every one of these launches.  No combination of sizes may surface as a HIP launch
 * error: one that cannot be served is declined by the argument checks, before anything is launched. */
jxlh_status jxlh_frame_begin(jxlh_ctx* ctx, const jxlh_frame_params* p);

/* CustomTransformData::weights2 / weights4 / weights8 (headers/transform_data.rs:337-344): 15 / 55 / 210 weights
 * of the 2x / 4x / 8x upsampling kernels; NULL selects the codestream defaults (DEFAULT_KERN_*, :34-333).
 * Per decoder like the reference's file header: persists across frames; callable outside a frame. */
jxlh_status jxlh_set_upsampling_weights(jxlh_ctx* ctx, const float* weights2, const float* weights4,
                                        const float* weights8);

/* ---------------------------------------------------------------- Modular frames
 * jxlh_frame_begin with JXLH_FRAME_MODULAR starts a Modular frame: the reference's render list for such a frame
 * (frame/render.rs:553-903) opens with ConvertModularToF32Stage x3 or ConvertModularXYBToF32Stage (:554-563), reads a
 * CONSTANT EPF sigma (features/epf.rs:81-84: INV_SIGMA_NUM / epf_sigma_for_modular) and is otherwise the VarDCT list.
 * upsampling, hshift / vshift, noise*, the restoration-filter fields and lf_quant_factors mean what they mean for a VarDCT
 * frame; JXLH_FRAME_STRIP, _EXPAND_SPARSE and _DENSE_DEQUANT are ignored.  The frame allocates no coefficient buffer, LF
 * planes, HF-meta maps or work list (its i32 sample planes take the coefficient buffer's place, 12 B/px); the limit of
 * 2^31 coefficients does not apply, the limit of 2^30 samples per plane does.  No dequant tables are needed.
 * JXLH_ERR_INVALID_ARGUMENT: epf_iters > 0 with epf_sigma_for_modular <= 0; JXLH_ERR_UNSUPPORTED: a sharded context.
 *
 * jxlh_frame_set_modular_channels hands over the three colour channels of a rect as the inverse transforms left them
 * (the Modular counterpart of jxlh_frame_set_lf): host or device memory, row stride `stride` >= w samples; per rect, in
 * any order, and again after a run to replace a rect.  The context keeps the samples (rows never set read as zero
 * samples), not the caller's pointers: the call returns when the copies have landed.
 *   sample_format  bits | exponent_bits << 8 as for the extra channels: integer samples give v * (1 / (2^bits - 1)),
 *                  float samples are widened exactly (convert.rs:416-533).  | JXLH_MODULAR_XYB selects
 *                  ConvertModularXYBToF32Stage (convert.rs:316-342): c0, c1, c2 are the coded order Y, X, B and
 *                  X = x * s[0], Y = y * s[1], B = ((float)b + (float)y) * s[2] with s = lf_quant_factors (the bit depth
 *                  is not read then; the frame must not be chroma-subsampled).  The same on every rect of a frame.
 *   grey frames    pass one pointer three times (the reference fans channel 0 out to pipeline channels 0..2,
 *                  modular/transforms/meta_apply.rs:697-701).
 *   sub-sampling   x0, y0, w, h are full-resolution coordinates, x0 and y0 multiples of the coarsest shift; channel c
 *                  supplies the ceil(w / 2^hshift[c]) x ceil(h / 2^vshift[c]) samples at (x0 >> hshift[c], y0 >> vshift[c]).
 * JXLH_ERR_INVALID_ARGUMENT: a null pointer, stride < w, a rect that leaves the coded size, a bad or changed format, a
 * misaligned sub-sampled origin; JXLH_ERR_BAD_STATE: outside a frame or on a VarDCT frame.  A refused call changes nothing.
 *
 * jxlh_frame_run on a Modular frame: group rows are 256-row bands whatever the codestream's group size.  The run takes in
 * the band's rows plus the filters' halo (k_modular_intake), upsamples sub-sampled channels, runs Gaborish / EPF and the
 * post stages exactly as for a VarDCT frame.  A band run whose halo would overwrite a neighbouring band's finished rows
 * (a stage list that ends in the planes the intake writes; any filtered chroma-subsampled frame, whose sub-sampled
 * channels are taken into the other set of planes) renders the whole frame instead.  jxlh_frame_rerender_groups
 * returns JXLH_ERR_UNSUPPORTED: a progressive Modular decode sets the changed rects and runs again.  The VarDCT-only calls
 * (jxlh_frame_set_lf*, jxlh_frame_set_hf_meta, jxlh_submit_group*, jxlh_frame_coeff_buffer, jxlh_frame_read_lf) return
 * JXLH_ERR_BAD_STATE with nothing launched.  Patches, splines, extra channels, read-outs, jxlh_frame_blend, jxlh_frame_save,
 * jxlh_frame_save_reference and jxlh_frame_save_lf serve the frame as they serve a VarDCT one. */
#define JXLH_MODULAR_XYB (1u << 16)
jxlh_status jxlh_frame_set_modular_channels(jxlh_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                            const int32_t* c0, const int32_t* c1, const int32_t* c2, size_t stride,
                                            uint32_t sample_format);

/* ---- group-local Modular transforms (frame/modular/transforms/apply_local.rs) ---------------------------------------
 * A lossless encoder picks an RCT per group and very often a per-group palette.  These calls take the channels of many
 * groups AS DECODED (before meta_apply_local_transforms' steps have run) plus each group's transform list, run every
 * group's inverse steps on the device and write the finished channels at the group's rect -- the whole batch in ONE
 * kernel launch (k_modular_local).  (Palettes with delta entries or a predictor: the _general calls of
 * jxl_hip_local_palette.h.)
 *
 *   arena    one block of i32 samples, host or device memory, that holds every group's coded channels and palettes;
 *            descriptors address it by sample offsets.
 *   group    the rect it covers, the image channels its steps see (n_channels), its steps in BITSTREAM order (the
 *            headers::modular::Transform entries of its GroupHeader) and where its coded channels sit.  The device
 *            applies the inverses last-to-first (TransformStep::local_apply).
 *   RCT      do_rct_step on channels begin_c .. begin_c + 2: wrapping i32, op = rct_type % 7, permutation = rct_type / 7.
 *   palette  the num_deltas == 0, predictor == Zero branch of do_palette_step_general (palette.rs:182-199): explicit
 *            entries, the implicit 4x4x4 and 5x5x5 cubes behind them, negative indices from the delta table scaled by
 *            the bit depth (taken as min(bit_depth, 24), palette.rs:177), channels >= 3 of implicit entries zero.
 *   begin_c  indexes the channel list AS IT STANDS when meta_apply_single_transform reaches the step: every palette in
 *            front of it has put its meta channel at position 0 and folded its num_c channels into one index channel.
 *   n_coded  the image-sized channels the list holds after all steps (palette meta channels not counted: their
 *            samples are at palette_offset), coded_offset[i] the i-th of them in list order, rows of w samples at
 *            coded_stride.
 * Rects of one call that overlap are not diagnosed; the order in which they land is unspecified.
 *
 * Every refusal is decided before anything is enqueued; a refused call changes nothing, *first_bad (may be null) and
 * jxlh_last_error name the group.
 *   JXLH_ERR_INVALID_ARGUMENT  a null pointer; n_channels, n_coded outside 1..4, n_steps above 4; an n_coded that is
 *                              not what the steps leave; rct_type >= 42; a channel range that leaves the list (the
 *                              reference's InvalidChannelRange); num_c == 0; coded_stride < w; an offset + extent beyond
 *                              arena_samples; num_colors + num_deltas == 0; a palette with a bit_depth outside 1..31;
 *                              a rect outside the frame / the out planes; a bad or changed sample_format.
 *   JXLH_ERR_UNSUPPORTED       (keep that group on the host and hand it over with jxlh_frame_set_modular_channels) a
 *                              palette with num_deltas > 0 or predictor != 0; a step whose range touches a palette meta
 *                              channel; any other transform kind (local squeeze: jxl_hip_local_squeeze.h); a chroma-subsampled frame; a sharded
 *                              context.
 *   JXLH_ERR_BAD_STATE         jxlh_frame_set_modular_groups* outside a frame or on a VarDCT frame. */
#define JXLH_LOCAL_MAX_STEPS 4
#define JXLH_LOCAL_MAX_CHANNELS 4
enum { JXLH_LOCAL_RCT = 0, JXLH_LOCAL_PALETTE = 1 };
typedef struct jxlh_local_step {
  uint32_t kind;        /* JXLH_LOCAL_* */
  uint32_t begin_c;     /* Transform::begin_channel */
  uint32_t rct_type;    /* RCT: 0..41 */
  uint32_t num_c, num_colors, num_deltas, predictor; /* palette */
  uint64_t palette_offset; /* palette: samples into the arena; num_c rows of num_colors + num_deltas values (the meta
                              channel's layout, size (num_colors + num_deltas, num_c)) */
} jxlh_local_step;
typedef struct jxlh_local_group {
  uint32_t x0, y0, w, h;      /* the rect of the frame (or of the out planes) this group covers; w or h 0: skipped */
  uint32_t n_channels;        /* image channels the steps see, 1..JXLH_LOCAL_MAX_CHANNELS */
  uint32_t n_steps;           /* 0..JXLH_LOCAL_MAX_STEPS; 0 = plain copy */
  jxlh_local_step steps[4];   /* [JXLH_LOCAL_MAX_STEPS] */
  uint32_t n_coded;
  uint64_t coded_offset[4];   /* [JXLH_LOCAL_MAX_CHANNELS] samples into the arena */
  uint32_t coded_stride;      /* >= w */
} jxlh_local_group;
/* What a group's list lowers to: the kernel keeps channel s of the finished group in SLOT s (a register per sample);
 * coded channel i is loaded into coded_slot[i], then ops[0 .. n_ops) run -- the inverse steps, last step first. */
typedef struct jxlh_local_op {
  uint32_t kind;         /* JXLH_LOCAL_* */
  uint32_t rct_op;       /* RCT: 0..6 */
  uint32_t n_slots;      /* RCT: 3; palette: num_c */
  uint32_t in_slot[3];   /* RCT: the slots read as v0, v1, v2; palette: in_slot[0] holds the index */
  uint32_t out_slot[4];  /* RCT: the slots w0, w1, w2 go to (permutation applied); palette: the slot of channel c */
  uint32_t num_colors;
  uint64_t palette_offset;
} jxlh_local_op;
typedef struct jxlh_local_program {
  uint32_t n_coded;
  uint32_t coded_slot[4];
  uint32_t n_ops;
  jxlh_local_op ops[4];
} jxlh_local_program;
/* Pure host code (no context, no device): mirrors meta_apply_single_transform on each group's channel list and checks
 * everything listed above that does not need a frame.  bit_depth: the channels' (0 allowed without palettes).
 * programs: n entries, or null for the checks alone.  The launches below lower through the same function. */
jxlh_status jxlh_modular_local_lower(const jxlh_local_group* groups, size_t n, uint32_t bit_depth, uint64_t arena_samples,
                                     jxlh_local_program* programs, size_t* first_bad);
/* The stage-level form: group g's n_channels finished channels go to out[0 .. n_channels) at (x0, y0); out: n_out
 * (1..4, >= every n_channels) DEVICE planes of out_w x out_h samples, rows out_stride apart.  What a frame with a global
 * transform behind the local ones feeds into jxlh_rct / jxlh_unsqueeze_chain, and how a fourth channel reaches
 * jxlh_frame_set_extra_channel without leaving the device.  Returns when the result is in `out`. */
jxlh_status jxlh_modular_local_transforms(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                          const jxlh_local_group* groups, size_t n, uint32_t bit_depth, int32_t* const out[],
                                          uint32_t n_out, uint32_t out_w, uint32_t out_h, size_t out_stride,
                                          size_t* first_bad);
/* The same launch into the frame's sample planes; the rules of jxlh_frame_set_modular_channels apply (rects inside the
 * coded size, one sample_format per frame, replaceable after a run, freely mixed with jxlh_frame_set_modular_channels on
 * other rects).  The palettes' bit depth is sample_format's.  n_channels is 3, or 1 for a grey frame, whose channel is
 * fanned out to all three planes (meta_apply.rs:697-701).  A host arena goes up in one asynchronous copy into context
 * scratch.  jxlh_frame_set_modular_groups returns when the caller's arena may be reused; the _async form returns after
 * enqueueing, and the arena stays valid until the next jxlh_ctx_sync / waited mark (as for jxlh_frame_save_async). */
jxlh_status jxlh_frame_set_modular_groups(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                          const jxlh_local_group* groups, size_t n, uint32_t sample_format,
                                          size_t* first_bad);
jxlh_status jxlh_frame_set_modular_groups_async(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                const jxlh_local_group* groups, size_t n, uint32_t sample_format,
                                                size_t* first_bad);

/* HfGlobalState::dequant_matrices (frame/quant_weights.rs:347-351): 17 tables, table t holds
 * 3 * n[t] inverse weights, channel-major (matrix(type, c), :1081-1086). */
jxlh_status jxlh_frame_set_dequant_tables(jxlh_ctx* ctx, const float* const tables[JXLH_NUM_QUANT_TABLES],
                                          const size_t n[JXLH_NUM_QUANT_TABLES]);

/* decode_vardct_lf -> dequant_lf (frame/modular/mod.rs:837-929), one LF-group rect at a time.
 * Rect in blocks, anywhere inside the frame (any origin, any size, zero-sized included; rects may arrive in
 * any order, between the other setters and the submissions, and a later call replaces an earlier one's samples,
 * also after a jxlh_frame_run: the next render smooths again from the stored LF).  qy/qx/qb are the three
 * modular channels in coded order (Y, X, B), host or device memory, row stride `stride` >= w samples; what lies
 * between w and stride is not read.  extra_precision (0..3) is the LF group's: the rect is dequantised with
 * (factor * inv_quant_lf) * (1 / (1 << extra_precision)).  Runs K0a on the device.
 * JXLH_ERR_INVALID_ARGUMENT: a null plane, stride < w, extra_precision > 3, a rect that leaves the frame;
 * JXLH_ERR_BAD_STATE outside a frame.  A refused call changes nothing.
 * Sub-sampled frames: see hshift / vshift above for what the samples outside each LF group's corner mean. */
jxlh_status jxlh_frame_set_lf_quantized(jxlh_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                        const int32_t* qy, const int32_t* qx, const int32_t* qb,
                                        size_t stride, uint32_t extra_precision);
/* Alternative: LF already dequantised by the host (lf_image, frame/mod.rs), channels X, Y, B; rects, strides,
 * ordering and errors as above.  Both setters may be mixed rect by rect inside one frame. */
jxlh_status jxlh_frame_set_lf(jxlh_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                              const float* x, const float* y, const float* b, size_t stride);

/* decode_hf_metadata (frame/modular/mod.rs:984-1081): HfMetadata maps for a rect in blocks
 * (frame/mod.rs:169-176).  ytox/ytob cover ceil(w/8) x ceil(h/8) colour tiles starting at
 * (x0/8, y0/8); x0, y0 must be multiples of 8, w and h need not be: a rect that ends inside a colour tile
 * sets that whole tile, so a neighbouring rect that delivers the tile again must carry the same value.
 * transform_map, raw_quant and epf_map share the row stride map_stride >= w (in elements of each map), ytox and
 * ytob cmap_stride >= ceil(w/8); host or device memory.  Which transform families the frame holds (and whether
 * the strip kernel may take every tile) is gathered over all rects of the frame from the host-resident maps; a
 * map in device memory is not inspected and every family is assumed present.  Any order, any number of calls.
 * JXLH_ERR_INVALID_ARGUMENT: a null map, map_stride < w, cmap_stride < ceil(w/8), x0 or y0 off the 8-block grid,
 * a rect that leaves the frame; JXLH_ERR_BAD_STATE outside a frame.  A refused call changes nothing. */
jxlh_status jxlh_frame_set_hf_meta(jxlh_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                   const uint8_t* transform_map, const int32_t* raw_quant,
                                   const uint8_t* epf_map, size_t map_stride, const int8_t* ytox,
                                   const int8_t* ytob, size_t cmap_stride);

/* Replaces the `if let Some(pixels)` branch of decode_vardct_group (frame/group.rs:579-611)
 * + pipeline.set_buffer_for_group for channels 0..2 (frame/decode.rs:776-784).
 * coeffs: 3 * 65536 i32 (X, Y, B planes of the group, varblocks back to back in raster order
 * of their top-left block, group.rs:437-440, :612).  Asynchronous: returns after enqueueing the
 * H2D copy on slot's stream; the slab may be reused after jxlh_slot_wait(slot). */
jxlh_status jxlh_submit_group(jxlh_ctx* ctx, int32_t slot, uint32_t group_id, const int32_t* coeffs,
                              uint32_t flags);
/* Flags of the submit calls.
 *   JXLH_GROUP_COMPLETE    set_buffer_for_group's `complete` (render/mod.rs:128-137): this is the last time the group
 *                          is submitted.  Without it the submission is a progressive pass: the frame can be rendered
 *                          with what has arrived (jxlh_frame_run), and groups that receive further passes later are
 *                          brought up to date with jxlh_frame_rerender_groups.
 *   JXLH_GROUP_ACCUMULATE  sparse forms only: the pairs are ADDED to the group's coefficients of the earlier passes
 *                          on the device (frame/group.rs:572 `+=` on Frame::hf_coefficients, frame/decode.rs:547-558)
 *                          instead of replacing them.  A dense slab always replaces the group's coefficients, so a
 *                          progressive caller that keeps dense slabs submits its accumulated slab.
 *   JXLH_GROUP_ENTRIES12   jxlh_submit_groups_slots only: the entries are 12 bits -- (position & 63) | (value & 63) << 6,
 *                          value in [-32, 31] -- packed two per three bytes (byte 0 = e0 & 255, byte 1 = e0 >> 8 |
 *                          (e1 & 15) << 4, byte 2 = e1 >> 4); every (group, channel) run holds an even number of them
 *                          (an odd run is closed with a zero update, counted in its last slot), so each run starts on
 *                          a byte.  1.5 bytes per update on the bus. */
enum { JXLH_GROUP_COMPLETE = 1u << 0, JXLH_GROUP_ACCUMULATE = 1u << 1, JXLH_GROUP_ENTRIES12 = 1u << 2 };

/* Sparse form of jxlh_submit_group (the dense i32 slab is ~90 % zeros at d1 and
 * its PCIe transfer bounds end-to-end decode).  The entropy loop of decode_vardct_group
 * (frame/group.rs:560-575: `coeffs[c][offset + order[k]] += v`) emits one pair per non-zero
 * coefficient instead of writing a dense slab:
 *   pairs   n[0] pairs of channel X, then n[1] of Y, then n[2] of B, contiguous; pos = index inside
 *           the channel's 65536-entry slab (the same index space as the dense form)
 *   wide    values that do not fit i16 (the reference stores i32), pos = channel * 65536 + index
 * Duplicate positions accumulate with wrapping i32 adds (multi-pass accumulation: put all passes'
 * updates of a group in ONE list -- a group may be submitted sparse once between two jxlh_frame_run
 * calls, JXLH_ERR_BAD_STATE otherwise).  When every group of the frame arrives this way the transforms
 * read the pairs directly (bucketed per varblock on the device); otherwise the device zero-fills the
 * groups' slabs and scatters the pairs.  Results are identical to the dense path bit for bit.  Asynchronous like jxlh_submit_group (H2D on the slot's stream;
 * pinned host memory from jxlh_alloc_pinned overlaps with compute). */
typedef struct jxlh_coeff16 {
  uint16_t pos;
  int16_t val;
} jxlh_coeff16;
typedef struct jxlh_coeff32 {
  uint32_t pos;
  int32_t val;
} jxlh_coeff32;
jxlh_status jxlh_submit_group_sparse(jxlh_ctx* ctx, int32_t slot, uint32_t group_id, const jxlh_coeff16* pairs,
                                     const uint32_t n[3], const jxlh_coeff32* wide, uint32_t n_wide,
                                     uint32_t flags);
/* The same for `count` groups decoded by one host thread: one H2D copy for all of them.
 * pairs holds the groups' pair runs back to back in the order of group_ids; n is count x 3;
 * wide positions carry the group: pos = (group_id * 3 + channel) * 65536 + index. */
jxlh_status jxlh_submit_groups_sparse(jxlh_ctx* ctx, int32_t slot, uint32_t count, const uint32_t* group_ids,
                                      const jxlh_coeff16* pairs, const uint32_t* n, const jxlh_coeff32* wide,
                                      uint32_t n_wide, uint32_t flags);
/* The same with 3 bytes per update on the bus: positions (u16) and values (i8) as two arrays in the order of the
 * pairs above; updates whose value does not fit 8 bits go to `wide` like those that do not fit 16 above.  At d1 nearly
 * every coefficient fits, and the host-to-device copy is what bounds the decode-to-device rate. */
jxlh_status jxlh_submit_groups_sparse8(jxlh_ctx* ctx, int32_t slot, uint32_t count, const uint32_t* group_ids,
                                       const uint16_t* pos, const int8_t* val, const uint32_t* n,
                                       const jxlh_coeff32* wide, uint32_t n_wide, uint32_t flags);
/* The same with 2 bytes per update on the bus (round 4): a channel's 65536 coefficient positions are cut into 16
 * SEGMENTS of 4096; an update is one u16 = (position inside its segment) | (value & 15) << 12 with the value in
 * [-8, 7] (two's complement nibble), and seg_counts[(i * 3 + c) * 16 + s] says how many entries group i, channel c,
 * segment s has; `entries` holds them in that order (group, channel, segment), any order inside a segment.  What a
 * decoder does at `coeffs[idx] += coeff` (frame/group.rs:572): append (idx & 4095) | coeff << 12 to the bucket of
 * idx >> 12.  Updates whose value does not fit the nibble go to the 3-byte overflow arrays pos8 / val8 (positions
 * inside the channel slab as in jxlh_submit_groups_sparse8; n8 is count x 3, may be NULL when there is none), values
 * beyond 8 bits to `wide`.  Every update is an addition into the group's slab, so the split changes nothing. */
jxlh_status jxlh_submit_groups_sparse4(jxlh_ctx* ctx, int32_t slot, uint32_t count, const uint32_t* group_ids,
                                       const uint16_t* entries, const uint16_t* seg_counts, const uint16_t* pos8,
                                       const int8_t* val8, const uint32_t* n8, const jxlh_coeff32* wide,
                                       uint32_t n_wide, uint32_t flags);
/* Slot-bucketed form: 2 bytes per update, read by the transforms IN PLACE (round 5: no device-side sort, no unpacking
 * pass, no slot tables).  A channel's 65536 positions are 1024 SLOTS of 64 coefficients (the unit varblock coefficient
 * offsets are counted in, frame/group.rs:612: an 8x8 block is one slot, a 16x16 varblock four); an update is one u16 =
 * (position & 63) | (value & 1023) << 6 with the value in [-512, 511]; slot_counts[(i * 3 + c) * 1024 + s] (u8) says how
 * many updates group i, channel c, slot s has and `entries` holds them in that order, any order inside a slot;
 * n[3 * i + c] = the channel's total.  A decoder appends to the slot buckets of the varblock it is decoding and flushes
 * them when the varblock ends (frame/group.rs:557-575).  Positions may repeat (several passes' updates in one list): they
 * add up as integers before the dequantisation, like `coeffs[i] += v`.  A slot-count table that disagrees with n stays
 * inside its run: counts beyond n are cut at the run's end, entries the table does not cover are ignored.
 *   When EVERY group of the frame arrives in this form (and nothing is added to earlier passes), jxlh_frame_run reads the
 * upload as it is: the transforms dequantise only the positions that have an entry (everything else is the +0.0f the
 * reference computes for a zero coefficient; varblocks with far more entries than d1 content has, or raw_quant == 0, take
 * a dense dequantisation pass -- same bits, see JXLH_FRAME_DENSE_DEQUANT).  The uploads land in a second set of buffers:
 * the call may be issued for the NEXT frame while the previous jxlh_frame_run is still executing and waits for nothing
 * of it (jxlh_ctx_mark / jxlh_ctx_wait_mark is the host loop for that).  Groups of the epoch that are NOT self-contained
 * slot-bucketed submissions -- another form (dense slab, plain pairs), a value in `wide`, JXLH_GROUP_ACCUMULATE -- are
 * brought into their dense slabs on the device and read from there, group by group, while the rest of the frame is still
 * read in place (round 6; as long as every group arrived in the epoch and at least half of them in place -- otherwise
 * the whole frame takes the general route: sort, or zero-fill + scatter into dense slabs).  Values beyond 10 bits
 * need not go to `wide`: see "WIDE VALUES" below.
 *   JXLH_ERR_INVALID_ARGUMENT is returned before anything is reserved (a rejected call leaves the epoch as it was). */
jxlh_status jxlh_submit_groups_slots(jxlh_ctx* ctx, int32_t slot, uint32_t count, const uint32_t* group_ids,
                                     const uint16_t* entries, const uint8_t* slot_counts, const uint32_t* n,
                                     const jxlh_coeff32* wide, uint32_t n_wide, uint32_t flags);
/* ---- host side of the slot-bucketed form (round 6): plain CPU code, no context, no device, any thread ----
 * WIDE VALUES.  An entry holds 10 bits (6 with JXLH_GROUP_ENTRIES12); the reference accumulates arbitrary i32
 * (`coeff = read_signed_inline(..) << shift; current_coeffs[idx] += coeff`, frame/group.rs:568-572).  A producer SPLITS a
 * value outside the range into repeated in-range entries at the same position -- 2000 = 511 + 511 + 511 + 467 -- which
 * add up as integers on the device before the dequantisation, exactly like several passes' updates of one coefficient:
 * the frame stays in the form the transforms read in place (varblocks with more entries than their lanes hold take a
 * dense dequantisation pass, same bits).  Only what no slot can hold (a slot's count is a u8: 255 entries) goes to
 * `wide`, and a group with a `wide` value -- like a group that arrives in another form, or adds a pass to earlier
 * content (JXLH_GROUP_ACCUMULATE) -- is read from its dense slab while every other group of the frame is still read in
 * place (per-group routing; round 5 took the whole frame out of the in-place form).  Both helpers below do the split.
 *
 * jxlh_host_pack_slots: one group's dense slab (3 x 65536 i32: VarDctBuffers::coeffs_storage, frame/group.rs:27-67,
 * :437-440) -> the arguments of jxlh_submit_groups_slots for that group.  entries: room for entries_capacity entries
 * (u16 each; with JXLH_GROUP_ENTRIES12 the three runs are written as bytes, 1.5 per entry, each closed to an even
 * count); slot_counts: 3 x 1024; n[3]: entries per channel; wide / n_wide: values that could not be split (positions
 * already carry group_id as the batched call wants them).  JXLH_ERR_INVALID_ARGUMENT when a capacity is too small. */
jxlh_status jxlh_host_pack_slots(const int32_t* coeffs, uint32_t group_id, uint32_t flags, void* entries,
                                 size_t entries_capacity, uint8_t* slot_counts, uint32_t n[3], jxlh_coeff32* wide,
                                 uint32_t wide_capacity, uint32_t* n_wide);
/* A batch of groups in one call: exactly the arrays of ONE jxlh_submit_groups_slots call for them -- group_coeffs[g] is
 * group group_ids[g]'s dense slab (the reference keeps one Vec per group: Frame::hf_coefficients, frame/mod.rs), entries
 * / slot_counts (n_groups x 3 x 1024) / n (n_groups x 3) are written group after group, *entries_used = entries written
 * (nullable).  What a decoder thread calls for its share of a frame (bench.py: host_pack_ms_per_frame times this). */
jxlh_status jxlh_host_pack_slots_many(const int32_t* const* group_coeffs, const uint32_t* group_ids, uint32_t n_groups,
                                      uint32_t flags, void* entries, size_t entries_capacity, uint8_t* slot_counts,
                                      uint32_t* n, jxlh_coeff32* wide, uint32_t wide_capacity, uint32_t* n_wide,
                                      size_t* entries_used);
/* The same form written by the entropy loop itself (frame/group.rs:557-575), one writer per decoding thread:
 *   begin_group(buffers)                                 once per group (zeroes slot_counts)
 *   begin_varblock(first_slot, num_slots)                coeffs_offset / 64 and cx * cy of the varblock (group.rs:612);
 *                                                        varblocks in the order they are decoded (ascending offsets)
 *   add(channel, pos, value)                             `coeffs[channel][coeffs_offset + pos] += value`, pos inside the
 *                                                        varblock (order[k]); channels and positions in any order
 *   end_group(n, n_wide)                                 closes the last varblock, writes the three runs to `entries`
 * Entries of a one-slot varblock (8x8: the common case) are appended as they arrive; a larger varblock's are
 * bucketed by slot when it ends. */
typedef struct jxlh_slot_writer jxlh_slot_writer;
jxlh_status jxlh_slot_writer_create(jxlh_slot_writer** out);
void jxlh_slot_writer_destroy(jxlh_slot_writer* w);
jxlh_status jxlh_slot_writer_begin_group(jxlh_slot_writer* w, uint32_t group_id, uint32_t flags, void* entries,
                                         size_t entries_capacity, uint8_t* slot_counts, jxlh_coeff32* wide,
                                         uint32_t wide_capacity);
jxlh_status jxlh_slot_writer_begin_varblock(jxlh_slot_writer* w, uint32_t first_slot, uint32_t num_slots);
jxlh_status jxlh_slot_writer_add(jxlh_slot_writer* w, uint32_t channel, uint32_t pos, int32_t value);
jxlh_status jxlh_slot_writer_add_many(jxlh_slot_writer* w, uint32_t channel, const uint32_t* pos, const int32_t* value,
                                      size_t count);
jxlh_status jxlh_slot_writer_end_group(jxlh_slot_writer* w, uint32_t n[3], uint32_t* n_wide);

/* Blocks until the host buffers of the submissions made on `slot` so far may be reused (their host-to-device copies have
 * landed).  Device-side work a submission queues behind its copies on the slot's stream (the unpack pass of
 * JXLH_GROUP_ENTRIES12) is NOT waited for here: jxlh_frame_run orders itself behind it. */
jxlh_status jxlh_slot_wait(jxlh_ctx* ctx, int32_t slot);
/* Orders uploads ACROSS contexts on the device: whatever is submitted on (ctx, slot) after this call starts when the
 * uploads enqueued so far on (after_ctx, after_slot) have landed -- the device-side form of "jxlh_slot_wait(after_ctx,
 * after_slot), then submit", without blocking the host.  Two contexts that stream frames keep the bus busy back to back
 * and stay in anti-phase (one uploads while the other computes) whatever the host's latency is (round 5,
 * profiles/r05_f_e2e_host_loops.txt).  Both contexts must live on the same device. */
jxlh_status jxlh_slot_after(jxlh_ctx* ctx, int32_t slot, jxlh_ctx* after_ctx, int32_t after_slot);

/* Device-resident coefficient store of the current frame (ngroups * 3 * 65536 i32), for callers
 * that already hold coefficients in HBM (bench harness, multi-GPU shards). */
jxlh_status jxlh_frame_coeff_buffer(jxlh_ctx* ctx, int32_t** device_ptr, size_t* n_int32);

/* Runs everything that has not run yet for the frame on the context's main stream:
 * K0b adaptive LF smoothing (Frame::finalize_lf, frame/mod.rs:360-378), K3sigma
 * (SigmaSource::new, features/epf.rs:35-87), K1 for every submitted group, then the stage list
 * of frame/render.rs:569-622 (Gaborish x3, EPF0/1/2).  group range [g0, g1) restricts K1 and the
 * filters to a band of group rows (multi-GPU sharding); pass 0, UINT32_MAX for the whole frame. */
jxlh_status jxlh_frame_run(jxlh_ctx* ctx, uint32_t group_row0, uint32_t group_row1);
/* mark_group_to_rerender + the re-render it triggers (render/mod.rs:143-146, callers frame/decode.rs:703-711): after
 * a jxlh_frame_run, groups whose coefficients changed (a later progressive pass) are reconstructed again -- the
 * transforms of exactly the listed groups, then the filters on every pixel row those groups influence (their rows
 * widened by the stage list's border: the part of the reference's 3x3 group neighbourhood that can change).  Stage
 * lists that overwrite the transforms' output (epf_iters == 3, per-stage kernels with an even stage count) and
 * chroma-subsampled frames re-render the whole frame instead; upsampled frames return JXLH_ERR_UNSUPPORTED. */
jxlh_status jxlh_frame_rerender_groups(jxlh_ctx* ctx, const uint32_t* group_ids, uint32_t count);
/* GROUPS WITHOUT HF.  The groups listed have no HF yet (DataStatus::Zero, frame/decode.rs:744-752): the next jxlh_frame_run /
 * jxlh_frame_rerender_groups fills their pixels from the frame's LF image, upsampled 8x with weights8, instead of
 * transforming them; every later stage treats them like any other group.  This is upsample_lf_group of the reference
 * (frame/decode.rs:51-158), the first paint of a file that is still arriving: mark every group, run, paint; then, as
 * groups arrive, submit them and call jxlh_frame_rerender_groups on them.
 *
 * Pixels: ahead of the filters a marked group's pixels equal, bit for bit, the group's rect of Upsample8x (three
 * accumulators, the reference's tap order, clamped to the 5x5 window's range) applied to the WHOLE LF image -- the
 * smoothed one, the raw one, or the LF slot's, whichever the frame uses -- with the window mirrored at the image's edges
 * only.  The kernels are the ones jxlh_set_upsampling_weights installed (its weights8), else the defaults; the frame's
 * own upsampling factor and the extra channels' keep their kernels.
 *   That is what the reference computes for every group except in two geometries, in which it reads its scratch row
 * beyond what it filled for that row (stale values of the previous row or channel, or zeros); the device does not
 * reproduce them, it mirrors properly:
 *   (a) a frame one group wide (xsize <= 256): the right padding is read from
 *       storage[save_start + mirror(save_end, save_end)], an index that is off by save_start = 2 (decode.rs:114-118);
 *   (b) xblocks % 32 == 1 (264 or 520 pixels wide, say): in the group column left of the one-block-wide last column,
 *       end_x = lf_x1 + 1 is neither lf_x1 nor two columns further, and the second padding column is never written.
 *
 * State: the marks are state of the frame.  jxlh_frame_begin clears them; they persist across runs.  Any later
 * submission of a group, in any form, with or without JXLH_GROUP_COMPLETE or JXLH_GROUP_ACCUMULATE, clears that group's
 * mark (the moment channel_status leaves Zero).  Marking a group after it was submitted in the same epoch marks it: the
 * last call wins; its coefficients stay where they are and are not read.
 *
 * Runs: a marked group's coefficient store is never read (on a long-lived context it holds an earlier frame's data).
 * K1 runs on the unmarked groups of the band only, the fill writes the marked ones into the planes K1 writes, whole
 * blocks up to xblocks * 8 x yblocks * 8, in the layout of that run.  A run over a group-row range fills the marked
 * groups of the band and of its halo group rows, like K1.  jxlh_frame_rerender_groups fills a listed group that is
 * marked and transforms one that is not; the filter bands are unchanged.  A frame with at least one marked group does
 * not take the strip kernel (JXLH_FRAME_STRIP): it falls to the two-kernel path with the same pixels, and
 * jxlh_frame_path says so.  A frame with no marked group enqueues exactly what it did without this call.
 *
 * Status, checked in this order, the marks unchanged by a refused call:
 *   JXLH_ERR_BAD_STATE         no frame begun, or a Modular frame (like the other VarDCT-only calls)
 *   JXLH_ERR_UNSUPPORTED       a chroma-subsampled frame (the reference's own code sizes the LF rect of such a frame
 *                              with hshift where it means vshift, decode.rs:88-89: there is nothing sound to match);
 *                              a context with comm_nranks > 1 (a rank holds only its band)
 *   JXLH_ERR_INVALID_ARGUMENT  an id >= the frame's number of groups (none of the call's ids is marked then)
 *   JXLH_OK                    count == 0 (nothing changes) */
jxlh_status jxlh_frame_set_groups_lf_only(jxlh_ctx* ctx, const uint32_t* group_ids, uint32_t count);
/* blocks until the main stream is idle */
jxlh_status jxlh_ctx_sync(jxlh_ctx* ctx);
/* PLACEMENT OF A CONTEXT'S BUFFERS (round 6; profiles/r06_q_context_placement.txt).  Where the driver places a context's
 * large buffers decides how fast the transforms and filters run on them: the same kernels on the same data are up to 10 %
 * apart between two contexts of one process -- persistently, reproducibly for a box and an allocation order, and not
 * visible in plain copies between the buffers.  jxlh_ctx_tune_placement(ctx, trials, ...) makes the context's NEXT first
 * allocation of {three planes, three filter planes, coefficient buffer} (the first jxlh_frame_begin, or the first one
 * after the buffers were released) a pick among `trials` candidate sets (up to twice as many while none of them stands
 * out), rated on the device by two byte movers with the streams of the 8x8 transform class and of the filters; the
 * candidates are held until the pick, then all but the best are freed.  Costs setup time (a few ms per candidate) and trials x the buffers' size in transient device memory (2.6 GB per
 * candidate at 8192^2); a candidate that cannot be allocated ends the trials early.  trials = 0: query only; 1: plain
 * allocation (the default).  report (nullable): the last pick's ratings, two floats per candidate (ms of the two
 * movers), *n_report floats; *picked: the candidate taken (-1: no pick yet).  No effect on results. */
jxlh_status jxlh_ctx_tune_placement(jxlh_ctx* ctx, int32_t trials, float* report, int32_t report_capacity, int32_t* n_report,
                                    int32_t* picked);

/* STREAM ORDERING OF DEVICE POINTERS.  Every stream of a context is a hipStreamNonBlocking stream: it does NOT
 * synchronise with the NULL (legacy default) stream or with any stream of the caller.  Host pointers are safe by
 * construction (the library's own copies are ordered on its streams), but a caller that fills a DEVICE buffer -- a
 * hipMemset / hipMemcpy on the NULL stream, a kernel on its own stream -- and then hands the pointer to an entry
 * point (jxlh_unsqueeze_chain, jxlh_rct, jxlh_palette*, jxlh_submit_group* with device sources, the stage hooks, the
 * *_device destinations of the read calls) must order that work in FRONT of the call, or the library's kernels may
 * run before the fill has (hipMemset returns before the fill has run; the same holds for the outputs: an output plane
 * the caller clears on the NULL stream can be cleared AFTER the library wrote it).  The reference hands buffers over by
 * ownership (RenderPipeline::set_buffer_for_group takes `buf: Image<T>`, render/mod.rs:124-137), so a binding has to
 * make the hand-over explicit with one of:
 *   jxlh_ctx_wait_stream(ctx, stream)   everything enqueued so far on `stream` (a hipStream_t; NULL = the legacy default
 *                                       stream) happens before whatever the context enqueues from now on -- on the
 *                                       device, the host does not block
 *   jxlh_ctx_wait_event(ctx, event)     the same for a hipEvent_t the caller has recorded
 *   jxlh_ctx_record_event(ctx, event)   the other direction: records the caller's event behind everything enqueued so
 *                                       far on the context's main stream, so a caller stream can hipStreamWaitEvent on
 *                                       the library's results without a host-side jxlh_ctx_sync
 * (a host-side hipDeviceSynchronize / hipStreamSynchronize before the call is the blunt alternative).  hipStream_t /
 * hipEvent_t travel as void* so that this header needs no HIP header. */
jxlh_status jxlh_ctx_wait_stream(jxlh_ctx* ctx, void* hip_stream);
jxlh_status jxlh_ctx_wait_event(jxlh_ctx* ctx, void* hip_event);
jxlh_status jxlh_ctx_record_event(jxlh_ctx* ctx, void* hip_event);
/* A point in the context's main stream: everything enqueued so far (frame runs, asynchronous reads).
 * jxlh_ctx_wait_mark blocks until that point has been reached and -- unlike jxlh_ctx_sync -- not for work enqueued after
 * the mark.  That is what lets ONE context stream consecutive frames (round 5: the slot-bucketed submission of frame
 * i + 1 no longer waits for frame i's transforms): submit frame i + 1 (its upload runs under frame i's kernels),
 * jxlh_frame_run, jxlh_frame_read_*_async, mark; then wait for the mark of frame i, whose output is complete.  Up to
 * JXLH_MAX_MARKS marks are alive at a time; waiting for an older one waits for the mark that replaced it.  Device-side
 * errors (JXLH_ERR_INVALID_TRANSFORM ...) are reported by jxlh_ctx_sync only. */
#define JXLH_MAX_MARKS 8
jxlh_status jxlh_ctx_mark(jxlh_ctx* ctx, uint32_t* mark);
jxlh_status jxlh_ctx_wait_mark(jxlh_ctx* ctx, uint32_t mark);
/* Copies the finished planes out (host or device destination).  Replaces the save stage for
 * f32 XYB output; xsize x ysize samples per plane. */
jxlh_status jxlh_frame_read_planes(jxlh_ctx* ctx, const jxlh_plane out[3]);
/* The same for one rectangle of the result: pixels [x0, x0 + w) x [y0, y0 + h), cut at the result's right and bottom
 * edge, into out[c] (row 0 of out[c] = row y0; at least min(w, xsize - x0) samples per row and min(h, ysize - y0)
 * rows; what lies beyond the cut is left untouched).  This is the unit the reference's pipeline moves:
 * RenderPipeline::get_buffer / set_buffer_for_group (render/mod.rs:124-137) hand over one 256 x 256 group per
 * channel, in buffers rounded up to 16 pixels (group_size_for_channel, render/internal.rs:144-167) -- a caller that
 * feeds the finished XYB planes to the remaining CPU stages group by group reads group g with
 * x0 = (g % xgroups) * 256, y0 = (g / xgroups) * 256, w = h = 256.  JXLH_ERR_INVALID_ARGUMENT
 * if the rect starts outside the result.  _async: without the final wait (host destinations should be pinned);
 * `out` is valid after the next jxlh_ctx_sync. */
jxlh_status jxlh_frame_read_planes_rect(jxlh_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                        const jxlh_plane out[3]);
jxlh_status jxlh_frame_read_planes_rect_async(jxlh_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                              const jxlh_plane out[3]);
/* device-resident result (row stride in floats), valid until the next frame_begin */
jxlh_status jxlh_frame_device_planes(jxlh_ctx* ctx, float* planes[3], size_t* stride);
/* Extra channels of the frame (alpha, depth, ...: channels 3 + ec of the reference's pipeline, frame/render.rs:564-567,
 * :624-637, :655-671).  jxlh_frame_set_extra_channel hands over Modular channel `ec` as decoded -- w x h i32 samples at
 * row stride `stride` (host or device memory) --; the next jxlh_frame_run (whole frame) applies
 * ConvertModularToF32Stage with the channel's bit depth (render/stages/convert.rs:488-533) and, for
 * ec_upsampling = 2 / 4 / 8, Upsample2x / 4x / 8x with the weights of jxlh_set_upsampling_weights
 * (render/stages/upsample.rs) -- before the colour channels' own upsampling or together with it, the result is the
 * same per channel.  ec_upsampling counts from the channel's own resolution: w = ceil(full width / ec_upsampling).
 * jxlh_frame_read_extra_channel copies the finished channel out: out_w x out_h f32 samples with
 * out_w = min(w * ec_upsampling, width of the frame's result), likewise the height.  Up to JXLH_MAX_EXTRA_CHANNELS. */
/* bits_per_sample carries the channel's BitDepth (headers/bit_depth.rs): bits_per_sample | exponent_bits_per_sample
 * << 8.  Exponent bits 0 = integer samples (val / (2^bits - 1)); otherwise the samples are `bits`-bit floats stored in
 * integers (binary16 = 16 | 5 << 8, binary32 = 32 | 8 << 8, any custom format) and are widened to binary32 exactly
 * (int_to_float, convert.rs:416-486).  The same convention holds for jxlh_modular_to_f32.  A channel handed over after
 * the frame's first render is converted by the next jxlh_frame_run or jxlh_frame_rerender_groups. */
#define JXLH_MAX_EXTRA_CHANNELS 8
jxlh_status jxlh_frame_set_extra_channel(jxlh_ctx* ctx, uint32_t ec, const int32_t* samples, size_t stride, uint32_t w,
                                         uint32_t h, uint32_t bits_per_sample, uint32_t ec_upsampling);
jxlh_status jxlh_frame_read_extra_channel(jxlh_ctx* ctx, uint32_t ec, const jxlh_plane* out);

/* ---------------------------------------------------------------- patches (features/patches.rs)
 * REFERENCE FRAMES.  DecoderState::reference_frames (4 slots of 3 + num_ec f32 planes, frame/mod.rs:77-80), held on the
 * device by the context: they survive jxlh_frame_begin and are freed by jxlh_ctx_clear_reference / jxlh_ctx_destroy.
 *   jxlh_ctx_set_reference     copies n_channels caller planes (w x h, row stride `stride` floats, host or device) into
 *                              `slot` -- a reference decoded elsewhere (a Modular reference-only frame, another
 *                              context's planes after jxlh_ctx_wait_event).  Returns when the copy has completed.
 *   jxlh_frame_save_reference  the save_before_ct save stage (frame/render.rs:711-722): the current frame's finished
 *                              result -- the colour planes after patches, upsampling and noise, and the patched extra
 *                              channels -- copied device to device, ordered on the context's stream.  Needs a
 *                              whole-frame render first (JXLH_ERR_BAD_STATE otherwise); every extra channel must have the
 *                              result's size (JXLH_ERR_UNSUPPORTED otherwise).
 * THE PATCH DICTIONARY of the current frame: PatchesDictionary (features/patches.rs:127-170) flattened.  patches[i] in
 * definition order, which is the order of application (set_patches_for_row's final sort, :676-679); blendings holds
 * n * (1 + num_ec) entries, entry i * (1 + num_ec) the colour blending of patch i, then one per extra channel (the
 * reference's blendings_stride layout); ec_flags[k] = JXLH_EC_* of extra channel k (the parts of ExtraChannelInfo that
 * perform_blending reads).  Checked like PatchesDictionary::read (:362-620), JXLH_ERR_INVALID_ARGUMENT with nothing
 * launched: the slot is set; num_ec == the slot's n_channels - 3 and == the number of extra channels the frame has been
 * handed so far (if any); the reference rectangle lies in the slot; mode < 8; alpha_channel < num_ec when the mode uses
 * alpha and num_ec > 1 (the reference reads it only then and leaves 0 otherwise: it is ignored); the patch rectangle
 * lies within the frame's PADDED size in its VarDCT form (FrameHeader::size_padded, headers/frame_header.rs:572-581:
 * whole 8x8 blocks of the coded size, as frame/decode.rs:317-323 passes it for a VarDCT frame), drawing is clipped at
 * the frame's edge.  A Modular frame's bound is its coded size (frame_header.rs:574-575): on a frame begun with
 * JXLH_FRAME_MODULAR the patch rectangle is checked against xsize x ysize, and a patch reaching into the 8x8 padding is
 * rejected; only a caller using the Modular seam (jxlh_stage_patches) still checks that bound itself.  The dictionary
 * needs a begun frame (jxlh_frame_begin with the frame's size).  n = 0 clears the dictionary; jxlh_frame_begin clears
 * it too.
 * Position in the frame: PatchesStage (frame/render.rs:644-650) -- after the filters and the extra channels' own
 * upsampling, BEFORE the colour upsampling and noise -- so patches are drawn at the coded size.  Extra channels are
 * drawn into a patched copy (jxlh_frame_read_extra_channel returns it); an upsampled frame may carry patches only
 * without extra channels, and every extra channel must cover the whole frame (JXLH_ERR_UNSUPPORTED / BAD_STATE from
 * jxlh_frame_set_patches / jxlh_frame_run otherwise).  A band run (jxlh_frame_run with a group-row range) of a frame
 * whose result lives in the planes the transforms write and whose transforms rewrite a group row beyond the band
 * (chroma-subsampled frames without a filter stage, stage lists that end in those planes) renders the whole frame
 * instead: the band's halo would undo the neighbouring band's patches.  Sharded runs of a frame with patches:
 * JXLH_ERR_UNSUPPORTED. */
#define JXLH_MAX_REFERENCE_FRAMES 4
enum { JXLH_EC_ALPHA = 1u << 0, JXLH_EC_ALPHA_ASSOCIATED = 1u << 1 };
/* PatchBlendMode (features/patches.rs:41-74) */
enum {
  JXLH_PATCH_NONE = 0, JXLH_PATCH_REPLACE = 1, JXLH_PATCH_ADD = 2, JXLH_PATCH_MUL = 3, JXLH_PATCH_BLEND_ABOVE = 4,
  JXLH_PATCH_BLEND_BELOW = 5, JXLH_PATCH_ALPHA_WEIGHTED_ADD_ABOVE = 6, JXLH_PATCH_ALPHA_WEIGHTED_ADD_BELOW = 7
};
typedef struct jxlh_patch {
  uint32_t x, y;            /* PatchPosition: top-left corner in the frame */
  uint32_t ref_slot;        /* PatchReferencePosition::reference */
  uint32_t ref_x0, ref_y0;  /* ... x0, y0 */
  uint32_t xsize, ysize;    /* ... xsize, ysize */
} jxlh_patch;
typedef struct jxlh_patch_blending {
  uint32_t mode;           /* JXLH_PATCH_* */
  uint32_t alpha_channel;  /* extra channel index */
  uint32_t clamp;          /* 0 / 1 */
} jxlh_patch_blending;
jxlh_status jxlh_ctx_set_reference(jxlh_ctx* ctx, uint32_t slot, uint32_t n_channels, uint32_t w, uint32_t h,
                                   const float* const* planes, size_t stride);
jxlh_status jxlh_frame_save_reference(jxlh_ctx* ctx, uint32_t slot);
jxlh_status jxlh_ctx_clear_reference(jxlh_ctx* ctx, uint32_t slot);
jxlh_status jxlh_frame_set_patches(jxlh_ctx* ctx, const jxlh_patch* patches, uint32_t n,
                                   const jxlh_patch_blending* blendings, uint32_t num_ec, const uint32_t* ec_flags);
/* The context's current dictionary applied to caller planes in place (3 colour + num_ec extra channels, w x h, row
 * stride `stride` floats, host or device), with the frame path's kernel: the Modular seam and tests. */
jxlh_status jxlh_stage_patches(jxlh_ctx* ctx, float* const planes[], uint32_t n_channels, uint32_t w, uint32_t h,
                               size_t stride);

/* ---------------------------------------------------------------- splines (features/spline.rs)
 * THE SEGMENTS of the current frame: the draw cache Splines::initialize_draw_cache leaves (SplineSegment, :338-346), in
 * its order.  They are taken as they are -- the reference filters at add_segment, not at the draw.  Segment s touches
 * pixel (x, y) of a w x h plane iff  max(0, round(cy - md)) <= y < min(h, round(cy + md) + 1)  and
 * round(cx - md) <= x < min(w, round(cx + md) + 1)  with Rust's conversions (round half away from zero; NaN -> 0; a
 * negative column -> 0, so a segment wholly left of the frame still adds to column 0 and one whose maximum_distance is
 * NaN adds to pixel (0, 0) only), and adds color[c] * sigma_over_4_times_intensity * (erf(a1) - erf(a2))^2 to channel
 * c there (draw_segment_inner, :540-584, its FMA form bit for bit).  Per pixel the segments are added in ascending
 * index.  Needs a begun frame (JXLH_ERR_BAD_STATE otherwise); n = 0 clears the segments, jxlh_frame_begin clears them
 * too; a null pointer with n > 0 is JXLH_ERR_INVALID_ARGUMENT with nothing launched.
 * Position in the frame: SplinesStage (frame/render.rs:652-653) -- after patches, BEFORE the colour upsampling and
 * noise, at the coded size; jxlh_frame_save_reference, jxlh_frame_blend, the read-outs and jxlh_frame_save see the
 * drawn result.  Splines are added in place like patches: what is said there about band runs holds here, a partial
 * re-render of a frame without a filter stage renders the frame again, and a sharded run is JXLH_ERR_UNSUPPORTED. */
typedef struct jxlh_spline_segment { /* SplineSegment, 32 bytes */
  float center_x, center_y, maximum_distance, inv_sigma, sigma_over_4_times_intensity;
  float color[3];
} jxlh_spline_segment;
jxlh_status jxlh_frame_set_splines(jxlh_ctx* ctx, const jxlh_spline_segment* segments, uint32_t n);
/* The context's current segments drawn onto three caller planes in place (w x h, row stride `stride` floats, host or
 * device; what lies beyond w in a row is not touched), with the frame path's kernel: the Modular seam and tests.
 * stride * h >= 2^31, or w or h >= 2147483520: JXLH_ERR_UNSUPPORTED.  Both set and stage calls wait for the context's
 * stream (their uploads come from host memory that is reused). */
jxlh_status jxlh_stage_splines(jxlh_ctx* ctx, float* const planes[3], uint32_t w, uint32_t h, size_t stride);
/* From the bitstream's form to segments, on the host (no context, no device): Splines::initialize_draw_cache
 * (features/spline.rs:733-797) -- dequantize with its range, distance and area checks, the adjacent-point check,
 * centripetal Catmull-Rom, equal spacing at distance 1, the continuous IDCT with fast_cos, add_segment's filter.
 * control_points: n_points (dx, dy) pairs, double-delta coded as read; color_dct: X, Y, B, 32 each.  out == NULL
 * counts only; *count is the number of segments either way, JXLH_ERR_INVALID_ARGUMENT if it exceeds `capacity` (nothing
 * partial is written) and for everything the reference answers with an error. */
typedef struct jxlh_quantized_spline {
  const int64_t* control_points;
  uint32_t n_points;
  int32_t color_dct[96];
  int32_t sigma_dct[32];
  float start_x, start_y; /* starting point */
} jxlh_quantized_spline;
jxlh_status jxlh_splines_build_segments(const jxlh_quantized_spline* splines, uint32_t n,
                                        int32_t quantization_adjustment, float y_to_x_lf, float y_to_b_lf,
                                        uint64_t image_xsize, uint64_t image_ysize, uint32_t high_precision,
                                        jxlh_spline_segment* out, size_t capacity, size_t* count);

/* smoothed LF image as used by K1 (tests) */
jxlh_status jxlh_frame_read_lf(jxlh_ctx* ctx, float* x, float* y, float* b, size_t stride);

/* ---------------------------------------------------------------- 8-bit sRGB output
 * The stages the reference runs after EPF for an XYB-encoded frame saved as 8-bit sRGB -- XybStage
 * (render/stages/xyb.rs:208-240), FromLinearStage with the sRGB curve (color/tf.rs:13-44),
 * ConvertF32ToU8Stage incl. its dither (render/stages/convert.rs:570-606), chained as in
 * frame/render.rs:757-762, :118 -- in one pass over the finished planes, written interleaved
 * (channels = 3: RGB, 4: RGBA with A = 255) for frame rows [y0, y1).  `out` points at row y0 and may be
 * host or device memory; for host memory the call returns after the copy has completed.
 * The parameters are the reference's XybParams::new(opsin, intensity_target) (xyb.rs:147-163):
 * inverse matrix, cbrt(biases), biases * intensity_scale, intensity_scale = 255 / intensity_target.
 * Frames whose output colour space is not sRGB/D65 with the sRGB transfer function go through
 * jxlh_frame_read_output, frames that need blending through jxlh_frame_blend first (this entry point does
 * what it says). */
typedef struct jxlh_xyb_params {
  float opsin_inverse_matrix[9];
  float bias_cbrt[3];
  float scaled_bias[3];
  float intensity_scale;
} jxlh_xyb_params;
jxlh_status jxlh_frame_read_rgb8(jxlh_ctx* ctx, const jxlh_xyb_params* p, uint32_t channels, uint32_t y0,
                                 uint32_t y1, void* out, size_t bytes_per_row);
/* jxlh_frame_read_rgb8 without the final wait: the conversion and the copy to `out` are queued on the context's
 * stream and the call returns; `out` (pinned host memory, or device memory) holds the image after the next
 * jxlh_ctx_sync.  Lets the download of frame i run while the caller submits frame i + 1 to another context. */
jxlh_status jxlh_frame_read_rgb8_async(jxlh_ctx* ctx, const jxlh_xyb_params* p, uint32_t channels, uint32_t y0,
                                       uint32_t y1, void* out, size_t bytes_per_row);
/* The same with ConvertF32ToU16Stage at 16 bits (render/stages/convert.rs:743-761: clamp to [0,1], x65535,
 * round to nearest even, no dither): native-endian u16 samples, interleaved. */
jxlh_status jxlh_frame_read_rgb16(jxlh_ctx* ctx, const jxlh_xyb_params* p, uint32_t channels, uint32_t y0,
                                  uint32_t y1, void* out, size_t bytes_per_row);

/* The same for a YCbCr frame (do_ycbcr, not XYB-encoded -- JPEG recompressions): YcbcrToRgbStage
 * (render/stages/ycbcr.rs:35-78) on the planes taken as Cb, Y, Cr, then the integer conversion; no
 * transfer-function stage (frame/render.rs:755-763). */
jxlh_status jxlh_frame_read_ycbcr_rgb8(jxlh_ctx* ctx, uint32_t channels, uint32_t y0, uint32_t y1, void* out,
                                       size_t bytes_per_row);
jxlh_status jxlh_frame_read_ycbcr_rgb16(jxlh_ctx* ctx, uint32_t channels, uint32_t y0, uint32_t y1, void* out,
                                        size_t bytes_per_row);

/* General form of the output calls: the colour stage of the frame (frame/render.rs:755-763) -- XybStage, for an
 * XYB-encoded frame, followed by FromLinearStage with one of the reference's transfer functions
 * (render/stages/from_linear.rs:133-145; curves of color/tf.rs and util/fast_math.rs, evaluated operation for
 * operation), YcbcrToRgbStage, or nothing -- then ConvertF32ToU8Stage (bits = 8) or ConvertF32ToU16Stage (16).
 *   JXLH_TF_LINEAR  no FromLinearStage (linear output, TransferFunction::is_linear)
 *   JXLH_TF_SRGB    linear_to_srgb_simd            JXLH_TF_BT709  linear_to_bt709_simd
 *   JXLH_TF_PQ      linear_to_pq_simd, tf_param = intensity_target
 *   JXLH_TF_HLG     hlg_display_to_scene + scene_to_hlg; tf_param = (1 - g) / g with the system gamma
 *                   g = 1.2 * 1.111^log2(intensity_target / 1000) evaluated by the caller exactly as
 *                   color/tf.rs:442-446 does (host libm), hlg_luminance_rgb = luminance_rgb
 *   JXLH_TF_GAMMA   fast_powf_simd(|v|, tf_param), tf_param = the encoding exponent in (0, 1] */
enum { JXLH_COLOR_XYB = 0, JXLH_COLOR_YCBCR = 1, JXLH_COLOR_NONE = 2 };
enum { JXLH_TF_LINEAR = 0, JXLH_TF_SRGB = 1, JXLH_TF_BT709 = 2, JXLH_TF_PQ = 3, JXLH_TF_HLG = 4, JXLH_TF_GAMMA = 5 };
typedef struct jxlh_output_desc {
  uint32_t color;     /* JXLH_COLOR_* */
  uint32_t transfer;  /* JXLH_TF_*, used with JXLH_COLOR_XYB */
  jxlh_xyb_params xyb;
  float tf_param;
  float hlg_luminance_rgb[3];
  uint32_t bits;      /* 8 or 16 */
  uint32_t channels;  /* 3 or 4 (alpha = opaque) */
} jxlh_output_desc;
jxlh_status jxlh_frame_read_output(jxlh_ctx* ctx, const jxlh_output_desc* d, uint32_t y0, uint32_t y1, void* out,
                                   size_t bytes_per_row);
/* without the final wait, like jxlh_frame_read_rgb8_async: `out` is valid after the next jxlh_ctx_sync */
jxlh_status jxlh_frame_read_output_async(jxlh_ctx* ctx, const jxlh_output_desc* d, uint32_t y0, uint32_t y1, void* out,
                                         size_t bytes_per_row);

/* ---------------------------------------------------------------- frame blending (render/stages/blending.rs, extend.rs)
 * How the reference closes a frame that needs_blending() (headers/frame_header.rs:540-552: every cropped frame, every
 * colour or extra-channel blend mode other than Replace -- animation deltas, layers, alpha compositing), as
 * frame/render.rs:754-791 orders it: colour stage, BlendingStage, ExtendToImageDimensionsStage, save into the reference
 * slot, conversion.
 * jxlh_frame_blend, on the context's stream without host synchronisation, in one pass over the image:
 *   1. the colour stage named by `colour` (color, transfer, xyb, tf_param, hlg_luminance_rgb; bits / channels are
 *      ignored; NULL = JXLH_COLOR_NONE) on the frame's three result planes, kept in f32;
 *   2. BlendingStage::process_row_chunk (blending.rs:97-166): the frame is perform_blending's bg, the slot named by
 *      `source` its fg, read at image coordinates (x0 + x, y0 + y).  Colour reads channels 0..2 of color.source, extra
 *      channel i reads channel 3 + i of ec[i].source; a slot that is not set is a row of zeros.  Modes map as
 *      From<&BlendingInfo> for PatchBlending does (blending.rs:41-56): Replace -> None, Add -> Add, Mul -> Mul,
 *      Blend -> BlendBelow, AlphaWeightedAdd -> AlphaWeightedAddBelow.  Frame pixels outside the image are dropped;
 *   3. ExtendToImageDimensionsStage (extend.rs:59-84): every image pixel outside the frame's rectangle takes the value
 *      of that channel's source slot, or zero.
 * The image_w x image_h set of 3 + num_ec planes BECOMES THE FRAME'S RESULT: jxlh_frame_read_planes / _rect /
 * jxlh_frame_device_planes return the composed colour planes, jxlh_frame_read_extra_channel the composed extra channels
 * (image-sized), jxlh_frame_save_reference saves them (the !save_before_ct save, render.rs:780-791), and the output
 * calls with JXLH_COLOR_NONE convert them to 8 / 16 bit; an output call with any other colour stage returns
 * JXLH_ERR_BAD_STATE (the stage has run already).  The frame is the result of the last whole-frame render
 * (JXLH_ERR_BAD_STATE without one) at the result's size (the upsampled size of an upsampled frame); its extra channels
 * are the converted / upsampled / patched planes jxlh_frame_save_reference would save, under the same conditions.  The
 * call reads the frame's own planes and the slots and writes a separate canvas: calling it again gives the same canvas.
 * A later jxlh_frame_run / jxlh_frame_rerender_groups discards the composition (the result is the frame's own planes
 * again), jxlh_frame_begin does too.
 * JXLH_ERR_INVALID_ARGUMENT, checked before anything is launched (an earlier composition stays as it is): mode > 4,
 * source >= 4, num_ec > 8, num_ec != the number of extra channels handed to the frame, alpha_channel >= num_ec for
 * Blend / AlphaWeightedAdd when num_ec > 0 (the reference's header check; the field is not read for other modes),
 * image_w * image_h zero or >= 2^31, a set source slot smaller than the image or with n_channels != 3 + num_ec.
 * Sharded contexts: JXLH_ERR_UNSUPPORTED.
 * jxlh_stage_blend: the same kernel on caller planes (host or device): frame[] are n_channels = 3 + num_ec planes of
 * w x h at row stride `stride` floats, already in the output colour space; out[] as many image_w x image_h planes at
 * row stride out_stride.  The Modular seam and tests.
 * Alpha taken from an extra channel into the interleaved output, premultiplication and spot colours belong to the
 * save tail behind this stage: jxlh_frame_save below.  (Splines are drawn before this stage: jxlh_frame_set_splines.) */
/* BlendingMode (headers/frame_header.rs:98-104) */
enum {
  JXLH_BLEND_REPLACE = 0, JXLH_BLEND_ADD = 1, JXLH_BLEND_BLEND = 2, JXLH_BLEND_ALPHA_WEIGHTED_ADD = 3, JXLH_BLEND_MUL = 4
};
typedef struct jxlh_blending_info { /* BlendingInfo (frame_header.rs:114-140) */
  uint32_t mode;           /* JXLH_BLEND_* */
  uint32_t alpha_channel;  /* extra channel index */
  uint32_t clamp;          /* 0 / 1 */
  uint32_t source;         /* reference slot */
} jxlh_blending_info;
typedef struct jxlh_blend_desc {
  int32_t x0, y0;             /* FrameHeader::x0, y0: the frame's origin in the image, may be negative */
  uint32_t image_w, image_h;  /* FileHeader::size */
  jxlh_blending_info color;   /* FrameHeader::blending_info */
  uint32_t num_ec;
  jxlh_blending_info ec[8];   /* FrameHeader::ec_blending_info */
  uint32_t ec_flags[8];       /* JXLH_EC_* per extra channel, as for jxlh_frame_set_patches */
} jxlh_blend_desc;
jxlh_status jxlh_frame_blend(jxlh_ctx* ctx, const jxlh_blend_desc* desc, const jxlh_output_desc* colour);
jxlh_status jxlh_stage_blend(jxlh_ctx* ctx, const jxlh_blend_desc* desc, const float* const frame[], uint32_t n_channels,
                             uint32_t w, uint32_t h, size_t stride, float* const out[], size_t out_stride);

/* ---------------------------------------------------------------- the save tail (frame/render.rs:793-903)
 * What the reference puts behind a frame's last f32 stage, fused into one pass over the frame's result (its planes, or
 * the canvas after jxlh_frame_blend) and its extra channels; nothing is written back to them, so a frame can be saved
 * any number of times, into several buffers, and jxlh_frame_read_planes keeps returning the planes in front of these
 * stages.  Per output sample, in registers:
 *   1. the colour stage `colour` names on channels 0..2 (as jxlh_frame_read_output; bits / channels are ignored; NULL =
 *      JXLH_COLOR_NONE).  After jxlh_frame_blend it has run already: anything but JXLH_COLOR_NONE is JXLH_ERR_BAD_STATE;
 *   2. SpotColorStage (render/stages/spot.rs:40-67) for spot[0 .. n_spot), in order: mix = rgba[3] * s,
 *      c = mix * rgba[k] + (1 - mix) * c, two products and a sum rounded separately;
 *   3. PremultiplyAlphaStage (premultiply_alpha.rs:47-92) when `premultiply`: the colour channels times the sample of
 *      pipeline channel premultiply_alpha_channel;
 *   4. conversion of each channel of `channels` (pipeline channels in output order: 0..2 colour, 3 + ec extra channel
 *      ec; BGR(A) is {2, 1, 0(, a)}, gray {0}, a lone extra channel {3 + ec}):
 *        JXLH_SAVE_U8   ConvertF32ToU8Stage, bit_depth 1..8: v * max + dither[(y + 13 ch) % 32][(x + 23 ch) % 32], clamped
 *                       to [0, max] (NaN -> 0), round to nearest even; ch is the PIPELINE channel
 *        JXLH_SAVE_U16  ConvertF32ToU16Stage, bit_depth 1..16: clamp to [0, 1] (NaN -> 0), * max, round to nearest even
 *        JXLH_SAVE_F16  ConvertF32ToF16Stage: f32::clamp(f16_clamp_min, f16_clamp_max) when f16_clamp (a NaN stays, the
 *                       reference uses (0, 1) for PQ and (-0.074, 1.1) for HLG), then f16::from_f32 of util/float16.rs as
 *                       written: nearest even in the normal range, TRUNCATION into f16 denormals, NaN -> sign | 0x7E00.
 *                       As written, that function shifts a denormal result one bit further than the 2^-24 unit asks for
 *                       ((mant | 0x800000) >> -unbiased): |v| in [2^-24, 2^-23) gives a zero and every f16 denormal comes
 *                       out at half its IEEE value.  The device gives the reference's bits, not IEEE's.
 *        JXLH_SAVE_F32  the bits
 *      16- and 32-bit samples little endian, or big endian when big_endian;
 *   5. when fill_opaque_alpha, one more sample behind them: 2^bit_depth - 1, 0x3C00 or 1.0f (api/data_types.rs:114-149);
 *   6. position: the samples of source pixel (x, y) go to pixel display_pixel((x, y), (w, h)) of the oriented image,
 *      orientation 1..8 as headers/image_metadata.rs:85-96 (1 identity, 2 flip horizontal, 3 rotate 180, 4 flip
 *      vertical, 5 transpose, 6 rotate 90 cw, 7 anti-transpose, 8 rotate 90 ccw); the image is h x w for 5..8.
 * (x, y) are the result's coordinates -- image coordinates after jxlh_frame_blend, upsampled ones for an upsampled frame.
 * jxlh_frame_save: `out` (host or device memory) is the origin of the WHOLE oriented image, bytes_per_row its row
 * pitch; rows [y0, y1) of the SOURCE (y1 is cut at the result's height) are written, each pixel to its display
 * position, so a caller can save in bands under every orientation.  Extra channels are the planes
 * jxlh_frame_read_extra_channel returns (patched, upsampled, converted, or the canvas channel).  Host memory goes
 * through the context's staging buffer; a chroma-subsampled frame materialises its chroma first.  _async: without the
 * final wait, as jxlh_frame_read_output_async.
 * jxlh_stage_save: the same kernel on caller planes (host or device): planes[] are n_planes >= 3 f32 planes (3 colour +
 * extra channels) of w x h at row stride `stride` floats; (frame_x0, frame_y0) is the position of plane pixel (0, 0) in
 * its frame, which only the dither table sees.  The Modular seam and tests.
 * Checked before anything is launched or written.  JXLH_ERR_INVALID_ARGUMENT: a null pointer; n_channels 0 or > 4, or
 * more than 4 samples with the fill; a channel >= 3 + JXLH_MAX_EXTRA_CHANNELS (jxlh_stage_save: >= n_planes); format,
 * orientation or bit_depth out of range; y0 >= y1; bytes_per_row smaller than the oriented row or, like `out`, not a
 * multiple of the sample size; f16_clamp with min > max or a NaN bound; a premultiply or spot channel that is not an
 * extra channel; n_spot > JXLH_MAX_EXTRA_CHANNELS.  JXLH_ERR_BAD_STATE: no result; a colour stage on a blended frame; an
 * extra channel that is not set or not rendered, or does not cover the result (an upsampled frame whose extra channels
 * stayed smaller).  JXLH_ERR_UNSUPPORTED: sharded contexts; w * h >= 2^31. */
enum { JXLH_SAVE_U8 = 0, JXLH_SAVE_U16 = 1, JXLH_SAVE_F16 = 2, JXLH_SAVE_F32 = 3 };
typedef struct jxlh_spot_color {
  uint32_t ec;    /* extra channel index */
  float rgba[4];  /* ExtraChannelInfo::spot_color */
} jxlh_spot_color;
typedef struct jxlh_save_desc {
  uint32_t n_channels;  /* 1..4 */
  uint32_t channels[4]; /* pipeline channels in output order */
  uint32_t fill_opaque_alpha;
  uint32_t format;      /* JXLH_SAVE_* */
  uint32_t bit_depth;   /* U8: 1..8, U16: 1..16; ignored for F16 / F32 */
  uint32_t big_endian;
  uint32_t orientation; /* 1..8 */
  uint32_t f16_clamp;
  float f16_clamp_min, f16_clamp_max;
  uint32_t premultiply;
  uint32_t premultiply_alpha_channel; /* pipeline channel, 3 + ec */
  uint32_t n_spot;
  jxlh_spot_color spot[8];
} jxlh_save_desc;
jxlh_status jxlh_frame_save(jxlh_ctx* ctx, const jxlh_output_desc* colour, const jxlh_save_desc* save, uint32_t y0,
                            uint32_t y1, void* out, size_t bytes_per_row);
jxlh_status jxlh_frame_save_async(jxlh_ctx* ctx, const jxlh_output_desc* colour, const jxlh_save_desc* save, uint32_t y0,
                                  uint32_t y1, void* out, size_t bytes_per_row);
jxlh_status jxlh_stage_save(jxlh_ctx* ctx, const jxlh_output_desc* colour, const jxlh_save_desc* save,
                            const float* const planes[], uint32_t n_planes, uint32_t w, uint32_t h, size_t stride,
                            uint32_t frame_x0, uint32_t frame_y0, uint32_t y0, uint32_t y1, void* out,
                            size_t bytes_per_row);

/* Save rectangles -- the same save for a LIST of rectangles of the source in one launch, so that a repaint moves only
 * the pixels a group re-render can have changed, and the host function that names those rectangles:
 * jxlh_frame_save_rects, jxlh_frame_save_rects_async, jxlh_stage_save_rects and jxlh_changed_rects (jxlh_rect,
 * JXLH_MAX_SAVE_RECTS), declared in jxl_hip_save_rects.h, which this header includes at its end.
 * Extra channels by rect -- a channel declared once and fed rect by rect as its groups arrive, converted and upsampled
 * only where a rect can have changed it: jxlh_frame_begin_extra_channel, jxlh_frame_set_extra_channel_rects (_async)
 * and jxlh_extra_channel_changed_rects (jxlh_ec_rect, JXLH_MAX_EC_RECTS), declared in jxl_hip_extra_rects.h, likewise.
 * Repaint -- the re-render of listed groups on every kind of unsharded frame, upsampled and Modular frames included, and
 * the rectangles of the result it can change: jxlh_frame_repaint_groups and jxlh_repaint_changed_rects, declared in
 * jxl_hip_repaint.h, likewise.
 * Blend rectangles -- after such a re-render of a blended frame, the recomposition of only the changed rectangles of the
 * canvas jxlh_frame_blend wrote, and the mapping of a frame's changed rects to the image: jxlh_frame_blend_rects,
 * jxlh_stage_blend_rects and jxlh_blend_image_rects, declared in jxl_hip_blend_rects.h, likewise. */

/* ---------------------------------------------------------------- LF frames
 * A frame with lf_level = L >= 1 (the layers of a progressive_dc file) is an ordinary frame of ceil(size / 8^L) pixels,
 * usually Modular XYB, sometimes VarDCT (FrameHeader::size_upsampled, headers/frame_header.rs:584-589): begin, fill and
 * run it like any other.  What sets it apart is where its result goes: the three colour planes ahead of the colour
 * transform are kept in DecoderState::lf_frames[L - 1] (frame/mod.rs:120,136,399-401; the Grayscale f32 save stages of
 * frame/render.rs:699-710), and a later VarDCT frame with USE_LF_FRAME takes lf_frames[its lf_level] as its LF image
 * (frame/decode.rs:172-178,737-743) -- it decodes no LF of its own and skips adaptive LF smoothing
 * (should_do_adaptive_lf_smoothing, frame_header.rs:496-500).  The context holds those JXLH_NUM_LF_FRAMES slots next to
 * the reference slots: three f32 planes (X, Y, B) of w x h each, rows 256-byte aligned, surviving jxlh_frame_begin, freed
 * by jxlh_ctx_clear_lf_frame and jxlh_ctx_destroy.  Slot mapping: an LF frame saves into slot lf_level - 1; the frame it
 * feeds (whose own lf_level is one lower) reads slot = ITS lf_level -- the same number.
 *   jxlh_ctx_set_lf_frame        slot <- caller planes (host or device, order X, Y, B as jxlh_frame_set_lf, row stride
 *                                `stride` >= w floats): an LF frame decoded elsewhere.  Returns when the copy has landed.
 *   jxlh_frame_save_lf           slot <- the current frame's finished colour result (what jxlh_frame_save_reference
 *                                saves: after filters, patches, splines, upsampling and noise, before the colour
 *                                transform), device to device on the context's stream.  VarDCT and Modular frames alike.
 *                                Needs a whole-frame render: JXLH_ERR_BAD_STATE before one and after jxlh_frame_blend.
 *   jxlh_ctx_clear_lf_frame      frees the slot (waits for the stream first).
 *   jxlh_frame_set_lf_from_slot  the WHOLE LF image of the current VarDCT frame becomes a copy of the slot's planes
 *                                (device to device, on the stream): overwriting or clearing the slot afterwards does
 *                                not change the frame.  The frame then never runs adaptive LF smoothing, whatever
 *                                params.do_lf_smoothing says, and jxlh_frame_read_lf returns the slot's samples.  A
 *                                later jxlh_frame_set_lf / _set_lf_quantized on such a frame is JXLH_ERR_BAD_STATE, and
 *                                so is this call after one of them in the same frame.  Everything downstream is
 *                                unchanged: HF metadata, coefficient submissions, bands, jxlh_frame_rerender_groups,
 *                                filters, post stages, save.
 * Checked before anything is launched; a refused call changes nothing.  JXLH_ERR_INVALID_ARGUMENT: slot >=
 * JXLH_NUM_LF_FRAMES; a null plane; stride < w; w or h zero or above 2^20; (set_lf_from_slot) an unset slot or one whose
 * size differs from the frame's size in blocks.  JXLH_ERR_BAD_STATE: outside a frame; (set_lf_from_slot) a Modular frame.
 * JXLH_ERR_UNSUPPORTED: a sharded context; (set_lf_from_slot) a chroma-subsampled frame, whose size in blocks rounds past
 * the LF frame's size (the reference has no defined answer there).
 *
 * jxlh_lf_preview: while such a file is still arriving, the reference shows lf_frames[0] as a full-size preview
 * (Frame::render_lf_frame_rect / maybe_preview_lf_frame, frame/lf_preview.rs:24-387): Upsample8x -> XybStage ->
 * FromLinearStage -> integer / f16 conversion -> oriented interleaved save, rect by rect.  This call is that chain for one
 * rect (x0, y0, w, h in LF pixels) of `slot`, one kernel, nothing in between written to memory; callable inside or outside
 * a frame, ordered on the context's stream.  image_w x image_h is the image the preview stands for: the slot must be
 * ceil(image_w / 8) x ceil(image_h / 8).  `out` is the origin of the WHOLE oriented image as for jxlh_frame_save (host or
 * device memory; host memory goes through the staging buffer); _async omits the final wait.  Per output pixel:
 *   1. Upsample8x of the slot's three planes with the weights of jxlh_set_upsampling_weights, bit for bit the stage of
 *      jxlh_stage_upsample; the 5x5 window is mirrored against the whole SLOT, not the rect (lf_preview.rs:127-140).  LF
 *      pixel (x, y) yields image pixels [8x, 8x + 8) x [8y, 8y + 8), clipped to the image (:364);
 *   2. the colour stage `colour` names: JXLH_COLOR_XYB with a non-linear transfer function, as jxlh_frame_save step 1;
 *   3. conversion as jxlh_frame_save step 4, with the pipeline position the reference's preview has: every converter is
 *      built for channel 0 and every row handed over at (0, 0) (:60,67,72,208-214).  JXLH_SAVE_U8 therefore dithers all
 *      three channels and all rows with dither[0][(X - 8 * x0) % 32], X the image column -- no channel term, no row term,
 *      and a phase that depends on the rect's left edge.  JXLH_SAVE_F16 is never clamped (f16_clamp* are ignored: a caller
 *      may pass the frame's own descriptor).  U16, F32 and the byte order as there;
 *   4. save->channels is {0, 1, 2} or {2, 1, 0} with n_channels == 3; fill_opaque_alpha appends the opaque sample (:56-83);
 *   5. position: display_pixel of save->orientation against image_w x image_h, as jxlh_frame_save step 6.
 * Checked before anything is launched or written.  JXLH_ERR_INVALID_ARGUMENT: a null ctx, save or out; slot >=
 * JXLH_NUM_LF_FRAMES or unset; a slot whose size is not ceil(image / 8); a rect that leaves the slot; any other channel
 * list; premultiply or n_spot non-zero; format, orientation, bit depth, bytes_per_row and alignment as jxlh_frame_save.
 * JXLH_ERR_UNSUPPORTED: colour NULL, not XYB or JXLH_TF_LINEAR (where the reference shows no preview); a sharded context;
 * image_w * image_h >= 2^31.  A zero-sized rect is JXLH_OK and writes nothing. */
#define JXLH_NUM_LF_FRAMES 4
jxlh_status jxlh_ctx_set_lf_frame(jxlh_ctx* ctx, uint32_t slot, uint32_t w, uint32_t h, const float* x, const float* y,
                                  const float* b, size_t stride);
jxlh_status jxlh_frame_save_lf(jxlh_ctx* ctx, uint32_t slot);
jxlh_status jxlh_ctx_clear_lf_frame(jxlh_ctx* ctx, uint32_t slot);
jxlh_status jxlh_frame_set_lf_from_slot(jxlh_ctx* ctx, uint32_t slot);
jxlh_status jxlh_lf_preview(jxlh_ctx* ctx, uint32_t slot, uint32_t image_w, uint32_t image_h, uint32_t x0, uint32_t y0,
                            uint32_t w, uint32_t h, const jxlh_output_desc* colour, const jxlh_save_desc* save, void* out,
                            size_t bytes_per_row);
jxlh_status jxlh_lf_preview_async(jxlh_ctx* ctx, uint32_t slot, uint32_t image_w, uint32_t image_h, uint32_t x0,
                                  uint32_t y0, uint32_t w, uint32_t h, const jxlh_output_desc* colour,
                                  const jxlh_save_desc* save, void* out, size_t bytes_per_row);

/* ---------------------------------------------------------------- stage-level hooks */
/* Whole-image single stages with the pipeline's mirror edge semantics; the analogue of
 * make_and_run_simple_pipeline (jxl/src/render/test.rs:83-179).  Planes: w x h f32, row stride
 * `stride` floats, host or device pointers. */
jxlh_status jxlh_stage_gaborish(jxlh_ctx* ctx, const float* in, float* out, uint32_t w, uint32_t h,
                                size_t stride, float w1, float w2);
/* stage = 0, 1, 2 (Epf0Stage / Epf1Stage / Epf2Stage); inv_sigma: ceil(w/8) x ceil(h/8) floats,
 * row stride sigma_stride; uses the epf_* fields of p */
jxlh_status jxlh_stage_epf(jxlh_ctx* ctx, int32_t stage, const jxlh_frame_params* p,
                           const float* const in[3], float* const out[3], uint32_t w, uint32_t h,
                           size_t stride, const float* inv_sigma, size_t sigma_stride);
/* HorizontalChromaUpsample (horizontal != 0: out is 2w x h) or VerticalChromaUpsample (out is w x 2h) on a
 * tight w x h plane, edges mirrored (render/stages/chroma_upsample.rs:31-63, :108-147) */
jxlh_status jxlh_stage_chroma_upsample(jxlh_ctx* ctx, const float* in, float* out, uint32_t w, uint32_t h,
                                       int32_t horizontal);
/* Upsample2x / 4x / 8x (render/stages/upsample.rs) on a tight w x h plane -> (n*w) x (n*h), n = 2, 4, 8, with the
 * weights of jxlh_set_upsampling_weights; input mirrored 2 pixels at its edges */
jxlh_status jxlh_stage_upsample(jxlh_ctx* ctx, int32_t n, const float* in, float* out, uint32_t w, uint32_t h);
/* Noise synthesis, stage by stage (tight arrays): the three random planes of a w x h image
 * (render_noise_for_group, frame/decode.rs:578-668); ConvolveNoiseStage (render/stages/noise.rs:32-86);
 * AddNoiseStage on n samples with p's noise_lut and colour-correlation fields (noise.rs:140-189), in place. */
jxlh_status jxlh_stage_noise_generate(jxlh_ctx* ctx, uint32_t visible_frame_index, uint32_t nonvisible_frame_index,
                                      uint32_t w, uint32_t h, float* const out[3]);
jxlh_status jxlh_stage_noise_convolve(jxlh_ctx* ctx, const float* in, float* out, uint32_t w, uint32_t h);
jxlh_status jxlh_stage_noise_add(jxlh_ctx* ctx, const jxlh_frame_params* p, float* const planes[3],
                                 const float* const rnd[3], size_t n);
/* adaptive_lf_smoothing on w x h tight planes (frame/adaptive_lf_smoothing.rs:44-125) */
jxlh_status jxlh_stage_lf_smooth(jxlh_ctx* ctx, const jxlh_frame_params* p, const float* const in[3],
                                 float* const out[3], uint32_t w, uint32_t h);
/* transform_to_pixels on a batch of independent varblocks of one type (transform.rs:666-677):
 * coeffs n * cx*cy*64 dequantised coefficients, lf n * cx*cy samples, pixels n * (cy*8)*(cx*8). */
jxlh_status jxlh_stage_transform_to_pixels(jxlh_ctx* ctx, int32_t type, uint32_t n, const float* coeffs,
                                           const float* lf, float* pixels);

/* ---------------------------------------------------------------- Modular (wrapping i32) */
/* do_rct_step (modular/transforms/rct.rs:118-157) on whole planes of n samples, in place. */
jxlh_status jxlh_rct(jxlh_ctx* ctx, int32_t* p0, int32_t* p1, int32_t* p2, size_t n, int32_t op,
                     int32_t perm);
/* do_palette_step_general, num_deltas == 0 && predictor == Zero branch (palette.rs:182-199).
 * palette: nb_channels rows x palette_stride; out: nb_channels planes of n samples, contiguous. */
jxlh_status jxlh_palette(jxlh_ctx* ctx, const int32_t* index, size_t n, const int32_t* palette,
                         int32_t num_colors, size_t palette_stride, int32_t nb_channels,
                         int32_t bit_depth, int32_t* out);
/* The same on a run of n samples of a larger image (device pointers only): channel c of the run is written at
 * out + c * out_channel_stride, so a rank can expand its share of the index plane straight into full-size planes. */
jxlh_status jxlh_palette_strided(jxlh_ctx* ctx, const int32_t* index, size_t n, const int32_t* palette,
                                 int32_t num_colors, size_t palette_stride, int32_t nb_channels, int32_t bit_depth,
                                 int32_t* out, size_t out_channel_stride);
/* do_palette_step_general with delta entries and / or a neighbour predictor (palette.rs:228-251): index is w x h,
 * entries below num_deltas are added to Predictor::predict_one (modular/predict.rs:152-198; predictor = Predictor
 * as u32; 6 = Weighted needs its header: jxlh_palette_delta_wp, JXLH_ERR_UNSUPPORTED here) of the already
 * reconstructed neighbours, palette_size =
 * num_colors + num_deltas.  Sequential by nature: runs as a skewed wavefront, far from bandwidth bound. */
jxlh_status jxlh_palette_delta(jxlh_ctx* ctx, const int32_t* index, uint32_t w, uint32_t h, const int32_t* palette,
                               int32_t num_colors, int32_t num_deltas, size_t palette_stride, int32_t nb_channels,
                               int32_t bit_depth, int32_t predictor, int32_t* out);
/* The same step with Predictor::Weighted (palette.rs:200-227): every pixel runs the self-correcting predictor
 * (WeightedPredictorState, modular/predict.rs:221-519) and updates its error state, delta entries are added to its
 * prediction.  wp = the group's WeightedHeader (headers/modular.rs:16-66; 5-bit p*, 4-bit w*). */
typedef struct jxlh_wp_header {
  uint32_t p1c, p2c, p3ca, p3cb, p3cc, p3cd, p3ce, w0, w1, w2, w3;
} jxlh_wp_header;
jxlh_status jxlh_palette_delta_wp(jxlh_ctx* ctx, const int32_t* index, uint32_t w, uint32_t h, const int32_t* palette,
                                  int32_t num_colors, int32_t num_deltas, size_t palette_stride, int32_t nb_channels,
                                  int32_t bit_depth, const jxlh_wp_header* wp, int32_t* out);
/* The stages between the Modular channels and the rest of the pipeline (render/stages/convert.rs), whole planes:
 *  - jxlh_modular_to_rgb8: ConvertI32ToU8Stage (:642-715) on three channels, interleaved -- what the pipeline builder
 *    substitutes for ConvertModularToF32 + ConvertF32ToU8 when the output depth is a multiple of the channel depth
 *    (render/builder.rs:152-170): multiplier = (2^8 - 1) / (2^bits - 1), max = 255; a lossless 8-bit image after
 *    RCT / Palette / Squeeze goes straight to displayable bytes
 *  - jxlh_modular_to_f32: ConvertModularToF32Stage for integer samples (:488-533), val * 1 / (2^bits - 1)
 *  - jxlh_modular_xyb_to_f32: ConvertModularXYBToF32Stage (:306-343), channels in coded order Y, X, B,
 *    quant_factors = LfQuantFactors::quant_factors (X, Y, B) */
jxlh_status jxlh_modular_to_rgb8(jxlh_ctx* ctx, const int32_t* const planes[3], size_t stride, uint32_t w, uint32_t h,
                                 int32_t multiplier, int32_t max, uint32_t channels, void* out, size_t bytes_per_row);
jxlh_status jxlh_modular_to_f32(jxlh_ctx* ctx, const int32_t* in, size_t n, uint32_t bits_per_sample, float* out);
jxlh_status jxlh_modular_xyb_to_f32(jxlh_ctx* ctx, const int32_t* y, const int32_t* x, const int32_t* b, size_t n,
                                    const float quant_factors[3], float* ox, float* oy, float* ob);
/* SAMPLE RANGE of every squeeze entry point below (jxlh_unsqueeze*, jxlh_unsqueeze_chain): averages, residuals and
 * reconstructed samples in [-2^28, 2^28).  Inside it the result equals BOTH forms the reference holds -- the i64
 * `unsqueeze_scalar` (squeeze.rs:187-194) and the wrapping-i32 `unsqueeze_impl` / `smooth_tendency_impl` of its SIMD
 * back-ends (squeeze.rs:107-185) -- bit for bit.  From about 2^29 on those two forms give DIFFERENT results for the
 * same input (which one a sample gets depends on its place in the back-end's tiling), so the reference defines no
 * value there; the device then computes a third wrapping-i32 form, deterministic but equal to neither.  8..24-bit
 * images, also after an RCT, are far inside the range (tests/test_oracle_pin.py pins the bound on all three forms). */
/* do_hsqueeze_step / do_vsqueeze_step (squeeze.rs:456-481, :661-682), whole plane.
 * horizontal: avg is ceil(out_w/2) x h, res floor(out_w/2) x h; vertical likewise in y.  `out` may not overlap `avg` or
 * `res` (lines are streamed: inputs are read ahead of the outputs being written). */
jxlh_status jxlh_unsqueeze(jxlh_ctx* ctx, int32_t horizontal, const int32_t* avg, size_t avg_stride,
                           const int32_t* res, size_t res_stride, uint32_t out_w, uint32_t out_h,
                           int32_t* out, size_t out_stride);

/* Batched form: the n_planes (1..3) channels one squeeze step covers (SqueezeParams::num_channels,
 * modular/transforms/squeeze.rs:20-37) in a single launch -- the recurrence is latency bound, so
 * extra planes are almost free.  All planes share geometry; device pointers only. */
jxlh_status jxlh_unsqueeze_planes(jxlh_ctx* ctx, int32_t horizontal, int32_t n_planes,
                                  const int32_t* const avg[], size_t avg_stride, const int32_t* const res[],
                                  size_t res_stride, uint32_t out_w, uint32_t out_h, int32_t* const out[],
                                  size_t out_stride);

/* Several consecutive squeeze steps in one call: level i takes the previous level's output (the base planes for
 * level 0) as its averages and levels[i].res as its residuals; only the last level's planes are written.  The first
 * levels of a chain are tiny (default_squeeze, squeeze.rs:71-105, starts from <= 8 x 8): as separate launches they cost
 * ~10 us each whatever their size, so up to 16 levels whose planes stay within 128 x 128 run as ONE launch with the
 * planes in LDS; anything else takes jxlh_unsqueeze_chain's route without an RCT (same result).  Device pointers only. */
typedef struct jxlh_squeeze_level {
  int32_t horizontal;
  uint32_t out_w, out_h;
  const int32_t* res[3]; /* floor(out_w/2) x out_h (horizontal) or out_w x floor(out_h/2); unused planes NULL */
  size_t res_stride;
} jxlh_squeeze_level;
jxlh_status jxlh_unsqueeze_levels(jxlh_ctx* ctx, int32_t n_planes, int32_t n_levels, const jxlh_squeeze_level* levels,
                                  const int32_t* const base[], size_t base_stride, uint32_t base_w, uint32_t base_h,
                                  int32_t* const out[], size_t out_stride);

/* The inverse of a WHOLE squeeze transform in one call: jxlh_unsqueeze_levels' level list (smallest level first, the
 * order the decoder applies the steps of default_squeeze / an explicit SqueezeParams list in, squeeze.rs:39-105,
 * transforms/apply.rs), optionally followed by the RCT that comes next in the transform list (rct_op 0..6 and
 * rct_perm 0..5 as in jxlh_rct, n_planes == 3; rct_op < 0: none) -- the last, full-resolution step and the RCT are
 * then one pass over the planes.  The library picks the launches (LDS-resident first levels; the streamed middle
 * levels as ONE dataflow launch in which a level starts on the rows / columns the level before it has finished;
 * fused last level); intermediate planes live in context scratch.  Device pointers only; `out` may not alias
 * the base or residual planes.  Asynchronous like every call on the context's stream; should a wait between two
 * levels of the dataflow launch ever outlast its deadline (4 s: a fault, not a load condition), the launch ends with
 * an undefined result and the next jxlh_ctx_sync returns JXLH_ERR_DEVICE.  JXLH_CHAIN_FLOW=0 in the environment
 * selects one launch per streamed level (same result; tests, A/B).
 * Layout advice (speed only, any layout is accepted): residual and output planes that start on 16-byte boundaries with
 * strides that are multiples of 4 samples are moved with 16-byte accesses (the library lays its own intermediate
 * planes out that way); other layouts take the 4-byte movers, about 1.3x the time of a streamed level. */
jxlh_status jxlh_unsqueeze_chain(jxlh_ctx* ctx, int32_t n_planes, int32_t n_levels, const jxlh_squeeze_level* levels,
                                 const int32_t* const base[], size_t base_stride, uint32_t base_w, uint32_t base_h,
                                 int32_t* const out[], size_t out_stride, int32_t rct_op, int32_t rct_perm);

/* A squeeze step of three channels followed by do_rct_step (rct.rs:118-157) on the same three channels, in one pass:
 * the shape the end of a colour image's inverse transform chain has (default_squeeze, squeeze.rs:71-105, finishes with
 * the full-size step -- vertical for square and tall images, horizontal for wide ones; the encoder applied the RCT
 * before the squeeze, so it is undone after it).  Equivalent to jxlh_unsqueeze_planes(horizontal, 3 planes) +
 * jxlh_rct(out[0..2], op, perm) without the second read and write of the image.  out planes may not alias avg / res.
 * Device pointers only. */
jxlh_status jxlh_unsqueeze_rct(jxlh_ctx* ctx, int32_t horizontal, const int32_t* const avg[3], size_t avg_stride,
                               const int32_t* const res[3], size_t res_stride, uint32_t out_w, uint32_t out_h,
                               int32_t* const out[3], size_t out_stride, int32_t op, int32_t perm);

/* smooth_h_unsqueeze / smooth_v_unsqueeze / smooth_2d_unsqueeze (modular/transforms/squeeze.rs:1010-1105, :1120-1225,
 * :908-1003): the step a squeeze runs while its residual channel has not arrived (DataStatus::Zero,
 * transforms/step.rs:138-150, dispatched at :841-851) -- the progressive previews of a squeezed image.  `avg` is the
 * WHOLE average channel (avg_w x avg_h; for JXLH_SMOOTH_2D the average of two steps back, half size in both axes);
 * the out_w x out_h output rectangle sits at (x0, y0) of the output channel -- (0, 0) and the full size for a whole
 * channel, a grid tile's Rect otherwise (the window reads across tile edges, columns clamp and rows mirror at the
 * CHANNEL's borders: TiledChannelView::load_row_to_scratch, step.rs:372-420).  As in the reference, a rectangle
 * without one complete sample pair on a doubled axis is left untouched.
 * Float-to-int conversion: the reference's `as_i32` differs between its SIMD back-ends -- truncation on the scalar,
 * NEON and wasm ones (jxl_simd/src/scalar.rs:178, aarch64/neon.rs:400, wasm32/simd128.rs:371), round-to-nearest-even
 * (cvtps2dq) on the x86 ones (x86_64/avx.rs:580, sse42.rs:472, avx512.rs:638), both applied after the +-0.5
 * (squeeze.rs:807-810, :882-883); the two differ by one on about half the samples.  The caller says which reference
 * build it stands in for: plain kind = truncation (an aarch64 / scalar reference), kind | JXLH_SMOOTH_CVT_NEAREST_EVEN
 * = an x86 reference.  Host or device pointers. */
enum { JXLH_SMOOTH_H = 0, JXLH_SMOOTH_V = 1, JXLH_SMOOTH_2D = 2, JXLH_SMOOTH_CVT_NEAREST_EVEN = 0x100 };
jxlh_status jxlh_smooth_unsqueeze(jxlh_ctx* ctx, int32_t kind, const int32_t* avg, size_t avg_stride, uint32_t avg_w,
                                  uint32_t avg_h, uint32_t x0, uint32_t y0, int32_t* out, size_t out_stride,
                                  uint32_t out_w, uint32_t out_h);

/* Progressive previews of a WHOLE squeeze transform in one call -- jxlh_unsqueeze_chain for an image whose finest
 * residual channels have not arrived: jxlh_unsqueeze_chain_preview and jxlh_squeeze_preview_kinds, declared in
 * jxl_hip_preview.h, which this header includes at its end.  jxl_hip_preview_tiles.h (included there too) is the same per
 * grid cell, for levels whose residual groups have partly arrived. */

/* ---------------------------------------------------------------- multi-GPU
 * The reference renders a frame's groups on a pool of host threads and joins them in the pipeline's output buffers
 * (frame/render.rs:395-479).  Here a frame is cut into contiguous bands of group rows, one per GPU ("rank"):
 * rank r owns group rows [r * per, min((r + 1) * per, ygroups)), per = ceil(ygroups / nranks).  Each rank gets the
 * replicated small inputs (LF, HfMetadata maps, dequant tables) and the coefficient groups of ITS band, runs the
 * transforms on exactly that band, exchanges the one block row (8 pixel rows x 3 channels, 0.8 MB at 8K) its filters
 * read across each band edge with the neighbour rank, filters its band, and the finished bands are all-gathered so
 * that every rank holds the whole frame.  Frames with upsampling run whole (JXLH_ERR_UNSUPPORTED here).
 * Chroma-subsampled frames recompute the halo group row instead of exchanging it (their chroma upsampling reads
 * across the band edge in the sub-sampled domain): for such a frame a rank must ALSO be given the coefficient
 * groups of the one group row above and the one below its band, [r * per - 1, (r + 1) * per + 1) clipped to the
 * frame; and its chroma is brought to full resolution before the gather even when no filter stage follows.
 *
 * One process per GPU (torch.distributed.run, mpirun, ...): the library owns an RCCL communicator.
 *   rank 0: jxlh_comm_unique_id(id); the launcher broadcasts the 128 bytes; every rank: jxlh_comm_init(ctx, id, rank, n)
 *   BEFORE its first jxlh_frame_begin (which sizes the planes for the in-place gather).  Per frame, every rank calls
 *   jxlh_frame_run_sharded then jxlh_frame_allgather (collectives: all ranks, same order); both only enqueue work on
 *   the context's stream (ncclSend/ncclRecv of the edge rows, ncclAllGather per plane).
 * One process driving several GPUs (or several contexts on one GPU): jxlh_comm_init_local(peers, n) makes peers[i]
 *   rank i, jxlh_frames_run_sharded_local / jxlh_frames_allgather_local drive all of them with direct device copies.
 *
 * A collective whose peer never arrives (a rank that died, calls in a different order) would park the stream for
 * ever: jxlh_ctx_sync of a context with an RCCL communicator of more than one rank therefore waits with a deadline
 * (JXLH_COMM_TIMEOUT_S, default 120; <= 0: none) and polls ncclCommGetAsyncError; on expiry it returns JXLH_ERR_DEVICE
 * and jxlh_last_error names the rank, the world size and the last collective enqueued (e.g. "halo exchange ... with
 * rank 3"). */
#define JXLH_COMM_ID_BYTES 128
jxlh_status jxlh_comm_unique_id(uint8_t id[JXLH_COMM_ID_BYTES]);
jxlh_status jxlh_comm_init(jxlh_ctx* ctx, const uint8_t id[JXLH_COMM_ID_BYTES], int32_t rank, int32_t nranks);
jxlh_status jxlh_comm_init_local(jxlh_ctx* const peers[], int32_t nranks);
jxlh_status jxlh_comm_destroy(jxlh_ctx* ctx);
/* rank / nranks of the context (0 / 1 without a communicator) and, inside a frame, the band of group rows it owns;
 * any output pointer may be NULL */
jxlh_status jxlh_comm_band(jxlh_ctx* ctx, int32_t* rank, int32_t* nranks, uint32_t* group_row0, uint32_t* group_row1);
jxlh_status jxlh_frame_run_sharded(jxlh_ctx* ctx);
jxlh_status jxlh_frame_allgather(jxlh_ctx* ctx);
jxlh_status jxlh_frames_run_sharded_local(jxlh_ctx* const peers[], int32_t nranks);
jxlh_status jxlh_frames_allgather_local(jxlh_ctx* const peers[], int32_t nranks);
/* The gather of the CONVERTED image instead of the f32 planes (round 6): every rank runs the frame's colour stage +
 * integer conversion (jxlh_frame_read_output's stages: XybStage / FromLinearStage / ConvertF32ToU8 / U16) on the pixel
 * rows of ITS band, writes them interleaved into `out` -- a DEVICE buffer of at least nranks * per * 256 *
 * bytes_per_row bytes (per = the band height in group rows, jxlh_comm_band) that holds the whole image, row y at
 * y * bytes_per_row -- and the bands are all-gathered in place: 201 MB for an 8K RGB8 image instead of the 805 MB of
 * jxlh_frame_allgather.  Replaces jxlh_frame_allgather (call one of the two after jxlh_frame_run_sharded; same rules:
 * all ranks, same order, work only enqueued on the context's stream).  Frames without upsampling / noise, like every
 * sharded run. */
jxlh_status jxlh_frame_allgather_output(jxlh_ctx* ctx, const jxlh_output_desc* d, void* out, size_t bytes_per_row);
/* the same for an in-process group: outs[i] = rank i's image buffer */
jxlh_status jxlh_frames_allgather_output_local(jxlh_ctx* const peers[], int32_t nranks, const jxlh_output_desc* d,
                                               void* const outs[], size_t bytes_per_row);
/* In-place all-gather of a device buffer of nranks * bytes_per_rank bytes (rank r's part at r * bytes_per_rank), on the
 * context's stream: the join of band-sharded Modular work (RCT / Palette on row bands of whole planes). */
jxlh_status jxlh_comm_allgather(jxlh_ctx* ctx, void* buf, size_t bytes_per_rank);
/* the same for an in-process group: bufs[i] = rank i's copy of the buffer */
jxlh_status jxlh_comm_allgather_local(jxlh_ctx* const peers[], int32_t nranks, void* const bufs[], size_t bytes_per_rank);
/* Modular across GPUs.  RCT and the non-delta Palette are per-sample: a rank runs jxlh_rct /
 * jxlh_palette on its contiguous share of the samples (any split the caller likes; jxl_rs_amd/shard.py uses
 * ceil(n / nranks) rounded up to 4 samples so that every share starts 16-byte aligned) and the planes are joined with
 * jxlh_comm_allgather.  Squeeze is NOT sharded: the recurrence along a line is a serial dependency chain, and the
 * kernel's time is that chain's latency (one full-resolution vertical step takes 0.46 ms for one plane and for three,
 * profiles/r02_h_modular.txt) -- giving each GPU fewer lines leaves the chain as long as it was, so N GPUs run N
 * images (or the channels of one) as replicas instead. */

/* Gaborish / EPF on a Modular frame (a lossless or lossy-modular frame whose restoration filter is on): the stage list
 * of frame/render.rs:569-622 on three f32 planes the caller holds on the device (the output of jxlh_modular_to_f32 /
 * jxlh_modular_xyb_to_f32), with the CONSTANT sigma of features/epf.rs:81-84 -- INV_SIGMA_NUM / epf_sigma_for_modular
 * for every pixel -- instead of the per-block map a VarDCT frame derives from its quantisation field.  Uses gab, gab_w*,
 * epf_iters and the epf_* fields of p; w x h samples per plane, row stride `stride` floats (a multiple of 4; planes
 * 16-byte aligned); the result is written to out[], in[] may be overwritten (epf_iters == 3). */
jxlh_status jxlh_modular_frame_filters(jxlh_ctx* ctx, const jxlh_frame_params* p, float* const in[3],
                                       float* const out[3], uint32_t w, uint32_t h, size_t stride);

/* library info */
uint32_t jxlh_abi_version(void);
/* covered_blocks_x / _y and the type -> dequant table map (transform_map.rs:97-107,
 * quant_weights.rs:321-343), for hosts that build coefficient slabs */
int32_t jxlh_covered_blocks_x(int32_t type);
int32_t jxlh_covered_blocks_y(int32_t type);
int32_t jxlh_quant_table_for_type(int32_t type);
int32_t jxlh_quant_table_size(int32_t table);

#ifdef __cplusplus
}
#endif
/* entry points added since ABI version 6 was recorded, in headers of their own: part of this interface all the same */
#include "jxl_hip_preview.h"
#include "jxl_hip_save_rects.h"
#include "jxl_hip_preview_tiles.h"
#include "jxl_hip_extra_rects.h"
#include "jxl_hip_repaint.h"
#include "jxl_hip_blend_rects.h"
/* ... and this one brings jxl_hip_local_squeeze.h and jxl_hip_local_palette.h, whose group form it takes: whichever of the
 * four a translation unit names first, it gets the whole interface */
#include "jxl_hip_local_extra.h"

#endif /* JXL_HIP_H_ */
