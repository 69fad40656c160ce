// C++ host side over the C ABI of include/jxl_hip.h: the calls a jxl-rs maintainer's shim makes, under the names of
// the reference functions they replace, with RAII and exceptions instead of status codes.  Header-only, no HIP or
// torch types: links against libjxl_hip.so only.  (The reference is Rust; INTEGRATION.md shows the same surface as an
// `extern "C"` block and a `RenderPipeline` implementation.  This header is what the compiled-language parity test
// tests/cpp/frame_parity.cc drives.)
//
//   reference (jxl/src/...)                                   here
//   Frame::from_header_and_toc + prepare_render_pipeline      VarDctFrame::begin            frame/decode.rs:172-204, frame/render.rs:907
//   decode_hf_global (dequant matrices)                       VarDctFrame::decode_hf_global frame/quant_weights.rs:347-351
//   decode_lf_group -> dequant_lf                             VarDctFrame::decode_lf_group  frame/modular/mod.rs:837-929
//   decode_hf_metadata                                        VarDctFrame::decode_hf_metadata  frame/modular/mod.rs:984-1081
//   decode_vardct_group (entropy loop stays on the host)      VarDctFrame::decode_vardct_group[_sparse]  frame/group.rs:509-613
//   finalize_lf, SigmaSource::new, the render pipeline        VarDctFrame::finalize_and_render  frame/mod.rs:360-378, frame/render.rs:569-683
//   pipeline output (save stages)                             VarDctFrame::read_planes / read_rgb8 / read_output
#pragma once
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "jxl_hip.h"
#include "jxl_hip_local_palette.h"
#include "jxl_hip_local_squeeze.h"
#include "jxl_hip_local_extra.h"

namespace jxlh {

class Error : public std::runtime_error {  // -> Error::Gpu(code) on the Rust side
 public:
  Error(jxlh_status st, const char* where, const std::string& detail)
      : std::runtime_error(std::string(where) + ": " + jxlh_status_string(st) + (detail.empty() ? "" : " / " + detail)),
        status(st) {}
  jxlh_status status;
};

class Context {
 public:
  explicit Context(int device = 0, int n_slots = 1) : n_slots_(n_slots) {
    const jxlh_status st = jxlh_ctx_create(device, n_slots, &c_);
    if (st != JXLH_OK) throw Error(st, "jxlh_ctx_create", "");
  }
  ~Context() { jxlh_ctx_destroy(c_); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  jxlh_ctx* raw() const { return c_; }
  int n_slots() const { return n_slots_; }
  void check(jxlh_status st, const char* where) const {
    if (st != JXLH_OK) throw Error(st, where, jxlh_last_error(c_));
  }
  void sync() { check(jxlh_ctx_sync(c_), "jxlh_ctx_sync"); }
  void* alloc_pinned(size_t bytes) {
    void* p = nullptr;
    check(jxlh_alloc_pinned(c_, bytes, &p), "jxlh_alloc_pinned");
    return p;
  }
  void free_pinned(void* p) { check(jxlh_free_pinned(c_, p), "jxlh_free_pinned"); }
  // DecoderState::reference_frames[slot] <- n_channels planes (w x h, row stride `stride` floats, host or device)
  void set_reference(uint32_t slot, const std::vector<const float*>& planes, uint32_t w, uint32_t h, size_t stride) {
    check(jxlh_ctx_set_reference(c_, slot, (uint32_t)planes.size(), w, h, planes.data(), stride), "jxlh_ctx_set_reference");
  }
  void clear_reference(uint32_t slot) { check(jxlh_ctx_clear_reference(c_, slot), "jxlh_ctx_clear_reference"); }
  // LF slots (DecoderState::lf_frames): an LF frame's X, Y, B planes from the caller / from the rendered frame; a VarDCT
  // frame's LF image from a slot (slot = that frame's lf_level); the full-size preview of one rect of a slot
  void set_lf_frame(uint32_t slot, uint32_t w, uint32_t h, const float* x, const float* y, const float* b, size_t stride) {
    check(jxlh_ctx_set_lf_frame(c_, slot, w, h, x, y, b, stride), "jxlh_ctx_set_lf_frame");
  }
  void save_lf(uint32_t slot) { check(jxlh_frame_save_lf(c_, slot), "jxlh_frame_save_lf"); }
  void clear_lf_frame(uint32_t slot) { check(jxlh_ctx_clear_lf_frame(c_, slot), "jxlh_ctx_clear_lf_frame"); }
  void set_lf_from_slot(uint32_t slot) { check(jxlh_frame_set_lf_from_slot(c_, slot), "jxlh_frame_set_lf_from_slot"); }
  void lf_preview(uint32_t slot, uint32_t image_w, uint32_t image_h, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                  const jxlh_output_desc& colour, const jxlh_save_desc& save, void* out, size_t bytes_per_row) {
    check(jxlh_lf_preview(c_, slot, image_w, image_h, x0, y0, w, h, &colour, &save, out, bytes_per_row), "jxlh_lf_preview");
  }
  // the current frame's patch dictionary on caller planes (3 + num_ec), in place
  void stage_patches(const std::vector<float*>& planes, uint32_t w, uint32_t h, size_t stride) {
    check(jxlh_stage_patches(c_, planes.data(), (uint32_t)planes.size(), w, h, stride), "jxlh_stage_patches");
  }
  // the current frame's spline segments drawn onto three caller planes, in place
  void stage_splines(float* const planes[3], uint32_t w, uint32_t h, size_t stride) {
    check(jxlh_stage_splines(c_, planes, w, h, stride), "jxlh_stage_splines");
  }
  // the inverse of a whole squeeze transform on device planes (levels smallest first; base / out: one pointer per
  // channel, 1..3), with the RCT that follows it fused into the last level (rct_op < 0: none): jxlh_unsqueeze_chain
  void unsqueeze_chain(const std::vector<jxlh_squeeze_level>& levels, const std::vector<const int32_t*>& base, size_t base_stride,
                       uint32_t base_w, uint32_t base_h, const std::vector<int32_t*>& out, size_t out_stride, int32_t rct_op = -1,
                       int32_t rct_perm = 0) {
    if (base.size() != out.size()) throw Error(JXLH_ERR_INVALID_ARGUMENT, "Context::unsqueeze_chain", "base and out planes differ in number");
    check(jxlh_unsqueeze_chain(c_, (int32_t)base.size(), (int32_t)levels.size(), levels.data(), base.data(), base_stride, base_w,
                               base_h, out.data(), out_stride, rct_op, rct_perm),
          "jxlh_unsqueeze_chain");
  }
  // ... while the finest residual channels have not arrived: a level with res[] all null runs the reference's smooth step
  // (SqueezeStepKind::Upsample1D / Upsample2D, transforms/step.rs:138-150).  nearest_even: the preview of an x86 reference
  // build (JXLH_SMOOTH_CVT_NEAREST_EVEN)
  void unsqueeze_chain_preview(const std::vector<jxlh_squeeze_level>& levels, const std::vector<const int32_t*>& base,
                               size_t base_stride, uint32_t base_w, uint32_t base_h, const std::vector<int32_t*>& out,
                               size_t out_stride, int32_t rct_op = -1, int32_t rct_perm = 0, bool nearest_even = false) {
    if (base.size() != out.size())
      throw Error(JXLH_ERR_INVALID_ARGUMENT, "Context::unsqueeze_chain_preview", "base and out planes differ in number");
    check(jxlh_unsqueeze_chain_preview(c_, (int32_t)base.size(), (int32_t)levels.size(), levels.data(), base.data(), base_stride,
                                       base_w, base_h, out.data(), out_stride, rct_op, rct_perm,
                                       nearest_even ? (uint32_t)JXLH_SMOOTH_CVT_NEAREST_EVEN : 0u),
          "jxlh_unsqueeze_chain_preview");
  }
  // ... while the residual GROUPS of some levels have partly arrived: tiles[L] is level L's grid and the host mask of the
  // cells whose residuals are there (jxl_hip_preview_tiles.h); the reference's per-cell choice (SqueezeInfo::new)
  void unsqueeze_chain_preview_tiles(const std::vector<jxlh_squeeze_level>& levels, const std::vector<jxlh_squeeze_tiles>& tiles,
                                     const std::vector<const int32_t*>& base, size_t base_stride, uint32_t base_w, uint32_t base_h,
                                     const std::vector<int32_t*>& out, size_t out_stride, int32_t rct_op = -1, int32_t rct_perm = 0,
                                     bool nearest_even = false) {
    if (base.size() != out.size() || tiles.size() != levels.size())
      throw Error(JXLH_ERR_INVALID_ARGUMENT, "Context::unsqueeze_chain_preview_tiles", "planes or grids differ in number");
    check(jxlh_unsqueeze_chain_preview_tiles(c_, (int32_t)base.size(), (int32_t)levels.size(), levels.data(), tiles.data(), base.data(),
                                             base_stride, base_w, base_h, out.data(), out_stride, rct_op, rct_perm,
                                             nearest_even ? (uint32_t)JXLH_SMOOTH_CVT_NEAREST_EVEN : 0u),
          "jxlh_unsqueeze_chain_preview_tiles");
  }
  // the save tail on caller planes (3 + num_ec, host or device) for a list of source rectangles: jxlh_stage_save_rects
  void stage_save_rects(const jxlh_output_desc* colour, const jxlh_save_desc& save, const std::vector<const float*>& planes,
                        uint32_t w, uint32_t h, size_t stride, uint32_t frame_x0, uint32_t frame_y0,
                        const std::vector<jxlh_rect>& rects, void* out, size_t bytes_per_row) {
    check(jxlh_stage_save_rects(c_, colour, &save, planes.data(), (uint32_t)planes.size(), w, h, stride, frame_x0, frame_y0,
                                rects.data(), (uint32_t)rects.size(), out, bytes_per_row),
          "jxlh_stage_save_rects");
  }

 private:
  jxlh_ctx* c_ = nullptr;
  int n_slots_ = 1;
};

// the rectangles of a frame's result that re-rendering `groups` can change (jxlh_changed_rects): host only
inline std::vector<jxlh_rect> changed_rects(const jxlh_frame_params& p, const std::vector<uint32_t>& groups) {
  uint32_t n = 0;
  jxlh_status st = jxlh_changed_rects(&p, groups.data(), (uint32_t)groups.size(), nullptr, 0, &n);
  std::vector<jxlh_rect> rects(n);
  if (n) st = jxlh_changed_rects(&p, groups.data(), (uint32_t)groups.size(), rects.data(), n, &n);
  if (st != JXLH_OK) throw Error(st, "jxlh_changed_rects", "");
  return rects;
}

// the rectangles of a frame's RESULT (upsampled size) that repainting `groups` can change, on any kind of frame
// (jxlh_repaint_changed_rects): host only
inline std::vector<jxlh_rect> repaint_changed_rects(const jxlh_frame_params& p, const std::vector<uint32_t>& groups) {
  uint32_t n = 0;
  jxlh_status st = jxlh_repaint_changed_rects(&p, groups.data(), (uint32_t)groups.size(), nullptr, 0, &n);
  std::vector<jxlh_rect> rects(n);
  if (n) st = jxlh_repaint_changed_rects(&p, groups.data(), (uint32_t)groups.size(), rects.data(), n, &n);
  if (st != JXLH_OK) throw Error(st, "jxlh_repaint_changed_rects", "");
  return rects;
}

// the rectangles of a finished extra channel (w x h samples, factor ec_upsampling, cut to res_w x res_h) outside which
// new samples in `rects` (source samples) change nothing (jxlh_extra_channel_changed_rects): host only
inline std::vector<jxlh_rect> extra_channel_changed_rects(uint32_t w, uint32_t h, uint32_t ec_upsampling, uint32_t res_w,
                                                          uint32_t res_h, const std::vector<jxlh_rect>& rects) {
  uint32_t n = 0;
  std::vector<jxlh_rect> out(rects.size());
  const jxlh_status st = jxlh_extra_channel_changed_rects(w, h, ec_upsampling, res_w, res_h, rects.data(), (uint32_t)rects.size(),
                                                          out.data(), (uint32_t)out.size(), &n);
  if (st != JXLH_OK) throw Error(st, "jxlh_extra_channel_changed_rects", "");
  return out;
}

// rects of a frame_w x frame_h result (what the three *_changed_rects functions return) as rects of the image `desc`
// composes the frame onto: shifted by the frame's origin, clipped to the image, empty ones dropped
// (jxlh_blend_image_rects): host only.  The list VarDctFrame::blend_rects and, after it, save_rects take
inline std::vector<jxlh_rect> blend_image_rects(const jxlh_blend_desc& desc, uint32_t frame_w, uint32_t frame_h,
                                                const std::vector<jxlh_rect>& rects) {
  uint32_t n = 0;
  std::vector<jxlh_rect> out(rects.size());  // never more than came in
  const jxlh_status st = jxlh_blend_image_rects(&desc, frame_w, frame_h, rects.data(), (uint32_t)rects.size(), out.data(),
                                                (uint32_t)out.size(), &n);
  if (st != JXLH_OK) throw Error(st, "jxlh_blend_image_rects", "");
  out.resize(n);
  return out;
}

// what each level of a preview chain runs (JXLH_PREVIEW_*) and whether the final planes depend on it: host only
struct SqueezePreviewKinds {
  std::vector<uint8_t> kinds, live;
};
inline SqueezePreviewKinds squeeze_preview_kinds(int n_planes, const std::vector<jxlh_squeeze_level>& levels, uint32_t base_w,
                                                 uint32_t base_h) {
  SqueezePreviewKinds r{std::vector<uint8_t>(levels.size()), std::vector<uint8_t>(levels.size())};
  const jxlh_status st =
      jxlh_squeeze_preview_kinds(n_planes, (int32_t)levels.size(), levels.data(), base_w, base_h, r.kinds.data(), r.live.data());
  if (st != JXLH_OK) throw Error(st, "jxlh_squeeze_preview_kinds", "");
  return r;
}
// ... per grid cell: the kinds of the tiles_x * tiles_y cells of `level`, row by row: host only
inline std::vector<uint8_t> squeeze_tile_kinds(int n_planes, const std::vector<jxlh_squeeze_level>& levels,
                                               const std::vector<jxlh_squeeze_tiles>& tiles, uint32_t base_w, uint32_t base_h, int32_t level) {
  if (tiles.size() != levels.size() || level < 0 || (size_t)level >= levels.size())
    throw Error(JXLH_ERR_INVALID_ARGUMENT, "squeeze_tile_kinds", "one grid per level, and a level of the chain");
  const jxlh_squeeze_tiles& t = tiles[level];
  const uint32_t tw = t.tile_w ? t.tile_w : levels[level].out_w, th = t.tile_h ? t.tile_h : levels[level].out_h;
  const uint64_t cells = tw && th ? (uint64_t)((levels[level].out_w + tw - 1) / tw) * ((levels[level].out_h + th - 1) / th) : 1;
  if (cells > (1u << 20)) throw Error(JXLH_ERR_INVALID_ARGUMENT, "squeeze_tile_kinds", "more than 2^20 cells in a level");
  std::vector<uint8_t> kinds((size_t)cells);
  const jxlh_status st = jxlh_squeeze_tile_kinds(n_planes, (int32_t)levels.size(), levels.data(), tiles.data(), base_w, base_h, level, kinds.data());
  if (st != JXLH_OK) throw Error(st, "jxlh_squeeze_tile_kinds", "");
  return kinds;
}

// One VarDCT frame on the device: the order of calls is the order of Frame's sections in the codestream.
class VarDctFrame {
 public:
  static jxlh_frame_params default_params(uint32_t xsize, uint32_t ysize) {
    jxlh_frame_params p;
    const jxlh_status st = jxlh_default_frame_params(&p, xsize, ysize);
    if (st != JXLH_OK) throw Error(st, "jxlh_default_frame_params", "");
    return p;
  }
  VarDctFrame(Context& ctx, const jxlh_frame_params& p) : ctx_(ctx), p_(p) {
    ctx_.check(jxlh_frame_begin(ctx_.raw(), &p_), "jxlh_frame_begin");
  }
  const jxlh_frame_params& params() const { return p_; }

  void decode_hf_global(const std::array<std::vector<float>, JXLH_NUM_QUANT_TABLES>& tables) {
    const float* ptr[JXLH_NUM_QUANT_TABLES];
    size_t n[JXLH_NUM_QUANT_TABLES];
    for (int t = 0; t < JXLH_NUM_QUANT_TABLES; t++) {
      ptr[t] = tables[t].data();
      n[t] = tables[t].size() / 3;
    }
    ctx_.check(jxlh_frame_set_dequant_tables(ctx_.raw(), ptr, n), "jxlh_frame_set_dequant_tables");
  }
  // rect in blocks; the three modular channels in coded order Y, X, B
  void decode_lf_group(uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const int32_t* qy, const int32_t* qx,
                       const int32_t* qb, size_t stride, uint32_t extra_precision = 0) {
    ctx_.check(jxlh_frame_set_lf_quantized(ctx_.raw(), x0, y0, w, h, qy, qx, qb, stride, extra_precision),
               "jxlh_frame_set_lf_quantized");
  }
  void decode_hf_metadata(uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const uint8_t* transform_map,
                          const int32_t* raw_quant, const uint8_t* epf_map, size_t map_stride, const int8_t* ytox,
                          const int8_t* ytob, size_t cmap_stride) {
    ctx_.check(jxlh_frame_set_hf_meta(ctx_.raw(), x0, y0, w, h, transform_map, raw_quant, epf_map, map_stride, ytox, ytob,
                                      cmap_stride),
               "jxlh_frame_set_hf_meta");
  }
  // the group's dense coefficient slab (3 x 65536 i32) as decode_vardct_group fills it; asynchronous per slot
  void decode_vardct_group(uint32_t group, const int32_t* coeffs, int slot = 0) {
    ctx_.check(jxlh_submit_group(ctx_.raw(), slot, group, coeffs, JXLH_GROUP_COMPLETE), "jxlh_submit_group");
  }
  // ... or the (position, value) updates its entropy loop produces (frame/group.rs:557-572)
  void decode_vardct_group_sparse(uint32_t group, const jxlh_coeff16* pairs, const uint32_t n[3],
                                  const jxlh_coeff32* wide = nullptr, uint32_t n_wide = 0, int slot = 0) {
    ctx_.check(jxlh_submit_group_sparse(ctx_.raw(), slot, group, pairs, n, wide, n_wide, JXLH_GROUP_COMPLETE),
               "jxlh_submit_group_sparse");
  }
  void slot_wait(int slot = 0) { ctx_.check(jxlh_slot_wait(ctx_.raw(), slot), "jxlh_slot_wait"); }
  // upsample_lf_group (frame/decode.rs:51-158) for the groups listed: they have no HF yet, and the next render fills them
  // from the LF image upsampled 8x instead of transforming them; a group's later decode_vardct_group* clears its mark
  void upsample_lf_groups(const uint32_t* groups, uint32_t n) {
    ctx_.check(jxlh_frame_set_groups_lf_only(ctx_.raw(), groups, n), "jxlh_frame_set_groups_lf_only");
  }
  // a frame begun with JXLH_FRAME_MODULAR takes samples instead of LF, HF metadata and coefficients: one rect of the
  // three colour channels as the inverse transforms left them (jxlh_frame_set_modular_channels)
  void set_modular_channels(uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const int32_t* const planes[3], size_t stride,
                            uint32_t sample_format) {
    ctx_.check(jxlh_frame_set_modular_channels(ctx_.raw(), x0, y0, w, h, planes[0], planes[1], planes[2], stride, sample_format),
               "jxlh_frame_set_modular_channels");
  }
  // ... or the channels of many groups AS DECODED plus each group's local transform list (decode_modular_section's
  // output instead of TransformStep::local_apply): RCTs and palettes run on the device, one launch for the batch.  The
  // arena (host or device memory) may be reused when the call returns; with async = true, after the next sync / mark.
  void set_modular_groups(const int32_t* arena, uint64_t arena_samples, const jxlh_local_group* groups, size_t n,
                          uint32_t sample_format, bool async = false) {
    size_t bad = 0;
    ctx_.check(async ? jxlh_frame_set_modular_groups_async(ctx_.raw(), arena, arena_samples, groups, n, sample_format, &bad)
                     : jxlh_frame_set_modular_groups(ctx_.raw(), arena, arena_samples, groups, n, sample_format, &bad),
               "jxlh_frame_set_modular_groups");
  }
  // ... with EVERY local palette on the device (jxl_hip_local_palette.h): delta entries and all 14 predictors.  wp: one
  // GroupHeader::wp_header per group, or null when no step has predictor 6; it is read before the call returns.
  void set_modular_groups_general(const int32_t* arena, uint64_t arena_samples, const jxlh_local_group* groups,
                                  const jxlh_wp_header* wp, size_t n, uint32_t sample_format, bool async = false) {
    size_t bad = 0;
    ctx_.check(async ? jxlh_frame_set_modular_groups_general_async(ctx_.raw(), arena, arena_samples, groups, wp, n, sample_format, &bad)
                     : jxlh_frame_set_modular_groups_general(ctx_.raw(), arena, arena_samples, groups, wp, n, sample_format, &bad),
               "jxlh_frame_set_modular_groups_general");
  }
  // ... and with local squeezes (jxl_hip_local_squeeze.h): self-contained groups whose coded channels and squeeze
  // parameters are ranges of the call-wide `coded` and `params` arrays; all of them are read before the call returns.
  void set_modular_groups_squeeze(const int32_t* arena, uint64_t arena_samples, const jxlh_local_squeeze_group* groups, size_t n,
                                  const jxlh_local_coded_channel* coded, size_t n_coded, const jxlh_squeeze_params* params,
                                  size_t n_params, const jxlh_wp_header* wp, uint32_t sample_format, bool async = false) {
    size_t bad = 0;
    ctx_.check(async ? jxlh_frame_set_modular_groups_squeeze_async(ctx_.raw(), arena, arena_samples, groups, n, coded, n_coded, params,
                                                                   n_params, wp, sample_format, &bad)
                     : jxlh_frame_set_modular_groups_squeeze(ctx_.raw(), arena, arena_samples, groups, n, coded, n_coded, params,
                                                             n_params, wp, sample_format, &bad),
               "jxlh_frame_set_modular_groups_squeeze");
  }
  // ... and for groups that hold extra channels behind (or instead of) the colour (jxl_hip_local_extra.h): RGBA, grey +
  // alpha, the alpha / depth / spot channels of a VarDCT frame.  Every finished channel goes where the frame keeps it;
  // the named extra channels are "not rendered" until the next run, rerender or repaint.  dest is read before the call
  // returns.
  void set_modular_groups_extra(const int32_t* arena, uint64_t arena_samples, const jxlh_local_squeeze_group* groups, size_t n,
                                const jxlh_local_coded_channel* coded, size_t n_coded, const jxlh_squeeze_params* params,
                                size_t n_params, const jxlh_wp_header* wp, uint32_t sample_format, const jxlh_local_dest& dest,
                                bool async = false) {
    size_t bad = 0;
    ctx_.check(async ? jxlh_frame_set_modular_groups_extra_async(ctx_.raw(), arena, arena_samples, groups, n, coded, n_coded, params,
                                                                 n_params, wp, sample_format, &dest, &bad)
                     : jxlh_frame_set_modular_groups_extra(ctx_.raw(), arena, arena_samples, groups, n, coded, n_coded, params,
                                                           n_params, wp, sample_format, &dest, &bad),
               "jxlh_frame_set_modular_groups_extra");
  }
  // An extra channel that arrives group by group (jxl_hip_extra_rects.h): declared once per frame, all zero ...
  void begin_extra_channel(uint32_t ec, uint32_t w, uint32_t h, uint32_t bits_per_sample, uint32_t ec_upsampling) {
    ctx_.check(jxlh_frame_begin_extra_channel(ctx_.raw(), ec, w, h, bits_per_sample, ec_upsampling), "jxlh_frame_begin_extra_channel");
  }
  // ... then the rects of its samples as their groups arrive, many per call, out of one block (host or device memory);
  // the next finalize_and_render() / rerender_groups() converts and upsamples only what they can have changed.  The
  // block may be reused when the call returns; _async: after the next sync / mark.
  void set_extra_channel_rects(const int32_t* samples, uint64_t n_samples, const std::vector<jxlh_ec_rect>& rects) {
    uint32_t bad = 0;
    ctx_.check(jxlh_frame_set_extra_channel_rects(ctx_.raw(), samples, n_samples, rects.data(), (uint32_t)rects.size(), &bad),
               "jxlh_frame_set_extra_channel_rects");
  }
  void set_extra_channel_rects_async(const int32_t* samples, uint64_t n_samples, const std::vector<jxlh_ec_rect>& rects) {
    uint32_t bad = 0;
    ctx_.check(jxlh_frame_set_extra_channel_rects_async(ctx_.raw(), samples, n_samples, rects.data(), (uint32_t)rects.size(), &bad),
               "jxlh_frame_set_extra_channel_rects_async");
  }
  // PatchesDictionary::read's result (decode_lf_global, frame/decode.rs:315-324), flattened: blendings holds
  // patches.size() * (1 + ec_flags.size()) entries, ec_flags the JXLH_EC_* of each extra channel
  void decode_patches(const std::vector<jxlh_patch>& patches, const std::vector<jxlh_patch_blending>& blendings,
                      const std::vector<uint32_t>& ec_flags) {
    if (blendings.size() != patches.size() * (1 + ec_flags.size()))
      throw Error(JXLH_ERR_INVALID_ARGUMENT, "VarDctFrame::decode_patches", "blendings != patches * (1 + num_ec)");
    ctx_.check(jxlh_frame_set_patches(ctx_.raw(), patches.data(), (uint32_t)patches.size(), blendings.data(),
                                      (uint32_t)ec_flags.size(), ec_flags.data()),
               "jxlh_frame_set_patches");
  }
  // Splines::initialize_draw_cache's result (frame/render.rs:652-653 hands it to SplinesStage): the draw cache's
  // segments, in its order
  void set_spline_segments(const std::vector<jxlh_spline_segment>& segments) {
    ctx_.check(jxlh_frame_set_splines(ctx_.raw(), segments.data(), (uint32_t)segments.size()), "jxlh_frame_set_splines");
  }
  // ... or the splines as Splines::read leaves them (decode_lf_global): built into segments on the host
  // (jxlh_splines_build_segments) with the frame's size and its LF colour correlation, then set.  Returns the segments.
  std::vector<jxlh_spline_segment> decode_splines(const std::vector<jxlh_quantized_spline>& splines,
                                                  int32_t quantization_adjustment, bool high_precision = false) {
    // the size is header.size(), the coded size also of an upsampled frame (frame/decode.rs:372-377): p_.xsize / ysize
    // ColorCorrelationParams::y_to_x_lf / y_to_b_lf (frame/color_correlation_map.rs:81-93)
    const float y_to_x_lf = p_.base_correlation_x + (float)p_.ytox_lf / (float)p_.color_factor;
    const float y_to_b_lf = p_.base_correlation_b + (float)p_.ytob_lf / (float)p_.color_factor;
    size_t n = 0;
    ctx_.check(jxlh_splines_build_segments(splines.data(), (uint32_t)splines.size(), quantization_adjustment, y_to_x_lf,
                                           y_to_b_lf, p_.xsize, p_.ysize, high_precision ? 1u : 0u, nullptr, 0, &n),
               "jxlh_splines_build_segments");
    std::vector<jxlh_spline_segment> seg(n);
    ctx_.check(jxlh_splines_build_segments(splines.data(), (uint32_t)splines.size(), quantization_adjustment, y_to_x_lf,
                                           y_to_b_lf, p_.xsize, p_.ysize, high_precision ? 1u : 0u, seg.data(), n, &n),
               "jxlh_splines_build_segments");
    set_spline_segments(seg);
    return seg;
  }
  // the save_before_ct save stage: the rendered frame becomes reference frame `slot`
  void save_reference(uint32_t slot) { ctx_.check(jxlh_frame_save_reference(ctx_.raw(), slot), "jxlh_frame_save_reference"); }
  // an LF frame's result into LF slot lf_level - 1 (frame/mod.rs:399-401)
  void save_lf(uint32_t slot) { ctx_.check(jxlh_frame_save_lf(ctx_.raw(), slot), "jxlh_frame_save_lf"); }
  // the colour stage (null: none), BlendingStage and ExtendToImageDimensionsStage (frame/render.rs:754-771): the rendered
  // frame composed onto the image from the reference slots; the image becomes what the read calls and save_reference see
  void blend(const jxlh_blend_desc& desc, const jxlh_output_desc* colour = nullptr) {
    ctx_.check(jxlh_frame_blend(ctx_.raw(), &desc, colour), "jxlh_frame_blend");
    blend_w_ = desc.image_w;
    blend_h_ = desc.image_h;
  }
  // After a re-render of a frame blend() has composed: only the listed rectangles of the IMAGE (blend_image_rects) are
  // composed again, in the canvas blend() left; the image is the frame's result again (jxlh_frame_blend_rects).  Same
  // descriptor and colour stage as the blend(); every pixel an input of which changed must lie in a rect
  void blend_rects(const jxlh_blend_desc& desc, const std::vector<jxlh_rect>& rects, const jxlh_output_desc* colour = nullptr) {
    ctx_.check(jxlh_frame_blend_rects(ctx_.raw(), &desc, colour, rects.data(), (uint32_t)rects.size()), "jxlh_frame_blend_rects");
    blend_w_ = desc.image_w;
    blend_h_ = desc.image_h;
  }
  // finalize_lf + SigmaSource::new + transforms + the frame's stage list, for group rows [row0, row1)
  void finalize_and_render(uint32_t group_row0 = 0, uint32_t group_row1 = 0xFFFFFFFFu) {
    blend_w_ = blend_h_ = 0;  // a render discards the composition
    ctx_.check(jxlh_frame_run(ctx_.raw(), group_row0, group_row1), "jxlh_frame_run");
  }
  // The listed cells of the 256 grid over the coded size again, behind a whole finalize_and_render(), on every kind of
  // unsharded frame -- upsampled and Modular frames included (jxlh_frame_repaint_groups); before any whole render it is one
  void repaint_groups(const std::vector<uint32_t>& groups) {
    if (!groups.empty()) blend_w_ = blend_h_ = 0;
    ctx_.check(jxlh_frame_repaint_groups(ctx_.raw(), groups.data(), (uint32_t)groups.size()), "jxlh_frame_repaint_groups");
  }
  // tight f32 planes X, Y, B of out_width() x out_height()
  void read_planes(float* x, float* y, float* b) {
    const size_t w = out_width(), h = out_height();
    const jxlh_plane pl[3] = {{x, w * sizeof(float), h, w * sizeof(float)},
                              {y, w * sizeof(float), h, w * sizeof(float)},
                              {b, w * sizeof(float), h, w * sizeof(float)}};
    ctx_.check(jxlh_frame_read_planes(ctx_.raw(), pl), "jxlh_frame_read_planes");
  }
  // one 256 x 256 group of the result per channel, the unit RenderPipeline::set_buffer_for_group moves
  // (render/mod.rs:124-137); buffers of `pitch` floats per row, at least the group's size rounded up to 16 pixels
  void read_group_planes(uint32_t group, float* x, float* y, float* b, size_t pitch, size_t rows) {
    const uint32_t xg = (out_width() + JXLH_GROUP_DIM - 1) / JXLH_GROUP_DIM;
    const jxlh_plane pl[3] = {{x, pitch * sizeof(float), rows, pitch * sizeof(float)},
                              {y, pitch * sizeof(float), rows, pitch * sizeof(float)},
                              {b, pitch * sizeof(float), rows, pitch * sizeof(float)}};
    ctx_.check(jxlh_frame_read_planes_rect(ctx_.raw(), (group % xg) * JXLH_GROUP_DIM, (group / xg) * JXLH_GROUP_DIM,
                                           JXLH_GROUP_DIM, JXLH_GROUP_DIM, pl),
               "jxlh_frame_read_planes_rect");
  }
  void read_rgb8(const jxlh_xyb_params& xyb, uint32_t channels, uint8_t* out) {
    ctx_.check(jxlh_frame_read_rgb8(ctx_.raw(), &xyb, channels, 0, out_height(), out, (size_t)out_width() * channels),
               "jxlh_frame_read_rgb8");
  }
  void read_output(const jxlh_output_desc& d, void* out) {
    ctx_.check(jxlh_frame_read_output(ctx_.raw(), &d, 0, out_height(), out,
                                      (size_t)out_width() * d.channels * (d.bits / 8)),
               "jxlh_frame_read_output");
  }
  // the save tail (jxlh_frame_save): rows [y0, y1) of the result through spot colours, premultiplication, conversion and
  // orientation into the oriented image at `out`; colour = the colour stage in front (nullptr after blend())
  void save(const jxlh_output_desc* colour, const jxlh_save_desc& desc, void* out, size_t bytes_per_row, uint32_t y0 = 0,
            uint32_t y1 = 0xFFFFFFFFu) {
    ctx_.check(jxlh_frame_save(ctx_.raw(), colour, &desc, y0, y1, out, bytes_per_row), "jxlh_frame_save");
  }
  // ... for a list of rectangles of the result instead of a row band (jxlh_frame_save_rects): only their pixels are
  // written, each at its display position in the whole oriented image at `out`; _async: without the final wait
  void save_rects(const jxlh_output_desc* colour, const jxlh_save_desc& desc, const std::vector<jxlh_rect>& rects, void* out,
                  size_t bytes_per_row) {
    ctx_.check(jxlh_frame_save_rects(ctx_.raw(), colour, &desc, rects.data(), (uint32_t)rects.size(), out, bytes_per_row),
               "jxlh_frame_save_rects");
  }
  void save_rects_async(const jxlh_output_desc* colour, const jxlh_save_desc& desc, const std::vector<jxlh_rect>& rects,
                        void* out, size_t bytes_per_row) {
    ctx_.check(jxlh_frame_save_rects_async(ctx_.raw(), colour, &desc, rects.data(), (uint32_t)rects.size(), out, bytes_per_row),
               "jxlh_frame_save_rects_async");
  }
  // the rectangles of this frame's result that re-rendering `groups` can change (before blend(): frame coordinates)
  std::vector<jxlh_rect> changed_rects(const std::vector<uint32_t>& groups) const { return jxlh::changed_rects(p_, groups); }
  // ... and that repaint_groups(groups) can change: the result's coordinates, at the upsampled size
  std::vector<jxlh_rect> repaint_changed_rects(const std::vector<uint32_t>& groups) const {
    return jxlh::repaint_changed_rects(p_, groups);
  }
  // the frame's own result, whether or not it has been blended onto an image: what the *_changed_rects speak about
  uint32_t frame_width() const {
    const uint32_t n = p_.upsampling > 1 ? p_.upsampling : 1;
    return p_.xsize_upsampled ? p_.xsize_upsampled : p_.xsize * n;
  }
  uint32_t frame_height() const {
    const uint32_t n = p_.upsampling > 1 ? p_.upsampling : 1;
    return p_.ysize_upsampled ? p_.ysize_upsampled : p_.ysize * n;
  }
  bool blended() const { return blend_w_ != 0; }  // the image blend() / blend_rects() composed is the result
  uint32_t out_width() const {
    if (blend_w_) return blend_w_;
    const uint32_t n = p_.upsampling > 1 ? p_.upsampling : 1;
    return p_.xsize_upsampled ? p_.xsize_upsampled : p_.xsize * n;
  }
  uint32_t out_height() const {
    if (blend_h_) return blend_h_;
    const uint32_t n = p_.upsampling > 1 ? p_.upsampling : 1;
    return p_.ysize_upsampled ? p_.ysize_upsampled : p_.ysize * n;
  }

 private:
  Context& ctx_;
  jxlh_frame_params p_;
  uint32_t blend_w_ = 0, blend_h_ = 0;  // the image the frame was blended onto (0: not blended)
};

}  // namespace jxlh
