// The reference's RenderPipeline (jxl/src/render/mod.rs:116-157) for the path this library replaces: what
// RenderPipelineBuilder::build() returns.
//
// The reference assembles a frame's post-processing as a list of stage objects and lets a RenderPipeline
// implementation run them row chunk by row chunk.  On the device the same list is ONE launch sequence behind
// jxlh_frame_run (K1, the fused Gaborish / EPF kernel, chroma / frame upsampling, noise) plus one output pass
// (jxlh_frame_read_output, jxlh_frame_blend, jxlh_frame_save).  jxl_hip_lowering.hpp holds the host-only half: the stage
// descriptors under the reference's names, the builder, and the lowering of a stage list onto jxlh_frame_params and the
// output / blend / save descriptors.  The classes here begin the frame on a context with what a list lowered to and
// carry the trait's methods for this path: set_buffer_for_group (with the `complete` flag of render/mod.rs:128-136),
// mark_group_to_rerender, do_render, check_buffer_sizes.
//
// Header-only, C++17, no HIP types; tests/cpp/pipeline_builder.cc drives it (a whole frame against the oracle).
#pragma once
#include <cstdint>
#include <memory>
#include <utility>
#include <vector>

#include "jxl_hip_lowering.hpp"

namespace jxlh {

// A batch of groups for the squeeze calls (jxl_hip_local_squeeze.h): the groups, and the call-wide arrays their
// coded_first / params_first ranges index.  wp: empty when no step has predictor 6, else one header per group.
struct LocalSqueezeGroups {
  std::vector<jxlh_local_squeeze_group> groups;
  std::vector<jxlh_local_coded_channel> coded;
  std::vector<jxlh_squeeze_params> params;
  std::vector<jxlh_wp_header> wp;
  // a group of w x h at (x0, y0) whose coded channels and squeeze parameters are appended to the arrays; squeeze ==
  // nullptr: the group has none; an empty list: default_squeeze
  jxlh_local_squeeze_group& add(uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t n_channels,
                                const std::vector<jxlh_local_step>& steps, const std::vector<jxlh_squeeze_params>* squeeze,
                                const std::vector<jxlh_local_coded_channel>& channels) {
    if (steps.size() > JXLH_LOCAL_MAX_STEPS) throw Error(JXLH_ERR_INVALID_ARGUMENT, "LocalSqueezeGroups::add", "at most 4 steps");
    jxlh_local_squeeze_group g{};
    g.x0 = x0, g.y0 = y0, g.w = w, g.h = h, g.n_channels = n_channels;
    g.n_steps = (uint32_t)steps.size();
    for (size_t i = 0; i < steps.size(); i++) g.steps[i] = steps[i];
    g.has_squeeze = squeeze ? 1 : 0;
    g.squeeze_pos = squeeze ? g.n_steps : 0;
    g.params_first = (uint32_t)params.size(), g.n_params = squeeze ? (uint32_t)squeeze->size() : 0;
    if (squeeze) params.insert(params.end(), squeeze->begin(), squeeze->end());
    g.coded_first = (uint32_t)coded.size(), g.n_coded = (uint32_t)channels.size();
    coded.insert(coded.end(), channels.begin(), channels.end());
    groups.push_back(g);
    return groups.back();
  }
  void check(const char* where) const {
    if (!wp.empty() && wp.size() != groups.size()) throw Error(JXLH_ERR_INVALID_ARGUMENT, where, "one wp header per group, or none");
  }
};

// What GpuRenderPipeline and GpuModularFramePipeline share: the frame begun on the context with the lowered parameters,
// its dictionary and splines, the extra channels, and the output side -- blend, save, read.
class GpuFramePipeline {
 public:
  GpuFramePipeline(Context& ctx, LoweredPipeline lp) : ctx_(ctx), lp_(std::move(lp)), frame_(ctx, lp_.frame) {
    const float* const* w = lp_.weights_by_factor;
    if (w[0] || w[1] || w[2])  // CustomTransformData::weights{2,4,8} of the factors in use; the others keep their state
      ctx_.check(jxlh_set_upsampling_weights(ctx_.raw(), w[0], w[1], w[2]), "jxlh_set_upsampling_weights");
    if (lp_.has_patches) frame_.decode_patches(lp_.patches.patches, lp_.patches.blendings, lp_.patches.ec_flags);
    if (lp_.has_splines) frame_.set_spline_segments(lp_.splines.segments);
  }
  VarDctFrame& frame() { return frame_; }  // decode_hf_global / decode_lf_group / decode_hf_metadata go here
  const LoweredPipeline& lowered() const { return lp_; }
  // render/mod.rs:141-144: nothing of the frame lies outside what the groups cover on this path
  void render_outside_frame() {}
  // render/mod.rs:138: the caller's buffer must hold out_height rows of out_width * channels samples
  void check_buffer_sizes(size_t bytes_per_row, size_t rows) const {
    const size_t need = lp_.has_output ? (size_t)lp_.out_w * lp_.output.channels * (lp_.output.bits / 8)
                                       : (size_t)lp_.out_w * sizeof(float);
    if (bytes_per_row < need || rows < lp_.out_h)
      throw Error(JXLH_ERR_INVALID_ARGUMENT, "GpuRenderPipeline::check_buffer_sizes", "output buffer too small");
  }
  // ... of output buffer `buffer_index` of a list with six-argument save stages: the ORIENTED image
  void check_buffer_sizes(size_t buffer_index, size_t bytes_per_row, size_t rows) const {
    const jxlh_save_desc& d = save_desc(buffer_index);
    const bool t = d.orientation >= 5;
    const size_t bps = d.format == JXLH_SAVE_U8 ? 1 : d.format == JXLH_SAVE_F32 ? 4 : 2;
    const size_t need = (size_t)(t ? lp_.out_h : lp_.out_w) * (d.n_channels + (d.fill_opaque_alpha ? 1 : 0)) * bps;
    if (bytes_per_row < need || rows < (t ? lp_.out_w : lp_.out_h))
      throw Error(JXLH_ERR_INVALID_ARGUMENT, "GpuRenderPipeline::check_buffer_sizes", "output buffer too small");
  }
  // the save stage: interleaved integers through the colour tail, or the three f32 planes
  void save(void* out) {
    if (lp_.has_output) frame_.read_output(lp_.output, out);
    else throw Error(JXLH_ERR_INVALID_ARGUMENT, "GpuRenderPipeline::save", "planar f32 pipeline: use save_planes");
  }
  // a six-argument save stage: output buffer `buffer_index` (host or device memory, the origin of the whole oriented
  // image), source rows [y0, y1)
  void save(size_t buffer_index, void* out, size_t bytes_per_row, uint32_t y0 = 0, uint32_t y1 = 0xFFFFFFFFu) {
    frame_.save(&lp_.output, save_desc(buffer_index), out, bytes_per_row, y0, y1);
  }
  // ... only the pixels of `rects` (source rectangles of the result), e.g. what changed_rects() names after a pass
  void save_rects(size_t buffer_index, const std::vector<jxlh_rect>& rects, void* out, size_t bytes_per_row) {
    frame_.save_rects(&lp_.output, save_desc(buffer_index), rects, out, bytes_per_row);
  }
  void save_planes(float* c0, float* c1, float* c2) { frame_.read_planes(c0, c1, c2); }
  // an LF frame's result (lf_level = L) into LF slot L - 1, where the reference's list has its three Grayscale f32 save
  // stages (frame/render.rs:699-710); those stages are not lowered
  void save_lf(uint32_t slot) { frame_.save_lf(slot); }
  // An extra channel's integer samples as the Modular decoder leaves them (w x h at the channel's own resolution, host
  // or device memory).  The stage list decides what happens to them: ConvertModularToF32Stage with the channel's bit
  // depth, then its Upsample stage if it has one; both run inside do_render() behind the colour channels' stages.
  void set_extra_channel_buffer(uint32_t ec, const int32_t* samples, size_t stride, uint32_t w, uint32_t h) {
    if (ec >= JXLH_MAX_EXTRA_CHANNELS || !lp_.extra[ec].bits)
      throw Error(JXLH_ERR_INVALID_ARGUMENT, "GpuRenderPipeline::set_extra_channel_buffer", "the stage list does not name this extra channel");
    ctx_.check(jxlh_frame_set_extra_channel(ctx_.raw(), ec, samples, stride, w, h, lp_.extra[ec].bits, lp_.extra[ec].upsampling),
               "jxlh_frame_set_extra_channel");
  }
  // ... or the channel declared without samples (w x h at its own resolution) and fed rect by rect as its groups
  // arrive: the stage list names its bit depth and factor as above, and the next do_render() converts and upsamples only
  // what the rects can have changed (jxl_hip_extra_rects.h).  samples: one block, host or device memory.
  void begin_extra_channel(uint32_t ec, uint32_t w, uint32_t h) {
    if (ec >= JXLH_MAX_EXTRA_CHANNELS || !lp_.extra[ec].bits)
      throw Error(JXLH_ERR_INVALID_ARGUMENT, "GpuRenderPipeline::begin_extra_channel", "the stage list does not name this extra channel");
    frame_.begin_extra_channel(ec, w, h, lp_.extra[ec].bits, lp_.extra[ec].upsampling);
  }
  void set_extra_channel_rects(const int32_t* samples, uint64_t n_samples, const std::vector<jxlh_ec_rect>& rects) {
    frame_.set_extra_channel_rects(samples, n_samples, rects);
  }
  void set_extra_channel_rects_async(const int32_t* samples, uint64_t n_samples, const std::vector<jxlh_ec_rect>& rects) {
    frame_.set_extra_channel_rects_async(samples, n_samples, rects);
  }
  // ... or many groups of extra channels AS DECODED, each with its local transform list (jxl_hip_local_extra.h, the
  // n_colour == 0 form): the channels dest.ec names share one size, the groups' rects are in that resolution, and the
  // finished samples land in the channels' sample stores without a plane in between.  VarDCT and Modular lists alike.
  void set_extra_groups(const int32_t* arena, uint64_t arena_samples, const LocalSqueezeGroups& batch, const jxlh_local_dest& dest,
                        bool async = false) {
    if (dest.n_colour != 0)
      throw Error(JXLH_ERR_INVALID_ARGUMENT, "GpuFramePipeline::set_extra_groups", "colour channels go through GpuModularFramePipeline::set_groups");
    batch.check("GpuFramePipeline::set_extra_groups");
    frame_.set_modular_groups_extra(arena, arena_samples, batch.groups.data(), batch.groups.size(), batch.coded.data(),
                                    batch.coded.size(), batch.params.data(), batch.params.size(),
                                    batch.wp.empty() ? nullptr : batch.wp.data(), 0u, dest, async);
  }
  // The rectangles of finished extra channel `ec` (w x h source samples) that new samples in `rects` can change
  // (jxlh_extra_channel_changed_rects): what save_rects repaints, with changed_rects(), after the do_render() of a pass
  std::vector<jxlh_rect> extra_channel_changed_rects(uint32_t ec, uint32_t w, uint32_t h, const std::vector<jxlh_rect>& rects) const {
    if (ec >= JXLH_MAX_EXTRA_CHANNELS || !lp_.extra[ec].bits)
      throw Error(JXLH_ERR_INVALID_ARGUMENT, "GpuRenderPipeline::extra_channel_changed_rects", "the stage list does not name this extra channel");
    uint32_t n = 0;
    std::vector<jxlh_rect> out(rects.size());
    const jxlh_status st = jxlh_extra_channel_changed_rects(w, h, lp_.extra[ec].upsampling, frame_.out_width(), frame_.out_height(),
                                                            rects.data(), (uint32_t)rects.size(), out.data(), (uint32_t)out.size(), &n);
    if (st != JXLH_OK) throw Error(st, "jxlh_extra_channel_changed_rects", "");
    return out;
  }
  // the save stage of an extra channel: one f32 plane of the frame's output size (out_width() x out_height())
  void save_extra_channel(uint32_t ec, float* out, size_t stride) {
    jxlh_plane pl{out, (size_t)frame_.out_width() * sizeof(float), frame_.out_height(), stride * sizeof(float)};
    ctx_.check(jxlh_frame_read_extra_channel(ctx_.raw(), ec, &pl), "jxlh_frame_read_extra_channel");
  }

 protected:
  // BlendingStage + extend (with the list's colour stage in front): the image becomes what the save stages read
  void blend_if_listed() {
    if (lp_.has_blend) frame_.blend(lp_.blend, &lp_.blend_colour);
  }
  // The *_rects forms of the render calls end here.  `changed`: rects of the frame's result a re-render can have changed.
  // Without a BlendingStage they are what save_rects takes.  With one, only they are composed again, in the canvas the
  // last blend left (jxlh_frame_blend_rects), and they come back in image coordinates (jxlh_blend_image_rects)
  std::vector<jxlh_rect> blend_rects_if_listed(const std::vector<jxlh_rect>& changed) {
    if (!lp_.has_blend) return changed;
    const std::vector<jxlh_rect> image = blend_image_rects(lp_.blend, frame_.frame_width(), frame_.frame_height(), changed);
    frame_.blend_rects(lp_.blend, image, &lp_.blend_colour);
    return image;
  }
  // ... and a whole render here: the whole blend, one rect of the whole result
  std::vector<jxlh_rect> blend_whole_if_listed() {
    blend_if_listed();
    return {jxlh_rect{0, 0, frame_.out_width(), frame_.out_height()}};
  }
  const jxlh_save_desc& save_desc(size_t buffer_index) const {
    if (buffer_index >= lp_.saves.size())
      throw Error(JXLH_ERR_INVALID_ARGUMENT, "GpuRenderPipeline::save", "the stage list has no save stage for this buffer");
    return lp_.saves[buffer_index];
  }
  Context& ctx_;
  LoweredPipeline lp_;
  VarDctFrame frame_;
};

// RenderPipeline (render/mod.rs:116-157) for this path: inputs are a group's coefficient slabs instead of its pixel
// buffers (the transforms run on the device too), everything else keeps the trait's meaning.
class GpuRenderPipeline : public GpuFramePipeline {
 public:
  using GpuFramePipeline::GpuFramePipeline;
  // render/mod.rs:128-136.  complete = false: a progressive pass that leaves the group open
  void set_buffer_for_group(uint32_t group_id, bool complete, const int32_t* coeffs, int slot = 0) {
    ctx_.check(jxlh_submit_group(ctx_.raw(), slot, group_id, coeffs, complete ? JXLH_GROUP_COMPLETE : 0u), "jxlh_submit_group");
    // the reference renders every group it is handed (render/mod.rs:128-136): once the frame has been rendered, a group
    // that receives new coefficients is re-rendered whether or not the caller also marks it (duplicates are merged by
    // jxlh_frame_rerender_groups)
    if (!dirty_first_) rerender_.push_back(group_id);
  }
  // render/mod.rs:146
  void mark_group_to_rerender(uint32_t g) { rerender_.push_back(g); }
  // The rectangles of the frame's result that re-rendering `groups` can change (jxlh_changed_rects): what save_rects
  // repaints after the do_render() of a pass that touched them.  Frame coordinates: with a BlendingStage in the list,
  // shift them by the frame's origin and clip them to the image.
  std::vector<jxlh_rect> changed_rects(const std::vector<uint32_t>& groups) const { return frame_.changed_rects(groups); }
  // do_render() for frames jxlh_frame_rerender_groups refuses as well (frame upsampling): the groups handed over or
  // marked since the last render are repainted (jxlh_frame_repaint_groups), the whole frame before the first render.
  // repaint_changed_rects: the rectangles of the result, at the upsampled size, that such a repaint can change.
  void repaint() {
    for (int s = 0; s < ctx_.n_slots(); s++) ctx_.check(jxlh_slot_wait(ctx_.raw(), s), "jxlh_slot_wait");
    if (!rerender_.empty() && !dirty_first_) frame_.repaint_groups(rerender_);
    else frame_.finalize_and_render();
    blend_if_listed();
    dirty_first_ = false;
    rerender_.clear();
  }
  std::vector<jxlh_rect> repaint_changed_rects(const std::vector<uint32_t>& groups) const {
    return frame_.repaint_changed_rects(groups);
  }
  // do_render() / repaint() for a progressive repaint that stays rect-sized to the end: they render as their siblings
  // do, but on a list with a BlendingStage only the changed rects are composed again (jxl_hip_blend_rects.h) instead of
  // the whole image, and they return the rects to hand to save_rects -- image coordinates with a blend, the changed
  // rects as they are without one; the first render does the whole blend and returns one rect of the whole result.
  // also_changed: further rects of the frame's result whose inputs changed since the last render, e.g.
  // extra_channel_changed_rects() of alpha samples that arrived by rect.
  std::vector<jxlh_rect> do_render_rects(const std::vector<jxlh_rect>& also_changed = {}) {
    for (int s = 0; s < ctx_.n_slots(); s++) ctx_.check(jxlh_slot_wait(ctx_.raw(), s), "jxlh_slot_wait");
    std::vector<jxlh_rect> out;
    if (!rerender_.empty() && !dirty_first_) {
      std::vector<jxlh_rect> changed = frame_.changed_rects(rerender_);  // (refuses what jxlh_frame_rerender_groups refuses)
      changed.insert(changed.end(), also_changed.begin(), also_changed.end());
      ctx_.check(jxlh_frame_rerender_groups(ctx_.raw(), rerender_.data(), (uint32_t)rerender_.size()), "jxlh_frame_rerender_groups");
      out = blend_rects_if_listed(changed);
    } else {
      frame_.finalize_and_render();
      out = blend_whole_if_listed();
    }
    dirty_first_ = false;
    rerender_.clear();
    return out;
  }
  std::vector<jxlh_rect> repaint_rects(const std::vector<jxlh_rect>& also_changed = {}) {
    for (int s = 0; s < ctx_.n_slots(); s++) ctx_.check(jxlh_slot_wait(ctx_.raw(), s), "jxlh_slot_wait");
    std::vector<jxlh_rect> out;
    if (!rerender_.empty() && !dirty_first_) {
      std::vector<jxlh_rect> changed = frame_.repaint_changed_rects(rerender_);
      changed.insert(changed.end(), also_changed.begin(), also_changed.end());
      frame_.repaint_groups(rerender_);
      out = blend_rects_if_listed(changed);
    } else {
      frame_.finalize_and_render();
      out = blend_whole_if_listed();
    }
    dirty_first_ = false;
    rerender_.clear();
    return out;
  }
  // A group that must be rendered while its HF has not arrived (force_render with DataStatus::Zero, frame/decode.rs:
  // 744-752): the reference hands the pipeline the LF image upsampled 8x as the group's buffers; here the group is marked
  // and the next do_render() fills it on the device.  set_buffer_for_group on the group later clears the mark.
  void set_lf_only_group(uint32_t group_id) {
    frame_.upsample_lf_groups(&group_id, 1);
    if (!dirty_first_) rerender_.push_back(group_id);
  }
  // what the reference does when the last group of a pass has been handed over (frame/decode.rs:547-558, :703-711)
  void do_render() {
    for (int s = 0; s < ctx_.n_slots(); s++) ctx_.check(jxlh_slot_wait(ctx_.raw(), s), "jxlh_slot_wait");
    if (!rerender_.empty() && !dirty_first_) {
      ctx_.check(jxlh_frame_rerender_groups(ctx_.raw(), rerender_.data(), (uint32_t)rerender_.size()), "jxlh_frame_rerender_groups");
    } else {
      frame_.finalize_and_render();
    }
    blend_if_listed();
    dirty_first_ = false;
    rerender_.clear();
  }

 private:
  std::vector<uint32_t> rerender_;
  bool dirty_first_ = true;
};

// A Modular frame as a frame of the context (lower_modular_frame): the samples come out of the Modular inverse
// transforms (jxlh_rct, jxlh_palette*, jxlh_unsqueeze_chain) as three i32 planes, host or device memory, and go in rect
// by rect; render() is the whole stage list behind jxlh_frame_run, and the output side is GpuRenderPipeline's.
class GpuModularFramePipeline : public GpuFramePipeline {
 public:
  GpuModularFramePipeline(Context& ctx, LoweredPipeline lp) : GpuFramePipeline(ctx, std::move(lp)) {
    if (!(lp_.frame.flags & JXLH_FRAME_MODULAR))
      throw Error(JXLH_ERR_INVALID_ARGUMENT, "GpuModularFramePipeline", "the list was not lowered by lower_modular_frame");
  }
  // one rect of the three colour channels (coded order Y, X, B for an XYB list; one pointer three times for a grey
  // frame), full-resolution coordinates, row stride in samples
  void set_channels(uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const int32_t* const planes[3], size_t stride) {
    frame_.set_modular_channels(x0, y0, w, h, planes, stride, lp_.modular_sample_format);
  }
  // the batched intake: many groups as decoded, each with its local transform list (jxlh_frame_set_modular_groups);
  // what a group's list holds that the device does not take comes back as JXLH_ERR_UNSUPPORTED before anything ran, and
  // that group goes through set_channels after the host's local_apply
  void set_groups(const int32_t* arena, uint64_t arena_samples, const std::vector<jxlh_local_group>& groups, bool async = false) {
    frame_.set_modular_groups(arena, arena_samples, groups.data(), groups.size(), lp_.modular_sample_format, async);
  }
  // the same with every local palette on the device (jxlh_frame_set_modular_groups_general): delta entries and all 14
  // predictors; a local squeeze goes through the LocalSqueezeGroups overload below.  wp: empty when no step has predictor 6, else one
  // GroupHeader::wp_header per group
  void set_groups_general(const int32_t* arena, uint64_t arena_samples, const std::vector<jxlh_local_group>& groups,
                          const std::vector<jxlh_wp_header>& wp, bool async = false) {
    if (!wp.empty() && wp.size() != groups.size())
      throw Error(JXLH_ERR_INVALID_ARGUMENT, "GpuModularFramePipeline::set_groups_general", "one wp header per group, or none");
    frame_.set_modular_groups_general(arena, arena_samples, groups.data(), wp.empty() ? nullptr : wp.data(), groups.size(),
                                      lp_.modular_sample_format, async);
  }
  // the same with local squeezes on the device too (jxlh_frame_set_modular_groups_squeeze): nothing group-local is left
  // to the host but what the header lists as unsupported
  void set_groups(const int32_t* arena, uint64_t arena_samples, const LocalSqueezeGroups& batch, bool async = false) {
    batch.check("GpuModularFramePipeline::set_groups");
    frame_.set_modular_groups_squeeze(arena, arena_samples, batch.groups.data(), batch.groups.size(), batch.coded.data(),
                                      batch.coded.size(), batch.params.data(), batch.params.size(),
                                      batch.wp.empty() ? nullptr : batch.wp.data(), lp_.modular_sample_format, async);
  }
  // ... into the colour planes AND extra channels (jxlh_frame_set_modular_groups_extra): the groups' leading
  // dest.n_colour channels are the frame's colour, the others the extra channels dest.ec names (begun or set before).
  // dest.n_colour == 0 is GpuFramePipeline::set_extra_groups
  void set_groups(const int32_t* arena, uint64_t arena_samples, const LocalSqueezeGroups& batch, const jxlh_local_dest& dest,
                  bool async = false) {
    batch.check("GpuModularFramePipeline::set_groups");
    frame_.set_modular_groups_extra(arena, arena_samples, batch.groups.data(), batch.groups.size(), batch.coded.data(),
                                    batch.coded.size(), batch.params.data(), batch.params.size(),
                                    batch.wp.empty() ? nullptr : batch.wp.data(), dest.n_colour ? lp_.modular_sample_format : 0u,
                                    dest, async);
  }
  // the whole frame, then the list's blending
  void render() {
    frame_.finalize_and_render();
    blend_if_listed();
  }
  // The listed cells of the 256 grid over the coded size again, after set_channels / set_groups replaced samples in them
  // and behind a whole render() (jxlh_frame_repaint_groups: frame upsampling included; before any render() it is one),
  // then the list's blending; repaint_changed_rects: the rectangles of the result such a repaint can change
  void repaint_groups(const std::vector<uint32_t>& groups) {
    frame_.repaint_groups(groups);
    blend_if_listed();
  }
  std::vector<jxlh_rect> repaint_changed_rects(const std::vector<uint32_t>& groups) const {
    return frame_.repaint_changed_rects(groups);
  }
  // repaint_groups() that stays rect-sized: on a list with a BlendingStage only repaint_changed_rects(groups) are composed
  // again (jxl_hip_blend_rects.h) and come back in image coordinates, for save_rects; before the first render() -- no
  // composition to patch -- it is the whole blend and one rect of the image.  Without a blend: the changed rects as they are
  std::vector<jxlh_rect> repaint_groups_rects(const std::vector<uint32_t>& groups) {
    const std::vector<jxlh_rect> changed = frame_.repaint_changed_rects(groups);
    const bool patch = !lp_.has_blend || frame_.blended();
    frame_.repaint_groups(groups);
    return patch ? blend_rects_if_listed(changed) : blend_whole_if_listed();
  }
  // 256-row bands [band0, band1) (a list with blending or frame upsampling renders whole)
  void render_band(uint32_t band0, uint32_t band1) {
    if (lp_.has_blend) throw Error(JXLH_ERR_UNSUPPORTED, "GpuModularFramePipeline::render_band", "a blended frame is rendered whole");
    frame_.finalize_and_render(band0, band1);
  }
};

// A Modular frame's stage list on the device: the samples come out of the Modular inverse transforms (jxlh_rct,
// jxlh_palette*, jxlh_unsqueeze_chain) as three i32 planes, host or device memory.
class GpuModularPipeline {
 public:
  GpuModularPipeline(Context& ctx, LoweredPipeline lp) : ctx_(ctx), lp_(std::move(lp)) {
    if (lp_.modular == LoweredPipeline::Modular::kNone)
      throw Error(JXLH_ERR_INVALID_ARGUMENT, "GpuModularPipeline", "the stage list holds no Modular conversion");
  }
  const LoweredPipeline& lowered() const { return lp_; }
  // the batched intake of the caller-held-planes form (jxlh_modular_local_transforms): every group's local transforms,
  // finished channels into `planes` (n_planes DEVICE planes of the frame's size) at the group's rect, one launch
  void local_transforms(const int32_t* arena, uint64_t arena_samples, const std::vector<jxlh_local_group>& groups,
                        uint32_t bit_depth, int32_t* const planes[], uint32_t n_planes, size_t stride) {
    size_t bad = 0;
    ctx_.check(jxlh_modular_local_transforms(ctx_.raw(), arena, arena_samples, groups.data(), groups.size(), bit_depth, planes,
                                             n_planes, lp_.frame.xsize, lp_.frame.ysize, stride, &bad),
               "jxlh_modular_local_transforms");
  }
  // ... with every local palette (jxlh_modular_local_transforms_general); wp as in set_groups_general
  void local_transforms_general(const int32_t* arena, uint64_t arena_samples, const std::vector<jxlh_local_group>& groups,
                                const std::vector<jxlh_wp_header>& wp, uint32_t bit_depth, int32_t* const planes[],
                                uint32_t n_planes, size_t stride) {
    if (!wp.empty() && wp.size() != groups.size())
      throw Error(JXLH_ERR_INVALID_ARGUMENT, "GpuModularPipeline::local_transforms_general", "one wp header per group, or none");
    size_t bad = 0;
    ctx_.check(jxlh_modular_local_transforms_general(ctx_.raw(), arena, arena_samples, groups.data(),
                                                     wp.empty() ? nullptr : wp.data(), groups.size(), bit_depth, planes, n_planes,
                                                     lp_.frame.xsize, lp_.frame.ysize, stride, &bad),
               "jxlh_modular_local_transforms_general");
  }
  // ... and with local squeezes (jxlh_modular_local_transforms_squeeze)
  void local_transforms(const int32_t* arena, uint64_t arena_samples, const LocalSqueezeGroups& batch, uint32_t bit_depth,
                        int32_t* const planes[], uint32_t n_planes, size_t stride) {
    batch.check("GpuModularPipeline::local_transforms");
    size_t bad = 0;
    ctx_.check(jxlh_modular_local_transforms_squeeze(ctx_.raw(), arena, arena_samples, batch.groups.data(), batch.groups.size(),
                                                     batch.coded.data(), batch.coded.size(), batch.params.data(),
                                                     batch.params.size(), batch.wp.empty() ? nullptr : batch.wp.data(), bit_depth,
                                                     planes, n_planes, lp_.frame.xsize, lp_.frame.ysize, stride, &bad),
               "jxlh_modular_local_transforms_squeeze");
  }
  // ConvertI32ToU8Stage: interleaved bytes (3 or 4 per pixel) in one pass
  void render_u8(const int32_t* const planes[3], size_t stride, void* out, size_t bytes_per_row) {
    if (lp_.modular != LoweredPipeline::Modular::kI32ToU8)
      throw Error(JXLH_ERR_INVALID_ARGUMENT, "GpuModularPipeline::render_u8", "not the I32 -> U8 special case");
    ctx_.check(jxlh_modular_to_rgb8(ctx_.raw(), planes, stride, lp_.frame.xsize, lp_.frame.ysize, lp_.i32_to_u8_multiplier,
                                    lp_.i32_to_u8_max, lp_.output.channels, out, bytes_per_row),
               "jxlh_modular_to_rgb8");
  }
  // conversion to f32 and, if the list holds them, Gaborish / EPF with the frame's constant sigma
  // (jxlh_modular_frame_filters: device planes, 16-byte aligned, row stride a multiple of 4 floats, tmp != out).
  // in[] in coded order for an XYB frame (Y, X, B); the result (X, Y, B) lands in out[]; tmp[] is only used when the
  // list holds filters.  Planes are tight: stride = xsize, which must then be a multiple of 4.
  void render_f32(const int32_t* const in[3], float* const tmp[3], float* const out[3]) {
    const size_t w = lp_.frame.xsize, h = lp_.frame.ysize, n = w * h;
    const bool filters = lp_.frame.gab || lp_.frame.epf_iters;
    float* const* dst = filters ? tmp : out;
    if (lp_.modular == LoweredPipeline::Modular::kXybToF32) {
      ctx_.check(jxlh_modular_xyb_to_f32(ctx_.raw(), in[0], in[1], in[2], n, lp_.modular_quant_factors.data(), dst[0], dst[1], dst[2]),
                 "jxlh_modular_xyb_to_f32");
    } else if (lp_.modular == LoweredPipeline::Modular::kToF32) {
      for (int c = 0; c < 3; c++)
        ctx_.check(jxlh_modular_to_f32(ctx_.raw(), in[c], n, lp_.modular_bits, dst[c]), "jxlh_modular_to_f32");
    } else {
      throw Error(JXLH_ERR_INVALID_ARGUMENT, "GpuModularPipeline::render_f32", "the list lowers to the I32 -> U8 special case");
    }
    if (filters) {
      if (w % 4) throw Error(JXLH_ERR_UNSUPPORTED, "GpuModularPipeline::render_f32", "filters need a row length that is a multiple of 4 samples");
      ctx_.check(jxlh_modular_frame_filters(ctx_.raw(), &lp_.frame, tmp, out, (uint32_t)w, (uint32_t)h, w), "jxlh_modular_frame_filters");
    }
  }

 private:
  Context& ctx_;
  LoweredPipeline lp_;
};

inline std::unique_ptr<GpuRenderPipeline> RenderPipelineBuilder::build(Context& ctx) && {
  return std::make_unique<GpuRenderPipeline>(ctx, lower());
}

inline std::unique_ptr<GpuModularPipeline> RenderPipelineBuilder::build_modular(Context& ctx) && {
  return std::make_unique<GpuModularPipeline>(ctx, lower());
}

inline std::unique_ptr<GpuModularFramePipeline> RenderPipelineBuilder::build_modular_frame(Context& ctx) && {
  return std::make_unique<GpuModularFramePipeline>(ctx, lower_modular_frame());
}

}  // namespace jxlh
