// Host-side lowering of a Modular frame's stage list (include/jxl_hip_lowering.hpp): lower_modular_frame() takes the
// reference's full Modular list (frame/render.rs:553-903) onto the LoweredPipeline fields a VarDCT list fills, under
// the same order and consistency checks; lower() still rejects those lists exactly as before, naming the stage hooks.
// No GPU involved.
#include <cstdio>
#include <string>

#include "lowering_helpers.h"

using namespace jxlh;
using namespace lowering_helpers;

namespace {
bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }
SplinesStage segs() {
  SplinesStage st;
  st.segments = {jxlh_spline_segment{10.0f, 20.0f, 3.5f, 1.25f, 0.1f, {0.5f, 0.6f, 0.7f}}};
  return st;
}
PatchesStage dict(size_t num_ec) {
  PatchesStage ps;
  ps.patches = {jxlh_patch{4, 5, 0, 0, 0, 16, 12}};
  ps.blendings.assign(1 + num_ec, jxlh_patch_blending{JXLH_PATCH_ADD, 0, 0});
  ps.ec_flags.assign(num_ec, JXLH_EC_ALPHA);
  return ps;
}
RenderPipelineBuilder conversions(RenderPipelineBuilder b, uint8_t bits = 8) {
  return std::move(b)
      .add_inout_stage(ConvertModularToF32Stage{0, bits})
      .add_inout_stage(ConvertModularToF32Stage{1, bits})
      .add_inout_stage(ConvertModularToF32Stage{2, bits});
}
BlendingStage blending() { return lowering_helpers::blending(5, 3, 1200, 900, jxlh_blending_info{}, 1, jxlh_blending_info{}); }
// the reference's full list of a 500 x 350 Modular frame shown at 1000 x 700: conversions, chroma upsampling, filters,
// the alpha channel's conversion, patches, splines, frame upsampling (the alpha with it), noise, colour stages,
// blending + extend, spot colour, premultiply, conversions, an RGBA8 save
RenderPipelineBuilder full_list(const jxlh_frame_params& q, bool xyb_form) {
  RenderPipelineBuilder b(8, {1000, 700}, 1, 8, q);
  if (xyb_form) {
    b = std::move(b).add_inout_stage(ConvertModularXYBToF32Stage{0, {0.25f, 0.5f, 0.125f}});
  } else {
    b = conversions(std::move(b), 12);
  }
  b = std::move(b).add_inout_stage(ConvertModularToF32Stage{3, 16}).add_inout_stage(ConvertModularToF32Stage{4, 8});
  if (!xyb_form)
    b = std::move(b).add_inout_stage(HorizontalChromaUpsample{0}).add_inout_stage(VerticalChromaUpsample{0})
            .add_inout_stage(HorizontalChromaUpsample{2}).add_inout_stage(VerticalChromaUpsample{2});
  const BlendingStage bl = blending();
  BlendingStage bl2 = bl;
  bl2.ec_blending_info.assign(2, jxlh_blending_info{});
  bl2.ec_flags = {JXLH_EC_ALPHA, 0};
  return filters(std::move(b), q)
      .add_inplace_stage(segs())
      .add_inout_stage(Upsample2x{nullptr, 0})
      .add_inout_stage(Upsample2x{nullptr, 1})
      .add_inout_stage(Upsample2x{nullptr, 2})
      .add_inout_stage(Upsample2x{nullptr, 3})
      .add_inout_stage(Upsample2x{nullptr, 4})
      .add_inout_stage(ConvolveNoiseStage{5})
      .add_inout_stage(ConvolveNoiseStage{6})
      .add_inout_stage(ConvolveNoiseStage{7})
      .add_inplace_stage(AddNoiseStage{{0.1f, 0.2f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.3f}, 0, 0, 5})
      .add_inplace_stage(XybStage{0, jxlh_xyb_params{}})
      .add_inplace_stage(FromLinearStage{0, JXLH_TF_SRGB, 0.0f, {0.2627f, 0.678f, 0.0593f}})
      .add_inplace_stage(bl2)
      .add_extend_stage(extend_of(bl2))
      .add_inplace_stage(SpotColorStage{1, {1.0f, 0.5f, 0.25f, 0.75f}})
      .add_inplace_stage(PremultiplyAlphaStage{0, 3, 3})
      .add_inout_stage(ConvertF32ToU8Stage{0, 8})
      .add_inout_stage(ConvertF32ToU8Stage{1, 8})
      .add_inout_stage(ConvertF32ToU8Stage{2, 8})
      .add_inout_stage(ConvertF32ToU8Stage{3, 8})
      .add_save_stage({0, 1, 2, 3}, 6, 0, ColorType::kRgba, DataFormat::u8(), false);
}
}  // namespace

int main() {
  const jxlh_frame_params p = base(1000, 700);
  std::string msg;
  // ---- the full list, integer form and XYB form
  {
    const jxlh_frame_params q = base(500, 350);
    const LoweredPipeline lp = full_list(q, false).lower_modular_frame();
    expect((lp.frame.flags & JXLH_FRAME_MODULAR) != 0, "the frame flag is set");
    expect(lp.modular == LoweredPipeline::Modular::kToF32 && lp.modular_bits == 12 && lp.modular_sample_format == 12,
           "integer conversions lower to the sample format");
    expect(lp.frame.hshift[0] == 1 && lp.frame.vshift[0] == 1 && lp.frame.hshift[1] == 0 && lp.frame.vshift[2] == 1, "chroma shifts");
    expect(lp.frame.gab == 1 && lp.frame.epf_iters == 1, "filters");
    expect(lp.extra[0].bits == 16 && lp.extra[0].upsampling == 2 && lp.extra[1].bits == 8 && lp.extra[1].upsampling == 2, "extra channels");
    expect(lp.has_splines && lp.splines.segments.size() == 1, "splines");
    expect(lp.frame.upsampling == 2 && lp.frame.xsize_upsampled == 1000 && lp.frame.ysize_upsampled == 700, "frame upsampling");
    expect(lp.frame.noise == 1 && lp.frame.noise_lut[7] == 0.3f, "noise");
    expect(lp.has_blend && lp.blend.x0 == 5 && lp.blend.image_w == 1200 && lp.blend.num_ec == 2, "blending + extend");
    expect(lp.blend_colour.color == JXLH_COLOR_XYB && lp.blend_colour.transfer == JXLH_TF_SRGB && lp.output.color == JXLH_COLOR_NONE,
           "the colour stage runs inside the blend");
    expect(lp.saves.size() == 1 && lp.saves[0].n_channels == 4 && lp.saves[0].orientation == 6 && lp.saves[0].premultiply &&
               lp.saves[0].n_spot == 1 && lp.saves[0].spot[0].ec == 1 && lp.saves[0].format == JXLH_SAVE_U8,
           "spot / premultiply / convert / save lower to one save descriptor");
    expect(lp.out_w == 1200 && lp.out_h == 900, "the save stages see the image");
    const LoweredPipeline lx = full_list(q, true).lower_modular_frame();
    expect(lx.modular == LoweredPipeline::Modular::kXybToF32 && lx.modular_sample_format == JXLH_MODULAR_XYB,
           "the XYB conversion lowers to JXLH_MODULAR_XYB");
    expect(lx.frame.lf_quant_factors[0] == 0.25f && lx.frame.lf_quant_factors[1] == 0.5f && lx.frame.lf_quant_factors[2] == 0.125f,
           "... and its factors to lf_quant_factors");
    expect((lx.frame.flags & JXLH_FRAME_MODULAR) != 0 && lx.frame.upsampling == 2 && lx.has_blend && lx.saves.size() == 1, "XYB form, the rest alike");
  }
  // patches (with an alpha channel) at the coded size, planar f32 save
  {
    const LoweredPipeline lp = filters(conversions(RenderPipelineBuilder(4, {1000, 700}, 0, 8, p)).add_inout_stage(ConvertModularToF32Stage{3, 8}), p)
                                   .add_inplace_stage(dict(1)).add_inplace_stage(segs()).add_save_stage({0, 1, 2}, 0, 3, 32).lower_modular_frame();
    expect(lp.has_patches && lp.patches.patches.size() == 1 && lp.patches.ec_flags.size() == 1 && lp.has_splines && !lp.has_output,
           "patches -> splines on a Modular frame");
  }
  // 8-bit samples to 8-bit output: the frame path converts through f32 (the I32 -> U8 special case stays with lower())
  {
    auto list = [&] {
      return conversions(RenderPipelineBuilder(3, {1000, 700}, 0, 8, p))
          .add_inout_stage(ConvertF32ToU8Stage{0, 8}).add_inout_stage(ConvertF32ToU8Stage{1, 8}).add_inout_stage(ConvertF32ToU8Stage{2, 8})
          .add_save_stage({0, 1, 2}, 0, 3, 8);
    };
    const LoweredPipeline lf = list().lower_modular_frame();
    expect(lf.modular == LoweredPipeline::Modular::kToF32 && lf.has_output && lf.output.bits == 8 && lf.output.color == JXLH_COLOR_NONE,
           "lower_modular_frame keeps the conversions");
    const LoweredPipeline lo = list().lower();
    expect(lo.modular == LoweredPipeline::Modular::kI32ToU8 && lo.i32_to_u8_multiplier == 1 && !(lo.frame.flags & JXLH_FRAME_MODULAR),
           "lower() keeps the I32 -> U8 special case");
  }
  // ---- rejected by lower_modular_frame with lower()'s messages for the VarDCT equivalents
  expect(status_of([&] { (void)filters(RenderPipelineBuilder(3, {1000, 700}, 0, 8, p), p).add_save_stage({0, 1, 2}, 0, 3, 32).lower_modular_frame(); },
                   &msg) == JXLH_ERR_INVALID_ARGUMENT && has(msg, "no Modular conversion"),
         "a list without conversions is no Modular frame");
  expect(status_of([&] { (void)RenderPipelineBuilder(3, {1000, 700}, 0, 8, p)
                             .add_inout_stage(ConvertModularToF32Stage{0, 8}).add_inout_stage(ConvertModularToF32Stage{1, 8})
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower_modular_frame(); }, &msg) == JXLH_ERR_INVALID_ARGUMENT &&
             has(msg, "some channels only"),
         "a partial conversion is rejected");
  expect(status_of([&] { (void)conversions(filters(RenderPipelineBuilder(3, {1000, 700}, 0, 8, p), p))
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower_modular_frame(); }, &msg) == JXLH_ERR_UNSUPPORTED &&
             has(msg, "out of the order of Frame::build_render_pipeline"),
         "conversions behind the filters are rejected");
  expect(status_of([&] { (void)filters(conversions(RenderPipelineBuilder(3, {1000, 700}, 0, 8, p)).add_inplace_stage(segs()), p)
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower_modular_frame(); }) == JXLH_ERR_UNSUPPORTED,
         "splines before the filters are rejected");
  expect(status_of([&] { (void)conversions(RenderPipelineBuilder(3, {1000, 700}, 0, 8, p)).add_inplace_stage(segs()).add_inplace_stage(dict(0))
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower_modular_frame(); }, &msg) == JXLH_ERR_UNSUPPORTED && has(msg, "patches"),
         "patches behind the splines are rejected");
  expect(status_of([&] { (void)conversions(RenderPipelineBuilder(3, {1000, 700}, 0, 8, p))
                             .add_inout_stage(GaborishStage{0, 0.1f, 0.05f}).add_save_stage({0, 1, 2}, 0, 3, 32).lower_modular_frame(); }, &msg) ==
                 JXLH_ERR_INVALID_ARGUMENT && has(msg, "Gaborish on some channels only"),
         "partial Gaborish is rejected");
  expect(status_of([&] { (void)conversions(RenderPipelineBuilder(3, {1000, 700}, 0, 8, p)).lower_modular_frame(); }, &msg) ==
                 JXLH_ERR_INVALID_ARGUMENT && has(msg, "no save stage"),
         "a list without a save stage is rejected");
  expect(status_of([&] { (void)conversions(RenderPipelineBuilder(4, {1000, 700}, 0, 8, p)).add_inout_stage(ConvertModularToF32Stage{3, 8})
                             .add_inplace_stage(blending()).add_save_stage({0, 1, 2}, 0, 3, 32).lower_modular_frame(); }, &msg) ==
                 JXLH_ERR_INVALID_ARGUMENT && has(msg, "between the blending stage and the extend stage"),
         "blending without extend is rejected");
  expect(status_of([&] { (void)RenderPipelineBuilder(3, {1000, 700}, 0, 8, p)
                             .add_inout_stage(ConvertModularXYBToF32Stage{0, {0.25f, 0.5f, 0.125f}})
                             .add_inout_stage(HorizontalChromaUpsample{0})
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower_modular_frame(); }) == JXLH_ERR_INVALID_ARGUMENT,
         "chroma subsampling on an XYB Modular frame is rejected");
  expect(status_of([&] { (void)conversions(RenderPipelineBuilder(3, {1000, 700}, 0, 8, p)).add_inplace_stage(CpuOnlyStage{"splines"})
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower_modular_frame(); }) == JXLH_ERR_UNSUPPORTED,
         "a CPU-only stage is still rejected");
  // ---- lower() on the Modular lists: exactly as before
  expect(status_of([&] { (void)conversions(RenderPipelineBuilder(3, {1000, 700}, 0, 8, p)).add_inplace_stage(segs())
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }, &msg) == JXLH_ERR_UNSUPPORTED &&
             has(msg, "splines on a Modular frame (jxlh_stage_splines on the planes instead)"),
         "lower(): splines on a Modular list names jxlh_stage_splines");
  expect(status_of([&] { (void)conversions(RenderPipelineBuilder(3, {1000, 700}, 0, 8, p)).add_inplace_stage(dict(0))
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }, &msg) == JXLH_ERR_UNSUPPORTED &&
             has(msg, "patches on a Modular frame (jxlh_stage_patches on the planes instead)"),
         "lower(): patches on a Modular list names jxlh_stage_patches");
  expect(status_of([&] { (void)conversions(RenderPipelineBuilder(4, {1000, 700}, 0, 8, p)).add_inout_stage(ConvertModularToF32Stage{3, 8})
                             .add_inplace_stage(blending()).add_extend_stage(extend_of(blending()))
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }, &msg) == JXLH_ERR_UNSUPPORTED &&
             has(msg, "blending on a Modular frame (jxlh_stage_blend on the planes instead)"),
         "lower(): blending on a Modular list names jxlh_stage_blend");
  expect(status_of([&] { (void)conversions(RenderPipelineBuilder(3, {1000, 700}, 0, 8, p))
                             .add_inout_stage(ConvertF32ToU8Stage{0, 8}).add_inout_stage(ConvertF32ToU8Stage{1, 8}).add_inout_stage(ConvertF32ToU8Stage{2, 8})
                             .add_save_stage({0, 1, 2}, 1, 0, ColorType::kRgb, DataFormat::u8(), false).lower(); }, &msg) == JXLH_ERR_UNSUPPORTED &&
             has(msg, "on a Modular frame (jxlh_stage_save on the planes instead)"),
         "lower(): the save tail on a Modular list names jxlh_stage_save");
  expect(status_of([&] { (void)conversions(RenderPipelineBuilder(3, {1000, 700}, 0, 8, p)).add_inplace_stage(XybStage{0, jxlh_xyb_params{}})
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }, &msg) == JXLH_ERR_UNSUPPORTED && has(msg, "colour stages on a Modular frame"),
         "lower(): colour stages on a Modular list");
  {
    const jxlh_frame_params q = base(500, 350);
    expect(status_of([&] { (void)conversions(RenderPipelineBuilder(3, {1000, 700}, 1, 8, q))
                               .add_inout_stage(Upsample2x{nullptr, 0}).add_inout_stage(Upsample2x{nullptr, 1}).add_inout_stage(Upsample2x{nullptr, 2})
                               .add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }, &msg) == JXLH_ERR_UNSUPPORTED &&
               has(msg, "upsampling / noise / chroma subsampling on a Modular frame"),
           "lower(): upsampling on a Modular list");
  }
  {
    const LoweredPipeline lo = filters(conversions(RenderPipelineBuilder(3, {1000, 700}, 0, 8, p)), p).add_save_stage({0, 1, 2}, 0, 3, 32).lower();
    expect(lo.modular == LoweredPipeline::Modular::kToF32 && !(lo.frame.flags & JXLH_FRAME_MODULAR) && lo.modular_sample_format == 0,
           "lower(): the caller-held-planes form lowers as before");
  }
  if (g_failed) return 1;
  printf("modular frame lowering: ok\n");
  return 0;
}
