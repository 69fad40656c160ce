// Host-side lowering of BlendingStage + ExtendToImageDimensionsStage (include/jxl_hip_lowering.hpp): accepted at the
// reference's position -- behind the colour stage, the blending stage followed at once by the extend stage, in front of
// the conversion / save stages (frame/render.rs:754-791) -- and lowered to a jxlh_blend_desc with the colour stage
// moved into the blend call.  No GPU involved.
#include <cstdio>
#include <string>

#include "lowering_helpers.h"

using namespace jxlh;
using namespace lowering_helpers;

namespace {
const jxlh_blending_info kColour{JXLH_BLEND_BLEND, 0, 1, 2};
const jxlh_blending_info kAlpha{JXLH_BLEND_ALPHA_WEIGHTED_ADD, 0, 0, 1};
BlendingStage blending(size_t num_ec) { return lowering_helpers::blending(-40, 100, 1280, 1024, kColour, num_ec, kAlpha); }
ExtendToImageDimensionsStage extend(size_t num_ec) { return extend_of(blending(num_ec)); }
RenderPipelineBuilder start(const jxlh_frame_params& p, size_t channels = 3) {
  return RenderPipelineBuilder(channels, {512, 384}, 0, 8, p)
      .add_inout_stage(GaborishStage{0, p.gab_w1[0], p.gab_w2[0]})
      .add_inout_stage(GaborishStage{1, p.gab_w1[1], p.gab_w2[1]})
      .add_inout_stage(GaborishStage{2, p.gab_w1[2], p.gab_w2[2]});
}
RenderPipelineBuilder u8_tail(RenderPipelineBuilder b) {
  return std::move(b)
      .add_inout_stage(ConvertF32ToU8Stage{0, 8})
      .add_inout_stage(ConvertF32ToU8Stage{1, 8})
      .add_inout_stage(ConvertF32ToU8Stage{2, 8})
      .add_save_stage({0, 1, 2}, 0, 4, 8);
}
}  // namespace

int main() {
  const jxlh_frame_params p = base(512, 384);
  const std::array<float, 3> lum{0.2627f, 0.678f, 0.0593f};
  // the reference's order: XybStage, FromLinearStage, BlendingStage, extend, conversions, save
  {
    const LoweredPipeline lp = u8_tail(start(p)
                                           .add_inplace_stage(XybStage{0, xyb()})
                                           .add_inplace_stage(FromLinearStage{0, JXLH_TF_PQ, 4000.0f, lum})
                                           .add_inplace_stage(blending(0))
                                           .add_extend_stage(extend(0)))
                                   .lower();
    expect(lp.has_blend, "the list blends");
    expect(lp.blend.x0 == -40 && lp.blend.y0 == 100 && lp.blend.image_w == 1280 && lp.blend.image_h == 1024, "origin and image size");
    expect(lp.blend.color.mode == JXLH_BLEND_BLEND && lp.blend.color.alpha_channel == 0 && lp.blend.color.clamp == 1 &&
               lp.blend.color.source == 2 && lp.blend.num_ec == 0,
           "blending_info");
    expect(lp.output.color == JXLH_COLOR_NONE && lp.output.transfer == JXLH_TF_LINEAR, "the output pass has no colour stage left");
    expect(lp.blend_colour.color == JXLH_COLOR_XYB && lp.blend_colour.transfer == JXLH_TF_PQ && lp.blend_colour.tf_param == 4000.0f &&
               lp.blend_colour.xyb.opsin_inverse_matrix[8] == 8.5f && lp.blend_colour.xyb.intensity_scale == 0.75f &&
               lp.blend_colour.hlg_luminance_rgb[1] == 0.678f,
           "the colour stage moved into the blend call");
    expect(lp.has_output && lp.output.bits == 8 && lp.output.channels == 4, "the conversion tail is kept");
    expect(lp.out_w == 1280 && lp.out_h == 1024, "the output is image-sized");
    expect(lp.frame.gab == 1 && lp.frame.xsize == 512 && lp.frame.ysize == 384, "the frame keeps its own size and filters");
    bool b = false, e = false;
    for (const auto& s : lp.stages) b |= s == "blending", e |= s == "extend-to-image-dims";
    expect(b && e, "both stages are listed under the reference's names");
  }
  // with extra channels, YCbCr, planar f32 save
  {
    const LoweredPipeline lp = RenderPipelineBuilder(5, {512, 384}, 0, 8, p)
                                   .add_inout_stage(ConvertModularToF32Stage{3, 8})
                                   .add_inout_stage(ConvertModularToF32Stage{4, 16})
                                   .add_inout_stage(Epf1Stage{1.0f, p.epf_border_sad_mul, {1.0f, 1.0f, 1.0f}})
                                   .add_inplace_stage(YcbcrToRgbStage{0})
                                   .add_inplace_stage(blending(2))
                                   .add_extend_stage(extend(2))
                                   .add_save_stage({0, 1, 2}, 0, 3, 32)
                                   .lower();
    expect(lp.has_blend && lp.blend.num_ec == 2 && lp.blend.ec[1].mode == JXLH_BLEND_ALPHA_WEIGHTED_ADD && lp.blend.ec[1].source == 1 &&
               lp.blend.ec_flags[0] == JXLH_EC_ALPHA && lp.blend.ec_flags[1] == JXLH_EC_ALPHA,
           "ec_blending_info and flags");
    expect(lp.blend_colour.color == JXLH_COLOR_YCBCR && lp.output.color == JXLH_COLOR_NONE && !lp.has_output, "YCbCr in front, f32 planes out");
    expect(lp.out_w == 1280 && lp.out_h == 1024, "image-sized planes");
  }
  // no colour stage at all (the frame is in the output colour space already)
  {
    const LoweredPipeline lp =
        start(p).add_inplace_stage(blending(0)).add_extend_stage(extend(0)).add_save_stage({0, 1, 2}, 0, 3, 32).lower();
    expect(lp.has_blend && lp.blend_colour.color == JXLH_COLOR_NONE, "blending without a colour stage");
  }
  // a list that does not blend is what it was
  {
    const LoweredPipeline lp = u8_tail(start(p).add_inplace_stage(XybStage{0, xyb()})).lower();
    expect(!lp.has_blend && lp.output.color == JXLH_COLOR_XYB && lp.out_w == 512 && lp.out_h == 384, "no blending: frame-sized, colour in the output pass");
  }
  // misplaced orders: JXLH_ERR_INVALID_ARGUMENT
  std::string msg;
  expect(status_of([&] { (void)start(p).add_extend_stage(extend(0)).add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }, &msg) ==
                 JXLH_ERR_INVALID_ARGUMENT && msg.find("without a blending stage") != std::string::npos,
         "an extend stage without a blending stage");
  expect(status_of([&] { (void)start(p).add_inplace_stage(blending(0)).add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }) ==
             JXLH_ERR_INVALID_ARGUMENT,
         "a blending stage without the extend stage");
  expect(status_of([&] { (void)start(p).add_inplace_stage(blending(0)).lower(); }) == JXLH_ERR_INVALID_ARGUMENT,
         "a blending stage at the end of the list");
  expect(status_of([&] { (void)start(p).add_inplace_stage(blending(0)).add_inplace_stage(blending(0)).add_extend_stage(extend(0))
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }) == JXLH_ERR_INVALID_ARGUMENT,
         "two blending stages in a row");
  expect(status_of([&] { (void)start(p).add_inplace_stage(blending(0)).add_extend_stage(extend(0)).add_inplace_stage(blending(0))
                             .add_extend_stage(extend(0)).add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }) == JXLH_ERR_INVALID_ARGUMENT,
         "two blending stages");
  expect(status_of([&] { (void)start(p).add_inplace_stage(blending(0)).add_extend_stage(extend(0)).add_extend_stage(extend(0))
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }, &msg) == JXLH_ERR_INVALID_ARGUMENT &&
             msg.find("two extend") != std::string::npos,
         "two extend stages");
  expect(status_of([&] { (void)u8_tail(start(p).add_inplace_stage(blending(0)).add_extend_stage(extend(0))
                                           .add_inplace_stage(XybStage{0, xyb()})).lower(); }, &msg) == JXLH_ERR_INVALID_ARGUMENT &&
             msg.find("before the colour stage") != std::string::npos,
         "blending before the colour stage");
  expect(status_of([&] { (void)start(p).add_inplace_stage(XybStage{0, xyb()}).add_inplace_stage(blending(0)).add_extend_stage(extend(0))
                             .add_inplace_stage(FromLinearStage{0, JXLH_TF_SRGB, 0.0f, lum}).add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }) ==
             JXLH_ERR_INVALID_ARGUMENT,
         "blending between XybStage and FromLinearStage");
  expect(status_of([&] { (void)start(p).add_inplace_stage(blending(0)).add_inplace_stage(XybStage{0, xyb()}).add_extend_stage(extend(0))
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }) == JXLH_ERR_INVALID_ARGUMENT,
         "a stage between blending and extend");
  expect(status_of([&] { (void)start(p)
                             .add_inout_stage(ConvertF32ToU8Stage{0, 8})
                             .add_inout_stage(ConvertF32ToU8Stage{1, 8})
                             .add_inout_stage(ConvertF32ToU8Stage{2, 8})
                             .add_inplace_stage(blending(0))
                             .add_extend_stage(extend(0))
                             .add_save_stage({0, 1, 2}, 0, 3, 8).lower(); }) == JXLH_ERR_INVALID_ARGUMENT,
         "blending behind the conversions");
  // the two stages come from the same headers
  {
    ExtendToImageDimensionsStage other = extend(0);
    other.x0 = 7;
    expect(status_of([&] { (void)start(p).add_inplace_stage(blending(0)).add_extend_stage(other).add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }) ==
               JXLH_ERR_INVALID_ARGUMENT,
           "extend stage with another origin");
  }
  // extra channels of the stage and of the list
  expect(status_of([&] { (void)start(p).add_inplace_stage(blending(1)).add_extend_stage(extend(1)).add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }) ==
             JXLH_ERR_INVALID_ARGUMENT,
         "ec_blending_info for an extra channel the list does not hold");
  // the builder's argument-less extend stage and the reference's stages by name stay outside the path, as before
  expect(status_of([&] { (void)start(p).add_extend_stage().add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }) == JXLH_ERR_UNSUPPORTED,
         "add_extend_stage() without arguments is still unsupported");
  expect(status_of([&] { (void)start(p).add_inplace_stage(CpuOnlyStage{"blending"}).add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }) ==
             JXLH_ERR_UNSUPPORTED,
         "CpuOnlyStage{\"blending\"} is still unsupported");
  // a Modular frame blends through jxlh_stage_blend
  expect(status_of([&] { (void)RenderPipelineBuilder(3, {512, 384}, 0, 8, p)
                             .add_inout_stage(ConvertModularToF32Stage{0, 8})
                             .add_inout_stage(ConvertModularToF32Stage{1, 8})
                             .add_inout_stage(ConvertModularToF32Stage{2, 8})
                             .add_inplace_stage(blending(0))
                             .add_extend_stage(extend(0))
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }, &msg) == JXLH_ERR_UNSUPPORTED &&
             msg.find("Modular") != std::string::npos,
         "blending on a Modular frame");
  if (g_failed) return 1;
  printf("blending lowering: ok\n");
  return 0;
}
