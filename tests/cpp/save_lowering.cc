// Host-side lowering of the save tail (include/jxl_hip_lowering.hpp): SpotColorStage, PremultiplyAlphaStage, the
// conversions to u8 / u16 / f16 at any bit depth and on extra channels, and the six-argument save stage, in the order of
// Frame::build_render_pipeline (frame/render.rs:793-903), lower to one jxlh_save_desc per output buffer; lists out of
// that order fail naming the stage; lists without these stages lower to what they did.  No GPU involved.
#include <cstdio>
#include <string>

#include "lowering_helpers.h"

using namespace jxlh;
using namespace lowering_helpers;

namespace {
const std::array<float, 3> kLum{0.2627f, 0.678f, 0.0593f};

BlendingStage blending(size_t num_ec) {
  return lowering_helpers::blending(-4, 9, 640, 480, jxlh_blending_info{JXLH_BLEND_BLEND, 0, 1, 0}, num_ec, jxlh_blending_info{JXLH_BLEND_BLEND, 0, 0, 0});
}
ExtendToImageDimensionsStage extend(size_t num_ec) { return extend_of(blending(num_ec)); }
// a VarDCT frame with `num_ec` 16-bit extra channels, Gaborish, XYB + sRGB
RenderPipelineBuilder start(const jxlh_frame_params& p, int num_ec, uint32_t tf = JXLH_TF_SRGB) {
  auto b = RenderPipelineBuilder(3 + num_ec, {512, 384}, 0, 8, p);
  for (int i = 0; i < num_ec; i++) b = std::move(b).add_inout_stage(ConvertModularToF32Stage{3 + i, 16});
  return std::move(b)
      .add_inout_stage(GaborishStage{0, p.gab_w1[0], p.gab_w2[0]})
      .add_inout_stage(GaborishStage{1, p.gab_w1[1], p.gab_w2[1]})
      .add_inout_stage(GaborishStage{2, p.gab_w1[2], p.gab_w2[2]})
      .add_inplace_stage(XybStage{0, xyb()})
      .add_inplace_stage(FromLinearStage{0, tf, tf == JXLH_TF_PQ ? 10000.0f : 0.0f, kLum});
}
// add_conversion_stages (frame/render.rs:868-873)
RenderPipelineBuilder convert(RenderPipelineBuilder b, const std::vector<int>& chs, DataFormat df, bool clamp = false,
                              float lo = 0.0f, float hi = 0.0f) {
  for (int c : chs) {
    if (df.format == JXLH_SAVE_U8) b = std::move(b).add_inout_stage(ConvertF32ToU8Stage{c, (uint8_t)df.bit_depth});
    if (df.format == JXLH_SAVE_U16) b = std::move(b).add_inout_stage(ConvertF32ToU16Stage{c, (uint8_t)df.bit_depth});
    if (df.format == JXLH_SAVE_F16) b = std::move(b).add_inout_stage(ConvertF32ToF16Stage{c, clamp, lo, hi});
  }
  return b;
}
bool channels_are(const jxlh_save_desc& d, std::initializer_list<uint32_t> want) {
  if (d.n_channels != want.size()) return false;
  size_t k = 0;
  for (uint32_t c : want)
    if (d.channels[k++] != c) return false;
  return true;
}
}  // namespace

int main() {
  jxlh_frame_params p;
  jxlh_default_frame_params(&p, 512, 384);
  std::string msg;
  // RGBA with real alpha, 8 bit, orientation 6
  {
    const LoweredPipeline lp = convert(start(p, 1), {0, 1, 2, 3}, DataFormat::u8())
                                   .add_save_stage({0, 1, 2, 3}, 6, 0, ColorType::kRgba, DataFormat::u8(), false)
                                   .lower();
    expect(lp.saves.size() == 1 && !lp.has_output, "RGBA: one save descriptor, no legacy output");
    const jxlh_save_desc& d = lp.saves[0];
    expect(channels_are(d, {0, 1, 2, 3}) && !d.fill_opaque_alpha && d.format == JXLH_SAVE_U8 && d.bit_depth == 8 &&
               d.orientation == 6 && !d.premultiply && d.n_spot == 0 && !d.big_endian,
           "RGBA: descriptor");
    expect(lp.output.color == JXLH_COLOR_XYB && lp.output.transfer == JXLH_TF_SRGB && lp.output.xyb.intensity_scale == 0.75f,
           "RGBA: the colour stage in front of the save");
    expect(lp.frame.gab == 1 && lp.extra[0].bits == 16 && lp.out_w == 512 && lp.out_h == 384, "RGBA: the rest of the list");
  }
  // RGBA without an alpha channel: fill
  {
    const LoweredPipeline lp = convert(start(p, 0), {0, 1, 2}, DataFormat::u8())
                                   .add_save_stage({0, 1, 2}, 1, 0, ColorType::kRgba, DataFormat::u8(), true)
                                   .lower();
    expect(lp.saves.size() == 1 && channels_are(lp.saves[0], {0, 1, 2}) && lp.saves[0].fill_opaque_alpha, "RGBA filled");
  }
  // gray + alpha from extra channel 1, 16 bit big endian
  {
    const LoweredPipeline lp = convert(start(p, 2), {0, 4}, DataFormat::u16(16, true))
                                   .add_save_stage({0, 4}, 1, 0, ColorType::kGrayscaleAlpha, DataFormat::u16(16, true), false)
                                   .lower();
    expect(lp.saves.size() == 1 && channels_are(lp.saves[0], {0, 4}) && lp.saves[0].format == JXLH_SAVE_U16 &&
               lp.saves[0].bit_depth == 16 && lp.saves[0].big_endian,
           "gray + alpha");
  }
  // BGRA premultiplied
  {
    const LoweredPipeline lp = convert(start(p, 1).add_inplace_stage(PremultiplyAlphaStage{0, 3, 3}), {0, 1, 2, 3}, DataFormat::u8())
                                   .add_save_stage({0, 1, 2, 3}, 1, 0, ColorType::kBgra, DataFormat::u8(), false)
                                   .lower();
    expect(lp.saves.size() == 1 && channels_are(lp.saves[0], {2, 1, 0, 3}) && lp.saves[0].premultiply &&
               lp.saves[0].premultiply_alpha_channel == 3,
           "BGRA premultiplied: channels 0 and 2 trade places, the alpha's channel is carried");
  }
  // two spot colours in front of an RGB f32 save (no conversion stages for f32)
  {
    const LoweredPipeline lp = start(p, 3)
                                   .add_inplace_stage(SpotColorStage{0, {0.1f, 0.2f, 0.3f, 0.4f}})
                                   .add_inplace_stage(SpotColorStage{2, {0.5f, 0.6f, 0.7f, 0.8f}})
                                   .add_save_stage({0, 1, 2}, 3, 0, ColorType::kRgb, DataFormat::f32(true), false)
                                   .lower();
    const jxlh_save_desc& d = lp.saves.at(0);
    expect(d.n_spot == 2 && d.spot[0].ec == 0 && d.spot[0].rgba[3] == 0.4f && d.spot[1].ec == 2 && d.spot[1].rgba[0] == 0.5f &&
               d.format == JXLH_SAVE_F32 && d.big_endian && d.orientation == 3,
           "spot colours in list order");
  }
  // f16 with the PQ clamp
  {
    const LoweredPipeline lp = convert(start(p, 0, JXLH_TF_PQ), {0, 1, 2}, DataFormat::f16(), true, 0.0f, 1.0f)
                                   .add_save_stage({0, 1, 2}, 1, 0, ColorType::kRgb, DataFormat::f16(), false)
                                   .lower();
    const jxlh_save_desc& d = lp.saves.at(0);
    expect(d.format == JXLH_SAVE_F16 && d.f16_clamp && d.f16_clamp_min == 0.0f && d.f16_clamp_max == 1.0f &&
               lp.output.transfer == JXLH_TF_PQ,
           "f16 with the PQ clamp");
  }
  // 10 bits in a u16
  {
    const LoweredPipeline lp = convert(start(p, 0), {0, 1, 2}, DataFormat::u16(10))
                                   .add_save_stage({0, 1, 2}, 1, 0, ColorType::kRgb, DataFormat::u16(10), false)
                                   .lower();
    expect(lp.saves.at(0).format == JXLH_SAVE_U16 && lp.saves.at(0).bit_depth == 10, "10-bit u16");
  }
  // colour + two extra-channel buffers (frame/render.rs:888-902): the extra-channel saves carry no spot / premultiply
  {
    auto b = convert(start(p, 2).add_inplace_stage(SpotColorStage{1, {1.0f, 0.0f, 0.0f, 0.5f}})
                         .add_inplace_stage(PremultiplyAlphaStage{0, 3, 3}),
                     {0, 1, 2, 3}, DataFormat::u8())
                 .add_save_stage({0, 1, 2, 3}, 8, 0, ColorType::kRgba, DataFormat::u8(), false);
    b = convert(std::move(b), {3}, DataFormat::u8()).add_save_stage({3}, 8, 1, ColorType::kGrayscale, DataFormat::u8(), false);
    b = convert(std::move(b), {4}, DataFormat::u16(12)).add_save_stage({4}, 8, 2, ColorType::kGrayscale, DataFormat::u16(12), false);
    const LoweredPipeline lp = std::move(b).lower();
    expect(lp.saves.size() == 3, "three output buffers");
    expect(lp.saves[0].n_spot == 1 && lp.saves[0].premultiply && channels_are(lp.saves[0], {0, 1, 2, 3}), "buffer 0: colour");
    expect(channels_are(lp.saves[1], {3}) && lp.saves[1].n_spot == 0 && !lp.saves[1].premultiply && lp.saves[1].orientation == 8,
           "buffer 1: extra channel 0");
    expect(channels_are(lp.saves[2], {4}) && lp.saves[2].format == JXLH_SAVE_U16 && lp.saves[2].bit_depth == 12 &&
               lp.saves[2].n_spot == 0,
           "buffer 2: extra channel 1");
  }
  // behind a blend the colour stage has moved into the blend call; a spot colour behind blend / extend is the
  // reference's order (frame/render.rs:765-806)
  {
    const LoweredPipeline lp = convert(start(p, 1).add_inplace_stage(blending(1)).add_extend_stage(extend(1))
                                           .add_inplace_stage(SpotColorStage{0, {0.1f, 0.2f, 0.3f, 0.4f}}),
                                       {0, 1, 2, 3}, DataFormat::u8())
                                   .add_save_stage({0, 1, 2, 3}, 5, 0, ColorType::kRgba, DataFormat::u8(), false)
                                   .lower();
    expect(lp.has_blend && lp.blend_colour.color == JXLH_COLOR_XYB && lp.output.color == JXLH_COLOR_NONE && lp.saves.size() == 1 &&
               lp.saves[0].n_spot == 1 && lp.out_w == 640 && lp.out_h == 480,
           "save and spot colour behind a blend");
  }
  // ... and in front of it the device would blend first and apply them afterwards: another image than the list's
  expect(status_of([&] { (void)convert(start(p, 1).add_inplace_stage(SpotColorStage{0, {0.1f, 0.2f, 0.3f, 0.4f}})
                                           .add_inplace_stage(blending(1)).add_extend_stage(extend(1)), {0, 1, 2, 3}, DataFormat::u8())
                             .add_save_stage({0, 1, 2, 3}, 1, 0, ColorType::kRgba, DataFormat::u8(), false).lower(); }, &msg) ==
                 JXLH_ERR_INVALID_ARGUMENT && msg.find("'blending'") != std::string::npos,
         "a spot colour in front of the blending stage");
  expect(status_of([&] { (void)convert(start(p, 1).add_inplace_stage(PremultiplyAlphaStage{0, 3, 3})
                                           .add_inplace_stage(blending(1)).add_extend_stage(extend(1)), {0, 1, 2, 3}, DataFormat::u8())
                             .add_save_stage({0, 1, 2, 3}, 1, 0, ColorType::kRgba, DataFormat::u8(), false).lower(); }, &msg) ==
                 JXLH_ERR_INVALID_ARGUMENT && msg.find("'blending'") != std::string::npos,
         "premultiply in front of the blending stage");
  expect(status_of([&] { (void)convert(start(p, 0), {0, 1, 2}, DataFormat::f16())
                             .add_inplace_stage(blending(0)).add_extend_stage(extend(0))
                             .add_save_stage({0, 1, 2}, 1, 0, ColorType::kRgb, DataFormat::f16(), false).lower(); }, &msg) ==
                 JXLH_ERR_INVALID_ARGUMENT && msg.find("'blending'") != std::string::npos,
         "f16 conversions in front of the blending stage");
  expect(status_of([&] { (void)convert(start(p, 1), {3}, DataFormat::u16(10))
                             .add_inplace_stage(blending(1)).add_extend_stage(extend(1))
                             .add_save_stage({3}, 1, 0, ColorType::kGrayscale, DataFormat::u16(10), false).lower(); }, &msg) ==
                 JXLH_ERR_INVALID_ARGUMENT && msg.find("'blending'") != std::string::npos,
         "an extra channel's reduced-depth conversion in front of the blending stage");
  {
    auto b = convert(start(p, 0), {0, 1, 2}, DataFormat::u8()).add_save_stage({0, 1, 2}, 1, 0, ColorType::kRgb, DataFormat::u8(), false);
    expect(status_of([&] { (void)std::move(b).add_inplace_stage(blending(0)).add_extend_stage(extend(0)).lower(); }) ==
               JXLH_ERR_INVALID_ARGUMENT,
           "a blending stage behind a save stage");
  }
  // ---- out of order / inconsistent: the documented status, naming the stage
  expect(status_of([&] { (void)convert(start(p, 1), {0, 1, 2, 3}, DataFormat::u8())
                             .add_inplace_stage(SpotColorStage{0, {0, 0, 0, 1}})
                             .add_save_stage({0, 1, 2, 3}, 1, 0, ColorType::kRgba, DataFormat::u8(), false).lower(); }, &msg) ==
                 JXLH_ERR_INVALID_ARGUMENT && msg.find("spot color stage for channel 3") != std::string::npos,
         "spot colour behind the conversions");
  expect(status_of([&] { (void)convert(start(p, 1).add_inplace_stage(PremultiplyAlphaStage{0, 3, 3})
                                           .add_inplace_stage(SpotColorStage{0, {0, 0, 0, 1}}), {0, 1, 2, 3}, DataFormat::u8())
                             .add_save_stage({0, 1, 2, 3}, 1, 0, ColorType::kRgba, DataFormat::u8(), false).lower(); }, &msg) ==
                 JXLH_ERR_INVALID_ARGUMENT && msg.find("spot color") != std::string::npos,
         "spot colour behind premultiply");
  expect(status_of([&] { (void)convert(start(p, 1), {0}, DataFormat::u8())
                             .add_inplace_stage(PremultiplyAlphaStage{0, 3, 3})
                             .add_save_stage({0, 1, 2, 3}, 1, 0, ColorType::kRgba, DataFormat::u8(), false).lower(); }, &msg) ==
                 JXLH_ERR_INVALID_ARGUMENT && msg.find("premultiply alpha stage") != std::string::npos,
         "premultiply between the conversions");
  expect(status_of([&] { (void)convert(start(p, 1).add_inplace_stage(PremultiplyAlphaStage{0, 3, 2}), {0, 1, 2, 3}, DataFormat::u8())
                             .add_save_stage({0, 1, 2, 3}, 1, 0, ColorType::kRgba, DataFormat::u8(), false).lower(); }, &msg) ==
                 JXLH_ERR_INVALID_ARGUMENT && msg.find("premultiply alpha stage") != std::string::npos,
         "premultiply by a colour channel");
  expect(status_of([&] { (void)convert(start(p, 2).add_inplace_stage(PremultiplyAlphaStage{0, 3, 4}), {0, 1, 2, 3}, DataFormat::u8())
                             .add_save_stage({0, 1, 2, 3}, 1, 0, ColorType::kRgba, DataFormat::u8(), false).lower(); }, &msg) ==
                 JXLH_ERR_INVALID_ARGUMENT && msg.find("premultiply") != std::string::npos,
         "premultiply by another channel than the save's alpha");
  expect(status_of([&] { (void)start(p, 1).add_inplace_stage(SpotColorStage{1, {0, 0, 0, 1}})
                             .add_save_stage({0, 1, 2}, 1, 0, ColorType::kRgb, DataFormat::f32(), false).lower(); }, &msg) ==
                 JXLH_ERR_INVALID_ARGUMENT && msg.find("spot color stage for channel 4") != std::string::npos,
         "spot colour from an extra channel the list does not hold");
  expect(status_of([&] { (void)convert(start(p, 0), {0, 1, 2}, DataFormat::u16(16))
                             .add_save_stage({0, 1, 2}, 1, 0, ColorType::kRgb, DataFormat::u8(), false).lower(); }, &msg) ==
                 JXLH_ERR_INVALID_ARGUMENT && msg.find("convert F32 to U16 in channel 0") != std::string::npos,
         "conversion and save disagree on the format");
  expect(status_of([&] { (void)convert(start(p, 0), {0, 1, 2}, DataFormat::u16(10))
                             .add_save_stage({0, 1, 2}, 1, 0, ColorType::kRgb, DataFormat::u16(12), false).lower(); }, &msg) ==
                 JXLH_ERR_INVALID_ARGUMENT && msg.find("bit depth") != std::string::npos,
         "conversion and save disagree on the depth");
  expect(status_of([&] { (void)convert(start(p, 0), {0, 1}, DataFormat::u8())
                             .add_save_stage({0, 1, 2}, 1, 0, ColorType::kRgb, DataFormat::u8(), false).lower(); }, &msg) ==
                 JXLH_ERR_INVALID_ARGUMENT && msg.find("channel 2 has no conversion") != std::string::npos,
         "a saved channel without its conversion");
  expect(status_of([&] { (void)convert(start(p, 1), {0, 1, 2, 3}, DataFormat::u8())
                             .add_save_stage({0, 1, 2}, 1, 0, ColorType::kRgb, DataFormat::u8(), false).lower(); }, &msg) ==
                 JXLH_ERR_INVALID_ARGUMENT && msg.find("convert F32 to U8 in channel 3") != std::string::npos,
         "a conversion the save does not use");
  expect(status_of([&] { (void)convert(start(p, 0), {0, 1, 2}, DataFormat::u8())
                             .add_save_stage({0, 1, 2}, 1, 0, ColorType::kRgba, DataFormat::u8(), false).lower(); }, &msg) ==
                 JXLH_ERR_INVALID_ARGUMENT && msg.find("save stage for buffer 0") != std::string::npos,
         "RGBA with three channels and no fill");
  expect(status_of([&] { (void)convert(start(p, 0), {0, 1, 2}, DataFormat::u8())
                             .add_save_stage({0, 1, 2}, 1, 0, ColorType::kRgb, DataFormat::u8(), true).lower(); }) ==
             JXLH_ERR_INVALID_ARGUMENT,
         "fill_opaque_alpha on a colour type without alpha");
  expect(status_of([&] { (void)convert(start(p, 0), {0, 1, 2}, DataFormat::u8())
                             .add_save_stage({0, 1, 2}, 9, 0, ColorType::kRgb, DataFormat::u8(), false).lower(); }) ==
             JXLH_ERR_INVALID_ARGUMENT,
         "orientation 9");
  expect(status_of([&] { (void)convert(start(p, 0), {0, 1, 2}, DataFormat::u8())
                             .add_save_stage({0, 1, 2}, 1, 1, ColorType::kRgb, DataFormat::u8(), false).lower(); }, &msg) ==
                 JXLH_ERR_INVALID_ARGUMENT && msg.find("buffer order") != std::string::npos,
         "the first save into buffer 1");
  expect(status_of([&] { (void)convert(start(p, 0), {0, 1, 2}, DataFormat::f16(), true, 1.0f, 0.0f)
                             .add_save_stage({0, 1, 2}, 1, 0, ColorType::kRgb, DataFormat::f16(), false).lower(); }, &msg) ==
                 JXLH_ERR_INVALID_ARGUMENT && msg.find("convert F32 to F16 in channel 0") != std::string::npos,
         "f16 clamp with min > max");
  expect(status_of([&] { (void)convert(start(p, 0), {0, 1, 2}, DataFormat::u8())
                             .add_save_stage({0, 1, 2}, 1, 0, ColorType::kRgb, DataFormat::u8(), false)
                             .add_inout_stage(ConvertF32ToU8Stage{0, 8}).lower(); }, &msg) ==
                 JXLH_ERR_INVALID_ARGUMENT && msg.find("without a save stage behind it") != std::string::npos,
         "a conversion at the end of the list");
  {
    auto b = convert(start(p, 0), {0, 1, 2}, DataFormat::u8()).add_save_stage({0, 1, 2}, 1, 0, ColorType::kRgb, DataFormat::u8(), false);
    expect(status_of([&] { (void)convert(std::move(b), {0, 1, 2}, DataFormat::u8())
                               .add_save_stage({0, 1, 2}, 1, 1, ColorType::kRgb, DataFormat::u8(), false).lower(); }, &msg) ==
                   JXLH_ERR_UNSUPPORTED && msg.find("second save of the colour") != std::string::npos,
           "two colour saves");
  }
  // the stages without the save stage that can express them, and the reference's stages by name, stay outside the path
  expect(status_of([&] { (void)convert(start(p, 0), {0, 1, 2}, DataFormat::u16(10)).add_save_stage({0, 1, 2}, 0, 3, 16).lower(); }) ==
             JXLH_ERR_UNSUPPORTED,
         "10-bit conversions in front of the four-argument save stage");
  expect(status_of([&] { (void)start(p, 1).add_inplace_stage(SpotColorStage{0, {0, 0, 0, 1}}).add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }) ==
             JXLH_ERR_UNSUPPORTED,
         "a spot colour in front of the four-argument save stage");
  expect(status_of([&] { (void)start(p, 0).add_inout_stage(ConvertF32ToU8Stage{0, 9}).add_save_stage({0, 1, 2}, 0, 3, 8).lower(); }) ==
             JXLH_ERR_UNSUPPORTED,
         "a depth above the sample size in front of the four-argument save stage: the status it had");
  expect(status_of([&] { (void)convert(start(p, 1), {0, 1, 2, 3}, DataFormat::u8()).add_save_stage({0, 1, 2}, 0, 3, 8).lower(); }) ==
             JXLH_ERR_INVALID_ARGUMENT,
         "an extra channel's conversion in front of the four-argument save stage: the status it had");
  expect(status_of([&] { (void)start(p, 0).add_inplace_stage(CpuOnlyStage{"spot color"})
                             .add_save_stage({0, 1, 2}, 1, 0, ColorType::kRgb, DataFormat::f32(), false).lower(); }, &msg) ==
                 JXLH_ERR_UNSUPPORTED && msg.find("spot color") != std::string::npos,
         "CpuOnlyStage by name is still unsupported");
  // a Modular frame reaches the pass through jxlh_stage_save
  expect(status_of([&] { (void)convert(RenderPipelineBuilder(3, {512, 384}, 0, 8, p)
                                           .add_inout_stage(ConvertModularToF32Stage{0, 8})
                                           .add_inout_stage(ConvertModularToF32Stage{1, 8})
                                           .add_inout_stage(ConvertModularToF32Stage{2, 8}), {0, 1, 2}, DataFormat::u16(10))
                             .add_save_stage({0, 1, 2}, 1, 0, ColorType::kRgb, DataFormat::u16(10), false).lower(); }, &msg) ==
                 JXLH_ERR_UNSUPPORTED && msg.find("Modular") != std::string::npos,
         "the save tail on a Modular frame");
  // ---- lists 1-4 of tests/cpp/pipeline_builder.cc, verbatim, lower to the fields that file asserts, and to no save
  // descriptor
  {
    const jxlh_frame_params base = VarDctFrame::default_params(1000, 700);
    const Rf rf = rf_of(base);
    // 1. the common VarDCT list: Gaborish x3, EPF1, EPF2, XYB, sRGB, U8 x3, save RGBA
    {
      auto b = add_filters(RenderPipelineBuilder(3, {1000, 700}, 0, 8, base), rf, true, 2);
      b = std::move(b)
              .add_inplace_stage(XybStage{0, some_xyb()})
              .add_inplace_stage(FromLinearStage{0, JXLH_TF_SRGB, 0.0f, {0.f, 0.f, 0.f}})
              .add_inout_stage(ConvertF32ToU8Stage{0, 8})
              .add_inout_stage(ConvertF32ToU8Stage{1, 8})
              .add_inout_stage(ConvertF32ToU8Stage{2, 8})
              .add_save_stage({0, 1, 2}, 0, 4, 8);
      const LoweredPipeline lp = b.lower();
      expect(lp.frame.gab == 1 && lp.frame.epf_iters == 2 && lp.frame.upsampling == 1 && lp.frame.noise == 0, "list 1: stage-derived fields");
      expect(lp.frame.gab_w1[1] == rf.gab_w1[1] && lp.frame.epf_pass2_sigma_scale == rf.pass2, "list 1: weights carried over");
      expect(lp.input_border.x == 4 && lp.input_border.y == 4, "list 1: accumulated border is 4");
      expect(lp.has_output && lp.output.color == JXLH_COLOR_XYB && lp.output.transfer == JXLH_TF_SRGB && lp.output.bits == 8 &&
                 lp.output.channels == 4,
             "list 1: output descriptor");
      expect(lp.stages.size() == 11 && lp.stages[0] == "Gaborish filter for channel 0", "list 1: Display strings");
      expect(lp.saves.empty() && lp.modular == LoweredPipeline::Modular::kNone && !lp.has_blend, "list 1: no save descriptor");
    }
    // 2. epf_iters = 3, planar f32 save: border 1 + 3 + 2 + 1
    {
      auto b = add_filters(RenderPipelineBuilder(3, {1000, 700}, 0, 8, base), rf, true, 3);
      const LoweredPipeline lp = std::move(b).add_save_stage({0, 1, 2}, 0, 3, 32).lower();
      expect(lp.frame.epf_iters == 3 && lp.input_border.x == 7 && !lp.has_output, "list 2: three EPF passes");
      expect(lp.saves.empty(), "list 2: no save descriptor");
    }
    // 3. a JPEG recompression: 4:2:0 chroma, no filters, YCbCr, U8, RGB
    {
      auto b = RenderPipelineBuilder(3, {1000, 700}, 0, 8, base)
                   .add_inout_stage(HorizontalChromaUpsample{0})
                   .add_inout_stage(VerticalChromaUpsample{0})
                   .add_inout_stage(HorizontalChromaUpsample{2})
                   .add_inout_stage(VerticalChromaUpsample{2})
                   .add_inplace_stage(YcbcrToRgbStage{0})
                   .add_inout_stage(ConvertF32ToU8Stage{0, 8})
                   .add_inout_stage(ConvertF32ToU8Stage{1, 8})
                   .add_inout_stage(ConvertF32ToU8Stage{2, 8})
                   .add_save_stage({0, 1, 2}, 0, 3, 8);
      const LoweredPipeline lp = b.lower();
      expect(lp.frame.hshift[0] == 1 && lp.frame.vshift[0] == 1 && lp.frame.hshift[1] == 0 && lp.frame.hshift[2] == 1 &&
                 lp.frame.gab == 0 && lp.frame.epf_iters == 0,
             "list 3: chroma shifts");
      expect(lp.output.color == JXLH_COLOR_YCBCR && lp.output.channels == 3, "list 3: YCbCr output");
      expect(lp.saves.empty() && lp.has_output && lp.output.bits == 8, "list 3: no save descriptor");
    }
    // 4. 2x frame upsampling + noise: size is size_upsampled, three noise temporaries behind the image channels
    {
      jxlh_frame_params small = VarDctFrame::default_params(500, 350);
      auto b = add_filters(RenderPipelineBuilder(6, {1000, 700}, 1, 8, small), rf_of(small), true, 1);
      std::array<float, 8> lut{0.1f, 0.2f, 0.3f, 0.4f, 0.5f, 0.6f, 0.7f, 0.8f};
      b = std::move(b)
              .add_inout_stage(Upsample2x{nullptr, 0})
              .add_inout_stage(Upsample2x{nullptr, 1})
              .add_inout_stage(Upsample2x{nullptr, 2})
              .add_inout_stage(ConvolveNoiseStage{3})
              .add_inout_stage(ConvolveNoiseStage{4})
              .add_inout_stage(ConvolveNoiseStage{5})
              .add_inplace_stage(AddNoiseStage{lut, 3, -2, 3})
              .add_save_stage({0, 1, 2}, 0, 3, 32);
      const LoweredPipeline lp = b.lower();
      expect(lp.frame.upsampling == 2 && lp.frame.xsize_upsampled == 1000 && lp.frame.ysize_upsampled == 700, "list 4: upsampling");
      expect(lp.frame.noise == 1 && lp.frame.noise_lut[7] == 0.8f && lp.frame.ytox_lf == 3 && lp.frame.ytob_lf == -2, "list 4: noise");
      expect(lp.input_border.x == 3, "list 4: border counts the stages before the upsampling");
      expect(lp.saves.empty() && !lp.has_output, "list 4: no save descriptor");
    }
    // and the Modular I32 -> U8 special case
    const LoweredPipeline m = RenderPipelineBuilder(3, {512, 384}, 0, 8, p)
                                  .add_inout_stage(ConvertModularToF32Stage{0, 4})
                                  .add_inout_stage(ConvertModularToF32Stage{1, 4})
                                  .add_inout_stage(ConvertModularToF32Stage{2, 4})
                                  .add_inout_stage(ConvertF32ToU8Stage{0, 8})
                                  .add_inout_stage(ConvertF32ToU8Stage{1, 8})
                                  .add_inout_stage(ConvertF32ToU8Stage{2, 8})
                                  .add_save_stage({0, 1, 2}, 0, 3, 8)
                                  .lower();
    expect(m.saves.empty() && m.modular == LoweredPipeline::Modular::kI32ToU8 && m.i32_to_u8_multiplier == 17,
           "the Modular I32 -> U8 special case as before");
  }
  if (g_failed) return 1;
  printf("save lowering: ok\n");
  return 0;
}
