// Host-side lowering of PatchesStage (include/jxl_hip_lowering.hpp): accepted at the reference's position -- after the
// filters and the extra channels' own upsampling, before the colour upsampling, noise and the colour stage
// (frame/render.rs:624-683) -- and only on a VarDCT frame.  No GPU involved.
#include <cstdio>
#include <string>

#include "lowering_helpers.h"

using namespace jxlh;
using namespace lowering_helpers;

namespace {
PatchesStage dict(size_t num_ec) {
  PatchesStage ps;
  ps.patches = {jxlh_patch{4, 5, 0, 0, 0, 16, 12}, jxlh_patch{40, 30, 1, 8, 2, 10, 20}};
  ps.blendings.assign(ps.patches.size() * (1 + num_ec), jxlh_patch_blending{JXLH_PATCH_BLEND_ABOVE, 0, 1});
  ps.ec_flags.assign(num_ec, JXLH_EC_ALPHA);
  return ps;
}
}  // namespace

int main() {
  const jxlh_frame_params p = base(1000, 700);
  // accepted: filters -> patches -> save
  {
    const LoweredPipeline lp =
        filters(RenderPipelineBuilder(3, {1000, 700}, 0, 8, p), p).add_inplace_stage(dict(0)).add_save_stage({0, 1, 2}, 0, 3, 32).lower();
    expect(lp.has_patches && lp.patches.patches.size() == 2 && lp.patches.blendings.size() == 2, "filters -> patches lowers");
    expect(lp.frame.gab == 1 && lp.frame.epf_iters == 1, "the filters are kept");
    bool named = false;
    for (const auto& s : lp.stages) named |= s == "patches";
    expect(named, "the stage is listed by name");
  }
  // accepted: extra channel conversion + its own upsampling -> patches -> colour upsampling -> noise
  {
    jxlh_frame_params q = base(500, 350);
    const LoweredPipeline lp = RenderPipelineBuilder(7, {1000, 700}, 1, 8, q)
                                   .add_inout_stage(ConvertModularToF32Stage{3, 8})
                                   .add_inout_stage(Upsample4x{nullptr, 3})
                                   .add_inplace_stage(dict(1))
                                   .add_inout_stage(Upsample2x{nullptr, 0})
                                   .add_inout_stage(Upsample2x{nullptr, 1})
                                   .add_inout_stage(Upsample2x{nullptr, 2})
                                   .add_inout_stage(ConvolveNoiseStage{4})
                                   .add_inout_stage(ConvolveNoiseStage{5})
                                   .add_inout_stage(ConvolveNoiseStage{6})
                                   .add_inplace_stage(AddNoiseStage{{0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f}, 0, 0, 4})
                                   .add_save_stage({0, 1, 2}, 0, 3, 32)
                                   .lower();
    expect(lp.has_patches && lp.frame.upsampling == 2 && lp.frame.noise == 1, "patches between the EC upsampling and the colour upsampling");
  }
  // rejected orders
  std::string msg;
  expect(status_of([&] { (void)filters(RenderPipelineBuilder(3, {1000, 700}, 0, 8, p).add_inplace_stage(dict(0)), p)
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }) == JXLH_ERR_UNSUPPORTED,
         "patches before the filters is rejected");
  {
    jxlh_frame_params q = base(500, 350);
    expect(status_of([&] { (void)RenderPipelineBuilder(3, {1000, 700}, 1, 8, q)
                               .add_inout_stage(Upsample2x{nullptr, 0})
                               .add_inout_stage(Upsample2x{nullptr, 1})
                               .add_inout_stage(Upsample2x{nullptr, 2})
                               .add_inplace_stage(dict(0))
                               .add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }, &msg) == JXLH_ERR_UNSUPPORTED &&
               msg.find("patches") != std::string::npos,
           "patches after the colour upsampling is rejected");
  }
  // an extra channel's own upsampling after the patches (the reference upsamples it first, frame/render.rs:624-650)
  expect(status_of([&] { (void)RenderPipelineBuilder(4, {1000, 700}, 0, 8, p)
                             .add_inout_stage(ConvertModularToF32Stage{3, 8})
                             .add_inplace_stage(dict(1))
                             .add_inout_stage(Upsample4x{nullptr, 3})
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }, &msg) == JXLH_ERR_UNSUPPORTED &&
             msg.find("after the patches") != std::string::npos,
         "an extra channel's own upsampling after the patches is rejected");
  // ... while the late form, with the colour channels after the patches, is accepted
  {
    jxlh_frame_params q = base(500, 350);
    const LoweredPipeline lp = RenderPipelineBuilder(4, {1000, 700}, 1, 8, q)
                                   .add_inout_stage(ConvertModularToF32Stage{3, 8})
                                   .add_inplace_stage(dict(1))
                                   .add_inout_stage(Upsample2x{nullptr, 0})
                                   .add_inout_stage(Upsample2x{nullptr, 1})
                                   .add_inout_stage(Upsample2x{nullptr, 2})
                                   .add_inout_stage(Upsample2x{nullptr, 3})
                                   .add_save_stage({0, 1, 2}, 0, 3, 32)
                                   .lower();
    expect(lp.has_patches && lp.extra[0].upsampling == 2, "late extra-channel upsampling after the patches");
  }
  expect(status_of([&] { (void)RenderPipelineBuilder(3, {1000, 700}, 0, 8, p)
                             .add_inplace_stage(XybStage{0, jxlh_xyb_params{}})
                             .add_inplace_stage(dict(0))
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }) == JXLH_ERR_UNSUPPORTED,
         "patches after the colour stage is rejected");
  expect(status_of([&] { (void)filters(RenderPipelineBuilder(3, {1000, 700}, 0, 8, p), p).add_inplace_stage(dict(0))
                             .add_inplace_stage(dict(0)).add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }) == JXLH_ERR_UNSUPPORTED,
         "two patch stages are rejected");
  // a Modular frame
  expect(status_of([&] { (void)RenderPipelineBuilder(3, {1000, 700}, 0, 8, p)
                             .add_inout_stage(ConvertModularToF32Stage{0, 8})
                             .add_inout_stage(ConvertModularToF32Stage{1, 8})
                             .add_inout_stage(ConvertModularToF32Stage{2, 8})
                             .add_inplace_stage(dict(0))
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }, &msg) == JXLH_ERR_UNSUPPORTED &&
             msg.find("Modular") != std::string::npos,
         "patches on a Modular frame is rejected");
  // an inconsistent dictionary
  {
    PatchesStage bad = dict(1);
    bad.blendings.pop_back();
    expect(status_of([&] { (void)filters(RenderPipelineBuilder(4, {1000, 700}, 0, 8, p), p).add_inout_stage(ConvertModularToF32Stage{3, 8})
                               .add_inplace_stage(bad).add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }) != JXLH_OK,
           "a dictionary with too few blendings is rejected");
  }
  // the reference's stage by name stays outside the path
  expect(status_of([&] { (void)filters(RenderPipelineBuilder(3, {1000, 700}, 0, 8, p), p).add_inplace_stage(CpuOnlyStage{"patches"})
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }) == JXLH_ERR_UNSUPPORTED,
         "CpuOnlyStage{\"patches\"} is still rejected");
  if (g_failed) return 1;
  printf("patches lowering: ok\n");
  return 0;
}
