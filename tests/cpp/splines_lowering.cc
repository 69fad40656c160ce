// Host-side lowering of SplinesStage (include/jxl_hip_lowering.hpp): accepted at the reference's position -- behind the
// patches stage (if any), before the colour upsampling, noise and the colour stage (frame/render.rs:644-683) -- and only
// on a VarDCT frame.  No GPU involved.
#include <cstdio>
#include <string>

#include "lowering_helpers.h"

using namespace jxlh;
using namespace lowering_helpers;

namespace {
SplinesStage segs() {
  SplinesStage st;
  st.segments = {jxlh_spline_segment{10.0f, 20.0f, 3.5f, 1.25f, 0.1f, {0.5f, 0.6f, 0.7f}},
                 jxlh_spline_segment{11.0f, 21.0f, 4.5f, -1.0f, -0.2f, {-0.8f, -0.8f, -0.7f}},
                 jxlh_spline_segment{12.0f, 21.0f, 4.5f, -1.0f, -0.2f, {-0.8f, -0.8f, -0.7f}}};
  return st;
}
PatchesStage dict() {
  PatchesStage ps;
  ps.patches = {jxlh_patch{4, 5, 0, 0, 0, 16, 12}};
  ps.blendings.assign(1, jxlh_patch_blending{JXLH_PATCH_ADD, 0, 0});
  return ps;
}
RenderPipelineBuilder upsample2(RenderPipelineBuilder b) {
  return std::move(b).add_inout_stage(Upsample2x{nullptr, 0}).add_inout_stage(Upsample2x{nullptr, 1}).add_inout_stage(Upsample2x{nullptr, 2});
}
}  // namespace

int main() {
  const jxlh_frame_params p = base(1000, 700);
  std::string msg;
  expect(SplinesStage{}.display() == "splines", "display()");
  // accepted: filters -> splines -> save; what it lowers to
  {
    const LoweredPipeline lp =
        filters(RenderPipelineBuilder(3, {1000, 700}, 0, 8, p), p).add_inplace_stage(segs()).add_save_stage({0, 1, 2}, 0, 3, 32).lower();
    expect(lp.has_splines && !lp.has_patches && lp.splines.segments.size() == 3, "filters -> splines lowers");
    expect(lp.splines.segments[1].inv_sigma == -1.0f && lp.splines.segments[0].color[2] == 0.7f &&
               lp.splines.segments[0].maximum_distance == 3.5f, "the segments are handed on as they are");
    expect(lp.frame.gab == 1 && lp.frame.epf_iters == 1, "the filters are kept");
    bool named = false;
    for (const auto& s : lp.stages) named |= s == "splines";
    expect(named, "the stage is listed by name");
  }
  // accepted: no filter at all; patches -> splines; splines -> colour upsampling -> noise -> colour stage
  {
    const LoweredPipeline lp = RenderPipelineBuilder(3, {1000, 700}, 0, 8, p).add_inplace_stage(segs())
                                   .add_save_stage({0, 1, 2}, 0, 3, 32).lower();
    expect(lp.has_splines && lp.frame.epf_iters == 0, "splines as the only stage");
  }
  {
    const LoweredPipeline lp = filters(RenderPipelineBuilder(3, {1000, 700}, 0, 8, p), p).add_inplace_stage(dict())
                                   .add_inplace_stage(segs()).add_save_stage({0, 1, 2}, 0, 3, 32).lower();
    expect(lp.has_patches && lp.has_splines, "patches -> splines");
  }
  {
    jxlh_frame_params q = base(500, 350);
    const LoweredPipeline lp = upsample2(RenderPipelineBuilder(6, {1000, 700}, 1, 8, q).add_inplace_stage(dict()).add_inplace_stage(segs()))
                                   .add_inout_stage(ConvolveNoiseStage{3})
                                   .add_inout_stage(ConvolveNoiseStage{4})
                                   .add_inout_stage(ConvolveNoiseStage{5})
                                   .add_inplace_stage(AddNoiseStage{{0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f}, 0, 0, 3})
                                   .add_inplace_stage(XybStage{0, jxlh_xyb_params{}})
                                   .add_save_stage({0, 1, 2}, 0, 3, 32)
                                   .lower();
    expect(lp.has_splines && lp.has_patches && lp.frame.upsampling == 2 && lp.frame.noise == 1,
           "splines between the patches and the colour upsampling");
  }
  // an extra channel: its own upsampling first, the late form afterwards
  {
    jxlh_frame_params q = base(500, 350);
    const LoweredPipeline lp = upsample2(RenderPipelineBuilder(4, {1000, 700}, 1, 8, q)
                                             .add_inout_stage(ConvertModularToF32Stage{3, 8})
                                             .add_inplace_stage(segs()))
                                   .add_inout_stage(Upsample2x{nullptr, 3})
                                   .add_save_stage({0, 1, 2}, 0, 3, 32)
                                   .lower();
    expect(lp.has_splines && lp.extra[0].upsampling == 2, "late extra-channel upsampling after the splines");
  }
  expect(status_of([&] { (void)RenderPipelineBuilder(4, {1000, 700}, 0, 8, p)
                             .add_inout_stage(ConvertModularToF32Stage{3, 8})
                             .add_inplace_stage(segs())
                             .add_inout_stage(Upsample4x{nullptr, 3})
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }, &msg) == JXLH_ERR_UNSUPPORTED &&
             msg.find("after the splines") != std::string::npos,
         "an extra channel's own upsampling after the splines is rejected");
  // rejected orders
  expect(status_of([&] { (void)filters(RenderPipelineBuilder(3, {1000, 700}, 0, 8, p).add_inplace_stage(segs()), p)
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }) == JXLH_ERR_UNSUPPORTED,
         "splines before the filters is rejected");
  expect(status_of([&] { (void)filters(RenderPipelineBuilder(3, {1000, 700}, 0, 8, p), p).add_inplace_stage(segs())
                             .add_inplace_stage(dict()).add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }, &msg) == JXLH_ERR_UNSUPPORTED &&
             msg.find("patches") != std::string::npos,
         "patches behind the splines is rejected");
  {
    jxlh_frame_params q = base(500, 350);
    expect(status_of([&] { (void)upsample2(RenderPipelineBuilder(3, {1000, 700}, 1, 8, q)).add_inplace_stage(segs())
                               .add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }, &msg) == JXLH_ERR_UNSUPPORTED &&
               msg.find("splines") != std::string::npos,
           "splines after the colour upsampling is rejected");
  }
  expect(status_of([&] { (void)RenderPipelineBuilder(6, {1000, 700}, 0, 8, p)
                             .add_inout_stage(ConvolveNoiseStage{3})
                             .add_inout_stage(ConvolveNoiseStage{4})
                             .add_inout_stage(ConvolveNoiseStage{5})
                             .add_inplace_stage(AddNoiseStage{{0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f}, 0, 0, 3})
                             .add_inplace_stage(segs())
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }) == JXLH_ERR_UNSUPPORTED,
         "splines after the noise is rejected");
  expect(status_of([&] { (void)RenderPipelineBuilder(3, {1000, 700}, 0, 8, p)
                             .add_inplace_stage(XybStage{0, jxlh_xyb_params{}})
                             .add_inplace_stage(segs())
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }) == JXLH_ERR_UNSUPPORTED,
         "splines after the colour stage is rejected");
  expect(status_of([&] { (void)filters(RenderPipelineBuilder(3, {1000, 700}, 0, 8, p), p).add_inplace_stage(segs())
                             .add_inplace_stage(segs()).add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }) == JXLH_ERR_UNSUPPORTED,
         "two spline stages are rejected");
  // a Modular frame: the stage hook is named
  expect(status_of([&] { (void)RenderPipelineBuilder(3, {1000, 700}, 0, 8, p)
                             .add_inout_stage(ConvertModularToF32Stage{0, 8})
                             .add_inout_stage(ConvertModularToF32Stage{1, 8})
                             .add_inout_stage(ConvertModularToF32Stage{2, 8})
                             .add_inplace_stage(segs())
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }, &msg) == JXLH_ERR_UNSUPPORTED &&
             msg.find("Modular") != std::string::npos && msg.find("jxlh_stage_splines") != std::string::npos,
         "splines on a Modular frame is rejected, naming jxlh_stage_splines");
  // the reference's stage by name stays outside the path
  expect(status_of([&] { (void)filters(RenderPipelineBuilder(3, {1000, 700}, 0, 8, p), p).add_inplace_stage(CpuOnlyStage{"splines"})
                             .add_save_stage({0, 1, 2}, 0, 3, 32).lower(); }) == JXLH_ERR_UNSUPPORTED,
         "CpuOnlyStage{\"splines\"} is still rejected");
  // a list without the stage lowers to no segments
  expect(!filters(RenderPipelineBuilder(3, {1000, 700}, 0, 8, p), p).add_save_stage({0, 1, 2}, 0, 3, 32).lower().has_splines,
         "no stage, no splines");
  if (g_failed) return 1;
  printf("splines lowering: ok\n");
  return 0;
}
