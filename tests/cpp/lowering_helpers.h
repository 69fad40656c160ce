// What the host programs that lower stage lists share (pipeline_builder.cc, save_lowering.cc, blending_lowering.cc,
// patches_lowering.cc, splines_lowering.cc, modular_frame_lowering.cc, and the corpus of lowering_corpus.h): the
// expectation counter, the status a lowering fails with, and the pieces of Frame::build_render_pipeline's list they
// all assemble.  Everything is inline: a program uses what it needs.
#pragma once
#include <array>
#include <cstdio>
#include <functional>
#include <string>
#include <utility>

#include "jxl_hip_pipeline.hpp"

namespace lowering_helpers {
using namespace jxlh;

inline int g_failed = 0;
inline void expect(bool ok, const char* what) {
  if (!ok) {
    g_failed++;
    fprintf(stderr, "FAILED: %s\n", what);
  }
}
// the status build() / lower() fails with, or JXLH_OK
inline jxlh_status status_of(const std::function<void()>& f, std::string* msg = nullptr) {
  try {
    f();
  } catch (const Error& e) {
    if (msg) *msg = e.what();
    return e.status;
  }
  return JXLH_OK;
}
inline jxlh_frame_params base(uint32_t w, uint32_t h) {
  jxlh_frame_params p;
  jxlh_default_frame_params(&p, w, h);
  return p;
}

// RestorationFilter defaults as jxlh_default_frame_params holds them
struct Rf {
  float gab_w1[3], gab_w2[3], pass0, pass2, border_sad_mul;
  std::array<float, 3> channel_scale;
};
inline Rf rf_of(const jxlh_frame_params& p) {
  Rf r;
  for (int c = 0; c < 3; c++) {
    r.gab_w1[c] = p.gab_w1[c];
    r.gab_w2[c] = p.gab_w2[c];
    r.channel_scale[c] = p.epf_channel_scale[c];
  }
  r.pass0 = p.epf_pass0_sigma_scale;
  r.pass2 = p.epf_pass2_sigma_scale;
  r.border_sad_mul = p.epf_border_sad_mul;
  return r;
}
// the filter part of Frame::build_render_pipeline (frame/render.rs:578-622)
inline RenderPipelineBuilder add_filters(RenderPipelineBuilder b, const Rf& rf, bool gab, int epf_iters) {
  if (gab) {
    b = std::move(b)
            .add_inout_stage(GaborishStage{0, rf.gab_w1[0], rf.gab_w2[0]})
            .add_inout_stage(GaborishStage{1, rf.gab_w1[1], rf.gab_w2[1]})
            .add_inout_stage(GaborishStage{2, rf.gab_w1[2], rf.gab_w2[2]});
  }
  if (epf_iters >= 3) b = std::move(b).add_inout_stage(Epf0Stage{rf.pass0, rf.border_sad_mul, rf.channel_scale});
  if (epf_iters >= 1) b = std::move(b).add_inout_stage(Epf1Stage{1.0f, rf.border_sad_mul, rf.channel_scale});
  if (epf_iters >= 2) b = std::move(b).add_inout_stage(Epf2Stage{rf.pass2, rf.border_sad_mul, rf.channel_scale});
  return b;
}
// Gaborish + EPF1 with the frame's own parameters
inline RenderPipelineBuilder filters(RenderPipelineBuilder b, const jxlh_frame_params& p) {
  return add_filters(std::move(b), rf_of(p), true, 1);
}
inline jxlh_xyb_params some_xyb() {
  jxlh_xyb_params x{};
  for (int i = 0; i < 9; i++) x.opsin_inverse_matrix[i] = (i % 4 == 0) ? 1.0f : 0.01f * (float)i;
  for (int i = 0; i < 3; i++) {
    x.bias_cbrt[i] = -0.15f;
    x.scaled_bias[i] = -0.0038f;
  }
  x.intensity_scale = 1.0f;
  return x;
}
// another XybParams, told from some_xyb() by its fields
inline jxlh_xyb_params xyb() {
  jxlh_xyb_params x{};
  for (int i = 0; i < 9; i++) x.opsin_inverse_matrix[i] = 0.5f + (float)i;
  x.intensity_scale = 0.75f;
  return x;
}
// BlendingStage and the ExtendToImageDimensionsStage built from the same headers: `num_ec` extra channels, each `ec`
inline BlendingStage blending(int32_t x0, int32_t y0, uint32_t image_w, uint32_t image_h, jxlh_blending_info colour, size_t num_ec,
                              jxlh_blending_info ec) {
  BlendingStage b;
  b.x0 = x0;
  b.y0 = y0;
  b.image_w = image_w;
  b.image_h = image_h;
  b.blending_info = colour;
  b.ec_blending_info.assign(num_ec, ec);
  b.ec_flags.assign(num_ec, JXLH_EC_ALPHA);
  return b;
}
inline ExtendToImageDimensionsStage extend_of(const BlendingStage& b) {
  ExtendToImageDimensionsStage e{};
  e.x0 = b.x0;
  e.y0 = b.y0;
  e.image_w = b.image_w;
  e.image_h = b.image_h;
  e.blending_info = b.blending_info;
  e.ec_blending_info = b.ec_blending_info;
  return e;
}
}  // namespace lowering_helpers
