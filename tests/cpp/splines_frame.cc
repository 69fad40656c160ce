// One synthetic VarDCT frame with a spline, three ways:
//   * VarDctFrame::decode_splines (jxlh_splines_build_segments + jxlh_frame_set_splines) and a plain render;
//   * GpuRenderPipeline with the reference's stage list holding SplinesStage{segments} behind the filters;
//   * the plain C calls without splines, then jxlh_stage_splines on the planes read back.
// The three results must be bit-identical and differ from the frame without splines (the Python tests hold the C calls
// to the reference's arithmetic; this one holds the C++ layers to the C calls).
//   splines_frame W H ITERS
#include <cstdio>
#include <cstring>
#include <string>

#include "jxl_hip_pipeline.hpp"
#include "synth_frame.hpp"

using namespace jxlh;

namespace {
void feed(VarDctFrame& frame, const synth::Frame& F) {
  frame.decode_hf_global(F.tables);
  frame.decode_lf_group(0, 0, (uint32_t)F.xb, (uint32_t)F.yb, F.qy.data(), F.qx.data(), F.qb.data(), (size_t)F.xb);
  frame.decode_hf_metadata(0, 0, (uint32_t)F.xb, (uint32_t)F.yb, F.tmap.data(), F.rq.data(), F.epf.data(), (size_t)F.xb,
                           F.ytox.data(), F.ytob.data(), (size_t)F.cw);
}
size_t differing_rows(const std::vector<float> a[3], const std::vector<float> b[3], int w, int h) {
  size_t bad = 0;
  for (int c = 0; c < 3; c++)
    for (int y = 0; y < h; y++) bad += memcmp(&a[c][(size_t)y * w], &b[c][(size_t)y * w], sizeof(float) * w) != 0;
  return bad;
}
}  // namespace

int main(int argc, char** argv) {
  const int w = argc > 1 ? atoi(argv[1]) : 300, h = argc > 2 ? atoi(argv[2]) : 270, epf_iters = argc > 3 ? atoi(argv[3]) : 2;
  synth::Frame F;
  if (!synth::make(w, h, epf_iters, &F)) return 2;
  // the spline of the reference's consistency test (render/stages/splines.rs:62-92)
  const int64_t deltas[] = {109, 105, -130, -261, -66, 193, 227, -52, -170, 290};
  jxlh_quantized_spline q{};
  q.control_points = deltas;
  q.n_points = 5;
  q.color_dct[0] = 168;
  q.color_dct[1] = 119;
  q.color_dct[32] = 9;
  q.color_dct[34] = 7;
  q.color_dct[64] = -10;
  q.color_dct[65] = 7;
  q.sigma_dct[0] = 4;
  q.sigma_dct[7] = 2;
  q.start_x = 9.0f;
  q.start_y = 54.0f;
  const size_t npx = (size_t)w * h;
  try {
    Context ctx(0, 1);
    jxlh_frame_params base = VarDctFrame::default_params((uint32_t)w, (uint32_t)h);
    base.epf_iters = (uint32_t)epf_iters;
    std::vector<float> a[3], b[3], c[3], plain[3];
    for (auto* set : {a, b, c, plain})
      for (int k = 0; k < 3; k++) set[k].assign(npx, -1.0f);
    std::vector<jxlh_spline_segment> segments;
    for (int with = 1; with >= 0; with--) {  // decode_splines, then the frame without
      VarDctFrame frame(ctx, base);
      feed(frame, F);
      for (int g = 0; g < F.ngroups; g++) frame.decode_vardct_group((uint32_t)g, &F.coeffs[(size_t)g * 3 * 65536]);
      frame.slot_wait();
      if (with) segments = frame.decode_splines({q}, 0, false);
      frame.finalize_and_render();
      std::vector<float>* out = with ? a : plain;
      frame.read_planes(out[0].data(), out[1].data(), out[2].data());
    }
    if (segments.size() < 500) {
      fprintf(stderr, "decode_splines built %zu segments\n", segments.size());
      return 1;
    }
    // the stage hook on the plain planes
    for (int k = 0; k < 3; k++) c[k] = plain[k];
    {
      VarDctFrame frame(ctx, base);
      frame.set_spline_segments(segments);
      float* pl[3] = {c[0].data(), c[1].data(), c[2].data()};
      ctx.stage_splines(pl, (uint32_t)w, (uint32_t)h, (size_t)w);
    }
    // the builder
    {
      auto bld = RenderPipelineBuilder(3, {(size_t)w, (size_t)h}, 0, 8, base)
                     .add_inout_stage(GaborishStage{0, base.gab_w1[0], base.gab_w2[0]})
                     .add_inout_stage(GaborishStage{1, base.gab_w1[1], base.gab_w2[1]})
                     .add_inout_stage(GaborishStage{2, base.gab_w1[2], base.gab_w2[2]});
      const std::array<float, 3> cs{base.epf_channel_scale[0], base.epf_channel_scale[1], base.epf_channel_scale[2]};
      if (epf_iters >= 3) bld = std::move(bld).add_inout_stage(Epf0Stage{base.epf_pass0_sigma_scale, base.epf_border_sad_mul, cs});
      if (epf_iters >= 1) bld = std::move(bld).add_inout_stage(Epf1Stage{1.0f, base.epf_border_sad_mul, cs});
      if (epf_iters >= 2) bld = std::move(bld).add_inout_stage(Epf2Stage{base.epf_pass2_sigma_scale, base.epf_border_sad_mul, cs});
      auto pipe = std::move(bld).add_inplace_stage(SplinesStage{segments}).add_save_stage({0, 1, 2}, 0, 3, 32).build(ctx);
      if (!pipe->lowered().has_splines || pipe->lowered().splines.segments.size() != segments.size()) {
        fprintf(stderr, "the stage list did not lower to splines\n");
        return 1;
      }
      feed(pipe->frame(), F);
      for (int g = 0; g < F.ngroups; g++) pipe->set_buffer_for_group((uint32_t)g, true, &F.coeffs[(size_t)g * 3 * 65536]);
      pipe->do_render();
      pipe->save_planes(b[0].data(), b[1].data(), b[2].data());
    }
    const size_t drawn = differing_rows(a, plain, w, h);
    printf("decode_splines vs stage hook: %zu differing rows; builder vs decode_splines: %zu differing rows; %zu rows drawn on\n",
           differing_rows(a, c, w, h), differing_rows(a, b, w, h), drawn);
    if (differing_rows(a, c, w, h) != 0 || differing_rows(a, b, w, h) != 0 || drawn == 0) return 1;
    // a Modular stage list is pointed at the stage hook
    try {
      (void)RenderPipelineBuilder(3, {(size_t)w, (size_t)h}, 0, 8, base)
          .add_inout_stage(ConvertModularToF32Stage{0, 8})
          .add_inout_stage(ConvertModularToF32Stage{1, 8})
          .add_inout_stage(ConvertModularToF32Stage{2, 8})
          .add_inplace_stage(SplinesStage{segments})
          .add_save_stage({0, 1, 2}, 0, 3, 32)
          .build(ctx);
      fprintf(stderr, "a Modular list with splines was built\n");
      return 1;
    } catch (const Error& e) {
      if (e.status != JXLH_ERR_UNSUPPORTED) return 1;
    }
  } catch (const Error& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  printf("splines frame: ok\n");
  return 0;
}
