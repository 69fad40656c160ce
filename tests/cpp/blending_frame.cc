// One synthetic VarDCT frame with an alpha extra channel, blended onto a larger image from a reference slot, twice:
//   * through GpuRenderPipeline with the reference's stage list (frame/render.rs:754-791): extra-channel conversion,
//     filters, XybStage, FromLinearStage, BlendingStage, ExtendToImageDimensionsStage, f32 save;
//   * through the plain C calls: jxlh_frame_run, jxlh_frame_blend with the same descriptor and colour stage.
// The two results must be image-sized and bit-identical (the Python tests hold the C calls to the reference's
// arithmetic; this one holds the builder layer to the C calls).
//   blending_frame W H ITERS
#include <cstdio>
#include <cstring>
#include <string>

#include "jxl_hip_pipeline.hpp"
#include "synth_frame.hpp"

using namespace jxlh;

namespace {
constexpr uint32_t kImageW = 700, kImageH = 500;
constexpr int32_t kX0 = -37, kY0 = 61;

jxlh_xyb_params some_xyb() {
  jxlh_xyb_params x{};
  for (int i = 0; i < 9; i++) x.opsin_inverse_matrix[i] = (i % 4 == 0) ? 1.0f : 0.01f * (float)i;
  for (int i = 0; i < 3; i++) {
    x.bias_cbrt[i] = 0.1f;
    x.scaled_bias[i] = 0.001f;
  }
  x.intensity_scale = 1.0f;
  return x;
}

void feed(VarDctFrame& frame, const synth::Frame& F) {
  frame.decode_hf_global(F.tables);
  frame.decode_lf_group(0, 0, (uint32_t)F.xb, (uint32_t)F.yb, F.qy.data(), F.qx.data(), F.qb.data(), (size_t)F.xb);
  frame.decode_hf_metadata(0, 0, (uint32_t)F.xb, (uint32_t)F.yb, F.tmap.data(), F.rq.data(), F.epf.data(), (size_t)F.xb,
                           F.ytox.data(), F.ytob.data(), (size_t)F.cw);
}
}  // namespace

int main(int argc, char** argv) {
  const int w = argc > 1 ? atoi(argv[1]) : 300, h = argc > 2 ? atoi(argv[2]) : 270, epf_iters = argc > 3 ? atoi(argv[3]) : 2;
  synth::Frame F;
  if (!synth::make(w, h, epf_iters, &F)) return 2;
  try {
    Context ctx(0, 1);
    // reference slot 1: an image-sized frame of 3 + 1 channels
    const size_t npx = (size_t)kImageW * kImageH;
    std::vector<float> ref[4];
    uint32_t lcg = 777u;
    for (auto& r : ref) {
      r.resize(npx);
      for (auto& v : r) v = (float)((lcg = lcg * 1664525u + 1013904223u) >> 8) * (2.0f / 16777216.0f) - 0.5f;
    }
    const float* rp[4] = {ref[0].data(), ref[1].data(), ref[2].data(), ref[3].data()};
    ctx.check(jxlh_ctx_set_reference(ctx.raw(), 1, 4, kImageW, kImageH, rp, kImageW), "jxlh_ctx_set_reference");
    std::vector<int32_t> alpha((size_t)w * h);
    for (auto& v : alpha) v = (int32_t)((lcg = lcg * 1664525u + 1013904223u) >> 24);

    const jxlh_blending_info colour_info{JXLH_BLEND_BLEND, 0, 1, 1}, alpha_info{JXLH_BLEND_BLEND, 0, 1, 1};
    BlendingStage bs;
    bs.x0 = kX0;
    bs.y0 = kY0;
    bs.image_w = kImageW;
    bs.image_h = kImageH;
    bs.blending_info = colour_info;
    bs.ec_blending_info = {alpha_info};
    bs.ec_flags = {JXLH_EC_ALPHA};
    ExtendToImageDimensionsStage es{kX0, kY0, kImageW, kImageH, colour_info, {alpha_info}};
    const jxlh_xyb_params xyb = some_xyb();
    const std::array<float, 3> lum{0.2627f, 0.678f, 0.0593f};

    jxlh_frame_params base = VarDctFrame::default_params((uint32_t)w, (uint32_t)h);
    auto b = RenderPipelineBuilder(4, {(size_t)w, (size_t)h}, 0, 8, base)
                 .add_inout_stage(ConvertModularToF32Stage{3, 8})
                 .add_inout_stage(GaborishStage{0, base.gab_w1[0], base.gab_w2[0]})
                 .add_inout_stage(GaborishStage{1, base.gab_w1[1], base.gab_w2[1]})
                 .add_inout_stage(GaborishStage{2, base.gab_w1[2], base.gab_w2[2]});
    const std::array<float, 3> cs{base.epf_channel_scale[0], base.epf_channel_scale[1], base.epf_channel_scale[2]};
    if (epf_iters >= 3) b = std::move(b).add_inout_stage(Epf0Stage{base.epf_pass0_sigma_scale, base.epf_border_sad_mul, cs});
    if (epf_iters >= 1) b = std::move(b).add_inout_stage(Epf1Stage{1.0f, base.epf_border_sad_mul, cs});
    if (epf_iters >= 2) b = std::move(b).add_inout_stage(Epf2Stage{base.epf_pass2_sigma_scale, base.epf_border_sad_mul, cs});
    auto pipe = std::move(b)
                    .add_inplace_stage(XybStage{0, xyb})
                    .add_inplace_stage(FromLinearStage{0, JXLH_TF_SRGB, 0.0f, lum})
                    .add_inplace_stage(bs)
                    .add_extend_stage(es)
                    .add_save_stage({0, 1, 2}, 0, 3, 32)
                    .build(ctx);
    const LoweredPipeline lowered = pipe->lowered();
    if (!lowered.has_blend || lowered.out_w != kImageW || lowered.out_h != kImageH) {
      fprintf(stderr, "the stage list did not lower to a blend\n");
      return 1;
    }
    pipe->set_extra_channel_buffer(0, alpha.data(), (size_t)w, (uint32_t)w, (uint32_t)h);
    feed(pipe->frame(), F);
    for (int g = 0; g < F.ngroups; g++) pipe->set_buffer_for_group((uint32_t)g, true, &F.coeffs[(size_t)g * 3 * 65536]);
    pipe->do_render();
    pipe->check_buffer_sizes((size_t)kImageW * sizeof(float), kImageH);
    if (pipe->frame().out_width() != kImageW || pipe->frame().out_height() != kImageH) {
      fprintf(stderr, "the pipeline's output is not image-sized\n");
      return 1;
    }
    std::vector<float> got[4], want[4];
    for (auto& o : got) o.assign(npx, -1.0f);
    for (auto& o : want) o.assign(npx, -2.0f);
    pipe->save_planes(got[0].data(), got[1].data(), got[2].data());
    pipe->save_extra_channel(0, got[3].data(), kImageW);
    pipe.reset();

    // the same frame through the plain C calls
    {
      VarDctFrame frame(ctx, lowered.frame);
      ctx.check(jxlh_frame_set_extra_channel(ctx.raw(), 0, alpha.data(), (size_t)w, (uint32_t)w, (uint32_t)h, 8, 1),
                "jxlh_frame_set_extra_channel");
      feed(frame, F);
      for (int g = 0; g < F.ngroups; g++) frame.decode_vardct_group((uint32_t)g, &F.coeffs[(size_t)g * 3 * 65536]);
      frame.slot_wait();
      ctx.check(jxlh_frame_run(ctx.raw(), 0, 0xFFFFFFFFu), "jxlh_frame_run");
      jxlh_blend_desc d{};
      d.x0 = kX0;
      d.y0 = kY0;
      d.image_w = kImageW;
      d.image_h = kImageH;
      d.color = colour_info;
      d.num_ec = 1;
      d.ec[0] = alpha_info;
      d.ec_flags[0] = JXLH_EC_ALPHA;
      jxlh_output_desc colour{};
      colour.color = JXLH_COLOR_XYB;
      colour.transfer = JXLH_TF_SRGB;
      colour.xyb = xyb;
      for (int i = 0; i < 3; i++) colour.hlg_luminance_rgb[i] = lum[i];
      ctx.check(jxlh_frame_blend(ctx.raw(), &d, &colour), "jxlh_frame_blend");
      jxlh_plane pl[3];
      for (int c = 0; c < 3; c++) pl[c] = jxlh_plane{want[c].data(), kImageW * sizeof(float), kImageH, kImageW * sizeof(float)};
      ctx.check(jxlh_frame_read_planes(ctx.raw(), pl), "jxlh_frame_read_planes");
      jxlh_plane ep{want[3].data(), kImageW * sizeof(float), kImageH, kImageW * sizeof(float)};
      ctx.check(jxlh_frame_read_extra_channel(ctx.raw(), 0, &ep), "jxlh_frame_read_extra_channel");
    }
    size_t bad = 0, from_slot = 0, blended = 0;
    for (int c = 0; c < 4; c++)
      for (uint32_t y = 0; y < kImageH; y++) {
        if (memcmp(&got[c][(size_t)y * kImageW], &want[c][(size_t)y * kImageW], sizeof(float) * kImageW) != 0) bad++;
        // outside the frame's rectangle the image is the slot, inside it is not
        const bool in_rows = (int32_t)y >= kY0 && (int32_t)y < kY0 + h;
        if (!in_rows && memcmp(&got[c][(size_t)y * kImageW], &ref[c][(size_t)y * kImageW], sizeof(float) * kImageW) == 0) from_slot++;
        if (in_rows && memcmp(&got[c][(size_t)y * kImageW], &ref[c][(size_t)y * kImageW], sizeof(float) * kImageW) != 0) blended++;
      }
    printf("builder vs C calls: %zu differing rows; %zu rows extended from the slot, %zu rows blended\n", bad, from_slot, blended);
    const size_t rows_in = (size_t)std::min<int>((int)kImageH, kY0 + h) - (size_t)std::max<int>(0, kY0);
    if (bad != 0 || from_slot != 4 * (kImageH - rows_in) || blended != 4 * rows_in) return 1;
  } catch (const Error& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  printf("blending frame: ok\n");
  return 0;
}
