// One synthetic VarDCT frame with an alpha extra channel, saved as premultiplied RGBA8 in orientation 6, twice:
//   * through GpuRenderPipeline with the reference's stage list (frame/render.rs:754-903): extra-channel conversion,
//     filters, XybStage, FromLinearStage, PremultiplyAlphaStage, ConvertF32ToU8Stage x4, the six-argument save stage,
//     and a second buffer with the alpha alone as 16-bit samples;
//   * through the plain C calls: jxlh_frame_run, jxlh_frame_save with the same descriptors and colour stage.
// The two results must be bit-identical (the Python tests hold the C calls to the reference's arithmetic; this one
// holds the builder layer to the C calls), and the image is the transposed size.
//   save_frame W H ITERS
#include <cstdio>
#include <cstring>
#include <string>

#include "jxl_hip_pipeline.hpp"
#include "synth_frame.hpp"

using namespace jxlh;

namespace {
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
    uint32_t lcg = 4242u;
    std::vector<int32_t> alpha((size_t)w * h);
    for (auto& v : alpha) v = (int32_t)((lcg = lcg * 1664525u + 1013904223u) >> 24);
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
                    .add_inplace_stage(PremultiplyAlphaStage{0, 3, 3})
                    .add_inout_stage(ConvertF32ToU8Stage{0, 8})
                    .add_inout_stage(ConvertF32ToU8Stage{1, 8})
                    .add_inout_stage(ConvertF32ToU8Stage{2, 8})
                    .add_inout_stage(ConvertF32ToU8Stage{3, 8})
                    .add_save_stage({0, 1, 2, 3}, 6, 0, ColorType::kRgba, DataFormat::u8(), false)
                    .add_inout_stage(ConvertF32ToU16Stage{3, 16})
                    .add_save_stage({3}, 6, 1, ColorType::kGrayscale, DataFormat::u16(), false)
                    .build(ctx);
    const LoweredPipeline lowered = pipe->lowered();
    if (lowered.saves.size() != 2 || !lowered.saves[0].premultiply || lowered.saves[0].orientation != 6) {
      fprintf(stderr, "the stage list did not lower to the two save descriptors\n");
      return 1;
    }
    pipe->set_extra_channel_buffer(0, alpha.data(), (size_t)w, (uint32_t)w, (uint32_t)h);
    feed(pipe->frame(), F);
    for (int g = 0; g < F.ngroups; g++) pipe->set_buffer_for_group((uint32_t)g, true, &F.coeffs[(size_t)g * 3 * 65536]);
    pipe->do_render();
    // the oriented image: h samples wide, w rows
    const size_t row8 = (size_t)h * 4, row16 = (size_t)h * sizeof(uint16_t);
    pipe->check_buffer_sizes(0, row8, (size_t)w);
    pipe->check_buffer_sizes(1, row16, (size_t)w);
    bool small_rejected = false;
    try {
      pipe->check_buffer_sizes(0, (size_t)w * 4, (size_t)h);  // the unoriented size
    } catch (const Error&) {
      small_rejected = true;
    }
    if (w != h && !small_rejected) {
      fprintf(stderr, "check_buffer_sizes accepted the unoriented size\n");
      return 1;
    }
    std::vector<uint8_t> got8(row8 * w, 0x11), want8(row8 * w, 0x22);
    std::vector<uint16_t> got16((size_t)h * w, 0x1111), want16((size_t)h * w, 0x2222);
    pipe->save(0, got8.data(), row8);
    pipe->save(1, got16.data(), row16);
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
      jxlh_output_desc colour{};
      colour.color = JXLH_COLOR_XYB;
      colour.transfer = JXLH_TF_SRGB;
      colour.xyb = xyb;
      for (int i = 0; i < 3; i++) colour.hlg_luminance_rgb[i] = lum[i];
      jxlh_save_desc d{};
      d.n_channels = 4;
      for (uint32_t k = 0; k < 4; k++) d.channels[k] = k;
      d.format = JXLH_SAVE_U8;
      d.bit_depth = 8;
      d.orientation = 6;
      d.premultiply = 1;
      d.premultiply_alpha_channel = 3;
      // in two bands, to hold the band arithmetic under a transposing orientation too
      const uint32_t cut = (uint32_t)h / 3 + 1;
      ctx.check(jxlh_frame_save(ctx.raw(), &colour, &d, cut, (uint32_t)h, want8.data(), row8), "jxlh_frame_save");
      ctx.check(jxlh_frame_save(ctx.raw(), &colour, &d, 0, cut, want8.data(), row8), "jxlh_frame_save");
      jxlh_save_desc a{};
      a.n_channels = 1;
      a.channels[0] = 3;
      a.format = JXLH_SAVE_U16;
      a.bit_depth = 16;
      a.orientation = 6;
      ctx.check(jxlh_frame_save(ctx.raw(), &colour, &a, 0, (uint32_t)h, want16.data(), row16), "jxlh_frame_save");
    }
    size_t bad = 0, flat = 0;
    for (int y = 0; y < w; y++) {
      if (memcmp(&got8[(size_t)y * row8], &want8[(size_t)y * row8], row8) != 0) bad++;
      if (memcmp(&got16[(size_t)y * h], &want16[(size_t)y * h], row16) != 0) bad++;
      bool same = true;
      for (size_t i = 4; i < row8 && same; i++) same = got8[(size_t)y * row8 + i] == got8[(size_t)y * row8 + i % 4];
      if (same) flat++;
    }
    printf("builder vs C calls: %zu differing rows; %zu flat rows\n", bad, flat);
    if (bad != 0 || flat != 0) return 1;
  } catch (const Error& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  printf("save frame: ok\n");
  return 0;
}
