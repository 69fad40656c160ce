// Blend rectangles through the C++ layer: one synthetic VarDCT frame with an alpha extra channel, blended onto an image
// from a reference slot behind a colour stage, in two passes (some groups arrive with zeroed coefficients first), three
// times over on one context:
//   * GpuRenderPipeline::do_render() for both passes: the whole image is composed after each (the existing route);
//   * GpuRenderPipeline::do_render_rects() for both passes: the first is the whole blend and returns one rect of the
//     image, the second composes only the changed rects again and returns them in image coordinates;
//   * the plain C calls: jxlh_frame_run, jxlh_frame_blend, jxlh_frame_rerender_groups, jxlh_changed_rects,
//     jxlh_blend_image_rects, jxlh_frame_blend_rects -- with VarDctFrame::blend_rects / jxlh::blend_image_rects beside.
// The three final images must be byte for byte the same, the image after the first pass must differ from them, and the
// returned rects must be the C call's and smaller than the image.
//   blend_rects W H ITERS
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

struct Image {
  std::vector<float> ch[4];
  bool operator==(const Image& o) const {
    for (int c = 0; c < 4; c++)
      if (memcmp(ch[c].data(), o.ch[c].data(), ch[c].size() * sizeof(float)) != 0) return false;
    return true;
  }
};

Image read_image(Context& ctx) {
  Image im;
  jxlh_plane pl[3];
  for (int c = 0; c < 4; c++) im.ch[c].assign((size_t)kImageW * kImageH, -1.0f);
  for (int c = 0; c < 3; c++) pl[c] = jxlh_plane{im.ch[c].data(), kImageW * sizeof(float), kImageH, kImageW * sizeof(float)};
  ctx.check(jxlh_frame_read_planes(ctx.raw(), pl), "jxlh_frame_read_planes");
  jxlh_plane ep{im.ch[3].data(), kImageW * sizeof(float), kImageH, kImageW * sizeof(float)};
  ctx.check(jxlh_frame_read_extra_channel(ctx.raw(), 0, &ep), "jxlh_frame_read_extra_channel");
  return im;
}
}  // namespace

int main(int argc, char** argv) {
  const int w = argc > 1 ? atoi(argv[1]) : 600, h = argc > 2 ? atoi(argv[2]) : 520, epf_iters = argc > 3 ? atoi(argv[3]) : 2;
  synth::Frame F;
  if (!synth::make(w, h, epf_iters, &F)) return 2;
  try {
    Context ctx(0, 1);
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
    const ExtendToImageDimensionsStage es{kX0, kY0, kImageW, kImageH, colour_info, {alpha_info}};
    const jxlh_xyb_params xyb = some_xyb();
    const std::array<float, 3> lum{0.2627f, 0.678f, 0.0593f};
    const jxlh_frame_params base = VarDctFrame::default_params((uint32_t)w, (uint32_t)h);

    auto build = [&]() {
      auto b = RenderPipelineBuilder(4, {(size_t)w, (size_t)h}, 0, 8, base)
                   .add_inout_stage(ConvertModularToF32Stage{3, 8})
                   .add_inout_stage(GaborishStage{0, base.gab_w1[0], base.gab_w2[0]})
                   .add_inout_stage(GaborishStage{1, base.gab_w1[1], base.gab_w2[1]})
                   .add_inout_stage(GaborishStage{2, base.gab_w1[2], base.gab_w2[2]});
      const std::array<float, 3> cs{base.epf_channel_scale[0], base.epf_channel_scale[1], base.epf_channel_scale[2]};
      if (epf_iters >= 3) b = std::move(b).add_inout_stage(Epf0Stage{base.epf_pass0_sigma_scale, base.epf_border_sad_mul, cs});
      if (epf_iters >= 1) b = std::move(b).add_inout_stage(Epf1Stage{1.0f, base.epf_border_sad_mul, cs});
      if (epf_iters >= 2) b = std::move(b).add_inout_stage(Epf2Stage{base.epf_pass2_sigma_scale, base.epf_border_sad_mul, cs});
      return std::move(b)
          .add_inplace_stage(XybStage{0, xyb})
          .add_inplace_stage(FromLinearStage{0, JXLH_TF_SRGB, 0.0f, lum})
          .add_inplace_stage(bs)
          .add_extend_stage(es)
          .add_save_stage({0, 1, 2}, 0, 3, 32)
          .build(ctx);
    };
    // the groups of the second pass: the first one, and the middle one with its right neighbour
    std::vector<uint32_t> later = {0u};
    if (F.ngroups >= 6) later.push_back((uint32_t)F.ngroups / 2), later.push_back((uint32_t)F.ngroups / 2 + 1);
    auto is_later = [&](int g) {
      for (uint32_t l : later)
        if ((int)l == g) return true;
      return false;
    };
    std::vector<int32_t> zeros((size_t)3 * 65536, 0);
    auto coeffs = [&](int g, bool final_pass) { return !final_pass && is_later(g) ? zeros.data() : &F.coeffs[(size_t)g * 3 * 65536]; };

    // the existing route, and the rect route, through the pipeline
    Image first_pass, whole, by_rects;
    std::vector<jxlh_rect> first_rects, second_rects;
    LoweredPipeline lowered;
    for (int route = 0; route < 2; route++) {
      auto pipe = build();
      lowered = pipe->lowered();
      if (!lowered.has_blend || lowered.out_w != kImageW || lowered.out_h != kImageH) {
        fprintf(stderr, "the stage list did not lower to a blend\n");
        return 1;
      }
      pipe->set_extra_channel_buffer(0, alpha.data(), (size_t)w, (uint32_t)w, (uint32_t)h);
      feed(pipe->frame(), F);
      for (int g = 0; g < F.ngroups; g++) pipe->set_buffer_for_group((uint32_t)g, !is_later(g), coeffs(g, false));
      if (route == 0) pipe->do_render();
      else first_rects = pipe->do_render_rects();
      if (route == 0) first_pass = read_image(ctx);
      else if (!(read_image(ctx) == first_pass)) {
        fprintf(stderr, "the first do_render_rects() is not the first do_render()\n");
        return 1;
      }
      for (uint32_t g : later) pipe->set_buffer_for_group(g, true, coeffs((int)g, true));
      if (route == 0) pipe->do_render();
      else second_rects = pipe->do_render_rects();
      if (pipe->frame().out_width() != kImageW || pipe->frame().out_height() != kImageH) {
        fprintf(stderr, "the pipeline's output is not image-sized\n");
        return 1;
      }
      (route == 0 ? whole : by_rects) = read_image(ctx);
    }

    // the plain C calls, with the thin wrappers beside them
    Image by_c;
    std::vector<jxlh_rect> c_rects;
    bool wrappers_same = false;
    {
      VarDctFrame frame(ctx, lowered.frame);
      ctx.check(jxlh_frame_set_extra_channel(ctx.raw(), 0, alpha.data(), (size_t)w, (uint32_t)w, (uint32_t)h, 8, 1),
                "jxlh_frame_set_extra_channel");
      feed(frame, F);
      for (int g = 0; g < F.ngroups; g++) frame.decode_vardct_group((uint32_t)g, coeffs(g, false));
      frame.slot_wait();
      ctx.check(jxlh_frame_run(ctx.raw(), 0, 0xFFFFFFFFu), "jxlh_frame_run");
      ctx.check(jxlh_frame_blend(ctx.raw(), &lowered.blend, &lowered.blend_colour), "jxlh_frame_blend");
      for (uint32_t g : later) frame.decode_vardct_group(g, coeffs((int)g, true));
      frame.slot_wait();
      ctx.check(jxlh_frame_rerender_groups(ctx.raw(), later.data(), (uint32_t)later.size()), "jxlh_frame_rerender_groups");
      uint32_t n = 0;
      std::vector<jxlh_rect> changed(later.size());
      ctx.check(jxlh_changed_rects(&lowered.frame, later.data(), (uint32_t)later.size(), changed.data(), (uint32_t)changed.size(), &n),
                "jxlh_changed_rects");
      changed.resize(n);
      c_rects.resize(n);
      ctx.check(jxlh_blend_image_rects(&lowered.blend, (uint32_t)w, (uint32_t)h, changed.data(), n, c_rects.data(), n, &n),
                "jxlh_blend_image_rects");
      c_rects.resize(n);
      const std::vector<jxlh_rect> wrapped = blend_image_rects(lowered.blend, (uint32_t)w, (uint32_t)h, changed);
      wrappers_same = wrapped.size() == c_rects.size() && memcmp(wrapped.data(), c_rects.data(), n * sizeof(jxlh_rect)) == 0;
      const uint32_t half = n / 2;  // one part through the C call, the other through the member
      ctx.check(jxlh_frame_blend_rects(ctx.raw(), &lowered.blend, &lowered.blend_colour, c_rects.data(), half), "jxlh_frame_blend_rects");
      frame.blend_rects(lowered.blend, std::vector<jxlh_rect>(c_rects.begin() + half, c_rects.end()), &lowered.blend_colour);
      wrappers_same = wrappers_same && frame.out_width() == kImageW && frame.out_height() == kImageH;
      by_c = read_image(ctx);
      bool threw = false;
      try {
        frame.blend_rects(lowered.blend, {jxlh_rect{kImageW, 0, 1, 1}}, &lowered.blend_colour);  // starts outside the image
      } catch (const Error& e) {
        threw = e.status == JXLH_ERR_INVALID_ARGUMENT;
      }
      wrappers_same = wrappers_same && threw && by_c == read_image(ctx);
    }
    size_t rect_px = 0;
    for (const jxlh_rect& r : second_rects) rect_px += (size_t)r.w * r.h;
    const bool one_whole = first_rects.size() == 1 && first_rects[0].x0 == 0 && first_rects[0].y0 == 0 &&
                           first_rects[0].w == kImageW && first_rects[0].h == kImageH;
    const bool same_rects = second_rects.size() == c_rects.size() && !c_rects.empty() &&
                            memcmp(second_rects.data(), c_rects.data(), c_rects.size() * sizeof(jxlh_rect)) == 0;
    const bool stale = !(first_pass == whole);
    printf("%dx%d epf_iters=%d: %zu groups in %zu rects, %zu of %zu pixels recomposed; do_render_rects vs do_render: %s, "
           "C calls vs do_render: %s, first pass %s, first render %s, rects %s, wrappers %s\n",
           w, h, epf_iters, later.size(), second_rects.size(), rect_px, npx, by_rects == whole ? "equal" : "DIFFER",
           by_c == whole ? "equal" : "DIFFER", stale ? "stale" : "ALREADY FINAL", one_whole ? "one whole rect" : "WRONG RECTS",
           same_rects ? "equal" : "DIFFER", wrappers_same ? "ok" : "WRONG");
    if (!(by_rects == whole) || !(by_c == whole) || !stale || !one_whole || !same_rects || !wrappers_same || rect_px >= npx) return 1;
  } catch (const Error& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  printf("blend rects frame: ok\n");
  return 0;
}
