// One repaint through the C++ layer, bit-exact against the oracle: a synthetic VarDCT frame goes through
// GpuRenderPipeline with the reference's stage list (filters, XybStage, FromLinearStage, ConvertF32ToU8Stage x3, the
// six-argument save stage as opaque RGBA8 in orientation 6).
//   pass 1: every group is handed over, some of them with zeroed coefficients and `complete = false`; the whole image is
//           saved into A;
//   pass 2: those groups arrive; do_render() re-renders them, changed_rects() names what can have changed and
//           save_rects() repaints only that into A.
// A must then be the oracle's frame through the oracle's output stage, oriented by display_pixel -- every pixel outside
// the rects still being the one pass 1 painted.  jxlh::changed_rects / VarDctFrame::save_rects_async / the C calls give
// the same bytes into a second buffer.
//   save_rects_frame W H ITERS
#include <cstdio>
#include <cstring>
#include <string>

#include "jxl_hip_pipeline.hpp"
#include "synth_frame.hpp"

using namespace jxlh;

int main(int argc, char** argv) {
  const int w = argc > 1 ? atoi(argv[1]) : 600, h = argc > 2 ? atoi(argv[2]) : 520, epf_iters = argc > 3 ? atoi(argv[3]) : 2;
  synth::Frame F;
  if (!synth::make(w, h, epf_iters, &F)) return 2;
  try {
    Context ctx(0, 1);
    JxloXybParams ox;
    const float mat[9] = {11.031566901960783f, -9.866943921568629f, -0.16462299647058826f, -3.254147380392157f,
                          4.418770392156863f, -0.16462299647058826f, -3.6588512862745097f, 2.7129230470588235f,
                          1.9459282392156863f};
    const float bias[3] = {-0.0037930732552754493f, -0.0037930732552754493f, -0.0037930732552754493f};
    jxlo_xyb_params(mat, bias, 255.0f, &ox);
    jxlh_xyb_params gx;
    memcpy(gx.opsin_inverse_matrix, ox.mat, sizeof(ox.mat));
    memcpy(gx.bias_cbrt, ox.bias_cbrt, sizeof(ox.bias_cbrt));
    memcpy(gx.scaled_bias, ox.scaled_bias, sizeof(ox.scaled_bias));
    gx.intensity_scale = ox.intensity_scale;

    jxlh_frame_params base = VarDctFrame::default_params((uint32_t)w, (uint32_t)h);
    auto b = RenderPipelineBuilder(3, {(size_t)w, (size_t)h}, 0, 8, base)
                 .add_inout_stage(GaborishStage{0, base.gab_w1[0], base.gab_w2[0]})
                 .add_inout_stage(GaborishStage{1, base.gab_w1[1], base.gab_w2[1]})
                 .add_inout_stage(GaborishStage{2, base.gab_w1[2], base.gab_w2[2]});
    const std::array<float, 3> cs{base.epf_channel_scale[0], base.epf_channel_scale[1], base.epf_channel_scale[2]};
    if (epf_iters >= 3) b = std::move(b).add_inout_stage(Epf0Stage{base.epf_pass0_sigma_scale, base.epf_border_sad_mul, cs});
    if (epf_iters >= 1) b = std::move(b).add_inout_stage(Epf1Stage{1.0f, base.epf_border_sad_mul, cs});
    if (epf_iters >= 2) b = std::move(b).add_inout_stage(Epf2Stage{base.epf_pass2_sigma_scale, base.epf_border_sad_mul, cs});
    auto pipe = std::move(b)
                    .add_inplace_stage(XybStage{0, gx})
                    .add_inplace_stage(FromLinearStage{0, JXLH_TF_SRGB, 0.0f, {0.f, 0.f, 0.f}})
                    .add_inout_stage(ConvertF32ToU8Stage{0, 8})
                    .add_inout_stage(ConvertF32ToU8Stage{1, 8})
                    .add_inout_stage(ConvertF32ToU8Stage{2, 8})
                    .add_save_stage({0, 1, 2}, 6, 0, ColorType::kRgba, DataFormat::u8(), true)
                    .build(ctx);
    const LoweredPipeline lowered = pipe->lowered();
    if (lowered.saves.size() != 1 || lowered.saves[0].orientation != 6 || !lowered.saves[0].fill_opaque_alpha) {
      fprintf(stderr, "the stage list did not lower to the save descriptor\n");
      return 1;
    }
    VarDctFrame& frame = pipe->frame();
    frame.decode_hf_global(F.tables);
    frame.decode_lf_group(0, 0, (uint32_t)F.xb, (uint32_t)F.yb, F.qy.data(), F.qx.data(), F.qb.data(), (size_t)F.xb);
    frame.decode_hf_metadata(0, 0, (uint32_t)F.xb, (uint32_t)F.yb, F.tmap.data(), F.rq.data(), F.epf.data(), (size_t)F.xb,
                             F.ytox.data(), F.ytob.data(), (size_t)F.cw);
    // the groups of the second pass: the first and the last one, and the middle one with its right neighbour
    std::vector<uint32_t> later = {0u, (uint32_t)F.ngroups - 1};
    if (F.ngroups >= 6) later.push_back((uint32_t)F.ngroups / 2), later.push_back((uint32_t)F.ngroups / 2 + 1);
    auto is_later = [&](int g) {
      for (uint32_t l : later)
        if ((int)l == g) return true;
      return false;
    };
    std::vector<int32_t> zeros((size_t)3 * 65536, 0);
    for (int g = 0; g < F.ngroups; g++)
      pipe->set_buffer_for_group((uint32_t)g, !is_later(g), is_later(g) ? zeros.data() : &F.coeffs[(size_t)g * 3 * 65536]);
    pipe->do_render();
    // the oriented image: h pixels wide, w rows; a pitch with padding that no call may touch
    const size_t row = (size_t)h * 4, pitch = row + 12;
    pipe->check_buffer_sizes(0, pitch, (size_t)w);
    std::vector<uint8_t> A(pitch * w, 0x5a), B(pitch * w, 0x5a), want(pitch * w, 0x5a);
    pipe->save(0, A.data(), pitch);
    B = A;

    // the oracle's finished frame through the oracle's output stage, then display_pixel of orientation 6: (h - 1 - y, x)
    {
      std::vector<uint8_t> flat((size_t)w * h * 4);
      jxlo_xyb_to_rgb8(&ox, F.pl[0].data(), F.pl[1].data(), F.pl[2].data(), (size_t)w, (size_t)h, F.stride, flat.data(),
                       (size_t)w * 4, 4);
      for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) memcpy(&want[(size_t)x * pitch + (size_t)(h - 1 - y) * 4], &flat[((size_t)y * w + x) * 4], 4);
    }
    const bool stale = memcmp(A.data(), want.data(), A.size()) != 0;  // pass 1 is not the finished picture

    for (uint32_t g : later) pipe->set_buffer_for_group(g, true, &F.coeffs[(size_t)g * 3 * 65536]);
    pipe->do_render();
    const std::vector<jxlh_rect> rects = pipe->changed_rects(later);
    size_t rect_px = 0;
    for (const jxlh_rect& r : rects) rect_px += (size_t)r.w * r.h;
    pipe->save_rects(0, rects, A.data(), pitch);
    size_t bad = 0;
    for (int y = 0; y < w; y++)
      if (memcmp(&A[(size_t)y * pitch], &want[(size_t)y * pitch], pitch) != 0) bad++;

    // the thin wrappers and the C calls: the same rects, the same bytes
    const std::vector<jxlh_rect> again = changed_rects(lowered.frame, later);
    bool same_rects = again.size() == rects.size() && memcmp(again.data(), rects.data(), rects.size() * sizeof(jxlh_rect)) == 0;
    const size_t half = rects.size() / 2;
    frame.save_rects_async(&lowered.output, lowered.saves[0], std::vector<jxlh_rect>(rects.begin(), rects.begin() + half),
                           B.data(), pitch);
    ctx.check(jxlh_frame_save_rects(ctx.raw(), &lowered.output, &lowered.saves[0], rects.data() + half,
                                    (uint32_t)(rects.size() - half), B.data(), pitch),
              "jxlh_frame_save_rects");
    ctx.sync();
    size_t bad_b = 0;
    for (int y = 0; y < w; y++)
      if (memcmp(&B[(size_t)y * pitch], &want[(size_t)y * pitch], pitch) != 0) bad_b++;
    bool threw = false;
    try {
      pipe->save_rects(0, {jxlh_rect{(uint32_t)w, 0, 1, 1}}, A.data(), pitch);  // starts outside the result
    } catch (const Error& e) {
      threw = e.status == JXLH_ERR_INVALID_ARGUMENT;
    }
    printf("%dx%d epf_iters=%d: %zu groups in %zu rects, %zu of %zu pixels repainted; repaint vs oracle: %zu differing rows, "
           "wrappers: %zu differing rows, first pass %s, rects %s, error path %s\n",
           w, h, epf_iters, later.size(), rects.size(), rect_px, (size_t)w * h, bad, bad_b, stale ? "stale" : "ALREADY FINAL",
           same_rects ? "equal" : "DIFFER", threw ? "ok" : "MISSING");
    if (bad != 0 || bad_b != 0 || !stale || !same_rects || !threw || rect_px >= (size_t)w * h) return 1;
  } catch (const Error& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  printf("save rects frame: ok\n");
  return 0;
}
