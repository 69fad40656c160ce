// One Modular frame with an alpha extra channel through build_modular_frame (include/jxl_hip_pipeline.hpp): the
// reference's list -- ConvertModularToF32Stage x3 and the alpha's, Gaborish, EPF1, patches, XybStage, FromLinearStage,
// ConvertF32ToU8Stage x4, an RGBA8 save -- on samples, reference planes and colour parameters read from a file the
// Python side wrote, byte-compared with the image the same side made through the C ABI (ctypes).
//   modular_frame INPUT EXPECTED
// INPUT: int32 w, h, ref_w, ref_h; 16 floats jxlh_xyb_params; 3 colour planes and the alpha plane (w * h int32 each);
// 4 reference planes (ref_w * ref_h floats each).  EXPECTED: h rows of w RGBA8 pixels.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "jxl_hip_pipeline.hpp"

using namespace jxlh;

namespace {
template <class T>
bool read_n(FILE* f, std::vector<T>* v, size_t n) {
  v->resize(n);
  return fread(v->data(), sizeof(T), n, f) == n;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[4];
  jxlh_xyb_params xyb;
  static_assert(sizeof(xyb) == 16 * sizeof(float), "jxlh_xyb_params is 16 floats");
  if (fread(hdr, sizeof hdr, 1, f) != 1 || fread(&xyb, sizeof xyb, 1, f) != 1) return 2;
  const uint32_t w = (uint32_t)hdr[0], h = (uint32_t)hdr[1], rw = (uint32_t)hdr[2], rh = (uint32_t)hdr[3];
  std::vector<int32_t> chan[3], alpha;
  std::vector<float> ref[4];
  for (auto& c : chan)
    if (!read_n(f, &c, (size_t)w * h)) return 2;
  if (!read_n(f, &alpha, (size_t)w * h)) return 2;
  for (auto& r : ref)
    if (!read_n(f, &r, (size_t)rw * rh)) return 2;
  fclose(f);
  std::vector<uint8_t> want;
  f = fopen(argv[2], "rb");
  if (!f || !read_n(f, &want, (size_t)w * h * 4)) return 2;
  fclose(f);
  try {
    Context ctx(0, 1);
    const float* rp[4] = {ref[0].data(), ref[1].data(), ref[2].data(), ref[3].data()};
    ctx.check(jxlh_ctx_set_reference(ctx.raw(), 0, 4, rw, rh, rp, rw), "jxlh_ctx_set_reference");
    PatchesStage ps;
    ps.patches = {jxlh_patch{3, 2, 0, 5, 4, 40, 20}, jxlh_patch{50, 20, 0, 0, 0, 20, 17}};
    ps.blendings = {jxlh_patch_blending{JXLH_PATCH_REPLACE, 0, 0}, jxlh_patch_blending{JXLH_PATCH_REPLACE, 0, 0},
                    jxlh_patch_blending{JXLH_PATCH_BLEND_ABOVE, 0, 1}, jxlh_patch_blending{JXLH_PATCH_BLEND_ABOVE, 0, 0}};
    ps.ec_flags = {JXLH_EC_ALPHA};
    const jxlh_frame_params base = VarDctFrame::default_params(w, h);
    const std::array<float, 3> cs{base.epf_channel_scale[0], base.epf_channel_scale[1], base.epf_channel_scale[2]};
    auto pipe = RenderPipelineBuilder(4, {(size_t)w, (size_t)h}, 0, 8, base)
                    .add_inout_stage(ConvertModularToF32Stage{0, 8})
                    .add_inout_stage(ConvertModularToF32Stage{1, 8})
                    .add_inout_stage(ConvertModularToF32Stage{2, 8})
                    .add_inout_stage(ConvertModularToF32Stage{3, 8})
                    .add_inout_stage(GaborishStage{0, base.gab_w1[0], base.gab_w2[0]})
                    .add_inout_stage(GaborishStage{1, base.gab_w1[1], base.gab_w2[1]})
                    .add_inout_stage(GaborishStage{2, base.gab_w1[2], base.gab_w2[2]})
                    .add_inout_stage(Epf1Stage{1.0f, base.epf_border_sad_mul, cs})
                    .add_inplace_stage(ps)
                    .add_inplace_stage(XybStage{0, xyb})
                    .add_inplace_stage(FromLinearStage{0, JXLH_TF_SRGB, 0.0f, {0.2627f, 0.678f, 0.0593f}})
                    .add_inout_stage(ConvertF32ToU8Stage{0, 8})
                    .add_inout_stage(ConvertF32ToU8Stage{1, 8})
                    .add_inout_stage(ConvertF32ToU8Stage{2, 8})
                    .add_inout_stage(ConvertF32ToU8Stage{3, 8})
                    .add_save_stage({0, 1, 2, 3}, 1, 0, ColorType::kRgba, DataFormat::u8(), false)
                    .build_modular_frame(ctx);
    const LoweredPipeline& lp = pipe->lowered();
    if (!(lp.frame.flags & JXLH_FRAME_MODULAR) || lp.modular_sample_format != 8 || !lp.has_patches || lp.saves.size() != 1) {
      fprintf(stderr, "the stage list did not lower to a Modular frame with patches and one save\n");
      return 1;
    }
    // in two rects, the lower one first
    const uint32_t cut = h / 2 + 1;
    const int32_t* lower[3] = {chan[0].data() + (size_t)cut * w, chan[1].data() + (size_t)cut * w, chan[2].data() + (size_t)cut * w};
    const int32_t* upper[3] = {chan[0].data(), chan[1].data(), chan[2].data()};
    pipe->set_channels(0, cut, w, h - cut, lower, w);
    pipe->set_channels(0, 0, w, cut, upper, w);
    pipe->set_extra_channel_buffer(0, alpha.data(), w, w, h);
    pipe->render();
    const size_t row = (size_t)w * 4;
    pipe->check_buffer_sizes(0, row, h);
    std::vector<uint8_t> got(row * h, 0x11);
    pipe->save(0, got.data(), row);
    size_t bad = 0;
    for (size_t i = 0; i < got.size(); i++) bad += got[i] != want[i];
    printf("builder vs ctypes: %zu differing bytes\n", bad);
    if (bad) return 1;
    // a band run of the same frame leaves the same image
    pipe->render_band(0, 1);
    std::vector<uint8_t> again(row * h, 0x22);
    pipe->save(0, again.data(), row);
    if (again != got) {
      fprintf(stderr, "render_band changed the image\n");
      return 1;
    }
    pipe.reset();
    ctx.check(jxlh_ctx_clear_reference(ctx.raw(), 0), "jxlh_ctx_clear_reference");
  } catch (const Error& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  printf("modular frame: ok\n");
  return 0;
}
