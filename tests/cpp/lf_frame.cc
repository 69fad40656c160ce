// A Modular XYB LF frame (lf_level 1) through build_modular_frame and GpuFramePipeline::save_lf into LF slot 0, then the
// full-size preview of the slot through Context::lf_preview, byte-compared with the image the Python side made from the
// same samples through the C ABI (ctypes); the same preview again from a slot filled by Context::set_lf_frame with the
// planes the pipeline hands back; Context::set_lf_from_slot / save_lf outside a frame throw JXLH_ERR_BAD_STATE.
//   lf_frame INPUT EXPECTED
// INPUT: int32 image_w, image_h; 16 floats jxlh_xyb_params; 3 floats lf_quant_factors; the coded Y, X, B planes
// (slot_w * slot_h int32 each, slot = ceil(image / 8)).  EXPECTED: image_h rows of image_w RGBA8 pixels.
#include <cstdio>
#include <vector>

#include "jxl_hip_pipeline.hpp"

using namespace jxlh;

namespace {
template <class T>
bool read_n(FILE* f, std::vector<T>* v, size_t n) {
  v->resize(n);
  return fread(v->data(), sizeof(T), n, f) == n;
}
template <class F>
jxlh_status status_of(F f) {
  try {
    f();
  } catch (const Error& e) {
    return e.status;
  }
  return JXLH_OK;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[2];
  jxlh_xyb_params xyb;
  float factors[3];
  if (fread(hdr, sizeof hdr, 1, f) != 1 || fread(&xyb, sizeof xyb, 1, f) != 1 || fread(factors, sizeof factors, 1, f) != 1)
    return 2;
  const uint32_t iw = (uint32_t)hdr[0], ih = (uint32_t)hdr[1], sw = (iw + 7) / 8, sh = (ih + 7) / 8;
  std::vector<int32_t> chan[3];
  for (auto& c : chan)
    if (!read_n(f, &c, (size_t)sw * sh)) return 2;
  fclose(f);
  std::vector<uint8_t> want;
  f = fopen(argv[2], "rb");
  if (!f || !read_n(f, &want, (size_t)iw * ih * 4)) return 2;
  fclose(f);
  try {
    Context ctx(0, 1);
    if (status_of([&] { ctx.set_lf_from_slot(0); }) != JXLH_ERR_BAD_STATE || status_of([&] { ctx.save_lf(0); }) != JXLH_ERR_BAD_STATE) {
      fprintf(stderr, "set_lf_from_slot / save_lf outside a frame were not refused\n");
      return 1;
    }
    jxlh_frame_params base = VarDctFrame::default_params(sw, sh);
    base.gab = 0;
    base.epf_iters = 0;
    auto pipe = RenderPipelineBuilder(3, {(size_t)sw, (size_t)sh}, 0, 8, base)
                    .add_inout_stage(ConvertModularXYBToF32Stage{0, {factors[0], factors[1], factors[2]}})
                    .add_save_stage({0, 1, 2}, 0, 3, 32)
                    .build_modular_frame(ctx);
    const int32_t* planes[3] = {chan[0].data(), chan[1].data(), chan[2].data()};
    pipe->set_channels(0, 0, sw, sh, planes, sw);
    pipe->render();
    pipe->save_lf(0);  // lf_level 1
    jxlh_output_desc colour{};
    colour.color = JXLH_COLOR_XYB;
    colour.transfer = JXLH_TF_SRGB;
    colour.xyb = xyb;
    jxlh_save_desc save{};
    save.n_channels = 3;
    save.channels[0] = 0;
    save.channels[1] = 1;
    save.channels[2] = 2;
    save.fill_opaque_alpha = 1;
    save.format = JXLH_SAVE_U8;
    save.bit_depth = 8;
    save.orientation = 1;
    const size_t row = (size_t)iw * 4;
    std::vector<uint8_t> got(row * ih, 0x11);
    ctx.lf_preview(0, iw, ih, 0, 0, sw, sh, colour, save, got.data(), row);
    size_t bad = 0;
    for (size_t i = 0; i < got.size(); i++) bad += got[i] != want[i];
    printf("pipeline save_lf + lf_preview vs ctypes: %zu differing bytes\n", bad);
    if (bad) return 1;
    // the same planes handed over by the caller, previewed in two rects
    std::vector<float> pl[3];
    for (auto& p : pl) p.resize((size_t)sw * sh);
    pipe->save_planes(pl[0].data(), pl[1].data(), pl[2].data());
    pipe.reset();
    ctx.set_lf_frame(1, sw, sh, pl[0].data(), pl[1].data(), pl[2].data(), sw);
    ctx.clear_lf_frame(0);
    std::vector<uint8_t> again(row * ih, 0x22);
    ctx.lf_preview(1, iw, ih, 0, 0, sw, 1, colour, save, again.data(), row);
    ctx.lf_preview(1, iw, ih, 0, 1, sw, sh - 1, colour, save, again.data(), row);
    if (again != got) {
      fprintf(stderr, "the preview of the slot set by set_lf_frame differs\n");
      return 1;
    }
    ctx.clear_lf_frame(1);
    if (status_of([&] { ctx.lf_preview(1, iw, ih, 0, 0, sw, sh, colour, save, again.data(), row); }) != JXLH_ERR_INVALID_ARGUMENT) {
      fprintf(stderr, "a cleared slot was previewed\n");
      return 1;
    }
  } catch (const Error& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  printf("lf frame: ok\n");
  return 0;
}
