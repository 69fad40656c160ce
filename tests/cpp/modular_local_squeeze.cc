// One Modular frame through GpuModularFramePipeline::set_groups (the LocalSqueezeGroups overload,
// include/jxl_hip_pipeline.hpp): every group as decoded plus its local transform list, local squeezes among them --
// jxlh_frame_set_modular_groups_squeeze -- then the conversions, compared byte for byte with the three f32 planes the
// Python side rendered from the same arena and descriptors through the C ABI (ctypes); and the stage-level wrapper
// GpuModularPipeline::local_transforms against jxlh_modular_local_transforms_squeeze itself.
//   modular_local_squeeze INPUT EXPECTED
// INPUT: uint64 w, h, n_groups, n_coded, n_params, arena_samples; the jxlh_local_squeeze_group, jxlh_local_coded_channel,
// jxlh_squeeze_params and jxlh_wp_header (one per group) structs; the arena (int32).  EXPECTED: three planes of w * h
// floats.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "jxl_hip_pipeline.hpp"

using namespace jxlh;

template <class T>
static bool read_all(FILE* f, std::vector<T>& v) {
  return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t hdr[6];
  if (fread(hdr, sizeof hdr, 1, f) != 1) return 2;
  const uint32_t w = (uint32_t)hdr[0], h = (uint32_t)hdr[1];
  LocalSqueezeGroups in;
  in.groups.resize(hdr[2]), in.coded.resize(hdr[3]), in.params.resize(hdr[4]), in.wp.resize(hdr[2]);
  std::vector<int32_t> arena(hdr[5]);
  if (!read_all(f, in.groups) || !read_all(f, in.coded) || !read_all(f, in.params) || !read_all(f, in.wp) || !read_all(f, arena)) return 2;
  fclose(f);
  std::vector<float> want[3], got[3];
  f = fopen(argv[2], "rb");
  if (!f) return 2;
  for (auto& p : want) {
    p.resize((size_t)w * h);
    if (!read_all(f, p)) return 2;
  }
  fclose(f);
  try {
    // the batch again through LocalSqueezeGroups::add, as a decoder would assemble it group by group
    LocalSqueezeGroups batch;
    batch.wp = in.wp;
    for (const jxlh_local_squeeze_group& g : in.groups) {
      const std::vector<jxlh_local_step> steps(g.steps, g.steps + g.n_steps);
      const std::vector<jxlh_squeeze_params> sq(in.params.begin() + g.params_first, in.params.begin() + g.params_first + g.n_params);
      const std::vector<jxlh_local_coded_channel> ch(in.coded.begin() + g.coded_first, in.coded.begin() + g.coded_first + g.n_coded);
      batch.add(g.x0, g.y0, g.w, g.h, g.n_channels, steps, g.has_squeeze ? &sq : nullptr, ch);
    }
    // the host lowering alone, as a decoder would ask before it decides where a group's transforms run
    std::vector<jxlh_local_squeeze_program> progs(batch.groups.size());
    size_t bad = 0, squeezed = 0;
    if (jxlh_modular_local_lower_squeeze(batch.groups.data(), batch.groups.size(), batch.coded.data(), batch.coded.size(),
                                         batch.params.data(), batch.params.size(), batch.wp.data(), 8, arena.size(), progs.data(),
                                         &bad) != JXLH_OK) {
      fprintf(stderr, "group %zu does not lower\n", bad);
      return 1;
    }
    for (const auto& p : progs)
      for (uint32_t k = 0; k < p.general.n_coded; k++) squeezed += p.chains[k].n_levels > 0;
    if (squeezed == 0) {
      fprintf(stderr, "the batch holds no squeeze\n");
      return 1;
    }
    uint32_t cw[3] = {w, w, w}, ch3[3] = {h, h, h}, n_default = 0;
    if (jxlh_modular_local_default_squeeze(cw, ch3, 3, 0, nullptr, 0, &n_default) != JXLH_ERR_INVALID_ARGUMENT || n_default < 2) return 1;
    Context ctx(0, 1);
    jxlh_frame_params base = VarDctFrame::default_params(w, h);
    base.gab = 0;
    base.epf_iters = 0;
    auto pipe = RenderPipelineBuilder(3, {(size_t)w, (size_t)h}, 0, 8, base)
                    .add_inout_stage(ConvertModularToF32Stage{0, 8})
                    .add_inout_stage(ConvertModularToF32Stage{1, 8})
                    .add_inout_stage(ConvertModularToF32Stage{2, 8})
                    .add_save_stage({0, 1, 2}, 1, 0, ColorType::kRgb, DataFormat::f32(), false)
                    .build_modular_frame(ctx);
    // in two batches over the same call-wide arrays, the second one asynchronous
    const size_t half = batch.groups.size() / 2;
    LocalSqueezeGroups a = batch, b = batch;
    a.groups.assign(batch.groups.begin(), batch.groups.begin() + half), a.wp.assign(batch.wp.begin(), batch.wp.begin() + half);
    b.groups.assign(batch.groups.begin() + half, batch.groups.end()), b.wp.assign(batch.wp.begin() + half, batch.wp.end());
    pipe->set_groups(arena.data(), arena.size(), a);
    pipe->set_groups(arena.data(), arena.size(), b, /*async=*/true);
    pipe->render();
    for (auto& p : got) p.assign((size_t)w * h, -7.0f);
    pipe->save_planes(got[0].data(), got[1].data(), got[2].data());
    size_t diff = 0;
    for (int c = 0; c < 3; c++) diff += memcmp(got[c].data(), want[c].data(), want[c].size() * sizeof(float)) != 0;
    printf("builder vs ctypes: %zu differing planes\n", diff);
    if (diff) return 1;
    // the stage-level wrapper against the C call: the same i32 planes
    auto stage = RenderPipelineBuilder(3, {(size_t)w, (size_t)h}, 0, 8, base)
                     .add_inout_stage(ConvertModularToF32Stage{0, 8})
                     .add_inout_stage(ConvertModularToF32Stage{1, 8})
                     .add_inout_stage(ConvertModularToF32Stage{2, 8})
                     .add_save_stage({0, 1, 2}, 0, 3, 32)
                     .build_modular(ctx);
    const size_t n = (size_t)w * h;
    int32_t* dev[2][3];
    for (auto& set : dev)
      for (auto& p : set)
        if (hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(int32_t)) != hipSuccess || hipMemset(p, 0x5a, n * sizeof(int32_t)) != hipSuccess) return 2;
    stage->local_transforms(arena.data(), arena.size(), batch, 8, dev[0], 3, w);
    if (jxlh_modular_local_transforms_squeeze(ctx.raw(), arena.data(), arena.size(), in.groups.data(), in.groups.size(), in.coded.data(),
                                              in.coded.size(), in.params.data(), in.params.size(), in.wp.data(), 8, dev[1], 3, w, h, w,
                                              nullptr) != JXLH_OK)
      return 1;
    std::vector<int32_t> x(n), y(n);
    size_t sdiff = 0;
    for (int c = 0; c < 3; c++) {
      if (hipMemcpy(x.data(), dev[0][c], n * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return 2;
      if (hipMemcpy(y.data(), dev[1][c], n * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return 2;
      sdiff += memcmp(x.data(), y.data(), n * sizeof(int32_t)) != 0;
    }
    for (auto& set : dev)
      for (auto& p : set) (void)hipFree(p);
    printf("stage wrapper vs C call: %zu differing planes\n", sdiff);
    if (sdiff) return 1;
    // a refused batch throws before anything ran and names its status
    LocalSqueezeGroups broken = batch;
    for (auto& g : broken.groups)
      if (g.has_squeeze) g.n_coded -= 1;  // a residual channel has not arrived: previews stay on the host
    bool threw = false;
    try {
      pipe->set_groups(arena.data(), arena.size(), broken);
    } catch (const Error& e) {
      threw = e.status == JXLH_ERR_UNSUPPORTED;
    }
    if (!threw) {
      fprintf(stderr, "a missing coded channel was not refused as unsupported\n");
      return 1;
    }
  } catch (const Error& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  printf("modular local squeeze: ok\n");
  return 0;
}
