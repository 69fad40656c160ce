// One Modular frame through GpuModularFramePipeline::set_groups_general (include/jxl_hip_pipeline.hpp): every group as
// decoded plus its local transform list, delta palettes under every kind of predictor among them --
// jxlh_frame_set_modular_groups_general -- then the conversions, compared byte for byte with the three f32 planes the
// Python side rendered from the same arena, descriptors and wp headers through the C ABI (ctypes); and the stage-level
// wrapper GpuModularPipeline::local_transforms_general against jxlh_modular_local_transforms_general itself.
//   modular_local_general INPUT EXPECTED
// INPUT: uint64 w, h, n_groups, arena_samples; n_groups jxlh_local_group structs; n_groups jxlh_wp_header structs; the
// arena (int32).  EXPECTED: three planes of w * h floats.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "jxl_hip_pipeline.hpp"

using namespace jxlh;

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t hdr[4];
  if (fread(hdr, sizeof hdr, 1, f) != 1) return 2;
  const uint32_t w = (uint32_t)hdr[0], h = (uint32_t)hdr[1];
  std::vector<jxlh_local_group> groups(hdr[2]);
  std::vector<jxlh_wp_header> wp(hdr[2]);
  std::vector<int32_t> arena(hdr[3]);
  if (fread(groups.data(), sizeof(jxlh_local_group), groups.size(), f) != groups.size()) return 2;
  if (fread(wp.data(), sizeof(jxlh_wp_header), wp.size(), f) != wp.size()) return 2;
  if (fread(arena.data(), sizeof(int32_t), arena.size(), f) != arena.size()) return 2;
  fclose(f);
  std::vector<float> want[3], got[3];
  f = fopen(argv[2], "rb");
  if (!f) return 2;
  for (auto& p : want) {
    p.resize((size_t)w * h);
    if (fread(p.data(), sizeof(float), p.size(), f) != p.size()) return 2;
  }
  fclose(f);
  try {
    // the host lowering alone, as a decoder would ask before it decides where a group's transforms run
    std::vector<jxlh_local_general_program> progs(groups.size());
    size_t bad = 0, general = 0;
    if (jxlh_modular_local_lower_general(groups.data(), wp.data(), groups.size(), 8, arena.size(), progs.data(), &bad) != JXLH_OK) {
      fprintf(stderr, "group %zu does not lower\n", bad);
      return 1;
    }
    for (const auto& p : progs) general += p.n_phases > 1;
    if (general == 0 || jxlh_modular_local_lower(groups.data(), groups.size(), 8, arena.size(), nullptr, &bad) != JXLH_ERR_UNSUPPORTED) {
      fprintf(stderr, "the batch holds no general palette\n");
      return 1;
    }
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
    // in two batches, the second one asynchronous
    const size_t half = groups.size() / 2;
    std::vector<jxlh_local_group> a(groups.begin(), groups.begin() + half), b(groups.begin() + half, groups.end());
    std::vector<jxlh_wp_header> wa(wp.begin(), wp.begin() + half), wb(wp.begin() + half, wp.end());
    pipe->set_groups_general(arena.data(), arena.size(), a, wa);
    pipe->set_groups_general(arena.data(), arena.size(), b, wb, /*async=*/true);
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
    stage->local_transforms_general(arena.data(), arena.size(), groups, wp, 8, dev[0], 3, w);
    if (jxlh_modular_local_transforms_general(ctx.raw(), arena.data(), arena.size(), groups.data(), wp.data(), groups.size(), 8, dev[1],
                                              3, w, h, w, nullptr) != JXLH_OK)
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
    std::vector<jxlh_local_group> broken(1, groups[0]);
    broken[0].steps[0].kind = 2;  // a squeeze
    broken[0].n_steps = 1;
    bool threw = false;
    try {
      pipe->set_groups_general(arena.data(), arena.size(), broken, {});
    } catch (const Error& e) {
      threw = e.status == JXLH_ERR_UNSUPPORTED;
    }
    if (!threw) {
      fprintf(stderr, "a local squeeze was not refused as unsupported\n");
      return 1;
    }
  } catch (const Error& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  printf("modular local general: ok\n");
  return 0;
}
