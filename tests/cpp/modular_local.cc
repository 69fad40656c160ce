// One Modular frame through GpuModularFramePipeline's batched intake (include/jxl_hip_pipeline.hpp): every group as
// decoded plus its local transform list -- jxlh_frame_set_modular_groups -- then the conversions, compared bit for bit
// with the three f32 planes the Python side rendered from the same arena through the C ABI (ctypes).
//   modular_local INPUT EXPECTED
// INPUT: uint64 w, h, n_groups, arena_samples; n_groups jxlh_local_group structs; the arena (int32).
// EXPECTED: three planes of w * h floats.
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
  std::vector<int32_t> arena(hdr[3]);
  if (fread(groups.data(), sizeof(jxlh_local_group), groups.size(), f) != groups.size()) return 2;
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
    std::vector<jxlh_local_program> progs(groups.size());
    size_t bad = 0;
    if (jxlh_modular_local_lower(groups.data(), groups.size(), 8, arena.size(), progs.data(), &bad) != JXLH_OK) {
      fprintf(stderr, "group %zu does not lower\n", bad);
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
    if (pipe->lowered().modular_sample_format != 8) {
      fprintf(stderr, "the stage list did not lower to an 8-bit Modular frame\n");
      return 1;
    }
    // in two batches, the second one asynchronous
    const size_t half = groups.size() / 2;
    std::vector<jxlh_local_group> a(groups.begin(), groups.begin() + half), b(groups.begin() + half, groups.end());
    pipe->set_groups(arena.data(), arena.size(), a);
    pipe->set_groups(arena.data(), arena.size(), b, /*async=*/true);
    pipe->render();
    for (auto& p : got) p.assign((size_t)w * h, -7.0f);
    pipe->save_planes(got[0].data(), got[1].data(), got[2].data());
    size_t diff = 0;
    for (int c = 0; c < 3; c++) diff += memcmp(got[c].data(), want[c].data(), want[c].size() * sizeof(float)) != 0;
    printf("builder vs ctypes: %zu differing planes\n", diff);
    if (diff) return 1;
    // a refused batch throws before anything ran and names its status
    std::vector<jxlh_local_group> broken(1, groups[0]);
    broken[0].steps[0].kind = 2;  // a squeeze
    broken[0].n_steps = 1;
    bool threw = false;
    try {
      pipe->set_groups(arena.data(), arena.size(), broken);
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
  printf("modular local: ok\n");
  return 0;
}
