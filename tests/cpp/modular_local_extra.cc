// One RGBA Modular frame through GpuModularFramePipeline::set_groups(..., dest) (include/jxl_hip_pipeline.hpp): every
// group as decoded with its four channels and local transform list -- jxlh_frame_set_modular_groups_extra -- the colour
// into the frame's planes, the alpha into extra channel 0's sample store; then a second extra channel through
// GpuFramePipeline::set_extra_groups (the n_colour == 0 form) from a batch of one-channel groups.  The rendered planes
// are compared byte for byte with the ones the Python side rendered from the same arena and descriptors through the C
// ABI (ctypes).
//   modular_local_extra INPUT EXPECTED
// INPUT: uint64 w, h, n_groups, n_coded, n_params, arena_samples, n_groups1, n_coded1; the jxlh_local_squeeze_group,
// jxlh_local_coded_channel, jxlh_squeeze_params and jxlh_wp_header (one per group) structs of the RGBA batch; the groups
// and coded channels of the one-channel batch (ranges of the same call-wide arrays, the same arena); the arena (int32).
// EXPECTED: five planes of w * h floats (colour, extra channel 0, extra channel 1).
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
  uint64_t hdr[8];
  if (fread(hdr, sizeof hdr, 1, f) != 1) return 2;
  const uint32_t w = (uint32_t)hdr[0], h = (uint32_t)hdr[1];
  LocalSqueezeGroups in, one;
  in.groups.resize(hdr[2]), in.coded.resize(hdr[3]), in.params.resize(hdr[4]), in.wp.resize(hdr[2]);
  one.groups.resize(hdr[6]), one.coded.resize(hdr[7]);
  std::vector<int32_t> arena(hdr[5]);
  if (!read_all(f, in.groups) || !read_all(f, in.coded) || !read_all(f, in.params) || !read_all(f, in.wp) ||
      !read_all(f, one.groups) || !read_all(f, one.coded) || !read_all(f, arena))
    return 2;
  fclose(f);
  one.params = in.params;  // both batches were packed as one: their ranges index the same call-wide arrays
  std::vector<float> want[5], got[5];
  f = fopen(argv[2], "rb");
  if (!f) return 2;
  for (auto& p : want) {
    p.resize((size_t)w * h);
    if (!read_all(f, p)) return 2;
  }
  fclose(f);
  try {
    Context ctx(0, 1);
    jxlh_frame_params base = VarDctFrame::default_params(w, h);
    base.gab = 0;
    base.epf_iters = 0;
    auto pipe = RenderPipelineBuilder(5, {(size_t)w, (size_t)h}, 0, 8, base)
                    .add_inout_stage(ConvertModularToF32Stage{0, 8})
                    .add_inout_stage(ConvertModularToF32Stage{1, 8})
                    .add_inout_stage(ConvertModularToF32Stage{2, 8})
                    .add_inout_stage(ConvertModularToF32Stage{3, 8})
                    .add_inout_stage(ConvertModularToF32Stage{4, 8})
                    .add_save_stage({0, 1, 2}, 1, 0, ColorType::kRgb, DataFormat::f32(), false)
                    .build_modular_frame(ctx);
    pipe->begin_extra_channel(0, w, h);
    pipe->begin_extra_channel(1, w, h);
    jxlh_local_dest rgba{};
    rgba.n_colour = 3, rgba.n_ec = 1, rgba.ec[0] = 0;
    // in two batches over the same call-wide arrays, the second one asynchronous
    const size_t half = in.groups.size() / 2;
    LocalSqueezeGroups a = in, b = in;
    a.groups.assign(in.groups.begin(), in.groups.begin() + half), a.wp.assign(in.wp.begin(), in.wp.begin() + half);
    b.groups.assign(in.groups.begin() + half, in.groups.end()), b.wp.assign(in.wp.begin() + half, in.wp.end());
    pipe->set_groups(arena.data(), arena.size(), a, rgba);
    pipe->set_groups(arena.data(), arena.size(), b, rgba, /*async=*/true);
    jxlh_local_dest extra{};
    extra.n_colour = 0, extra.n_ec = 1, extra.ec[0] = 1, extra.bit_depth = 8;
    pipe->set_extra_groups(arena.data(), arena.size(), one, extra, /*async=*/true);
    // the channel is not rendered between the call and the run
    bool refused = false;
    std::vector<float> tmp((size_t)w * h);
    try {
      pipe->save_extra_channel(1, tmp.data(), w);
    } catch (const Error& e) {
      refused = e.status == JXLH_ERR_BAD_STATE;
    }
    pipe->render();
    for (auto& p : got) p.assign((size_t)w * h, -7.0f);
    pipe->save_planes(got[0].data(), got[1].data(), got[2].data());
    pipe->save_extra_channel(0, got[3].data(), w);
    pipe->save_extra_channel(1, got[4].data(), w);
    size_t diff = 0;
    for (int c = 0; c < 5; c++) diff += memcmp(got[c].data(), want[c].data(), want[c].size() * sizeof(float)) != 0;
    printf("builder vs ctypes: %zu differing planes\n", diff);
    printf("not-rendered read %s\n", refused ? "refused" : "ACCEPTED");
    if (diff || !refused) return 1;
    // refusals throw before anything ran and name their status: colour through the extra-only wrapper, a channel that is
    // not set, a group with three channels
    int threw = 0;
    try {
      pipe->set_extra_groups(arena.data(), arena.size(), in, rgba);
    } catch (const Error& e) {
      threw += e.status == JXLH_ERR_INVALID_ARGUMENT;
    }
    jxlh_local_dest unset = rgba;
    unset.ec[0] = 5;
    try {
      pipe->set_groups(arena.data(), arena.size(), in, unset);
    } catch (const Error& e) {
      threw += e.status == JXLH_ERR_BAD_STATE;
    }
    LocalSqueezeGroups three = in;
    three.groups[0].n_channels = 3;
    try {
      pipe->set_groups(arena.data(), arena.size(), three, rgba);
    } catch (const Error& e) {
      threw += e.status == JXLH_ERR_INVALID_ARGUMENT;
    }
    printf("refusals: %d of 3\n", threw);
    if (threw != 3) return 1;
  } catch (const Error& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  printf("modular local extra: ok\n");
  return 0;
}
