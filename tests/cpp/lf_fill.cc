// The streaming sequence of a file that is still arriving, three ways, on one synthetic VarDCT frame:
//   * the plain C calls: jxlh_frame_set_groups_lf_only on every group, jxlh_frame_run (the first paint), then two groups
//     arrive (jxlh_submit_group + jxlh_frame_rerender_groups), then the rest;
//   * VarDctFrame::upsample_lf_groups / decode_vardct_group with the same renders;
//   * GpuRenderPipeline::set_lf_only_group / set_buffer_for_group / do_render with the reference's stage list.
// After each of the three steps the three results must be bit-identical; the first paint must differ from the final
// image, and the final image must be the oracle's frame (the Python tests hold the C calls to the builder of
// tests/lf_fill_ref.py; this one holds the C++ layers to the C calls).
//   lf_fill W H ITERS
#include <cstdio>
#include <cstring>

#include "jxl_hip_pipeline.hpp"
#include "synth_frame.hpp"

using namespace jxlh;

namespace {
struct Planes {
  std::vector<float> c[3];
  explicit Planes(size_t n) {
    for (auto& p : c) p.assign(n, -1.0f);
  }
};
void feed(VarDctFrame& frame, const synth::Frame& F) {
  frame.decode_hf_global(F.tables);
  frame.decode_lf_group(0, 0, (uint32_t)F.xb, (uint32_t)F.yb, F.qy.data(), F.qx.data(), F.qb.data(), (size_t)F.xb);
  frame.decode_hf_metadata(0, 0, (uint32_t)F.xb, (uint32_t)F.yb, F.tmap.data(), F.rq.data(), F.epf.data(), (size_t)F.xb,
                           F.ytox.data(), F.ytob.data(), (size_t)F.cw);
}
size_t differing_rows(const Planes& a, const Planes& b, int w, int h) {
  size_t bad = 0;
  for (int c = 0; c < 3; c++)
    for (int y = 0; y < h; y++) bad += memcmp(&a.c[c][(size_t)y * w], &b.c[c][(size_t)y * w], sizeof(float) * w) != 0;
  return bad;
}
}  // namespace

int main(int argc, char** argv) {
  const int w = argc > 1 ? atoi(argv[1]) : 520, h = argc > 2 ? atoi(argv[2]) : 300, epf_iters = argc > 3 ? atoi(argv[3]) : 2;
  synth::Frame F;
  if (!synth::make(w, h, epf_iters, &F)) return 2;
  if (F.ngroups < 3) return 2;
  const size_t npx = (size_t)w * h;
  std::vector<uint32_t> every, first{(uint32_t)F.ngroups - 1, 0}, rest;
  for (int g = 0; g < F.ngroups; g++) every.push_back((uint32_t)g);
  for (int g = 1; g + 1 < F.ngroups; g++) rest.push_back((uint32_t)g);
  auto slab = [&](uint32_t g) { return &F.coeffs[(size_t)g * 3 * 65536]; };
  try {
    Context ctx(0, 1);
    jxlh_frame_params base = VarDctFrame::default_params((uint32_t)w, (uint32_t)h);
    base.epf_iters = (uint32_t)epf_iters;
    Planes c0(npx), c1(npx), c2(npx), v0(npx), v1(npx), v2(npx), p0(npx), p1(npx), p2(npx);
    // ---- the C calls
    {
      VarDctFrame frame(ctx, base);  // (jxlh_frame_begin)
      feed(frame, F);
      auto read = [&](Planes& o) { frame.read_planes(o.c[0].data(), o.c[1].data(), o.c[2].data()); };
      ctx.check(jxlh_frame_set_groups_lf_only(ctx.raw(), every.data(), (uint32_t)every.size()), "set_groups_lf_only");
      ctx.check(jxlh_frame_run(ctx.raw(), 0, 0xFFFFFFFFu), "jxlh_frame_run");
      read(c0);
      for (uint32_t g : first) ctx.check(jxlh_submit_group(ctx.raw(), 0, g, slab(g), JXLH_GROUP_COMPLETE), "jxlh_submit_group");
      ctx.check(jxlh_slot_wait(ctx.raw(), 0), "jxlh_slot_wait");
      ctx.check(jxlh_frame_rerender_groups(ctx.raw(), first.data(), (uint32_t)first.size()), "rerender");
      read(c1);
      for (uint32_t g : rest) ctx.check(jxlh_submit_group(ctx.raw(), 0, g, slab(g), JXLH_GROUP_COMPLETE), "jxlh_submit_group");
      ctx.check(jxlh_slot_wait(ctx.raw(), 0), "jxlh_slot_wait");
      ctx.check(jxlh_frame_rerender_groups(ctx.raw(), rest.data(), (uint32_t)rest.size()), "rerender");
      read(c2);
    }
    // ---- VarDctFrame
    {
      VarDctFrame frame(ctx, base);
      feed(frame, F);
      auto read = [&](Planes& o) { frame.read_planes(o.c[0].data(), o.c[1].data(), o.c[2].data()); };
      frame.upsample_lf_groups(every.data(), (uint32_t)every.size());
      frame.finalize_and_render();
      read(v0);
      for (uint32_t g : first) frame.decode_vardct_group(g, slab(g));
      frame.slot_wait();
      ctx.check(jxlh_frame_rerender_groups(ctx.raw(), first.data(), (uint32_t)first.size()), "rerender");
      read(v1);
      for (uint32_t g : rest) frame.decode_vardct_group(g, slab(g));
      frame.slot_wait();
      frame.finalize_and_render();  // (a whole run: no group is marked any more)
      read(v2);
    }
    // ---- the builder
    {
      auto bld = RenderPipelineBuilder(3, {(size_t)w, (size_t)h}, 0, 8, base)
                     .add_inout_stage(GaborishStage{0, base.gab_w1[0], base.gab_w2[0]})
                     .add_inout_stage(GaborishStage{1, base.gab_w1[1], base.gab_w2[1]})
                     .add_inout_stage(GaborishStage{2, base.gab_w1[2], base.gab_w2[2]});
      const std::array<float, 3> cs{base.epf_channel_scale[0], base.epf_channel_scale[1], base.epf_channel_scale[2]};
      if (epf_iters >= 3) bld = std::move(bld).add_inout_stage(Epf0Stage{base.epf_pass0_sigma_scale, base.epf_border_sad_mul, cs});
      if (epf_iters >= 1) bld = std::move(bld).add_inout_stage(Epf1Stage{1.0f, base.epf_border_sad_mul, cs});
      if (epf_iters >= 2) bld = std::move(bld).add_inout_stage(Epf2Stage{base.epf_pass2_sigma_scale, base.epf_border_sad_mul, cs});
      auto pipe = std::move(bld).add_save_stage({0, 1, 2}, 0, 3, 32).build(ctx);
      feed(pipe->frame(), F);
      for (uint32_t g : every) pipe->set_lf_only_group(g);
      pipe->do_render();
      pipe->save_planes(p0.c[0].data(), p0.c[1].data(), p0.c[2].data());
      for (uint32_t g : first) pipe->set_buffer_for_group(g, true, slab(g));
      pipe->do_render();
      pipe->save_planes(p1.c[0].data(), p1.c[1].data(), p1.c[2].data());
      // one group is handed back to the LF before it arrives for good: the pipeline re-renders it both times
      pipe->set_lf_only_group(first[0]);
      for (uint32_t g : rest) pipe->set_buffer_for_group(g, true, slab(g));
      pipe->set_buffer_for_group(first[0], true, slab(first[0]));
      pipe->do_render();
      pipe->save_planes(p2.c[0].data(), p2.c[1].data(), p2.c[2].data());
    }
    const size_t s0 = differing_rows(c0, v0, w, h) + differing_rows(c0, p0, w, h);
    const size_t s1 = differing_rows(c1, v1, w, h) + differing_rows(c1, p1, w, h);
    const size_t s2 = differing_rows(c2, v2, w, h) + differing_rows(c2, p2, w, h);
    size_t vs_oracle = 0;
    for (int c = 0; c < 3; c++)
      for (int y = 0; y < h; y++) vs_oracle += memcmp(&c2.c[c][(size_t)y * w], &F.pl[c][(size_t)y * F.stride], sizeof(float) * w) != 0;
    const size_t painted = differing_rows(c0, c2, w, h), arrived = differing_rows(c0, c1, w, h);
    printf("first paint: %zu differing rows; two groups: %zu; all groups: %zu; final vs oracle: %zu; first paint vs final: %zu rows, "
           "vs two groups: %zu rows\n", s0, s1, s2, vs_oracle, painted, arrived);
    if (s0 || s1 || s2 || vs_oracle || painted == 0 || arrived == 0) return 1;
  } catch (const Error& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  printf("lf fill: ok\n");
  return 0;
}
