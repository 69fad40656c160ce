// Extra channels by rect through the C++ layer: one synthetic VarDCT frame whose two extra channels -- 8-bit alpha
// coded at half resolution (Upsample2x) and a 16-bit channel at full resolution -- are declared with
// GpuFramePipeline::begin_extra_channel and arrive as rects (set_extra_channel_rects, blocking and _async, from host
// blocks with padded strides); after the first do_render() one rect of each channel is replaced and group 1 is
// re-rendered.  The two finished channels are written to OUT as raw f32 (alpha, then depth, w x h each), where
// tests/test_gpu_extra_rects_cpp.py compares them byte for byte with the ctypes route fed the same samples; the
// wrappers of jxlh_extra_channel_changed_rects are held to the C call here.
//   extra_rects W H OUT
#include <cstdio>
#include <cstring>
#include <string>

#include "jxl_hip_pipeline.hpp"
#include "synth_frame.hpp"

using namespace jxlh;

namespace {
// the rects of a cw x ch channel cut at (x1, x2) x (y1, y2), rows `pad` samples apart beyond their width, appended to
// one block
void cut_rects(uint32_t ec, const std::vector<int32_t>& plane, uint32_t cw, uint32_t ch, uint32_t pad, std::vector<int32_t>& block,
               std::vector<jxlh_ec_rect>& rects) {
  const uint32_t xs[4] = {0, 1, cw / 2 + 1, cw}, ys[4] = {0, ch / 3, ch - 1, ch};
  for (int j = 0; j < 3; j++)
    for (int i = 0; i < 3; i++) {
      jxlh_ec_rect r{};
      r.ec = ec;
      r.x0 = xs[i], r.y0 = ys[j], r.w = xs[i + 1] - xs[i], r.h = ys[j + 1] - ys[j];
      r.offset = block.size();
      r.stride = r.w + pad;
      for (uint32_t y = 0; y < r.h; y++) {
        for (uint32_t x = 0; x < r.w; x++) block.push_back(plane[(size_t)(r.y0 + y) * cw + r.x0 + x]);
        for (uint32_t x = 0; x < pad; x++) block.push_back(0x7fffffff);
      }
      rects.push_back(r);
    }
}
}  // namespace

int main(int argc, char** argv) {
  const int w = argc > 1 ? atoi(argv[1]) : 264, h = argc > 2 ? atoi(argv[2]) : 200;
  const char* out_path = argc > 3 ? argv[3] : "extra_rects.f32";
  synth::Frame F;
  if (!synth::make(w, h, 1, &F)) return 2;
  try {
    Context ctx(0, 1);
    jxlh_frame_params base = VarDctFrame::default_params((uint32_t)w, (uint32_t)h);
    const std::array<float, 3> cs{base.epf_channel_scale[0], base.epf_channel_scale[1], base.epf_channel_scale[2]};
    auto pipe = RenderPipelineBuilder(5, {(size_t)w, (size_t)h}, 0, 8, base)
                    .add_inout_stage(ConvertModularToF32Stage{3, 8})
                    .add_inout_stage(ConvertModularToF32Stage{4, 16})
                    .add_inout_stage(GaborishStage{0, base.gab_w1[0], base.gab_w2[0]})
                    .add_inout_stage(GaborishStage{1, base.gab_w1[1], base.gab_w2[1]})
                    .add_inout_stage(GaborishStage{2, base.gab_w1[2], base.gab_w2[2]})
                    .add_inout_stage(Epf1Stage{1.0f, base.epf_border_sad_mul, cs})
                    .add_inout_stage(Upsample2x{nullptr, 3})
                    .add_save_stage({0, 1, 2}, 0, 3, 32)
                    .build(ctx);
    const uint32_t aw = (uint32_t)(w + 1) / 2, ah = (uint32_t)(h + 1) / 2;
    std::vector<int32_t> alpha((size_t)aw * ah), depth((size_t)w * h);
    uint32_t lcg = 12345u;
    for (auto& v : alpha) v = (int32_t)((lcg = lcg * 1664525u + 1013904223u) >> 24);
    for (auto& v : depth) v = (int32_t)((lcg = lcg * 1664525u + 1013904223u) >> 16);
    pipe->begin_extra_channel(0, aw, ah);
    pipe->begin_extra_channel(1, (uint32_t)w, (uint32_t)h);
    {
      std::vector<int32_t> block;
      std::vector<jxlh_ec_rect> rects;
      cut_rects(0, alpha, aw, ah, 3, block, rects);
      pipe->set_extra_channel_rects(block.data(), block.size(), rects);
      std::fill(block.begin(), block.end(), 0);  // the blocking form has returned: the block may be reused
      std::vector<int32_t> block2;
      rects.clear();
      cut_rects(1, depth, (uint32_t)w, (uint32_t)h, 0, block2, rects);
      pipe->set_extra_channel_rects_async(block2.data(), block2.size(), rects);
      ctx.sync();
    }
    VarDctFrame& frame = pipe->frame();
    frame.decode_hf_global(F.tables);
    frame.decode_lf_group(0, 0, (uint32_t)F.xb, (uint32_t)F.yb, F.qy.data(), F.qx.data(), F.qb.data(), (size_t)F.xb);
    frame.decode_hf_metadata(0, 0, (uint32_t)F.xb, (uint32_t)F.yb, F.tmap.data(), F.rq.data(), F.epf.data(), (size_t)F.xb,
                             F.ytox.data(), F.ytob.data(), (size_t)F.cw);
    for (int g = 0; g < F.ngroups; g++) pipe->set_buffer_for_group((uint32_t)g, true, &F.coeffs[(size_t)g * 3 * 65536]);
    pipe->do_render();
    // the update: a rect of each channel across its tile seams (x = 64, y = 16), then group 1 again
    std::vector<jxlh_rect> upd = {{60, 13, 9, 7}};
    {
      std::vector<int32_t> block;
      std::vector<jxlh_ec_rect> rects;
      for (uint32_t ec = 0; ec < 2; ec++) {
        std::vector<int32_t>& plane = ec ? depth : alpha;
        const uint32_t cw = ec ? (uint32_t)w : aw;
        jxlh_ec_rect r{ec, upd[0].x0, upd[0].y0, upd[0].w, upd[0].h, block.size(), upd[0].w};
        for (uint32_t y = 0; y < r.h; y++)
          for (uint32_t x = 0; x < r.w; x++) {
            int32_t& v = plane[(size_t)(r.y0 + y) * cw + r.x0 + x];
            v ^= 0x55;
            block.push_back(v);
          }
        rects.push_back(r);
      }
      pipe->set_extra_channel_rects(block.data(), block.size(), rects);
    }
    bool refused = false;
    std::vector<float> got((size_t)w * h);
    try {
      pipe->save_extra_channel(0, got.data(), (size_t)w);  // handed over, not rendered
    } catch (const Error& e) {
      refused = e.status == JXLH_ERR_BAD_STATE;
    }
    pipe->mark_group_to_rerender(1);
    pipe->do_render();
    ctx.sync();
    FILE* f = fopen(out_path, "wb");
    if (!f) return 2;
    for (uint32_t ec = 0; ec < 2; ec++) {
      pipe->save_extra_channel(ec, got.data(), (size_t)w);
      if (fwrite(got.data(), sizeof(float), got.size(), f) != got.size()) return 2;
    }
    fclose(f);
    // the wrappers name the rects the C call names
    size_t bad = 0;
    for (uint32_t ec = 0; ec < 2; ec++) {
      const uint32_t cw = ec ? (uint32_t)w : aw, chh = ec ? (uint32_t)h : ah, up = ec ? 1u : 2u;
      jxlh_rect want{};
      uint32_t n = 0;
      if (jxlh_extra_channel_changed_rects(cw, chh, up, (uint32_t)w, (uint32_t)h, upd.data(), 1, &want, 1, &n) != JXLH_OK || n != 1) bad++;
      const std::vector<jxlh_rect> a = pipe->extra_channel_changed_rects(ec, cw, chh, upd);
      const std::vector<jxlh_rect> b = extra_channel_changed_rects(cw, chh, up, (uint32_t)w, (uint32_t)h, upd);
      if (a.size() != 1 || b.size() != 1 || memcmp(&a[0], &want, sizeof want) != 0 || memcmp(&b[0], &want, sizeof want) != 0) bad++;
    }
    bool threw = false;
    try {
      pipe->begin_extra_channel(0, aw, ah);  // begun already in this frame
    } catch (const Error& e) {
      threw = e.status == JXLH_ERR_BAD_STATE;
    }
    printf("rects %s, not-rendered read %s, second begin %s\n", bad ? "DIFFER" : "equal", refused ? "refused" : "ACCEPTED",
           threw ? "refused" : "ACCEPTED");
    if (bad || !refused || !threw) return 1;
  } catch (const Error& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  printf("extra rects: ok\n");
  return 0;
}
