// jxlh_frame_repaint_groups through the C++ layer, byte for byte against the C calls and bit-exact against the oracle.
//   VarDCT, upsampling N: pass 1 renders the frame with some groups' coefficients zeroed; they arrive,
//     VarDctFrame::repaint_groups repaints them.  The planes must be the oracle's frame through jxlo_upsample, the planes
//     the same sequence gives through jxlh_frame_repaint_groups itself on a second context, and a third context's whole run.
//   Modular (through build_modular_frame): a whole render of 8-bit samples, two cells replaced through set_channels,
//     GpuModularFramePipeline::repaint_groups; against jxlo_modular_to_f32, the C call and a whole run.
//   The rect lists of VarDctFrame::repaint_changed_rects, jxlh::repaint_changed_rects and the C call are equal.
//   repaint W H ITERS N
#include <cstdio>
#include <cstring>
#include <vector>

#include "jxl_hip_pipeline.hpp"
#include "synth_frame.hpp"

using namespace jxlh;

namespace {

struct Planes {
  std::vector<float> c[3];
  void read(VarDctFrame& f) {
    const size_t n = (size_t)f.out_width() * f.out_height();
    for (auto& v : c) v.assign(n, -1.0f);
    f.read_planes(c[0].data(), c[1].data(), c[2].data());
  }
  size_t differing(const Planes& o) const {
    size_t bad = 0;
    for (int k = 0; k < 3; k++) bad += c[k].size() != o.c[k].size() || memcmp(c[k].data(), o.c[k].data(), c[k].size() * 4) != 0;
    return bad;
  }
};

void upsampled(int n, const float* in, int w, int h, size_t stride, std::vector<float>& out) {
  out.assign((size_t)w * n * h * n, 0.0f);
  jxlo_upsample(n, nullptr, in, w, h, stride, out.data(), (size_t)w * n);
}

void load(VarDctFrame& frame, const synth::Frame& F) {
  frame.decode_hf_global(F.tables);
  frame.decode_lf_group(0, 0, (uint32_t)F.xb, (uint32_t)F.yb, F.qy.data(), F.qx.data(), F.qb.data(), (size_t)F.xb);
  frame.decode_hf_metadata(0, 0, (uint32_t)F.xb, (uint32_t)F.yb, F.tmap.data(), F.rq.data(), F.epf.data(), (size_t)F.xb,
                           F.ytox.data(), F.ytob.data(), (size_t)F.cw);
}

}  // namespace

int main(int argc, char** argv) {
  const int w = argc > 1 ? atoi(argv[1]) : 300, h = argc > 2 ? atoi(argv[2]) : 600, epf_iters = argc > 3 ? atoi(argv[3]) : 2;
  const int n = argc > 4 ? atoi(argv[4]) : 2;
  synth::Frame F;
  if (!synth::make(w, h, epf_iters, &F)) return 2;
  try {
    // ---------------------------------------------------------------- VarDCT
    jxlh_frame_params p = VarDctFrame::default_params((uint32_t)w, (uint32_t)h);
    p.epf_iters = (uint32_t)epf_iters;
    p.upsampling = (uint32_t)n;
    std::vector<uint32_t> later = {0u, (uint32_t)F.ngroups - 1};
    if (F.ngroups >= 6) later.push_back((uint32_t)F.ngroups / 2);
    auto is_later = [&](int g) {
      for (uint32_t l : later)
        if ((int)l == g) return true;
      return false;
    };
    const size_t slab = (size_t)3 * 65536;
    std::vector<int32_t> zeros(slab, 0);
    Planes want, first, cpp, c_abi, whole;
    for (int c = 0; c < 3; c++) upsampled(n, F.pl[c].data(), w, h, F.stride, want.c[c]);
    Context ctx(0, 1), ctx2(0, 1), ctx3(0, 1);
    std::vector<jxlh_rect> rects_frame;
    for (int route = 0; route < 3; route++) {  // the C++ method; the C call; a whole run of the final inputs
      VarDctFrame frame(route == 0 ? ctx : route == 1 ? ctx2 : ctx3, p);
      load(frame, F);
      for (int g = 0; g < F.ngroups; g++)
        frame.decode_vardct_group((uint32_t)g, route < 2 && is_later(g) ? zeros.data() : &F.coeffs[(size_t)g * slab]);
      frame.slot_wait();
      frame.finalize_and_render();
      if (route == 2) {
        whole.read(frame);
        continue;
      }
      if (route == 0) first.read(frame);
      for (uint32_t g : later) frame.decode_vardct_group(g, &F.coeffs[(size_t)g * slab]);
      frame.slot_wait();
      if (route == 0) {
        frame.repaint_groups(later);
        rects_frame = frame.repaint_changed_rects(later);
        cpp.read(frame);
      } else {
        ctx2.check(jxlh_frame_repaint_groups(ctx2.raw(), later.data(), (uint32_t)later.size()), "jxlh_frame_repaint_groups");
        c_abi.read(frame);
      }
    }
    const std::vector<jxlh_rect> rects_free = repaint_changed_rects(p, later);
    uint32_t nr = 0;
    std::vector<jxlh_rect> rects_c(rects_free.size() + 1);
    const jxlh_status st = jxlh_repaint_changed_rects(&p, later.data(), (uint32_t)later.size(), rects_c.data(), (uint32_t)rects_c.size(), &nr);
    const bool same_rects = st == JXLH_OK && nr == rects_free.size() && rects_frame.size() == nr && nr > 0 &&
                            !memcmp(rects_c.data(), rects_free.data(), nr * sizeof(jxlh_rect)) &&
                            !memcmp(rects_frame.data(), rects_free.data(), nr * sizeof(jxlh_rect));
    // every pixel that changed between the passes lies in a rect
    size_t outside = 0;
    const size_t ow = (size_t)w * n, oh = (size_t)h * n;
    std::vector<uint8_t> covered(ow * oh, 0);
    for (const jxlh_rect& r : rects_free)
      for (uint32_t y = r.y0; y < r.y0 + r.h; y++) memset(&covered[(size_t)y * ow + r.x0], 1, r.w);
    for (int c = 0; c < 3; c++)
      for (size_t i = 0; i < ow * oh; i++) outside += !covered[i] && memcmp(&first.c[c][i], &cpp.c[c][i], 4) != 0;
    const bool stale = first.differing(want) != 0;
    printf("vardct %dx%d epf_iters=%d x%d: repaint vs oracle: %zu differing planes, vs the C call: %zu, vs a whole run: %zu, "
           "first pass %s, rects %s, %zu changed pixels outside the rects\n",
           w, h, epf_iters, n, cpp.differing(want), cpp.differing(c_abi), cpp.differing(whole), stale ? "stale" : "ALREADY FINAL",
           same_rects ? "equal" : "DIFFER", outside);
    if (cpp.differing(want) || cpp.differing(c_abi) || cpp.differing(whole) || !stale || !same_rects || outside) return 1;

    // ---------------------------------------------------------------- Modular
    std::vector<int32_t> chan[3], other[3];
    synth::Rng rng{12345};
    for (int c = 0; c < 3; c++) {
      chan[c].resize((size_t)w * h);
      other[c].resize((size_t)w * h);
      for (size_t i = 0; i < chan[c].size(); i++) chan[c][i] = rng.range(0, 255), other[c][i] = rng.range(0, 255);
    }
    jxlh_frame_params base = VarDctFrame::default_params((uint32_t)w, (uint32_t)h);
    base.gab = 0;
    base.epf_iters = 0;
    const std::vector<uint32_t> cells = {0u, (uint32_t)F.ngroups - 1};
    Planes mcpp, mc, mwhole, mwant;
    for (int route = 0; route < 3; route++) {
      Context& cx = route == 0 ? ctx : route == 1 ? ctx2 : ctx3;
      auto pipe = RenderPipelineBuilder(3, {(size_t)w, (size_t)h}, 0, 8, base)
                      .add_inout_stage(ConvertModularToF32Stage{0, 8})
                      .add_inout_stage(ConvertModularToF32Stage{1, 8})
                      .add_inout_stage(ConvertModularToF32Stage{2, 8})
                      .add_save_stage({0, 1, 2}, 1, 0, ColorType::kRgb, DataFormat::f32(), false)
                      .build_modular_frame(cx);
      const int32_t* planes[3] = {chan[0].data(), chan[1].data(), chan[2].data()};
      std::vector<int32_t> fin[3] = {chan[0], chan[1], chan[2]};
      for (uint32_t g : cells) {
        const int x0 = (int)(g % (uint32_t)F.xg) * 256, y0 = (int)(g / (uint32_t)F.xg) * 256;
        for (int c = 0; c < 3; c++)
          for (int y = y0; y < std::min(h, y0 + 256); y++)
            for (int x = x0; x < std::min(w, x0 + 256); x++) fin[c][(size_t)y * w + x] = other[c][(size_t)y * w + x];
      }
      const int32_t* final_planes[3] = {fin[0].data(), fin[1].data(), fin[2].data()};
      pipe->set_channels(0, 0, (uint32_t)w, (uint32_t)h, route == 2 ? final_planes : planes, (size_t)w);
      pipe->render();
      if (route < 2) {
        for (uint32_t g : cells) {
          const uint32_t x0 = g % (uint32_t)F.xg * 256, y0 = g / (uint32_t)F.xg * 256;
          const uint32_t cw = std::min<uint32_t>(256, (uint32_t)w - x0), ch = std::min<uint32_t>(256, (uint32_t)h - y0);
          const int32_t* at[3];
          for (int c = 0; c < 3; c++) at[c] = fin[c].data() + (size_t)y0 * w + x0;
          pipe->set_channels(x0, y0, cw, ch, at, (size_t)w);
        }
        if (route == 0) pipe->repaint_groups(cells);
        else cx.check(jxlh_frame_repaint_groups(cx.raw(), cells.data(), (uint32_t)cells.size()), "jxlh_frame_repaint_groups");
      }
      (route == 0 ? mcpp : route == 1 ? mc : mwhole).read(pipe->frame());
      if (route == 0)
        for (int c = 0; c < 3; c++) {
          mwant.c[c].resize((size_t)w * h);
          jxlo_modular_to_f32(fin[c].data(), mwant.c[c].size(), 8, mwant.c[c].data());
        }
    }
    printf("modular %dx%d: repaint vs oracle: %zu differing planes, vs the C call: %zu, vs a whole run: %zu\n", w, h,
           mcpp.differing(mwant), mcpp.differing(mc), mcpp.differing(mwhole));
    if (mcpp.differing(mwant) || mcpp.differing(mc) || mcpp.differing(mwhole)) return 1;
  } catch (const Error& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  printf("repaint: ok\n");
  return 0;
}
