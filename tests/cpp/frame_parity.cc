// Compiled-language parity test of the drop-in boundary: a VarDCT frame goes through the C++ host side
// (include/jxl_hip.hpp over the C ABI of libjxl_hip.so) and through the CPU oracle (oracle/libjxlo_fused.so, test
// infrastructure), and the reconstructed planes must be equal bit for bit.  No Python, no torch: what a maintainer's
// compiled shim would link.  Built and run by tests/test_cpp_host.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jxl_hip.hpp"
#include "synth_frame.hpp"

int main(int argc, char** argv) {
  const int w = argc > 1 ? atoi(argv[1]) : 300, h = argc > 2 ? atoi(argv[2]) : 270;
  const int epf_iters = argc > 3 ? atoi(argv[3]) : 2;
  // "rects": LF and HfMetadata arrive one rect at a time (below) instead of as two whole-frame calls
  const bool per_rect = argc > 4 && strcmp(argv[4], "rects") == 0;
  synth::Frame F;
  if (!synth::make(w, h, epf_iters, &F)) return 2;
  const int xb = F.xb, yb = F.yb, cw = F.cw, ngroups = F.ngroups;
  const size_t stride = F.stride;
  auto &tables = F.tables;
  auto &qy = F.qy, &qx = F.qx, &qb = F.qb, &rq = F.rq, &coeffs = F.coeffs;
  auto &tmap = F.tmap, &epf = F.epf;
  auto &ytox = F.ytox, &ytob = F.ytob;
  std::vector<float>* pl = F.pl;

  // ---- device, through the C++ host side
  try {
    jxlh::Context ctx(0, 2);
    jxlh_frame_params p = jxlh::VarDctFrame::default_params((uint32_t)w, (uint32_t)h);
    p.epf_iters = (uint32_t)epf_iters;
    jxlh::VarDctFrame frame(ctx, p);
    frame.decode_hf_global(tables);
    if (!per_rect) {
      frame.decode_lf_group(0, 0, (uint32_t)xb, (uint32_t)yb, qy.data(), qx.data(), qb.data(), (size_t)xb);
      frame.decode_hf_metadata(0, 0, (uint32_t)xb, (uint32_t)yb, tmap.data(), rq.data(), epf.data(), (size_t)xb,
                               ytox.data(), ytob.data(), (size_t)cw);
    } else {
      // The way a decoder calls the setters: one rect per call, each in a buffer of its own whose rows are longer than
      // the rect (the padding holds values that would show), the quantised LF scaled by 1 << extra_precision.  The
      // maps go first and bottom-up, the LF rects start at odd blocks and change size from call to call.
      const int pad = 5;
      const int ch = (yb + 7) / 8;
      for (int y0 = (yb - 1) / 24 * 24; y0 >= 0; y0 -= 24)
        for (int x0 = 0; x0 < xb; x0 += 16) {
          const int rw = std::min(16, xb - x0), rh = std::min(24, yb - y0), ms = rw + pad;
          const int tw = (rw + 7) / 8, th = (rh + 7) / 8, cs = tw + pad;
          std::vector<uint8_t> t((size_t)ms * rh, 0xff), e((size_t)ms * rh, 0xff);
          std::vector<int32_t> q((size_t)ms * rh, 0x7fffffff);
          std::vector<int8_t> cx((size_t)cs * th, 0x7f), cb((size_t)cs * th, 0x7f);
          for (int y = 0; y < rh; y++)
            for (int x = 0; x < rw; x++) {
              const size_t src = (size_t)(y0 + y) * xb + x0 + x, dst = (size_t)y * ms + x;
              t[dst] = tmap[src], e[dst] = epf[src], q[dst] = rq[src];
            }
          for (int y = 0; y < th; y++)
            for (int x = 0; x < tw; x++) {
              const size_t src = (size_t)(y0 / 8 + y) * cw + x0 / 8 + x, dst = (size_t)y * cs + x;
              cx[dst] = ytox[src], cb[dst] = ytob[src];
            }
          if (y0 / 8 + th > ch) return 2;
          frame.decode_hf_metadata((uint32_t)x0, (uint32_t)y0, (uint32_t)rw, (uint32_t)rh, t.data(), q.data(), e.data(),
                                   (size_t)ms, cx.data(), cb.data(), (size_t)cs);
        }
      int call = 0;
      for (int y0 = 0; y0 < yb;) {
        const int rh = std::min(yb - y0, 3 + 7 * (call % 3));
        for (int x0 = 0; x0 < xb; call++) {
          const int rw = std::min(xb - x0, 1 + 10 * (call % 4)), ls = rw + pad;
          const uint32_t ep = (uint32_t)(1 + call % 3);
          std::vector<int32_t> l[3];
          const std::vector<int32_t>* from[3] = {&qy, &qx, &qb};
          for (int c = 0; c < 3; c++) {
            l[c].assign((size_t)ls * rh, 0x7fffffff);
            for (int y = 0; y < rh; y++)
              for (int x = 0; x < rw; x++)
                l[c][(size_t)y * ls + x] = (*from[c])[(size_t)(y0 + y) * xb + x0 + x] * (int32_t)(1u << ep);
          }
          frame.decode_lf_group((uint32_t)x0, (uint32_t)y0, (uint32_t)rw, (uint32_t)rh, l[0].data(), l[1].data(),
                                l[2].data(), (size_t)ls, ep);
          x0 += rw;
        }
        y0 += rh;
      }
    }
    for (int g = 0; g < ngroups; g++) frame.decode_vardct_group((uint32_t)g, &coeffs[(size_t)g * 3 * 65536], g % 2);
    frame.slot_wait(0);
    frame.slot_wait(1);
    frame.finalize_and_render();
    ctx.sync();
    std::vector<float> out[3];
    for (auto& o : out) o.resize((size_t)w * h);
    frame.read_planes(out[0].data(), out[1].data(), out[2].data());
    size_t bad = 0;
    for (int c = 0; c < 3; c++)
      for (int y = 0; y < h; y++)
        if (memcmp(&out[c][(size_t)y * w], &pl[c][(size_t)y * stride], sizeof(float) * w) != 0) bad++;
    // an invalid call must come back as an exception carrying the status
    bool threw = false;
    try {
      frame.decode_vardct_group((uint32_t)ngroups + 5, coeffs.data());
    } catch (const jxlh::Error& e) {
      threw = e.status == JXLH_ERR_INVALID_ARGUMENT;
    }
    printf("%dx%d epf_iters=%d groups=%d%s: %zu differing rows, error path %s\n", w, h, epf_iters, ngroups,
           per_rect ? " per rect" : "", bad, threw ? "ok" : "MISSING");
    return (bad == 0 && threw) ? 0 : 1;
  } catch (const std::exception& e) {
    fprintf(stderr, "device path failed: %s\n", e.what());
    return 3;
  }
}
