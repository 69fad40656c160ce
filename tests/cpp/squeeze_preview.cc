// The C++ wrappers of the preview calls (include/jxl_hip.hpp: Context::unsqueeze_chain_preview,
// jxlh::squeeze_preview_kinds) on a chain read from a file, the planes written back to a file:
// tests/test_gpu_squeeze_preview_cpp.py compares them byte for byte with what the ctypes route gives.
//   squeeze_preview IN OUT
// IN (int32 words): n_planes, n_levels, n_missing (a suffix), rct_op, rct_perm, nearest_even, base_w, base_h; per level
// horizontal, out_w, out_h; the base planes; per level and plane the residual plane (tight rows).
// OUT: kinds and live (one int32 per level each), then the output planes (tight rows).
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <vector>

#include "jxl_hip.hpp"

namespace {
int32_t* upload(const int32_t* src, size_t n) {
  int32_t* d = nullptr;
  if (hipMalloc((void**)&d, (n ? n : 1) * 4) != hipSuccess) return nullptr;
  if (n && src && hipMemcpy(d, src, n * 4, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
  return d;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return std::fprintf(stderr, "usage: squeeze_preview IN OUT\n"), 2;
  std::vector<int32_t> in;
  {
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return std::fprintf(stderr, "cannot read %s\n", argv[1]), 2;
    std::fseek(f, 0, SEEK_END);
    in.resize((size_t)std::ftell(f) / 4);
    std::fseek(f, 0, SEEK_SET);
    if (std::fread(in.data(), 4, in.size(), f) != in.size()) return std::fprintf(stderr, "short read\n"), 2;
    std::fclose(f);
  }
  const int n_planes = in[0], n_levels = in[1], n_missing = in[2], rct_op = in[3], rct_perm = in[4], nearest_even = in[5];
  const uint32_t base_w = (uint32_t)in[6], base_h = (uint32_t)in[7];
  size_t at = 8 + 3 * (size_t)n_levels;
  std::vector<void*> owned;
  try {
    jxlh::Context ctx(0);
    std::vector<const int32_t*> base;
    for (int p = 0; p < n_planes; p++) {
      base.push_back(upload(&in[at], (size_t)base_w * base_h));
      owned.push_back((void*)base.back());
      at += (size_t)base_w * base_h;
    }
    std::vector<jxlh_squeeze_level> levels((size_t)n_levels);
    for (int i = 0; i < n_levels; i++) {
      jxlh_squeeze_level& lv = levels[(size_t)i];
      lv = jxlh_squeeze_level{};
      lv.horizontal = in[8 + 3 * (size_t)i];
      lv.out_w = (uint32_t)in[9 + 3 * (size_t)i];
      lv.out_h = (uint32_t)in[10 + 3 * (size_t)i];
      const uint32_t rw = lv.horizontal ? lv.out_w / 2 : lv.out_w, rh = lv.horizontal ? lv.out_h : lv.out_h / 2;
      lv.res_stride = rw ? rw : 1;
      for (int p = 0; p < n_planes; p++) {
        if (i < n_levels - n_missing) {
          lv.res[p] = upload(&in[at], (size_t)rw * rh);
          owned.push_back((void*)lv.res[p]);
        }
        at += (size_t)rw * rh;
      }
    }
    if (at != in.size()) return std::fprintf(stderr, "input has %zu words, %zu expected\n", in.size(), at), 2;
    const uint32_t w = levels.back().out_w, h = levels.back().out_h;
    std::vector<int32_t*> out;
    for (int p = 0; p < n_planes; p++) {
      out.push_back(upload(nullptr, (size_t)w * h));
      owned.push_back(out.back());
    }
    for (void* p : owned)
      if (!p) return std::fprintf(stderr, "device allocation failed\n"), 3;
    const jxlh::SqueezePreviewKinds k = jxlh::squeeze_preview_kinds(n_planes, levels, base_w, base_h);
    ctx.unsqueeze_chain_preview(levels, base, base_w, base_w, base_h, out, w, rct_op, rct_perm, nearest_even != 0);
    ctx.sync();
    // an error surfaces as the wrapper's exception with the status in it
    bool threw = false;
    try {
      std::vector<jxlh_squeeze_level> bad = levels;
      bad.back().out_w += 2;
      ctx.unsqueeze_chain_preview(bad, base, base_w, base_w, base_h, out, w + 2, rct_op, rct_perm);
    } catch (const jxlh::Error& e) {
      threw = e.status == JXLH_ERR_INVALID_ARGUMENT;
    }
    if (!threw) return std::fprintf(stderr, "a wrong geometry did not throw JXLH_ERR_INVALID_ARGUMENT\n"), 4;
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return std::fprintf(stderr, "cannot write %s\n", argv[2]), 2;
    std::vector<int32_t> words;
    for (uint8_t v : k.kinds) words.push_back(v);
    for (uint8_t v : k.live) words.push_back(v);
    std::fwrite(words.data(), 4, words.size(), f);
    std::vector<int32_t> plane((size_t)w * h);
    for (int p = 0; p < n_planes; p++) {
      if (hipMemcpy(plane.data(), out[(size_t)p], plane.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return 3;
      std::fwrite(plane.data(), 4, plane.size(), f);
    }
    std::fclose(f);
    for (void* p : owned) (void)hipFree(p);
    std::printf("squeeze preview: %d planes, %d levels, %d missing written; error path ok\n", n_planes, n_levels, n_missing);
  } catch (const jxlh::Error& e) {
    return std::fprintf(stderr, "%s\n", e.what()), 1;
  }
  return 0;
}
