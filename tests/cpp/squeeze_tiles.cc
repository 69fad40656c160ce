// The C++ wrappers of the per-cell preview calls (include/jxl_hip.hpp: Context::unsqueeze_chain_preview_tiles,
// jxlh::squeeze_tile_kinds) on a chain and a sequence of masks read from a file -- a download, painted after every
// group -- the planes of every paint written back to a file: tests/test_gpu_squeeze_tiles_cpp.py compares them byte for
// byte with what the ctypes route gives.
//   squeeze_tiles IN OUT
// IN (int32 words): n_planes, n_levels, rct_op, rct_perm, nearest_even, base_w, base_h, n_paints; per level horizontal,
// out_w, out_h, tile_w, tile_h; the base planes; per level and plane the residual plane (tight rows); per paint and level
// the number of mask bytes (0: no mask) and the bytes, one per word.
// OUT: per paint the kinds of the last level's cells (one int32 each), then the output planes (tight rows).
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
  if (argc < 3) return std::fprintf(stderr, "usage: squeeze_tiles IN OUT\n"), 2;
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
  const int n_planes = in[0], n_levels = in[1], rct_op = in[2], rct_perm = in[3], nearest_even = in[4];
  const uint32_t base_w = (uint32_t)in[5], base_h = (uint32_t)in[6];
  const int n_paints = in[7];
  size_t at = 8 + 5 * (size_t)n_levels;
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
    std::vector<jxlh_squeeze_tiles> tiles((size_t)n_levels);
    for (int i = 0; i < n_levels; i++) {
      const int32_t* w5 = &in[8 + 5 * (size_t)i];
      jxlh_squeeze_level& lv = levels[(size_t)i];
      lv = jxlh_squeeze_level{};
      lv.horizontal = w5[0];
      lv.out_w = (uint32_t)w5[1];
      lv.out_h = (uint32_t)w5[2];
      tiles[(size_t)i] = jxlh_squeeze_tiles{(uint32_t)w5[3], (uint32_t)w5[4], nullptr};
      const uint32_t rw = lv.horizontal ? lv.out_w / 2 : lv.out_w, rh = lv.horizontal ? lv.out_h : lv.out_h / 2;
      lv.res_stride = rw ? rw : 1;
      for (int p = 0; p < n_planes; p++) {
        lv.res[p] = upload(&in[at], (size_t)rw * rh);
        owned.push_back((void*)lv.res[p]);
        at += (size_t)rw * rh;
      }
    }
    const uint32_t w = levels.back().out_w, h = levels.back().out_h;
    std::vector<int32_t*> out;
    for (int p = 0; p < n_planes; p++) {
      out.push_back(upload(nullptr, (size_t)w * h));
      owned.push_back(out.back());
    }
    for (void* p : owned)
      if (!p) return std::fprintf(stderr, "device allocation failed\n"), 3;
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return std::fprintf(stderr, "cannot write %s\n", argv[2]), 2;
    std::vector<int32_t> plane((size_t)w * h);
    for (int paint = 0; paint < n_paints; paint++) {
      std::vector<std::vector<uint8_t>> masks((size_t)n_levels);
      for (int i = 0; i < n_levels; i++) {
        if (at >= in.size()) return std::fprintf(stderr, "input ends inside paint %d\n", paint), 2;
        const size_t n = (size_t)in[at++];
        if (at + n > in.size()) return std::fprintf(stderr, "input ends inside paint %d\n", paint), 2;
        for (size_t k = 0; k < n; k++) masks[(size_t)i].push_back((uint8_t)in[at++]);
        tiles[(size_t)i].present = n ? masks[(size_t)i].data() : nullptr;
      }
      const std::vector<uint8_t> kinds = jxlh::squeeze_tile_kinds(n_planes, levels, tiles, base_w, base_h, n_levels - 1);
      // (the masks are copied by the call: they go out of scope while the work may still be queued)
      ctx.unsqueeze_chain_preview_tiles(levels, tiles, base, base_w, base_w, base_h, out, w, rct_op, rct_perm, nearest_even != 0);
      std::vector<int32_t> words(kinds.begin(), kinds.end());
      std::fwrite(words.data(), 4, words.size(), f);
      ctx.sync();
      for (int p = 0; p < n_planes; p++) {
        if (hipMemcpy(plane.data(), out[(size_t)p], plane.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return 3;
        std::fwrite(plane.data(), 4, plane.size(), f);
      }
    }
    std::fclose(f);
    if (at != in.size()) return std::fprintf(stderr, "input has %zu words, %zu read\n", in.size(), at), 2;
    // an error surfaces as the wrapper's exception with the status in it
    bool threw = false;
    try {
      std::vector<jxlh_squeeze_tiles> bad = tiles;
      bad.back() = jxlh_squeeze_tiles{8, 0, nullptr};
      ctx.unsqueeze_chain_preview_tiles(levels, bad, base, base_w, base_w, base_h, out, w, rct_op, rct_perm);
    } catch (const jxlh::Error& e) {
      threw = e.status == JXLH_ERR_INVALID_ARGUMENT;
    }
    if (!threw) return std::fprintf(stderr, "a grid with one zero side did not throw JXLH_ERR_INVALID_ARGUMENT\n"), 4;
    for (void* p : owned) (void)hipFree(p);
    std::printf("squeeze tiles: %d planes, %d levels, %d paints written; error path ok\n", n_planes, n_levels, n_paints);
  } catch (const jxlh::Error& e) {
    return std::fprintf(stderr, "%s\n", e.what()), 1;
  }
  return 0;
}
