// The rectangle-list blend (jxlh_frame_blend_rects, jxlh_stage_blend_rects) and jxlh_blend_image_rects, decided here and
// issued by abi_blend.hip / k_blend_rects.hip: validation and clipping of the list, the kernel's work list, and the
// mapping of rects of the frame's result to rects of the image.  Plain C++: host logic, tested without a device against
// a per-pixel transcription (tests/cpp/blend_rects_plan.cc).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/jxl_hip.h"
#include "save_rects_plan.h"

namespace jxlh {

// ---- the kernel's geometry (k_blend_rects.hip reads the same constants): the row form of save_rects_plan.h.  A
// workgroup takes kBlendRectRows image rows of a rect, one per wave, and kBlendRectPixels consecutive pixels of each,
// four per lane.  The pixel columns start at the rect's x0 rounded DOWN to a multiple of four, so that a lane's four
// pixels keep the 16-byte alignment the canvas and slot rows have.
constexpr uint32_t kBlendRectPixels = kRectRowPixels, kBlendRectRows = kRectRowsPerGroup;

// One rect of the work list as the kernel reads it (device memory, scalar loads): the clipped, non-empty rectangle of
// the image and `first`, the first of its workgroups (ascending over the list: a workgroup finds its rect by
// bisection), laid nbx per row of pieces.
struct BlendRectWork {
  uint32_t x0, y0, w, h;
  uint32_t first, nbx;
};

struct BlendRectsPlan {
  jxlh_status status = JXLH_OK;
  std::vector<BlendRectWork> work;  // one per non-empty rect, in list order
  uint32_t groups = 0;              // workgroups of the one launch (0: nothing to do)
};

// the list's own checks, against an image_w x image_h canvas: those of the rect-list save
inline jxlh_status check_blend_rects(const jxlh_rect* rects, uint32_t n, uint32_t image_w, uint32_t image_h) {
  return check_save_rects(rects, n, image_w, image_h);
}

// The plan of one call (the list has passed check_blend_rects).  JXLH_ERR_UNSUPPORTED: 2^31 workgroups or more.
inline BlendRectsPlan plan_blend_rects(const jxlh_rect* rects, uint32_t n, uint32_t image_w, uint32_t image_h) {
  BlendRectsPlan p;
  uint64_t groups = 0;
  for (uint32_t i = 0; i < n; i++) {
    const jxlh_rect& r = rects[i];
    if (r.w == 0 || r.h == 0) continue;
    BlendRectWork k{};
    k.x0 = r.x0;
    k.y0 = r.y0;
    k.w = (uint32_t)std::min<uint64_t>(r.w, image_w - r.x0);  // cut at the right and bottom edge
    k.h = (uint32_t)std::min<uint64_t>(r.h, image_h - r.y0);
    const uint64_t xa = k.x0 & ~3u;
    const uint64_t nbx = ((uint64_t)k.x0 + k.w - xa + kBlendRectPixels - 1) / kBlendRectPixels;
    const uint64_t nby = ((uint64_t)k.h + kBlendRectRows - 1) / kBlendRectRows;
    if (groups + nbx * nby >= (1ull << 31)) {
      p = BlendRectsPlan{};
      p.status = JXLH_ERR_UNSUPPORTED;
      return p;
    }
    k.first = (uint32_t)groups;
    k.nbx = (uint32_t)nbx;
    groups += nbx * nby;
    p.work.push_back(k);
  }
  p.groups = (uint32_t)groups;
  return p;
}

// the frame's origin as the blend takes it: an origin beyond +-2^30 leaves the frame wholly outside the image, and so
// does the clamped one (fill_desc, abi_blend.hip)
inline int32_t blend_clamp_origin(int32_t v) { return std::min(std::max(v, -(1 << 30)), 1 << 30); }

// ---- jxlh_blend_image_rects: rects of a frame_w x frame_h result at origin (x0, y0) as rects of the image_w x image_h
// image.  Each rect is cut at the frame, shifted by the clamped origin (64-bit arithmetic) and intersected with the
// image; what becomes empty is dropped, the order of the others is kept.
inline void map_blend_image_rects(int32_t x0, int32_t y0, uint32_t image_w, uint32_t image_h, uint32_t frame_w,
                                  uint32_t frame_h, const jxlh_rect* rects, uint32_t n, std::vector<jxlh_rect>& out) {
  out.clear();
  const int64_t ox = blend_clamp_origin(x0), oy = blend_clamp_origin(y0);
  for (uint32_t i = 0; i < n; i++) {
    const jxlh_rect& r = rects[i];
    const int64_t fx0 = r.x0, fy0 = r.y0;
    const int64_t fx1 = std::min<int64_t>(fx0 + (int64_t)r.w, frame_w), fy1 = std::min<int64_t>(fy0 + (int64_t)r.h, frame_h);
    const int64_t ix0 = std::max<int64_t>(fx0 + ox, 0), iy0 = std::max<int64_t>(fy0 + oy, 0);
    const int64_t ix1 = std::min<int64_t>(fx1 + ox, image_w), iy1 = std::min<int64_t>(fy1 + oy, image_h);
    if (fx1 <= fx0 || fy1 <= fy0 || ix1 <= ix0 || iy1 <= iy0) continue;
    out.push_back(jxlh_rect{(uint32_t)ix0, (uint32_t)iy0, (uint32_t)(ix1 - ix0), (uint32_t)(iy1 - iy0)});
  }
}

}  // namespace jxlh
