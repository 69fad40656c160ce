// The rectangle-list save (jxlh_frame_save_rects, jxlh_stage_save_rects) and jxlh_changed_rects, decided here and
// issued by abi_save.hip / k_save.hip: validation and clipping of the list, the kernels' work list, every rect's
// rectangle in the oriented image, and the staging layout of a host destination.  Plain C++: host logic, tested
// without a device against a per-pixel transcription (tests/cpp/save_rects_plan.cc).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/jxl_hip.h"
#include "run_plan.h"

namespace jxlh {

// ---- the kernels' geometry (k_save.hip reads the same constants)
// row form (orientations 1-4): a workgroup takes kRectRowsPerGroup source rows of a rect, one per wave, and
// kRectRowPixels consecutive pixels of each, four per lane.  The pixel columns start at the rect's x0 rounded DOWN to a
// multiple of four, so that a lane's four pixels keep the 16-byte alignment the planes' rows have.
constexpr uint32_t kRectRowPixels = 256, kRectRowsPerGroup = 4;
// tile form (orientations 5-8): k_save_tiles' tile, laid from the rect's own corner
constexpr uint32_t kRectTileCols = 64;
constexpr uint32_t rect_tile_rows(uint32_t pixel_bytes) { return pixel_bytes > 8 ? 32 : 64; }

// One rect of the work list as the kernels read it (device memory, scalar loads): the clipped, non-empty source
// rectangle; `first`, the first of its workgroups (ascending over the list: a workgroup finds its rect by bisection),
// laid nbx per row of pieces; and where ITS destination has the oriented image's pixel (0, 0) and how far apart its
// rows are -- the caller's image for a device destination, the rect's own packed staging block for a host one.
struct SaveRectWork {
  uint32_t x0, y0, w, h;
  uint32_t first, nbx;
  int64_t origin;  // bytes from SaveLaunch::out; negative for a staged rect (never dereferenced outside the block)
  uint64_t pitch;  // bytes
};

// ... and what the host does with it afterwards: the rect's rectangle in the oriented image, and for a host
// destination its block in the staging buffer (offset, dword-rounded pitch) and the pixel bytes of one of its rows
struct SaveRectOut {
  uint64_t ox0, oy0, ow, oh;
  uint64_t stage_off, stage_pitch, row_bytes;
};

struct SaveRectsPlan {
  jxlh_status status = JXLH_OK;
  std::vector<SaveRectWork> work;  // one per non-empty rect, in list order
  std::vector<SaveRectOut> out;    // parallel to `work`
  uint32_t groups = 0;             // workgroups of the one launch (0: nothing to do)
  uint64_t staging_bytes = 0;      // of ctx->rgb8 (staged only)
};

// the list's own checks, against a w x h result
inline jxlh_status check_save_rects(const jxlh_rect* rects, uint32_t n, uint32_t w, uint32_t h) {
  if (n > JXLH_MAX_SAVE_RECTS || (n && !rects)) return JXLH_ERR_INVALID_ARGUMENT;
  for (uint32_t i = 0; i < n; i++) {
    const jxlh_rect& r = rects[i];
    if (r.w == 0 || r.h == 0) continue;
    if (r.x0 >= w || r.y0 >= h) return JXLH_ERR_INVALID_ARGUMENT;
    if ((uint64_t)r.x0 + r.w > 0xffffffffull || (uint64_t)r.y0 + r.h > 0xffffffffull) return JXLH_ERR_INVALID_ARGUMENT;
  }
  return JXLH_OK;
}

// the source rectangle (x0, y0, w, h) of a W x H result in the image of `orientation` (display_pixel of its corners)
inline void orient_rect(uint32_t orientation, uint64_t W, uint64_t H, uint64_t x0, uint64_t y0, uint64_t w, uint64_t h,
                        SaveRectOut& o) {
  const bool transpose = orientation >= 5;
  const bool flip_x = orientation == 2 || orientation == 3 || orientation == 6 || orientation == 7;
  const bool flip_y = orientation == 3 || orientation == 4 || orientation == 7 || orientation == 8;
  const uint64_t OW = transpose ? H : W, OH = transpose ? W : H;
  const uint64_t ax = transpose ? y0 : x0, ay = transpose ? x0 : y0;
  o.ow = transpose ? h : w;
  o.oh = transpose ? w : h;
  o.ox0 = flip_x ? OW - ax - o.ow : ax;
  o.oy0 = flip_y ? OH - ay - o.oh : ay;
}

// The plan of one call (the list has passed check_save_rects): rects of a w x h result under `orientation`, pixels of
// pixel_bytes; staged: the destination is host memory (each rect's pixels go to its own block of the staging buffer),
// else device memory of rows bytes_per_row apart.  JXLH_ERR_UNSUPPORTED: 2^31 workgroups or more.
inline SaveRectsPlan plan_save_rects(const jxlh_rect* rects, uint32_t n, uint32_t w, uint32_t h, uint32_t orientation,
                                     uint32_t pixel_bytes, bool staged, uint64_t bytes_per_row) {
  SaveRectsPlan p;
  const bool tiles = orientation >= 5;
  uint64_t groups = 0, stage = 0;
  for (uint32_t i = 0; i < n; i++) {
    const jxlh_rect& r = rects[i];
    if (r.w == 0 || r.h == 0) continue;
    SaveRectWork k{};
    k.x0 = r.x0;
    k.y0 = r.y0;
    k.w = (uint32_t)std::min<uint64_t>(r.w, w - r.x0);  // cut at the right and bottom edge
    k.h = (uint32_t)std::min<uint64_t>(r.h, h - r.y0);
    uint64_t nbx, nby;
    if (tiles) {
      const uint32_t th = rect_tile_rows(pixel_bytes);
      nbx = ((uint64_t)k.w + kRectTileCols - 1) / kRectTileCols;
      nby = ((uint64_t)k.h + th - 1) / th;
    } else {
      const uint64_t xa = k.x0 & ~3u;
      nbx = ((uint64_t)k.x0 + k.w - xa + kRectRowPixels - 1) / kRectRowPixels;
      nby = ((uint64_t)k.h + kRectRowsPerGroup - 1) / kRectRowsPerGroup;
    }
    if (groups + nbx * nby >= (1ull << 31)) {
      p = SaveRectsPlan{};
      p.status = JXLH_ERR_UNSUPPORTED;
      return p;
    }
    k.first = (uint32_t)groups;
    k.nbx = (uint32_t)nbx;
    groups += nbx * nby;
    SaveRectOut o{};
    orient_rect(orientation, w, h, k.x0, k.y0, k.w, k.h, o);
    o.row_bytes = o.ow * pixel_bytes;
    if (staged) {
      o.stage_off = stage;
      o.stage_pitch = (o.row_bytes + 3) / 4 * 4;
      stage += o.stage_pitch * o.oh;
      k.pitch = o.stage_pitch;
      k.origin = (int64_t)o.stage_off - (int64_t)(o.oy0 * o.stage_pitch) - (int64_t)(o.ox0 * pixel_bytes);
    } else {
      k.pitch = bytes_per_row;
      k.origin = 0;
    }
    p.work.push_back(k);
    p.out.push_back(o);
  }
  p.groups = (uint32_t)groups;
  p.staging_bytes = stage;
  return p;
}

// ---- jxlh_changed_rects
// How far beyond a re-rendered group a pixel of the result can change: the stage list's reach (Gaborish 1, EPF0 3,
// EPF1 2, EPF2 1: StageList::halo_px), and on an axis on which a channel is sub-sampled one pixel more -- the chroma
// upsampling in front of the filters reads one sub-sampled neighbour.  Patches, splines and noise act per pixel.
struct ChangedReach { uint32_t x, y; };
inline ChangedReach changed_reach(const jxlh_frame_params& p) {
  StageList s;
  s.gab = p.gab != 0;
  s.epf_iters = (int)p.epf_iters;
  uint32_t hs = 0, vs = 0;
  for (int c = 0; c < 3; c++) hs |= p.hshift[c], vs |= p.vshift[c];
  const uint32_t halo = (uint32_t)s.halo_px();
  return {halo + (hs ? 1u : 0u), halo + (vs ? 1u : 0u)};
}

// The rects (ascending group order; one per maximal run of horizontally neighbouring listed groups of a group row)
// into `rects`; returns the status jxlh_changed_rects returns apart from the cap protocol.
inline jxlh_status plan_changed_rects(const jxlh_frame_params& p, const uint32_t* group_ids, uint32_t count,
                                      std::vector<jxlh_rect>& rects) {
  rects.clear();
  if (p.abi_version != JXLH_ABI_VERSION) return JXLH_ERR_INVALID_ARGUMENT;
  if (p.xsize == 0 || p.ysize == 0 || p.xsize > (1u << 20) || p.ysize > (1u << 20) || p.epf_iters > 3)
    return JXLH_ERR_INVALID_ARGUMENT;
  for (int c = 0; c < 3; c++)
    if (p.hshift[c] > 1 || p.vshift[c] > 1) return JXLH_ERR_INVALID_ARGUMENT;
  if (p.upsampling > 1 || (p.flags & JXLH_FRAME_MODULAR)) return JXLH_ERR_UNSUPPORTED;
  const uint32_t xg = (p.xsize + 255) / 256, yg = (p.ysize + 255) / 256;
  for (uint32_t i = 0; i < count; i++)
    if (group_ids[i] >= (uint64_t)xg * yg) return JXLH_ERR_INVALID_ARGUMENT;
  std::vector<uint32_t> ids(group_ids, group_ids + count);
  std::sort(ids.begin(), ids.end());
  ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
  const ChangedReach reach = changed_reach(p);
  for (size_t i = 0; i < ids.size();) {
    size_t j = i + 1;
    while (j < ids.size() && ids[j] == ids[j - 1] + 1 && ids[j] / xg == ids[i] / xg) j++;
    const uint32_t gy = ids[i] / xg, gx0 = ids[i] % xg, gx1 = ids[j - 1] % xg + 1;
    const uint32_t x_lo = gx0 * 256 > reach.x ? gx0 * 256 - reach.x : 0, x_hi = std::min(p.xsize, gx1 * 256 + reach.x);
    const uint32_t y_lo = gy * 256 > reach.y ? gy * 256 - reach.y : 0, y_hi = std::min(p.ysize, (gy + 1) * 256 + reach.y);
    rects.push_back(jxlh_rect{x_lo, y_lo, x_hi - x_lo, y_hi - y_lo});
    i = j;
  }
  return JXLH_OK;
}

}  // namespace jxlh
