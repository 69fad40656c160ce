// Extra channels by rect (jxl_hip_extra_rects.h), decided here and issued by abi_extra_rects.hip / frame_run.hip /
// k_extra_rects.hip: a channel's tile grid and dirty bitmap, the item list of a run's finish launches, the argument
// checks and the scatter layout of jxlh_frame_set_extra_channel_rects, and the rule of
// jxlh_extra_channel_changed_rects.  Plain C++: no HIP, no context, no environment; tested without a device against a
// per-sample model (tests/cpp/ec_rects_plan.cc).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/jxl_hip.h"

namespace jxlh {

// ---- the kernels' geometry (k_extra_rects.hip reads the same constants)
// finish: a workgroup takes one tile of kEcTileW x kEcTileH SOURCE samples, laid from the channel's corner: one wave
// per kEcTileH / 4 rows, a lane per column.  A factor above 1 loads the tile with kEcHalo samples around it.
constexpr uint32_t kEcTileW = 64, kEcTileH = 16;
constexpr uint32_t kEcHalo = 2;  // Upsample<N>'s BORDER: the 5 x 5 window (upsample.rs)
// scatter: a workgroup takes a piece of kEcPieceW x kEcPieceH samples of a rect, laid from the rect's corner, four
// consecutive samples per lane
constexpr uint32_t kEcPieceW = 256, kEcPieceH = 16;

// How far a changed sample reaches in its channel: [x0, x0 + w) of a row (column) of `size` samples, widened by kEcHalo
// on both sides when the channel is upsampled, clipped.  x0 < size, w >= 1, x0 + w <= size.
struct EcSpan { uint32_t lo, hi; };  // [lo, hi)
inline EcSpan ec_reach(uint32_t x0, uint32_t w, uint32_t size, uint32_t up) {
  const uint32_t r = up > 1 ? kEcHalo : 0;
  return {x0 > r ? x0 - r : 0, (uint32_t)std::min<uint64_t>((uint64_t)x0 + w + r, size)};
}

// ---- jxlh_extra_channel_changed_rects
inline bool ec_factor_ok(uint32_t up) { return up == 1 || up == 2 || up == 4 || up == 8; }
// one rect (non-empty, inside the w x h channel) in the finished channel of min(w * up, res_w) x min(h * up, res_h)
inline jxlh_rect ec_changed_rect(uint32_t w, uint32_t h, uint32_t up, uint32_t res_w, uint32_t res_h, const jxlh_rect& r) {
  const uint64_t out_w = std::min<uint64_t>((uint64_t)w * up, res_w), out_h = std::min<uint64_t>((uint64_t)h * up, res_h);
  const EcSpan sx = ec_reach(r.x0, r.w, w, up), sy = ec_reach(r.y0, r.h, h, up);
  const uint64_t x_lo = (uint64_t)sx.lo * up, x_hi = std::min<uint64_t>((uint64_t)sx.hi * up, out_w);
  const uint64_t y_lo = (uint64_t)sy.lo * up, y_hi = std::min<uint64_t>((uint64_t)sy.hi * up, out_h);
  if (x_lo >= x_hi || y_lo >= y_hi) return jxlh_rect{0, 0, 0, 0};  // all of it is cut off
  return jxlh_rect{(uint32_t)x_lo, (uint32_t)y_lo, (uint32_t)(x_hi - x_lo), (uint32_t)(y_hi - y_lo)};
}
// the call apart from the cap protocol: `out` gets one rect per input rect
inline jxlh_status plan_ec_changed_rects(uint32_t w, uint32_t h, uint32_t up, uint32_t res_w, uint32_t res_h,
                                         const jxlh_rect* src, uint32_t n_src, std::vector<jxlh_rect>& out) {
  out.clear();
  if (w == 0 || h == 0 || res_w == 0 || res_h == 0 || !ec_factor_ok(up) || (n_src && !src)) return JXLH_ERR_INVALID_ARGUMENT;
  for (uint32_t i = 0; i < n_src; i++) {
    const jxlh_rect& r = src[i];
    if (r.w == 0 || r.h == 0) {
      out.push_back(jxlh_rect{0, 0, 0, 0});
      continue;
    }
    if ((uint64_t)r.x0 + r.w > w || (uint64_t)r.y0 + r.h > h) return JXLH_ERR_INVALID_ARGUMENT;
    out.push_back(ec_changed_rect(w, h, up, res_w, res_h, r));
  }
  return JXLH_OK;
}

// ---- a channel's tile grid and dirty bitmap
struct EcGrid {
  uint32_t w = 0, h = 0, up = 1;
  uint32_t ntx = 0, nty = 0;
  uint64_t n_dirty = 0;
  std::vector<uint64_t> bits;  // tile ty * ntx + tx

  bool active() const { return ntx != 0; }  // the channel has rect state
  void clear() { *this = EcGrid{}; }
  // a clean grid of a w x h channel (w, h >= 1) with factor up
  void reset(uint32_t w_, uint32_t h_, uint32_t up_) {
    w = w_, h = h_, up = up_;
    ntx = (w + kEcTileW - 1) / kEcTileW;
    nty = (h + kEcTileH - 1) / kEcTileH;
    n_dirty = 0;
    bits.assign(((uint64_t)ntx * nty + 63) / 64, 0);
  }
  bool test(uint64_t tile) const { return (bits[tile >> 6] >> (tile & 63)) & 1; }
  // every tile that holds a sample whose finished values the rect's samples reach (ec_reach) becomes dirty; the rect is
  // non-empty and inside the channel
  void mark(uint32_t x0, uint32_t y0, uint32_t rw, uint32_t rh) {
    const EcSpan sx = ec_reach(x0, rw, w, up), sy = ec_reach(y0, rh, h, up);
    const uint32_t tx0 = sx.lo / kEcTileW, tx1 = (sx.hi - 1) / kEcTileW, ty0 = sy.lo / kEcTileH, ty1 = (sy.hi - 1) / kEcTileH;
    for (uint32_t ty = ty0; ty <= ty1; ty++)
      for (uint32_t tx = tx0; tx <= tx1; tx++) {
        const uint64_t t = (uint64_t)ty * ntx + tx;
        const uint64_t m = 1ull << (t & 63);
        if (!(bits[t >> 6] & m)) {
          bits[t >> 6] |= m;
          n_dirty++;
        }
      }
  }
  void mark_all() { mark(0, 0, w, h); }
};

// one workgroup of a finish launch (device memory, scalar loads)
struct EcItem { uint32_t ec, tile; };

// The dirty tiles of all channels with rect state, as one item list grouped by factor: the items of factor 1 << k are
// [first[k], first[k + 1]), each dirty tile listed once, channels ascending, tiles ascending.  Every bitmap is clean
// afterwards.
struct EcRectsPlan {
  EcGrid ch[JXLH_MAX_EXTRA_CHANNELS];

  bool dirty(uint32_t ec) const { return ch[ec].n_dirty != 0; }
  void collect(std::vector<EcItem>& items, uint32_t (&first)[5]) {
    items.clear();
    for (uint32_t k = 0; k < 4; k++) {
      first[k] = (uint32_t)items.size();
      for (uint32_t ec = 0; ec < JXLH_MAX_EXTRA_CHANNELS; ec++) {
        EcGrid& g = ch[ec];
        if (!g.active() || g.up != (1u << k) || g.n_dirty == 0) continue;
        for (size_t wd = 0; wd < g.bits.size(); wd++) {
          uint64_t v = g.bits[wd];
          while (v) {
            const uint32_t b = (uint32_t)__builtin_ctzll(v);
            v &= v - 1;
            items.push_back(EcItem{ec, (uint32_t)(wd * 64 + b)});
          }
          g.bits[wd] = 0;
        }
        g.n_dirty = 0;
      }
    }
    first[4] = (uint32_t)items.size();
  }
};

// ---- jxlh_frame_set_extra_channel_rects: the argument checks
// what the checks depend on, read out of the context
struct EcCallState {
  bool in_frame = false, sharded = false;
  struct { bool set = false; uint32_t w = 0, h = 0; } ch[JXLH_MAX_EXTRA_CHANNELS];
};
// samples a rect names: [offset, offset + stride * (h - 1) + w); the extent fits 64 bits for any 32-bit stride, h, w
inline uint64_t ec_rect_extent(const jxlh_ec_rect& r) { return (uint64_t)r.stride * (r.h - 1) + r.w; }
// The status of the call; on a refusal that a rect caused *first_bad is its index and *why says what is wrong with it.
// JXLH_OK with n == 0 or only empty rects: nothing to do.
inline jxlh_status check_ec_rects(const EcCallState& s, bool have_samples, uint64_t n_samples, const jxlh_ec_rect* rects,
                                  uint32_t n, uint32_t* first_bad, std::string* why) {
  auto bad = [&](uint32_t i, jxlh_status st, const char* what) {
    if (first_bad) *first_bad = i;
    if (why) *why = "rect " + std::to_string(i) + ": " + what;
    return st;
  };
  if (n > JXLH_MAX_EC_RECTS || (n && (!rects || !have_samples))) return JXLH_ERR_INVALID_ARGUMENT;
  if (!s.in_frame) return JXLH_ERR_BAD_STATE;
  if (s.sharded) return JXLH_ERR_UNSUPPORTED;
  for (uint32_t i = 0; i < n; i++) {
    const jxlh_ec_rect& r = rects[i];
    if (r.ec >= JXLH_MAX_EXTRA_CHANNELS) return bad(i, JXLH_ERR_INVALID_ARGUMENT, "no such extra channel");
    if (r.w == 0 || r.h == 0) continue;
    if (!s.ch[r.ec].set) return bad(i, JXLH_ERR_BAD_STATE, "the channel is not set in this frame");
    if (r.stride < r.w) return bad(i, JXLH_ERR_INVALID_ARGUMENT, "stride < w");
    if ((uint64_t)r.x0 + r.w > s.ch[r.ec].w || (uint64_t)r.y0 + r.h > s.ch[r.ec].h)
      return bad(i, JXLH_ERR_INVALID_ARGUMENT, "the rect leaves the channel");
    const uint64_t extent = ec_rect_extent(r);
    if (r.offset > n_samples || extent > n_samples - r.offset)
      return bad(i, JXLH_ERR_INVALID_ARGUMENT, "offset + extent beyond n_samples");
  }
  return JXLH_OK;
}

// ---- ... and its scatter launch
// One non-empty rect as k_ec_scatter reads it (device memory, scalar loads): `first`, the first of its pieces in the
// launch's flat numbering (ascending over the list: a workgroup finds its rect by bisection), laid npx per row of
// pieces; vec: 16-byte accesses on both sides
struct EcScatterDesc {
  uint64_t src_off;  // samples from the block the kernel reads
  uint64_t dst_off;  // samples from the channel's plane: y0 * channel width + x0
  uint64_t first;
  uint32_t ec, w, h, src_stride, dst_stride, npx, vec, pad;
};
struct EcScatterPlan {
  std::vector<EcScatterDesc> descs;
  uint64_t pieces = 0;          // of the one launch (0: nothing to do)
  uint64_t span_lo = 0, span_hi = 0;  // the samples of the block the rects name, span_lo a multiple of 4
};
// The list has passed check_ec_rects.  staged: the block is host memory; [span_lo, span_hi) of it goes to a 16-byte
// aligned scratch block and src_off counts from span_lo.  Otherwise src_off counts from the block, whose address is
// block_addr.  A rect takes 16-byte accesses when its first sample and every row of it are 16-byte aligned on both
// sides: the source (address, offset, stride) and the plane (x0 and the channel's width, its base being aligned).
inline EcScatterPlan plan_ec_scatter(const EcCallState& s, const jxlh_ec_rect* rects, uint32_t n, bool staged,
                                     uint64_t block_addr) {
  EcScatterPlan p;
  uint64_t lo = UINT64_MAX, hi = 0;
  for (uint32_t i = 0; i < n; i++) {
    const jxlh_ec_rect& r = rects[i];
    if (r.w == 0 || r.h == 0) continue;
    lo = std::min(lo, r.offset);
    hi = std::max(hi, r.offset + ec_rect_extent(r));
  }
  if (hi == 0) return p;
  p.span_lo = lo & ~3ull;
  p.span_hi = hi;
  for (uint32_t i = 0; i < n; i++) {
    const jxlh_ec_rect& r = rects[i];
    if (r.w == 0 || r.h == 0) continue;
    const uint32_t cw = s.ch[r.ec].w;
    EcScatterDesc d{};
    d.src_off = staged ? r.offset - p.span_lo : r.offset;
    d.dst_off = (uint64_t)r.y0 * cw + r.x0;
    d.ec = r.ec;
    d.w = r.w;
    d.h = r.h;
    d.src_stride = r.stride;
    d.dst_stride = cw;
    d.npx = (r.w + kEcPieceW - 1) / kEcPieceW;
    const uint64_t src_first = staged ? d.src_off : block_addr / 4 + r.offset;
    const bool src_ok = (staged || block_addr % 4 == 0) && src_first % 4 == 0 && (r.h == 1 || r.stride % 4 == 0);
    const bool dst_ok = d.dst_off % 4 == 0 && (r.h == 1 || cw % 4 == 0);
    d.vec = src_ok && dst_ok;
    d.first = p.pieces;
    p.pieces += (uint64_t)d.npx * ((r.h + kEcPieceH - 1) / kEcPieceH);
    p.descs.push_back(d);
  }
  return p;
}

}  // namespace jxlh
