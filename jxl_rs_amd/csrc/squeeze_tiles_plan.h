// The route of a progressive preview of a squeezed image whose residual GROUPS have partly arrived
// (jxlh_unsqueeze_chain_preview_tiles): the kind of every grid cell of every level, which levels the final planes depend
// on, and per level either the whole-level launch of squeeze_preview_plan.h or two work lists -- its smooth cells and its
// regular runs.  Plain C++ on top of squeeze_preview_plan.h; the lists are std::vectors (a level has up to 2^20 cells).
// Host logic, tested without a device (tests/cpp/squeeze_tiles_plan.cc).
//
// The rule is the reference's per grid position (SqueezeInfo::new, step.rs:123-198; get_grid_idx, mod.rs:133-148), moved
// from grid indices to sample positions: see include/jxl_hip_preview_tiles.h.
#pragma once
#include <vector>

#include "squeeze_preview_plan.h"

// Geometry of the smooth tile body (k_smooth_unsqueeze.hip ties its tile to them) and of the run kernel
#define JXLH_SQC_TX 64     // average samples per tile row
#define JXLH_SQC_TY 32     // average rows per tile
#define JXLH_SQC_LINES 64  // lines per workgroup of the run kernel: one wave, a lane per line

namespace jxlh {

constexpr uint32_t kSqueezeMaxCells = 1u << 20;  // cells of one level

// ---- a level's grid: the effective cell size and the cell counts
struct SqTileGrid { uint32_t tw, th, nx, ny; };
inline SqTileGrid squeeze_tile_grid(const jxlh_squeeze_level& lv, const jxlh_squeeze_tiles& t) {
  const uint32_t tw = t.tile_w ? t.tile_w : lv.out_w, th = t.tile_h ? t.tile_h : lv.out_h;
  return {tw, th, (lv.out_w + tw - 1) / tw, (lv.out_h + th - 1) / th};
}
// the rules on top of check_squeeze_chain's (the levels have passed it)
inline jxlh_status check_squeeze_tiles(int n_levels, const jxlh_squeeze_level* levels, const jxlh_squeeze_tiles* tiles) {
  if (!tiles) return JXLH_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < n_levels; i++) {
    const jxlh_squeeze_tiles& t = tiles[i];
    if ((t.tile_w == 0) != (t.tile_h == 0)) return JXLH_ERR_INVALID_ARGUMENT;
    const SqTileGrid g = squeeze_tile_grid(levels[i], t);
    if ((uint64_t)g.nx * g.ny > kSqueezeMaxCells) return JXLH_ERR_INVALID_ARGUMENT;
    // a cell starts on a pair
    if (levels[i].horizontal ? (g.nx > 1 && g.tw % 2) : (g.ny > 1 && g.th % 2)) return JXLH_ERR_INVALID_ARGUMENT;
  }
  return JXLH_OK;
}
inline bool squeeze_cell_missing(int n_planes, const jxlh_squeeze_level& lv, const jxlh_squeeze_tiles& t, const SqTileGrid& g,
                                 uint32_t tx, uint32_t ty) {
  if (!squeeze_extents(lv.horizontal != 0, lv.out_w, lv.out_h).has_res) return false;
  if (squeeze_level_missing(n_planes, lv)) return true;
  return t.present && t.present[(size_t)ty * g.nx + tx] == 0;
}
// ---- kinds[ty * nx + tx] of level `level`: JXLH_PREVIEW_*
inline void squeeze_tile_kinds(int n_planes, const jxlh_squeeze_level* levels, const jxlh_squeeze_tiles* tiles, int level,
                               uint8_t* kinds) {
  const jxlh_squeeze_level& lv = levels[level];
  const SqTileGrid g = squeeze_tile_grid(lv, tiles[level]);
  const bool horiz = lv.horizontal != 0;
  const bool crossed = level > 0 && (levels[level - 1].horizontal != 0) != horiz;
  const SqTileGrid g1 = crossed ? squeeze_tile_grid(levels[level - 1], tiles[level - 1]) : SqTileGrid{};
  for (uint32_t ty = 0; ty < g.ny; ty++)
    for (uint32_t tx = 0; tx < g.nx; tx++) {
      uint8_t& k = kinds[(size_t)ty * g.nx + tx];
      if (!squeeze_cell_missing(n_planes, lv, tiles[level], g, tx, ty)) {
        k = JXLH_PREVIEW_REGULAR;
        continue;
      }
      k = JXLH_PREVIEW_SMOOTH_1D;
      if (!crossed) continue;
      // the cell's top-left sample in this level's average, which is level - 1's output
      const uint32_t px = horiz ? (tx * g.tw) >> 1 : tx * g.tw, py = horiz ? ty * g.th : (ty * g.th) >> 1;
      const uint32_t cx = std::min(px / g1.tw, g1.nx - 1), cy = std::min(py / g1.th, g1.ny - 1);
      if (squeeze_cell_missing(n_planes, levels[level - 1], tiles[level - 1], g1, cx, cy)) k = JXLH_PREVIEW_SMOOTH_2D;
    }
}

// a smooth cell without one complete pair on an axis it doubles (the 1-wide last cell of out_w = k tile_w + 1): the
// reference leaves its fresh buffer untouched -- the cell is zero, where the whole-channel step writes the same samples
inline bool squeeze_tiles_ragged_smooth(const jxlh_squeeze_level& lv, const SqTileGrid& g, const uint8_t* kinds) {
  const bool horiz = lv.horizontal != 0;
  const bool last_w1 = lv.out_w - (g.nx - 1) * g.tw < 2, last_h1 = lv.out_h - (g.ny - 1) * g.th < 2;
  for (uint32_t ty = 0; ty < g.ny; ty++)
    for (uint32_t tx = 0; tx < g.nx; tx++) {
      const uint8_t k = kinds[(size_t)ty * g.nx + tx];
      if (k == JXLH_PREVIEW_REGULAR) continue;
      const bool two_d = k == JXLH_PREVIEW_SMOOTH_2D;
      if (((two_d || horiz) && last_w1 && tx == g.nx - 1) || ((two_d || !horiz) && last_h1 && ty == g.ny - 1)) return true;
    }
  return false;
}

// ---- the work lists of a mixed level, as the kernels read them: 16-byte records
struct SqTileSmoothCell { int32_t x0, y0, w, h_kind; };    // the cell's rect in the output; h_kind = h << 2 | JXLH_PREVIEW_SMOOTH_*
struct SqTileRun { int32_t pair0, n_pairs, line0, n_lines_tail; };  // n_lines_tail = n_lines << 1 | (the odd tail follows the run)

// one level behind the regular prefix
struct SqTilesEntry {
  int level;
  int kind;                    // the kind all cells share (JXLH_PREVIEW_*), or -1: mixed -- the two lists
  bool horizontal;
  SqueezeLoc src, src2, dst;   // src: the level's average (level - 1's output); src2: what level - 1 reads (2-D cells)
  uint32_t src_w, src_h, src2_w, src2_h;
  bool rct;                    // whole smooth level: the fused kernel applies the RCT; mixed: an RCT launch follows
  int n_launch;                // whole regular level: as PreviewEntry
  SqueezeLaunch launch[2];
  SqTileGrid grid;
  std::vector<uint8_t> kinds;
  std::vector<SqTileSmoothCell> smooth;
  std::vector<SqTileRun> runs;
  uint32_t tiles_x, tiles_per_cell;  // smooth launch: tiles_per_cell workgroups per listed cell, tiles_x of them in a row
  uint32_t groups_per_run;           // run launch: workgroups of JXLH_SQC_LINES lines per listed run
  size_t smooth_off, runs_off;       // the lists' places in the call's upload, in records
};
struct SqueezeTilesPlan {
  bool mixed;                          // some level goes cell by cell; false: the call is jxlh_unsqueeze_chain_preview of `folded`
  std::vector<jxlh_squeeze_level> folded;  // the levels with res[] = NULL where every cell is missing
  std::vector<uint8_t> need;           // need[i]: the final planes depend on level i
  SqueezeArena arena;
  int n_prefix;                        // levels [0, n_prefix): no missing cell, through plan_squeeze_chain
  SqueezeChainIn prefix_in;
  SqueezePlan prefix;
  std::vector<SqTilesEntry> entry;
  size_t upload_records;               // all lists of the call, one upload
  bool too_large;                      // a launch would need 2^31 workgroups or more
};

// the regular runs of a mixed level: maximal sequences of regular cells along the squeezed axis inside one cell row
// (horizontal) or cell column (vertical)
inline void squeeze_tile_runs(const jxlh_squeeze_level& lv, const SqTileGrid& g, const uint8_t* kinds, std::vector<SqTileRun>& runs) {
  const bool horiz = lv.horizontal != 0;
  const uint32_t n_along = horiz ? g.nx : g.ny, n_across = horiz ? g.ny : g.nx;
  const uint32_t t_along = horiz ? g.tw : g.th, t_across = horiz ? g.th : g.tw;
  const uint32_t len = horiz ? lv.out_w : lv.out_h, lines = horiz ? lv.out_h : lv.out_w;
  for (uint32_t a = 0; a < n_across; a++) {
    const uint32_t line0 = a * t_across, n_lines = std::min(t_across, lines - line0);
    for (uint32_t c = 0; c < n_along;) {
      auto kind = [&](uint32_t i) { return kinds[horiz ? (size_t)a * g.nx + i : (size_t)i * g.nx + a]; };
      if (kind(c) != JXLH_PREVIEW_REGULAR) {
        c++;
        continue;
      }
      uint32_t e = c;
      while (e < n_along && kind(e) == JXLH_PREVIEW_REGULAR) e++;
      const uint32_t s0 = c * t_along, s1 = std::min(len, e * t_along);  // s0 is even (check_squeeze_tiles)
      runs.push_back({(int32_t)(s0 / 2), (int32_t)(s1 / 2 - s0 / 2), (int32_t)line0, (int32_t)(n_lines << 1 | (s1 == len && (len & 1)))});
      c = e;
    }
  }
}

// `in` as for plan_squeeze_preview, levels checked with allow_missing, tiles with check_squeeze_tiles
inline SqueezeTilesPlan plan_squeeze_tiles(const SqueezeChainIn& in, const jxlh_squeeze_tiles* tiles) {
  SqueezeTilesPlan P{};
  const int nl = in.n_levels, np = in.n_planes;
  std::vector<std::vector<uint8_t>> kinds(nl);
  std::vector<int> uniform(nl);  // the kind all cells share, or -1
  P.folded.assign(in.levels, in.levels + nl);
  for (int i = 0; i < nl; i++) {
    const SqTileGrid g = squeeze_tile_grid(in.levels[i], tiles[i]);
    kinds[i].resize((size_t)g.nx * g.ny);
    squeeze_tile_kinds(np, in.levels, tiles, i, kinds[i].data());
    uniform[i] = kinds[i][0];
    bool any_regular = false, any_smooth = false;
    for (uint8_t k : kinds[i]) {
      if (k != uniform[i]) uniform[i] = -1;
      (k == JXLH_PREVIEW_REGULAR ? any_regular : any_smooth) = true;
    }
    // a smooth cell without a complete pair is zero, which no whole-level launch writes: such a level goes cell by cell
    const bool ragged = any_smooth && squeeze_tiles_ragged_smooth(in.levels[i], g, kinds[i].data());
    if (ragged) uniform[i] = -1;
    if ((any_regular && any_smooth) || ragged) P.mixed = true;
    if (!any_regular)
      for (int p = 0; p < 3; p++) P.folded[i].res[p] = nullptr;
  }
  if (!P.mixed) return P;  // every mask uniform: the whole-level rule decides the same kinds

  P.arena = squeeze_arena(np, nl, in.levels);
  auto loc = [&](int i) {
    return i < 0 ? SqueezeLoc{kSqBase, in.base_stride} : i == nl - 1 ? SqueezeLoc{kSqOut, in.out_stride} : SqueezeLoc{i, P.arena.stride[i]};
  };
  while (P.n_prefix < nl && uniform[P.n_prefix] == JXLH_PREVIEW_REGULAR) P.n_prefix++;
  if (P.n_prefix > 0) {  // (a mixed level follows: the prefix ends in the arena, and the RCT is not its business)
    P.prefix_in = in;
    P.prefix_in.n_levels = P.n_prefix;
    const SqueezeLoc d = loc(P.n_prefix - 1);
    for (int p = 0; p < np; p++) P.prefix_in.out[p] = squeeze_plane_addr(in, P.arena, d, p);
    P.prefix_in.out_stride = d.stride;
    P.prefix_in.with_rct = false;
    P.prefix = plan_squeeze_chain(P.prefix_in);
  }
  // a level's regular and 1-D cells read the level before, its 2-D cells the one before that
  P.need.assign(nl, 0);
  P.need[nl - 1] = 1;
  for (int i = nl - 1; i >= P.n_prefix; i--) {
    if (!P.need[i]) continue;
    bool any_2d = false, any_other = false;
    for (uint8_t k : kinds[i]) (k == JXLH_PREVIEW_SMOOTH_2D ? any_2d : any_other) = true;
    if (any_other && i >= 1) P.need[i - 1] = 1;
    if (any_2d && i >= 2) P.need[i - 2] = 1;
  }
  for (int i = 0; i < P.n_prefix; i++) P.need[i] = 1;

  for (int i = P.n_prefix; i < nl; i++) {
    if (!P.need[i]) continue;
    P.entry.emplace_back();
    SqTilesEntry& e = P.entry.back();
    const jxlh_squeeze_level& lv = in.levels[i];
    const bool horiz = lv.horizontal != 0;
    e.level = i;
    e.kind = uniform[i];
    e.horizontal = horiz;
    e.src = loc(i - 1);
    e.src2 = loc(i - 2);
    e.dst = loc(i);
    const SqueezeExtents x = squeeze_extents(horiz, lv.out_w, lv.out_h);
    e.src_w = x.avg_w;
    e.src_h = x.avg_h;
    e.src2_w = (lv.out_w + 1) / 2;
    e.src2_h = (lv.out_h + 1) / 2;
    e.grid = squeeze_tile_grid(lv, tiles[i]);
    const bool last_rct = i == nl - 1 && in.with_rct;
    e.rct = last_rct;
    if (e.kind == JXLH_PREVIEW_REGULAR) {
      const SqueezeStep s = squeeze_level_step(in, P.arena, i, e.src, e.dst);
      e.n_launch = last_rct ? plan_squeeze_step_rct(s, in.separate_rct, e.launch) : (e.launch[0] = plan_squeeze_step(s), 1);
    } else if (e.kind < 0) {
      e.kinds = kinds[i];
      const SqTileGrid& g = e.grid;
      for (uint32_t ty = 0; ty < g.ny; ty++)
        for (uint32_t tx = 0; tx < g.nx; tx++) {
          const uint8_t k = e.kinds[(size_t)ty * g.nx + tx];
          if (k == JXLH_PREVIEW_REGULAR) continue;
          const uint32_t x0 = tx * g.tw, y0 = ty * g.th;
          e.smooth.push_back({(int32_t)x0, (int32_t)y0, (int32_t)std::min(g.tw, lv.out_w - x0),
                              (int32_t)(std::min(g.th, lv.out_h - y0) << 2 | k)});
        }
      squeeze_tile_runs(lv, g, e.kinds.data(), e.runs);
      // a 1-D cell has the most tiles: only the squeezed axis is halved
      const uint32_t cw = std::min(g.tw, lv.out_w), ch = std::min(g.th, lv.out_h);
      const uint32_t nx = horiz ? (cw + 1) / 2 : cw, ny = horiz ? ch : (ch + 1) / 2;
      e.tiles_x = (nx + JXLH_SQC_TX - 1) / JXLH_SQC_TX;
      e.tiles_per_cell = e.tiles_x * ((ny + JXLH_SQC_TY - 1) / JXLH_SQC_TY);
      e.groups_per_run = ((horiz ? ch : cw) + JXLH_SQC_LINES - 1) / JXLH_SQC_LINES;
      if ((uint64_t)e.tiles_per_cell * e.smooth.size() >= (1ull << 31) || (uint64_t)e.groups_per_run * e.runs.size() >= (1ull << 31))
        P.too_large = true;
      e.smooth_off = P.upload_records;
      e.runs_off = e.smooth_off + e.smooth.size();
      P.upload_records = e.runs_off + e.runs.size();
    }
  }
  return P;
}

}  // namespace jxlh
