// The route of a progressive preview of a squeezed image (jxlh_unsqueeze_chain_preview, jxlh_unsqueeze_chain_preview_tiles):
// the kind of every grid cell of every level, which levels the final planes depend on, and the launches in order -- per
// level one whole-level launch group, or two work lists: its smooth cells and its regular runs.  A call without grids is
// the call whose every level is one cell without a mask.  Plain C++ on top of squeeze_plan.h; fixed-size arrays but for
// the work lists and the cell kinds of levels with more than one cell (a level has up to 2^20 cells).  Host logic, tested
// without a device (tests/cpp/squeeze_preview_plan.cc, tests/cpp/squeeze_tiles_plan.cc).
//
// The rule is the reference's.  For whole channels (meta_apply.rs:150-161 links a step to the step of the other axis that
// feeds it; step.rs:138-150 picks the kind from the two residuals' DataStatus):
//   regular    the level's residual is there;
//   SMOOTH_2D  it is missing, level L - 1 squeezes the other axis and is missing too: the level upsamples the average
//              that level L - 1 reads (the output of level L - 2, or the base) in both axes at once;
//   SMOOTH_1D  it is missing otherwise: smooth_h / smooth_v on its own average, the output of level L - 1.
// Per grid position (SqueezeInfo::new, step.rs:123-198; get_grid_idx, mod.rs:133-148) it is the same rule on the cell and
// the cell of level L - 1 under it, moved from grid indices to sample positions: see include/jxl_hip_preview_tiles.h.
// A level whose cells are all 2-D does not read level L - 1's output, so that level may be dead: nothing the final planes
// depend on.  The reference computes dead levels all the same; here they are not launched.
#pragma once
#include <vector>

#include "squeeze_plan.h"

// Geometry of the smooth tile body (k_smooth_unsqueeze.hip ties its tile to them) and of the run kernel
#define JXLH_SQC_TX 64     // average samples per tile row
#define JXLH_SQC_TY 32     // average rows per tile
#define JXLH_SQC_LINES 64  // lines per workgroup of the run kernel: one wave, a lane per line

namespace jxlh {

constexpr uint32_t kSqueezeMaxCells = 1u << 20;  // cells of one level

// ---- whole levels.  kinds[i]: JXLH_PREVIEW_*; live[i] (may be null): 1 when the last level's planes depend on level i's
inline void squeeze_preview_kinds(int n_planes, int n_levels, const jxlh_squeeze_level* levels, uint8_t* kinds, uint8_t* live) {
  for (int i = 0; i < n_levels; i++) {
    if (!squeeze_level_missing(n_planes, levels[i])) kinds[i] = JXLH_PREVIEW_REGULAR;
    else if (i > 0 && (levels[i - 1].horizontal != 0) != (levels[i].horizontal != 0) && squeeze_level_missing(n_planes, levels[i - 1]))
      kinds[i] = JXLH_PREVIEW_SMOOTH_2D;
    else kinds[i] = JXLH_PREVIEW_SMOOTH_1D;
  }
  if (!live) return;
  for (int i = 0; i < n_levels; i++) live[i] = 0;
  for (int i = n_levels - 1; i >= 0; i -= kinds[i] == JXLH_PREVIEW_SMOOTH_2D ? 2 : 1) live[i] = 1;
}

// ---- a level's grid: the effective cell size and the cell counts.  tiles == nullptr: every level is one cell, no mask
struct SqTileGrid { uint32_t tw, th, nx, ny; };
inline jxlh_squeeze_tiles squeeze_tiles_of(const jxlh_squeeze_tiles* tiles, int level) {
  return tiles ? tiles[level] : jxlh_squeeze_tiles{};
}
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
  const jxlh_squeeze_tiles t = squeeze_tiles_of(tiles, level);
  const SqTileGrid g = squeeze_tile_grid(lv, t);
  const bool horiz = lv.horizontal != 0;
  const bool crossed = level > 0 && (levels[level - 1].horizontal != 0) != horiz;
  const jxlh_squeeze_tiles t1 = crossed ? squeeze_tiles_of(tiles, level - 1) : jxlh_squeeze_tiles{};
  const SqTileGrid g1 = crossed ? squeeze_tile_grid(levels[level - 1], t1) : SqTileGrid{};
  for (uint32_t ty = 0; ty < g.ny; ty++)
    for (uint32_t tx = 0; tx < g.nx; tx++) {
      uint8_t& k = kinds[(size_t)ty * g.nx + tx];
      if (!squeeze_cell_missing(n_planes, lv, t, g, tx, ty)) {
        k = JXLH_PREVIEW_REGULAR;
        continue;
      }
      k = JXLH_PREVIEW_SMOOTH_1D;
      if (!crossed) continue;
      // the cell's top-left sample in this level's average, which is level - 1's output
      const uint32_t px = horiz ? (tx * g.tw) >> 1 : tx * g.tw, py = horiz ? ty * g.th : (ty * g.th) >> 1;
      const uint32_t cx = std::min(px / g1.tw, g1.nx - 1), cy = std::min(py / g1.th, g1.ny - 1);
      if (squeeze_cell_missing(n_planes, levels[level - 1], t1, g1, cx, cy)) k = JXLH_PREVIEW_SMOOTH_2D;
    }
}

// a smooth cell without one complete pair on an axis it doubles (the 1-wide last cell of out_w = k tile_w + 1): the
// reference leaves its fresh buffer untouched -- the cell is zero, where the whole-channel step writes the same samples.
// (Never a one-cell level: a 1-wide or 1-high level has no residual samples on that axis, so it is not missing.)
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

// ---- the work lists of a level that goes cell by cell, as the kernels read them: 16-byte records
struct SqTileSmoothCell { int32_t x0, y0, w, h_kind; };    // the cell's rect in the output; h_kind = h << 2 | JXLH_PREVIEW_SMOOTH_*
struct SqTileRun { int32_t pair0, n_pairs, line0, n_lines_tail; };  // n_lines_tail = n_lines << 1 | (the odd tail follows the run)
union SqTileRecord { SqTileSmoothCell cell; SqTileRun run; };       // all lists of a call live in one array of these
static_assert(sizeof(SqTileRecord) == 16 && sizeof(SqTileSmoothCell) == 16 && sizeof(SqTileRun) == 16, "the lists are 16-byte records");

// the regular runs of such a level: maximal sequences of regular cells along the squeezed axis inside one cell row
// (horizontal) or cell column (vertical)
inline void squeeze_tile_runs(const jxlh_squeeze_level& lv, const SqTileGrid& g, const uint8_t* kinds, std::vector<SqTileRecord>& runs) {
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
      SqTileRecord r;
      r.run = {(int32_t)(s0 / 2), (int32_t)(s1 / 2 - s0 / 2), (int32_t)line0, (int32_t)(n_lines << 1 | (s1 == len && (len & 1)))};
      runs.push_back(r);
      c = e;
    }
  }
}

// ---- one live level behind the regular prefix
struct PreviewEntry {
  int level;
  int kind;                    // the kind all cells share (JXLH_PREVIEW_*), or -1: cell by cell -- the two lists
  SqueezeLoc src, src2, dst;   // src: the level's average (level - 1's output), read by regular and 1-D cells; src2: what
                               // level - 1 reads (level - 2's output, or the base), read by 2-D cells
  uint32_t src_w, src_h, src2_w, src2_h;
  bool rct;                    // the RCT follows this level.  Whole regular level: the launches below say how; whole
                               // smooth level: the fused kernel applies it; cell by cell: an RCT launch follows
  int n_launch;                // whole regular level: 1 or 2 (step, or fused step + RCT, or step and RCT)
  SqueezeLaunch launch[2];
  // cell by cell
  SqTileGrid grid;
  uint32_t tiles_x, tiles_per_cell;  // smooth launch: tiles_per_cell workgroups per listed cell, tiles_x of them in a row
  uint32_t groups_per_run;           // run launch: workgroups of JXLH_SQC_LINES lines per listed run
  size_t smooth_off, runs_off;       // the two lists' places in the plan's records ...
  uint32_t n_smooth, n_runs;         // ... and their lengths
};
struct SqueezePreviewPlan {
  int8_t kind[kSqueezeMaxLevels];  // the kind all cells of the level share, or -1: mixed kinds or a ragged smooth cell
  uint8_t live[kSqueezeMaxLevels]; // the final planes depend on the level
  SqueezeArena arena;          // of the WHOLE chain: the prefix's plane sets are its first ones
  int n_prefix;                // levels [0, n_prefix): every cell regular, through plan_squeeze_chain
  SqueezeChainIn prefix_in;    // ... as that chain: its `out` is the arena's plane set of level n_prefix - 1 unless nothing follows
  SqueezePlan prefix;
  int n;
  PreviewEntry entry[kSqueezeMaxLevels];
  std::vector<SqTileRecord> records;  // all lists of the call in upload order: one copy
  bool too_large;              // a launch would need 2^31 workgroups or more
};

// `in` as for plan_squeeze_chain, levels checked with allow_missing (check_squeeze_chain); tiles: null, or checked with
// check_squeeze_tiles
inline SqueezePreviewPlan plan_squeeze_preview(const SqueezeChainIn& in, const jxlh_squeeze_tiles* tiles) {
  SqueezePreviewPlan P{};
  const int nl = in.n_levels, np = in.n_planes;
  // ---- the kinds of every level's cells: a one-cell level's in one[], the others' in `cells`
  uint8_t one[kSqueezeMaxLevels], reads[kSqueezeMaxLevels];  // reads: 1: some cell reads level - 1's output, 2: ... level - 2's
  size_t cell_off[kSqueezeMaxLevels], n_cells = 0;
  std::vector<uint8_t> cells;
  auto grid = [&](int i) { return squeeze_tile_grid(in.levels[i], squeeze_tiles_of(tiles, i)); };
  for (int i = 0; i < nl && tiles; i++) {
    const SqTileGrid g = grid(i);
    cell_off[i] = n_cells;
    if (g.nx * g.ny > 1) n_cells += (size_t)g.nx * g.ny;
  }
  cells.resize(n_cells);
  auto kinds_of = [&](int i, const SqTileGrid& g) { return g.nx * g.ny > 1 ? cells.data() + cell_off[i] : one + i; };
  for (int i = 0; i < nl; i++) {
    const SqTileGrid g = grid(i);
    uint8_t* k = kinds_of(i, g);
    squeeze_tile_kinds(np, in.levels, tiles, i, k);
    bool any[3] = {};
    for (size_t c = 0, n = (size_t)g.nx * g.ny; c < n; c++) any[k[c]] = true;
    const bool any_smooth = any[JXLH_PREVIEW_SMOOTH_1D] || any[JXLH_PREVIEW_SMOOTH_2D];
    // a smooth cell without a complete pair is zero, which no whole-level launch writes: such a level goes cell by cell
    const bool cellwise = any[0] + any[1] + any[2] > 1 || (any_smooth && squeeze_tiles_ragged_smooth(in.levels[i], g, k));
    P.kind[i] = cellwise ? -1 : (int8_t)k[0];
    reads[i] = (any[JXLH_PREVIEW_REGULAR] || any[JXLH_PREVIEW_SMOOTH_1D] ? 1 : 0) | (any[JXLH_PREVIEW_SMOOTH_2D] ? 2 : 0);
  }
  // ---- a level's regular and 1-D cells read the level before, its 2-D cells the one before that
  P.live[nl - 1] = 1;
  for (int i = nl - 1; i >= 1; i--) {
    if (!P.live[i]) continue;
    if (reads[i] & 1) P.live[i - 1] = 1;
    if ((reads[i] & 2) && i >= 2) P.live[i - 2] = 1;
  }

  P.arena = squeeze_arena(np, nl, in.levels);
  auto loc = [&](int i) {
    return i < 0 ? SqueezeLoc{kSqBase, in.base_stride} : i == nl - 1 ? SqueezeLoc{kSqOut, in.out_stride} : SqueezeLoc{i, P.arena.stride[i]};
  };
  while (P.n_prefix < nl && P.kind[P.n_prefix] == JXLH_PREVIEW_REGULAR) P.n_prefix++;
  if (P.n_prefix > 0) {
    P.prefix_in = in;
    P.prefix_in.n_levels = P.n_prefix;
    if (P.n_prefix < nl) {  // something follows: the prefix ends in the arena, and the RCT is not its business
      const SqueezeLoc d = loc(P.n_prefix - 1);
      for (int p = 0; p < np; p++) P.prefix_in.out[p] = squeeze_plane_addr(in, P.arena, d, p);
      P.prefix_in.out_stride = d.stride;
      P.prefix_in.with_rct = false;
    }
    P.prefix = plan_squeeze_chain(P.prefix_in);
  }
  for (int i = P.n_prefix; i < nl; i++) {
    if (!P.live[i]) continue;
    PreviewEntry& e = P.entry[P.n++];
    const jxlh_squeeze_level& lv = in.levels[i];
    const bool horiz = lv.horizontal != 0;
    e.level = i;
    e.kind = P.kind[i];
    e.src = loc(i - 1);
    e.src2 = loc(i - 2);
    e.dst = loc(i);
    const SqueezeExtents x = squeeze_extents(horiz, lv.out_w, lv.out_h);
    e.src_w = x.avg_w;
    e.src_h = x.avg_h;
    e.src2_w = (lv.out_w + 1) / 2;
    e.src2_h = (lv.out_h + 1) / 2;
    e.rct = i == nl - 1 && in.with_rct;
    if (e.kind == JXLH_PREVIEW_REGULAR) {
      const SqueezeStep s = squeeze_level_step(in, P.arena, i, e.src, e.dst);
      e.n_launch = e.rct ? plan_squeeze_step_rct(s, in.separate_rct, e.launch) : (e.launch[0] = plan_squeeze_step(s), 1);
    } else if (e.kind < 0) {
      const SqTileGrid g = e.grid = grid(i);
      const uint8_t* kinds = kinds_of(i, g);
      e.smooth_off = P.records.size();
      for (uint32_t ty = 0; ty < g.ny; ty++)
        for (uint32_t tx = 0; tx < g.nx; tx++) {
          const uint8_t k = kinds[(size_t)ty * g.nx + tx];
          if (k == JXLH_PREVIEW_REGULAR) continue;
          const uint32_t x0 = tx * g.tw, y0 = ty * g.th;
          SqTileRecord r;
          r.cell = {(int32_t)x0, (int32_t)y0, (int32_t)std::min(g.tw, lv.out_w - x0), (int32_t)(std::min(g.th, lv.out_h - y0) << 2 | k)};
          P.records.push_back(r);
        }
      e.runs_off = P.records.size();
      squeeze_tile_runs(lv, g, kinds, P.records);
      e.n_smooth = (uint32_t)(e.runs_off - e.smooth_off);
      e.n_runs = (uint32_t)(P.records.size() - e.runs_off);
      // a 1-D cell has the most tiles: only the squeezed axis is halved
      const uint32_t cw = std::min(g.tw, lv.out_w), ch = std::min(g.th, lv.out_h);
      const uint32_t nx = horiz ? (cw + 1) / 2 : cw, ny = horiz ? ch : (ch + 1) / 2;
      e.tiles_x = (nx + JXLH_SQC_TX - 1) / JXLH_SQC_TX;
      e.tiles_per_cell = e.tiles_x * ((ny + JXLH_SQC_TY - 1) / JXLH_SQC_TY);
      e.groups_per_run = ((horiz ? ch : cw) + JXLH_SQC_LINES - 1) / JXLH_SQC_LINES;
      if ((uint64_t)e.tiles_per_cell * e.n_smooth >= (1ull << 31) || (uint64_t)e.groups_per_run * e.n_runs >= (1ull << 31)) P.too_large = true;
    }
  }
  return P;
}

}  // namespace jxlh
