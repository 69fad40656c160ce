// The preview planner (jxl_rs_amd/csrc/squeeze_preview_plan.h) with grids: the geometries of the tile tests and random
// chains, grids and masks.  Checked: kinds by their definition; a level goes cell by cell exactly when its kinds are mixed
// or a smooth cell is ragged; a chain without such a level plans as the same chain without grids whose all-missing levels
// name no residuals, field by field; the prefix ends in front of the first level with a missing cell, levels the final
// planes do not depend on have no entry, every whole-level entry -- beside cell-wise ones too -- passes the checks of a
// plan without grids (squeeze_preview_checks.h), and in a cell-wise entry every cell is in exactly one list -- the smooth
// list, or exactly one regular run; runs are maximal (a smooth cell or the channel's edge on either side), disjoint,
// start on a pair, carry the tail only at the channel's odd end, and every sample offset a run or a smooth cell touches
// stays inside the planes.  Host only, no device: addresses are numbers.  Built plain and with
// -fsanitize=address,undefined (tests/test_squeeze_tiles_cpu.py).
#include "squeeze_preview_checks.h"

namespace {

int g_mixed = 0, g_runs = 0, g_smooth = 0;
int g_equal = 0;                                // chains without a cell-wise level, held against the plan without grids
int g_whole_smooth = 0, g_whole_regular = 0;    // whole-level entries behind a cell-wise level

// P, planned with grids and no cell-wise level, against Q: the chain with res[] cleared where every cell is missing,
// planned without grids
void check_same_plan(int id, const SqueezePreviewPlan& P, const SqueezePreviewPlan& Q, int nl) {
  CHECK(P.n_prefix == Q.n_prefix && P.n == Q.n && P.records.empty() && Q.records.empty() && !P.too_large && !Q.too_large,
        "chain %d: prefix %d / %d, entries %d / %d", id, P.n_prefix, Q.n_prefix, P.n, Q.n);
  CHECK(!std::memcmp(&P.arena, &Q.arena, sizeof P.arena), "chain %d: arena", id);
  for (int i = 0; i < nl; i++) CHECK(P.kind[i] == Q.kind[i] && P.live[i] == Q.live[i], "chain %d level %d: kind, live", id, i);
  if (P.n_prefix > 0) {
    const SqueezeChainIn &a = P.prefix_in, &b = Q.prefix_in;
    CHECK(a.n_planes == b.n_planes && a.n_levels == b.n_levels && a.base_w == b.base_w && a.base_h == b.base_h && a.base_stride == b.base_stride &&
              a.out_stride == b.out_stride && !std::memcmp(a.base, b.base, sizeof a.base) && !std::memcmp(a.out, b.out, sizeof a.out) &&
              a.arena == b.arena && a.with_rct == b.with_rct && a.separate_rct == b.separate_rct && a.flow == b.flow,
          "chain %d: the prefix's chain", id);
    CHECK(P.prefix.n == Q.prefix.n && P.prefix.flow_words == Q.prefix.flow_words && !std::memcmp(P.prefix.vec, Q.prefix.vec, sizeof P.prefix.vec) &&
              !std::memcmp(&P.prefix.arena, &Q.prefix.arena, sizeof P.prefix.arena), "chain %d: the prefix's plan", id);
    for (int k = 0; k < P.prefix.n && k < Q.prefix.n; k++) CHECK(same_launch(P.prefix.launch[k], Q.prefix.launch[k]), "chain %d: prefix launch %d", id, k);
  }
  for (int k = 0; k < P.n && k < Q.n; k++) {
    const PreviewEntry &a = P.entry[k], &b = Q.entry[k];
    CHECK(a.level == b.level && a.kind == b.kind && a.kind >= 0 && same_loc(a.src, b.src) && same_loc(a.src2, b.src2) && same_loc(a.dst, b.dst) &&
              a.src_w == b.src_w && a.src_h == b.src_h && a.src2_w == b.src2_w && a.src2_h == b.src2_h && a.rct == b.rct && a.n_launch == b.n_launch &&
              a.n_smooth == 0 && a.n_runs == 0 && b.n_smooth == 0 && b.n_runs == 0, "chain %d entry %d (level %d / %d)", id, k, a.level, b.level);
    for (int j = 0; j < a.n_launch && j < b.n_launch; j++) CHECK(same_launch(a.launch[j], b.launch[j]), "chain %d entry %d launch %d", id, k, j);
  }
}

// w x h, nl levels alternating from `first_hz` at the finest; finest cell tw x th halved per level (0: one cell);
// density: per cent of present cells
void one_chain(int id, uint32_t w, uint32_t h, int nl, bool finest_hz, uint32_t tw, uint32_t th, int n_grid, uint32_t density,
               bool random_dirs) {
  jxlh_squeeze_level lv[kSqueezeMaxLevels];
  jxlh_squeeze_tiles tl[kSqueezeMaxLevels];
  std::memset(lv, 0, sizeof lv);
  std::memset(tl, 0, sizeof tl);
  std::vector<std::vector<uint8_t>> masks(nl);
  const int n_planes = (int)rnd(1, 3);
  const uintptr_t kRes = 0x100000000ull;
  uint32_t cw = w, ch = h;
  for (int i = nl - 1; i >= 0; i--) {
    const int k = nl - 1 - i;
    const bool hz = random_dirs ? (rnd() & 1) : ((k & 1) == 0) == finest_hz;
    lv[i].horizontal = hz;
    lv[i].out_w = cw;
    lv[i].out_h = ch;
    const SqueezeExtents e = squeeze_extents(hz, cw, ch);
    lv[i].res_stride = e.res_w + (rnd() % 3 ? 0 : rnd(1, 7));
    const bool null_res = rnd() % 7 == 0;
    for (int p = 0; p < n_planes; p++) lv[i].res[p] = null_res ? nullptr : (const int32_t*)(kRes + ((uintptr_t)i << 28) + ((uintptr_t)p << 26));
    if (k < n_grid && tw && th) {
      // a cell starts on a pair
      uint32_t a = tw, b = th;
      if (hz && a % 2 && a < cw) a++;
      if (!hz && b % 2 && b < ch) b++;
      tl[i].tile_w = a;
      tl[i].tile_h = b;
    }
    const SqTileGrid g = squeeze_tile_grid(lv[i], tl[i]);
    if (rnd() % 5) {
      masks[i].resize((size_t)g.nx * g.ny);
      const uint32_t mode = rnd(0, 5);  // 0, 1: uniform; else random
      for (auto& m : masks[i]) m = mode == 0 ? 0 : mode == 1 ? 1 : (rnd() % 100 < density ? (uint8_t)rnd(1, 255) : 0);
      tl[i].present = masks[i].data();
    }
    if (hz) { cw = (cw + 1) / 2; tw = tw > 1 ? tw / 2 : tw; } else { ch = (ch + 1) / 2; th = th > 1 ? th / 2 : th; }
  }
  const uint32_t base_w = cw, base_h = ch;
  const size_t out_stride = w + (rnd() % 2 ? 0 : rnd(1, 9));
  const size_t base_stride = base_w + rnd(0, 3);
  const int32_t* base[3];
  int32_t* out[3];
  for (int p = 0; p < 3; p++) {
    base[p] = (const int32_t*)(0x10000000ull + ((uintptr_t)p << 24));
    out[p] = (int32_t*)(0x20000000ull + ((uintptr_t)p << 26));
  }
  const jxlh_status st = check_squeeze_chain(n_planes, nl, lv, base, base_stride, base_w, base_h, out, out_stride, [](const void*) { return true; }, true);
  CHECK(st == JXLH_OK, "chain %d: the chain was refused", id);
  if (st) return;
  const jxlh_status st2 = check_squeeze_tiles(nl, lv, tl);
  CHECK(st2 == JXLH_OK, "chain %d: the tiles were refused", id);
  if (st2) return;

  SqueezeChainIn in{n_planes, nl, lv, base_w, base_h, base_stride, out_stride, {}, {}, 0x40000000ull, n_planes == 3 && (rnd() & 1), false, true};
  for (int p = 0; p < n_planes; p++) {
    in.base[p] = (uintptr_t)base[p];
    in.out[p] = (uintptr_t)out[p];
  }
  const SqueezePreviewPlan P = plan_squeeze_preview(in, tl);

  // ---- kinds by definition, and what "mixed" means
  std::vector<std::vector<uint8_t>> kinds(nl);
  bool mixed = false;
  std::vector<uint8_t> cellwise(nl, 0);
  jxlh_squeeze_level folded[kSqueezeMaxLevels];  // res[] cleared where every cell is missing
  std::memcpy(folded, lv, sizeof folded);
  int first_missing = nl;
  for (int i = 0; i < nl; i++) {
    const SqTileGrid g = squeeze_tile_grid(lv[i], tl[i]);
    kinds[i].resize((size_t)g.nx * g.ny);
    squeeze_tile_kinds(n_planes, lv, tl, i, kinds[i].data());
    bool any_r = false, any_s = false;
    const bool has_res = squeeze_extents(lv[i].horizontal != 0, lv[i].out_w, lv[i].out_h).has_res;
    for (uint32_t ty = 0; ty < g.ny; ty++)
      for (uint32_t tx = 0; tx < g.nx; tx++) {
        const bool missing = has_res && (!lv[i].res[0] || (tl[i].present && !tl[i].present[ty * g.nx + tx]));
        const uint8_t k = kinds[i][ty * g.nx + tx];
        CHECK((k == JXLH_PREVIEW_REGULAR) == !missing, "chain %d level %d cell %u %u: kind %d, missing %d", id, i, tx, ty, k, missing);
        if (k == JXLH_PREVIEW_SMOOTH_2D) {
          CHECK(i > 0 && (lv[i - 1].horizontal != 0) != (lv[i].horizontal != 0), "chain %d level %d: 2-D without a crossed level", id, i);
          if (i > 0) {
            const SqTileGrid g1 = squeeze_tile_grid(lv[i - 1], tl[i - 1]);
            const uint32_t px = lv[i].horizontal ? tx * g.tw / 2 : tx * g.tw, py = lv[i].horizontal ? ty * g.th : ty * g.th / 2;
            CHECK(px < lv[i - 1].out_w && py < lv[i - 1].out_h, "chain %d level %d: mapped position outside", id, i);
            CHECK(kinds[i - 1][std::min(py / g1.th, g1.ny - 1) * g1.nx + std::min(px / g1.tw, g1.nx - 1)] != JXLH_PREVIEW_REGULAR,
                  "chain %d level %d: 2-D over a present cell", id, i);
          }
        }
        (missing ? any_s : any_r) = true;
      }
    if (any_r && any_s) mixed = true;
    for (uint8_t k : kinds[i]) cellwise[i] = cellwise[i] || k != kinds[i][0];  // (1-D beside 2-D: level i - 1 is mixed)
    // a smooth cell without a complete pair on a doubled axis is zero: the level goes cell by cell
    bool ragged = false;
    for (uint32_t ty = 0; ty < g.ny; ty++)
      for (uint32_t tx = 0; tx < g.nx; tx++) {
        const uint8_t k = kinds[i][ty * g.nx + tx];
        const uint32_t cw_ = std::min(g.tw, lv[i].out_w - tx * g.tw), ch_ = std::min(g.th, lv[i].out_h - ty * g.th);
        const bool fx = k == JXLH_PREVIEW_SMOOTH_2D || lv[i].horizontal, fy = k == JXLH_PREVIEW_SMOOTH_2D || !lv[i].horizontal;
        if (k != JXLH_PREVIEW_REGULAR && ((fx && cw_ < 2) || (fy && ch_ < 2))) ragged = true;
      }
    if (ragged) mixed = true;
    cellwise[i] = cellwise[i] || ragged;
    if (any_s && first_missing == nl) first_missing = i;
    if (!any_r)
      for (int p = 0; p < 3; p++) folded[i].res[p] = nullptr;
    CHECK(P.kind[i] == (cellwise[i] ? -1 : (int)kinds[i][0]), "chain %d level %d: kind %d", id, i, P.kind[i]);
  }
  bool any_cellwise = false;
  for (int i = 0; i < nl; i++) any_cellwise = any_cellwise || cellwise[i];
  CHECK(any_cellwise == mixed, "chain %d: a cell-wise level %d, mixed %d", id, any_cellwise, mixed);
  if (!mixed) {
    // no level goes cell by cell: the plan is the plan without grids of the folded chain
    SqueezeChainIn fin = in;
    fin.levels = folded;
    check_same_plan(id, P, plan_squeeze_preview(fin, nullptr), nl);
    CHECK(P.records.empty(), "chain %d: a plan without a cell-wise level", id);
    g_equal++;
  } else {
    g_mixed++;
  }
  CHECK(P.n_prefix == first_missing, "chain %d: prefix %d, first level with a missing cell %d", id, P.n_prefix, first_missing);
  CHECK(P.n_prefix == 0 || P.n_prefix == nl || (!P.prefix_in.with_rct && P.prefix_in.n_levels == P.n_prefix), "chain %d: the prefix", id);

  // ---- need: the last level, and what a needed level reads
  std::vector<uint8_t> need(nl, 0);
  need[nl - 1] = 1;
  for (int i = nl - 1; i >= 0; i--) {
    if (!need[i]) continue;
    for (uint8_t k : kinds[i]) {
      if (k == JXLH_PREVIEW_SMOOTH_2D) { if (i >= 2) need[i - 2] = 1; }
      else if (i >= 1) need[i - 1] = 1;
    }
  }
  for (int i = 0; i < nl; i++) CHECK(P.live[i] == need[i], "chain %d level %d: live %d", id, i, P.live[i]);
  // some entry goes cell by cell exactly when a cell-wise level is needed (one may be dead)
  bool plan_mixed = false, want_mixed = false;
  for (int k = 0; k < P.n; k++) plan_mixed = plan_mixed || P.entry[k].kind < 0;
  for (int i = 0; i < nl; i++) want_mixed = want_mixed || (need[i] && cellwise[i]);
  CHECK(plan_mixed == want_mixed, "chain %d: mixed %d, want %d", id, plan_mixed, want_mixed);
  int e_at = 0;
  size_t records = 0;
  bool written[kSqueezeMaxLevels] = {};
  for (int i = 0; i < P.n_prefix; i++) written[i] = true;
  bool behind_cellwise = false;
  for (int i = 0; i < nl; i++) {
    if (i < P.n_prefix) { CHECK(need[i], "chain %d: prefix level %d is not needed", id, i); continue; }
    if (!need[i]) {
      CHECK(e_at >= P.n || P.entry[e_at].level != i, "chain %d: an entry for dead level %d", id, i);
      continue;
    }
    CHECK(e_at < P.n && P.entry[e_at].level == i, "chain %d: no entry for level %d", id, i);
    if (e_at >= P.n || P.entry[e_at].level != i) return;  // (the checks below index by the level's own grid)
    const PreviewEntry& e = P.entry[e_at++];
    const bool hz = lv[i].horizontal != 0;
    const uint32_t ow = lv[i].out_w, oh = lv[i].out_h;
    CHECK(e.dst.where == (i == nl - 1 ? (int)kSqOut : i) && e.src.where == (i == 0 ? (int)kSqBase : i - 1) &&
              e.src2.where == (i <= 1 ? (int)kSqBase : i - 2), "chain %d level %d: planes", id, i);
    CHECK(e.rct == (i == nl - 1 && in.with_rct), "chain %d level %d: rct", id, i);
    const uint8_t k0 = kinds[i][0];
    const bool uniform = !cellwise[i];
    CHECK(e.kind == (uniform ? (int)k0 : -1), "chain %d level %d: kind %d", id, i, e.kind);
    if (uniform) {  // a whole level: what a plan without grids is held to
      check_whole_entry(id, in, e, P.n_prefix, written);
      written[i] = true;
      if (behind_cellwise) (k0 == JXLH_PREVIEW_REGULAR ? g_whole_regular : g_whole_smooth)++;
      continue;
    }
    written[i] = true;
    behind_cellwise = true;
    const SqTileGrid g = e.grid;
    const SqTileGrid want_g = squeeze_tile_grid(lv[i], tl[i]);
    CHECK(g.tw == want_g.tw && g.th == want_g.th && g.nx == want_g.nx && g.ny == want_g.ny, "chain %d level %d: grid", id, i);
    CHECK(e.smooth_off + e.n_smooth == e.runs_off && e.runs_off + e.n_runs <= P.records.size(), "chain %d level %d: lists outside the records", id, i);
    if (e.runs_off + e.n_runs > P.records.size() || e.smooth_off > e.runs_off) return;
    std::vector<int> covered(kinds[i].size(), 0);
    for (uint32_t j = 0; j < e.n_smooth; j++) {
      const SqTileSmoothCell& c = P.records[e.smooth_off + j].cell;
      const uint32_t tx = (uint32_t)c.x0 / g.tw, ty = (uint32_t)c.y0 / g.th;
      const int w_ = c.w, h_ = c.h_kind >> 2;
      CHECK((uint32_t)c.x0 == tx * g.tw && (uint32_t)c.y0 == ty * g.th && tx < g.nx && ty < g.ny, "chain %d level %d: a cell off the grid", id, i);
      if (tx >= g.nx || ty >= g.ny) continue;
      CHECK(w_ > 0 && h_ > 0 && (uint32_t)(c.x0 + w_) <= ow && (uint32_t)(c.y0 + h_) <= oh, "chain %d level %d: a cell outside the plane", id, i);
      CHECK((uint32_t)w_ == std::min(g.tw, ow - c.x0) && (uint32_t)h_ == std::min(g.th, oh - c.y0), "chain %d level %d: a cell's size", id, i);
      CHECK((c.h_kind & 3) == kinds[i][ty * g.nx + tx] && (c.h_kind & 3) != JXLH_PREVIEW_REGULAR, "chain %d level %d: a cell's kind", id, i);
      covered[ty * g.nx + tx]++;
      // the workgroups of the launch reach the whole cell
      const bool two_d = (c.h_kind & 3) == JXLH_PREVIEW_SMOOTH_2D;
      const uint32_t nx = two_d || hz ? (w_ + 1) / 2 : w_, ny = two_d || !hz ? (h_ + 1) / 2 : h_;
      CHECK(nx <= e.tiles_x * JXLH_SQC_TX && ny <= (e.tiles_per_cell / e.tiles_x) * JXLH_SQC_TY, "chain %d level %d: tiles per cell", id, i);
      g_smooth++;
    }
    const uint32_t len = hz ? ow : oh, lines = hz ? oh : ow, n_avg = len - len / 2;
    const size_t out_str = e.dst.stride, res_str = lv[i].res_stride, avg_str = e.src.stride;
    CHECK(out_str >= ow && avg_str >= (hz ? n_avg : ow), "chain %d level %d: strides", id, i);
    for (uint32_t j = 0; j < e.n_runs; j++) {
      const SqTileRun& r = P.records[e.runs_off + j].run;
      const uint32_t n_lines = (uint32_t)r.n_lines_tail >> 1;
      const bool tail = r.n_lines_tail & 1;
      const uint32_t s0 = 2 * (uint32_t)r.pair0, s1 = s0 + 2 * (uint32_t)r.n_pairs + tail;
      const uint32_t t_along = hz ? g.tw : g.th, t_across = hz ? g.th : g.tw, n_along = hz ? g.nx : g.ny;
      CHECK(r.pair0 >= 0 && r.n_pairs >= 0 && r.line0 >= 0 && n_lines > 0 && s1 <= len && (uint32_t)r.line0 + n_lines <= lines,
            "chain %d level %d: a run outside the plane", id, i);
      CHECK(tail == ((len & 1) && s1 == len), "chain %d level %d: tail", id, i);
      CHECK(s0 % t_along == 0 && (s1 % t_along == 0 || s1 == len) && (uint32_t)r.line0 % t_across == 0 && n_lines <= e.groups_per_run * JXLH_SQC_LINES &&
                n_lines == std::min(t_across, lines - r.line0), "chain %d level %d: a run off the grid", id, i);
      if (s1 > len || s0 % t_along) continue;
      const uint32_t c0 = s0 / t_along, c1 = (s1 + t_along - 1) / t_along, a = (uint32_t)r.line0 / t_across;
      auto at = [&](uint32_t c) { return hz ? a * g.nx + c : c * g.nx + a; };
      CHECK(c1 > c0, "chain %d level %d: an empty run", id, i);
      for (uint32_t c = c0; c < c1; c++) {
        CHECK(kinds[i][at(c)] == JXLH_PREVIEW_REGULAR, "chain %d level %d: a run over a smooth cell", id, i);
        covered[at(c)]++;
      }
      CHECK(c0 == 0 || kinds[i][at(c0 - 1)] != JXLH_PREVIEW_REGULAR, "chain %d level %d: a run that could start earlier", id, i);
      CHECK(c1 == n_along || kinds[i][at(c1)] != JXLH_PREVIEW_REGULAR, "chain %d level %d: a run that could go on", id, i);
      // the largest offsets the kernel forms: residuals of the run's own pairs, averages up to next_avg, the seed
      const size_t last_line = (size_t)r.line0 + n_lines - 1;
      if (r.n_pairs > 0) {
        const size_t last_pair = (size_t)r.pair0 + r.n_pairs - 1, next = std::min<size_t>(last_pair + 1, n_avg - 1);
        const SqueezeExtents x = squeeze_extents(hz, ow, oh);
        CHECK(last_pair < (hz ? x.res_w : x.res_h) && last_line < (hz ? x.res_h : x.res_w), "chain %d level %d: residual outside", id, i);
        CHECK((hz ? last_line * res_str + last_pair : last_pair * res_str + last_line) < res_str * x.res_h, "chain %d level %d: residual offset", id, i);
        CHECK((hz ? last_line * avg_str + next : next * avg_str + last_line) < avg_str * x.avg_h, "chain %d level %d: average offset", id, i);
      }
      CHECK((hz ? last_line * out_str + (s1 - 1) : (size_t)(s1 - 1) * out_str + last_line) < out_str * oh, "chain %d level %d: output offset", id, i);
      g_runs++;
    }
    for (size_t c = 0; c < covered.size(); c++) CHECK(covered[c] == 1, "chain %d level %d: cell %zu is in %d lists", id, i, c, covered[c]);
    CHECK(e.smooth_off == records && e.runs_off == records + e.n_smooth, "chain %d level %d: list offsets", id, i);
    records += (size_t)e.n_smooth + e.n_runs;
  }
  CHECK(e_at == P.n && records == P.records.size(), "chain %d: entries %d of %d, records %zu of %zu", id, e_at, P.n, records, P.records.size());
}

}  // namespace

int main() {
  // the tile tests' geometries, a few densities each
  const struct { uint32_t w, h, tw, th; int nl; bool finest_hz; } geo[] = {
      {40, 24, 8, 8, 5, true}, {33, 29, 16, 8, 5, true}, {200, 70, 32, 96, 9, true}, {600, 40, 256, 40, 6, true}, {24, 600, 40, 256, 6, false}};
  int id = 0;
  for (const auto& g : geo)
    for (int rep = 0; rep < 400; rep++) one_chain(id++, g.w, g.h, g.nl, g.finest_hz, g.tw, g.th, 3, 20 + 20 * (rep % 4), false);
  // random chains, grids and masks
  for (int rep = 0; rep < 20000; rep++) {
    const uint32_t big = rep % 11 == 0 ? 700 : 90;
    one_chain(id++, rnd(1, big), rnd(1, big), (int)rnd(1, 8), rnd() & 1, rep % 9 == 0 ? 0 : rnd(1, 40), rep % 9 == 0 ? 0 : rnd(1, 40), (int)rnd(1, 8),
              rnd(5, 95), rep % 3 == 0);
  }
  // refusals
  {
    jxlh_squeeze_level lv{};
    lv.horizontal = 1;
    lv.out_w = 40;
    lv.out_h = 24;
    jxlh_squeeze_tiles t{8, 8, nullptr};
    CHECK(check_squeeze_tiles(1, &lv, &t) == JXLH_OK, "a plain grid");
    CHECK(check_squeeze_tiles(1, &lv, nullptr) == JXLH_ERR_INVALID_ARGUMENT, "no tiles");
    t = {8, 0, nullptr};
    CHECK(check_squeeze_tiles(1, &lv, &t) == JXLH_ERR_INVALID_ARGUMENT, "one of the two zero");
    t = {7, 8, nullptr};
    CHECK(check_squeeze_tiles(1, &lv, &t) == JXLH_ERR_INVALID_ARGUMENT, "an odd tile_w");
    t = {41, 7, nullptr};
    CHECK(check_squeeze_tiles(1, &lv, &t) == JXLH_OK, "one odd cell column");
    lv.out_w = lv.out_h = 4096;
    t = {2, 2, nullptr};
    CHECK(check_squeeze_tiles(1, &lv, &t) == JXLH_ERR_INVALID_ARGUMENT, "2^22 cells");
    t = {4, 4, nullptr};
    CHECK(check_squeeze_tiles(1, &lv, &t) == JXLH_OK, "2^20 cells");
  }
  if (g_fail) {
    std::printf("%d failures\n", g_fail);
    return 1;
  }
  std::printf("squeeze tile plans: ok (%d chains, %d mixed, %d smooth cells, %d runs; %d equal to the plan without grids; behind a cell-wise "
              "level %d whole smooth and %d whole regular entries)\n", id, g_mixed, g_smooth, g_runs, g_equal, g_whole_smooth, g_whole_regular);
  return g_mixed > 1000 && g_runs > 1000 && g_smooth > 1000 && g_equal >= 1000 && g_whole_smooth >= 1000 && g_whole_regular >= 1000 ? 0 : 1;
}
