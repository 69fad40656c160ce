// The plan of the extra channels' rect form (jxl_rs_amd/csrc/ec_rects_plan.h) against a brute-force per-sample model,
// over random channel sizes (1, and both sides of every tile and piece seam), factors and rect lists (1 x 1, on the
// edges, overlapping, empty):
//   * mark: every source sample within a rect widened by the upsampling's reach lies in a dirty tile, and a tile that
//     holds no such sample is clean;
//   * collect: each dirty tile once, grouped by factor, channels and tiles ascending, every bitmap clean afterwards;
//   * the scatter layout, walked the way k_ec_scatter walks it (bisection for the rect, pieces, four samples per lane,
//     16-byte accesses only where both addresses are aligned): every sample of the union holds a sample of a rect that
//     covers it, nothing else is written, nothing outside the block is read;
//   * the rule of jxlh_extra_channel_changed_rects: no output sample whose 5 x 5 mirrored window reads a changed sample
//     lies outside the returned rect;
//   * every argument error with its status and first_bad, at the wrap of 32 and 64 bits too.
// Host only, no device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../jxl_rs_amd/csrc/ec_rects_plan.h"

namespace {

using namespace jxlh;

int g_fail = 0;
long g_cases = 0;
#define CHECK(c, ...)                          \
  do {                                         \
    if (!(c)) {                                \
      if (g_fail++ < 20) {                     \
        std::printf("FAIL %s: ", #c);          \
        std::printf(__VA_ARGS__);              \
        std::printf("\n");                     \
      }                                        \
    }                                          \
  } while (0)

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 32);
}
uint32_t rnd(uint32_t lo, uint32_t hi) { return lo + rnd() % (hi - lo + 1); }  // inclusive

uint32_t pick_size(uint32_t tile) {
  const uint32_t seams[] = {1, 2, 3, 4, 5, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1, 3 * tile + 2};
  return rnd() % 3 ? seams[rnd() % (sizeof seams / sizeof *seams)] : rnd(1, 4 * tile + 9);
}

jxlh_rect pick_rect(uint32_t w, uint32_t h) {
  jxlh_rect r;
  switch (rnd() % 6) {
    case 0: r = {rnd(0, w - 1), rnd(0, h - 1), 1, 1}; break;               // 1 x 1
    case 1: r = {0, rnd(0, h - 1), w, 1}; break;                            // a full row
    case 2: r = {w - 1, 0, 1, h}; break;                                    // the last column
    case 3: r = {0, 0, rnd(1, w), rnd(1, h)}; break;                        // the first corner
    case 4: {                                                               // ends at the last sample
      const uint32_t rw = rnd(1, w), rh = rnd(1, h);
      r = {w - rw, h - rh, rw, rh};
      break;
    }
    default: {
      const uint32_t x0 = rnd(0, w - 1), y0 = rnd(0, h - 1);
      r = {x0, y0, rnd(1, w - x0), rnd(1, h - y0)};
    }
  }
  return r;
}

long mirror(long v, long s) {  // util/mirror.rs
  while (v < 0 || v >= s) v = v < 0 ? -v - 1 : 2 * s - v - 1;
  return v;
}

// ---- mark + collect
void test_dirty_tiles() {
  for (int iter = 0; iter < 60000; iter++, g_cases++) {
    EcRectsPlan plan;
    struct Model { uint32_t w, h, up; std::vector<uint8_t> need; };
    Model model[JXLH_MAX_EXTRA_CHANNELS] = {};
    const uint32_t nch = rnd(1, 3);
    uint32_t used[JXLH_MAX_EXTRA_CHANNELS] = {};
    for (uint32_t k = 0; k < nch; k++) {
      const uint32_t ec = rnd(0, JXLH_MAX_EXTRA_CHANNELS - 1);
      if (used[ec]) continue;
      used[ec] = 1;
      Model& m = model[ec];
      m.w = pick_size(kEcTileW), m.h = pick_size(kEcTileH), m.up = 1u << rnd(0, 3);
      m.need.assign((size_t)m.w * m.h, 0);
      EcGrid& g = plan.ch[ec];
      g.reset(m.w, m.h, m.up);
      CHECK(g.active() && g.n_dirty == 0, "reset");
      const uint32_t nr = rnd(0, 5);
      const long reach = m.up > 1 ? 2 : 0;
      for (uint32_t i = 0; i < nr; i++) {
        const jxlh_rect r = pick_rect(m.w, m.h);
        g.mark(r.x0, r.y0, r.w, r.h);
        for (long y = 0; y < (long)m.h; y++)
          for (long x = 0; x < (long)m.w; x++)
            if (x >= (long)r.x0 - reach && x < (long)r.x0 + (long)r.w + reach && y >= (long)r.y0 - reach &&
                y < (long)r.y0 + (long)r.h + reach)
              m.need[(size_t)y * m.w + x] = 1;
      }
    }
    // the bitmap against the model, tile by tile
    uint64_t want_items[4] = {0, 0, 0, 0};
    for (uint32_t ec = 0; ec < JXLH_MAX_EXTRA_CHANNELS; ec++) {
      if (!used[ec]) continue;
      const Model& m = model[ec];
      const EcGrid& g = plan.ch[ec];
      CHECK(g.ntx == (m.w + kEcTileW - 1) / kEcTileW && g.nty == (m.h + kEcTileH - 1) / kEcTileH, "grid %u x %u", m.w, m.h);
      uint64_t dirty = 0;
      for (uint32_t ty = 0; ty < g.nty; ty++)
        for (uint32_t tx = 0; tx < g.ntx; tx++) {
          bool any = false;
          for (uint32_t y = ty * kEcTileH; y < std::min(m.h, (ty + 1) * kEcTileH); y++)
            for (uint32_t x = tx * kEcTileW; x < std::min(m.w, (tx + 1) * kEcTileW); x++) any |= m.need[(size_t)y * m.w + x] != 0;
          CHECK(g.test((uint64_t)ty * g.ntx + tx) == any, "channel %u (%u x %u, x%u) tile (%u, %u): dirty %d, model %d", ec, m.w,
                m.h, m.up, tx, ty, (int)g.test((uint64_t)ty * g.ntx + tx), (int)any);
          dirty += any;
        }
      CHECK(g.n_dirty == dirty && plan.dirty(ec) == (dirty != 0), "n_dirty %llu, model %llu", (unsigned long long)g.n_dirty,
            (unsigned long long)dirty);
      for (int k = 0; k < 4; k++)
        if (m.up == (1u << k)) want_items[k] += dirty;
    }
    std::vector<EcGrid> before(plan.ch, plan.ch + JXLH_MAX_EXTRA_CHANNELS);
    std::vector<EcItem> items;
    uint32_t first[5];
    plan.collect(items, first);
    CHECK(first[0] == 0 && first[4] == items.size(), "first[]");
    for (int k = 0; k < 4; k++) {
      CHECK(first[k + 1] - first[k] == want_items[k], "factor %d: %u items, model %llu", 1 << k, first[k + 1] - first[k],
            (unsigned long long)want_items[k]);
      for (uint32_t i = first[k]; i < first[k + 1]; i++) {
        const EcItem& it = items[i];
        CHECK(it.ec < JXLH_MAX_EXTRA_CHANNELS && used[it.ec] && model[it.ec].up == (1u << k), "item %u: channel %u", i, it.ec);
        if (it.ec >= JXLH_MAX_EXTRA_CHANNELS || !used[it.ec]) continue;
        CHECK(it.tile < (uint64_t)before[it.ec].ntx * before[it.ec].nty && before[it.ec].test(it.tile), "item %u: tile %u is clean", i,
              it.tile);
        if (i > first[k])  // ascending: no tile twice
          CHECK(items[i - 1].ec < it.ec || (items[i - 1].ec == it.ec && items[i - 1].tile < it.tile), "item %u out of order", i);
      }
    }
    for (uint32_t ec = 0; ec < JXLH_MAX_EXTRA_CHANNELS; ec++) {
      const EcGrid& g = plan.ch[ec];
      CHECK(g.n_dirty == 0 && !plan.dirty(ec), "channel %u not clean after collect", ec);
      for (uint64_t v : g.bits) CHECK(v == 0, "channel %u: bits left", ec);
    }
    plan.collect(items, first);
    CHECK(items.empty(), "a second collect lists %zu tiles", items.size());
  }
}

// ---- the scatter layout, walked like the kernel
void test_scatter() {
  for (int iter = 0; iter < 25000; iter++, g_cases++) {
    EcCallState s;
    s.in_frame = true;
    std::vector<int64_t> plane[JXLH_MAX_EXTRA_CHANNELS];
    const uint32_t nch = rnd(1, 2);
    for (uint32_t ec = 0; ec < nch; ec++) {
      s.ch[ec].set = true;
      s.ch[ec].w = rnd() % 2 ? pick_size(kEcPieceW) : pick_size(8);
      s.ch[ec].h = rnd() % 2 ? pick_size(kEcPieceH) : pick_size(4);
      plane[ec].assign((size_t)s.ch[ec].w * s.ch[ec].h, -1);
    }
    const uint32_t n = rnd(0, 5);
    std::vector<jxlh_ec_rect> rects(n);
    uint64_t off = rnd(0, 7), n_samples = 0;
    for (uint32_t i = 0; i < n; i++) {
      jxlh_ec_rect& r = rects[i];
      r.ec = rnd(0, nch - 1);
      const jxlh_rect q = pick_rect(s.ch[r.ec].w, s.ch[r.ec].h);
      r.x0 = q.x0, r.y0 = q.y0, r.w = q.w, r.h = q.h;
      if (rnd() % 8 == 0) (rnd() % 2 ? r.w : r.h) = 0;  // an empty rect, skipped
      r.stride = r.w + (rnd() % 3 ? 0 : rnd(0, 9));
      r.offset = off;
      if (r.w && r.h) {
        off += ec_rect_extent(r) + rnd(0, 5);
        n_samples = std::max(n_samples, r.offset + ec_rect_extent(r));
      }
    }
    n_samples += rnd(0, 3);
    uint32_t bad = 77;
    std::string why;
    CHECK(check_ec_rects(s, true, n_samples, rects.data(), n, &bad, &why) == JXLH_OK && bad == 77, "a valid list is refused: %s",
          why.c_str());
    const bool staged = rnd() % 2;
    const uint64_t block_addr = 4096 + 4 * (uint64_t)rnd(0, 3);  // the caller's block: 4-byte aligned, no more
    const EcScatterPlan p = plan_ec_scatter(s, rects.data(), n, staged, block_addr);
    // the source the kernel reads: the staged span at a 16-byte aligned base, or the block in place
    const uint64_t src_addr = staged ? 8192 : block_addr, src_n = staged ? p.span_hi - p.span_lo : n_samples;
    if (staged && !p.descs.empty()) CHECK(p.span_lo % 4 == 0 && p.span_hi <= n_samples && p.span_lo <= p.span_hi, "span");
    uint64_t next = 0;
    for (const EcScatterDesc& d : p.descs) {
      CHECK(d.first == next && d.npx == (d.w + kEcPieceW - 1) / kEcPieceW, "first / npx");
      next += (uint64_t)d.npx * ((d.h + kEcPieceH - 1) / kEcPieceH);
    }
    CHECK(next == p.pieces, "pieces");
    for (uint64_t g = 0; g < p.pieces; g++) {
      uint32_t lo = 0, hi = (uint32_t)p.descs.size();
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (p.descs[mid].first <= g) lo = mid;
        else hi = mid;
      }
      const EcScatterDesc& d = p.descs[lo];
      const uint64_t piece = g - d.first;
      const uint32_t px = (uint32_t)(piece % d.npx), py = (uint32_t)(piece / d.npx);
      for (uint32_t tid = 0; tid < 256; tid++) {
        const uint32_t x = px * kEcPieceW + (tid & 63u) * 4u;
        if (x >= d.w) continue;
        for (uint32_t j = 0; j < kEcPieceH / 4; j++) {
          const uint32_t y = py * kEcPieceH + (tid >> 6) + 4u * j;
          if (y >= d.h) break;
          const uint64_t si = d.src_off + (uint64_t)y * d.src_stride + x, ti = d.dst_off + (uint64_t)y * d.dst_stride + x;
          const bool vec = d.vec && x + 4u <= d.w;
          if (vec) CHECK((src_addr + 4 * si) % 16 == 0 && (4 * ti) % 16 == 0, "a 16-byte access at an unaligned address");
          for (uint32_t i = 0; i < 4; i++) {
            if (!vec && x + i >= d.w) continue;
            CHECK(si + i < src_n && ti + i < plane[d.ec].size(), "out of bounds: src %llu of %llu, dst %llu of %zu",
                  (unsigned long long)(si + i), (unsigned long long)src_n, (unsigned long long)(ti + i), plane[d.ec].size());
            if (si + i < src_n && ti + i < plane[d.ec].size())
              plane[d.ec][ti + i] = (int64_t)(si + i + (staged ? p.span_lo : 0));  // the sample's index in the caller's block
          }
        }
      }
    }
    // every sample of the union holds a block sample of a rect that covers it; nothing else was written
    for (uint32_t ec = 0; ec < nch; ec++)
      for (uint32_t y = 0; y < s.ch[ec].h; y++)
        for (uint32_t x = 0; x < s.ch[ec].w; x++) {
          const int64_t got = plane[ec][(size_t)y * s.ch[ec].w + x];
          bool covered = false, match = false;
          for (const jxlh_ec_rect& r : rects) {
            if (r.ec != ec || !r.w || !r.h || x < r.x0 || x >= r.x0 + r.w || y < r.y0 || y >= r.y0 + r.h) continue;
            covered = true;
            match |= got == (int64_t)(r.offset + (uint64_t)(y - r.y0) * r.stride + (x - r.x0));
          }
          CHECK(covered ? match : got == -1, "channel %u sample (%u, %u): covered %d, holds %lld", ec, x, y, (int)covered,
                (long long)got);
        }
  }
}

// ---- the rule of jxlh_extra_channel_changed_rects
void test_changed_rects() {
  for (int iter = 0; iter < 25000; iter++, g_cases++) {
    const uint32_t w = pick_size(8), h = pick_size(4), up = 1u << rnd(0, 3);
    const uint32_t res_w = rnd() % 2 ? w * up : rnd(std::max(1u, (w - 1) * up), w * up + 3);
    const uint32_t res_h = rnd() % 2 ? h * up : rnd(std::max(1u, (h - 1) * up), h * up + 3);
    const uint32_t out_w = std::min(w * up, res_w), out_h = std::min(h * up, res_h);
    const jxlh_rect r = pick_rect(w, h);
    std::vector<jxlh_rect> out;
    jxlh_rect src[2] = {r, {w + 5, 3, 0, 9}};
    CHECK(plan_ec_changed_rects(w, h, up, res_w, res_h, src, 2, out) == JXLH_OK && out.size() == 2, "status");
    if (out.size() != 2) continue;
    CHECK(out[1].x0 == 0 && out[1].y0 == 0 && out[1].w == 0 && out[1].h == 0, "an empty rect gives an empty rect");
    const jxlh_rect q = out[0];
    CHECK((uint64_t)q.x0 + q.w <= out_w && (uint64_t)q.y0 + q.h <= out_h, "the rect leaves the finished channel");
    // the source pixels whose mirrored window reads a sample of the rect, per axis
    auto affected = [&](long p, long size, long lo, long n) {
      if (up == 1) return p >= lo && p < lo + n;
      for (long k = -2; k <= 2; k++) {
        const long v = mirror(p + k, size);
        if (v >= lo && v < lo + n) return true;
      }
      return false;
    };
    long xa = -1, xb = -1, ya = -1, yb = -1;  // bounding box of the affected OUTPUT samples
    for (long ox = 0; ox < (long)out_w; ox++)
      if (affected(ox / up, w, r.x0, r.w)) xa = xa < 0 ? ox : xa, xb = ox + 1;
    for (long oy = 0; oy < (long)out_h; oy++)
      if (affected(oy / up, h, r.y0, r.h)) ya = ya < 0 ? oy : ya, yb = oy + 1;
    if (xa < 0 || ya < 0) continue;  // all of it is cut off
    CHECK((long)q.x0 <= xa && xb <= (long)q.x0 + (long)q.w && (long)q.y0 <= ya && yb <= (long)q.y0 + (long)q.h,
          "%u x %u x%u rect (%u, %u, %u, %u): changed [%ld, %ld) x [%ld, %ld) outside (%u, %u, %u, %u)", w, h, up, r.x0, r.y0, r.w, r.h,
          xa, xb, ya, yb, q.x0, q.y0, q.w, q.h);
    // ... and the rule is exact per axis: mirroring only folds the window back onto samples it reads anyway
    CHECK((long)q.x0 == xa && (long)q.x0 + (long)q.w == xb && (long)q.y0 == ya && (long)q.y0 + (long)q.h == yb, "the rule is not tight");
  }
  std::vector<jxlh_rect> out;
  const jxlh_rect one = {0, 0, 1, 1};
  CHECK(plan_ec_changed_rects(0, 4, 1, 4, 4, &one, 1, out) == JXLH_ERR_INVALID_ARGUMENT, "w == 0");
  CHECK(plan_ec_changed_rects(4, 0, 1, 4, 4, &one, 1, out) == JXLH_ERR_INVALID_ARGUMENT, "h == 0");
  CHECK(plan_ec_changed_rects(4, 4, 1, 0, 4, &one, 1, out) == JXLH_ERR_INVALID_ARGUMENT, "res_w == 0");
  CHECK(plan_ec_changed_rects(4, 4, 1, 4, 0, &one, 1, out) == JXLH_ERR_INVALID_ARGUMENT, "res_h == 0");
  for (uint32_t up : {0u, 3u, 5u, 6u, 16u}) CHECK(plan_ec_changed_rects(4, 4, up, 4, 4, &one, 1, out) == JXLH_ERR_INVALID_ARGUMENT, "factor");
  CHECK(plan_ec_changed_rects(4, 4, 2, 8, 8, nullptr, 1, out) == JXLH_ERR_INVALID_ARGUMENT, "src == NULL");
  CHECK(plan_ec_changed_rects(4, 4, 2, 8, 8, nullptr, 0, out) == JXLH_OK && out.empty(), "no rects");
  const jxlh_rect leaves[] = {{4, 0, 1, 1}, {0, 4, 1, 1}, {3, 0, 2, 1}, {0, 3, 1, 2}, {0xffffffffu, 0, 2, 1}, {0, 0xffffffffu, 1, 2},
                              {1, 0, 0xffffffffu, 1}};
  for (const jxlh_rect& r : leaves) CHECK(plan_ec_changed_rects(4, 4, 2, 8, 8, &r, 1, out) == JXLH_ERR_INVALID_ARGUMENT, "a rect that leaves");
  g_cases += 20;
}

// ---- the argument checks of the rects call
void test_argument_errors() {
  EcCallState s;
  s.in_frame = true;
  s.ch[0].set = true, s.ch[0].w = 66, s.ch[0].h = 50;
  s.ch[3].set = true, s.ch[3].w = 0xffffffffu, s.ch[3].h = 1;  // (not a channel a context accepts: the wrap alone)
  const jxlh_ec_rect good = {0, 1, 1, 4, 4, 0, 4};
  const uint64_t N = 4096, M = ~0ull;
  struct Case { jxlh_ec_rect r; uint64_t n_samples; jxlh_status want; const char* what; };
  const Case cases[] = {
      {{8, 0, 0, 1, 1, 0, 1}, N, JXLH_ERR_INVALID_ARGUMENT, "ec out of range"},
      {{0xffffffffu, 0, 0, 0, 0, 0, 0}, N, JXLH_ERR_INVALID_ARGUMENT, "ec out of range on an empty rect"},
      {{1, 0, 0, 1, 1, 0, 1}, N, JXLH_ERR_BAD_STATE, "a channel that is not set"},
      {{0, 0, 0, 4, 4, 0, 3}, N, JXLH_ERR_INVALID_ARGUMENT, "stride < w"},
      {{0, 63, 0, 4, 1, 0, 4}, N, JXLH_ERR_INVALID_ARGUMENT, "x0 + w beyond the channel"},
      {{0, 0, 47, 1, 4, 0, 1}, N, JXLH_ERR_INVALID_ARGUMENT, "y0 + h beyond the channel"},
      {{0, 66, 0, 1, 1, 0, 1}, N, JXLH_ERR_INVALID_ARGUMENT, "x0 == w"},
      {{0, 0xffffffffu, 0, 2, 1, 0, 2}, N, JXLH_ERR_INVALID_ARGUMENT, "x0 + w wraps 32 bits"},
      {{0, 0, 0xffffffffu, 1, 2, 0, 1}, N, JXLH_ERR_INVALID_ARGUMENT, "y0 + h wraps 32 bits"},
      {{0, 2, 0, 0xffffffffu, 1, 0, 0xffffffffu}, M, JXLH_ERR_INVALID_ARGUMENT, "x0 + w wraps 32 bits (w)"},
      {{3, 0xfffffffeu, 0, 2, 1, 0, 2}, N, JXLH_ERR_INVALID_ARGUMENT, "x0 + w == 2^32 in a 2^32 - 1 wide channel"},
      {{0, 0, 0, 4, 4, N - 15, 4}, N, JXLH_ERR_INVALID_ARGUMENT, "one sample beyond n_samples"},
      {{0, 0, 0, 4, 4, 0, 1365}, N, JXLH_ERR_INVALID_ARGUMENT, "stride * (h - 1) + w beyond n_samples"},
      {{0, 0, 0, 4, 4, N + 1, 4}, N, JXLH_ERR_INVALID_ARGUMENT, "offset beyond n_samples"},
      {{0, 0, 0, 4, 4, M, 4}, N, JXLH_ERR_INVALID_ARGUMENT, "offset + extent wraps 64 bits"},
      {{0, 0, 0, 4, 4, M - 15, 4}, M, JXLH_ERR_INVALID_ARGUMENT, "offset + extent == 2^64"},
      {{0, 0, 0, 4, 50, 5, 0xffffffffu}, M, JXLH_OK, "stride * (h - 1) + w beyond 32 bits is no wrap"},
      {{0, 0, 0, 4, 4, M - 16, 4}, M, JXLH_OK, "offset + extent == n_samples == 2^64 - 1"},
      {{0, 0, 0, 4, 4, N - 16, 4}, N, JXLH_OK, "ends at the last sample"},
      {{0, 0, 0, 4, 4, 0, 1364}, N, JXLH_OK, "the last row ends at the last sample"},
      {{0, 65, 49, 1, 1, N - 1, 0xffffffffu}, N, JXLH_OK, "h == 1: the stride is not used"},
      {{0, 500, 500, 0, 7, M, 0}, 0, JXLH_OK, "an empty rect, wherever it starts"},
  };
  for (const Case& c : cases)
    for (int pos = 0; pos < 3; pos++, g_cases++) {  // alone, behind good rects, in front of a bad one
      std::vector<jxlh_ec_rect> list;
      for (int i = 0; i < pos; i++) list.push_back(good);
      list.push_back(c.r);
      if (pos == 2) list.push_back({9, 0, 0, 1, 1, 0, 1});
      const uint64_t ns = std::max<uint64_t>(c.n_samples, 16);
      uint32_t bad = 77;
      std::string why;
      jxlh_status want = c.want;
      uint32_t want_bad = (uint32_t)pos;
      if (want == JXLH_OK && pos == 2) want = JXLH_ERR_INVALID_ARGUMENT, want_bad = 3;
      const jxlh_status st = check_ec_rects(s, true, ns, list.data(), (uint32_t)list.size(), &bad, &why);
      CHECK(st == want, "%s (at %d): status %d, want %d", c.what, pos, (int)st, (int)want);
      CHECK(bad == (want == JXLH_OK ? 77u : want_bad), "%s (at %d): first_bad %u", c.what, pos, bad);
      CHECK(why.empty() == (want == JXLH_OK), "%s: the message", c.what);
      CHECK(check_ec_rects(s, true, ns, list.data(), (uint32_t)list.size(), nullptr, nullptr) == want, "%s: null outputs", c.what);
    }
  uint32_t bad = 77;
  std::string why;
  std::vector<jxlh_ec_rect> many(JXLH_MAX_EC_RECTS + 1, good);
  CHECK(check_ec_rects(s, true, N, many.data(), JXLH_MAX_EC_RECTS, &bad, &why) == JXLH_OK, "4096 rects");
  CHECK(check_ec_rects(s, true, N, many.data(), JXLH_MAX_EC_RECTS + 1, &bad, &why) == JXLH_ERR_INVALID_ARGUMENT, "4097 rects");
  CHECK(check_ec_rects(s, true, N, nullptr, 1, &bad, &why) == JXLH_ERR_INVALID_ARGUMENT, "rects == NULL");
  CHECK(check_ec_rects(s, false, N, &good, 1, &bad, &why) == JXLH_ERR_INVALID_ARGUMENT, "samples == NULL");
  CHECK(check_ec_rects(s, false, 0, nullptr, 0, &bad, &why) == JXLH_OK, "n == 0");
  CHECK(bad == 77 && why.empty(), "a refusal of the call names no rect");
  EcCallState out = s;
  out.in_frame = false;
  CHECK(check_ec_rects(out, true, N, &good, 1, &bad, &why) == JXLH_ERR_BAD_STATE, "outside a frame");
  CHECK(check_ec_rects(out, true, N, nullptr, 1, &bad, &why) == JXLH_ERR_INVALID_ARGUMENT, "... the arguments come first");
  EcCallState sh = s;
  sh.sharded = true;
  CHECK(check_ec_rects(sh, true, N, &good, 1, &bad, &why) == JXLH_ERR_UNSUPPORTED, "a sharded context");
  CHECK(bad == 77, "first_bad untouched");
  g_cases += 9;
}

}  // namespace

int main() {
  test_dirty_tiles();
  test_scatter();
  test_changed_rects();
  test_argument_errors();
  if (g_fail) {
    std::printf("ec rects plan: %d failures in %ld cases\n", g_fail, g_cases);
    return 1;
  }
  std::printf("ec rects plan: ok (%ld cases)\n", g_cases);
  return g_cases >= 100000 ? 0 : 1;
}
