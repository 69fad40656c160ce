// The squeeze chain's planner (jxl_rs_amd/csrc/squeeze_plan.h) against the expressions it replaced.  Those stood in the
// launchers of the kernel file and between the launches of jxlh_unsqueeze_chain, jxlh_unsqueeze_levels, jxlh_unsqueeze,
// jxlh_unsqueeze_planes and jxlh_unsqueeze_rct; they are transcribed below as they were, one function per place they came
// from, and none of them calls the header.  Plus the invariants of a plan.  Host only, no device: addresses are numbers.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../jxl_rs_amd/csrc/squeeze_plan.h"

using namespace jxlh;

namespace {

int g_fail = 0;
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

typedef const int32_t* cptr;
typedef int32_t* mptr;
cptr at(uintptr_t a) { return reinterpret_cast<cptr>(a); }

// ---- what a launch is, in addresses: the old code's launches and the plan's are both brought to this form
struct Rec {
  int kind, level0, n, vec, ncw;
  uintptr_t src[3], dst[3];
  size_t src_stride, dst_stride;
  std::vector<int> flow_vec;
  size_t flow_words;
};
constexpr int kLevels = 0, kFlow = 1, kTiled = 2, kOneWave = 3, kFusedRct = 4, kRctFlat = 5, kRctRows = 6;
static_assert((int)SqueezeLaunch::kLevels == kLevels && (int)SqueezeLaunch::kFlow == kFlow && (int)SqueezeLaunch::kTiled == kTiled &&
                  (int)SqueezeLaunch::kOneWave == kOneWave && (int)SqueezeLaunch::kFusedRct == kFusedRct &&
                  (int)SqueezeLaunch::kRctFlat == kRctFlat && (int)SqueezeLaunch::kRctRows == kRctRows,
              "the kinds by number");

// ---- k_modular.hip: tiled_vec_ok (without the JXLH_SQ_VEC hook)
int old_tiled_vec_ok(int horizontal, int n_planes, const cptr avg[], size_t avg_stride, const cptr res[], size_t res_stride,
                     uint32_t out_w, uint32_t out_h, const mptr out[], size_t out_stride) {
  if (avg_stride % 4 || res_stride % 4 || out_stride % 4) return 0;
  if (!horizontal && out_w % 4) return 0;
  for (int i = 0; i < n_planes && i < 3; i++)
    if ((uintptr_t)avg[i] % 16 || (uintptr_t)res[i] % 16 || (uintptr_t)out[i] % 16) return 0;
  const size_t lim = (size_t)1 << 30;
  return out_stride * (size_t)out_h < lim && avg_stride * (size_t)out_h < lim && res_stride * (size_t)out_h < lim;
}
// ---- k_modular.hip: launch_unsqueeze (which kernel, which variant)
Rec old_launch_unsqueeze(int horizontal, int n_planes, const cptr avg[], size_t avg_stride, const cptr res[], size_t res_stride,
                         uint32_t out_w, uint32_t out_h, const mptr out[], size_t out_stride) {
  Rec r{};
  r.n = 1;
  r.ncw = 1;
  bool aligned = (avg_stride % 4 == 0) && (res_stride % 4 == 0) && (out_stride % 4 == 0);
  for (int i = 0; i < n_planes && i < 3; i++)
    aligned = aligned && ((uintptr_t)avg[i] % 16 == 0) && ((uintptr_t)res[i] % 16 == 0) && ((uintptr_t)out[i] % 16 == 0);
  const int n_steps = (int)(horizontal ? out_w : out_h) / 2;
  const size_t span = out_stride * (size_t)out_h;
  if (n_steps >= 4 * 32 && span < ((size_t)1 << 31) && avg_stride * (size_t)out_h < ((size_t)1 << 31) &&
      res_stride * (size_t)out_h < ((size_t)1 << 31)) {
    r.kind = kTiled;
    r.vec = old_tiled_vec_ok(horizontal, n_planes, avg, avg_stride, res, res_stride, out_w, out_h, out, out_stride);
    return r;
  }
  r.kind = kOneWave;
  r.vec = horizontal ? (aligned ? 1 : 0) : 0;
  return r;
}
// ---- k_modular.hip: unsqueeze_tiled_eligible
bool old_tiled_eligible(int horizontal, uint32_t out_w, uint32_t out_h, size_t avg_stride, size_t res_stride, size_t out_stride) {
  const int n_steps = (int)(horizontal ? out_w : out_h) / 2;
  const size_t lim = (size_t)1 << 31;
  return n_steps >= 4 * 32 && out_stride * (size_t)out_h < lim && avg_stride * (size_t)out_h < lim &&
         res_stride * (size_t)out_h < lim;
}
// ---- k_modular.hip: launch_unsqueeze_rct (false: nothing launched)
bool old_launch_unsqueeze_rct(int horizontal, const cptr avg[3], size_t avg_stride, const cptr res[3], size_t res_stride,
                              uint32_t out_w, uint32_t out_h, const mptr out[3], size_t out_stride, Rec* r) {
  const size_t lim = (size_t)1 << 31;
  if (out_stride * (size_t)out_h >= lim || avg_stride * (size_t)out_h >= lim || res_stride * (size_t)out_h >= lim) return false;
  *r = Rec{};
  r->kind = kFusedRct;
  r->n = 1;
  r->ncw = 1;
  if (!horizontal) {
    bool vec = out_w % 4 == 0 && avg_stride % 4 == 0 && res_stride % 4 == 0 && out_stride % 4 == 0;
    for (int i = 0; i < 3; i++)
      vec = vec && ((uintptr_t)avg[i] % 16 == 0) && ((uintptr_t)res[i] % 16 == 0) && ((uintptr_t)out[i] % 16 == 0);
    r->vec = vec;
    if (vec && out_w >= 4096 && out_w % 32 == 0) r->ncw = 2;
  }
  return true;
}
// ---- k_modular.hip: launch_unsqueeze_levels (its return value)
bool old_launch_unsqueeze_levels(int n_planes, int n_levels, const int* horizontal, const uint32_t* out_w, const uint32_t* out_h,
                                 uint32_t base_w, uint32_t base_h) {
  if (n_levels < 1 || n_levels > 16 || n_planes < 1 || n_planes > 3) return false;
  if (base_w == 0 || base_h == 0 || base_w > 128 || base_h > 128) return false;
  for (int i = 0; i < n_levels; i++)
    if (out_w[i] == 0 || out_h[i] == 0 || out_w[i] > 128 || out_h[i] > 128) return false;
  const size_t half_cap = (size_t)128 * (128 / 2 + 1);
  auto fits_half = [&](uint32_t pw, uint32_t ph) { return (size_t)ph * (pw | 1u) <= half_cap; };
  if ((n_levels & 1) && !fits_half(base_w, base_h)) return false;
  for (int i = n_levels - 2; i >= 0; i -= 2)
    if (!fits_half(out_w[i], out_h[i])) return false;
  for (int i = 0; i < n_levels; i++) {
    const uint32_t rw = horizontal[i] ? out_w[i] / 2 : out_w[i], rh = horizontal[i] ? out_h[i] : out_h[i] / 2;
    if (rw && rh && !fits_half(rw, rh)) return false;
  }
  return true;
}
// ---- abi_squeeze.hip: the geometry check of jxlh_unsqueeze_levels and jxlh_unsqueeze_chain (every pointer a device one)
jxlh_status old_check(int n_planes, int n_levels, const jxlh_squeeze_level* levels, const cptr base[], size_t base_stride,
                      uint32_t base_w, uint32_t base_h, const mptr out[], size_t out_stride) {
  if (!levels || !base || !out || n_planes < 1 || n_planes > 3 || n_levels < 1 || n_levels > 64 || base_w == 0 ||
      base_h == 0 || base_stride < base_w)
    return JXLH_ERR_INVALID_ARGUMENT;
  uint32_t cw = base_w, ch = base_h;
  for (int i = 0; i < n_levels; i++) {
    const jxlh_squeeze_level& lv = levels[i];
    if (lv.out_w == 0 || lv.out_h == 0 || lv.out_w > (1u << 20) || lv.out_h > (1u << 20)) return JXLH_ERR_INVALID_ARGUMENT;
    const uint32_t aw = lv.horizontal ? (lv.out_w + 1) / 2 : lv.out_w, ah = lv.horizontal ? lv.out_h : (lv.out_h + 1) / 2;
    if (aw != cw || ah != ch) return JXLH_ERR_INVALID_ARGUMENT;
    const uint32_t rw = lv.horizontal ? lv.out_w / 2 : lv.out_w, rh = lv.horizontal ? lv.out_h : lv.out_h / 2;
    for (int p = 0; p < n_planes; p++)
      if ((size_t)rw * rh > 0 && (!lv.res[p] || lv.res_stride < rw)) return JXLH_ERR_INVALID_ARGUMENT;
    cw = lv.out_w;
    ch = lv.out_h;
  }
  if (out_stride < cw) return JXLH_ERR_INVALID_ARGUMENT;
  for (int p = 0; p < n_planes; p++)
    if (!base[p] || !out[p]) return JXLH_ERR_INVALID_ARGUMENT;
  return JXLH_OK;
}
// ---- abi_squeeze.hip: jxlh_unsqueeze_chain between the check and the return, launches recorded instead of issued
struct Chain {
  int n_planes, n_levels;
  std::vector<jxlh_squeeze_level> levels;
  uint32_t base_w, base_h;
  size_t base_stride, out_stride;
  uintptr_t base[3], out[3], arena;
  bool with_rct, sep, flow;
};
std::vector<Rec> old_chain(const Chain& c, size_t* arena_out) {
  std::vector<Rec> recs;
  const int n_planes = c.n_planes, n_levels = c.n_levels;
  const jxlh_squeeze_level* levels = c.levels.data();
  const bool with_rct = c.with_rct;
  cptr base[3] = {at(c.base[0]), at(c.base[1]), at(c.base[2])};
  mptr out[3] = {(mptr)c.out[0], (mptr)c.out[1], (mptr)c.out[2]};
  mptr hook = (mptr)c.arena;
  size_t level_off[64], level_stride[64], level_plane[64], arena = 0;
  for (int i = 0; i < n_levels - 1; i++) {
    level_off[i] = arena;
    level_stride[i] = ((size_t)levels[i].out_w + 3) & ~(size_t)3;
    level_plane[i] = (level_stride[i] * levels[i].out_h + 63) & ~(size_t)63;
    arena += level_plane[i] * n_planes;
  }
  *arena_out = arena;
  cptr cur[3] = {nullptr, nullptr, nullptr};
  size_t cur_stride = c.base_stride;
  for (int p = 0; p < n_planes; p++) cur[p] = base[p];
  auto dst_of = [&](int i, mptr dst[3], size_t* stride) {
    const bool last = i == n_levels - 1;
    for (int p = 0; p < n_planes; p++) dst[p] = last ? out[p] : hook + level_off[i] + (size_t)p * level_plane[i];
    *stride = last ? c.out_stride : level_stride[i];
  };
  auto record = [&](Rec r, int level0, const cptr* s, size_t ss, const mptr* d, size_t ds) {
    r.level0 = level0;
    for (int p = 0; p < n_planes; p++) {
      r.src[p] = (uintptr_t)s[p];
      r.dst[p] = (uintptr_t)d[p];
    }
    r.src_stride = ss;
    r.dst_stride = ds;
    recs.push_back(r);
  };
  int i = 0;
  {
    int n_small = 0;
    while (n_small < n_levels - (with_rct ? 1 : 0) && n_small < 16 && levels[n_small].out_w <= 128 && levels[n_small].out_h <= 128)
      n_small++;
    while (n_small >= 2) {
      int hz[16];
      uint32_t ow[16], oh[16];
      for (int k = 0; k < n_small; k++) {
        hz[k] = levels[k].horizontal ? 1 : 0;
        ow[k] = levels[k].out_w;
        oh[k] = levels[k].out_h;
      }
      mptr dst[3] = {nullptr, nullptr, nullptr};
      size_t dst_stride;
      dst_of(n_small - 1, dst, &dst_stride);
      if (old_launch_unsqueeze_levels(n_planes, n_small, hz, ow, oh, c.base_w, c.base_h)) {
        Rec r{};
        r.kind = kLevels;
        r.n = n_small;
        r.ncw = 1;
        record(r, 0, base, c.base_stride, dst, dst_stride);
        for (int p = 0; p < n_planes; p++) cur[p] = dst[p];
        cur_stride = dst_stride;
        i = n_small;
        break;
      }
      n_small--;
    }
  }
  const bool fuse_rct = with_rct && !c.sep;
  const bool flow = c.flow;
  while (i < n_levels) {
    if (flow) {
      const int max_run = std::min(16, 16 /* unsqueeze_flow_max_steps() */);
      cptr a[3] = {nullptr, nullptr, nullptr};
      size_t a_stride = cur_stride;
      for (int p = 0; p < n_planes; p++) a[p] = cur[p];
      int n = 0;
      Rec r{};
      size_t words = 2 * 64;
      mptr last_dst[3] = {nullptr, nullptr, nullptr};
      for (int j = i; j < n_levels && n < max_run; j++, n++) {
        const jxlh_squeeze_level& lv = levels[j];
        if (j == n_levels - 1 && with_rct) break;
        mptr dst[3] = {nullptr, nullptr, nullptr};
        size_t dst_stride;
        dst_of(j, dst, &dst_stride);
        if (!old_tiled_eligible(lv.horizontal ? 1 : 0, lv.out_w, lv.out_h, a_stride, lv.res_stride, dst_stride)) break;
        cptr fa[3], fr[3];
        mptr fo[3];
        for (int p = 0; p < 3; p++) {
          const int q = p < n_planes ? p : 0;
          fa[p] = a[q];
          fr[p] = lv.res[q] ? lv.res[q] : a[q];
          fo[p] = dst[q];
        }
        // launch_unsqueeze_flow: L.vec; unsqueeze_flow_words
        r.flow_vec.push_back(old_tiled_vec_ok(lv.horizontal ? 1 : 0, n_planes, fa, a_stride, fr, lv.res_stride, lv.out_w, lv.out_h,
                                              fo, dst_stride));
        const int n_lines = (int)(lv.horizontal ? lv.out_h : lv.out_w);
        words += (size_t)n_planes * ((n_lines + 63) / 64) * 64;
        for (int p = 0; p < n_planes; p++) a[p] = last_dst[p] = dst[p];
        a_stride = dst_stride;
      }
      if (n >= 2) {
        r.kind = kFlow;
        r.n = n;
        r.ncw = 1;
        r.flow_words = words;
        record(r, i, cur, cur_stride, last_dst, a_stride);
        for (int p = 0; p < n_planes; p++) cur[p] = a[p];
        cur_stride = a_stride;
        i += n;
        continue;
      }
    }
    const jxlh_squeeze_level& lv = levels[i];
    const bool last = i == n_levels - 1;
    mptr dst[3] = {nullptr, nullptr, nullptr};
    size_t dst_stride;
    dst_of(i, dst, &dst_stride);
    cptr rv[3] = {nullptr, nullptr, nullptr};
    for (int p = 0; p < n_planes; p++) rv[p] = lv.res[p] ? lv.res[p] : cur[p];
    bool fused = false;
    Rec r{};
    if (last && fuse_rct)
      fused = old_launch_unsqueeze_rct(lv.horizontal ? 1 : 0, cur, cur_stride, rv, lv.res_stride, lv.out_w, lv.out_h, dst, dst_stride, &r);
    if (!fused) r = old_launch_unsqueeze(lv.horizontal ? 1 : 0, n_planes, cur, cur_stride, rv, lv.res_stride, lv.out_w, lv.out_h, dst, dst_stride);
    record(r, i, cur, cur_stride, dst, dst_stride);
    if (last && with_rct && !fused) {
      Rec q{};
      q.kind = dst_stride == lv.out_w ? kRctFlat : kRctRows;
      q.ncw = 1;
      cptr d2[3] = {dst[0], dst[1], dst[2]};
      record(q, i, d2, dst_stride, dst, dst_stride);
    }
    for (int p = 0; p < n_planes; p++) cur[p] = dst[p];
    cur_stride = dst_stride;
    i++;
  }
  return recs;
}

// ---- the default chain of a w x h channel, inverse order (jxl_rs_amd/synth.py: default_squeeze_steps)
struct Step { bool horizontal; uint32_t w, h; };
std::vector<Step> default_chain(uint32_t w, uint32_t h, uint32_t* bw, uint32_t* bh) {
  std::vector<Step> fwd;
  uint32_t cw = w, ch = h;
  if (cw <= ch && ch > 8) {
    fwd.push_back({false, cw, ch});
    ch = (ch + 1) / 2;
  }
  while (cw > 8 || ch > 8) {
    if (cw > 8) {
      fwd.push_back({true, cw, ch});
      cw = (cw + 1) / 2;
    }
    if (ch > 8) {
      fwd.push_back({false, cw, ch});
      ch = (ch + 1) / 2;
    }
  }
  std::reverse(fwd.begin(), fwd.end());
  *bw = cw;
  *bh = ch;
  return fwd;
}
size_t stride_of(uint32_t w, int form, size_t forced) {  // 0 tight, 1 padded to 4, 2 odd
  if (forced) return forced;
  return form == 0 ? w : form == 1 ? (((size_t)w + 3) & ~(size_t)3) : ((size_t)w | 1);
}

long g_plans = 0, g_launches = 0;
int g_kinds[7] = {0};

void check_chain(const Chain& c) {
  size_t old_arena = 0;
  const std::vector<Rec> old = old_chain(c, &old_arena);
  SqueezeChainIn in{c.n_planes, c.n_levels, c.levels.data(), c.base_w, c.base_h, c.base_stride, c.out_stride,
                    {c.base[0], c.base[1], c.base[2]}, {c.out[0], c.out[1], c.out[2]}, c.arena, c.with_rct, c.sep, c.flow};
  const SqueezePlan P = plan_squeeze_chain(in);
  g_plans++;
  const int nl = c.n_levels, np = c.n_planes;
  CHECK(P.arena.total == old_arena && squeeze_arena(np, nl, c.levels.data()).total == old_arena, "arena %zu %zu", P.arena.total, old_arena);
  CHECK((size_t)P.n == old.size(), "launch count %d %zu", P.n, old.size());
  auto addr = [&](SqueezeLoc l, int p) {
    return l.where == kSqBase ? c.base[p] : l.where == kSqOut ? c.out[p]
                                                              : c.arena + 4 * (P.arena.off[l.where] + (size_t)p * P.arena.plane[l.where]);
  };
  size_t old_words = 0;
  int next_level = 0;
  for (int k = 0; k < P.n && k < (int)old.size(); k++) {
    const SqueezeLaunch& L = P.launch[k];
    const Rec& r = old[k];
    g_launches++;
    g_kinds[L.kind]++;
    CHECK(L.kind == r.kind && L.level0 == r.level0 && L.n_levels == r.n, "launch %d: kind %d/%d level0 %d/%d n %d/%d", k, L.kind,
          r.kind, L.level0, r.level0, L.n_levels, r.n);
    if (L.kind != kFlow && L.kind != kLevels && L.kind != kRctFlat && L.kind != kRctRows)
      CHECK(L.vec == r.vec && L.ncw == r.ncw, "launch %d kind %d: vec %d/%d ncw %d/%d", k, L.kind, L.vec, r.vec, L.ncw, r.ncw);
    CHECK(L.src.stride == r.src_stride && L.dst.stride == r.dst_stride, "launch %d strides", k);
    for (int p = 0; p < np; p++) CHECK(addr(L.src, p) == r.src[p] && addr(L.dst, p) == r.dst[p], "launch %d plane %d addresses", k, p);
    if (L.kind == kFlow) {
      for (int j = 0; j < L.n_levels && j < (int)r.flow_vec.size(); j++)
        CHECK(P.vec[L.level0 + j] == r.flow_vec[j], "flow level %d vec", L.level0 + j);
      CHECK(squeeze_flow_words(np, L.n_levels, c.levels.data() + L.level0) == r.flow_words, "flow words");
      old_words = std::max(old_words, r.flow_words);
      CHECK(L.n_levels >= 2 && L.n_levels <= kFlowRunCap, "flow run of %d", L.n_levels);
      CHECK(!(c.with_rct && L.level0 + L.n_levels == nl), "a flow run took the level the RCT follows");
    }
    if (L.kind == kLevels) {
      CHECK(k == 0 && L.level0 == 0 && L.n_levels >= 2 && squeeze_levels_fit(L.n_levels, c.levels.data(), c.base_w, c.base_h), "prefix");
      CHECK(!(c.with_rct && L.n_levels == nl), "the prefix took the level the RCT follows");
    }
    // invariants: levels covered once and in order; a launch reads what the one before wrote; a fused RCT is last
    CHECK(L.level0 == (L.n_levels ? next_level : next_level - 1), "launch %d starts at level %d, expected %d", k, L.level0, next_level);
    next_level += L.n_levels;
    const SqueezeLoc prev = k ? P.launch[k - 1].dst : SqueezeLoc{kSqBase, c.base_stride};
    CHECK(L.src.where == prev.where && L.src.stride == prev.stride, "launch %d does not read what launch %d wrote", k, k - 1);
    if (L.kind == kFusedRct || L.kind == kRctFlat || L.kind == kRctRows) CHECK(k == P.n - 1 && c.with_rct, "RCT at %d of %d", k, P.n);
    if (L.kind == kRctFlat || L.kind == kRctRows) CHECK(L.dst.where == L.src.where, "the RCT runs in place");
    if (L.n_levels && L.dst.where >= 0) CHECK(L.dst.where == L.level0 + L.n_levels - 1, "plane set of the launch's last level");
  }
  CHECK(next_level == nl, "levels covered: %d of %d", next_level, nl);
  if (P.n) {
    CHECK(P.launch[P.n - 1].dst.where == kSqOut && P.launch[P.n - 1].dst.stride == c.out_stride, "the last launch writes out");
    const int k = P.launch[P.n - 1].kind;
    CHECK(!c.with_rct || k == kFusedRct || k == kRctFlat || k == kRctRows, "the RCT is missing");
  }
  CHECK(P.flow_words == old_words, "flow words %zu %zu", P.flow_words, old_words);
  // the arena: plane sets disjoint, in order, every plane on a 256-byte boundary, rows padded to 4 samples
  size_t end = 0;
  for (int i = 0; i < nl - 1; i++) {
    CHECK(P.arena.off[i] == end && P.arena.off[i] % 64 == 0 && P.arena.plane[i] % 64 == 0 && P.arena.stride[i] % 4 == 0 &&
              P.arena.stride[i] >= c.levels[i].out_w && P.arena.plane[i] >= P.arena.stride[i] * c.levels[i].out_h,
          "arena level %d", i);
    end = P.arena.off[i] + P.arena.plane[i] * np;
  }
  CHECK(end == P.arena.total, "arena total");
}

void check_steps_and_entries(const Chain& c) {
  const int np = c.n_planes;
  // jxlh_unsqueeze_levels: the whole chain in one launch, or the chain's route
  for (int n = 1; n <= c.n_levels && n <= 17; n++) {
    int hz[64];
    uint32_t ow[64], oh[64];
    for (int k = 0; k < n; k++) {
      hz[k] = c.levels[k].horizontal ? 1 : 0;
      ow[k] = c.levels[k].out_w;
      oh[k] = c.levels[k].out_h;
    }
    const bool old = n <= 16 && old_launch_unsqueeze_levels(np, n, hz, ow, oh, c.base_w, c.base_h);
    CHECK(squeeze_levels_fit(n, c.levels.data(), c.base_w, c.base_h) == old, "levels fit, n = %d", n);
  }
  // jxlh_unsqueeze / jxlh_unsqueeze_planes / jxlh_unsqueeze_rct on every level of the chain as a step of its own
  size_t avg_stride = c.base_stride;
  for (int i = 0; i < c.n_levels; i++) {
    const jxlh_squeeze_level& lv = c.levels[i];
    const size_t out_stride = i == c.n_levels - 1 ? c.out_stride : stride_of(lv.out_w, (int)(c.out_stride % 3), 0);
    cptr avg[3], res[3];
    mptr out[3];
    SqueezeStep s{lv.horizontal != 0, np, lv.out_w, lv.out_h, avg_stride, lv.res_stride, out_stride, {}, {}, {}};
    for (int p = 0; p < 3; p++) {
      s.avg[p] = c.base[p] + 0x100 * i;
      s.res[p] = (uintptr_t)lv.res[p < np ? p : 0];
      s.out[p] = c.out[p] + 0x100 * i;
      avg[p] = at(s.avg[p]);
      res[p] = at(s.res[p]);
      out[p] = (mptr)s.out[p];
    }
    const Rec o = old_launch_unsqueeze(lv.horizontal ? 1 : 0, np, avg, avg_stride, res, lv.res_stride, lv.out_w, lv.out_h, out, out_stride);
    const SqueezeLaunch L = plan_squeeze_step(s);
    CHECK(L.kind == o.kind && L.vec == o.vec && L.n_levels == 1, "step %d: kind %d/%d vec %d/%d", i, L.kind, o.kind, L.vec, o.vec);
    CHECK(squeeze_streamed(s) == old_tiled_eligible(lv.horizontal ? 1 : 0, lv.out_w, lv.out_h, avg_stride, lv.res_stride, out_stride), "streamed");
    const SqueezeExtents e = squeeze_extents(lv.horizontal != 0, lv.out_w, lv.out_h);
    const uint32_t aw = lv.horizontal ? (lv.out_w + 1) / 2 : lv.out_w, ah = lv.horizontal ? lv.out_h : (lv.out_h + 1) / 2;
    const uint32_t rw = lv.horizontal ? lv.out_w / 2 : lv.out_w, rh = lv.horizontal ? lv.out_h : lv.out_h / 2;
    CHECK(e.avg_w == aw && e.avg_h == ah && e.res_w == rw && e.res_h == rh && e.has_res == ((size_t)rw * rh > 0), "extents");
    if (np == 3) {
      SqueezeLaunch L2[2];
      const int n = plan_squeeze_step_rct(s, c.sep, L2);
      Rec f{};
      const bool fused = !c.sep && old_launch_unsqueeze_rct(lv.horizontal ? 1 : 0, avg, avg_stride, res, lv.res_stride, lv.out_w, lv.out_h, out, out_stride, &f);
      if (fused) {
        CHECK(n == 1 && L2[0].kind == kFusedRct && L2[0].vec == f.vec && L2[0].ncw == f.ncw, "fused step %d", i);
      } else {
        CHECK(n == 2 && L2[0].kind == o.kind && L2[0].vec == o.vec && L2[1].kind == (out_stride == lv.out_w ? kRctFlat : kRctRows),
              "two-pass step %d", i);
      }
    }
    avg_stride = out_stride;
  }
}

void sweep_size(uint32_t w, uint32_t h, bool full) {
  uint32_t bw, bh;
  const std::vector<Step> steps = default_chain(w, h, &bw, &bh);
  if (steps.empty()) return;
  const uint32_t lh = steps.back().h;
  // span limits: strides of the out planes / the last level's residuals that put a plane's span next to 2^30 and 2^31
  std::vector<size_t> forced = {0};
  if (full)
    for (int lg = 30; lg <= 31; lg++)
      for (size_t s : {(((size_t)1 << lg) / lh - 4) & ~(size_t)3, ((((size_t)1 << lg) + lh - 1) / lh + 3) & ~(size_t)3})
        if (s >= w) forced.push_back(s);
  for (int np = 1; np <= 3; np++)
    for (int rct = 0; rct <= (np == 3 ? 1 : 0); rct++)
      for (int sform = 0; sform < 3; sform++)
        for (int rform = 0; rform < 3; rform++)
          for (int mis = 0; mis < (full ? 16 : 2); mis++)  // bit 0 out, 1 base, 2 residuals, 3 arena: 4 bytes off
            for (int sw = 0; sw < 4; sw++)
              for (size_t f_out : forced)
                for (size_t f_res : forced) {
                  if (f_out && f_res && f_out != f_res) continue;
                  Chain c{};
                  c.n_planes = np;
                  c.n_levels = (int)steps.size();
                  c.base_w = bw;
                  c.base_h = bh;
                  c.base_stride = stride_of(bw, sform, 0);
                  c.out_stride = stride_of(w, sform, f_out);
                  c.with_rct = rct != 0;
                  c.sep = (sw & 1) != 0;
                  c.flow = (sw & 2) == 0;
                  c.arena = 0x7f0000000000ull + ((mis & 8) ? 4 : 0);
                  for (int p = 0; p < 3; p++) {
                    c.base[p] = 0x100000000ull + 0x1000000ull * p + ((mis & 2) ? 4 : 0);
                    c.out[p] = 0x200000000ull + 0x10000000000ull * p + ((mis & 1) ? 4 : 0);
                  }
                  for (size_t i = 0; i < steps.size(); i++) {
                    jxlh_squeeze_level lv{};
                    lv.horizontal = steps[i].horizontal;
                    lv.out_w = steps[i].w;
                    lv.out_h = steps[i].h;
                    const SqueezeExtents e = squeeze_extents(steps[i].horizontal, steps[i].w, steps[i].h);
                    lv.res_stride = stride_of(e.res_w, rform, i + 1 == steps.size() ? f_res : 0);
                    for (int p = 0; p < np; p++)
                      lv.res[p] = at(0x1000000000000ull + 0x40000000000ull * i + 0x10000000000ull * p + ((mis & 4) ? 4 : 0));
                    c.levels.push_back(lv);
                  }
                  cptr base[3] = {at(c.base[0]), at(c.base[1]), at(c.base[2])};
                  mptr out[3] = {(mptr)c.out[0], (mptr)c.out[1], (mptr)c.out[2]};
                  auto is_dev = [](const void*) { return true; };
                  const jxlh_status st = check_squeeze_chain(np, c.n_levels, c.levels.data(), base, c.base_stride, bw, bh, out, c.out_stride, is_dev);
                  CHECK(st == JXLH_OK && st == old_check(np, c.n_levels, c.levels.data(), base, c.base_stride, bw, bh, out, c.out_stride),
                        "check of a valid chain %ux%u", w, h);
                  check_chain(c);
                  if (sw == 0 || sw == 1) check_steps_and_entries(c);
                  if (mis == 0 && sw == 0 && !f_out && !f_res) {  // the check: one field off at a time
                    for (int bad = 0; bad < 6; bad++) {
                      Chain d = c;
                      jxlh_squeeze_level& lv = d.levels[d.levels.size() / 2];
                      size_t os = d.out_stride, bs = d.base_stride;
                      if (bad == 0) lv.out_w += 2;
                      if (bad == 1) lv.res[np - 1] = nullptr;
                      if (bad == 2) lv.res_stride = squeeze_extents(lv.horizontal != 0, lv.out_w, lv.out_h).res_w - 1;
                      if (bad == 3) os = w - 1;
                      if (bad == 4) bs = bw - 1;
                      if (bad == 5) lv.out_h = (1u << 20) + 1;
                      const jxlh_status a = check_squeeze_chain(np, d.n_levels, d.levels.data(), base, bs, bw, bh, out, os, is_dev);
                      CHECK(a == JXLH_ERR_INVALID_ARGUMENT && a == old_check(np, d.n_levels, d.levels.data(), base, bs, bw, bh, out, os),
                            "check of a broken chain (%d)", bad);
                    }
                    auto host_res = [&](const void* q) { return q != (const void*)c.levels[0].res[0]; };
                    CHECK(check_squeeze_chain(np, c.n_levels, c.levels.data(), base, c.base_stride, bw, bh, out, c.out_stride, host_res) ==
                              JXLH_ERR_INVALID_ARGUMENT, "a host residual plane");
                  }
                }
}

}  // namespace

int main() {
  const uint32_t full[][2] = {{16, 16},     {257, 129},   {9, 300},     {1031, 17},    {130, 2000}, {700, 500},
                              {2048, 2048}, {8192, 8192}, {70000, 300}, {200, 66000}};
  for (auto& s : full) sweep_size(s[0], s[1], true);
  // the thresholds: lines of 255 / 256 / 257 output samples (streamed at 256), sides of 128 / 129 (LDS), chains of one
  // and two levels, a chain whose only streamed level is the last one
  const uint32_t edge[] = {9, 16, 17, 127, 128, 129, 255, 256, 257, 258, 511, 512, 513, 600};
  for (uint32_t w : edge)
    for (uint32_t h : edge) sweep_size(w, h, false);
  sweep_size(8, 9, false);
  sweep_size(9, 8, false);
  sweep_size(4096, 4100, false);
  sweep_size(4128, 4096, false);
  std::printf("plans %ld launches %ld: levels %d flow %d tiled %d one-wave %d fused %d rct-flat %d rct-rows %d\n", g_plans, g_launches,
              g_kinds[0], g_kinds[1], g_kinds[2], g_kinds[3], g_kinds[4], g_kinds[5], g_kinds[6]);
  for (int k = 0; k < 7; k++)
    if (!g_kinds[k]) {
      std::printf("FAIL: launch kind %d never planned\n", k);
      g_fail++;
    }
  if (g_fail) {
    std::printf("squeeze plans: %d FAILED\n", g_fail);
    return 1;
  }
  std::printf("squeeze plans: ok\n");
  return 0;
}
