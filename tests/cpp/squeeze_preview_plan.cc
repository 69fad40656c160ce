// The preview planner (jxl_rs_amd/csrc/squeeze_preview_plan.h) without grids, over random chains: directions, sizes,
// plane counts, missing sets with holes, strides and addresses.  Checked: the argument rule for missing levels; kinds and
// liveness by their definitions; the regular prefix is the chain plan of exactly those levels; behind it one entry per
// live level and none for a dead one; every entry reads a plane set that was written before it, of the size it expects,
// and writes its own; nothing reaches past the arena; the RCT rides on the last level only (the entry checks are
// squeeze_preview_checks.h's, shared with squeeze_tiles_plan.cc).  Host only, no device: addresses are numbers.  Built plain and with -fsanitize=address,undefined (tests/test_squeeze_preview_cpu.py).
#include "squeeze_preview_checks.h"

namespace {

void one_chain(int id) {
  // ---- a chain: final size, directions from the last level down, sizes halving towards the base
  jxlh_squeeze_level lv[kSqueezeMaxLevels];
  std::memset(lv, 0, sizeof lv);
  const int nl = (int)rnd(1, id % 50 == 0 ? 24 : 9);
  const int n_planes = (int)rnd(1, 3);
  const uint32_t big = id % 17 == 0 ? 9000 : id % 5 == 0 ? 1200 : 90;
  uint32_t cw = rnd(1, big), ch = rnd(1, big);
  const int pattern = (int)rnd(0, 3);  // 0: alternate, 1: random, 2: all one way, 3: pairs
  for (int i = nl - 1; i >= 0; i--) {
    const int k = nl - 1 - i;
    const bool hz = pattern == 0 ? (k & 1) : pattern == 1 ? (rnd() & 1) : pattern == 2 ? (id & 1) : ((k >> 1) & 1);
    lv[i].horizontal = hz ? (int32_t)rnd(1, 3) : 0;  // any non-zero value is "horizontal"
    lv[i].out_w = cw;
    lv[i].out_h = ch;
    if (hz) cw = (cw + 1) / 2; else ch = (ch + 1) / 2;
  }
  const uint32_t base_w = cw, base_h = ch;
  const uint32_t miss_mode = rnd(0, 3);  // 0: none, 1: a suffix, 2/3: random with holes
  const int suffix = (int)rnd(0, (uint32_t)nl);
  bool missing[kSqueezeMaxLevels];
  const uintptr_t kRes = 0x100000000ull;
  for (int i = 0; i < nl; i++) {
    const SqueezeExtents e = squeeze_extents(lv[i].horizontal != 0, lv[i].out_w, lv[i].out_h);
    const bool want = miss_mode == 0 ? false : miss_mode == 1 ? i >= nl - suffix : (rnd() % 3) != 0;
    missing[i] = want && e.has_res;
    lv[i].res_stride = e.res_w + (rnd() % 3 ? 0 : rnd(1, 7));
    for (int p = 0; p < n_planes; p++)
      if (!want) lv[i].res[p] = reinterpret_cast<const int32_t*>(kRes + 0x1000000ull * (uintptr_t)(i * 3 + p) + (rnd() % 4 ? 0 : 4 * rnd(1, 3)));
  }
  SqueezeChainIn in{};
  in.n_planes = n_planes;
  in.n_levels = nl;
  in.levels = lv;
  in.base_w = base_w;
  in.base_h = base_h;
  in.base_stride = base_w + (rnd() % 3 ? 0 : rnd(1, 5));
  in.out_stride = lv[nl - 1].out_w + (rnd() % 3 ? 0 : rnd(1, 9));
  const int32_t* base[3] = {};
  int32_t* out[3] = {};
  for (int p = 0; p < n_planes; p++) {
    in.base[p] = 0x10000000ull + 0x100000ull * (uintptr_t)p + (rnd() % 4 ? 0 : 4);
    in.out[p] = 0x40000000ull + 0x10000000ull * (uintptr_t)p + (rnd() % 4 ? 0 : 8);
    base[p] = reinterpret_cast<const int32_t*>(in.base[p]);
    out[p] = reinterpret_cast<int32_t*>(in.out[p]);
  }
  in.arena = 0x7000000000ull;
  in.with_rct = n_planes == 3 && (rnd() & 1);
  in.separate_rct = rnd() % 4 == 0;
  in.flow = rnd() % 4 != 0;
  auto is_dev = [](const void*) { return true; };

  // ---- the argument rule
  const bool any_missing = [&] { for (int i = 0; i < nl; i++) if (missing[i]) return true; return false; }();
  CHECK(check_squeeze_chain(n_planes, nl, lv, base, in.base_stride, base_w, base_h, out, in.out_stride, is_dev, true) == JXLH_OK, "chain %d", id);
  CHECK((check_squeeze_chain(n_planes, nl, lv, base, in.base_stride, base_w, base_h, out, in.out_stride, is_dev) == JXLH_OK) == !any_missing,
        "chain %d: the chain call takes no missing level", id);
  for (int i = 0; i < nl; i++) CHECK(squeeze_level_missing(n_planes, lv[i]) == missing[i], "chain %d level %d", id, i);
  if (n_planes > 1) {  // some planes of a level named, others not
    const int i = (int)rnd(0, (uint32_t)nl - 1), p = (int)rnd(0, (uint32_t)n_planes - 1);
    if (squeeze_extents(lv[i].horizontal != 0, lv[i].out_w, lv[i].out_h).has_res) {
      const int32_t* keep[3] = {lv[i].res[0], lv[i].res[1], lv[i].res[2]};
      for (int q = 0; q < n_planes; q++) lv[i].res[q] = q == p ? nullptr : reinterpret_cast<const int32_t*>(kRes);
      CHECK(check_squeeze_chain(n_planes, nl, lv, base, in.base_stride, base_w, base_h, out, in.out_stride, is_dev, true) ==
                JXLH_ERR_INVALID_ARGUMENT, "chain %d: partly named level %d", id, i);
      for (int q = 0; q < 3; q++) lv[i].res[q] = keep[q];
    }
  }

  // ---- kinds and liveness, by their definitions
  const SqueezePreviewPlan P = plan_squeeze_preview(in, nullptr);
  uint8_t kinds[kSqueezeMaxLevels], live[kSqueezeMaxLevels];
  squeeze_preview_kinds(n_planes, nl, lv, kinds, live);
  for (int i = 0; i < nl; i++)
    CHECK(P.kind[i] == (int)kinds[i] && P.live[i] == live[i], "chain %d level %d: the plan's kinds are the public ones", id, i);
  CHECK(P.records.empty() && !P.too_large, "chain %d: lists without a grid", id);
  int reads[kSqueezeMaxLevels];  // the level whose output a level reads
  for (int i = 0; i < nl; i++) {
    const bool two_d = missing[i] && i > 0 && missing[i - 1] && (lv[i].horizontal != 0) != (lv[i - 1].horizontal != 0);
    const int want = !missing[i] ? JXLH_PREVIEW_REGULAR : two_d ? JXLH_PREVIEW_SMOOTH_2D : JXLH_PREVIEW_SMOOTH_1D;
    CHECK(kinds[i] == want, "chain %d level %d: kind %d, expected %d", id, i, kinds[i], want);
    reads[i] = two_d ? i - 2 : i - 1;
  }
  bool want_live[kSqueezeMaxLevels] = {};
  want_live[nl - 1] = true;
  for (int i = nl - 1; i >= 0; i--)
    if (want_live[i] && reads[i] >= 0) want_live[reads[i]] = true;
  for (int i = 0; i < nl; i++) CHECK((live[i] != 0) == want_live[i], "chain %d level %d: live %d", id, i, live[i]);

  // ---- the prefix is the chain plan of its levels
  int n_pre = 0;
  while (n_pre < nl && !missing[n_pre]) n_pre++;
  CHECK(P.n_prefix == n_pre, "chain %d: prefix %d, expected %d", id, P.n_prefix, n_pre);
  const SqueezeArena A = squeeze_arena(n_planes, nl, lv);
  CHECK(!std::memcmp(&A, &P.arena, sizeof A), "chain %d: arena", id);
  auto arena_addr = [&](int level, int p) { return in.arena + sizeof(int32_t) * (A.off[level] + (size_t)p * A.plane[level]); };
  if (n_pre > 0) {
    SqueezeChainIn want = in;
    want.n_levels = n_pre;
    if (n_pre < nl) {
      want.with_rct = false;
      want.out_stride = A.stride[n_pre - 1];
      for (int p = 0; p < n_planes; p++) want.out[p] = arena_addr(n_pre - 1, p);
    }
    const SqueezePlan ref = plan_squeeze_chain(want);
    CHECK(P.prefix_in.n_levels == want.n_levels && P.prefix_in.with_rct == want.with_rct && P.prefix_in.out_stride == want.out_stride &&
              !std::memcmp(P.prefix_in.out, want.out, sizeof want.out) && !std::memcmp(P.prefix_in.base, want.base, sizeof want.base) &&
              P.prefix_in.flow == want.flow && P.prefix_in.separate_rct == want.separate_rct && P.prefix_in.arena == want.arena,
          "chain %d: the prefix's chain", id);
    CHECK(P.prefix.n == ref.n && P.prefix.flow_words == ref.flow_words, "chain %d: prefix launches", id);
    for (int k = 0; k < ref.n && k < P.prefix.n; k++) CHECK(same_launch(P.prefix.launch[k], ref.launch[k]), "chain %d: prefix launch %d", id, k);
    // the prefix's own arena is the head of the whole chain's
    for (int i = 0; i + 1 < n_pre; i++)
      CHECK(P.prefix.arena.off[i] == A.off[i] && P.prefix.arena.stride[i] == A.stride[i] && P.prefix.arena.plane[i] == A.plane[i], "chain %d", id);
  }
  if (n_pre == nl) CHECK(P.n == 0, "chain %d: nothing behind a complete chain", id);

  // ---- the entries chain: one per live level behind the prefix, each reading what was written
  bool written[kSqueezeMaxLevels] = {};
  for (int i = 0; i < n_pre; i++) written[i] = true;  // (the prefix's intermediate planes too; nothing may read them: below)
  int k = 0;
  for (int i = n_pre; i < nl; i++) {
    if (!live[i]) continue;
    CHECK(k < P.n, "chain %d: live level %d has no entry", id, i);
    if (k >= P.n) break;
    const PreviewEntry& e = P.entry[k++];
    CHECK(e.level == i && e.kind == kinds[i], "chain %d entry %d: level %d kind %d", id, k - 1, e.level, e.kind);
    // (check_whole_entry holds the level read against the kind; reads[] is the definition's)
    const int s = e.kind == JXLH_PREVIEW_SMOOTH_2D ? e.src2.where : e.src.where;
    CHECK((s == kSqBase ? -1 : s) == reads[i], "chain %d level %d reads %d, expected %d", id, i, s, reads[i]);
    check_whole_entry(id, in, e, n_pre, written);
    written[i] = true;
  }
  CHECK(k == P.n, "chain %d: %d entries, %d live levels behind the prefix", id, P.n, k);
  if (n_pre < nl) CHECK(P.n > 0 && P.entry[P.n - 1].level == nl - 1, "chain %d: ends with the last level", id);
}

}  // namespace

int main(int argc, char** argv) {
  const int n = argc > 1 ? std::atoi(argv[1]) : 100000;
  for (int id = 0; id < n; id++) one_chain(id);
  // the cap on levels
  {
    jxlh_squeeze_level lv[kSqueezeMaxLevels + 1];
    std::memset(lv, 0, sizeof lv);
    for (int i = 0; i <= kSqueezeMaxLevels; i++) { lv[i].horizontal = 1; lv[i].out_w = 1; lv[i].out_h = 3; }
    const int32_t some = 0;
    const int32_t* base[1] = {&some};
    int32_t* out[1] = {const_cast<int32_t*>(&some)};
    auto is_dev = [](const void*) { return true; };
    CHECK(check_squeeze_chain(1, kSqueezeMaxLevels, lv, base, 1, 1, 3, out, 1, is_dev, true) == JXLH_OK, "64 levels");
    CHECK(check_squeeze_chain(1, kSqueezeMaxLevels + 1, lv, base, 1, 1, 3, out, 1, is_dev, true) == JXLH_ERR_INVALID_ARGUMENT, "65 levels");
    SqueezeChainIn in{};
    in.n_planes = 1; in.n_levels = kSqueezeMaxLevels; in.levels = lv; in.base_w = 1; in.base_h = 3; in.base_stride = 1; in.out_stride = 1;
    in.base[0] = in.out[0] = 64; in.arena = 4096;
    const SqueezePreviewPlan P = plan_squeeze_preview(in, nullptr);  // no residual samples anywhere: all regular
    CHECK(P.n_prefix == kSqueezeMaxLevels && P.n == 0, "64 levels without residuals");
  }
  if (g_fail) {
    std::printf("squeeze preview plans: %d FAILED\n", g_fail);
    return 1;
  }
  std::printf("squeeze preview plans: ok (%d chains)\n", n);
  return 0;
}
