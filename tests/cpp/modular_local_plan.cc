// The batch plan of the group-local transforms (jxl_rs_amd/csrc/modular_local_plan.h) on its own: plain C++, no device,
// no library -- the program a sanitizer build runs (-fsanitize=address,undefined).
//   modular_local_plan         plans the named batches below and checks every decision of the plan: the route of each
//                              group, the launch list, where slots live between phases, the chains' LDS levels and
//                              scratch planes, the block's layout and bytes, and every refusal
//   modular_local_plan dump    prints per batch
//                                batch NAME status FIRST_BAD scratch SCRATCH total TOTAL
//                                step KERNEL desc OFF BYTES items OFF BYTES n_items N step K weighted W lds_palette L fan_grey F
//                                block HEX
//                              for the test to read the launch lists, and for comparing plans across versions
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../jxl_rs_amd/csrc/modular_local_plan.h"

using namespace jxlh;

static int fails = 0;
#define EXPECT(c)                                        \
  do {                                                   \
    if (!(c)) {                                          \
      fprintf(stderr, "line %d: %s\n", __LINE__, #c);    \
      fails++;                                           \
    }                                                    \
  } while (0)

static const jxlh_wp_header kWp = {16, 10, 7, 7, 7, 0, 0, 13, 12, 12, 12};

// one call: the groups of either form, the call-wide tables, and an arena handed out by a bump pointer
struct Call {
  LocalBatchIn::Form form = LocalBatchIn::kGeneral;
  std::vector<jxlh_local_group> groups;
  std::vector<jxlh_local_squeeze_group> sgroups;
  std::vector<jxlh_local_coded_channel> coded;
  std::vector<jxlh_squeeze_params> params;
  std::vector<jxlh_wp_header> wp;
  uint32_t bit_depth = 8, n_out = 4, w = 1056, h = 660;
  bool frame = false;
  uint64_t arena = 64, arena_samples = 0;  // arena_samples == 0: what was handed out
  uint64_t take(uint64_t n) {
    const uint64_t at = arena;
    arena += n;
    return at;
  }
  LocalBatchIn in() const {
    LocalBatchIn v;
    v.form = form;
    v.groups = groups.data(), v.sgroups = sgroups.data();
    v.coded = coded.data(), v.n_coded = coded.size(), v.params = params.data(), v.n_params = params.size();
    v.n = form == LocalBatchIn::kSqueeze ? sgroups.size() : groups.size();
    v.wp = wp.data();
    v.bit_depth = bit_depth, v.arena_samples = arena_samples ? arena_samples : arena;
    v.n_out = n_out, v.w = w, v.h = h, v.frame = frame;
    return v;
  }
  LocalPlan plan(bool aligned = true) const { return plan_local_batch(in(), aligned); }
};

static jxlh_local_step rct(uint32_t begin, uint32_t type) {
  jxlh_local_step s;
  memset(&s, 0, sizeof s);
  s.kind = JXLH_LOCAL_RCT, s.begin_c = begin, s.rct_type = type;
  return s;
}
static jxlh_local_step pal(Call& c, uint32_t begin, uint32_t num_c, uint32_t colors, uint32_t deltas, uint32_t predictor) {
  jxlh_local_step s;
  memset(&s, 0, sizeof s);
  s.kind = JXLH_LOCAL_PALETTE, s.begin_c = begin, s.num_c = num_c, s.num_colors = colors, s.num_deltas = deltas;
  s.predictor = predictor, s.palette_offset = c.take((uint64_t)num_c * (colors + deltas));
  return s;
}

// image channels the steps leave, and their meta channels
static void channels_left(uint32_t n_channels, const std::vector<jxlh_local_step>& steps, uint32_t* n_image, uint32_t* n_meta) {
  jxlh_local_group g;
  memset(&g, 0, sizeof g);
  g.n_channels = n_channels, g.n_steps = (uint32_t)steps.size();
  for (size_t i = 0; i < steps.size(); i++) g.steps[i] = steps[i];
  jxlh_local_general_program gp;
  const jxlh_status st = local_lower_core(g, 8, ~0ull, true, &kWp, nullptr, &gp, nullptr, false);
  EXPECT(st == JXLH_OK);
  *n_image = st == JXLH_OK ? gp.n_coded : 0;
  *n_meta = 0;
  for (const jxlh_local_step& s : steps) *n_meta += s.kind == JXLH_LOCAL_PALETTE;
}

// a group of the plain / _general calls; its coded channels are rows of w + stride_pad samples
static size_t add_group(Call& c, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t n_channels,
                        const std::vector<jxlh_local_step>& steps, uint32_t stride_pad = 0) {
  jxlh_local_group g;
  memset(&g, 0, sizeof g);
  g.x0 = x0, g.y0 = y0, g.w = w, g.h = h, g.n_channels = n_channels, g.n_steps = (uint32_t)steps.size();
  for (size_t i = 0; i < steps.size(); i++) g.steps[i] = steps[i];
  uint32_t n_meta;
  channels_left(n_channels, steps, &g.n_coded, &n_meta);
  g.coded_stride = w + stride_pad;
  for (uint32_t k = 0; k < g.n_coded; k++) g.coded_offset[k] = c.take((uint64_t)g.coded_stride * h);
  c.groups.push_back(g);
  c.wp.push_back(kWp);
  return c.groups.size() - 1;
}

// a group of the _squeeze calls: squeeze == nullptr: no squeeze; empty: the default one; else the explicit list.  Coded
// channel k is rows of its width + k * stride_skew samples
static size_t add_squeeze_group(Call& c, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t n_channels,
                                const std::vector<jxlh_local_step>& steps, const std::vector<jxlh_squeeze_params>* squeeze,
                                uint32_t stride_skew = 0) {
  jxlh_local_squeeze_group g;
  memset(&g, 0, sizeof g);
  g.x0 = x0, g.y0 = y0, g.w = w, g.h = h, g.n_channels = n_channels, g.n_steps = (uint32_t)steps.size();
  for (size_t i = 0; i < steps.size(); i++) g.steps[i] = steps[i];
  uint32_t n_image, n_meta;
  channels_left(n_channels, steps, &n_image, &n_meta);
  // the bookkeeping of meta_apply.rs on sizes only
  struct E { uint32_t w, h; };
  std::vector<E> list(n_meta + n_image, E{w, h});
  if (squeeze) {
    g.has_squeeze = 1, g.squeeze_pos = g.n_steps;
    std::vector<jxlh_squeeze_params> ps = *squeeze;
    g.params_first = (uint32_t)c.params.size(), g.n_params = (uint32_t)ps.size();
    c.params.insert(c.params.end(), ps.begin(), ps.end());
    if (ps.empty()) {
      jxlh_squeeze_params d[kLsMaxDefaultParams];
      uint32_t cw[4], ch[4];
      for (uint32_t k = 0; k < n_image; k++) cw[k] = w, ch[k] = h;
      ps.assign(d, d + default_squeeze_list(cw, ch, n_image, n_meta, d, kLsMaxDefaultParams));
    }
    for (const jxlh_squeeze_params& p : ps) {
      const size_t end = p.begin_c + p.num_c, at0 = p.in_place ? end : list.size();
      for (uint32_t ic = 0; ic < p.num_c; ic++) {
        E& e = list[p.begin_c + ic];
        E r = e;
        if (p.horizontal) e.w = (e.w + 1) / 2, r.w -= e.w;
        else e.h = (e.h + 1) / 2, r.h -= e.h;
        list.insert(list.begin() + at0 + ic, r);
      }
    }
  }
  g.coded_first = (uint32_t)c.coded.size(), g.n_coded = (uint32_t)list.size() - n_meta;
  for (uint32_t k = 0; k < g.n_coded; k++) {
    const E& e = list[n_meta + k];
    const uint32_t stride = e.w + k * stride_skew;
    c.coded.push_back(jxlh_local_coded_channel{c.take((uint64_t)stride * e.h), stride, e.w, e.h});
  }
  c.sgroups.push_back(g);
  c.wp.push_back(kWp);
  return c.sgroups.size() - 1;
}

static const std::vector<jxlh_squeeze_params> kDefault;

// ---------------------------------------------------------------- what a plan says about one group
static size_t plain_items(const LocalPlan& p, size_t gi) {
  size_t n = 0;
  for (const LocalItem& it : p.items) n += it.group == gi;
  return n;
}
static size_t phase_descs(const LocalPlan& p, uint32_t x0) {  // groups of a batch are told apart by x0
  size_t n = 0;
  for (uint32_t ph = 0; ph < kLpMaxPhases; ph++) {
    for (const LpPhaseDev& d : p.general.pointwise[ph]) n += d.x0 == x0;
    for (const LpJobDev& j : p.general.jobs[ph]) n += j.x0 == x0;
  }
  return n;
}
static size_t chains_of(const LocalPlan& p, uint32_t x0) {
  size_t n = 0;
  for (const LsChainDev& c : p.squeeze.chains) n += c.x0 == x0;
  return n;
}
static bool zero_desc(const LocalGroupDev& d) {
  LocalGroupDev z;
  memset(&z, 0, sizeof z);
  return memcmp(&d, &z, sizeof z) == 0;
}
static const char* kernel_name(LocalKernel k) {
  switch (k) {
    case LocalKernel::kLocal: return "k_modular_local";
    case LocalKernel::kSqueezeLds: return "k_modular_local_squeeze_lds";
    case LocalKernel::kSqueezeLevel: return "k_modular_local_squeeze_level";
    case LocalKernel::kPalette: return "k_modular_local_palette";
    case LocalKernel::kPhase: return "k_modular_local_phase";
  }
  return "?";
}
static std::string launches(const LocalPlan& p) {  // "kernel:n_items kernel:n_items ..."
  std::string s;
  for (const LocalStep& st : p.steps) s += std::string(s.empty() ? "" : " ") + kernel_name(st.kernel) + ":" + std::to_string(st.n_items);
  return s;
}
static std::string kernels(const LocalPlan& p) {
  std::string s;
  for (const LocalStep& st : p.steps) s += std::string(s.empty() ? "" : " ") + kernel_name(st.kernel);
  return s;
}
static std::vector<uint8_t> block(const LocalPlan& p) {
  std::vector<uint8_t> b(p.layout.total + 32, 0xa5);
  p.serialize(b.data() + 16);
  for (int i = 0; i < 16; i++) EXPECT(b[i] == 0xa5 && b[16 + p.layout.total + i] == 0xa5);  // exactly `total` bytes
  return std::vector<uint8_t>(b.begin() + 16, b.end() - 16);
}

// ---------------------------------------------------------------- the layout of any accepted plan
static void check_layout(const LocalPlan& p) {
  EXPECT(p.status == JXLH_OK);
  std::vector<std::pair<const LocalSection*, std::pair<const void*, size_t>>> secs;
  auto add = [&](const LocalSection& s, const void* data, size_t bytes) { secs.push_back({&s, {data, bytes}}); };
  const LocalLayout& L = p.layout;
  add(L.groups, p.groups.data(), p.groups.size() * sizeof(LocalGroupDev));
  add(L.items, p.items.data(), p.items.size() * sizeof(LocalItem));
  for (uint32_t ph = 0; ph < kLpMaxPhases; ph++) {
    if (ph & 1) add(L.phase_desc[ph], p.general.jobs[ph].data(), p.general.jobs[ph].size() * sizeof(LpJobDev));
    else add(L.phase_desc[ph], p.general.pointwise[ph].data(), p.general.pointwise[ph].size() * sizeof(LpPhaseDev));
    EXPECT(((ph & 1) ? p.general.pointwise[ph].size() : p.general.jobs[ph].size()) == 0);  // even: point-wise, odd: palettes
    add(L.phase_items[ph], p.general.items[ph].data(), p.general.items[ph].size() * sizeof(LocalItem));
  }
  add(L.chains, p.squeeze.chains.data(), p.squeeze.chains.size() * sizeof(LsChainDev));
  add(L.lds_items, p.squeeze.lds_items.data(), p.squeeze.lds_items.size() * sizeof(LocalItem));
  for (int k = 0; k < kLsLevels; k++) add(L.level_items[k], p.squeeze.level_items[k].data(), p.squeeze.level_items[k].size() * sizeof(LocalItem));
  const std::vector<uint8_t> b = block(p);
  size_t end = 0;  // of the section before, rounded up: the documented order, no overlap, no gap beyond the padding
  for (const auto& s : secs) {
    EXPECT(s.first->off % 16 == 0 && s.first->off == end && s.first->bytes == s.second.second);
    EXPECT(s.first->off + s.first->bytes <= L.total);
    if (s.first->bytes && s.first->off + s.first->bytes <= L.total) EXPECT(memcmp(b.data() + s.first->off, s.second.first, s.first->bytes) == 0);
    for (size_t i = s.first->off + s.first->bytes; i < (s.first->off + s.first->bytes + 15) / 16 * 16 && i < L.total; i++) EXPECT(b[i] == 0);
    end = (s.first->off + s.first->bytes + 15) / 16 * 16;
  }
  EXPECT(L.total == end);
  // the steps: each reads sections of the layout, in the documented order of launches; none is empty
  int last = -1;
  for (const LocalStep& st : p.steps) {
    EXPECT(st.n_items > 0 && st.items.bytes == st.n_items * sizeof(LocalItem));
    int order = 0;
    if (st.kernel == LocalKernel::kLocal) {
      EXPECT(st.desc.off == L.groups.off && st.items.off == L.items.off && st.n_items == p.items.size());
    } else if (st.kernel == LocalKernel::kSqueezeLds) {
      order = 1;
      EXPECT(st.desc.off == L.chains.off && st.items.off == L.lds_items.off && st.n_items == p.squeeze.lds_items.size());
    } else if (st.kernel == LocalKernel::kSqueezeLevel) {
      order = 2 + (int)st.step;
      EXPECT(st.step < (uint32_t)kLsLevels);
      if (st.step < (uint32_t)kLsLevels)
        EXPECT(st.desc.off == L.chains.off && st.items.off == L.level_items[st.step].off && st.n_items == p.squeeze.level_items[st.step].size());
    } else {
      uint32_t ph = 0;
      while (ph < kLpMaxPhases && L.phase_items[ph].off != st.items.off) ph++;
      EXPECT(ph < kLpMaxPhases);
      if (ph == kLpMaxPhases) continue;
      order = 2 + kLsLevels + (int)ph;
      EXPECT(st.kernel == ((ph & 1) ? LocalKernel::kPalette : LocalKernel::kPhase));
      EXPECT(st.desc.off == L.phase_desc[ph].off && st.n_items == p.general.items[ph].size());
      EXPECT(st.weighted == ((ph & 1) && p.general.weighted[ph]) && st.lds_palette == ((ph & 1) && p.general.lds_palette[ph]));
    }
    EXPECT(order > last);
    last = order;
  }
  size_t lists = !p.items.empty() + !p.squeeze.lds_items.empty();
  for (const auto& v : p.squeeze.level_items) lists += !v.empty();
  for (const auto& v : p.general.items) lists += !v.empty();
  EXPECT(p.steps.size() == lists);  // every non-empty work list is launched, once
}

// ---------------------------------------------------------------- chains and scratch
static void check_chains_and_scratch(const LocalPlan& p) {
  std::set<std::pair<uint64_t, uint64_t>> ranges;  // (offset, samples) of everything the batch keeps in scratch
  for (const LsChainDev& c : p.squeeze.chains) {
    EXPECT(c.n_levels >= 1 && c.n_levels <= (uint32_t)kLsLevels && c.n_lds <= c.n_levels);
    jxlh_squeeze_level lv[kLsLevels];
    memset(lv, 0, sizeof lv);
    uint32_t prefix = 0;  // levels whose planes are inside the tile
    for (uint32_t i = 0; i < c.n_levels; i++) lv[i].horizontal = c.lv[i].horizontal, lv[i].out_w = c.lv[i].out_w, lv[i].out_h = c.lv[i].out_h;
    while (prefix < c.n_levels && c.lv[prefix].out_w <= (uint32_t)kLsTile && c.lv[prefix].out_h <= (uint32_t)kLsTile) prefix++;
    EXPECT(c.n_lds <= prefix);
    if (c.n_lds > 0) EXPECT(squeeze_levels_fit((int)c.n_lds, lv, c.base_w, c.base_h));
    for (uint32_t n = c.n_lds + 1; n <= prefix; n++) EXPECT(!squeeze_levels_fit((int)n, lv, c.base_w, c.base_h));
    // what leaves a launch without being the chain's last level goes to plane i & 1
    uint64_t need[2] = {0, 0};
    for (uint32_t i = 0; i + 1 < c.n_levels; i++)
      if (i + 1 >= c.n_lds) need[i & 1] = std::max(need[i & 1], (uint64_t)c.lv[i].out_w * c.lv[i].out_h);
    for (int q = 0; q < 2; q++) ranges.insert({c.scratch_off[q], need[q]});
  }
  for (uint32_t ph = 0; ph < kLpMaxPhases; ph++) {
    for (const LpPhaseDev& d : p.general.pointwise[ph])
      for (int t = 0; t < 4; t++)
        if (d.dst[t].space == kLpScratch) ranges.insert({d.dst[t].off, (uint64_t)d.w * d.h});
    for (const LpJobDev& j : p.general.jobs[ph]) {
      const bool rows = j.predictor == 6 && j.h > (uint32_t)kLpRows;  // the weighted predictor's state between bands
      if (rows) ranges.insert({j.wp_rows_off, (uint64_t)j.n_slots * 10 * j.w});
      else EXPECT(j.wp_rows_off == 0);
    }
  }
  // disjoint, each as large as what it holds, and nothing else: the ranges tile [0, scratch)
  uint64_t at = 0;
  for (const auto& r : ranges) {
    EXPECT(r.first == at);
    at = r.first + r.second;
  }
  EXPECT(at == p.scratch);
}

// ---------------------------------------------------------------- the batches
struct Named {
  const char* name;
  Call call;
};

// the _general call of the route test: x0 = 40 * index
static Call general_routes() {
  Call c;
  c.n_out = 3;
  add_group(c, 0, 0, 37, 53, 3, {rct(0, 17)}, 3);                         // 0 plain
  add_group(c, 40, 0, 37, 53, 3, {pal(c, 0, 3, 20, 6, 0)});               // 1 predictor 0 with deltas: the single launch
  add_group(c, 80, 0, 37, 53, 3, {pal(c, 0, 3, 20, 6, 5)});               // 2 predictor 5: phases
  add_group(c, 120, 0, 37, 70, 3, {pal(c, 0, 3, 3000, 6, 6)});            // 3 predictor 6, h > 64, palette beyond LDS
  add_group(c, 160, 0, 0, 53, 3, {rct(0, 1)});                            // 4 zero-area plain
  add_group(c, 200, 0, 37, 0, 3, {pal(c, 0, 3, 20, 6, 5)});               // 5 zero-area phases
  return c;
}
// the _squeeze call of the route test: x0 = 140 * index
static Call squeeze_routes() {
  static const std::vector<jxlh_squeeze_params> h3 = {{1, 1, 0, 1}, {1, 1, 0, 1}, {1, 1, 0, 1}};
  Call c;
  c.form = LocalBatchIn::kSqueeze;
  c.w = 1400, c.h = 300;
  add_squeeze_group(c, 0, 0, 37, 53, 3, {rct(0, 5)}, nullptr);            // 0 no squeeze, equal strides: as general (plain)
  add_squeeze_group(c, 140, 0, 37, 53, 3, {rct(0, 5)}, nullptr, 1);       // 1 unequal strides: chains without levels
  add_squeeze_group(c, 280, 0, 130, 131, 3, {}, &kDefault);               // 2 LDS launch + streamed levels
  add_squeeze_group(c, 420, 0, 256, 256, 1, {}, &h3);                     // 3 never in the LDS launch
  add_squeeze_group(c, 700, 0, 0, 9, 3, {}, nullptr);                     // 4 zero-area, no squeeze
  add_squeeze_group(c, 840, 0, 0, 9, 3, {}, nullptr, 1);                  // 5 zero-area: no rows for strides to differ on
  add_squeeze_group(c, 980, 0, 9, 0, 3, {}, &kDefault);                   // 6 zero-area with a (default) squeeze
  add_squeeze_group(c, 1120, 0, 37, 53, 3, {pal(c, 0, 3, 20, 6, 5)}, nullptr);      // 7 no squeeze, predicted: as general (phases)
  add_squeeze_group(c, 1260, 0, 130, 131, 3, {pal(c, 0, 3, 20, 6, 6)}, &kDefault);  // 8 chains, then a weighted palette
  return c;
}
// tests/test_gpu_modular_local_squeeze.py::test_launch_accounting: k groups of 130 x 130, three channels, default squeeze
static Call accounting(int k0, int k1, bool deep_and_plain = false) {
  Call c;
  c.form = LocalBatchIn::kSqueeze;
  c.n_out = 3;
  if (deep_and_plain) {
    add_squeeze_group(c, 0, 0, 130, 130, 3, {rct(0, 5)}, &kDefault);
    add_squeeze_group(c, 0, 140, 30, 30, 3, {rct(0, 6)}, nullptr);
  }
  for (int k = k0; k < k1; k++) add_squeeze_group(c, 132 * (k % 8), 132 * (k / 8), 130, 130, 3, {}, &kDefault);
  return c;
}
// a batch without a squeeze group, as a _squeeze call and as the _general call of the same groups (the same arena)
static Call no_squeeze(bool as_general) {
  Call c;
  c.form = as_general ? LocalBatchIn::kGeneral : LocalBatchIn::kSqueeze;
  c.w = 902, c.h = 1052;
  for (uint32_t k = 0; k < 14; k++) {
    const uint32_t x0 = 150 * (k % 6) + k % 3, y0 = 150 * (k / 6), w = 20 + 9 * k, h = 147 - 10 * k;
    uint32_t nc = 3;
    std::vector<jxlh_local_step> steps;
    switch (k % 7) {
      case 0: break;
      case 1: steps = {rct(0, 17)}; break;
      case 2: steps = {pal(c, 0, 3, 300, 0, 0)}; break;
      case 3: steps = {pal(c, 0, 3, 40, 5, 5)}; break;
      case 4: steps = {pal(c, 0, 3, 40, 5, 6)}; break;
      case 5: steps = {rct(0, 40), pal(c, 1, 1, 90, 0, 0)}; break;
      case 6: nc = 4, steps = {pal(c, 3, 1, 30, 4, 5), rct(1, 10)}; break;
    }
    if (as_general) add_group(c, x0, y0, w, h, nc, steps);
    else add_squeeze_group(c, x0, y0, w, h, nc, steps, nullptr);
  }
  return c;
}
// slot placement: an RCT, a general palette and an RCT, in the order they run
static Call placement(bool index_changed) {
  Call c;
  if (index_changed)  // [c0 c1 c2] -> rct -> palette of c0 -> [meta idx c1 c2] -> rct of idx c1 c2: the first phase rewrites the index
    add_group(c, 0, 0, 37, 53, 3, {rct(0, 9), pal(c, 0, 1, 20, 6, 5), rct(1, 2)});
  else  // four channels, palette of c3, RCTs of c0..c2: the index stays where it was decoded
    add_group(c, 0, 0, 37, 53, 4, {rct(0, 9), pal(c, 3, 1, 20, 6, 5), rct(1, 2)});
  return c;
}
static Call grey(bool frame) {
  Call c;
  c.frame = frame, c.n_out = 3;
  add_group(c, 0, 0, 37, 53, 1, {pal(c, 0, 1, 20, 6, 5)});
  return c;
}
static Call weighted_rows(uint32_t h) {
  Call c;
  add_group(c, 0, 0, 37, h, 3, {pal(c, 0, 3, 20, 6, 6)});
  return c;
}

static std::vector<Named> batches() {
  return {{"general_routes", general_routes()}, {"squeeze_routes", squeeze_routes()},
          {"accounting_one", accounting(0, 1)}, {"accounting_many", accounting(0, 40)},
          {"accounting_deep_plain_many", accounting(1, 8, true)},
          {"no_squeeze", no_squeeze(false)}, {"no_squeeze_general", no_squeeze(true)},
          {"placement_index_changed", placement(true)}, {"placement_index_kept", placement(false)},
          {"grey_frame", grey(true)}, {"grey_stage", grey(false)},
          {"weighted_h64", weighted_rows(64)}, {"weighted_h65", weighted_rows(65)}};
}

static int dump() {
  for (const Named& b : batches()) {
    for (int aligned = 0; aligned < 2; aligned++) {
      const LocalPlan p = b.call.plan(aligned != 0);
      printf("batch %s%s %d %zu scratch %llu total %zu\n", b.name, aligned ? "" : "_unaligned", (int)p.status, p.first_bad,
             (unsigned long long)p.scratch, p.layout.total);
      for (const LocalStep& s : p.steps)
        printf("step %s desc %zu %zu items %zu %zu n_items %u step %u weighted %u lds_palette %u fan_grey %u\n", kernel_name(s.kernel),
               s.desc.off, s.desc.bytes, s.items.off, s.items.bytes, s.n_items, s.step, s.weighted, s.lds_palette, s.fan_grey);
      printf("block ");
      for (uint8_t v : block(p)) printf("%02x", v);
      printf("\n");
    }
  }
  return fails ? 1 : 0;
}

// ---------------------------------------------------------------- refusals
static void expect_refused(const Call& c, jxlh_status st, size_t bad, const char* why, int line) {
  const LocalPlan p = c.plan();
  const bool ok = p.status == st && p.first_bad == bad && p.why && strcmp(p.why, why) == 0 && p.steps.empty();
  if (!ok) {
    fprintf(stderr, "line %d: got %d at %zu \"%s\" with %zu steps, want %d at %zu \"%s\"\n", line, (int)p.status, p.first_bad,
            p.why ? p.why : "(null)", p.steps.size(), (int)st, bad, why);
    fails++;
  }
}
#define REFUSED(c, st, bad, why) expect_refused(c, st, bad, why, __LINE__)

static void refusals() {
  const jxlh_status INV = JXLH_ERR_INVALID_ARGUMENT, UNS = JXLH_ERR_UNSUPPORTED;
  auto stage = [](LocalBatchIn::Form form) {  // three good groups on 96 x 40, three planes
    Call c;
    c.form = form, c.n_out = 3, c.w = 96, c.h = 40;
    for (uint32_t k = 0; k < 3; k++) {
      if (form == LocalBatchIn::kSqueeze) add_squeeze_group(c, 32 * k, 0, 30, 30, 3, {rct(0, k)}, k == 1 ? nullptr : &kDefault);
      else add_group(c, 32 * k, 0, 30, 30, 3, {rct(0, k)});
    }
    EXPECT(c.plan().status == JXLH_OK && !c.plan().steps.empty());
    return c;
  };
  for (LocalBatchIn::Form form : {LocalBatchIn::kPlain, LocalBatchIn::kGeneral, LocalBatchIn::kSqueeze}) {
    const bool sq = form == LocalBatchIn::kSqueeze;
    auto x0 = [&](Call& c, size_t g) -> uint32_t& { return sq ? c.sgroups[g].x0 : c.groups[g].x0; };
    auto n_channels = [&](Call& c, size_t g) -> uint32_t& { return sq ? c.sgroups[g].n_channels : c.groups[g].n_channels; };
    auto step0 = [&](Call& c, size_t g) -> jxlh_local_step& { return sq ? c.sgroups[g].steps[0] : c.groups[g].steps[0]; };
    Call c = stage(form);
    // 1. the lowering, with its own text
    step0(c, 2).rct_type = 42;
    REFUSED(c, INV, 2, "rct_type above 41");
    step0(c, 2).kind = 2;
    REFUSED(c, UNS, 2, "a transform other than RCT and palette (local squeeze)");
    // 3. the rect leaves the planes
    c = stage(form);
    x0(c, 2) = 70;
    REFUSED(c, INV, 2, "the rect leaves the planes");
    x0(c, 2) = 0xfffffff0u;  // ... without wrapping
    REFUSED(c, INV, 2, "the rect leaves the planes");
    // two bad groups: the lower index; lowering before the rect in one group
    x0(c, 1) = 90;
    REFUSED(c, INV, 1, "the rect leaves the planes");
    step0(c, 1).rct_type = 50;
    REFUSED(c, INV, 1, "rct_type above 41");
    // 2. the channel count, before the rect
    c = stage(form);
    c.n_out = 2;
    x0(c, 0) = 90;
    REFUSED(c, INV, 0, "more channels than out planes");
    c = stage(form);
    c.frame = true;
    c.plan();
    EXPECT(c.plan().status == JXLH_OK);
    if (!sq) {  // (two channels of a squeeze group need another coded list: the lowering would speak first)
      n_channels(c, 2) = 2, c.groups[2].n_steps = 0, c.groups[2].n_coded = 2;
      x0(c, 2) = 90;
      REFUSED(c, INV, 2, "a frame's groups hold 3 channels, or 1 (grey)");
    }
  }
  {  // the plain call refuses what the _general call lowers
    Call c = general_routes();
    EXPECT(c.plan().status == JXLH_OK);
    c.form = LocalBatchIn::kPlain;
    REFUSED(c, UNS, 1, "delta / predicted local palette");
    c.form = LocalBatchIn::kGeneral;
    c.wp[3].w3 = 16;
    REFUSED(c, INV, 3, "wp header field outside its width");
  }
  {  // the squeeze lowering's refusals, as tests/test_gpu_modular_local_squeeze.py::test_refusals_launch_nothing makes them
    Call c = stage(LocalBatchIn::kSqueeze);
    c.sgroups[2].squeeze_pos = 0;
    REFUSED(c, UNS, 2, "a transform behind a local squeeze");
    c = stage(LocalBatchIn::kSqueeze);
    c.sgroups[2].n_coded--;
    REFUSED(c, UNS, 2, "a coded channel is missing (previews of local squeezes stay on the host)");
    c = stage(LocalBatchIn::kSqueeze);
    c.coded.back().stride = 1;
    REFUSED(c, INV, 2, "coded stride below w");
    c = stage(LocalBatchIn::kSqueeze);
    c.coded.back().offset = 1ull << 63;
    REFUSED(c, INV, 2, "coded channel beyond the arena");
    c = stage(LocalBatchIn::kSqueeze);
    c.coded.back().w++;
    REFUSED(c, INV, 2, "a coded channel's size is not what the transforms leave");
  }
  {  // 4. a predicted palette on a group wider than 2^30 (nothing of that size is touched: the arena is a number here)
    Call c;
    c.w = 0x7fffffffu, c.h = 4, c.arena_samples = 1ull << 40;
    add_group(c, 0, 0, 30, 4, 3, {rct(0, 1)});
    add_group(c, 0, 0, (1u << 30) + 1, 1, 3, {pal(c, 0, 3, 20, 6, 5)});
    REFUSED(c, INV, 1, "a predicted palette on a group wider than 2^30");
    c.groups[1].w = 1u << 30, c.groups[1].coded_stride = 1u << 30, c.groups[1].h = 0;  // at the cap, and empty: passes
    EXPECT(c.plan().status == JXLH_OK && kernels(c.plan()) == "k_modular_local");
    c.groups[1].w = (1u << 30) + 1, c.groups[1].coded_stride = (1u << 30) + 1;  // beyond it: refused even when empty
    REFUSED(c, INV, 1, "a predicted palette on a group wider than 2^30");
    c.groups[1].x0 = 0x7fffffffu;  // the rect speaks first
    REFUSED(c, INV, 1, "the rect leaves the planes");
  }
  // 5. the item cap, on the count itself
  EXPECT(local_item_count_ok(0) && local_item_count_ok(0x7fffffffull) && !local_item_count_ok(0x80000000ull) && !local_item_count_ok(~0ull));
  {  // the call as a whole: no group is named
    Call c = stage(LocalBatchIn::kGeneral);
    c.w = 0x80000000u;
    const LocalPlan p = c.plan();
    EXPECT(p.status == INV && p.why == nullptr && p.steps.empty());
  }
}

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "dump") == 0) return dump();
  const uint32_t rct_kind = JXLH_LOCAL_RCT;
  for (const Named& b : batches()) {
    for (int aligned = 0; aligned < 2; aligned++) {
      const LocalPlan p = b.call.plan(aligned != 0);
      const int before = fails;
      check_layout(p);
      check_chains_and_scratch(p);
      if (fails != before) fprintf(stderr, "... in batch %s\n", b.name);
    }
  }
  {  // ---- routes, _general call
    const Call c = general_routes();
    const LocalPlan p = c.plan();
    EXPECT(kernels(p) == "k_modular_local k_modular_local_palette");
    // plain and predictor 0: items of the single launch, no phase; the palette op keeps its kind
    EXPECT(plain_items(p, 0) == 1 && plain_items(p, 1) == 1 && phase_descs(p, 0) == 0 && phase_descs(p, 40) == 0);
    EXPECT(p.groups[1].n_ops == 1 && p.groups[1].ops[0].kind == JXLH_LOCAL_PALETTE && p.groups[1].ops[0].num_colors == 26);
    EXPECT(p.groups[1].ops[0].lds_off == 0 && p.groups[1].lds_entries == 3 * 26);
    // predictors 5 and 6: one palette job each in phase 1, no item of the single launch, a zero descriptor there
    EXPECT(plain_items(p, 2) == 0 && plain_items(p, 3) == 0 && zero_desc(p.groups[2]) && zero_desc(p.groups[3]));
    EXPECT(phase_descs(p, 80) == 1 && phase_descs(p, 120) == 1 && p.general.jobs[1].size() == 2 && p.general.items[1].size() == 6);
    EXPECT(p.general.jobs[1][0].predictor == 5 && p.general.jobs[1][0].lds == 1 && p.general.jobs[1][0].index.space == kLpArena);
    EXPECT(p.general.jobs[1][1].predictor == 6 && p.general.jobs[1][1].lds == 0 && p.general.jobs[1][1].wp.p1c == 16 && p.general.jobs[1][1].wp.w[0] == 13);
    EXPECT(p.steps[1].weighted == 1 && p.steps[1].lds_palette == 1);
    EXPECT(p.scratch == 3 * 10 * 37);  // group 3's state rows; no index leaves the arena
    // zero-area: checked, not planned -- no item, no phase; the plain one's descriptor names no rows
    EXPECT(plain_items(p, 4) == 0 && plain_items(p, 5) == 0 && phase_descs(p, 160) == 0 && phase_descs(p, 200) == 0);
    EXPECT(p.groups[4].rows_per_item == 0 && zero_desc(p.groups[5]));
    // the vector path: the caller's alignment, the stride, x0 and every offset
    // group 0: x0 = 0, rows of 40, offsets 64 + k * 40 * 53: the vector path; group 1: rows of 37
    EXPECT(p.groups[0].vec == 1 && p.groups[0].coded_stride == 40 && p.groups[1].vec == 0);
    const LocalPlan u = c.plan(false);
    for (const LocalGroupDev& g : u.groups) EXPECT(g.vec == 0);
  }
  {  // ---- routes, _squeeze call
    const Call c = squeeze_routes();
    const LocalPlan p = c.plan();
    EXPECT(kernels(p) == "k_modular_local k_modular_local_squeeze_lds k_modular_local_squeeze_level k_modular_local_squeeze_level "
                         "k_modular_local_squeeze_level k_modular_local_phase k_modular_local_palette");
    // 0: as a group of the _general calls, in the single launch, its coded channels the group's
    EXPECT(plain_items(p, 0) == 1 && chains_of(p, 0) == 0 && phase_descs(p, 0) == 0);
    EXPECT(p.groups[0].coded_stride == 37 && p.groups[0].slot_mask == 7 && p.groups[0].slot_off[1] == c.coded[1].offset && p.groups[0].ops[0].kind == rct_kind);
    // 1: unequal strides: chains without levels -- no chain, one point-wise phase 0 that reads every channel at its stride
    EXPECT(plain_items(p, 1) == 0 && zero_desc(p.groups[1]) && chains_of(p, 140) == 0 && phase_descs(p, 140) == 1);
    for (const LpPhaseDev& d : p.general.pointwise[0]) {
      if (d.x0 != 140) continue;
      for (uint32_t t = 0; t < 3; t++)
        EXPECT(d.src[t].space == kLpArena && d.src[t].stride == 37 + t && d.src[t].off == c.coded[3 + t].offset && d.dst[t].space == kLpOut);
      EXPECT(d.n_ops == 1 && d.fan == 0);
    }
    // 2: three chains, each with levels in the LDS launch and two streamed ones; no phase (nothing runs behind the squeeze)
    EXPECT(chains_of(p, 280) == 3 && phase_descs(p, 280) == 0 && zero_desc(p.groups[2]));
    for (const LsChainDev& ch : p.squeeze.chains)
      if (ch.x0 == 280) EXPECT(ch.n_lds >= 1 && ch.n_levels == ch.n_lds + 2 && ch.lv[ch.n_levels - 1].out_w == 130 && ch.lv[ch.n_levels - 1].out_h == 131);
    // 3: 256 rows at every level: never in the LDS launch, three streamed levels of 4 workgroups
    EXPECT(chains_of(p, 420) == 1);
    for (const LsChainDev& ch : p.squeeze.chains)
      if (ch.x0 == 420) EXPECT(ch.n_lds == 0 && ch.n_levels == 3 && ch.lv[0].out_w == 64 && ch.lv[2].out_w == 256 && ch.base_w == 32);
    EXPECT(p.squeeze.level_items[2].size() == 4 + 0);  // only that chain reaches streamed launch 2
    // 4, 5, 6: zero-area of each kind: nothing planned (4 and 5 keep the plain descriptor; no item names it)
    for (size_t g = 4; g <= 6; g++) EXPECT(plain_items(p, g) == 0);
    EXPECT(chains_of(p, 700) + chains_of(p, 840) + chains_of(p, 980) == 0 && phase_descs(p, 700) + phase_descs(p, 840) + phase_descs(p, 980) == 0);
    EXPECT(p.groups[4].n_channels == 3 && p.groups[5].n_channels == 3 && p.groups[4].rows_per_item == 0);
    // 7: as general, with a predicted palette: the phases, its index in the arena
    EXPECT(plain_items(p, 7) == 0 && chains_of(p, 1120) == 0 && phase_descs(p, 1120) == 1 && zero_desc(p.groups[7]));
    // 8: a chain for the index channel, which ends in the rect: the phase in front of the palette moves it to scratch
    EXPECT(chains_of(p, 1260) == 1 && phase_descs(p, 1260) == 2);
    for (const LpPhaseDev& d : p.general.pointwise[0])
      if (d.x0 == 1260) EXPECT(d.src[0].space == kLpOut && d.dst[0].space == kLpScratch && d.dst[0].stride == 130 && d.n_ops == 0);
    for (const LpJobDev& j : p.general.jobs[1])
      if (j.x0 == 1260) EXPECT(j.index.space == kLpScratch && j.predictor == 6 && j.wp_rows_off != 0 && j.n_slots == 3);
    // the route, asked directly
    jxlh_local_squeeze_program sp;
    const LocalBatchIn in = c.in();
    const LocalRoute want[9] = {LocalRoute::kPlain, LocalRoute::kChains, LocalRoute::kChains, LocalRoute::kChains, LocalRoute::kPlain,
                                LocalRoute::kPlain, LocalRoute::kChains, LocalRoute::kPhases, LocalRoute::kChains};  // 6: its squeeze has a level
    for (size_t g = 0; g < 9; g++) {
      EXPECT(local_lower_squeeze_group(c.sgroups[g], in.coded, in.n_coded, in.params, in.n_params, &kWp, 8, in.arena_samples, &sp, nullptr) == JXLH_OK);
      EXPECT(local_route(&c.sgroups[g], &sp, in.coded, sp.general.n_phases) == want[g]);
    }
    EXPECT(local_route(nullptr, nullptr, nullptr, 1) == LocalRoute::kPlain && local_route(nullptr, nullptr, nullptr, 3) == LocalRoute::kPhases);
  }
  {  // ---- the launch lists of test_launch_accounting
    // 130 x 130, three channels, default squeeze: every level up to 65 x 65 runs in the LDS launch (one item per chain);
    // the last two of each chain are streamed, 64 lines per item: channel 0 ends 130 x 65 (h: 65 rows, 2 items), then
    // 130 x 130 (v: 130 columns, 3 items); channels 1 and 2 end 65 x 130 (v: 65 columns, 2), then 130 x 130 (h: 130 rows, 3)
    const LocalPlan one = accounting(0, 1).plan(), many = accounting(0, 40).plan();
    EXPECT(launches(one) == "k_modular_local_squeeze_lds:3 k_modular_local_squeeze_level:6 k_modular_local_squeeze_level:9");
    EXPECT(launches(many) == "k_modular_local_squeeze_lds:120 k_modular_local_squeeze_level:240 k_modular_local_squeeze_level:360");
    EXPECT(kernels(one) == kernels(many));  // the number of launches does not depend on the number of groups
    for (int n : {2, 7, 23}) EXPECT(kernels(accounting(0, n).plan()) == kernels(one));
    // the deepest group decides: an RCT behind the chains adds its phase (130 rows, 62 per item); the plain group its launch
    const LocalPlan deep = accounting(1, 8, true).plan();
    EXPECT(launches(deep) == "k_modular_local:1 k_modular_local_squeeze_lds:24 k_modular_local_squeeze_level:48 "
                             "k_modular_local_squeeze_level:72 k_modular_local_phase:3");
    // a batch without a squeeze group is the _general call's plan of the same groups, to the byte
    const LocalPlan a = no_squeeze(false).plan(), b = no_squeeze(true).plan();
    EXPECT(launches(a) == launches(b) && a.steps.size() >= 3 && kernels(a).find("squeeze") == std::string::npos);
    EXPECT(a.scratch == b.scratch && a.layout.total == b.layout.total && block(a) == block(b));
    for (size_t i = 0; i < a.steps.size() && i < b.steps.size(); i++)
      EXPECT(a.steps[i].weighted == b.steps[i].weighted && a.steps[i].lds_palette == b.steps[i].lds_palette && a.steps[i].items.off == b.steps[i].items.off);
  }
  {  // ---- slot placement: rct, general palette, rct
    const LocalPlan p = placement(true).plan();
    EXPECT(launches(p) == "k_modular_local_phase:1 k_modular_local_palette:1 k_modular_local_phase:1");
    EXPECT(p.general.pointwise[0].size() == 1 && p.general.jobs[1].size() == 1 && p.general.pointwise[2].size() == 1);
    if (!fails) {
      const LpPhaseDev& d0 = p.general.pointwise[0][0];
      const LpJobDev& j = p.general.jobs[1][0];
      const LpPhaseDev& d2 = p.general.pointwise[2][0];
      // phase 0: everything comes from the arena; the RCT rewrites the index (slot 0), which the palette's other workgroups
      // read while its own is written: to scratch; slots 1 and 2 are final for now: to the rect
      for (int t = 0; t < 3; t++) EXPECT(d0.src[t].space == kLpArena && d0.src[t].stride == 37);
      EXPECT(d0.src[3].space == kLpNone && d0.n_ops == 1 && d0.ops[0].kind == rct_kind && d0.ops[0].lds_off == kLocalNoLds);
      EXPECT(d0.dst[0].space == kLpScratch && d0.dst[0].off == 0 && d0.dst[0].stride == 37);
      EXPECT(d0.dst[1].space == kLpOut && d0.dst[2].space == kLpOut && d0.dst[3].space == kLpNone && d0.fan == 0);
      EXPECT(j.index.space == kLpScratch && j.index.off == 0 && j.n_slots == 1 && j.out_slot[0] == 0 && j.predictor == 5 && j.palette_size == 26);
      // phase 2: every slot is in the rect, the RCT changes all three: all stored, all in the rect at the end
      for (int t = 0; t < 3; t++) EXPECT(d2.src[t].space == kLpOut && d2.dst[t].space == kLpOut);
      EXPECT(d2.n_ops == 1 && d2.fan == 0 && p.scratch == 37 * 53);
    }
    const LocalPlan q = placement(false).plan();
    EXPECT(launches(q) == "k_modular_local_phase:1 k_modular_local_palette:1 k_modular_local_phase:1");
    EXPECT(q.general.pointwise[0].size() == 1 && q.general.jobs[1].size() == 1 && q.general.pointwise[2].size() == 1);
    if (q.general.pointwise[0].size() == 1 && q.general.jobs[1].size() == 1 && q.general.pointwise[2].size() == 1) {
      const LpPhaseDev& d0 = q.general.pointwise[0][0];
      const LpPhaseDev& d2 = q.general.pointwise[2][0];
      // the index (slot 3) was neither changed nor in the rect: it stays in the arena, no scratch
      EXPECT(d0.src[3].space == kLpArena && d0.dst[3].space == kLpNone && q.general.jobs[1][0].index.space == kLpArena && q.scratch == 0);
      for (int t = 0; t < 3; t++) EXPECT(d0.dst[t].space == kLpOut && d2.src[t].space == kLpOut && d2.dst[t].space == kLpOut);
      EXPECT(d2.src[3].space == kLpOut && d2.dst[3].space == kLpNone);  // the palette left it in the rect; nothing changes it
    }
    // fan: only a grey group of a frame -- there the last phase exists for it alone
    const LocalPlan gf = grey(true).plan(), gs = grey(false).plan();
    EXPECT(launches(gf) == "k_modular_local_palette:1 k_modular_local_phase:1" && launches(gs) == "k_modular_local_palette:1");
    EXPECT(gf.general.pointwise[2].size() == 1 && gf.general.pointwise[2][0].fan == 1 && gf.general.pointwise[2][0].n_ops == 0);
    for (const Named& b : batches())
      for (const auto& v : b.call.plan().general.pointwise)
        for (const LpPhaseDev& d : v) EXPECT(d.fan == (strcmp(b.name, "grey_frame") == 0));
    // the plain launch of a frame fans its grey groups out
    Call fr = accounting(1, 2, true);
    fr.frame = true;
    EXPECT(fr.plan().steps[0].kernel == LocalKernel::kLocal && fr.plan().steps[0].fan_grey == 1 && accounting(1, 2, true).plan().steps[0].fan_grey == 0);
  }
  {  // ---- the weighted predictor's row state: only when the group is taller than one band
    EXPECT(weighted_rows(kLpRows).plan().scratch == 0 && weighted_rows(kLpRows).plan().general.jobs[1][0].wp_rows_off == 0);
    EXPECT(weighted_rows(kLpRows + 1).plan().scratch == 3 * 10 * 37);
  }
  refusals();
  if (fails) return 1;
  printf("modular local plan: ok (%zu batches)\n", batches().size());
  return 0;
}
